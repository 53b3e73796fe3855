"""A Python restatement of the timestamp conversions (reference: cpp/src/strings/datetime.cu, NVStrings::timestamp2long /
long2timestamp), with the two deviations of DESIGN.md §4c: bytes past the end of a row read as NUL, and signed overflow
wraps (64-bit; the int fields 32-bit).  Also the CPU harness: custrings_amd/csrc/datetime_ops.h built with g++."""
import numpy as np

UNITS = {"Y": 0, "M": 1, "D": 2, "h": 3, "m": 4, "s": 5, "ms": 6, "us": 7, "ns": 8}
YEARS, MONTHS, DAYS, HOURS, MINUTES, SECONDS, MS, US, NS = range(9)
DEFAULT_FORMAT = b"%Y-%m-%dT%H:%M:%SZ"
_WIDTH = {b"a": 0, b"A": 0, b"b": 0, b"B": 0, b"w": 1, b"Y": 4, b"j": 3, b"Z": 3, b"z": 5}
_WIDTH.update({c.encode(): 2 for c in "ymdHIMSpUW"})
_WRITES_NOTHING = set(b"zaAwbBUW")


def _s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def _s64(v):
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def _tdiv(a, b):  # C: truncation toward zero
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def _tmod(a, b):
    return a - b * _tdiv(a, b)


def compile_format(fmt, units):
    """-> list of (spec or None, literal byte or None, width); ValueError like the reference's std::invalid_argument"""
    if fmt is None:
        fmt = DEFAULT_FORMAT
    if units not in range(9):
        raise ValueError("units")
    items, i = [], 0
    while i < len(fmt):
        c = fmt[i:i + 1]
        i += 1
        if c != b"%":
            items.append((None, c, 1))
            continue
        if i == len(fmt):
            raise ValueError("unfinished specifier")
        c = fmt[i:i + 1]
        i += 1
        if c == b"%":
            items.append((None, c, 1))
            continue
        if c == b"f":
            w = 3 if units == MS else 9 if units == NS else 6
        elif c in _WIDTH:
            w = _WIDTH[c]
        else:
            raise ValueError("invalid specifier")
        items.append((c.decode(), None, w))
    return items


def out_width(fmt, units):
    """W: the bytes of every formatted row"""
    return sum(0 if s is not None and ord(s) in _WRITES_NOTHING else w for s, _, w in compile_format(fmt, units))


# ---- parse ----------------------------------------------------------------------------------------------------------------
def _str2int(row, at, n):
    v = 0
    for k in range(n):
        c = row[at + k] if at + k < len(row) else 0
        if not 48 <= c <= 57:
            break
        v = v * 10 + c - 48
    return v


def _up(c):
    return c - 32 if 97 <= c <= 122 else c


def _byte(row, i):
    return row[i] if i < len(row) else 0


def parse_parts(row, items):
    tp = [0, 1, 1, 0, 0, 0, 0, 0]  # year month day hour minute second subsecond tz-minutes
    pos = 0
    for spec, _, w in items:
        if spec is None:
            pos += 1  # literals are skipped, never checked
            continue
        if 0 <= len(row) - pos < w:
            return None
        if spec == "Y":
            tp[0] = _str2int(row, pos, w)
        elif spec == "y":
            tp[0] = _str2int(row, pos, w) + 1900
        elif spec == "m":
            tp[1] = _str2int(row, pos, w)
        elif spec in "dj":
            tp[2] = _str2int(row, pos, w)
        elif spec in "HI":
            tp[3] = _str2int(row, pos, w)
        elif spec == "M":
            tp[4] = _str2int(row, pos, w)
        elif spec == "S":
            tp[5] = _str2int(row, pos, w)
        elif spec == "f":
            tp[6] = _str2int(row, pos, w)
        elif spec == "p":
            if tp[3] <= 12 and _up(_byte(row, pos)) == 80 and _up(_byte(row, pos + 1)) == 77:
                tp[3] += 12
        elif spec == "z":
            sign = -1 if _byte(row, pos) == 45 else 1
            tp[7] = sign * (_str2int(row, pos + 1, 2) * 60 + _str2int(row, pos + 3, 2))
        elif spec == "Z":
            if [_up(_byte(row, pos + k)) for k in range(3)] != [85, 84, 67]:
                return None
        else:
            return None  # a A w b B U W
        pos += w
    return tp


def from_parts(tp, units):
    year, month, day, hour, minute, second, sub, tz = tp
    if units == YEARS:
        return year - 1970
    if units == MONTHS:
        return (year - 1970) * 12 + month - 1
    year -= 1 if month <= 2 else 0
    era = _tdiv(year if year >= 0 else year - 399, 400)
    yoe = year - era * 400
    doy = day if month == 0 else _tdiv(153 * (month + (-3 if month > 2 else 9)) + 2, 5) + day - 1
    doe = yoe * 365 + _tdiv(yoe, 4) - _tdiv(yoe, 100) + doy
    days = era * 146097 + doe - 719468
    if units == DAYS:
        return days
    if units == HOURS:
        return days * 24 + hour + _tdiv(tz, 60)
    if units == MINUTES:
        return days * 1440 + hour * 60 + minute + tz
    ts = days * 86400 + hour * 3600 + minute * 60 + second + tz * 60
    if units == SECONDS:
        return ts
    return _s64(ts * {MS: 1000, US: 10**6, NS: 10**9}[units] + sub)


def parse(row, items, units):
    """one row (bytes, or None for null) -> int64"""
    if not row:
        return 0
    tp = parse_parts(row, items)
    return 0 if tp is None else from_parts(tp, units)


def parse_column(rows, fmt=None, units=SECONDS):
    items = compile_format(fmt, units)
    return np.array([parse(r, items, units) for r in rows], dtype=np.int64)


# ---- format ---------------------------------------------------------------------------------------------------------------
_MDO = [0, 31, 61, 92, 122, 153, 184, 214, 245, 275, 306, 337, 366]


def dissect(v, units):
    """dissect_timestamp: [year, month, day, hour, minute, second, subsecond]"""
    tp = [0] * 7
    if units == YEARS:
        tp[:3] = [_s32(_s32(v) + 1970), 1, 1]
        return tp
    if units == MONTHS:
        tp[:3] = [_s32(_tdiv(v, 12) + 1970), _tmod(v, 12) + 1, 1]
        return tp
    per_day = {DAYS: 1, HOURS: 24, MINUTES: 1440, SECONDS: 86400, MS: 86400 * 10**3, US: 86400 * 10**6, NS: 86400 * 10**9}[units]
    days = _s32(_s32(_tdiv(v, per_day)) + 719468)
    year = 400 * _tdiv(days, 146097)
    days = _tmod(days, 146097)
    leapy = _tdiv(days, 36524)
    days = _tmod(days, 36524)
    if leapy == 4:
        days += 36524
        leapy -= 1
    year += 100 * leapy
    year += 4 * _tdiv(days, 1461)
    days = _tmod(days, 1461)
    leapy = _tdiv(days, 365)
    days = _tmod(days, 365)
    if leapy == 4:
        days += 365
        leapy -= 1
    year += leapy
    month = 12
    for i in range(12):
        if days < _MDO[i + 1]:
            month = i
            break
    day = days - _MDO[month] + 1
    if month >= 10:
        year += 1
    tp[:3] = [year, (month + 2) % 12 + 1, day]
    if units == DAYS:
        return tp
    if units == HOURS:
        tp[3] = _tmod(v, 24)
        return tp
    if units == MINUTES:
        tp[3] = _tmod(_tdiv(v, 60), 24)
        tp[4] = _tmod(v, 60)
        return tp
    per_s = {SECONDS: 1, MS: 10**3, US: 10**6, NS: 10**9}[units]
    tp[3] = _tmod(_tdiv(v, 3600 * per_s), 24)
    tp[4] = _tmod(_tdiv(v, 60 * per_s), 60)
    tp[5] = _tmod(_tdiv(v, per_s), 60)
    if units != SECONDS:
        tp[6] = _tmod(v, per_s)
    return tp


def _int2str(n, val):
    return b"0" * n if val <= 0 else str(val).encode()[-n:].rjust(n, b"0") if n else b""


def format_value(v, items, units):
    year, month, day, hour, minute, second, sub = dissect(v, units)
    out = []
    for spec, lit, w in items:
        if spec is None:
            out.append(lit)
        elif spec == "Y":
            out.append(_int2str(w, year))
        elif spec == "y":
            out.append(_int2str(w, _s32(year - 1900)))
        elif spec == "m":
            out.append(_int2str(w, month))
        elif spec in "dj":
            out.append(_int2str(w, day))
        elif spec == "H":
            out.append(_int2str(w, hour))
        elif spec == "I":
            out.append(_int2str(w, _tmod(hour, 12)))
        elif spec == "M":
            out.append(_int2str(w, minute))
        elif spec == "S":
            out.append(_int2str(w, second))
        elif spec == "f":
            out.append(_int2str(w, sub))
        elif spec == "p":
            out.append(b"AM" if hour <= 12 else b"PM")
        elif spec == "Z":
            out.append(b"UTC")
    return b"".join(out)


def format_column(values, nulls=None, fmt=None, units=SECONDS):
    """int64 values -> list of bytes / None (nulls: LSB-first validity bytes)"""
    items = compile_format(fmt, units)
    out = []
    for i, v in enumerate(np.asarray(values, dtype=np.int64).tolist()):
        if nulls is not None and not (nulls[i >> 3] >> (i & 7)) & 1:
            out.append(None)
        else:
            out.append(format_value(v, items, units))
    return out


# ---- generated inputs ---------------------------------------------------------------------------------------------------
FORMATS = [None, b"%Y-%m-%d", b"%Y-%m-%dT%H:%M:%S.%fZ", b"%m/%d/%y %I:%M %p", b"%Y%m%d%H%M%S%f", b"%d.%m.%Y %H:%M:%S%z",
           b"%j %Y %%%Z", b"%Y-%m-%d %a", b"literal only", b"%I%p %U", b"%y-%m-%dT%H:%M:%S%z %Z"]
_PIECES = [b"-", b"+", b":", b".", b"T", b"Z", b"UTC", b"utc", b"Utc", b"PM", b"pm", b"AM", b"am", b"%", b" ", b"0", b"00", b"1",
           b"12", b"13", b"31", b"59", b"60", b"99", b"1970", b"2019", b"9999", b"0000", b"-0530", b"+1245", b"x", b"\x00", b"\x80",
           b"\xc3\xa9", b"\xe2\x82\xac", b"\xff", b"123456789", b"2019-03-20", b"2019-03-20T12:34:56Z", b"1969-12-31T23:59:59Z"]


def gen_rows(n, seed, null_every=37, empty_every=41):
    """n rows: well-formed timestamps (shortened, lengthened, corrupted), and junk built from pieces"""
    rng = np.random.default_rng(seed)
    secs = rng.integers(-(10**10), 10**11, size=n)
    kind = rng.integers(0, 6, size=n)
    cut = rng.integers(0, 30, size=n)
    k = rng.integers(1, 7, size=n)
    picks = rng.integers(0, len(_PIECES), size=int(k.sum()))
    pos = rng.integers(0, 1 << 30, size=n)
    rows, j = [], 0
    fmts = [f for f in FORMATS if f is not None]
    for i in range(n):
        if null_every and i % null_every == 3:
            rows.append(None)
        elif empty_every and i % empty_every == 5:
            rows.append(b"")
        else:
            if kind[i] <= 2:
                r = format_value(int(secs[i]), compile_format(fmts[int(pos[i]) % len(fmts)] if kind[i] == 2 else None, SECONDS), SECONDS)
                if kind[i] == 1:
                    r = r[:cut[i]]
            else:
                r = b"".join(_PIECES[p] for p in picks[j:j + k[i]])
                if kind[i] == 5:
                    r = b"2019-03-20T12:34:56Z"[: cut[i]] + r
            if kind[i] == 0 and cut[i] < 8 and r:
                b = bytearray(r)
                b[int(pos[i]) % len(b)] = int(pos[i] >> 8) & 0xFF  # one byte corrupted
                r = bytes(b)
            rows.append(r)
        j += k[i]
    return rows


def gen_values(n, seed):
    """int64 values: random bit patterns, plausible epochs in every unit, and the edges"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-(1 << 63), (1 << 63) - 1, size=n, dtype=np.int64, endpoint=True)
    small = rng.integers(0, 3, size=n) == 0
    v[small] = rng.integers(-(10**12), 10**18, size=int(small.sum()), dtype=np.int64)
    tiny = rng.integers(0, 5, size=n) == 0
    v[tiny] = rng.integers(-100000, 3000000, size=int(tiny.sum()), dtype=np.int64)
    edges = [0, 1, -1, (1 << 63) - 1, -(1 << 63), (1 << 31) - 1, -(1 << 31), 1 << 31, (1 << 32) - 1, 1 << 32, 719468, -719468,
             -719469, 2147483647 - 719468, 2147483648 - 719468, 86399, 86400, -86400, -86401, 951782400, 4107542400,
             253402300799, 253402300800, 9223372036, 1553085296, 1582934400]
    for i, e in enumerate(edges):
        v[i] = e
    return v


def to_arrow(rows):
    """list of bytes / None -> (chars u8, offsets i64, null flags u8)"""
    lens = np.array([0 if r is None else len(r) for r in rows], dtype=np.int64)
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = np.frombuffer(b"".join(r for r in rows if r is not None), dtype=np.uint8)
    nulls = np.array([r is None for r in rows], dtype=np.uint8)
    return chars, offs, nulls


# ---- the CPU harness: datetime_ops.h compiled by the host compiler ------------------------------------------------------------
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "datetime_ops.h"
using namespace csdt;
static std::vector<char> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) exit(2);
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> b(n + 64);
  if (fread(b.data(), 1, n, f) != (size_t)n) exit(3);
  fclose(f);
  return b;
}
// compile: harness compile UNITS FORMAT|- out      (writes the status, then W)
// parse:   harness parse UNITS FORMAT|- rows chars offsets nulls out
// format:  harness format UNITS FORMAT|- rows values out   (every row W bytes)
int main(int argc, char** argv) {
  std::string op = argv[1];
  const int units = atoi(argv[2]);
  const char* fmt = strcmp(argv[3], "-") ? argv[3] : nullptr;
  FILE* out = fopen(argv[argc - 1], "wb");
  TsProgram prog;
  const int st = compile_ts_format(fmt, units, &prog);
  if (op == "compile") {
    int r[2] = {st, st == TS_OK ? prog.width : -1};
    fwrite(r, 4, 2, out);
    fclose(out);
    return 0;
  }
  if (st != TS_OK) return 6;
  const long rows = atol(argv[4]);
  if (op == "parse") {
    std::vector<char> c = slurp(argv[5]), o = slurp(argv[6]), nl = slurp(argv[7]);
    const long long* off = (const long long*)o.data();
    const uint8_t* p = (const uint8_t*)c.data();
    std::vector<int64_t> res(rows);
    ts_dispatch(units, [&](auto u) {
      constexpr int U = decltype(u)::value;
      for (long r = 0; r < rows; ++r)
        res[r] = nl[r] ? 0 : parse_ts_row<U>(p + off[r], (int)(off[r + 1] - off[r]), prog);
      return 0;
    });
    fwrite(res.data(), 8, rows, out);
  } else {
    std::vector<char> v = slurp(argv[5]);
    std::vector<char> buf((size_t)rows * prog.width + 1);
    ts_dispatch(units, [&](auto u) {
      constexpr int U = decltype(u)::value;
      for (long r = 0; r < rows; ++r) {
        int64_t x;
        memcpy(&x, v.data() + 8 * r, 8);
        format_ts_row<U>(x, prog, buf.data() + (size_t)r * prog.width);
      }
      return 0;
    });
    fwrite(buf.data(), 1, (size_t)rows * prog.width, out);
  }
  fclose(out);
  return 0;
}
"""


class Harness:
    """datetime_ops.h built with g++ into `workdir`"""

    def __init__(self, workdir, root):
        import os
        import subprocess

        self.dir = workdir
        src = os.path.join(workdir, "dt_harness.cpp")
        self.exe = os.path.join(workdir, "dt_harness")
        open(src, "w").write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "custrings_amd", "csrc"), src, "-o", self.exe],
                       check=True)

    def _run(self, args):
        import os
        import subprocess

        out = os.path.join(self.dir, "dt_out.bin")
        subprocess.run([self.exe] + [a if isinstance(a, (str, bytes)) else str(a) for a in args] + [out], check=True, timeout=600)
        return open(out, "rb").read()

    @staticmethod
    def _fmt(fmt):
        return "-" if fmt is None else fmt

    def compile(self, fmt, units):
        """-> (status, W): status 0 ok, else the TsCompile code"""
        st, w = np.frombuffer(self._run(["compile", units, self._fmt(fmt)]), dtype=np.int32)
        return int(st), int(w)

    def parse(self, rows, fmt=None, units=SECONDS):
        import os

        chars, offs, nulls = to_arrow(rows)
        paths = []
        for name, a in (("c", chars), ("o", offs), ("n", nulls)):
            p = os.path.join(self.dir, "dt_" + name + ".bin")
            np.ascontiguousarray(a).tofile(p)
            paths.append(p)
        return np.frombuffer(self._run(["parse", units, self._fmt(fmt), len(rows)] + paths), dtype=np.int64)

    def format(self, values, fmt=None, units=SECONDS):
        """-> one bytes object of len(values) x W"""
        import os

        p = os.path.join(self.dir, "dt_v.bin")
        np.ascontiguousarray(values, dtype=np.int64).tofile(p)
        return self._run(["format", units, self._fmt(fmt), len(values), p])
