"""Python restatement of the 14 conversion ops (reference: cpp/src/strings/convert.cu with the parsers of
custring.inl / custring_view.inl), written independently of custrings_amd/csrc/convert_ops.h so the two can be
checked against each other.  Rows are bytes (None = null); floats come back as Python floats / numpy float32."""
import struct

import numpy as np

# P[e + 308]: the double nearest to 10^e (Python's float() of a decimal literal is correctly rounded)
POW10 = [float("1e%d" % e) for e in range(-308, 309)]
U32, U64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
NAN, INF = float("nan"), float("inf")


def _s32(v):
    v &= U32
    return v - (1 << 32) if v >> 31 else v


def _s64(v):
    v &= U64
    return v - (1 << 64) if v >> 63 else v


def hash_(row):
    if row is None:
        return 0
    h, n = 31, len(row)

    def rotl(x, r):
        return ((x << r) | (x >> (32 - r))) & U32

    for i in range(0, n - n % 4, 4):
        k = int.from_bytes(row[i:i + 4], "little")
        k = rotl((k * 0xcc9e2d51) & U32, 15) * 0x1b873593 & U32
        h = (rotl(h ^ k, 13) * 5 + 0xe6546b64) & U32
    tail = row[n - n % 4:]
    if tail:
        k = int.from_bytes(tail, "little")
        h ^= rotl((k * 0xcc9e2d51) & U32, 15) * 0x1b873593 & U32
    h ^= n
    h ^= h >> 16
    h = h * 0x85ebca6b & U32
    h ^= h >> 13
    h = h * 0xc2b2ae35 & U32
    return h ^ (h >> 16)


def stol(row):
    if not row:
        return 0
    i, neg = 0, False
    if row[0] in b"-+":
        neg, i = row[0] == 45, 1
    v = 0
    while i < len(row) and 48 <= row[i] <= 57:
        v = (v * 10 + row[i] - 48) & U64
        i += 1
    return _s64(-v if neg else v)


def stoi(row):
    return _s32(stol(row))


def stod(row):
    if row is None:
        return 0.0
    if row in (b"NaN", b"nan"):
        return NAN
    if row in (b"Inf", b"inf"):
        return INF
    if row in (b"-Inf", b"-inf"):
        return -INF
    if not row:
        return 0.0
    n, i, sign = len(row), 0, 1.0
    if row[0] in b"-+":
        sign, i = (-1.0 if row[0] == 45 else 1.0), 1
    maxm, digits, exp_off, decimal = 0x0FFFFFFFFFFFFF, 0, 0, False
    while i < n:
        c = row[i]
        i += 1
        if c == 46:
            decimal = True
            continue
        if not 48 <= c <= 57:
            i -= 1
            break
        if digits > maxm:
            exp_off += not decimal
        else:
            digits = digits * 10 + c - 48
            if digits > maxm:
                digits //= 10
                exp_off += not decimal
            else:
                exp_off -= decimal
    exp10, exp_sign = 0, 1
    if i < n:
        c = row[i]
        i += 1
        if c in b"eE" and i < n:
            c = row[i]
            i += 1
            if c in b"-+":
                exp_sign = -1 if c == 45 else 1
            while i < n:
                c = row[i]
                i += 1
                if not 48 <= c <= 57:
                    break
                exp10 = _s32(exp10 * 10 + c - 48)
    e = _s32(_s32(exp10 * exp_sign) + exp_off)
    if e > 308:
        return INF if sign > 0 else -INF
    if e < -308:
        return 0.0
    return float(digits) * POW10[e + 308] * sign


def stof(row):
    with np.errstate(over="ignore"):
        return np.float32(stod(row))


def htoi(row):
    if not row:
        return 0
    v, base = 0, 1
    for c in reversed(row):
        if 48 <= c <= 57:
            d = c - 48
        elif 65 <= c <= 90:
            d = c - 55
        elif 97 <= c <= 122:
            d = c - 87
        else:
            continue
        v = (v + d * base) & U64
        base = (base * 16) & U64
    return v & U32


def ip2int(row):
    if not row or row.count(b".") != 3:
        return 0
    vals, iv = [0, 0, 0, 0], 0
    for c in row:
        if 48 <= c <= 57:
            vals[iv] = (vals[iv] * 10 + c - 48) & U32
        elif c == 46:
            iv += 1
    return (vals[0] * 16777216 + vals[1] * 65536 + vals[2] * 256 + vals[3]) & U32


def to_bool(row, true):
    if row is None:
        return true is None
    return true is not None and row == true


def ltos(v):
    return str(int(v)).encode()  # (INT64_MIN prints its digits: deviation 2)


def int2ip(v):
    v = int(v)
    return ("%d.%d.%d.%d" % ((v >> 24) & 255, (v >> 16) & 255, (v >> 8) & 255, v & 255)).encode()


_UP = [10.0, 100.0, 1e4, 1e8, 1e16, 1e32, 1e64, 1e128, 1e256]
_LO = [0.1, 0.01, 1e-4, 1e-8, 1e-16, 1e-32, 1e-64, 1e-128, 1e-256]
_BLO = [1.0, 0.1, 0.001, 1e-7, 1e-15, 1e-31, 1e-63, 1e-127, 1e-255]


def dtos(value):
    value = float(value)
    if value != value:
        return b"NaN"
    neg = value < 0.0
    if neg:
        value = -value
    if value == INF:
        return b"-Inf" if neg else b"Inf"
    places, exp10 = 9, 0
    if value > 1e9:
        fx = 256
        for k in range(8, -1, -1):
            if value >= _UP[k]:
                value *= _LO[k]
                exp10 += fx
            fx >>= 1
    elif 0.0 < value < 1e-4:
        fx = 256
        for k in range(8, -1, -1):
            if value < _BLO[k]:
                value *= _UP[k]
                exp10 -= fx
            fx >>= 1
    maxd = 1000000000
    integer = int(value)
    i = integer
    while i >= 10:
        places -= 1
        maxd //= 10
        i //= 10
    rem = (value - float(integer)) * float(maxd)
    decimal = int(rem)
    rem -= float(decimal)
    decimal += int(2.0 * rem)
    if decimal >= maxd:
        decimal = 0
        integer += 1
        if exp10 and integer >= 10:
            exp10 += 1
            integer = 1
    while decimal % 10 == 0 and places > 0:
        decimal //= 10
        places -= 1
    out = ("-" if neg else "") + str(integer) + "."
    out += ("%0*d" % (places, decimal)) if places else "0"
    if exp10:
        out += "e" + ("-" if exp10 < 0 else "+") + ("%02d" % abs(exp10))
    return out.encode()


def ftos(value):
    return dtos(float(np.float32(value)))


PARSE = {"hash": hash_, "stoi": stoi, "stol": stol, "stof": stof, "stod": stod, "htoi": htoi, "ip2int": ip2int}
PARSE_DTYPE = {"hash": np.uint32, "stoi": np.int32, "stol": np.int64, "stof": np.float32, "stod": np.float64,
               "htoi": np.uint32, "ip2int": np.uint32, "to_bools": np.uint8}
FORMAT = {"itos": ltos, "ltos": ltos, "ftos": ftos, "dtos": dtos, "int2ip": int2ip}
FORMAT_DTYPE = {"itos": np.int32, "ltos": np.int64, "ftos": np.float32, "dtos": np.float64, "int2ip": np.uint32, "from_bools": np.uint8}


def parse_column(op, rows, true=None):
    """op over a list of bytes / None -> numpy array of the op's result type (null rows: 0 / to_bools' rule)"""
    dt = PARSE_DTYPE[op]
    if op == "to_bools":
        return np.array([to_bool(r, true) for r in rows], dtype=dt)
    f = PARSE[op]
    with np.errstate(over="ignore"):
        return np.array([f(r) if r is not None else 0 for r in rows], dtype=dt)


def nonzero_count(res):
    return int(np.count_nonzero(res != 0))


def bits(a):
    """float results as integers, NaN as the canonical quiet NaN"""
    a = np.asarray(a)
    if a.dtype == np.float32:
        u = a.view(np.uint32).copy()
        u[np.isnan(a)] = 0x7FC00000
        return u
    if a.dtype == np.float64:
        u = a.view(np.uint64).copy()
        u[np.isnan(a)] = 0x7FF8000000000000
        return u
    return a


def hexbits(h, op):
    v = int(h, 16)
    return struct.unpack("<f" if op in ("stof", "ftos") else "<d", v.to_bytes(4 if op in ("stof", "ftos") else 8, "little"))[0]


# ---- generated inputs (shared by tests/test_convert_cpu.py and tests/test_gpu_convert.py) -------------------------------
_PIECES = [b"-", b"+", b".", b"e", b"E", b"e-", b"e+", b"0", b"00", b"1", b"9", b"12", b"255", b"256", b"4294967296",
           b"9223372036854775807", b"9223372036854775808", b"18446744073709551616", b"123456789012345678901234", b"NaN",
           b"Inf", b"-Inf", b"nan", b"inf", b"-inf", b"True", b"true", b"x", b"G", b"z", b"ff", b"CAFE", b"\x00", b"\x80",
           b"\xc3\xa9", b"\xff", b" ", b"e308", b"e309", b"e-308", b"e-309", b"e-330", b"e400", b"192.168.0.1", b"10.0.0.1",
           b"1.2.3", b"...", b"999.999.999.999"]


def gen_rows(n, seed, null_every=37, empty_every=41):
    """n rows (bytes, or None for null) built from number-like pieces, junk, NUL and >= 0x80 bytes"""
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 6, size=n)
    picks = rng.integers(0, len(_PIECES), size=int(k.sum()))
    digits = rng.integers(0, 10**9, size=n)
    rows, j = [], 0
    for i in range(n):
        if null_every and i % null_every == 3:
            rows.append(None)
        elif empty_every and i % empty_every == 5:
            rows.append(b"")
        else:
            parts = [_PIECES[p] for p in picks[j:j + k[i]]]
            if i % 3 == 0:
                parts.insert(int(digits[i]) % (len(parts) + 1), str(int(digits[i])).encode())
            rows.append(b"".join(parts))
        j += k[i]
    return rows


def gen_values(op, n, seed):
    """values for a format op: random bit patterns plus the edges (INT_MIN, LONG_MIN, subnormals, NaN, +-inf, +-0,
    the normaliser's 1e9 / 1e-4 limits, values that round up to 10)"""
    rng = np.random.default_rng(seed)
    dt = FORMAT_DTYPE[op]
    if op == "from_bools":
        return rng.integers(0, 2, size=n).astype(np.uint8)
    if dt in (np.float32, np.float64):
        ib = np.uint32 if dt == np.float32 else np.uint64
        v = rng.integers(0, np.iinfo(ib).max, size=n, dtype=ib, endpoint=True).view(dt).copy()
        edges = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e9, -1e9, 1e9 * (1 + 1e-15), 1e-4, 9.9999e-5, 0.0001000001,
                 9.9999999999, 99999.999999, 999999999.5, 9999999999.5, 1.5e-45, 5e-324, 2.2250738585072014e-308,
                 1.7976931348623157e308, 3.4028234663852886e38, 1.0, 0.1, 123.456, 9.999999999e22]
        with np.errstate(over="ignore"):
            for i, e in enumerate(edges):
                v[i] = e
        m = rng.integers(0, 4, size=n) == 0  # a quarter of moderate decimals
        v[m] = (rng.standard_normal(int(m.sum())) * 10.0 ** rng.integers(-12, 12, size=int(m.sum()))).astype(dt)
        return v
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max, size=n, dtype=dt, endpoint=True)
    edges = [0, info.min, info.max, -1, 1, 9, 10, 99, 100, 255, 256] if info.min < 0 else [0, info.max, 1, 255, 256, 0x0A000001]
    for i, e in enumerate(edges):
        v[i] = e
    small = rng.integers(0, 3, size=n) == 0
    v[small] = rng.integers(-1000 if info.min < 0 else 0, 1000, size=int(small.sum())).astype(dt)
    return v


def format_column(op, values, nulls=None, true=b"True", false=b"False"):
    """op over numpy values -> list of bytes / None (nulls: LSB-first validity bytes)"""
    out = []
    f = FORMAT.get(op)
    for i, v in enumerate(values.tolist()):
        if nulls is not None and not (nulls[i >> 3] >> (i & 7)) & 1:
            out.append(None)
        elif op == "from_bools":
            out.append(true if v else false)
        else:
            out.append(f(v))
    return out


def to_arrow(rows):
    """list of bytes / None -> (chars u8, offsets i64, null flags u8)"""
    lens = np.array([0 if r is None else len(r) for r in rows], dtype=np.int64)
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = np.frombuffer(b"".join(r for r in rows if r is not None), dtype=np.uint8)
    nulls = np.array([r is None for r in rows], dtype=np.uint8)
    return chars, offs, nulls


# ---- the CPU harness: convert_ops.h compiled by the host compiler -----------------------------------------------------------
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "convert_ops.h"
using namespace csconv;
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
// parse:  harness OP rows chars offsets nulls true|- out
// format: harness OP rows values - - true false out   (writes int32 lengths, then the chars)
int main(int argc, char** argv) {
  std::string op = argv[1];
  long rows = atol(argv[2]);
  FILE* out = fopen(argv[argc - 1], "wb");
  if (op == "itos" || op == "ltos" || op == "ftos" || op == "dtos" || op == "int2ip" || op == "from_bools") {
    std::vector<char> v = slurp(argv[3]);
    std::string t = argv[6], fs = argv[7];
    std::vector<int> lens(rows);
    std::string chars;
    for (long r = 0; r < rows; ++r) {
      char buf[64];
      int n = 0;
      if (op == "itos") { int x; memcpy(&x, v.data() + 4 * r, 4); n = ltos_row(x, buf); }
      else if (op == "ltos") { long long x; memcpy(&x, v.data() + 8 * r, 8); n = ltos_row(x, buf); }
      else if (op == "ftos") { float x; memcpy(&x, v.data() + 4 * r, 4); n = ftos_row(x, buf); }
      else if (op == "dtos") { double x; memcpy(&x, v.data() + 8 * r, 8); n = dtos_row(x, buf); }
      else if (op == "int2ip") { unsigned x; memcpy(&x, v.data() + 4 * r, 4); n = int2ip_row(x, buf); }
      else { const std::string& s = v[r] ? t : fs; n = (int)s.size(); memcpy(buf, s.data(), n); }
      if (n > kMaxNumWidth && op != "from_bools") return 4;
      lens[r] = n;
      chars.append(buf, n);
    }
    fwrite(lens.data(), 4, rows, out);
    fwrite(chars.data(), 1, chars.size(), out);
  } else {
    std::vector<char> c = slurp(argv[3]), o = slurp(argv[4]), nl = slurp(argv[5]);
    const long long* off = (const long long*)o.data();
    const uint8_t* p = (const uint8_t*)c.data();
    std::string t = argv[6];
    const bool has_t = t != "-";
    for (long r = 0; r < rows; ++r) {
      const bool ok = !nl[r];
      const uint8_t* s = p + off[r];
      const int n = ok ? (int)(off[r + 1] - off[r]) : 0;
      if (op == "hash") { unsigned x = ok ? hash_row(s, n) : 0; fwrite(&x, 4, 1, out); }
      else if (op == "stoi") { int x = ok ? stoi_row(s, n) : 0; fwrite(&x, 4, 1, out); }
      else if (op == "stol") { long long x = ok ? stol_row(s, n) : 0; fwrite(&x, 8, 1, out); }
      else if (op == "stof") { float x = ok ? stof_row(s, n) : 0.f; fwrite(&x, 4, 1, out); }
      else if (op == "stod") { double x = ok ? stod_row(s, n) : 0.0; fwrite(&x, 8, 1, out); }
      else if (op == "htoi") { unsigned x = ok ? htoi_row(s, n) : 0; fwrite(&x, 4, 1, out); }
      else if (op == "ip2int") { unsigned x = ok ? ip2int_row(s, n) : 0; fwrite(&x, 4, 1, out); }
      else if (op == "to_bools") {
        uint8_t x = ok ? to_bool_row(s, n, has_t ? (const uint8_t*)t.data() : nullptr, (int)t.size()) : (uint8_t)!has_t;
        fwrite(&x, 1, 1, out);
      } else return 5;
    }
  }
  fclose(out);
  return 0;
}
"""


class Harness:
    """convert_ops.h built with g++ into `workdir` (contraction off, as the kernels are built)"""

    def __init__(self, workdir, root):
        import os
        import subprocess

        self.dir = workdir
        src = os.path.join(workdir, "harness.cpp")
        self.exe = os.path.join(workdir, "harness")
        open(src, "w").write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(root, "custrings_amd", "csrc"),
                        src, "-o", self.exe], check=True)

    def _run(self, args):
        import os
        import subprocess

        out = os.path.join(self.dir, "out.bin")
        subprocess.run([self.exe] + [str(a) for a in args] + [out], check=True, timeout=600)
        return open(out, "rb").read()

    def parse(self, op, chars, offs, nulls, true=None):
        import os

        n = len(offs) - 1
        paths = []
        for name, a in (("c", chars), ("o", offs), ("n", nulls)):
            p = os.path.join(self.dir, name + ".bin")
            np.ascontiguousarray(a).tofile(p)
            paths.append(p)
        t = "-" if true is None else true.decode()
        return np.frombuffer(self._run([op, n] + paths + [t]), dtype=PARSE_DTYPE[op])

    def format(self, op, values, true=b"True", false=b"False"):
        import os

        p = os.path.join(self.dir, "v.bin")
        np.ascontiguousarray(values, dtype=FORMAT_DTYPE[op]).tofile(p)
        n = len(values)
        raw = self._run([op, n, p, "-", "-", true.decode(), false.decode()])
        lens = np.frombuffer(raw[: 4 * n], dtype=np.int32)
        return lens, raw[4 * n:]
