"""An independent Python restatement of the substring / padding / wrapping ops (reference: cpp/src/strings/substr.cu,
pad.cu, modify.cu:35-106,494-552), over characters of decoded rows, with the reference's quirks (unsigned character
positions, slice_replace's signed / unsigned compare, insert's signed one, zfill of non-numeric rows, wrap's rule) and
the one intended deviation: a strided slice takes characters start, start + step, ... below stop.  Plus the g++ harness
of custrings_amd/csrc/pad_ops.h (the text the kernels compile) and generated rows."""
import os
import subprocess

import numpy as np

U32 = 0xFFFFFFFF
OPS = {"slice": 0, "slice_replace": 1, "insert": 2, "repeat": 3, "rjust": 4, "ljust": 5, "center": 6, "zfill": 7, "wrap": 8}


def u32(x):
    return x & U32


def i32(x):
    x &= U32
    return x - (1 << 32) if x >= 1 << 31 else x


def slice_row(s, start, stop=-1, step=1):
    n = len(s)
    e = n if i32(stop) <= 0 else u32(stop)
    a, z = min(u32(start), n), min(e, n)
    if a >= z:
        return ""
    st = u32(step)
    return s[a:z] if st <= 1 else s[a:z:st]


def slice_replace_row(s, repl, start, stop):
    n = len(s)
    if u32(start) < n:  # (int) start < (unsigned) chars_count
        pos, end = u32(start), min(u32(stop), n)
        if pos > end:
            return s
        return s[:pos] + repl + s[end:]
    return s + repl


def insert_row(s, repl, start):
    n = len(s)
    if i32(start) > n:
        return s
    pos = n if i32(start) < 0 else i32(start)
    return s[:pos] + repl + s[pos:]


def repeat_row(s, count):
    return s * max(u32(count), 1)


def fill_of(fillchar):
    if not fillchar:
        return " "
    return fillchar[0]


def pad_row(s, width, side, fillchar=None):
    f = fill_of(fillchar)
    width = u32(width)
    n = len(s)
    if width <= n:
        return s
    pad = width - n
    if side == "left":
        return f * pad + s
    if side == "right":
        return s + f * pad
    left = pad // 2
    return f * left + s + f * (pad - left)


def zfill_row(s, width):
    width = u32(width)
    if width <= len(s):
        return s
    pos = 1 if s[:1] in ("-", "+") else 0
    return s[:pos] + "0" * (width - len(s)) + s[pos:]


def wrap_row(s, width):
    width = u32(width)
    out = list(s)
    last, spos = -1, 0
    for pos, ch in enumerate(s):
        if ord(ch) <= 0x20:
            out[pos] = " "
            last = pos
        if pos - spos >= width and last >= 0:
            out[last] = "\n"
            spos, last = last, -1
    return "".join(out)


def apply(op, row, args, row_args=None):
    """one row (str or None) through `op` with the member's positional arguments (slice_from: row_args = (start, stop))"""
    if row is None:
        return None
    if op == "get":
        return slice_row(row, u32(args[0]), u32(args[0] + 1))
    if op == "slice":
        return slice_row(row, *args)
    if op == "slice_from":
        return slice_row(row, *row_args)
    if op == "slice_replace":
        return slice_replace_row(row, *args)
    if op == "insert":
        return insert_row(row, *args)
    if op == "repeat":
        return repeat_row(row, *args)
    if op in ("ljust", "rjust", "center"):
        return pad_row(row, args[0], {"ljust": "right", "rjust": "left", "center": "both"}[op], *args[1:])
    if op == "pad":
        return pad_row(row, args[0], args[1] if len(args) > 1 else "left", *args[2:])
    if op == "zfill":
        return zfill_row(row, *args)
    if op == "wrap":
        return wrap_row(row, *args)
    raise ValueError(op)


def apply_column(op, rows, args, starts=None, stops=None):
    """rows of bytes / None -> rows of bytes / None"""
    out = []
    for i, r in enumerate(rows):
        ra = None
        if op == "slice_from":
            ra = (0 if starts is None else int(starts[i]), -1 if stops is None else int(stops[i]))
        s = apply(op, None if r is None else r.decode("utf-8"), args, ra)
        out.append(None if s is None else s.encode("utf-8"))
    return out


# ---- generated rows ----------------------------------------------------------------------------------------------------------
ALPHABET = ["a", "b", "Z", "0", "7", "-", "+", " ", "\t", "\n", ".", "é", "ñ", "ß", "€", "中", "😀", "\x01"]


def gen_rows(n, seed, maxlen=24, null_rate=0.05):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, size=n)
    lens[rng.random(n) < 0.05] = 0
    picks = rng.integers(0, len(ALPHABET), size=int(lens.sum()))
    nulls = rng.random(n) < null_rate
    rows, k = [], 0
    for i in range(n):
        L = int(lens[i])
        rows.append(None if nulls[i] else "".join(ALPHABET[j] for j in picks[k:k + L]).encode())
        k += L
    return rows


def to_arrow(rows):
    """-> chars uint8, offsets int64 (rows + 1), nulls uint8 (1 = null)"""
    lens = np.array([0 if r is None else len(r) for r in rows], dtype=np.int64)
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = np.frombuffer(b"".join(r for r in rows if r is not None), dtype=np.uint8)
    nulls = np.array([r is None for r in rows], dtype=np.uint8)
    return chars, offs, nulls


# ---- the harness: pad_ops.h built with g++ -----------------------------------------------------------------------------------
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pad_ops.h"
template <class T> static std::vector<T> slurp(const char* path) {
  std::vector<T> v;
  if (!strcmp(path, "-")) return v;
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize(n / sizeof(T) + 1);
  if (n && fread(v.data(), 1, n, f) != (size_t)n) exit(2);
  v.resize(n / sizeof(T));
  return v;
}
// harness OP START STOP STEP WIDTH REPS FILL REPL CHARS OFFS NULLS STARTS STOPS OUT
// OUT: int64 length per row (-1 null, -2 a row of 2^31 bytes or more), then the rows' bytes
int main(int argc, char** argv) {
  if (argc != 15) return 2;
  cspad::Params P{};
  P.op = atoi(argv[1]);
  P.start = (int)strtol(argv[2], 0, 10);
  P.stop = (int)strtol(argv[3], 0, 10);
  P.step = (unsigned)strtoll(argv[4], 0, 10);
  P.width = (unsigned)strtoll(argv[5], 0, 10);
  P.reps = (unsigned)strtoll(argv[6], 0, 10);
  std::vector<uint8_t> fill = slurp<uint8_t>(argv[7]), repl = slurp<uint8_t>(argv[8]);
  fill.push_back(0);
  cspad::set_fill(P, (const char*)fill.data());
  if (P.op == cspad::OP_ZFILL) { P.fill = '0'; P.fillw = 1; }
  P.replen = (int)repl.size();
  repl.push_back(0);
  P.repl = repl.data();
  std::vector<uint8_t> chars = slurp<uint8_t>(argv[9]), nulls = slurp<uint8_t>(argv[11]);
  std::vector<int64_t> offs = slurp<int64_t>(argv[10]);
  std::vector<int32_t> starts = slurp<int32_t>(argv[12]), stops = slurp<int32_t>(argv[13]);
  const size_t rows = offs.size() - 1;
  chars.resize(chars.size() + 16, 0);
  std::vector<int64_t> lens(rows);
  std::vector<uint8_t> out;
  for (size_t r = 0; r < rows; ++r) {
    if (nulls[r]) { lens[r] = -1; continue; }
    const uint8_t* p = chars.data() + offs[r];
    const int n = (int)(offs[r + 1] - offs[r]);
    const int st = starts.empty() ? P.start : starts[r], sp = stops.empty() ? P.stop : stops[r];
    const cspad::Pieces pc = cspad::plan_row(P, p, n, st, sp);
    const int64_t sz = cspad::out_size(P, pc, p);
    if (sz >= ((int64_t)1 << 31)) { lens[r] = -2; continue; }
    lens[r] = sz;
    const size_t at = out.size();
    out.resize(at + sz);
    cspad::write_row(P, pc, p, n, out.data() + at);
  }
  FILE* f = fopen(argv[14], "wb");
  fwrite(lens.data(), 8, rows, f);
  fwrite(out.data(), 1, out.size(), f);
  fclose(f);
  return 0;
}
"""


class Harness:
    """pad_ops.h built with g++ into `workdir`"""

    def __init__(self, workdir, root):
        self.dir = workdir
        src = os.path.join(workdir, "pad_harness.cpp")
        self.exe = os.path.join(workdir, "pad_harness")
        open(src, "w").write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "custrings_amd", "csrc"), src, "-o", self.exe],
                       check=True)

    def _file(self, name, data):
        if data is None:
            return "-"
        p = os.path.join(self.dir, name)
        if isinstance(data, (bytes, bytearray)):
            open(p, "wb").write(data)
        else:
            np.ascontiguousarray(data).tofile(p)
        return p

    def run_arrow(self, op, chars, offs, nulls, start=0, stop=-1, step=1, width=0, reps=0, fill=None, repl=None,
                  starts=None, stops=None):
        """-> (lengths int64: -1 null, -2 too long; chars uint8)"""
        code = OPS[op]
        args = [str(code), str(i32(start)), str(i32(stop)), str(u32(step)), str(u32(width)), str(u32(reps)),
                self._file("fill.bin", fill if fill is not None else b""), self._file("repl.bin", repl),
                self._file("c.bin", chars), self._file("o.bin", offs), self._file("n.bin", nulls),
                self._file("s.bin", None if starts is None else np.asarray(starts, dtype=np.int32)),
                self._file("e.bin", None if stops is None else np.asarray(stops, dtype=np.int32))]
        out = os.path.join(self.dir, "out.bin")
        subprocess.run([self.exe] + args + [out], check=True, timeout=900)
        data = np.fromfile(out, dtype=np.uint8)
        rows = len(offs) - 1
        lens = data[:8 * rows].view(np.int64)
        return lens, data[8 * rows:]

    def run(self, op, rows, **kw):
        """rows of bytes / None -> rows of bytes / None ("RANGE" for a row of 2^31 bytes or more)"""
        chars, offs, nulls = to_arrow(rows)
        lens, out = self.run_arrow(op, chars, offs, nulls, **kw)
        res, k = [], 0
        for L in lens.tolist():
            if L == -1:
                res.append(None)
            elif L == -2:
                res.append("RANGE")
            else:
                res.append(out[k:k + L].tobytes())
                k += L
        return res


def member_args(op, args, api):
    """a golden case's arguments in the member's order: the Python API has (start, stop, repl) for slice_replace, (start,
    repl) for insert and None for slice's defaults"""
    args = list(args)
    if api == "python":
        if op == "slice_replace":
            a = args + [None] * (3 - len(args))
            args = [a[2], 0 if a[0] is None else a[0], -1 if a[1] is None else a[1]]
        elif op == "insert":
            a = args + [None] * (2 - len(args))
            args = [a[1], 0 if a[0] is None else a[0]]
    if op == "slice":
        a = args + [None] * (3 - len(args))
        args = [a[0], -1 if a[1] is None else a[1], 1 if a[2] is None else a[2]]
    return args


def member_kwargs(op, args):
    """the member's positional arguments -> (harness op, harness keywords)"""
    if op == "get":
        return "slice", dict(start=args[0], stop=args[0] + 1)
    if op == "slice":
        a = list(args) + [None, None]
        return "slice", dict(start=a[0], stop=-1 if a[1] is None else a[1], step=1 if a[2] is None else a[2])
    if op == "slice_replace":
        return "slice_replace", dict(repl=args[0].encode(), start=args[1], stop=args[2])
    if op == "insert":
        return "insert", dict(repl=args[0].encode(), start=args[1])
    if op == "repeat":
        return "repeat", dict(reps=args[0])
    if op in ("ljust", "rjust", "center"):
        return op, dict(width=args[0], fill=(args[1] if len(args) > 1 else " ").encode())
    if op == "pad":
        side = args[1] if len(args) > 1 else "left"
        return {"left": "rjust", "right": "ljust", "both": "center"}[side], dict(width=args[0], fill=(args[2] if len(args) > 2 else " ").encode())
    if op in ("zfill", "wrap"):
        return op, dict(width=args[0])
    raise ValueError(op)
