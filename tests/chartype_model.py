"""A model of the character-type predicates and of swapcase / capitalize / title, written over CHARACTERS (Python str) from
the semantics of DESIGN.md section 4e, with the tables of tools/unicode_tables.build(); the generators of the test columns;
and the g++ harness of custrings_amd/csrc/chartype_ops.h (the text the kernels compile), which works on bytes."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import unicode_tables  # noqa: E402

PREDS = ["isalnum", "isalpha", "isdigit", "isspace", "isdecimal", "isnumeric", "islower", "isupper", "is_empty"]
CASE_OPS = ["swapcase", "capitalize", "title"]
MEMBERS = PREDS + CASE_OPS
DECIMAL, NUMERIC, DIGIT, ALPHA, SPACE, UPPER, LOWER = 1, 2, 4, 8, 16, 32, 64
MASKS = {"isalnum": 15, "isalpha": ALPHA, "isdigit": DIGIT, "isspace": SPACE, "isdecimal": DECIMAL, "isnumeric": NUMERIC}

_tables = None


def tables():
    global _tables
    if _tables is None:
        f, c = unicode_tables.build()
        _tables = (f.tolist(), c.tolist())
    return _tables


def flags_of(ch):
    cp = ord(ch)
    return tables()[0][cp] if cp <= 0xFFFF else 0


def predicate(op, row):
    """row: str or None -> bool (what the device buffer holds: a null row is False, True for is_empty)"""
    if op == "is_empty":
        return row is None or row == ""
    if row is None or row == "":
        return False
    if op in MASKS:
        return all(flags_of(ch) & MASKS[op] for ch in row)
    bit = LOWER if op == "islower" else UPPER
    return all((not flags_of(ch) & ALPHA) or (flags_of(ch) & bit) for ch in row)


def case_op(op, row):
    """row: str or None -> str or None"""
    if row is None:
        return None
    cases = tables()[1]
    out = []
    if op == "swapcase":
        for ch in row:
            out.append(chr(cases[ord(ch)]) if flags_of(ch) & (UPPER | LOWER) else ch)
    elif op == "capitalize":
        for i, ch in enumerate(row):
            f = flags_of(ch)
            if (f & LOWER) if i == 0 else (f & UPPER):
                ch = chr(cases[ord(ch)]) if ord(ch) <= 0x0FFF else ch  # (the reference's bound: 0x00FFF)
            out.append(ch)
    else:
        capnext = True
        for ch in row:
            f = flags_of(ch)
            if not f & ALPHA:
                capnext = True
            else:
                if (f & LOWER) if capnext else (f & UPPER):
                    ch = chr(cases[ord(ch)])
                capnext = False
            out.append(ch)
    return "".join(out)


def apply(op, row):
    return predicate(op, row) if op in PREDS else case_op(op, row)


def api_column(op, rows):
    """what the Python API's host list holds: None for a null row, for the predicates too"""
    return [None if r is None else apply(op, r) for r in rows]


def width_changing():
    """the cased BMP code points whose opposite-case character has another UTF-8 width"""
    f, c = tables()
    w = lambda u: 1 if u < 0x80 else 2 if u < 0x800 else 3  # noqa: E731
    return [u for u in range(65536) if f[u] & (UPPER | LOWER) and w(u) != w(c[u])]


# ---- generated columns ---------------------------------------------------------------------------------------------------------
ASCII_WORDS = ["the", "Quick", "BROWN", "fox", "o'neil", "mc-donald", "1st", "42", "2019", "a1b", "X", "z", "Hello", "wORLD", "tab\tsep",
               "0", "007", "3.14", "-34", "snake_case", "CamelCase", "ALLCAPS", "lower", "\x1c", "\x1f", "\r\n", " ", "  "]
KEEP = ["é", "É", "ñ", "Ü", "ö", "à", "Ω", "ω", "Д", "д", "¼", "³", "²", "٣", "Ⅰ", "ⅰ", " ", " ", "€", "語", "Ａ", "ａ",
        "Ḁ", "ა", "\U0001F600", "\U00010400"]


def _alphabets():
    wide = set(width_changing())
    keep = [k for k in KEEP if k and all(ord(ch) not in wide for ch in k)]
    change = [chr(u) for u in (0xDF, 0x130, 0x131, 0x17F, 0x212A, 0x23A, 0x2C65, 0x1E9E, 0x250)]
    assert all(ord(ch) in wide for ch in change)
    return keep, change


def pool(kind, n, seed):
    """n distinct-ish rows (str / None): 'ascii'; 'keep' -- some accents that keep their width in every op; 'wide' -- some
    width-changing characters; 'uniform' -- rows on which a predicate holds (all digits / letters / spaces / ...)"""
    rng = np.random.default_rng(seed)
    keep, change = _alphabets()
    uniform = ["0123456789", "abcdefghijklmnopqrstuvwxyz", "ABCDEFGHIJKLMNOPQRSTUVWXYZ", " \t\r\n\x1c\x1f", "abcXYZ019", "٣²³¼", "éàñω", "ÉÜΩД"]
    rows = []
    for _ in range(n):
        t = rng.random()
        if t < 0.03:
            rows.append(None)
            continue
        if t < 0.06:
            rows.append("")
            continue
        if kind == "uniform" or (kind != "ascii" and t < 0.30) or t < 0.25:
            alpha = uniform[int(rng.integers(0, 5 if kind == "ascii" else len(uniform)))]
            s = "".join(alpha[int(j)] for j in rng.integers(0, len(alpha), size=int(rng.integers(1, 24))))
            if kind == "uniform" and rng.random() < 0.2:
                s += "?"  # (decided at the last character)
        else:
            parts = [ASCII_WORDS[int(j)] for j in rng.integers(0, len(ASCII_WORDS), size=int(rng.integers(1, 6)))]
            s = " ".join(parts) if rng.random() < 0.8 else "".join(parts)
        if kind == "keep" and rng.random() < 0.5:
            at = int(rng.integers(0, len(s) + 1))
            s = s[:at] + keep[int(rng.integers(0, len(keep)))] + s[at:]
        if kind == "wide" and rng.random() < 0.5:
            at = int(rng.integers(0, len(s) + 1))
            s = s[:at] + change[int(rng.integers(0, len(change)))] + s[at:]
        rows.append(s)
    return rows


def gen_rows(n, seed, kind="mixed"):
    """n rows (str / None) for the model: ASCII words, digits, white space, accents, width-changing characters, nulls, empties"""
    kinds = ["ascii", "keep", "wide", "uniform"] if kind == "mixed" else [kind]
    out = []
    for k, kd in enumerate(kinds):
        out += pool(kd, n // len(kinds) + 1, seed * 16 + k)
    return out[:n]


def encode(rows):
    return [None if r is None else (r if isinstance(r, bytes) else r.encode("utf-8", "surrogatepass")) for r in rows]


def to_arrow(rows):
    """rows of bytes / None -> chars uint8, offsets int64 (rows + 1), nulls uint8 (1 = null)"""
    lens = np.array([0 if r is None else len(r) for r in rows], dtype=np.int64)
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = np.frombuffer(b"".join(r for r in rows if r is not None), dtype=np.uint8)
    nulls = np.array([r is None for r in rows], dtype=np.uint8)
    return chars, offs, nulls


def big_column(pool_rows, n, seed, one_in=1, base_rows=None):
    """an n-row column as arrow arrays: every row drawn from `base_rows` (encoded), one row in `one_in` from `pool_rows`"""
    rng = np.random.default_rng(seed)
    base = encode(base_rows if base_rows is not None else pool_rows)
    special = encode(pool_rows)
    idx = rng.integers(0, len(base), size=n)
    pick = rng.integers(0, len(special), size=n)
    take = (rng.integers(0, one_in, size=n) == 0) if one_in > 1 else np.ones(n, dtype=bool)
    rows = [special[p] if t else base[i] for i, p, t in zip(idx.tolist(), pick.tolist(), take.tolist())]
    return rows


# ---- the harness: chartype_ops.h built with g++ ----------------------------------------------------------------------------------
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "chartype_ops.h"
template <class T> static std::vector<T> slurp(const char* path) {
  std::vector<T> v;
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
// harness MODE OP FLAGS CASES CHARS OFFS NULLS OUT
//   MODE seq:  the sequential routines.  OP 0..8: a predicate, OUT one byte a row.  OP 100..102: swapcase / capitalize /
//              title, OUT int64 length per row (-1 null), then the rows' bytes.
//   MODE tile: OP 100..102 the way the tile kernel does it -- the chars buffer in 16-byte pieces through swar_piece
//              (the byte before a piece read from the buffer), then every row: one with a byte >= 0x80 redone with the
//              sequential routine (length -2 when its size would change), any other gets its first byte patched.
int main(int argc, char** argv) {
  if (argc != 9) return 2;
  const bool tile = !strcmp(argv[1], "tile");
  const int op = atoi(argv[2]);
  std::vector<uint8_t> flags = slurp<uint8_t>(argv[3]);
  std::vector<uint16_t> cases = slurp<uint16_t>(argv[4]);
  if (flags.size() != 65536 || cases.size() != 65536) return 3;
  std::vector<uint8_t> chars = slurp<uint8_t>(argv[5]), nulls = slurp<uint8_t>(argv[7]);
  std::vector<int64_t> offs = slurp<int64_t>(argv[6]);
  const size_t rows = offs.size() - 1, nbytes = chars.size();
  chars.resize(nbytes + 32, 0);
  FILE* f = fopen(argv[8], "wb");
  if (op < 100) {
    std::vector<uint8_t> out(rows);
    if (op == cschr::P_EMPTY) {
      for (size_t r = 0; r < rows; ++r) out[r] = nulls[r] || offs[r + 1] == offs[r];
    } else {
      const cschr::PredSpec spec = cschr::make_pred(op, flags.data(), flags.data());
      for (size_t r = 0; r < rows; ++r) out[r] = !nulls[r] && cschr::pred_row(chars.data() + offs[r], (int)(offs[r + 1] - offs[r]), spec);
    }
    fwrite(out.data(), 1, rows, f);
    fclose(f);
    return 0;
  }
  const int cop = op - 100;
  std::vector<int64_t> lens(rows);
  std::vector<uint8_t> out;
  if (!tile) {
    for (size_t r = 0; r < rows; ++r) {
      if (nulls[r]) { lens[r] = -1; continue; }
      const uint8_t* p = chars.data() + offs[r];
      const int n = (int)(offs[r + 1] - offs[r]);
      const int sz = cschr::case_size(p, n, flags.data(), cases.data(), cop);
      lens[r] = sz;
      const size_t at = out.size();
      out.resize(at + sz);
      cschr::case_write(p, n, flags.data(), cases.data(), cop, out.data() + at);
    }
  } else {
    if (!cschr::ascii_plain(flags.data(), cases.data())) return 4;
    std::vector<uint8_t> tilebuf(nbytes + 32, 0);
    for (size_t i = 0; i < nbytes; i += 16) {
      uint32_t q[4], o[4];
      memcpy(q, chars.data() + i, 16);
      cschr::swar_piece(cop, q, i ? chars[i - 1] : 0u, o);
      memcpy(tilebuf.data() + i, o, 16);
    }
    for (size_t r = 0; r < rows; ++r) {
      if (nulls[r]) { lens[r] = -1; continue; }
      const uint8_t* p = chars.data() + offs[r];
      const int n = (int)(offs[r + 1] - offs[r]);
      uint8_t* o = tilebuf.data() + offs[r];
      bool high = false;
      for (int i = 0; i < n; ++i) high |= p[i] >= 0x80;
      lens[r] = n;
      if (high) {
        if (cschr::case_size(p, n, flags.data(), cases.data(), cop) != n) { lens[r] = -2; continue; }
        cschr::case_write(p, n, flags.data(), cases.data(), cop, o);
      } else if (cop != cschr::OP_SWAPCASE && n > 0) {
        o[0] = cschr::ascii_first(p[0]);
      }
      out.insert(out.end(), o, o + n);
    }
  }
  fwrite(lens.data(), 8, rows, f);
  fwrite(out.data(), 1, out.size(), f);
  fclose(f);
  return 0;
}
"""


class Harness:
    """chartype_ops.h built with g++ into `workdir`"""

    def __init__(self, workdir, root=ROOT):
        self.dir = workdir
        src = os.path.join(workdir, "chartype_harness.cpp")
        self.exe = os.path.join(workdir, "chartype_harness")
        open(src, "w").write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "custrings_amd", "csrc"), src, "-o", self.exe],
                       check=True)
        f, c = unicode_tables.build()
        self.flags = os.path.join(workdir, "flags.bin")
        self.cases = os.path.join(workdir, "cases.bin")
        f.tofile(self.flags)
        c.tofile(self.cases)

    def _file(self, name, data):
        p = os.path.join(self.dir, name)
        np.ascontiguousarray(data).tofile(p)
        return p

    def run_arrow(self, op, chars, offs, nulls, mode="seq"):
        """a predicate -> uint8 per row; a case op -> (lengths int64: -1 null, -2 size would change (tile mode); chars uint8)"""
        code = PREDS.index(op) if op in PREDS else 100 + CASE_OPS.index(op)
        out = os.path.join(self.dir, "out.bin")
        subprocess.run([self.exe, mode, str(code), self.flags, self.cases, self._file("c.bin", chars), self._file("o.bin", offs),
                        self._file("n.bin", nulls), out], check=True, timeout=900)
        data = np.fromfile(out, dtype=np.uint8)
        rows = len(offs) - 1
        if op in PREDS:
            return data
        return data[:8 * rows].view(np.int64), data[8 * rows:]

    def run(self, op, rows, mode="seq"):
        """rows of bytes / None -> a predicate: list of bool; a case op: rows of bytes / None ("CHANGED" in tile mode)"""
        chars, offs, nulls = to_arrow(rows)
        res = self.run_arrow(op, chars, offs, nulls, mode)
        if op in PREDS:
            return [bool(x) for x in res.tolist()]
        lens, out = res
        got, k = [], 0
        data = out.tobytes()
        for L in lens.tolist():
            if L == -1:
                got.append(None)
            elif L == -2:
                got.append("CHANGED")
            else:
                got.append(data[k:k + L])
                k += L
        return got
