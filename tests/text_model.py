"""A Python model of the NVText members contains_strings / strings_counts / edit_distance / porter_stemmer_measure /
scatter_count (reference: cpp/src/text/NVText.cu:32-172, edit_distance.cu:33-228, stemmer.cu:29-104; find:
custring_view.inl:476-543), restated over Python strings independently of custrings_amd/csrc/text_ops.h; a harness that builds
that header with g++ (both edit_distance forms selectable); and a row generator.  Valid UTF-8 only: on malformed bytes
text_ops.h is the definition.

The quirks the model restates:
  find compares BYTES at every byte offset of the row and answers with the number of characters that start in front of the
      match; strings_counts restarts chars(target) CHARACTERS behind that answer.  A target whose bytes match across a
      character boundary is found.  A null row, a null target, an empty target: False / 0.
  edit_distance counts characters.  A null or empty row: chars(target) (0 for a null target); a null or empty target: chars(row).
  porter_stemmer_measure: y_char is a consonant at index 0 or behind a vowel, else it counts as a vowel; null / empty rows: 0.
  scatter_count: row i repeated counts[i] times, null rows stay null.
"""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEMBERS = ["contains_strings", "strings_counts", "edit_distance", "edit_distance_column", "porter_stemmer_measure", "scatter_count"]


def _b(s):
    return s if isinstance(s, bytes) else s.encode("utf-8")


def _starts(data):
    """characters that start in `data` (bytes that are no continuation byte)"""
    return sum(1 for x in data if (x & 0xC0) != 0x80)


def find(row, target, pos=0):
    """custring_view::find(str, pos): character position of the first byte-wise match at or behind character `pos`, or -1"""
    rb, tb = _b(row), _b(target)
    if not tb:
        return -1
    nchars = _starts(rb)
    if pos >= nchars:
        spos = len(rb) if pos > 0 else 0
    else:  # byte offset of character `pos`
        spos, seen = 0, 0
        while seen < pos:
            spos += 1
            while spos < len(rb) and (rb[spos] & 0xC0) == 0x80:
                spos += 1
            seen += 1
    m = rb.find(tb, spos)
    return -1 if m < 0 else _starts(rb[:m])


def contains(row, target):
    return row is not None and target is not None and find(row, target) >= 0


def count(row, target):
    if row is None or target is None:
        return 0
    n, tch = 0, _starts(_b(target))
    pos = find(row, target)
    while pos >= 0:
        pos = find(row, target, pos + tch)
        n += 1
    return n


def contains_strings(rows, targets):
    return [[contains(r, t) for t in targets] for r in rows]


def strings_counts(rows, targets):
    return [[count(r, t) for t in targets] for r in rows]


def _chars(s):
    return s.decode("utf-8") if isinstance(s, bytes) else s


def levenshtein(a, b):
    """the textbook table, two rows"""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[len(b)]


def edit_distance_pair(row, target):
    if row is None or len(row) == 0:
        return 0 if target is None else len(_chars(target))
    if target is None or len(target) == 0:
        return len(_chars(row))
    return levenshtein(_chars(row), _chars(target))


def edit_distance(rows, target):
    if isinstance(target, (str, bytes)):
        return [edit_distance_pair(r, target) for r in rows]
    if len(target) != len(rows):
        raise ValueError("sizes must match")
    return [edit_distance_pair(r, t) for r, t in zip(rows, target)]


def measure(row, vowels="aeiou", y_char="y"):
    if row is None:
        return 0
    s = _chars(row)
    y = _chars(y_char)[:1]

    def consonant(i):
        if s[i] in vowels:
            return False
        if s[i] != y or i == 0:
            return True
        return s[i - 1] in vowels

    vcs, run = 0, bool(s) and not consonant(0)
    for i in range(len(s)):
        if consonant(i):
            vcs += run
            run = False
        else:
            run = True
    return vcs


def porter_stemmer_measure(rows, vowels="aeiou", y_char="y"):
    return [measure(r, vowels, y_char) for r in rows]


def scatter_count(rows, counts):
    out = []
    for r, c in zip(rows, counts):
        out += [r] * (0 if c is None else int(c))
    return out


def apply_case(case):
    """a case of tests/golden/reference_text.json through the model"""
    op, rows = case["op"], case["input"]
    if op == "contains_strings":
        return contains_strings(rows, case["targets"])
    if op == "strings_counts":
        return strings_counts(rows, case["targets"])
    if op in ("edit_distance", "edit_distance_column"):
        return edit_distance(rows, case["targets"])
    if op == "porter_stemmer_measure":
        return porter_stemmer_measure(rows)
    return scatter_count(rows, case["counts"])


# ---- rows ----------------------------------------------------------------------------------------------------------------
WORDS = ["the", "fox", "yearly", "abbey", "trouble", "a", "I", "sky", "by", "ayy", "queue", "rhythm", "cat ", "dog", "aa", "aaaa", "e", "y"]
WIDE = ["é", "ü", "ñ", "ß", "€", "☃", "日", "本", "ÿ", "à"]


def gen_rows(n, seed, nulls=True):
    """ASCII words, rows with two- and three-byte characters, empty rows and (with `nulls`) null rows"""
    rng = np.random.default_rng(seed)
    kinds = rng.integers(0, 20, size=n)
    counts = rng.integers(1, 6, size=n)
    picks = rng.integers(0, 1 << 30, size=(n, 6))
    rows = []
    for k, c, pk in zip(kinds.tolist(), counts.tolist(), picks.tolist()):
        if k == 0:
            rows.append(None if nulls else "")
        elif k == 1:
            rows.append("")
        elif k < 12:
            rows.append(" ".join(WORDS[p % len(WORDS)] for p in pk[:c]))
        else:
            rows.append("".join((WIDE[p % len(WIDE)] if (p >> 8) % 3 == 0 else WORDS[p % len(WORDS)]) for p in pk[:c]))
    return rows


def letter_rows(n, seed, alphabet, max_len=100):
    """n rows of 0..max_len characters over `alphabet` (a list of str), as arrow arrays (chars, offsets, nulls)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n)
    total = int(lens.sum())
    letters = rng.integers(0, len(alphabet), size=total)
    enc = [a.encode("utf-8") for a in alphabet]
    widths = np.array([len(e) for e in enc], dtype=np.int64)[letters]
    char_off = np.zeros(total + 1, dtype=np.int64)
    np.cumsum(widths, out=char_off[1:])
    chars = np.zeros(int(char_off[-1]), dtype=np.uint8)
    for k, e in enumerate(enc):
        at = char_off[:-1][letters == k]
        for j, byte in enumerate(e):
            chars[at + j] = byte
    row_first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=row_first[1:])
    return chars, char_off[row_first], np.zeros(n, dtype=np.uint8)


def encode(rows):
    return [None if r is None else (r if isinstance(r, bytes) else r.encode("utf-8", "surrogatepass")) for r in rows]


def to_arrow(rows):
    """rows of str / bytes / None -> chars uint8, offsets int64 (rows + 1), nulls uint8 (1 = null)"""
    rows = encode(rows)
    lens = np.array([0 if r is None else len(r) for r in rows], dtype=np.int64)
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    chars = np.frombuffer(b"".join(r for r in rows if r is not None), dtype=np.uint8)
    nulls = np.array([r is None for r in rows], dtype=np.uint8)
    return chars, offs, nulls


# ---- the harness: text_ops.h built with g++ ----------------------------------------------------------------------------------
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "text_ops.h"
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
struct Col {
  std::vector<uint8_t> chars, nulls;
  std::vector<int64_t> offs;
  size_t rows() const { return offs.size() - 1; }
  const uint8_t* p(size_t r) const { return chars.data() + offs[r]; }
  int n(size_t r) const { return nulls[r] ? 0 : (int)(offs[r + 1] - offs[r]); }
  bool ok(size_t r) const { return !nulls[r]; }
  void load(char** a) { chars = slurp<uint8_t>(a[0]); offs = slurp<int64_t>(a[1]); nulls = slurp<uint8_t>(a[2]); chars.resize(chars.size() + 8, 0); }
};
// harness OP FORM  CHARS OFFS NULLS  TCHARS TOFFS TNULLS  A1 A2  OUT
//   contains / counts: OUT uint8 / uint32, rows x targets.   measure: A1 the vowels, A2 y_char; OUT uint32 a row.
//   edit_scalar: every row against target row 0; edit_pairs: row r against target row r.  FORM dp: the one-row dynamic
//       program; FORM bits: the bit-vector form where the target has 1..64 characters (else the dynamic program).  OUT uint32.
//   scatter: A1 a file of uint32 counts; OUT int64: the source row of every output row, over their exclusive scan.
int main(int argc, char** argv) {
  if (argc != 12) return 2;
  const char* op = argv[1];
  const bool bits = !strcmp(argv[2], "bits");
  Col c, t;
  c.load(argv + 3);
  t.load(argv + 6);
  const size_t rows = c.rows(), M = t.rows();
  FILE* f = fopen(argv[11], "wb");
  if (!f) return 2;
  if (!strcmp(op, "contains")) {
    std::vector<uint8_t> out(rows * M);
    for (size_t r = 0; r < rows; ++r)
      for (size_t j = 0; j < M; ++j) out[r * M + j] = c.ok(r) && cstxt::contains_row(c.p(r), c.n(r), t.p(j), t.n(j));
    fwrite(out.data(), 1, out.size(), f);
  } else if (!strcmp(op, "counts")) {
    std::vector<uint32_t> out(rows * M);
    for (size_t r = 0; r < rows; ++r)
      for (size_t j = 0; j < M; ++j) out[r * M + j] = c.ok(r) ? cstxt::count_row(c.p(r), c.n(r), t.p(j), t.n(j)) : 0u;
    fwrite(out.data(), 4, out.size(), f);
  } else if (!strcmp(op, "measure")) {
    std::vector<cstxt::Char> more(strlen(argv[9]) + 1);
    const cstxt::VowelSpec spec = cstxt::make_vowels(argv[9], argv[10], more.data(), (int)more.size(), more.data());
    std::vector<uint32_t> out(rows);
    for (size_t r = 0; r < rows; ++r) out[r] = cstxt::measure_row(c.p(r), c.n(r), spec);
    fwrite(out.data(), 4, out.size(), f);
  } else if (!strcmp(op, "edit_scalar") || !strcmp(op, "edit_pairs")) {
    const bool scalar = !strcmp(op, "edit_scalar");
    if (scalar ? M < 1 : M != rows) return 3;
    std::vector<uint32_t> out(rows);
    std::vector<uint16_t> row;
    cstxt::PeqTable q;
    q.m = 0;
    if (scalar && bits) cstxt::build_peq(t.p(0), t.n(0), q);
    for (size_t r = 0; r < rows; ++r) {
      const size_t j = scalar ? 0 : r;
      if (!scalar && bits) cstxt::build_peq(t.p(j), t.n(j), q);
      if (bits && t.ok(j) && q.m) {
        out[r] = cstxt::edit_distance_bits(c.p(r), c.n(r), q.ascii, q.ch, q.mask, q.nlist, q.m);
        continue;
      }
      row.assign((size_t)cstxt::edit_row_entries(c.p(r), c.n(r), c.ok(r), t.p(j), t.n(j), t.ok(j)) + 1, 0xFFFF);
      out[r] = cstxt::edit_distance_dp(c.p(r), c.n(r), c.ok(r), t.p(j), t.n(j), t.ok(j), row.data());
      if (row.back() != 0xFFFF) return 4;  // (wrote beyond the entries it asked for)
    }
    fwrite(out.data(), 4, out.size(), f);
  } else if (!strcmp(op, "scatter")) {
    std::vector<uint32_t> counts = slurp<uint32_t>(argv[9]);
    if (counts.size() != rows) return 3;
    std::vector<int64_t> scan(rows + 1, 0);
    for (size_t r = 0; r < rows; ++r) scan[r + 1] = scan[r] + counts[r];
    std::vector<int64_t> out((size_t)scan[rows]);
    for (int64_t o = 0; o < scan[rows]; ++o) out[(size_t)o] = cstxt::scatter_source(scan.data(), (int64_t)rows, o);
    fwrite(out.data(), 8, out.size(), f);
  } else {
    return 2;
  }
  fclose(f);
  return 0;
}
"""


class Harness:
    """text_ops.h built with g++ into `workdir`"""

    def __init__(self, workdir, root=ROOT):
        self.dir = workdir
        src = os.path.join(workdir, "text_harness.cpp")
        self.exe = os.path.join(workdir, "text_harness")
        with open(src, "w") as f:
            f.write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "custrings_amd", "csrc"), src, "-o", self.exe], check=True)

    def _files(self, tag, arrow):
        out = []
        for name, data in zip(("c", "o", "n"), arrow):
            p = os.path.join(self.dir, "%s_%s.bin" % (tag, name))
            np.ascontiguousarray(data).tofile(p)
            out.append(p)
        return out

    def run_arrow(self, op, rows, targets=None, form="dp", a1="", a2="", dtype=np.uint32):
        """`rows` / `targets`: arrow triples (chars, offsets, nulls)"""
        if targets is None:
            targets = to_arrow([])
        out = os.path.join(self.dir, "out.bin")
        subprocess.run([self.exe, op, form] + self._files("r", rows) + self._files("t", targets) + [a1, a2, out], check=True, timeout=900)
        return np.fromfile(out, dtype=dtype)

    def contains_strings(self, rows, targets):
        res = self.run_arrow("contains", to_arrow(rows), to_arrow(targets), dtype=np.uint8)
        return [[bool(v) for v in r] for r in res.reshape(len(rows), len(targets)).tolist()]

    def strings_counts(self, rows, targets):
        return self.run_arrow("counts", to_arrow(rows), to_arrow(targets)).reshape(len(rows), len(targets)).tolist()

    def edit_distance(self, rows, target, form="dp"):
        if isinstance(target, (str, bytes)):
            return self.run_arrow("edit_scalar", to_arrow(rows), to_arrow([target]), form).tolist()
        return self.run_arrow("edit_pairs", to_arrow(rows), to_arrow(target), form).tolist()

    def porter_stemmer_measure(self, rows, vowels="aeiou", y_char="y"):
        return self.run_arrow("measure", to_arrow(rows), a1=vowels, a2=y_char).tolist()

    def scatter_count(self, rows, counts):
        p = os.path.join(self.dir, "counts.bin")
        np.array([0 if c is None else c for c in counts], dtype=np.uint32).tofile(p)
        src = self.run_arrow("scatter", to_arrow(rows), a1=p, dtype=np.int64).tolist()
        return [rows[i] for i in src]

    def apply_case(self, case):
        op, rows = case["op"], case["input"]
        if op == "contains_strings":
            return self.contains_strings(rows, case["targets"])
        if op == "strings_counts":
            return self.strings_counts(rows, case["targets"])
        if op in ("edit_distance", "edit_distance_column"):
            return self.edit_distance(rows, case["targets"])
        if op == "porter_stemmer_measure":
            return self.porter_stemmer_measure(rows)
        return self.scatter_count(rows, case["counts"])
