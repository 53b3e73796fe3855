"""A model of compute_statistics / get_info in plain Python, from the semantics in include/custrings_amd.h at
cs_column_statistics and DESIGN.md section 4j, with the flag table of chartype_model; and the g++ harness of
custrings_amd/csrc/stats_ops.h (the text the kernels compile).

Rows are bytes (None = null row).  `chars` is cs_len's rule: the bytes that are no continuation byte.  The classes and the
histogram follow the character walk of DESIGN.md section 9, restated here over bytes (characters()): a lead byte takes the
bytes its width announces (past the row's end they read as 0), a continuation byte where a lead byte should be is a
character of its own.  On well-formed UTF-8 the walk yields the row's code points (model_from_str restates the figures over
Python str for that case)."""
import os
import subprocess
from collections import Counter

import numpy as np

import chartype_model as ctm

ROOT = ctm.ROOT
SPACE, DIGIT, UPPER, LOWER = ctm.SPACE, ctm.DIGIT, ctm.UPPER, ctm.LOWER
FIELDS = ("total_bytes total_chars bytes_avg bytes_max bytes_min bytes_95 chars_avg chars_max chars_min chars_95 "
          "mem_avg mem_max mem_min mem_95 total_strings total_nulls total_empty unique_strings whitespace_count digits_count "
          "uppercase_count lowercase_count").split()  # (total_memory is the column's footprint: not the model's business)
INFO_KEYS = ("total_strings null_strings empty_strings unique_strings total_bytes total_chars device_memory bytes_avg bytes_min "
             "bytes_max chars_avg chars_min chars_max memory_avg memory_min memory_max whitespace digits uppercase lowercase "
             "chars_histogram").split()
INFO_OF = {"total_strings": "total_strings", "null_strings": "total_nulls", "empty_strings": "total_empty", "unique_strings": "unique_strings",
           "total_bytes": "total_bytes", "total_chars": "total_chars", "bytes_avg": "bytes_avg", "bytes_min": "bytes_min",
           "bytes_max": "bytes_max", "chars_avg": "chars_avg", "chars_min": "chars_min", "chars_max": "chars_max", "memory_avg": "mem_avg",
           "memory_min": "mem_min", "memory_max": "mem_max", "whitespace": "whitespace_count", "digits": "digits_count",
           "uppercase": "uppercase_count", "lowercase": "lowercase_count"}


def count_chars(row):
    return sum((b & 0xC0) != 0x80 for b in row)


def characters(row):
    """the code points the character walk meets (None for one above U+FFFF)"""
    out, i, n = [], 0, len(row)
    while i < n:
        b = row[i]
        if b < 0x80:
            out.append(b)
            i += 1
            continue
        w = 0 if b < 0xC0 else 2 if b < 0xE0 else 3 if b < 0xF0 else 4
        tail = [row[i + k] if i + k < n else 0 for k in range(1, w)]
        if w == 0:
            cp = b & 0x3F
        elif w == 2:
            cp = ((b & 0x1F) << 6) | (tail[0] & 0x3F)
        elif w == 3:
            cp = ((b & 0x0F) << 12) | ((tail[0] & 0x3F) << 6) | (tail[1] & 0x3F)
        else:
            packed = (b << 24) | (tail[0] << 16) | (tail[1] << 8) | tail[2]
            # (the reference's u82u masks the lead byte with 0x03, and gives 0 beyond 0xF8000000)
            cp = 0 if packed > 0xF8000000 else ((b & 0x03) << 18) | ((tail[0] & 0x3F) << 12) | ((tail[1] & 0x3F) << 6) | (tail[2] & 0x3F)
        out.append(cp if cp <= 0xFFFF else None)
        i += w if w else 1
    return out


def packed(cp):
    """the character as the reference's u2u8 packs it: its UTF-8 bytes, first byte highest"""
    if cp < 0x80:
        return cp
    if cp < 0x800:
        return 0xC080 | ((cp >> 6) << 8) | (cp & 0x3F)
    return 0xE08080 | ((cp >> 12) << 16) | (((cp >> 6) & 0x3F) << 8) | (cp & 0x3F)


def row_mem(row):
    if row is None:
        return 0
    b, c = len(row), count_chars(row)
    return 8 + b + 1 + ((c + 3) // 4 if c != b else 0)


def _figures(bytes_, chars, mem, rows, classes, hist):
    count = len(rows)
    st = dict.fromkeys(FIELDS, 0)
    if count == 0:
        return st, []
    nonzero_min = lambda v: min([x for x in v if x] or [0])  # noqa: E731
    st.update(total_strings=count, total_nulls=sum(r is None for r in rows), total_empty=sum(r is not None and len(r) == 0 for r in rows),
              total_bytes=sum(bytes_), total_chars=sum(chars), bytes_avg=sum(bytes_) // count, chars_avg=sum(bytes_) // count,
              mem_avg=sum(mem) // count, bytes_max=max(bytes_), chars_max=max(chars), mem_max=max(mem), bytes_min=nonzero_min(bytes_),
              chars_min=nonzero_min(chars), mem_min=nonzero_min(mem), unique_strings=len(set(rows)),
              whitespace_count=classes[SPACE], digits_count=classes[DIGIT], uppercase_count=classes[UPPER], lowercase_count=classes[LOWER])
    pairs = [(packed(cp), n & 0xFFFFFFFF) for cp, n in sorted(hist.items()) if cp != 0]
    return st, pairs


def model(rows):
    """rows of bytes / None -> (dict of FIELDS, [(packed character, count)] in code-point order)"""
    flags = ctm.tables()[0]
    hist = Counter()
    classes = {SPACE: 0, DIGIT: 0, UPPER: 0, LOWER: 0}
    for r in rows:
        if r is None:
            continue
        for cp in characters(r):
            if cp is None:
                continue
            hist[cp] += 1
            for bit in classes:
                classes[bit] += (flags[cp] & bit) != 0
    return _figures([0 if r is None else len(r) for r in rows], [0 if r is None else count_chars(r) for r in rows],
                    [row_mem(r) for r in rows], rows, classes, hist)


def model_from_str(rows):
    """the same over str rows (well-formed text only), by Python's own notion of a character"""
    flags = ctm.tables()[0]
    hist = Counter(ord(ch) for r in rows if r is not None for ch in r if ord(ch) <= 0xFFFF)
    classes = {bit: sum(n for cp, n in hist.items() if flags[cp] & bit) for bit in (SPACE, DIGIT, UPPER, LOWER)}
    enc = [None if r is None else r.encode("utf-8", "surrogatepass") for r in rows]
    bytes_ = [0 if r is None else len(r) for r in enc]
    chars = [0 if r is None else len(r) for r in rows]
    mem = [0 if r is None else 8 + b + 1 + ((c + 3) // 4 if c != b else 0) for r, b, c in zip(rows, bytes_, chars)]
    return _figures(bytes_, chars, mem, enc, classes, hist)


def info_dict(st, pairs, device_memory):
    """what get_info returns for the model's figures"""
    d = {k: st[v] for k, v in INFO_OF.items()}
    d["device_memory"] = device_memory
    hist = {}
    for p, n in pairs:
        try:
            hist[p.to_bytes(4, "big").lstrip(b"\0").decode("utf-8")] = n
        except UnicodeDecodeError:
            pass
    d["chars_histogram"] = hist
    return d


# ---- generated rows ----------------------------------------------------------------------------------------------------------
EDGE_CPS = [0x00, 0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x1F600, 0x3FFFF]


def edge_rows():
    """the code points on either side of every width and of the histogram's end, NUL among them; the surrogate range is
    encoded as it stands"""
    enc = lambda cp: chr(cp).encode("utf-8", "surrogatepass")  # noqa: E731
    rows = [enc(cp) for cp in EDGE_CPS] + [b"a" + enc(cp) + b"Z 9" for cp in EDGE_CPS] + [enc(0xD800), enc(0xFFFF) * 3 + enc(0x10000) * 2]
    return rows + [b"\0\0x\0", None, b""]


def malformed_rows():
    return [b"\xc3", b"ab\xe2\x82", b"x\xf0\x9f", b"\x80", b"\xbf\xbfa", b"a\x80b", b"\xc3a", b"\xe2a\x82b", b"\xf0abc\xf0", b"\xff", b"\xf8\x80\x80\x80",
            b"\xf4\x8f\xbf\xbf", b"\xf4\x80\x80\x80", b"\xc0\x80", b"\xed\xa0\x80", b"ok \xc3\xa9\xc3", b"\xe9", b"\xc3\xa9\xa9"]


def random_bytes_rows(n, seed, max_len=40, null_every=7, empty_every=11):
    """rows of 0..max_len random bytes (any value: mostly malformed); every `null_every`-th row null, every `empty_every`-th empty"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n)
    data = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8).tobytes()
    rows, at = [], 0
    for i, ln in enumerate(lens.tolist()):
        if null_every and i % null_every == null_every - 1:
            rows.append(None)
        elif empty_every and i % empty_every == empty_every - 1:
            rows.append(b"")
        else:
            rows.append(data[at:at + ln])
        at += ln
    return rows


def text_rows(n, seed):
    """well-formed rows (str / None): chartype_model's generator -- ASCII, accents, 3- and 4-byte characters, nulls, empties"""
    return ctm.gen_rows(n, seed)


# ---- the harness: stats_ops.h built with g++ ---------------------------------------------------------------------------------------
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "stats_ops.h"
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
// harness FLAGS CHARS OFFS NULLS OUT: per row six int64 (chars, mem, space, digit, upper, lower; a null row all 0), then
// the 65536 histogram counters as uint32 (bin 0 included)
int main(int argc, char** argv) {
  if (argc != 6) return 2;
  std::vector<uint8_t> flags = slurp<uint8_t>(argv[1]);
  if (flags.size() != 65536) return 3;
  std::vector<uint8_t> chars = slurp<uint8_t>(argv[2]), nulls = slurp<uint8_t>(argv[4]);
  std::vector<int64_t> offs = slurp<int64_t>(argv[3]);
  const size_t rows = offs.size() - 1;
  chars.resize(chars.size() + 32, 0xC3);  // (bytes behind the last row: a walk that ran on would count them)
  const csstat::ClassSpec spec = csstat::make_classes(flags.data(), flags.data());
  std::vector<uint32_t> hist(65536, 0);
  std::vector<int64_t> out(rows * 6, 0);
  for (size_t r = 0; r < rows; ++r) {
    if (nulls[r]) continue;
    const int n = (int)(offs[r + 1] - offs[r]);
    const csstat::RowStats st = csstat::walk_row<true>(chars.data() + offs[r], n, spec, [&](unsigned cp) { ++hist[cp]; });
    const csstat::RowStats plain = csstat::walk_row<false>(chars.data() + offs[r], n, spec, [](unsigned) {});
    if (plain.chars != st.chars || plain.space || plain.digit || plain.upper || plain.lower) return 4;
    int64_t* o = &out[r * 6];
    o[0] = st.chars; o[1] = csstat::row_mem(n, st.chars); o[2] = st.space; o[3] = st.digit; o[4] = st.upper; o[5] = st.lower;
  }
  FILE* f = fopen(argv[5], "wb");
  fwrite(out.data(), 8, out.size(), f);
  fwrite(hist.data(), 4, hist.size(), f);
  fclose(f);
  return 0;
}
"""


class Harness:
    """stats_ops.h built with g++ into `workdir`"""

    def __init__(self, workdir, root=ROOT):
        self.dir = workdir
        src = os.path.join(workdir, "stats_harness.cpp")
        self.exe = os.path.join(workdir, "stats_harness")
        open(src, "w").write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "custrings_amd", "csrc"), src, "-o", self.exe], check=True)
        self.flags = os.path.join(workdir, "flags.bin")
        np.array(ctm.tables()[0], dtype=np.uint8).tofile(self.flags)

    def run(self, rows):
        """rows of bytes / None -> (per-row int64[rows, 6]: chars, mem, space, digit, upper, lower; histogram uint32[65536])"""
        chars, offs, nulls = ctm.to_arrow(rows)
        paths = []
        for name, data in (("c.bin", chars), ("o.bin", offs), ("n.bin", nulls)):
            paths.append(os.path.join(self.dir, name))
            np.ascontiguousarray(data).tofile(paths[-1])
        out = os.path.join(self.dir, "out.bin")
        subprocess.run([self.exe, self.flags] + paths + [out], check=True, timeout=900)
        raw = np.fromfile(out, dtype=np.uint8)
        per_row = raw[:len(rows) * 48].view(np.int64).reshape(len(rows), 6)
        return per_row, raw[len(rows) * 48:].view(np.uint32)

    def figures(self, rows):
        """the harness's per-row results folded into the model's (dict, pairs) form"""
        per_row, hist = self.run(rows)
        classes = {SPACE: int(per_row[:, 2].sum()), DIGIT: int(per_row[:, 3].sum()), UPPER: int(per_row[:, 4].sum()), LOWER: int(per_row[:, 5].sum())}
        counts = {cp: int(hist[cp]) for cp in np.nonzero(hist)[0].tolist()}
        return _figures([0 if r is None else len(r) for r in rows], per_row[:, 0].tolist(), per_row[:, 1].tolist(), rows, classes, counts)
