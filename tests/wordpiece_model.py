"""A model of WordPiece tokenization in plain Python, from the definition in custrings_amd/csrc/wordpiece_ops.h's header
comment and include/custrings_amd.h at cs_wordpiece_*; and the g++ harness of wordpiece_ops.h (the text the kernels
compile).  Rows and vocabulary rows are bytes (None = null row).

Vocabulary: row index = id; null and empty rows are no entry; the lowest index of equal rows wins.  Words: maximal runs of
bytes > 0x20; with punct every ASCII punctuation byte is a word of its own.  A word's character boundaries: its front, every
later byte that is no continuation byte, its end.  More than max_word_chars characters: [unk].  Else from s = 0 the longest
run of whole characters that is an entry (behind the front: with the prefix before it), and so on; no match anywhere: [unk]
for the whole word.  The model tries the longest run first and works on byte strings in a dict: nothing of the table, the
hash or the forward walk of the header is in it."""
import os
import subprocess

import numpy as np

from minhash_model import murmur3_32, to_arrow  # noqa: F401  (murmur3_32: for the tests' colliding keys)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUNCT = frozenset(list(range(33, 48)) + list(range(58, 65)) + list(range(91, 97)) + list(range(123, 127)))
SEED_WHOLE, SEED_CONT = 0x5770, 0x2323  # the table's hash seeds (only the colliding keys of the tests need them)


class Vocab:
    def __init__(self, entries, prefix=b"##", unk=b"[UNK]"):
        self.prefix = bytes(prefix)
        self.ids = {}
        for i, e in enumerate(entries):
            if e:
                self.ids.setdefault(bytes(e), i)
        self.unk = self.ids.get(bytes(unk), -1)

    @property
    def entries(self):
        return len(self.ids)

    @property
    def max_entry_bytes(self):
        return max((len(e) for e in self.ids), default=0)

    def id_of(self, token):
        return self.ids.get(bytes(token), -1)


def words(row, punct):
    """the (lo, hi) byte ranges of the row's words"""
    if row is None:
        return []
    out, lo = [], None
    for i, c in enumerate(row):
        if c <= 0x20 or (punct and c in PUNCT):
            if lo is not None:
                out.append((lo, i))
                lo = None
            if c > 0x20:
                out.append((i, i + 1))
        elif lo is None:
            lo = i
    if lo is not None:
        out.append((lo, len(row)))
    return out


def boundaries(word):
    return [0] + [i for i in range(1, len(word)) if (word[i] & 0xC0) != 0x80] + [len(word)]


def word_ids(word, v, max_word_chars):
    b = boundaries(word)
    nch = len(b) - 1
    if nch > max_word_chars:
        return [v.unk]
    out, s = [], 0
    while s < nch:
        for e in range(nch, s, -1):
            piece = word[b[s]:b[e]]
            hit = v.ids.get(piece if s == 0 else v.prefix + piece)
            if hit is not None:
                out.append(hit)
                s = e
                break
        else:
            return [v.unk]
    return out


def row_ids(row, v, max_word_chars=100, punct=0):
    out = []
    for lo, hi in words(row, punct):
        out += word_ids(bytes(row[lo:hi]), v, max_word_chars)
    return out


def tokenize(rows, v, max_word_chars=100, punct=0):
    """-> (ids int32[total], offsets int64[rows + 1])"""
    per = [row_ids(r, v, max_word_chars, punct) for r in rows]
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in per], out=offs[1:])
    return np.array([i for p in per for i in p], dtype=np.int32), offs


def encode(rows, v, max_length, cls=-1, sep=-1, pad=0, max_word_chars=100, punct=0):
    """-> (ids int32[rows, max_length], mask uint8[rows, max_length])"""
    ids = np.full((len(rows), max_length), pad, dtype=np.int32)
    mask = np.zeros((len(rows), max_length), dtype=np.uint8)
    room = max_length - (cls >= 0) - (sep >= 0)
    for r, row in enumerate(rows):
        line = ([cls] if cls >= 0 else []) + row_ids(row, v, max_word_chars, punct)[:room] + ([sep] if sep >= 0 else [])
        ids[r, :len(line)] = line
        mask[r, :len(line)] = 1
    return ids, mask


# ---- generated vocabularies and rows ---------------------------------------------------------------------------------------------
LETTERS = [b"a", b"b", b"c", b"d", b"e", "é".encode(), "ß".encode(), "€".encode(), "語".encode(), "😀".encode(), "𐍈".encode(), b"#"]
BLANKS = [b" ", b" ", b" ", b"\t", b"\n", b"\r", b"\x0b", b"\x0c", b"  "]
MARKS = [b",", b".", b"!", b"-", b"(", b")", b"'", b"$", b"~", b"[", b"]", b"_", b"@"]
SPECIAL_ENTRIES = [b"##", b"#", b"###", b"##a#", b"a##b"]


def make_vocab(n, seed, letters=LETTERS, max_chars=4, extra=()):
    """[UNK], [CLS], [SEP], [PAD], `extra`, the entries of the "trap in the key", most single letters whole and as
    continuations, and generated runs of 2..max_chars letters, whole or with the prefix, up to `n` rows"""
    rng = np.random.default_rng(seed)
    out = [b"[UNK]", b"[CLS]", b"[SEP]", b"[PAD]"] + list(extra) + SPECIAL_ENTRIES
    out += [c for c in letters[:-2]] + [b"##" + c for c in letters[:-3]] + [b",", b".", b"!", b"(", b"$"]
    seen = set(out)
    while len(out) < n:
        k = int(rng.integers(2, max_chars + 1))
        run = b"".join(letters[i] for i in rng.integers(0, len(letters), size=k))
        e = run if rng.integers(0, 3) else b"##" + run
        if e not in seen:
            seen.add(e)
            out.append(e)
    return out


def make_rows(n, seed, letters=LETTERS, max_words=8, max_chars=6, null_every=0, marks_every=3):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        if null_every and i % null_every == null_every - 1:
            rows.append(None)
            continue
        parts = []
        if i % 17 == 3:
            parts.append(BLANKS[int(rng.integers(0, len(BLANKS)))])
        for w in range(int(rng.integers(0, max_words + 1))):
            k = int(rng.integers(1, max_chars + 1))
            word = b"".join(letters[j] for j in rng.integers(0, len(letters), size=k))
            if marks_every and (i + w) % marks_every == 0:
                at = int(rng.integers(0, 3))
                mark = MARKS[int(rng.integers(0, len(MARKS)))]
                word = mark + word if at == 0 else word + mark if at == 1 else word[:1] + mark + word[1:] if (word[0] & 0x80) == 0 else word + mark + mark
            parts.append(word)
            parts.append(BLANKS[int(rng.integers(0, len(BLANKS)))])
        if parts and i % 5 == 0:
            parts.pop()  # (no blank behind the last word)
        rows.append(b"".join(parts))
    return rows


def hostile_rows():
    """what a reference fixture may not hold: malformed bytes, continuation bytes only, control and NUL bytes, words that
    start with the prefix"""
    return [b"\x80", b"\x80\x80\x80", b"\xbf\xbfa", b"a\x80\x80b", b"\xc3", b"ab\xe2\x82", b"a\xf0\x9f b", b"\x80ab\x80 \x80", b"\0\0\0", b"a\0b\0c\0d",
            b"ab\x01cd\x1fe", b"\x7fab", b"\xffab\xfe", b"ab \xc3a\xc3 cd", b"##ab", b"##", b"###", b"####", b"##a#", b"a##b", b"#a ##a a## a#a",
            b"[UNK]", b"[UNK]a", b"a,b", b",", b",,", b" , ", b"\t\n", b"", None, b"a" * 300, b"ab" * 40 + b" ab", b"\x80" * 70 + b" a"]


# ---- keys that meet in the table ---------------------------------------------------------------------------------------------------
# pairs of six bytes with one MurmurHash3_x86_32 under the table's seeds (found by a birthday search over 600 000 strings;
# test_wordpiece_cpu.py checks them against the model's murmur): whole keys, and continuation keys
SAME_HASH_WHOLE = (b"brqjke", b"jpsxwj")
SAME_HASH_CONT = (b"rtzycj", b"wvrnhy")


def slot_sharer(entry, slots, taken, seed=SEED_WHOLE):
    """a string of entry's length that is none of `taken` and whose hash starts its probe at entry's slot of a table of
    `slots` slots: by search"""
    want = murmur3_32(entry, seed) & (slots - 1)
    n = 0
    while True:
        cand = ("%0*d" % (len(entry), n)).encode()[:len(entry)]
        if cand not in taken and murmur3_32(cand, seed) & (slots - 1) == want:
            return cand
        n += 1


# ---- the harness: wordpiece_ops.h built with g++ -----------------------------------------------------------------------------------
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "wordpiece_ops.h"
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
  Col(const char* c, const char* o, const char* n) : chars(slurp<uint8_t>(c)), nulls(slurp<uint8_t>(n)), offs(slurp<int64_t>(o)) {
    chars.resize(chars.size() + 32, 0x61);  // (bytes behind the last row: a walk that ran on would take them in)
  }
  size_t rows() const { return offs.size() - 1; }
  const uint8_t* row(size_t r) const { return chars.data() + offs[r]; }
  int len(size_t r) const { return nulls[r] ? 0 : (int)(offs[r + 1] - offs[r]); }
};
struct PutWithin {
  int32_t* at;
  int n;
  void operator()(int k, int32_t id) const { if (k < n) at[k] = id; }
};
// harness DIR PREFIX UNK MAX_WORD_CHARS PUNCT SLOTS MAX_LENGTH CLS SEP PAD: the columns v (vocabulary), r (rows), q (queries)
// as DIR/{v,r,q}_{c,o,n}.bin -> DIR/out.bin: int64 {unk id, entries, longest entry, slots}, int32 counts[rows], int32
// ids[total], int32 query ids[queries], int32 encoded[rows x MAX_LENGTH], uint8 mask[rows x MAX_LENGTH]
int main(int argc, char** argv) {
  if (argc != 11) return 2;
  const std::string d = argv[1];
  auto path = [&](const char* name) { return d + "/" + name; };
  const Col v(path("v_c.bin").c_str(), path("v_o.bin").c_str(), path("v_n.bin").c_str());
  const Col r(path("r_c.bin").c_str(), path("r_o.bin").c_str(), path("r_n.bin").c_str());
  const Col q(path("q_c.bin").c_str(), path("q_o.bin").c_str(), path("q_n.bin").c_str());
  cswp::Prefix px{};
  px.n = (int)strlen(argv[2]);
  memcpy(px.b, argv[2], px.n);
  const int mwc = atoi(argv[4]), punct = atoi(argv[5]), L = atoi(argv[7]);
  int64_t nslots = atoll(argv[6]);
  if (nslots == 0) nslots = cswp::slots_for((int64_t)v.rows());
  std::vector<cswp::Slot> slots(nslots, cswp::Slot{0u, cswp::kNoId, 0u, 0u});
  int64_t entries = 0;
  int longest[2] = {0, 0};
  for (size_t i = 0; i < v.rows(); ++i) {
    const int res = cswp::insert_row<cswp::PlainAtomics>(slots.data(), (uint32_t)(nslots - 1), v.chars.data(), v.offs.data(), px, (int32_t)i, !v.nulls[i]);
    if (res < 0) return 3;
    entries += res;
    const int len = v.len(i);
    if (len <= 0 || len > cswp::kMaxEntryBytes) continue;
    if (len > longest[0]) longest[0] = len;
    if (len > px.n && cswp::bytes_equal(v.row(i), px.b, px.n) && len - px.n > longest[1]) longest[1] = len - px.n;
  }
  cswp::Table t{slots.data(), v.chars.data(), (uint32_t)(nslots - 1), {longest[0], longest[1]}, -1};
  t.unk = cswp::find_entry(t, (const uint8_t*)argv[3], (int)strlen(argv[3]));
  const int64_t head[4] = {t.unk, entries, longest[0], nslots};
  std::vector<int32_t> counts(r.rows()), ids, found(q.rows()), enc(r.rows() * (size_t)L);
  std::vector<uint8_t> mask(r.rows() * (size_t)L);
  const cswp::Specials sp{atoi(argv[8]), atoi(argv[9]), atoi(argv[10]), L};
  if (t.unk >= 0) {
    for (size_t i = 0; i < r.rows(); ++i) {
      counts[i] = cswp::row_ids(t, r.row(i), r.len(i), mwc, punct, 0x7fffffff, cswp::NoOutput{});
      const size_t at = ids.size();
      ids.resize(at + counts[i] + 1);
      if (cswp::row_ids(t, r.row(i), r.len(i), mwc, punct, 0x7fffffff, PutWithin{ids.data() + at, counts[i]}) != counts[i]) return 4;
      ids.resize(at + counts[i]);
      if (L > 0) {  // the encode launch's steps: the row's ids within room(), then every other place from filler()
        int32_t* line = enc.data() + i * L;
        const int count = cswp::row_ids(t, r.row(i), r.len(i), mwc, punct, sp.room(), PutWithin{line + sp.front(), sp.room()});
        const int kept = count < sp.room() ? count : sp.room();
        for (int j = 0; j < L; ++j) {
          if (j < sp.front() || j >= sp.front() + kept) line[j] = cswp::filler(sp, kept, j);
          mask[i * L + j] = j < cswp::used(sp, kept);
        }
      }
    }
  }
  for (size_t i = 0; i < q.rows(); ++i) found[i] = cswp::find_entry(t, q.row(i), q.len(i));
  FILE* f = fopen(path("out.bin").c_str(), "wb");
  auto put = [&](const void* p, size_t width, size_t n) { if (n) fwrite(p, width, n, f); };
  put(head, 8, 4);
  put(counts.data(), 4, counts.size());
  put(ids.data(), 4, ids.size());
  put(found.data(), 4, found.size());
  put(enc.data(), 4, enc.size());
  put(mask.data(), 1, mask.size());
  fclose(f);
  return 0;
}
"""


class Harness:
    """wordpiece_ops.h built with g++ into `workdir`"""

    def __init__(self, workdir, root=ROOT):
        self.dir = workdir
        src = os.path.join(workdir, "wordpiece_harness.cpp")
        self.exe = os.path.join(workdir, "wordpiece_harness")
        open(src, "w").write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "custrings_amd", "csrc"), src, "-o", self.exe], check=True)

    def run(self, vocab, rows, queries=(), prefix=b"##", unk=b"[UNK]", max_word_chars=100, punct=0, slots=0, max_length=0, cls=-1, sep=-1, pad=0):
        """-> dict: unk, entries, max_entry_bytes, slots, counts int32[rows], ids int32[total], found int32[queries],
        encoded int32[rows, max_length], mask uint8[rows, max_length]"""
        for tag, col in (("v", list(vocab)), ("r", list(rows)), ("q", list(queries))):
            chars, offs, nulls = to_arrow(col)
            for part, data in (("c", chars), ("o", offs), ("n", nulls)):
                np.ascontiguousarray(data).tofile(os.path.join(self.dir, "%s_%s.bin" % (tag, part)))
        args = [prefix.decode(), unk.decode(), max_word_chars, punct, slots, max_length, cls, sep, pad]
        subprocess.run([self.exe, self.dir] + [str(a) for a in args], check=True, timeout=600)
        raw = np.fromfile(os.path.join(self.dir, "out.bin"), dtype=np.uint8)
        head = raw[:32].view(np.int64)
        n, nq, cells = len(rows), len(queries), len(rows) * max_length
        counts = raw[32:32 + 4 * n].view(np.int32)
        total = int(counts.sum())
        at = 32 + 4 * n
        ids = raw[at:at + 4 * total].view(np.int32)
        at += 4 * total
        found = raw[at:at + 4 * nq].view(np.int32)
        at += 4 * nq
        enc = raw[at:at + 4 * cells].view(np.int32).reshape(n, max_length)
        at += 4 * cells
        assert at + cells == raw.size
        return {"unk": int(head[0]), "entries": int(head[1]), "max_entry_bytes": int(head[2]), "slots": int(head[3]), "counts": counts, "ids": ids,
                "found": found, "encoded": enc, "mask": raw[at:].reshape(n, max_length)}
