"""A model of minhash in plain Python, from the definition in custrings_amd/csrc/minhash_ops.h's header comment and
include/custrings_amd.h at cs_minhash / cs_minhash_bands; and the g++ harness of minhash_ops.h (the text the kernels
compile).  Rows are bytes (None = null row).

Characters start at every byte that is no continuation byte; S = their offsets, S[nch] = len(row).  nch >= width: the
n-grams are row[S[i]:S[i + width]]; 1 <= nch < width: the whole row; nch == 0: none.  h = MurmurHash3_x86_32(n-gram, seed);
sig[i] = min over the n-grams of ((h a[i] + b[i]) mod (2^61 - 1)) & 0xFFFFFFFF, all ones without n-grams.  Band j of r =
nperm / bands values: key = j << 32 | MurmurHash3_x86_32(the r values as little-endian bytes, seed j)."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 61) - 1
M32 = 0xFFFFFFFF
NO_GRAM = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def murmur3_32(data, seed=0):
    """MurmurHash3_x86_32, from the published description"""
    h = seed & M32
    n = len(data)
    for i in range(0, n - n % 4, 4):
        k = struct.unpack_from("<I", data, i)[0]
        k = (_rotl((k * 0xcc9e2d51) & M32, 15) * 0x1b873593) & M32
        h = (_rotl(h ^ k, 13) * 5 + 0xe6546b64) & M32
    tail = data[n - n % 4:]
    if tail:
        k = int.from_bytes(tail, "little")
        h ^= (_rotl((k * 0xcc9e2d51) & M32, 15) * 0x1b873593) & M32
    h ^= n
    h = ((h ^ (h >> 16)) * 0x85ebca6b) & M32
    h = ((h ^ (h >> 13)) * 0xc2b2ae35) & M32
    return h ^ (h >> 16)


def fold61(v):
    """v mod P for a 64-bit v, the way the library computes it"""
    x = (v & P) + (v >> 61)
    return x - P if x >= P else x


def ngrams(row, width):
    if row is None:
        return []
    starts = [i for i, c in enumerate(row) if (c & 0xC0) != 0x80]
    nch = len(starts)
    if nch == 0:
        return []
    if nch < width:
        return [bytes(row)]
    starts.append(len(row))
    return [bytes(row[starts[i]:starts[i + width]]) for i in range(nch - width + 1)]


def signature(row, width, seed, a, b):
    hs = np.array(sorted({murmur3_32(g, seed) for g in ngrams(row, width)}), dtype=object)
    if hs.size == 0:
        return [NO_GRAM] * len(a)
    return [min((int(h) * int(ai) + int(bi)) % P & M32 for h in hs) for ai, bi in zip(a, b)]


def signatures(rows, width, seed, a, b):
    """rows x nperm uint32"""
    a64 = [int(x) for x in a]
    b64 = [int(x) for x in b]
    out = np.empty((len(rows), len(a64)), dtype=np.uint32)
    for r, row in enumerate(rows):
        out[r] = signature(row, width, seed, a64, b64)
    return out


def band_keys(sig, bands):
    """rows x bands int64"""
    sig = np.asarray(sig, dtype=np.uint32)
    rows, nperm = sig.shape
    r = nperm // bands
    out = np.empty((rows, bands), dtype=np.int64)
    for i in range(rows):
        for j in range(bands):
            out[i, j] = (j << 32) | murmur3_32(sig[i, j * r:(j + 1) * r].astype("<u4").tobytes(), j)
    return out


def jaccard(row_a, row_b, width):
    ga, gb = set(ngrams(row_a, width)), set(ngrams(row_b, width))
    return len(ga & gb) / len(ga | gb)


def to_arrow(rows):
    chars = np.frombuffer(b"".join(r or b"" for r in rows), dtype=np.uint8)
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([0 if r is None else len(r) for r in rows], out=offs[1:])
    nulls = np.array([r is None for r in rows], dtype=np.uint8)
    return chars, offs, nulls


# ---- generated rows ----------------------------------------------------------------------------------------------------------
UNITS = [b"a", b"Z", b" ", b"\0", "é".encode(), "ß".encode(), "€".encode(), "語".encode(), "😀".encode(), "𐍈".encode()]
MALFORMED = [b"\x80", b"\xbf\xbf", b"\xc3", b"\xe2\x82", b"\xf0\x9f\x98"]


def boundary_rows(width):
    """nch from 0 to width + 2 of every character width, and rows in which the one wide character sits at every position
    of an n-gram"""
    rows = [None, b""]
    for u in (b"a", "é".encode(), "€".encode(), "😀".encode()):
        for nch in range(1, width + 3):
            rows.append(u * nch)
    if width <= 8:
        for wide in ("é".encode(), "€".encode(), "😀".encode()):
            for at in range(width + 2):
                rows.append(b"x" * at + wide + b"y" * (width + 1 - at))
    return rows


def malformed_rows():
    rows = [b"\x80", b"\xbf\xbf\xbf", b"\x80" * 70, b"a\x80\x80b", b"\xc3", b"ab\xe2\x82", b"x\xf0\x9f", b"\x80ab\x80", b"\0\0\0", b"a\0b\0c\0d",
            b"\xc3a\xc3", b"\xf0\x9f\x98", b"\x80\x80a", b"\xffab\xfe"]
    return rows + [b"ok " + m + b" end" + m for m in MALFORMED]


def mixed_rows(n, seed, max_units=14, null_every=7, empty_every=11, malformed_every=5):
    """rows of 0..max_units pieces of every character width (at most ~40 bytes for the default), NULs and malformed bytes
    among them"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, max_units + 1, size=n)
    picks = rng.integers(0, len(UNITS), size=(n, max_units))
    bad = rng.integers(0, len(MALFORMED), size=n)
    rows = []
    for i in range(n):
        if null_every and i % null_every == null_every - 1:
            rows.append(None)
        elif empty_every and i % empty_every == empty_every - 1:
            rows.append(b"")
        else:
            parts = [UNITS[p] for p in picks[i, :counts[i]]]
            if malformed_every and i % malformed_every == 0:
                parts.insert(len(parts) // 2, MALFORMED[bad[i]])
            rows.append(b"".join(parts)[:40] if max_units <= 14 else b"".join(parts))
    return rows


def text_row(nchars, seed, wide_every=9):
    """a well-formed row of exactly `nchars` characters, a wide one every few"""
    rng = np.random.default_rng(seed)
    words = rng.integers(97, 123, size=nchars)
    out = []
    for i, c in enumerate(words.tolist()):
        out.append(UNITS[4 + (i // wide_every) % 6] if wide_every and i % wide_every == wide_every - 1 else b" " if i % 6 == 5 else bytes([c]))
    return b"".join(out)


# ---- the harness: minhash_ops.h built with g++ -----------------------------------------------------------------------------------
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "minhash_ops.h"
#include "convert_ops.h"
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
// harness CHARS OFFS NULLS AB WIDTH SEED BANDS OUT: rows x nperm uint32 signatures, rows x bands int64 keys, rows uint32
// n-gram counts, rows uint32 hash_row values
int main(int argc, char** argv) {
  if (argc != 9) return 2;
  std::vector<uint8_t> chars = slurp<uint8_t>(argv[1]), nulls = slurp<uint8_t>(argv[3]);
  std::vector<int64_t> offs = slurp<int64_t>(argv[2]);
  std::vector<uint32_t> ab = slurp<uint32_t>(argv[4]);
  const int nperm = (int)(ab.size() / 2), width = atoi(argv[5]), bands = atoi(argv[7]);
  const uint32_t seed = (uint32_t)strtoul(argv[6], nullptr, 10);
  const size_t rows = offs.size() - 1;
  chars.resize(chars.size() + 32, 0x61);  // (bytes behind the last row: a walk that ran on would take them in)
  std::vector<uint32_t> sig(rows * nperm), counts(rows), hashes(rows);
  std::vector<int64_t> keys(rows * bands);
  for (size_t r = 0; r < rows; ++r) {
    const int n = nulls[r] ? 0 : (int)(offs[r + 1] - offs[r]);
    const uint8_t* p = chars.data() + offs[r];
    csmh::row_signature(p, n, width, seed, ab.data(), ab.data() + nperm, nperm, &sig[r * nperm]);
    counts[r] = (uint32_t)csmh::for_each_gram(p, n, width, seed, [](uint32_t) {});
    hashes[r] = csconv::hash_row(p, n);
    for (int j = 0; j < bands; ++j) keys[r * bands + j] = csmh::band_key(&sig[r * nperm + j * (nperm / bands)], nperm / bands, j);
  }
  FILE* f = fopen(argv[8], "wb");
  fwrite(sig.data(), 4, sig.size(), f);
  fwrite(keys.data(), 8, keys.size(), f);
  fwrite(counts.data(), 4, counts.size(), f);
  fwrite(hashes.data(), 4, hashes.size(), f);
  fclose(f);
  return 0;
}
"""


class Harness:
    """minhash_ops.h built with g++ into `workdir`"""

    def __init__(self, workdir, root=ROOT):
        self.dir = workdir
        src = os.path.join(workdir, "minhash_harness.cpp")
        self.exe = os.path.join(workdir, "minhash_harness")
        open(src, "w").write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(root, "custrings_amd", "csrc"), src, "-o", self.exe], check=True)

    def run(self, rows, width, seed, a, b, bands):
        """-> (signatures uint32[rows, nperm], keys int64[rows, bands], n-gram counts uint32[rows], hash_row uint32[rows])"""
        chars, offs, nulls = to_arrow(rows)
        ab = np.concatenate([np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)])
        paths = []
        for name, data in (("c.bin", chars), ("o.bin", offs), ("n.bin", nulls), ("ab.bin", ab)):
            paths.append(os.path.join(self.dir, name))
            np.ascontiguousarray(data).tofile(paths[-1])
        out = os.path.join(self.dir, "out.bin")
        subprocess.run([self.exe] + paths + [str(width), str(seed), str(bands), out], check=True, timeout=600)
        raw = np.fromfile(out, dtype=np.uint8)
        n, nperm = len(rows), len(a)
        s0, s1 = n * nperm * 4, n * nperm * 4 + n * bands * 8
        return (raw[:s0].view(np.uint32).reshape(n, nperm), raw[s0:s1].view(np.int64).reshape(n, bands),
                raw[s1:s1 + 4 * n].view(np.uint32), raw[s1 + 4 * n:s1 + 8 * n].view(np.uint32))
