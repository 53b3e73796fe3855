// Per-row logic of minhash: MinHash signatures of a strings column and the LSH band keys made from them.  Shared by the
// kernels of cs_minhash.hip and the g++ harness of tests/minhash_model.py, which restates it independently in Python.
// hash_row of convert_ops.h (NVStrings::hash) calls the murmur below with seed 31.
//
// Characters: a character starts at every byte that is no continuation byte (10xxxxxx) -- the rule of cs_len; the
//   continuation bytes behind a start belong to it, so malformed bytes are well defined.  S[0] < S[1] < ... < S[nch - 1]
//   are a row's character starts and S[nch] = n, its length in bytes.
// N-grams: nch >= width: the nch - width + 1 byte ranges [S[i], S[i + width]).  1 <= nch < width: one n-gram, the whole
//   row [0, n).  nch == 0 (a null row, an empty one, a row of continuation bytes only): none.
// Hash: h = MurmurHash3_x86_32(the n-gram's bytes, seed).
// Signature: sig[i] = the minimum over the row's n-grams of ((h * a[i] + b[i]) mod (2^61 - 1)) & 0xFFFFFFFF; the sum is
//   taken in 64 bits, which three operands below 2^32 cannot overflow.  A row without n-grams: 0xFFFFFFFF everywhere.
// Band keys: nperm = bands * r; band j's key is (int64)j << 32 | MurmurHash3_x86_32(sig[j r .. j r + r) as little-endian
//   bytes, seed j): keys of different bands never collide, equal keys mean the rows agree on the whole band.
#pragma once
#include <stdint.h>

#include "row_ops.h"

namespace csmh {

constexpr int kMaxWidth = 255;
constexpr int kMaxPerm = 4096;
constexpr uint32_t kNoGram = 0xFFFFFFFFu;
constexpr uint64_t kPrime = ((uint64_t)1 << 61) - 1;

CS_HD bool char_start(uint8_t c) { return (c & 0xC0) != 0x80; }

// ---- MurmurHash3_x86_32 ----------------------------------------------------------------------------------------------
CS_HD uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
CS_HD uint32_t murmur_scramble(uint32_t k) {
  k *= 0xcc9e2d51u;
  k = rotl32(k, 15);
  return k * 0x1b873593u;
}
// one whole 4-byte block, first byte lowest
CS_HD uint32_t murmur_block(uint32_t h, uint32_t k) {
  h ^= murmur_scramble(k);
  h = rotl32(h, 13);
  return h * 5u + 0xe6546b64u;
}
// the 1..3 bytes behind the last whole block (first byte lowest in k), then the length and the final mix
CS_HD uint32_t murmur_finish(uint32_t h, uint32_t tail, uint32_t n) {
  if (n & 3u) h ^= murmur_scramble(tail);
  h ^= n;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
CS_HD uint32_t murmur3_32(const uint8_t* p, int n, uint32_t seed) {
  uint32_t h = seed;
  const int nblocks = n / 4;
  for (int i = 0; i < nblocks; ++i) {
    const uint8_t* q = p + 4 * i;
    h = murmur_block(h, (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24));
  }
  const uint8_t* t = p + 4 * nblocks;
  uint32_t k = 0;
  for (int j = (n & 3) - 1; j >= 0; --j) k = (k << 8) | t[j];
  return murmur_finish(h, k, (uint32_t)n);
}

// ---- one permutation ---------------------------------------------------------------------------------------------------
// v mod (2^61 - 1) for any 64-bit v: 2^61 = 1 (mod P), so the bits above bit 60 are added to the bits below
CS_HD uint64_t fold61(uint64_t v) {
  uint64_t x = (v & kPrime) + (v >> 61);
  if (x >= kPrime) x -= kPrime;
  return x;
}
CS_HD uint32_t permute(uint32_t h, uint32_t a, uint32_t b) { return (uint32_t)fold61((uint64_t)h * a + b); }

// ---- a row's n-grams -----------------------------------------------------------------------------------------------------
// The byte just behind the n-gram of `width` characters that starts at the character start `s`: S[i + width] for s = S[i];
// -1 when fewer than `width` characters start in [s, n).
CS_HD int gram_end(const uint8_t* p, int n, int s, int width) {
  int starts = 1, e = s + 1;
  for (; e < n; ++e) {
    if (!char_start(p[e])) continue;
    if (starts == width) return e;
    ++starts;
  }
  return starts == width ? n : -1;
}
// f(h) for the hash of every n-gram of the row, in order; returns their number.  Two cursors: [s, e) is the current
// n-gram, both move on by a character.
template <class F>
CS_HD int for_each_gram(const uint8_t* p, int n, int width, uint32_t seed, F&& f) {
  int s = 0;
  while (s < n && !char_start(p[s])) ++s;
  if (s >= n) return 0;  // no character: no n-gram
  int e = gram_end(p, n, s, width);
  if (e < 0) {  // fewer characters than `width`: the whole row
    f(murmur3_32(p, n, seed));
    return 1;
  }
  int count = 0;
  for (;;) {
    f(murmur3_32(p + s, e - s, seed));
    ++count;
    if (e >= n) return count;
    for (++s; !char_start(p[s]); ++s) {
    }
    for (++e; e < n && !char_start(p[e]); ++e) {
    }
  }
}

// one row's signature, the plain way (the kernels keep the hashes and run the permutations in chunks: the same values)
CS_HD void row_signature(const uint8_t* p, int n, int width, uint32_t seed, const uint32_t* a, const uint32_t* b, int nperm, uint32_t* sig) {
  for (int i = 0; i < nperm; ++i) sig[i] = kNoGram;
  for_each_gram(p, n, width, seed, [&](uint32_t h) {
    for (int i = 0; i < nperm; ++i) {
      const uint32_t v = permute(h, a[i], b[i]);
      if (v < sig[i]) sig[i] = v;
    }
  });
}

// band j of a signature: its r values are the hash's blocks (a uint32 read as little-endian bytes is its own block)
CS_HD int64_t band_key(const uint32_t* vals, int r, int j) {
  uint32_t h = (uint32_t)j;
  for (int i = 0; i < r; ++i) h = murmur_block(h, vals[i]);
  return (int64_t)(((uint64_t)(uint32_t)j << 32) | murmur_finish(h, 0u, 4u * (uint32_t)r));
}

}  // namespace csmh
