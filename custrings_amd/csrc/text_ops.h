// Per-row logic of the NVText members contains_strings / strings_counts / edit_distance / porter_stemmer_measure /
// scatter_count (reference: cpp/src/text/NVText.cu:32-172, edit_distance.cu:33-228, stemmer.cu:29-104; find:
// custring_view.inl:476-543).  Shared by the kernels of cs_textops.hip and the g++ harness of tests/text_model.py, which
// also restates it independently in Python, over characters.
//
// contains_strings / strings_counts: a rows x M matrix, results[r * M + j] for row r and target j.
//   contains: find(target) >= 0.  counts: find(target, pos + chars(target)) repeated until -1.  find compares BYTES at
//   every byte offset of the row -- not only where a character starts -- and returns the number of characters that start
//   in front of the match; the next search starts chars(target) CHARACTERS after that.  So a target whose bytes match
//   across a character boundary is found, and the restart may land before or behind the end of the matched bytes.
//   A null row, a null target and an empty target give false / 0.
// edit_distance: Levenshtein over characters.  A null or empty row gives chars(target) (0 for a null target), a null or
//   empty target gives chars(row).  Two forms: a one-row dynamic program for any pair (the row of the table indexed by the
//   string of fewer characters, uint16 entries: the callers refuse more than 32767 characters), and Myers' bit-vector
//   algorithm in Hyyro's global-distance form for a target of 1..64 characters (the target's characters are the bits).
// porter_stemmer_measure: the number of vowel-run -> consonant transitions.  y_char is a consonant at index 0 or when the
//   character before it is a vowel, else it counts as a vowel; a null and an empty row give 0.
// scatter_count: row i repeated counts[i] times: scatter_source maps an output row to its source row over the exclusive
//   scan of the counts.
// Characters: a row's characters are the steps of row_ops.h's decode_at (a stray continuation byte is a character of its
// own, a truncated one reads its missing bytes as 0) -- on malformed UTF-8 these routines ARE the definition, and
// nothing reads beyond [p, p + n).
#pragma once
#include <stdint.h>

#include "row_ops.h"

namespace cstxt {

using csrow::Char;
using csrow::count_chars;
using csrow::decode_at;
using csrow::find_bytes;
using csrow::lead_width;
using csrow::skip_chars;

constexpr int kMaxChars = 32767;      // edit_distance: the table's entries are 16 bits wide
constexpr int kBitTargetChars = 64;   // the bit-vector form: one bit a target character

enum Algo { ALGO_LEVENSHTEIN = 0 };

// ---- contains_strings / strings_counts -----------------------------------------------------------------------------------
CS_HD bool contains_row(const uint8_t* p, int n, const uint8_t* t, int tn) {
  return tn > 0 && find_bytes(p, 0, n, t, tn) >= 0;
}
// (cb, cc): byte offset and index of a character start the walk from 0 reaches: every restart is at or behind it
CS_HD uint32_t count_row(const uint8_t* p, int n, const uint8_t* t, int tn) {
  if (tn <= 0 || tn > n) return 0;
  const int nchars = count_chars(p, n);
  int tch = count_chars(t, tn);
  if (tch < 1) tch = 1;  // (a target of continuation bytes only: the reference would not terminate)
  int cb = 0, cc = 0;
  uint32_t found = 0;
  for (;;) {
    const int m = find_bytes(p, cb, n, t, tn);
    if (m < 0) break;
    ++found;
    const int next = cc + count_chars(p + cb, m - cb) + tch;  // the match's character position + chars(target)
    if (next >= nchars) break;                                // (the window [next, nchars) is empty)
    cb = skip_chars(p, n, cb, next - cc);
    cc = next;
  }
  return found;
}

// ---- edit_distance -----------------------------------------------------------------------------------------------------------
CS_HD int walk_chars(const uint8_t* p, int n) {
  int k = 0;
  for (int i = 0; i < n; ++k) {
    const unsigned w = lead_width(p[i]);
    i += w ? (int)w : 1;
  }
  return k;
}
CS_HD Char next_char(const uint8_t* p, int n, int& i) {
  Char c = 0;
  if (i < n) {
    const unsigned w = decode_at(p, i, n, c);
    i += w ? (int)w : 1;
  }
  return c;
}
// entries of the one-row table a pair needs (0: decided without a table)
CS_HD int edit_row_entries(const uint8_t* p, int n, bool pv, const uint8_t* t, int tn, bool tv) {
  if (!pv || n == 0 || !tv || tn == 0) return 0;
  const int a = walk_chars(p, n), b = walk_chars(t, tn);
  return a < b ? a : b;
}
// `row`: edit_row_entries(...) entries of scratch.  row[j] is D[i][j + 1] over the string of fewer characters; D[i][0] = i.
CS_HD uint32_t edit_distance_dp(const uint8_t* p, int n, bool pv, const uint8_t* t, int tn, bool tv, uint16_t* row) {
  if (!pv || n == 0) return tv ? (uint32_t)walk_chars(t, tn) : 0u;
  if (!tv || tn == 0) return (uint32_t)walk_chars(p, n);
  int la = walk_chars(p, n), lb = walk_chars(t, tn);
  const uint8_t *A = p, *B = t;
  int an = n, bn = tn;
  if (la > lb) {
    A = t, an = tn, B = p, bn = n;
    const int x = la;
    la = lb, lb = x;
  }
  for (int j = 0; j < la; ++j) row[j] = (uint16_t)(j + 1);
  int bi = 0;
  for (int i = 1; i <= lb; ++i) {
    const Char cb = next_char(B, bn, bi);
    unsigned diag = (unsigned)(i - 1), left = (unsigned)i;
    int ai = 0;
    for (int j = 0; j < la; ++j) {
      const Char ca = next_char(A, an, ai);
      const unsigned up = row[j];
      unsigned v = up < left ? up + 1 : left + 1;
      const unsigned w = diag + (ca != cb);
      if (w < v) v = w;
      diag = up;
      left = v;
      row[j] = (uint16_t)v;
    }
  }
  return row[la - 1];
}

// The bit-vector form's table: bit k of a character's word = target character k is that character.  One word for each of
// the 128 ASCII values, then (character, word) pairs for the target's distinct non-ASCII characters.
struct PeqTable {
  uint64_t ascii[128];
  uint64_t mask[kBitTargetChars];
  Char ch[kBitTargetChars];
  int nlist, m;  // m: the target's characters; 0 when the target does not fit (no character, or more than 64)
};
inline void build_peq(const uint8_t* t, int tn, PeqTable& q) {
  for (int b = 0; b < 128; ++b) q.ascii[b] = 0;
  for (int k = 0; k < kBitTargetChars; ++k) q.mask[k] = 0, q.ch[k] = 0;
  q.nlist = 0;
  q.m = 0;
  const int m = walk_chars(t, tn);
  if (m < 1 || m > kBitTargetChars) return;
  q.m = m;
  int i = 0;
  for (int k = 0; k < m; ++k) {
    const Char c = next_char(t, tn, i);
    if (c < 0x80) {
      q.ascii[c] |= (uint64_t)1 << k;
      continue;
    }
    int s = 0;
    while (s < q.nlist && q.ch[s] != c) ++s;
    if (s == q.nlist) q.ch[q.nlist++] = c;
    q.mask[s] |= (uint64_t)1 << k;
  }
}
// one text character: Pv / Mv the vertical deltas of the column, the score follows bit m - 1 of the horizontal ones; the
// horizontal +1 shifted in at the bottom is row 0 of the global table (D[0][j] = j)
CS_HD void bit_step(uint64_t eq, uint64_t& pv, uint64_t& mv, uint32_t& score, int top) {
  const uint64_t xv = eq | mv;
  const uint64_t xh = (((eq & pv) + pv) ^ pv) | eq;  // (a 64-bit add: two 32-bit adds with carry on the device)
  uint64_t ph = mv | ~(xh | pv);
  uint64_t mh = pv & xh;
  score += (uint32_t)(ph >> top) & 1u;
  score -= (uint32_t)(mh >> top) & 1u;
  ph = (ph << 1) | 1;
  mh <<= 1;
  pv = mh | ~(xv | ph);
  mv = ph & xv;
}
// a row against a target of m = 1..64 characters; a null row: n = 0.  `ascii` / `lch` / `lmask`: the PeqTable where the
// routine runs (LDS in the tile kernel).  Only a row with a byte >= 0x80 decodes characters and searches the list.
CS_HD uint32_t edit_distance_bits(const uint8_t* p, int n, const uint64_t* ascii, const Char* lch, const uint64_t* lmask, int nlist, int m) {
  uint64_t pv = ~(uint64_t)0, mv = 0;
  uint32_t score = (uint32_t)m;
  const int top = m - 1;
  int i = 0;
  for (; i < n && p[i] < 0x80; ++i) bit_step(ascii[p[i]], pv, mv, score, top);
  while (i < n) {
    const Char c = next_char(p, n, i);
    uint64_t eq = 0;
    if (c < 0x80) {
      eq = ascii[c];
    } else {
      for (int s = 0; s < nlist; ++s)
        if (lch[s] == c) eq = lmask[s];
    }
    bit_step(eq, pv, mv, score, top);
  }
  return score;
}

// ---- porter_stemmer_measure --------------------------------------------------------------------------------------------
// The vowels: the ASCII ones as a 128-bit mask (two words, not an array: an indexed array in the kernel arguments goes
// to scratch), up to eight non-ASCII ones packed beside it, any further ones in memory (`more`: the row-wise route only).
struct VowelSpec {
  uint64_t ascii_lo, ascii_hi;
  Char nv[8];
  int nn;
  const Char* more;
  int nmore;
  Char y;
};
constexpr int kPackedVowels = 8;
// `more_where_it_runs`: room for the non-ASCII vowels beyond eight as the routine will read them (the caller fills it
// from `overflow`, which gets them here)
inline VowelSpec make_vowels(const char* vowels, const char* y_char, Char* overflow, int overflow_cap, const Char* more_where_it_runs) {
  VowelSpec s{};
  if (!vowels) vowels = "aeiou";
  if (!y_char) y_char = "y";
  const uint8_t* v = reinterpret_cast<const uint8_t*>(vowels);
  int vn = 0;
  while (v[vn]) ++vn;
  for (int i = 0; i < vn;) {
    const Char c = next_char(v, vn, i);
    if (c < 0x80) {
      (c < 64 ? s.ascii_lo : s.ascii_hi) |= (uint64_t)1 << (c & 63);
    } else if (s.nn < kPackedVowels) {
      s.nv[s.nn++] = c;
    } else if (s.nmore < overflow_cap) {
      overflow[s.nmore++] = c;
    }
  }
  s.more = more_where_it_runs;
  const uint8_t* y = reinterpret_cast<const uint8_t*>(y_char);
  int yn = 0;
  while (y[yn]) ++yn;
  int yi = 0;
  s.y = next_char(y, yn, yi);  // its first character (0 for an empty string: no character is y)
  return s;
}
CS_HD bool is_vowel(Char c, const VowelSpec& s) {
  if (c < 0x80) return (((c & 64) ? s.ascii_hi : s.ascii_lo) >> (c & 63)) & 1;
  bool hit = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < kPackedVowels; ++k) hit |= (k < s.nn) & (s.nv[k] == c);
  for (int k = 0; k < s.nmore; ++k) hit |= s.more[k] == c;
  return hit;
}
CS_HD uint32_t measure_row(const uint8_t* p, int n, const VowelSpec& s) {
  uint32_t vcs = 0;
  bool run = false, prev_vowel = false;  // (the reference starts the run as "character 0 is a vowel": character 0 sets it again)
  for (int i = 0, idx = 0; i < n; ++idx) {
    const Char c = next_char(p, n, i);
    const bool v = is_vowel(c, s);
    const bool consonant = !v && (c != s.y || idx == 0 || prev_vowel);
    vcs += consonant & run;
    run = !consonant;
    prev_vowel = v;
  }
  return vcs;
}

// ---- scatter_count -------------------------------------------------------------------------------------------------------
// scan[0 .. rows]: exclusive scan of the counts (scan[rows] the total); the source row of output row `o` < scan[rows] is the
// last i with scan[i] <= o (rows of count 0 are stepped over)
CS_HD int64_t scatter_source(const int64_t* scan, int64_t rows, int64_t o) {
  int64_t lo = 0, hi = rows;  // scan[lo] <= o < scan[hi]
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (scan[mid] <= o) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace cstxt
