// Per-row logic of compute_statistics / get_info (reference: cpp/src/strings/NVStrings.cu:604-775; the per-row memory figure
// custring_view.inl:146-171).  Shared by the kernels of cs_stats.hip and the g++ harness of tests/test_stats_cpu.py;
// tests/stats_model.py restates it independently.
//
// ONE walk over a row's bytes yields
//   chars   the row's characters as cs_len counts them: the bytes that are no continuation byte (10xxxxxx)
//   the four class counts: the characters whose code point is <= U+FFFF and whose flag-table byte has the space (16),
//           digit (4), upper (32) or lower (64) bit.  The ASCII half of each class is a 128-bit membership mask made on the
//           host from the table's first 128 entries (as PredSpec has it, chartype_ops.h): an ASCII byte costs no look-up.
//   hist(cp) for every character whose code point is <= U+FFFF (the caller counts it; code point 0 is counted like any
//           other and left out when the table is compacted)
// A character is what row_ops.h's decode_at takes: a lead byte and the bytes its width announces,
// bytes past the row's end read as 0; a continuation byte where a lead byte should be is a character of its own (its code
// point the low six bits).  On well-formed UTF-8 the walk meets exactly `chars` characters; on malformed bytes `chars`
// keeps cs_len's rule (every non-continuation byte counts, also one a lead byte announced over) while the classes and the
// histogram follow the walk.
#pragma once
#include <stdint.h>

#include "row_ops.h"

namespace csstat {

using csrow::is_cont;
using csrow::lead_width;
using csrow::packed_to_cp;

// flag bits of the 64 K table (chartype_ops.h)
constexpr unsigned kSpace = 16, kDigit = 4, kUpper = 32, kLower = 64;

// two 64-bit words per class, not an array: an indexed array in the kernel arguments goes to scratch
struct ClassSpec {
  uint64_t space_lo, space_hi, digit_lo, digit_hi, upper_lo, upper_hi, lower_lo, lower_hi;
  const uint8_t* flags;  // the 64 K table where the routine runs (device memory in kernels)
};
// `table`: the flag table as the caller of this function can read it (its first 128 entries make the masks)
inline ClassSpec make_classes(const uint8_t* table, const uint8_t* flags_where_it_runs) {
  ClassSpec s{0, 0, 0, 0, 0, 0, 0, 0, flags_where_it_runs};
  for (unsigned b = 0; b < 128; ++b) {
    const uint64_t bit = (uint64_t)1 << (b & 63);
    const unsigned f = table[b];
    if (f & kSpace) (b < 64 ? s.space_lo : s.space_hi) |= bit;
    if (f & kDigit) (b < 64 ? s.digit_lo : s.digit_hi) |= bit;
    if (f & kUpper) (b < 64 ? s.upper_lo : s.upper_hi) |= bit;
    if (f & kLower) (b < 64 ? s.lower_lo : s.lower_hi) |= bit;
  }
  return s;
}

struct RowStats {
  int chars, space, digit, upper, lower;
};

// per-row memory of the reference's string object (custring_view::alloc_size): header, bytes, NUL and -- when some
// character is wider than a byte -- a 2-bit width entry per character, in whole words
CS_HD unsigned row_mem(int bytes, int chars) { return 8u + (unsigned)bytes + 1u + (chars != bytes ? ((unsigned)chars + 3u) / 4u : 0u); }

// CLASSES false: `chars` and the histogram only (the class counts stay 0)
template <bool CLASSES, class Hist>
CS_HD RowStats walk_row(const uint8_t* p, int n, const ClassSpec& s, Hist&& hist) {
  RowStats r{0, 0, 0, 0, 0};
  for (int i = 0; i < n;) {
    const uint8_t b = p[i];
    if (b < 0x80) {
      ++r.chars;
      if (CLASSES) {
        const unsigned sh = b & 63;
        const bool hi = (b & 64) != 0;
        r.space += (int)(((hi ? s.space_hi : s.space_lo) >> sh) & 1);
        r.digit += (int)(((hi ? s.digit_hi : s.digit_lo) >> sh) & 1);
        r.upper += (int)(((hi ? s.upper_hi : s.upper_lo) >> sh) & 1);
        r.lower += (int)(((hi ? s.lower_hi : s.lower_lo) >> sh) & 1);
      }
      hist((unsigned)b);
      ++i;
      continue;
    }
    const unsigned w = lead_width(b);
    uint32_t c = b;
    r.chars += w != 0;
    for (unsigned k = 1; k < w; ++k) {
      uint8_t x = 0;
      if (i + (int)k < n) {
        x = p[i + k];
        r.chars += !is_cont(x);
      }
      c = (c << 8) | x;
    }
    const unsigned u = packed_to_cp(c);
    if (u <= 0xFFFF) {
      if (CLASSES) {
        const unsigned f = s.flags[u];
        r.space += (f & kSpace) != 0;
        r.digit += (f & kDigit) != 0;
        r.upper += (f & kUpper) != 0;
        r.lower += (f & kLower) != 0;
      }
      hist(u);
    }
    i += w ? (int)w : 1;
  }
  return r;
}

}  // namespace csstat
