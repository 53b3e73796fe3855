// Per-row logic of the character-type predicates and of swapcase / capitalize / title (reference:
// cpp/src/strings/attrs.cu:115-438, case.cu:169-397; flag bits is_flags.h:33-40).  Shared by the kernels of
// cs_chartype.hip / cs_casemodes.hip and the g++ harness of tests/test_chartype_cpu.py; tests/chartype_model.py restates it
// independently, over characters.
//
// Flag bits of the 64 K table: decimal 1, numeric 2, digit 4, alpha 8, space 16, upper 32, lower 64; a character above
// U+FFFF has flags 0.  cases[cp] is the opposite-case code point.
//
// Predicates (one byte a row):
//   isalnum (flags & 15), isalpha (8), isdigit (4), isspace (16), isdecimal (1), isnumeric (2):
//       true when the row is not empty and EVERY character has one of the bits; a null row and an empty one are false
//   islower: not empty and every character is `!alpha || lower`;  isupper: `!alpha || upper`
//       ("123" is both; a cased character the table does not call alphabetic -- U+2160 -- never makes either false)
//   is_empty: true for a null row and for an empty one (offsets and validity only: cs_chartype.hip)
// Case ops (a new row; null rows stay null):
//   swapcase:   every character with the upper or the lower bit becomes cases[cp]
//   capitalize: the first character, if lower, and every later one, if upper, is mapped -- but only when its code point is
//               <= 0x0FFF (the reference compares with 0x00FFF, three F's): a cased character above U+0FFF passes through
//   title:      `capnext` starts true; a non-alphabetic character sets it and is copied (also when it is cased); an
//               alphabetic one is mapped if (capnext && lower) || (!capnext && upper) and clears it.  Every non-letter is
//               a word break.
// A mapping may change a character's UTF-8 width (U+00DF -> 'S', U+0131 -> 'I', U+023A -> U+2C65, ...).
// Malformed UTF-8: these routines over row_ops.h's decode_at ARE the definition: a character is what
// decode_at takes, a mapped one is re-encoded from its code point, an unmapped one keeps its bytes (a truncated
// character at the end of a row is written at its announced width, the missing bytes as 0, as lower / upper do).
#pragma once
#include <stdint.h>

#include "row_ops.h"

namespace cschr {

using csrow::Char;
using csrow::cp_to_packed;
using csrow::decode_at;
using csrow::packed_to_cp;
using csrow::packed_width;

enum Pred { P_ALNUM = 0, P_ALPHA, P_DIGIT, P_SPACE, P_DECIMAL, P_NUMERIC, P_LOWER, P_UPPER, P_EMPTY, P_COUNT };
enum Rule { RULE_ANY_BIT = 0, RULE_CASED = 1 };  // (flags & mask) != 0;  !alpha || (flags & mask)
enum CaseOp { OP_SWAPCASE = 0, OP_CAPITALIZE = 1, OP_TITLE = 2 };

CS_HD unsigned pred_mask(int pred) {
  return pred == P_ALNUM ? 15u : pred == P_ALPHA ? 8u : pred == P_DIGIT ? 4u : pred == P_SPACE ? 16u : pred == P_DECIMAL ? 1u
       : pred == P_NUMERIC ? 2u : pred == P_LOWER ? 64u : 32u;
}
CS_HD int pred_rule(int pred) { return pred == P_LOWER || pred == P_UPPER ? RULE_CASED : RULE_ANY_BIT; }
CS_HD bool flags_pass(unsigned f, unsigned mask, int rule) { return rule == RULE_CASED ? (!(f & 8u) || (f & mask)) : (f & mask) != 0; }

// A predicate with its ASCII half folded into a 128-bit membership mask (bit b: ASCII byte b passes), so that an ASCII byte
// costs no table look-up; two 64-bit words, not an array: an indexed array in the kernel arguments goes to scratch.
struct PredSpec {
  uint64_t ascii_lo, ascii_hi;
  unsigned mask;
  int rule;
  const uint8_t* flags;  // the 64 K table where the routine runs (device memory in kernels)
};
// `table`: the flag table as the caller of this function can read it (its first 128 entries make the mask)
inline PredSpec make_pred(int pred, const uint8_t* table, const uint8_t* flags_where_it_runs) {
  PredSpec s{0, 0, pred_mask(pred), pred_rule(pred), flags_where_it_runs};
  for (unsigned b = 0; b < 128; ++b)
    if (flags_pass(table[b], s.mask, s.rule)) (b < 64 ? s.ascii_lo : s.ascii_hi) |= (uint64_t)1 << (b & 63);
  return s;
}
// stops at the first character that decides the row
CS_HD bool pred_row(const uint8_t* p, int n, const PredSpec& s) {
  for (int i = 0; i < n;) {
    const uint8_t b = p[i];
    if (b < 0x80) {
      if (!(((b & 64) ? s.ascii_hi : s.ascii_lo) >> (b & 63) & 1)) return false;
      ++i;
      continue;
    }
    Char ch;
    unsigned w = decode_at(p, i, n, ch);
    if (w == 0) w = 1;
    const unsigned u = packed_to_cp(ch);
    if (!flags_pass(u <= 0xFFFF ? s.flags[u] : 0u, s.mask, s.rule)) return false;
    i += (int)w;
  }
  return n > 0;
}

// one character of a case op; `start`: capitalize -- no character seen yet; title -- capnext
CS_HD Char case_char(Char ch, int op, const uint8_t* flags, const uint16_t* cases, bool& start) {
  const unsigned u = packed_to_cp(ch);
  const unsigned f = u <= 0xFFFF ? flags[u] : 0u;
  if (op == OP_SWAPCASE) {
    if (f & 96u) ch = cp_to_packed(cases[u]);
  } else if (op == OP_CAPITALIZE) {
    if (start ? (f & 64u) : (f & 32u)) ch = cp_to_packed(u <= 0x0FFF ? cases[u] : u);
    start = false;
  } else {
    if (!(f & 8u)) {
      start = true;
    } else {
      if (start ? (f & 64u) : (f & 32u)) ch = cp_to_packed(cases[u]);
      start = false;
    }
  }
  return ch;
}
CS_HD int case_size(const uint8_t* p, int n, const uint8_t* flags, const uint16_t* cases, int op) {
  int out = 0;
  bool start = true;
  for (int i = 0; i < n;) {
    Char ch;
    unsigned w = decode_at(p, i, n, ch);
    if (w == 0) w = 1;
    out += (int)packed_width(case_char(ch, op, flags, cases, start));
    i += (int)w;
  }
  return out;
}
CS_HD void case_write(const uint8_t* p, int n, const uint8_t* flags, const uint16_t* cases, int op, uint8_t* o) {
  bool start = true;
  for (int i = 0; i < n;) {
    Char ch;
    unsigned w = decode_at(p, i, n, ch);
    if (w == 0) w = 1;
    ch = case_char(ch, op, flags, cases, start);
    const unsigned ow = packed_width(ch);
    for (unsigned k = 0; k < ow; ++k) *o++ = (uint8_t)(ch >> (8 * (ow - 1 - k)));
    i += (int)w;
  }
}

// ---- the tile kernels' byte-parallel steps (four bytes a word; valid when the table's ASCII half is the plain one:
// ascii_plain below) ------------------------------------------------------------------------------------------------------
// 0x80 in every byte lane that holds an ASCII upper-case (`upper` true) / lower-case letter
CS_HD uint32_t swar_letters(uint32_t w, bool upper) {
  const uint32_t x = w & 0x7F7F7F7Fu;
  const uint32_t lo = upper ? 0x3F3F3F3Fu : 0x1F1F1F1Fu;  // 0x80 - first letter
  const uint32_t hi = upper ? 0x25252525u : 0x05050505u;  // 0x7F - last letter
  return (x + lo) & ~(x + hi) & ~w & 0x80808080u;
}
CS_HD uint32_t swar_swapcase(uint32_t w) { return w ^ ((swar_letters(w, true) | swar_letters(w, false)) >> 2); }
CS_HD uint32_t swar_lower(uint32_t w) { return w ^ (swar_letters(w, true) >> 2); }
// `before`: the byte in front of the word's first byte.  A letter becomes upper case when the byte before it is not a
// letter, lower case otherwise.
CS_HD uint32_t swar_title(uint32_t w, uint32_t before) {
  const uint32_t up = swar_letters(w, true), lw = swar_letters(w, false);
  const uint32_t pw = (w << 8) | (before & 0xFFu);
  const uint32_t after_letter = swar_letters(pw, true) | swar_letters(pw, false);
  return w ^ (((lw & ~after_letter) | (up & after_letter)) >> 2);
}
// a row's first byte after the piece pass of capitalize / title: its predecessor belongs to another row
CS_HD uint8_t ascii_first(uint8_t b) { return (b >= 'a' && b <= 'z') ? (uint8_t)(b - 32) : b; }
// one 16-byte piece (q[0..3], little-endian words); `before`: the byte in front of it (title only)
CS_HD void swar_piece(int op, const uint32_t q[4], uint32_t before, uint32_t o[4]) {
  if (op == OP_SWAPCASE) {
    for (int k = 0; k < 4; ++k) o[k] = swar_swapcase(q[k]);
  } else if (op == OP_CAPITALIZE) {
    for (int k = 0; k < 4; ++k) o[k] = swar_lower(q[k]);
  } else {
    o[0] = swar_title(q[0], before);
    for (int k = 1; k < 4; ++k) o[k] = swar_title(q[k], q[k - 1] >> 24);
  }
}
// The byte-parallel steps hold when ASCII maps the plain way (A-Z <-> a-z, nothing else cased) and, for title, the
// alphabetic ASCII bytes are exactly the 52 letters.
inline bool ascii_plain(const uint8_t* f, const uint16_t* c) {
  for (unsigned b = 0; b < 128; ++b) {
    const bool up = b >= 'A' && b <= 'Z', lw = b >= 'a' && b <= 'z';
    if (((f[b] & 32u) != 0) != up || ((f[b] & 64u) != 0) != lw || ((f[b] & 8u) != 0) != (up || lw)) return false;
    if (up && c[b] != b + 32) return false;
    if (lw && c[b] != b - 32) return false;
  }
  return true;
}

}  // namespace cschr
