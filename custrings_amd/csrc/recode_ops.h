// Per-row logic of url_encode / url_decode (reference: cpp/src/strings/urlencode.cu, functors url_encoder and
// url_decoder) and translate (modify.cu:302-390).  Shared by the kernels of cs_recode.hip and the g++ harness of
// tests/test_recode_cpu.py; tests/recode_model.py restates it independently.
//
// Every op is a size function and a write function over the row's bytes; the two walk a row the same way, so the write
// puts exactly the bytes the size counted.
//   url_encode  the BYTE rule: an unreserved ASCII byte (0-9 A-Z a-z . _ ~ -, a 128-bit mask) is copied, every other byte
//               becomes '%' and two upper-case hex digits.  On valid UTF-8 that is what the reference's decode-and-re-emit
//               gives; a row that is not valid UTF-8 follows the byte rule too.
//   url_decode  a '%' at byte i with two bytes behind it (i + 2 < n) consumes them and emits one byte; every other byte is
//               copied.  The reference's hex_to_byte takes all of A-Z and a-z as digits (c - 55, c - 87), anything else as
//               0, and wraps in eight bits.
//   translate   each character is looked up once in a table of code point -> code point (0: the character is dropped);
//               unlisted characters are copied.  Characters are walked by lead byte, a sequence the row's end cuts short
//               keeping the bytes there are (chartype_ops.h, pad_ops.h).  A sequence that is not one well-formed character
//               (a stray continuation byte, a cut or broken sequence, an over-long form, an encoded surrogate
//               U+D800..DFFF, a lead byte >= 0xF8) matches no key and is copied byte for byte.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "row_ops.h"

namespace csrecode {

using csrow::is_cont;
using csrow::lead_width;

enum Op { OP_URL_ENCODE = 0, OP_URL_DECODE = 1, OP_TRANSLATE = 2 };

// ---- url_encode ------------------------------------------------------------------------------------------------------------
// the unreserved set as two words (bit c of lo / bit c - 64 of hi); bytes >= 0x80 are never in it
struct SafeMask {
  uint64_t lo, hi;
};
inline SafeMask url_safe_mask() {
  SafeMask m{0, 0};
  const char* keep = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz._~-";
  for (const char* k = keep; *k; ++k) {
    const unsigned c = (unsigned char)*k;
    if (c < 64) m.lo |= (uint64_t)1 << c;
    else m.hi |= (uint64_t)1 << (c - 64);
  }
  return m;
}
CS_HD bool is_safe(const SafeMask& m, uint8_t c) {
  const uint64_t w = c < 64 ? m.lo : m.hi;
  return c < 128 && ((w >> (c & 63)) & 1);
}
CS_HD uint8_t hex_digit(unsigned v) { return (uint8_t)(v < 10 ? '0' + v : 'A' + (v - 10)); }

CS_HD int64_t encode_size(const SafeMask& m, const uint8_t* p, int n) {
  int64_t esc = 0;
  for (int i = 0; i < n; ++i) esc += !is_safe(m, p[i]);
  return (int64_t)n + 2 * esc;
}
CS_HD void encode_write(const SafeMask& m, const uint8_t* p, int n, uint8_t* o) {
  for (int i = 0; i < n; ++i) {
    const uint8_t c = p[i];
    if (is_safe(m, c)) {
      *o++ = c;
    } else {
      *o++ = '%';
      *o++ = hex_digit(c >> 4);
      *o++ = hex_digit(c & 15);
    }
  }
}

// ---- url_decode ------------------------------------------------------------------------------------------------------------
CS_HD unsigned hex_value(uint8_t c) {  // urlencode.cu:188-205
  if (c >= '0' && c <= '9') return c - 48u;
  if (c >= 'A' && c <= 'Z') return c - 55u;
  if (c >= 'a' && c <= 'z') return c - 87u;
  return 0;
}
CS_HD uint8_t hex_to_byte(uint8_t c1, uint8_t c2) { return (uint8_t)((uint8_t)(hex_value(c1) * 16u) + hex_value(c2)); }

CS_HD int64_t decode_size(const uint8_t* p, int n) {
  int64_t k = 0;
  for (int i = 0; i < n; ++k) i += (p[i] == '%' && i + 2 < n) ? 3 : 1;
  return k;
}
CS_HD void decode_write(const uint8_t* p, int n, uint8_t* o) {
  for (int i = 0; i < n;) {
    if (p[i] == '%' && i + 2 < n) {
      *o++ = hex_to_byte(p[i + 1], p[i + 2]);
      i += 3;
    } else {
      *o++ = p[i++];
    }
  }
}

// ---- translate -------------------------------------------------------------------------------------------------------------
constexpr uint32_t kNoKey = 0xFFFFFFFFu;  // an ASCII character the table does not list
constexpr uint32_t kMaxCodePoint = 0x10FFFFu;
constexpr int kAsciiKeys = 128;

struct Table {
  const uint32_t* ascii;  // kAsciiKeys entries: the target of an ASCII key, kNoKey where there is none
  const uint32_t* keys;   // the other keys, ascending and unique
  const uint32_t* vals;   // their targets
  int nkeys;
};

CS_HD int cp_width(uint32_t cp) { return 1 + (cp >= 0x80) + (cp >= 0x800) + (cp >= 0x10000); }
CS_HD void put_cp(uint32_t cp, uint8_t* o) {
  if (cp < 0x80) {
    o[0] = (uint8_t)cp;
  } else if (cp < 0x800) {
    o[0] = (uint8_t)(0xC0 | (cp >> 6));
    o[1] = (uint8_t)(0x80 | (cp & 0x3F));
  } else if (cp < 0x10000) {
    o[0] = (uint8_t)(0xE0 | (cp >> 12));
    o[1] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F));
    o[2] = (uint8_t)(0x80 | (cp & 0x3F));
  } else {
    o[0] = (uint8_t)(0xF0 | (cp >> 18));
    o[1] = (uint8_t)(0x80 | ((cp >> 12) & 0x3F));
    o[2] = (uint8_t)(0x80 | ((cp >> 6) & 0x3F));
    o[3] = (uint8_t)(0x80 | (cp & 0x3F));
  }
}

// the character at p[i]: its bytes in the row (1 .. 4, never past n) and its code point, kNoKey for a malformed sequence
CS_HD int char_at(const uint8_t* p, int i, int n, uint32_t& cp) {
  const uint8_t b = p[i];
  cp = b;
  if (b < 0x80) return 1;
  cp = kNoKey;
  const int w = (int)lead_width(b);
  if (w == 0) return 1;         // a stray continuation byte counts as one
  if (i + w > n) return n - i;  // cut short by the row's end
  if (b >= 0xF8) return w;
  uint32_t u = b & (0xFFu >> (w + 1));
  bool ok = true;
  for (int k = 1; k < w; ++k) {
    ok = ok && is_cont(p[i + k]);
    u = (u << 6) | (p[i + k] & 0x3Fu);
  }
  if (ok && cp_width(u) == w && u <= kMaxCodePoint && (u < 0xD800u || u > 0xDFFFu)) cp = u;
  return w;
}

// the target of code point cp: kNoKey when the table does not list it
CS_HD uint32_t lookup(const Table& t, uint32_t cp) {
  if (cp < (uint32_t)kAsciiKeys) return t.ascii[cp];
  int lo = 0, hi = t.nkeys;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t.keys[mid] < cp) lo = mid + 1;
    else hi = mid;
  }
  return (lo < t.nkeys && t.keys[lo] == cp) ? t.vals[lo] : kNoKey;
}

CS_HD int64_t translate_size(const Table& t, const uint8_t* p, int n) {
  int64_t bytes = 0;
  for (int i = 0; i < n;) {
    uint32_t cp;
    const int w = char_at(p, i, n, cp);
    const uint32_t to = cp == kNoKey ? kNoKey : lookup(t, cp);
    bytes += to == kNoKey ? w : (to ? cp_width(to) : 0);
    i += w;
  }
  return bytes;
}
CS_HD void translate_write(const Table& t, const uint8_t* p, int n, uint8_t* o) {
  for (int i = 0; i < n;) {
    uint32_t cp;
    const int w = char_at(p, i, n, cp);
    const uint32_t to = cp == kNoKey ? kNoKey : lookup(t, cp);
    if (to == kNoKey) {
      for (int k = 0; k < w; ++k) *o++ = p[i + k];
    } else if (to) {
      put_cp(to, o);
      o += cp_width(to);
    }
    i += w;
  }
}

// The table of the caller's n pairs on the host: ASCII keys in the 128-entry array, the others sorted.  Of several pairs
// with one key the last in the caller's order wins (the reference's unstable sort leaves that open).  false: a code point
// above U+10FFFF.
struct HostTable {
  uint32_t ascii[kAsciiKeys];
  std::vector<uint32_t> keys, vals;
};
inline bool make_table(const uint32_t* from, const uint32_t* to, int n, HostTable& h) {
  for (int k = 0; k < kAsciiKeys; ++k) h.ascii[k] = kNoKey;
  std::vector<int> order;
  for (int k = 0; k < n; ++k) {
    if (from[k] > kMaxCodePoint || to[k] > kMaxCodePoint) return false;
    if (from[k] < (uint32_t)kAsciiKeys) h.ascii[from[k]] = to[k];
    else order.push_back(k);
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return from[a] < from[b]; });
  h.keys.clear();
  h.vals.clear();
  for (size_t j = 0; j < order.size(); ++j) {
    if (j + 1 < order.size() && from[order[j + 1]] == from[order[j]]) continue;  // (a later pair has the key)
    h.keys.push_back(from[order[j]]);
    h.vals.push_back(to[order[j]]);
  }
  return true;
}

}  // namespace csrecode
