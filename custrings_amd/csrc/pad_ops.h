// Per-row logic of the substring / padding / wrapping ops (reference: cpp/src/strings/substr.cu, pad.cu and the
// slice_replace / insert members of modify.cu; custring_view.inl:801-860, 964-1148).  Shared by the kernels of
// cs_pad.hip and the g++ harness of tests/test_pad_cpu.py; tests/pad_model.py restates it independently.
//
// Every op but wrap turns a row into at most four pieces, in this order:
//   `pre` fill characters, source bytes [a0, a1), an insert (`fill` fill characters or the replacement), source bytes
//   [b0, b1)
// and repeat emits the whole `reps` times.  A slice with a step > 1 takes every step-th character of [a0, a1) instead
// (`stride`).  wrap keeps every byte's place and changes some of them (wrap_row).
//
// Character positions are UNSIGNED as in the reference (a negative start is past the end), with its quirks:
//   slice:          stop <= 0 means the end of the row; (the host throws when stop > 0 && start > stop)
//   slice_replace:  `start < chars_count()` compares signed with unsigned, so a negative start appends;
//                   a stop before the start leaves the row as it is
//   insert:         `start <= (int)chars_count()` (signed), -1 = the end; beyond the end the row is left as it is
//   zfill:          fills every row, numeric or not, after a leading '+' / '-'
// One deviation: a strided slice takes characters start, start + step, ... below stop (Python's rule),
// where the reference counts the slice's length in bytes and reads past stop on multi-byte rows.
#pragma once
#include <stdint.h>

#include "row_ops.h"

namespace cspad {

using csrow::count_chars;
using csrow::lead_width;
using csrow::offset_for_char_pos;

enum Op {
  OP_SLICE = 0,  // slice / get / slice_from
  OP_SLICE_REPLACE = 1,
  OP_INSERT = 2,
  OP_REPEAT = 3,
  OP_RJUST = 4,  // pad, side left (padside::left)
  OP_LJUST = 5,  // pad, side right
  OP_CENTER = 6, // pad, side both
  OP_ZFILL = 7,
  OP_WRAP = 8,
};

struct Params {
  int op;
  int start, stop;      // slice, slice_replace, insert (slice_from: per row)
  unsigned step;        // slice
  unsigned width;       // pad family, zfill, wrap
  unsigned reps;        // repeat
  uint32_t fill;        // the fill character's UTF-8 bytes, the first in the low byte (zfill: '0'); a word, not an array:
                        // an indexed array in the kernel arguments' copy goes to scratch
  int fillw;            // its byte count
  int replen;           // slice_replace / insert
  const uint8_t* repl;  // replen bytes
};

struct Pieces {
  int64_t pre;      // fill characters in front
  int a0, a1;       // first source range
  int64_t fill;     // fill characters after it (unless `repl`)
  bool repl;        // the insert is the replacement
  int b0, b1;       // second source range
  int64_t reps;     // the pieces repeated (repeat; else 1)
  unsigned stride;  // > 1: every stride-th character of [a0, a1) only (strided slice)
};

// one character on from byte i (a stray continuation byte counts as one, as byte_of_char has it)
CS_HD int next_char(const uint8_t* p, int i) {
  const unsigned w = lead_width(p[i]);
  return i + (w ? (int)w : 1);
}

CS_HD uint8_t fill_byte(const Params& P, int b) { return (uint8_t)(P.fill >> (8 * b)); }

// the pieces of a valid row p[0, n); start / stop are the op's, or the row's own for slice_from
CS_HD Pieces plan_row(const Params& P, const uint8_t* p, int n, int start, int stop) {
  Pieces pc;
  pc.pre = 0;
  pc.a0 = 0;
  pc.a1 = n;
  pc.fill = 0;
  pc.repl = false;
  pc.b0 = pc.b1 = 0;
  pc.reps = 1;
  pc.stride = 1;
  if (P.op == OP_REPEAT) {  // pad.cu:28-85
    pc.reps = P.reps > 1 && n > 0 ? (int64_t)P.reps : 1;  // (an empty row stays empty: no loop over the count)
    return pc;
  }
  if (P.op == OP_WRAP) return pc;
  const int nchars = count_chars(p, n);
  switch (P.op) {
    case OP_SLICE: {  // substr.cu:39-130: len = (stop <= 0 ? nchars : stop) - start, the end at start + len (unsigned)
      const unsigned e = stop <= 0 ? (unsigned)nchars : (unsigned)stop;
      const int spos = offset_for_char_pos(p, n, nchars, (unsigned)start);
      const int epos = offset_for_char_pos(p, n, nchars, e);
      pc.a0 = spos;
      pc.a1 = spos < epos ? epos : spos;
      pc.stride = P.step > 1 ? P.step : 1;
      return pc;
    }
    case OP_SLICE_REPLACE: {  // modify.cu:35-106; custring_view.inl:1041-1069
      pc.repl = true;
      if ((unsigned)start < (unsigned)nchars) {
        unsigned end = (unsigned)start + ((unsigned)stop - (unsigned)start);
        if (end > (unsigned)nchars) end = (unsigned)nchars;
        if ((unsigned)start > end) {  // (the range overlaps itself: the row as it is)
          pc.repl = false;
          return pc;
        }
        pc.a1 = offset_for_char_pos(p, n, nchars, (unsigned)start);
        pc.b0 = offset_for_char_pos(p, n, nchars, end);
        pc.b1 = n;
      }  // (else the replacement is appended)
      return pc;
    }
    case OP_INSERT: {  // modify.cu:494-552
      if (start <= nchars) {
        const unsigned pos = start < 0 ? (unsigned)nchars : (unsigned)start;
        const int spos = offset_for_char_pos(p, n, nchars, pos);
        pc.a1 = spos;
        pc.repl = true;
        pc.b0 = spos;
        pc.b1 = n;
      }
      return pc;
    }
    default: break;
  }
  // the pad family and zfill (pad.cu:98-353)
  if (P.width <= (unsigned)nchars) return pc;
  const int64_t pad = (int64_t)(P.width - (unsigned)nchars);
  if (P.op == OP_LJUST) {
    pc.fill = pad;
  } else if (P.op == OP_RJUST) {
    pc.pre = pad;
  } else if (P.op == OP_CENTER) {
    pc.pre = pad / 2;
    pc.fill = pad - pad / 2;
  } else {  // zfill: after a leading sign
    const int pos = (n > 0 && (p[0] == '-' || p[0] == '+')) ? 1 : 0;
    pc.a1 = pos;
    pc.fill = pad;
    pc.b0 = pos;
    pc.b1 = n;
  }
  return pc;
}

// bytes of one copy of the pieces (no stride)
CS_HD int64_t period_bytes(const Params& P, const Pieces& pc) {
  return pc.pre * P.fillw + (pc.a1 - pc.a0) + (pc.repl ? (int64_t)P.replen : pc.fill * P.fillw) + (pc.b1 - pc.b0);
}

// the output row's size in bytes (it may reach 2^31 and more: the caller checks)
CS_HD int64_t out_size(const Params& P, const Pieces& pc, const uint8_t* p) {
  if (pc.stride > 1) {
    int64_t bytes = 0;
    unsigned k = 0;
    for (int i = pc.a0; i < pc.a1; ++k) {
      const int j = next_char(p, i);
      if (k % pc.stride == 0) bytes += (j < pc.a1 ? j : pc.a1) - i;
      i = j;
    }
    return bytes;
  }
  return period_bytes(P, pc) * pc.reps;
}

// byte j of one period of the pieces (the long rows of the from-memory path: a byte a lane); no stride
CS_HD uint8_t period_byte(const Params& P, const Pieces& pc, const uint8_t* p, int64_t j) {
  const int64_t lp = pc.pre * P.fillw;
  if (j < lp) return fill_byte(P, (int)(j % P.fillw));
  j -= lp;
  const int64_t la = pc.a1 - pc.a0;
  if (j < la) return p[pc.a0 + j];
  j -= la;
  const int64_t li = pc.repl ? (int64_t)P.replen : pc.fill * P.fillw;
  if (j < li) return pc.repl ? P.repl[j] : fill_byte(P, (int)(j % P.fillw));
  return p[pc.b0 + (j - li)];
}

CS_HD void put_fill(const Params& P, int64_t k, uint8_t* o) {
  for (int64_t i = 0; i < k; ++i)
    for (int b = 0; b < P.fillw; ++b) *o++ = fill_byte(P, b);
}

// wrap (pad.cu:355-436) over a row already copied to `o`: every character <= ' ' becomes ' ', some of them '\n'
CS_HD void wrap_row(const uint8_t* p, int n, unsigned width, uint8_t* o) {
  int last_b = -1, last_c = -1, spos = 0;
  unsigned pos = 0;
  for (int i = 0; i < n; i = next_char(p, i), ++pos) {
    if (p[i] <= ' ') {  // (a multi-byte character is never <= ' ')
      o[i] = ' ';
      last_b = i;
      last_c = (int)pos;
    }
    if (pos - (unsigned)spos >= width && last_b >= 0) {
      o[last_b] = '\n';
      spos = last_c;
      last_b = last_c = -1;
    }
  }
}

// the strided slice's characters to o
CS_HD void write_strided(const Pieces& pc, const uint8_t* p, uint8_t* o) {
  unsigned k = 0;
  for (int i = pc.a0; i < pc.a1; ++k) {
    const int j = next_char(p, i);
    if (k % pc.stride == 0)
      for (int t = i; t < j && t < pc.a1; ++t) *o++ = p[t];
    i = j;
  }
}

// the whole output row to o[0, out_size) -- the row-wise write and the harness
CS_HD void write_row(const Params& P, const Pieces& pc, const uint8_t* p, int n, uint8_t* o) {
  if (P.op == OP_WRAP) {
    for (int i = 0; i < n; ++i) o[i] = p[i];
    wrap_row(p, n, P.width, o);
    return;
  }
  if (pc.stride > 1) {
    write_strided(pc, p, o);
    return;
  }
  for (int64_t r = 0; r < pc.reps; ++r) {
    put_fill(P, pc.pre, o);
    o += pc.pre * P.fillw;
    for (int i = pc.a0; i < pc.a1; ++i) *o++ = p[i];
    if (pc.repl) {
      for (int i = 0; i < P.replen; ++i) *o++ = P.repl[i];
    } else {
      put_fill(P, pc.fill, o);
      o += pc.fill * P.fillw;
    }
    for (int i = pc.b0; i < pc.b1; ++i) *o++ = p[i];
  }
}

// the fill character of the pad family: the first UTF-8 character of `fillchar`, null or empty = ' ' (pad.cu:104-107); a
// character cut short by the string's end keeps the bytes there are
inline void set_fill(Params& P, const char* fillchar) {
  const uint8_t* f = reinterpret_cast<const uint8_t*>(fillchar);
  if (!f || !*f) f = reinterpret_cast<const uint8_t*>(" ");
  const unsigned w = lead_width(f[0]);
  P.fillw = w ? (int)w : 1;
  P.fill = 0;
  for (int i = 0; i < P.fillw; ++i) {
    if (i > 0 && !f[i]) {
      P.fillw = i;
      break;
    }
    P.fill |= (uint32_t)f[i] << (8 * i);
  }
}

}  // namespace cspad
