// Per-row logic of from_csv (reference: cpp/src/util.cu:42-169, createFromCSV): the byte classes of the line scan and the
// walk that finds one column's field in a row.  Shared by the kernels of cs_csv.hip and the g++ harness of
// tests/test_csv_cpu.py; tests/csv_model.py restates it independently.
//
// A row is the span between two line starts: the line's bytes, its first terminator ('\r' or '\n') and the control bytes
// (1..31) the line scan skipped behind it.  The reference overwrites the first terminator with a NUL before the walk; here
// nothing is written into the text: the walk reads the first '\r' or '\n' of the span as 0 and every later byte as it is
// (no span holds a NUL byte of its own: the text ends at the first one).
//   a '"' while quoted, followed by another: both are taken and stay in the field (length += 2); else: quoted mode ends
//   a '"' while not quoted at length 0: quoted mode begins and the field begins behind it
//   any other '"' is left out of the COUNT but not out of the span: "abc"def, gives abc"de
//   a ',' outside quotes, or the 0, ends the field: the walk stops when it is the column asked for, else the next field begins
//   a row with too few columns runs on past its terminator into the skipped control bytes
#pragma once
#include <stdint.h>

#include "row_ops.h"

namespace cscsv {

enum Flags { kSortLength = 1, kSortName = 2, kNullIsEmpty = 8 };  // util.h:27-29

CS_HD bool is_control(uint8_t b) { return (uint8_t)(b - 1) < 31; }  // 1..31: what the line scan skips behind a terminator
CS_HD bool is_terminator(uint8_t b) { return b == '\r' || b == '\n'; }

// ---- the line scan by 16-byte pieces (cs_csv.hip: a piece per lane) ---------------------------------------------------------
// A position p is a line start when b[p] is no control byte, b[p - 1] is one, and the run of control bytes that ends at
// p - 1 holds a terminator.  Walking the text, that is a state: 0 the last byte was no control byte, 1 inside a run
// of control bytes with no terminator so far, 2 inside one that holds a terminator; a byte that is no control byte is a
// line start when the state before it is 2.
constexpr int kPieceBytes = 16;
struct Piece {  // bit i of each mask: byte i of the piece
  uint32_t control, terminator, nul;
};
// 0x80 in every byte of x that is zero (exact: no borrow between bytes)
CS_HD uint32_t zero_bytes(uint32_t x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }
// the four 0x80 bits of m as bits 0..3 (bit 7 -> 28, 15 -> 29, 23 -> 30, 31 -> 31: no two products meet)
CS_HD uint32_t pack_high_bits(uint32_t m) { return ((m >> 7) * 0x10204080u) >> 28; }
CS_HD Piece classify(const uint32_t w[4]) {  // the piece as four little-endian words
  Piece p{0, 0, 0};
  for (int k = 0; k < 4; ++k) {
    const uint32_t nul = zero_bytes(w[k]), low = zero_bytes(w[k] & 0xE0E0E0E0u);  // low: bytes below 0x20
    const uint32_t term = zero_bytes(w[k] ^ 0x0A0A0A0Au) | zero_bytes(w[k] ^ 0x0D0D0D0Du);
    p.nul |= pack_high_bits(nul) << (4 * k);
    p.control |= pack_high_bits(low & ~nul) << (4 * k);
    p.terminator |= pack_high_bits(term) << (4 * k);
  }
  return p;
}
// The line starts inside a piece entered in state `in`, as a mask; `out`: the state behind it.  One addition does the walk:
// a terminator generates a carry, a control byte passes it on, any other byte takes it (a line start) and ends it.
CS_HD uint32_t piece_starts(const Piece& p, int in, int& out) {
  const uint32_t sum = p.control + p.terminator + (in == 2 ? 1u : 0u);
  out = (sum >> kPieceBytes) & 1 ? 2 : (int)((p.control >> (kPieceBytes - 1)) & 1);
  return sum & ~p.control & 0xFFFFu;
}

// the field of a row: bytes [begin, begin + length) of the span; begin < 0: a null row
struct Field {
  int32_t begin, length;
  CS_HD Field() : begin(0), length(0) {}
  CS_HD Field(int32_t b, int32_t n) : begin(b), length(n) {}
  CS_HD explicit Field(int) : begin(0), length(0) {}  // (the parse route compares results with T(0))
  CS_HD bool is_null() const { return begin < 0; }
  CS_HD bool operator!=(const Field& o) const { return begin != o.begin || length != o.length; }
};

// util.cu:103-160 over the span line[0, n), n >= 1
CS_HD Field locate_field(const uint8_t* line, int n, unsigned column, bool null_is_empty) {
  int sptr = 0, length = 0;
  unsigned col = 0;
  bool quoted = false, terminated = false;
  for (int i = 0; i < n; ++i) {
    uint8_t ch = line[i];
    if (!terminated && is_terminator(ch)) {
      terminated = true;
      ch = 0;
    }
    if (ch) {
      if (ch == '"') {
        if (quoted) {
          // (the byte behind a quote is inside the span: a span ends with its terminator or a control byte)
          if (line[i + 1] != '"') {
            quoted = false;
          } else {
            ++i;
            length += 2;
          }
          continue;
        }
        if (length == 0) {
          quoted = true;
          ++sptr;
        }
        continue;
      }
      if (quoted || ch != ',') {
        ++length;
        continue;
      }
    }
    if (col++ >= column) break;
    sptr = i + 1;
    length = 0;
    quoted = false;
  }
  if (length == 0 && !null_is_empty) return Field(-1, 0);
  return Field(sptr, length);
}

}  // namespace cscsv
