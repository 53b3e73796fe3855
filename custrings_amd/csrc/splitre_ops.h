// Per-row logic of split_re / rsplit_re: a row's token spans from its match spans.  Shared by the kernel k_token_spans of
// cs_regex.hip (both span layouts) and the g++ harness of tests/test_splitre_cpu.py, which checks it against the model of
// tests/splitre_model.py.
//
// Matches: a row's matches are exactly those count_re counts and findall returns -- left to right, not overlapping, in
//   that order (DESIGN.md section 9 for rows with a NUL byte).  They are always found left to right; only the choice of
//   which ones cut differs between the two directions.
// Cuts: a row with m matches has s = m cuts when maxsplit <= 0, else min(m, maxsplit).  split_re cuts at the first s
//   matches: its last token runs to the row's end and keeps any further match inside it.  rsplit_re cuts at the last s:
//   its first token starts at the row's beginning and keeps any earlier match inside it.
// Tokens: a row has s + 1 of them.  A token between two adjacent matches, before a match at the row's start or after
//   one at the row's end is an empty string, not a null; a valid empty row has one empty token.
// Columns: column k holds every row's token k; a row is null in every column from its token count on, a null row in
//   every column (and has an empty record in the record form).  The column count is the largest token count of a row;
//   zero rows and only null rows answer as cs_split answers for the same column.
// Refused (CS_ERR_INVALID_ARG): the empty pattern and a pattern that can match the empty string.
#pragma once
#include <stdint.h>

#include "row_ops.h"

namespace cssre {

constexpr uint32_t kNullSpan = 0xFFFFFFFFu;  // packed spans (begin << 16 | length): a null

// cuts of a row with m matches
CS_HD int cuts(int m, int maxsplit) { return maxsplit <= 0 || m < maxsplit ? m : maxsplit; }
// the match that makes cut 0: cut j is match first_cut + j
CS_HD int first_cut(int m, int s, bool reverse) { return reverse ? m - s : 0; }

// A row's walk over its tokens, k = 0, 1, ...: where the previous cut ended.
struct Walk {
  int prev_end = 0;
};
// Token k of a row of n bytes with s cuts.  For k < s the caller passes cut k's match (mb, ml: begin and length);
// for k >= s they are not read.  False: the row has no token k (null in column k).
CS_HD bool token_span(Walk& w, int k, int s, int n, int mb, int ml, int& tb, int& tl) {
  if (k > s) return false;
  tb = w.prev_end;
  if (k == s) {
    tl = n - tb;
    return true;
  }
  tl = mb - tb;
  w.prev_end = mb + ml;
  return true;
}

}  // namespace cssre
