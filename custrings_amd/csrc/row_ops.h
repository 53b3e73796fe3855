// Per-row string logic of the hot path, written in BYTE-OFFSET space over the
// native offsets+chars column (the reference works in character positions on
// its custring_view objects; results are identical for valid UTF-8, which is
// the reference's own input contract).
//
// Everything here is `__host__ __device__` so that the very same functions run
// inside the HIP kernels (kernels.hip) and inside the CPU row-emulation harness
// tests/rowemu (which checks them against oracle/ without a GPU).
//
// Reference semantics restated (paths under /root/reference/cpp/src):
//   UTF-8 helpers      custring_view.inl:48-57,1714-1766 ; util.inl:22-75
//   find / contains    custring_view.inl:481-514 ; strings/find.cu:75-120,237-272
//   replace            strings/modify.cu:109-192
//   strip              custring_view.inl:1398-1598 ; strings/strip.cu
//   lower / upper      strings/case.cu:31-170
//   split              custring_view.inl:1223-1250 ; strings/split.cu:32-87,734-956
//   tokenize           text/tokens.cu:41-121
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CS_HD __host__ __device__ __forceinline__
#else
#define CS_HD inline
#endif

namespace csrow {

typedef uint32_t Char;  // 1-4 raw UTF-8 bytes, big-endian packed

CS_HD bool is_cont(uint8_t b) { return (b & 0xC0) == 0x80; }
// width implied by a lead byte; 0 for a continuation byte
CS_HD unsigned lead_width(uint8_t b) {
  return 1u + ((b & 0xF0) == 0xF0) + ((b & 0xE0) == 0xE0) + ((b & 0xC0) == 0xC0) -
         ((b & 0xC0) == 0x80);
}
// decode the char starting at p[i]; bytes at or past `n` read as 0
CS_HD unsigned decode_at(const uint8_t* p, int i, int n, Char& c) {
  uint8_t b = p[i];
  c = b;
  if (b < 0x80) return 1;
  unsigned w = lead_width(b);
  for (unsigned k = 1; k < w; ++k) c = (c << 8) | ((i + (int)k < n) ? p[i + k] : 0);
  return w;
}
CS_HD unsigned packed_width(Char c) {
  return 1u + ((c & 0xFF00u) > 0) + ((c & 0xFF0000u) > 0) + ((c & 0xFF000000u) > 0);
}
CS_HD unsigned cp_to_packed(unsigned u) {
  if (u < 0x80) return u;
  if (u < 0x800) return ((u << 2) & 0x1F00) | (u & 0x3F) | 0xC080;
  if (u < 0x10000) return ((u << 4) & 0x0F0000) | ((u << 2) & 0x003F00) | (u & 0x3F) | 0xE08080;
  if (u < 0x110000)
    return ((u << 6) & 0x07000000) | ((u << 4) & 0x003F0000) | ((u << 2) & 0x3F00) | (u & 0x3F) |
           0xF0808080u;
  return 0;
}
CS_HD unsigned packed_to_cp(unsigned c) {
  if (c < 0x80) return c;
  if (c < 0xE000) return ((c & 0x1F00) >> 2) | (c & 0x3F);
  if (c < 0xF00000) return ((c & 0x0F0000) >> 4) | ((c & 0x3F00) >> 2) | (c & 0x3F);
  if (c <= 0xF8000000u)  // lead-byte mask 0x03, not 0x07: contract quirk (util.inl:67)
    return ((c & 0x03000000) >> 6) | ((c & 0x3F0000) >> 4) | ((c & 0x3F00) >> 2) | (c & 0x3F);
  return 0;
}
CS_HD int count_chars(const uint8_t* p, int n) {
  int k = 0;
  for (int i = 0; i < n; ++i) k += !is_cont(p[i]);
  return k;
}
// byte offset of character position `chpos` (clamped to n)
CS_HD int byte_of_char(const uint8_t* p, int n, int chpos) {
  int i = 0;
  while (chpos > 0 && i < n) {
    unsigned w = lead_width(p[i]);
    i += w ? (int)w : 1;
    chpos -= w != 0;
  }
  return i < n ? i : n;
}
// advance `k` characters from byte offset i
CS_HD int skip_chars(const uint8_t* p, int n, int i, int k) {
  while (k > 0 && i < n) {
    unsigned w = lead_width(p[i]);
    i += w ? (int)w : 1;
    k -= w != 0;
  }
  return i < n ? i : n;
}

// first byte offset m in [from, to - nb] with p[m..m+nb) == needle; -1 if none
CS_HD int find_bytes(const uint8_t* p, int from, int to, const uint8_t* needle, int nb) {
  for (int m = from; m + nb <= to; ++m) {
    int j = 0;
    while (j < nb && p[m + j] == needle[j]) ++j;
    if (j == nb) return m;
  }
  return -1;
}

// ---- find: char-position window in, char position out -----------------------
// byte offset of character position `chpos` by the reference's table of widths (custring_view.inl:261-281): 0 for position
// 0, the size from the character count on, position k for a row with as many characters as bytes, else the widths the
// first chpos lead bytes ANNOUNCE, added up -- whatever stands behind a lead byte.  On well-formed rows that is the
// character's offset.  (A sum beyond the row: the reference compares what lies behind the row; here the row ends.)
CS_HD int window_byte(const uint8_t* p, int n, int nchars, int chpos) {
  if (chpos <= 0) return 0;
  if (chpos >= nchars) return n;
  if (nchars == n) return chpos;
  int off = 0;
  for (int i = 0; chpos > 0 && i < n; ++i) {
    const unsigned w = lead_width(p[i]);
    off += (int)w;
    chpos -= w != 0;
  }
  return off < n ? off : n;
}
// a row of continuation bytes alone has no character: the reference's window over it is [0, 0) (custring_view.inl:486-495)
CS_HD bool no_chars_before(const uint8_t* p, int n, int m) {
  return is_cont(p[0]) && count_chars(p, m) == 0 && count_chars(p + m, n - m) == 0;
}
CS_HD int row_find(const uint8_t* p, int n, const uint8_t* needle, int nb, int start, int end) {
  if (nb == 0) return -1;  // an empty needle never matches
  if (start < 0) start = 0;
  // the reference turns (start,end) into a count: end - start, negative = rest
  const int count = end - start;
  int lo = 0, hi = n;
  if (start > 0 || count >= 0) {
    const int nchars = count_chars(p, n);
    const int last = (count >= 0 && start <= nchars && count < nchars - start) ? start + count : nchars;
    lo = window_byte(p, n, nchars, start);
    hi = window_byte(p, n, nchars, last);
  }
  int m = find_bytes(p, lo, hi, needle, nb);
  if (m < 0 || no_chars_before(p, n, m)) return -1;
  return count_chars(p, m);
}
// contains(str) by bytes: the reference's find over the whole row (find.cu:237-272), so nothing in a row without a character
CS_HD bool row_contains(const uint8_t* p, int n, const uint8_t* needle, int nb) {
  if (nb == 0) return false;
  const int m = find_bytes(p, 0, n, needle, nb);
  return m >= 0 && !no_chars_before(p, n, m);
}

// ---- the rest of the find family (find.cu:36-72, 123-236, 276-387; custring_view.inl:434-442, 481-515, 550-582, 1673-1703) ----
// byte offset of character position `chpos` as custring_view::offset_for_char_pos has it: 0 for 0, the size from the
// character count on (the position is UNSIGNED there: a negative argument is past the end)
CS_HD int offset_for_char_pos(const uint8_t* p, int n, int nchars, unsigned chpos) {
  if (chpos == 0) return 0;
  if (chpos >= (unsigned)nchars) return n;
  return byte_of_char(p, n, (int)chpos);
}
// custring_view::find(str, bytes, pos, count): the window is [pos, pos + count) in characters, count < 0 = the rest
CS_HD int row_find_count(const uint8_t* p, int n, const uint8_t* needle, int nb, unsigned pos, int count) {
  if (nb == 0) return -1;
  const int nchars = count_chars(p, n);
  if (count < 0) count = nchars;
  int end = (int)pos + count;
  if (end < 0 || end > nchars) end = nchars;
  const int spos = offset_for_char_pos(p, n, nchars, pos), epos = offset_for_char_pos(p, n, nchars, (unsigned)end);
  const int m = find_bytes(p, spos, epos, needle, nb);  // (an empty or inverted window: no start fits)
  return m < 0 ? -1 : count_chars(p, m);
}
// custring_view::rfind(str, bytes, pos, count): the LAST occurrence inside the window; the count is taken as it comes
// (a negative one moves the window's end in front of its start unless the sum is negative too)
CS_HD int row_rfind_count(const uint8_t* p, int n, const uint8_t* needle, int nb, unsigned pos, int count) {
  if (nb == 0) return -1;
  const int nchars = count_chars(p, n);
  int end = (int)pos + count;
  if (end < 0 || end > nchars) end = nchars;
  const int spos = offset_for_char_pos(p, n, nchars, pos), epos = offset_for_char_pos(p, n, nchars, (unsigned)end);
  for (int m = epos - nb; m >= spos; --m) {
    int j = 0;
    while (j < nb && p[m + j] == needle[j]) ++j;
    if (j == nb) return count_chars(p, m);
  }
  return -1;
}
// custr::compare (custring.inl:240-261): the difference of the first bytes that differ, else +1 / -1 for the longer side
CS_HD int row_compare(const uint8_t* p, int n, const uint8_t* q, int m) {
  int i = 0;
  for (; i < n && i < m; ++i)
    if (p[i] != q[i]) return (int)p[i] - (int)q[i];
  if (i < n) return 1;
  if (i < m) return -1;
  return 0;
}
CS_HD bool row_starts_with(const uint8_t* p, int n, const uint8_t* q, int m) {
  if (m > n) return false;
  for (int i = 0; i < m; ++i)
    if (p[i] != q[i]) return false;
  return true;
}
CS_HD bool row_ends_with(const uint8_t* p, int n, const uint8_t* q, int m) {
  if (m > n) return false;
  for (int i = 0; i < m; ++i)
    if (p[n - m + i] != q[i]) return false;
  return true;
}

// ---- replace -------------------------------------------------------------------
// maxrepl < 0: unlimited (the reference's cap, nchars, can never bind)
CS_HD int row_replace_size(const uint8_t* p, int n, const uint8_t* needle, int nb, int rb,
                           int maxrepl) {
  int out = n, from = 0;
  for (int left = maxrepl; left != 0; --left) {
    int m = find_bytes(p, from, n, needle, nb);
    if (m < 0) break;
    out += rb - nb;
    from = m + nb;
  }
  return out;
}
CS_HD void row_replace_write(const uint8_t* p, int n, const uint8_t* needle, int nb,
                             const uint8_t* repl, int rb, int maxrepl, uint8_t* o) {
  int from = 0;
  for (int left = maxrepl; left != 0; --left) {
    int m = find_bytes(p, from, n, needle, nb);
    if (m < 0) break;
    for (int i = from; i < m; ++i) *o++ = p[i];
    for (int i = 0; i < rb; ++i) *o++ = repl[i];
    from = m + nb;
  }
  for (int i = from; i < n; ++i) *o++ = p[i];
}

// ---- strip ---------------------------------------------------------------------
struct CharSet {  // a set of characters of any size (custring_view.inl:93-105 walks the caller's string, whatever its length)
  Char c[64];        // the members -- of a set of more than 64 characters: its first 64 non-ASCII members
  int n;             // members in c[]
  uint32_t ascii[4]; // the set's ASCII members as a bitmap (charset_finish): one bit test instead of a walk over c[]
  int wide;          // more than 64 characters: the ASCII members are in the bitmap ONLY, non-ASCII ones beyond c[] in `more`
  const Char* more;  // sorted ascending (device memory in kernels, host memory in the host emulation)
  int nmore;
};
// call once the members are in c[0 .. n)
CS_HD void charset_finish(CharSet& s) {
  s.ascii[0] = s.ascii[1] = s.ascii[2] = s.ascii[3] = 0;
  s.wide = 0;
  s.more = nullptr;
  s.nmore = 0;
  for (int i = 0; i < s.n; ++i)
    if (s.c[i] < 128u) s.ascii[s.c[i] >> 5] |= 1u << (s.c[i] & 31u);
}
CS_HD bool in_set(const CharSet& s, Char ch) {
  if ((s.n > 4 || s.wide) && ch < 128u) {  // (a handful of members: the walk below is cheaper than the word select)
    const unsigned k = ch >> 5;
    const uint32_t w = k == 0 ? s.ascii[0] : (k == 1 ? s.ascii[1] : (k == 2 ? s.ascii[2] : s.ascii[3]));
    return ((w >> (ch & 31u)) & 1u) != 0;
  }
  for (int i = 0; i < s.n; ++i)
    if (s.c[i] == ch) return true;
  int lo = 0, hi = s.nmore;  // (sets beyond 64 non-ASCII characters)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const Char m = s.more[mid];
    if (m == ch) return true;
    if (m < ch) lo = mid + 1;
    else hi = mid;
  }
  return false;
}
// Host: the set of the characters of the UTF-8 string `s` (n bytes).  Up to 64 characters: all of them in c[], as ever.
// Beyond: ASCII members in the bitmap, the first 64 non-ASCII ones in c[], the others sorted into `overflow` -- the caller
// puts them where the kernels can read them and sets `more` / `nmore`.
template <class Vec>
inline CharSet charset_from_utf8(const uint8_t* s, int n, Vec& overflow) {
  CharSet cs;
  cs.n = 0;
  overflow.clear();
  int count = 0;
  for (int i = 0; i < n; ++count) {
    Char c;
    const unsigned w = decode_at(s, i, n, c);
    i += w ? (int)w : 1;
  }
  if (count <= 64) {
    for (int i = 0; i < n;) {
      Char c;
      const unsigned w = decode_at(s, i, n, c);
      cs.c[cs.n++] = c;
      i += w ? (int)w : 1;
    }
    charset_finish(cs);
    return cs;
  }
  uint32_t bits[4] = {0, 0, 0, 0};
  for (int i = 0; i < n;) {
    Char c;
    const unsigned w = decode_at(s, i, n, c);
    i += w ? (int)w : 1;
    if (c < 128u) {
      bits[c >> 5] |= 1u << (c & 31u);
      continue;
    }
    bool seen = false;
    for (int k = 0; k < cs.n && !seen; ++k) seen = cs.c[k] == c;
    if (seen) continue;
    if (cs.n < 64) cs.c[cs.n++] = c;
    else overflow.push_back(c);
  }
  charset_finish(cs);
  for (int k = 0; k < 4; ++k) cs.ascii[k] = bits[k];
  cs.wide = 1;
  for (int a = 1; a < (int)overflow.size(); ++a)  // (insertion sort: a few characters)
    for (int b = a; b > 0 && overflow[b - 1] > overflow[b]; --b) {
      const Char t = overflow[b - 1];
      overflow[b - 1] = overflow[b];
      overflow[b] = t;
    }
  return cs;
}
// side: 0 both, 1 left, 2 right.  Returns [lo,hi) of the kept bytes.
CS_HD void row_strip(const uint8_t* p, int n, const CharSet& set, int side, int& lo, int& hi) {
  lo = 0;
  hi = n;
  if (side != 2) {
    while (lo < n) {
      Char ch;
      unsigned w = decode_at(p, lo, n, ch);
      if (!in_set(set, ch)) break;
      lo += w ? (int)w : 1;
    }
    if (lo >= n) {
      lo = hi = n;
      return;
    }
  }
  if (side != 1) {
    // The reference steps back to the byte in front that is no continuation byte and takes the WIDTH of the member it
    // decodes there off the row's end (custring_view.inl:1426-1437, 1560-1571), a step for every character at the most: on a
    // well-formed row the walk and the end move together; stray continuation bytes behind a member are walked over but stay
    // counted as kept, and a walk that meets the stripped left end takes the row (lead + trail > size: :1439).
    int q = n;
    for (;;) {
      int k = q - 1;
      while (k >= 0 && is_cont(p[k])) --k;
      if (k < 0) break;
      Char ch;
      const unsigned w = decode_at(p, k, n, ch);
      if (!in_set(set, ch)) break;
      q = k;
      hi -= (int)w;
    }
    if (hi < lo) lo = hi = n;
  }
}

// ---- lower / upper -------------------------------------------------------------
// flag bit 32 = upper (lower() maps these), 64 = lower (upper() maps these)
// The reference walks a row with its character iterator (case.cu:49,81; custring_view.inl:361-392): one step for every byte
// that is no continuation byte, each step decoding at the iterator's offset and advancing it by the width the byte there
// implies.  On well-formed rows that is one step a character.  On any other row it is restated as it stands: a stray
// continuation byte has width 0, so every remaining step reads it again; a lead byte takes the bytes behind it whatever
// they are, and a step at or past the row's end reads the terminator (a zero byte of width 1).
template <class Emit>
CS_HD void row_case_walk(const uint8_t* p, int n, const uint8_t* flags, const uint16_t* cases, unsigned bit, Emit&& emit) {
  int i = 0;
  for (int left = count_chars(p, n); left > 0; --left) {
    if (i < n && p[i] < 0x80) {  // ASCII maps to ASCII
      const uint8_t b = p[i];
      emit((Char)((flags[b] & bit) ? (uint8_t)cases[b] : b), 1u);
      ++i;
      continue;
    }
    Char ch = 0;
    unsigned w = 1;
    if (i < n) w = decode_at(p, i, n, ch);
    unsigned u = packed_to_cp(ch);
    unsigned f = u <= 0xFFFF ? flags[u] : 0;
    if (f & bit) ch = cp_to_packed(cases[u]);
    emit(ch, packed_width(ch));
    i += (int)w;
  }
}
CS_HD int row_case_size(const uint8_t* p, int n, const uint8_t* flags, const uint16_t* cases,
                        unsigned bit) {
  int out = 0;
  row_case_walk(p, n, flags, cases, bit, [&](Char, unsigned ow) { out += (int)ow; });
  return out;
}
CS_HD void row_case_write(const uint8_t* p, int n, const uint8_t* flags, const uint16_t* cases,
                          unsigned bit, uint8_t* o) {
  row_case_walk(p, n, flags, cases, bit, [&](Char ch, unsigned ow) {
    for (unsigned k = 0; k < ow; ++k) *o++ = (uint8_t)(ch >> (8 * (ow - 1 - k)));
  });
}

// ---- split on a delimiter string -------------------------------------------------
// Token COUNT advances the search by `nb` CHARACTERS past the match start (the
// reference adds the delimiter's byte length to a character position,
// custring_view.inl:1243) while token EXTRACTION advances by the delimiter
// itself (split.cu:779-793).  They only differ for multi-byte delimiters.
CS_HD int row_split_count(const uint8_t* p, int n, const uint8_t* d, int nb, int tokens) {
  if (n == 0) return 1;
  int cnt = 1, from = 0;
  for (;;) {
    int m = find_bytes(p, from, n, d, nb);
    if (m < 0) break;
    ++cnt;
    from = skip_chars(p, n, m, nb);
  }
  if (tokens > 0 && cnt > tokens) cnt = tokens;
  return cnt;
}
// Walks the row's `cnt` tokens in order; emit(k, lo, hi) for token k.
template <class Emit>
CS_HD void row_split_tokens(const uint8_t* p, int n, const uint8_t* d, int nb, int cnt,
                            Emit&& emit) {
  int lo = 0;
  for (int k = 0; k < cnt; ++k) {
    int hi = n;
    bool more = k + 1 < cnt;
    int m = more ? find_bytes(p, lo, n, d, nb) : -1;
    if (m >= 0) hi = m;
    emit(k, lo, hi);
    if (more && m < 0) {  // counted more tokens than there are delimiters left
      for (int j = k + 1; j < cnt; ++j) emit(j, lo, n);
      return;
    }
    lo = m + nb;
  }
}

// ---- split / tokenize on whitespace (byte <= ' ') ---------------------------------
CS_HD int row_ws_count(const uint8_t* p, int n) {
  int cnt = 0;
  bool in_tok = false;
  for (int i = 0; i < n; ++i) {
    bool sp = p[i] <= 0x20;
    cnt += (!sp && !in_tok);
    in_tok = !sp;
  }
  return cnt;
}
// split(None,n) column count for a row: natural tokens capped by `tokens`,
// at least 1 (split.cu:52-87)
CS_HD int row_wssplit_count(const uint8_t* p, int n, int tokens) {
  int cnt = row_ws_count(p, n);
  if (tokens > 0 && cnt > tokens) cnt = tokens;
  return cnt == 0 ? 1 : cnt;
}
// emit(k, lo, hi) for each of the row's natural whitespace tokens k < limit;
// when `tokens` > 0 the token with index tokens-1 runs to the end of the row.
template <class Emit>
CS_HD void row_ws_tokens(const uint8_t* p, int n, int tokens, Emit&& emit) {
  int k = 0, i = 0;
  while (i < n) {
    while (i < n && p[i] <= 0x20) ++i;
    if (i >= n) break;
    int lo = i;
    if (tokens > 0 && k == tokens - 1) {
      emit(k, lo, n);
      return;
    }
    while (i < n && p[i] > 0x20) ++i;
    emit(k, lo, i);
    ++k;
  }
}

// ---- rsplit (split.cu:960-1148): the forward token COUNT, tokens located from the right ----
CS_HD int rfind_bytes(const uint8_t* p, int to, const uint8_t* needle, int nb) {  // last occurrence inside [0, to)
  for (int m = to - nb; m >= 0; --m) {
    int j = 0;
    while (j < nb && p[m + j] == needle[j]) ++j;
    if (j == nb) return m;
  }
  return -1;
}
// emit(k, lo, hi) for every column k < cnt (empty tokens included); one walk from the right:
// token k runs from behind the k-th delimiter found from the right to the previous one; when
// the delimiters run out early every remaining column repeats [0, hi) (split.cu:1006-1021)
template <class Emit>
CS_HD void row_rsplit_tokens(const uint8_t* p, int n, const uint8_t* d, int nb, int cnt, Emit&& emit) {
  int hi = n;
  for (int k = cnt - 1; k > 0; --k) {
    const int m = rfind_bytes(p, hi, d, nb);
    if (m < 0) {
      for (int j = k; j > 0; --j) emit(j, 0, hi);
      break;
    }
    emit(k, m + nb, m + nb < hi ? hi : m + nb);
    hi = m;
  }
  emit(0, 0, hi);
}
// Whitespace rsplit, column `col` of a row holding `cnt` columns (split.cu:1098-1124 restated on
// bytes: every byte of a multi-byte character is above ' ').  `ncols` is the column count of the
// whole call, which the reference compares with `tokens`.  false = null in this column.
CS_HD bool row_ws_rtoken(const uint8_t* p, int n, int tokens, int cnt, int ncols, int col, int& lo, int& hi) {
  int c = cnt - 1, spos = 0, epos = n;
  bool spaces = true;
  for (int pos = n; pos > 0; --pos) {
    const bool sp = p[pos - 1] <= 0x20;
    if (spaces == sp) {
      if (spaces) epos = pos - 1;
      else spos = pos - 1;
      continue;
    }
    if (!spaces) {
      spos = 0;
      if (ncols - c == tokens) break;
      spos = pos;
      if (c == col) break;
      epos = pos - 1;
      spos = 0;
      --c;
    }
    spaces = !spaces;
  }
  lo = spos;
  hi = epos;
  return spos < epos;
}

// ---- tokenize on a set of delimiter characters -------------------------------------
template <class Emit>
CS_HD int row_set_tokens(const uint8_t* p, int n, const CharSet& set, Emit&& emit) {
  int k = 0, i = 0;
  while (i < n) {
    Char ch;
    unsigned w = 1;
    // skip delimiters
    while (i < n) {
      w = decode_at(p, i, n, ch);
      if (w == 0) w = 1;
      if (!in_set(set, ch)) break;
      i += (int)w;
    }
    if (i >= n) break;
    int lo = i;
    while (i < n) {
      w = decode_at(p, i, n, ch);
      if (w == 0) w = 1;
      if (in_set(set, ch)) break;
      i += (int)w;
    }
    emit(k, lo, i < n ? i : n);
    ++k;
  }
  return k;
}

// ---- NVText::tokenize: the reference's walk of one row (tokens.cu:41-121) -------------------------
// The delimiters of tokenize(): whitespace (use_set 0: a character <= ' '), or the characters of the
// delimiter string.  The reference looks a character up with custring_view::find(Char), which decodes
// the delimiter string at EVERY byte offset: a continuation byte of a member is found too, so a stray
// byte 10xxxxxx of a row is a delimiter when a member holds the same byte (`cont`: one bit a byte
// 0x80..0xBF); the character 0 is never found.
struct TokDelims {
  CharSet set;
  int use_set;    // 0 = whitespace
  uint64_t cont;  // the continuation bytes of the set's members
};
CS_HD void tokdelims_finish(TokDelims& d, const uint8_t* delim, int nb) {  // (d.set, d.use_set are the caller's)
  d.cont = 0;
  for (int i = 0; i < nb; ++i)
    if (is_cont(delim[i])) d.cont |= 1ull << (delim[i] - 0x80u);
}
CS_HD bool is_tok_delim(const TokDelims& d, Char ch) {
  if (!d.use_set) return ch <= 0x20u;
  if (ch == 0) return false;
  if (ch - 0x80u < 64u) return ((d.cont >> (ch - 0x80u)) & 1u) != 0;
  return in_set(d.set, ch);
}
// emit(k, lo, hi) for the row's tokens in order; returns their number.  On well-formed UTF-8 this is
// the walk over bytes of row_ws_tokens / row_set_tokens.  On other rows the reference's own steps
// decide, and they are restated here:
//   * the row has as many characters as it has bytes that are no continuation bytes (chars_count);
//   * the iterator stands at a byte offset and moves on by the width THE BYTE UNDER IT announces
//     (custring_view.inl:361): over bytes that are no continuation bytes when a lead byte announced
//     them, and not at all from a stray continuation byte, which it then reads once for every
//     character the row has left;
//   * a token's character positions become byte offsets by the sum of the widths that the row's first
//     k lead bytes announce (byte_offset_for, :261; position k of a row with as many characters as
//     bytes is byte k, a position at or beyond the row's characters is the row's size).
// Where the reference reads behind the row its result is undefined; here the byte at the row's size and
// every byte behind it reads as 0 (the reference has its terminator there), a token ends at the row's
// end at the latest, and a token that would begin there is dropped.
template <class Emit>
CS_HD int row_tok_walk(const uint8_t* p, int n, const TokDelims& d, Emit&& emit) {
  int nch = 0;
  for (int i = 0; i < n; ++i) nch += !is_cont(p[i]);
  int scan = 0, seen = 0, sum = 0;  // byte_offset_for, asked with rising positions: one pass over the row
  auto byte_of = [&](int k) {
    if (k >= nch) return n;
    if (nch == n) return k;
    while (seen < k) {
      const unsigned w = lead_width(p[scan++]);
      if (w) sum += (int)w, ++seen;
    }
    return sum < n ? sum : n;
  };
  int spos = 0, epos = nch, off = 0, cpos = 0, k = 0;
  bool spaces = true;
  while (spos < nch) {
    for (; cpos != nch; ++cpos) {
      Char ch = 0;
      unsigned w = 1;
      if (off < n) w = decode_at(p, off, n, ch);  // (a continuation byte: itself, width 0)
      if (spaces == is_tok_delim(d, ch)) {
        if (spaces) spos = cpos + 1;
        else epos = cpos + 1;
      } else {
        spaces = !spaces;
        if (spaces) {
          epos = cpos;
          break;
        }
      }
      off += (int)w;
    }
    if (!(spos < epos)) break;
    const int lo = byte_of(spos), hi = byte_of(epos);
    if (lo < hi) emit(k++, lo, hi);
    spos = epos + 1;
    epos = nch;
    off += off < n ? (int)lead_width(p[off]) : 1;  // (the reference's ++itr behind a token)
    ++cpos;
  }
  return k;
}

}  // namespace csrow
