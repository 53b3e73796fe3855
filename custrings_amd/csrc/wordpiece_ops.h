// Per-word and per-row logic of WordPiece tokenization: a strings column to the integer ids of a vocabulary.  Shared by
// the kernels of cs_wordpiece.hip and the g++ harness of tests/wordpiece_model.py, which restates it independently in Python.
//
// Vocabulary: a strings column; the row index is the id (int32).  Null rows and empty rows are no entry; among equal rows
//   the lowest index wins.  `prefix` is the continuation prefix (default "##", 1..8 bytes), `unk` the unknown token (default
//   "[UNK]"), which must be an entry.  Entries have at most 255 bytes; at most 2^24 rows; 1 <= max_word_chars <= 1024.
// Characters: a character starts at every byte that is no continuation byte (10xxxxxx) -- the rule of cs_len and of
//   minhash_ops.h (char_start) --, and the continuation bytes behind a start belong to it, so malformed bytes are well
//   defined.  Continuation bytes at the very front of a word have no start in the word: they go with its first character
//   (such a word has one character at least, and its first piece starts at its first byte).
// Words of a row: the maximal runs of bytes > 0x20 (tokenize's whitespace rule, row_ops.h row_ws_tokens).  With punct = 1
//   every ASCII punctuation byte (33-47, 58-64, 91-96, 123-126) is also a word of its own and ends the word on either side
//   of it.  A null row has no words.
// Pieces of a word, greedy, longest match first: a word of more than max_word_chars characters gives the single id unk.
//   Otherwise start at character s = 0; take the longest run of whole characters [s, e) whose bytes -- for s > 0: `prefix`
//   followed by them -- are an entry; emit its id, go on at s = e until the word is used up.  If at some s no run matches,
//   the whole word gives the single id unk: the ids already emitted for it are dropped.
// Row result: the ids of its words, in order.
//
// The table: open addressing over a power of two of 16-byte slots, load <= 0.5, keyed by (continuation flag, the bytes BEHIND
//   the prefix), so that a lookup hashes the row's own bytes only.  An entry that starts with the prefix and is longer than
//   it therefore goes in twice: whole with flag 0 (the word "##ab" finds the entry "##ab" at s = 0) and stripped with flag 1
//   (the same entry as the continuation "ab" at s > 0); an entry equal to the prefix goes in once, whole.  The hash is the
//   murmur of minhash_ops.h, seeded by the flag.  A key's bytes stay in the vocabulary's chars: the slot holds their place.
// The matcher walks FORWARD from s, one incremental murmur over the bytes, probes at every character boundary and keeps the
//   last hit: longest first in one pass, bounded by the longest key of that flag.
#pragma once
#include <stdint.h>

#include "minhash_ops.h"

namespace cswp {

constexpr int kMaxPrefix = 8;
constexpr int kMaxEntryBytes = 255;
constexpr int64_t kMaxEntries = (int64_t)1 << 24;
constexpr int kMaxWordChars = 1024;
CS_HD uint32_t key_seed(int flag) { return flag ? 0x2323u : 0x5770u; }  // whole keys, continuation keys

// key: 0 = empty, else 1 + (row << 1 | flag) of the vocabulary row that CLAIMED the slot (an equal key of a lower row lowers
// the id, not this).  len_id: the key's bytes << 24 | the lowest row with this key (all ones until the first insert lands).
// hash, off: the key's murmur and where its bytes start in the vocabulary's chars -- written by the claimer, read by lookups.
struct alignas(16) Slot {
  uint32_t key, len_id, hash, off;
};
constexpr uint32_t kNoId = 0xFFFFFFFFu;

struct Prefix {
  uint8_t b[kMaxPrefix];
  int n;
};

// what a lookup needs (by value to the kernels)
struct Table {
  const Slot* slots;
  const uint8_t* chars;  // the vocabulary's
  uint32_t mask;         // slots - 1
  int max_key[2];        // the longest key of either flag, bytes
  int32_t unk;
};

// slots for `rows` vocabulary rows, each of which may go in twice: load <= 0.5
CS_HD int64_t slots_for(int64_t rows) {
  int64_t n = 16;
  while (n < 4 * rows) n <<= 1;
  return n;
}

CS_HD bool is_punct(uint8_t c) { return (c >= 33 && c <= 47) || (c >= 58 && c <= 64) || (c >= 91 && c <= 96) || (c >= 123 && c <= 126); }
CS_HD bool bytes_equal(const uint8_t* a, const uint8_t* b, int n) {
  for (int i = 0; i < n; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

// ---- insert ------------------------------------------------------------------------------------------------------------------
// The atomics of an insert: the kernels' (device atomics: rows insert side by side) and the harness's (one row after the other).
struct PlainAtomics {
  static inline uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) {
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
  }
  static inline void lower(uint32_t* p, uint32_t v) {
    if (v < *p) *p = v;
  }
};
// the key bytes of the row behind a slot's `key`: its whole row, or what follows the prefix
struct KeyBytes {
  int64_t off;
  int len;
};
CS_HD KeyBytes key_bytes_of(uint32_t key, const int64_t* offsets, int plen) {
  const uint32_t rf = key - 1;
  const int64_t o = offsets[rf >> 1];
  const int skip = (rf & 1u) ? plen : 0;
  return KeyBytes{o + skip, (int)(offsets[(rf >> 1) + 1] - o) - skip};
}
// One key of row `row`, chars[off, off + len), flag 0 or 1.  Returns 1: it claimed a slot (a key nobody had), 0: an equal
// key was there, -1: no slot in `mask + 1` probes (cannot happen at load <= 0.5).  Slots start as {0, kNoId, 0, 0}.
template <class A>
CS_HD int insert_key(Slot* slots, uint32_t mask, const uint8_t* chars, const int64_t* offsets, int plen, int64_t off, int len, int flag, int32_t row) {
  const uint32_t h = csmh::murmur3_32(chars + off, len, key_seed(flag));
  const uint32_t mine = 1u + (((uint32_t)row << 1) | (uint32_t)flag), len_id = ((uint32_t)len << 24) | (uint32_t)row;
  uint32_t i = h & mask;
  for (uint32_t step = 0; step <= mask; ++step, i = (i + 1) & mask) {
    Slot* s = slots + i;
    const uint32_t was = A::cas(&s->key, 0u, mine);
    if (was == 0u) {
      s->hash = h;
      s->off = (uint32_t)off;
      A::lower(&s->len_id, len_id);
      return 1;
    }
    // (the claimer's hash and off may not have landed: its row says what its key is)
    const KeyBytes k = key_bytes_of(was, offsets, plen);
    if (((was - 1) & 1u) == (uint32_t)flag && k.len == len && bytes_equal(chars + k.off, chars + off, len)) {
      A::lower(&s->len_id, len_id);
      return 0;
    }
  }
  return -1;
}
// What one vocabulary row puts in.  Returns 1 when the row is a new entry (its whole key claimed a slot), 0 when it is no
// entry or an equal one was there, -1 when the table is full.
template <class A>
CS_HD int insert_row(Slot* slots, uint32_t mask, const uint8_t* chars, const int64_t* offsets, const Prefix& px, int32_t row, bool valid) {
  const int64_t off = offsets[row];
  const int len = valid ? (int)(offsets[row + 1] - off) : 0;
  if (len <= 0 || len > kMaxEntryBytes) return 0;
  const int whole = insert_key<A>(slots, mask, chars, offsets, px.n, off, len, 0, row);
  if (whole < 0) return -1;
  if (len > px.n && bytes_equal(chars + off, px.b, px.n) && insert_key<A>(slots, mask, chars, offsets, px.n, off + px.n, len - px.n, 1, row) < 0) return -1;
  return whole;
}

// ---- probe -------------------------------------------------------------------------------------------------------------------
// the id of the key (flag, p[0, len)) whose murmur is h; -1: no such key
CS_HD int32_t probe(const Table& t, int flag, uint32_t h, const uint8_t* p, int len) {
  uint32_t i = h & t.mask;
  for (uint32_t step = 0; step <= t.mask; ++step, i = (i + 1) & t.mask) {
    const Slot s = t.slots[i];
    if (s.key == 0u) return -1;
    if (s.hash == h && ((s.key - 1) & 1u) == (uint32_t)flag && (int)(s.len_id >> 24) == len && bytes_equal(t.chars + s.off, p, len))
      return (int32_t)(s.len_id & 0xFFFFFFu);
  }
  return -1;
}
CS_HD int32_t find_key(const Table& t, int flag, const uint8_t* p, int len) {
  return len > 0 && len <= kMaxEntryBytes ? probe(t, flag, csmh::murmur3_32(p, len, key_seed(flag)), p, len) : -1;
}
// the id of the entry p[0, len), as the vocabulary lists it; -1: none
CS_HD int32_t find_entry(const Table& t, const uint8_t* p, int len) { return find_key(t, 0, p, len); }

// murmur3_32 a byte at a time: value() after n bytes is murmur3_32 of those n bytes
struct RunningMurmur {
  uint32_t h, k, n;
  CS_HD explicit RunningMurmur(uint32_t seed) : h(seed), k(0), n(0) {}
  CS_HD void add(uint8_t c) {
    k |= (uint32_t)c << (8 * (n & 3u));
    if ((++n & 3u) == 0) {
      h = csmh::murmur_block(h, k);
      k = 0;
    }
  }
  CS_HD uint32_t value() const { return csmh::murmur_finish(h, k, n); }
};

// ---- words ---------------------------------------------------------------------------------------------------------------------
// a word starts at p[i]: a punctuation byte under `punct`, else a byte > 0x20 with the row's front, a blank or (punct) a
// punctuation byte before it
CS_HD bool word_starts_at(const uint8_t* p, int i, int punct) {
  const uint8_t c = p[i];
  if (c <= 0x20) return false;
  if (punct && is_punct(c)) return true;
  if (i == 0) return true;
  const uint8_t b = p[i - 1];
  return b <= 0x20 || (punct && is_punct(b));
}
// the end of the word that starts at p[lo] (word_starts_at), and its characters
CS_HD int word_end(const uint8_t* p, int n, int lo, int punct, int& nch) {
  nch = 1;
  int i = lo + 1;
  if (punct && is_punct(p[lo])) return i;
  for (; i < n && p[i] > 0x20 && !(punct && is_punct(p[i])); ++i) nch += csmh::char_start(p[i]);
  return i;
}
// f(lo, hi, characters) for every word of the row, in order, while it returns true
template <class F>
CS_HD void for_each_word(const uint8_t* p, int n, int punct, F&& f) {
  int i = 0;
  while (i < n) {
    if (p[i] <= 0x20) {
      ++i;
      continue;
    }
    int nch;
    const int lo = i;
    i = word_end(p, n, lo, punct, nch);
    if (!f(lo, i, nch)) return;
  }
}

// ---- pieces ----------------------------------------------------------------------------------------------------------------------
struct NoOutput {  // the size pass
  CS_HD void operator()(int, int32_t) const {}
};
// The ids of the word w[0, len) of `nch` characters: out(k0 + j, id) for its j-th; returns their number.  A word that fails
// half way puts unk over its first id (what it had put behind that is beyond the count returned, and overwritten or unused).
template <class Out>
CS_HD int match_word(const Table& t, const uint8_t* w, int len, int nch, int max_word_chars, int k0, Out&& out) {
  if (nch > max_word_chars) {
    out(k0, t.unk);
    return 1;
  }
  int k = k0;
  for (int s = 0; s < len;) {
    const int flag = s > 0;
    const int lim = len - s < t.max_key[flag] ? len : s + t.max_key[flag];
    RunningMurmur m(key_seed(flag));
    int hit_e = -1;
    int32_t hit_id = -1;
    for (int e = s + 1; e <= lim; ++e) {
      m.add(w[e - 1]);
      if (e < len && !csmh::char_start(w[e])) continue;
      const int32_t id = probe(t, flag, m.value(), w + s, e - s);
      if (id >= 0) {
        hit_e = e;
        hit_id = id;
      }
    }
    if (hit_e < 0) {
      out(k0, t.unk);
      return 1;
    }
    out(k++, hit_id);
    s = hit_e;
  }
  return k - k0;
}
// the ids of a row: out(k, id), k = 0, 1, ...; stops behind the word that reaches `limit` ids (what lies beyond it the
// caller does not want); returns the ids put, which may exceed `limit` by that word's
template <class Out>
CS_HD int row_ids(const Table& t, const uint8_t* p, int n, int max_word_chars, int punct, int limit, Out&& out) {
  int k = 0;
  for_each_word(p, n, punct, [&](int lo, int hi, int nch) {
    k += match_word(t, p + lo, hi - lo, nch, max_word_chars, k, out);
    return k < limit;
  });
  return k;
}

// ---- encode: a row of max_length ids -------------------------------------------------------------------------------------------
struct Specials {
  int32_t cls, sep, pad;  // cls / sep negative: none
  int max_length;
  CS_HD int front() const { return cls >= 0; }
  CS_HD int room() const { return max_length - (cls >= 0) - (sep >= 0); }  // ids of the row itself at most
};
// what stands at position j of a row whose own ids are cut to `kept` (<= room()), when it is none of them; mask: j < used(kept)
CS_HD int used(const Specials& sp, int kept) { return sp.front() + kept + (sp.sep >= 0); }
CS_HD int32_t filler(const Specials& sp, int kept, int j) {
  if (j == 0 && sp.cls >= 0) return sp.cls;
  if (sp.sep >= 0 && j == sp.front() + kept) return sp.sep;
  return sp.pad;
}

}  // namespace cswp
