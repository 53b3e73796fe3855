// The compiled pattern: cs_regex_compile with its cache of kept patterns and the handle's other entries, the upload of
// its images, and what the regex units (cs_regex_scan.hip, cs_regex.hip) ask about a pattern
// and a column before they launch -- which executor, which launch plan, which tile, which route (regex_exec.h declares
// them).  No kernel lives here.
#include <hip/hip_runtime.h>

#include <list>
#include <mutex>

#include "cs_internal.h"
#include "regex_exec.h"
#include "regex_stream.h"

using namespace cs;
using namespace csdev;
using namespace cs::rx;

namespace cs {
namespace rx {

// the tagged DFA with at most four live threads: every DFA kernel (lean scans, unit decomposition, capture groups)
bool use_tdfa(const cs_regex* re) { return !re->tdfa.empty() && re->tdfa[12] <= cstd::kMaxSlots && !cs::cfg("CS_REGEX_NO_TDFA"); }
// ... with five to eight (counted repetitions): contains_re / match / count_re and replace_re run it on the generic executor
// with eight start offsets (regex_tdfa.h: TdfaWide); the other ops keep the list simulator for such programs
bool use_tdfa_wide(const cs_regex* re) { return !re->tdfa.empty() && re->tdfa[12] > cstd::kMaxSlots && !cs::cfg("CS_REGEX_NO_TDFA"); }
// The bit-parallel form (regex_bits.h) is taken when the pattern has one, is no chain (chains run on two SWAR-classified
// bitmaps, cheaper than the class-table lookup), the column's sample is plain ASCII, and the automaton's candidate bytes --
// the bytes at which its idle skip has to stop -- make up a good part of the column's sample: with few candidates the lean
// scans skip most of every row and win; with candidates everywhere (alternations of word-bounded literals, small sets in
// a `+` loop) they walk every byte in a dependent chain of table reads (VERDICT r4 missing #3: 8.9 / 21.4 ms on C3).
// Thresholds from tools/probe_bits.py on the C3 column (profiles/r05/probe_bits.txt): share of candidate bytes -> bits / automaton ms
//   contains_re: 86.6 % ([^ ]+) 2.15 / 1.82 (a match at once: the first-match scan wins), 11.9 % ([aeiou]+) 2.2 / 4.4, 7.2 % (the
//   gtest pattern) 3.9 / 8.9, 2.4 % with three live threads (cat|cot|cut) 3.3 / 5.3, 2.4-2.6 % with one 2.3-2.7 / 2.5-2.7, below 1 % 2.3-3.3 / 1.4-2.9
//   count_re:    from 2 % up the bit form wins or ties (1.9 / 41.6 at 11.9 %, 2.5 / 4.1 at 2.4 %), below 1 % it loses (2.2 / 1.6)
//   replace_re:  (two workgroups a CU against three) 7.3 / 21.4 at 7.2 %, 8.6 / 51.7 at 11.9 %, 6.4 / 9.3 at 2.4 % with three threads;
//   5.4-5.8 / 4.6-4.9 at 2.4 % with one thread
// the share of the column's sampled bytes at which the automaton's idle skip has to stop
double candidate_share(const cs_regex* re, const cs_column* col, hipStream_t s) {
  if (re->tdfa.empty()) return 1.0;
  const uint32_t* hist = sample_byte_hist(col, s);
  uint64_t all = 0, cand = 0;
  for (unsigned c = 0; c < 256; ++c) {
    all += hist[c];
    if (c < 128 && (((uint32_t)re->tdfa[21 + (c >> 5)] >> (c & 31)) & 1u)) cand += hist[c];
  }
  return all ? (double)cand / (double)all : 0.0;
}
// Rows with a byte >= 0x80 or a NUL, by the column's sample: are they few enough (at most about one row in thirty -- an upper
// bound: every lead byte and every NUL counted as a row of its own) for a scan to put them off (ScanStreamArgs::deferred) and run
// as on plain ASCII?  (Measured on the C2 column, one row in twenty: the bit form's ops gain -- gtest contains_re 1.08 -> 0.57 ms,
// replace_re 2.31 -> 1.56 --, but a pattern whose generic scan is slow pays more for its rows on the list, a thread each, than the
// sub-tiles cost row by row: `[a-z]+ing\b` replace_re 3.9 -> 5.6, `\d+` 0.72 -> 1.35.  At one row in 170 -- C5 -- everything gains.)
bool odd_rows_few(const cs_column* col, hipStream_t s) {
  if (cs::cfg("CS_NO_DEFERRED_ROWS") || col->rows == 0) return false;
  const uint32_t* hist = sample_byte_hist(col, s);
  uint64_t all = 0, oddb = hist[0];
  for (unsigned c = 0; c < 256; ++c) {
    all += hist[c];
    if (c >= 0xC0) oddb += hist[c];  // (one lead byte a character; a stray continuation byte has no lead in front of it -- rare enough not to matter for a hint)
  }
  if (all == 0) return false;
  return (double)oddb / (double)all * ((double)col->nbytes / (double)col->rows) <= cs::cfg_int("CS_ODD_ROWS_PERMILLE", 30) / 1000.0;
}
bool bits_route(const cs_regex* re, const cs_column* col, hipStream_t s, int op, bool high_ok) {
  if (re->bits.empty() || cs::cfg("CS_NO_BITS_FORM")) return false;
  if (!re->tdfa.empty() && ((re->tdfa[30] >> 16) & 15) != 0) return false;  // a chain
  if (sample_has_high_bytes(col, s) && !high_ok) return false;
  if (cs::cfg("CS_BITS_ALWAYS")) return true;
  if (re->tdfa.empty()) return true;  // (no automaton: the list simulator is the alternative)
  const uint32_t* hist = sample_byte_hist(col, s);
  uint64_t all = 0, cand = 0;
  for (unsigned c = 0; c < 128; ++c) {
    all += hist[c];
    if (((uint32_t)re->tdfa[21 + (c >> 5)] >> (c & 31)) & 1u) cand += hist[c];
  }
  if (cs::cfg("CS_STREAM_INFO"))
    fprintf(stderr, "bits route: candidates %.2f %% of the sample (%d classes, %d alternatives, %d states, %d threads)\n", all ? 100.0 * (double)cand / (double)all : 0.0,
            re->bits[1], re->bits[3], re->tdfa[1], re->tdfa[12]);
  if (all == 0) return false;
  const double f = (double)cand / (double)all;
  const bool threads3 = re->tdfa[12] >= 3;
  if (op == BITS_COUNT) return f >= 0.02;
  // (the C5 column's pieces, the gtest pattern, 4.8 %: 4.0 / 7.1 -- the line between the 2.4 % tie and 7.2 % moved from 5 % to 3.5 %)
  // (candidates everywhere and assertions behind the `+` loop -- `[^ ]+$` --: the first-match scan does not "find a match at once",
  // it fails at every start: 8.4 ms on the C3 column against the bit form's 2.3)
  const bool tail = (re->bits[2] & csbits::F_TAIL) != 0;
  if (op == BITS_CONTAINS) return (f >= 0.035 && (f <= 0.5 || tail)) || (threads3 && f >= 0.02 && f <= 0.5);
  // (a pattern whose shortest match is one byte matches at most of its candidates: the automaton's routes then pay per match --
  // replace_re('e') on the C3 column, 4 % candidates: units 7.65, the bit form 6.45 ms)
  return f >= 0.05 || ((threads3 || re->tdfa[13] == 1) && f >= 0.02);
}
void upload(cs_regex* re, hipStream_t s) {
  // a compiled pattern may be shared between host threads (and is kept in the process-wide pattern cache): the device
  // images are made once.  All three are built into locals and committed together only after the copies completed --
  // an allocation or copy that throws half way must not leave d_image set with the DFA images missing (the guard
  // below would then skip the upload for every later caller of the cached pattern).
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (re->d_image) return;
  Buf image = dev_alloc(re->image.size() * 4, s), tdfa, gtags, bits;
  CS_HIP(hipMemcpyAsync(image->p, re->image.data(), re->image.size() * 4, hipMemcpyHostToDevice, s));
  if (!re->bits.empty()) {
    bits = dev_alloc(re->bits.size() * 4, s);
    CS_HIP(hipMemcpyAsync(bits->p, re->bits.data(), re->bits.size() * 4, hipMemcpyHostToDevice, s));
  }
  if (!re->tdfa.empty()) {
    tdfa = dev_alloc(re->tdfa.size() * 4, s);
    CS_HIP(hipMemcpyAsync(tdfa->p, re->tdfa.data(), re->tdfa.size() * 4, hipMemcpyHostToDevice, s));
    if (!re->gtags.empty()) {
      gtags = dev_alloc(re->gtags.size() * 4, s);
      CS_HIP(hipMemcpyAsync(gtags->p, re->gtags.data(), re->gtags.size() * 4, hipMemcpyHostToDevice, s));
    }
  }
  CS_HIP(hipStreamSynchronize(s));
  re->d_tdfa = std::move(tdfa);
  re->d_gtags = std::move(gtags);
  re->d_bits = std::move(bits);
  re->d_image = std::move(image);  // (last: it is what the guard looks at)
}
TPlan tplan(cs_regex* re, int64_t rows, hipStream_t s) {
  require_device();
  upload(re, s);
  if (!re->d_tdfa) fail(CS_ERR_INTERNAL, "regex: the tagged-DFA image is not on the device");
  TPlan pl{};
  pl.d.tdfa = ptr<const int32_t>(re->d_tdfa);
  pl.d.tdfa_words = (int)re->tdfa.size();
  pl.d.image = ptr<const int32_t>(re->d_image);
  pl.d.in_lds = re->tdfa.size() * 4 <= kLdsBudget && !cs::cfg("CS_TDFA_GLOBAL_TABLE");
  pl.lds_bytes = pl.d.in_lds ? ((re->tdfa.size() * 4 + 15) & ~size_t(15)) : 0;
  int64_t nblk = (rows + 255) / 256;
  pl.grid = (unsigned)std::min<int64_t>(std::max<int64_t>(nblk, 1), 256 * 8);
  return pl;
}

Plan plan(cs_regex* re, int64_t rows, hipStream_t s) {
  require_device();
  upload(re, s);
  Plan pl{};
  Launch& L = pl.d;
  L.image = ptr<const int32_t>(re->d_image);
  L.image_words = (int)re->image.size();
  const int ninst = (int)re->prog.insts.size();
  pl.small = ninst <= 64;
  L.slots = csvm::vm_slots(ninst);
  const size_t img_bytes = (((size_t)L.image_words + 3) & ~size_t(3)) * 4;
  L.image_in_lds = img_bytes <= kLdsBudget / 2;
  L.arena = nullptr;
  pl.threads = 0;
  for (int t : {256, 128, 64}) {
    size_t need = (L.image_in_lds ? img_bytes : 0) + (size_t)t * L.slots * 4;
    if (need <= kLdsBudget) {
      pl.threads = t;
      pl.lds_bytes = need;
      break;
    }
  }
  if (pl.threads) {
    int64_t nblk = (rows + pl.threads - 1) / pl.threads;
    pl.grid = (unsigned)std::min<int64_t>(nblk, 256 * 16);
  } else {
    // lists in a global arena, one region per resident workgroup
    pl.threads = 256;
    pl.lds_bytes = L.image_in_lds ? img_bytes : 0;
    int64_t nblk = (rows + pl.threads - 1) / pl.threads;
    pl.grid = (unsigned)std::min<int64_t>(nblk, 256 * 4);
    if (pl.grid == 0) pl.grid = 1;
    size_t bytes = (size_t)pl.grid * pl.threads * L.slots * 4;
    pl.arena_buf = dev_alloc(bytes, s);
    L.arena = ptr<uint32_t>(pl.arena_buf);
  }
  if (pl.grid == 0) pl.grid = 1;
  return pl;
}

// Rows per tile and staging capacity for the stream kernels: 64 rows when their widest span fits
// the prefetch registers and no row outgrows the 96-byte candidate masks; otherwise the long-row
// variants (rows up to 255 bytes) with 64, 32 or 16 rows per tile.  R == 0: no stream kernel.
// `small`: also tiles of eight and four rows, also for rows beyond the sliding window (replace_re: its alternative is the
// two-pass thread-per-row kernels; the scans' row-wise kernels beat such tiles: contains_re 1.9 against 4.6 ms, findall 27
// against 64 ms on 520-byte rows)
// (replace_re on 64-row tiles of up to 8 KB for long rows -- eight prefetch chunks a lane -- was built and measured in round 6:
// 14.5 ms on the C5 column either way.  What such a column waits for is its tiles' PREFIXES, and twice the work per tile does
// not shorten that; nor does drawing the tickets an iteration later (4.33 ms on C3, 14.7 on C5 either way): profiles/r06/prefix_latency.txt.)
TileChoice choose_tile(const cs_column* col, hipStream_t s, bool small) {
  const int64_t longest = max_row_bytes(col, s);
  auto cap_of = [](int64_t span) { return (int64_t)((span + 15 + 32 + 127) & ~(int64_t)127); };
  const int64_t span64 = max_span64(col, s);
  const int64_t cap64 = cap_of(span64);
  const bool fits64 = cap64 <= cstile::kPfBytes;
  if (fits64 && longest + 3 <= cstd::Tdfa::kMaskBytes) return {64, (int)cap64, false, span64};
  if (longest > cstd::Tdfa::kLongBytes && (fits64 || !small)) return {fits64 ? 64 : 0, (int)cap64, false, span64};  // (such tiles scan generically)
  if (fits64) return {64, (int)cap64, true, span64};
  // (eight and four rows a tile: rows of hundreds of bytes -- few lanes of a wave hold a row then, but the rows still arrive
  // through coalesced tiles and are scanned in LDS; the thread-per-row kernels read them byte by byte from memory)
  for (int r : {32, 16, 8, 4}) {
    if (r < 16 && !small) break;
    const int64_t sp = max_span_rows(col, r, s);
    const int64_t c = cap_of(sp);
    if (c <= cstile::kPfBytes) return {r, (int)c, true, sp};
  }
  return {0, (int)cap64, false, span64};
}

// A column with rows beyond the 96-bit masks, a program for which white space is a safe cut (regex_tdfa.cpp, header word 31
// bit 25): the op runs on the column's PIECES (cs_virtual.hip) -- chain arithmetic, bit form, unit scan as on short rows --
// and the rows' results follow from the pieces'.
// Not for a single class, once or in a `+` loop (cs_runs.hip takes rows of any length byte-parallel: count_re([aeiou]+) on the
// C5 column 3.0 ms there, 5.6 on the pieces), and not -- `replacing` -- for a program that would take the unit scan on a column
// whose sample holds bytes >= 0x80: the unit route hands every sub-tile with such a byte to the row-by-row scan, and more,
// shorter rows make that worse (replace_re of the gtest pattern on C5: 40 ms on the pieces, 30 on the long-row form).
const VirtualRows* pieces_for(const cs_column* col, const cs_regex* re, hipStream_t s, bool replacing, bool containing) {
  if (cs::cfg("CS_NO_VIRTUAL_ROWS") || col->virt_state < 0 || !use_tdfa(re) || !((re->tdfa[31] >> 25) & 1)) return nullptr;
  if (max_row_bytes(col, s) + 3 <= cstd::Tdfa::kMaskBytes) return nullptr;  // (the masks hold the rows as they are)
  const bool chain = ((re->tdfa[30] >> 16) & 15) != 0;
  // One class, once or in a `+` loop: cs_runs.hip counts and replaces such a pattern byte-parallel on rows of any length -- and
  // keeps the patterns that would take the chain arithmetic here (`[a-z]+` -> '_' on the C5 column: 11.2 ms there, 13.1 on the
  // pieces) and the columns where bytes >= 0x80 are common (it takes them as they come; the mask forms do not).  The others go to
  // the pieces' bit form once such rows are put off / left holes: `\w+` 27.7 -> 7.9 ms (cs_runs.hip sends every tile with such a
  // byte row by row for a class with builtins), `[aeiou]+` 11.1 -> 8.0, count_re 2.9 -> 2.5; contains_re has no form there at all.
  if (!containing && !re->bits.empty() && (re->bits[2] & (csbits::F_BYTE_CLASS | csbits::F_FLAG_CLASS)) && !cs::cfg("CS_NO_CLASS_RUNS") &&
      (chain || (sample_has_high_bytes(col, s) && !odd_rows_few(col, s)) || cs::cfg("CS_CLASS_RUNS_ALWAYS")))
    return nullptr;
  // (... unless such bytes are rare: the single pass then leaves the rows that hold them holes -- StreamArgs::hole_mask)
  if (replacing && (re->tdfa[31] & 1) && !chain && sample_has_high_bytes(col, s) && !odd_rows_few(col, s)) return nullptr;
  // The executor ends a row's scan at a NUL byte and takes a character's width from its lead byte (an ASCII byte behind a
  // lead without its continuation bytes is swallowed -- a cut byte too): a piece behind such a byte would be scanned where
  // the row is not.  Columns of well-formed text only (`plain_bytes`: column metadata, one pass when nobody has looked yet).
  if (!bytes_plain(col, s)) return nullptr;
  return virtual_rows(col, s);
}

// ---- shared by the scans and the span ops (extract, findall, replace_with_backrefs) -------------------------------------
// The column's rows for a kernel that reads them from memory: chars from the pool carry 64 bytes of slack that may be read.
// (cs_replace_re_multi passes col->nbytes without the slack; left as it is.)
RowSrc row_src(const cs_column* col) { return RowSrc{view_of(col), d_unicode_flags(), col->nbytes + (col->chars && col->chars->capacity ? 64 : 0)}; }
// The group tags' share of a stream launch's LDS: 0 when there are none or they take more than 16 KB (they stay in memory
// then), else their size rounded up to 16.
size_t gtags_lds_bytes(const cs_regex* re) {
  const size_t bytes = re->gtags.size() * 4;
  return bytes && bytes <= 16 * 1024 ? (bytes + 15) & ~size_t(15) : 0;
}
// What every launch of k_tdfa_scan_stream says about its input: the column, the tables, the tiles.  The caller adds its own
// fields (tbl_bytes, the group tags, the outputs, L.in_lds = 2 for tables in memory).
ScanStreamArgs stream_args(const cs_column* col, const TPlan& tp, const TileChoice& tc) {
  ScanStreamArgs sa{};
  sa.in = view_of(col);
  sa.flags = d_unicode_flags();
  sa.L = tp.d;
  sa.nsub = (col->rows + tc.R - 1) / tc.R;
  sa.rows_per_tile = tc.R;
  sa.cap_in = tc.cap;
  return sa;
}

}  // namespace rx
}  // namespace cs

extern "C" {

// Reprog::create_from + dreprog::create_from -- regcomp.cpp:954-960, regexec.cpp:12-73
int cs_regex_compile(const char* pattern, cs_regex** out) {
  return guard([&] {
    if (!pattern || !out) fail(CS_ERR_INVALID_ARG, "regex pattern cannot be null");
    // A compiled pattern is immutable (the device images are uploaded once, under a lock) and costs 0.6 - 1.6 ms of host
    // time to build -- a tenth of the replace_re kernel on 100M rows, more than the kernel on a few million -- while
    // the callers above the C ABI compile per call, as the reference does.  The last 32 patterns are kept; a handle
    // is a counted reference to the shared object.
    static std::mutex& mu = *new std::mutex;  // (never destroyed: see the note on process exit in cs_core.hip's buffer cache)
    static auto& kept = *new std::list<std::pair<std::string, cs_regex*>>;
    const bool keep = !cs::cfg("CS_REGEX_NO_CACHE");
    if (keep) {
      std::lock_guard<std::mutex> lk(mu);
      for (auto it = kept.begin(); it != kept.end(); ++it)
        if (it->first == pattern) {
          kept.splice(kept.begin(), kept, it);
          it->second->refs.fetch_add(1);
          *out = it->second;
          return;
        }
    }
    std::unique_ptr<cs_regex> re(new cs_regex);
    re->empty_pattern = *pattern == 0;
    re->prog = csrx::compile(pattern);
    re->blob = re->prog.to_blob();
    re->image = re->prog.to_device_image(h_unicode_flags());
    re->tdfa = csrx::build_tdfa(re->prog, re->image, h_unicode_flags(), &re->gtags);
    re->bits = csrx::build_bits(re->prog, re->image, h_unicode_flags());
    cs_regex* dropped = nullptr;
    if (keep) {
      std::lock_guard<std::mutex> lk(mu);
      re->refs.store(2);
      kept.emplace_front(pattern, re.get());
      if (kept.size() > 32) {
        dropped = kept.back().second;
        kept.pop_back();
      }
    }
    *out = re.release();
    if (dropped && dropped->refs.fetch_sub(1) == 1) delete dropped;
  });
}
int cs_regex_destroy(cs_regex* re) {
  return guard([&] {
    if (re && re->refs.fetch_sub(1) == 1) delete re;
  });
}
int cs_regex_inst_count(const cs_regex* re) { return re ? (int)re->prog.insts.size() : 0; }
int cs_regex_engine(const cs_regex* re) {
  if (!re) return 0;
  int e = 0;
  if (!re->tdfa.empty()) {
    e |= 1;                               // the tagged DFA (regex_tdfa.h) runs the pattern
    if (re->tdfa[31] & 1) e |= 2;         // ... and offers the unit decomposition (regex_tdfa.cpp)
    if (!re->gtags.empty()) e |= 4;       // ... and carries the capture-group tags
    e |= (re->tdfa[12] & 15) << 8;        // live threads the automaton keeps at most
    e |= (re->tdfa[1] & 0xFFFF) << 16;    // states
  }
  return e;
}
int cs_regex_blob(const cs_regex* re, const int32_t** words, int* nwords) {
  return guard([&] {
    if (!re || !words || !nwords) fail(CS_ERR_INVALID_ARG, "null argument");
    *words = re->blob.data();
    *nwords = (int)re->blob.size();
  });
}

}  // extern "C"
