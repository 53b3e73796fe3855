// Private to the regex units: the persistent scan kernel over row tiles, k_tdfa_scan_stream, with its arguments -- a
// template in a header because each unit instantiates its own modes (the scans 0-2 and 7-9, findall 3, extract 4,
// replace_with_backrefs 5 and 6) --, and the unit-scan and bit-form device helpers it shares with
// k_tdfa_replace_stream (cs_regex.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "cs_internal.h"
#include "device_utils.h"
#include "regex_bits.h"
#include "regex_exec.h"
#include "tile_utils.h"

using namespace cs;
using namespace csdev;
using namespace cs::rx;

namespace {

// ---- unit scan (regex_tdfa.cpp, header word 31): helpers shared by the stream kernels ------------------
constexpr int kUnitQueue = 128;  // units one round of the queue holds (a busier sub-tile scans its rows whole)
// Row lanes: the row's candidate bits (returned in m0..m2) and x bits give its units; all units of the sub-tile are
// queued as (row | first byte << 8 | end << 16).  `between` runs once every lane holds its masks (the bitmaps may
// be re-used from there on).  Returns the number of units, or -1 when the queue cannot hold them (nothing is
// written then and `between` has not run).
template <class Between>
__device__ __forceinline__ int unit_discover(const cstd::View& D, const uint32_t* bitmap, const uint32_t* xbitmap, int p0, int n, int lane,
                                             uint32_t* uqueue, uint32_t& m0, uint32_t& m1, uint32_t& m2, Between&& between) {
  using namespace cstd;
  uint32_t x0 = 0, x1 = 0, x2 = 0;
  cstile::row_bits96(bitmap, p0, n, m0, m1, m2);
  if ((D.units >> 8) & 127u) cstile::row_bits96(xbitmap, p0, n, x0, x1, x2);
  const U128 C = u128(m0 | ((unsigned long long)m1 << 32), m2), X = u128(x0 | ((unsigned long long)x1 << 32), x2);
  U128 N;
  U128 W = unit_ends(C, X, ((D.units >> 16) & 1u) != 0, N);
  const int cnt = u128_popc(W);
  const int uincl = csdev::wave_inclusive_scan(cnt);
  const int total = __builtin_amdgcn_readlane(uincl, 63);
  if (total > kUnitQueue) return -1;
  cstile::wave_lds_fence();
  between();
  int slot = uincl - cnt;
  while (__any(u128_any(W))) {
    if (u128_any(W)) {
      const int q = u128_ctz(W);
      W = u128_clear_lowest(W);
      uqueue[slot++] = (uint32_t)lane | ((uint32_t)unit_start(N, q) << 8) | ((uint32_t)q << 16);
    }
  }
  cstile::wave_lds_fence();
  return total;
}
// Unit lanes: queue entry -> the unit's row (its position and length come from the row's lane) and the row's
// candidate bits cut to the unit.  Every lane of the wave must call this (shuffles).
// `clip`: the row handed to the unit's scan ends where the unit ends (see reclassify_high: the byte behind it may be >= 0x80).
__device__ __forceinline__ void unit_take(uint32_t ent, int rbeg, int n, uint32_t m0, uint32_t m1, uint32_t m2, int& r, int& rbeg_r, int& n_r,
                                          uint32_t& c0, uint32_t& c1, uint32_t& c2, bool clip = false) {
  using namespace cstd;
  r = (int)(ent & 63u);
  const int us = (int)((ent >> 8) & 255u), uq = (int)((ent >> 16) & 255u);
  rbeg_r = __shfl(rbeg, r, 64);
  n_r = __shfl(n, r, 64);
  if (clip && uq < n_r) n_r = uq;
  const U128 keep = u128_andn(u128_below(uq), u128_below(us));
  c0 = (uint32_t)__shfl((int)m0, r, 64) & (uint32_t)keep.lo;
  c1 = (uint32_t)__shfl((int)m1, r, 64) & (uint32_t)(keep.lo >> 32);
  c2 = (uint32_t)__shfl((int)m2, r, 64) & (uint32_t)keep.hi;
}
// "byte == x" bits of one 16-byte piece (staging, from the prefetch registers)
__device__ __forceinline__ uint32_t unit_xbits16(const uint4& q, uint32_t xpat) {
  auto eq = [&](uint32_t w) {  // bit 7 of every byte lane that equals x (exact: no borrow between lanes)
    const uint32_t t = w ^ xpat;
    return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
  };
  return cstile::gather16_bit7(eq(q.x), eq(q.y), eq(q.z), eq(q.w));
}

// Sub-tiles that hold bytes >= 0x80 (non-ASCII text).  The lean scan indexes its table with ASCII bytes only, so such a
// sub-tile used to take the generic per-character scan, three to four times slower.  For a pattern none of whose atoms can
// match a non-ASCII character and that has no anchors and no \b (header word 31, bit 17) such a character kills every
// thread, as the end of the row does: the UNIT route can take the sub-tile -- units are runs of candidate / x bytes, ASCII
// all of them -- provided a unit's scan ends at the unit's end (unit_take: clip) instead of reading the killer behind it.
// This pass re-derives the candidate bits from the staged bytes with the bytes >= 0x80 taken out (the classification out
// of the prefetch registers looks at their low seven bits) and says whether the sub-tile holds a NUL byte (then: generic).
// Header word 31 bit 18 (mask in bits 19-23): the pattern's builtin classes (\w, \s, \d) do match some non-ASCII characters
// -- those whose unicode flags meet the mask; the row lanes then walk their rows' non-ASCII characters: the sub-tile
// qualifies when its UTF-8 is well formed inside every row and no character's flags meet the mask.
__device__ __forceinline__ bool reclassify_high(const cstd::View& D, bool has_r2, const uint8_t* lds_in, int want, int lane, uint32_t* bitmap,
                                                const uint8_t* flags, const uint8_t* row, int n) {
  const unsigned fmask = (D.units >> 19) & 31u;
  bool row_bad = false;
  {
    // aligned words of the row, only the bytes >= 0x80 looked at one by one (a lead byte checks its continuation bytes and
    // covers them; a byte >= 0x80 that no lead covers is a stray one).  Also for the patterns such characters can only kill
    // (bit 17): a lead byte WITHOUT its continuation bytes swallows the ASCII bytes behind it (regex_vm.h: char_at), which the
    // unit route would scan -- count_re(b|ab) counted the b of `4\xc3b` (found by the soak, round 5)
    const int al = (int)((uintptr_t)row & 3);
    int covered = 0;  // row offsets below this one belong to a character already checked
    for (int i = -al; i < n && !row_bad; i += 4) {
      uint32_t h = *reinterpret_cast<const uint32_t*>(row + i) & 0x80808080u;
      if (i < 0) h &= 0xFFFFFFFFu << (8 * -i);
      if (i + 4 > n) h &= ~(0xFFFFFFFFu << (8 * (n - i)));
      while (h && !row_bad) {
        const int p = i + (__builtin_ctz(h) >> 3);
        h &= h - 1;
        if (p < covered) continue;
        const uint8_t b = row[p];
        const unsigned w = csrow::lead_width(b);
        row_bad = w < 2 || p + (int)w > n;
        for (unsigned k = 1; k < w && !row_bad; ++k) row_bad = !csrow::is_cont(row[p + (int)k]);
        if (!row_bad) {
          csrow::Char ch;
          csrow::decode_at(row, p, n, ch);
          const unsigned u = csrow::packed_to_cp(ch);
          row_bad = ((D.units >> 18) & 1u) != 0 && u <= 0xFFFFu && (flags[u] & fmask) != 0;
        }
        covered = p + (int)w;
      }
    }
  }
  uint32_t zr = row_bad ? 0x80u : 0u;
  for (int i = lane * 16; i < want; i += 64 * 16) {
    const uint4 q = *reinterpret_cast<const uint4*>(lds_in + i);
    zr |= ((q.x - 0x01010101u) & ~q.x) | ((q.y - 0x01010101u) & ~q.y) | ((q.z - 0x01010101u) & ~q.z) | ((q.w - 0x01010101u) & ~q.w);
    uint32_t bits;
    if (has_r2)
      bits = cstile::gather16_bit7(cstd::Tdfa::cand_bits_ascii<true>(D, q.x) & ~q.x, cstd::Tdfa::cand_bits_ascii<true>(D, q.y) & ~q.y,
                                   cstd::Tdfa::cand_bits_ascii<true>(D, q.z) & ~q.z, cstd::Tdfa::cand_bits_ascii<true>(D, q.w) & ~q.w);
    else
      bits = cstile::gather16_bit7(cstd::Tdfa::cand_bits_ascii<false>(D, q.x) & ~q.x, cstd::Tdfa::cand_bits_ascii<false>(D, q.y) & ~q.y,
                                   cstd::Tdfa::cand_bits_ascii<false>(D, q.z) & ~q.z, cstd::Tdfa::cand_bits_ascii<false>(D, q.w) & ~q.w);
    cstile::put_bits16(bitmap, i, bits);
  }
  cstile::wave_lds_fence();
  // (a zero byte below a byte >= 0x80 may go unseen by the borrow trick's neighbour term; a byte >= 0x80 never looks like one)
  return __any((zr & 0x80808080u) != 0);
}

// ---- the bit-parallel form (regex_bits.h): staging helpers shared by the stream kernels ------------------
// LDS image of the form: the program words as built by the host, then 128 words of the SPREAD class table --
// entry b holds byte b's class set with class k at bit 4k, so that the entries of four bytes, shifted by 0..3
// and OR-ed, leave a nibble per class: the four bytes' membership bits.
__device__ __forceinline__ const uint32_t* bits_stage(const int32_t* g_bits, int words, int32_t* lds) {
  for (int i = threadIdx.x; i < words; i += blockDim.x) lds[i] = g_bits[i];
  uint32_t* sp = reinterpret_cast<uint32_t*>(lds + ((words + 3) & ~3));
  if (threadIdx.x < 128) {
    const uint32_t set = ((uint32_t)g_bits[csbits::kHeaderWords + (threadIdx.x >> 2)] >> (8 * (threadIdx.x & 3))) & 255u;
    sp[threadIdx.x] = csbits::spread_entry(set);
  }
  __syncthreads();
  return sp;
}
__host__ __device__ inline int bits_lds_bytes(int words) { return ((words + 3) & ~3) * 4 + 128 * 4; }
// sixteen staged bytes -> for every class the sixteen membership bits (regex_bits.h: classify16)
__device__ __forceinline__ void bits_classify16(const uint32_t* spread, const uint4& q, uint32_t pair[4]) {
  csbits::classify16(spread, q.x, q.y, q.z, q.w, pair);
}
// a row lane's mask of class k, shifted right by `off`: cut out of the class's bitmap on demand (regex_bits.h: cls(k, off))
#define CS_BITS_CLS(bitmap, bm_words, p0, n)                                                                       \
  [&](int k_, int off_) -> csbits::M96 {                                                                           \
    uint32_t m0_, m1_, m2_;                                                                                        \
    cstile::row_bits96((bitmap) + __builtin_amdgcn_readfirstlane(k_) * (bm_words), (p0) + off_, max((n) - off_, 0), m0_, m1_, m2_); \
    return csbits::m96(m0_, m1_, m2_);                                                                             \
  }
// ... without the cut at the row's end (regex_bits.h: raw(k, off)): three funnel shifts over four words of the bitmap
#define CS_BITS_RAW(bitmap, bm_words, p0)                                                                          \
  [&](int k_, int off_) -> csbits::M96 {                                                                           \
    const int q_ = (p0) + off_;                                                                                    \
    const uint32_t* w_ = (bitmap) + __builtin_amdgcn_readfirstlane(k_) * (bm_words) + (q_ >> 5);                   \
    const uint32_t a_ = w_[0], b_ = w_[1], c_ = w_[2], d_ = w_[3];                                                 \
    const unsigned sh_ = (unsigned)q_ & 31u;                                                                       \
    const uint32_t m0_ = __builtin_amdgcn_alignbit(b_, a_, sh_), m1_ = __builtin_amdgcn_alignbit(c_, b_, sh_),     \
                   m2_ = __builtin_amdgcn_alignbit(d_, c_, sh_);                                                   \
    return csbits::m96(m0_, m1_, m2_);                                                                             \
  }

}  // namespace

// ---- persistent contains_re / count_re over row tiles -----------------------------------
// Same staging as the replace kernel (contiguous tile runs per wave, next tile's chars in
// flight), no output assembly: LDS holds the DFA table and one input tile per wave, so seven
// workgroups fit a CU.  MODE 0 contains_re, 2 count_re, 3 findall spans (begins / lens [k * rows + row]),
// 4 extract spans (leftmost match, then Tdfa::group_find per capture group, all on the staged row),
// 5 / 6 replace_with_backrefs sizes / bytes (csvm::row_backrefs on the staged row; the bytes go out per row lane).
namespace cs {
namespace rx {
struct ScanStreamArgs {
  ColView in;
  const uint8_t* flags;
  TLaunch L;
  uint8_t* out8;
  int32_t* out32;
  unsigned long long* found;
  long long nsub;
  int cap_in, tbl_bytes;
  int rows_per_tile;  // LONG variant: 64, 32 or 16
  int32_t* begins;    // MODE 3, 4
  int32_t* lens;
  int ncols;
  int* maxp;             // MODE 3 (optional): receives the largest match count of a row
  // MODE 3, 4 (optional): the spans as ONE word per (column, row) -- begin << 16 | length, 0xFFFFFFFF = null -- instead of
  // begins / lens (half the span traffic; rows of a tile are far shorter than 64 KiB), and the bytes every 64-row tile
  // gives to each column, [column][tile] (rows_per_tile == 64 only): k_spans_write_tile2 sizes the columns from those
  uint32_t* spans;
  int32_t* tile_tot;
  const int32_t* gtags;  // MODE 4, 5, 6: capture-group tag image
  int gt_off, gt_words;  // when gt_words > 0 the image is staged into LDS at byte offset gt_off (inside tbl_bytes)
  const csvm::BackrefTemplate* tmpl;  // MODE 5, 6 (device memory: indexed per reference, must not live in the kernel arguments)
  const int64_t* out_off;      // MODE 6
  uint8_t* out_chars;
  // BITS: the bit-parallel form of the pattern (regex_bits.h), staged at byte offset bits_off of the LDS (inside tbl_bytes)
  const int32_t* bits;
  int bits_off, bits_words, bits_k;
  // MODE 0 / 2, 64-row tiles (optional): rows that hold a byte >= 0x80 or a NUL are not scanned here -- their indices go to
  // this list (k_tdfa_scan_list scans them afterwards, a thread a row), and the tile's other rows keep the form the launch was
  // chosen for (bit form, chain arithmetic, unit scan, lean scan) instead of the whole sub-tile going to the row-by-row scan
  int32_t* deferred;
  unsigned* ndeferred;
  unsigned deferred_cap;
};
using ScanStreamKernel = void (*)(ScanStreamArgs);
}  // namespace rx
}  // namespace cs

namespace {

// UNITS (MODE 0 and 2, !LONG): the unit scan of the replace kernel -- units queued by the row lanes, one unit per lane
// whatever its row, the per-row result summed (count_re) / OR-ed (contains_re) in LDS.
// CHAIN (a UNITS form, count_re / findall): the pattern is a chain and the column's sample holds no byte >= 0x80 -- the unit
// and lean scans are compiled out, a sub-tile the chain arithmetic does not take is scanned row by row by the generic executor.
// BITS (a CHAIN form, contains_re / count_re): the pattern has a bit-parallel form (regex_bits.h) and the column's sample holds
// no byte >= 0x80 -- every staged byte is classified into one bitmap per character class by table lookup, the row lanes
// read their rows' class masks and derive the matches by mask arithmetic; no automaton on a plain-ASCII sub-tile.
template <int MODE, bool IN_LDS, bool LONG = false, bool UNITS = false, bool CHAIN = false, bool BITS = false>
__global__ void __launch_bounds__(256, MODE == 4 ? ((CHAIN && !IN_LDS) ? 4 : 3) : CHAIN ? 4 : (UNITS && MODE == 3) ? 3 : (UNITS || MODE == 3) ? 4 : (MODE <= 1 && !LONG) ? 5 : 1) k_tdfa_scan_stream(ScanStreamArgs a) {
  static_assert(!UNITS || ((MODE == 0 || MODE == 2 || MODE == 3 || (MODE == 4 && CHAIN)) && !LONG), "unit scan: contains_re / count_re / findall on rows within the 96-byte masks");
  static_assert(!CHAIN || (UNITS && (MODE == 2 || MODE == 3 || MODE == 4 || (BITS && MODE == 0))), "the chain form: count_re / findall / extract");
  static_assert(!BITS || (CHAIN && (MODE == 0 || MODE == 2)), "the bit form: contains_re / count_re");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint8_t* base = reinterpret_cast<uint8_t*>(smem);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;  // (scalar: what derives from it stays in SGPRs)
  const int bm_bytes = (a.cap_in >> 3) + 32;
  const int nbm = BITS ? max(a.bits_k, 2) : 2;  // bitmaps per wave (BITS: one per character class)
  // (MODE 4 keeps a lane-private byte per step of a group run behind the bitmap: regex_tdfa.h, group_find_back)
  const int unit_bytes = UNITS ? (nbm - 1) * bm_bytes + kUnitQueue * 4 + 64 * 4 + 16 : (MODE == 4 ? cstd::Tdfa::kBackSteps * 64 + kMaxGroups * 4 : 0);  // x bitmap, unit queue, per-row results, bail word
  uint8_t* lds_in = base + a.tbl_bytes + (size_t)wv * (a.cap_in + 32 + bm_bytes + unit_bytes + (((MODE == 0 || MODE == 2) && !LONG && a.deferred) ? bm_bytes + 64 * 4 : 0));
  uint32_t* bitmap = reinterpret_cast<uint32_t*>(lds_in + a.cap_in + 32);
  uint32_t* xbitmap = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(bitmap) + bm_bytes);
  uint32_t* uqueue = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(bitmap) + (size_t)nbm * bm_bytes);
  uint32_t* rowres = uqueue + kUnitQueue;
  uint32_t* bailw = rowres + 64;
  constexpr bool kDefer = (MODE == 0 || MODE == 2) && !LONG;
  const bool deferring = kDefer && a.deferred != nullptr;  // (wave-uniform)
  uint32_t* oddmap = reinterpret_cast<uint32_t*>(lds_in + a.cap_in + 32 + bm_bytes + unit_bytes);  // (behind everything else of the wave)
  // the wave's rows put off and not yet in the list: one atomic on the list's counter per 64 of them at most (one per sub-tile
  // with such a row was 600K on one address for the C5 column's pieces -- 2 ms of a 4 ms kernel)
  int32_t* pend = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(oddmap) + bm_bytes);
  int npend = 0;  // (wave-uniform)
  auto flush_pend = [&] {
    cstile::wave_lds_fence();
    unsigned at = 0;
    if (lane == 0) at = atomicAdd(a.ndeferred, (unsigned)npend);
    at = (unsigned)__builtin_amdgcn_readfirstlane((int)at);
    if (lane < npend && at + (unsigned)lane < a.deferred_cap) a.deferred[at + lane] = pend[lane];
    cstile::wave_lds_fence();
    npend = 0;
  };
  // MODE 4: per group, the tile's bytes (the chain form keeps the "equals x" bitmap where the plain form has its history bytes)
  uint32_t* gtot = UNITS ? rowres : reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(xbitmap) + cstd::Tdfa::kBackSteps * 64);
  if (MODE == 4 && lane < kMaxGroups) gtot[lane] = 0;
  const TCtx c = tsetup<IN_LDS>(a.L, a.flags, smem);
  const cstd::View& D = c.D;
  const csvm::ProgView& P = c.P;
  const ColView& in = a.in;
  if (MODE >= 4 && a.gt_words > 0) {  // the group-tag tables are read once per DFA step: keep them next to the DFA table
    int32_t* g = reinterpret_cast<int32_t*>(base + a.gt_off);
    for (int i = threadIdx.x; i < a.gt_words; i += blockDim.x) g[i] = a.gtags[i];
    __syncthreads();
    a.gtags = g;
  }
  const uint32_t* spread = nullptr;
  csbits::View BV{};
  if (BITS) {
    int32_t* bl = reinterpret_cast<int32_t*>(base + a.bits_off);
    spread = bits_stage(a.bits, a.bits_words, bl);
    BV = csbits::make_view(bl);
  }
  const bool has_r2 = (((uint32_t)D.img[30] & 255u) <= (((uint32_t)D.img[30] >> 8) & 255u));
  const uint32_t unit_x = (D.units >> 8) & 127u, unit_xpat = unit_x * 0x01010101u;
  const int R = LONG ? a.rows_per_tile : 64;
  const long long waves = (long long)gridDim.x * 4;
  const long long per = (a.nsub + waves - 1) / waves;
  long long tile = ((long long)blockIdx.x * 4 + wv) * per;
  const long long tile_end = min(a.nsub, tile + per);
  if (tile >= tile_end) return;
  cstile::TileOffs cur = cstile::load_tile_offsets_r(in.offsets, in.rows, tile, R, lane);
  cstile::TileOffs nxt = cur;
  if (tile + 1 < tile_end) nxt = cstile::load_tile_offsets_r(in.offsets, in.rows, tile + 1, R, lane);
  cstile::TileChars pf;
#pragma unroll
  for (int j = 0; j < cstile::kPfChunks; ++j) pf.v[j] = make_uint4(0, 0, 0, 0);
  cstile::issue_chars(in.chars, cstile::rl64(cur.o0, 0), cstile::rl64(cur.o1, 63), lane, pf);
  int hits = 0;
  for (;;) {
    const long long r0 = tile * R;
    const int nrows = (int)min((long long)R, in.rows - r0);
    const long long g0 = cstile::rl64(cur.o0, 0), g1 = cstile::rl64(cur.o1, 63);
    const bool live0 = lane < nrows && row_is_valid(in.validity, r0 + lane);
    const int rbeg = (int)(cur.o0 - g0);
    const int n0 = live0 ? (int)(cur.o1 - cur.o0) : 0;
    const int lead = (int)((uintptr_t)(in.chars + g0) & 15);
    const int want = (int)(g1 - g0) + lead;
    cstile::stage_chars(lds_in, want, lane, pf);
    uint32_t odd = 0;
#pragma unroll
    for (int j = 0; j < cstile::kPfChunks; ++j)
      if (j * 1024 + lane * 16 < want) {
        const uint4 q = pf.v[j];
        const uint32_t ox = q.x | ((q.x - 0x01010101u) & ~q.x), oy = q.y | ((q.y - 0x01010101u) & ~q.y);
        const uint32_t oz = q.z | ((q.z - 0x01010101u) & ~q.z), ow = q.w | ((q.w - 0x01010101u) & ~q.w);
        odd |= ox | oy | oz | ow;
        if (deferring) cstile::put_bits16(oddmap, j * 1024 + lane * 16, cstile::gather16_bit7(ox & 0x80808080u, oy & 0x80808080u, oz & 0x80808080u, ow & 0x80808080u));
        if (BITS) {
          uint32_t pair[4];
          bits_classify16(spread, q, pair);
#pragma unroll
          for (int k = 0; k < csbits::kMaxClasses; ++k)
            if (k < BV.K) cstile::put_bits16(bitmap + k * (bm_bytes >> 2), j * 1024 + lane * 16, (pair[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
          continue;
        }
        uint32_t bits;
        if (has_r2)
          bits = cstile::gather16_bit7(cstd::Tdfa::cand_bits_ascii<true>(D, q.x), cstd::Tdfa::cand_bits_ascii<true>(D, q.y), cstd::Tdfa::cand_bits_ascii<true>(D, q.z),
                                       cstd::Tdfa::cand_bits_ascii<true>(D, q.w));
        else
          bits = cstile::gather16_bit7(cstd::Tdfa::cand_bits_ascii<false>(D, q.x), cstd::Tdfa::cand_bits_ascii<false>(D, q.y), cstd::Tdfa::cand_bits_ascii<false>(D, q.z),
                                       cstd::Tdfa::cand_bits_ascii<false>(D, q.w));
        cstile::put_bits16(bitmap, j * 1024 + lane * 16, bits);
        if (UNITS && unit_x != 0) cstile::put_bits16(xbitmap, j * 1024 + lane * 16, unit_xbits16(q, unit_xpat));
      }
    const bool has_next = tile + 1 < tile_end;
    // (the offsets two tiles ahead are fetched unconditionally, at a clamped index, and become `nxt` at the bottom of
    // the iteration: see the note in k_tdfa_replace_stream)
    const cstile::TileOffs nn = cstile::load_tile_offsets_r(in.offsets, in.rows, tile + 2 < tile_end ? tile + 2 : tile_end - 1, R, lane);
    if (has_next) {
      cur = nxt;
      cstile::issue_chars(in.chars, cstile::rl64(cur.o0, 0), cstile::rl64(cur.o1, 63), lane, pf);
    }
    cstile::wave_lds_fence();
    bool has_odd = __any((odd & 0x80808080u) != 0);
    bool live = live0;
    if (deferring && has_odd) {  // (wave-uniform)
      uint32_t d0, d1, d2;
      cstile::row_bits96(oddmap, lead + rbeg, n0 < 96 ? n0 : 96, d0, d1, d2);
      // (a row beyond the masks is not looked at: the tile is scanned row by row as before)
      const bool fits = !__any(live0 && n0 + ((lead + rbeg) & 3) > cstd::Tdfa::kMaskBytes);
      const bool put_off = fits && live0 && (d0 | d1 | d2) != 0;
      const unsigned long long who = __ballot(put_off);
      if (who) {
        const int k = __builtin_popcountll(who);
        if (npend + k > 64) flush_pend();
        if (put_off) pend[npend + __builtin_popcountll(who & ((1ull << lane) - 1ull))] = (int32_t)(r0 + lane);
        npend += k;
      }
      if (fits) {
        live = live0 && !put_off;
        has_odd = false;  // (what is left of the tile is plain)
        odd = 0;
      }
    }
    const int n = live ? n0 : 0;
    int v = 0;
    if (MODE == 5 || MODE == 6) {
      const uint8_t* p = lds_in + lead + rbeg;
      cstd::Tdfa vm(D, P, p, n, (lead + rbeg) & 3);
      auto find = [&](auto&& f) { csvm::walk_matches(vm, f); };
      // the groups of a match come four at a time from ONE anchored run (regex_tdfa.h: group_find_all) and are kept
      // until the walk moves to the next match: a template with four references costs one run, not four
      int c_mb = -1, c_batch = -1, c_ok = 0, c_end = 0;
      int c_gb[cstd::Tdfa::kGroupBatch], c_ge[cstd::Tdfa::kGroupBatch];
      const int tgroups = a.tmpl->groups;
      auto group = [&](int mb, int g, int& x, int& y) -> bool {
        if (n >= 255 || !a.gtags) return g == 0 ? vm.find(mb, mb + 1, x, y) > 0 : vm.group_find(mb, a.gtags, g, x, y) > 0;
        const int batch = g == 0 ? (c_mb == mb ? c_batch : 0) : (g - 1) / cstd::Tdfa::kGroupBatch;
        if (c_mb != mb || c_batch != batch) {
          const int first = batch * cstd::Tdfa::kGroupBatch + 1;
          int cnt = tgroups - first + 1;
          cnt = cnt < 0 ? 0 : (cnt > cstd::Tdfa::kGroupBatch ? cstd::Tdfa::kGroupBatch : cnt);
          c_ok = vm.group_find_all(mb, a.gtags, first, cnt, c_gb, c_ge, c_end);
          c_mb = mb;
          c_batch = batch;
        }
        if (g == 0) {
          x = mb;
          y = c_end;
        } else {
          const int k = (g - 1) % cstd::Tdfa::kGroupBatch;
#pragma unroll
          for (int i = 0; i < cstd::Tdfa::kGroupBatch; ++i)
            if (i == k) {
              x = c_gb[i];
              y = c_ge[i];
            }
        }
        return c_ok > 0;
      };
      if (MODE == 5) {
        int len = -1;
        if (live) {
          len = 0;
          csvm::row_backrefs(p, n, *a.tmpl, find, group, [&](const uint8_t*, int k) { len += k; });
        }
        if (lane < nrows) a.out32[r0 + lane] = len;
      } else if (live) {
        uint8_t* o = a.out_chars + a.out_off[r0 + lane];
        csvm::row_backrefs(p, n, *a.tmpl, find, group, [&](const uint8_t* q, int k) {
          for (int i = 0; i < k; ++i) *o++ = q[i];
        });
      }
    } else if (MODE == 1) {
      // match (count.cu:113-165): the anchored run on the staged row -- the rows arrive through the same coalesced
      // tiles as contains_re's instead of a thread per row reading its bytes from HBM
      cstd::Tdfa vm(D, P, lds_in + lead + rbeg, n, (lead + rbeg) & 3);
      v = live ? csvm::row_contains_re(vm, true) : 0;
    } else if (MODE >= 7) {
      // programs of five to eight live threads (MODE 7 contains_re, 8 match, 9 count_re): the generic executor with
      // eight start offsets on the staged row (regex_tdfa.h: TdfaWide)
      cstd::TdfaWide vm(D, P, lds_in + lead + rbeg, n, (lead + rbeg) & 3);
      v = !live ? 0 : (MODE == 9 ? csvm::row_count_re(vm) : csvm::row_contains_re(vm, MODE == 8));
    } else if (MODE == 4) {
      cstd::Tdfa vm(D, P, lds_in + lead + rbeg, n, (lead + rbeg) & 3);
      int mb = 0, me = 0;
      bool chain_done = false;
      if (CHAIN) {
        // extract on a chain pattern whose groups are runs of items (regex_tdfa.h: chain_match, chain_group_bounds) on a
        // sub-tile of plain ASCII: the row's first match and its group ranges from the row's two masks, no table walk
        const bool plain = D.nskip > 0 && D.img[12] <= 4 && !__any((odd & 0x80808080u) != 0) && !__any(live && !vm.masks_fit());
        if (plain && (D.chain >> 16) && (((uint32_t)D.img[30] >> 20) & 1u) && a.ncols <= 4 && a.spans) {  // (wave-uniform)
          using namespace cstd;
          uint32_t r0w, r1w, r2w, x0w = 0, x1w = 0, x2w = 0;
          cstile::row_bits96(bitmap, lead + rbeg, n, r0w, r1w, r2w);
          if (unit_x != 0) cstile::row_bits96(xbitmap, lead + rbeg, n, x0w, x1w, x2w);
          const U128 Rm = u128(r0w | ((unsigned long long)r1w << 32), r2w), Xm = u128(x0w | ((unsigned long long)x1w << 32), x2w);
          U128 S = u128(0, 0), E = u128(0, 0);
          if (live) chain_match96(r0w, r1w, r2w, x0w, x1w, x2w, D.chain, D.img, S, E, D.sfx, n, [&](int i) { return lds_in[lead + rbeg + i]; });
          const bool hit = live && u128_any(S);
          v = hit;
          int gb[4], ge[4];
          chain_group_bounds(Rm, Xm, D.chain, D.img, (uint32_t)D.img[D.img[15] - 1], hit ? u128_ctz(S) : 0, gb, ge);
          if (lane < nrows) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (k < a.ncols) {
                const bool ok = hit && gb[k] >= 0 && ge[k] > gb[k];
                a.spans[(long long)k * in.rows + r0 + lane] = ok ? (((uint32_t)gb[k] << 16) | (uint32_t)(ge[k] - gb[k])) : 0xFFFFFFFFu;
                if (a.tile_tot && ok) __hip_atomic_fetch_add(gtot + k, (uint32_t)(ge[k] - gb[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
              }
          }
          chain_done = true;
        }
      }
      if (__builtin_expect(!chain_done, !CHAIN)) {  // (the chain form: a cold path)
      // leftmost match: the lean scan on ASCII tiles of short rows (as contains_re), else the generic find
      const bool lean = !LONG && D.nskip > 0 && D.img[12] <= 4 && !__any((odd & 0x80808080u) != 0) && !__any(live && !vm.masks_fit());
      int f = -1;
      if (lean && live) {
        uint32_t m0, m1, m2;
        cstile::row_bits96(bitmap, lead + rbeg, n, m0, m1, m2);
        f = vm.scan_lean_first(m0, m1, m2, [&](int b0, int e0, int) {
          mb = b0;
          me = e0;
        });
      }
      if (live && f < 0) f = vm.find(0, n, mb, me);
      const bool hit = live && f > 0;
      v = hit;
      if (lane < nrows) {
        if (n < 255) {  // every group of the match from one anchored run, four at a time (regex_tdfa.h: group_find_all)
          for (int g0 = 0; g0 < a.ncols; g0 += cstd::Tdfa::kGroupBatch) {
            int gb[cstd::Tdfa::kGroupBatch], ge[cstd::Tdfa::kGroupBatch], mend = 0;
            const int cnt = min(cstd::Tdfa::kGroupBatch, a.ncols - g0);
            // (backwards from the match where that applies -- short ASCII matches: regex_tdfa.h -- else the forward run)
            int got = -1;
            if (!UNITS && hit) got = vm.group_find_back(mb, a.gtags, g0 + 1, cnt, gb, ge, mend, cstd::Tdfa::HistBytes{reinterpret_cast<uint8_t*>(xbitmap) + lane, 64});
            if (hit && got < 0) got = vm.group_find_all(mb, a.gtags, g0 + 1, cnt, gb, ge, mend);
            const bool found = hit && got > 0;
#pragma unroll
            for (int k = 0; k < cstd::Tdfa::kGroupBatch; ++k)
              if (k < cnt) {
                const bool ok = found && gb[k] >= 0 && ge[k] > gb[k];
                if (a.spans) {
                  a.spans[(long long)(g0 + k) * in.rows + r0 + lane] = ok ? (((uint32_t)gb[k] << 16) | (uint32_t)(ge[k] - gb[k])) : 0xFFFFFFFFu;
                } else {
                  a.begins[(long long)(g0 + k) * in.rows + r0 + lane] = ok ? gb[k] : 0;
                  a.lens[(long long)(g0 + k) * in.rows + r0 + lane] = ok ? ge[k] - gb[k] : -1;
                }
                if (a.tile_tot && ok) __hip_atomic_fetch_add(gtot + g0 + k, (uint32_t)(ge[k] - gb[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
              }
          }
        } else {
          for (int g = 0; g < a.ncols; ++g) {
            int x = -1, y = -1;
            const bool ok = hit && vm.group_find(mb, a.gtags, g + 1, x, y) && x >= 0 && y > x;
            if (a.tile_tot && ok) __hip_atomic_fetch_add(gtot + g, (uint32_t)(y - x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if (a.spans) {
              a.spans[(long long)g * in.rows + r0 + lane] = ok ? (((uint32_t)x << 16) | (uint32_t)(y - x)) : 0xFFFFFFFFu;
            } else {
              a.begins[(long long)g * in.rows + r0 + lane] = ok ? x : 0;
              a.lens[(long long)g * in.rows + r0 + lane] = ok ? y - x : -1;
            }
          }
        }
      }
      }  // (!chain_done)
      if (a.tile_tot) {  // the bytes this tile gives to each group's column (summed in LDS by the row lanes above)
        cstile::wave_lds_fence();
        if (lane < a.ncols) {
          a.tile_tot[(long long)lane * a.nsub + tile] = (int32_t)gtot[lane];
          gtot[lane] = 0;
        }
        cstile::wave_lds_fence();
      }
    } else {
      cstd::Tdfa vm(D, P, lds_in + lead + rbeg, n, (lead + rbeg) & 3);
      bool hi_units = false;  // (bytes >= 0x80 that can only kill: the unit route alone -- reclassify_high)
      if (!CHAIN && UNITS && (MODE == 0 || MODE == 2 || MODE == 3) && has_odd && ((D.units >> 17) & 3u) && (D.units & 1u))
        hi_units = !reclassify_high(D, has_r2, lds_in, want, lane, bitmap, a.flags, lds_in + lead + rbeg, n);
      const bool lean = D.nskip > 0 && D.img[12] <= 4 && (!has_odd || hi_units) &&
                        !__any(live && (LONG ? n > cstd::Tdfa::kLongBytes : !vm.masks_fit()));
      bool redo = live && !lean;
      int k = 0;  // MODE 3: matches reported so far
      int cl[4] = {0, 0, 0, 0};  // (packed spans: the lengths of the row's first four matches, for the tile's column totals)
      auto span = [&](int mb, int me, int) {
        if (k < a.ncols) {
          if (a.spans) {
            a.spans[(long long)k * in.rows + r0 + lane] = ((uint32_t)mb << 16) | (uint32_t)(me - mb);
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (c == k) cl[c] = me - mb;
          } else {
            a.begins[(long long)k * in.rows + r0 + lane] = mb;
            a.lens[(long long)k * in.rows + r0 + lane] = me - mb;
          }
        }
        ++k;
      };
      bool units_done = false;
      if (UNITS && MODE == 3) {
        // findall: the units leave each match's first and last byte in the two bitmaps (as in the replace kernel);
        // the row lanes read their matches back in order
        if (lean && !has_odd && (D.chain >> 16)) {  // (wave-uniform) a chain pattern on plain ASCII: regex_tdfa.h, chain_match
          using namespace cstd;
          uint32_t r0, r1, r2, x0 = 0, x1 = 0, x2 = 0;
          cstile::row_bits96(bitmap, lead + rbeg, n, r0, r1, r2);
          if (unit_x != 0) cstile::row_bits96(xbitmap, lead + rbeg, n, x0, x1, x2);
          if (live) {
            U128 S, E;
            chain_match96(r0, r1, r2, x0, x1, x2, D.chain, D.img, S, E, D.sfx, n, [&](int i) { return lds_in[lead + rbeg + i]; });
            while (u128_any(S)) {
              const int mb = u128_ctz(S), me = u128_ctz(E) + 1;
              S = u128_clear_lowest(S);
              E = u128_clear_lowest(E);
              span(mb, me, 0);
            }
            v = k;
          }
          redo = false;
          units_done = true;
        } else if (!CHAIN && lean && (D.units & 1u)) {  // (wave-uniform)
          using namespace cstd;
          uint32_t m0, m1, m2;
          const int total_units = unit_discover(D, bitmap, xbitmap, lead + rbeg, n, lane, uqueue, m0, m1, m2, [&] {
            for (int i = lane * 16; i < bm_bytes; i += 64 * 16) {
              *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(bitmap) + i) = make_uint4(0, 0, 0, 0);
              *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(xbitmap) + i) = make_uint4(0, 0, 0, 0);
            }
            if (lane < 2) bailw[lane] = 0;
          });
          if (total_units >= 0) {
            for (int u0 = 0; u0 < total_units; u0 += 64) {
              const bool act = u0 + lane < total_units;
              int r, rbeg_r, n_r;
              uint32_t c0, c1, c2;
              unit_take(act ? uqueue[u0 + lane] : 0u, rbeg, n, m0, m1, m2, r, rbeg_r, n_r, c0, c1, c2, hi_units);
              if (act) {
                const int pu = lead + rbeg_r;
                cstd::Tdfa vu(D, P, lds_in + pu, n_r, pu & 3);
                bool ubail = false;
                auto recu = [&](int mb, int me, int) {
                  const int ps = pu + mb, pe = pu + me - 1;
                  __hip_atomic_fetch_or(bitmap + (ps >> 5), 1u << (ps & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                  __hip_atomic_fetch_or(xbitmap + (pe >> 5), 1u << (pe & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                };
                vu.scan_lean_dispatch(-1, c0, c1, c2, recu, ubail);
                if (ubail) __hip_atomic_fetch_or(bailw + (r >> 5), 1u << (r & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
              }
            }
            cstile::wave_lds_fence();
            uint32_t s0, s1, s2, e0, e1, e2;
            cstile::row_bits96(bitmap, lead + rbeg, n, s0, s1, s2);
            cstile::row_bits96(xbitmap, lead + rbeg, n, e0, e1, e2);
            const bool rbail = ((bailw[lane >> 5] >> (lane & 31)) & 1u) != 0;
            if (live && !rbail) {
              U128 S = u128(s0 | ((unsigned long long)s1 << 32), s2), E = u128(e0 | ((unsigned long long)e1 << 32), e2);
              while (u128_any(S)) {
                const int mb = u128_ctz(S), me = u128_ctz(E) + 1;
                S = u128_clear_lowest(S);
                E = u128_clear_lowest(E);
                span(mb, me, 0);
              }
              v = k;
            }
            redo = live && rbail;  // (such a row is scanned whole)
            units_done = true;
          }
        }
      } else if (UNITS) {
        // (contains_re stops at a row's first match: its ASCII tiles keep the row lanes' scan -- scanning every unit cost more
        // than the balance won --, the unit route serves its tiles with bytes >= 0x80, which the row lanes' scan cannot take)
        if (BITS && !has_odd && !__any(live && n > csbits::kMaxRowBytes)) {  // (wave-uniform) plain ASCII, rows within the masks
          using namespace cstd;
          auto cls = CS_BITS_CLS(bitmap, bm_bytes >> 2, lead + rbeg, n);
          auto raw = CS_BITS_RAW(bitmap, bm_bytes >> 2, lead + rbeg);
          if (MODE == 0) {
            v = live && csbits::contains(BV, cls, raw, n) ? 1 : 0;
          } else {
            U128 S = u128(0, 0), E;
            if (live) csbits::match(BV, cls, raw, n, S, E);
            v = u128_popc(S);
          }
          redo = false;
          units_done = true;
        } else if (!BITS && lean && !has_odd && (D.chain >> 16)) {  // (wave-uniform) a chain pattern on plain ASCII: regex_tdfa.h, chain_match
          using namespace cstd;
          uint32_t r0, r1, r2, x0 = 0, x1 = 0, x2 = 0;
          cstile::row_bits96(bitmap, lead + rbeg, n, r0, r1, r2);
          if (unit_x != 0) cstile::row_bits96(xbitmap, lead + rbeg, n, x0, x1, x2);
          const U128 R = u128(r0 | ((unsigned long long)r1 << 32), r2), X = u128(x0 | ((unsigned long long)x1 << 32), x2);
          if (MODE == 0 && !(D.chain & kChainLeadB)) {  // (a `\b` in front of the chain is checked per match: chain_match)
            v = live && u128_any(chain_suffix_filter(chain_ends(R, X, D.chain, D.img), D.chain, D.sfx, n, [&](int i) { return lds_in[lead + rbeg + i]; })) ? 1 : 0;
          } else if (MODE == 0) {
            U128 S = u128(0, 0), E;
            if (live) chain_match96(r0, r1, r2, x0, x1, x2, D.chain, D.img, S, E, D.sfx, n, [&](int i) { return lds_in[lead + rbeg + i]; });
            v = u128_any(S) ? 1 : 0;
          } else {
            U128 S = u128(0, 0), E;
            if (live) chain_match96(r0, r1, r2, x0, x1, x2, D.chain, D.img, S, E, D.sfx, n, [&](int i) { return lds_in[lead + rbeg + i]; });
            v = u128_popc(S);
          }
          redo = false;
          units_done = true;
        } else if (!CHAIN && lean && (D.units & 1u) && (MODE != 0 || hi_units)) {  // (wave-uniform)
          constexpr int KIND = MODE == 0 ? cstd::Tdfa::K_CONTAINS : cstd::Tdfa::K_COUNT;
          uint32_t m0, m1, m2;
          const int total_units = unit_discover(D, bitmap, xbitmap, lead + rbeg, n, lane, uqueue, m0, m1, m2, [&] {
            rowres[lane] = 0;
            if (lane < 2) bailw[lane] = 0;
          });
          if (total_units >= 0) {
            for (int u0 = 0; u0 < total_units; u0 += 64) {
              const bool act = u0 + lane < total_units;
              int r, rbeg_r, n_r;
              uint32_t c0, c1, c2;
              unit_take(act ? uqueue[u0 + lane] : 0u, rbeg, n, m0, m1, m2, r, rbeg_r, n_r, c0, c1, c2, hi_units);
              if (act) {
                const int pu = lead + rbeg_r;
                cstd::Tdfa vu(D, P, lds_in + pu, n_r, pu & 3);
                const int got = vu.template scan_lean_count<KIND>(c0, c1, c2);
                if (got < 0) __hip_atomic_fetch_or(bailw + (r >> 5), 1u << (r & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                else if (got > 0 && MODE == 0) __hip_atomic_fetch_or(rowres + r, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                else if (got > 0) __hip_atomic_fetch_add(rowres + r, (uint32_t)got, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
              }
            }
            cstile::wave_lds_fence();
            v = live ? (int)rowres[lane] : 0;
            redo = live && ((bailw[lane >> 5] >> (lane & 31)) & 1u) != 0;  // (such a row is scanned whole)
            units_done = true;
          }
        }
      }
      if (hi_units && !units_done) redo = live;  // (never the lean scan over whole rows of such a tile)
      if (CHAIN && !units_done) redo = live;       // (the generic scan)
      if (!CHAIN && !units_done && lean && !hi_units && live) {
        uint32_t m0, m1, m2;
        constexpr int KIND = MODE == 0 ? cstd::Tdfa::K_CONTAINS : cstd::Tdfa::K_COUNT;
        if (LONG) {
          const int p0 = lead + rbeg;
          cstile::row_bits96(bitmap, p0, min(n, 96), m0, m1, m2);
          auto refill = [&](int wb, uint32_t& x0, uint32_t& x1, uint32_t& x2) {
            cstile::row_bits96(bitmap, p0 + wb, min(n - wb, 96), x0, x1, x2);
          };
          if (MODE == 3) v = vm.scan_lean_spans_long(m0, m1, m2, span, refill);
          else v = vm.template scan_lean_count_long<KIND>(m0, m1, m2, refill);
        } else {
          cstile::row_bits96(bitmap, lead + rbeg, n, m0, m1, m2);
          if (MODE == 3) v = vm.scan_lean_spans(m0, m1, m2, span);
          else v = vm.template scan_lean_count<KIND>(m0, m1, m2);
        }
        redo = v < 0;
      }
      // (count_re / findall: a cold path, and saying so straightens the hot one -- findall 6.3 -> 5.7 ms; contains_re measured
      // slower with the hint, 2.09 -> 2.22, and keeps the plain branch)
      if ((MODE == 2 || MODE == 3) ? __builtin_expect(__any(redo), 0) : __any(redo)) {
        if (redo) {
          if (MODE == 3) {
            k = 0;  // (the spans reported so far are written again, identically)
#pragma unroll
            for (int c = 0; c < 4; ++c) cl[c] = 0;
            v = csvm::row_findall(vm, [&](int, int mb, int me) {
              span(mb, me, 1);
              return true;
            });
          } else {
            v = MODE == 2 ? csvm::row_count_re(vm) : csvm::row_contains_re(vm, false);
          }
        }
      }
      if (MODE == 3 && lane < nrows) {
        if (a.spans)
          for (int j = live ? k : 0; j < a.ncols; ++j) a.spans[(long long)j * in.rows + r0 + lane] = 0xFFFFFFFFu;
        else
          for (int j = live ? k : 0; j < a.ncols; ++j) a.lens[(long long)j * in.rows + r0 + lane] = -1;
      }
      if (MODE == 3 && a.tile_tot) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < a.ncols) {
            // (most tiles give the later columns nothing: no reduction then)
            const int t = __any(live && k > c) ? wave_reduce_sum(live ? cl[c] : 0) : 0;
            if (lane == 0) a.tile_tot[(long long)c * a.nsub + tile] = t;
          }
        // (columns beyond the fourth -- rows with many matches, `[a-z]+` on log lines: eighteen --: no registers kept their lengths;
        // every lane reads its own spans back, just written, and the wave adds them up.  The exact-width pass then leaves packed
        // spans and tile totals like the provisional one, where it used to write begins / lens for a scan over the lengths of
        // every column: findall([a-z]+) on the C3 column 31.8 ms)
        for (int c = 4; c < a.ncols; ++c) {
          int t = 0;
          if (__any(live && k > c)) {  // (wave-uniform)
            const uint32_t w = (live && k > c) ? a.spans[(long long)c * in.rows + r0 + lane] : 0u;
            t = wave_reduce_sum((int)(w & 0xFFFFu));
          }
          if (lane == 0) a.tile_tot[(long long)c * a.nsub + tile] = t;
        }
      }
      if (MODE == 3 && a.maxp) {
        int m = live ? k : 0;
        for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
        // (only a wave that would raise the maximum issues the same-address atomic)
        if (lane == 0 && m > __hip_atomic_load(a.maxp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.maxp, m);
      }
    }
    if (lane < nrows) {
      if (MODE == 2 || MODE == 9) a.out32[r0 + lane] = v;
      else if (MODE == 0 || MODE == 1 || MODE == 7 || MODE == 8) a.out8[r0 + lane] = (uint8_t)v;
    }
    hits += v > 0;
    cstile::wave_lds_fence();  // the next tile overwrites lds_in
    if (!has_next) break;
    ++tile;
    nxt = nn;
  }
  if (kDefer && npend > 0) flush_pend();
  const int t = wave_reduce_sum(hits);
  if (lane == 0 && t) atomicAdd(a.found, (unsigned long long)t);
}

}  // namespace
