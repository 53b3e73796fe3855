// compute_statistics / get_info (reference: cpp/src/strings/NVStrings.cu:604-775): every length, memory and class figure of
// a column and its 64 K-bin character histogram from ONE read of the chars.  The per-row logic is stats_ops.h
// (walk_row), shared with the CPU harness of tests/test_stats_cpu.py.
//
// Two routes, as parse_route.h has them:
//  - tile: persistent waves stage R = 64 / 32 / 16 rows in LDS (cstile::walk_staged_tiles: the next tile's bytes in flight)
//    and a lane walks its row out of LDS;
//  - rows: a thread per row from memory, for the columns no tile size fits (rows of several KB).
// Either way a lane keeps the sums, the non-zero minima, the maxima, the null / empty counts and the class counts in
// registers over all of its rows; they are reduced per wave (shuffles), per workgroup (LDS) and end in ONE set of 64-bit
// global atomics per workgroup into a block of kSlots words.  Nothing column-sized is written.
// Histogram: code points below kLdsBins are counted in LDS and flushed once per workgroup with 32-bit global atomic adds of
// the non-zero bins; the others go straight to the 64 K x uint32 table in device memory.  The layouts (the switch
// CS_STATS_HIST: 1 the product's, 2 and 3 the measured alternatives) are described at HistSink.  k_stats_compact then turns
// the table into (packed character, count) pairs in code-point order, so that only the occupied pairs travel to the host.
// The distinct count is the key count of the category build (cs_category.hip), which is dropped at once.
#include <hip/hip_runtime.h>

#include "cs_internal.h"
#include "device_utils.h"
#include "stats_ops.h"
#include "tile_utils.h"

using namespace cs;
using namespace csdev;

namespace {

// code points below this are counted in LDS (1- and 2-byte characters: 8 KB of bins a workgroup)
constexpr int kLdsBins = 0x800;
constexpr int kTableBins = 0x10000;

// the result block: sums, then maxima, then the minima over the non-zero values (all ones: none yet)
enum Slot { S_BYTES = 0, S_CHARS, S_MEM, S_NULLS, S_EMPTY, S_SPACE, S_DIGIT, S_UPPER, S_LOWER, kSums,
            S_BMAX = kSums, S_CMAX, S_MMAX, kMaxEnd, S_BMIN = kMaxEnd, S_CMIN, S_MMIN, kSlots };

struct Acc {
  unsigned long long v[kSlots];
  __device__ __forceinline__ Acc() {
#pragma unroll
    for (int k = 0; k < kSlots; ++k) v[k] = k < kMaxEnd ? 0ull : ~0ull;
  }
  __device__ __forceinline__ void fold(int k, unsigned long long x) {
    v[k] = k < kSums ? v[k] + x : k < kMaxEnd ? max(v[k], x) : min(v[k], x);
  }
  __device__ __forceinline__ void row(bool live, int n, const csstat::RowStats& st) {
    if (!live) {
      v[S_NULLS] += 1;
      return;
    }
    const unsigned long long b = (unsigned)n, c = (unsigned)st.chars, m = csstat::row_mem(n, st.chars);
    v[S_BYTES] += b;
    v[S_CHARS] += c;
    v[S_MEM] += m;
    v[S_EMPTY] += n == 0;
    v[S_SPACE] += (unsigned)st.space;
    v[S_DIGIT] += (unsigned)st.digit;
    v[S_UPPER] += (unsigned)st.upper;
    v[S_LOWER] += (unsigned)st.lower;
    v[S_BMAX] = max(v[S_BMAX], b);
    v[S_CMAX] = max(v[S_CMAX], c);
    v[S_MMAX] = max(v[S_MMAX], m);
    if (b) v[S_BMIN] = min(v[S_BMIN], b);
    if (c) v[S_CMIN] = min(v[S_CMIN], c);
    v[S_MMIN] = min(v[S_MMIN], m);  // (a live row's figure is 9 at least)
  }
};

// wave (shuffles) -> workgroup (LDS) -> one set of atomics: thread k < kSlots adds / maxes / mins slot k
__device__ __forceinline__ void reduce_and_publish(Acc& a, unsigned long long* __restrict__ result) {
  __shared__ unsigned long long part[kMaxWaves][kSlots];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwaves = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int k = 0; k < kSlots; ++k) {
    unsigned long long x = a.v[k];
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned long long y = __shfl_xor(x, d, 64);
      x = k < kSums ? x + y : k < kMaxEnd ? max(x, y) : min(x, y);
    }
    if (lane == 0) part[wv][k] = x;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= kSlots) return;
  unsigned long long x = part[0][k];
  for (int w = 1; w < nwaves; ++w) {
    const unsigned long long y = part[w][k];
    x = k < kSums ? x + y : k < kMaxEnd ? max(x, y) : min(x, y);
  }
  if (k < kSums) {
    if (x) atomicAdd(result + k, x);
  } else if (k < kMaxEnd) {
    if (x) atomicMax(result + k, x);
  } else if (x != ~0ull) {
    atomicMin(result + k, x);
  }
}

// The histogram's counting step.  HIST:
//   0  no histogram
//   1  bins [0, kLdsBins) once per WORKGROUP in LDS, one LDS atomic a character (the product's)
//   2  the same bins once per WAVE (four sets a workgroup): a quarter of the lanes on a hot bin, four times the LDS
//   3  layout 1 behind a wave-level step: the lanes whose character equals the first active lane's add once, together
// (text is skewed -- most lanes of a log column meet a blank in the same step -- and same-address LDS atomics serialise:
// DESIGN.md section 4j has the times of all three)
template <int HIST>
struct HistSink {
  uint32_t* bins;   // LDS
  uint32_t* table;  // device memory, kTableBins counters
  __device__ __forceinline__ void operator()(unsigned cp) const {
    if constexpr (HIST == 0) return;
    if constexpr (HIST == 3) {
      const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)cp);
      const unsigned long long same = __ballot(cp == first);
      if (cp == first) {
        if ((int)(threadIdx.x & 63) != __ffsll((long long)same) - 1) return;
        const unsigned n = (unsigned)__popcll(same);
        if (cp < (unsigned)kLdsBins) atomicAdd(bins + cp, n);
        else atomicAdd(table + cp, n);
        return;
      }
    }
    if (cp < (unsigned)kLdsBins) atomicAdd(bins + cp, 1u);
    else atomicAdd(table + cp, 1u);
  }
};
template <int HIST>
constexpr int hist_sets() { return HIST == 0 ? 0 : HIST == 2 ? 4 : 1; }
template <int HIST>
constexpr size_t hist_lds_bytes() { return (size_t)hist_sets<HIST>() * kLdsBins * sizeof(uint32_t); }

template <int HIST>
__device__ __forceinline__ void hist_clear(uint32_t* bins) {
  if constexpr (HIST != 0) {
    for (int i = threadIdx.x; i < hist_sets<HIST>() * kLdsBins; i += blockDim.x) bins[i] = 0;
    __syncthreads();
  }
}
// (every thread of the workgroup arrives here)
template <int HIST>
__device__ __forceinline__ void hist_flush(const uint32_t* bins, uint32_t* __restrict__ table) {
  if constexpr (HIST != 0) {
    __syncthreads();
    for (int i = threadIdx.x; i < kLdsBins; i += blockDim.x) {
      uint32_t n = 0;
#pragma unroll
      for (int k = 0; k < hist_sets<HIST>(); ++k) n += bins[k * kLdsBins + i];
      if (n) atomicAdd(table + i, n);
    }
  }
}

struct StatsArgs {
  ColView in;
  csstat::ClassSpec classes;
  unsigned long long* result;  // kSlots words
  uint32_t* table;             // kTableBins counters (histogram only)
  int rows_per_tile, cap;      // tile route
  long long ntiles;
};

template <bool CLASSES, int HIST>
__global__ void __launch_bounds__(256) k_stats_tile(StatsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint32_t* bins = smem;
  uint8_t* lds_in = reinterpret_cast<uint8_t*>(smem) + hist_lds_bytes<HIST>() + (size_t)wv * a.cap;
  hist_clear<HIST>(bins);
  const HistSink<HIST> sink{bins + (HIST == 2 ? wv * kLdsBins : 0), a.table};
  Acc acc;
  // (every tile's span fits the staging buffer: checked by the host)
  cstile::walk_staged_tiles<cstile::Oversize::kHostChecked>(a.in, a.rows_per_tile, a.ntiles, lds_in, a.cap, wv, lane,
                                                            [&](const cstile::RowTile& cur, const uint8_t* p) {
    if (!cur.in_tile) return;
    acc.row(cur.live, cur.n, csstat::walk_row<CLASSES>(p, cur.n, a.classes, sink));
  });
  hist_flush<HIST>(bins, a.table);
  reduce_and_publish(acc, a.result);
}

template <bool CLASSES, int HIST>
__global__ void __launch_bounds__(256) k_stats_rows(StatsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = threadIdx.x >> 6;
  uint32_t* bins = smem;
  hist_clear<HIST>(bins);
  const HistSink<HIST> sink{bins + (HIST == 2 ? wv * kLdsBins : 0), a.table};
  Acc acc;
  for_each_row(a.in, [&](int64_t, const uint8_t* p, int n, bool ok) { acc.row(ok, n, csstat::walk_row<CLASSES>(p, n, a.classes, sink)); });
  hist_flush<HIST>(bins, a.table);
  reduce_and_publish(acc, a.result);
}

// The table as (packed character, count) pairs in code-point order: one workgroup of 1024 threads, 64 bins a thread.
// Code point 0 is never listed.  pairs[2 i], pairs[2 i + 1]; *npairs the count.
__global__ void __launch_bounds__(1024) k_stats_compact(const uint32_t* __restrict__ table, uint32_t* __restrict__ pairs,
                                                        unsigned long long* __restrict__ npairs) {
  constexpr int kPer = kTableBins / 1024;
  const int first = (int)threadIdx.x * kPer;
  int mine = 0;
  for (int i = 0; i < kPer; ++i) mine += (first + i) != 0 && table[first + i] != 0;
  long long total;
  long long at = block_exclusive_scan(mine, &total);
  for (int i = 0; i < kPer; ++i) {
    const uint32_t n = table[first + i];
    if ((first + i) != 0 && n != 0) {
      pairs[2 * at] = csrow::cp_to_packed((unsigned)(first + i));
      pairs[2 * at + 1] = n;
      ++at;
    }
  }
  if (threadIdx.x == 0) *npairs = (unsigned long long)total;
}

template <bool CLASSES, int HIST>
void launch_pass(const cs_column* col, StatsArgs a, hipStream_t s) {
  const StagedTiles t = plan_staged_tiles(col, cstile::kStageSlack, false, {1, hist_lds_bytes<HIST>() / 4, 150 * 1024}, s);
  note_route(t.R ? "tile" : "rows");
  if (t.R) {
    a.rows_per_tile = t.R;
    a.cap = t.cap;
    a.ntiles = t.ntiles;
    launch_resident(&k_stats_tile<CLASSES, HIST>, t.lds, t.grid, s, a);
    return;
  }
  hipLaunchKernelGGL((k_stats_rows<CLASSES, HIST>), dim3(std::min(blocks_for(col->rows), 8192u)), dim3(kBlock), hist_lds_bytes<HIST>(), s, a);
  CS_HIP(hipGetLastError());
}
template <bool CLASSES>
void launch_pass(const cs_column* col, const StatsArgs& a, int hist, hipStream_t s) {
  switch (hist) {
    case 0: return launch_pass<CLASSES, 0>(col, a, s);
    case 2: return launch_pass<CLASSES, 2>(col, a, s);
    case 3: return launch_pass<CLASSES, 3>(col, a, s);
    default: return launch_pass<CLASSES, 1>(col, a, s);
  }
}

// one cs_column_statistics call, all of its parameters in sight
struct StatsCall {
  const cs_column* col;
  int what;
  cs_statistics* out;
  uint32_t* pairs;
  int64_t pairs_cap;
  int64_t* npairs;
  int on_device;
  hipStream_t s;
};

// the fused pass; fills the figures of `what` and returns the table (null without the histogram)
Buf run_pass(const StatsCall& c) {
  const bool hist = (c.what & CS_STATS_HISTOGRAM) != 0, classes = (c.what & CS_STATS_CLASSES) != 0;
  StatsArgs a{};
  a.in = view_of(c.col);
  a.classes = csstat::make_classes(h_unicode_flags(), d_unicode_flags());
  const Buf result = dev_alloc(sizeof(unsigned long long) * kSlots, c.s);
  CS_HIP(hipMemsetAsync(result->p, 0, sizeof(unsigned long long) * kMaxEnd, c.s));
  CS_HIP(hipMemsetAsync(ptr<unsigned long long>(result) + kMaxEnd, 0xFF, sizeof(unsigned long long) * (kSlots - kMaxEnd), c.s));
  a.result = ptr<unsigned long long>(result);
  Buf table;
  if (hist) {
    table = dev_alloc(sizeof(uint32_t) * kTableBins, c.s);
    CS_HIP(hipMemsetAsync(table->p, 0, sizeof(uint32_t) * kTableBins, c.s));
    a.table = ptr<uint32_t>(table);
  }
  const int layout = hist ? std::max(1, std::min(3, cfg_int("CS_STATS_HIST", 1))) : 0;
  {
    ProfScope ps("k_stats", c.s);
    if (classes) launch_pass<true>(c.col, a, layout, c.s);
    else launch_pass<false>(c.col, a, layout, c.s);
  }
  unsigned long long* h = (unsigned long long*)pinned_scratch(sizeof(unsigned long long) * kSlots);
  CS_HIP(hipMemcpyAsync(h, result->p, sizeof(unsigned long long) * kSlots, hipMemcpyDeviceToHost, c.s));
  CS_HIP(hipStreamSynchronize(c.s));
  cs_statistics* o = c.out;
  const uint64_t rows = (uint64_t)c.col->rows;
  if (c.what & CS_STATS_LENGTHS) {
    o->total_bytes = h[S_BYTES];
    o->total_chars = h[S_CHARS];
    o->total_nulls = h[S_NULLS];
    o->total_empty = h[S_EMPTY];
    o->bytes_avg = h[S_BYTES] / rows;
    o->chars_avg = h[S_BYTES] / rows;  // (the reference divides the BYTES here too: NVStrings.cu:679)
    o->mem_avg = h[S_MEM] / rows;
    o->bytes_max = h[S_BMAX];
    o->chars_max = h[S_CMAX];
    o->mem_max = h[S_MMAX];
    o->bytes_min = h[S_BMIN] == ~0ull ? 0 : h[S_BMIN];
    o->chars_min = h[S_CMIN] == ~0ull ? 0 : h[S_CMIN];
    o->mem_min = h[S_MMIN] == ~0ull ? 0 : h[S_MMIN];
  }
  if (classes) {
    o->whitespace_count = h[S_SPACE];
    o->digits_count = h[S_DIGIT];
    o->uppercase_count = h[S_UPPER];
    o->lowercase_count = h[S_LOWER];
  }
  return table;
}

// table -> pairs in the caller's buffer; throws when it is too small (*npairs then holds the count it needs)
void hand_out_pairs(const StatsCall& c, const Buf& table) {
  const Buf packed = dev_alloc(sizeof(uint32_t) * 2 * (kTableBins - 1), c.s);
  const Buf count = zeroed_count(c.s);
  hipLaunchKernelGGL(k_stats_compact, dim3(1), dim3(1024), 0, c.s, ptr<const uint32_t>(table), ptr<uint32_t>(packed),
                     ptr<unsigned long long>(count));
  CS_HIP(hipGetLastError());
  const int64_t n = read_count(count, c.s);
  *c.npairs = n;
  if (n > c.pairs_cap) fail(CS_ERR_INVALID_ARG, "statistics: the histogram has more pairs than the caller's buffer holds");
  if (n == 0) return;
  CS_HIP(hipMemcpyAsync(c.pairs, packed->p, sizeof(uint32_t) * 2 * (size_t)n, c.on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.s));
  CS_HIP(hipStreamSynchronize(c.s));
}

// distinct rows, all nulls one value: the key count of the category build; the category is dropped here
uint64_t count_unique(const StatsCall& c) {
  const std::unique_ptr<cs_category> cat(category_build(c.col, c.s));
  return (uint64_t)cat->keys->rows;
}

}  // namespace

extern "C" {

int cs_stats_lds_bins(void) { return kLdsBins; }

int cs_column_statistics(const cs_column* col, int what, cs_statistics* out, uint32_t* pairs, int64_t pairs_cap, int64_t* npairs, int on_device,
                         cs_stream stream) {
  return guard([&] {
    const bool hist = (what & CS_STATS_HISTOGRAM) != 0;
    if (!col || !out || (hist && (!npairs || pairs_cap < 0 || (pairs_cap > 0 && !pairs)))) fail(CS_ERR_INVALID_ARG, "statistics: bad arguments");
    *out = cs_statistics{};
    if (npairs) *npairs = 0;
    const int64_t rows = col->rows;
    if (rows == 0) return;  // all zeros and no pair (NVStrings.cu:607)
    require_device();
    const StatsCall c{col, what, out, pairs, pairs_cap, npairs, on_device, S(stream)};
    out->total_strings = (uint64_t)rows;
    out->total_memory = (uint64_t)col->nbytes + (uint64_t)cs_column_offset_width(col) * (uint64_t)(rows + 1) + (uint64_t)(rows + 7) / 8;
    if (what & (CS_STATS_LENGTHS | CS_STATS_CLASSES | CS_STATS_HISTOGRAM)) {
      const Buf table = run_pass(c);
      if (hist) hand_out_pairs(c, table);
    }
    if (what & CS_STATS_UNIQUE) out->unique_strings = count_unique(c);
  });
}

}  // extern "C"
