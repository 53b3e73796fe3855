// The NVText members contains_strings / strings_counts / edit_distance / porter_stemmer_measure / scatter_count
// (reference: cpp/src/text/NVText.cu:32-172, edit_distance.cu:33-228, stemmer.cu:29-104).  The per-row logic is
// text_ops.h, shared with the CPU harness of tests/text_model.py.
//
// Two routes, those of parse_route.h, under a switch of their own (CS_TEXT_ROWWISE=1 takes the row-wise one); the ops of one
// value a row (porter_stemmer_measure, edit_distance against a short target) are parsers of that header:
//  - tile: a wave stages the bytes of R = 64 / 32 / 16 consecutive rows in LDS (cstile::RowTileWalk: the next tile's bytes
//    in flight while this one is worked on) and each lane runs its row out of LDS.  What every row needs beside its bytes
//    is copied into LDS once per workgroup: the bit-vector table of edit_distance (1792 bytes), the target column of
//    contains_strings / strings_counts (when it fits kTargetBytes / kTargetCount; beyond that the targets are read from
//    memory).  A wave's R x M block of match results is contiguous in memory: when it fits kOutTileBytes it is assembled
//    in LDS and stored side by side, else each lane stores its own M values.
//  - rows: a thread per row reading its bytes from memory (also: columns no tile size fits).
// edit_distance against one target of 1..64 characters runs Myers' bit-vector algorithm on the tile route; a longer
// target, the row-wise route and the two-column overload run the one-row dynamic program, a thread per row, its row of
// uint16 entries in a scratch buffer sized by a length pass and the shared scan (min(chars_a, chars_b) entries a row).
// scatter_count: the exclusive scan of the counts, one kernel that fills the int32 source-row map -- a thread per OUTPUT
// row bisecting the scan: the stores are coalesced and the work per thread is log2(rows) whatever the counts are, where a
// wave per source row would idle on the rows of count 0 and serialise on one of count 10^6 -- then the existing gather.
#include <hip/hip_runtime.h>

#include <cstring>

#include "cs_internal.h"
#include "device_utils.h"
#include "parse_route.h"
#include "text_ops.h"
#include "tile_utils.h"

using namespace cs;
using namespace csdev;

namespace {

constexpr int kTargetBytes = 8192;   // LDS budget of the staged target column: its bytes ...
constexpr int kTargetCount = 512;    // ... and its rows (8 bytes each)
constexpr int kOutTileBytes = 4096;  // a wave's assembled block of match results

bool rowwise() { return cfg("CS_TEXT_ROWWISE") != nullptr && std::strcmp(cfg("CS_TEXT_ROWWISE"), "0") != 0; }

StagedTiles plan(const cs_column* col, hipStream_t s) {
  return rowwise() ? StagedTiles{} : plan_staged_tiles(col, cstile::kStageSlack, false, {1, 0, 150 * 1024}, s);
}

// ---- one value a row: parsers of parse_route.h, not counted -----------------------------------------------------------------
struct MeasureParse {
  using T = uint32_t;
  static constexpr bool kCounted = false;
  cstxt::VowelSpec spec;
  __device__ __forceinline__ T operator()(const uint8_t* p, int n, bool) const { return cstxt::measure_row(p, n, spec); }
};

// the bit-vector table in LDS: ascii[128] (uint64), mask[64] (uint64), ch[64] (uint32)
constexpr int kPeqBytes = 128 * 8 + cstxt::kBitTargetChars * 8 + cstxt::kBitTargetChars * 4;
struct EditBitsParse {
  using T = uint32_t;
  static constexpr bool kCounted = false;
  static constexpr int kSharedBytes = kPeqBytes;
  const uint32_t* table;  // the same layout in device memory
  int nlist, m;
  __device__ __forceinline__ void stage(uint8_t* lds, int tid) const {
    uint32_t* w = reinterpret_cast<uint32_t*>(lds);
    for (int i = tid; i < kPeqBytes / 4; i += 256) w[i] = table[i];
  }
  __device__ __forceinline__ T operator()(const uint8_t* p, int n, bool, const uint8_t* shared) const {
    const uint64_t* ascii = reinterpret_cast<const uint64_t*>(shared);
    const uint64_t* mask = ascii + 128;
    const cstxt::Char* ch = reinterpret_cast<const cstxt::Char*>(mask + cstxt::kBitTargetChars);
    return cstxt::edit_distance_bits(p, n, ascii, ch, mask, nlist, m);
  }
};

// ---- edit_distance: the one-row dynamic program, a thread per pair -------------------------------------------------------
struct PairArgs {
  ColView in, tg;           // tg: the second column (pairs) ...
  const uint8_t* target;    // ... or one target for every row (tg.rows == 0)
  int target_bytes;
  int32_t* entries;         // the length pass: table entries per row
  const int64_t* scratch_off;
  uint16_t* scratch;
  uint32_t* out;
};
// More than 32767 characters do not fit the table's entries (the reference's `short` wraps there): refused on every route.
// The column's cached longest-row bound first; characters are counted only when some row has more BYTES than that.
__global__ void __launch_bounds__(256) k_most_chars(ColView in, int* __restrict__ most) {
  int v = 0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < in.rows; r += (int64_t)gridDim.x * kBlock) {
    if (!row_is_valid(in.validity, r)) continue;
    const int64_t o0 = in.offsets[r], n = in.offsets[r + 1] - o0;
    if (n > cstxt::kMaxChars) v = max(v, n > 0x7fffffff ? 0x7fffffff : cstxt::walk_chars(in.chars + o0, (int)n));
  }
  if (v > cstxt::kMaxChars) atomicMax(most, v);
}
void refuse_long_rows(const cs_column* col, hipStream_t s) {
  if (col->rows == 0 || max_row_bytes(col, s) <= cstxt::kMaxChars) return;
  Buf most = dev_alloc(sizeof(int), s);
  CS_HIP(hipMemsetAsync(most->p, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_most_chars, dim3(std::min(blocks_for(col->rows), 8192u)), dim3(kBlock), 0, s, view_of(col), ptr<int>(most));
  CS_HIP(hipGetLastError());
  int* host = (int*)pinned_scratch(sizeof(int));
  CS_HIP(hipMemcpyAsync(host, most->p, sizeof(int), hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  if (host[0] > cstxt::kMaxChars) fail(CS_ERR_RANGE, "nvtext: edit_distance takes at most 32767 characters a string");
}
__device__ __forceinline__ void pair_of(const PairArgs& a, int64_t r, const uint8_t*& p, int& n, bool& pv, const uint8_t*& t, int& tn, bool& tv) {
  pv = row_is_valid(a.in.validity, r);
  const int64_t o0 = a.in.offsets[r];
  p = a.in.chars + o0;
  n = pv ? (int)(a.in.offsets[r + 1] - o0) : 0;
  if (a.tg.rows == 0) {
    t = a.target, tn = a.target_bytes, tv = true;
    return;
  }
  tv = row_is_valid(a.tg.validity, r);
  const int64_t q0 = a.tg.offsets[r];
  t = a.tg.chars + q0;
  tn = tv ? (int)(a.tg.offsets[r + 1] - q0) : 0;
}
__global__ void __launch_bounds__(256) k_edit_entries(PairArgs a) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < a.in.rows; r += (int64_t)gridDim.x * kBlock) {
    const uint8_t *p, *t;
    int n, tn;
    bool pv, tv;
    pair_of(a, r, p, n, pv, t, tn, tv);
    a.entries[r] = cstxt::edit_row_entries(p, n, pv, t, tn, tv);
  }
}
__global__ void __launch_bounds__(256) k_edit_dp(PairArgs a) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < a.in.rows; r += (int64_t)gridDim.x * kBlock) {
    const uint8_t *p, *t;
    int n, tn;
    bool pv, tv;
    pair_of(a, r, p, n, pv, t, tn, tv);
    a.out[r] = cstxt::edit_distance_dp(p, n, pv, t, tn, tv, a.scratch + a.scratch_off[r]);
  }
}
void run_edit_dp(const cs_column* col, const cs_column* targets, const char* target, uint32_t* d_out, hipStream_t s) {
  const int64_t rows = col->rows;
  PairArgs a{};
  a.in = view_of(col);
  Buf tbuf;
  if (targets) {
    a.tg = view_of(targets);
  } else {
    a.target_bytes = (int)std::strlen(target);
    tbuf = dev_alloc((size_t)a.target_bytes + 1, s);
    CS_HIP(hipMemcpyAsync(tbuf->p, target, (size_t)a.target_bytes, hipMemcpyHostToDevice, s));
    a.target = ptr<const uint8_t>(tbuf);
  }
  Buf lens = dev_alloc(sizeof(int32_t) * (size_t)rows, s), offs = dev_alloc(sizeof(int64_t) * (size_t)(rows + 1), s);
  a.entries = ptr<int32_t>(lens);
  const dim3 grid(std::min(blocks_for(rows), 8192u));
  hipLaunchKernelGGL(k_edit_entries, grid, dim3(kBlock), 0, s, a);
  CS_HIP(hipGetLastError());
  const int64_t total = offsets_from_lengths(a.entries, rows, ptr<int64_t>(offs), s);
  Buf scratch = dev_alloc(sizeof(uint16_t) * (size_t)(total + 1), s);
  a.scratch_off = ptr<const int64_t>(offs);
  a.scratch = ptr<uint16_t>(scratch);
  a.out = d_out;
  hipLaunchKernelGGL(k_edit_dp, grid, dim3(kBlock), 0, s, a);
  CS_HIP(hipGetLastError());
  note_route("rows");
  CS_HIP(hipStreamSynchronize(s));  // (the scratch goes back to the pool behind this)
}
void run_edit_scalar(const cs_column* col, const char* target, uint32_t* d_out, hipStream_t s) {
  const uint8_t* t = reinterpret_cast<const uint8_t*>(target);
  const int tn = (int)std::strlen(target);
  if (cstxt::walk_chars(t, tn) > cstxt::kMaxChars) fail(CS_ERR_RANGE, "nvtext: edit_distance takes at most 32767 characters a string");
  refuse_long_rows(col, s);
  cstxt::PeqTable q;
  cstxt::build_peq(t, tn, q);
  if (!q.m || !plan(col, s).R) return run_edit_dp(col, nullptr, target, d_out, s);
  uint32_t* host = (uint32_t*)pinned_scratch(kPeqBytes);
  std::memcpy(host, q.ascii, 128 * 8);
  std::memcpy(host + 256, q.mask, cstxt::kBitTargetChars * 8);
  std::memcpy(host + 256 + 2 * cstxt::kBitTargetChars, q.ch, cstxt::kBitTargetChars * 4);
  Buf table = dev_alloc(kPeqBytes, s);
  CS_HIP(hipMemcpyAsync(table->p, host, kPeqBytes, hipMemcpyHostToDevice, s));
  CS_HIP(hipStreamSynchronize(s));  // (the pinned scratch is free again)
  csparse::launch_parse(col, EditBitsParse{ptr<const uint32_t>(table), q.nlist, q.m}, d_out, nullptr, true, s);
  CS_HIP(hipStreamSynchronize(s));
}

// ---- contains_strings / strings_counts ------------------------------------------------------------------------------------
template <class T>
struct MatchArgs {
  ColView in, tg;
  T* out;
  int M, rows_per_tile, cap, tg_bytes, out_cap;  // tg_bytes: the staged targets' bytes padded to 16 (0: read from memory)
  long long ntiles;
};
struct TargetsInMemory {
  ColView tg;
  __device__ __forceinline__ const uint8_t* get(int j, int& tn) const {
    const int64_t q0 = tg.offsets[j];
    tn = row_is_valid(tg.validity, j) ? (int)(tg.offsets[j + 1] - q0) : 0;  // (a null target matches like an empty one: never)
    return tg.chars + q0;
  }
};
struct TargetsInLds {
  const uint8_t* bytes;
  const int2* ext;  // (start, length)
  __device__ __forceinline__ const uint8_t* get(int j, int& tn) const {
    const int2 e = ext[j];
    tn = e.y;
    return bytes + e.x;
  }
};
template <class T, bool COUNT, class TG>
__device__ __forceinline__ void match_row(const uint8_t* p, int n, bool live, const TG& tg, int M, T* o) {
  for (int j = 0; j < M; ++j) {
    int tn;
    const uint8_t* t = tg.get(j, tn);
    if (COUNT) o[j] = (T)(live ? cstxt::count_row(p, n, t, tn) : 0u);
    else o[j] = (T)(live && cstxt::contains_row(p, n, t, tn));
  }
}
template <class T, bool COUNT>
__global__ void __launch_bounds__(256) k_match_rows(MatchArgs<T> a) {
  const TargetsInMemory tg{a.tg};
  for_each_row(a.in, [&](int64_t r, const uint8_t* p, int n, bool ok) { match_row<T, COUNT>(p, n, ok, tg, a.M, a.out + r * a.M); });
}
template <class T, bool COUNT, bool STAGED>
__global__ void __launch_bounds__(256) k_match_tile(MatchArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint8_t* base = reinterpret_cast<uint8_t*>(smem);
  // [targets' bytes | their (start, length) pairs] [4 x staged rows] [4 x assembled results]
  uint8_t* tg_bytes = base;
  int2* tg_ext = reinterpret_cast<int2*>(base + a.tg_bytes);
  const int tg_total = STAGED ? a.tg_bytes + ((a.M * 8 + 15) & ~15) : 0;
  uint8_t* lds_in = base + tg_total + (size_t)wv * a.cap;
  T* lds_out = reinterpret_cast<T*>(base + tg_total + (size_t)4 * a.cap + (size_t)wv * a.out_cap);
  if (STAGED) {
    const int64_t q0 = a.tg.offsets[0];
    const int nb = (int)(a.tg.offsets[a.M] - q0);
    for (int i = threadIdx.x; i < nb; i += 256) tg_bytes[i] = a.tg.chars[q0 + i];
    for (int j = threadIdx.x; j < a.M; j += 256) {
      const int64_t b = a.tg.offsets[j];
      tg_ext[j] = make_int2((int)(b - q0), row_is_valid(a.tg.validity, j) ? (int)(a.tg.offsets[j + 1] - b) : 0);
    }
    __syncthreads();
  }
  // (every tile's span fits the staging buffer: checked by the host)
  cstile::walk_staged_tiles<cstile::Oversize::kHostChecked>(a.in, a.rows_per_tile, a.ntiles, lds_in, a.cap, wv, lane,
                                                            [&](const cstile::RowTile& cur, const uint8_t* p) {
    T* o = a.out_cap ? lds_out + (size_t)lane * a.M : a.out + (cur.r0 + lane) * a.M;
    if (cur.in_tile) {
      if (STAGED) match_row<T, COUNT>(p, cur.n, cur.live, TargetsInLds{tg_bytes, tg_ext}, a.M, o);
      else match_row<T, COUNT>(p, cur.n, cur.live, TargetsInMemory{a.tg}, a.M, o);
    }
    if (a.out_cap) {  // the wave's nrows x M results lie side by side in memory
      cstile::wave_lds_fence();
      T* g = a.out + cur.r0 * a.M;
      const int total = cur.nrows * a.M;
      for (int i = lane; i < total; i += 64) g[i] = lds_out[i];
    }
  });
}
template <class T, bool COUNT>
void run_match(const cs_column* col, const cs_column* targets, T* d_out, hipStream_t s) {
  MatchArgs<T> a{};
  a.in = view_of(col);
  a.tg = view_of(targets);
  a.out = d_out;
  a.M = (int)targets->rows;
  const StagedTiles t = plan(col, s);
  if (!t.R) {
    hipLaunchKernelGGL((k_match_rows<T, COUNT>), dim3(std::min(blocks_for(col->rows), 8192u)), dim3(kBlock), 0, s, a);
    CS_HIP(hipGetLastError());
    note_route("rows");
    return;
  }
  a.rows_per_tile = t.R;
  a.cap = t.cap;
  a.ntiles = t.ntiles;
  const bool staged = targets->nbytes <= kTargetBytes && targets->rows <= kTargetCount;
  a.tg_bytes = staged ? (int)((targets->nbytes + 15) & ~(int64_t)15) : 0;
  const size_t block = sizeof(T) * (size_t)t.R * (size_t)a.M;
  a.out_cap = block <= (size_t)kOutTileBytes ? (int)((block + 15) & ~(size_t)15) : 0;
  const size_t lds = (staged ? (size_t)a.tg_bytes + (((size_t)a.M * 8 + 15) & ~(size_t)15) : 0) + t.lds + (size_t)4 * a.out_cap;
  if (staged) launch_resident(&k_match_tile<T, COUNT, true>, lds, t.grid, s, a);
  else launch_resident(&k_match_tile<T, COUNT, false>, lds, t.grid, s, a);
  note_route("tile");
}
template <class T, bool COUNT>
void match_entry(const cs_column* col, const cs_column* targets, T* results, int on_device, cs_stream stream) {
  if (!col || !targets) fail(CS_ERR_INVALID_ARG, "nvtext: bad arguments");
  if (!results || col->rows == 0 || targets->rows == 0) return;  // NVText.cu:36,81: nothing is written
  if (targets->rows > (1 << 20)) fail(CS_ERR_RANGE, "nvtext: more than 2^20 targets");
  require_device();
  const hipStream_t s = S(stream);
  const ResultsOut res(results, sizeof(T) * (size_t)col->rows * (size_t)targets->rows, on_device, s);
  run_match<T, COUNT>(col, targets, static_cast<T*>(res.dev), s);
  res.finish(s);
}

// ---- scatter_count ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sum_counts(const uint32_t* __restrict__ counts, int64_t rows, unsigned long long* __restrict__ total) {
  long long v = 0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kBlock) v += counts[r];
  const long long t = block_reduce_sum_ll(v);
  if (threadIdx.x == 0 && t) atomicAdd(total, (unsigned long long)t);
}
__global__ void __launch_bounds__(256) k_scatter_map(const int64_t* __restrict__ scan, int64_t rows, int64_t total, int32_t* __restrict__ map) {
  for (int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x; o < total; o += (int64_t)gridDim.x * kBlock)
    map[o] = (int32_t)cstxt::scatter_source(scan, rows, o);
}

}  // namespace

extern "C" {

int cs_contains_strings(const cs_column* col, const cs_column* targets, uint8_t* results, int on_device, cs_stream stream) {
  return guard([&] { match_entry<uint8_t, false>(col, targets, results, on_device, stream); });
}
int cs_strings_counts(const cs_column* col, const cs_column* targets, uint32_t* results, int on_device, cs_stream stream) {
  return guard([&] { match_entry<uint32_t, true>(col, targets, results, on_device, stream); });
}
int cs_edit_distance(const cs_column* col, const char* target, int algo, uint32_t* results, int on_device, cs_stream stream) {
  return guard([&] {
    if (!col || algo != cstxt::ALGO_LEVENSHTEIN || !target || !results) fail(CS_ERR_INVALID_ARG, "invalid algorithm");
    if (col->rows == 0) return;
    require_device();
    const hipStream_t s = S(stream);
    const ResultsOut res(results, sizeof(uint32_t) * (size_t)col->rows, on_device, s);
    run_edit_scalar(col, target, static_cast<uint32_t*>(res.dev), s);
    res.finish(s);
  });
}
int cs_edit_distance_column(const cs_column* col, const cs_column* targets, int algo, uint32_t* results, int on_device, cs_stream stream) {
  return guard([&] {
    if (!col || !targets || algo != cstxt::ALGO_LEVENSHTEIN) fail(CS_ERR_INVALID_ARG, "invalid algorithm");
    if (col->rows != targets->rows) fail(CS_ERR_INVALID_ARG, "sizes must match");
    if (col->rows == 0) return;
    if (!results) fail(CS_ERR_INVALID_ARG, "nvtext: no results array");
    require_device();
    const hipStream_t s = S(stream);
    refuse_long_rows(col, s);
    refuse_long_rows(targets, s);
    const ResultsOut res(results, sizeof(uint32_t) * (size_t)col->rows, on_device, s);
    run_edit_dp(col, targets, nullptr, static_cast<uint32_t*>(res.dev), s);
    res.finish(s);
  });
}
int cs_porter_stemmer_measure(const cs_column* col, const char* vowels, const char* y_char, uint32_t* results, int on_device, cs_stream stream) {
  return guard([&] {
    if (!col) fail(CS_ERR_INVALID_ARG, "nvtext: bad arguments");
    if (col->rows == 0 || !results) return;
    require_device();
    const hipStream_t s = S(stream);
    // the non-ASCII vowels beyond the eight the parser carries: in memory, and the column goes row-wise
    const size_t cap = std::strlen(vowels ? vowels : "") + 1;
    std::vector<cstxt::Char> overflow(cap);
    Buf more = dev_alloc(sizeof(cstxt::Char) * cap, s);
    const cstxt::VowelSpec spec = cstxt::make_vowels(vowels, y_char, overflow.data(), (int)cap, ptr<const cstxt::Char>(more));
    if (spec.nmore) CS_HIP(hipMemcpyAsync(more->p, overflow.data(), sizeof(cstxt::Char) * (size_t)spec.nmore, hipMemcpyHostToDevice, s));
    // (synchronises: `overflow` and `more` stay alive until the copy and the kernel are done)
    csparse::run_parse(col, MeasureParse{spec}, results, on_device, !rowwise() && spec.nmore == 0, s);
  });
}
int cs_scatter_count(const cs_column* col, const uint32_t* counts, int on_device, cs_stream stream, cs_column** out) {
  return guard([&] {
    if (!out) fail(CS_ERR_INVALID_ARG, "nvtext: bad arguments");
    *out = nullptr;
    if (!col) fail(CS_ERR_INVALID_ARG, "nvtext: bad arguments");
    if (col->rows == 0 || !counts) return;  // NVText.cu:129: no instance
    require_device();
    const hipStream_t s = S(stream);
    const int64_t rows = col->rows;
    Buf held;
    const uint32_t* d_counts = counts;
    if (!on_device) {
      held = dev_alloc(sizeof(uint32_t) * (size_t)rows, s);
      CS_HIP(hipMemcpyAsync(held->p, counts, sizeof(uint32_t) * (size_t)rows, hipMemcpyHostToDevice, s));
      d_counts = ptr<const uint32_t>(held);
    }
    const Buf acc = zeroed_count(s);
    hipLaunchKernelGGL(k_sum_counts, dim3(std::min(blocks_for(rows), 8192u)), dim3(kBlock), 0, s, d_counts, rows, ptr<unsigned long long>(acc));
    CS_HIP(hipGetLastError());
    const int64_t total = read_count(acc, s);
    if (total >= ((int64_t)1 << 31)) fail(CS_ERR_RANGE, "nvtext: scatter_count would make 2^31 rows or more");
    note_route("rows");
    if (total == 0) {
      *out = make_all_null(0, s);
      return;
    }
    // (every count is below 2^31 now: the scan reads them as the int32 lengths it is made for)
    Buf scan = dev_alloc(sizeof(int64_t) * (size_t)(rows + 1), s), map = dev_alloc(sizeof(int32_t) * (size_t)total, s);
    offsets_from_lengths(reinterpret_cast<const int32_t*>(d_counts), rows, ptr<int64_t>(scan), s);
    hipLaunchKernelGGL(k_scatter_map, dim3(std::min(blocks_for(total), 65536u)), dim3(kBlock), 0, s, ptr<const int64_t>(scan), rows, total, ptr<int32_t>(map));
    CS_HIP(hipGetLastError());
    *out = gather_rows(col, ptr<const int32_t>(map), total, s);
    CS_HIP(hipStreamSynchronize(s));
  });
}

}  // extern "C"
