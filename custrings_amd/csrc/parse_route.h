// The parse route (string -> one value per row): cs_convert.hip (hash / stoi / ... / to_bools), cs_datetime.hip
// (timestamp2long), cs_chartype.hip (the predicates) and cs_textops.hip (stemmer measure, bit-vector edit distance)
// each instantiate it with a per-row parser, in their own translation unit (the numeric parsers are built with
// -ffp-contract=off).  A parser P is a functor
//   using T = <result type>;
//   __device__ T operator()(const uint8_t* p, int n, bool valid) const;  // row bytes [p, p + n); valid false = null row
// passed by value in the kernel arguments with its state (the true string of to_bools, the timestamp program).
// Two routes:
//  - tile: a wave stages the bytes of R = 64 / 32 / 16 consecutive rows in LDS with one coalesced prefetch
//    (cstile::RowTileWalk: the next tile's bytes in flight while this one is parsed), each lane parses its row out of
//    LDS and the wave stores its R results side by side.  Taken when every R-row tile of the column fits the prefetch.
//  - rows: a thread per row reading its bytes from memory (columns no tile size fits -- rows of several KB -- and
//    the caller's row-wise switch: CS_CONVERT_ROWWISE=1, CS_TEXT_ROWWISE=1).
//  Both count the non-zero results with one atomic per workgroup (see k_len, cs_array.hip).
// A parser may declare two more things (cs_textops.hip does):
//   static constexpr int kSharedBytes = <n>;  // LDS filled once per workgroup by `stage(lds, tid)` in front of the staged
//                                             // rows and handed to `operator()(p, n, valid, shared)`; tile route only
//   static constexpr bool kCounted = false;   // nobody asks for the count: no reduction, no atomic
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "cs_internal.h"
#include "device_utils.h"
#include "tile_utils.h"

namespace csparse {

using cs::ColView;

using cstile::SharedBytes;
template <class P, class = void>
struct Counted : std::true_type {};
template <class P>
struct Counted<P, std::void_t<decltype(P::kCounted)>> : std::integral_constant<bool, P::kCounted> {};

template <class P>
struct ParseArgs {
  ColView in;
  typename P::T* out;
  unsigned long long* nonzero;
  int rows_per_tile, cap;  // tile route
  long long ntiles;
  P parse;
};

// the parser on a row; `shared`: its LDS region (nullptr on the row-wise route)
template <class P>
__device__ __forceinline__ typename P::T parse_row(const P& parse, const uint8_t* p, int n, bool valid, const uint8_t* shared) {
  if constexpr (SharedBytes<P>::value != 0) return parse(p, n, valid, shared);
  else return parse(p, n, valid);
}
template <class P>
__device__ __forceinline__ void add_nonzero(const ParseArgs<P>& a, long long v) {
  if constexpr (Counted<P>::value) {
    const long long t = csdev::block_reduce_sum_ll(v);
    if (threadIdx.x == 0 && t) atomicAdd(a.nonzero, (unsigned long long)t);
  }
}

template <class P>
__global__ void __launch_bounds__(256) k_parse_rows(ParseArgs<P> a) {
  using T = typename P::T;
  long long v = 0;
  csdev::for_each_row(a.in, [&](int64_t r, const uint8_t* p, int n, bool ok) {
    const T x = parse_row(a.parse, p, n, ok, nullptr);
    a.out[r] = x;
    v += x != (T)0;
  });
  add_nonzero(a, v);
}

// A wave per R-row tile, persistent over a contiguous run of tiles (every wave reaches the reduction at the end).
template <class P>
__global__ void __launch_bounds__(256) k_parse_tile(ParseArgs<P> a) {
  using T = typename P::T;
  constexpr int kShared = SharedBytes<P>::value;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint8_t* shared = reinterpret_cast<uint8_t*>(smem);
  uint8_t* lds_in = shared + kShared + (size_t)wv * a.cap;
  if constexpr (kShared != 0) {
    a.parse.stage(shared, (int)threadIdx.x);
    __syncthreads();
  }
  long long v = 0;
  // (every tile's span fits the staging buffer: checked by the host)
  cstile::walk_staged_tiles<cstile::Oversize::kHostChecked>(a.in, a.rows_per_tile, a.ntiles, lds_in, a.cap, wv, lane,
                                                            [&](const cstile::RowTile& cur, const uint8_t* p) {
    if (!cur.in_tile) return;
    const T x = parse_row(a.parse, p, cur.n, cur.live, shared);
    a.out[cur.r0 + lane] = x;
    v += x != (T)0;
  });
  add_nonzero(a, v);
}

// The launch, results to device memory; `tiles`: the tile route may be taken (the family's row-wise switch is off and
// the parser works out of LDS).  Returns true when it was.
template <class P>
bool launch_parse(const cs_column* col, const P& parse, typename P::T* d_out, unsigned long long* nonzero, bool tiles, hipStream_t s) {
  ParseArgs<P> a{};
  a.in = cs::view_of(col);
  a.out = d_out;
  a.nonzero = nonzero;
  a.parse = parse;
  const cs::StagedTiles t = tiles ? cs::plan_staged_tiles(col, cstile::kStageSlack, false, {1, 0, 150 * 1024}, s) : cs::StagedTiles{};
  cs::note_route(t.R ? "tile" : "rows");
  if (t.R) {
    a.rows_per_tile = t.R;
    a.cap = t.cap;
    a.ntiles = t.ntiles;
    cs::launch_resident(&k_parse_tile<P>, SharedBytes<P>::value + t.lds, t.grid, s, a);
    return true;
  }
  hipLaunchKernelGGL(k_parse_rows<P>, dim3(std::min(cs::blocks_for(col->rows), 8192u)), dim3(csdev::kBlock), 0, s, a);
  CS_HIP(hipGetLastError());
  return false;
}

// results to the caller's buffer (device or host); returns the count of non-zero results (0 for a parser that is not counted)
template <class P>
int64_t run_parse(const cs_column* col, const P& parse, void* results, int on_device, bool tiles, hipStream_t s) {
  using T = typename P::T;
  const cs::ResultsOut res(results, sizeof(T) * (size_t)col->rows, on_device, s);
  const cs::Buf acc = Counted<P>::value ? cs::zeroed_count(s) : nullptr;
  launch_parse(col, parse, static_cast<T*>(res.dev), cs::ptr<unsigned long long>(acc), tiles, s);
  res.copy_back(s);
  if (Counted<P>::value) return cs::read_count(acc, s);
  CS_HIP(hipStreamSynchronize(s));
  return 0;
}

// the format ops' input validity: LSB-first, bit = 1 valid; nullptr = all valid
__device__ __forceinline__ bool value_valid(const uint8_t* nulls, int64_t r) {
  return nulls == nullptr || ((nulls[r >> 3] >> (r & 7)) & 1);
}

}  // namespace csparse
