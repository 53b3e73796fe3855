// The parse route of the conversions (string -> one value per row): cs_convert.hip (hash / stoi / ... / to_bools) and
// cs_datetime.hip (timestamp2long) each instantiate it with a per-row parser, in their own translation unit (the
// numeric parsers are built with -ffp-contract=off).  A parser P is a functor
//   using T = <result type>;
//   __device__ T operator()(const uint8_t* p, int n, bool valid) const;  // row bytes [p, p + n); valid false = null row
// passed by value in the kernel arguments with its state (the true string of to_bools, the timestamp program).
// Two routes:
//  - tile: a wave stages the bytes of R = 64 / 32 / 16 consecutive rows in LDS with one coalesced prefetch
//    (cstile::RowTileWalk: the next tile's bytes in flight while this one is parsed), each lane parses its row out of
//    LDS and the wave stores its R results side by side.  Taken when every R-row tile of the column fits the prefetch.
//  - rows: a thread per row reading its bytes from memory (columns no tile size fits -- rows of several KB -- and
//    CS_CONVERT_ROWWISE=1).
//  Both count the non-zero results with one atomic per workgroup (see k_len, cs_array.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "cs_internal.h"
#include "device_utils.h"
#include "tile_utils.h"

namespace csparse {

using cs::ColView;

template <class P>
struct ParseArgs {
  ColView in;
  typename P::T* out;
  unsigned long long* nonzero;
  int rows_per_tile, cap;  // tile route
  long long ntiles;
  P parse;
};

template <class P>
__global__ void __launch_bounds__(256) k_parse_rows(ParseArgs<P> a) {
  using T = typename P::T;
  long long v = 0;
  for (int64_t r = (int64_t)blockIdx.x * csdev::kBlock + threadIdx.x; r < a.in.rows; r += (int64_t)gridDim.x * csdev::kBlock) {
    const bool ok = csdev::row_is_valid(a.in.validity, r);
    const int64_t o0 = a.in.offsets[r];
    const T x = a.parse(a.in.chars + o0, ok ? (int)(a.in.offsets[r + 1] - o0) : 0, ok);
    a.out[r] = x;
    v += x != (T)0;
  }
  const long long t = csdev::block_reduce_sum_ll(v);
  if (threadIdx.x == 0 && t) atomicAdd(a.nonzero, (unsigned long long)t);
}

// A wave per R-row tile, persistent over a contiguous run of tiles (every wave reaches the reduction at the end).
template <class P>
__global__ void __launch_bounds__(256) k_parse_tile(ParseArgs<P> a) {
  using T = typename P::T;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint8_t* lds_in = reinterpret_cast<uint8_t*>(smem) + (size_t)wv * a.cap;
  cstile::RowTileWalk walk(a.in, a.rows_per_tile, a.ntiles, wv, lane);
  long long v = 0;
  if (!walk.done()) {
    for (;;) {
      const cstile::RowTile cur = walk.current();
      // (lead + span <= cap: every tile's span fits, checked by the host)
      cstile::stage_chars(lds_in, (int)(cur.g1 - cur.g0) + cur.lead, lane, walk.pf);
      const bool more = walk.advance();  // the next tile's bytes travel while this one is parsed
      cstile::wave_lds_fence();
      if (cur.in_tile) {
        const T x = a.parse(lds_in + cur.lead + cur.rbeg, cur.n, cur.live);
        a.out[cur.r0 + lane] = x;
        v += x != (T)0;
      }
      cstile::wave_lds_fence();  // (the LDS is restaged next round)
      if (!more) break;
    }
  }
  const long long t = csdev::block_reduce_sum_ll(v);
  if (threadIdx.x == 0 && t) atomicAdd(a.nonzero, (unsigned long long)t);
}

template <class P>
bool parse_tiles(const cs_column* col, ParseArgs<P> a, hipStream_t s) {
  if (cs::cfg("CS_CONVERT_ROWWISE")) return false;
  const cs::TilePlan tp = cs::plan_row_tiles(col, 32, s);
  if (!tp.R) return false;
  a.rows_per_tile = tp.R;
  a.cap = (int)((tp.span + 48 + 15) & ~(int64_t)15);
  a.ntiles = (col->rows + tp.R - 1) / tp.R;
  const size_t lds = (size_t)a.cap * 4;
  if (lds > 150 * 1024) return false;
  cs::launch_resident(&k_parse_tile<P>, lds, (a.ntiles + 3) / 4, s, a);
  return true;
}

// results to the caller's buffer (device or host); returns the count of non-zero results
template <class P>
int64_t run_parse(const cs_column* col, const P& parse, void* results, int on_device, hipStream_t s) {
  using T = typename P::T;
  const int64_t rows = col->rows;
  cs::Buf tmp;
  void* d_out = results;
  if (!on_device) {
    tmp = cs::dev_alloc(sizeof(T) * (size_t)rows, s);
    d_out = tmp->p;
  }
  cs::Buf acc = cs::dev_alloc(8, s);
  CS_HIP(hipMemsetAsync(acc->p, 0, 8, s));
  ParseArgs<P> a{};
  a.in = cs::view_of(col);
  a.out = static_cast<T*>(d_out);
  a.nonzero = cs::ptr<unsigned long long>(acc);
  a.parse = parse;
  if (parse_tiles(col, a, s)) {
    cs::note_route("tile");
  } else {
    cs::note_route("rows");
    hipLaunchKernelGGL(k_parse_rows<P>, dim3(std::min(cs::blocks_for(rows), 8192u)), dim3(csdev::kBlock), 0, s, a);
    CS_HIP(hipGetLastError());
  }
  if (!on_device) CS_HIP(hipMemcpyAsync(results, d_out, sizeof(T) * (size_t)rows, hipMemcpyDeviceToHost, s));
  int64_t* host = (int64_t*)cs::pinned_scratch(8);
  CS_HIP(hipMemcpyAsync(host, acc->p, 8, hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  return host[0];
}

// the format ops' input validity: LSB-first, bit = 1 valid; nullptr = all valid
__device__ __forceinline__ bool value_valid(const uint8_t* nulls, int64_t r) {
  return nulls == nullptr || ((nulls[r >> 3] >> (r & 7)) & 1);
}

}  // namespace csparse
