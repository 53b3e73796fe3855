// The int32 pieces every category remap is made of -- fill / iota, "send each value through a table", mark the keys the
// values use, compact the flagged entries -- and the host helpers around them.  Shared by the string categories
// (cs_catops.hip) and the numeric ones (cs_numcat.hip); file-local to each (anonymous namespace).
//
// RESTRICTION: this header is for those two .hip files only.  It opens an anonymous namespace and brings `cs` and `csdev`
// into it, so every includer compiles its own copy of each kernel and sees those names unqualified.  A third includer
// should be a conscious choice -- at that point give the kernels a named namespace and qualified names instead.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cs_internal.h"
#include "device_utils.h"

namespace {

using namespace cs;
using namespace csdev;

__global__ void k_fill(int32_t* __restrict__ a, int64_t n, int32_t v) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) a[i] = v;
}
__global__ void k_iota(int32_t* __restrict__ a, int64_t n, int32_t base) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) a[i] = base + (int32_t)i;
}
// out[i] = v < 0 ? v : table[v]
__global__ void k_remap_values(const int32_t* __restrict__ values, int64_t n, const int32_t* __restrict__ table, int32_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t v = values[i];
  out[i] = v < 0 ? v : table[v];
}
__global__ void k_mark_used(const int32_t* __restrict__ values, int64_t n, int64_t nkeys, int lo_ok, int32_t* __restrict__ used, unsigned* __restrict__ bad) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool oob = false;
  if (i < n) {
    const int32_t v = values[i];
    if (v >= 0 && v < nkeys) used[v] = 1;
    else oob = v < lo_ok || v >= nkeys;
  }
  if (__any(oob) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}
__global__ void k_flag_not(const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = in[i] ? 0 : 1;
}
// compaction: pos[slot[i]] = i for flagged i
__global__ void k_compact(const int32_t* __restrict__ flags, const int64_t* __restrict__ slot, int64_t n, int32_t* __restrict__ pos) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n && flags[i]) pos[slot[i]] = (int32_t)i;
}
// table[i] = flags[i] ? base + slot[i] : keep[i]
__global__ void k_table_from_slots(const int32_t* __restrict__ flags, const int64_t* __restrict__ slot, int64_t n, int32_t base, const int32_t* __restrict__ keep,
                                   int32_t* __restrict__ table) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) table[i] = flags[i] ? base + (int32_t)slot[i] : (keep ? keep[i] : -1);
}
__global__ void k_flag_negative(const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = in[i] < 0 ? 1 : 0;
}

struct Compacted {
  Buf pos;  // indices of the flagged entries, ascending
  Buf slot; // exclusive scan of the flags
  int64_t n = 0;
};
Compacted compact(const int32_t* d_flags, int64_t n, hipStream_t s) {
  Compacted c;
  if (n == 0) return c;
  c.slot = dev_alloc(sizeof(int64_t) * (n + 1), s);
  c.n = offsets_from_lengths(d_flags, n, ptr<int64_t>(c.slot), s);
  c.pos = dev_alloc(sizeof(int32_t) * std::max<int64_t>(c.n, 1), s);
  if (c.n) hipLaunchKernelGGL(k_compact, dim3(blocks_for(n)), dim3(kBlock), 0, s, d_flags, ptr<const int64_t>(c.slot), n, ptr<int32_t>(c.pos));
  return c;
}
Buf zeros32(int64_t n, hipStream_t s) {
  Buf b = dev_alloc(sizeof(int32_t) * std::max<int64_t>(n, 1), s);
  CS_HIP(hipMemsetAsync(b->p, 0, sizeof(int32_t) * std::max<int64_t>(n, 1), s));
  return b;
}

}  // namespace
