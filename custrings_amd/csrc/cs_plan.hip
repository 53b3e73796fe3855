// What the host asks of a finished column before it picks a kernel: the longest row and the widest
// tile, hints about its bytes -- each one pass, remembered on the (immutable) column -- and the tile planners that
// turn those numbers into a launch (cs_internal.h: plan_row_tiles, plan_staged_tiles, resident_grid).
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>

#include "cs_internal.h"
#include "device_utils.h"
#include "tile_utils.h"

using namespace csdev;

namespace cs {

__global__ void k_max_span64(const int64_t* __restrict__ offsets, int64_t rows, unsigned long long* __restrict__ out) {
  int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int64_t r0 = t * 64;
  int v = 0;
  if (r0 < rows) {
    int64_t r1 = r0 + 64 < rows ? r0 + 64 : rows;
    v = (int)(offsets[r1] - offsets[r0] > 0x7fffffff ? 0x7fffffff : offsets[r1] - offsets[r0]);
  }
  int m = block_reduce_max(v);
  if (threadIdx.x == 0 && (unsigned long long)m > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, (unsigned long long)m);
}
// Number of 256-thread workgroups of `kern` that are resident at once on this device
// (capped by `wanted`): the persistent kernels' look-back needs every wave of the grid
// to be running.
unsigned resident_grid(const void* kern, size_t lds, int64_t wanted) {
  // the occupancy query costs about a millisecond: remember the answers
  static std::mutex mu;
  static std::map<std::pair<const void*, size_t>, std::pair<int, int>> cache;
  int cus = 0, per = 0;
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find({kern, lds});
    if (it == cache.end()) {
      int dev = 0;
      CS_HIP(hipGetDevice(&dev));
      CS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
      CS_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kern, 256, lds));
      cache[{kern, lds}] = {cus, per};
    } else {
      cus = it->second.first;
      per = it->second.second;
    }
  }
  if (per < 1) per = 1;
  if (const char* e = cs::cfg("CS_STREAM_BLOCKS_PER_CU")) per = std::max(1, std::min(per, atoi(e)));
  const int64_t cap = (int64_t)cus * per;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cap, wanted));
}

__global__ void k_max_span_rows(const int64_t* __restrict__ offsets, int64_t rows, int per,
                                unsigned long long* __restrict__ out) {
  int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int64_t r0 = t * per;
  int v = 0;
  if (r0 < rows) {
    int64_t r1 = r0 + per < rows ? r0 + per : rows;
    v = (int)(offsets[r1] - offsets[r0] > 0x7fffffff ? 0x7fffffff : offsets[r1] - offsets[r0]);
  }
  int m = block_reduce_max(v);
  // (only a workgroup that would raise the maximum issues the same-address atomic: 390 K of them in a row cost
  // 4.4 ms on a 100M-row column, more than most kernels that ask for this number)
  if (threadIdx.x == 0 && (unsigned long long)m > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, (unsigned long long)m);
}
int64_t max_span_rows(const cs_column* c, int per, hipStream_t s) {
  if (per == 64) return max_span64(c, s);
  if (c->rows == 0) return 0;
  Buf acc = zeroed_count(s);
  int64_t n = (c->rows + per - 1) / per;
  hipLaunchKernelGGL(k_max_span_rows, dim3(blocks_for(n)), dim3(kBlock), 0, s, c->d_offsets(), c->rows, per,
                     ptr<unsigned long long>(acc));
  return read_count(acc, s);
}
TilePlan plan_row_tiles(const cs_column* c, int slack, hipStream_t s, bool outliers) {
  for (int r : {64, 32, 16}) {
    const int64_t span = max_span_rows(c, r, s);
    if (span + slack <= cstile::kPfBytes) return {r, span};
  }
  if (outliers && !cs::cfg("CS_NO_OUTLIER_TILES")) return {64, cstile::kPfBytes - 64};
  return {0, 0};
}
StagedTiles plan_staged_tiles(const cs_column* c, int slack, bool outliers, WaveLds w, hipStream_t s) {
  StagedTiles t;
  const TilePlan tp = plan_row_tiles(c, 32, s, outliers);
  const int cap = (int)((tp.span + slack + 15) & ~(int64_t)15);
  const size_t lds = ((size_t)w.bufs * cap + w.extra) * 4;
  if (!tp.R || lds > w.ceiling) return t;
  t.R = tp.R;
  t.cap = cap;
  t.ntiles = (c->rows + tp.R - 1) / tp.R;
  t.grid = (t.ntiles + 3) / 4;
  t.lds = lds;
  return t;
}
// How many 64-row tiles span more than `limit` bytes: a column whose LARGEST tile does not fit a tile kernel's staging
// buffer may still have all but a few that do (one long row among millions of short ones) -- the tile kernels then take
// the column and handle the oversize tiles a thread per row themselves, instead of the whole column going row-wise.
__global__ void k_count_spans_over(const int64_t* __restrict__ offsets, int64_t rows, int64_t limit, unsigned long long* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t r0 = t * 64;
  int v = 0;
  if (r0 < rows) {
    const int64_t r1 = r0 + 64 < rows ? r0 + 64 : rows;
    v = offsets[r1] - offsets[r0] > limit ? 1 : 0;
  }
  const long long n = block_reduce_sum(v);
  if (threadIdx.x == 0 && n) atomicAdd(out, (unsigned long long)n);
}
int64_t count_spans64_over(const cs_column* c, int64_t limit, hipStream_t s) {
  if (c->rows == 0) return 0;
  if (max_span64(c, s) <= limit) return 0;
  Buf acc = zeroed_count(s);
  const int64_t nsub = (c->rows + 63) / 64;
  hipLaunchKernelGGL(k_count_spans_over, dim3(blocks_for(nsub)), dim3(kBlock), 0, s, c->d_offsets(), c->rows, limit, ptr<unsigned long long>(acc));
  return read_count(acc, s);
}
// true when all but a few (at most 8, or one in a thousand) of the 64-row tiles span at most `limit` bytes
bool few_spans64_over(const cs_column* c, int64_t limit, hipStream_t s) {
  const int64_t nsub = (c->rows + 63) / 64;
  const int64_t over = count_spans64_over(c, limit, s);
  return over <= std::max<int64_t>(8, nsub / 1000);
}
// A hint for choosing between kernel forms (never for correctness): does the column look like non-ASCII text?  Three windows
// of 64 KiB (start, middle, end of the chars), cached on the immutable column.
__global__ void k_sample_high(const uint8_t* __restrict__ chars, int64_t nbytes, int* __restrict__ out) {
  const int64_t win = 64 * 1024;
  const int64_t base = blockIdx.x == 0 ? 0 : (blockIdx.x == 1 ? (nbytes / 2) & ~(int64_t)15 : (nbytes > win ? (nbytes - win) & ~(int64_t)15 : 0));
  uint32_t any = 0;
  for (int64_t i = base + (int64_t)threadIdx.x * 16; i + 16 <= nbytes && i < base + win; i += (int64_t)blockDim.x * 16) {
    const uint4 q = *reinterpret_cast<const uint4*>(chars + i);
    any |= (q.x | q.y | q.z | q.w) & 0x80808080u;
  }
  if (any) *out = 1;
}
bool sample_has_high_bytes(const cs_column* c, hipStream_t s) {
  if (c->high_sample >= 0) return c->high_sample != 0;
  if (c->nbytes < 16 || !c->chars) return (c->high_sample = 0) != 0;
  Buf flag = dev_alloc(sizeof(int), s);
  CS_HIP(hipMemsetAsync(flag->p, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_sample_high, dim3(3), dim3(256), 0, s, c->d_chars(), c->nbytes, ptr<int>(flag));
  return (c->high_sample = read_back<int>(flag->p, s) ? 1 : 0) != 0;
}
// Byte counts over the same three windows: how common a pattern's candidate bytes are in THIS column (regex route choice).
__global__ void __launch_bounds__(256) k_sample_hist(const uint8_t* __restrict__ chars, int64_t nbytes, uint32_t* __restrict__ out) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t win = 64 * 1024;
  const int64_t base = blockIdx.x == 0 ? 0 : (blockIdx.x == 1 ? (nbytes / 2) & ~(int64_t)15 : (nbytes > win ? (nbytes - win) & ~(int64_t)15 : 0));
  // (windows that coincide on a short column are counted once)
  const bool dup = (blockIdx.x == 1 && base == 0) || (blockIdx.x == 2 && (base == 0 || base == ((nbytes / 2) & ~(int64_t)15)));
  if (!dup)
    for (int64_t i = base + threadIdx.x; i < nbytes && i < base + win; i += blockDim.x) atomicAdd(&h[chars[i]], 1u);
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(out + threadIdx.x, h[threadIdx.x]);
}
const uint32_t* sample_byte_hist(const cs_column* c, hipStream_t s) {
  static std::mutex mu;
  {
    std::lock_guard<std::mutex> lk(mu);
    if (c->byte_hist) return c->byte_hist->data();
  }
  auto hist = std::make_shared<std::array<uint32_t, 256>>();
  hist->fill(0);
  if (c->nbytes > 0 && c->chars) {
    Buf acc = dev_alloc(256 * sizeof(uint32_t), s);
    CS_HIP(hipMemsetAsync(acc->p, 0, 256 * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_sample_hist, dim3(3), dim3(256), 0, s, c->d_chars(), c->nbytes, ptr<uint32_t>(acc));
    uint32_t* host = (uint32_t*)pinned_scratch(256 * sizeof(uint32_t));
    CS_HIP(hipMemcpyAsync(host, acc->p, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    std::copy(host, host + 256, hist->begin());
  }
  std::lock_guard<std::mutex> lk(mu);
  if (!c->byte_hist) c->byte_hist = hist;
  return c->byte_hist->data();
}
int64_t max_row_bytes(const cs_column* c, hipStream_t s) {
  if (c->max_row >= 0) return c->max_row;
  return c->max_row = max_span_rows(c, 1, s);
}
int64_t max_span64(const cs_column* c, hipStream_t s) {
  if (c->max_span64 >= 0) return c->max_span64;
  if (c->rows == 0) return c->max_span64 = 0;
  Buf acc = zeroed_count(s);
  int64_t nsub = (c->rows + 63) / 64;
  hipLaunchKernelGGL(k_max_span64, dim3(blocks_for(nsub)), dim3(kBlock), 0, s, c->d_offsets(), c->rows,
                     ptr<unsigned long long>(acc));
  return c->max_span64 = read_count(acc, s);
}

// One streaming pass over the chars buffer, remembered on the (immutable) column: true when
// the bytes hold no NUL and no UTF-8 lead byte whose announced continuation positions hold an
// ASCII byte.  On such a column a per-character scan and a per-byte scan see every ASCII byte
// at a character boundary, so an ASCII needle may be searched either way (cs_replace routes a
// literal needle through the regex stream kernel on the strength of this).
__global__ void __launch_bounds__(256) k_bytes_plain(const uint8_t* __restrict__ chars, int64_t nbytes, unsigned* __restrict__ flag) {
  const int64_t pieces = (nbytes + 15) / 16;
  uint32_t hit = 0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < pieces; p += (int64_t)gridDim.x * 256) {
    uint32_t w[5];
    w[0] = p > 0 ? *reinterpret_cast<const uint32_t*>(chars + 16 * p - 4) : 0x20202020u;
    if (16 * p + 16 <= nbytes) {
      const uint4 q = *reinterpret_cast<const uint4*>(chars + 16 * p);
      w[1] = q.x, w[2] = q.y, w[3] = q.z, w[4] = q.w;
    } else {
      for (int k = 1; k < 5; ++k) w[k] = 0x20202020u;
      for (int64_t i = 16 * p; i < nbytes; ++i) {
        const int j = (int)(i - 16 * p);
        w[1 + (j >> 2)] = (w[1 + (j >> 2)] & ~(0xFFu << (8 * (j & 3)))) | ((uint32_t)chars[i] << (8 * (j & 3)));
      }
    }
    uint32_t l2[5], l3[5], l4[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      l2[k] = w[k] & (w[k] << 1) & 0x80808080u;  // bytes >= 0xC0
      l3[k] = l2[k] & (w[k] << 2);               // >= 0xE0
      l4[k] = l3[k] & (w[k] << 3);               // >= 0xF0
    }
#pragma unroll
    for (int k = 1; k < 5; ++k) {
      const uint32_t announced = __funnelshift_l(l2[k - 1], l2[k], 8) | __funnelshift_l(l3[k - 1], l3[k], 16) |
                                 __funnelshift_l(l4[k - 1], l4[k], 24);
      hit |= (announced | (w[k] - 0x01010101u)) & ~w[k] & 0x80808080u;
    }
  }
  if (__any(hit != 0) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
bool bytes_plain(const cs_column* c, hipStream_t s) {
  if (c->plain_bytes >= 0) return c->plain_bytes != 0;
  if (c->nbytes == 0) return (c->plain_bytes = 1) != 0;
  // (a wrapped caller buffer at an odd address: the check reads aligned 16-byte pieces -- decline)
  if ((uintptr_t)c->d_chars() & 15) return (c->plain_bytes = 0) != 0;
  Buf acc = zeroed_count(s);
  const int64_t pieces = (c->nbytes + 15) / 16;
  const unsigned grid = (unsigned)std::min<int64_t>((pieces + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(k_bytes_plain, dim3(grid), dim3(256), 0, s, c->d_chars(), c->nbytes, ptr<unsigned>(acc));
  CS_HIP(hipGetLastError());
  return (c->plain_bytes = read_back<unsigned>(acc->p, s) ? 0 : 1) != 0;
}

}  // namespace cs
