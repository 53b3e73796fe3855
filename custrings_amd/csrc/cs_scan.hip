// The lengths -> offsets scan (cs_internal.h: offsets_from_lengths and its variants): every op that sizes its rows
// first comes through here.  Three routes -- chunks of 2048 lengths a wave, 256 lengths a workgroup, and the segmented
// form of the latter -- that differ in their sums kernel and their write kernel and share the rest.
#include <hip/hip_runtime.h>

#include "cs_internal.h"
#include "device_utils.h"
#include "tile_utils.h"

using namespace csdev;

namespace cs {

// ------------------------------------------------------------ scan kernels --
// block sums of 256 lengths (negative = null -> 0)
__global__ void k_block_sums(const int32_t* __restrict__ lens, int64_t n, int64_t* __restrict__ sums) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int v = (i < n) ? lens[i] : 0;
  if (v < 0) v = 0;
  long long t = block_reduce_sum(v);
  if (threadIdx.x == 0) sums[blockIdx.x] = t;
}
// One workgroup per segment scans `nb` int64 block sums in place (exclusive),
// 8 per thread per sweep, and publishes the segment total.
__global__ void __launch_bounds__(1024) k_scan_block_sums(int64_t* __restrict__ sums, int64_t nb,
                                                          int64_t* __restrict__ totals) {
  __shared__ long long wave_tot[16];
  __shared__ long long carry_s;
  int64_t* seg = sums + (int64_t)blockIdx.x * nb;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int64_t base = 0; base < nb; base += 8192) {
    long long v[8], run = 0;
    int64_t i0 = base + (int64_t)threadIdx.x * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      v[k] = (i0 + k < nb) ? seg[i0 + k] : 0;
      run += v[k];
    }
    long long incl = wave_inclusive_scan(run);
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    long long before = carry_s, all = 0;
    for (int k = 0; k < 16; ++k) {
      long long t = wave_tot[k];
      if (k < wv) before += t;
      all += t;
    }
    long long ex = before + incl - run;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (i0 + k < nb) seg[i0 + k] = ex;
      ex += v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) carry_s += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry_s;
}
// offsets[i] = block_base[b] + in-block exclusive prefix; offsets[n] = total
// (meta: [0] longest row, [1] largest 64-row span -- a wave holds 64 consecutive rows starting at a multiple of 64; only a
// wave that would raise a maximum issues the same-address atomic)
__device__ __forceinline__ void meta_raise(unsigned long long* slot, long long v) {
  if ((unsigned long long)v > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, (unsigned long long)v);
}
__global__ void k_write_offsets(const int32_t* __restrict__ lens, int64_t n,
                                const int64_t* __restrict__ block_base, int64_t nb,
                                int64_t* __restrict__ offsets, unsigned long long* __restrict__ meta) {
  // grid.y = segment
  const int32_t* sl = lens + (int64_t)blockIdx.y * n;
  const int64_t* sb = block_base + (int64_t)blockIdx.y * nb;
  int64_t* so = offsets + (int64_t)blockIdx.y * (n + 1);
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int v = (i < n) ? sl[i] : 0;
  if (v < 0) v = 0;
  long long ex = block_exclusive_scan(v, nullptr) + sb[blockIdx.x];
  if (i < n) so[i] = ex;
  if (i == n - 1) so[n] = ex + v;
  if (meta) {  // (two words per segment)
    const int longest = wave_reduce_max(v);
    long long span = v;
    for (int d = 32; d > 0; d >>= 1) span += __shfl_xor(span, d, 64);
    if ((threadIdx.x & 63) == 0) {
      meta_raise(meta + 2 * blockIdx.y, longest);
      meta_raise(meta + 2 * blockIdx.y + 1, span);
    }
  }
}
__global__ void k_block_sums_seg(const int32_t* __restrict__ lens, int64_t n, int64_t nb,
                                 int64_t* __restrict__ sums) {
  const int32_t* sl = lens + (int64_t)blockIdx.y * n;
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int v = (i < n) ? sl[i] : 0;
  if (v < 0) v = 0;
  long long t = block_reduce_sum(v);
  if (threadIdx.x == 0) sums[(int64_t)blockIdx.y * nb + blockIdx.x] = t;
}

// lengths -> offsets on chunks of 2048 lengths, a wave each, with whole 16-byte loads and stores: chunk sums, the
// single-workgroup scan of the sums (49 K of them for 100 M rows), offsets.  (The kernels above work on 256
// lengths per workgroup, one per thread, with two workgroup barriers per scan: 1.0 ms for 100 M lengths against
// the 0.3 ms the 1.6 GB of traffic needs.  A one-pass form with a decoupled look-back per 1024-length tile was
// measured slower than either -- 1.23 ms: with thousands of small tiles in flight each walks many windows back.)
constexpr int kChunkRounds = 8, kChunk = kChunkRounds * 256;
// (gfx950 takes 16-byte global accesses at dword alignment: a column's lengths may start anywhere in a span array)
typedef int int4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef long long ll2_a8 __attribute__((ext_vector_type(2), aligned(8)));
struct ChunkVals {
  int v[kChunkRounds][4];
  unsigned ok[kChunkRounds];  // bit k: length k of the round is not negative (a row, not a null) and lies below n
};
__device__ __forceinline__ void load_chunk(const int32_t* __restrict__ lens, int64_t n, int64_t base, int lane, ChunkVals& c) {
#pragma unroll
  for (int j = 0; j < kChunkRounds; ++j) {
    const int64_t i = base + j * 256 + lane * 4;
    if (i + 3 < n) {
      const int4_a4 q = *reinterpret_cast<const int4_a4*>(lens + i);
      c.v[j][0] = q.x;
      c.v[j][1] = q.y;
      c.v[j][2] = q.z;
      c.v[j][3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) c.v[j][k] = i + k < n ? lens[i + k] : 0;
    }
    c.ok[j] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (i + k < n && c.v[j][k] >= 0) c.ok[j] |= 1u << k;
      c.v[j][k] = c.v[j][k] < 0 ? 0 : c.v[j][k];
    }
  }
}
__device__ __forceinline__ long long chunk_total(const ChunkVals& c) {
  long long t = 0;
#pragma unroll
  for (int j = 0; j < kChunkRounds; ++j) t += (long long)c.v[j][0] + c.v[j][1] + c.v[j][2] + c.v[j][3];
  for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d, 64);
  return t;
}
__global__ void __launch_bounds__(256) k_chunk_sums(const int32_t* __restrict__ lens, int64_t n, int64_t nchunks, int64_t* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;
  ChunkVals c;
  load_chunk(lens, n, chunk * kChunk, lane, c);
  const long long t = chunk_total(c);
  if (lane == 0) sums[chunk] = t;
}
__global__ void __launch_bounds__(256) k_chunk_offsets(const int32_t* __restrict__ lens, int64_t n, int64_t nchunks,
                                                       const int64_t* __restrict__ chunk_base, int64_t* __restrict__ offsets,
                                                       uint8_t* __restrict__ validity, int64_t validity_len, unsigned long long* __restrict__ meta) {
  const int lane = threadIdx.x & 63;
  const int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (chunk >= nchunks) return;
  const int64_t base = chunk * kChunk;
  long long carry = chunk_base[chunk];
  ChunkVals c;
  load_chunk(lens, n, base, lane, c);
  const bool narrow = chunk_total(c) < 0x7fffffffLL;  // (wave-uniform: the sums inside the chunk fit 32 bits)
  if (meta) {
    // the column's metadata as a by-product: a lane holds four consecutive rows, sixteen lanes the 64 rows of a tile
    // that starts at a multiple of 64 (the chunk starts at a multiple of 2048)
    long long span = 0;
    int longest = 0;
#pragma unroll
    for (int j = 0; j < kChunkRounds; ++j) {
      long long s4 = (long long)c.v[j][0] + c.v[j][1] + c.v[j][2] + c.v[j][3];
      longest = max(longest, max(max(c.v[j][0], c.v[j][1]), max(c.v[j][2], c.v[j][3])));
      for (int d = 8; d > 0; d >>= 1) s4 += __shfl_xor(s4, d, 64);
      span = max(span, s4);
    }
    longest = wave_reduce_max(longest);
    for (int d = 32; d > 0; d >>= 1) span = max(span, (long long)__shfl_xor(span, d, 64));
    if (lane == 0) {
      meta_raise(meta, longest);
      meta_raise(meta + 1, span);
    }
  }
#pragma unroll
  for (int j = 0; j < kChunkRounds; ++j) {
    const int64_t i = base + j * 256 + lane * 4;
    long long first, round_total;
    if (narrow) {
      const int s4 = c.v[j][0] + c.v[j][1] + c.v[j][2] + c.v[j][3];
      const int inc = wave_inclusive_scan(s4);
      first = carry + (inc - s4);
      round_total = __builtin_amdgcn_readlane(inc, 63);
    } else {
      const long long s4 = (long long)c.v[j][0] + c.v[j][1] + c.v[j][2] + c.v[j][3];
      const long long inc = wave_inclusive_scan(s4);
      first = carry + (inc - s4);
      round_total = cstile::rl64(inc, 63);
    }
    long long o[5];
    o[0] = first;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k + 1] = o[k] + c.v[j][k];
    if (i + 3 < n) {
      *reinterpret_cast<ll2_a8*>(offsets + i) = ll2_a8{o[0], o[1]};
      *reinterpret_cast<ll2_a8*>(offsets + i + 2) = ll2_a8{o[2], o[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (i + k < n) offsets[i + k] = o[k];
    }
    // the end of the last row: the column's byte count
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k == n - 1) offsets[n] = o[k + 1];
    // the validity bits of the round's 256 rows: two lanes' nibbles make a byte
    if (validity) {
      const unsigned pair = c.ok[j] | ((unsigned)__shfl_down((int)c.ok[j], 1, 64) << 4);
      const int64_t at = ((base + j * 256) >> 3) + (lane >> 1);
      if (!(lane & 1) && at < validity_len) validity[at] = (uint8_t)pair;
    }
    carry += round_total;
  }
}

// ---------------------------------------------------- the routes' shared steps --
// The scan's small results live in one buffer of three words per segment: [0, segs) the totals, then two maxima per
// segment.  One buffer and one copy back: the metadata costs no extra synchronisation.
// zero: the buffer; cleared when a write kernel is to raise the maxima in it
static Buf zeroed_totals(int segs, bool with_meta, hipStream_t s) {
  Buf totals = dev_alloc(sizeof(int64_t) * segs * 3, s);
  if (with_meta) CS_HIP(hipMemsetAsync(totals->p, 0, sizeof(int64_t) * segs * 3, s));
  return totals;
}
// a workgroup per segment turns the `nb` sums into exclusive bases and leaves the segment's total
static void scan_sums(const Buf& sums, int64_t nb, int segs, const Buf& totals, hipStream_t s) {
  hipLaunchKernelGGL(k_scan_block_sums, dim3(segs), dim3(1024), 0, s, ptr<int64_t>(sums), nb, ptr<int64_t>(totals));
}
// read: one word per segment, or all three, through the pinned scratch (synchronises `s`)
static const int64_t* read_totals(const Buf& totals, int segs, bool with_meta, hipStream_t s) {
  int64_t* host = (int64_t*)pinned_scratch(sizeof(int64_t) * segs * 3);
  CS_HIP(hipMemcpyAsync(host, ptr<int64_t>(totals), sizeof(int64_t) * segs * (with_meta ? 3 : 1), hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  return host;
}
// unpack: a single segment's total, its maxima to `meta`
static int64_t unpack_total(const int64_t* host, LenMeta* meta) {
  if (meta) {
    meta->max_row = host[1];
    meta->max_span64 = host[2];
  }
  return host[0];
}

// ------------------------------------------------------------------ routes --
static int64_t offsets_by_chunks(const int32_t* lens, int64_t n, int64_t* offsets, uint8_t* validity, hipStream_t s, LenMeta* meta) {
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  Buf sums = dev_alloc(sizeof(int64_t) * nchunks, s);
  Buf total = zeroed_totals(1, meta != nullptr, s);
  const unsigned grid = (unsigned)((nchunks + 3) / 4);
  hipLaunchKernelGGL(k_chunk_sums, dim3(grid), dim3(kBlock), 0, s, lens, n, nchunks, ptr<int64_t>(sums));
  scan_sums(sums, nchunks, 1, total, s);
  {
    ProfScope ps("k_write_offsets", s);
    hipLaunchKernelGGL(k_chunk_offsets, dim3(grid), dim3(kBlock), 0, s, lens, n, nchunks, ptr<const int64_t>(sums), offsets, validity,
                       (int64_t)validity_bytes(n), meta ? ptr<unsigned long long>(total) + 1 : nullptr);
  }
  return unpack_total(read_totals(total, 1, meta != nullptr, s), meta);
}
static int64_t offsets_by_workgroups(const int32_t* lens, int64_t n, int64_t* offsets, hipStream_t s, Buf block_sums, LenMeta* meta) {
  int64_t nb = (n + kBlock - 1) / kBlock;
  Buf sums = block_sums;
  if (!sums) {
    sums = dev_alloc(sizeof(int64_t) * nb, s);
    hipLaunchKernelGGL(k_block_sums, dim3((unsigned)nb), dim3(kBlock), 0, s, lens, n, ptr<int64_t>(sums));
  }
  Buf total = zeroed_totals(1, meta != nullptr, s);
  scan_sums(sums, nb, 1, total, s);
  {
    ProfScope ps("k_write_offsets", s);
    hipLaunchKernelGGL(k_write_offsets, dim3((unsigned)nb, 1), dim3(kBlock), 0, s, lens, n,
                       ptr<int64_t>(sums), nb, offsets, meta ? ptr<unsigned long long>(total) + 1 : nullptr);
  }
  return unpack_total(read_totals(total, 1, meta != nullptr, s), meta);
}
void offsets_from_lengths_segmented(const int32_t* lens, int64_t n, int segs, int64_t* offsets,
                                    int64_t* totals_host, hipStream_t s, int64_t* largest_host) {
  if (n == 0) {
    CS_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t) * segs, s));
    for (int k = 0; k < segs; ++k) totals_host[k] = 0;
    for (int k = 0; largest_host && k < segs; ++k) largest_host[k] = 0;
    return;
  }
  int64_t nb = (n + kBlock - 1) / kBlock;
  Buf sums = dev_alloc(sizeof(int64_t) * nb * segs, s);
  // (of a segment's two maxima only [0], the largest length, is handed out here)
  Buf totals = zeroed_totals(segs, largest_host != nullptr, s);
  hipLaunchKernelGGL(k_block_sums_seg, dim3((unsigned)nb, segs), dim3(kBlock), 0, s, lens, n, nb,
                     ptr<int64_t>(sums));
  scan_sums(sums, nb, segs, totals, s);
  hipLaunchKernelGGL(k_write_offsets, dim3((unsigned)nb, segs), dim3(kBlock), 0, s, lens, n,
                     ptr<int64_t>(sums), nb, offsets, largest_host ? ptr<unsigned long long>(totals) + segs : nullptr);
  const int64_t* host = read_totals(totals, segs, largest_host != nullptr, s);
  for (int k = 0; k < segs; ++k) totals_host[k] = host[k];
  for (int k = 0; largest_host && k < segs; ++k) largest_host[k] = host[segs + 2 * k];
}

int64_t offsets_from_lengths(const int32_t* lens, int64_t n, int64_t* offsets, hipStream_t s,
                             Buf block_sums, LenMeta* meta) {
  if (n == 0) {
    CS_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t), s));
    if (meta) meta->max_row = meta->max_span64 = 0;
    return 0;
  }
  if (!block_sums && !cs::cfg("CS_SCAN_BY_WORKGROUPS")) return offsets_by_chunks(lens, n, offsets, nullptr, s, meta);
  return offsets_by_workgroups(lens, n, offsets, s, block_sums, meta);
}
// the same scan, nothing read back: the total is offsets[n] in device memory, the stream is not waited for (the radix sort's
// eight passes each scan their tile counts -- a round trip to the host per pass was most of its time on a million keys)
void offsets_from_lengths_async(const int32_t* lens, int64_t n, int64_t* offsets, hipStream_t s) {
  if (n == 0) {
    CS_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t), s));
    return;
  }
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  Buf sums = dev_alloc(sizeof(int64_t) * nchunks, s);
  Buf total = zeroed_totals(1, false, s);
  const unsigned grid = (unsigned)((nchunks + 3) / 4);
  hipLaunchKernelGGL(k_chunk_sums, dim3(grid), dim3(kBlock), 0, s, lens, n, nchunks, ptr<int64_t>(sums));
  scan_sums(sums, nchunks, 1, total, s);
  hipLaunchKernelGGL(k_chunk_offsets, dim3(grid), dim3(kBlock), 0, s, lens, n, nchunks, ptr<const int64_t>(sums), offsets, (uint8_t*)nullptr, (int64_t)validity_bytes(n),
                     (unsigned long long*)nullptr);
  CS_HIP(hipGetLastError());
}
// offsets and the validity mask (length >= 0) of a column in the same pass over its lengths
int64_t offsets_and_validity_from_lengths(const int32_t* lens, int64_t n, int64_t* offsets, Buf* validity, hipStream_t s, LenMeta* meta) {
  if (n == 0 || cs::cfg("CS_SCAN_BY_WORKGROUPS")) {
    *validity = validity_from_lengths(lens, n, s);
    return offsets_from_lengths(lens, n, offsets, s, nullptr, meta);
  }
  *validity = dev_alloc(validity_bytes(n), s);
  return offsets_by_chunks(lens, n, offsets, ptr<uint8_t>(*validity), s, meta);
}

__global__ void k_validity_from_lengths(const int32_t* __restrict__ lens, int64_t n,
                                        uint8_t* __restrict__ validity) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool ok = i < n && lens[i] >= 0;
  store_validity_word(validity, i - (threadIdx.x & 63), ok, n);
}
Buf validity_from_lengths(const int32_t* lens, int64_t n, hipStream_t s) {
  Buf v = dev_alloc(validity_bytes(n), s);
  if (n)
    hipLaunchKernelGGL(k_validity_from_lengths, dim3(blocks_for(n)), dim3(kBlock), 0, s, lens, n,
                       ptr<uint8_t>(v));
  return v;
}


// (count_nulls stands here, beside the scan kernels, and not with the column's other cached numbers in cs_plan.hip: in a
// module without k_block_sums ahead of it the compiler orders the operands of one 64-bit add in k_count_valid's inlined
// block_reduce_sum the other way round -- the same sum, other bytes, and the kernels' bytes are what a move must not change)
// one thread per 64-row validity word (the bits past `rows` in the last word are zero)
__global__ void k_count_valid(const uint8_t* __restrict__ validity, int64_t rows,
                              unsigned long long* __restrict__ out) {
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int v = 0;
  if (w * 64 < rows) {
    unsigned long long bits = reinterpret_cast<const unsigned long long*>(validity)[w];
    const int64_t left = rows - w * 64;
    if (left < 64) bits &= (1ull << left) - 1ull;
    v = __builtin_popcountll(bits);
  }
  long long t = block_reduce_sum(v);
  if (threadIdx.x == 0 && t) atomicAdd(out, (unsigned long long)t);
}
int64_t count_nulls(const cs_column* c, hipStream_t s) {
  if (c->null_count >= 0) return c->null_count;
  if (!c->validity || c->rows == 0) return c->null_count = 0;
  Buf cnt = zeroed_count(s);
  hipLaunchKernelGGL(k_count_valid, dim3(blocks_for((c->rows + 63) / 64)), dim3(kBlock), 0, s, c->d_validity(),
                     c->rows, ptr<unsigned long long>(cnt));
  return c->null_count = c->rows - read_count(cnt, s);
}

}  // namespace cs

using namespace cs;

extern "C" {

// The lengths-to-offsets scans by themselves, one host function per route, nothing changed in any of them (tests/test_gpu_scan.py).
int cs_debug_offsets_from_lengths(const int32_t* lens, int64_t n, int segs, int route, int64_t* offsets, uint8_t* validity, int64_t* out,
                                  cs_stream stream) {
  return guard([&] {
    if (!lens || !offsets || !out || n < 0 || route < 0 || route > 4 || segs < 1 || (segs != 1 && route != 4) || (validity && route != 1))
      fail(CS_ERR_INVALID_ARG, "debug_offsets_from_lengths: bad arguments");
    require_device();
    hipStream_t s = S(stream);
    LenMeta meta;
    switch (route) {
      case 0:
        if (n == 0) out[0] = offsets_from_lengths(lens, n, offsets, s, nullptr, &meta);
        else out[0] = offsets_by_chunks(lens, n, offsets, nullptr, s, &meta);
        break;
      case 1: {
        Buf v;
        out[0] = offsets_and_validity_from_lengths(lens, n, offsets, &v, s, &meta);
        if (validity && n) CS_HIP(hipMemcpyAsync(validity, v->p, validity_bytes(n), hipMemcpyDeviceToDevice, s));
        break;
      }
      case 2:
        if (n == 0) out[0] = offsets_from_lengths(lens, n, offsets, s, nullptr, &meta);
        else out[0] = offsets_by_workgroups(lens, n, offsets, s, nullptr, &meta);
        break;
      case 3:
        offsets_from_lengths_async(lens, n, offsets, s);
        CS_HIP(hipMemcpyAsync(out, offsets + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        break;
      case 4: {
        std::vector<int64_t> totals(segs), largest(segs);
        offsets_from_lengths_segmented(lens, n, segs, offsets, totals.data(), s, largest.data());
        for (int k = 0; k < segs; ++k) {
          out[3 * k] = totals[k];
          out[3 * k + 1] = largest[k];
          out[3 * k + 2] = -1;
        }
        break;
      }
    }
    CS_HIP(hipGetLastError());
    CS_HIP(hipStreamSynchronize(s));
    if (route != 4) {
      out[1] = meta.max_row;
      out[2] = meta.max_span64;
    }
  });
}

}  // extern "C"
