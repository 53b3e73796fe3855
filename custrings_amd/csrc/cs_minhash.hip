// minhash: the MinHash signatures of a column (rows x nperm uint32) and the LSH band keys made from them.  The definition
// and the per-row logic are minhash_ops.h, shared with the CPU harness of tests/minhash_model.py.
//
// Work per row is n-grams x nperm multiply-adds, so every n-gram is hashed ONCE and kept, and the permutations run over
// the kept hashes in chunks of kChunk: a chunk's a[i], b[i] are wave-uniform (scalar registers), its kChunk running minima
// one register each.  Two forms, chosen by the host as run_match chooses (cs_textops.hip):
//  - tile ("tile"): short rows, the staged-row route.  A wave stages R = 64 / 32 / 16 rows in LDS, a lane walks its row
//    and leaves the hashes of its n-grams in LDS (a row of n bytes has at most n: the lane's slots are those of its
//    bytes), then runs the chunks over them.  A wave's nrows x nperm block is contiguous in memory: where it fits
//    kOutTileBytes it is assembled in LDS and stored side by side, else each lane stores its own values.
//  - wave ("wave"): rows of any length, a wave per row, the bytes read from memory.  The row is cut into segments of
//    64 x kGrams byte positions; a lane takes the n-grams that start at its kGrams positions and keeps their hashes in
//    registers (a position without one repeats a hash of the same segment: the minimum does not change), runs the
//    chunks, and each of a chunk's minima is reduced across the lanes by DPP; the last lane folds them into the row's
//    running signature in LDS, which the wave stores at the row's end, side by side.
// The band keys: a thread per (row, band).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "cs_internal.h"
#include "device_utils.h"
#include "minhash_ops.h"
#include "tile_utils.h"

using namespace cs;
using namespace csdev;

namespace {

constexpr int kChunk = 16;            // permutations a pass: their minima in registers, a[] and b[] in scalar registers
constexpr int kGrams = 8;             // wave form: byte positions a lane takes per segment
constexpr int kOutTileBytes = 16384;  // tile form: a wave's assembled block of results (64 rows x 64 permutations)

struct MinhashArgs {
  ColView in;
  int width, nperm, npad;  // npad: nperm rounded up to kChunk (a[] and b[] are padded to it)
  uint32_t seed;
  int rows_per_tile, cap, out_cap;  // tile form
  long long ntiles;
};

// chunk c0's multipliers and addends: uniform values, forced into scalar registers
struct Chunk {
  uint32_t a[kChunk], b[kChunk];
  __device__ __forceinline__ Chunk(const uint32_t* __restrict__ ab, int npad, int c0) {
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      a[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)ab[c0 + i]);
      b[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)ab[npad + c0 + i]);
    }
  }
};

template <bool STAGE_OUT>
__global__ void __launch_bounds__(256) k_minhash_tile(MinhashArgs a, const uint32_t* __restrict__ ab, uint32_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint8_t* base = reinterpret_cast<uint8_t*>(smem);
  // [4 x staged rows: cap bytes] [4 x kept hashes: cap words] [4 x assembled results: out_cap bytes]
  uint8_t* lds_in = base + (size_t)wv * a.cap;
  uint32_t* hashes = reinterpret_cast<uint32_t*>(base + (size_t)4 * a.cap) + (size_t)wv * a.cap;
  uint32_t* lds_out = reinterpret_cast<uint32_t*>(base + (size_t)20 * a.cap + (size_t)wv * a.out_cap);
  // (every tile's span fits the staging buffer: checked by the host)
  cstile::walk_staged_tiles<cstile::Oversize::kHostChecked>(a.in, a.rows_per_tile, a.ntiles, lds_in, a.cap, wv, lane,
                                                            [&](const cstile::RowTile& cur, const uint8_t* p) {
    uint32_t* mine = hashes + cur.rbeg;  // (rbeg + n <= the tile's span <= cap)
    int count = 0;
    if (cur.n > 0) csmh::for_each_gram(p, cur.n, a.width, a.seed, [&](uint32_t h) { mine[count++] = h; });
    uint32_t* o = STAGE_OUT ? lds_out + (size_t)lane * a.nperm : out + (cur.r0 + lane) * a.nperm;
    for (int c0 = 0; c0 < a.npad; c0 += kChunk) {
      const Chunk ch(ab, a.npad, c0);
      uint32_t m[kChunk];
#pragma unroll
      for (int i = 0; i < kChunk; ++i) m[i] = csmh::kNoGram;
      for (int k = 0; k < count; ++k) {
        const uint32_t h = mine[k];
#pragma unroll
        for (int i = 0; i < kChunk; ++i) m[i] = min(m[i], csmh::permute(h, ch.a[i], ch.b[i]));
      }
      if (cur.in_tile) {
#pragma unroll
        for (int i = 0; i < kChunk; ++i)
          if (c0 + i < a.nperm) o[c0 + i] = m[i];
      }
    }
    if (STAGE_OUT) {  // the wave's nrows x nperm results lie side by side in memory
      cstile::wave_lds_fence();
      uint32_t* g = out + cur.r0 * a.nperm;
      const int total = cur.nrows * a.nperm;
      for (int i = lane; i < total; i += 64) g[i] = lds_out[i];
    }
  });
}

// the minimum of the wave's 64 values, in lane 63 (the steps of wave_inclusive_scan; a lane without a source keeps its own)
__device__ __forceinline__ uint32_t wave_min_to_last(uint32_t v) {
  v = min(v, (uint32_t)dpp_mov<DPP_ROW_SHR1>((int)v, (int)v));
  v = min(v, (uint32_t)dpp_mov<DPP_ROW_SHR2>((int)v, (int)v));
  v = min(v, (uint32_t)dpp_mov<DPP_ROW_SHR4>((int)v, (int)v));
  v = min(v, (uint32_t)dpp_mov<DPP_ROW_SHR8>((int)v, (int)v));
  v = min(v, (uint32_t)dpp_mov<DPP_ROW_BCAST15, 0xA>((int)v, (int)v));
  v = min(v, (uint32_t)dpp_mov<DPP_ROW_BCAST31, 0xC>((int)v, (int)v));
  return v;
}

// every chunk over a segment's kept hashes; lane 63 folds the wave's minima into the row's signature
__device__ __forceinline__ void fold_segment(const uint32_t (&hs)[kGrams], const MinhashArgs& a, const uint32_t* __restrict__ ab, uint32_t* sig, int lane) {
  for (int c0 = 0; c0 < a.npad; c0 += kChunk) {
    const Chunk ch(ab, a.npad, c0);
    uint32_t m[kChunk];
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      m[i] = csmh::permute(hs[0], ch.a[i], ch.b[i]);
#pragma unroll
      for (int g = 1; g < kGrams; ++g) m[i] = min(m[i], csmh::permute(hs[g], ch.a[i], ch.b[i]));
      m[i] = wave_min_to_last(m[i]);
    }
    if (lane == 63) {
#pragma unroll
      for (int i = 0; i < kChunk; ++i) sig[c0 + i] = min(sig[c0 + i], m[i]);
    }
  }
}

__global__ void __launch_bounds__(256) k_minhash_wave(MinhashArgs a, const uint32_t* __restrict__ ab, uint32_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint32_t* sig = smem + (size_t)wv * a.npad;  // the row's running signature (only lane 63 touches it inside a row)
  for (int64_t r = (int64_t)blockIdx.x * 4 + wv; r < a.in.rows; r += (int64_t)gridDim.x * 4) {
    const int64_t o0 = a.in.offsets[r];
    const int n = row_is_valid(a.in.validity, r) ? (int)(a.in.offsets[r + 1] - o0) : 0;
    const uint8_t* p = a.in.chars + o0;
    for (int i = lane; i < a.npad; i += 64) sig[i] = csmh::kNoGram;
    int starts = 0;
    for (int64_t i = lane; i < n; i += 64) starts += csmh::char_start(p[i]);
    const int nch = wave_reduce_sum(starts);
    cstile::wave_lds_fence();
    uint32_t hs[kGrams];
    if (nch > 0 && nch < a.width) {  // one n-gram, the whole row (every lane hashes it: no lane has anything else to do)
      const uint32_t h = csmh::murmur3_32(p, n, a.seed);
#pragma unroll
      for (int g = 0; g < kGrams; ++g) hs[g] = h;
      fold_segment(hs, a, ab, sig, lane);
    } else if (nch > 0) {
      for (int64_t seg = 0; seg < n; seg += 64 * kGrams) {
        unsigned have = 0;
        uint32_t any = 0;
#pragma unroll
        for (int g = 0; g < kGrams; ++g) {
          const int64_t pos = seg + g * 64 + lane;
          hs[g] = 0;
          if (pos >= n || !csmh::char_start(p[pos])) continue;
          const int e = csmh::gram_end(p, n, (int)pos, a.width);
          if (e < 0) continue;  // fewer than `width` characters from here on
          hs[g] = csmh::murmur3_32(p + pos, e - (int)pos, a.seed);
          if (!have) any = hs[g];
          have |= 1u << g;
        }
        const unsigned long long owners = __ballot(have != 0);
        if (!owners) continue;
        const uint32_t fill = (uint32_t)__shfl((int)any, __ffsll((long long)owners) - 1, 64);
#pragma unroll
        for (int g = 0; g < kGrams; ++g)
          if (!((have >> g) & 1u)) hs[g] = fill;
        fold_segment(hs, a, ab, sig, lane);
      }
    }
    cstile::wave_lds_fence();
    uint32_t* g = out + r * a.nperm;
    for (int i = lane; i < a.nperm; i += 64) g[i] = sig[i];
    cstile::wave_lds_fence();  // (the signature is reset next round)
  }
}

__global__ void __launch_bounds__(256) k_band_keys(const uint32_t* __restrict__ sigs, int64_t rows, int nperm, int bands, int64_t* __restrict__ keys) {
  const int r = nperm / bands;
  const int64_t total = rows * bands;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
    const int64_t row = i / bands;
    const int j = (int)(i - row * bands);
    keys[i] = csmh::band_key(sigs + row * nperm + (int64_t)j * r, r, j);
  }
}

// one cs_minhash call, all of its parameters in sight
struct MinhashCall {
  const cs_column* col;
  int width;
  uint32_t seed;
  const uint32_t *a, *b;  // host
  int nperm;
  uint32_t* out;  // device
  hipStream_t s;
};

// a[] then b[], each padded to npad values (multiplier 1, addend 0: what they give is never stored), on the device
Buf upload_permutations(const MinhashCall& c, int npad) {
  const size_t bytes = sizeof(uint32_t) * 2 * (size_t)npad;
  uint32_t* h = (uint32_t*)pinned_scratch(bytes);
  for (int i = 0; i < npad; ++i) {
    h[i] = i < c.nperm ? c.a[i] : 1u;
    h[npad + i] = i < c.nperm ? c.b[i] : 0u;
  }
  const Buf ab = dev_alloc(bytes, c.s);
  CS_HIP(hipMemcpyAsync(ab->p, h, bytes, hipMemcpyHostToDevice, c.s));
  CS_HIP(hipStreamSynchronize(c.s));  // (the pinned scratch is free again)
  return ab;
}

bool wave_form_only() { return cfg_int("CS_MINHASH_WAVE", 0) != 0; }

void run_minhash(const MinhashCall& c) {
  MinhashArgs a{};
  a.in = view_of(c.col);
  a.width = c.width;
  a.nperm = c.nperm;
  a.npad = (c.nperm + kChunk - 1) / kChunk * kChunk;
  a.seed = c.seed;
  const Buf ab = upload_permutations(c, a.npad);
  // tile form: the staged rows and a hash slot per staged byte; the results' block where the widest tile's fits
  constexpr size_t kLdsCeiling = 150 * 1024;
  StagedTiles t;
  if (!wave_form_only()) t = plan_staged_tiles(c.col, cstile::kStageSlack, false, {5, 0, kLdsCeiling}, c.s);
  if (t.R) {
    const size_t block = sizeof(uint32_t) * (size_t)t.R * (size_t)c.nperm;
    if (block <= (size_t)kOutTileBytes && t.lds + 4 * block <= kLdsCeiling) a.out_cap = (int)((block + 15) & ~(size_t)15);
    t.lds += (size_t)4 * a.out_cap;
  }
  ProfScope ps("k_minhash", c.s);
  if (t.R) {
    a.rows_per_tile = t.R;
    a.cap = t.cap;
    a.ntiles = t.ntiles;
    if (a.out_cap) launch_resident(&k_minhash_tile<true>, t.lds, t.grid, c.s, a, ptr<const uint32_t>(ab), c.out);
    else launch_resident(&k_minhash_tile<false>, t.lds, t.grid, c.s, a, ptr<const uint32_t>(ab), c.out);
    note_route("tile");
  } else {
    a.out_cap = 0;
    launch_resident(&k_minhash_wave, sizeof(uint32_t) * 4 * (size_t)a.npad, (c.col->rows + 3) / 4, c.s, a, ptr<const uint32_t>(ab), c.out);
    note_route("wave");
  }
  CS_HIP(hipStreamSynchronize(c.s));  // (`ab` goes back to the pool behind this)
}

}  // namespace

extern "C" {

int cs_minhash(const cs_column* col, int width, uint32_t seed, const uint32_t* a, const uint32_t* b, int nperm, uint32_t* results, int on_device,
               cs_stream stream) {
  return guard([&] {
    if (!col || !a || !b || width < 1 || nperm < 1) fail(CS_ERR_INVALID_ARG, "minhash: bad arguments");
    if (width > csmh::kMaxWidth) fail(CS_ERR_RANGE, "minhash: an n-gram has at most 255 characters");
    if (nperm > csmh::kMaxPerm) fail(CS_ERR_RANGE, "minhash: at most 4096 permutations");
    for (int i = 0; i < nperm; ++i)
      if (a[i] == 0) fail(CS_ERR_RANGE, "minhash: a multiplier is 0");
    if (!results || col->rows == 0) return;  // nothing is written
    require_device();
    const hipStream_t s = S(stream);
    const ResultsOut res(results, sizeof(uint32_t) * (size_t)col->rows * (size_t)nperm, on_device, s);
    run_minhash(MinhashCall{col, width, seed, a, b, nperm, static_cast<uint32_t*>(res.dev), s});
    res.finish(s);
  });
}

int cs_minhash_bands(const uint32_t* signatures, int64_t rows, int nperm, int bands, int64_t* keys, int on_device, cs_stream stream) {
  return guard([&] {
    if (nperm < 1 || bands < 1 || nperm % bands != 0 || rows < 0 || (rows > 0 && !signatures)) fail(CS_ERR_INVALID_ARG, "minhash: bad band arguments");
    if (nperm > csmh::kMaxPerm) fail(CS_ERR_RANGE, "minhash: at most 4096 permutations");
    if (!keys || rows == 0) return;  // nothing is written
    require_device();
    const hipStream_t s = S(stream);
    const uint32_t* sigs = signatures;
    Buf staged;
    if (!on_device) {
      const size_t bytes = sizeof(uint32_t) * (size_t)rows * (size_t)nperm;
      staged = dev_alloc(bytes, s);
      CS_HIP(hipMemcpyAsync(staged->p, signatures, bytes, hipMemcpyHostToDevice, s));
      sigs = ptr<const uint32_t>(staged);
    }
    const ResultsOut res(keys, sizeof(int64_t) * (size_t)rows * (size_t)bands, on_device, s);
    hipLaunchKernelGGL(k_band_keys, dim3(std::min(blocks_for(rows * bands), 65536u)), dim3(kBlock), 0, s, sigs, rows, nperm, bands,
                       static_cast<int64_t*>(res.dev));
    CS_HIP(hipGetLastError());
    res.finish(s);
  });
}

}  // extern "C"
