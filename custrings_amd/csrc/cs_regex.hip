// The regex ops that build columns.  replace_re: the two-pass row-wise kernels, the kernel for the rows a single pass
// leaves as holes, the persistent single-pass kernel k_tdfa_replace_stream, the host route cs::replace_re_column
// (cs_internal.h: ReplaceCall) and cs_replace_re; replace_re with several patterns.  extract / findall /
// replace_with_backrefs: the row-wise span and backrefs kernels, the writers of the spans' bytes, the host routes on
// SpanRun and the C entries; regex_stream.h's kernel is instantiated here for MODE 3 (findall), 4 (extract), 5 and 6
// (replace_with_backrefs).  The compiled pattern is cs_regex_pattern.hip's, the scans are cs_regex_scan.hip's.
#include <hip/hip_runtime.h>

#include <atomic>
#include <list>

#include <cstring>

#include "cs_internal.h"
#include "device_utils.h"
#include "regex_program.h"
#include "regex_tdfa.h"
#include "regex_bits.h"
#include "regex_vm.h"
#include <mutex>

#include "tile_utils.h"
#include "regex_exec.h"
#include "regex_stream.h"
#include "splitre_ops.h"

using namespace cs;
using namespace csdev;
using namespace cs::rx;

namespace cs {
bool replace_class_runs(const cs_column* col, const int32_t* d_bits, const std::vector<int32_t>& bits, const char* repl, int rb, hipStream_t s, cs_column** out);
}

namespace {


// replace_re size pass: output bytes per row (-1 for null rows) + block sums
template <bool SMALL>
__global__ void k_replace_re_size(RowSrc src, Launch L, int rb, int maxrepl, int32_t* __restrict__ lens) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Ctx c = setup(L, src.flags, smem);
  const ColView& in = src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows) continue;
    int len = -1;
    if (row_is_valid(in.validity, r)) {
      int64_t b = in.offsets[r];
      int n = (int)(in.offsets[r + 1] - b);
      csvm::Vm<SMALL> vm(c.P, c.mem, c.stride, in.chars + b, n);
      len = n;
      csvm::row_replace_matches(vm, maxrepl, [&](int mb, int me, int reps) { len += reps * rb - (me - mb); });
    }
    lens[r] = len;
  }
}
template <bool SMALL>
__global__ void k_replace_re_write(RowSrc src, Launch L, const uint8_t* __restrict__ repl, int rb,
                                   int maxrepl, const int64_t* __restrict__ out_off,
                                   uint8_t* __restrict__ out_chars) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Ctx c = setup(L, src.flags, smem);
  const ColView& in = src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows || !row_is_valid(in.validity, r)) continue;
    int64_t b = in.offsets[r];
    int n = (int)(in.offsets[r + 1] - b);
    const uint8_t* p = in.chars + b;
    uint8_t* o = out_chars + out_off[r];
    int copied = 0;
    csvm::Vm<SMALL> vm(c.P, c.mem, c.stride, p, n);
    csvm::row_replace_matches(vm, maxrepl, [&](int mb, int me, int reps) {
      for (int i = copied; i < mb; ++i) *o++ = p[i];
      for (int k = 0; k < reps; ++k)
        for (int i = 0; i < rb; ++i) *o++ = repl[i];
      copied = me;
    });
    for (int i = copied; i < n; ++i) *o++ = p[i];
  }
}

// ---- extract (extract.cu:36-151): capture-group spans ------------------------------------
// One thread per row: find() the leftmost match (list simulator), then one anchored run per
// capture group with that group's ranges tracked (csvm::GroupVm).  The spans go to
// begins / lens [group * rows + row] (len -1 = null row); a second kernel copies the bytes.
// The thread lists live in a global arena (12 slots per instruction per thread), interleaved
// across the lanes of a workgroup so the list walks coalesce.
template <bool SMALL>
__global__ void __launch_bounds__(256) k_extract_spans(RowSrc src, Launch L, int groups, int32_t* __restrict__ begins,
                                                       int32_t* __restrict__ lens) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Ctx c = setup(L, src.flags, smem);
  const ColView& in = src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows) continue;
    int mb = 0, me = 0;
    bool hit = false;
    const int64_t b = in.offsets[r];
    const int n = (int)(in.offsets[r + 1] - b);
    if (row_is_valid(in.validity, r)) {
      csvm::Vm<SMALL> vm(c.P, c.mem, c.stride, in.chars + b, n);
      hit = vm.find(0, n, mb, me) > 0;
    }
    for (int g = 0; g < groups; ++g) {
      int x = 0, y = -1;
      if (hit) {
        csvm::GroupVm<SMALL> gv(c.P, c.mem, c.stride, in.chars + b, n);
        if (!csvm::row_group_span(gv, mb, g + 1, x, y)) y = -1;
      }
      begins[(int64_t)g * in.rows + r] = x;
      lens[(int64_t)g * in.rows + r] = y < 0 ? -1 : y - x;
    }
  }
}
struct ExtractOut {
  const int64_t* off[kMaxGroups];
  uint8_t* chars[kMaxGroups];
};
// thread per row: every group's span is copied by the row's thread (spans are short)
__global__ void __launch_bounds__(256) k_extract_write(ColView in, int groups, const int32_t* __restrict__ begins,
                                                       const int32_t* __restrict__ lens, ExtractOut out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= in.rows) return;
  const uint8_t* p = in.chars + in.offsets[r];
  for (int g = 0; g < groups; ++g) {
    const int len = lens[(int64_t)g * in.rows + r];
    if (len <= 0) continue;
    const uint8_t* q = p + begins[(int64_t)g * in.rows + r];
    uint8_t* o = out.chars[g] + out.off[g][r];
    for (int i = 0; i < len; ++i) o[i] = q[i];
  }
}

// The same on 64-row sub-tiles, a wave each (columns whose sub-tiles fit the staging buffer): the sub-tile's bytes
// arrive in LDS with whole 16-byte loads; per output column the row lanes put their span into the column's region
// with exact-size stores at any alignment (16 / 8 / 4 / 2 / 1 bytes from unaligned 16-byte reads of the staged row)
// and the wave flushes the region -- the 64 rows' spans are consecutive in the column's chars -- with aligned
// 16-byte stores.  The thread-per-row kernel above reads every row byte by byte from 64 different cache lines.
struct SpanWriteArgs {
  ColView in;
  int ncols;
  const int32_t* begins;
  const int32_t* lens;
  ExtractOut out;
  long long nsub;
  int cap;
};
__global__ void __launch_bounds__(256) k_spans_write_tile(SpanWriteArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;  // (scalar: what derives from it stays in SGPRs)
  uint8_t* lds_in = reinterpret_cast<uint8_t*>(smem) + (size_t)wv * (2 * a.cap + 64);
  uint8_t* region = lds_in + a.cap + 32;
  const ColView& in = a.in;
  for (long long tile = (long long)blockIdx.x * 4 + wv; tile < a.nsub; tile += (long long)gridDim.x * 4) {
    const long long r0 = tile * 64;
    const int nrows = (int)min(64ll, in.rows - r0);
    const cstile::TileOffs t = cstile::load_tile_offsets_r(in.offsets, in.rows, tile, 64, lane);
    const long long g0 = cstile::rl64(t.o0, 0), g1 = cstile::rl64(t.o1, 63);
    const int lead = (int)((uintptr_t)(in.chars + g0) & 15);
    const int want = (int)(g1 - g0) + lead;
    for (int i = lane * 16; i < want; i += 64 * 16) *reinterpret_cast<uint4*>(lds_in + i) = *reinterpret_cast<const uint4*>(in.chars + (g0 - lead) + i);
    const int rpos = lead + (int)(t.o0 - g0);
    cstile::wave_lds_fence();
    for (int g = 0; g < a.ncols; ++g) {
      const long long at = (long long)g * in.rows + r0 + lane;
      int len = lane < nrows ? a.lens[at] : 0;
      const int beg = len > 0 ? a.begins[at] : 0;
      if (len < 0) len = 0;
      const long long d0 = a.out.off[g][r0 + min(lane, nrows)];
      const long long base = cstile::rl64(d0, 0);
      const int total = (int)(cstile::rl64(d0, 63) - base) + __builtin_amdgcn_readlane(len, 63);
      if (total == 0) continue;
      const int di = (int)(d0 - base);
      for (int k = 0; k < len; k += 16)
        cstile::lds_put16(region + di + k, *reinterpret_cast<const cstile::lds_u32x4u*>(lds_in + rpos + beg + k), len - k);
      cstile::wave_lds_fence();
      cstile::wave_flush_shift(a.out.chars[g] + base, total, region, lane);
      cstile::wave_lds_fence();  // the next column re-uses the region
    }
  }
}

// The same from PACKED spans (begin << 16 | length, 0xFFFFFFFF = null; written by the scan stream kernels together with
// every tile's bytes per column), sizing the columns on the way: `tile_base[c][t]` = bytes of column c before tile t
// (the exclusive scan of the scan kernel's tile totals), so a tile's wave turns its rows' lengths into offsets itself --
// one wave scan per column -- and writes offsets, validity bits and chars.  The lengths -> offsets passes over every
// column (k_chunk_sums / k_chunk_offsets: 0.35 ms per column of 100M rows) and the write kernel's reads of the offsets
// they produced are gone, and the span arrays are half as large.
struct SpanOut2 {
  void* off[kMaxGroups];  // int32 offsets when every column stays below 2 GiB (half the offset bytes: as the split kernels write them), else int64
  uint8_t* chars[kMaxGroups];
  uint8_t* valid[kMaxGroups];
};
struct SpanWrite2Args {
  ColView in;
  int ncols;
  const uint32_t* spans;     // [column][row]
  const int64_t* tile_base;  // [column][nsub + 1]
  SpanOut2 out;
  long long nsub;
  int cap;
  int off32;
};
__global__ void __launch_bounds__(256) k_spans_write_tile2(SpanWrite2Args a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint8_t* lds_in = reinterpret_cast<uint8_t*>(smem) + (size_t)wv * (2 * a.cap + 64);
  uint8_t* region = lds_in + a.cap + 32;
  const ColView& in = a.in;
  // a wave walks a run of consecutive tiles with the next tile's chars in flight (register prefetch, tile_utils.h)
  const long long waves = (long long)gridDim.x * 4;
  const long long per = (a.nsub + waves - 1) / waves;
  long long tile = ((long long)blockIdx.x * 4 + wv) * per;
  const long long tile_end = min(a.nsub, tile + per);
  if (tile >= tile_end) return;
  cstile::TileOffs cur = cstile::load_tile_offsets_r(in.offsets, in.rows, tile, 64, lane);
  cstile::TileOffs nxt = cur;
  if (tile + 1 < tile_end) nxt = cstile::load_tile_offsets_r(in.offsets, in.rows, tile + 1, 64, lane);
  cstile::TileChars pf;
#pragma unroll
  for (int j = 0; j < cstile::kPfChunks; ++j) pf.v[j] = make_uint4(0, 0, 0, 0);
  cstile::issue_chars(in.chars, cstile::rl64(cur.o0, 0), cstile::rl64(cur.o1, 63), lane, pf);
  for (;;) {
    const long long r0 = tile * 64;
    const int nrows = (int)min(64ll, in.rows - r0);
    const long long g0 = cstile::rl64(cur.o0, 0), g1 = cstile::rl64(cur.o1, 63);
    const int lead = (int)((uintptr_t)(in.chars + g0) & 15);
    const int want = (int)(g1 - g0) + lead;
    const int rpos = lead + (int)(cur.o0 - g0);
    cstile::stage_chars(lds_in, want, lane, pf);
    // this tile's spans and column positions, the next tile's chars, the offsets of the one after (handed over at the bottom)
    uint32_t sp[4];
    long long cb[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      sp[g] = g < a.ncols && lane < nrows ? a.spans[(long long)g * in.rows + r0 + lane] : 0xFFFFFFFFu;
      cb[g] = g < a.ncols ? a.tile_base[(long long)g * (a.nsub + 1) + tile] : 0;
    }
    const bool has_next = tile + 1 < tile_end;
    const cstile::TileOffs nn = cstile::load_tile_offsets_r(in.offsets, in.rows, tile + 2 < tile_end ? tile + 2 : tile_end - 1, 64, lane);
    if (has_next) {
      cur = nxt;
      cstile::issue_chars(in.chars, cstile::rl64(cur.o0, 0), cstile::rl64(cur.o1, 63), lane, pf);
    }
    cstile::wave_lds_fence();
    for (int g = 0; g < a.ncols; ++g) {
      uint32_t w;
      long long base;
      if (g < 4) {  // (requested above)
        w = sp[0];
        base = cb[0];
#pragma unroll
        for (int c = 1; c < 4; ++c)
          if (c == g) {
            w = sp[c];
            base = cb[c];
          }
      } else {
        w = lane < nrows ? a.spans[(long long)g * in.rows + r0 + lane] : 0xFFFFFFFFu;
        base = a.tile_base[(long long)g * (a.nsub + 1) + tile];
      }
      const bool valid = w != 0xFFFFFFFFu;
      const int len = valid ? (int)(w & 0xFFFFu) : 0;
      const int beg = valid ? (int)(w >> 16) : 0;
      const int inc = csdev::wave_inclusive_scan(len);
      const int di = inc - len;
      const int total = __builtin_amdgcn_readlane(inc, 63);
      if (a.off32) {
        int32_t* o32 = static_cast<int32_t*>(a.out.off[g]);
        if (lane < nrows) o32[r0 + lane] = (int32_t)(base + di);
        if (tile + 1 == a.nsub && lane == nrows - 1) o32[in.rows] = (int32_t)(base + total);
      } else {
        int64_t* o64 = static_cast<int64_t*>(a.out.off[g]);
        if (lane < nrows) o64[r0 + lane] = base + di;
        if (tile + 1 == a.nsub && lane == nrows - 1) o64[in.rows] = base + total;
      }
      const unsigned long long vbits = __ballot(valid);
      if (lane == 0) *reinterpret_cast<unsigned long long*>(a.out.valid[g] + tile * 8) = vbits;
      if (total == 0) continue;
      for (int k = 0; k < len; k += 16)
        cstile::lds_put16(region + di + k, *reinterpret_cast<const cstile::lds_u32x4u*>(lds_in + rpos + beg + k), len - k);
      cstile::wave_lds_fence();
      cstile::wave_flush_shift(a.out.chars[g] + base, total, region, lane);
      cstile::wave_lds_fence();  // the next column re-uses the region
    }
    cstile::wave_lds_fence();  // the next tile overwrites lds_in
    if (!has_next) break;
    ++tile;
    nxt = nn;
  }
}

template <bool IN_LDS, bool WIDE = false>
__global__ void __launch_bounds__(256) k_tdfa_replace_size(RowSrc src, TLaunch L, int rb, int maxrepl,
                                                           int32_t* __restrict__ lens) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  TCtx c = tsetup<IN_LDS>(L, src.flags, smem);
  const ColView& in = src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows) continue;
    int len = -1;
    if (row_is_valid(in.validity, r)) {
      int64_t b = in.offsets[r];
      int n = (int)(in.offsets[r + 1] - b);
      typename std::conditional<WIDE, cstd::TdfaWide, cstd::Tdfa>::type vm(c.D, c.P, in.chars + b, n);
      vm.wide_ok = (b & ~(int64_t)3) + cstd::Tdfa::kMaskBytes <= src.safe_end;
      len = n;
      csvm::row_replace_matches(vm, maxrepl, [&](int mb, int me, int reps) { len += reps * rb - (me - mb); });
    }
    lens[r] = len;
  }
}
template <bool IN_LDS, bool WIDE = false>
__global__ void __launch_bounds__(256) k_tdfa_replace_write(RowSrc src, TLaunch L, const uint8_t* __restrict__ repl,
                                                            int rb, int maxrepl, const int64_t* __restrict__ out_off,
                                                            uint8_t* __restrict__ out_chars) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  TCtx c = tsetup<IN_LDS>(L, src.flags, smem);
  const ColView& in = src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows || !row_is_valid(in.validity, r)) continue;
    int64_t b = in.offsets[r];
    int n = (int)(in.offsets[r + 1] - b);
    const uint8_t* p = in.chars + b;
    uint8_t* o = out_chars + out_off[r];
    int copied = 0;
    typename std::conditional<WIDE, cstd::TdfaWide, cstd::Tdfa>::type vm(c.D, c.P, p, n);
    vm.wide_ok = (b & ~(int64_t)3) + cstd::Tdfa::kMaskBytes <= src.safe_end;
    csvm::row_replace_matches(vm, maxrepl, [&](int mb, int me, int reps) {
      for (int i = copied; i < mb; ++i) *o++ = p[i];
      for (int k = 0; k < reps; ++k)
        for (int i = 0; i < rb; ++i) *o++ = repl[i];
      copied = me;
    });
    for (int i = copied; i < n; ++i) *o++ = p[i];
  }
}

// replace_re of the rows in `list` (StreamArgs::hole_*): their output sizes (lens[i] for list[i]), or -- WRITE -- their bytes at
// the offsets the stream launch left them
template <bool WRITE>
__global__ void __launch_bounds__(256) k_tdfa_replace_list(RowSrc src, TLaunch L, const int32_t* __restrict__ list, int64_t count, const uint8_t* __restrict__ repl, int rb,
                                                           int32_t* __restrict__ lens, const int64_t* __restrict__ out_off, uint8_t* __restrict__ out_chars) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  TCtx c = tsetup<true>(L, src.flags, smem);
  const ColView& in = src.in;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    const int64_t r = list[i];
    if (!row_is_valid(in.validity, r)) continue;  // (a null row over bytes of the chars: no hole was left for it)
    const int64_t b = in.offsets[r];
    const int n = (int)(in.offsets[r + 1] - b);
    uint8_t* buf = reinterpret_cast<uint8_t*>(smem) + (((size_t)L.tdfa_words * 4 + 15) & ~(size_t)15) + (size_t)threadIdx.x * kListRowBytes;
    const uint8_t* p = list_row_to_lds(in.chars + b, n, buf, in.chars, in.chars + src.safe_end);
    cstd::Tdfa vm(c.D, c.P, p, n);
    vm.wide_ok = p != in.chars + b || (b & ~(int64_t)3) + cstd::Tdfa::kMaskBytes <= src.safe_end;
    if (!WRITE) {
      int len = n;
      csvm::row_replace_matches(vm, -1, [&](int mb, int me, int reps) { len += reps * rb - (me - mb); });
      lens[i] = len;
    } else {
      uint8_t* o = out_chars + out_off[r];
      int copied = 0;
      csvm::row_replace_matches(vm, -1, [&](int mb, int me, int reps) {
        for (int k = copied; k < mb; ++k) *o++ = p[k];
        for (int k = 0; k < reps; ++k)
          for (int q = 0; q < rb; ++q) *o++ = repl[q];
        copied = me;
      });
      for (int k = copied; k < n; ++k) *o++ = p[k];
    }
  }
}

// extract with the leftmost match found by the tagged DFA (table in LDS); only rows that hold a
// match run the list simulation, and only from the match start
template <bool IN_LDS, bool SMALL>
__global__ void __launch_bounds__(256) k_extract_spans_tdfa(RowSrc src, TLaunch TL, Launch L, int groups, int use_fast,
                                                            int32_t* __restrict__ begins, int32_t* __restrict__ lens) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  TCtx c = tsetup<IN_LDS>(TL, src.flags, smem);
  uint32_t* mem = L.arena + (size_t)blockIdx.x * blockDim.x * L.slots + threadIdx.x;
  // the head of every thread's lists and closure stack in LDS, behind the DFA table
  uint32_t* region = smem + (IN_LDS ? ((TL.tdfa_words + 3) & ~3) : 0);
  uint32_t* fast = use_fast ? region + threadIdx.x : nullptr;
  if (L.image_in_lds) {  // the program image behind the fast region: the list simulation fetches an instruction per step
    uint32_t* img = region + (use_fast ? 256 * csvm::GroupVm<true>::kFastSlots : 0);
    for (int i = threadIdx.x; i < L.image_words; i += blockDim.x) img[i] = (uint32_t)L.image[i];
    __syncthreads();
    c.P = csvm::make_view((const int32_t*)img, src.flags);
  }
  const ColView& in = src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows) continue;
    int mb = 0, me = 0;
    bool hit = false;
    const int64_t b = in.offsets[r];
    const int n = (int)(in.offsets[r + 1] - b);
    if (row_is_valid(in.validity, r)) {
      cstd::Tdfa vm(c.D, c.P, in.chars + b, n);
      vm.wide_ok = (b & ~(int64_t)3) + cstd::Tdfa::kMaskBytes <= src.safe_end;
      hit = vm.find(0, n, mb, me) > 0;
    }
    for (int g = 0; g < groups; ++g) {
      int x = 0, y = -1;
      if (hit) {
        csvm::GroupVm<SMALL> gv(c.P, mem, blockDim.x, in.chars + b, n, fast, blockDim.x);
        if (!csvm::row_group_span(gv, mb, g + 1, x, y)) y = -1;
      }
      begins[(int64_t)g * in.rows + r] = x;
      lens[(int64_t)g * in.rows + r] = y < 0 ? -1 : y - x;
    }
  }
}

// extract with the group ranges carried by the tagged DFA (Tdfa::group_find): the leftmost match, then
// one anchored DFA run per capture group -- no thread lists, no scratch memory
template <bool IN_LDS>
__global__ void __launch_bounds__(256) k_extract_spans_dfa(RowSrc src, TLaunch TL, const int32_t* __restrict__ gtags, int groups,
                                                           int32_t* __restrict__ begins, int32_t* __restrict__ lens) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  TCtx c = tsetup<IN_LDS>(TL, src.flags, smem);
  const ColView& in = src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows) continue;
    int mb = 0, me = 0;
    bool hit = false;
    const int64_t b = in.offsets[r];
    const int n = (int)(in.offsets[r + 1] - b);
    cstd::Tdfa vm(c.D, c.P, in.chars + b, n);
    vm.wide_ok = (b & ~(int64_t)3) + cstd::Tdfa::kMaskBytes <= src.safe_end;
    if (row_is_valid(in.validity, r)) hit = vm.find(0, n, mb, me) > 0;
    for (int g = 0; g < groups; ++g) {
      int x = -1, y = -1;
      const bool ok = hit && vm.group_find(mb, gtags, g + 1, x, y) && x >= 0 && y > x;
      begins[(int64_t)g * in.rows + r] = ok ? x : 0;
      lens[(int64_t)g * in.rows + r] = ok ? y - x : -1;
    }
  }
}

// ---- replace_with_backrefs (replace_backref.cu:36-207) ---------------------------------------
// Two passes, one thread per row (csvm::row_backrefs): sizes, then the bytes.  DFA: matches and group
// ranges by the tagged DFA (Tdfa::find / group_find); otherwise the list simulators over a global arena.
template <bool DFA, bool IN_LDS, bool SMALL, class Out>
__device__ __forceinline__ void backrefs_for_row(const TCtx& c, const csvm::ProgView& P, uint32_t* mem, int stride, const RowSrc& src,
                                                 const int32_t* gtags, const csvm::BackrefTemplate& t, int64_t r, Out&& out) {
  const ColView& in = src.in;
  const int64_t b = in.offsets[r];
  const int n = (int)(in.offsets[r + 1] - b);
  const uint8_t* p = in.chars + b;
  if constexpr (DFA) {
    cstd::Tdfa vm(c.D, c.P, p, n);
    vm.wide_ok = (b & ~(int64_t)3) + cstd::Tdfa::kMaskBytes <= src.safe_end;
    // the matches by the flat scan loop of replace_re (word-wise idle skipping), not by one find() per match
    csvm::row_backrefs(
        p, n, t, [&](auto&& f) { csvm::walk_matches(vm, f); },
        [&](int mb, int g, int& x, int& y) { return g == 0 ? vm.find(mb, mb + 1, x, y) > 0 : vm.group_find(mb, gtags, g, x, y) > 0; }, out);
  } else {
    csvm::row_backrefs(
        p, n, t,
        [&](auto&& f) {
          csvm::walk_matches_by_find(
              [&](int from, int& mb, int& me) {
                csvm::Vm<SMALL> vm(P, mem, stride, p, n);
                return vm.find(from, n, mb, me) > 0;
              },
              f);
        },
        [&](int mb, int g, int& x, int& y) {
          if (g == 0) {
            csvm::Vm<SMALL> vm(P, mem, stride, p, n);
            return vm.find(mb, mb + 1, x, y) > 0;
          }
          csvm::GroupVm<SMALL> gv(P, mem, stride, p, n);
          return gv.run(mb, g, x, y) > 0;
        },
        out);
  }
}
struct BackrefArgs {
  RowSrc src;
  TLaunch TL;
  Launch L;
  const int32_t* gtags;
  csvm::BackrefTemplate t;
};
template <bool DFA, bool IN_LDS, bool SMALL, bool WRITE>
__global__ void __launch_bounds__(256) k_backrefs(BackrefArgs a, int32_t* __restrict__ lens, const int64_t* __restrict__ out_off,
                                                  uint8_t* __restrict__ out_chars) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  TCtx c{};
  csvm::ProgView P{};
  uint32_t* mem = nullptr;
  if (DFA) {
    c = tsetup<IN_LDS>(a.TL, a.src.flags, smem);
  } else {
    P = csvm::make_view(a.L.image, a.src.flags);
    mem = a.L.arena + (size_t)blockIdx.x * blockDim.x * a.L.slots + threadIdx.x;
  }
  const ColView& in = a.src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows) continue;
    const bool valid = row_is_valid(in.validity, r);
    if (!WRITE) {
      int len = -1;
      if (valid) {
        len = 0;
        backrefs_for_row<DFA, IN_LDS, SMALL>(c, P, mem, blockDim.x, a.src, a.gtags, a.t, r, [&](const uint8_t*, int k) { len += k; });
      }
      lens[r] = len;
    } else if (valid) {
      uint8_t* o = out_chars + out_off[r];
      backrefs_for_row<DFA, IN_LDS, SMALL>(c, P, mem, blockDim.x, a.src, a.gtags, a.t, r, [&](const uint8_t* q, int k) {
        for (int i = 0; i < k; ++i) *o++ = q[i];
      });
    }
  }
}

// ---- replace_re with several patterns (replace_multi.cu:39-189) ----------------------------
// At every character position the patterns are tried in order, each anchored at that position
// (regexec.inl: start window [pos, pos + 1)); the first that matches is replaced and the walk
// continues behind the match.  Thread per row, size pass + write pass.  `first` holds, per
// pattern, the ASCII bytes an anchored match can begin with (a superset): most (position,
// pattern) pairs are turned away by one bit test.
struct MultiProg {
  const int32_t* tdfa;   // tagged DFA image (DFA variant)
  const int32_t* image;  // list-simulator image
  uint32_t first[4];     // ASCII bytes that can start a match; all ones when unknown
};
struct MultiArgs {
  RowSrc src;
  const MultiProg* progs;
  int nprogs;
  ColView repls;
  uint32_t* arena;  // list simulator scratch (VM variant)
  int slots;
};
template <bool DFA, bool WRITE>
__global__ void __launch_bounds__(256) k_multi_replace(MultiArgs a, int32_t* __restrict__ lens, const int64_t* __restrict__ out_off,
                                                       uint8_t* __restrict__ out_chars, unsigned* __restrict__ bad) {
  const ColView& in = a.src.in;
  uint32_t* mem = DFA ? nullptr : a.arena + (size_t)blockIdx.x * blockDim.x * a.slots + threadIdx.x;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows) continue;
    if (!row_is_valid(in.validity, r)) {
      if (!WRITE) lens[r] = -1;
      continue;
    }
    const int64_t b = in.offsets[r];
    const int n = (int)(in.offsets[r + 1] - b);
    const uint8_t* p = in.chars + b;
    uint8_t* o = WRITE ? out_chars + out_off[r] : nullptr;
    int total = n, copied = 0, pos = 0;
    while (pos < n) {
      const uint8_t c0 = p[pos];
      int mb = 0, me = 0;
      bool hit = false;
      int t = 0;
      for (; t < a.nprogs && !hit; ++t) {
        const MultiProg& mp = a.progs[t];
        if (c0 < 128 && !((mp.first[c0 >> 5] >> (c0 & 31)) & 1u)) continue;
        if (DFA) {
          const cstd::View D = cstd::make_view(mp.tdfa);
          const csvm::ProgView P = csvm::make_view(mp.image, a.src.flags);
          cstd::Tdfa vm(D, P, p, n);
          vm.wide_ok = false;
          hit = vm.find(pos, pos + 1, mb, me) > 0;
        } else {
          const csvm::ProgView P = csvm::make_view(mp.image, a.src.flags);
          csvm::Vm<false> vm(P, mem, blockDim.x, p, n);
          hit = vm.find(pos, pos + 1, mb, me) > 0;
        }
      }
      if (!hit) {
        unsigned w = csrow::lead_width(c0);
        pos += w ? (int)w : 1;
        continue;
      }
      --t;  // the pattern that matched
      if (me <= mb) {  // an empty match: the reference never leaves this position
        atomicOr(bad, 1u);
        break;
      }
      const int64_t rr = a.repls.rows == 1 ? 0 : t;
      const bool has = row_is_valid(a.repls.validity, rr);
      const int rn = has ? (int)(a.repls.offsets[rr + 1] - a.repls.offsets[rr]) : 0;
      total += rn - (me - mb);
      if (WRITE) {
        copy_bytes(o, p + copied, mb - copied);
        o += mb - copied;
        if (rn) copy_bytes(o, a.repls.chars + a.repls.offsets[rr], rn);
        o += rn;
        copied = me;
      }
      pos = me;
    }
    if (WRITE) copy_bytes(o, p + copied, n - copied);
    else lens[r] = total;
  }
}

// ---- findall (findall.cu:39-179): column k = every row's k-th match ------------------------
// The per-row match counts come from the count_re kernels; this pass walks the matches again
// (tagged DFA, or the list simulator) and leaves the first `ncols` spans in begins / lens
// [k * rows + row]  (len -1: the row has no k-th match).  k_extract_write copies the bytes.
__global__ void __launch_bounds__(256) k_max_i32(const int32_t* __restrict__ v, int64_t n, int* __restrict__ out) {
  int m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) m = max(m, v[i]);
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, m);
}
template <class VM>
__device__ __forceinline__ void findall_row(VM& vm, int64_t r, int64_t rows, int ncols, int32_t* __restrict__ begins,
                                            int32_t* __restrict__ lens) {
  const int k = csvm::row_findall(vm, [&](int j, int mb, int me) {
    if (j < ncols) {
      begins[(int64_t)j * rows + r] = mb;
      lens[(int64_t)j * rows + r] = me - mb;
    }
    return j + 1 < ncols;
  });
  for (int j = k; j < ncols; ++j) lens[(int64_t)j * rows + r] = -1;
}
template <bool IN_LDS>
__global__ void __launch_bounds__(256) k_findall_spans_tdfa(RowSrc src, TLaunch L, int ncols, int32_t* __restrict__ begins,
                                                            int32_t* __restrict__ lens) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  TCtx c = tsetup<IN_LDS>(L, src.flags, smem);
  const ColView& in = src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows) continue;
    if (!row_is_valid(in.validity, r)) {
      for (int j = 0; j < ncols; ++j) lens[(int64_t)j * in.rows + r] = -1;
      continue;
    }
    const int64_t b = in.offsets[r];
    cstd::Tdfa vm(c.D, c.P, in.chars + b, (int)(in.offsets[r + 1] - b));
    vm.wide_ok = (b & ~(int64_t)3) + cstd::Tdfa::kMaskBytes <= src.safe_end;
    findall_row(vm, r, in.rows, ncols, begins, lens);
  }
}
template <bool SMALL>
__global__ void k_findall_spans(RowSrc src, Launch L, int ncols, int32_t* __restrict__ begins, int32_t* __restrict__ lens) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  Ctx c = setup(L, src.flags, smem);
  const ColView& in = src.in;
  const int64_t nblk = (in.rows + blockDim.x - 1) / blockDim.x;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t r = blk * blockDim.x + threadIdx.x;
    if (r >= in.rows) continue;
    if (!row_is_valid(in.validity, r)) {
      for (int j = 0; j < ncols; ++j) lens[(int64_t)j * in.rows + r] = -1;
      continue;
    }
    const int64_t b = in.offsets[r];
    csvm::Vm<SMALL> vm(c.P, c.mem, c.stride, in.chars + b, (int)(in.offsets[r + 1] - b));
    findall_row(vm, r, in.rows, ncols, begins, lens);
  }
}

// ---- single-pass replace_re over row tiles (tile_utils.h) -----------------------------
// Used when the output is known not to outgrow the input (replacement no longer
// than the shortest possible match): the output buffer is allocated at the input
// size, every input byte is read once, the automaton runs once per row, and
// offsets come from a look-back scan inside the same kernel.
// CS_TILE_DEBUG (measurement switches of the stream kernels: phases skipped, other tile sequences, the decoupled look-back
// instead of the scanner team) exists in profiling builds only (make prof): in the product kernels the switches are
// compile-time zeros -- their cold code moved the hot loops out of the instruction cache (replace_re 5.4 -> 4.9 ms).
#if defined(CS_PHASE_PROF)
#define CS_DBG(a) ((a).debug)
#else
#define CS_DBG(a) 0
#endif
constexpr int kMaxRec = 4;  // matches per row kept in registers between the size and write phases

template <class VM, class Rec>
__device__ __forceinline__ int tile_row_size(VM& vm, int n, int rb, int maxrepl, Rec&& rec) {
  int len = n;
  csvm::row_replace_matches(vm, maxrepl, [&](int mb, int me, int reps) {
    len += reps * rb - (me - mb);
    rec(mb, me, reps);
  });
  return len;
}


// ---- persistent single-pass replace_re (tile_utils.h: sub-tile stream) ----------------
// (its non-persistent predecessor, k_tdfa_replace_tile -- one sub-tile a wave, plain look-back, reached only for replacements
// beyond 16 bytes that do not grow a row -- left the library in round 6: no test reached it, the two-pass kernels answer.)
// The grid is sized to
// the device's residency, wave `wid` of W walks sub-tiles wid, wid + W, ...; the chars of
// the next sub-tile are prefetched into registers while the current one is scanned, the
// look-back poll is issued before the output rows are assembled and consumed after, and
// the flush takes the destination alignment as it comes (no dependence of the assembly
// on the global position).
struct StreamArgs {
  ColView in;
  const uint8_t* flags;
  TLaunch L;
  const uint8_t* repl;
  int rb, maxrepl;
  int64_t* out_off;
  uint8_t* out_chars;
  cstile::u64* status;
  cstile::u64* excl;  // exclusive prefix per tile, written by the scanner wave (tile_utils.h: prefix_scanner)
  unsigned* error;
  long long nsub;
  int cap_in, cap_out, tbl_bytes;
  int debug;
  int outliers;  // the buffers are sized for all but a few sub-tiles: an oversize one is handled a thread per row in the kernel
  long long out_cap;  // bytes provisioned at out_chars (growing replacements)
  int rows_per_tile;  // LONG variants: 64, 32 or 16
  unsigned long long* tickets;  // 16 tile counters, 64 bytes apart, zeroed before the launch
  unsigned long long lit;       // UNITS: a literal needle (first byte lowest), litn bytes; litn == 0: none
  int litn;
  // BREFS (replace_with_backrefs on the unit scan): the template, the capture-group tag image and where both are
  // staged in LDS (behind the DFA table, inside tbl_bytes)
  const csvm::BackrefTemplate* tmpl;
  const int32_t* gtags;
  int gt_off, gt_words;
  // BITS: the bit-parallel form of the pattern (regex_bits.h), staged at byte offset bits_off of the LDS (inside tbl_bytes)
  const int32_t* bits;
  int bits_off, bits_words, bits_k;
  // HOLES (every form of 64-row tiles without a template; optional): the column's rows that hold a byte >= 0x80 or a NUL
  // (cs_virtual.hip: OddRows) are not scanned here.  Their output sizes were taken beforehand, a thread a row
  // (k_tdfa_replace_list<false>); a row lane of such a row leaves a hole of that size in the tile's output, which
  // k_tdfa_replace_list<true> fills after the launch -- and the other rows of its sub-tile keep the bit form / the chain
  // arithmetic / the unit scan, where one such row used to send all 64 to the row-by-row scan.
  const unsigned long long* hole_mask;  // [tile]
  const int64_t* hole_first;            // [tile]: index of the tile's first such row in hole_len
  const int32_t* hole_len;
};
#ifndef CS_STREAM_WAVES
#define CS_STREAM_WAVES 3
#endif
// REP16: replacement of 9..16 bytes (four registers) -- and, since round 3, of up to kMaxStreamRepl bytes, whose text the
// assembly reads from memory (a 21-byte replacement used to fall to the two-pass row kernels: 48.8 ms on the 100M-row column);
// the common short replacement keeps two registers.
constexpr int kMaxStreamRepl = 64;
// INPLACE (the output cannot outgrow the input): every row is compacted inside its own extent of
// the input tile while it is scanned -- the bytes before a match move down to the write cursor,
// the replacement follows -- so any number of matches per row costs no registers and the
// assembly is one contiguous copy per row.  Otherwise (growing replacement) up to kMaxRec matches
// per row are kept in registers and the rows are assembled piecewise; with RESCAN a row with more
// matches is scanned a second time during assembly (its size is known from the first scan),
// without it such a row fails the launch and the host repeats it with the RESCAN variant.
// LONG: rows of up to 255 bytes keep the lean scan (a sliding 96-byte window of candidate bits).
// the replacement text (rb <= 8 bytes in two registers) to an LDS position of any alignment: one to three stores
__device__ __forceinline__ void lds_put_short(uint8_t* at, uint32_t r0, uint32_t r1, int rb) {
  if (rb >= 8) {
    *reinterpret_cast<cstile::lds_u64u*>(at) = ((unsigned long long)r1 << 32) | r0;
    return;
  }
  if (rb & 4) {
    *reinterpret_cast<cstile::lds_u32u*>(at) = r0;
    at += 4;
    r0 = r1;
  }
  if (rb & 2) {
    *reinterpret_cast<cstile::lds_u16u*>(at) = (uint16_t)r0;
    at += 2;
    r0 >>= 16;
  }
  if (rb & 1) *at = (uint8_t)r0;
}



// The backrefs template in registers (the replace kernel's BREFS form).  The struct lives in device memory; read per match
// and per reference in the kernel's inner loops -- `T.nrefs`, `T.idx[j]`, `T.pos[j]` -- every read was a scalar load and a
// wait that also drains the LDS counter.  Up to sixteen references, group numbers up to 15 and positions up to 255 pack into
// three 64-bit words that stay in scalar registers; the host offers the single pass only to templates that fit.
struct TemplateRegs {
  int bytes, nrefs, groups;
  unsigned long long idx4, pos8lo, pos8hi;
  __device__ __forceinline__ int idx(int j) const { return (int)((idx4 >> (4 * j)) & 15ull); }
  __device__ __forceinline__ int pos(int j) const { return (int)(((j < 8 ? pos8lo >> (8 * j) : pos8hi >> (8 * (j - 8)))) & 255ull); }
};
__device__ __forceinline__ TemplateRegs template_regs(const csvm::BackrefTemplate* t) {
  TemplateRegs r;
  r.bytes = __builtin_amdgcn_readfirstlane(t->bytes);
  r.nrefs = __builtin_amdgcn_readfirstlane(t->nrefs);
  r.groups = __builtin_amdgcn_readfirstlane(t->groups);
  unsigned long long i4 = 0, lo = 0, hi = 0;
  for (int j = 0; j < csvm::BackrefTemplate::kMaxRefs; ++j) {
    const unsigned long long g = (unsigned long long)(t->idx[j] & 15), p = (unsigned long long)(t->pos[j] & 255);
    if (j < r.nrefs) {
      i4 |= g << (4 * j);
      if (j < 8) lo |= p << (8 * j);
      else hi |= p << (8 * (j - 8));
    }
  }
  r.idx4 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(i4 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)i4);
  r.pos8lo = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(lo >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)lo);
  r.pos8hi = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(hi >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)hi);
  return r;
}

// UNITS (with !INPLACE, RESCAN, !LONG): the scan runs per UNIT instead of per row (regex_tdfa.cpp, header word 31).
// Row lanes cut their rows into units with bit arithmetic on two per-byte bitmaps (candidate bytes, bytes equal
// to x) and queue them in LDS; then every lane takes a unit -- whichever row it belongs to -- and runs the lean scan
// over it, leaving a start bit and a last-byte bit per match in the (re-used) bitmaps, from which the row lanes
// read their rows' matches.  A wave's lock-step scan then costs the longest UNIT (a dotted quad) instead of the
// busiest ROW (two dotted quads and a status code), and runs that cannot hold a match are never scanned.
// PF: 16-byte chunks per lane of the register prefetch (1 KB of the sub-tile each): 6 covers every span the kernel
// takes; the unit variant also exists with 5 (spans up to 5 KB, the usual case), four registers less where it spills.
// BREFS (a UNITS variant): replace_with_backrefs in the same single pass.  The matches come from the unit scan; every
// row lane then runs ONE anchored group run per match of its row (Tdfa::group_find_all) to size the expansion of the
// template, keeps the group ranges of its first two matches, and assembles text pieces and group substrings straight
// from the staged row -- where the two-pass form ran the groups twice at two waves per SIMD and wrote its output a
// byte per lane.
// WIDE: programs of five to eight live threads (counted repetitions): no lean scan, the rows' generic scan with eight start
// offsets (regex_tdfa.h: TdfaWide) -- on the staged rows, where the two-pass kernels read them from memory a thread per row.
// OUTL: the buffers are sized for all but a few sub-tiles (one long row among millions of short ones); an oversize
// sub-tile's rows are sized and written a thread each, straight from memory, inside the prefix chain (separate forms:
// the code costs the others registers).
// HOLES: the hole words of StreamArgs are compiled in.  On by default -- the chain, bit and plain forms measured the same with
// and without them -- but the unit form proper (UNITS, no CHAIN), which literal needles ride too, lost 15 % to the eight registers
// (replace('a','xx') on C2: 0.73 -> 0.83 ms): it exists in both variants, and the host takes the one with holes only when it has some.
template <bool IN_LDS, bool REP16, bool INPLACE, bool RESCAN = false, bool LONG = false, bool UNITS = false, int PF = cstile::kPfChunks, bool BREFS = false,
          bool WIDE = false, bool OUTL = false, bool CHAIN = false, bool BITS = false, bool HOLES = true>
__global__ void __launch_bounds__(256, ((BREFS && !CHAIN) || (BITS && IN_LDS)) ? 2 : CS_STREAM_WAVES) k_tdfa_replace_stream(StreamArgs a) {
  // BITS (a CHAIN form): the pattern has a bit-parallel form (regex_bits.h) -- one bitmap per character class, staged by
  // table lookup; the row lanes derive their rows' matches from the class masks (alternations of word-bounded literals,
  // small sets in a `+` loop: patterns whose candidates are everywhere); a sub-tile with a byte >= 0x80 / NUL or a row
  // beyond the masks goes to the generic scan row by row.  A bitmap per class: two workgroups a CU.
  static_assert(!BITS || CHAIN, "the bit form is a chain-form variant (no unit / lean scans compiled in)");
  // CHAIN (a UNITS form): the pattern is a chain and a sample of the column holds no byte >= 0x80 -- the unit scan, the
  // literal scan and the lean scans are compiled out (their registers with them); a sub-tile the chain arithmetic does
  // not take (a non-ASCII byte after all, a row beyond the masks) goes to the generic scan row by row.
  static_assert(!CHAIN || UNITS, "the chain form is a unit-scan variant");
  // BREFS + CHAIN: replace_with_backrefs on a chain pattern whose groups are runs of items, a sample of the column plain ASCII
  // -- matches and group ranges by marker arithmetic alone, so no table, no group tags, no unit queue in LDS and none of the
  // unit / lean / group-run code in the kernel: three workgroups a CU where the backrefs form proper holds two.  A sub-tile
  // the arithmetic does not take gives the launch up exactly as it does there (error 32: the two-pass form).
  static_assert(!(BREFS && CHAIN) || (!IN_LDS && !BITS), "the backrefs chain form reads no table");
  static_assert(!OUTL || (IN_LDS && !LONG && !UNITS && !BREFS && !WIDE), "oversize sub-tiles: the plain forms only");
  static_assert(!UNITS || (!INPLACE && RESCAN && !LONG), "the unit scan builds on the register-record assembly");
  static_assert(!WIDE || (!UNITS && IN_LDS && !BREFS), "the wide form: generic scan only");
  static_assert(!BREFS || (UNITS && (IN_LDS || CHAIN) && !REP16), "the backrefs form is a unit-scan variant");
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  uint8_t* base = reinterpret_cast<uint8_t*>(smem);
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;  // (scalar: what derives from it stays in SGPRs)
  // one candidate bit per staged byte (BITS: sixteen bytes of slack instead of thirty-two -- a class bitmap is written up to
  // cap / 8 and read a few words beyond that into the next one, whose bits do not count: the seven bitmaps of the gtest
  // pattern then leave room for a third workgroup)
  const int bm_bytes = (a.cap_in >> 3) + (BITS ? 16 : 32);
  // second bitmap, unit queue, bail word (+ BREFS: a record of three words per match, a growth counter per row)
  const int nbm = BITS ? max(a.bits_k, 2) : 2;  // bitmaps per wave (BITS: one per character class)
  // (BREFS + CHAIN: the second bitmap, the bail word's slot and the match records -- no unit queue, no growth counters)
  // (CHAIN, BITS: no unit queue either)
  const int unit_bytes = (BREFS && CHAIN) ? bm_bytes + 16 + kUnitQueue * 12
                         : CHAIN          ? (nbm - 1) * bm_bytes + 16
                         : UNITS          ? (nbm - 1) * bm_bytes + kUnitQueue * 4 + 16 + (BREFS ? kUnitQueue * 12 + 64 * 4 : 0)
                                          : 0;
  uint8_t* lds_in = base + a.tbl_bytes + (size_t)wv * (a.cap_in + a.cap_out + 64 + bm_bytes + unit_bytes);
  uint8_t* lds_out = lds_in + a.cap_in + 32;
  uint32_t* bitmap = reinterpret_cast<uint32_t*>(lds_out + a.cap_out + 32);
  uint32_t* xbitmap = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(bitmap) + bm_bytes);  // UNITS: "byte == x", later the matches' last bytes
  uint32_t* uqueue = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(bitmap) + (size_t)nbm * bm_bytes);
  uint32_t* bailw = uqueue + (CHAIN ? 0 : kUnitQueue);  // one bit per row: the lean scan handed a unit of the row over
  uint32_t* mrec = bailw + 4;              // BREFS: per match (group ranges of groups 1-2, of groups 3-4, match end | ok << 8)
  uint32_t* rowgrow = mrec + kUnitQueue * 3;  // BREFS: bytes the row's expansions add
  const TCtx c = tsetup<IN_LDS>(a.L, a.flags, smem);  // (block barrier inside when staging)
  const cstd::View& D = c.D;
  const csvm::ProgView& P = c.P;
  const ColView& in = a.in;
  const int rb = a.rb;
  const int32_t* gt = nullptr;    // BREFS: the group tags and the template text, in LDS
  const uint8_t* ttext = nullptr;
  if (BREFS) {
    int32_t* g = reinterpret_cast<int32_t*>(base + a.gt_off);
    for (int i = threadIdx.x; i < a.gt_words; i += blockDim.x) g[i] = a.gtags[i];
    uint8_t* tt = base + a.gt_off + ((a.gt_words * 4 + 15) & ~15);
    const int tb = a.tmpl->bytes;
    for (int i = threadIdx.x; i < tb; i += blockDim.x) tt[i] = a.tmpl->text[i];
    __syncthreads();
    gt = g;
    ttext = tt;
  }
  TemplateRegs T{};
  if (BREFS) T = template_regs(a.tmpl);
  const uint32_t* spread = nullptr;
  csbits::View BV{};
  if (BITS) {
    int32_t* bl = reinterpret_cast<int32_t*>(base + a.bits_off);
    spread = bits_stage(a.bits, a.bits_words, bl);
    BV = csbits::make_view(bl);
  }
  const bool has_r2 = (((uint32_t)D.img[30] & 255u) <= (((uint32_t)D.img[30] >> 8) & 255u));
  const uint32_t unit_x = (D.units >> 8) & 127u, unit_xpat = unit_x * 0x01010101u;
  // rows per tile: 64, or fewer for the long-row variants (so that the tile fits the prefetch registers)
  const int R = LONG ? a.rows_per_tile : 64;
  // Tiles are handed out by tickets, so every tile's predecessors were started before it and a
  // wave that meets a slow tile does not hold back the tiles it would have taken next (with a static
  // round-robin the look-back of everybody else waits for them).  One counter per class of
  // workgroups (blockIdx mod K, K = 16): counter k hands out tiles k, k + K, ...; a single word hands out some 65 tickets a
  // microsecond (measured with the strip kernel, cs_rows.hip), this kernel takes 320 -- eight counters ran at 40 each and
  // still cost 0.1 ms against sixteen (4.87 -> 4.75 ms; thirty-two: the same).  The
  // ticket of the tile after next is in flight while the current tile is processed.
  // (sixteen for the launches that hold three workgroups a CU; the slower forms -- two a CU -- measured a little better with eight)
  const long long K = gridDim.x >= 640 ? 16 : (gridDim.x >= 16 ? 8 : 1);  // (every class needs a workgroup that takes tiles: workgroup 0 may be the scanners')
  const long long key = (long long)blockIdx.x % K;
  const bool fixed = (CS_DBG(a) & (256 | 16384)) != 0;  // measurement: the static round-robin
  // Workgroup 0 takes no tiles: its four waves turn the aggregates the other waves publish into each tile's exclusive
  // prefix, in order (a tile then needs ONE load instead of a walk over its predecessors' words): tile_utils.h,
  // prefix_scanner_team.  (debug 512: the decoupled look-back, for comparison; debug 1024: the single scanner wave.)
  const bool fixed_team = (CS_DBG(a) & 16384) != 0 && gridDim.x > 1;  // measurement: the static round-robin with the scanner team
  const bool team = (fixed_team || !fixed) && !(CS_DBG(a) & (512 | 1024)) && gridDim.x > 1;
  const bool scanner = team || (!fixed && !(CS_DBG(a) & 512) && a.cap_in + a.cap_out + 32 >= cstile::kScanBatch * 512);
  if (team && blockIdx.x == 0) {
    cstile::TeamRing* ring = reinterpret_cast<cstile::TeamRing*>(lds_in - (size_t)wv * (a.cap_in + a.cap_out + 64 + bm_bytes + unit_bytes));
    if (threadIdx.x < 8) cstile::team_ring_init(ring, threadIdx.x);
    __syncthreads();
    if (cstile::prefix_scanner_team(a.status, a.excl, a.nsub, lane, wv, 4, ring, a.error) == 1 && lane == 0) atomicOr(a.error, 1u | 16u);  // (16: the scanners timed out)
    return;
  }
  if (scanner && !team && blockIdx.x == 0 && wv == 0) {
    // (its tile buffers are free: they hold the fetched status words)
    if (!cstile::prefix_scanner(a.status, a.excl, a.nsub, lane, reinterpret_cast<cstile::u64*>(lds_in)) && lane == 0)
      atomicOr(a.error, 1u | 16u);  // (16: the scanner wave timed out)
    return;
  }
  const long long W = (long long)gridDim.x * 4;
  unsigned long long* my_ticket = a.tickets + key * 8;
  auto take = [&]() -> unsigned long long {
    unsigned long long t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(my_ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return t;
  };
  auto tile_of = [&](unsigned long long t) -> long long { return (long long)cstile::rl64((long long)t, 0) * K + key; };
  long long tile, t_nxt, t_nn = 0;
  unsigned long long pending = 0;
  if (fixed_team) {  // (workgroup 0 is the scanners')
    tile = ((long long)blockIdx.x - 1) * 4 + wv;
    t_nxt = tile + W - 4;
  } else if (fixed) {
    tile = (long long)blockIdx.x * 4 + wv;
    t_nxt = tile + W;
  } else {
    // A wave's first three tickets are drawn ONE AT A TIME, each after the one before has arrived (the tile number is
    // read out of it) and the first tile's loads have been issued: drawn back to back they are consecutive numbers, a wave's
    // second and third tile then lie in front of its neighbour's first, whose prefix has to wait for them -- a dependency
    // chain through every wave of the class.  A round trip apart they land among the other waves' tickets of the same round, as in the steady state (one
    // ticket a wave and iteration).  Nothing here counts waves: workgroups that are not resident draw nothing.
    const unsigned long long q0 = take();
    tile = tile_of(q0);
    t_nxt = a.nsub;  // (known below)
  }
  if (tile >= a.nsub) return;
  // replacement text in registers (this kernel is only taken for rb <= 8, or <= 16 with REP16)
  constexpr int kRepRegs = REP16 ? 4 : 2;
  uint32_t rep[kRepRegs];
#pragma unroll
  for (int i = 0; i < kRepRegs; ++i) rep[i] = 0;
#pragma unroll
  for (int i = 0; i < 4 * kRepRegs; ++i)
    if (i < rb) rep[i >> 2] |= (uint32_t)a.repl[i] << (8 * (i & 3));
  cstile::TileOffs cur = cstile::load_tile_offsets_r(in.offsets, in.rows, tile, R, lane);
  cstile::TileCharsT<PF> pf;
#pragma unroll
  for (int j = 0; j < PF; ++j) pf.v[j] = make_uint4(0, 0, 0, 0);
  cstile::issue_chars(in.chars, cstile::rl64(cur.o0, 0), cstile::rl64(cur.o1, 63), lane, pf);
  if (!fixed) {
    const unsigned long long q1 = take();
    t_nxt = tile_of(q1);
  }
  cstile::TileOffs nxt = cur;
  if (t_nxt < a.nsub) nxt = cstile::load_tile_offsets_r(in.offsets, in.rows, t_nxt, R, lane);
  if (!fixed) pending = take();
  // The previous sub-tile's output stays assembled in lds_out while this one is scanned;
  // its look-back completes afterwards, when every predecessor's aggregate has long been
  // published, so waves do not wait on each other's scans.
  long long p_tile = -1;
  int p_total = 0, p_lo = 0, p_len = 0;
  int m_span = 0;  // the output column's largest 64-row span as a by-product (wave-uniform: a scalar maximum per sub-tile)
  // HOLES: the tile's mask of rows that are sized and written elsewhere, and where their sizes begin -- fetched a tile ahead,
  // like the offsets (unconditionally, from a harmless address when the launch has none: see the note at the first poll)
#if defined(CS_NO_HOLE_FORMS)  // (measurement: the kernels without the hole words)
  constexpr bool kHoles = false;
#else
  constexpr bool kHoles = HOLES && !BREFS && !LONG && !OUTL && !WIDE;
#endif
  const bool holes = kHoles && a.hole_mask != nullptr;
  // (the column's first offsets: read-only, sixteen bytes at least -- not the ticket words, which every wave's atomics hammer)
  const unsigned long long* hole_mask_p = holes ? a.hole_mask : reinterpret_cast<const unsigned long long*>(in.offsets);
  const int64_t* hole_first_p = holes ? a.hole_first : in.offsets;
  unsigned long long c_hm = 0;
  long long c_hf = 0;
  if (kHoles) {
    c_hm = hole_mask_p[holes ? tile : 0];
    c_hf = hole_first_p[holes ? tile : 0];
  }
#if defined(CS_PHASE_PROF)
  unsigned long long phase_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long lb_acc[3] = {0, 0, 0};
  unsigned long long phase_t = __builtin_readcyclecounter();
#endif
  auto finish_pending = [&](cstile::u64 first) {
    long long gb;
    if (lane == 0) CS_TILE_TRACE(p_tile, 2);
    if (CS_DBG(a) & 128) {  // measurement only: one late poll, no chase for an inclusive prefix
      const cstile::u64 v = cstile::lookback_poll(a.status, p_tile, lane);
      const int part = (int)(unsigned)(v & 0xffffffffull);
      gb = p_tile * 4096 + (csdev::wave_reduce_sum(part) & 0) + (long long)(first & 0);
      if (lane == 0) cstile::status_store(a.status + p_tile, cstile::kFlagInc | 1);
    } else if (__builtin_expect(scanner, 1)) {
      gb = (CS_DBG(a) & 8) ? p_tile * 4096 : cstile::prefix_wait(a.excl, p_tile, first, a.error, lane);
    } else {
#if defined(CS_PHASE_PROF)
      gb = (CS_DBG(a) & 8) ? p_tile * 4096 : cstile::lookback_end(a.status, p_tile, p_total, first, lane, lb_acc);
#else
      gb = (CS_DBG(a) & 8) ? p_tile * 4096 : cstile::lookback_end(a.status, p_tile, p_total, first, lane);
#endif
    }
    if (gb < 0) {
#if defined(CS_PHASE_PROF)  // (a device printf costs every variant of this kernel thousands of instructions: profiling builds only)
      if (lane == 0 && (CS_DBG(a) & 2048)) printf("no prefix: tile %lld (wave %d of block %d, current tile %lld) error %u\n", p_tile, wv, (int)blockIdx.x, tile, *a.error);
#endif
      if (lane == 0) atomicOr(a.error, 1u | 8u);  // (8: no prefix for the tile)
      gb = 0;
    }
    CS_PHASE_MARK(6);
    if (lane == 0) CS_TILE_TRACE(p_tile, 3);
    const long long pr0 = p_tile * R;
    const int pn = (int)min((long long)R, in.rows - pr0);
#if defined(CS_NT_STORES)
    if (lane < pn) __builtin_nontemporal_store(gb + p_lo, a.out_off + pr0 + lane);
#else
    if (lane < pn) a.out_off[pr0 + lane] = gb + p_lo;
#endif
    if (lane == pn - 1 && pr0 + pn == in.rows) a.out_off[in.rows] = gb + p_lo + p_len;
    if (!INPLACE && gb + p_total > a.out_cap) {  // more growth than the host provisioned for
      if (lane == 0) atomicOr(a.error, 2u);
      return;
    }
    if (!(CS_DBG(a) & 4)) cstile::wave_flush_shift(a.out_chars + gb, p_total, lds_out, lane);
  };
  for (;;) {
    const long long r0 = tile * R;
    const int nrows = (int)min((long long)R, in.rows - r0);
    const long long g0 = cstile::rl64(cur.o0, 0), g1 = cstile::rl64(cur.o1, 63);
    const bool live0 = lane < nrows && row_is_valid(in.validity, r0 + lane);
    const int rbeg = (int)(cur.o0 - g0);
    const int n0 = live0 ? (int)(cur.o1 - cur.o0) : 0;
    const int lead = (int)((uintptr_t)(in.chars + g0) & 15);
    const long long want = g1 - g0 + lead;
    bool bad = want + 16 > a.cap_in || want > PF * 1024;
    // A sub-tile beyond the staging buffer.  The host sizes the buffers for all but a few sub-tiles when the column's
    // largest does not fit (one long row among millions of short ones): such a sub-tile's rows are sized and written a
    // thread each, straight from memory -- inside the prefix chain -- instead of the whole column leaving the single pass.
    const bool oversize = OUTL && bad && a.outliers;
    if (!bad) cstile::stage_chars(lds_in, (int)want, lane, pf);
    CS_PHASE_MARK(9);   // (wait for the prefetched chars + the LDS writes)
    // bytes that the lean scan does not take (non-ASCII, NUL) anywhere in the staged span, and one
    // candidate bit per byte for the row lanes (classified here, out of the prefetch registers)
    uint32_t odd = 0;
#pragma unroll
    for (int j = 0; j < PF; ++j)
      if (j * 1024 + lane * 16 < (int)want) {
        uint4 q = pf.v[j];
        if (__builtin_expect(tile + 1 == a.nsub && j * 1024 + lane * 16 + 16 > (int)want, 0)) {
          // the column's last piece: what lies behind its last byte is allocation slack, not data (zeros there made the
          // last sub-tile look as if it held NUL bytes and sent it to the generic scan)
          const int keep = (int)want - (j * 1024 + lane * 16);  // 1..15 bytes of data
          auto cut = [&](uint32_t w, int k) {
            const int left = keep - 4 * k;
            const uint32_t m = left >= 4 ? 0xFFFFFFFFu : (left <= 0 ? 0u : (1u << (8 * left)) - 1u);
            return (w & m) | (0x20202020u & ~m);
          };
          q = make_uint4(cut(q.x, 0), cut(q.y, 1), cut(q.z, 2), cut(q.w, 3));
        }
        odd |= q.x | ((q.x - 0x01010101u) & ~q.x);
        odd |= q.y | ((q.y - 0x01010101u) & ~q.y);
        odd |= q.z | ((q.z - 0x01010101u) & ~q.z);
        odd |= q.w | ((q.w - 0x01010101u) & ~q.w);
        if (BITS) {
          uint32_t pair[4];
          bits_classify16(spread, q, pair);
#pragma unroll
          for (int k = 0; k < csbits::kMaxClasses; ++k)
            if (k < BV.K && !bad) cstile::put_bits16(bitmap + k * (bm_bytes >> 2), j * 1024 + lane * 16, (pair[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
          continue;
        }
        uint32_t bits;
        if (has_r2)
          bits = cstile::gather16_bit7(cstd::Tdfa::cand_bits_ascii<true>(D, q.x), cstd::Tdfa::cand_bits_ascii<true>(D, q.y), cstd::Tdfa::cand_bits_ascii<true>(D, q.z),
                                       cstd::Tdfa::cand_bits_ascii<true>(D, q.w));
        else
          bits = cstile::gather16_bit7(cstd::Tdfa::cand_bits_ascii<false>(D, q.x), cstd::Tdfa::cand_bits_ascii<false>(D, q.y), cstd::Tdfa::cand_bits_ascii<false>(D, q.z),
                                       cstd::Tdfa::cand_bits_ascii<false>(D, q.w));
        if (!bad) cstile::put_bits16(bitmap, j * 1024 + lane * 16, bits);
        if (UNITS && unit_x != 0 && !bad) cstile::put_bits16(xbitmap, j * 1024 + lane * 16, unit_xbits16(q, unit_xpat));
      }
    // first look-back poll for the previous sub-tile: issued only now, after the staging above has
    // waited for its own data (vmcnt is in order: a poll issued earlier would sit in front of it)
    CS_PHASE_MARK(10);  // (classification into the bitmaps)
    // Everything fetched here for later -- the poll, the ticket, the offsets two tiles ahead -- is assigned
    // UNCONDITIONALLY (clamped addresses) and handed to its loop-carried variable only at the bottom of the iteration:
    // a conditional assignment of a value that is still in flight makes the compiler copy it at the join of the branch,
    // i.e. wait for the load right behind its issue -- s_waitcnt vmcnt(0), which drained the whole prefetch every
    // iteration (found in the ISA of every stream kernel; the "prefetch" had never overlapped anything).
    cstile::u64 p_first, p_second;
    bool has_second = false;
    {
      const long long pt = p_tile >= 0 ? p_tile : 0;
      p_first = __builtin_expect(scanner, 1) ? cstile::status_load(a.excl + pt) : cstile::lookback_poll(a.status, pt, lane);
    }
    // keep the memory pipe busy: next sub-tile's chars, and the offsets of the one after
    const bool has_next = t_nxt < a.nsub;
    t_nn = fixed ? t_nxt + (fixed_team ? W - 4 : W) : tile_of(pending);
    const unsigned long long pending_new = fixed ? 0ull : take();  // (tickets drawn past the end are harmless)
    const cstile::TileOffs nn = cstile::load_tile_offsets_r(in.offsets, in.rows, t_nn < a.nsub ? t_nn : a.nsub - 1, R, lane);
    unsigned long long n_hm = 0;
    long long n_hf = 0;
    if (kHoles) {
      const long long tq = holes ? (has_next ? t_nxt : tile) : 0;
      n_hm = hole_mask_p[tq];
      n_hf = hole_first_p[tq];
    }
    if (has_next) {
      cur = nxt;
      cstile::issue_chars(in.chars, cstile::rl64(cur.o0, 0), cstile::rl64(cur.o1, 63), lane, pf);
    }
    cstile::wave_lds_fence();
    CS_PHASE_MARK(0);
    // HOLES: the rows of this sub-tile that hold a byte >= 0x80 or a NUL take no part below -- and the others are plain
    bool hole = false, tile_plain = false;
    int hole_bytes = 0;
    if (kHoles && holes && !bad) {
      const unsigned long long hm = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(c_hm >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)c_hm);
      // (a row beyond the masks: the sub-tile goes row by row as before -- its rows of the list are then written twice, the same bytes)
      tile_plain = !__any(live0 && n0 + ((lead + rbeg) & 3) > cstd::Tdfa::kMaskBytes);
      if (tile_plain && hm) {
        hole = live0 && ((hm >> lane) & 1ull) != 0;
        if (hole) hole_bytes = a.hole_len[cstile::rl64(c_hf, 0) + __builtin_popcountll(hm & ((1ull << lane) - 1ull))];
      }
    }
    const bool live = live0 && !hole;
    const int n = live ? n0 : 0;

    int rec_mb[kMaxRec], rec_me[kMaxRec], rec_reps[kMaxRec];
    int nm = 0;
    int out_len = 0;
    cstd::U128 uS = cstd::u128(0, 0), uE = cstd::u128(0, 0);  // UNITS: the row's match starts / last bytes
    bool from_masks = false;
    int mslot = 0;  // BREFS: where the row's matches stand in the match queue / record table
    bool dense_tile = false;  // BREFS + CHAIN: more matches than the record table holds -- the assembly derives the groups again
    if (live && !bad) out_len = n;
    if (oversize && live) {  // the row's output size by the generic scan on the row in memory
      cstd::Tdfa vg(D, P, in.chars + (g0 + rbeg), n);
      int len = n;
      auto add = [&](int mb, int me, int reps) { len += reps * rb - (me - mb); };
      if (WIDE) vg.template scan<cstd::Tdfa::K_REPLACE, decltype(add)&, cstd::kMaxSlotsWide>(a.maxrepl, add, 0, 0);
      else vg.template scan<cstd::Tdfa::K_REPLACE>(a.maxrepl, add, 0, 0);
      out_len = len;
    }
    if (!bad && !(CS_DBG(a) & 1)) {
      cstd::Tdfa vm(D, P, lds_in + lead + rbeg, n, (lead + rbeg) & 3);
      const int pi = lead + rbeg;          // byte index of the row in lds_in
      int wr = 0, copied = 0, pend = -1;   // INPLACE: write cursor, input consumed, replacement not yet written
      auto put_repl_at = [&](int at) {
        if (REP16) {
          if (rb > 16) {  // (a long replacement: its bytes from memory, the same for every lane)
            for (int i = 0; i < rb; ++i) lds_in[pi + at + i] = a.repl[i];
          } else {
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (i < rb) lds_in[pi + at + i] = (uint8_t)(rep[i >> 2] >> (8 * (i & 3)));
          }
        } else {
          lds_put_short(lds_in + pi + at, rep[0], rep[1], rb);
        }
      };
      auto rec = [&](int mb, int me, int reps) {
        if (INPLACE) {
          // the previous match's replacement is written only now: until the next round has started the
          // scan may still look at the byte in front of that match's end (word / line context)
          if (pend >= 0) put_repl_at(pend);
          if (wr != copied) cstile::lds_copy(lds_in, pi + wr, lds_in, pi + copied, mb - copied);  // moves down: ascending copy is safe
          wr += mb - copied;
          pend = wr;
          wr += reps * rb;  // (reps > 1 only for patterns that match the empty string, where rb == 0)
          copied = me;
        } else {
          out_len += reps * rb - (me - mb);
          // (UNITS: the rows that come through here -- non-ASCII sub-tiles, rows a unit handed over -- are only
          // measured; the assembly scans them again.  Twelve registers less in a kernel at its VGPR limit, whose
          // spill reloads -- VMEM operations -- otherwise wait behind the prefix poll in every iteration.)
          if (!UNITS) {
#pragma unroll
            for (int j = 0; j < kMaxRec; ++j)
              if (nm == j) {
                rec_mb[j] = mb;
                rec_me[j] = me;
                rec_reps[j] = reps;
              }
          }
        }
        ++nm;
      };
      // wave-uniform choice: the lean scan when every row of the sub-tile qualifies
      const bool has_odd = !tile_plain && __any((odd & 0x80808080u) != 0);
      // (a sub-tile with bytes >= 0x80, a pattern they can only kill: the UNIT route alone -- reclassify_high)
      bool hi_units = false;
      if (!CHAIN && UNITS && !BREFS && has_odd && a.litn == 0 && ((D.units >> 17) & 3u) && (D.units & 1u) && a.maxrepl < 0 && !(CS_DBG(a) & 4096))
        hi_units = !reclassify_high(D, has_r2, lds_in, (int)want, lane, bitmap, a.flags, lds_in + lead + rbeg, n);
      const bool lean = D.nskip > 0 && D.img[12] <= 4 && !(CS_DBG(a) & 32) && (!has_odd || hi_units) &&
                        !__any(live && (LONG ? n > cstd::Tdfa::kLongBytes : !vm.masks_fit()));
      bool redo = live && !lean && a.maxrepl != 0;
      int resume = 0;
      bool units_done = false;
      from_masks = false;
      if (!CHAIN && UNITS && a.litn > 0) {
        // A literal needle without a border: every match of the sub-tile by byte comparison, sixteen positions per
        // lane and step -- no automaton.  Match starts land in `bitmap`; `xbitmap` holds the row starts, so that a
        // match never spans two rows (or the end of the staged span).  Rows of any bytes qualify (an ASCII needle
        // never matches inside a multi-byte character), rows beyond the 96-bit masks do not.
        if (a.maxrepl < 0 && !__any(live && !vm.masks_fit())) {  // (wave-uniform)
          using namespace cstd;
          const int m = a.litn;
          for (int i = lane * 16; i < bm_bytes; i += 64 * 16) *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(xbitmap) + i) = make_uint4(0, 0, 0, 0);
          cstile::wave_lds_fence();
          {
            const int p = lane < nrows ? lead + rbeg : (int)want;  // (every row, null or not)
            __hip_atomic_fetch_or(xbitmap + (p >> 5), 1u << (p & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            // and the end of the staged span: the last row's match must not run on into the next sub-tile's bytes
            if (lane == 0) __hip_atomic_fetch_or(xbitmap + ((int)want >> 5), 1u << ((int)want & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
          }
          cstile::wave_lds_fence();
#pragma unroll
          for (int j = 0; j < PF; ++j) {
            const int i = j * 1024 + lane * 16;
            if (i < (int)want) {
              const uint32_t* wp = reinterpret_cast<const uint32_t*>(lds_in + i);
              const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3], w4 = wp[4], w5 = wp[5];
              uint32_t M = 0xFFFFFFu;
              for (int k = 0; k < m; ++k) {
                const uint32_t cpat = (uint32_t)((a.lit >> (8 * k)) & 255u) * 0x01010101u;
                auto eq = [&](uint32_t w) {
                  const uint32_t t = w ^ cpat;
                  return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
                };
                const uint32_t hi8 = __builtin_amdgcn_udot4(eq(w5), 0x80402010u, __builtin_amdgcn_udot4(eq(w4), 0x08040201u, 0u, false), false) >> 7;
                M &= (cstile::gather16_bit7(eq(w0), eq(w1), eq(w2), eq(w3)) | (hi8 << 16)) >> k;
              }
              // row starts at i .. i + 23 (a row start at p + k, 0 < k < m, forbids a match at p)
              const uint32_t* xb = xbitmap + (i >> 5);
              const unsigned sh = (unsigned)(i & 31);
              const uint32_t rs = sh ? (xb[0] >> sh) | (xb[1] << (32 - sh)) : xb[0];
              for (int k = 1; k < m; ++k) M &= ~(rs >> k);
              const int room = (int)want - i;  // positions of this piece inside the staged span
              if (room < 16) M &= (1u << room) - 1u;
              cstile::put_bits16(bitmap, i, M & 0xFFFFu);
            }
          }
          cstile::wave_lds_fence();
          uint32_t s0, s1, s2;
          cstile::row_bits96(bitmap, lead + rbeg, n, s0, s1, s2);
          if (live) {
            uS = u128(s0 | ((unsigned long long)s1 << 32), s2);
            const int up = m - 1;  // the match's last byte
            uE = up ? u128(uS.lo << up, (uS.hi << up) | (uS.lo >> (64 - up))) : uS;
            nm = u128_popc(uS);
            out_len = n + nm * (rb - m);
            from_masks = true;
          }
          redo = false;  // (no row needs the automaton)
          units_done = true;
        }
      } else if (UNITS) {
        if (BITS && !has_odd && a.maxrepl < 0 && !__any(live && n > csbits::kMaxRowBytes)) {  // (wave-uniform) plain ASCII, rows within the masks
          using namespace cstd;
          p_second = cstile::status_load(a.excl + (p_tile >= 0 ? p_tile : 0));
          has_second = scanner;
          if (live) {
            auto cls = CS_BITS_CLS(bitmap, bm_bytes >> 2, lead + rbeg, n);
            auto raw = CS_BITS_RAW(bitmap, bm_bytes >> 2, lead + rbeg);
            csbits::match(BV, cls, raw, n, uS, uE);
            nm = u128_popc(uS);
            out_len = n - u128_popc(u128_sub(u128_shl1(uE), uS)) + nm * rb;
            from_masks = true;
          }
          redo = false;
          units_done = true;
        } else if (!BITS && !BREFS && lean && !has_odd && a.maxrepl < 0 && (D.chain >> 16) && !(CS_DBG(a) & 8192)) {  // (wave-uniform)
          // A chain pattern (regex_tdfa.h: chain_match) on a sub-tile of plain ASCII: every row lane derives its row's
          // matches from the row's candidate and x bits by integer arithmetic -- no unit queue, no table walk, no LDS
          // traffic beyond the two mask reads.
          using namespace cstd;
          uint32_t r0, r1, r2, x0 = 0, x1 = 0, x2 = 0;
          cstile::row_bits96(bitmap, lead + rbeg, n, r0, r1, r2);
          if (unit_x != 0) cstile::row_bits96(xbitmap, lead + rbeg, n, x0, x1, x2);
          p_second = cstile::status_load(a.excl + (p_tile >= 0 ? p_tile : 0));
          has_second = scanner;
          if (live) {
            chain_match96(r0, r1, r2, x0, x1, x2, D.chain, D.img, uS, uE, D.sfx, n, [&](int i) { return lds_in[lead + rbeg + i]; });
            nm = u128_popc(uS);
            out_len = n - u128_popc(u128_sub(u128_shl1(uE), uS)) + nm * rb;
            from_masks = true;
          }
          redo = false;
          units_done = true;
        } else if (BREFS && lean && !has_odd && a.maxrepl < 0 && (D.chain >> 16) && (((uint32_t)D.img[30] >> 20) & 1u) && !(CS_DBG(a) & 8192)) {  // (wave-uniform)
          // replace_with_backrefs on a chain pattern: the matches by chain_match, and every capture group is a run of
          // items, so its range follows from the item boundaries of the match -- a walk over the row's two masks per
          // match where the automaton needed an anchored group run (half the kernel's time).
          using namespace cstd;
          const uint32_t gmap = (uint32_t)D.img[D.img[15] - 1];
          uint32_t r0, r1, r2, x0 = 0, x1 = 0, x2 = 0;
          cstile::row_bits96(bitmap, lead + rbeg, n, r0, r1, r2);
          if (unit_x != 0) cstile::row_bits96(xbitmap, lead + rbeg, n, x0, x1, x2);
          const U128 R = u128(r0 | ((unsigned long long)r1 << 32), r2), X = u128(x0 | ((unsigned long long)x1 << 32), x2);
          p_second = cstile::status_load(a.excl + (p_tile >= 0 ? p_tile : 0));
          has_second = scanner;
          if (live) {
            chain_match96(r0, r1, r2, x0, x1, x2, D.chain, D.img, uS, uE, D.sfx, n, [&](int i) { return lds_in[lead + rbeg + i]; });
            nm = u128_popc(uS);
            from_masks = true;
          }
          const int cnt = from_masks ? nm : 0;
          const int mincl = csdev::wave_inclusive_scan(cnt);
          const int total_m = __builtin_amdgcn_readlane(mincl, 63);
          mslot = mincl - cnt;
          // (the chain form proper keeps going when the sub-tile holds more matches than the record table: the sizes now, the
          // group ranges once more at the assembly -- replace_with_backrefs((\d+), <\1>) on the C3 column, 5 numbers a row, gave
          // every launch up and took 174 ms on the two-pass form)
          dense_tile = CHAIN && total_m > kUnitQueue;
          if (!CHAIN && total_m > kUnitQueue) {
            if (lane == 0) atomicOr(a.error, 1u | 32u);
          } else {
            int grow_row = 0, mi = 0;
            U128 S = uS, E = uE;
            while (u128_any(S)) {
              const int mb = u128_ctz(S), me = u128_ctz(E) + 1;
              S = u128_clear_lowest(S);
              E = u128_clear_lowest(E);
              int gb[4] = {-1, -1, -1, -1}, ge[4] = {-1, -1, -1, -1};
              if (T.nrefs > 0) chain_group_bounds(R, X, D.chain, D.img, gmap, mb, gb, ge);  // (a template without references needs no groups)
              int grow = T.bytes - (me - mb);
              for (int j = 0; j < T.nrefs; ++j) {
                const int g = T.idx(j);
                int x = -1, y = -1;
                if (g == 0) {
                  x = mb;
                  y = me;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                  if (g == q + 1 && g <= T.groups) {
                    x = gb[q];
                    y = ge[q];
                  }
                if (x >= 0 && y > x) grow += y - x;
              }
              grow_row += grow;
              auto by = [&](int v) { return (uint32_t)(v >= 0 ? v : 255) & 255u; };
              if (!dense_tile) {
                uint32_t* rec = mrec + (mslot + mi) * 3;
                rec[0] = by(gb[0]) | (by(ge[0]) << 8) | (by(gb[1]) << 16) | (by(ge[1]) << 24);
                rec[1] = by(gb[2]) | (by(ge[2]) << 8) | (by(gb[3]) << 16) | (by(ge[3]) << 24);
                rec[2] = by(me) | (1u << 8);
              }
              ++mi;
            }
            if (from_masks) out_len = n + grow_row;
          }
          redo = false;
          units_done = true;
        } else if (!CHAIN && lean && a.maxrepl < 0 && (D.units & 1u) && !(CS_DBG(a) & 1024)) {  // (wave-uniform)
          using namespace cstd;
          // -- row lanes: the row's units from its candidate and x bits
          uint32_t m0, m1, m2;
          const int total_units = unit_discover(D, bitmap, xbitmap, lead + rbeg, n, lane, uqueue, m0, m1, m2, [&] {
            // every lane holds its masks: both bitmaps are re-used for the matches
            for (int i = lane * 16; i < bm_bytes; i += 64 * 16) {
              *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(bitmap) + i) = make_uint4(0, 0, 0, 0);
              *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(xbitmap) + i) = make_uint4(0, 0, 0, 0);
            }
            if (lane < 2) bailw[lane] = 0;
          });
          if (total_units >= 0) {
            CS_PHASE_MARK(7);
            // -- unit lanes: one unit each, whatever row it lies in
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
            CS_PHASE_MARK(8);
            // the previous tile's prefix: the poll issued before the scan came too early more often than not (the
            // scanner wave needs every earlier aggregate first); this one has the extraction below to arrive in
            // (into its own variable, unconditionally: see the note at the first poll)
            p_second = cstile::status_load(a.excl + (p_tile >= 0 ? p_tile : 0));
            has_second = scanner;
            // -- row lanes again: the row's matches from the start / last-byte bits
            uint32_t s0, s1, s2, e0, e1, e2;
            cstile::row_bits96(bitmap, lead + rbeg, n, s0, s1, s2);
            cstile::row_bits96(xbitmap, lead + rbeg, n, e0, e1, e2);
            const bool rbail = ((bailw[lane >> 5] >> (lane & 31)) & 1u) != 0;
            if (live && !rbail) {
              // the matches stay in the two masks until the rows are assembled (any number of them per row)
              uS = u128(s0 | ((unsigned long long)s1 << 32), s2);
              uE = u128(e0 | ((unsigned long long)e1 << 32), e2);
              nm = u128_popc(uS);
              out_len = n - u128_popc(u128_sub(u128_shl1(uE), uS)) + nm * rb;
              from_masks = true;
            }
            redo = live && rbail;  // (such a row is scanned whole; nothing of it was recorded above)
            if (BREFS) {
              if (__any(redo)) {  // (the template needs the unit route's masks: the host repeats with the two-pass form)
                if (lane == 0) atomicOr(a.error, 1u | 32u);
                redo = false;
              }
              {
                // the matches of the sub-tile go through the queue once more, one per lane whatever its row (as the units
                // did): ONE anchored group run per match sizes its expansion and leaves its group ranges in LDS
                const int cnt = from_masks ? nm : 0;
                const int mincl = csdev::wave_inclusive_scan(cnt);
                const int total_m = __builtin_amdgcn_readlane(mincl, 63);
                mslot = mincl - cnt;
                if (total_m > kUnitQueue) {
                  if (lane == 0) atomicOr(a.error, 1u | 32u);
                } else {
                  cstile::wave_lds_fence();  // (the unit lanes are done with the queue)
                  {
                    U128 S = uS, E = uE;
                    int at = mslot;
                    while (__any(u128_any(S))) {
                      if (u128_any(S)) {
                        const int mb = u128_ctz(S), me = u128_ctz(E) + 1;
                        S = u128_clear_lowest(S);
                        E = u128_clear_lowest(E);
                        uqueue[at++] = (uint32_t)lane | ((uint32_t)mb << 8) | ((uint32_t)me << 16);
                      }
                    }
                  }
                  rowgrow[lane] = 0;
                  cstile::wave_lds_fence();
                  for (int u0 = 0; u0 < total_m; u0 += 64) {
                    const bool act = u0 + lane < total_m;
                    const uint32_t ent = act ? uqueue[u0 + lane] : 0u;
                    const int r = (int)(ent & 63u), mb = (int)((ent >> 8) & 255u), me = (int)((ent >> 16) & 255u);
                    const int rbeg_r = __shfl(rbeg, r, 64), n_r = __shfl(n, r, 64);
                    if (act) {
                      const int pu = lead + rbeg_r;
                      cstd::Tdfa vg(D, P, lds_in + pu, n_r, pu & 3);
                      int gb[cstd::Tdfa::kGroupBatch], ge[cstd::Tdfa::kGroupBatch], mend = me;
                      // backwards from the match where that applies (regex_tdfa.h: group_find_back); the history bytes
                      // lie in the two bitmaps, whose bits every row lane has taken into its masks by now
                      const int hsteps = min(cstd::Tdfa::kBackSteps, (2 * bm_bytes) >> 6);
                      int got = T.nrefs > 0 ? vg.group_find_back(mb, gt, 1, T.groups, gb, ge, mend, cstd::Tdfa::HistBytes{reinterpret_cast<uint8_t*>(bitmap) + lane, 64}, hsteps) : 0;
                      if (got < 0) got = vg.group_find_all(mb, gt, 1, T.groups, gb, ge, mend);
                      const bool ok = got > 0;
                      int grow = T.bytes - (me - mb);
                      for (int j = 0; j < T.nrefs; ++j) {
                        const int g = T.idx(j);
                        int x = -1, y = -1;
                        if (g == 0) {
                          x = mb;
                          y = mend;
                        }
#pragma unroll
                        for (int q = 0; q < cstd::Tdfa::kGroupBatch; ++q)
                          if (g == q + 1 && g <= T.groups) {
                            x = gb[q];
                            y = ge[q];
                          }
                        if (ok && x >= 0 && y > x) grow += y - x;
                      }
                      __hip_atomic_fetch_add(rowgrow + r, (uint32_t)grow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                      auto by = [&](int v) { return (uint32_t)(ok && v >= 0 ? v : 255) & 255u; };
                      uint32_t* rec = mrec + (u0 + lane) * 3;
                      rec[0] = by(gb[0]) | (by(ge[0]) << 8) | (by(gb[1]) << 16) | (by(ge[1]) << 24);
                      rec[1] = by(gb[2]) | (by(ge[2]) << 8) | (by(gb[3]) << 16) | (by(ge[3]) << 24);
                      rec[2] = by(mend) | ((ok ? 1u : 0u) << 8);
                    }
                  }
                  cstile::wave_lds_fence();
                  if (from_masks) out_len = n + (int)rowgrow[lane];
                }
              }
            }
            units_done = true;
          }
        }
      }
      if (BREFS && !units_done) {  // (only the unit route carries the template: the host repeats with the two-pass form)
        if (lane == 0) atomicOr(a.error, 1u | 32u);
        redo = false;
      }
      if (hi_units && !units_done) redo = live;  // (more units than the queue holds: the generic scan, never the lean scan on such bytes)
      if (CHAIN && !BREFS && !units_done) redo = live && a.maxrepl != 0;  // (the generic scan)
      if (!CHAIN && UNITS && !BREFS && !units_done && lean && !hi_units && a.maxrepl < 0 && D.img[13] >= 1 && !(CS_DBG(a) & 2048)) {  // (wave-uniform)
        // A sub-tile the unit route did not take (more units than the queue holds: patterns whose candidate bytes are
        // everywhere, such as alternations of word-bounded literals; or no decomposition at all): every row lane scans its
        // own row, but the matches still go into the two bitmaps -- a start bit and a last-byte bit each, as the unit lanes
        // leave them -- so that the rows are assembled from the masks.  Before, such rows were only MEASURED here and
        // scanned a second time at assembly by the generic byte-at-a-time scanner: one matching row in a wave made the
        // other 63 lanes wait for that whole scan (52 ms on the 100M-row column for (\bin\b)|(\ba\b)|(\bthe\b), which
        // matches in 1.3 % of the rows).
        using namespace cstd;
        uint32_t m0, m1, m2;
        cstile::row_bits96(bitmap, lead + rbeg, n, m0, m1, m2);
        cstile::wave_lds_fence();
        for (int i = lane * 16; i < bm_bytes; i += 64 * 16) {
          *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(bitmap) + i) = make_uint4(0, 0, 0, 0);
          *reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(xbitmap) + i) = make_uint4(0, 0, 0, 0);
        }
        cstile::wave_lds_fence();
        bool bail = false;
        if (live) {
          const int pu = lead + rbeg;
          auto recm = [&](int mb, int me, int) {
            const int ps = pu + mb, pe = pu + me - 1;
            __hip_atomic_fetch_or(bitmap + (ps >> 5), 1u << (ps & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            __hip_atomic_fetch_or(xbitmap + (pe >> 5), 1u << (pe & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
          };
          vm.scan_lean_dispatch(-1, m0, m1, m2, recm, bail);
        }
        cstile::wave_lds_fence();
        uint32_t s0, s1, s2, e0, e1, e2;
        cstile::row_bits96(bitmap, lead + rbeg, n, s0, s1, s2);
        cstile::row_bits96(xbitmap, lead + rbeg, n, e0, e1, e2);
        if (live && !bail) {
          uS = u128(s0 | ((unsigned long long)s1 << 32), s2);
          uE = u128(e0 | ((unsigned long long)e1 << 32), e2);
          nm = u128_popc(uS);
          out_len = n - u128_popc(u128_sub(u128_shl1(uE), uS)) + nm * rb;
          from_masks = true;
        }
        redo = live && bail;  // (such a row is scanned whole by the generic scan below; nothing of it counts from above)
        units_done = true;
      }
      if (!CHAIN && !BREFS && !units_done && lean && !hi_units && live && a.maxrepl != 0) {
        bool bail = false;
        uint32_t m0, m1, m2;  // candidate bits, bit i = byte i of the row
        if (LONG) {
          const int p0 = lead + rbeg;
          cstile::row_bits96(bitmap, p0, min(n, 96), m0, m1, m2);
          auto refill = [&](int wb, uint32_t& x0, uint32_t& x1, uint32_t& x2) {
            cstile::row_bits96(bitmap, p0 + wb, min(n - wb, 96), x0, x1, x2);
          };
          vm.scan_lean_dispatch_long(a.maxrepl, m0, m1, m2, rec, bail, refill);
        } else {
          cstile::row_bits96(bitmap, lead + rbeg, n, m0, m1, m2);
          vm.scan_lean_dispatch(a.maxrepl, m0, m1, m2, rec, bail);
        }
        redo = bail;
        resume = vm.lean_resume_from;
      }
      if (!(BREFS && CHAIN) && __builtin_expect(__any(redo), 0)) {
        // rows the lean scan handed over continue with the generic scan in the round they stopped in
        // (the matches reported so far are final)
        if (redo) {
          if (WIDE) vm.template scan<cstd::Tdfa::K_REPLACE, decltype(rec)&, cstd::kMaxSlotsWide>(a.maxrepl, rec, resume, nm);
          else vm.template scan<cstd::Tdfa::K_REPLACE>(a.maxrepl, rec, resume, nm);
        }
      }
      if (INPLACE && live) {
        if (pend >= 0) put_repl_at(pend);
        if (nm > 0) {
          if (wr != copied) cstile::lds_copy(lds_in, pi + wr, lds_in, pi + copied, n - copied);
          out_len = wr + (n - copied);
        }
      }
    }
    CS_PHASE_MARK(1);
    if (kHoles && hole) out_len = hole_bytes;
    const int incl = csdev::wave_inclusive_scan(out_len);
    const int lo = incl - out_len;
    const int total = __builtin_amdgcn_readlane(incl, 63);
    m_span = max(m_span, total);
    // (error bit 1: a roomier launch, which also takes rows with many matches, can succeed)
    bool grew = false;
    if (!INPLACE) grew = !bad && (total + 32 > a.cap_out || (!RESCAN && __any(nm > kMaxRec)));
    bad |= total + 32 > a.cap_out;
    if (!INPLACE) bad |= grew;
    if (oversize) {
      cstile::lookback_publish(a.status, tile, total, lane);
      if (p_tile >= 0) finish_pending(p_first);
      p_tile = -1;
      // this sub-tile is finished at once: its prefix, the offsets, every row written by its lane
      long long gb = __builtin_expect(scanner, 1) ? cstile::prefix_wait(a.excl, tile, cstile::status_load(a.excl + tile), a.error, lane)
                             : cstile::lookback_end(a.status, tile, total, cstile::lookback_poll(a.status, tile, lane), lane);
      if (gb < 0) {
        if (lane == 0) atomicOr(a.error, 1u | 8u);
        gb = 0;
      }
      if (lane < nrows) a.out_off[r0 + lane] = gb + lo;
      if (lane == nrows - 1 && r0 + nrows == in.rows) a.out_off[in.rows] = gb + lo + out_len;
      if (gb + total > a.out_cap) {
        if (lane == 0) atomicOr(a.error, 2u);
        return;
      }
      if (live) {
        const uint8_t* p = in.chars + (g0 + rbeg);
        uint8_t* o = a.out_chars + gb + lo;
        int copied = 0;
        auto piece = [&](int mb, int me, int reps) {
          for (int i = copied; i < mb; ++i) *o++ = p[i];
          for (int k = 0; k < reps; ++k)
            for (int i = 0; i < rb; ++i) *o++ = a.repl[i];
          copied = me;
        };
        cstd::Tdfa vg(D, P, p, n);
        if (WIDE) vg.template scan<cstd::Tdfa::K_REPLACE, decltype(piece)&, cstd::kMaxSlotsWide>(a.maxrepl, piece, 0, 0);
        else vg.template scan<cstd::Tdfa::K_REPLACE>(a.maxrepl, piece, 0, 0);
        for (int i = copied; i < n; ++i) *o++ = p[i];
      }
    } else if (__builtin_expect(bad, 0)) {
      // the host discards this launch's output; publish something so successors do not spin
      if (lane == 0) {
        atomicOr(a.error, !INPLACE && grew ? 2u : (1u | 4u));  // (4: a sub-tile beyond the staging capacity)
        cstile::status_store(a.status + tile, cstile::kFlagInc);
      }
      if (p_tile >= 0) finish_pending(p_first);
      p_tile = -1;
    } else {
      if (!(CS_DBG(a) & 8)) cstile::lookback_publish(a.status, tile, total, lane);
      if (lane == 0) CS_TILE_TRACE(tile, 0);
      CS_PHASE_MARK(2);
      if (p_tile >= 0)
        finish_pending((CS_DBG(a) & 64) ? (__builtin_expect(scanner, 1) ? cstile::status_load(a.excl + p_tile) : cstile::lookback_poll(a.status, p_tile, lane))
                                      : (has_second && (p_first >> 62) == 0 ? p_second : p_first));
      CS_PHASE_MARK(3);
      if (INPLACE) {
        if (live && !(CS_DBG(a) & 2)) cstile::lds_copy_ov(lds_out, lo, lds_in, lead + rbeg, out_len);
      } else if (live && !(CS_DBG(a) & 2)) {
        int oi = lo;                 // byte index into lds_out
        const int pi = lead + rbeg;  // byte index of the row in lds_in
        int copied = 0;
        if (BREFS && from_masks) {
          int mi = 0;
          while (cstd::u128_any(uS)) {
            const int mb = cstd::u128_ctz(uS), me = cstd::u128_ctz(uE) + 1;
            uS = cstd::u128_clear_lowest(uS);
            uE = cstd::u128_clear_lowest(uE);
            cstile::lds_copy_ov(lds_out, oi, lds_in, pi + copied, mb - copied);
            oi += mb - copied;
            int gb[cstd::Tdfa::kGroupBatch], ge[cstd::Tdfa::kGroupBatch], mend = me;
            bool ok;
            if (CHAIN && dense_tile) {  // (wave-uniform) no record of this match: its groups off the row's masks again
              uint32_t r0, r1, r2, x0 = 0, x1 = 0, x2 = 0;
              cstile::row_bits96(bitmap, pi, n, r0, r1, r2);
              if (unit_x != 0) cstile::row_bits96(xbitmap, pi, n, x0, x1, x2);
              int g4b[4], g4e[4];
              cstd::chain_group_bounds(cstd::u128(r0 | ((unsigned long long)r1 << 32), r2), cstd::u128(x0 | ((unsigned long long)x1 << 32), x2), D.chain, D.img,
                                       (uint32_t)D.img[D.img[15] - 1], mb, g4b, g4e);
#pragma unroll
              for (int q = 0; q < cstd::Tdfa::kGroupBatch; ++q) gb[q] = q < 4 ? g4b[q] : -1, ge[q] = q < 4 ? g4e[q] : -1;
              ok = true;
            } else {
              const uint32_t* rec = mrec + (mslot + mi) * 3;
              const uint32_t lo4 = rec[0], hi4 = rec[1], e4 = rec[2];
              auto un = [](uint32_t v) { return v == 255u ? -1 : (int)v; };
              gb[0] = un(lo4 & 255u), ge[0] = un((lo4 >> 8) & 255u), gb[1] = un((lo4 >> 16) & 255u), ge[1] = un(lo4 >> 24);
              gb[2] = un(hi4 & 255u), ge[2] = un((hi4 >> 8) & 255u), gb[3] = un((hi4 >> 16) & 255u), ge[3] = un(hi4 >> 24);
              mend = (int)(e4 & 255u);
              ok = ((e4 >> 8) & 1u) != 0;
            }
            int il = 0;
            for (int j = 0; j < T.nrefs; ++j) {
              cstile::lds_copy_ov(lds_out, oi, ttext, il, T.pos(j) - il);
              oi += T.pos(j) - il;
              il = T.pos(j);
              const int g = T.idx(j);
              int x = -1, y = -1;
              if (g == 0) {
                x = mb;
                y = mend;
              }
#pragma unroll
              for (int q = 0; q < cstd::Tdfa::kGroupBatch; ++q)
                if (g == q + 1 && g <= T.groups) {
                  x = gb[q];
                  y = ge[q];
                }
              if (ok && x >= 0 && y > x) {
                cstile::lds_copy_ov(lds_out, oi, lds_in, pi + x, y - x);
                oi += y - x;
              }
            }
            cstile::lds_copy_ov(lds_out, oi, ttext, il, T.bytes - il);
            oi += T.bytes - il;
            copied = me;
            ++mi;
          }
        } else if (UNITS && from_masks) {
          while (cstd::u128_any(uS)) {
            const int mb = cstd::u128_ctz(uS), me = cstd::u128_ctz(uE) + 1;
            uS = cstd::u128_clear_lowest(uS);
            uE = cstd::u128_clear_lowest(uE);
            cstile::lds_copy_ov(lds_out, oi, lds_in, pi + copied, mb - copied);
            oi += mb - copied;
            if (REP16) {
              if (rb > 16) {
                for (int i = 0; i < rb; ++i) lds_out[oi + i] = a.repl[i];
              } else {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                  if (i < rb) lds_out[oi + i] = (uint8_t)(rep[i >> 2] >> (8 * (i & 3)));
              }
              oi += rb;
            } else {
              for (int i = 0; i < rb; ++i) lds_out[oi++] = (uint8_t)((i < 4 ? rep[0] >> (8 * i) : rep[1] >> (8 * (i - 4))));
            }
            copied = me;
          }
        } else if (!UNITS && (!RESCAN || nm <= kMaxRec)) {
#pragma unroll
          for (int j = 0; j < kMaxRec; ++j)
            if (j < nm) {
              cstile::lds_copy_ov(lds_out, oi, lds_in, pi + copied, rec_mb[j] - copied);
              oi += rec_mb[j] - copied;
              for (int k = 0; k < rec_reps[j]; ++k) {
                if (REP16) {
                  if (rb > 16) {
                    for (int i = 0; i < rb; ++i) lds_out[oi + i] = a.repl[i];
                  } else {
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                      if (i < rb) lds_out[oi + i] = (uint8_t)(rep[i >> 2] >> (8 * (i & 3)));
                  }
                  oi += rb;
                } else {
                  for (int i = 0; i < rb; ++i) lds_out[oi++] = (uint8_t)((i < 4 ? rep[0] >> (8 * i) : rep[1] >> (8 * (i - 4))));
                }
              }
              copied = rec_me[j];
            }
        } else if (!(BREFS && CHAIN) && __builtin_expect(nm > 0, 0)) {
          // more matches than the registers keep (UNITS: any row measured by the generic scan): the row's size is
          // known from the first scan, so scan it again and assemble as the matches are reported
          auto piece2 = [&](int mb, int me, int reps) {
            cstile::lds_copy_ov(lds_out, oi, lds_in, pi + copied, mb - copied);
            oi += mb - copied;
            for (int k = 0; k < reps; ++k)
              for (int i = 0; i < rb; ++i) lds_out[oi++] = a.repl[i];
            copied = me;
          };
          cstd::Tdfa vm2(D, P, lds_in + pi, n, pi & 3);
          if (WIDE) vm2.template scan<cstd::Tdfa::K_REPLACE, decltype(piece2)&, cstd::kMaxSlotsWide>(a.maxrepl, piece2, 0, 0);
          else vm2.template scan<cstd::Tdfa::K_REPLACE>(a.maxrepl, piece2, 0, 0);
        }
        cstile::lds_copy_ov(lds_out, oi, lds_in, pi + copied, n - copied);
      }
      cstile::wave_lds_fence();
      CS_PHASE_MARK(4);
      p_tile = tile;
      p_total = total;
      p_lo = lo;
      p_len = out_len;
    }
    if (!has_next) break;
    tile = t_nxt;
    t_nxt = t_nn;
    nxt = nn;
    pending = pending_new;
    c_hm = n_hm;
    c_hf = n_hf;
  }
  if (p_tile >= 0) finish_pending((CS_DBG(a) & 8) ? 0 : (__builtin_expect(scanner, 1) ? cstile::status_load(a.excl + p_tile) : cstile::lookback_poll(a.status, p_tile, lane)));
  {
    // (only a wave that would raise the maximum issues the same-address atomic; slot 14 behind the error word)
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(a.error) + 14;
    if (lane == 0 && (unsigned long long)m_span > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, (unsigned long long)m_span);
  }
#if defined(CS_PHASE_PROF)
  CS_PHASE_MARK(5);
  if (lane == 0)
    for (int k = 0; k < 12; ++k) atomicAdd(reinterpret_cast<unsigned long long*>(a.error) + 1 + k, phase_acc[k]);
  if (lane == 0)
    for (int k = 0; k < 3; ++k) atomicAdd(&cstile::g_lb_stats[k], lb_acc[k]);
#endif
}


// matches per tile of R rows out of count_re's per-row counts: the column's total and the busiest tile's (replace_re with a
// growing replacement sizes its out tile and its output from them instead of provisioning for the worst case)
__global__ void __launch_bounds__(256) k_match_stats(const int32_t* __restrict__ counts, int64_t rows, int R, unsigned long long* __restrict__ total, unsigned* __restrict__ tilemax) {
  const int lane = threadIdx.x & 63;
  const int64_t ntiles = (rows + R - 1) / R;
  unsigned long long sum = 0;
  unsigned most = 0;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < ntiles; t += (int64_t)gridDim.x * 4) {
    const int64_t r = t * R + lane;
    const int c = lane < R && r < rows ? max(counts[r], 0) : 0;
    const int ts = wave_reduce_sum(c);
    sum += (unsigned)ts;
    most = max(most, (unsigned)ts);
  }
  if (lane == 0) {
    if (sum) atomicAdd(total, sum);
    if (most > __hip_atomic_load(tilemax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(tilemax, most);
  }
}

}  // namespace

// ---- replace_re: the host route ---------------------------------------------------------------------------------------
// cs::replace_re_column runs a cs::ReplaceCall (cs_internal.h) as the sequence it is -- the column's pieces, class runs,
// the single pass, the two-pass kernels -- each step a function that returns the column, or nullptr when it declines.
// The single pass in turn: its SHAPE (what is fixed for the call), its FORM (which variant of k_tdfa_replace_stream runs),
// per attempt its SIZING (out tile, output buffer, LDS layout -- the second, roomier attempt differs only there), the
// KERNEL (replace_stream_kernel: the one place that names the instantiations) and the LAUNCH.
// Several questions below launch kernels or wait on the stream the first time they are asked of a column
// (sample_has_high_bytes, odd_rows_few, odd_rows, candidate_share, bits_route, max_span64, few_spans64_over, choose_tile):
// the order of the `&&` chains decides whether they are asked at all.  Keep it.
namespace {

struct ReplaceRun {  // a call and what its steps share
  const cs::ReplaceCall& c;
  cs_regex* re;
  bool tdfa, wide;  // the tagged DFA runs the program; ... with five to eight live threads (the two-pass kernels on TdfaWide)
  TPlan tp;         // (tdfa || wide)
  Plan pl;          // (neither: the list simulator)
  Buf d_repl;       // the replacement text on the device
  RowSrc src;
};

// rows beyond the 96-bit masks, white space a safe cut for this program: the pieces' replace_re is the rows' (cs_virtual.hip)
cs_column* replace_on_pieces(const ReplaceRun& r) {
  const cs::ReplaceCall& c = r.c;
  if (c.tmpl_dev || c.single_pass_only || c.maxrepl >= 0 || !r.tdfa || cs::cfg("CS_CLASS_RUNS_ALWAYS")) return nullptr;
  const VirtualRows* vr = pieces_for(c.col, r.re, c.s, true);
  if (!vr) return nullptr;
  cs::ReplaceCall pieces = c;
  pieces.col = vr->col.get();
  std::unique_ptr<cs_column> po(cs::replace_re_column(pieces));
  note_route_pieces();
  return virtual_rows_to_rows(c.col, vr, std::move(po), c.s);
}

// One character class, once or in a `+` loop, on a column the 96-bit-mask forms do not take -- rows beyond 93 bytes,
// tiles of fewer than 64 rows, non-ASCII text -- and whose candidates are everywhere: byte-parallel stream compaction
// (cs_runs.hip; BASELINE.json C5: replace_re([aeiou]+) on 40-150-byte rows, 82.8 ms on the long-row automaton forms).
cs_column* replace_by_class_runs(const ReplaceRun& r) {
  const cs::ReplaceCall& c = r.c;
  const cs_column* col = c.col;
  const cs_regex* re = r.re;
  if (c.tmpl_dev || c.single_pass_only || c.maxrepl >= 0 || col->rows <= 0 || re->bits.empty() || !(re->bits[2] & (csbits::F_BYTE_CLASS | csbits::F_FLAG_CLASS)) || !re->d_bits)
    return nullptr;
  const TileChoice tc0 = choose_tile(col, c.s, true);
  const bool masks_form = tc0.R == 64 && !tc0.lng && (!sample_has_high_bytes(col, c.s) || odd_rows_few(col, c.s));  // (few rows with such bytes: holes)
  // (a class with builtins -- `\w+` -- sends every tile with a byte >= 0x80 row by row: worth it against the automaton's
  // long-row and dense forms -- `\w+` on the C5 column 97.7 -> 11.2 ms, on C2 16.2 -> 5.1 --, not against the chain
  // arithmetic where that runs: `\s+` on C2 4.4 there, 6.7 here)
  const bool chain_there = !re->tdfa.empty() && ((re->tdfa[30] >> 16) & 15) != 0 && tc0.R == 64 && !tc0.lng;
  const bool flag_class = (re->bits[2] & csbits::F_BYTE_CLASS) == 0;
  const bool wanted = cs::cfg("CS_CLASS_RUNS_ALWAYS") || (!masks_form && !(flag_class && chain_there) && candidate_share(re, col, c.s) >= 0.05);
  cs_column* out = nullptr;
  if (!wanted || !replace_class_runs(col, ptr<const int32_t>(re->d_bits), re->bits, c.repl, c.rb, c.s, &out)) return nullptr;
  note_route("runs");
  return out;
}

// What is fixed for a call's single pass, whichever form runs and however many attempts it takes.
struct ReplaceShape {
  // A match is at least `minlen` bytes, so a row grows by at most `growth` = rb - minlen bytes per match; no growth means
  // "never grows" and the rows are rewritten in place.  A growing replacement is provisioned for kMaxRec matches per row
  // first (or, `roomy_first`, for up to the worst case: patterns of one or two bytes tend to match often); a launch that
  // runs out of room says so in its error word and is repeated once with the roomier sizing.
  int minlen, minlen_p, growth;
  // (a pattern that matches the empty string inserts at most one replacement per character and one at the row's end:
  // short replacements are provisioned for exactly that -- `x*` -> '-' doubles the column -- and stay on the single pass;
  // with a longer one the pattern is unbounded -- the zero-length repeat rule -- and takes the two-pass kernels)
  bool empties;
  // (programs of five to eight threads: the stream kernel's WIDE forms -- tables in LDS, replacements of up to 16 bytes)
  bool wide_stream;
  TileChoice tc;
  // (the column's largest 64-row span does not fit, all but a few do: buffers for those, the kernel handles the rest)
  bool outliers;
  int cap;  // bytes of the in tile
  // a column whose sample holds a few bytes >= 0x80: the unit forms run as on plain ASCII, the rows that hold such bytes are
  // sized beforehand and written afterwards, a thread a row (StreamArgs::hole_mask) -- replace_re of the gtest pattern on the C5
  // column's pieces: 34 ms when a third of the sub-tiles went to the row-by-row scan for the sake of one row each
  bool holes_ok;
  bool roomy_first;
  int64_t sized_total = -1, sized_tilemax = 0;  // matches in the column / in its busiest tile, when they were counted first
};

// A growing replacement for a pattern of one or two bytes (`\d+` -> '<number>', `\d` -> '##'): provisioned for the worst
// case the out tile is three times the in tile -- two workgroups a CU -- and the output twice the column (18 ms on the
// C3 column where `\d+` -> '#' takes 5.9).  count_re first (2.4 ms) says how many matches the column and its busiest
// tile hold: the out tile and the output are sized exactly: 17.9 -> 12.1 ms.
// (where the worst case is within three times the in tile anyway -- `\d` -> '##' -- the count only costs: 15.6 -> 17.9 ms)
void count_matches_first(const ReplaceRun& r, ReplaceShape* sh) {
  const cs_column* col = r.c.col;
  const hipStream_t s = r.c.s;
  Buf counts = dev_alloc(sizeof(int32_t) * (size_t)col->rows, s), stats = dev_alloc(16, s);
  scan<2>(ScanCall{col, r.re, counts->p, sizeof(int32_t), 1, s, nullptr, "k_count_re"});
  CS_HIP(hipMemsetAsync(stats->p, 0, 16, s));
  hipLaunchKernelGGL(k_match_stats, dim3(1024), dim3(256), 0, s, ptr<const int32_t>(counts), col->rows, sh->tc.R, ptr<unsigned long long>(stats),
                     reinterpret_cast<unsigned*>(ptr<unsigned long long>(stats) + 1));
  CS_HIP(hipGetLastError());
  unsigned long long* h = (unsigned long long*)pinned_scratch(16);
  CS_HIP(hipMemcpyAsync(h, stats->p, 16, hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  sh->sized_total = (int64_t)h[0];
  sh->sized_tilemax = (int64_t)(unsigned)h[1];
  note_route("");
}

// The shape of the call; false: no single pass for it.
bool replace_shape(const ReplaceRun& r, ReplaceShape* shape) {
  const cs::ReplaceCall& c = r.c;
  const cs_column* col = c.col;
  const cs_regex* re = r.re;
  const hipStream_t s = c.s;
  const int rb = c.rb;
  ReplaceShape& sh = *shape;
  const int minlen = sh.minlen = (r.tdfa || r.wide) ? re->tdfa[13] : 0;
  sh.minlen_p = std::max(minlen, 1);
  sh.growth = rb > minlen ? rb - minlen : 0;
  sh.empties = minlen == 0 && sh.growth > 0;
  const bool bounded = sh.growth == 0 || minlen >= 1 || rb <= 8;  // (longer ones: the out tile of 1 + rb times the input does not fit the LDS)
  sh.wide_stream = r.wide && r.tp.d.in_lds && rb <= 16 && !c.tmpl_dev && !cs::cfg("CS_WIDE_TWO_PASS");
  if (!(r.tdfa || sh.wide_stream) || !bounded || cs::cfg("CS_REGEX_TWO_PASS")) return false;
  sh.tc = choose_tile(col, s, !cs::cfg("CS_NO_SMALL_TILES"));
  constexpr int64_t kOutlierSpan = cstile::kPfBytes - 176;  // (its capacity is kPfBytes)
  sh.outliers = !sh.tc.R && r.tdfa && r.tp.d.in_lds && rb <= 16 && !c.tmpl_dev && !cs::cfg("CS_NO_OUTLIER_TILES") && max_span64(col, s) <= (16 << 20) &&
                few_spans64_over(col, kOutlierSpan, s);
  if (sh.outliers) sh.tc = TileChoice{64, (int)((kOutlierSpan + 15 + 32 + 127) & ~(int64_t)127), false, kOutlierSpan};
  const TileChoice& tc = sh.tc;
  const int cap = sh.cap = tc.cap;
  sh.holes_ok = r.tdfa && r.tp.d.in_lds && c.maxrepl < 0 && !c.tmpl_dev && !c.single_pass_only && !sh.wide_stream && !sh.outliers && tc.R == 64 && !tc.lng &&
                sample_has_high_bytes(col, s) && odd_rows_few(col, s);
  // (replacements of 17 .. kMaxStreamRepl bytes ride the four-register variants, their text read from memory at assembly)
  // (... where a match is long enough for the row not to outgrow the out tile: a 19-byte replacement of one-digit matches
  // goes to the two-pass kernels at once instead of failing the single pass twice first)
  // (... or where the sample says matches are few: at most about three candidate bytes a row -- the first attempt is
  // provisioned for kMaxRec matches a row; `-` -> 35 bytes on the log lines, two or three dashes each: 58 ms on the two-pass
  // kernels.  A column that has more after all loses one launch before them)
  const bool few_matches = rb <= kMaxStreamRepl && minlen >= 1 && col->rows > 0 &&
                           candidate_share(re, col, s) * ((double)col->nbytes / (double)col->rows) <= (double)(kMaxRec - 1);
  const size_t lds = (r.tp.d.in_lds ? r.tp.lds_bytes : 0) + (size_t)(cap + cap + 64 + (cap >> 3) + 32) * 4 + 16;
  if (lds > 150 * 1024 || !(rb <= 16 || (rb <= kMaxStreamRepl && rb <= 4 * minlen) || few_matches) || !tc.R) return false;
  sh.roomy_first = sh.growth > 0 && (minlen <= 2 || sh.wide_stream || sh.outliers || cs::cfg("CS_REPLACE_ROOMY"));
  if (sh.roomy_first && rb >= 3 * sh.minlen_p && r.tdfa && !sh.wide_stream && !sh.outliers && !c.tmpl_dev && !c.single_pass_only && c.maxrepl < 0 && !sh.empties && r.tp.d.in_lds &&
      !cs::cfg("CS_NO_COUNT_SIZING"))
    count_matches_first(r, shape);
  return true;
}

// replace_with_backrefs on a chain whose groups are runs of items: an expansion is the template's literal bytes plus the
// groups it names, so a match grows by at most
//   G = literal bytes + sum over items of (times the item is named - 1) * its length
// -- with every item named at most once, G = literal bytes - the least length of the items NOT named, often <= 0
// (`\4.\3.\2.\1` on four dotted groups: 3 - 3).  An item named twice and unbounded: -1, unknown.
int64_t brefs_chain_growth(const cs_regex* re, const csvm::BackrefTemplate* ht) {
  const cstd::View hv = cstd::make_view(re->tdfa.data());
  const int ni = (int)((hv.chain >> 16) & 15u);
  const unsigned long long hcrep = cstd::chain_crep(re->tdfa.data());
  const uint32_t gmap = (uint32_t)re->tdfa[re->tdfa[15] - 1];
  int named[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < ht->nrefs; ++j) {
    const int g = ht->idx[j];
    int lo = 0, hi = 0;
    if (g == 0) hi = ni;
    else if (g <= 4 && g <= ht->groups) lo = (int)((gmap >> (8 * (g - 1))) & 15u), hi = (int)((gmap >> (8 * (g - 1) + 4)) & 15u);
    for (int k = lo; k < hi && k < 8; ++k) ++named[k];
  }
  int64_t G = ht->bytes;
  for (int k = 0; k < ni && k < 8; ++k) {
    const int least = (int)(cstd::chain_rep(hcrep, k) & 15u), most = (int)(cstd::chain_rep(hcrep, k) >> 4);
    if (named[k] == 0) G -= least;
    else if (named[k] > 1) {
      if (most == 0) return -1;
      G += (int64_t)(named[k] - 1) * most;
    }
  }
  return std::max<int64_t>(G, 0);
}

// Which variant of the stream kernel runs (the template parameters' meaning: at k_tdfa_replace_stream).
struct ReplaceForm {
  bool brefs;    // replace_with_backrefs: the unit scan, groups carried by the DFA (four at most), tables in LDS
  bool literal;  // cs_replace's needle by byte comparison
  bool bits_form;  // the bit-parallel form (regex_bits.h): patterns whose candidates are everywhere -- a bitmap per character class
  // replace_with_backrefs on a chain whose groups are runs of items, the sample plain ASCII: the form that keeps neither
  // tables nor group tags in LDS (<.., BREFS, .., CHAIN>); its out tile is sized from the template (brefs_chain_growth)
  bool bchain;
  int64_t brefs_grow;  // per match; -1: unknown (the old "twice the input")
  // the unit scan (<.., UNITS>): patterns whose tagged DFA offers the decomposition, no limit on the number of
  // replacements, rows within the 96-byte masks
  bool units;
  bool chain_form;     // (a chain pattern on a column whose sample is plain ASCII: the form without the unit / lean scans)
  bool chain_pattern;  // (the route note: "chain" or "units")
  bool lng;            // rows beyond the 96-byte candidate masks (and up to 255 bytes) take the sliding-window form
  bool inplace;        // no growth; otherwise the register-record assembly, with the rescan on the roomy attempt and in every unit form
  bool rep16;          // rb > 8
};

// The form of the call; false: the template has no form here (the caller's two-pass form runs).
bool replace_form(const ReplaceRun& r, const ReplaceShape& sh, ReplaceForm* form) {
  const cs::ReplaceCall& c = r.c;
  const cs_column* col = c.col;
  const cs_regex* re = r.re;
  const hipStream_t s = c.s;
  const TileChoice& tc = sh.tc;
  const bool in_lds = r.tp.d.in_lds, all = c.maxrepl < 0, outliers = sh.outliers, wide_stream = sh.wide_stream;
  const bool offers_units = (re->tdfa[31] & 1) != 0, chain = ((re->tdfa[30] >> 16) & 15) != 0, group_chain = chain && ((re->tdfa[30] >> 20) & 1) != 0;
  ReplaceForm& f = *form;
  f.brefs = c.tmpl_dev != nullptr;
  // (a chain without a unit decomposition has no route for sub-tiles with bytes >= 0x80 in this form: only on columns whose sample is plain ASCII)
  if (f.brefs && !((offers_units || (group_chain && !sample_has_high_bytes(col, s))) && !tc.lng && tc.R == 64 && in_lds && !re->gtags.empty() && re->prog.num_groups <= cstd::Tdfa::kGroupBatch &&
                   re->gtags.size() * 4 <= 8 * 1024))
    return false;
  // (not the unit scan for the literal needles of cs_replace: short needles match densely, and then the per-row kernel with
  // its in-place compaction is the faster one -- 'ab' -> 'x' on the C2 column: 1.25 against 1.77 ms)
  f.literal = !f.brefs && !outliers && c.single_pass_only && c.literal_len > 0 && all && !tc.lng && tc.R == 64 && !cs::cfg("CS_NO_LITERAL_SCAN");
  // (the bit form builds on the unit forms' layout and assembly, whether or not the pattern offers a unit decomposition)
  f.bits_form = !f.literal && !f.brefs && !wide_stream && r.tdfa && all && !tc.lng && tc.R == 64 && !outliers && !c.single_pass_only && in_lds &&
                bits_route(re, col, s, BITS_REPLACE, sh.holes_ok);
  f.bchain = f.brefs && group_chain && !tc.lng && tc.R == 64 && all && c.tmpl_host && !cs::cfg("CS_NO_BREFS_CHAIN") && !sample_has_high_bytes(col, s);
  f.brefs_grow = f.bchain ? brefs_chain_growth(re, static_cast<const csvm::BackrefTemplate*>(c.tmpl_host)) : -1;
  // (units, or a chain pattern without them: one with a suffix)
  f.units = f.literal || f.brefs || f.bits_form || ((offers_units || chain) && all && !tc.lng && tc.R == 64 && !outliers && !c.single_pass_only && !cs::cfg("CS_NO_UNITS"));
  f.chain_form = !f.bits_form && !f.brefs && !wide_stream && !outliers && f.units && sh.cap <= 5 * 1024 && in_lds && !f.literal && all && chain &&
                 (!sample_has_high_bytes(col, s) || sh.holes_ok) && !cs::cfg("CS_NO_CHAIN_FORM");
  f.chain_pattern = chain;
  f.lng = tc.lng;
  f.inplace = sh.growth == 0;
  f.rep16 = c.rb > 8;
  return true;
}

// An attempt's sizes: the out tile and the output buffer, then the LDS layout (k_tdfa_replace_stream's).
struct StreamSizing {
  int cap_out;    // bytes of the out tile
  int64_t extra;  // bytes of output beyond the input's
  size_t gt_bytes, bits_lds, tbl_lds, lds1;  // group tags + template text, the bit form, the tables (or their header), all of it
  bool chain_global;                         // the tables stay in memory
};

// The out tile and the output of an attempt: `cap_out` and `extra`.
void size_stream_output(const ReplaceRun& r, const ReplaceShape& sh, const ReplaceForm& f, bool roomy, StreamSizing* z) {
  const cs_column* col = r.c.col;
  const int rb = r.c.rb, cap = sh.cap, growth = sh.growth, minlen_p = sh.minlen_p;
  const int64_t span_room = std::min<int64_t>(cap, (sh.tc.span + 15 + 32 + 15) & ~(int64_t)15);
  const int64_t few = (int64_t)col->rows * kMaxRec * growth;  // extra bytes if no row has more than kMaxRec matches
  int cap_out = cap + ((64 * kMaxRec * growth + 127) & ~127);
  // (no growth: the out tile holds at most the in tile's span -- rounded up to 16, not to the in tile's 128: a form of
  // 54 496 bytes of LDS ran two workgroups per CU where 54 240 run three)
  if (growth == 0 && !sh.outliers) cap_out = (int)span_room;
  int64_t extra = std::min<int64_t>(few, col->nbytes + (1ll << 30));
  if (roomy && sh.sized_total >= 0) {
    // (the matches were counted first: the busiest tile's growth and the column's, exactly)
    cap_out = (int)((span_room + sh.sized_tilemax * growth + 127) & ~(int64_t)127);
    extra = sh.sized_total * growth + 64;
  } else if (roomy) {
    const int64_t worst = ((int64_t)cap * rb + minlen_p - 1) / minlen_p;
    cap_out = std::max(cap_out, (int)((std::min<int64_t>(worst, 3ll * cap) + 127) & ~(int64_t)127));
    const int64_t worst_extra = (col->nbytes * growth + minlen_p - 1) / minlen_p;
    extra = std::min(worst_extra, std::max<int64_t>(extra, col->nbytes));
    if (sh.empties) {  // every character and every row end may take a replacement
      cap_out = (int)(((int64_t)cap * (1 + rb) + 64 * rb + 127) & ~(int64_t)127);
      extra = col->nbytes * rb + col->rows * rb;
    }
  }
  if (f.brefs && f.brefs_grow >= 0) {
    // (at most span / minlen matches in a sub-tile, each growing by at most brefs_grow bytes -- the roomy sizing; the first
    // attempt provisions a quarter of the input instead when that is less: `(\d+)` -> `<\1>` may triple a row of digits
    // and spaces, and adds a sixth to a log line -- at the worst case's 84 KB of LDS one workgroup fits a CU, 48.8 ms on the
    // C3 column; a launch that runs out of room says so and the roomy one follows)
    int64_t tile_grow = (sh.tc.span / minlen_p + 1) * f.brefs_grow, col_grow = (col->nbytes / minlen_p + 1) * f.brefs_grow;
    if (!roomy) {
      tile_grow = std::min<int64_t>(tile_grow, std::max<int64_t>(sh.tc.span / 4, 256));
      col_grow = std::min<int64_t>(col_grow, col->nbytes / 4 + (1 << 20));
    }
    cap_out = (int)((span_room + tile_grow + (tile_grow ? 127 : 0)) & ~(int64_t)(tile_grow ? 127 : 15));
    extra = col_grow;
  } else if (f.brefs) {
    // (the template may grow a row by any amount: room for twice the input, a launch that needs more says so and the
    // two-pass form takes over)
    cap_out = std::max(cap_out, 2 * cap);
    extra = std::max<int64_t>(extra, col->nbytes);
  }
  z->cap_out = cap_out;
  z->extra = extra;
}

StreamSizing replace_sizing(const ReplaceRun& r, const ReplaceShape& sh, const ReplaceForm& f, bool roomy) {
  const cs_regex* re = r.re;
  const int cap = sh.cap;
  StreamSizing z{};
  size_stream_output(r, sh, f, roomy, &z);
  const int bits_k = f.bits_form ? std::max(re->bits[1], 2) : 2;
  z.bits_lds = f.bits_form ? (size_t)bits_lds_bytes((int)re->bits.size()) : 0;
  // (the kernel's layout, k_tdfa_replace_stream: a bitmap's bytes, what stands behind the first one)
  const size_t bm = (size_t)(cap >> 3) + (f.bits_form ? 16 : 32);
  const size_t unit_bytes = f.bchain                          ? bm + 16 + kUnitQueue * 12
                            : (f.chain_form || f.bits_form) ? (size_t)(bits_k - 1) * bm + 16
                            : f.units                         ? (size_t)(bits_k - 1) * bm + kUnitQueue * 4 + 16 + (f.brefs ? kUnitQueue * 12 + 64 * 4 : 0)
                                                              : 0;
  // (backrefs: the group tags and the template text sit behind the DFA table)
  z.gt_bytes = f.brefs ? (f.bchain ? 0 : ((re->gtags.size() * 4 + 15) & ~size_t(15))) + (((size_t)r.c.tmpl_text_bytes + 31) & ~size_t(15)) : 0;
  // The chain arithmetic reads no table: when the tables are what keeps a third workgroup off the CU (the 26-instruction
  // dotted quad with `\b` and {1,3}: 36 states, 19 KB), they stay in memory -- only a sub-tile the arithmetic does not take
  // (bytes >= 0x80, a row beyond the masks) walks them there, and the sample says those are rare.
  const size_t tbl = r.tp.d.in_lds ? r.tp.lds_bytes : 0;
  const size_t tile_lds = z.gt_bytes + z.bits_lds + (size_t)(cap + z.cap_out + 64 + bm + unit_bytes) * 4 + 16;
  constexpr size_t kThird = 160 * 1024 / 3;
  // (the bit form likewise: its kernel with the tables in memory is built for three workgroups a CU -- 168 registers)
  // (... whenever its tile leaves room for three, whatever the tables' size: the form with the tables in LDS is the 189-register
  // one -- for patterns of up to five classes: the gtest pattern's seven fit a third workgroup too once the layout was trimmed,
  // but its evaluation then spills where it hurts: 8.4 against 7.1 ms)
  z.chain_global = ((f.chain_form && tbl + tile_lds > kThird && tile_lds + cstd::kHeadTailWords * 4 <= kThird) ||
                    (f.bits_form && re->bits[1] <= 5 && tile_lds + cstd::kHeadTailWords * 4 <= kThird) || ((f.chain_form || f.bits_form) && cs::cfg("CS_CHAIN_TABLES_IN_MEMORY"))) &&
                   !cs::cfg("CS_CHAIN_TABLES_IN_LDS");
  z.tbl_lds = (z.chain_global || f.bchain) ? (size_t)cstd::kHeadTailWords * 4 : tbl;  // (header + tail words: tsetup)
  z.lds1 = z.tbl_lds + tile_lds;
  return z;
}

// The rows a single pass leaves holes for (cs_virtual.hip: OddRows), a thread a row: sized before the launch (`lens`),
// written after it (`out_off`, `out_chars`).
void launch_hole_rows(const ReplaceRun& r, const OddRows* od, int32_t* lens, const int64_t* out_off, uint8_t* out_chars) {
  const hipStream_t s = r.c.s;
  const unsigned grid = (unsigned)std::min<int64_t>((od->count + 255) / 256, 2048);
  const size_t lds = r.tp.lds_bytes + (size_t)256 * kListRowBytes;  // (the tables and a row a thread)
  const auto kern = lens ? &k_tdfa_replace_list<false> : &k_tdfa_replace_list<true>;
  if (lds > 48 * 1024) CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope ps("k_tdfa_replace_list", s);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, r.src, r.tp.d, ptr<const int32_t>(od->list), od->count, ptr<const uint8_t>(r.d_repl), r.c.rb, lens, out_off, out_chars);
  CS_HIP(hipGetLastError());
  if (!lens) CS_HIP(hipStreamSynchronize(s));  // (the write pass: the column is handed out next)
}

// The route note of a form (cs_debug_last_route).
const char* replace_stream_route(const ReplaceShape& sh, const ReplaceForm& f) {
  return f.bits_form ? "bits" : f.bchain ? "brefs-chain" : f.brefs ? "brefs" : f.literal ? "literal" : sh.wide_stream ? "wide" : f.units ? (f.chain_pattern ? "chain" : "units") : "plain";
}

// The instantiation of k_tdfa_replace_stream a form runs on: every one the library holds is named here, once.  The
// parameters are <IN_LDS, REP16, INPLACE, RESCAN, LONG, UNITS, PF, BREFS, WIDE, OUTL, CHAIN, BITS, HOLES> (their
// meaning: at the kernel).  REP16 follows the replacement's length in every form but the templates'; a unit form is
// never in place and always rescans; the plain, wide and outlier forms are in place when nothing grows and rescan on
// the roomy attempt (the outlier and wide forms' first attempt is the roomy one).
// (tables in LDS: a DFA beyond the LDS budget never gets here -- the forms with the tables in memory that are not
// chain forms were never reached by a test and spilled 20-60 registers: out since round 6, kernel_coverage.txt)
using StreamKernel = void (*)(StreamArgs);
StreamKernel replace_stream_kernel(const ReplaceShape& sh, const ReplaceForm& f, bool chain_global, bool with_holes, bool roomy) {
  constexpr int P6 = cstile::kPfChunks;
  const bool r16 = f.rep16, lng = f.lng, pf5 = sh.cap <= 5 * 1024;
  if (!sh.outliers && !sh.wide_stream && !f.units) {  // the plain forms: the rows' lean scan
    if (f.inplace)
      return lng ? (r16 ? &k_tdfa_replace_stream<true, true, true, false, true> : &k_tdfa_replace_stream<true, false, true, false, true>)
                 : (r16 ? &k_tdfa_replace_stream<true, true, true, false, false> : &k_tdfa_replace_stream<true, false, true, false, false>);
    if (roomy)
      return lng ? (r16 ? &k_tdfa_replace_stream<true, true, false, true, true> : &k_tdfa_replace_stream<true, false, false, true, true>)
                 : (r16 ? &k_tdfa_replace_stream<true, true, false, true, false> : &k_tdfa_replace_stream<true, false, false, true, false>);
    return lng ? (r16 ? &k_tdfa_replace_stream<true, true, false, false, true> : &k_tdfa_replace_stream<true, false, false, false, true>)
               : (r16 ? &k_tdfa_replace_stream<true, true, false, false, false> : &k_tdfa_replace_stream<true, false, false, false, false>);
  }
  if (sh.outliers) {  // (the forms that handle oversize sub-tiles: in place, or with the rescan assembly)
    if (f.inplace)
      return r16 ? &k_tdfa_replace_stream<true, true, true, false, false, false, P6, false, false, true>
                 : &k_tdfa_replace_stream<true, false, true, false, false, false, P6, false, false, true>;
    return r16 ? &k_tdfa_replace_stream<true, true, false, true, false, false, P6, false, false, true>
               : &k_tdfa_replace_stream<true, false, false, true, false, false, P6, false, false, true>;
  }
  if (sh.wide_stream) {
    if (!r16) {
      if (f.inplace) return lng ? &k_tdfa_replace_stream<true, false, true, false, true, false, P6, false, true> : &k_tdfa_replace_stream<true, false, true, false, false, false, P6, false, true>;
      return lng ? &k_tdfa_replace_stream<true, false, false, true, true, false, P6, false, true> : &k_tdfa_replace_stream<true, false, false, true, false, false, P6, false, true>;
    }
    if (f.inplace) return lng ? &k_tdfa_replace_stream<true, true, true, false, true, false, P6, false, true> : &k_tdfa_replace_stream<true, true, true, false, false, false, P6, false, true>;
    return lng ? &k_tdfa_replace_stream<true, true, false, true, true, false, P6, false, true> : &k_tdfa_replace_stream<true, true, false, true, false, false, P6, false, true>;
  }
  if (f.bchain)
    return pf5 ? &k_tdfa_replace_stream<false, false, false, true, false, true, 5, true, false, false, true>
               : &k_tdfa_replace_stream<false, false, false, true, false, true, P6, true, false, false, true>;
  if (f.brefs) return pf5 ? &k_tdfa_replace_stream<true, false, false, true, false, true, 5, true> : &k_tdfa_replace_stream<true, false, false, true, false, true, P6, true>;
  if (f.bits_form && chain_global)
    return r16 ? &k_tdfa_replace_stream<false, true, false, true, false, true, P6, false, false, false, true, true>
               : &k_tdfa_replace_stream<false, false, false, true, false, true, P6, false, false, false, true, true>;
  if (f.bits_form)
    return r16 ? &k_tdfa_replace_stream<true, true, false, true, false, true, P6, false, false, false, true, true>
               : &k_tdfa_replace_stream<true, false, false, true, false, true, P6, false, false, false, true, true>;
  if (f.chain_form && chain_global)
    return r16 ? &k_tdfa_replace_stream<false, true, false, true, false, true, 5, false, false, false, true>
               : &k_tdfa_replace_stream<false, false, false, true, false, true, 5, false, false, false, true>;
  if (f.chain_form)
    return r16 ? &k_tdfa_replace_stream<true, true, false, true, false, true, 5, false, false, false, true>
               : &k_tdfa_replace_stream<true, false, false, true, false, true, 5, false, false, false, true>;
  // the unit form proper (literal needles ride it too): with the hole words only when the column has holes
  if (pf5 && with_holes) return r16 ? &k_tdfa_replace_stream<true, true, false, true, false, true, 5> : &k_tdfa_replace_stream<true, false, false, true, false, true, 5>;
  if (with_holes) return r16 ? &k_tdfa_replace_stream<true, true, false, true, false, true> : &k_tdfa_replace_stream<true, false, false, true, false, true>;
  if (pf5)
    return r16 ? &k_tdfa_replace_stream<true, true, false, true, false, true, 5, false, false, false, false, false, false>
               : &k_tdfa_replace_stream<true, false, false, true, false, true, 5, false, false, false, false, false, false>;
  return r16 ? &k_tdfa_replace_stream<true, true, false, true, false, true, P6, false, false, false, false, false, false>
             : &k_tdfa_replace_stream<true, false, false, true, false, true, P6, false, false, false, false, false, false>;
}

// The kernel's arguments.  `status` is carved into
// [aggregates nsub][error word + phase counters 16][tickets 128: sixteen counters][exclusive prefixes nsub]
// (+ kScanBatch windows of slack: the scanner wave fetches whole batches)
size_t stream_status_bytes(int64_t nsub) { return sizeof(cstile::u64) * (2 * (size_t)nsub + 16 + 128 + 64 * cstile::kScanBatch); }
StreamArgs replace_stream_args(const ReplaceRun& r, const ReplaceShape& sh, const ReplaceForm& f, const StreamSizing& z, const Buf& out_off, const Buf& out_chars, const Buf& status) {
  const cs::ReplaceCall& c = r.c;
  const cs_regex* re = r.re;
  StreamArgs sa{};
  sa.in = view_of(c.col);
  sa.flags = d_unicode_flags();
  sa.L = r.tp.d;
  if (z.chain_global || f.bchain) sa.L.in_lds = 2;
  sa.repl = ptr<const uint8_t>(r.d_repl);
  sa.rb = c.rb;
  sa.maxrepl = c.maxrepl;
  sa.out_off = ptr<int64_t>(out_off);
  sa.out_chars = ptr<uint8_t>(out_chars);
  sa.out_cap = c.col->nbytes + z.extra;
  sa.rows_per_tile = sh.tc.R;
  sa.nsub = (c.col->rows + sh.tc.R - 1) / sh.tc.R;
  sa.status = ptr<cstile::u64>(status);
  sa.error = reinterpret_cast<unsigned*>(sa.status + sa.nsub);
  sa.tickets = sa.status + sa.nsub + 16;
  sa.excl = sa.status + sa.nsub + 16 + 128;
  sa.cap_in = sh.cap;
  sa.cap_out = z.cap_out;
  sa.tbl_bytes = (int)(z.tbl_lds + z.gt_bytes + z.bits_lds);
  sa.bits = f.bits_form ? ptr<const int32_t>(re->d_bits) : nullptr;
  sa.bits_off = (int)(z.tbl_lds + z.gt_bytes);
  sa.bits_words = f.bits_form ? (int)re->bits.size() : 0;
  sa.bits_k = f.bits_form ? re->bits[1] : 0;
  sa.tmpl = static_cast<const csvm::BackrefTemplate*>(c.tmpl_dev);
  sa.gtags = f.brefs ? ptr<const int32_t>(re->d_gtags) : nullptr;
  sa.gt_off = (int)z.tbl_lds;
  sa.gt_words = f.brefs && !f.bchain ? (int)re->gtags.size() : 0;
  sa.debug = cs::cfg_int("CS_TILE_DEBUG", 0);
  sa.outliers = sh.outliers ? 1 : 0;
  sa.lit = f.literal ? c.literal : 0;
  sa.litn = f.literal ? c.literal_len : 0;
  return sa;
}

#if defined(CS_PHASE_PROF)
// CS_REPLACE_TRACE: a time stamp buffer for every 1024th sub-tile (cstile::g_tile_trace), null without the switch
Buf phase_prof_begin(int64_t nsub, hipStream_t s) {
  Buf tracebuf;
  const long long ntrace = (nsub >> 10) + 1;
  unsigned long long* tp_ = nullptr;
  if (cs::cfg("CS_REPLACE_TRACE")) {
    tracebuf = dev_alloc(sizeof(unsigned long long) * 4 * ntrace, s);
    CS_HIP(hipMemsetAsync(tracebuf->p, 0, sizeof(unsigned long long) * 4 * ntrace, s));
    tp_ = ptr<unsigned long long>(tracebuf);
  }
  CS_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(cstile::g_tile_trace), &tp_, sizeof(tp_), 0, hipMemcpyHostToDevice, s));
  return tracebuf;
}
void phase_prof_report(const StreamArgs& sa, const Buf& tracebuf, unsigned grid) {
  const long long nsub1 = sa.nsub, ntrace = (nsub1 >> 10) + 1;
  unsigned long long ph[12];
  CS_HIP(hipMemcpy(ph, reinterpret_cast<unsigned long long*>(sa.error) + 1, sizeof(ph), hipMemcpyDeviceToHost));
  if (tracebuf) {
    std::vector<unsigned long long> tr(4 * ntrace);
    CS_HIP(hipMemcpy(tr.data(), tracebuf->p, sizeof(unsigned long long) * 4 * ntrace, hipMemcpyDeviceToHost));
    unsigned long long t0 = ~0ull;
    for (long long i = 0; i < ntrace; ++i)
      if (tr[4 * i]) t0 = std::min(t0, tr[4 * i]);
    fprintf(stderr, "trace (us since the first publish; every 1024th sub-tile): tile published scanned start-of-finish prefix-seen\n");
    for (long long i = 0; i < ntrace; i += std::max<long long>(1, ntrace / 40))
      fprintf(stderr, "trace %8lld %9.1f %9.1f %9.1f %9.1f\n", i << 10, (double)(tr[4 * i] - t0) / 100.0, (double)(tr[4 * i + 1] - t0) / 100.0,
              (double)(tr[4 * i + 2] - t0) / 100.0, (double)(tr[4 * i + 3] - t0) / 100.0);
  }
  unsigned long long lb[4] = {0, 0, 0, 0};
  CS_HIP(hipMemcpyFromSymbol(lb, HIP_SYMBOL(cstile::g_lb_stats), sizeof(lb)));
  fprintf(stderr, "look-back (cumulative): %llu calls, %.2f windows per call, %.2f re-polls per call\n", lb[0], (double)lb[1] / (double)(lb[0] ? lb[0] : 1),
          (double)lb[2] / (double)(lb[0] ? lb[0] : 1));
  const double waves = (double)grid * 4;
  fprintf(stderr, "stage split: wait+lds %.0f classify %.0f rest %.0f | ", ph[9] / waves / (nsub1 / waves), ph[10] / waves / (nsub1 / waves), ph[0] / waves / (nsub1 / waves));
  fprintf(stderr, "phase cycles/wave-iteration: stage %.0f scan %.0f (units: discovery %.0f rounds %.0f) wscan+publish %.0f finish_prev(offsets+flush) %.0f assemble %.0f tail %.0f lookback %.0f (iters/wave %.1f)\n",
          ph[0] / waves / (nsub1 / waves), ph[1] / waves / (nsub1 / waves), ph[7] / waves / (nsub1 / waves), ph[8] / waves / (nsub1 / waves), ph[2] / waves / (nsub1 / waves),
          ph[3] / waves / (nsub1 / waves), ph[4] / waves / (nsub1 / waves), ph[5] / waves / (nsub1 / waves), ph[6] / waves / (nsub1 / waves), nsub1 / waves);
}
#endif

// CS_STREAM_INFO: what was launched
void print_stream_info(const ReplaceRun& r, const ReplaceShape& sh, const ReplaceForm& f, const StreamSizing& z, bool roomy, unsigned grid) {
  fprintf(stderr, "replace stream: grid %u lds %zu (tables %zu, tile %d + %d) rows/tile %d units %d chain %d wide %d brefs %d roomy %d growth %d rb %d\n", grid, z.lds1, z.tbl_lds + z.gt_bytes, sh.cap,
          z.cap_out, sh.tc.R, (int)f.units, f.bchain ? 3 : f.chain_form ? (z.chain_global ? 2 : 1) : 0, (int)sh.wide_stream, (int)f.brefs, (int)roomy, (int)sh.growth, r.c.rb);
}

// CS_DUMP_STATUS, development aid: where did the prefix chain stop?
void dump_stream_status(const StreamArgs& sa, int err, unsigned grid) {
  const int64_t nsub1 = sa.nsub;
  std::vector<cstile::u64> st((size_t)nsub1), ex((size_t)nsub1);
  CS_HIP(hipMemcpy(st.data(), sa.status, sizeof(cstile::u64) * nsub1, hipMemcpyDeviceToHost));
  CS_HIP(hipMemcpy(ex.data(), sa.excl, sizeof(cstile::u64) * nsub1, hipMemcpyDeviceToHost));
  unsigned long long tk[8];
  CS_HIP(hipMemcpy(tk, sa.tickets, sizeof(tk), hipMemcpyDeviceToHost));
  fprintf(stderr, "status dump: err %d nsub %lld grid %u ticket0 %llu\n", err, (long long)nsub1, grid, tk[0]);
  for (int64_t t = 0; t < nsub1 && t < 64; ++t)
    fprintf(stderr, "  tile %lld: agg flag %u val %llu | excl flag %u val %llu\n", (long long)t, (unsigned)(st[t] >> 62), (unsigned long long)(st[t] & cstile::kValMask),
            (unsigned)(ex[t] >> 62), (unsigned long long)(ex[t] & cstile::kValMask));
}

// what gave up, in words: the error word's bits and the column's shape (profiles/r04/soak.txt showed "error word 33"
// without saying that it is the backrefs form meeting a sub-tile with more than 128 matches); counted: cs_fallback_count
void note_stream_fallback(const ReplaceRun& r, int err) {
  const cs_column* col = r.c.col;
  char what[256];
  snprintf(what, sizeof(what), "%s (error word %d:%s%s%s%s%s%s; %lld rows, longest %lld bytes, largest 64-row span %lld)",
           r.c.tmpl_dev ? "replace_with_backrefs" : "replace_re", err, (err & 1) ? " launch abandoned" : "", (err & 2) ? " out of output room" : "",
           (err & 4) ? " a sub-tile beyond the staging buffer" : "", (err & 8) ? " no prefix for a tile" : "", (err & 16) ? " the scanners timed out" : "",
           (err & 32) ? " a sub-tile with more than 128 matches or a row handed over by the unit route (the template needs the unit route's masks)" : "",
           (long long)col->rows, (long long)col->max_row, (long long)col->max_span64);
  note_fallback(what);
}

// The output of a launch that succeeded becomes the column's, with metadata as a by-product: the largest 64-row span is
// the largest sub-tile total the kernel saw; a replacement no longer than the shortest match cannot lengthen a row (an
// upper bound serves: the numbers size staging buffers and pick routes); plain input + plain replacement stays plain
void adopt_stream_output(const ReplaceRun& r, const ReplaceShape& sh, const ReplaceForm& f, cs_column* o, const Buf& out_off, const Buf& out_chars, const int64_t* host) {
  const cs_column* col = r.c.col;
  o->offsets = out_off;
  o->chars = out_chars;
  o->nbytes = host[0];
  if (sh.tc.R == 64) o->max_span64 = host[2];
  if (sh.growth == 0 && col->max_row >= 0) o->max_row = col->max_row;
  if (col->high_sample == 0 && !f.brefs) {
    bool ascii = true;
    for (int i = 0; i < r.c.rb; ++i) ascii = ascii && (unsigned char)r.c.repl[i] < 0x80 && r.c.repl[i] != 0;
    if (ascii) o->high_sample = 0;
  }
}

// One launch of the persistent stream kernel (grid = what is resident at once).  Returns its error word (0: `o` holds the
// column), or -1 when the sizing does not fit.  `hole_lens` is taken once: a second, roomier attempt uses them again.
int replace_stream_attempt(const ReplaceRun& r, const ReplaceShape& sh, const ReplaceForm& f, bool roomy, Buf& hole_lens, cs_column* o) {
  const cs_column* col = r.c.col;
  const hipStream_t s = r.c.s;
  const StreamSizing z = replace_sizing(r, sh, f, roomy);
  if (z.lds1 > 150 * 1024) return -1;
  const int64_t rows = col->rows, nsub1 = (rows + sh.tc.R - 1) / sh.tc.R;
  Buf out_off = dev_alloc(sizeof(int64_t) * (rows + 1), s);
  Buf out_chars = dev_alloc((size_t)col->nbytes + (size_t)z.extra + 64, s);
  Buf status = dev_alloc(stream_status_bytes(nsub1), s);
  CS_HIP(hipMemsetAsync(status->p, 0, stream_status_bytes(nsub1), s));
  StreamArgs sa = replace_stream_args(r, sh, f, z, out_off, out_chars, status);
  const OddRows* od = sh.holes_ok && !f.literal && !f.brefs ? odd_rows(col, s) : nullptr;
  const bool with_holes = od && od->count > 0;
  if (with_holes) {
    if (!hole_lens) {
      hole_lens = dev_alloc(sizeof(int32_t) * (size_t)od->count, s);
      launch_hole_rows(r, od, ptr<int32_t>(hole_lens), nullptr, nullptr);
    }
    sa.hole_mask = ptr<const unsigned long long>(od->mask);
    sa.hole_first = ptr<const int64_t>(od->first);
    sa.hole_len = ptr<const int32_t>(hole_lens);
  }
  const StreamKernel kern = replace_stream_kernel(sh, f, z.chain_global, with_holes, roomy);
  note_route(replace_stream_route(sh, f));
  if (with_holes) note_route_put_off();
#if defined(CS_PHASE_PROF)
  Buf tracebuf = phase_prof_begin(nsub1, s);
#endif
  unsigned grid;
  {
    ProfScope ps("k_replace_re", s);
    grid = launch_resident(kern, z.lds1, (nsub1 + 3) / 4, s, sa);
  }
  if (cs::cfg("CS_STREAM_INFO")) print_stream_info(r, sh, f, z, roomy, grid);
  int64_t* host = (int64_t*)pinned_scratch(24);
  CS_HIP(hipMemcpyAsync(host, ptr<int64_t>(out_off) + rows, 8, hipMemcpyDeviceToHost, s));
  CS_HIP(hipMemcpyAsync(host + 1, sa.error, 4, hipMemcpyDeviceToHost, s));
  CS_HIP(hipMemcpyAsync(host + 2, reinterpret_cast<unsigned long long*>(sa.error) + 14, 8, hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
#if defined(CS_PHASE_PROF)
  phase_prof_report(sa, tracebuf, grid);
#endif
  const int err = (int)(uint32_t)host[1];
  if (err != 0 && cs::cfg("CS_DUMP_STATUS")) dump_stream_status(sa, err, grid);
  if (err != 0) return err;  // (a launch whose error word is set never yields a column, measurement switches or not)
  if (with_holes) {  // the holes' bytes
    launch_hole_rows(r, od, nullptr, ptr<const int64_t>(out_off), ptr<uint8_t>(out_chars));
  }
  adopt_stream_output(r, sh, f, o, out_off, out_chars, host);
  return 0;
}

// The single pass (when a match cannot be empty, or its replacement is short): shape, form, one attempt or two.
// An oversize sub-tile or a look-back timeout is counted as a fallback; the caller goes on to the two-pass kernels.
cs_column* replace_single_pass(const ReplaceRun& r, Built& b) {
  ReplaceShape sh;
  if (!replace_shape(r, &sh)) return nullptr;
  // (a DFA whose tables do not fit the LDS budget: the two-pass kernels read them from memory)
  if (!r.tp.d.in_lds) return nullptr;
  ReplaceForm f;
  if (!replace_form(r, sh, &f)) return nullptr;
  Buf hole_lens;
  int err = replace_stream_attempt(r, sh, f, sh.roomy_first, hole_lens, b.col.get());
  if (err == 2 && !sh.roomy_first) err = replace_stream_attempt(r, sh, f, true, hole_lens, b.col.get());  // only ran out of room: once more, roomier
  if (err == 0) return b.col.release();
  if (err > 0) note_stream_fallback(r, err);
  return nullptr;
}

// The two-pass kernels, a thread a row: `lens` for the size pass, `off` and `chars` for the write pass -- one pick by
// executor (wide DFA, DFA, list simulator) and by where its tables are serves both.
void launch_two_pass(const ReplaceRun& r, int32_t* lens, const int64_t* off, uint8_t* chars) {
  const cs::ReplaceCall& c = r.c;
  const TPlan& tp = r.tp;
  const Plan& pl = r.pl;
  // [the wide DFA, tables in LDS / in memory; the DFA, in LDS / in memory]  [the list simulator: small programs / the others]
  static constexpr decltype(&k_tdfa_replace_size<true>) dfa_size[4] = {&k_tdfa_replace_size<true, true>, &k_tdfa_replace_size<false, true>, &k_tdfa_replace_size<true>, &k_tdfa_replace_size<false>};
  static constexpr decltype(&k_replace_re_size<true>) vm_size[2] = {&k_replace_re_size<true>, &k_replace_re_size<false>};
  static constexpr decltype(&k_tdfa_replace_write<true>) dfa_write[4] = {&k_tdfa_replace_write<true, true>, &k_tdfa_replace_write<false, true>, &k_tdfa_replace_write<true>, &k_tdfa_replace_write<false>};
  static constexpr decltype(&k_replace_re_write<true>) vm_write[2] = {&k_replace_re_write<true>, &k_replace_re_write<false>};
  {
    ProfScope ps(lens ? "k_replace_re_size" : "k_replace_re_write", c.s);
    if (r.wide || r.tdfa) {
      const int k = (r.wide ? 0 : 2) + (tp.d.in_lds ? 0 : 1);
      const size_t lds = tp.d.in_lds ? tp.lds_bytes : 0;
      if (lens) hipLaunchKernelGGL(dfa_size[k], dim3(tp.grid), dim3(256), lds, c.s, r.src, tp.d, c.rb, c.maxrepl, lens);
      else hipLaunchKernelGGL(dfa_write[k], dim3(tp.grid), dim3(256), lds, c.s, r.src, tp.d, ptr<const uint8_t>(r.d_repl), c.rb, c.maxrepl, off, chars);
    } else {
      const int k = pl.small ? 0 : 1;
      if (lens) hipLaunchKernelGGL(vm_size[k], dim3(pl.grid), dim3(pl.threads), pl.lds_bytes, c.s, r.src, pl.d, c.rb, c.maxrepl, lens);
      else hipLaunchKernelGGL(vm_write[k], dim3(pl.grid), dim3(pl.threads), pl.lds_bytes, c.s, r.src, pl.d, ptr<const uint8_t>(r.d_repl), c.rb, c.maxrepl, off, chars);
    }
  }
  CS_HIP(hipGetLastError());
}
cs_column* replace_two_pass(const ReplaceRun& r, Built& b) {
  Buf lens = dev_alloc(sizeof(int32_t) * r.c.col->rows, r.c.s);
  launch_two_pass(r, ptr<int32_t>(lens), nullptr, nullptr);
  b.scan(ptr<int32_t>(lens));
  b.alloc_chars();
  launch_two_pass(r, nullptr, b.off, b.chars);
  CS_HIP(hipStreamSynchronize(r.c.s));  // d_repl / arena lifetime
  return b.col.release();
}

}  // namespace

namespace cs {
cs_column* replace_re_column(const ReplaceCall& c) {
  if (c.col->rows == 0) return make_all_null(0, c.s);
  note_route("");
  cs_regex* re = const_cast<cs_regex*>(c.re);
  ReplaceRun r{c, re, use_tdfa(re), use_tdfa_wide(re)};
  r.d_repl = dev_alloc((size_t)c.rb + 1, c.s);
  CS_HIP(hipMemcpyAsync(r.d_repl->p, c.repl, (size_t)c.rb + 1, hipMemcpyHostToDevice, c.s));
  if (r.tdfa || r.wide) r.tp = tplan(re, c.col->rows, c.s);
  else r.pl = plan(re, c.col->rows, c.s);
  if (cs_column* o = replace_on_pieces(r)) return o;
  if (cs_column* o = replace_by_class_runs(r)) return o;
  r.src = RowSrc{view_of(c.col), d_unicode_flags(), c.col->nbytes + (c.col->chars && c.col->chars->capacity ? 64 : 0)};
  Built b(c.col, c.s);  // (the single pass fills it itself: it allocates before it knows the sizes)
  if (cs_column* o = replace_single_pass(r, b)) return o;
  if (c.single_pass_only) fail(CS_ERR_INTERNAL, "literal replace: single-pass kernel not applicable");  // (the caller's own kernels are the fallback)
  return replace_two_pass(r, b);
}
}  // namespace cs

extern "C" {

// NVStrings::replace_re -- replace.cu:110-189
int cs_replace_re(const cs_column* col, const cs_regex* cre, const char* repl, int maxrepl, cs_stream stream,
                  cs_column** out) {
  return guard([&] {
    if (!col || !cre || !out) fail(CS_ERR_INVALID_ARG, "replace_re: null argument");
    if (cre->empty_pattern)
      fail(CS_ERR_INVALID_ARG, "nvstrings::replace_re parameter cannot be null or empty");  // replace.cu:112-113
    require_device();
    if (!repl) repl = "";
    *out = cs::replace_re_column(cs::ReplaceCall{col, cre, repl, (int)strlen(repl), maxrepl, S(stream)});
  });
}

// The spans' bytes into the output columns (extract / findall): 64-row sub-tiles through LDS when the column's
// sub-tiles fit the staging buffer, else the thread-per-row kernel.
void write_spans(const cs_column* col, int ncols, const int32_t* begins, const int32_t* lens, const ExtractOut& eo, hipStream_t s) {
  const int64_t rows = col->rows;
  const TileChoice tc = choose_tile(col, s);
  ProfScope ps("k_extract_write", s);
  if (tc.R == 64 && !cs::cfg("CS_SPANS_ROWWISE")) {
    SpanWriteArgs a{};
    a.in = view_of(col);
    a.ncols = ncols;
    a.begins = begins;
    a.lens = lens;
    a.out = eo;
    a.nsub = (rows + 63) / 64;
    a.cap = tc.cap;
    const size_t lds = (size_t)4 * (2 * tc.cap + 64);
    if (lds > 48 * 1024)
      CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_spans_write_tile), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned grid = (unsigned)std::min<long long>((a.nsub + 3) / 4, 256 * 16);
    hipLaunchKernelGGL(k_spans_write_tile, dim3(grid), dim3(256), lds, s, a);
  } else {
    hipLaunchKernelGGL(k_extract_write, dim3(blocks_for(rows)), dim3(256), 0, s, view_of(col), ncols, begins, lens, eo);
  }
}

// The output columns from PACKED spans and the scan kernel's tile totals (k_spans_write_tile2): no pass over the lengths.
void columns_from_packed_spans(const cs_column* col, int ncols, const uint32_t* spans, const int32_t* tile_tot, int cap, hipStream_t s,
                               std::vector<std::unique_ptr<cs_column>>& cols) {
  const int64_t rows = col->rows, nsub = (rows + 63) / 64;
  Buf base = dev_alloc(sizeof(int64_t) * (nsub + 1) * ncols, s);
  std::vector<int64_t> totals(ncols), largest(ncols);
  offsets_from_lengths_segmented(tile_tot, nsub, ncols, ptr<int64_t>(base), totals.data(), s, largest.data());
  SpanWrite2Args a{};
  a.in = view_of(col);
  a.ncols = ncols;
  a.spans = spans;
  a.tile_base = ptr<const int64_t>(base);
  a.nsub = nsub;
  a.cap = cap;
  bool off32 = !cs::cfg("CS_SPANS_OFF64");
  for (int k = 0; k < ncols; ++k) off32 = off32 && totals[k] < ((int64_t)1 << 31);
  a.off32 = off32 ? 1 : 0;
  for (int k = 0; k < ncols; ++k) {
    auto o = std::make_unique<cs_column>();
    o->rows = rows;
    o->nbytes = totals[k];
    if (off32) o->offsets32 = dev_alloc(sizeof(int32_t) * (rows + 1), s);
    else o->offsets = dev_alloc(sizeof(int64_t) * (rows + 1), s);
    o->validity = dev_alloc(validity_bytes(rows), s);
    o->chars = dev_alloc((size_t)o->nbytes, s);
    // (metadata for free: the largest tile total is the column's largest 64-row span; a span is a piece of its row)
    o->max_span64 = largest[k];
    o->max_row = col->max_row >= 0 ? std::min<int64_t>(col->max_row, largest[k]) : largest[k];
    if (col->plain_bytes == 1) o->plain_bytes = 1;
    if (col->high_sample == 0) o->high_sample = 0;
    a.out.off[k] = off32 ? o->offsets32->p : o->offsets->p;
    a.out.valid[k] = ptr<uint8_t>(o->validity);
    a.out.chars[k] = ptr<uint8_t>(o->chars);
    cols.push_back(std::move(o));
  }
  const size_t lds = (size_t)4 * (2 * cap + 64);
  if (lds > 48 * 1024)
    CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_spans_write_tile2), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const unsigned grid = (unsigned)std::min<long long>((nsub + 3) / 4, 256 * 64);  // (runs of consecutive tiles per wave; short ones share the tail out)
  {
    ProfScope ps("k_extract_write", s);
    hipLaunchKernelGGL(k_spans_write_tile2, dim3(grid), dim3(256), lds, s, a);
  }
  CS_HIP(hipGetLastError());
  CS_HIP(hipStreamSynchronize(s));  // `base` / span buffers
}

}  // extern "C"

// ---- extract / findall / replace_with_backrefs: the host routes ---------------------------------------------------------
// Each entry below reads as its sequence: the checks, the stream kernel (its FORM -- which variant of k_tdfa_scan_stream
// runs, on how much LDS --, the launch), otherwise the row-wise kernels, then the output columns.  Every kernel family's
// instantiations are named in one function.  As in the scans, choose_tile, sample_has_high_bytes, plan and scan<2> may
// launch a metadata pass the first time they are asked of a column: the order of the questions is kept.
namespace {

// The spans a scan leaves for the column writers: begins / lens [k * rows + row], or -- packed -- one word a span and the
// bytes every 64-row tile gives to each column (ScanStreamArgs::spans).
struct SpanBufs {
  Buf begins, lens, spans, tile_tot;
  bool packed = false;
  int cap = 0;  // packed: the tile size the scan staged its rows by (k_spans_write_tile2 stages by the same)
  void alloc(int64_t rows, int width, bool pack, hipStream_t s) {
    packed = pack;
    if (packed) {
      spans = dev_alloc(sizeof(uint32_t) * rows * width, s);
      tile_tot = dev_alloc(sizeof(int32_t) * ((rows + 63) / 64) * width, s);
    } else {
      begins = dev_alloc(sizeof(int32_t) * rows * width, s);
      lens = dev_alloc(sizeof(int32_t) * rows * width, s);
    }
  }
  // the outputs of a stream launch of `width` columns: the pair in use, the other null
  void give(ScanStreamArgs& sa, int width) const {
    sa.begins = packed ? nullptr : ptr<int32_t>(begins);
    sa.lens = packed ? nullptr : ptr<int32_t>(lens);
    sa.spans = packed ? ptr<uint32_t>(spans) : nullptr;
    sa.tile_tot = packed ? ptr<int32_t>(tile_tot) : nullptr;
    sa.ncols = width;
  }
};

// A call and what its steps share: the tagged DFA's launch plan is asked once, by the first step that needs it.
struct SpanRun {
  const cs_column* col;
  cs_regex* re;
  hipStream_t s;
  TPlan tp{};
  bool planned = false;
  const TPlan& plan_once() {
    if (!planned) tp = tplan(re, col->rows, s);
    planned = true;
    return tp;
  }
};

// The output columns from begins / lens, kMaxGroups at a time through the shared write kernel: a column's offsets from its
// lengths, its chars, then the spans' bytes.  Waits for the stream: the span buffers (and the list simulator's arena) are
// the caller's to release.
void columns_from_spans(const cs_column* col, int ncols, const int32_t* begins, const int32_t* lens, hipStream_t s,
                        std::vector<std::unique_ptr<cs_column>>& cols) {
  const int64_t rows = col->rows;
  for (int k0 = 0; k0 < ncols; k0 += kMaxGroups) {
    const int nk = std::min(kMaxGroups, ncols - k0);
    ExtractOut eo{};
    for (int k = 0; k < nk; ++k) {
      Built b(rows, Nulls::fused, s);
      b.scan(lens + (size_t)(k0 + k) * rows);
      eo.off[k] = b.off;
      eo.chars[k] = b.alloc_chars();
      cols.push_back(std::move(b.col));
    }
    write_spans(col, nk, begins + (size_t)k0 * rows, lens + (size_t)k0 * rows, eo, s);
  }
  CS_HIP(hipGetLastError());
  CS_HIP(hipStreamSynchronize(s));
}
void columns_from(const cs_column* col, int ncols, const SpanBufs& sp, hipStream_t s, std::vector<std::unique_ptr<cs_column>>& cols) {
  if (sp.packed) columns_from_packed_spans(col, ncols, ptr<const uint32_t>(sp.spans), ptr<const int32_t>(sp.tile_tot), sp.cap, s, cols);
  else columns_from_spans(col, ncols, ptr<int32_t>(sp.begins), ptr<int32_t>(sp.lens), s, cols);
}

// ---- extract ----
// Which variant of k_tdfa_scan_stream<4, ..> runs, and on how much LDS.
struct ExtractForm {
  // a chain pattern whose groups are runs of items, on a column whose sample is plain ASCII: the match and the group ranges
  // by mask arithmetic; it keeps the "equals x" bitmap and the unit form's layout
  bool chain_form;
  // ... with the tables in memory: a fourth workgroup per CU -- the kernel is built for 128 registers then
  bool chain_mem;
  bool packed;      // 64-row tiles: packed spans and tile totals, no pass over the lengths
  size_t tbl_x;     // bytes of the automaton's tables in LDS: all of them, or -- chain_mem -- header + tail words
  size_t gt_bytes;  // the group tags behind them
  size_t lds;       // dynamic LDS of a workgroup; beyond 150 KB there is no stream launch
  ScanStreamKernel kern;
};
// The instantiations of k_tdfa_scan_stream extract holds: <4, IN_LDS, LONG, UNITS, CHAIN>.
ScanStreamKernel extract_stream_kernel(bool lng, bool chain_form, bool chain_mem) {
  if (!chain_form) return lng ? &k_tdfa_scan_stream<4, true, true> : &k_tdfa_scan_stream<4, true, false>;
  return chain_mem ? &k_tdfa_scan_stream<4, false, false, true, true> : &k_tdfa_scan_stream<4, true, false, true, true>;
}
ExtractForm extract_form(const SpanRun& r, int groups, const TileChoice& tc) {
  const cs_regex* re = r.re;
  const int cap = tc.cap;
  ExtractForm f{};
  f.gt_bytes = gtags_lds_bytes(re);
  f.chain_form = r.tp.d.in_lds && tc.R == 64 && !tc.lng && !cs::cfg("CS_SPANS_UNPACKED") && ((re->tdfa[30] >> 16) & 15) != 0 && ((re->tdfa[30] >> 20) & 1) != 0 &&
                 groups <= 4 && !cs::cfg("CS_NO_CHAIN_FORM") && !sample_has_high_bytes(r.col, r.s);
  f.chain_mem = f.chain_form && !cs::cfg("CS_CHAIN_TABLES_IN_LDS");
  f.tbl_x = f.chain_mem ? (size_t)cstd::kHeadTailWords * 4 : r.tp.lds_bytes;
  f.lds = f.chain_form ? f.tbl_x + f.gt_bytes + (size_t)(cap + 32 + 2 * ((cap >> 3) + 32) + kUnitQueue * 4 + 64 * 4 + 16) * 4
                       : r.tp.lds_bytes + f.gt_bytes + (size_t)(cap + 32 + (cap >> 3) + 32 + cstd::Tdfa::kBackSteps * 64 + kMaxGroups * 4) * 4;
  f.packed = tc.R == 64 && !cs::cfg("CS_SPANS_UNPACKED");
  f.kern = extract_stream_kernel(tc.lng, f.chain_form, f.chain_mem);
  return f;
}

// The stream kernel: rows staged through LDS tiles, the DFA carries the group ranges.
bool extract_stream(SpanRun& r, int groups, SpanBufs& sp) {
  const hipStream_t s = r.s;
  const TPlan& tp = r.plan_once();
  const TileChoice tc = choose_tile(r.col, s);
  const ExtractForm f = extract_form(r, groups, tc);
  if (!tp.d.in_lds || !tc.R || f.lds > 150 * 1024) return false;
  sp.alloc(r.col->rows, groups, f.packed, s);
  sp.cap = tc.cap;
  const Buf cnt = zeroed_count(s);
  ScanStreamArgs sa = stream_args(r.col, tp, tc);
  sa.found = ptr<unsigned long long>(cnt);
  sa.tbl_bytes = (int)(f.tbl_x + f.gt_bytes);
  sa.gt_off = (int)f.tbl_x;
  if (f.chain_mem) sa.L.in_lds = 2;
  sa.gt_words = f.gt_bytes ? (int)r.re->gtags.size() : 0;
  sp.give(sa, groups);
  sa.gtags = ptr<const int32_t>(r.re->d_gtags);
  ProfScope ps("k_extract_spans", s);
  launch_resident(f.kern, f.lds, (sa.nsub + 3) / 4, s, sa);
  return true;
}

// The row-wise kernels' instantiations, a family each: the DFA with the group ranges, the DFA for the match and the list
// simulator for the groups, the list simulator alone (SMALL: at most 64 instructions).
using ExtractDfaKernel = void (*)(RowSrc, TLaunch, const int32_t*, int, int32_t*, int32_t*);
using ExtractTdfaKernel = void (*)(RowSrc, TLaunch, Launch, int, int, int32_t*, int32_t*);
using ExtractListKernel = void (*)(RowSrc, Launch, int, int32_t*, int32_t*);
ExtractDfaKernel extract_dfa_kernel(bool in_lds) { return in_lds ? &k_extract_spans_dfa<true> : &k_extract_spans_dfa<false>; }
ExtractTdfaKernel extract_tdfa_kernel(bool in_lds, bool small) {
  if (in_lds) return small ? &k_extract_spans_tdfa<true, true> : &k_extract_spans_tdfa<true, false>;
  return small ? &k_extract_spans_tdfa<false, true> : &k_extract_spans_tdfa<false, false>;
}
ExtractListKernel extract_list_kernel(bool small) { return small ? &k_extract_spans<true> : &k_extract_spans<false>; }

// A thread a row, begins / lens.  `arena`: the thread lists of the list simulation, not needed when the DFA carries the
// group ranges; the caller keeps it until it has waited for the stream.
void extract_rowwise(SpanRun& r, int groups, bool dfa_groups, Buf& arena, SpanBufs& sp) {
  const hipStream_t s = r.s;
  const int64_t rows = r.col->rows;
  const int ninst = (int)r.re->prog.insts.size();
  Launch L{};
  L.image = ptr<const int32_t>(r.re->d_image);
  L.image_words = (int)r.re->image.size();
  L.slots = csvm::gvm_slots(ninst);
  const size_t img_bytes = (((size_t)L.image_words + 3) & ~size_t(3)) * 4;
  L.image_in_lds = img_bytes <= kLdsBudget / 2;
  const unsigned grid = (unsigned)std::min<int64_t>((rows + 255) / 256, 256 * 4);
  if (!dfa_groups) {
    arena = dev_alloc((size_t)grid * 256 * L.slots * 4, s);
    L.arena = ptr<uint32_t>(arena);
  }
  const RowSrc src = row_src(r.col);
  sp.alloc(rows, groups, false, s);
  int32_t* const begins = ptr<int32_t>(sp.begins);
  int32_t* const lens = ptr<int32_t>(sp.lens);
  if (dfa_groups) {
    const TPlan& tp = r.plan_once();
    ProfScope ps("k_extract_spans", s);
    hipLaunchKernelGGL(extract_dfa_kernel(tp.d.in_lds), dim3(tp.grid), dim3(256), tp.lds_bytes, s, src, tp.d, ptr<const int32_t>(r.re->d_gtags), groups, begins, lens);
  } else if (use_tdfa(r.re)) {
    const TPlan& tp = r.plan_once();
    size_t fast_bytes = (size_t)256 * csvm::GroupVm<true>::kFastSlots * 4;
    const int use_fast = tp.lds_bytes + fast_bytes <= kLdsBudget;
    if (!use_fast) fast_bytes = 0;
    L.image_in_lds = tp.lds_bytes + fast_bytes + img_bytes <= kLdsBudget;
    const size_t lds = tp.lds_bytes + fast_bytes + (L.image_in_lds ? img_bytes : 0);
    ProfScope ps("k_extract_spans", s);
    hipLaunchKernelGGL(extract_tdfa_kernel(tp.d.in_lds, ninst <= 64), dim3(grid), dim3(256), lds, s, src, tp.d, L, groups, use_fast, begins, lens);
  } else {
    ProfScope ps("k_extract_spans", s);
    hipLaunchKernelGGL(extract_list_kernel(ninst <= 64), dim3(grid), dim3(256), L.image_in_lds ? img_bytes : 0, s, src, L, groups, begins, lens);
  }
}

// ---- findall ----
// Which variant of k_tdfa_scan_stream<3, ..> runs, and on how much LDS (as count_re's: scan_form).
struct FindallForm {
  bool units;         // the unit scan where the tagged DFA offers the decomposition
  bool chain_scan;    // a chain pattern on a column whose sample is plain ASCII
  bool chain_global;  // ... its tables in memory where that makes room for a fourth workgroup per CU
  size_t lds;         // dynamic LDS of a workgroup; beyond 150 KB there is no stream launch
  size_t scan_tbl;    // bytes of the automaton's tables in LDS: all of them, or -- chain_global -- header + tail words
  ScanStreamKernel kern;
};
// (the instantiations of k_tdfa_scan_stream findall holds are named here: <3, IN_LDS, LONG, UNITS, CHAIN>)
FindallForm findall_form(const SpanRun& r, const TileChoice& tc) {
  const cs_regex* re = r.re;
  const TPlan& tp = r.tp;
  const int cap = tc.cap;
  FindallForm f{};
  f.units = ((re->tdfa[31] & 1) != 0 || ((re->tdfa[30] >> 16) & 15) != 0) && !tc.lng && tc.R == 64 && !cs::cfg("CS_NO_UNITS");
  f.lds = tp.lds_bytes + (size_t)(cap + 32 + (cap >> 3) + 32 + (f.units ? (cap >> 3) + 32 + kUnitQueue * 4 + 64 * 4 + 16 : 0)) * 4;
  f.chain_scan = f.units && ((re->tdfa[30] >> 16) & 15) != 0 && !sample_has_high_bytes(r.col, r.s) && !cs::cfg("CS_NO_CHAIN_FORM");
  f.chain_global = f.chain_scan && tp.d.in_lds && f.lds > 40 * 1024 && f.lds - tp.lds_bytes + cstd::kHeadTailWords * 4 <= 40 * 1024 && !cs::cfg("CS_CHAIN_TABLES_IN_LDS");
  f.scan_tbl = f.chain_global ? (size_t)cstd::kHeadTailWords * 4 : tp.lds_bytes;
  if (f.chain_global) f.lds -= tp.lds_bytes - f.scan_tbl;
  if (!f.units) f.kern = tc.lng ? &k_tdfa_scan_stream<3, true, true> : &k_tdfa_scan_stream<3, true, false>;
  else if (!f.chain_scan) f.kern = &k_tdfa_scan_stream<3, true, false, true>;
  else if (!f.chain_global) f.kern = &k_tdfa_scan_stream<3, true, false, true, true>;
  else f.kern = &k_tdfa_scan_stream<3, false, false, true, true>;
  return f;
}

// The largest match count of a row: an int the kernels raise, zeroed before every launch that reports it and read as the
// four bytes it is (read_count copies a 64-bit count: another copy, so findall keeps its reader).
int read_max(const Buf& dmax, hipStream_t s) {
  int* hmax = (int*)pinned_scratch(8);
  CS_HIP(hipMemcpyAsync(hmax, dmax->p, 4, hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  return hmax[0];
}

// The stream kernel reports spans and the largest match count in ONE pass when the rows hold at most kProvisional matches
// (the span arrays are laid out [k * rows + row], so unused columns cost only memory); a column with busier rows is scanned
// a second time with the exact column count, into span buffers of its own.  Returns the column count, -1: not taken.
// `exact_width` (split_re: the count scan ran first, the width is known): one launch at that width, packed up to
// `pack_limit` columns, no maximum reported or read back.
int findall_stream(SpanRun& r, const Buf& dmax, SpanBufs& sp, int exact_width = 0, int pack_limit = kMaxGroups) {
  constexpr int kProvisional = 4;
  const hipStream_t s = r.s;
  const int64_t rows = r.col->rows;
  const TPlan& tp = r.plan_once();
  const TileChoice tc = choose_tile(r.col, s);
  const FindallForm f = findall_form(r, tc);
  if (!tp.d.in_lds || !tc.R || f.lds > 150 * 1024) return -1;
  const Buf hits = zeroed_count(s);
  ScanStreamArgs sa = stream_args(r.col, tp, tc);
  sa.found = ptr<unsigned long long>(hits);  // (hit counter: nobody reads it, the kernel writes through it)
  sa.tbl_bytes = (int)f.scan_tbl;
  if (f.chain_global) sa.L.in_lds = 2;
  sa.maxp = exact_width ? nullptr : ptr<int>(dmax);
  sp.cap = tc.cap;
  int ncols = 0, width = exact_width ? exact_width : kProvisional;
  for (int pass = 0; pass < 2; ++pass) {
    // (the provisional pass on 64-row tiles leaves packed spans and tile totals: k_spans_write_tile2 needs no pass
    // over the lengths; a second pass -- rows with more than kProvisional matches -- writes begins / lens)
    sp.alloc(rows, width, tc.R == 64 && width <= pack_limit && (pass == 0 || !cs::cfg("CS_SPANS_EXACT_UNPACKED")) && !cs::cfg("CS_SPANS_UNPACKED"), s);
    CS_HIP(hipMemsetAsync(dmax->p, 0, 8, s));
    sp.give(sa, width);
    {
      ProfScope ps("k_findall_spans", s);
      launch_resident(f.kern, f.lds, (sa.nsub + 3) / 4, s, sa);
    }
    if (exact_width) return width;
    ncols = read_max(dmax, s);
    if (ncols <= width) break;
    width = ncols;  // busier rows than provisioned for: once more, exactly
  }
  return ncols;
}

// Matches per row (count_re: scan<2>), their maximum = the number of columns.
// `keep` (split_re): receives the counts.
int findall_count_rows(const SpanRun& r, const Buf& dmax, Buf* keep = nullptr) {
  const hipStream_t s = r.s;
  const int64_t rows = r.col->rows;
  Buf counts = dev_alloc(sizeof(int32_t) * rows, s);
  if (keep) *keep = counts;
  scan<2>(ScanCall{r.col, r.re, counts->p, sizeof(int32_t), 1, s, nullptr, "k_count_re"});
  CS_HIP(hipMemsetAsync(dmax->p, 0, 8, s));
  hipLaunchKernelGGL(k_max_i32, dim3((unsigned)std::min<int64_t>((rows + 255) / 256, 2048)), dim3(256), 0, s, ptr<int32_t>(counts), rows,
                     ptr<int>(dmax));
  return read_max(dmax, s);
}

// The row-wise kernels' instantiations: the tagged DFA (tables in LDS or in memory), the list simulator (SMALL: at most 64
// instructions).
using FindallTdfaKernel = void (*)(RowSrc, TLaunch, int, int32_t*, int32_t*);
using FindallListKernel = void (*)(RowSrc, Launch, int, int32_t*, int32_t*);
FindallTdfaKernel findall_tdfa_kernel(bool in_lds) { return in_lds ? &k_findall_spans_tdfa<true> : &k_findall_spans_tdfa<false>; }
FindallListKernel findall_list_kernel(bool small) { return small ? &k_findall_spans<true> : &k_findall_spans<false>; }

// A thread a row, the first `ncols` spans of every row into begins / lens.  Returns the list simulator's plan: its arena is
// the caller's to keep until it has waited for the stream.
Plan findall_rowwise(SpanRun& r, int ncols, SpanBufs& sp) {
  const hipStream_t s = r.s;
  const int64_t rows = r.col->rows;
  const RowSrc src = row_src(r.col);
  Plan pl{};
  sp.alloc(rows, ncols, false, s);
  ProfScope ps("k_findall_spans", s);
  if (use_tdfa(r.re)) {
    const TPlan& tp = r.plan_once();
    hipLaunchKernelGGL(findall_tdfa_kernel(tp.d.in_lds), dim3(tp.grid), dim3(256), tp.lds_bytes, s, src, tp.d, ncols, ptr<int32_t>(sp.begins), ptr<int32_t>(sp.lens));
  } else {
    pl = plan(r.re, rows, s);
    hipLaunchKernelGGL(findall_list_kernel(pl.small), dim3(pl.grid), dim3(pl.threads), pl.lds_bytes, s, src, pl.d, ncols, ptr<int32_t>(sp.begins), ptr<int32_t>(sp.lens));
  }
  return pl;
}

// ---- replace_with_backrefs ----
struct BackrefTemplateText {
  csvm::BackrefTemplate t;  // (t.text is set once the text is on the device)
  std::string text;         // the template without its references
};
// backref.h:31-57: a backslash followed by digits is a reference.  Host only.
BackrefTemplateText parse_backref_template(const char* repl, const cs_regex* re) {
  BackrefTemplateText p{};
  csvm::BackrefTemplate& t = p.t;
  for (const char* c = repl; *c;) {
    if (*c == '\\' && c[1] >= '0' && c[1] <= '9') {
      const char* q = c + 1;
      while (*q >= '0' && *q <= '9') ++q;
      if (t.nrefs == csvm::BackrefTemplate::kMaxRefs) fail(CS_ERR_RANGE, "replace_with_backrefs: more than 16 references in the template");
      t.idx[t.nrefs] = atoi(c + 1);
      t.pos[t.nrefs] = (int)p.text.size();
      ++t.nrefs;
      c = q;
    } else {
      p.text.push_back(*c++);
    }
  }
  t.bytes = (int)p.text.size();
  t.groups = re->prog.num_groups;
  return p;
}

// First choice: the single-pass replace kernel in its backrefs form (unit scan, one group run per match, coalesced
// output).  It declines patterns without the unit decomposition, more than four groups, long rows; a launch that
// runs out of output room or meets a row the unit route hands over reports it.  Says whether it answered: whatever
// fails in there -- declined, out of room, a HIP error --, the two-pass form answers.
bool backrefs_single_pass(const cs_column* col, cs_regex* re, const csvm::BackrefTemplate& t, bool dfa, hipStream_t s, cs_column** out) {
  bool packs = t.bytes <= 255;  // (the kernel keeps the references' group numbers and positions packed in registers)
  for (int j = 0; j < t.nrefs; ++j) packs = packs && t.idx[j] <= 15 && t.pos[j] <= 255;
  if (!dfa || !packs || re->prog.num_groups < 1 || cs::cfg("CS_BACKREFS_TWO_PASS")) return false;
  Buf d_t = dev_alloc(sizeof(csvm::BackrefTemplate), s);
  CS_HIP(hipMemcpyAsync(d_t->p, &t, sizeof(t), hipMemcpyHostToDevice, s));
  CS_HIP(hipStreamSynchronize(s));  // (`t` lives on the caller's stack frame)
  cs::ReplaceCall call{col, re, "", 0, -1, s};
  call.tmpl_host = &t;
  call.tmpl_dev = d_t->p;
  call.tmpl_text_bytes = t.bytes;
  call.single_pass_only = true;
  return guard([&] { *out = cs::replace_re_column(call); }) == CS_OK;
}

// The instantiations of the two-pass form: k_backrefs<DFA, IN_LDS, SMALL, WRITE>, a thread a row, and the stream kernel
// k_tdfa_scan_stream<5 sizes | 6 bytes, IN_LDS, LONG>.
using BackrefsKernel = void (*)(BackrefArgs, int32_t*, const int64_t*, uint8_t*);
BackrefsKernel backrefs_kernel(bool dfa, bool in_lds, bool small, bool write) {
  if (dfa && in_lds) return write ? &k_backrefs<true, true, true, true> : &k_backrefs<true, true, true, false>;
  if (dfa) return write ? &k_backrefs<true, false, true, true> : &k_backrefs<true, false, true, false>;
  if (small) return write ? &k_backrefs<false, false, true, true> : &k_backrefs<false, false, true, false>;
  return write ? &k_backrefs<false, false, false, true> : &k_backrefs<false, false, false, false>;
}
ScanStreamKernel backrefs_stream_kernel(bool write, bool lng) {
  if (write) return lng ? &k_tdfa_scan_stream<6, true, true> : &k_tdfa_scan_stream<6, true, false>;
  return lng ? &k_tdfa_scan_stream<5, true, true> : &k_tdfa_scan_stream<5, true, false>;
}

// The two-pass form: sizes, offsets, bytes.  What its two launches share.
struct BackrefsTwoPass {
  hipStream_t s;
  bool dfa;       // the tagged DFA carries the groups (or there are none)
  bool small;     // the list simulator's program has at most 64 instructions
  BackrefArgs a;  // the row-wise kernels': a thread a row
  unsigned grid;
  size_t lds;
  Buf arena;      // (the list simulator's thread lists)
  // rows staged through LDS tiles by the scan stream kernel when the DFA carries the groups and the tiles fit
  bool stream, lng;
  size_t slds;
  ScanStreamArgs sa;
  Buf d_tmpl;  // the template once more, in device memory: the stream kernel indexes it per reference
  Buf scnt;    // the stream kernel's hit counter, made at its first launch
};
BackrefsTwoPass backrefs_plan(const cs_column* col, cs_regex* re, const csvm::BackrefTemplate& t, bool dfa, hipStream_t s) {
  const int64_t rows = col->rows;
  const int ninst = (int)re->prog.insts.size();
  BackrefsTwoPass p{};
  p.s = s;
  p.dfa = dfa;
  p.small = ninst <= 64;
  p.a.src = row_src(col);
  p.a.gtags = ptr<const int32_t>(re->d_gtags);
  p.a.t = t;
  p.grid = (unsigned)std::min<int64_t>((rows + 255) / 256, 256 * 8);
  TPlan tp{};
  if (dfa) {
    tp = tplan(re, rows, s);
    p.a.TL = tp.d;
    p.lds = tp.lds_bytes;
  } else {
    p.a.L.image = ptr<const int32_t>(re->d_image);
    p.a.L.image_words = (int)re->image.size();
    p.a.L.slots = csvm::gvm_slots(ninst);
    p.grid = std::min(p.grid, 1024u);
    p.arena = dev_alloc((size_t)p.grid * 256 * p.a.L.slots * 4, s);
    p.a.L.arena = ptr<uint32_t>(p.arena);
  }
  if (!(dfa && p.a.TL.in_lds && !cs::cfg("CS_REGEX_ROWWISE"))) return p;
  const TileChoice tc = choose_tile(col, s);
  const size_t gt_bytes = gtags_lds_bytes(re);
  p.slds = p.lds + gt_bytes + (size_t)(tc.cap + 32 + (tc.cap >> 3) + 32) * 4;
  if (!tc.R || p.slds > 150 * 1024) return p;
  p.stream = true;
  p.lng = tc.lng;
  p.sa = stream_args(col, tp, tc);
  p.sa.gt_off = (int)p.lds;
  p.sa.gt_words = gt_bytes ? (int)re->gtags.size() : 0;
  p.sa.tbl_bytes = (int)(p.lds + gt_bytes);
  p.sa.gtags = p.a.gtags;
  p.d_tmpl = dev_alloc(sizeof(csvm::BackrefTemplate), s);
  CS_HIP(hipMemcpyAsync(p.d_tmpl->p, &t, sizeof(t), hipMemcpyHostToDevice, s));
  p.sa.tmpl = ptr<const csvm::BackrefTemplate>(p.d_tmpl);
  return p;
}
// One of the two launches: sizes into `lens`, or -- write -- the bytes at `off` into `chars`.
void backrefs_launch(BackrefsTwoPass& p, bool write, int32_t* lens, const int64_t* off, uint8_t* chars) {
  if (!p.stream) {
    hipLaunchKernelGGL(backrefs_kernel(p.dfa, p.a.TL.in_lds, p.small, write), dim3(p.grid), dim3(256), p.lds, p.s, p.a, lens, off, chars);
    CS_HIP(hipGetLastError());
    return;
  }
  if (!p.scnt) {
    p.scnt = zeroed_count(p.s);
    p.sa.found = ptr<unsigned long long>(p.scnt);
  }
  launch_resident(backrefs_stream_kernel(write, p.lng), p.slds, (p.sa.nsub + 3) / 4, p.s, p.sa);
}
void backrefs_size(BackrefsTwoPass& p, int32_t* lens) {
  p.sa.out32 = lens;
  backrefs_launch(p, false, lens, nullptr, nullptr);
}
void backrefs_write(BackrefsTwoPass& p, const int64_t* off, uint8_t* chars) {
  p.sa.out_off = off;
  p.sa.out_chars = chars;
  backrefs_launch(p, true, nullptr, off, chars);
}

cs_column* backrefs_two_pass(const cs_column* col, cs_regex* re, const csvm::BackrefTemplate& t, bool dfa, hipStream_t s) {
  BackrefsTwoPass p = backrefs_plan(col, re, t, dfa, s);
  Built b(col, s);
  Buf lens = dev_alloc(sizeof(int32_t) * col->rows, s);
  {
    ProfScope ps("k_backrefs_size", s);
    backrefs_size(p, ptr<int32_t>(lens));
  }
  b.scan(ptr<int32_t>(lens));
  b.alloc_chars();
  {
    ProfScope ps("k_backrefs_write", s);
    backrefs_write(p, b.off, b.chars);
  }
  CS_HIP(hipStreamSynchronize(s));
  return b.col.release();
}

// ---- split_re / rsplit_re (splitre_ops.h) ----
// Token spans from match spans.  A wave takes a 64-row tile, a lane a row: for token column k the lanes read their
// rows' cut k -- match span k, or for rsplit_re with a limit match span m - s + k, m from the count scan -- from the
// span arrays [k * rows + row], form token k from the end of the previous cut, the begin of this one and the row's
// byte length (cssre::token_span), and write it in the layout the match spans came in.  PACKED: one word a span and
// every column's bytes of the tile, summed over the wave, as tile_tot[column][tile] (what k_spans_write_tile2 sizes
// the columns from); otherwise begins / lens.  No LDS.
struct TokenSpanArgs {
  ColView in;
  const int32_t* counts;  // matches per row (count_re)
  int maxsplit, reverse;
  int mwidth;  // match columns the scan left
  int ncols;   // token columns
  const uint32_t* mspans;  // PACKED
  const int32_t* mbegins;  // otherwise
  const int32_t* mlens;
  uint32_t* tspans;   // PACKED
  int32_t* tile_tot;
  int32_t* tbegins;   // otherwise
  int32_t* tlens;
  long long nsub;
};
template <bool PACKED>
__global__ void __launch_bounds__(256) k_token_spans(TokenSpanArgs a) {
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const long long rows = a.in.rows;
  for (long long tile = (long long)blockIdx.x * 4 + wv; tile < a.nsub; tile += (long long)gridDim.x * 4) {
    const long long r = tile * 64 + lane;
    const bool in_rows = r < rows;
    const bool live = in_rows && row_is_valid(a.in.validity, r);
    int n = 0, m = 0;
    if (live) {
      n = (int)(a.in.offsets[r + 1] - a.in.offsets[r]);
      m = max(a.counts[r], 0);
    }
    const int s = live ? cssre::cuts(m, a.maxsplit) : -1;  // (-1: no token 0 either)
    const int c0 = cssre::first_cut(m, max(s, 0), a.reverse != 0);
    cssre::Walk w;
    for (int k = 0; k < a.ncols; ++k) {
      int mb = n, ml = 0;
      if (in_rows && c0 + k < a.mwidth) {  // (not `k < s`: the address does not wait for the row's cut count)
        const long long at = (long long)(c0 + k) * rows + r;
        if (PACKED) {
          const uint32_t x = a.mspans[at];
          if (x != cssre::kNullSpan) {
            mb = (int)(x >> 16);
            ml = (int)(x & 0xFFFFu);
          }
        } else {
          const int len = a.mlens[at];
          if (len >= 0) {
            mb = a.mbegins[at];
            ml = len;
          }
        }
      }
      // (the span writers trust begin + length to lie inside the row: a cut is kept behind the previous one and inside the row)
      mb = min(max(mb, w.prev_end), n);
      ml = min(ml, n - mb);
      int tb = 0, tl = 0;
      const bool has = live && cssre::token_span(w, k, s, n, mb, ml, tb, tl);
      const long long to = (long long)k * rows + r;
      if (PACKED) {
        if (in_rows) a.tspans[to] = has ? ((uint32_t)tb << 16) | (uint32_t)tl : cssre::kNullSpan;
        const int tot = wave_reduce_sum(has ? tl : 0);
        if (lane == 0) a.tile_tot[(long long)k * a.nsub + tile] = tot;
      } else if (in_rows) {
        a.tbegins[to] = has ? tb : 0;
        a.tlens[to] = has ? tl : -1;
      }
    }
  }
}

// One split_re / rsplit_re call and what its steps share.
struct SplitReCall {
  SpanRun r;
  int maxsplit;
  bool reverse;
  Buf counts;          // matches per row
  int most = 0;        // ... of the busiest row (M)
  int width = 0;       // match columns scanned (W)
  int ntokens = 0;     // token columns
  SpanBufs matches, tokens;
  Plan pl{};           // (findall_rowwise: the list simulator's arena lives until the columns are written)
};
// Step 1: matches per row and their maximum; with it the widths of the match scan and of the result.
void splitre_count(SplitReCall& c) {
  Buf dmax = dev_alloc(8, c.r.s);
  c.most = findall_count_rows(c.r, dmax, &c.counts);
  const int cut = c.maxsplit > 0 ? std::min(c.most, c.maxsplit) : c.most;
  c.width = c.reverse ? c.most : cut;  // (from the right the last matches cut: all of them are needed)
  c.ntokens = cut + 1;
}
// Step 2: the first `width` match spans of every row -- the stream kernel on its tiles (packed while the token columns
// fit one launch of the packed writer), else a thread a row.
void splitre_match_spans(SplitReCall& c) {
  Buf unused = dev_alloc(8, c.r.s);
  const bool stream = use_tdfa(c.r.re) && !cs::cfg("CS_REGEX_ROWWISE") && findall_stream(c.r, unused, c.matches, c.width, kMaxGroups - 1) >= 0;
  if (!stream) c.pl = findall_rowwise(c.r, c.width, c.matches);
  CS_HIP(hipGetLastError());
  note_route(c.matches.packed ? "splitre-packed" : stream ? "splitre-stream" : "splitre-rowwise");
}
// Step 3: token spans, in the layout of the match spans.
void splitre_token_spans(SplitReCall& c) {
  const hipStream_t s = c.r.s;
  const int64_t rows = c.r.col->rows;
  c.tokens.alloc(rows, c.ntokens, c.matches.packed, s);
  c.tokens.cap = c.matches.cap;
  TokenSpanArgs a{};
  a.in = view_of(c.r.col);
  a.counts = ptr<const int32_t>(c.counts);
  a.maxsplit = c.maxsplit;
  a.reverse = c.reverse ? 1 : 0;
  a.mwidth = c.width;
  a.ncols = c.ntokens;
  a.mspans = ptr<const uint32_t>(c.matches.spans);
  a.mbegins = ptr<const int32_t>(c.matches.begins);
  a.mlens = ptr<const int32_t>(c.matches.lens);
  a.tspans = ptr<uint32_t>(c.tokens.spans);
  a.tile_tot = ptr<int32_t>(c.tokens.tile_tot);
  a.tbegins = ptr<int32_t>(c.tokens.begins);
  a.tlens = ptr<int32_t>(c.tokens.lens);
  a.nsub = (rows + 63) / 64;
  const unsigned grid = (unsigned)std::min<long long>((a.nsub + 3) / 4, 256 * 16);
  ProfScope ps("k_token_spans", s);
  if (c.matches.packed) hipLaunchKernelGGL(k_token_spans<true>, dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_token_spans<false>, dim3(grid), dim3(256), 0, s, a);
  CS_HIP(hipGetLastError());
}
// The whole route; step 4 is columns_from on the token spans.
void split_re_columns(const cs_column* col, const cs_regex* cre, int maxsplit, bool reverse, hipStream_t s,
                      std::vector<std::unique_ptr<cs_column>>& cols) {
  if (cre->empty_pattern) fail(CS_ERR_INVALID_ARG, "split_re: the pattern cannot be null or empty");
  if (csrx::min_match_chars(cre->prog) == 0) fail(CS_ERR_INVALID_ARG, "split_re: the pattern matches the empty string");
  if (col->rows == 0) {  // (as cs_split: one column of no rows)
    cols.emplace_back(make_all_null(0, s));
    return;
  }
  SplitReCall c{SpanRun{col, const_cast<cs_regex*>(cre), s}, maxsplit, reverse};
  splitre_count(c);
  if (c.most == 0) {  // no row is cut: the one column is the input's rows
    cols.emplace_back(share_column(col, s));
    return;
  }
  splitre_match_spans(c);
  splitre_token_spans(c);
  columns_from(col, c.ntokens, c.tokens, s, cols);
}
int split_re_entry(const cs_column* col, const cs_regex* cre, int maxsplit, bool reverse, cs_stream stream, cs_column*** out_cols, int* ncols_out) {
  return guard([&] {
    if (!col || !cre || !out_cols || !ncols_out) fail(CS_ERR_INVALID_ARG, "split_re: null argument");
    *out_cols = nullptr;
    *ncols_out = 0;
    require_device();
    std::vector<std::unique_ptr<cs_column>> cols;
    split_re_columns(col, cre, maxsplit, reverse, S(stream), cols);
    release_columns(cols, out_cols, ncols_out);
  });
}
// The record form: the columns above through the transposition of cs_records_from_columns(ragged = 1) -- a row's
// leading non-null columns are its tokens.
int split_record_re_entry(const cs_column* col, const cs_regex* cre, int maxsplit, bool reverse, int64_t* list_offsets, int on_device,
                          cs_stream stream, cs_column** out) {
  int transposed = CS_OK;
  const int made = guard([&] {
    if (!col || !cre || !out || !list_offsets) fail(CS_ERR_INVALID_ARG, "split_record_re: null argument");
    *out = nullptr;
    require_device();
    std::vector<std::unique_ptr<cs_column>> cols;
    split_re_columns(col, cre, maxsplit, reverse, S(stream), cols);
    std::vector<const cs_column*> view;
    for (const auto& c : cols) view.push_back(c.get());
    transposed = cs_records_from_columns(view.data(), (int)view.size(), 1, list_offsets, on_device, stream, out);
  });
  return made != CS_OK ? made : transposed;
}

}  // namespace

extern "C" {

// split_re / rsplit_re and their record forms (no member of the reference: DESIGN.md section 4l; splitre_ops.h).
int cs_split_re(const cs_column* col, const cs_regex* re, int maxsplit, cs_stream stream, cs_column*** out_cols, int* ncols) {
  return split_re_entry(col, re, maxsplit, false, stream, out_cols, ncols);
}
int cs_rsplit_re(const cs_column* col, const cs_regex* re, int maxsplit, cs_stream stream, cs_column*** out_cols, int* ncols) {
  return split_re_entry(col, re, maxsplit, true, stream, out_cols, ncols);
}
int cs_split_record_re(const cs_column* col, const cs_regex* re, int maxsplit, int64_t* list_offsets, int on_device, cs_stream stream,
                       cs_column** out) {
  return split_record_re_entry(col, re, maxsplit, false, list_offsets, on_device, stream, out);
}
int cs_rsplit_record_re(const cs_column* col, const cs_regex* re, int maxsplit, int64_t* list_offsets, int on_device, cs_stream stream,
                        cs_column** out) {
  return split_record_re_entry(col, re, maxsplit, true, list_offsets, on_device, stream, out);
}

// NVStrings::extract(pattern, results) (NVStrings.h:682; extract.cu:69-151): one column per
// capture group; a pattern without groups, or an empty column, yields no columns.
int cs_extract(const cs_column* col, const cs_regex* cre, cs_stream stream, cs_column*** out_cols, int* ncols_out) {
  return guard([&] {
    if (!col || !cre || !out_cols || !ncols_out) fail(CS_ERR_INVALID_ARG, "null argument");
    require_device();
    SpanRun r{col, const_cast<cs_regex*>(cre), S(stream)};
    *out_cols = nullptr;
    *ncols_out = 0;
    const int groups = r.re->prog.num_groups;
    if (groups <= 0 || col->rows == 0) return;
    if (groups > kMaxGroups) fail(CS_ERR_RANGE, "extract: more than 32 capture groups");
    upload(r.re, r.s);
    const bool dfa_groups = use_tdfa(r.re) && r.re->d_gtags && !cs::cfg("CS_EXTRACT_LISTS");
    Buf arena;  // (extract_rowwise)
    SpanBufs sp;
    if (!(dfa_groups && !cs::cfg("CS_REGEX_ROWWISE") && extract_stream(r, groups, sp))) extract_rowwise(r, groups, dfa_groups, arena, sp);
    CS_HIP(hipGetLastError());
    std::vector<std::unique_ptr<cs_column>> cols;
    columns_from(col, groups, sp, r.s, cols);
    release_columns(cols, out_cols, ncols_out);
  });
}

// NVStrings::findall(pattern, results) (NVStrings.h:943; findall.cu:99-179): column k holds each
// row's k-th match (null where the row has fewer); no match in any row -> one all-null column.
int cs_findall(const cs_column* col, const cs_regex* cre, cs_stream stream, cs_column*** out_cols, int* ncols_out) {
  return guard([&] {
    if (!col || !cre || !out_cols || !ncols_out) fail(CS_ERR_INVALID_ARG, "null argument");
    require_device();
    SpanRun r{col, const_cast<cs_regex*>(cre), S(stream)};
    *out_cols = nullptr;
    *ncols_out = 0;
    if (col->rows == 0) return;
    std::vector<std::unique_ptr<cs_column>> cols;
    Buf dmax = dev_alloc(8, r.s);  // (read_max)
    SpanBufs sp;
    Plan pl{};  // (findall_rowwise)
    int ncols = use_tdfa(r.re) && !cs::cfg("CS_REGEX_ROWWISE") ? findall_stream(r, dmax, sp) : -1;
    const bool streamed = ncols >= 0;
    if (!streamed) ncols = findall_count_rows(r, dmax);
    if (ncols == 0) {  // findall.cu:149-151
      cols.emplace_back(make_all_null(col->rows, r.s));
      release_columns(cols, out_cols, ncols_out);
      return;
    }
    if (!streamed) pl = findall_rowwise(r, ncols, sp);
    CS_HIP(hipGetLastError());
    columns_from(col, ncols, sp, r.s, cols);
    release_columns(cols, out_cols, ncols_out);
  });
}

// NVStrings::replace_with_backrefs(pattern, repl) (NVStrings.h:788; replace_backref.cu:128-207).
// repl NULL -> a column of all nulls, as the reference returns.  A pattern that can match the empty
// string is refused (CS_ERR_INVALID_ARG): the reference does not terminate on it (replace_backref.cu:112).
int cs_replace_with_backrefs(const cs_column* col, const cs_regex* cre, const char* repl, cs_stream stream, cs_column** out) {
  return guard([&] {
    if (!col || !cre || !out) fail(CS_ERR_INVALID_ARG, "null argument");
    require_device();
    hipStream_t s = S(stream);
    cs_regex* re = const_cast<cs_regex*>(cre);
    if (re->empty_pattern) fail(CS_ERR_INVALID_ARG, "nvstrings::replace_with_backrefs parameter cannot be null or empty");
    if (col->rows == 0 || !repl) {
      *out = make_all_null(col->rows, s);
      return;
    }
    BackrefTemplateText tt = parse_backref_template(repl, re);
    upload(re, s);
    const bool dfa = use_tdfa(re) && (re->d_gtags || re->prog.num_groups == 0);
    if (csrx::min_match_chars(re->prog) == 0) fail(CS_ERR_INVALID_ARG, "replace_with_backrefs: the pattern matches the empty string");
    Buf d_text = dev_alloc(tt.text.size() + 1, s);
    CS_HIP(hipMemcpyAsync(d_text->p, tt.text.c_str(), tt.text.size() + 1, hipMemcpyHostToDevice, s));
    tt.t.text = ptr<const uint8_t>(d_text);
    if (backrefs_single_pass(col, re, tt.t, dfa, s, out)) return;
    *out = backrefs_two_pass(col, re, tt.t, dfa, s);
  });
}

// NVStrings::replace_re(patterns, repls) (NVStrings.h:777; replace_multi.cu:110-189)
int cs_replace_re_multi(const cs_column* col, const cs_regex* const* res, int npatterns, const cs_column* repls, cs_stream stream,
                        cs_column** out) {
  return guard([&] {
    if (!col || !out) fail(CS_ERR_INVALID_ARG, "null argument");
    if (npatterns <= 0 || !res || !repls || repls->rows == 0)
      fail(CS_ERR_INVALID_ARG, "replace_re patterns and repls parameters cannot be empty");
    if (repls->rows > 1 && repls->rows != npatterns)
      fail(CS_ERR_INVALID_ARG, "replace_re patterns and repls must have the same number of strings");
    require_device();
    hipStream_t s = S(stream);
    const int64_t rows = col->rows;
    if (rows == 0) {
      *out = make_all_null(0, s);
      return;
    }
    std::vector<MultiProg> progs;
    bool all_dfa = !cs::cfg("CS_REGEX_NO_TDFA");
    int max_inst = 0;
    for (int i = 0; i < npatterns; ++i) {
      cs_regex* re = const_cast<cs_regex*>(res[i]);
      if (!re || re->empty_pattern) continue;  // (a null pattern is skipped, replace_multi.cu:125-127)
      upload(re, s);
      if (csrx::min_match_chars(re->prog) == 0) fail(CS_ERR_INVALID_ARG, "replace_re: a pattern matches the empty string");
      MultiProg mp{};
      mp.tdfa = ptr<const int32_t>(re->d_tdfa);
      mp.image = ptr<const int32_t>(re->d_image);
      for (int k = 0; k < 4; ++k) mp.first[k] = 0xFFFFFFFFu;
      if (!re->tdfa.empty() && re->tdfa[16] > 0)  // idle states exist: the candidate bitmap says which bytes leave them
        for (int k = 0; k < 4; ++k) mp.first[k] = (uint32_t)re->tdfa[21 + k];
      all_dfa = all_dfa && use_tdfa(re);  // (a program of more than four threads takes the list simulator here)
      max_inst = std::max(max_inst, (int)re->prog.insts.size());
      progs.push_back(mp);
      if (repls->rows > 1 && (int)progs.size() - 1 != i) fail(CS_ERR_INVALID_ARG, "replace_re: a null pattern among several replacements");
    }
    if (progs.empty()) fail(CS_ERR_INVALID_ARG, "replace_re invalid patterns");
    Buf d_progs = dev_alloc(sizeof(MultiProg) * progs.size(), s);
    CS_HIP(hipMemcpyAsync(d_progs->p, progs.data(), sizeof(MultiProg) * progs.size(), hipMemcpyHostToDevice, s));
    MultiArgs a{};
    a.src = RowSrc{view_of(col), d_unicode_flags(), col->nbytes};
    a.progs = ptr<const MultiProg>(d_progs);
    a.nprogs = (int)progs.size();
    a.repls = view_of(repls);
    unsigned grid = (unsigned)std::min<int64_t>((rows + 255) / 256, 256 * 8);
    Buf arena;
    if (!all_dfa) {
      a.slots = 6 * max_inst + (max_inst + 31) / 32 + 2;
      grid = std::min(grid, 1024u);
      arena = dev_alloc((size_t)grid * 256 * a.slots * 4, s);
      a.arena = ptr<uint32_t>(arena);
    }
    Buf bad = dev_alloc(sizeof(unsigned), s);
    CS_HIP(hipMemsetAsync(bad->p, 0, sizeof(unsigned), s));
    Buf lens = dev_alloc(sizeof(int32_t) * rows, s);
    if (all_dfa) hipLaunchKernelGGL((k_multi_replace<true, false>), dim3(grid), dim3(256), 0, s, a, ptr<int32_t>(lens), (const int64_t*)nullptr, (uint8_t*)nullptr, ptr<unsigned>(bad));
    else hipLaunchKernelGGL((k_multi_replace<false, false>), dim3(grid), dim3(256), 0, s, a, ptr<int32_t>(lens), (const int64_t*)nullptr, (uint8_t*)nullptr, ptr<unsigned>(bad));
    CS_HIP(hipGetLastError());
    Built b(col, s);
    b.scan(ptr<int32_t>(lens));
    unsigned* hb = (unsigned*)pinned_scratch(sizeof(unsigned));
    CS_HIP(hipMemcpyAsync(hb, bad->p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    if (*hb) fail(CS_ERR_INVALID_ARG, "replace_re: a pattern matched the empty string");
    b.alloc_chars();
    if (all_dfa) hipLaunchKernelGGL((k_multi_replace<true, true>), dim3(grid), dim3(256), 0, s, a, (int32_t*)nullptr, b.off, b.chars, ptr<unsigned>(bad));
    else hipLaunchKernelGGL((k_multi_replace<false, true>), dim3(grid), dim3(256), 0, s, a, (int32_t*)nullptr, b.off, b.chars, ptr<unsigned>(bad));
    CS_HIP(hipGetLastError());
    CS_HIP(hipStreamSynchronize(s));
    *out = b.col.release();
  });
}

}  // extern "C"
