// Substring, padding and wrapping ops (reference: cpp/src/strings/substr.cu, pad.cu, modify.cu slice_replace / insert).
// The per-row logic is pad_ops.h, shared with the CPU harness of tests/test_pad_cpu.py: a row becomes at most four pieces
// (fill, a source range, an insert, a source range), repeated for repeat; a strided slice walks a source range; wrap
// keeps the row's extents.
//
// Every op but wrap is a size pass, a scan (offsets_from_lengths) and a write pass.  Two routes, both templated on the op:
//  - tile: a wave stages R consecutive rows in LDS (cstile::RowTileWalk).  The size pass maps its rows to one int32 each
//    out of LDS; the write pass assembles the R output rows in an LDS out-tile from their pieces and the tile leaves with
//    16-byte stores (cstile::wave_flush_shift).  A tile whose input bytes or output bytes exceed the staging sizes takes
//    the from-memory path of k_strip_tile: a short row by its lane, a long one by the whole wave (a byte a lane).
//  - rows: a thread per row from memory (CS_PAD_ROWWISE=1, and columns the tile plan refuses).
// wrap changes no length: the output shares the input's extents and only the write pass runs.
// An output row of 2^31 bytes or more is CS_ERR_RANGE (the reference's unsigned size would wrap); the offsets are int64.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "cs_internal.h"
#include "device_utils.h"
#include "pad_ops.h"
#include "tile_utils.h"

using namespace cs;
using namespace csdev;
using cspad::Params;
using cspad::Pieces;

namespace {

constexpr int kOutCapMax = 16 * 1024;  // LDS out-tile per wave at most (tiles beyond it take the from-memory path)
constexpr int kWaveRow = 256;          // output rows longer than this are written by the whole wave (from-memory path)

struct PadArgs {
  ColView in;
  Params P;
  const int32_t* starts;  // slice_from: per-row start / stop (nullptr: 0 / -1)
  const int32_t* stops;
  int32_t* lens;             // size pass
  unsigned* overflow;        // size pass: set when a row reaches 2^31 bytes
  const int64_t* out_off;    // write pass
  uint8_t* out_chars;
  int rows_per_tile, cap, out_cap;
  long long ntiles;
};

template <int OP>
__device__ __forceinline__ Params params_of(const PadArgs& a) {
  Params P = a.P;
  P.op = OP;  // (a compile-time op: the other ops' branches fold away)
  return P;
}
__device__ __forceinline__ int row_start(const PadArgs& a, int64_t r) { return a.starts ? a.starts[r] : a.P.start; }
__device__ __forceinline__ int row_stop(const PadArgs& a, int64_t r) { return a.stops ? a.stops[r] : a.P.stop; }

__device__ __forceinline__ int32_t size_or_flag(const PadArgs& a, int64_t sz) {
  if (sz >= ((int64_t)1 << 31)) {
    atomicOr(a.overflow, 1u);
    return 0;
  }
  return (int32_t)sz;
}

// ---- size pass ---------------------------------------------------------------------------------------------------------
// the size of row r, its n bytes at p (memory or LDS); -1 for a null row
__device__ __forceinline__ void size_row(const PadArgs& a, const Params& P, int64_t r, const uint8_t* p, int n, bool valid) {
  int32_t len = -1;
  if (valid) {
    const Pieces pc = cspad::plan_row(P, p, n, row_start(a, r), row_stop(a, r));
    len = size_or_flag(a, cspad::out_size(P, pc, p));
  }
  a.lens[r] = len;
}

template <int OP>
__global__ void __launch_bounds__(256) k_pad_size_rows(PadArgs a) {
  const Params P = params_of<OP>(a);
  for_each_row(a.in, [&](int64_t r, const uint8_t* p, int n, bool valid) { size_row(a, P, r, p, n, valid); });
}

template <int OP>
__global__ void __launch_bounds__(256) k_pad_size_tile(PadArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint8_t* lds_in = reinterpret_cast<uint8_t*>(smem) + (size_t)wv * a.cap;
  const Params P = params_of<OP>(a);
  // (a tile beyond the staging buffer -- a long row among short ones -- is read from memory)
  cstile::walk_staged_tiles<cstile::Oversize::kFromMemory>(a.in, a.rows_per_tile, a.ntiles, lds_in, a.cap, wv, lane,
                                                           [&](const cstile::RowTile& cur, const uint8_t* p) {
    if (cur.in_tile) size_row(a, P, cur.r0 + lane, p, cur.n, cur.live);
  });
}

// ---- write pass --------------------------------------------------------------------------------------------------------
template <int OP>
__global__ void __launch_bounds__(256) k_pad_write_rows(PadArgs a) {
  const Params P = params_of<OP>(a);
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < a.in.rows; r += (int64_t)gridDim.x * kBlock) {
    if (!row_is_valid(a.in.validity, r)) continue;
    const int64_t o0 = a.in.offsets[r];
    const uint8_t* p = a.in.chars + o0;
    const int n = (int)(a.in.offsets[r + 1] - o0);
    const Pieces pc = cspad::plan_row(P, p, n, row_start(a, r), row_stop(a, r));
    cspad::write_row(P, pc, p, n, a.out_chars + a.out_off[r]);
  }
}

// k fill characters to LDS at dbase[di ..): 16-byte stores for a one-byte character
__device__ __forceinline__ void lds_fill(uint8_t* dbase, int di, const Params& P, int64_t k) {
  if (P.fillw == 1) {
    const uint32_t w = (P.fill & 0xFFu) * 0x01010101u;
    const cstile::lds_u32x4u v = {w, w, w, w};
    int i = 0;
    for (; i + 16 <= (int)k; i += 16) *reinterpret_cast<cstile::lds_u32x4u*>(dbase + di + i) = v;
    if (i < (int)k) cstile::lds_put16(dbase + di + i, v, (int)k - i);
    return;
  }
  for (int64_t i = 0; i < k; ++i)
    for (int b = 0; b < P.fillw; ++b) dbase[di++] = cspad::fill_byte(P, b);
}

// the pieces of a row staged at sbase[si ..) to dbase[di ..)
__device__ __forceinline__ void lds_pieces(uint8_t* dbase, int di, const uint8_t* sbase, int si, const Params& P, const Pieces& pc) {
  for (int64_t r = 0; r < pc.reps; ++r) {
    lds_fill(dbase, di, P, pc.pre);
    di += (int)(pc.pre * P.fillw);
    cstile::lds_copy(dbase, di, sbase, si + pc.a0, pc.a1 - pc.a0);
    di += pc.a1 - pc.a0;
    if (pc.repl) {
      for (int i = 0; i < P.replen; ++i) dbase[di + i] = P.repl[i];
      di += P.replen;
    } else {
      lds_fill(dbase, di, P, pc.fill);
      di += (int)(pc.fill * P.fillw);
    }
    cstile::lds_copy(dbase, di, sbase, si + pc.b0, pc.b1 - pc.b0);
    di += pc.b1 - pc.b0;
  }
}

__device__ __forceinline__ Pieces read_pieces(const Pieces& pc, int l) {
  Pieces q;
  q.pre = cstile::rl64(pc.pre, l);
  q.a0 = __builtin_amdgcn_readlane(pc.a0, l);
  q.a1 = __builtin_amdgcn_readlane(pc.a1, l);
  q.fill = cstile::rl64(pc.fill, l);
  q.repl = __builtin_amdgcn_readlane((int)pc.repl, l) != 0;
  q.b0 = __builtin_amdgcn_readlane(pc.b0, l);
  q.b1 = __builtin_amdgcn_readlane(pc.b1, l);
  q.reps = cstile::rl64(pc.reps, l);
  q.stride = 1;
  return q;
}

template <int OP>
__global__ void __launch_bounds__(256) k_pad_write_tile(PadArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint8_t* lds_in = reinterpret_cast<uint8_t*>(smem) + (size_t)wv * (a.cap + a.out_cap);
  uint8_t* lds_out = lds_in + a.cap;
  const Params P = params_of<OP>(a);
  const ColView& in = a.in;
  cstile::RowTileWalk walk(in, a.rows_per_tile, a.ntiles, wv, lane);
  if (walk.done()) return;
  for (;;) {
    const cstile::RowTile cur = walk.current();
    const long long r0 = cur.r0, g0 = cur.g0;
    const int nrows = cur.nrows, rbeg = cur.rbeg, n = cur.n, lead = cur.lead;
    const bool live = cur.live;
    const long long oo0 = a.out_off[r0 + min(lane, nrows)];
    const long long oo1 = a.out_off[r0 + min(lane + 1, nrows)];
    const long long ob = cstile::rl64(oo0, 0), oe = cstile::rl64(oo1, 63);
    const long long want64 = cur.g1 - g0 + lead;
    const bool oversize = want64 + 48 > a.cap || oe - ob + 16 > a.out_cap;
    cstile::stage_chars(lds_in, oversize ? 0 : (int)want64, lane, walk.pf);
    const int64_t r = r0 + lane;
    const int st = cur.in_tile ? row_start(a, r) : 0, sp = cur.in_tile ? row_stop(a, r) : 0;
    const bool has_next = walk.advance();
    cstile::wave_lds_fence();
    if (oversize) {
      // straight from memory: a short row by its lane, a long one by the whole wave (a byte a lane)
      const uint8_t* p = in.chars + (g0 + rbeg);
      uint8_t* o = a.out_chars + oo0;
      Pieces pc{};
      if (live) pc = cspad::plan_row(P, p, n, st, sp);
      const long long len = live ? oo1 - oo0 : 0;
      const bool by_wave = len > kWaveRow && OP != cspad::OP_WRAP && pc.stride <= 1;
      if (live && !by_wave) cspad::write_row(P, pc, p, n, o);
      for (unsigned long long m = __ballot(by_wave); m; m &= m - 1) {
        const int l = __builtin_ctzll(m);
        const Pieces q = read_pieces(pc, l);
        const uint8_t* lp = in.chars + cstile::rl64(g0 + rbeg, l);
        uint8_t* lo = a.out_chars + cstile::rl64(oo0, l);
        const long long L = cstile::rl64(len, l);
        const int64_t per = cspad::period_bytes(P, q);
        for (long long j = lane; j < L; j += 64) lo[j] = cspad::period_byte(P, q, lp, j % per);
      }
      if (!has_next) break;
      continue;
    }
    if (live) {
      const int di = (int)(oo0 - ob), si = lead + rbeg;
      const uint8_t* p = lds_in + si;
      if constexpr (OP == cspad::OP_WRAP) {
        cstile::lds_copy(lds_out, di, lds_in, si, n);
        cspad::wrap_row(p, n, P.width, lds_out + di);
      } else {
        const Pieces pc = cspad::plan_row(P, p, n, st, sp);
        if (pc.stride > 1) cspad::write_strided(pc, p, lds_out + di);
        else lds_pieces(lds_out, di, lds_in, si, P, pc);
      }
    }
    cstile::wave_lds_fence();
    cstile::wave_flush_shift(a.out_chars + ob, (int)(oe - ob), lds_out, lane);
    cstile::wave_lds_fence();
    if (!has_next) break;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------
template <int OP>
cs_column* run_pad_op(const cs_column* col, PadArgs a, hipStream_t s) {
  const int64_t rows = col->rows;
  Built b(col, s);
  cs_column* const o = b.col.get();
  a.in = view_of(col);
  // the tile plan: R rows whose bytes fit the prefetch (a column with a few longer tiles still gets it: those tiles go from
  // memory); the staging buffers of four waves must fit the LDS
  StagedTiles t;
  if (!cs::cfg("CS_PAD_ROWWISE")) t = plan_staged_tiles(col, cstile::kStageSlack, true, {1, 0, 100 * 1024}, s);
  const bool tile = t.R != 0;
  a.rows_per_tile = t.R;
  a.cap = t.cap;
  a.ntiles = t.ntiles;
  const unsigned row_grid = std::min(blocks_for(rows), 65536u);
  if (OP == cspad::OP_WRAP) {
    col->share_extents_with(o, s);
    o->nbytes = col->nbytes;
    o->max_row = col->max_row;
    o->max_span64 = col->max_span64;
  } else {
    Buf lens = dev_alloc(sizeof(int32_t) * (size_t)rows, s);
    Buf flag = dev_alloc(sizeof(unsigned), s);
    CS_HIP(hipMemsetAsync(flag->p, 0, sizeof(unsigned), s));
    a.lens = ptr<int32_t>(lens);
    a.overflow = ptr<unsigned>(flag);
    {
      ProfScope ps("k_pad_size", s);
      // (repeat's sizes need the offsets only: staging its bytes made the tile form 5x slower than the row-wise one)
      if (tile && OP != cspad::OP_REPEAT) {
        launch_resident(&k_pad_size_tile<OP>, t.lds, t.grid, s, a);
      } else {
        hipLaunchKernelGGL(k_pad_size_rows<OP>, dim3(row_grid), dim3(kBlock), 0, s, a);
        CS_HIP(hipGetLastError());
      }
    }
    b.scan(ptr<int32_t>(lens));
    unsigned over = 0;
    CS_HIP(hipMemcpy(&over, flag->p, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (over) fail(CS_ERR_RANGE, "nvstrings: an output row would reach 2^31 bytes");
  }
  a.out_chars = b.alloc_chars();
  a.out_off = o->d_offsets();  // (wrap: the input's extents)
  {
    ProfScope ps("k_pad_write", s);
    if (tile) {
      // the out-tile: the widest 64-row span of the output (an R-row tile lies inside one), capped
      const int64_t span = o->max_span64 >= 0 ? o->max_span64 : max_span64(o, s);
      a.out_cap = (int)((std::min<int64_t>(span, kOutCapMax) + 16 + 15) & ~(int64_t)15);
      launch_resident(&k_pad_write_tile<OP>, t.lds + (size_t)a.out_cap * 4, t.grid, s, a);
    } else {
      hipLaunchKernelGGL(k_pad_write_rows<OP>, dim3(row_grid), dim3(kBlock), 0, s, a);
      CS_HIP(hipGetLastError());
    }
  }
  note_route(tile ? "tile" : "rows");
  return b.col.release();
}

cs_column* run_pad(const cs_column* col, const Params& P, const int32_t* starts, const int32_t* stops, hipStream_t s) {
  if (col->rows == 0) return make_all_null(0, s);
  PadArgs a{};
  a.P = P;
  a.starts = starts;
  a.stops = stops;
  switch (P.op) {
    case cspad::OP_SLICE: return run_pad_op<cspad::OP_SLICE>(col, a, s);
    case cspad::OP_SLICE_REPLACE: return run_pad_op<cspad::OP_SLICE_REPLACE>(col, a, s);
    case cspad::OP_INSERT: return run_pad_op<cspad::OP_INSERT>(col, a, s);
    case cspad::OP_REPEAT: return run_pad_op<cspad::OP_REPEAT>(col, a, s);
    case cspad::OP_RJUST: return run_pad_op<cspad::OP_RJUST>(col, a, s);
    case cspad::OP_LJUST: return run_pad_op<cspad::OP_LJUST>(col, a, s);
    case cspad::OP_CENTER: return run_pad_op<cspad::OP_CENTER>(col, a, s);
    case cspad::OP_ZFILL: return run_pad_op<cspad::OP_ZFILL>(col, a, s);
    default: return run_pad_op<cspad::OP_WRAP>(col, a, s);
  }
}

Params base_params(int op) {
  Params P{};
  P.op = op;
  P.stop = -1;
  P.step = 1;
  P.fill = ' ';
  P.fillw = 1;
  return P;
}

// the replacement of slice_replace / insert in device memory; null is CS_ERR_INVALID_ARG (std::invalid_argument)
Buf put_repl(Params& P, const char* repl, const char* what, hipStream_t s) {
  if (!repl) fail(CS_ERR_INVALID_ARG, std::string("nvstrings::") + what + " parameter cannot be null");
  P.replen = (int)strlen(repl);
  Buf d = dev_alloc((size_t)P.replen + 1, s);
  CS_HIP(hipMemcpyAsync(d->p, repl, (size_t)P.replen + 1, hipMemcpyHostToDevice, s));
  P.repl = ptr<const uint8_t>(d);
  return d;
}

template <class F>
int pad_entry(const cs_column* col, cs_column** out, F&& f) {
  return guard([&] {
    if (!col || !out) fail(CS_ERR_INVALID_ARG, "null column or output");
    *out = nullptr;
    require_device();
    *out = f();
  });
}

}  // namespace

extern "C" {

int cs_slice(const cs_column* col, int start, int stop, int step, cs_stream stream, cs_column** out) {
  return pad_entry(col, out, [&] {
    if (stop > 0 && start > stop) fail(CS_ERR_INVALID_ARG, "nvstrings::slice start cannot be greater than stop");
    Params P = base_params(cspad::OP_SLICE);
    P.start = start;
    P.stop = stop;
    P.step = (unsigned)step;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

int cs_slice_from(const cs_column* col, const int32_t* starts, const int32_t* stops, int on_device, cs_stream stream,
                  cs_column** out) {
  return pad_entry(col, out, [&] {
    hipStream_t s = S(stream);
    Params P = base_params(cspad::OP_SLICE);
    Buf ds, de;
    const size_t bytes = sizeof(int32_t) * (size_t)col->rows;
    if (!on_device && col->rows > 0) {
      if (starts) {
        ds = dev_alloc(bytes, s);
        CS_HIP(hipMemcpyAsync(ds->p, starts, bytes, hipMemcpyHostToDevice, s));
        starts = ptr<const int32_t>(ds);
      }
      if (stops) {
        de = dev_alloc(bytes, s);
        CS_HIP(hipMemcpyAsync(de->p, stops, bytes, hipMemcpyHostToDevice, s));
        stops = ptr<const int32_t>(de);
      }
    }
    cs_column* c = run_pad(col, P, starts, stops, s);
    CS_HIP(hipStreamSynchronize(s));  // (the caller's arrays are done with)
    return c;
  });
}

int cs_slice_replace(const cs_column* col, const char* repl, int start, int stop, cs_stream stream, cs_column** out) {
  return pad_entry(col, out, [&] {
    Params P = base_params(cspad::OP_SLICE_REPLACE);
    Buf keep = put_repl(P, repl, "slice_replace", S(stream));
    P.start = start;
    P.stop = stop;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

int cs_insert(const cs_column* col, const char* repl, int start, cs_stream stream, cs_column** out) {
  return pad_entry(col, out, [&] {
    Params P = base_params(cspad::OP_INSERT);
    Buf keep = put_repl(P, repl, "insert", S(stream));
    P.start = start;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

int cs_repeat(const cs_column* col, unsigned count, cs_stream stream, cs_column** out) {
  return pad_entry(col, out, [&] {
    Params P = base_params(cspad::OP_REPEAT);
    P.reps = count;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

int cs_pad(const cs_column* col, unsigned width, int side, const char* fillchar, cs_stream stream, cs_column** out) {
  return pad_entry(col, out, [&] {
    if (side < 0 || side > 2) fail(CS_ERR_INVALID_ARG, "pad: side must be 0 (left), 1 (right) or 2 (both)");
    static const int ops[3] = {cspad::OP_RJUST, cspad::OP_LJUST, cspad::OP_CENTER};
    Params P = base_params(ops[side]);
    cspad::set_fill(P, fillchar);
    P.width = width;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

int cs_zfill(const cs_column* col, unsigned width, cs_stream stream, cs_column** out) {
  return pad_entry(col, out, [&] {
    Params P = base_params(cspad::OP_ZFILL);
    P.fill = '0';
    P.width = width;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

int cs_wrap(const cs_column* col, unsigned width, cs_stream stream, cs_column** out) {
  return pad_entry(col, out, [&] {
    Params P = base_params(cspad::OP_WRAP);
    P.width = width;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

}  // extern "C"
