// Substring, padding and wrapping ops (reference: cpp/src/strings/substr.cu, pad.cu, modify.cu slice_replace / insert).
// The per-row logic is pad_ops.h, shared with the CPU harness of tests/test_pad_cpu.py: a row becomes at most four pieces
// (fill, a source range, an insert, a source range), repeated for repeat; a strided slice walks a source range; wrap
// keeps the row's extents.
//
// The ops run on the sized route (sized_route.h: size pass, scan, write pass; tile and rows, CS_PAD_ROWWISE=1), as PadOp<OP>.
// What is pad's own on it: the tile's write body assembles the R output rows in the LDS out-tile from their pieces with
// 16-byte accesses, and a tile whose input or output exceeds the staging sizes takes the from-memory path of
// k_strip_tile: a short row by its lane, a long one by the whole wave (a byte a lane).
// wrap changes no length: the output shares the input's extents and only the write pass runs.
// An output row of 2^31 bytes or more is CS_ERR_RANGE (the reference's unsigned size would wrap).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "cs_internal.h"
#include "device_utils.h"
#include "pad_ops.h"
#include "sized_route.h"
#include "tile_utils.h"

using namespace cs;
using namespace csdev;
using cspad::Params;
using cspad::Pieces;

namespace {

constexpr int kWaveRow = 256;  // output rows longer than this are written by the whole wave (from-memory path)

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
struct PadOp {
  Params P;
  const int32_t* starts;  // slice_from: per-row start / stop (nullptr: P's)
  const int32_t* stops;
  static constexpr bool kSizeFromOffsets = OP == cspad::OP_REPEAT;

  __device__ __forceinline__ Params params() const {
    Params q = P;
    q.op = OP;  // (a compile-time op: the other ops' branches fold away)
    return q;
  }
  __device__ __forceinline__ Pieces plan(const Params& q, int64_t r, const uint8_t* p, int n) const {
    return cspad::plan_row(q, p, n, starts ? starts[r] : P.start, stops ? stops[r] : P.stop);
  }
  __device__ __forceinline__ int64_t size(int64_t r, const uint8_t* p, int n) const {
    const Params q = params();
    return cspad::out_size(q, plan(q, r, p, n), p);
  }
  __device__ __forceinline__ void write(int64_t r, const uint8_t* p, int n, uint8_t* o) const {
    const Params q = params();
    cspad::write_row(q, plan(q, r, p, n), p, n, o);
  }
  __device__ __forceinline__ void write_tile(const cssized::TileWrite& w) const {
    const Params q = params();
    const cstile::RowTile& cur = w.cur;
    const int n = cur.n, lane = w.lane;
    if (!w.out.staged) {
      // straight from memory: a short row by its lane, a long one by the whole wave (a byte a lane)
      const uint8_t* p = w.chars + (cur.g0 + cur.rbeg);
      Pieces pc{};
      if (cur.live) pc = plan(q, cur.r0 + lane, p, n);
      const long long len = cur.live ? w.out.oo1 - w.out.oo0 : 0;
      const bool by_wave = len > kWaveRow && OP != cspad::OP_WRAP && pc.stride <= 1;
      if (cur.live && !by_wave) cspad::write_row(q, pc, p, n, w.out_chars + w.out.oo0);
      for (unsigned long long m = __ballot(by_wave); m; m &= m - 1) {
        const int l = __builtin_ctzll(m);
        const Pieces ql = read_pieces(pc, l);
        const uint8_t* lp = w.chars + cstile::rl64(cur.g0 + cur.rbeg, l);
        uint8_t* lo = w.out_chars + cstile::rl64(w.out.oo0, l);
        const long long L = cstile::rl64(len, l);
        const int64_t per = cspad::period_bytes(q, ql);
        for (long long j = lane; j < L; j += 64) lo[j] = cspad::period_byte(q, ql, lp, j % per);
      }
      return;
    }
    if (!cur.live) return;
    const int di = (int)(w.out.oo0 - w.out.ob), si = cur.lead + cur.rbeg;
    const uint8_t* p = w.lds_in + si;
    if constexpr (OP == cspad::OP_WRAP) {
      cstile::lds_copy(w.lds_out, di, w.lds_in, si, n);
      cspad::wrap_row(p, n, q.width, w.lds_out + di);
    } else {
      const Pieces pc = plan(q, cur.r0 + lane, p, n);
      if (pc.stride > 1) cspad::write_strided(pc, p, w.lds_out + di);
      else lds_pieces(w.lds_out, di, w.lds_in, si, q, pc);
    }
  }
};

// ---- host ----------------------------------------------------------------------------------------------------------------
template <int OP>
cs_column* run_pad_op(const cs_column* col, const Params& P, const int32_t* starts, const int32_t* stops, hipStream_t s) {
  const PadOp<OP> op{P, starts, stops};
  if constexpr (OP == cspad::OP_WRAP) return cssized::run_sized_in_place(col, op, "CS_PAD_ROWWISE", "k_pad_write", s);
  else return cssized::run_sized(col, op, "CS_PAD_ROWWISE", "k_pad_size", "k_pad_write", s);
}

cs_column* run_pad(const cs_column* col, const Params& P, const int32_t* starts, const int32_t* stops, hipStream_t s) {
  if (col->rows == 0) return make_all_null(0, s);
  switch (P.op) {
    case cspad::OP_SLICE: return run_pad_op<cspad::OP_SLICE>(col, P, starts, stops, s);
    case cspad::OP_SLICE_REPLACE: return run_pad_op<cspad::OP_SLICE_REPLACE>(col, P, starts, stops, s);
    case cspad::OP_INSERT: return run_pad_op<cspad::OP_INSERT>(col, P, starts, stops, s);
    case cspad::OP_REPEAT: return run_pad_op<cspad::OP_REPEAT>(col, P, starts, stops, s);
    case cspad::OP_RJUST: return run_pad_op<cspad::OP_RJUST>(col, P, starts, stops, s);
    case cspad::OP_LJUST: return run_pad_op<cspad::OP_LJUST>(col, P, starts, stops, s);
    case cspad::OP_CENTER: return run_pad_op<cspad::OP_CENTER>(col, P, starts, stops, s);
    case cspad::OP_ZFILL: return run_pad_op<cspad::OP_ZFILL>(col, P, starts, stops, s);
    default: return run_pad_op<cspad::OP_WRAP>(col, P, starts, stops, s);
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

}  // namespace

extern "C" {

int cs_slice(const cs_column* col, int start, int stop, int step, cs_stream stream, cs_column** out) {
  return column_entry(col, out, [&] {
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
  return column_entry(col, out, [&] {
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
  return column_entry(col, out, [&] {
    Params P = base_params(cspad::OP_SLICE_REPLACE);
    Buf keep = put_repl(P, repl, "slice_replace", S(stream));
    P.start = start;
    P.stop = stop;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

int cs_insert(const cs_column* col, const char* repl, int start, cs_stream stream, cs_column** out) {
  return column_entry(col, out, [&] {
    Params P = base_params(cspad::OP_INSERT);
    Buf keep = put_repl(P, repl, "insert", S(stream));
    P.start = start;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

int cs_repeat(const cs_column* col, unsigned count, cs_stream stream, cs_column** out) {
  return column_entry(col, out, [&] {
    Params P = base_params(cspad::OP_REPEAT);
    P.reps = count;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

int cs_pad(const cs_column* col, unsigned width, int side, const char* fillchar, cs_stream stream, cs_column** out) {
  return column_entry(col, out, [&] {
    if (side < 0 || side > 2) fail(CS_ERR_INVALID_ARG, "pad: side must be 0 (left), 1 (right) or 2 (both)");
    static const int ops[3] = {cspad::OP_RJUST, cspad::OP_LJUST, cspad::OP_CENTER};
    Params P = base_params(ops[side]);
    cspad::set_fill(P, fillchar);
    P.width = width;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

int cs_zfill(const cs_column* col, unsigned width, cs_stream stream, cs_column** out) {
  return column_entry(col, out, [&] {
    Params P = base_params(cspad::OP_ZFILL);
    P.fill = '0';
    P.width = width;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

int cs_wrap(const cs_column* col, unsigned width, cs_stream stream, cs_column** out) {
  return column_entry(col, out, [&] {
    Params P = base_params(cspad::OP_WRAP);
    P.width = width;
    return run_pad(col, P, nullptr, nullptr, S(stream));
  });
}

}  // extern "C"
