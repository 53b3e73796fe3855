// The sized route (string -> string of another length per row): a size pass, a scan (cs::Built) and a write pass.
// cs_pad.hip (slice ... zfill, wrap) and cs_recode.hip (url_encode, url_decode, translate) each instantiate it with a
// per-row op, in their own translation unit.  An op is a struct passed by value in the kernel arguments with its state
// (pad's Params, translate's table):
//   __device__ int64_t size(int64_t r, const uint8_t* p, int n) const;            // bytes of valid row r = [p, p + n)
//   __device__ void write(int64_t r, const uint8_t* p, int n, uint8_t* o) const;  // ... written to o[0, size)
// p and o may point to memory or to LDS.  A row of 2^31 bytes or more is CS_ERR_RANGE; the offsets are int64.
// Two routes, both passes on the same one:
//  - tile: a wave stages R consecutive rows in LDS (cstile::walk_staged_tiles).  The size pass maps its rows to one
//    int32 each out of LDS; the write pass has every lane write its row into an LDS out-tile and the tile leaves with
//    16-byte stores (cstile::wave_flush_shift).  A tile whose input exceeds the staging buffer is read from memory; a
//    tile whose OUTPUT exceeds the out-tile is written to memory by its lanes, from wherever its input is.
//  - rows: a thread per row from memory (the family's row-wise switch, and columns the tile plan refuses).
// An op may declare three more things:
//   static constexpr int kSharedBytes = <n>;         // LDS filled once per workgroup by `stage(lds, tid)` in front of the waves'
//                                                    // buffers; the tile route then calls size / write with it as a last
//                                                    // argument `shared` (the row-wise route the forms above): translate's
//                                                    // ASCII table
//   static constexpr bool kSizeFromOffsets = true;   // the size needs no bytes: the size pass is row-wise on the tile route
//                                                    // too (repeat: staging its bytes made the tile form 5x slower)
//   __device__ void write_tile(const TileWrite&) const;  // the tile's write body of its own in place of "a lane writes its
//                                                    // row": the rows to w.lds_out + (oo0 - ob) when w.out.staged, else to
//                                                    // memory.  Such a tile is staged only when its output fits the out-tile
//                                                    // as well, so the body's from-memory form finds input and output there
//                                                    // (pad: rows assembled from pieces in LDS; long rows by the whole wave)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "cs_internal.h"
#include "device_utils.h"
#include "tile_utils.h"

namespace cssized {

using cs::ColView;
using cstile::SharedBytes;

constexpr int kOutCapMax = 16 * 1024;  // LDS out-tile per wave at most (tiles beyond it leave through memory)

template <class Op, class = void>
struct SizeFromOffsets : std::false_type {};
template <class Op>
struct SizeFromOffsets<Op, std::void_t<decltype(Op::kSizeFromOffsets)>> : std::integral_constant<bool, Op::kSizeFromOffsets> {};
template <class Op, class = void>
struct OwnTileWrite : std::false_type {};
template <class Op>
struct OwnTileWrite<Op, std::void_t<decltype(&Op::write_tile)>> : std::true_type {};

template <class Op>
struct SizedArgs {
  ColView in;
  int32_t* lens;           // size pass
  unsigned* overflow;      // size pass: set when a row reaches 2^31 bytes
  const int64_t* out_off;  // write pass
  uint8_t* out_chars;
  int rows_per_tile, cap, out_cap;  // tile route
  long long ntiles;
  Op op;
};

// a tile's output, loaded in front of its staging
struct TileOut {
  long long oo0, oo1;  // the lane's row: out_chars[oo0, oo1) (lanes beyond the tile's rows repeat its end)
  long long ob, oe;    // the tile's rows: out_chars[ob, oe)
  bool fits;           // ... fit the out-tile
  bool staged;         // the tile's input is in LDS
};
// what an op's own write body gets
struct TileWrite {
  const cstile::RowTile& cur;
  const TileOut& out;
  uint8_t *lds_in, *lds_out;  // the wave's staging buffer (the lane's row at cur.lead + cur.rbeg when out.staged) and its out-tile
  const uint8_t* chars;       // the column's (the lane's row at cur.g0 + cur.rbeg)
  uint8_t* out_chars;
  int lane;
};

__device__ __forceinline__ int32_t size_or_flag(unsigned* overflow, int64_t sz) {
  if (sz >= ((int64_t)1 << 31)) {
    atomicOr(overflow, 1u);
    return 0;
  }
  return (int32_t)sz;
}
// the size of row r to lens[r]; -1 for a null row.  `shared`: the op's LDS region, or nullptr (the row-wise route)
template <class Op, class S>
__device__ __forceinline__ void size_row(const SizedArgs<Op>& a, int64_t r, const uint8_t* p, int n, bool valid, S shared) {
  int32_t len = -1;
  if (valid) {
    if constexpr (SharedBytes<Op>::value != 0 && !std::is_null_pointer_v<S>) len = size_or_flag(a.overflow, a.op.size(r, p, n, shared));
    else len = size_or_flag(a.overflow, a.op.size(r, p, n));
  }
  a.lens[r] = len;
}
template <class Op, class S>
__device__ __forceinline__ void write_row(const Op& op, int64_t r, const uint8_t* p, int n, uint8_t* o, S shared) {
  if constexpr (SharedBytes<Op>::value != 0 && !std::is_null_pointer_v<S>) op.write(r, p, n, o, shared);
  else op.write(r, p, n, o);
}
// the op's region at the front of the workgroup's LDS; the waves' buffers follow it
template <class Op>
__device__ __forceinline__ void stage_shared(const Op& op, uint8_t* shared) {
  if constexpr (SharedBytes<Op>::value != 0) {
    op.stage(shared, (int)threadIdx.x);
    __syncthreads();
  }
}

template <class Op>
__global__ void __launch_bounds__(256) k_sized_size_rows(SizedArgs<Op> a) {
  csdev::for_each_row(a.in, [&](int64_t r, const uint8_t* p, int n, bool valid) { size_row(a, r, p, n, valid, nullptr); });
}

template <class Op>
__global__ void __launch_bounds__(256) k_sized_write_rows(SizedArgs<Op> a) {
  csdev::for_each_row(a.in, [&](int64_t r, const uint8_t* p, int n, bool valid) {
    if (valid) write_row(a.op, r, p, n, a.out_chars + a.out_off[r], nullptr);
  });
}

template <class Op>
__global__ void __launch_bounds__(256) k_sized_size_tile(SizedArgs<Op> a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint8_t* shared = reinterpret_cast<uint8_t*>(smem);
  uint8_t* lds_in = shared + SharedBytes<Op>::value + (size_t)wv * a.cap;
  stage_shared(a.op, shared);
  // (a tile beyond the staging buffer -- a long row among short ones -- is read from memory)
  cstile::walk_staged_tiles<cstile::Oversize::kFromMemory>(a.in, a.rows_per_tile, a.ntiles, lds_in, a.cap, wv, lane,
                                                           [&](const cstile::RowTile& cur, const uint8_t* p) {
    if (cur.in_tile) size_row(a, cur.r0 + lane, p, cur.n, cur.live, shared);
  });
}

template <class Op>
__global__ void __launch_bounds__(256) k_sized_write_tile(SizedArgs<Op> a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint8_t* shared = reinterpret_cast<uint8_t*>(smem);
  uint8_t* lds_in = shared + SharedBytes<Op>::value + (size_t)wv * (a.cap + a.out_cap);
  uint8_t* lds_out = lds_in + a.cap;
  stage_shared(a.op, shared);
  cstile::walk_staged_tiles<cstile::Oversize::kFromMemory>(
      a.in, a.rows_per_tile, a.ntiles, lds_in, a.cap, wv, lane,
      [&](const cstile::RowTile& cur, bool& unstaged) {
        TileOut t;
        t.oo0 = a.out_off[cur.r0 + min(lane, cur.nrows)];
        t.oo1 = a.out_off[cur.r0 + min(lane + 1, cur.nrows)];
        t.ob = cstile::rl64(t.oo0, 0);
        t.oe = cstile::rl64(t.oo1, 63);
        t.fits = t.oe - t.ob + 16 <= a.out_cap;  // (wave-uniform)
        if constexpr (OwnTileWrite<Op>::value) unstaged |= !t.fits;
        t.staged = !unstaged;
        return t;
      },
      [&](const cstile::RowTile& cur, const uint8_t* p, const TileOut& t) {
        if constexpr (OwnTileWrite<Op>::value) {
          a.op.write_tile(TileWrite{cur, t, lds_in, lds_out, a.in.chars, a.out_chars, lane});
          if (!t.staged) return;
        } else {
          if (!t.fits) {  // beyond the out-tile: every row to memory by its lane
            if (cur.live) write_row(a.op, cur.r0 + lane, p, cur.n, a.out_chars + t.oo0, shared);
            return;
          }
          if (cur.live) write_row(a.op, cur.r0 + lane, p, cur.n, lds_out + (int)(t.oo0 - t.ob), shared);
        }
        cstile::wave_lds_fence();
        cstile::wave_flush_shift(a.out_chars + t.ob, (int)(t.oe - t.ob), lds_out, lane);
      });
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// The tile plan: R rows whose bytes fit the prefetch (a column with a few longer tiles still gets it: those tiles go from
// memory); the staging buffers of four waves and the out-tiles must fit the LDS.  R = 0: the row-wise route.
template <class Op>
cs::StagedTiles plan_sized(const cs_column* col, const Op& op, const char* rowwise_switch, SizedArgs<Op>& a, hipStream_t s) {
  a.in = cs::view_of(col);
  a.op = op;
  cs::StagedTiles t;
  if (!cs::cfg(rowwise_switch)) t = cs::plan_staged_tiles(col, cstile::kStageSlack, true, {1, 0, 100 * 1024}, s);
  a.rows_per_tile = t.R;
  a.cap = t.cap;
  a.ntiles = t.ntiles;
  return t;
}
template <class K, class Op>
void launch_rows(K kern, const SizedArgs<Op>& a, hipStream_t s) {
  hipLaunchKernelGGL(kern, dim3(std::min(cs::blocks_for(a.in.rows), 65536u)), dim3(csdev::kBlock), 0, s, a);
  CS_HIP(hipGetLastError());
}
// the write pass into b's column, whose offsets are there; returns the column
template <class Op>
cs_column* write_sized(cs::Built& b, const cs::StagedTiles& t, SizedArgs<Op>& a, const char* write_scope, hipStream_t s) {
  cs_column* const o = b.col.get();
  a.out_chars = b.alloc_chars();
  a.out_off = o->d_offsets();
  {
    cs::ProfScope ps(write_scope, s);
    if (t.R) {
      // the out-tile: the widest 64-row span of the output (an R-row tile lies inside one), capped
      const int64_t span = o->max_span64 >= 0 ? o->max_span64 : cs::max_span64(o, s);
      a.out_cap = (int)((std::min<int64_t>(span, kOutCapMax) + 16 + 15) & ~(int64_t)15);
      cs::launch_resident(&k_sized_write_tile<Op>, SharedBytes<Op>::value + t.lds + (size_t)a.out_cap * 4, t.grid, s, a);
    } else {
      launch_rows(k_sized_write_rows<Op>, a, s);
    }
  }
  cs::note_route(t.R ? "tile" : "rows");
  return b.col.release();
}

// `rowwise_switch`: the family's CS_*_ROWWISE; the scopes: its cs_prof names.  col has rows.
template <class Op>
cs_column* run_sized(const cs_column* col, const Op& op, const char* rowwise_switch, const char* size_scope, const char* write_scope,
                     hipStream_t s) {
  cs::Built b(col, s);
  SizedArgs<Op> a{};
  const cs::StagedTiles t = plan_sized(col, op, rowwise_switch, a, s);
  cs::Buf lens = cs::dev_alloc(sizeof(int32_t) * (size_t)col->rows, s);
  cs::Buf flag = cs::dev_alloc(sizeof(unsigned), s);
  CS_HIP(hipMemsetAsync(flag->p, 0, sizeof(unsigned), s));
  a.lens = cs::ptr<int32_t>(lens);
  a.overflow = cs::ptr<unsigned>(flag);
  {
    cs::ProfScope ps(size_scope, s);
    if (t.R && !SizeFromOffsets<Op>::value) cs::launch_resident(&k_sized_size_tile<Op>, SharedBytes<Op>::value + t.lds, t.grid, s, a);
    else launch_rows(k_sized_size_rows<Op>, a, s);
  }
  b.scan(cs::ptr<int32_t>(lens));
  unsigned over = 0;
  CS_HIP(hipMemcpy(&over, flag->p, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (over) cs::fail(CS_ERR_RANGE, "nvstrings: an output row would reach 2^31 bytes");
  return write_sized(b, t, a, write_scope, s);
}

// An op that changes no length (wrap): the output shares the input's extents and only the write pass runs.
template <class Op>
cs_column* run_sized_in_place(const cs_column* col, const Op& op, const char* rowwise_switch, const char* write_scope, hipStream_t s) {
  cs::Built b(col, s);
  SizedArgs<Op> a{};
  const cs::StagedTiles t = plan_sized(col, op, rowwise_switch, a, s);
  cs_column* const o = b.col.get();
  col->share_extents_with(o, s);
  o->nbytes = col->nbytes;
  o->max_row = col->max_row;
  o->max_span64 = col->max_span64;
  return write_sized(b, t, a, write_scope, s);
}

}  // namespace cssized
