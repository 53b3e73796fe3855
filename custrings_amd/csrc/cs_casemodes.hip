// NVStrings::swapcase / capitalize / title over row tiles (case.cu:169-397), on the design of k_case_tile (cs_case.hip),
// in a kernel of their own: lower / upper keep the object code they had (NOTES.md).
//
// A wave takes a tile of R consecutive rows (one contiguous span of chars).  Every lane transforms the 16-byte pieces it
// prefetched with the byte-parallel steps of chartype_ops.h (swar_piece) into the output tile in LDS and leaves a
// "byte >= 0x80" bit per byte in a bitmap:
//   swapcase    both letter ranges flipped in one step
//   capitalize  every ASCII letter to lower case; then each row lane restores its row's first byte (upper-cased)
//   title       a letter is upper-cased when the byte before it is not a letter, lower-cased otherwise; the byte before
//               a piece's first byte is read from the staged tile in LDS; then each row lane patches its row's first
//               byte, whose predecessor belongs to another row
// A row with a byte >= 0x80 is redone by its row lane with the sequential routine (case_size / case_write), LDS to LDS;
// a row whose size would change raises `changed` and the host recomputes the column with the two-pass row kernels.  The
// tile leaves with 16-byte stores to the positions it came from: the output shares the input's offsets and validity.
// A tile beyond the staging buffer is mapped straight from memory, sixteen bytes a lane.
#include <hip/hip_runtime.h>

#include "case_tile.h"
#include "chartype_ops.h"
#include "cs_internal.h"
#include "device_utils.h"
#include "tile_utils.h"

using namespace cs;
using namespace csdev;

namespace cs {
bool case_modes_fast(const cs_column* col, int op, bool ascii_ok, hipStream_t s, cs_column** out);
}

namespace {

using CaseModeArgs = cscase::TileArgs;  // (`bit` is not used)

template <int OP>
__device__ __forceinline__ uint4 map_piece(const uint4& q, uint32_t before) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  uint32_t o[4];
  cschr::swar_piece(OP, w, before, o);
  return make_uint4(o[0], o[1], o[2], o[3]);
}

template <int OP>
__global__ void __launch_bounds__(256) k_casemode_tile(CaseModeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const cscase::TileLds lds = cscase::carve_lds(smem, wv, a.cap);
  uint8_t *lds_in = lds.in, *lds_out = lds.out;
  uint32_t* bitmap = lds.bitmap;
  const ColView& in = a.in;
  cstile::RowTileWalk walk(in, a.rows_per_tile, a.ntiles, wv, lane);
  if (walk.done()) return;
  for (;;) {
    const cstile::RowTile cur = walk.current();
    const long long g0 = cur.g0, g1 = cur.g1;
    const int rbeg = cur.rbeg, n = cur.n, lead = cur.lead;
    const long long want64 = g1 - g0 + lead;
    if (want64 + 16 > a.cap) {
      // a tile beyond the staging buffer: the whole span with the wave straight from memory; then the row lanes patch first
      // bytes, or redo their rows when the tile holds other bytes
      const bool any_high = cscase::map_span_from_memory<OP != cschr::OP_SWAPCASE>(in.chars, a.out_chars, g0, lead, want64, lane,
                                                                                  [&](const uint4& q, const uint8_t* src, long long i) {
        return map_piece<OP>(q, (OP == cschr::OP_TITLE && i > 0) ? src[i - 1] : 0u);
      });
      if (n > 0) {
        const uint8_t* p = in.chars + (g0 + rbeg);
        if (any_high) {
          if (cschr::case_size(p, n, a.flags, a.cases, OP) != n) atomicOr(a.changed, 1u);
          else cschr::case_write(p, n, a.flags, a.cases, OP, a.out_chars + (g0 + rbeg));
        } else if (OP != cschr::OP_SWAPCASE) {
          a.out_chars[g0 + rbeg] = cschr::ascii_first(p[0]);
        }
      }
      if (!walk.advance()) break;
      continue;
    }
    const int want = (int)want64;
    if (OP == cschr::OP_TITLE) {  // the byte before a piece is read from the staged tile
      cstile::stage_chars(lds_in, want, lane, walk.pf);
      cstile::wave_lds_fence();
    }
    uint32_t any_high = 0;
#pragma unroll
    for (int j = 0; j < cstile::kPfChunks; ++j) {
      const int i = j * 1024 + lane * 16;
      if (i < want) {
        const uint4 q = walk.pf.v[j];
        if (OP != cschr::OP_TITLE) *reinterpret_cast<uint4*>(lds_in + i) = q;
        const uint32_t before = (OP == cschr::OP_TITLE && i > 0) ? lds_in[i - 1] : 0u;
        *reinterpret_cast<uint4*>(lds_out + i) = map_piece<OP>(q, before);
        const uint32_t hx = q.x & 0x80808080u, hy = q.y & 0x80808080u, hz = q.z & 0x80808080u, hw = q.w & 0x80808080u;
        any_high |= hx | hy | hz | hw;
        cstile::put_bits16(bitmap, i, cstile::gather16_bit7(hx, hy, hz, hw));
      }
    }
    const bool has_next = walk.advance();
    cstile::wave_lds_fence();
    const bool tile_high = __any(any_high != 0);
    if (n > 0) {
      const int p0 = lead + rbeg, p1 = p0 + n;  // this row's bytes [p0, p1) of the tile
      const uint8_t* p = lds_in + p0;
      uint8_t* o = lds_out + p0;
      const bool high = tile_high && cscase::row_has_high(bitmap, p0, p1);
      if (high) {
        if (cschr::case_size(p, n, a.flags, a.cases, OP) != n) atomicOr(a.changed, 1u);
        else cschr::case_write(p, n, a.flags, a.cases, OP, o);
      } else if (OP != cschr::OP_SWAPCASE) {
        o[0] = cschr::ascii_first(p[0]);
      }
    }
    if (OP != cschr::OP_SWAPCASE || tile_high) cstile::wave_lds_fence();
    cstile::wave_flush(a.out_chars + g0, (int)(g1 - g0), lds_out, lead, lane);
    cstile::wave_lds_fence();
    if (!has_next) break;
  }
}

template <int OP>
void launch_mode(const CaseModeArgs& a, const StagedTiles& t, hipStream_t s) {
  ProfScope ps(OP == cschr::OP_SWAPCASE ? "k_swapcase_write" : OP == cschr::OP_CAPITALIZE ? "k_capitalize_write" : "k_title_write", s);
  launch_resident(&k_casemode_tile<OP>, t.lds, t.grid, s, a);
}

}  // namespace

namespace cs {

// false: not applicable, or some row changes size -- the caller runs the two-pass row kernels
bool case_modes_fast(const cs_column* col, int op, bool ascii_ok, hipStream_t s, cs_column** out) {
  return cscase::run_case_tiles(col, ascii_ok, 0, s, out, [&](const CaseModeArgs& a, const StagedTiles& t) {
    if (op == cschr::OP_SWAPCASE) launch_mode<cschr::OP_SWAPCASE>(a, t, s);
    else if (op == cschr::OP_CAPITALIZE) launch_mode<cschr::OP_CAPITALIZE>(a, t, s);
    else launch_mode<cschr::OP_TITLE>(a, t, s);
  });
}

}  // namespace cs
