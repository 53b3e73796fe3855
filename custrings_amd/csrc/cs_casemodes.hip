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

struct CaseModeArgs {
  ColView in;
  int rows_per_tile;
  long long ntiles;
  const uint8_t* flags;
  const uint16_t* cases;
  uint8_t* out_chars;
  unsigned* changed;  // set when a row's size would change
  int cap;            // LDS bytes per tile buffer
};

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
  constexpr int kBitmapBytes = cstile::kPfBytes / 8 + 32;
  uint8_t* base = reinterpret_cast<uint8_t*>(smem) + (size_t)wv * (2 * a.cap + kBitmapBytes);
  uint8_t* lds_in = base;
  uint8_t* lds_out = base + a.cap;
  uint32_t* bitmap = reinterpret_cast<uint32_t*>(base + 2 * a.cap);  // bit i: byte i of the tile is >= 0x80
  const ColView& in = a.in;
  cstile::RowTileWalk walk(in, a.rows_per_tile, a.ntiles, wv, lane);
  if (walk.done()) return;
  for (;;) {
    const cstile::RowTile cur = walk.current();
    const long long g0 = cur.g0, g1 = cur.g1;
    const int rbeg = cur.rbeg, n = cur.n, lead = cur.lead;
    const long long want64 = g1 - g0 + lead;
    if (want64 + 16 > a.cap) {
      // a tile beyond the staging buffer (one long row among short ones): the whole span with the wave, sixteen bytes a
      // lane, straight from memory; then the row lanes patch first bytes, or redo their rows when the tile holds other bytes
      bool high = false;
      const uint8_t* src = in.chars + (g0 - lead);
      uint8_t* dst = a.out_chars + (g0 - lead);
      for (long long i = (long long)lane * 16; i < want64; i += 64 * 16) {
        const uint4 q = *reinterpret_cast<const uint4*>(src + i);
        high |= ((q.x | q.y | q.z | q.w) & 0x80808080u) != 0;
        const uint32_t before = (OP == cschr::OP_TITLE && i > 0) ? src[i - 1] : 0u;
        const uint4 o = map_piece<OP>(q, before);
        const long long lo = lead - i, hi = want64 - i;  // the span's bytes inside this piece: [lo, hi)
        if (lo <= 0 && hi >= 16) {
          *reinterpret_cast<uint4*>(dst + i) = o;
        } else {
          const uint32_t w[4] = {o.x, o.y, o.z, o.w};
          for (int k = (int)(lo > 0 ? lo : 0); k < (int)(hi < 16 ? hi : 16); ++k) dst[i + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
      }
      const bool any_high = __any(high);
      // the row lanes rewrite bytes the piece lanes have just stored: the first stores must have left the wave before the
      // second ones are issued (two stores to one address from different lanes are not ordered otherwise)
      if (OP != cschr::OP_SWAPCASE || any_high) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
      bool high = false;
      if (tile_high) {
        for (int w = p0 >> 5; w <= (p1 - 1) >> 5; ++w) {
          uint32_t m = bitmap[w];
          if (w == (p0 >> 5)) m &= 0xFFFFFFFFu << (p0 & 31);
          if (w == ((p1 - 1) >> 5) && (p1 & 31)) m &= ~(0xFFFFFFFFu << (p1 & 31));
          high |= m != 0;
        }
      }
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
void launch_mode(const CaseModeArgs& a, size_t lds, hipStream_t s) {
  ProfScope ps(OP == cschr::OP_SWAPCASE ? "k_swapcase_write" : OP == cschr::OP_CAPITALIZE ? "k_capitalize_write" : "k_title_write", s);
  launch_resident(&k_casemode_tile<OP>, lds, (a.ntiles + 3) / 4, s, a);
}

}  // namespace

namespace cs {

// false: not applicable, or some row changes size -- the caller runs the two-pass row kernels
bool case_modes_fast(const cs_column* col, int op, bool ascii_ok, hipStream_t s, cs_column** out) {
  const int64_t rows = col->rows;
  if (rows == 0 || !ascii_ok || col->nbytes == 0 || cs::cfg("CS_CASE_ROWWISE")) return false;
  const TilePlan tp = plan_row_tiles(col, 32, s, true);
  const int R = tp.R;
  if (!R) return false;
  CaseModeArgs a{};
  a.in = view_of(col);
  a.rows_per_tile = R;
  a.ntiles = (rows + R - 1) / R;
  a.flags = d_unicode_flags();
  a.cases = d_charcases();
  a.cap = (int)((tp.span + 32 + 15) & ~(int64_t)15);
  constexpr size_t kBitmapBytes = cstile::kPfBytes / 8 + 32;
  const size_t lds = (2 * (size_t)a.cap + kBitmapBytes) * 4;
  if (lds > 150 * 1024) return false;
  Buf chars = dev_alloc((size_t)col->nbytes, s);
  Buf flag = dev_alloc(sizeof(unsigned), s);
  CS_HIP(hipMemsetAsync(flag->p, 0, sizeof(unsigned), s));
  a.out_chars = ptr<uint8_t>(chars);
  a.changed = ptr<unsigned>(flag);
  if (op == cschr::OP_SWAPCASE) launch_mode<cschr::OP_SWAPCASE>(a, lds, s);
  else if (op == cschr::OP_CAPITALIZE) launch_mode<cschr::OP_CAPITALIZE>(a, lds, s);
  else launch_mode<cschr::OP_TITLE>(a, lds, s);
  unsigned* h = (unsigned*)pinned_scratch(sizeof(unsigned));
  CS_HIP(hipMemcpyAsync(h, flag->p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  if (*h) return false;  // some row changes size: the two-pass row kernels recompute the column
  auto* o = new cs_column;
  o->rows = rows;
  o->nbytes = col->nbytes;
  o->null_count = col->null_count;
  o->max_span64 = col->max_span64;
  o->max_row = col->max_row;
  col->share_extents_with(o);  // same row extents: share the immutable buffers
  o->validity = col->validity;
  o->chars = chars;
  *out = o;
  return true;
}

}  // namespace cs
