// NVStrings::lower / upper over row tiles (case.cu:31-170).
//
// Case mapping almost never changes a character's UTF-8 width, and ASCII text needs no
// table at all, so the common case is a streaming pass: a wave takes a tile of R consecutive
// rows (their chars are one contiguous span), every lane flips the ASCII letters of the
// 16-byte pieces it loaded with SWAR arithmetic and writes them to the output tile in LDS,
// and only rows that contain non-ASCII bytes (found through a per-byte bitmap the piece
// lanes leave in LDS) are redone by their row lane with the same per-character routine the
// row-wise kernels use (row_ops.h: decode, flag/case tables, re-encode) -- LDS to LDS.  The
// tile is then flushed with 16-byte stores to the same positions it came from: the output
// shares the input's offsets and validity buffers.  A row whose mapped size differs from its
// input size raises a flag and the host recomputes the column with the two-pass row kernels.
#include <hip/hip_runtime.h>

#include "case_tile.h"
#include "cs_internal.h"
#include "device_utils.h"
#include "row_ops.h"
#include "tile_utils.h"

using namespace cs;
using namespace csdev;
using namespace csrow;

namespace cs {
bool change_case_fast(const cs_column* col, unsigned bit, bool ascii_rule_ok, hipStream_t s, cs_column** out);
}

namespace {

using CaseTileArgs = cscase::TileArgs;

// ASCII letters of the other case, flipped (bit 5 toggled); other bytes untouched
__device__ __forceinline__ uint32_t flip_ascii(uint32_t w, unsigned bit) {
  const uint32_t x = w & 0x7F7F7F7Fu;
  // to lower: bytes 0x41..0x5A; to upper: 0x61..0x7A
  const uint32_t lo = bit == 32 ? 0x3F3F3F3Fu : 0x1F1F1F1Fu;  // 0x80 - first letter
  const uint32_t hi = bit == 32 ? 0x25252525u : 0x05050505u;  // 0x7F - last letter
  const uint32_t m = (x + lo) & ~(x + hi) & ~w & 0x80808080u;
  return w ^ (m >> 2);
}

__global__ void __launch_bounds__(256) k_case_tile(CaseTileArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;  // (scalar: what derives from it stays in SGPRs)
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
      // A tile beyond the staging buffer: the whole span with the wave (an ASCII tile -- the usual case -- is done after
      // that); only a tile with other bytes goes row by row, a thread each, as the row-wise kernels do.
      const bool any_high = cscase::map_span_from_memory<false>(in.chars, a.out_chars, g0, lead, want64, lane, [&](const uint4& q, const uint8_t*, long long) {
        return make_uint4(flip_ascii(q.x, a.bit), flip_ascii(q.y, a.bit), flip_ascii(q.z, a.bit), flip_ascii(q.w, a.bit));
      });
      if (any_high && n > 0) {
        const uint8_t* p = in.chars + (g0 + rbeg);
        if (row_case_size(p, n, a.flags, a.cases, a.bit) != n) atomicOr(a.changed, 1u);
        else row_case_write(p, n, a.flags, a.cases, a.bit, a.out_chars + (g0 + rbeg));
      }
      if (!walk.advance()) break;
      continue;
    }
    const int want = (int)want64;
    // pieces: keep the input in LDS for the row lanes, ASCII-flipped copy in the output tile,
    // one "byte >= 0x80" bit per byte in the bitmap
    uint32_t any_high = 0;
#pragma unroll
    for (int j = 0; j < cstile::kPfChunks; ++j) {
      const int i = j * 1024 + lane * 16;
      if (i < want) {
        const uint4 q = walk.pf.v[j];
        *reinterpret_cast<uint4*>(lds_in + i) = q;
        uint4 o;
        o.x = flip_ascii(q.x, a.bit);
        o.y = flip_ascii(q.y, a.bit);
        o.z = flip_ascii(q.z, a.bit);
        o.w = flip_ascii(q.w, a.bit);
        *reinterpret_cast<uint4*>(lds_out + i) = o;
        const uint32_t hx = q.x & 0x80808080u, hy = q.y & 0x80808080u, hz = q.z & 0x80808080u, hw = q.w & 0x80808080u;
        any_high |= hx | hy | hz | hw;
        cstile::put_bits16(bitmap, i, cstile::gather16_bit7(hx, hy, hz, hw));
      }
    }
    const bool has_next = walk.advance();
    cstile::wave_lds_fence();
    if (__any(any_high != 0)) {  // some row of the tile holds non-ASCII characters
      // Row lanes visit only the non-ASCII bytes of their row (bitmap bits), in order: a lead byte
      // followed by exactly its continuation bytes is mapped through the tables and patched into
      // the output tile; anything else (stray or missing continuation bytes) sends the row through
      // the sequential routines of row_ops.h, which define the behaviour for malformed input.
      if (n > 0) {
        const int p0 = lead + rbeg, p1 = p0 + n;  // this row's bits [p0, p1)
        const uint8_t* p = lds_in + p0;
        uint8_t* o = lds_out + p0;
        bool any = false, malformed = false, resized = false;
        int expect = 0, last = -2;
        for (int w = p0 >> 5; w <= (p1 - 1) >> 5; ++w) {
          uint32_t m = cscase::row_word(bitmap, w, p0, p1);
          while (m) {
            const int i = (w << 5) + __builtin_ctz(m) - p0;  // row offset of this non-ASCII byte
            m &= m - 1;
            any = true;
            const uint8_t b = p[i];
            if (expect > 0) {
              malformed |= !is_cont(b) || i != last + 1;
              --expect;
            } else {
              const unsigned w8 = lead_width(b);
              malformed |= w8 < 2 || i + (int)w8 > n;
              expect = (int)w8 - 1;
              if (!malformed) {
                Char ch;
                decode_at(p, i, n, ch);
                const unsigned u = packed_to_cp(ch);
                const unsigned f = u <= 0xFFFF ? a.flags[u] : 0;
                if (f & a.bit) {
                  const Char nc = cp_to_packed(a.cases[u]);
                  if (packed_width(nc) != w8) resized = true;
                  else
                    for (unsigned k = 0; k < w8; ++k) o[i + (int)k] = (uint8_t)(nc >> (8 * (w8 - 1 - k)));
                }
              }
            }
            last = i;
          }
        }
        malformed |= expect != 0;
        if (any && malformed) {
          // the sequential routine alone decides for such a row: a character that changes its width in front of the
          // malformed bytes may be made up for behind them (what `resized` holds is of the walk above, which stopped)
          resized = row_case_size(p, n, a.flags, a.cases, a.bit) != n;
          if (!resized) row_case_write(p, n, a.flags, a.cases, a.bit, o);
        }
        if (resized) atomicOr(a.changed, 1u);
      }
      cstile::wave_lds_fence();
    }
    cstile::wave_flush(a.out_chars + g0, (int)(g1 - g0), lds_out, lead, lane);
    cstile::wave_lds_fence();
    if (!has_next) break;
  }
}

}  // namespace

namespace cs {

bool change_case_fast(const cs_column* col, unsigned bit, bool ascii_rule_ok, hipStream_t s, cs_column** out) {
  return cscase::run_case_tiles(col, ascii_rule_ok, bit, s, out, [&](const CaseTileArgs& a, const StagedTiles& t) {
    ProfScope ps(bit == 32 ? "k_lower_write" : "k_upper_write", s);
    launch_resident(&k_case_tile, t.lds, t.grid, s, a);
  });
}

}  // namespace cs
