// What k_case_tile (cs_case.hip) and k_casemode_tile (cs_casemodes.hip) have in common: the per-wave LDS layout, the
// map of a tile beyond the staging buffer straight from memory, the row lane's test of its bits of the bitmap, and the
// host side (plan, output chars and the `changed` flag, the output column that shares the input's extents).
#pragma once
#include <hip/hip_runtime.h>

#include "cs_internal.h"
#include "tile_utils.h"

namespace cscase {

constexpr int kBitmapBytes = cstile::kPfBytes / 8 + 32;
constexpr int kSlack = 32;  // a tile is staged when its bytes + lead + 16 fit `cap`

struct TileArgs {
  cs::ColView in;
  int rows_per_tile;
  long long ntiles;
  unsigned bit;  // lower / upper: 32 = to lower, 64 = to upper (flag bit of the characters to change)
  const uint8_t* flags;
  const uint16_t* cases;
  uint8_t* out_chars;
  unsigned* changed;  // set when a row's size would change
  int cap;            // LDS bytes per tile buffer
};

// a wave's LDS: [input tile | output tile | bitmap], the tiles `cap` bytes each
struct TileLds {
  uint8_t *in, *out;
  uint32_t* bitmap;  // bit i: byte i of the tile is >= 0x80
};
__device__ __forceinline__ TileLds carve_lds(uint32_t* smem, int wv, int cap) {
  uint8_t* base = reinterpret_cast<uint8_t*>(smem) + (size_t)wv * (2 * cap + kBitmapBytes);
  return TileLds{base, base + cap, reinterpret_cast<uint32_t*>(base + 2 * cap)};
}

// word w of the bitmap, cut to the row's bits [p0, p1)
__device__ __forceinline__ uint32_t row_word(const uint32_t* bitmap, int w, int p0, int p1) {
  uint32_t m = bitmap[w];
  if (w == (p0 >> 5)) m &= 0xFFFFFFFFu << (p0 & 31);
  if (w == ((p1 - 1) >> 5) && (p1 & 31)) m &= ~(0xFFFFFFFFu << (p1 & 31));
  return m;
}
__device__ __forceinline__ bool row_has_high(const uint32_t* bitmap, int p0, int p1) {
  bool high = false;
  for (int w = p0 >> 5; w <= (p1 - 1) >> 5; ++w) high |= row_word(bitmap, w, p0, p1) != 0;
  return high;
}

// A tile beyond the staging buffer (the host sized it for all but a few tiles: one long row among millions of short
// ones): the whole span [g0, g0 + want64 - lead) with the wave, sixteen bytes a lane, straight from memory to the same
// positions of `out_chars` -- a long row would otherwise keep ONE lane busy for milliseconds.  `map(q, src, i)` gives
// the mapped piece of the 16 bytes q = src[i .. i + 16).  Returns whether the span holds a byte >= 0x80 (wave-uniform).
// The row lanes may rewrite bytes the piece lanes have just stored: those first stores must have left the wave before
// the second ones are issued (two stores to one address from different lanes are not ordered otherwise), so the wave
// waits for them when the rows will store -- always (ROWS_PATCH), or when there are high bytes.
template <bool ROWS_PATCH, class Map>
__device__ __forceinline__ bool map_span_from_memory(const uint8_t* chars, uint8_t* out_chars, long long g0, int lead, long long want64,
                                                     int lane, Map&& map) {
  bool high = false;
  const uint8_t* src = chars + (g0 - lead);
  uint8_t* dst = out_chars + (g0 - lead);
  for (long long i = (long long)lane * 16; i < want64; i += 64 * 16) {
    const uint4 q = *reinterpret_cast<const uint4*>(src + i);
    high |= ((q.x | q.y | q.z | q.w) & 0x80808080u) != 0;
    const uint4 o = map(q, src, i);
    const long long lo = lead - i, hi = want64 - i;  // the span's bytes inside this piece: [lo, hi)
    if (lo <= 0 && hi >= 16) {
      *reinterpret_cast<uint4*>(dst + i) = o;
    } else {
      const uint32_t w[4] = {o.x, o.y, o.z, o.w};
      for (int k = (int)(lo > 0 ? lo : 0); k < (int)(hi < 16 ? hi : 16); ++k) dst[i + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
  }
  const bool any_high = __any(high);
  if (ROWS_PATCH || any_high) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return any_high;
}

// The host side.  `launch(a, t)` runs the kernel with the arguments `a` on the plan `t`; false: not applicable, or some row
// changes size (`changed` was raised) -- the caller runs the two-pass row kernels.  On success *out is the output column:
// the new chars, the input's extents and validity (immutable buffers: shared).
template <class Launch>
bool run_case_tiles(const cs_column* col, bool ascii_ok, unsigned bit, hipStream_t s, cs_column** out, Launch&& launch) {
  using namespace cs;
  if (col->rows == 0 || !ascii_ok || col->nbytes == 0 || cfg("CS_CASE_ROWWISE")) return false;
  // (no tile size fits every tile -- one long row among short ones, or rows of hundreds of bytes throughout: 64-row tiles,
  // and the kernel maps a tile beyond the staging size with map_span_from_memory)
  const StagedTiles t = plan_staged_tiles(col, kSlack, true, {2, kBitmapBytes, 150 * 1024}, s);
  if (!t.R) return false;
  Buf chars = dev_alloc((size_t)col->nbytes, s);
  Buf flag = dev_alloc(sizeof(unsigned), s);
  CS_HIP(hipMemsetAsync(flag->p, 0, sizeof(unsigned), s));
  launch(TileArgs{view_of(col), t.R, t.ntiles, bit, d_unicode_flags(), d_charcases(), ptr<uint8_t>(chars), ptr<unsigned>(flag), t.cap}, t);
  unsigned* h = (unsigned*)pinned_scratch(sizeof(unsigned));
  CS_HIP(hipMemcpyAsync(h, flag->p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  if (*h) return false;
  auto* o = new cs_column;
  o->rows = col->rows;
  o->nbytes = col->nbytes;
  o->null_count = col->null_count;
  o->max_span64 = col->max_span64;
  o->max_row = col->max_row;
  col->share_extents_with(o, s);
  o->validity = col->validity;
  o->chars = chars;
  *out = o;
  return true;
}

}  // namespace cscase
