// url_encode / url_decode (reference: cpp/src/strings/urlencode.cu), translate and fillna (modify.cu:302-489).
// The per-row logic of the three ops that change row lengths is recode_ops.h, shared with the CPU harness of
// tests/test_recode_cpu.py.
//
// url_encode, url_decode and translate are a size pass, a scan (cs::Built) and a write pass, on two routes, both templated
// on the op:
//  - tile: a wave stages R consecutive rows in LDS (cstile::walk_staged_tiles, both passes).  The size pass maps its rows
//    to one int32 each out of LDS; the write pass has every lane write its row into an LDS out-tile and the tile leaves
//    with 16-byte stores (cstile::wave_flush_shift).  A tile whose input exceeds the staging buffer is read from memory
//    (Oversize::kFromMemory); a tile whose OUTPUT exceeds the out-tile -- url_encode grows a row up to 3x, translate up to
//    4x -- is written to memory by its lanes, from wherever its input is.  translate's 128 ASCII targets are staged once
//    per workgroup in front of the waves' buffers.
//  - rows: a thread per row from memory (CS_RECODE_ROWWISE=1, and columns the tile plan refuses).
// An output row of 2^31 bytes or more is CS_ERR_RANGE; the offsets are int64.
// fillna sizes its rows from offsets and validity alone and copies spans (a thread per row, as cs_scatter's copy does).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "cs_internal.h"
#include "device_utils.h"
#include "recode_ops.h"
#include "tile_utils.h"

using namespace cs;
using namespace csdev;
using csrecode::SafeMask;
using csrecode::Table;

namespace {

constexpr int kOutCapMax = 16 * 1024;  // LDS out-tile per wave at most (tiles beyond it are written to memory)
constexpr int kAsciiBytes = csrecode::kAsciiKeys * (int)sizeof(uint32_t);

struct RecodeArgs {
  ColView in;
  SafeMask safe;  // url_encode
  Table tab;      // translate (device memory)
  int32_t* lens;           // size pass
  unsigned* overflow;      // size pass: set when a row reaches 2^31 bytes
  const int64_t* out_off;  // write pass
  uint8_t* out_chars;
  int rows_per_tile, cap, out_cap;
  long long ntiles;
};

template <int OP>
constexpr int shared_bytes() {
  return OP == csrecode::OP_TRANSLATE ? kAsciiBytes : 0;
}

template <int OP>
__device__ __forceinline__ int64_t row_size(const RecodeArgs& a, const Table& t, const uint8_t* p, int n) {
  if constexpr (OP == csrecode::OP_URL_ENCODE) return csrecode::encode_size(a.safe, p, n);
  else if constexpr (OP == csrecode::OP_URL_DECODE) return csrecode::decode_size(p, n);
  else return csrecode::translate_size(t, p, n);
}
template <int OP>
__device__ __forceinline__ void row_write(const RecodeArgs& a, const Table& t, const uint8_t* p, int n, uint8_t* o) {
  if constexpr (OP == csrecode::OP_URL_ENCODE) csrecode::encode_write(a.safe, p, n, o);
  else if constexpr (OP == csrecode::OP_URL_DECODE) csrecode::decode_write(p, n, o);
  else csrecode::translate_write(t, p, n, o);
}

// the size of row r, its n bytes at p (memory or LDS); -1 for a null row
template <int OP>
__device__ __forceinline__ void size_row(const RecodeArgs& a, const Table& t, int64_t r, const uint8_t* p, int n, bool valid) {
  int32_t len = -1;
  if (valid) {
    const int64_t sz = row_size<OP>(a, t, p, n);
    if (sz >= ((int64_t)1 << 31)) {
      atomicOr(a.overflow, 1u);
      len = 0;
    } else {
      len = (int32_t)sz;
    }
  }
  a.lens[r] = len;
}

// the workgroup's copy of translate's ASCII targets at the front of the LDS; the waves' buffers follow it
template <int OP>
__device__ __forceinline__ Table stage_table(const RecodeArgs& a, uint32_t* smem) {
  Table t = a.tab;
  if constexpr (OP == csrecode::OP_TRANSLATE) {
    if (threadIdx.x < csrecode::kAsciiKeys) smem[threadIdx.x] = a.tab.ascii[threadIdx.x];
    __syncthreads();
    t.ascii = smem;
  }
  return t;
}

// ---- rows ----------------------------------------------------------------------------------------------------------------
template <int OP>
__global__ void __launch_bounds__(256) k_recode_size_rows(RecodeArgs a) {
  for_each_row(a.in, [&](int64_t r, const uint8_t* p, int n, bool valid) { size_row<OP>(a, a.tab, r, p, n, valid); });
}

template <int OP>
__global__ void __launch_bounds__(256) k_recode_write_rows(RecodeArgs a) {
  for_each_row(a.in, [&](int64_t r, const uint8_t* p, int n, bool valid) {
    if (valid) row_write<OP>(a, a.tab, p, n, a.out_chars + a.out_off[r]);
  });
}

// ---- tiles ---------------------------------------------------------------------------------------------------------------
template <int OP>
__global__ void __launch_bounds__(256) k_recode_size_tile(RecodeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const Table t = stage_table<OP>(a, smem);
  uint8_t* lds_in = reinterpret_cast<uint8_t*>(smem) + shared_bytes<OP>() + (size_t)wv * a.cap;
  cstile::walk_staged_tiles<cstile::Oversize::kFromMemory>(a.in, a.rows_per_tile, a.ntiles, lds_in, a.cap, wv, lane,
                                                           [&](const cstile::RowTile& cur, const uint8_t* p) {
    if (cur.in_tile) size_row<OP>(a, t, cur.r0 + lane, p, cur.n, cur.live);
  });
}

template <int OP>
__global__ void __launch_bounds__(256) k_recode_write_tile(RecodeArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const Table t = stage_table<OP>(a, smem);
  uint8_t* lds_in = reinterpret_cast<uint8_t*>(smem) + shared_bytes<OP>() + (size_t)wv * (a.cap + a.out_cap);
  uint8_t* lds_out = lds_in + a.cap;
  cstile::walk_staged_tiles<cstile::Oversize::kFromMemory>(a.in, a.rows_per_tile, a.ntiles, lds_in, a.cap, wv, lane,
                                                           [&](const cstile::RowTile& cur, const uint8_t* p) {
    // the tile's output rows [ob, oe): lanes beyond its rows repeat the end
    const long long oo0 = a.out_off[cur.r0 + min(lane, cur.nrows)];
    const long long oo1 = a.out_off[cur.r0 + min(lane + 1, cur.nrows)];
    const long long ob = cstile::rl64(oo0, 0), oe = cstile::rl64(oo1, 63);
    if (oe - ob + 16 > a.out_cap) {  // (wave-uniform) beyond the out-tile: every row to memory by its lane
      if (cur.live) row_write<OP>(a, t, p, cur.n, a.out_chars + oo0);
      return;
    }
    if (cur.live) row_write<OP>(a, t, p, cur.n, lds_out + (int)(oo0 - ob));
    cstile::wave_lds_fence();
    cstile::wave_flush_shift(a.out_chars + ob, (int)(oe - ob), lds_out, lane);
  });
}

// ---- host ------------------------------------------------------------------------------------------------------------------
template <int OP>
cs_column* run_recode(const cs_column* col, RecodeArgs a, hipStream_t s) {
  const int64_t rows = col->rows;
  if (rows == 0) return make_all_null(0, s);
  Built b(col, s);
  cs_column* const o = b.col.get();
  a.in = view_of(col);
  // the tile plan: R rows whose bytes fit the prefetch (a column with a few longer tiles still gets it: those tiles go from
  // memory); the staging buffers of four waves and the out-tiles must fit the LDS
  StagedTiles t;
  if (!cs::cfg("CS_RECODE_ROWWISE")) t = plan_staged_tiles(col, cstile::kStageSlack, true, {1, 0, 100 * 1024}, s);
  const bool tile = t.R != 0;
  a.rows_per_tile = t.R;
  a.cap = t.cap;
  a.ntiles = t.ntiles;
  const unsigned row_grid = std::min(blocks_for(rows), 65536u);
  Buf lens = dev_alloc(sizeof(int32_t) * (size_t)rows, s);
  Buf flag = dev_alloc(sizeof(unsigned), s);
  CS_HIP(hipMemsetAsync(flag->p, 0, sizeof(unsigned), s));
  a.lens = ptr<int32_t>(lens);
  a.overflow = ptr<unsigned>(flag);
  {
    ProfScope ps("k_recode_size", s);
    if (tile) {
      launch_resident(&k_recode_size_tile<OP>, shared_bytes<OP>() + t.lds, t.grid, s, a);
    } else {
      hipLaunchKernelGGL(k_recode_size_rows<OP>, dim3(row_grid), dim3(kBlock), 0, s, a);
      CS_HIP(hipGetLastError());
    }
  }
  b.scan(ptr<int32_t>(lens));
  unsigned over = 0;
  CS_HIP(hipMemcpy(&over, flag->p, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (over) fail(CS_ERR_RANGE, "nvstrings: an output row would reach 2^31 bytes");
  a.out_chars = b.alloc_chars();
  a.out_off = b.off;
  {
    ProfScope ps("k_recode_write", s);
    if (tile) {
      // the out-tile: the widest 64-row span of the output (an R-row tile lies inside one), capped
      const int64_t span = o->max_span64 >= 0 ? o->max_span64 : max_span64(o, s);
      a.out_cap = (int)((std::min<int64_t>(span, kOutCapMax) + 16 + 15) & ~(int64_t)15);
      launch_resident(&k_recode_write_tile<OP>, shared_bytes<OP>() + t.lds + (size_t)a.out_cap * 4, t.grid, s, a);
    } else {
      hipLaunchKernelGGL(k_recode_write_rows<OP>, dim3(row_grid), dim3(kBlock), 0, s, a);
      CS_HIP(hipGetLastError());
    }
  }
  note_route(tile ? "tile" : "rows");
  return b.col.release();
}

// ---- fillna ----------------------------------------------------------------------------------------------------------------
// a null row takes row r of `repl`, or the string when repl has no offsets (sn bytes at `str`)
__global__ void __launch_bounds__(256) k_fillna_lengths(ColView in, ColView repl, int sn, int32_t* __restrict__ lens) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= in.rows) return;
  int32_t len;
  if (row_is_valid(in.validity, r)) len = (int32_t)(in.offsets[r + 1] - in.offsets[r]);
  else if (!repl.offsets) len = sn;
  else len = row_is_valid(repl.validity, r) ? (int32_t)(repl.offsets[r + 1] - repl.offsets[r]) : -1;
  lens[r] = len;
}
__global__ void __launch_bounds__(256) k_fillna_copy(ColView in, ColView repl, const uint8_t* __restrict__ str,
                                                     const int64_t* __restrict__ off, uint8_t* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= in.rows) return;
  const int len = (int)(off[r + 1] - off[r]);
  if (len <= 0) return;
  const uint8_t* p = row_is_valid(in.validity, r) ? in.chars + in.offsets[r] : (repl.offsets ? repl.chars + repl.offsets[r] : str);
  copy_bytes(out + off[r], p, len);
}

cs_column* run_fillna(const cs_column* col, const cs_column* repl, const char* str, hipStream_t s) {
  const int64_t rows = col->rows;
  if (rows == 0) return make_all_null(0, s);
  const int sn = repl ? 0 : (int)strlen(str);
  Buf dstr;
  if (!repl) {
    dstr = dev_alloc((size_t)sn + 1, s);
    CS_HIP(hipMemcpyAsync(dstr->p, str, (size_t)sn + 1, hipMemcpyHostToDevice, s));
  }
  const ColView rv = repl ? view_of(repl) : ColView{nullptr, nullptr, nullptr, 0};
  Buf lens = dev_alloc(sizeof(int32_t) * (size_t)rows, s);
  hipLaunchKernelGGL(k_fillna_lengths, dim3(blocks_for(rows)), dim3(kBlock), 0, s, view_of(col), rv, sn, ptr<int32_t>(lens));
  CS_HIP(hipGetLastError());
  Built b(rows, repl ? Nulls::separate : Nulls::none, s);
  b.scan(ptr<int32_t>(lens));
  b.alloc_chars();
  hipLaunchKernelGGL(k_fillna_copy, dim3(blocks_for(rows)), dim3(kBlock), 0, s, view_of(col), rv, ptr<const uint8_t>(dstr), b.off, b.chars);
  CS_HIP(hipGetLastError());
  CS_HIP(hipStreamSynchronize(s));  // (the caller's string and the temporaries are done with)
  return b.col.release();
}

template <class F>
int recode_entry(const cs_column* col, cs_column** out, F&& f) {
  return guard([&] {
    if (!col || !out) fail(CS_ERR_INVALID_ARG, "null column or output");
    *out = nullptr;
    require_device();
    *out = f();
  });
}

}  // namespace

extern "C" {

int cs_url_encode(const cs_column* col, cs_stream stream, cs_column** out) {
  return recode_entry(col, out, [&] {
    RecodeArgs a{};
    a.safe = csrecode::url_safe_mask();
    return run_recode<csrecode::OP_URL_ENCODE>(col, a, S(stream));
  });
}

int cs_url_decode(const cs_column* col, cs_stream stream, cs_column** out) {
  return recode_entry(col, out, [&] { return run_recode<csrecode::OP_URL_DECODE>(col, RecodeArgs{}, S(stream)); });
}

int cs_translate(const cs_column* col, const uint32_t* from, const uint32_t* to, int n, cs_stream stream, cs_column** out) {
  return recode_entry(col, out, [&] {
    if (n < 0 || (n > 0 && (!from || !to))) fail(CS_ERR_INVALID_ARG, "nvstrings::translate: the table is missing");
    hipStream_t s = S(stream);
    csrecode::HostTable h;
    if (!csrecode::make_table(from, to, n, h)) fail(CS_ERR_INVALID_ARG, "nvstrings::translate: a code point above U+10FFFF");
    // one buffer: the ASCII targets, the other keys, their targets
    const size_t nk = h.keys.size();
    std::vector<uint32_t> host(h.ascii, h.ascii + csrecode::kAsciiKeys);
    host.insert(host.end(), h.keys.begin(), h.keys.end());
    host.insert(host.end(), h.vals.begin(), h.vals.end());
    Buf d = dev_alloc(host.size() * sizeof(uint32_t), s);
    CS_HIP(hipMemcpyAsync(d->p, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    RecodeArgs a{};
    a.tab.ascii = ptr<const uint32_t>(d);
    a.tab.keys = a.tab.ascii + csrecode::kAsciiKeys;
    a.tab.vals = a.tab.keys + nk;
    a.tab.nkeys = (int)nk;
    cs_column* c = run_recode<csrecode::OP_TRANSLATE>(col, a, s);
    CS_HIP(hipStreamSynchronize(s));  // (the table is done with)
    return c;
  });
}

int cs_fillna(const cs_column* col, const char* str, cs_stream stream, cs_column** out) {
  return recode_entry(col, out, [&] {
    if (!str) fail(CS_ERR_INVALID_ARG, "nvstrings::fillna parameter cannot be null");
    return run_fillna(col, nullptr, str, S(stream));
  });
}

int cs_fillna_column(const cs_column* col, const cs_column* repl, cs_stream stream, cs_column** out) {
  return recode_entry(col, out, [&] {
    if (!repl) fail(CS_ERR_INVALID_ARG, "nvstrings::fillna parameter cannot be null");
    if (repl->rows != col->rows) fail(CS_ERR_INVALID_ARG, "nvstrings::fillna parameter must have the same number of strings");
    return run_fillna(col, repl, nullptr, S(stream));
  });
}

}  // extern "C"
