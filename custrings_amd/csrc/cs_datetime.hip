// Timestamp conversions to and from string columns (reference: cpp/src/strings/datetime.cu, the members
// timestamp2long / long2timestamp).  The per-row logic is datetime_ops.h, shared with the CPU harness of
// tests/test_datetime_cpu.py; the format program is compiled once per call on the host and passed by value in the
// kernel arguments, the units are a template parameter (every divisor a compile-time constant).
//
// Parse (string -> int64 per row): the tile and row-wise routes of parse_route.h, with csdt::parse_ts_row.
// Format (int64 -> string): every non-null row is W bytes, W a function of the format and the units alone, so there is
// no length pass.  Without nulls row r starts at r x W; with nulls at the scan of W x (valid rows per 64-row word) plus
// W x the valid rows in front of it in its word.  A wave formats its 64 rows -- one contiguous span of the output --
// and writes their offsets and validity word:
//  - lds: the rows are assembled in LDS and the span goes out with 16-byte stores (cstile::wave_flush_shift);
//  - rows: every lane writes its row with byte stores (formats too wide for the LDS budget, and CS_CONVERT_ROWWISE=1).
// The offsets are int32 when rows x W < 2^31, else int64 -- the rule of the other format ops, with W exact here.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <type_traits>

#include "cs_internal.h"
#include "datetime_ops.h"
#include "device_utils.h"
#include "parse_route.h"
#include "tile_utils.h"

using namespace cs;
using namespace csdev;
using csdt::TsProgram;

namespace {

constexpr int kTsLdsMaxWidth = 256;  // widest row the LDS writer takes: 4 waves x 64 rows x 256 B = 64 KB per workgroup

template <int U>
struct TsParse {
  using T = int64_t;
  TsProgram prog;
  // (the row's bytes end at n: parse_ts_row reads nothing of the neighbour's bytes staged behind it)
  __device__ __forceinline__ int64_t operator()(const uint8_t* p, int n, bool valid) const {
    return valid ? csdt::parse_ts_row<U>(p, n, prog) : 0;
  }
};

void compile_or_fail(const char* format, int units, TsProgram* prog, const char* what) {
  switch (csdt::compile_ts_format(format, units, prog)) {
    case csdt::TS_OK: return;
    case csdt::TS_ERR_UNITS: fail(CS_ERR_INVALID_ARG, std::string(what) + ": units value unrecognized");
    case csdt::TS_ERR_UNFINISHED: fail(CS_ERR_INVALID_ARG, std::string(what) + ": unfinished specifier");
    case csdt::TS_ERR_SPECIFIER: fail(CS_ERR_INVALID_ARG, std::string(what) + ": invalid specifier");
    default: fail(CS_ERR_INVALID_ARG, std::string(what) + ": format too long (at most 64 specifiers and literal runs, 256 literal bytes)");
  }
}

int64_t run_ts_parse(const cs_column* col, const TsProgram& prog, int64_t* results, int on_device, hipStream_t s) {
  int64_t n = 0;
  csdt::ts_dispatch(prog.units, [&](auto u) { n = csparse::run_parse(col, TsParse<decltype(u)::value>{prog}, results, on_device, !cfg("CS_CONVERT_ROWWISE"), s); });
  return n;
}

// ---- format ------------------------------------------------------------------------------------------------------------
struct TsFormatArgs {
  const int64_t* values;
  const uint8_t* nulls;       // LSB-first, bit = 1 valid; nullptr = all valid
  const int64_t* word_base;   // with nulls: the first output byte of every 64-row word (nullptr: r0 x W)
  uint64_t* validity;         // with nulls: the column's validity words
  uint8_t* chars;
  int64_t rows;
  int lds_stride;             // LDS writer: bytes per wave
  TsProgram prog;
};

// W x the valid rows of every 64-row word (the caller's mask is (rows + 7) / 8 bytes: nothing past it is read)
__global__ void k_ts_word_bytes(const uint8_t* __restrict__ nulls, int64_t rows, int width, int32_t* __restrict__ out) {
  const int64_t words = (rows + 63) / 64;
  const int64_t nbytes = (rows + 7) / 8;
  for (int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x; w < words; w += (int64_t)gridDim.x * kBlock) {
    uint64_t m = 0;
    for (int k = 0; k < 8; ++k)
      if (w * 8 + k < nbytes) m |= (uint64_t)nulls[w * 8 + k] << (8 * k);
    const int64_t left = rows - w * 64;
    if (left < 64) m &= ((uint64_t)1 << left) - 1;
    out[w] = __popcll(m) * width;
  }
}

// A wave per 64-row word (grid-stride): offsets, the validity word, the rows' bytes.
template <int U, bool LDS, class Off>
__global__ void __launch_bounds__(256) k_ts_format(TsFormatArgs a, Off* __restrict__ offsets) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  uint8_t* lds = reinterpret_cast<uint8_t*>(smem) + (size_t)wv * a.lds_stride;
  const int64_t W = a.prog.width;
  const int64_t words = (a.rows + 63) / 64;
  for (int64_t w = (int64_t)blockIdx.x * 4 + wv; w < words; w += (int64_t)gridDim.x * 4) {
    const int64_t r = w * 64 + lane;
    const bool in = r < a.rows;
    const bool valid = in && csparse::value_valid(a.nulls, r);
    const uint64_t mask = __ballot(valid);
    const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    const int64_t base = a.word_base ? a.word_base[w] : w * 64 * W;
    if (in) offsets[r] = (Off)(base + rank * W);
    if (r == a.rows - 1) offsets[a.rows] = (Off)(base + (rank + (valid ? 1 : 0)) * W);
    if (a.validity && lane == 0) a.validity[w] = mask;
    const int64_t x = valid ? a.values[r] : 0;
    if constexpr (LDS) {
      if (valid) csdt::format_ts_row<U>(x, a.prog, lds + rank * W);
      cstile::wave_lds_fence();
      cstile::wave_flush_shift(a.chars + base, (int)(__popcll(mask) * W), lds, lane);
      cstile::wave_lds_fence();  // (the LDS is reused by the next word)
    } else {
      if (valid) csdt::format_ts_row<U>(x, a.prog, a.chars + base + rank * W);
    }
  }
}

cs_column* run_ts_format(const int64_t* values, int64_t rows, const uint8_t* nulls, int on_device, const TsProgram& prog,
                         hipStream_t s) {
  Buf vtmp, ntmp;
  TsFormatArgs a{};
  a.rows = rows;
  a.values = values;
  a.nulls = nulls;
  a.prog = prog;
  if (!on_device) {
    vtmp = dev_alloc(sizeof(int64_t) * (size_t)rows, s);
    CS_HIP(hipMemcpyAsync(vtmp->p, values, sizeof(int64_t) * (size_t)rows, hipMemcpyHostToDevice, s));
    a.values = ptr<const int64_t>(vtmp);
    if (nulls) {
      ntmp = dev_alloc((size_t)(rows + 7) / 8, s);
      CS_HIP(hipMemcpyAsync(ntmp->p, nulls, (size_t)(rows + 7) / 8, hipMemcpyHostToDevice, s));
      a.nulls = ptr<const uint8_t>(ntmp);
    }
  }
  const int64_t W = prog.width;
  const int64_t words = (rows + 63) / 64;
  auto c = std::make_unique<cs_column>();
  c->rows = rows;
  Buf word_base;
  if (a.nulls) {
    Buf wb = dev_alloc(sizeof(int32_t) * (size_t)words, s);
    hipLaunchKernelGGL(k_ts_word_bytes, dim3(std::min(blocks_for(words), 8192u)), dim3(kBlock), 0, s, a.nulls, rows, (int)W,
                       ptr<int32_t>(wb));
    CS_HIP(hipGetLastError());
    word_base = dev_alloc(sizeof(int64_t) * (size_t)(words + 1), s);
    c->nbytes = offsets_from_lengths(ptr<const int32_t>(wb), words, ptr<int64_t>(word_base), s);
    a.word_base = ptr<const int64_t>(word_base);
    c->validity = dev_alloc(validity_bytes(rows), s);
    a.validity = ptr<uint64_t>(c->validity);
  } else {
    c->nbytes = rows * W;
    c->null_count = 0;
    c->max_row = W;
    c->max_span64 = std::min<int64_t>(rows, 64) * W;
  }
  c->chars = dev_alloc((size_t)c->nbytes, s);
  a.chars = ptr<uint8_t>(c->chars);
  const bool narrow = rows * W < ((int64_t)1 << 31);
  if (narrow) c->offsets32 = dev_alloc(sizeof(int32_t) * (size_t)(rows + 1), s);
  else c->offsets = dev_alloc(sizeof(int64_t) * (size_t)(rows + 1), s);
  const bool lds = W <= kTsLdsMaxWidth && !cs::cfg("CS_CONVERT_ROWWISE");
  a.lds_stride = lds ? (int)((64 * W + 15) & ~(int64_t)15) : 0;
  const size_t lds_bytes = (size_t)a.lds_stride * 4;
  const unsigned grid = (unsigned)std::min<int64_t>((words + 3) / 4, 32768);
  csdt::ts_dispatch(prog.units, [&](auto u) {
    constexpr int U = decltype(u)::value;
    if (lds_bytes > 48 * 1024) {
      CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ts_format<U, true, int32_t>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
      CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ts_format<U, true, int64_t>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    }
    if (lds && narrow) hipLaunchKernelGGL((k_ts_format<U, true, int32_t>), dim3(grid), dim3(256), lds_bytes, s, a, ptr<int32_t>(c->offsets32));
    else if (lds) hipLaunchKernelGGL((k_ts_format<U, true, int64_t>), dim3(grid), dim3(256), lds_bytes, s, a, ptr<int64_t>(c->offsets));
    else if (narrow) hipLaunchKernelGGL((k_ts_format<U, false, int32_t>), dim3(grid), dim3(256), 0, s, a, ptr<int32_t>(c->offsets32));
    else hipLaunchKernelGGL((k_ts_format<U, false, int64_t>), dim3(grid), dim3(256), 0, s, a, ptr<int64_t>(c->offsets));
    CS_HIP(hipGetLastError());
  });
  CS_HIP(hipStreamSynchronize(s));  // (the caller's buffers are done with)
  note_route(lds ? "lds" : "rows");
  return c.release();
}

}  // namespace

extern "C" {

int cs_timestamp2long(const cs_column* col, const char* format, int units, int64_t* results, int on_device, cs_stream stream,
                      int64_t* count) {
  return guard([&] {
    if (!col) fail(CS_ERR_INVALID_ARG, "null column");
    if (count) *count = -1;  // datetime.cu:325-327: an empty column or no output array returns -1, before the format is read
    if (!results || col->rows == 0) return;
    TsProgram prog;
    compile_or_fail(format, units, &prog, "nvstrings::timestamp2long");
    require_device();
    const int64_t n = run_ts_parse(col, prog, results, on_device, S(stream));
    if (count) *count = n;
  });
}

int cs_long2timestamp(const int64_t* values, int64_t count, int units, const char* format, const uint8_t* nulls, int on_device,
                      cs_stream stream, cs_column** out) {
  return guard([&] {
    if (!out) fail(CS_ERR_INVALID_ARG, "long2timestamp: null output");
    *out = nullptr;
    if (!values || count <= 0) fail(CS_ERR_INVALID_ARG, "nvstrings::long2timestamp values or count invalid");
    TsProgram prog;
    compile_or_fail(format, units, &prog, "nvstrings::long2timestamp");
    require_device();
    *out = run_ts_format(values, count, nulls, on_device, prog, S(stream));
  });
}

}  // extern "C"
