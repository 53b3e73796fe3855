// Numeric and boolean conversions to and from string columns (reference: cpp/src/strings/convert.cu, the members
// hash / stoi / stol / stof / stod / htoi / ip2int / to_bools and itos / ltos / ftos / dtos / int2ip /
// create_from_bools; the timestamp pair is cs_datetime.hip).  The per-row logic is convert_ops.h, shared with the CPU
// harness of tests/test_convert_cpu.py.
//
// Parse ops (string -> one value per row), two routes:
//  - tile: a wave stages the bytes of R = 64 / 32 / 16 consecutive rows in LDS with one coalesced prefetch
//    (cstile::issue_chars / stage_chars; R as find_tiles chooses it), each lane parses its row out of LDS and the
//    wave stores its R results side by side.  Taken when every R-row tile of the column fits the prefetch.
//  - rows: a thread per row reading its bytes from memory (columns no tile size fits -- rows of several KB -- and
//    CS_CONVERT_ROWWISE=1).  hash reads every byte of a long row.
//  Both count the non-zero results with one atomic per workgroup (see k_len, cs_array.hip).
// Format ops (value -> string): a length pass (-1 = null), the shared lengths -> offsets scan, a write pass; the
// output has int32 offsets when rows x the op's widest row < 2^31, else int64 (include/custrings_amd.h).
//
// cs_convert.hip is built with -ffp-contract=off (csrc/Makefile): ftos / dtos print other digits when the
// normaliser's `(v - integer) * max_digits - decimal` is fused into an FMA.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "convert_ops.h"
#include "cs_internal.h"
#include "device_utils.h"
#include "tile_utils.h"

using namespace cs;
using namespace csdev;

namespace {

enum ParseOp { P_HASH, P_STOI, P_STOL, P_STOF, P_STOD, P_HTOI, P_IP2INT, P_BOOL };
template <int OP> struct ParseOut;
template <> struct ParseOut<P_HASH> { using T = uint32_t; };
template <> struct ParseOut<P_STOI> { using T = int32_t; };
template <> struct ParseOut<P_STOL> { using T = int64_t; };
template <> struct ParseOut<P_STOF> { using T = float; };
template <> struct ParseOut<P_STOD> { using T = double; };
template <> struct ParseOut<P_HTOI> { using T = uint32_t; };
template <> struct ParseOut<P_IP2INT> { using T = uint32_t; };
template <> struct ParseOut<P_BOOL> { using T = uint8_t; };

struct ParseArgs {
  ColView in;
  void* out;
  const uint8_t* tstr;  // to_bools: the true string on the device (nullptr: none given)
  int tlen;
  unsigned long long* nonzero;
  // tile route
  int rows_per_tile, cap;
  long long ntiles;
};

// the value of a row; `valid` false = a null row (0, or `true_string == nullptr` for to_bools)
template <int OP>
__device__ __forceinline__ typename ParseOut<OP>::T parse_row(const uint8_t* p, int n, bool valid, const ParseArgs& a) {
  using T = typename ParseOut<OP>::T;
  if constexpr (OP == P_BOOL) return valid ? csconv::to_bool_row(p, n, a.tstr, a.tlen) : (T)(a.tstr == nullptr);
  if (!valid) return (T)0;
  if constexpr (OP == P_HASH) return csconv::hash_row(p, n);
  else if constexpr (OP == P_STOI) return csconv::stoi_row(p, n);
  else if constexpr (OP == P_STOL) return csconv::stol_row(p, n);
  else if constexpr (OP == P_STOF) return csconv::stof_row(p, n);
  else if constexpr (OP == P_STOD) return csconv::stod_row(p, n);
  else if constexpr (OP == P_HTOI) return csconv::htoi_row(p, n);
  else return csconv::ip2int_row(p, n);
}

template <int OP>
__global__ void __launch_bounds__(256) k_convert_rows(ParseArgs a) {
  using T = typename ParseOut<OP>::T;
  T* out = static_cast<T*>(a.out);
  long long v = 0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < a.in.rows; r += (int64_t)gridDim.x * kBlock) {
    const bool ok = row_is_valid(a.in.validity, r);
    const int64_t o0 = a.in.offsets[r];
    const T x = parse_row<OP>(a.in.chars + o0, ok ? (int)(a.in.offsets[r + 1] - o0) : 0, ok, a);
    out[r] = x;
    v += x != (T)0;
  }
  const long long t = block_reduce_sum_ll(v);
  if (threadIdx.x == 0 && t) atomicAdd(a.nonzero, (unsigned long long)t);
}

// A wave per R-row tile (persistent: each wave walks a contiguous run of tiles, prefetching the next tile's bytes while
// it parses the current one out of LDS).
template <int OP>
__global__ void __launch_bounds__(256) k_convert_tile(ParseArgs a) {
  using T = typename ParseOut<OP>::T;
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint8_t* lds_in = reinterpret_cast<uint8_t*>(smem) + (size_t)wv * a.cap;
  const ColView& in = a.in;
  const int R = a.rows_per_tile;
  T* out = static_cast<T*>(a.out);
  const long long waves = (long long)gridDim.x * 4;
  const long long per = (a.ntiles + waves - 1) / waves;
  long long tile = ((long long)blockIdx.x * 4 + wv) * per;
  const long long tile_end = min(a.ntiles, tile + per);
  long long v = 0;
  if (tile < tile_end) {
    auto load_offs = [&](long long t) {
      const long long r0 = t * R;
      const int nrows = (int)min((long long)R, in.rows - r0);
      cstile::TileOffs o;
      o.o0 = in.offsets[r0 + min(lane, nrows)];
      o.o1 = in.offsets[r0 + min(lane + 1, nrows)];
      return o;
    };
    cstile::TileOffs cur = load_offs(tile);
    cstile::TileChars pf;
#pragma unroll
    for (int j = 0; j < cstile::kPfChunks; ++j) pf.v[j] = make_uint4(0, 0, 0, 0);
    cstile::issue_chars(in.chars, cstile::rl64(cur.o0, 0), cstile::rl64(cur.o1, 63), lane, pf);
    for (;;) {
      const long long r0 = tile * R;
      const int nrows = (int)min((long long)R, in.rows - r0);
      const long long g0 = cstile::rl64(cur.o0, 0), g1 = cstile::rl64(cur.o1, 63);
      const int lead = (int)((uintptr_t)(in.chars + g0) & 15);
      const int want = (int)(g1 - g0) + lead;  // <= cap: every tile's span fits (checked by the host)
      cstile::stage_chars(lds_in, want, lane, pf);
      const bool in_tile = lane < nrows;
      const bool ok = in_tile && row_is_valid(in.validity, r0 + lane);
      const int rbeg = (int)(cur.o0 - g0) + lead;
      const int n = ok ? (int)(cur.o1 - cur.o0) : 0;
      const bool more = tile + 1 < tile_end;
      if (more) {  // the next tile's bytes travel while this one is parsed
        cur = load_offs(tile + 1);
        cstile::issue_chars(in.chars, cstile::rl64(cur.o0, 0), cstile::rl64(cur.o1, 63), lane, pf);
      }
      cstile::wave_lds_fence();
      if (in_tile) {
        const T x = parse_row<OP>(lds_in + rbeg, n, ok, a);
        out[r0 + lane] = x;
        v += x != (T)0;
      }
      cstile::wave_lds_fence();  // (the LDS is restaged next round)
      if (!more) break;
      ++tile;
    }
  }
  const long long t = block_reduce_sum_ll(v);
  if (threadIdx.x == 0 && t) atomicAdd(a.nonzero, (unsigned long long)t);
}

template <int OP>
bool parse_tiles(const cs_column* col, ParseArgs a, hipStream_t s) {
  if (cs::cfg("CS_CONVERT_ROWWISE")) return false;
  int R = 0;
  for (int r : {64, 32, 16}) {
    if (max_span_rows(col, r, s) + 32 <= cstile::kPfBytes) {
      R = r;
      break;
    }
  }
  if (!R) return false;
  a.rows_per_tile = R;
  a.cap = (int)((max_span_rows(col, R, s) + 48 + 15) & ~(int64_t)15);
  a.ntiles = (col->rows + R - 1) / R;
  const size_t lds = (size_t)a.cap * 4;
  if (lds > 150 * 1024) return false;
  auto kern = &k_convert_tile<OP>;
  if (lds > 48 * 1024)
    CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const unsigned g = resident_grid(reinterpret_cast<const void*>(kern), lds, (a.ntiles + 3) / 4);
  hipLaunchKernelGGL(kern, dim3(g), dim3(256), lds, s, a);
  CS_HIP(hipGetLastError());
  return true;
}

// results to the caller's buffer (device or host); returns the count of non-zero results
template <int OP>
int64_t run_parse(const cs_column* col, void* results, int on_device, const char* true_string, hipStream_t s) {
  using T = typename ParseOut<OP>::T;
  const int64_t rows = col->rows;
  Buf tmp, tb;
  void* d_out = results;
  if (!on_device) {
    tmp = dev_alloc(sizeof(T) * (size_t)rows, s);
    d_out = tmp->p;
  }
  Buf acc = dev_alloc(8, s);
  CS_HIP(hipMemsetAsync(acc->p, 0, 8, s));
  ParseArgs a{};
  a.in = view_of(col);
  a.out = d_out;
  a.nonzero = ptr<unsigned long long>(acc);
  if (OP == P_BOOL && true_string) {
    a.tlen = (int)strlen(true_string);
    tb = dev_alloc((size_t)a.tlen + 1, s);
    CS_HIP(hipMemcpyAsync(tb->p, true_string, (size_t)a.tlen + 1, hipMemcpyHostToDevice, s));
    a.tstr = ptr<const uint8_t>(tb);
  }
  if (parse_tiles<OP>(col, a, s)) {
    note_route("tile");
  } else {
    note_route("rows");
    hipLaunchKernelGGL(k_convert_rows<OP>, dim3(std::min(blocks_for(rows), 8192u)), dim3(kBlock), 0, s, a);
    CS_HIP(hipGetLastError());
  }
  if (!on_device) CS_HIP(hipMemcpyAsync(results, d_out, sizeof(T) * (size_t)rows, hipMemcpyDeviceToHost, s));
  int64_t* host = (int64_t*)pinned_scratch(8);
  CS_HIP(hipMemcpyAsync(host, acc->p, 8, hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  return host[0];
}

template <int OP>
int parse_entry(const cs_column* col, void* results, int on_device, const char* true_string, cs_stream stream, int64_t* count) {
  return guard([&] {
    if (!col) fail(CS_ERR_INVALID_ARG, "null column");
    if (count) *count = -1;  // convert.cu: an empty column or no output array returns -1
    if (!results || col->rows == 0) return;
    require_device();
    const int64_t n = run_parse<OP>(col, results, on_device, true_string, S(stream));
    if (count) *count = n;
  });
}

// ---- format ops --------------------------------------------------------------------------------------------------------
enum FormatOp { F_ITOS, F_LTOS, F_FTOS, F_DTOS, F_INT2IP, F_BOOLS };
template <int OP> struct FormatIn;
template <> struct FormatIn<F_ITOS> { using T = int32_t; };
template <> struct FormatIn<F_LTOS> { using T = int64_t; };
template <> struct FormatIn<F_FTOS> { using T = float; };
template <> struct FormatIn<F_DTOS> { using T = double; };
template <> struct FormatIn<F_INT2IP> { using T = uint32_t; };
template <> struct FormatIn<F_BOOLS> { using T = uint8_t; };

struct FormatArgs {
  const void* values;
  const uint8_t* nulls;  // LSB-first, bit = 1 valid; nullptr = all valid
  int64_t rows;
  const uint8_t* tf;  // from_bools: the true string, then the false string
  int tlen, flen;
};
__device__ __forceinline__ bool value_valid(const uint8_t* nulls, int64_t r) {
  return nulls == nullptr || ((nulls[r >> 3] >> (r & 7)) & 1);
}
// writes row r's text (at most kMaxNumWidth bytes for the numeric formats) to `buf`, returns its length
template <int OP>
__device__ __forceinline__ int format_row(const FormatArgs& a, int64_t r, char* buf) {
  using T = typename FormatIn<OP>::T;
  const T x = static_cast<const T*>(a.values)[r];
  if constexpr (OP == F_ITOS || OP == F_LTOS) return csconv::ltos_row((int64_t)x, buf);
  else if constexpr (OP == F_FTOS) return csconv::ftos_row(x, buf);
  else if constexpr (OP == F_DTOS) return csconv::dtos_row(x, buf);
  else return csconv::int2ip_row((uint32_t)x, buf);
}
template <int OP>
__global__ void k_format_len(FormatArgs a, int32_t* __restrict__ lens) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < a.rows; r += (int64_t)gridDim.x * kBlock) {
    int n = -1;
    if (value_valid(a.nulls, r)) {
      if constexpr (OP == F_BOOLS) {
        n = static_cast<const uint8_t*>(a.values)[r] ? a.tlen : a.flen;
      } else {
        char buf[csconv::kMaxNumWidth + 4];
        n = format_row<OP>(a, r, buf);
      }
    }
    lens[r] = n;
  }
}
template <int OP>
__global__ void k_format_write(FormatArgs a, const int64_t* __restrict__ off, uint8_t* __restrict__ chars) {
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < a.rows; r += (int64_t)gridDim.x * kBlock) {
    if (!value_valid(a.nulls, r)) continue;
    uint8_t* dst = chars + off[r];
    if constexpr (OP == F_BOOLS) {
      const bool t = static_cast<const uint8_t*>(a.values)[r] != 0;
      copy_bytes(dst, t ? a.tf : a.tf + a.tlen, t ? a.tlen : a.flen);
    } else {
      char buf[csconv::kMaxNumWidth + 4];
      const int n = format_row<OP>(a, r, buf);
      for (int i = 0; i < n; ++i) dst[i] = (uint8_t)buf[i];
    }
  }
}

template <int OP>
cs_column* run_format(const void* values, int64_t rows, const uint8_t* nulls, int on_device, const char* t, const char* f,
                      hipStream_t s) {
  using T = typename FormatIn<OP>::T;
  Buf vtmp, ntmp, tf;
  FormatArgs a{};
  a.rows = rows;
  a.values = values;
  a.nulls = nulls;
  if (!on_device) {
    vtmp = dev_alloc(sizeof(T) * (size_t)rows, s);
    CS_HIP(hipMemcpyAsync(vtmp->p, values, sizeof(T) * (size_t)rows, hipMemcpyHostToDevice, s));
    a.values = vtmp->p;
    if (nulls) {
      ntmp = dev_alloc((size_t)(rows + 7) / 8, s);
      CS_HIP(hipMemcpyAsync(ntmp->p, nulls, (size_t)(rows + 7) / 8, hipMemcpyHostToDevice, s));
      a.nulls = ptr<const uint8_t>(ntmp);
    }
  }
  if (OP == F_BOOLS) {
    a.tlen = (int)strlen(t);
    a.flen = (int)strlen(f);
    tf = dev_alloc((size_t)a.tlen + (size_t)a.flen + 1, s);
    CS_HIP(hipMemcpyAsync(tf->p, t, (size_t)a.tlen, hipMemcpyHostToDevice, s));
    CS_HIP(hipMemcpyAsync(static_cast<char*>(tf->p) + a.tlen, f, (size_t)a.flen, hipMemcpyHostToDevice, s));
    a.tf = ptr<const uint8_t>(tf);
  }
  Buf lens = dev_alloc(sizeof(int32_t) * (size_t)rows, s);
  const unsigned grid = std::min(blocks_for(rows), 16384u);
  hipLaunchKernelGGL(k_format_len<OP>, dim3(grid), dim3(kBlock), 0, s, a, ptr<int32_t>(lens));
  CS_HIP(hipGetLastError());
  Built b = column_from_lengths(ptr<int32_t>(lens), rows, a.nulls != nullptr, s);
  hipLaunchKernelGGL(k_format_write<OP>, dim3(grid), dim3(kBlock), 0, s, a, b.off, ptr<uint8_t>(b.col->chars));
  CS_HIP(hipGetLastError());
  // the offset width is decided by the widest row the op can write (rows x max_width < 2^31: int32), not by the bytes
  // written, as a one-pass kernel has to decide it before the first row is placed
  const int64_t max_width = OP == F_BOOLS ? std::max(a.tlen, a.flen) : OP == F_ITOS ? 11 : OP == F_INT2IP ? 15 : csconv::kMaxNumWidth;
  if (rows * max_width < ((int64_t)1 << 31)) prefer_offsets32(b.col.get(), s);
  CS_HIP(hipStreamSynchronize(s));  // (the caller's buffers are done with)
  note_route("rows");
  return b.col.release();
}

template <int OP>
int format_entry(const void* values, int64_t count, const uint8_t* nulls, int on_device, const char* t, const char* f,
                 cs_stream stream, cs_column** out, const char* what) {
  return guard([&] {
    if (!out) fail(CS_ERR_INVALID_ARG, std::string(what) + ": null output");
    *out = nullptr;
    if (!values || count <= 0) fail(CS_ERR_INVALID_ARG, std::string("nvstrings::") + what + " values or count invalid");
    if (OP == F_BOOLS && (!t || !f))
      fail(CS_ERR_INVALID_ARG, "nvstrings::create_from_bools false and true strings must not be null");
    require_device();
    *out = run_format<OP>(values, count, nulls, on_device, t, f, S(stream));
  });
}

}  // namespace

extern "C" {

int cs_hash(const cs_column* col, uint32_t* results, int on_device, cs_stream stream, int64_t* count) {
  return parse_entry<P_HASH>(col, results, on_device, nullptr, stream, count);
}
int cs_stoi(const cs_column* col, int32_t* results, int on_device, cs_stream stream, int64_t* count) {
  return parse_entry<P_STOI>(col, results, on_device, nullptr, stream, count);
}
int cs_stol(const cs_column* col, int64_t* results, int on_device, cs_stream stream, int64_t* count) {
  return parse_entry<P_STOL>(col, results, on_device, nullptr, stream, count);
}
int cs_stof(const cs_column* col, float* results, int on_device, cs_stream stream, int64_t* count) {
  return parse_entry<P_STOF>(col, results, on_device, nullptr, stream, count);
}
int cs_stod(const cs_column* col, double* results, int on_device, cs_stream stream, int64_t* count) {
  return parse_entry<P_STOD>(col, results, on_device, nullptr, stream, count);
}
int cs_htoi(const cs_column* col, uint32_t* results, int on_device, cs_stream stream, int64_t* count) {
  return parse_entry<P_HTOI>(col, results, on_device, nullptr, stream, count);
}
int cs_ip2int(const cs_column* col, uint32_t* results, int on_device, cs_stream stream, int64_t* count) {
  return parse_entry<P_IP2INT>(col, results, on_device, nullptr, stream, count);
}
int cs_to_bools(const cs_column* col, const char* true_string, uint8_t* results, int on_device, cs_stream stream, int64_t* count) {
  return parse_entry<P_BOOL>(col, results, on_device, true_string, stream, count);
}

int cs_itos(const int32_t* values, int64_t count, const uint8_t* nulls, int on_device, cs_stream stream, cs_column** out) {
  return format_entry<F_ITOS>(values, count, nulls, on_device, nullptr, nullptr, stream, out, "itos");
}
int cs_ltos(const int64_t* values, int64_t count, const uint8_t* nulls, int on_device, cs_stream stream, cs_column** out) {
  return format_entry<F_LTOS>(values, count, nulls, on_device, nullptr, nullptr, stream, out, "ltos");
}
int cs_ftos(const float* values, int64_t count, const uint8_t* nulls, int on_device, cs_stream stream, cs_column** out) {
  return format_entry<F_FTOS>(values, count, nulls, on_device, nullptr, nullptr, stream, out, "ftos");
}
int cs_dtos(const double* values, int64_t count, const uint8_t* nulls, int on_device, cs_stream stream, cs_column** out) {
  return format_entry<F_DTOS>(values, count, nulls, on_device, nullptr, nullptr, stream, out, "dtos");
}
int cs_int2ip(const uint32_t* values, int64_t count, const uint8_t* nulls, int on_device, cs_stream stream, cs_column** out) {
  return format_entry<F_INT2IP>(values, count, nulls, on_device, nullptr, nullptr, stream, out, "int2ip");
}
int cs_from_bools(const uint8_t* values, int64_t count, const char* true_string, const char* false_string, const uint8_t* nulls,
                  int on_device, cs_stream stream, cs_column** out) {
  return format_entry<F_BOOLS>(values, count, nulls, on_device, true_string, false_string, stream, out, "create_from_bools");
}

}  // extern "C"
