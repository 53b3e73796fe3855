// Numeric and boolean conversions to and from string columns (reference: cpp/src/strings/convert.cu, the members
// hash / stoi / stol / stof / stod / htoi / ip2int / to_bools and itos / ltos / ftos / dtos / int2ip /
// create_from_bools; the timestamp pair is cs_datetime.hip).  The per-row logic is convert_ops.h, shared with the CPU
// harness of tests/test_convert_cpu.py.
//
// Parse ops (string -> one value per row): the tile and row-wise routes of parse_route.h, with the per-row parsers of
// convert_ops.h.
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
#include "parse_route.h"

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

// the value of a row; `valid` false = a null row (0, or `true_string == nullptr` for to_bools)
template <int OP>
struct ConvertParse {
  using T = typename ParseOut<OP>::T;
  const uint8_t* tstr;  // to_bools: the true string on the device (nullptr: none given)
  int tlen;
  __device__ __forceinline__ T operator()(const uint8_t* p, int n, bool valid) const {
    if constexpr (OP == P_BOOL) return valid ? csconv::to_bool_row(p, n, tstr, tlen) : (T)(tstr == nullptr);
    if (!valid) return (T)0;
    if constexpr (OP == P_HASH) return csconv::hash_row(p, n);
    else if constexpr (OP == P_STOI) return csconv::stoi_row(p, n);
    else if constexpr (OP == P_STOL) return csconv::stol_row(p, n);
    else if constexpr (OP == P_STOF) return csconv::stof_row(p, n);
    else if constexpr (OP == P_STOD) return csconv::stod_row(p, n);
    else if constexpr (OP == P_HTOI) return csconv::htoi_row(p, n);
    else return csconv::ip2int_row(p, n);
  }
};

template <int OP>
int parse_entry(const cs_column* col, void* results, int on_device, const char* true_string, cs_stream stream, int64_t* count) {
  return guard([&] {
    if (!col) fail(CS_ERR_INVALID_ARG, "null column");
    if (count) *count = -1;  // convert.cu: an empty column or no output array returns -1
    if (!results || col->rows == 0) return;
    require_device();
    const hipStream_t s = S(stream);
    ConvertParse<OP> parse{};
    Buf tb;
    if (OP == P_BOOL && true_string) {
      parse.tlen = (int)strlen(true_string);
      tb = dev_alloc((size_t)parse.tlen + 1, s);
      CS_HIP(hipMemcpyAsync(tb->p, true_string, (size_t)parse.tlen + 1, hipMemcpyHostToDevice, s));
      parse.tstr = ptr<const uint8_t>(tb);
    }
    const int64_t n = csparse::run_parse(col, parse, results, on_device, !cfg("CS_CONVERT_ROWWISE"), s);
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
    if (csparse::value_valid(a.nulls, r)) {
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
    if (!csparse::value_valid(a.nulls, r)) continue;
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
