// The character-type predicates of NVStrings (reference: cpp/src/strings/attrs.cu:115-438): isalnum / isalpha / isdigit /
// isspace / isdecimal / isnumeric / islower / isupper and is_empty -- one byte a row, the count of true rows returned.
// The per-row logic is chartype_ops.h (pred_row), shared with the CPU harness of tests/test_chartype_cpu.py.
//
// The eight predicates that read characters are parsers of parse_route.h (T = uint8_t, the route's non-zero counter is the
// count of trues): the tile route stages R rows in LDS and a lane walks its row, the row-wise route (CS_CONVERT_ROWWISE=1,
// and columns no tile fits) reads the row from memory.  The ASCII half of a predicate is a 128-bit membership mask made on
// the host from the table's first 128 entries and carried in the kernel arguments (wave-uniform: scalar registers); only a
// byte >= 0x80 decodes a character and reads the 64 KB flag table.  The walk stops at the first character that decides
// the row.
// is_empty reads offsets and validity only: one kernel on a capped grid (the shape of k_len, cs_array.hip), whatever the
// route switch says; it reports the route "rows".
#include <hip/hip_runtime.h>

#include "chartype_ops.h"
#include "cs_internal.h"
#include "device_utils.h"
#include "parse_route.h"

using namespace cs;
using namespace csdev;

namespace {

struct PredParse {
  using T = uint8_t;
  cschr::PredSpec spec;
  __device__ __forceinline__ T operator()(const uint8_t* p, int n, bool valid) const {
    return (T)(valid && cschr::pred_row(p, n, spec));
  }
};

__global__ void __launch_bounds__(256) k_is_empty(ColView in, uint8_t* __restrict__ out, unsigned long long* __restrict__ total) {
  long long v = 0;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < in.rows; r += (int64_t)gridDim.x * kBlock) {
    const bool e = !row_is_valid(in.validity, r) || in.offsets[r + 1] == in.offsets[r];
    out[r] = (uint8_t)e;
    v += e;
  }
  const long long t = block_reduce_sum_ll(v);
  if (threadIdx.x == 0 && t) atomicAdd(total, (unsigned long long)t);
}

int64_t run_is_empty(const cs_column* col, uint8_t* results, int on_device, hipStream_t s) {
  const ResultsOut res(results, (size_t)col->rows, on_device, s);
  const Buf acc = zeroed_count(s);
  hipLaunchKernelGGL(k_is_empty, dim3(std::min(blocks_for(col->rows), 8192u)), dim3(kBlock), 0, s, view_of(col),
                     static_cast<uint8_t*>(res.dev), ptr<unsigned long long>(acc));
  CS_HIP(hipGetLastError());
  note_route("rows");
  res.copy_back(s);
  return read_count(acc, s);
}

}  // namespace

extern "C" {

int cs_chartype(const cs_column* col, int pred, uint8_t* results, int on_device, cs_stream stream, int64_t* count) {
  return guard([&] {
    if (!col || pred < 0 || pred >= cschr::P_COUNT) fail(CS_ERR_INVALID_ARG, "chartype: bad arguments");
    if (count) *count = 0;  // attrs.cu: a column of no rows or no output array returns 0
    if (!results || col->rows == 0) return;
    require_device();
    const hipStream_t s = S(stream);
    int64_t n;
    if (pred == cschr::P_EMPTY) n = run_is_empty(col, results, on_device, s);
    else n = csparse::run_parse(col, PredParse{cschr::make_pred(pred, h_unicode_flags(), d_unicode_flags())}, results, on_device,
                                   !cfg("CS_CONVERT_ROWWISE"), s);
    if (count) *count = n;
  });
}
int cs_isalnum(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count) {
  return cs_chartype(col, cschr::P_ALNUM, results, on_device, stream, count);
}
int cs_isalpha(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count) {
  return cs_chartype(col, cschr::P_ALPHA, results, on_device, stream, count);
}
int cs_isdigit(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count) {
  return cs_chartype(col, cschr::P_DIGIT, results, on_device, stream, count);
}
int cs_isspace(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count) {
  return cs_chartype(col, cschr::P_SPACE, results, on_device, stream, count);
}
int cs_isdecimal(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count) {
  return cs_chartype(col, cschr::P_DECIMAL, results, on_device, stream, count);
}
int cs_isnumeric(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count) {
  return cs_chartype(col, cschr::P_NUMERIC, results, on_device, stream, count);
}
int cs_islower(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count) {
  return cs_chartype(col, cschr::P_LOWER, results, on_device, stream, count);
}
int cs_isupper(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count) {
  return cs_chartype(col, cschr::P_UPPER, results, on_device, stream, count);
}
int cs_is_empty(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count) {
  return cs_chartype(col, cschr::P_EMPTY, results, on_device, stream, count);
}

}  // extern "C"
