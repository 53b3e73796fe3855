// url_encode / url_decode (reference: cpp/src/strings/urlencode.cu), translate and fillna (modify.cu:302-489).
// The per-row logic of the three ops that change row lengths is recode_ops.h, shared with the CPU harness of
// tests/test_recode_cpu.py.
//
// url_encode, url_decode and translate run on the sized route (sized_route.h: size pass, scan, write pass; tile and rows,
// CS_RECODE_ROWWISE=1) with the route's own write body: url_encode grows a row up to 3x, translate up to 4x, and a staged
// tile whose output exceeds the out-tile is written to memory by its lanes out of LDS.  translate's 128 ASCII targets
// are the op's shared region.
// fillna sizes its rows from offsets and validity alone and copies spans (a thread per row, as cs_scatter's copy does).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "cs_internal.h"
#include "device_utils.h"
#include "recode_ops.h"
#include "sized_route.h"

using namespace cs;
using namespace csdev;
using csrecode::SafeMask;
using csrecode::Table;

namespace {

struct UrlEncode {
  SafeMask safe;
  __device__ __forceinline__ int64_t size(int64_t, const uint8_t* p, int n) const { return csrecode::encode_size(safe, p, n); }
  __device__ __forceinline__ void write(int64_t, const uint8_t* p, int n, uint8_t* o) const { csrecode::encode_write(safe, p, n, o); }
};
struct UrlDecode {
  __device__ __forceinline__ int64_t size(int64_t, const uint8_t* p, int n) const { return csrecode::decode_size(p, n); }
  __device__ __forceinline__ void write(int64_t, const uint8_t* p, int n, uint8_t* o) const { csrecode::decode_write(p, n, o); }
};
struct Translate {
  Table tab;  // (device memory)
  // the workgroup's copy of the 128 ASCII targets
  static constexpr int kSharedBytes = csrecode::kAsciiKeys * (int)sizeof(uint32_t);
  __device__ __forceinline__ void stage(uint8_t* lds, int tid) const {
    if (tid < csrecode::kAsciiKeys) reinterpret_cast<uint32_t*>(lds)[tid] = tab.ascii[tid];
  }
  __device__ __forceinline__ Table staged(const uint8_t* shared) const {
    Table t = tab;
    t.ascii = reinterpret_cast<const uint32_t*>(shared);
    return t;
  }
  __device__ __forceinline__ int64_t size(int64_t, const uint8_t* p, int n) const { return csrecode::translate_size(tab, p, n); }
  __device__ __forceinline__ int64_t size(int64_t, const uint8_t* p, int n, const uint8_t* shared) const {
    return csrecode::translate_size(staged(shared), p, n);
  }
  __device__ __forceinline__ void write(int64_t, const uint8_t* p, int n, uint8_t* o) const { csrecode::translate_write(tab, p, n, o); }
  __device__ __forceinline__ void write(int64_t, const uint8_t* p, int n, uint8_t* o, const uint8_t* shared) const {
    csrecode::translate_write(staged(shared), p, n, o);
  }
};

template <class Op>
cs_column* run_recode(const cs_column* col, const Op& op, hipStream_t s) {
  if (col->rows == 0) return make_all_null(0, s);
  return cssized::run_sized(col, op, "CS_RECODE_ROWWISE", "k_recode_size", "k_recode_write", s);
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

}  // namespace

extern "C" {

int cs_url_encode(const cs_column* col, cs_stream stream, cs_column** out) {
  return column_entry(col, out, [&] { return run_recode(col, UrlEncode{csrecode::url_safe_mask()}, S(stream)); });
}

int cs_url_decode(const cs_column* col, cs_stream stream, cs_column** out) {
  return column_entry(col, out, [&] { return run_recode(col, UrlDecode{}, S(stream)); });
}

int cs_translate(const cs_column* col, const uint32_t* from, const uint32_t* to, int n, cs_stream stream, cs_column** out) {
  return column_entry(col, out, [&] {
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
    Translate a{};
    a.tab.ascii = ptr<const uint32_t>(d);
    a.tab.keys = a.tab.ascii + csrecode::kAsciiKeys;
    a.tab.vals = a.tab.keys + nk;
    a.tab.nkeys = (int)nk;
    cs_column* c = run_recode(col, a, s);
    CS_HIP(hipStreamSynchronize(s));  // (the table is done with)
    return c;
  });
}

int cs_fillna(const cs_column* col, const char* str, cs_stream stream, cs_column** out) {
  return column_entry(col, out, [&] {
    if (!str) fail(CS_ERR_INVALID_ARG, "nvstrings::fillna parameter cannot be null");
    return run_fillna(col, nullptr, str, S(stream));
  });
}

int cs_fillna_column(const cs_column* col, const cs_column* repl, cs_stream stream, cs_column** out) {
  return column_entry(col, out, [&] {
    if (!repl) fail(CS_ERR_INVALID_ARG, "nvstrings::fillna parameter cannot be null");
    if (repl->rows != col->rows) fail(CS_ERR_INVALID_ARG, "nvstrings::fillna parameter must have the same number of strings");
    return run_fillna(col, repl, nullptr, S(stream));
  });
}

}  // extern "C"
