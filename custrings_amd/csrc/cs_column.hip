// The column object: construction / export (NVStrings.cu:74-153,402-544; NVStringsImpl.cu:126-444; attrs.cu:72-112),
// the builder of output columns from per-row lengths (cs_internal.h: Built), row-wise concatenation, slices, HIP IPC
// and the digest.  Memory comes from the pool (cs_core.hip), offsets from the scan (cs_scan.hip).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <mutex>

#include "cs_internal.h"
#include "cs_synth_spec.h"
#include "device_utils.h"

using namespace csdev;

namespace cs {

cs_column* make_all_null(int64_t rows, hipStream_t s) {
  auto* c = new cs_column;
  c->rows = rows;
  c->nbytes = 0;
  c->null_count = rows;
  c->chars = dev_alloc(0, s);
  c->offsets = dev_alloc(sizeof(int64_t) * (rows + 1), s);
  CS_HIP(hipMemsetAsync(c->offsets->p, 0, sizeof(int64_t) * (rows + 1), s));
  if (rows) {
    c->validity = dev_alloc(validity_bytes(rows), s);
    CS_HIP(hipMemsetAsync(c->validity->p, 0, validity_bytes(rows), s));
  }
  return c;
}

// ------------------------------------------------------- ingest / export ----
__global__ void k_widen_offsets(const int32_t* __restrict__ in, int64_t n, int64_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = in[i];
}
__global__ void k_narrow_offsets(const int64_t* __restrict__ in, int64_t n, int32_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = (int32_t)in[i];
}
}  // namespace cs
// int64 form of a column born with int32 offsets, built once (any thread) and kept
static std::mutex g_widen_mu;
const int64_t* cs_column::d_offsets() const {
  std::lock_guard<std::mutex> lk(g_widen_mu);
  if (!offsets && offsets32) {
    cs::Buf o64 = cs::dev_alloc(sizeof(int64_t) * (rows + 1), nullptr);
    hipLaunchKernelGGL(cs::k_widen_offsets, dim3(cs::blocks_for(rows + 1)), dim3(kBlock), 0, nullptr, d_offsets32(), rows + 1,
                       cs::ptr<int64_t>(o64));
    CS_HIP(hipGetLastError());
    CS_HIP(hipStreamSynchronize(nullptr));
    offsets = o64;
  }
  return cs::ptr<const int64_t>(offsets);
}
void cs_column::share_extents_with(cs_column* o, hipStream_t s) const {
  std::lock_guard<std::mutex> lk(g_widen_mu);
  o->offsets = cs::dev_owned(offsets, s);
  o->offsets32 = cs::dev_owned(offsets32, s);
}
cs_column* cs::share_column(const cs_column* in, hipStream_t s) {
  auto o = std::make_unique<cs_column>(*in);
  in->share_extents_with(o.get(), s);
  if (in->chars && in->chars->borrowed) {
    o->chars = cs::dev_owned(in->chars, s);
    o->virt = nullptr;  // (views over the input's chars: built again on first use)
    o->virt_state = 0;
    o->odd = nullptr;
  }
  return o.release();
}
namespace cs {

// ---------------------------------------------- columns from per-row lengths --
// The builder of output columns from per-row lengths (cs_internal.h: Built): offsets, nulls, the chars
// buffer; the copy kernel uses the int64 offsets (always produced: the scan writes int64) -- the narrow
// form (int32 when the chars stay below 2 GiB) is derived.
__global__ void k_narrow(const int64_t* __restrict__ in, int64_t n, int32_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) out[i] = (int32_t)in[i];
}
Built::Built(int64_t rows, Nulls nulls, hipStream_t s) : col(std::make_unique<cs_column>()), nulls_(nulls), s_(s) {
  col->rows = rows;
  if (nulls == Nulls::none) col->null_count = 0;
}
Built::Built(const cs_column* like, hipStream_t s) : Built(like->rows, Nulls::shared, s) {
  col->validity = like->validity;
  col->null_count = like->null_count;
}
int64_t Built::scan(const int32_t* lens, Buf block_sums) {
  cs_column* c = col.get();
  lens_ = lens;
  // (an op that allocates its lengths after the offsets has set them already: the pool sees the order it always saw)
  if (!c->offsets) c->offsets = dev_alloc(sizeof(int64_t) * (size_t)(c->rows + 1), s_);
  int64_t* o = ptr<int64_t>(c->offsets);
  LenMeta meta;  // (the longest row and the largest 64-row span come out of the same pass: no op on the new column pays for them)
  c->nbytes = nulls_ == Nulls::fused ? offsets_and_validity_from_lengths(lens, c->rows, o, &c->validity, s_, &meta)
                                     : offsets_from_lengths(lens, c->rows, o, s_, block_sums, &meta);
  meta.give(c);
  off = o;
  return c->nbytes;
}
uint8_t* Built::alloc_chars() {
  col->chars = dev_alloc((size_t)col->nbytes, s_);
  if (nulls_ == Nulls::separate) col->validity = validity_from_lengths(lens_, col->rows, s_);
  return chars = ptr<uint8_t>(col->chars);
}
Built column_from_lengths(const int32_t* lens, int64_t rows, bool any_null_possible, hipStream_t s) {
  Built b(rows, any_null_possible ? Nulls::separate : Nulls::none, s);
  b.scan(lens);
  b.alloc_chars();
  return b;
}
void release_columns(std::vector<std::unique_ptr<cs_column>>& cols, cs_column*** out_cols, int* ncols_out) {
  cs_column** arr = (cs_column**)malloc(sizeof(cs_column*) * cols.size());
  if (!arr) fail(CS_ERR_ALLOC, "host allocation failed");
  for (size_t k = 0; k < cols.size(); ++k) arr[k] = cols[k].release();
  *out_cols = arr;
  *ncols_out = (int)cols.size();
}
// (after the copy kernel ran) keep the narrow offsets only, when they suffice
void prefer_offsets32(cs_column* c, hipStream_t s) {
  if (c->nbytes >= ((int64_t)1 << 31) || c->rows == 0) return;
  Buf o32 = dev_alloc(sizeof(int32_t) * (c->rows + 1), s);
  hipLaunchKernelGGL(k_narrow, dim3(blocks_for(c->rows + 1)), dim3(kBlock), 0, s, ptr<const int64_t>(c->offsets), c->rows + 1,
                     ptr<int32_t>(o32));
  CS_HIP(hipStreamSynchronize(s));
  c->offsets32 = o32;
  c->offsets = nullptr;
}

// a null row contributes no bytes: clamp its extent to zero while copying
// (NVStringsImpl.cu:408-432 skips rows whose validity bit is clear)
__global__ void k_lengths_from_offsets(cs::ColView in, int32_t* __restrict__ lens) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= in.rows) return;
  lens[r] = row_is_valid(in.validity, r) ? (int32_t)(in.offsets[r + 1] - in.offsets[r]) : -1;
}
__global__ void k_gather_rows(cs::ColView in, const int64_t* __restrict__ out_off,
                              uint8_t* __restrict__ out_chars) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= in.rows || !row_is_valid(in.validity, r)) return;
  const uint8_t* src = in.chars + in.offsets[r];
  uint8_t* dst = out_chars + out_off[r];
  int n = (int)(in.offsets[r + 1] - in.offsets[r]);
  for (int i = 0; i < n; ++i) dst[i] = src[i];
}
__global__ void k_null_bitarray(cs::ColView in, int empty_is_null, uint8_t* __restrict__ bits,
                                unsigned long long* __restrict__ nulls) {
  // one thread per output byte (NVStrings.cu:512-527)
  int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int64_t nb = (in.rows + 7) / 8;
  int cleared = 0;
  if (b < nb) {
    unsigned byte = 0;
    for (int i = 0; i < 8; ++i) {
      int64_t r = b * 8 + i;
      if (r >= in.rows) break;
      bool ok = row_is_valid(in.validity, r);
      if (ok && empty_is_null) ok = in.offsets[r + 1] > in.offsets[r];
      if (ok) byte |= 1u << i;
      else ++cleared;
    }
    bits[b] = (uint8_t)byte;
  }
  long long t = block_reduce_sum(cleared);
  if (threadIdx.x == 0 && t) atomicAdd(nulls, (unsigned long long)t);
}
__global__ void k_digest(cs::ColView in, unsigned long long* __restrict__ out) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned long long h = 0;
  if (r < in.rows) {
    bool ok = row_is_valid(in.validity, r);
    int n = ok ? (int)(in.offsets[r + 1] - in.offsets[r]) : 0;
    h = cs_digest_row((uint64_t)r, ok ? in.chars + in.offsets[r] : nullptr, n, ok);
  }
  for (int d = 32; d > 0; d >>= 1) h += __shfl_xor(h, d, 64);
  if ((threadIdx.x & 63) == 0 && h) atomicAdd(out, h);
}

__global__ void k_slice(cs::ColView in, int64_t first, int64_t rows, int64_t* __restrict__ out_off,
                        uint8_t* __restrict__ out_valid) {
  int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t base = in.offsets[first];
  if (i <= rows) out_off[i] = in.offsets[first + i] - base;
  if (out_valid) {
    bool ok = i < rows && row_is_valid(in.validity, first + i);
    store_validity_word(out_valid, i - (threadIdx.x & 63), ok, rows);
  }
}

static void copy_in(void* dst, const void* src, size_t bytes, int on_device, hipStream_t s) {
  if (!bytes) return;
  CS_HIP(hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
}
static void copy_out(void* dst, const void* src, size_t bytes, int on_device, hipStream_t s) {
  if (!bytes) return;
  CS_HIP(hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
}

// the caller's (rows + 7) / 8 mask bytes in zeroed 8-byte words: the engine writes / reads validity by the word
static Buf ingest_validity(const uint8_t* validity, int64_t rows, int on_device, hipStream_t s) {
  Buf v = dev_alloc(validity_bytes(rows), s);
  CS_HIP(hipMemsetAsync(v->p, 0, validity_bytes(rows), s));
  copy_in(v->p, validity, (size_t)((rows + 7) / 8), on_device, s);
  return v;
}
// sets *flag when a null row has a non-empty extent
__global__ void k_null_rows_hold_bytes(cs::ColView in, unsigned* __restrict__ flag) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool bad = false;
  if (r < in.rows) bad = !row_is_valid(in.validity, r) && in.offsets[r + 1] != in.offsets[r];
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
// Turns an ingested (chars, offsets, validity) triple into a canonical column:
// offsets[0] == 0, null rows have zero extent, chars packed.
static cs_column* canonicalise(Buf chars, Buf offs, Buf validity, int64_t rows, bool has_validity, hipStream_t s) {
  auto* c = new cs_column;
  std::unique_ptr<cs_column> guard_c(c);
  c->rows = rows;
  if (!has_validity) {
    // offsets may start at a non-zero base: rebase by gathering only when needed
    int64_t* host = (int64_t*)pinned_scratch(16);
    CS_HIP(hipMemcpyAsync(host, offs->p, 8, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(host + 1, ptr<int64_t>(offs) + rows, 8, hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    if (host[0] == 0) {
      c->chars = chars;
      c->offsets = offs;
      c->nbytes = host[1];
      c->null_count = 0;
      return guard_c.release();
    }
  }
  ColView in{ptr<const uint8_t>(chars), ptr<const int64_t>(offs), ptr<const uint8_t>(validity), rows};
  if (has_validity) {
    // The usual Arrow column is canonical already (offsets from 0, nothing stored under a null):
    // one pass over offsets + bitmask decides, and the ingested buffers are then used as they are.
    Buf flag = dev_alloc(sizeof(unsigned), s);
    CS_HIP(hipMemsetAsync(flag->p, 0, sizeof(unsigned), s));
    hipLaunchKernelGGL(k_null_rows_hold_bytes, dim3(blocks_for(rows)), dim3(kBlock), 0, s, in, ptr<unsigned>(flag));
    int64_t* host = (int64_t*)pinned_scratch(24);
    CS_HIP(hipMemcpyAsync(host, offs->p, 8, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(host + 1, ptr<int64_t>(offs) + rows, 8, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(host + 2, flag->p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    if (host[0] == 0 && (unsigned)host[2] == 0) {
      c->chars = chars;
      c->offsets = offs;
      c->validity = validity;
      c->nbytes = host[1];
      return guard_c.release();
    }
  }
  Buf lens = dev_alloc(sizeof(int32_t) * rows, s);
  hipLaunchKernelGGL(k_lengths_from_offsets, dim3(blocks_for(rows)), dim3(kBlock), 0, s, in, ptr<int32_t>(lens));
  c->offsets = dev_alloc(sizeof(int64_t) * (rows + 1), s);
  c->nbytes = offsets_from_lengths(ptr<int32_t>(lens), rows, ptr<int64_t>(c->offsets), s);
  c->chars = dev_alloc((size_t)c->nbytes, s);
  hipLaunchKernelGGL(k_gather_rows, dim3(blocks_for(rows)), dim3(kBlock), 0, s, in, c->d_offsets(), ptr<uint8_t>(c->chars));
  c->validity = validity;
  return guard_c.release();
}

__global__ void k_gather_rows_at(cs::ColView in, const int64_t* __restrict__ out_off,
                                 uint8_t* __restrict__ out_chars) {
  // out_off is already advanced to this input's first output row
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= in.rows || !row_is_valid(in.validity, r)) return;
  const uint8_t* src = in.chars + in.offsets[r];
  uint8_t* dst = out_chars + out_off[r];
  int n = (int)(in.offsets[r + 1] - in.offsets[r]);
  for (int i = 0; i < n; ++i) dst[i] = src[i];
}

cs_column* concat_columns(const std::vector<const cs_column*>& cols, hipStream_t s) {
  int64_t rows = 0;
  bool any_mask = false;
  for (auto* c : cols) {
    rows += c->rows;
    any_mask |= c->validity != nullptr;
  }
  if (rows == 0) return make_all_null(0, s);
  Built b(rows, any_mask ? Nulls::separate : Nulls::none, s);
  Buf lens = dev_alloc(sizeof(int32_t) * rows, s);
  int64_t base = 0;
  for (auto* c : cols) {
    if (c->rows)
      hipLaunchKernelGGL(k_lengths_from_offsets, dim3(blocks_for(c->rows)), dim3(kBlock), 0, s, view_of(c),
                         ptr<int32_t>(lens) + base);
    base += c->rows;
  }
  b.scan(ptr<int32_t>(lens));
  b.alloc_chars();
  base = 0;
  for (auto* c : cols) {
    if (c->rows)
      hipLaunchKernelGGL(k_gather_rows_at, dim3(blocks_for(c->rows)), dim3(kBlock), 0, s, view_of(c),
                         b.off + base, b.chars);
    base += c->rows;
  }
  CS_HIP(hipStreamSynchronize(s));
  return b.col.release();
}

}  // namespace cs

using namespace cs;

extern "C" {

int cs_column_from_host_strings(const char* const* strs, int64_t rows, cs_stream stream, cs_column** out) {
  return guard([&] {
    if (!out || (rows > 0 && !strs) || rows < 0) fail(CS_ERR_INVALID_ARG, "create_from_array: bad arguments");
    require_device();
    hipStream_t s = S(stream);
    // one staging buffer, one H2D copy (NVStringsImpl.cu:126-206)
    std::vector<int64_t> off((size_t)rows + 1, 0);
    bool any_null = false;
    for (int64_t r = 0; r < rows; ++r) {
      size_t n = strs[r] ? strlen(strs[r]) : 0;
      any_null |= strs[r] == nullptr;
      off[r + 1] = off[r] + (int64_t)n;
    }
    std::vector<uint8_t> chars((size_t)off[rows]);
    std::vector<uint8_t> valid;
    if (any_null) valid.assign(validity_bytes(rows), 0);
    for (int64_t r = 0; r < rows; ++r) {
      if (!strs[r]) continue;
      memcpy(chars.data() + off[r], strs[r], (size_t)(off[r + 1] - off[r]));
      if (any_null) valid[r >> 3] |= (uint8_t)(1u << (r & 7));
    }
    auto* c = new cs_column;
    std::unique_ptr<cs_column> holder(c);
    c->rows = rows;
    c->nbytes = off[rows];
    c->chars = dev_alloc(chars.size(), s);
    c->offsets = dev_alloc(sizeof(int64_t) * (rows + 1), s);
    copy_in(c->chars->p, chars.data(), chars.size(), 0, s);
    copy_in(c->offsets->p, off.data(), sizeof(int64_t) * (rows + 1), 0, s);
    if (any_null) {
      c->validity = dev_alloc(valid.size(), s);
      copy_in(c->validity->p, valid.data(), valid.size(), 0, s);
    } else {
      c->null_count = 0;
    }
    CS_HIP(hipStreamSynchronize(s));  // staging vectors die here
    *out = holder.release();
  });
}

int cs_column_from_offsets32(const char* chars, int64_t rows, const int32_t* offsets,
                             const uint8_t* validity, int on_device, cs_stream stream, cs_column** out) {
  return guard([&] {
    if (!out || rows < 0 || (rows > 0 && (!offsets))) fail(CS_ERR_INVALID_ARG, "create_from_offsets: bad arguments");
    require_device();
    hipStream_t s = S(stream);
    if (rows == 0) {
      *out = make_all_null(0, s);
      return;
    }
    Buf o32 = dev_alloc(sizeof(int32_t) * (rows + 1), s);
    copy_in(o32->p, offsets, sizeof(int32_t) * (rows + 1), on_device, s);
    int32_t ends[2];
    CS_HIP(hipMemcpyAsync(&ends[0], ptr<int32_t>(o32), 4, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(&ends[1], ptr<int32_t>(o32) + rows, 4, hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    if (ends[1] < ends[0] || ends[0] < 0) fail(CS_ERR_INVALID_ARG, "create_from_offsets: offsets are not ascending");
    int64_t span = ends[1];
    if (span > 0 && !chars) fail(CS_ERR_INVALID_ARG, "create_from_offsets: chars is null");
    Buf o64 = dev_alloc(sizeof(int64_t) * (rows + 1), s);
    hipLaunchKernelGGL(k_widen_offsets, dim3(blocks_for(rows + 1)), dim3(kBlock), 0, s,
                       ptr<int32_t>(o32), rows + 1, ptr<int64_t>(o64));
    Buf ch = dev_alloc((size_t)span, s);
    copy_in(ch->p, chars, (size_t)span, on_device, s);
    Buf v;
    if (validity) v = ingest_validity(validity, rows, on_device, s);
    *out = canonicalise(ch, o64, v, rows, validity != nullptr, s);
  });
}

int cs_column_from_offsets64(const uint8_t* chars, int64_t rows, const int64_t* offsets,
                             const uint8_t* validity, int on_device, int copy, cs_stream stream,
                             cs_column** out) {
  return guard([&] {
    if (!out || rows < 0 || (rows > 0 && !offsets)) fail(CS_ERR_INVALID_ARG, "from_offsets64: bad arguments");
    if (!copy && !on_device) fail(CS_ERR_INVALID_ARG, "from_offsets64: zero-copy needs device buffers");
    require_device();
    hipStream_t s = S(stream);
    if (rows == 0) {
      *out = make_all_null(0, s);
      return;
    }
    int64_t ends[2];
    if (on_device) {
      CS_HIP(hipMemcpyAsync(&ends[0], offsets, 8, hipMemcpyDeviceToHost, s));
      CS_HIP(hipMemcpyAsync(&ends[1], offsets + rows, 8, hipMemcpyDeviceToHost, s));
      CS_HIP(hipStreamSynchronize(s));
    } else {
      ends[0] = offsets[0];
      ends[1] = offsets[rows];
    }
    if (ends[1] < ends[0] || ends[0] < 0) fail(CS_ERR_INVALID_ARG, "from_offsets64: offsets are not ascending");
    if (!copy) {
      // borrowed buffers must already be canonical (offsets[0]==0; null rows empty)
      if (ends[0] != 0) fail(CS_ERR_INVALID_ARG, "from_offsets64: zero-copy needs offsets[0]==0");
      auto* c = new cs_column;
      c->rows = rows;
      c->nbytes = ends[1];
      c->chars = dev_wrap(chars, (size_t)ends[1]);
      c->offsets = dev_wrap(offsets, sizeof(int64_t) * (rows + 1));
      if (validity) c->validity = ingest_validity(validity, rows, 1, s);  // (the small mask is copied)
      else c->null_count = 0;
      *out = c;
      return;
    }
    Buf o64 = dev_alloc(sizeof(int64_t) * (rows + 1), s);
    copy_in(o64->p, offsets, sizeof(int64_t) * (rows + 1), on_device, s);
    Buf ch = dev_alloc((size_t)ends[1], s);
    copy_in(ch->p, chars, (size_t)ends[1], on_device, s);
    Buf v;
    if (validity) v = ingest_validity(validity, rows, on_device, s);
    cs_column* c = canonicalise(ch, o64, v, rows, validity != nullptr, s);
    if (!on_device) CS_HIP(hipStreamSynchronize(s));
    *out = c;
  });
}

int cs_column_concat(const cs_column* const* cols, int n, cs_stream stream, cs_column** out) {
  return guard([&] {
    if (!out || n < 0 || (n > 0 && !cols)) fail(CS_ERR_INVALID_ARG, "create_from_strings: bad arguments");
    require_device();
    std::vector<const cs_column*> v;
    for (int i = 0; i < n; ++i) {
      if (!cols[i]) fail(CS_ERR_INVALID_ARG, "create_from_strings: null column");
      v.push_back(cols[i]);
    }
    *out = concat_columns(v, S(stream));
  });
}

int cs_column_slice(const cs_column* col, int64_t first, int64_t rows, cs_stream stream, cs_column** out) {
  return guard([&] {
    if (!col || !out || first < 0 || rows < 0 || first + rows > col->rows)
      fail(CS_ERR_INVALID_ARG, "sublist: row range out of bounds");
    require_device();
    hipStream_t s = S(stream);
    if (rows == 0) {
      *out = make_all_null(0, s);
      return;
    }
    auto c = std::make_unique<cs_column>();
    c->rows = rows;
    c->offsets = dev_alloc(sizeof(int64_t) * (rows + 1), s);
    if (col->validity) c->validity = dev_alloc(validity_bytes(rows), s);
    else c->null_count = 0;
    hipLaunchKernelGGL(k_slice, dim3(blocks_for(rows + 1)), dim3(kBlock), 0, s, view_of(col), first, rows,
                       ptr<int64_t>(c->offsets), ptr<uint8_t>(c->validity));
    int64_t* host = (int64_t*)pinned_scratch(16);
    CS_HIP(hipMemcpyAsync(host, col->d_offsets() + first, 8, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(host + 1, col->d_offsets() + first + rows, 8, hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    c->nbytes = host[1] - host[0];
    c->chars = dev_alloc((size_t)c->nbytes, s);
    if (c->nbytes)
      CS_HIP(hipMemcpyAsync(c->chars->p, col->d_chars() + host[0], (size_t)c->nbytes, hipMemcpyDeviceToDevice, s));
    *out = c.release();
  });
}

// ---- HIP IPC (NVStrings::create_ipc_transfer / create_from_ipc; ipc_transfer.h:31-107) ----
namespace {
void ipc_handle_of(const Buf& b, unsigned char* out) {
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "cs_ipc_column carries 64-byte handles");
  hipIpcMemHandle_t h;
  CS_HIP(hipIpcGetMemHandle(&h, b->p));
  memcpy(out, &h, sizeof(h));
}
Buf ipc_open(const unsigned char* handle, size_t bytes) {
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof(h));
  void* p = nullptr;
  CS_HIP(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
  auto b = std::make_shared<DevBuf>();
  b->p = p;
  b->bytes = bytes;
  b->capacity = 0;
  b->ipc_mapped = true;
  return b;
}
void export_column(const cs_column* col, cs_ipc_column* out) {
  memset(out, 0, sizeof(*out));
  for (const Buf& b : {col->chars, col->offsets, col->offsets32, col->validity})
    if (b && b->p && b->capacity == 0) fail(CS_ERR_INVALID_ARG, "ipc export: the column wraps memory it does not own (zero-copy ingest): copy it first");
  out->rows = col->rows;
  out->nbytes = col->nbytes;
  out->null_count = col->null_count;
  out->device = bound_device();
  if (col->chars && col->chars->p) ipc_handle_of(col->chars, out->chars);
  else out->nbytes = 0;
  if (col->offsets32) {
    out->offset_width = 4;
    ipc_handle_of(col->offsets32, out->offsets);
  } else {
    out->offset_width = 8;
    (void)col->d_offsets();
    ipc_handle_of(col->offsets, out->offsets);
  }
  if (col->validity && col->validity->p) {
    out->has_validity = 1;
    ipc_handle_of(col->validity, out->validity);
  }
}
cs_column* import_column(const cs_ipc_column* ipc) {
  if (ipc->rows < 0 || ipc->nbytes < 0 || (ipc->offset_width != 4 && ipc->offset_width != 8)) fail(CS_ERR_INVALID_ARG, "ipc import: malformed transfer record");
  auto c = std::make_unique<cs_column>();
  c->rows = ipc->rows;
  c->nbytes = ipc->nbytes;
  c->null_count = ipc->null_count;
  if (ipc->nbytes > 0) c->chars = ipc_open(ipc->chars, (size_t)ipc->nbytes);
  if (ipc->offset_width == 4) c->offsets32 = ipc_open(ipc->offsets, sizeof(int32_t) * (size_t)(ipc->rows + 1));
  else c->offsets = ipc_open(ipc->offsets, sizeof(int64_t) * (size_t)(ipc->rows + 1));
  if (ipc->has_validity) c->validity = ipc_open(ipc->validity, validity_bytes(ipc->rows));
  return c.release();
}
}  // namespace

int cs_column_ipc_export(const cs_column* col, cs_ipc_column* out) {
  return guard([&] {
    if (!col || !out) fail(CS_ERR_INVALID_ARG, "ipc export: null argument");
    require_device();
    CS_HIP(hipDeviceSynchronize());  // the importer must find finished buffers
    export_column(col, out);
  });
}
int cs_column_ipc_import(const cs_ipc_column* ipc, cs_column** out) {
  return guard([&] {
    if (!ipc || !out) fail(CS_ERR_INVALID_ARG, "ipc import: null argument");
    require_device();
    *out = import_column(ipc);
  });
}
int cs_category_ipc_export(const cs_category* cat, cs_ipc_category* out) {
  return guard([&] {
    if (!cat || !out) fail(CS_ERR_INVALID_ARG, "ipc export: null argument");
    require_device();
    CS_HIP(hipDeviceSynchronize());
    memset(out, 0, sizeof(*out));
    export_column(cat->keys.get(), &out->keys);
    out->rows = cat->rows;
    if (cat->rows > 0) {
      if (cat->values->capacity == 0) fail(CS_ERR_INVALID_ARG, "ipc export: the category's values are not owned memory");
      ipc_handle_of(cat->values, out->values);
    }
  });
}
int cs_category_ipc_import(const cs_ipc_category* ipc, cs_category** out) {
  return guard([&] {
    if (!ipc || !out) fail(CS_ERR_INVALID_ARG, "ipc import: null argument");
    require_device();
    auto c = std::make_unique<cs_category>();
    c->keys.reset(import_column(&ipc->keys));
    c->rows = ipc->rows;
    if (ipc->rows > 0) c->values = ipc_open(ipc->values, sizeof(int32_t) * (size_t)ipc->rows);
    *out = c.release();
  });
}

int cs_column_destroy(cs_column* col) {
  return guard([&] { delete col; });
}
int64_t cs_column_rows(const cs_column* col) { return col ? col->rows : 0; }
int64_t cs_column_nbytes(const cs_column* col) { return col ? col->nbytes : 0; }
int cs_column_offset_width(const cs_column* col) { return !col ? 0 : (col->offsets32 ? 4 : 8); }
int64_t cs_column_null_count(const cs_column* col) {
  int64_t n = -1;
  int st = guard([&] {
    if (!col) fail(CS_ERR_INVALID_ARG, "null column");
    n = count_nulls(col, nullptr);
  });
  return st == CS_OK ? n : -1;
}
int cs_column_cached_meta(const cs_column* col, int64_t out[4]) {
  return guard([&] {
    if (!col || !out) fail(CS_ERR_INVALID_ARG, "null argument");
    out[0] = col->max_span64;
    out[1] = col->max_row;
    out[2] = col->plain_bytes;
    out[3] = col->high_sample;
  });
}
int cs_column_get_view(const cs_column* col, cs_column_view* view) {
  return guard([&] {
    if (!col || !view) fail(CS_ERR_INVALID_ARG, "null argument");
    view->chars = col->d_chars();
    view->offsets = col->d_offsets();
    view->validity = col->d_validity();
    view->rows = col->rows;
    view->nbytes = col->nbytes;
    view->null_count = col->null_count;
  });
}

int cs_column_export_offsets64(const cs_column* col, uint8_t* chars, int64_t* offsets, uint8_t* validity,
                               int on_device, cs_stream stream) {
  return guard([&] {
    if (!col) fail(CS_ERR_INVALID_ARG, "null column");
    hipStream_t s = S(stream);
    if (col->rows == 0) return;
    if (chars) copy_out(chars, col->d_chars(), (size_t)col->nbytes, on_device, s);
    if (offsets) copy_out(offsets, col->d_offsets(), sizeof(int64_t) * (col->rows + 1), on_device, s);
    if (validity) {
      // materialise (rows+7)/8 bytes even when the column has no mask
      Buf bits = dev_alloc((size_t)((col->rows + 7) / 8) + 8, s);
      Buf cnt = zeroed_count(s);
      hipLaunchKernelGGL(k_null_bitarray, dim3(blocks_for((col->rows + 7) / 8)), dim3(kBlock), 0, s,
                         view_of(col), 0, ptr<uint8_t>(bits), ptr<unsigned long long>(cnt));
      copy_out(validity, bits->p, (size_t)((col->rows + 7) / 8), on_device, s);
      CS_HIP(hipStreamSynchronize(s));
    }
    if (!on_device) CS_HIP(hipStreamSynchronize(s));
  });
}

int cs_column_export_offsets32(const cs_column* col, char* chars, int32_t* offsets, uint8_t* validity,
                               int on_device, cs_stream stream) {
  return guard([&] {
    if (!col) fail(CS_ERR_INVALID_ARG, "null column");
    if (col->rows == 0) return;
    if (!chars || !offsets) return;  // the reference returns 0 without doing anything (NVStrings.cu:406-407)
    if (col->nbytes >= (1LL << 31)) fail(CS_ERR_RANGE, "create_offsets: column holds >= 2 GiB of chars; int32 offsets cannot address it");
    hipStream_t s = S(stream);
    if (col->offsets32) {  // born with int32 offsets: they go out as they are
      copy_out(offsets, col->d_offsets32(), sizeof(int32_t) * (col->rows + 1), on_device, s);
    } else {
      Buf o32 = dev_alloc(sizeof(int32_t) * (col->rows + 1), s);
      hipLaunchKernelGGL(k_narrow_offsets, dim3(blocks_for(col->rows + 1)), dim3(kBlock), 0, s,
                         col->d_offsets(), col->rows + 1, ptr<int32_t>(o32));
      copy_out(offsets, o32->p, sizeof(int32_t) * (col->rows + 1), on_device, s);
    }
    CS_HIP(hipStreamSynchronize(s));
    int st = cs_column_export_offsets64(col, (uint8_t*)chars, nullptr, validity, on_device, stream);
    if (st != CS_OK) fail(st, cs_last_error());
  });
}

int cs_column_byte_count(const cs_column* col, int32_t* lengths, int on_device, cs_stream stream,
                         int64_t* total) {
  return guard([&] {
    if (!col) fail(CS_ERR_INVALID_ARG, "null column");
    hipStream_t s = S(stream);
    if (total) *total = 0;
    if (col->rows == 0) return;
    const ResultsOut res(lengths, sizeof(int32_t) * col->rows, on_device && lengths, s);  // (without `lengths`: a temporary nobody fills)
    // (null rows have zero extent, so the total is the column's byte count: no reduction)
    if (lengths) {
      hipLaunchKernelGGL(k_lengths_from_offsets, dim3(blocks_for(col->rows)), dim3(kBlock), 0, s, view_of(col), static_cast<int32_t*>(res.dev));
      res.finish(s);
    }
    if (total) *total = col->nbytes;
  });
}

int cs_column_null_bitarray(const cs_column* col, uint8_t* bitarray, int empty_is_null, int on_device,
                            cs_stream stream, int64_t* null_count) {
  return guard([&] {
    if (!col || !bitarray) fail(CS_ERR_INVALID_ARG, "null argument");
    hipStream_t s = S(stream);
    if (null_count) *null_count = 0;
    if (col->rows == 0) return;
    size_t nb = (size_t)((col->rows + 7) / 8);
    const ResultsOut res(bitarray, nb, on_device, s);
    const Buf cnt = zeroed_count(s);
    hipLaunchKernelGGL(k_null_bitarray, dim3(blocks_for((int64_t)nb)), dim3(kBlock), 0, s, view_of(col),
                       empty_is_null, static_cast<uint8_t*>(res.dev), ptr<unsigned long long>(cnt));
    res.copy_back(s);
    const int64_t n = read_count(cnt, s);
    if (null_count) *null_count = n;
  });
}

int cs_column_digest(const cs_column* col, cs_stream stream, uint64_t* digest) {
  return guard([&] {
    if (!col || !digest) fail(CS_ERR_INVALID_ARG, "null argument");
    hipStream_t s = S(stream);
    *digest = 0;
    if (col->rows == 0) return;
    const Buf acc = zeroed_count(s);
    hipLaunchKernelGGL(k_digest, dim3(blocks_for(col->rows)), dim3(kBlock), 0, s, view_of(col), ptr<unsigned long long>(acc));
    *digest = (uint64_t)read_count(acc, s);
  });
}

}  // extern "C"
