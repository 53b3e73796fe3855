// The C entries of the case, strip, find, replace, split, tokenize and ngrams families and their row-wise kernels: one
// thread a row, the per-row logic in row_ops.h.  The tile routes of these families live in cs_rows.hip (strip, find,
// contains), cs_case.hip, cs_casemodes.hip, cs_split.hip, cs_tokenize.hip and cs_ngram.hip; an entry here tries its
// tile route first and what is in this file answers when that declines: long rows, non-ASCII arguments, a row-wise switch.
//  - ops that make a column (case, strip, replace): two_pass -- a size kernel with fused block sums, the scan to offsets,
//    a write kernel; split, tokenize and ngrams have kernels of their own with the same three steps;
//  - ops that make one value a row and a count of the hits (find, rfind, find_from, compare, startswith, endswith,
//    contains, match_strings): the counted-rows route, k_counted_rows<Op> / run_counted, with an op struct each.
// Reference call sites are cited at each entry point.
#include <hip/hip_runtime.h>

#include <cstring>

#include "cs_internal.h"
#include "device_utils.h"
#include "chartype_ops.h"
#include "row_ops.h"

using namespace cs;
using namespace csdev;

namespace cs {
bool tokenize_fast(const cs_column* col, const unsigned char* delims, int ndel, hipStream_t s, cs_column** out);
bool change_case_fast(const cs_column* col, unsigned bit, bool ascii_rule_ok, hipStream_t s, cs_column** out);
bool case_modes_fast(const cs_column* col, int op, bool ascii_ok, hipStream_t s, cs_column** out);  // cs_casemodes.hip
bool ngrams_fast(const cs_column* tokens, int n, const unsigned char* sep, int sepn, hipStream_t s, cs_column** out);
}
namespace csrow {
struct CharSet;
}
namespace cs {
bool strip_single(const cs_column* in, const csrow::CharSet& set, int side, hipStream_t s, cs_column* o);
bool strip_write_tiles(const cs_column* in, const csrow::CharSet& set, int side, const int64_t* out_off, uint8_t* out_chars,
                       hipStream_t s);
bool find_tiles(const cs_column* in, const unsigned char* needle, int nb, int mode, int start, int end, int32_t* out32,
                uint8_t* out8, unsigned long long* found, hipStream_t s);
}
using namespace csrow;

namespace cs {
// the character set of a UTF-8 string of any length; `more` keeps what does not fit the struct alive for the caller's kernels
CharSet make_charset(const char* s, Buf& more, hipStream_t st) {
  std::vector<Char> overflow;
  CharSet cs = charset_from_utf8(reinterpret_cast<const uint8_t*>(s), (int)strlen(s), overflow);
  if (!overflow.empty()) {
    more = dev_alloc(sizeof(Char) * overflow.size(), st);
    CS_HIP(hipMemcpyAsync(more->p, overflow.data(), sizeof(Char) * overflow.size(), hipMemcpyHostToDevice, st));
    CS_HIP(hipStreamSynchronize(st));  // (`overflow` is pageable and leaves scope)
    cs.more = ptr<const Char>(more);
    cs.nmore = (int)overflow.size();
  }
  return cs;
}
}  // namespace cs
namespace {

// ---- generic two-pass driver -------------------------------------------------
// SizeFn:  int  operator()(const uint8_t* row, int len, int64_t r) const
// WriteFn: void operator()(const uint8_t* row, int len, int64_t r, uint8_t* dst) const
template <class SizeFn>
__global__ void k_row_sizes(ColView in, SizeFn f, int32_t* __restrict__ lens,
                            int64_t* __restrict__ block_sums) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int len = -1;
  if (r < in.rows && row_is_valid(in.validity, r)) {
    int64_t b = in.offsets[r];
    len = f(in.chars + b, (int)(in.offsets[r + 1] - b), r);
  }
  if (r < in.rows) lens[r] = len;
  long long t = block_reduce_sum(len < 0 ? 0 : len);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = t;
}
template <class WriteFn>
__global__ void k_row_write(ColView in, WriteFn f, const int64_t* __restrict__ out_off,
                            uint8_t* __restrict__ out_chars) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= in.rows || !row_is_valid(in.validity, r)) return;
  int64_t b = in.offsets[r];
  f(in.chars + b, (int)(in.offsets[r + 1] - b), r, out_chars + out_off[r]);
}

// the size pass and the scan of `b`'s offsets; the lengths and block sums stay the caller's until its write pass is launched
struct RowSizes {
  Buf lens, sums;
};
template <class SizeFn>
RowSizes size_rows(const cs_column* in, SizeFn sf, hipStream_t s, const char* size_name, Built& b) {
  const unsigned nb = blocks_for(in->rows);
  RowSizes z{dev_alloc(sizeof(int32_t) * in->rows, s), dev_alloc(sizeof(int64_t) * nb, s)};
  {
    ProfScope ps(size_name, s);
    hipLaunchKernelGGL(k_row_sizes<SizeFn>, dim3(nb), dim3(kBlock), 0, s, view_of(in), sf,
                       ptr<int32_t>(z.lens), ptr<int64_t>(z.sums));
  }
  b.scan(ptr<int32_t>(z.lens), z.sums);
  return z;
}
template <class WriteFn>
void write_rows(const cs_column* in, WriteFn wf, hipStream_t s, const char* write_name, const Built& b) {
  ProfScope ps(write_name, s);
  hipLaunchKernelGGL(k_row_write<WriteFn>, dim3(blocks_for(in->rows)), dim3(kBlock), 0, s, view_of(in), wf, b.off, b.chars);
}

template <class SizeFn, class WriteFn>
cs_column* two_pass(const cs_column* in, SizeFn sf, WriteFn wf, hipStream_t s, const char* size_name,
                    const char* write_name) {
  if (in->rows == 0) return make_all_null(0, s);
  Built b(in, s);
  const RowSizes z = size_rows(in, sf, s, size_name, b);
  b.alloc_chars();
  write_rows(in, wf, s, write_name, b);
  return b.col.release();
}

// ---- functors ---------------------------------------------------------------------
struct CaseSize {
  const uint8_t* flags;
  const uint16_t* cases;
  unsigned bit;
  __device__ int operator()(const uint8_t* p, int n, int64_t) const { return row_case_size(p, n, flags, cases, bit); }
};
struct CaseWrite {
  const uint8_t* flags;
  const uint16_t* cases;
  unsigned bit;
  __device__ void operator()(const uint8_t* p, int n, int64_t, uint8_t* o) const { row_case_write(p, n, flags, cases, bit, o); }
};
struct CaseModeSize {  // swapcase / capitalize / title (chartype_ops.h)
  const uint8_t* flags;
  const uint16_t* cases;
  int op;
  __device__ int operator()(const uint8_t* p, int n, int64_t) const { return cschr::case_size(p, n, flags, cases, op); }
};
struct CaseModeWrite {
  const uint8_t* flags;
  const uint16_t* cases;
  int op;
  __device__ void operator()(const uint8_t* p, int n, int64_t, uint8_t* o) const { cschr::case_write(p, n, flags, cases, op, o); }
};
struct StripSize {
  CharSet set;
  int side;
  __device__ int operator()(const uint8_t* p, int n, int64_t) const {
    int lo, hi;
    row_strip(p, n, set, side, lo, hi);
    return hi - lo;
  }
};
struct StripWrite {
  CharSet set;
  int side;
  __device__ void operator()(const uint8_t* p, int n, int64_t, uint8_t* o) const {
    int lo, hi;
    row_strip(p, n, set, side, lo, hi);
    for (int i = lo; i < hi; ++i) *o++ = p[i];
  }
};
struct ReplaceSize {
  const uint8_t* needle;
  int nb, rb, maxrepl;
  __device__ int operator()(const uint8_t* p, int n, int64_t) const { return row_replace_size(p, n, needle, nb, rb, maxrepl); }
};
struct ReplaceWrite {
  const uint8_t* needle;
  const uint8_t* repl;
  int nb, rb, maxrepl;
  __device__ void operator()(const uint8_t* p, int n, int64_t, uint8_t* o) const { row_replace_write(p, n, needle, nb, repl, rb, maxrepl, o); }
};

// ---- the counted-rows route: one value a row and the count of the hits (the find family, find.cu:36-387) --------------
// An op is a struct passed by value with its state (the needle, the bounds, the other column):
//   using T = int32_t or uint8_t;                                                    // the result type
//   __device__ T operator()(int64_t r, const uint8_t* p, int n, bool valid) const;  // row r's bytes [p, p + n); a null row's value too
//   static __device__ bool counts(T v);                                              // is this result a hit
// A thread a row on a capped grid (rows a grid apart), so the count takes one same-address atomic per workgroup and not
// one per 256 rows, and none from a workgroup without a hit.
template <class Op>
__global__ void __launch_bounds__(256) k_counted_rows(ColView in, Op op, typename Op::T* __restrict__ out,
                                                      unsigned long long* __restrict__ count) {
  int hits = 0;
  for_each_row(in, [&](int64_t r, const uint8_t* p, int n, bool valid) {
    const typename Op::T v = op(r, p, n, valid);
    out[r] = v;
    hits += Op::counts(v);
  });
  const long long t = block_reduce_sum(hits);
  if (threadIdx.x == 0 && t) atomicAdd(count, (unsigned long long)t);
}
// The host tail of every counted op: the results to the caller's buffer (host or device), the count returned.  `tiles`
// (find, contains): the tile route, tried first -- true when it wrote the results and the count.  Synchronises `s`, so
// what the op points to may go when this returns.
template <class Op, class Tiles>
int64_t run_counted(const cs_column* col, const Op& op, void* results, int on_device, const char* prof_name, hipStream_t s,
                    Tiles&& tiles) {
  using T = typename Op::T;
  const Buf cnt = zeroed_count(s);
  const ResultsOut res(results, sizeof(T) * (size_t)col->rows, on_device, s);
  T* out = static_cast<T*>(res.dev);
  {
    ProfScope ps(prof_name, s);
    const bool tiled = tiles(out, ptr<unsigned long long>(cnt));
    note_route(tiled ? "tile" : "rows");
    if (!tiled)
      hipLaunchKernelGGL(k_counted_rows<Op>, dim3(std::min(blocks_for(col->rows), 8192u)), dim3(kBlock), 0, s, view_of(col), op,
                         out, ptr<unsigned long long>(cnt));
  }
  CS_HIP(hipGetLastError());
  res.copy_back(s);
  return read_count(cnt, s);
}
template <class Op>
int64_t run_counted(const cs_column* col, const Op& op, void* results, int on_device, const char* prof_name, hipStream_t s) {
  return run_counted(col, op, results, on_device, prof_name, s, [](typename Op::T*, unsigned long long*) { return false; });
}

// positions in characters, -1 no occurrence, -2 a null row -- which the reference counts like a hit (find.cu:108-112)
struct FindOp {  // find(str, start, end)
  using T = int32_t;
  const uint8_t* needle;
  int nb, start, end;
  __device__ T operator()(int64_t, const uint8_t* p, int n, bool valid) const { return valid ? row_find(p, n, needle, nb, start, end) : -2; }
  static __device__ bool counts(T v) { return v != -1; }
};
struct RfindOp {  // rfind(str, start, end), start >= 0
  using T = int32_t;
  const uint8_t* needle;
  int nb, start, end;
  __device__ T operator()(int64_t, const uint8_t* p, int n, bool valid) const {
    return valid ? row_rfind_count(p, n, needle, nb, (unsigned)start, end - start) : -2;
  }
  static __device__ bool counts(T v) { return v != -1; }
};
struct FindFromOp {  // find_from(str, starts[], ends[]): a window a row; no starts: from 0, no ends: to the row's end
  using T = int32_t;
  const uint8_t* needle;
  int nb;
  const int32_t *starts, *ends;
  __device__ T operator()(int64_t r, const uint8_t* p, int n, bool valid) const {
    if (!valid) return -2;
    const int pos = starts ? starts[r] : 0;
    return row_find_count(p, n, needle, nb, (unsigned)pos, ends ? ends[r] - pos : -1);
  }
  static __device__ bool counts(T v) { return v != -1; }
};
struct CompareOp {  // compare(str): 0 equal, and those are counted; a null row -1
  using T = int32_t;
  const uint8_t* needle;
  int nb;
  __device__ T operator()(int64_t, const uint8_t* p, int n, bool valid) const { return valid ? row_compare(p, n, needle, nb) : -1; }
  static __device__ bool counts(T v) { return v == 0; }
};
template <bool kEnd>
struct AffixOp {  // startswith(str) / endswith(str); a null row is false
  using T = uint8_t;
  const uint8_t* needle;
  int nb;
  __device__ T operator()(int64_t, const uint8_t* p, int n, bool valid) const {
    return valid && (kEnd ? row_ends_with(p, n, needle, nb) : row_starts_with(p, n, needle, nb));
  }
  static __device__ bool counts(T v) { return v; }
};
struct ContainsOp {  // contains(str) by bytes; an empty needle and a null row are false
  using T = uint8_t;
  const uint8_t* needle;
  int nb;
  __device__ T operator()(int64_t, const uint8_t* p, int n, bool valid) const { return valid && row_contains(p, n, needle, nb); }
  static __device__ bool counts(T v) { return v; }
};
struct MatchStringsOp {  // match_strings(other): equal rows; two nulls are equal
  using T = uint8_t;
  ColView other;
  __device__ T operator()(int64_t r, const uint8_t* p, int n, bool valid) const {
    if (!row_is_valid(other.validity, r)) return !valid;
    const int64_t o0 = other.offsets[r];
    return valid && row_compare(p, n, other.chars + o0, (int)(other.offsets[r + 1] - o0)) == 0;
  }
  static __device__ bool counts(T v) { return v; }
};

// ---- split ---------------------------------------------------------------------------------
struct SplitArgs {
  const uint8_t* delim;  // nullptr = whitespace
  int nb;
  int tokens;
  int reverse;  // rsplit: tokens located from the right
  int ncols;    // rsplit on whitespace: the column count of the whole call (known after k_split_count)
};
// the row's tokens through emit(k, lo, hi), forward or (rsplit) from the right
template <class Emit>
__device__ __forceinline__ void split_row_tokens(const SplitArgs& a, const uint8_t* p, int n, int c, Emit&& emit) {
  if (!a.reverse) {
    if (a.delim) row_split_tokens(p, n, a.delim, a.nb, c, emit);
    else row_ws_tokens(p, n, a.tokens, emit);
  } else if (a.delim) {
    row_rsplit_tokens(p, n, a.delim, a.nb, c, emit);
  } else {
    for (int k = 0; k < c; ++k) {
      int lo, hi;
      if (row_ws_rtoken(p, n, a.tokens, c, a.ncols, k, lo, hi)) emit(k, lo, hi);
    }
  }
}
__global__ void k_split_count(ColView in, SplitArgs a, int32_t* __restrict__ counts, int* __restrict__ max_out) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int c = 0;
  if (r < in.rows) {
    if (row_is_valid(in.validity, r)) {
      int64_t b = in.offsets[r];
      int n = (int)(in.offsets[r + 1] - b);
      c = a.delim ? row_split_count(in.chars + b, n, a.delim, a.nb, a.tokens)
                  : row_wssplit_count(in.chars + b, n, a.tokens);
    }
    counts[r] = c;
  }
  int m = block_reduce_max(c);
  // (only a workgroup that would raise the maximum issues the same-address atomic)
  if (threadIdx.x == 0 && m > __hip_atomic_load(max_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(max_out, m);
}
// lens[k * rows + r] = byte length of token k of row r, -1 when the row has no
// such token (null in that column); block sums per column are fused in.
__global__ void k_split_sizes(ColView in, SplitArgs a, const int32_t* __restrict__ counts, int ncols,
                              int32_t* __restrict__ lens, int64_t* __restrict__ block_sums) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t rows = in.rows;
  if (r < rows) {
    for (int k = 0; k < ncols; ++k) lens[(int64_t)k * rows + r] = -1;
    int c = counts[r];
    if (c > 0) {
      int64_t b = in.offsets[r];
      int n = (int)(in.offsets[r + 1] - b);
      auto emit = [&](int k, int lo, int hi) {
        if (k < ncols) lens[(int64_t)k * rows + r] = hi - lo;
      };
      split_row_tokens(a, in.chars + b, n, c, emit);
    }
  }
  for (int k = 0; k < ncols; ++k) {
    int v = (r < rows) ? lens[(int64_t)k * rows + r] : 0;
    long long t = block_reduce_sum(v < 0 ? 0 : v);
    if (threadIdx.x == 0) block_sums[(int64_t)k * gridDim.x + blockIdx.x] = t;
  }
}
struct SplitOut {
  uint8_t* chars;
  const int64_t* offsets;
};
__global__ void k_split_write(ColView in, SplitArgs a, const int32_t* __restrict__ counts, int ncols,
                              const SplitOut* __restrict__ outs) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= in.rows) return;
  int c = counts[r];
  if (c <= 0) return;
  int64_t b = in.offsets[r];
  int n = (int)(in.offsets[r + 1] - b);
  const uint8_t* p = in.chars + b;
  auto emit = [&](int k, int lo, int hi) {
    if (k >= ncols) return;
    uint8_t* o = outs[k].chars + outs[k].offsets[r];
    for (int i = lo; i < hi; ++i) *o++ = p[i];
  };
  split_row_tokens(a, p, n, c, emit);
}

// ---- tokenize --------------------------------------------------------------------------------
// (row_tok_walk, row_ops.h: the reference's walk over characters; cs_text.hip's counters keep row_ws_tokens / row_set_tokens)
using TokArgs = TokDelims;
__global__ void k_tok_count(ColView in, TokArgs a, int32_t* __restrict__ counts,
                            int64_t* __restrict__ block_sums) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int c = 0;
  if (r < in.rows && row_is_valid(in.validity, r)) {
    int64_t b = in.offsets[r];
    int n = (int)(in.offsets[r + 1] - b);
    c = row_tok_walk(in.chars + b, n, a, [](int, int, int) {});
  }
  if (r < in.rows) counts[r] = c;
  long long t = block_reduce_sum(c);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = t;
}
// phase 0: token lengths into tok_lens[tok_base[r] + k]; phase 1: copy bytes
template <int PHASE>
__global__ void k_tok_emit(ColView in, TokArgs a, const int64_t* __restrict__ tok_base,
                           int32_t* __restrict__ tok_lens, const int64_t* __restrict__ out_off,
                           uint8_t* __restrict__ out_chars) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= in.rows || !row_is_valid(in.validity, r)) return;
  int64_t t0 = tok_base[r];
  if (tok_base[r + 1] == t0) return;
  int64_t b = in.offsets[r];
  int n = (int)(in.offsets[r + 1] - b);
  const uint8_t* p = in.chars + b;
  auto emit = [&](int k, int lo, int hi) {
    if (PHASE == 0) {
      tok_lens[t0 + k] = hi - lo;
    } else {
      uint8_t* o = out_chars + out_off[t0 + k];
      for (int i = lo; i < hi; ++i) *o++ = p[i];
    }
  };
  row_tok_walk(p, n, a, emit);
}

// ---- ngrams -----------------------------------------------------------------------------------
__global__ void k_keep_flags(ColView in, int32_t* __restrict__ flags) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r < in.rows) flags[r] = row_is_valid(in.validity, r) && in.offsets[r + 1] > in.offsets[r];
}
__global__ void k_keep_scatter(const int32_t* __restrict__ flags, const int64_t* __restrict__ pos,
                               int64_t rows, int32_t* __restrict__ kept) {
  int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r < rows && flags[r]) kept[pos[r]] = (int32_t)r;
}
__global__ void k_ngram_sizes(ColView in, const int32_t* __restrict__ kept, int64_t count, int n,
                              int sep, int32_t* __restrict__ lens) {
  int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= count) return;
  int sz = (n - 1) * sep;
  for (int k = 0; k < n; ++k) {
    int64_t r = kept[g + k];
    sz += (int)(in.offsets[r + 1] - in.offsets[r]);
  }
  lens[g] = sz;
}
__global__ void k_ngram_write(ColView in, const int32_t* __restrict__ kept, int64_t count, int n,
                              const uint8_t* __restrict__ sep, int sepn,
                              const int64_t* __restrict__ out_off, uint8_t* __restrict__ out_chars) {
  int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= count) return;
  uint8_t* o = out_chars + out_off[g];
  for (int k = 0; k < n; ++k) {
    int64_t r = kept[g + k];
    const uint8_t* p = in.chars + in.offsets[r];
    int len = (int)(in.offsets[r + 1] - in.offsets[r]);
    for (int i = 0; i < len; ++i) *o++ = p[i];
    if (k + 1 < n)
      for (int i = 0; i < sepn; ++i) *o++ = sep[i];
  }
}

}  // namespace

extern "C" {

// NVStrings::lower / upper -- case.cu:31-97 / :100-170
static int change_case(const cs_column* col, unsigned bit, cs_stream stream, cs_column** out, const char* nm) {
  return guard([&] {
    if (!col || !out) fail(CS_ERR_INVALID_ARG, "null argument");
    require_device();
    // tile kernel (cs_case.hip) when the tables map ASCII the plain way (A-Z <-> a-z only)
    static const bool ascii_rule_ok = [] {
      const uint8_t* f = h_unicode_flags();
      const uint16_t* c = h_charcases();
      for (unsigned b = 0; b < 128; ++b) {
        const unsigned lower = (b >= 'A' && b <= 'Z') ? b + 32 : b, upper = (b >= 'a' && b <= 'z') ? b - 32 : b;
        if (((f[b] & 32) ? c[b] : b) != lower || ((f[b] & 64) ? c[b] : b) != upper) return false;
      }
      return true;
    }();
    if (change_case_fast(col, bit, ascii_rule_ok, S(stream), out)) {
      note_route("tile");
      return;
    }
    note_route("rows");
    *out = two_pass(col, CaseSize{d_unicode_flags(), d_charcases(), bit},
                    CaseWrite{d_unicode_flags(), d_charcases(), bit}, S(stream),
                    bit == 32 ? "k_lower_size" : "k_upper_size", nm);
  });
}
int cs_lower(const cs_column* col, cs_stream stream, cs_column** out) { return change_case(col, 32, stream, out, "k_lower_write"); }
int cs_upper(const cs_column* col, cs_stream stream, cs_column** out) { return change_case(col, 64, stream, out, "k_upper_write"); }

// NVStrings::swapcase / capitalize / title -- case.cu:169-235 / :238-311 / :314-397
static int case_mode(const cs_column* col, int op, cs_stream stream, cs_column** out, const char* size_name, const char* write_name) {
  return guard([&] {
    if (!col || !out) fail(CS_ERR_INVALID_ARG, "null argument");
    require_device();
    // tile kernel (cs_casemodes.hip) when the tables' ASCII half is the plain one: A-Z <-> a-z, the only alphabetic bytes
    static const bool ascii_ok = cschr::ascii_plain(h_unicode_flags(), h_charcases());
    if (case_modes_fast(col, op, ascii_ok, S(stream), out)) {
      note_route("tile");
      return;
    }
    note_route("rows");
    *out = two_pass(col, CaseModeSize{d_unicode_flags(), d_charcases(), op}, CaseModeWrite{d_unicode_flags(), d_charcases(), op},
                    S(stream), size_name, write_name);
  });
}
int cs_swapcase(const cs_column* col, cs_stream stream, cs_column** out) {
  return case_mode(col, cschr::OP_SWAPCASE, stream, out, "k_swapcase_size", "k_swapcase_write");
}
int cs_capitalize(const cs_column* col, cs_stream stream, cs_column** out) {
  return case_mode(col, cschr::OP_CAPITALIZE, stream, out, "k_capitalize_size", "k_capitalize_write");
}
int cs_title(const cs_column* col, cs_stream stream, cs_column** out) {
  return case_mode(col, cschr::OP_TITLE, stream, out, "k_title_size", "k_title_write");
}

// NVStrings::strip family -- strip.cu:30-199
int cs_strip(const cs_column* col, const char* to_strip, int side, cs_stream stream, cs_column** out) {
  return guard([&] {
    if (!col || !out || side < 0 || side > 2) fail(CS_ERR_INVALID_ARG, "strip: bad arguments");
    require_device();
    hipStream_t s = S(stream);
    Buf set_more;
    CharSet set = make_charset(to_strip ? to_strip : " \n\t", set_more, s);
    // size pass + scan as for every row-wise op; the write pass runs on row tiles (cs_rows.hip)
    if (col->rows > 0 && !cs::cfg("CS_STRIP_ROWWISE")) {
      Built b(col, s);
      if (strip_single(col, set, side, s, b.col.get())) {  // one pass (cs_rows.hip: k_strip_stream)
        note_route("strip-stream");
        *out = b.col.release();
        return;
      }
      const RowSizes z = size_rows(col, StripSize{set, side}, s, "k_strip_size", b);
      if (col->plain_bytes == 1) b.col->plain_bytes = 1;  // (rows cut at character boundaries of a plain column stay plain)
      if (col->high_sample == 0) b.col->high_sample = 0;
      b.alloc_chars();
      const bool tiled = strip_write_tiles(col, set, side, b.off, b.chars, s);
      note_route(tiled ? "tile" : "rows");
      if (!tiled) write_rows(col, StripWrite{set, side}, s, "k_strip_write", b);
      *out = b.col.release();
      return;
    }
    note_route("rows");
    *out = two_pass(col, StripSize{set, side}, StripWrite{set, side}, S(stream), "k_strip_size", "k_strip_write");
  });
}

// NVStrings::find -- find.cu:75-120
int cs_find(const cs_column* col, const char* str, int start, int end, int32_t* results, int on_device,
            cs_stream stream, int64_t* found) {
  return guard([&] {
    if (found) *found = 0;
    if (!col || !str || !results || col->rows == 0) return;  // reference returns 0 (find.cu:78-79)
    require_device();
    hipStream_t s = S(stream);
    const HostText nd(str, s);
    const int64_t n = run_counted(col, FindOp{nd.d(), nd.n, start, end}, results, on_device, "k_find", s, [&](int32_t* out, unsigned long long* cnt) {
      return find_tiles(col, reinterpret_cast<const unsigned char*>(str), nd.n, 0, start, end, out, nullptr, cnt, s);
    });
    if (found) *found = n;
  });
}

// ---- rfind, find_from, compare, startswith, endswith, match_strings, find_multiple (find.cu:36-72, 123-236, 276-387):
// no tile route, a thread a row (these are not on the benchmarked path) ----
// find_multiple has rows x targets results, so kernels of its own: out[r * tcount + j] = position of target j in row r
__global__ void k_find_multiple(ColView in, ColView targets, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= in.rows * targets.rows) return;
  const int64_t r = i / targets.rows, j = i - r * targets.rows;
  int v = -2;
  if (row_is_valid(in.validity, r) && row_is_valid(targets.validity, j)) {
    const int64_t b = in.offsets[r], tb = targets.offsets[j];
    v = row_find_count(in.chars + b, (int)(in.offsets[r + 1] - b), targets.chars + tb, (int)(targets.offsets[j + 1] - tb), 0u, -1);
  }
  out[i] = v;
}
__global__ void k_count_not_minus_one(const int32_t* __restrict__ v, int64_t n, unsigned long long* __restrict__ count) {
  int hit = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) hit += v[i] != -1;
  const long long t = block_reduce_sum(hit);
  if (threadIdx.x == 0 && t) atomicAdd(count, (unsigned long long)t);
}
// NVStrings::rfind -- find.cu:163-200
int cs_rfind(const cs_column* col, const char* str, int start, int end, int32_t* results, int on_device, cs_stream stream, int64_t* found) {
  return guard([&] {
    if (found) *found = 0;
    if (!col || !str || !results || col->rows == 0) return;  // the reference returns 0
    require_device();
    hipStream_t s = S(stream);
    const HostText nd(str, s);
    const int64_t n = run_counted(col, RfindOp{nd.d(), nd.n, start < 0 ? 0 : start, end}, results, on_device, "k_find_family", s);
    if (found) *found = n;
  });
}
// NVStrings::find_from -- find.cu:123-160 (`starts` / `ends`: one int32 per row, either may be null)
int cs_find_from(const cs_column* col, const char* str, const int32_t* starts, const int32_t* ends, int bounds_on_device, int32_t* results, int on_device,
                 cs_stream stream, int64_t* found) {
  return guard([&] {
    if (found) *found = 0;
    if (!col || !str || !results || col->rows == 0) return;
    require_device();
    hipStream_t s = S(stream);
    const HostText nd(str, s);
    const DevArray<int32_t> from(starts, col->rows, bounds_on_device, s), to(ends, col->rows, bounds_on_device, s);
    const int64_t n = run_counted(col, FindFromOp{nd.d(), nd.n, from.d, to.d}, results, on_device, "k_find_family", s);
    if (found) *found = n;
  });
}
// NVStrings::compare -- find.cu:36-72
int cs_compare(const cs_column* col, const char* str, int32_t* results, int on_device, cs_stream stream, int64_t* matches) {
  return guard([&] {
    if (matches) *matches = 0;
    // (an empty `str`: the reference returns without writing -- find.cu -- and its callers read an uninitialised buffer; here
    // the comparison with the empty string is computed like any other: 1 for a non-empty row, 0 for an empty one)
    if (!col || !str || !results || col->rows == 0) return;
    require_device();
    hipStream_t s = S(stream);
    const HostText nd(str, s);
    const int64_t n = run_counted(col, CompareOp{nd.d(), nd.n}, results, on_device, "k_find_family", s);
    if (matches) *matches = n;
  });
}
// NVStrings::startswith / endswith -- find.cu:316-387
int cs_startswith(const cs_column* col, const char* str, uint8_t* results, int on_device, cs_stream stream, int64_t* matches) {
  return guard([&] {
    if (matches) *matches = 0;
    if (!col || !str || !results || col->rows == 0) return;
    require_device();
    hipStream_t s = S(stream);
    const HostText nd(str, s);
    const int64_t n = run_counted(col, AffixOp<false>{nd.d(), nd.n}, results, on_device, "k_find_family", s);
    if (matches) *matches = n;
  });
}
int cs_endswith(const cs_column* col, const char* str, uint8_t* results, int on_device, cs_stream stream, int64_t* matches) {
  return guard([&] {
    if (matches) *matches = 0;
    if (!col || !str || !results || col->rows == 0) return;
    require_device();
    hipStream_t s = S(stream);
    const HostText nd(str, s);
    const int64_t n = run_counted(col, AffixOp<true>{nd.d(), nd.n}, results, on_device, "k_find_family", s);
    if (matches) *matches = n;
  });
}
// NVStrings::match_strings -- find.cu:276-314 (sizes must match: std::invalid_argument there)
int cs_match_strings(const cs_column* col, const cs_column* other, uint8_t* results, int on_device, cs_stream stream, int64_t* matches) {
  return guard([&] {
    if (matches) *matches = -1;
    if (!col || !other || !results) fail(CS_ERR_INVALID_ARG, "match_strings: null argument");
    if (matches) *matches = 0;
    if (col->rows == 0) return;
    if (col->rows != other->rows) fail(CS_ERR_INVALID_ARG, "sizes must match");
    require_device();
    const int64_t n = run_counted(col, MatchStringsOp{view_of(other)}, results, on_device, "k_match_strings", S(stream));
    if (matches) *matches = n;
  });
}
// NVStrings::find_multiple -- find.cu:202-234: results[r * targets + j]; the returned count looks at the first rows()
// entries only, as the reference's does
int cs_find_multiple(const cs_column* col, const cs_column* targets, int32_t* results, int on_device, cs_stream stream, int64_t* found) {
  return guard([&] {
    if (found) *found = 0;
    if (!col || !targets || !results || col->rows == 0 || targets->rows == 0) return;
    require_device();
    hipStream_t s = S(stream);
    const int64_t total = col->rows * targets->rows;
    note_route("rows");
    const Buf cnt = zeroed_count(s);
    const ResultsOut res(results, sizeof(int32_t) * total, on_device, s);
    int32_t* d_out = static_cast<int32_t*>(res.dev);
    hipLaunchKernelGGL(k_find_multiple, dim3(blocks_for(total)), dim3(kBlock), 0, s, view_of(col), view_of(targets), d_out);
    hipLaunchKernelGGL(k_count_not_minus_one, dim3(std::min(blocks_for(col->rows), 8192u)), dim3(kBlock), 0, s, d_out, col->rows, ptr<unsigned long long>(cnt));
    CS_HIP(hipGetLastError());
    res.copy_back(s);
    const int64_t n = read_count(cnt, s);
    if (found) *found = n;
  });
}

// NVStrings::contains -- find.cu:237-272
int cs_contains(const cs_column* col, const char* str, uint8_t* results, int on_device, cs_stream stream,
                int64_t* found) {
  return guard([&] {
    if (found) *found = -1;
    if (!col || !str || !results) fail(CS_ERR_INVALID_ARG, "contains: null argument");  // reference returns -1
    if (found) *found = 0;
    if (col->rows == 0) return;
    require_device();
    hipStream_t s = S(stream);
    const HostText nd(str, s);
    const int64_t n = run_counted(col, ContainsOp{nd.d(), nd.n}, results, on_device, "k_contains", s, [&](uint8_t* out, unsigned long long* cnt) {
      return find_tiles(col, reinterpret_cast<const unsigned char*>(str), nd.n, 1, 0, 0, nullptr, out, cnt, s);
    });
    if (found) *found = n;
  });
}

// NVStrings::replace -- modify.cu:109-192
int cs_replace(const cs_column* col, const char* str, const char* repl, int maxrepl, cs_stream stream,
               cs_column** out) {
  return guard([&] {
    if (!col || !out) fail(CS_ERR_INVALID_ARG, "null argument");
    if (!str || !*str) fail(CS_ERR_INVALID_ARG, "replace parameter cannot be null or empty");
    require_device();
    hipStream_t s = S(stream);
    if (!repl) repl = "";
    // An ASCII needle and a replacement of at most 16 bytes run on the persistent single-pass
    // replace_re kernel (same leftmost, non-overlapping semantics; modify.cu:109-192 restarts at
    // pos + nchars(str), replace.cu:91-92 at the match end): the needle becomes a pattern with
    // its regex metacharacters escaped.
    {
      bool plain = true;
      std::string pattern;
      for (const char* p = str; *p && plain; ++p) {
        const unsigned char c = (unsigned char)*p;
        plain = c >= 0x20 && c < 0x7F;
        if (strchr(".*+?{|()^$[\\", c)) pattern.push_back('\\');
        pattern.push_back((char)c);
      }
      plain = plain && pattern.size() <= 128;
      const size_t rb = strlen(repl);
      if (plain && rb <= 64 && col->rows > 0 && !cs::cfg("CS_REPLACE_ROWWISE") && bytes_plain(col, S(stream))) {
        cs_regex* re = nullptr;
        if (cs_regex_compile(pattern.c_str(), &re) == CS_OK) {
          cs::ReplaceCall call{col, re, repl, (int)rb, maxrepl, s};
          call.single_pass_only = true;  // the single-pass kernel or nothing: this function's own kernels are the fallback
          {  // a needle of up to eight bytes without a border is matched by byte comparison (cs_regex.hip)
            const size_t m = strlen(str);
            bool border_free = m >= 1 && m <= 8;
            for (size_t b = 1; border_free && b < m; ++b) border_free = memcmp(str, str + m - b, b) != 0;
            call.literal_len = border_free ? (int)m : 0;
            for (size_t i = 0; border_free && i < m; ++i) call.literal |= (unsigned long long)(unsigned char)str[i] << (8 * i);
          }
          // (whatever fails in there -- declined, out of room, a HIP error --, the kernels below answer)
          const int rc = guard([&] { *out = cs::replace_re_column(call); });
          cs_regex_destroy(re);
          if (rc == CS_OK) return;
        }
      }
    }
    const HostText nd(str, s), rp(repl, s);
    *out = two_pass(col, ReplaceSize{nd.d(), nd.n, rp.n, maxrepl},
                    ReplaceWrite{nd.d(), rp.d(), nd.n, rp.n, maxrepl}, s, "k_replace_size", "k_replace_write");
  });
}

// Without a split limit the walk from the right meets the same tokens as the walk from the left
// when the delimiter is whitespace, or ASCII and border-free (no proper prefix that is also a
// suffix: occurrences cannot overlap, and the character/byte quirk of the token count
// (row_ops.h) does not arise): those calls take the split kernels.  Everything else -- a
// limit, a delimiter that can overlap itself, a multi-byte delimiter -- is located from the
// right.
static bool rsplit_walks_like_split(const char* delimiter, int maxsplit) {
  bool same = maxsplit <= 0;
  if (same && delimiter) {
    const int n = (int)strlen(delimiter);
    same = n > 0;
    for (int i = 0; same && i < n; ++i) same = (unsigned char)delimiter[i] < 128;
    for (int b = 1; same && b < n; ++b) same = memcmp(delimiter, delimiter + n - b, (size_t)b) != 0;
  }
  return same;
}
// The gate of the tile kernels (cs_split.hip).  From the left: whitespace, or a delimiter of 1..8 ASCII bytes.  From the
// right -- an rsplit that does not walk like split --: a limit on a one-byte ASCII delimiter (the first delimiters of a
// row are struck from its mask: split_parts.h TokensT).
static bool split_on_tile_kernels(const char* delimiter, const SplitArgs& a) {
  bool ascii_delim = delimiter && a.nb >= 1 && a.nb <= 8;
  for (int i = 0; ascii_delim && i < a.nb; ++i) ascii_delim = (unsigned char)delimiter[i] < 128;
  if (!a.reverse) return !delimiter || ascii_delim;
  return ascii_delim && a.nb == 1 && a.tokens > 0 && !cs::cfg("CS_RSPLIT_ROWWISE");
}
// The row-wise kernels: count the tokens of every row, size every column's rows, write.
static void split_rowwise(const cs_column* col, SplitArgs a, hipStream_t s, cs_column*** out_cols, int* ncols_out) {
  const int64_t rows = col->rows;
  note_route("split-rowwise");
  int ncols = 0;
  Buf counts;
  const unsigned nb = blocks_for(rows);
  if (rows) {
    counts = dev_alloc(sizeof(int32_t) * rows, s);
    Buf mx = dev_alloc(sizeof(int), s);
    CS_HIP(hipMemsetAsync(mx->p, 0, sizeof(int), s));
    {
      ProfScope ps("k_split_count", s);
      hipLaunchKernelGGL(k_split_count, dim3(nb), dim3(kBlock), 0, s, view_of(col), a,
                         ptr<int32_t>(counts), ptr<int>(mx));
    }
    ncols = read_back<int>(mx->p, s);
    a.ncols = ncols;
  }
  std::vector<std::unique_ptr<cs_column>> cols;
  if (ncols == 0) {
    // no columns: one all-null column (split.cu:756-757)
    cols.emplace_back(make_all_null(rows, s));
  } else {
    Buf lens = dev_alloc(sizeof(int32_t) * rows * ncols, s);
    Buf sums = dev_alloc(sizeof(int64_t) * (size_t)nb * ncols, s);
    {
      ProfScope ps("k_split_sizes", s);
      hipLaunchKernelGGL(k_split_sizes, dim3(nb), dim3(kBlock), 0, s, view_of(col), a,
                         ptr<int32_t>(counts), ncols, ptr<int32_t>(lens), ptr<int64_t>(sums));
    }
    // per-column offsets: one segmented scan over the fused block sums
    Buf offs = dev_alloc(sizeof(int64_t) * (rows + 1) * ncols, s);
    std::vector<int64_t> totals(ncols);
    offsets_from_lengths_segmented(ptr<int32_t>(lens), rows, ncols, ptr<int64_t>(offs), totals.data(), s);
    std::vector<SplitOut> outs(ncols);
    for (int k = 0; k < ncols; ++k) {
      auto* c = new cs_column;
      cols.emplace_back(c);
      c->rows = rows;
      c->nbytes = totals[k];
      c->chars = dev_alloc((size_t)totals[k], s);
      // each column owns its offsets: copy its segment out of the scan buffer
      c->offsets = dev_alloc(sizeof(int64_t) * (rows + 1), s);
      CS_HIP(hipMemcpyAsync(c->offsets->p, ptr<int64_t>(offs) + (int64_t)k * (rows + 1),
                            sizeof(int64_t) * (rows + 1), hipMemcpyDeviceToDevice, s));
      c->validity = validity_from_lengths(ptr<int32_t>(lens) + (int64_t)k * rows, rows, s);
      outs[k] = SplitOut{ptr<uint8_t>(c->chars), c->d_offsets()};
    }
    Buf d_outs = dev_alloc(sizeof(SplitOut) * ncols, s);
    CS_HIP(hipMemcpyAsync(d_outs->p, outs.data(), sizeof(SplitOut) * ncols, hipMemcpyHostToDevice, s));
    {
      ProfScope ps("k_split_write", s);
      hipLaunchKernelGGL(k_split_write, dim3(nb), dim3(kBlock), 0, s, view_of(col), a,
                         ptr<int32_t>(counts), ncols, ptr<const SplitOut>(d_outs));
    }
    CS_HIP(hipStreamSynchronize(s));  // `outs` staging is on the host stack
  }
  release_columns(cols, out_cols, ncols_out);
}

// NVStrings::split(delimiter,maxsplit,results) / split(maxsplit,results) -- split.cu:734-956
static int split_impl(const cs_column* col, const char* delimiter, int maxsplit, cs_stream stream, cs_column*** out_cols,
                      int* ncols_out, bool reverse) {
  return guard([&] {
    if (!col || !out_cols || !ncols_out) fail(CS_ERR_INVALID_ARG, "null argument");
    require_device();
    hipStream_t s = S(stream);
    SplitArgs a{nullptr, 0, maxsplit > 0 ? maxsplit + 1 : 0, 0, 0};
    a.reverse = reverse && !rsplit_walks_like_split(delimiter, maxsplit) ? 1 : 0;
    const HostText nd(delimiter, s);
    if (delimiter) {
      a.delim = nd.d();
      a.nb = nd.n;
    }
    if (split_on_tile_kernels(delimiter, a)) {
      std::vector<std::unique_ptr<cs_column>> fast;
      if (split_fast(SplitCall(col, reinterpret_cast<const unsigned char*>(delimiter), a.nb, a.tokens, a.reverse != 0, s), fast)) {
        release_columns(fast, out_cols, ncols_out);
        return;
      }
    }
    split_rowwise(col, a, s, out_cols, ncols_out);
  });
}

int cs_split(const cs_column* col, const char* delimiter, int maxsplit, cs_stream stream, cs_column*** out_cols,
             int* ncols_out) {
  return split_impl(col, delimiter, maxsplit, stream, out_cols, ncols_out, false);
}
// NVStrings::rsplit(delimiter, maxsplit, results) / rsplit(maxsplit, results) -- split.cu:960-1148
int cs_rsplit(const cs_column* col, const char* delimiter, int maxsplit, cs_stream stream, cs_column*** out_cols,
              int* ncols_out) {
  return split_impl(col, delimiter, maxsplit, stream, out_cols, ncols_out, true);
}

// NVText::tokenize(strs, delimiter) -- tokens.cu:123-155
int cs_tokenize(const cs_column* col, const char* delimiter, cs_stream stream, cs_column** out) {
  return guard([&] {
    if (!col || !out) fail(CS_ERR_INVALID_ARG, "null argument");
    require_device();
    hipStream_t s = S(stream);
    const int64_t rows = col->rows;
    note_route("rows");  // (tokenize_fast notes "tile" / "tile-segs" when it answers)
    if (rows == 0) {
      *out = make_all_null(0, s);
      return;
    }
    // byte-parallel tile kernels (cs_tokenize.hip) for whitespace or a few ASCII delimiters
    if (!delimiter || (*delimiter && strlen(delimiter) <= 4)) {
      const unsigned char* d = reinterpret_cast<const unsigned char*>(delimiter ? delimiter : "");
      if (tokenize_fast(col, d, (int)strlen(reinterpret_cast<const char*>(d)), s, out)) return;
    }
    TokArgs a;
    a.use_set = delimiter != nullptr;
    Buf set_more;
    a.set = make_charset(delimiter ? delimiter : "", set_more, s);
    tokdelims_finish(a, reinterpret_cast<const uint8_t*>(delimiter ? delimiter : ""), delimiter ? (int)strlen(delimiter) : 0);
    const unsigned nb = blocks_for(rows);
    Buf counts = dev_alloc(sizeof(int32_t) * rows, s);
    Buf sums = dev_alloc(sizeof(int64_t) * nb, s);
    {
      ProfScope ps("k_tok_count", s);
      hipLaunchKernelGGL(k_tok_count, dim3(nb), dim3(kBlock), 0, s, view_of(col), a, ptr<int32_t>(counts),
                         ptr<int64_t>(sums));
    }
    Buf tok_base = dev_alloc(sizeof(int64_t) * (rows + 1), s);
    int64_t ntok = offsets_from_lengths(ptr<int32_t>(counts), rows, ptr<int64_t>(tok_base), s, sums);
    Built b(ntok, Nulls::none, s);
    b.col->offsets = dev_alloc(sizeof(int64_t) * (ntok + 1), s);  // (before the lengths, as the pool has always seen them)
    Buf tok_lens;
    if (ntok) {
      tok_lens = dev_alloc(sizeof(int32_t) * ntok, s);
      ProfScope ps("k_tok_sizes", s);
      hipLaunchKernelGGL(k_tok_emit<0>, dim3(nb), dim3(kBlock), 0, s, view_of(col), a,
                         ptr<const int64_t>(tok_base), ptr<int32_t>(tok_lens), (const int64_t*)nullptr,
                         (uint8_t*)nullptr);
    }
    b.scan(ptr<int32_t>(tok_lens));
    b.alloc_chars();
    if (ntok) {
      ProfScope ps("k_tok_write", s);
      hipLaunchKernelGGL(k_tok_emit<1>, dim3(nb), dim3(kBlock), 0, s, view_of(col), a,
                         ptr<const int64_t>(tok_base), (int32_t*)nullptr, b.off, b.chars);
    }
    *out = b.col.release();
  });
}

// NVText::create_ngrams -- ngram.cu:32-110
int cs_ngrams(const cs_column* tokens, unsigned ngrams, const char* separator, cs_stream stream,
              cs_column** out) {
  return guard([&] {
    if (!tokens || !out) fail(CS_ERR_INVALID_ARG, "null argument");
    require_device();
    hipStream_t s = S(stream);
    if (ngrams == 0) ngrams = 2;
    if (!separator) separator = "";
    const int64_t rows = tokens->rows;
    note_route("rows");  // (ngrams_fast notes "tile-m8" .. "tile-m1" when it answers)
    if (rows == 0) {
      *out = share_column(tokens, s);
      return;
    }
    // tile kernel with closed-form offsets when no row is dropped (cs_ngram.hip)
    if (ngrams_fast(tokens, (int)ngrams, reinterpret_cast<const unsigned char*>(separator), (int)strlen(separator), s, out))
      return;
    const HostText sep(separator, s);
    // drop null and empty rows (ngram.cu:48-50)
    Buf flags = dev_alloc(sizeof(int32_t) * rows, s);
    hipLaunchKernelGGL(k_keep_flags, dim3(blocks_for(rows)), dim3(kBlock), 0, s, view_of(tokens),
                       ptr<int32_t>(flags));
    Buf pos = dev_alloc(sizeof(int64_t) * (rows + 1), s);
    int64_t count = offsets_from_lengths(ptr<int32_t>(flags), rows, ptr<int64_t>(pos), s);
    if (count <= (int64_t)ngrams) {
      // join(separator, "") over ALL rows, nulls contributing "" (ngram.cu:51-52)
      *out = join_rows(tokens, separator, "", s);
      return;
    }
    if (ngrams == 1) {
      *out = share_column(tokens, s);
      return;
    }
    Buf kept = dev_alloc(sizeof(int32_t) * count, s);
    hipLaunchKernelGGL(k_keep_scatter, dim3(blocks_for(rows)), dim3(kBlock), 0, s, ptr<const int32_t>(flags),
                       ptr<const int64_t>(pos), rows, ptr<int32_t>(kept));
    const int64_t ng = count - ngrams + 1;
    Buf lens = dev_alloc(sizeof(int32_t) * ng, s);
    {
      ProfScope ps("k_ngram_sizes", s);
      hipLaunchKernelGGL(k_ngram_sizes, dim3(blocks_for(ng)), dim3(kBlock), 0, s, view_of(tokens),
                         ptr<const int32_t>(kept), ng, (int)ngrams, sep.n, ptr<int32_t>(lens));
    }
    Built b = column_from_lengths(ptr<int32_t>(lens), ng, false, s);
    {
      ProfScope ps("k_ngram_write", s);
      hipLaunchKernelGGL(k_ngram_write, dim3(blocks_for(ng)), dim3(kBlock), 0, s, view_of(tokens),
                         ptr<const int32_t>(kept), ng, (int)ngrams, sep.d(), sep.n, b.off, b.chars);
    }
    *out = b.col.release();
  });
}

}  // extern "C"
