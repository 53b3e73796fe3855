// Private to the regex units (cs_regex.hip, cs_regex_pattern.hip, cs_regex_scan.hip): the compiled
// pattern, the launch types and device prologues the kernel families share, and the host helpers that more than one
// family calls (defined in cs_regex_pattern.hip, their notes with them; scan<MODE> in cs_regex_scan.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <vector>

#include "cs_internal.h"
#include "regex_program.h"
#include "regex_tdfa.h"
#include "regex_vm.h"

using namespace cs;

struct cs_regex {
  csrx::Program prog;
  std::vector<int32_t> blob;   // program only (ABI: cs_regex_blob)
  std::vector<int32_t> image;  // blob + executor extras
  std::vector<int32_t> tdfa;   // tagged DFA image (empty = not convertible)
  std::vector<int32_t> gtags;  // capture-group tag image of the tagged DFA (empty = no groups / not convertible)
  std::vector<int32_t> bits;   // bit-parallel form (regex_bits.h; empty = the program does not convert)
  Buf d_image;                 // uploaded lazily
  Buf d_tdfa;
  Buf d_gtags;
  Buf d_bits;
  bool empty_pattern = false;
  std::atomic<int> refs{1};    // handles given out by cs_regex_compile + one for the list of kept patterns
};

namespace cs {
namespace rx {

constexpr size_t kLdsBudget = 64 * 1024;

// ---- the list simulator, one thread per row ----
// One thread per row.  The compiled program image (instructions, classes,
// ASCII bitmaps, first-character prefilter) is staged into LDS once per
// workgroup; each thread's two ordered thread lists + closure stack also live
// in LDS, interleaved across lanes (slot-major) so accesses are bank-conflict
// free.  Programs whose lists do not fit in LDS run with the same code against
// a global scratch arena (the reference switches to a global `relists_mem`
// above 1000 instructions, regexec.cpp:81-95; count.cu:74-85).
// Workgroups walk the rows grid-stride so the arena is bounded by the grid.
struct Launch {  // kernel-visible part of the launch plan (POD)
  const int32_t* image;
  int image_words;
  int slots;        // 32-bit scratch slots per thread
  uint32_t* arena;  // global scratch (nullptr = lists in LDS)
  int image_in_lds;
};
struct Plan {
  Launch d;
  int threads;       // workgroup size
  size_t lds_bytes;  // dynamic LDS
  unsigned grid;
  bool small;
  Buf arena_buf;
};

struct RowSrc {
  ColView in;
  const uint8_t* flags;
  int64_t safe_end;  // chars bytes that may be read (logical size + allocation slack)
};

// common prologue: stage the image, carve per-thread scratch
struct Ctx {
  csvm::ProgView P;
  uint32_t* mem;
  int stride;
};
__device__ __forceinline__ Ctx setup(const Launch& L, const uint8_t* flags, uint32_t* smem) {
  Ctx c;
  const int32_t* img = L.image;
  int used = 0;
  if (L.image_in_lds) {
    for (int i = threadIdx.x; i < L.image_words; i += blockDim.x) smem[i] = (uint32_t)L.image[i];
    __syncthreads();
    img = (const int32_t*)smem;
    used = (L.image_words + 3) & ~3;
  }
  c.P = csvm::make_view(img, flags);
  if (L.arena) {
    c.mem = L.arena + (size_t)blockIdx.x * blockDim.x * L.slots + threadIdx.x;
  } else {
    c.mem = smem + used + threadIdx.x;
  }
  c.stride = blockDim.x;
  return c;
}

constexpr int kMaxGroups = 32;  // capture groups of extract; columns one launch of the span writers takes

// ---- tagged-DFA kernels (regex_tdfa.h): tables staged in LDS, no per-thread lists ----
struct TLaunch {
  const int32_t* tdfa;   // device image
  int tdfa_words;
  int in_lds;
  const int32_t* image;  // list-simulator image (global; consulted for non-ASCII chars only)
};
struct TCtx {
  cstd::View D;
  csvm::ProgView P;
};
template <bool IN_LDS>
__device__ __forceinline__ TCtx tsetup(const TLaunch& L, const uint8_t* flags, uint32_t* smem) {
  TCtx c;
  if (IN_LDS) {
    for (int i = threadIdx.x; i < L.tdfa_words; i += blockDim.x) smem[i] = (uint32_t)L.tdfa[i];
    __syncthreads();
    c.D = cstd::make_view((const int32_t*)smem);
  } else if (L.in_lds == 2) {
    // the tables stay in memory, the header and the image's last words (suffix, repetition counts, group map) come into LDS:
    // what the hot loops read of the image -- as scalar loads from memory each read also waited for every LDS access in flight
    // (replace_re of the dotted quad on this form: 5.1 against 4.7 ms)
    if (threadIdx.x < cstd::kHeadTailWords)
      smem[threadIdx.x] = threadIdx.x == 15 ? (uint32_t)cstd::kHeadTailWords
                                            : (uint32_t)L.tdfa[threadIdx.x < 32 ? (int)threadIdx.x : L.tdfa_words - cstd::kHeadTailWords + (int)threadIdx.x];
    __syncthreads();
    c.D = cstd::make_view((const int32_t*)smem, L.tdfa);
  } else {
    c.D = cstd::make_view(L.tdfa);
  }
  c.P = csvm::make_view(L.image, flags);
  return c;
}
// A row of the list kernels in LDS: the aligned 16-byte pieces that cover it (rows within the masks: seven at most), copied by
// the row's own thread -- the generic executor then walks LDS bytes instead of a chain of dependent loads from memory
// (k_tdfa_replace_list on the C5 pieces: 0.38 ms a launch from memory).  Returns the row's first byte; a longer row stays in memory.
constexpr int kListRowBytes = 112;
// (the pieces must lie inside the chars buffer -- [lo, hi): a caller's memory wrapped at an odd address has no slack around it)
__device__ __forceinline__ const uint8_t* list_row_to_lds(const uint8_t* src, int n, uint8_t* buf, const uint8_t* lo, const uint8_t* hi) {
  const int sh = (int)((uintptr_t)src & 15);
  if (sh + n > kListRowBytes || src - sh < lo || src - sh + ((sh + n + 15) & ~15) > hi) return src;
  const uint4* a = reinterpret_cast<const uint4*>(src - sh);
  for (int k = 0; k * 16 < sh + n; ++k) *reinterpret_cast<uint4*>(buf + 16 * k) = a[k];
  return buf + sh;
}

struct TPlan {
  TLaunch d;
  size_t lds_bytes;
  unsigned grid;
};
struct TileChoice {
  int R, cap;
  bool lng;
  int64_t span;  // the largest span of R consecutive rows (cap = that plus slack, rounded up to 128)
};

// ---- host helpers of more than one family (cs_regex_pattern.hip) ----
bool use_tdfa(const cs_regex* re);
bool use_tdfa_wide(const cs_regex* re);
enum { BITS_CONTAINS = 0, BITS_COUNT = 2, BITS_REPLACE = 3 };
double candidate_share(const cs_regex* re, const cs_column* col, hipStream_t s);
bool odd_rows_few(const cs_column* col, hipStream_t s);
bool bits_route(const cs_regex* re, const cs_column* col, hipStream_t s, int op, bool high_ok = false);
void upload(cs_regex* re, hipStream_t s);
TPlan tplan(cs_regex* re, int64_t rows, hipStream_t s);
Plan plan(cs_regex* re, int64_t rows, hipStream_t s);
TileChoice choose_tile(const cs_column* col, hipStream_t s, bool small = false);
const VirtualRows* pieces_for(const cs_column* col, const cs_regex* re, hipStream_t s, bool replacing, bool containing = false);
RowSrc row_src(const cs_column* col);
size_t gtags_lds_bytes(const cs_regex* re);
struct ScanStreamArgs;  // (regex_stream.h)
ScanStreamArgs stream_args(const cs_column* col, const TPlan& tp, const TileChoice& tc);

// ---- contains_re / match_re / count_re as a call (cs_regex_scan.hip; instantiated there for MODE 0, 1, 2) ----
struct ScanCall {
  const cs_column* col;
  cs_regex* re;
  void* results;     // one per row: uint8 flags (contains_re, match_re) or int32 counts (count_re) ...
  size_t esz;        // ... of this many bytes each
  int on_device;     // `results` is device memory
  hipStream_t s;
  int64_t* found;    // out: rows that hold a match / matches in the column (may be null)
  const char* name;  // the ProfScope of the stream or row-wise launch
};
template <int MODE>
void scan(const ScanCall& c);

}  // namespace rx
}  // namespace cs
