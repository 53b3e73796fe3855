// Internal host-side plumbing shared by the library's translation units:
// error handling, the device buffer cache, the column object and the
// lengths -> offsets scan.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <array>
#include <memory>
#include <string>
#include <vector>

#include "../../include/custrings_amd.h"
#include "cs_config.h"

namespace cs {

struct Error {
  int code;
  std::string msg;
};
[[noreturn]] void fail(int code, const std::string& msg);
void set_last_error(const std::string& msg);

#define CS_HIP(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      ::cs::fail(CS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
  } while (0)

// Runs `f`, mapping exceptions to status codes (nothing throws across the ABI).
template <class F>
int guard(F&& f) {
  try {
    f();
    return CS_OK;
  } catch (const Error& e) {
    set_last_error(e.msg);
    return e.code;
  } catch (const std::bad_alloc&) {
    set_last_error("host allocation failed");
    return CS_ERR_ALLOC;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return CS_ERR_INTERNAL;
  }
}

// Throws CS_ERR_NO_DEVICE unless cs_init succeeded; binds the calling thread to the library's
// device when its current device differs (hipSetDevice is per thread).
void require_device();
int bound_device();  // -1 before cs_init
// A C entry that makes a column from a column: `*out` is f()'s column, null when anything fails.
template <class F>
int column_entry(const cs_column* col, cs_column** out, F&& f) {
  return guard([&] {
    if (!col || !out) fail(CS_ERR_INVALID_ARG, "null column or output");
    *out = nullptr;
    require_device();
    *out = f();
  });
}
// One message per process on stderr and a counter (cs_fallback_count): a persistent single-pass
// kernel gave up and the host recomputed the column with the two-pass kernels.
void note_fallback(const char* what);
void note_route(const char* route);  // cs_debug_last_route (per thread)
void note_route_put_off();            // ... of a scan that left its rows with bytes >= 0x80 to a second launch
void note_route_pieces();             // ... of an op that ran on the column's pieces (cs_virtual.hip)

// ---- device memory ----------------------------------------------------------
// Buffers come from a size-bucketed cache over hipMalloc (one output allocation
// per produced buffer, no allocation inside kernels).  Every buffer carries 64
// bytes of slack so 16-byte vector loads may run past the logical end.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;     // usable bytes requested
  size_t capacity = 0;  // bytes actually held (0 for wrapped buffers)
  hipStream_t stream = nullptr;
  bool ipc_mapped = false;  // opened with hipIpcOpenMemHandle: closed, not freed (cs_column_ipc_import)
  bool borrowed = false;    // dev_wrap: memory this Buf does not keep alive (a zero-copy ingest's chars and offsets)
  ~DevBuf();
};
using Buf = std::shared_ptr<DevBuf>;
Buf dev_alloc(size_t bytes, hipStream_t stream);
Buf dev_wrap(const void* p, size_t bytes);  // caller-owned, never freed
// What an output column may keep of an input's buffer: the Buf itself, or -- when it is borrowed -- a pool copy of its
// bytes (made on `s` and waited for: the caller may take its memory back once the op returns).  Owned and IPC-mapped
// buffers stay alive through the Buf and are shared as they are.
Buf dev_owned(const Buf& b, hipStream_t s);
template <class T>
T* ptr(const Buf& b) {
  return b ? static_cast<T*>(b->p) : nullptr;
}
int64_t dev_bytes_in_use();

// pinned host scratch for small device->host results (per thread)
void* pinned_scratch(size_t bytes);

// unicode tables on the device (uploaded by cs_init)
const uint8_t* d_unicode_flags();
const uint16_t* d_charcases();
const uint8_t* h_unicode_flags();
const uint16_t* h_charcases();

}  // namespace cs

namespace cs {
struct OddRows;      // cs_virtual.hip: the rows that hold a byte >= 0x80 or a NUL, as a list and as a mask per 64-row tile
struct VirtualRows;  // cs_virtual.hip: the column's rows cut into pieces of at most 92 bytes (a second column over the same chars)
}
// ---- the column ---------------------------------------------------------------
struct cs_column {
  int64_t rows = 0;
  int64_t nbytes = 0;
  mutable int64_t null_count = -1;  // -1 = not counted yet
  mutable int64_t max_span64 = -1;  // max bytes spanned by 64 consecutive rows (tile kernels); -1 = unknown
  mutable int64_t max_row = -1;     // longest row in bytes; -1 = unknown
  mutable int drops = -1;           // 1: some row is null or empty (rows create_ngrams drops), 0: none; -1 = unknown
  mutable int plain_bytes = -1;     // 1: no NUL byte and no lead byte announcing over an ASCII byte; -1 = unknown
  mutable int high_sample = -1;     // 1: a sample of the chars (three 64 KiB windows) holds a byte >= 0x80; -1 = not looked at
  mutable std::shared_ptr<std::array<uint32_t, 256>> byte_hist;  // byte counts of the same sample (a hint for kernel choice); null = not taken
  mutable std::shared_ptr<cs::VirtualRows> virt;  // the view of a long-row column as pieces (built on first use; cs_virtual.hip)
  mutable int virt_state = 0;                     // 0: not looked at, 1: `virt` holds it, -1: the column has none
  mutable std::shared_ptr<cs::OddRows> odd;       // the rows with a byte >= 0x80 or a NUL (built on first use; cs_virtual.hip)
  cs::Buf chars, validity;  // validity may be null (all valid)
  // Row extents: int64 offsets (`offsets`) and / or int32 offsets (`offsets32`, columns whose
  // chars stay below 2 GiB -- what split produces: half the bytes written per output row).  A
  // column born with int32 offsets gets its int64 form on first use by a kernel that reads
  // int64 (d_offsets(), under a lock; the widened buffer is kept).
  mutable cs::Buf offsets;
  cs::Buf offsets32;
  const uint8_t* d_chars() const { return cs::ptr<const uint8_t>(chars); }
  const int64_t* d_offsets() const;
  const int32_t* d_offsets32() const { return cs::ptr<const int32_t>(offsets32); }
  const uint8_t* d_validity() const { return cs::ptr<const uint8_t>(validity); }
  // the other column gets the same (immutable) extents (copies of them where they are borrowed: dev_owned)
  void share_extents_with(cs_column* o, hipStream_t s) const;
};

// ---- the category: sorted unique keys + one int32 code per row (-1 / key 0 conventions: cs_category.hip)
struct cs_category {
  std::unique_ptr<cs_column> keys;
  cs::Buf values;  // int32[rows]
  int64_t rows = 0;
};

namespace cs {

struct ColView {  // passed to kernels by value
  const uint8_t* chars;
  const int64_t* offsets;
  const uint8_t* validity;
  int64_t rows;
};
inline ColView view_of(const cs_column* c) {
  return ColView{c->d_chars(), c->d_offsets(), c->d_validity(), c->rows};
}
inline hipStream_t S(cs_stream s) { return static_cast<hipStream_t>(s); }
inline unsigned blocks_for(int64_t rows) { return (unsigned)((rows + 255) / 256); }
inline size_t validity_bytes(int64_t rows) { return (size_t)((rows + 63) / 64) * 8; }

// A second handle on the column's (immutable) buffers: the result of an op that changes nothing.  Borrowed buffers are
// copied (dev_owned), so that no column an op returns refers to memory the library does not own.
cs_column* share_column(const cs_column* in, hipStream_t s);
// Empty column with `rows` rows, all null (NVStrings(count)) or zero rows.
cs_column* make_all_null(int64_t rows, hipStream_t s);

// Exclusive scan of int32 lengths (negative = null row, counts as 0) into int64
// offsets[n+1]; returns the total (synchronises `s`).  When `block_sums` is
// given it must hold the per-256-row sums already (fused into the caller's size
// kernel) and the lengths are read only once.
// `meta` (optional): the column metadata the tile kernels ask for, as a by-product of the same pass -- the longest row and
// the largest byte span of 64 consecutive rows starting at a multiple of 64 (what max_row_bytes / max_span64 would compute
// with passes of their own over the finished offsets).
struct LenMeta {
  int64_t max_row = -1, max_span64 = -1;
  void give(cs_column* c) const {
    if (max_row >= 0) c->max_row = max_row;
    if (max_span64 >= 0) c->max_span64 = max_span64;
  }
};
int64_t offsets_from_lengths(const int32_t* lens, int64_t n, int64_t* offsets, hipStream_t s,
                             Buf block_sums = nullptr, LenMeta* meta = nullptr);
void offsets_from_lengths_async(const int32_t* lens, int64_t n, int64_t* offsets, hipStream_t s);  // nothing read back, no wait: the total is offsets[n] on the device
// the same and the validity mask (length >= 0) from one pass over the lengths
int64_t offsets_and_validity_from_lengths(const int32_t* lens, int64_t n, int64_t* offsets, Buf* validity, hipStream_t s, LenMeta* meta = nullptr);
// Segmented variant: `segs` independent arrays of n lengths laid out back to
// back (lens[seg * n + i]); offsets[seg * (n + 1) + i]; totals[seg] on the host.
// (`largest_host`, optional: the largest length of every segment -- for per-tile byte counts that is the column's largest
// 64-row span, by-product of the same pass)
void offsets_from_lengths_segmented(const int32_t* lens, int64_t n, int segs, int64_t* offsets,
                                    int64_t* totals_host, hipStream_t s, int64_t* largest_host = nullptr);
// Validity bitmask from int32 lengths (bit set when len >= 0).
Buf validity_from_lengths(const int32_t* lens, int64_t n, hipStream_t s);
int64_t count_nulls(const cs_column* c, hipStream_t s);
// Largest byte span of 64 consecutive rows starting at a multiple of 64 (cached
// in the column; sizes the LDS staging buffers of the tile kernels).
int64_t max_span64(const cs_column* c, hipStream_t s);
int64_t max_row_bytes(const cs_column* c, hipStream_t s);
bool bytes_plain(const cs_column* c, hipStream_t s);
// Same for tiles of `per` consecutive rows (per = 64 is the cached one).
int64_t max_span_rows(const cs_column* c, int per, hipStream_t s);
bool sample_has_high_bytes(const cs_column* c, hipStream_t s);
const uint32_t* sample_byte_hist(const cs_column* c, hipStream_t s);  // 256 counts over the same three windows (a hint, cached on the column)  // a hint (kernel choice only): non-ASCII text, by three windows of the chars
int64_t count_spans64_over(const cs_column* c, int64_t limit, hipStream_t s);
bool few_spans64_over(const cs_column* c, int64_t limit, hipStream_t s);  // all but a few 64-row tiles fit `limit` bytes
// Workgroups (256 threads, `lds` dynamic bytes) of `kern` resident at once on the device,
// capped by `wanted`: grid size of the persistent tile kernels.
unsigned resident_grid(const void* kern, size_t lds, int64_t wanted);
// Launches a persistent kernel (256 threads, `lds` dynamic bytes -- above 48 KB the kernel's limit is raised) on the
// grid resident_grid gives it; returns that grid.
template <class... P, class... A>
unsigned launch_resident(void (*kern)(P...), size_t lds, int64_t wanted, hipStream_t s, const A&... args) {
  const void* k = reinterpret_cast<const void*>(kern);
  if (lds > 48 * 1024) CS_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const unsigned grid = resident_grid(k, lds, wanted);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, args...);
  CS_HIP(hipGetLastError());
  return grid;
}
// Rows per tile of the row-tile kernels: the largest R of 64 / 32 / 16 whose widest R-row tile, plus `slack` bytes, fits
// the prefetch registers (cstile::kPfBytes), and that tile's span; R = 0 when none fits.  With `outliers` a column no R
// fits still gets 64-row tiles sized for all but a few (the kernel takes a tile beyond the staging size straight from
// memory), unless CS_NO_OUTLIER_TILES is set.
struct TilePlan {
  int R;
  int64_t span;
};
TilePlan plan_row_tiles(const cs_column* c, int slack, hipStream_t s, bool outliers = false);
// What a kernel that stages its tiles in LDS is launched with, from plan_row_tiles: a wave's staging buffer holds `cap`
// bytes (the widest tile and `slack`, 32 at least, rounded up to 16), a wave takes a tile at a time and a workgroup has
// four waves.
// A wave's LDS is `bufs` buffers of `cap` bytes and `extra` bytes more; R = 0 as well when four of them exceed `ceiling`.
struct WaveLds {
  int bufs;
  size_t extra, ceiling;
};
struct StagedTiles {
  int R = 0, cap = 0;
  long long ntiles = 0;
  int64_t grid = 0;  // workgroups wanted (launch_resident caps them)
  size_t lds = 0;    // dynamic LDS of a workgroup
};
StagedTiles plan_staged_tiles(const cs_column* c, int slack, bool outliers, WaveLds w, hipStream_t s);

// Results to the caller's buffer, device or host: the kernels write to `dev` (a temporary for a host caller).
struct ResultsOut {
  Buf tmp;
  void* caller;
  void* dev;
  size_t bytes;
  ResultsOut(void* results, size_t nbytes, int on_device, hipStream_t s) : caller(results), dev(results), bytes(nbytes) {
    if (on_device) return;
    tmp = dev_alloc(bytes ? bytes : 1, s);
    dev = tmp->p;
  }
  void copy_back(hipStream_t s) const {  // (nothing waits: finish, read_count or the caller synchronises)
    if (tmp) CS_HIP(hipMemcpyAsync(caller, dev, bytes, hipMemcpyDeviceToHost, s));
  }
  void finish(hipStream_t s) const {
    copy_back(s);
    CS_HIP(hipStreamSynchronize(s));
  }
};
// A 64-bit count the kernels add to: zeroed on the device; read_count brings it back (synchronises `s`).
Buf zeroed_count(hipStream_t s);
int64_t read_count(const Buf& acc, hipStream_t s);
// One word of device memory -- a flag, a maximum, a position -- brought back through the pinned scratch (synchronises `s`).
template <class T>
T read_back(const void* d, hipStream_t s) {
  T* host = (T*)pinned_scratch(sizeof(T));
  CS_HIP(hipMemcpyAsync(host, d, sizeof(T), hipMemcpyDeviceToHost, s));
  CS_HIP(hipStreamSynchronize(s));
  return *host;
}

template <class T>
struct DevArray {  // caller array made device-visible (copied when it lives on the host)
  Buf tmp;
  const T* d = nullptr;
  DevArray(const T* p, int64_t n, int on_device, hipStream_t s) {
    if (on_device || !p || n == 0) {
      d = p;
      return;
    }
    tmp = dev_alloc(sizeof(T) * (size_t)n, s);
    CS_HIP(hipMemcpyAsync(tmp->p, p, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, s));
    d = ptr<const T>(tmp);
  }
};
struct HostText {  // small host string on the device (nullptr stays nullptr)
  Buf buf;
  int n = -1;
  HostText(const char* t, hipStream_t s) {
    if (!t) return;
    n = (int)strlen(t);
    buf = dev_alloc((size_t)n + 1, s);
    CS_HIP(hipMemcpyAsync(buf->p, t, (size_t)n + 1, hipMemcpyHostToDevice, s));
  }
  const uint8_t* d() const { return ptr<const uint8_t>(buf); }
};
}  // namespace cs
namespace csrow {
struct CharSet;
}
namespace cs {
// cs_ops.hip: the character set of a UTF-8 string of any length (strip, tokenize with a delimiter set, the NVText counters);
// `more` keeps what does not fit the struct alive for the caller's kernels
csrow::CharSet make_charset(const char* s, Buf& more, hipStream_t st);
// Row-wise concatenation of columns into one new column.
cs_column* concat_columns(const std::vector<const cs_column*>& cols, hipStream_t s);

// cs_virtual.hip: a long-row column as a column of pieces that fit the 96-bit masks
struct VirtualRows {
  std::unique_ptr<cs_column> col;  // the pieces: the same chars buffer, offsets of their own
  Buf first;                       // int64[rows + 1]: row r's pieces are first[r] .. first[r + 1] - 1
};
const VirtualRows* virtual_rows(const cs_column* col, hipStream_t s);
// the rows that hold a byte >= 0x80 or a NUL byte -- the rows the 96-bit-mask forms of the regex kernels do not take: replace_re
// leaves them holes in its single pass and fills them from a thread a row (cs_regex.hip); column metadata, one pass over the chars
struct OddRows {
  int64_t count = 0;
  Buf list;   // int32[count]: their indices, ascending
  Buf mask;   // uint64[tiles]: bit j of word t = row 64 t + j is such a row
  Buf first;  // int64[tiles + 1]: list[first[t]] is tile t's first
};
const OddRows* odd_rows(const cs_column* col, hipStream_t s);
int virtual_piece_bytes();
int64_t virtual_reduce_u8(const VirtualRows* vr, const uint8_t* piece_res, int64_t rows, uint8_t* out, hipStream_t s);
int64_t virtual_reduce_i32(const VirtualRows* vr, const int32_t* piece_res, int64_t rows, int32_t* out, hipStream_t s);
cs_column* virtual_rows_to_rows(const cs_column* col, const VirtualRows* vr, std::unique_ptr<cs_column> pieces_out, hipStream_t s);
// cs_regex.hip: one replace_re call, all of its parameters in sight.  cs_replace_re fills the first six; cs_replace adds its
// needle and cs_replace_with_backrefs its template, and both ask for the single pass only: their own kernels are the
// fallback, so replace_re_column throws where the single pass does not apply or gives up.
struct ReplaceCall {
  const cs_column* col;
  const cs_regex* re;
  const char* repl;  // the replacement text (host), `rb` bytes and a NUL
  int rb;
  int maxrepl;  // replacements per row at most; negative: all
  hipStream_t s;
  // the needle itself when it has at most eight bytes and no border (no proper prefix that is also a suffix: occurrences
  // cannot overlap), first byte lowest: the stream kernel then finds the matches by byte comparison; literal_len 0: none
  unsigned long long literal = 0;
  int literal_len = 0;
  // the template (a csvm::BackrefTemplate): host copy (sizing: how much a match can grow), device copy, bytes of its text;
  // null: plain replace_re
  const void* tmpl_host = nullptr;
  const void* tmpl_dev = nullptr;
  int tmpl_text_bytes = 0;
  bool single_pass_only = false;
};
cs_column* replace_re_column(const ReplaceCall& c);  // the new column (the caller's), or throws
// cs_split.hip: one split / rsplit call on the tile kernels, all of its parameters in sight; what the kernels take of the
// delimiter is derived here, once.  cs_ops.hip (split_impl) makes it where its gates let the call through.
struct SplitCall {
  const cs_column* col;
  const unsigned char* delim;  // the delimiter (host): `dlen` = 1..8 ASCII bytes; nullptr: whitespace
  int dlen;
  int tokens;    // columns at most (the split limit + 1); 0 or less: no limit
  bool reverse;  // rsplit with a limit on a one-byte delimiter (the masked kernels only)
  hipStream_t s;
  int mode = 0;                // 0: a one-byte delimiter, 1: whitespace, 2: a delimiter of 2..8 bytes
  unsigned long long d64 = 0;  // the delimiter's bytes, first byte lowest
  uint32_t dpat = 0;           // its first byte in every byte of a word
  SplitCall(const cs_column* col_, const unsigned char* delim_, int dlen_, int tokens_, bool reverse_, hipStream_t s_)
      : col(col_), delim(delim_), dlen(dlen_), tokens(tokens_), reverse(reverse_), s(s_) {
    mode = !delim ? 1 : (dlen > 1 ? 2 : 0);
    for (int i = 0; delim && i < dlen; ++i) d64 |= (unsigned long long)delim[i] << (8 * i);
    dpat = 0x01010101u * (delim ? (uint32_t)delim[0] : 0u);
  }
};
// the tiles of a split call (split_tile_plan): rows a sub-tile, its largest span and the LDS tiles that hold it
struct SplitPlan {
  bool fits = false;      // some tile size fits the LDS (else: the row-wise kernels)
  int rows_per_sub = 64;  // 64, or 32 / 16 / 8: the first generation on rows of hundreds of bytes
  bool outliers = false;  // 64-row tiles sized for all but a few sub-tiles (the first generation reads those from memory)
  int64_t span = 0;       // bytes of the largest sub-tile (outliers: of the largest that is staged)
  int cap_in = 0, cap_out = 0;  // the first generation's in and out tile
  int walk_words = 0;     // mask words of the sentinel walk, 3 or 6; 0: the general token walker
};
// the tile kernels; false: not this path's call (nothing done), the row-wise kernels answer
bool split_fast(const SplitCall& c, std::vector<std::unique_ptr<cs_column>>& cols);
// cs_split1.hip (the experiments build): the single pass.  1: columns written; 0: not this path's case (nothing done);
// -1: it gave up (fallback counted)
int split_single(const SplitCall& c, const SplitPlan& p, std::vector<std::unique_ptr<cs_column>>& cols);
// cs_radix.hip: stable LSD radix sort of n (64-bit key, 32-bit item) pairs by key, ascending, in place (synchronises `s`)
void radix_sort_pairs64(uint64_t* keys, int32_t* items, int64_t n, hipStream_t s);
// cs_category.hip: keys = sorted unique rows (null first), values[r] = index of row r's key
cs_category* category_build(const cs_column* col, hipStream_t s);
// cs_category.hip: out[i] = table[codes[i]] for n codes (a negative code stays as it is); queued on `s`, not waited for
void remap_codes(const int32_t* codes, int64_t n, const int32_t* table, int32_t* out, hipStream_t s);
// cs_category.hip: the merge that follows the exchange of a distributed build.  `sets[r]` = rank r's sorted key set
// (this rank's own, local->keys, at `rank`).  The category of their concatenation has the merged keys, and its codes are
// the ranks' old-code -> new-code tables, back to back: the local rows' codes go through this rank's slice of them into
// `values` (room for local->rows int32; null: allocated here, after the build).  Waits for `s`: the sets may leave scope.
cs_category* merge_key_sets(const cs_category* local, const std::vector<const cs_column*>& sets, int rank, Buf values, hipStream_t s);
// cs_array.hip: rows of `col` at the given device positions; with `null_when_negative` a negative
// position yields a null row instead of CS_ERR_RANGE
cs_column* gather_rows(const cs_column* col, const int32_t* d_pos, int64_t n, hipStream_t s, bool null_when_negative = false);
// cs_array.hip: the column of `count` (pointer, byte length) spans in device memory (std::pair<const char*, size_t>; null
// pointer = null row), sorted when `sorttype` says so (NVStrings::sorttype bits): create_from_index and from_csv
cs_column* column_from_spans(const void* spans, int64_t count, int sorttype, hipStream_t s);
// cs_array.hip: every row of `col` in one row, `delimiter` between them; a null row is `narep`, or without one leaves
// nothing, no delimiter either (cs_join, and create_ngrams of a column with no more tokens than an n-gram takes)
cs_column* join_rows(const cs_column* col, const char* delimiter, const char* narep, hipStream_t s);
// The output column of an op that sizes its rows first (int32 lengths, negative = null row): the one host tail from
// lengths to a column.  The constructor makes the column with its row count and nulls; scan() allocates the offsets
// and scans the lengths into them (the total is the column's nbytes, the scan's metadata goes to the column; no rows:
// one zero offset); alloc_chars() allocates the chars (no bytes: an empty buffer) and, for Nulls::separate, writes the
// validity.  Between the two the caller may act on the total or read a flag of its size kernel.  The caller's write
// kernel fills `chars` by `off`; prefer_offsets32 afterwards keeps the narrow offsets.
enum class Nulls {
  shared,    // the input's validity and null_count (null rows stay null; columns are immutable, so share)
  none,      // no row can be null: null_count = 0
  separate,  // validity from the negative lengths, by a kernel of its own once the chars are allocated
  fused,     // validity from the negative lengths, written by the scan's own pass over them
};
struct Built {
  std::unique_ptr<cs_column> col;
  const int64_t* off = nullptr;  // col's int64 offsets (after scan)
  uint8_t* chars = nullptr;      // col's chars (after alloc_chars)
  Built(int64_t rows, Nulls nulls, hipStream_t s);
  Built(const cs_column* like, hipStream_t s);  // like's rows, Nulls::shared with it
  // `block_sums`: the per-256-row sums, when the caller's size kernel fused them
  int64_t scan(const int32_t* lens, Buf block_sums = nullptr);
  uint8_t* alloc_chars();

 private:
  Nulls nulls_;
  hipStream_t s_;
  const int32_t* lens_ = nullptr;
};
// scan and alloc_chars with nothing in between
Built column_from_lengths(const int32_t* lens, int64_t rows, bool any_null_possible, hipStream_t s);
void prefer_offsets32(cs_column* c, hipStream_t s);
// hands a vector of columns to a C caller: a malloc'ed array of the released pointers and their count (cs_free frees it)
void release_columns(std::vector<std::unique_ptr<cs_column>>& cols, cs_column*** out_cols, int* ncols_out);

// profiling hooks (cs_prof_*): time a named kernel launch with HIP events
struct ProfScope {
  const char* name;
  hipStream_t s;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(const char* name, hipStream_t s);
  ~ProfScope();
};

}  // namespace cs
