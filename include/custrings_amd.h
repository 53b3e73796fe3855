/* custrings_amd.h -- C ABI of the MI355X-native columnar string engine.
 *
 * This is the drop-in boundary for the hot path of rapidsai/custrings: the
 * entry points below are what the reference's host classes (NVStrings /
 * NVCategory / NVText, /root/reference/cpp/include/) need from a device
 * back-end for split / find / contains / replace / strip / lower,
 * contains_re / replace_re, the category key build and tokenize / ngrams.
 * Each function cites the reference interface it stands in for.
 *
 * Conventions
 *  - Strings live in an Arrow-style device column: chars (u8), offsets
 *    (rows+1 entries; int64, or int32 for columns an op produced with less
 *    than 2 GiB of chars -- cs_column_get_view always hands out int64,
 *    widening once on demand), validity bitmask (LSB-first, bit=1 valid,
 *    NULL pointer = all valid).  Columns are immutable and reference counted
 *    internally; every producing call returns a new handle the caller must
 *    release with cs_column_destroy (the reference's "new instance, caller
 *    destroys" rule, NVStrings.h:52-57,156).
 *  - Scalars (patterns, delimiters, replacement text) are host NUL-terminated
 *    UTF-8, exactly as in the reference.
 *  - Array arguments carry an `on_device` flag like the reference's trailing
 *    `bool devmem` (NVStrings.h:861,907,963): non-zero = device pointer.
 *  - Every call returns a cs_status; no C++ exception crosses the boundary.
 *    cs_last_error() returns the thread-local message of the last failure.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls
 *    that return host-visible values synchronise that stream before returning.
 *  - There is no CPU fallback: without a usable gfx950 device every compute
 *    call fails with CS_ERR_NO_DEVICE.
 */
#ifndef CUSTRINGS_AMD_H
#define CUSTRINGS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cs_column cs_column;     /* device strings column            */
typedef struct cs_regex cs_regex;       /* compiled pattern (host + device) */
typedef struct cs_category cs_category; /* sorted unique keys + int32 codes */
typedef void* cs_stream;                /* hipStream_t                      */

typedef enum cs_status {
  CS_OK = 0,
  CS_ERR_INVALID_ARG = 1, /* std::invalid_argument in the reference */
  CS_ERR_ALLOC = 2,       /* std::runtime_error("allocate error")   */
  CS_ERR_HIP = 3,
  CS_ERR_NO_DEVICE = 4,
  CS_ERR_RANGE = 5, /* column does not fit an int32-offset export */
  CS_ERR_INTERNAL = 6
} cs_status;

/* Borrowed, read-only view of a column's device buffers. */
typedef struct cs_column_view {
  const uint8_t* chars;
  const int64_t* offsets; /* rows + 1 entries, offsets[0] == 0 */
  const uint8_t* validity; /* may be NULL */
  int64_t rows;
  int64_t nbytes;
  int64_t null_count;
} cs_column_view;

/* ---- library ----------------------------------------------------------- */
int cs_version(void);
/* 1 when the library was built with the experiments (`make exp`: the one-pass split and strip kernels -- bit-exact,
 * measured slower than the product's two passes, kept out of the product library), else 0. */
int cs_has_experiments(void);
const char* cs_last_error(void);
int cs_device_count(void);
/* Binds the calling thread to `device`, creates the stream-ordered memory
 * pool and uploads the unicode tables (reference: lazy get_unicode_flags /
 * get_charcases, NVStringsImpl.cu:69-91). Idempotent. */
int cs_init(int device);
/* A stream the caller is about to destroy: the buffer cache stops recording release events on it (blocks released after
 * a second stream appeared are ordered behind every stream that allocated so far; a destroyed stream is otherwise only
 * noticed when recording on its stale handle fails, which HIP does not promise).  The null stream cannot be forgotten. */
int cs_stream_forget(cs_stream stream);
/* Device the process is bound to (cs_init), or -1.  Compute calls from any host
 * thread run on it (the library re-binds the calling thread when needed). */
int cs_current_device(void);
/* Number of times a persistent single-pass kernel gave up (its grid was not
 * fully resident, e.g. a co-tenant on the device) and the column was recomputed
 * with the two-pass kernels.  Correct either way; a benchmark should see 0. */
int64_t cs_fallback_count(void);
/* Diagnostics / tests: which route the calling thread's last regex stream launch took -- "bits" (the bit-parallel form,
 * regex_bits.h), "chain", "units", "literal", "wide", "plain", "brefs", "brefs-chain" -- or "" when the call used other kernels. */
const char* cs_debug_last_route(void);
/* The CS_* switches (measurement aids, route overrides, opt-in experiments) are read from the environment ONCE, at the
 * library's first look (cs_init); the dispatch paths never call getenv.  This changes one at run time, thread-safely
 * (value NULL: unset) -- for tests and tools; a production host sets its environment before cs_init. */
int cs_config_set(const char* name, const char* value);
/* Bytes currently held by live columns/categories on this device. */
int64_t cs_device_bytes_in_use(void);
/* The buffer pool (reference: the RMM pool behind device_alloc, cpp/src/util.inl:90-106): released blocks are kept and
 * re-used; a new block's capacity is rounded up to a geometric size class (eight per octave, 3 % of headroom) so that a
 * column a little larger than the last one finds a block.  cs_debug_malloc_count: hipMalloc calls so far (tests: a
 * pipeline on columns of slightly different sizes allocates once); cs_pool_cached_bytes: bytes idle in the pool (bounded
 * by half the device's memory, CS_POOL_MAX_MB); cs_pool_trim: give idle blocks back down to `keep_bytes`. */
int64_t cs_debug_malloc_count(void);
/* What this box's memory delivers to hand-written streaming kernels (custrings_amd/csrc/box_rates.h), in TB/s (bytes read
 * + bytes written over the median of `reps` launches): tbps[0] a 16-byte-a-lane copy, [1] a read-only stream, [2] a
 * write-only stream, [3] the split emit kernel's shape -- one read stream into 20 x (256 + 192 + 8)-byte pieces per
 * 64-row sub-tile -- with plain stores, [4] the same with non-temporal stores; tbps[5]: the shader clock in GHz under an
 * all-CU integer + LDS load (six doubles in all).  `mbytes`: buffer size.  bench.py prints them as the `box` block of
 * its line (the headline's kernels follow the box's mixed read / write rate and its clock). */
int cs_box_rates(int64_t mbytes, int reps, cs_stream stream, double* tbps);
int64_t cs_pool_cached_bytes(void);
int cs_pool_trim(int64_t keep_bytes);

/* ---- column construction / export -------------------------------------- */
/* NVStrings::create_from_array (NVStrings.h:86): NULL entry = null row. */
int cs_column_from_host_strings(const char* const* strs, int64_t rows, cs_stream stream,
                                cs_column** out);
/* NVStrings::create_from_offsets (NVStrings.h:116): int32 Arrow offsets,
 * optional validity bitmask; buffers are copied. */
int cs_column_from_offsets32(const char* chars, int64_t rows, const int32_t* offsets,
                             const uint8_t* validity, int on_device, cs_stream stream,
                             cs_column** out);
/* Native ingest: int64 offsets. copy=0 wraps caller-owned DEVICE buffers that
 * must outlive the handle (zero-copy); copy=1 copies (host or device). */
int cs_column_from_offsets64(const uint8_t* chars, int64_t rows, const int64_t* offsets,
                             const uint8_t* validity, int on_device, int copy,
                             cs_stream stream, cs_column** out);
/* NVStrings::create_ipc_transfer / create_from_ipc (NVStrings.h:132,214; cpp/include/ipc_transfer.h:31-107):
 * a column handed to another process of the same node without a copy.  The exporter fills a plain
 * struct with the HIP IPC handles of the column's buffers (chars, offsets, validity) and their sizes;
 * the struct travels by any byte channel (pipe, socket, shared memory); the importer maps the buffers
 * and gets a read-only column over them.  The exporter's column must stay alive until every importer
 * has destroyed its handle.  (The reference ships an array of custring_view pointers plus the memory
 * they point into, rebased by the importer; the native layout has no pointers to rebase.) */
typedef struct cs_ipc_column {
  unsigned char chars[64], offsets[64], validity[64]; /* hipIpcMemHandle_t each */
  int64_t rows, nbytes, null_count;
  int32_t offset_width; /* 4 or 8 */
  int32_t has_validity;
  int32_t device;       /* the exporter's device ordinal (the importer must be able to reach it) */
  int32_t reserved;
} cs_ipc_column;
int cs_column_ipc_export(const cs_column* col, cs_ipc_column* out);
int cs_column_ipc_import(const cs_ipc_column* ipc, cs_column** out);
/* NVStrings::create_from_strings(std::vector<NVStrings*>) (NVStrings.h:125):
 * row-wise concatenation of `n` columns into a new column. */
int cs_column_concat(const cs_column* const* cols, int n, cs_stream stream, cs_column** out);
/* NVStrings::sublist(start, end) with step 1 (NVStrings.h:261): rows
 * [first, first + rows) as a new column (offsets rebased to 0).  This is also
 * how a column is cut into row-range shards for the multi-GPU path. */
int cs_column_slice(const cs_column* col, int64_t first, int64_t rows, cs_stream stream,
                    cs_column** out);
/* NVStrings::destroy (NVStrings.h:156). NULL is ignored. */
int cs_column_destroy(cs_column* col);
/* NVStrings::size (NVStrings.h:167) and friends. */
int64_t cs_column_rows(const cs_column* col);
int64_t cs_column_nbytes(const cs_column* col);
/* Bytes per offset the column was produced with: 4 (int32, an op's output below
 * 2 GiB of chars) or 8.  Either way cs_column_get_view hands out int64 offsets. */
int cs_column_offset_width(const cs_column* col);
int64_t cs_column_null_count(const cs_column* col);
/* What the column already knows about itself, without computing anything (diagnostics / tests): out[0] largest byte
 * span of 64 consecutive rows starting at a multiple of 64, out[1] longest row in bytes -- both upper bounds when an op
 * derived them as a by-product, exact when a pass measured them --, out[2] "plain bytes" (1 / 0), out[3] the non-ASCII
 * sample (1 / 0); -1 = not known yet (the first op that needs the number pays a pass for it).  The reference sizes its
 * strings once at ingest (NVStringsImpl.cu:399-444); here producers hand the numbers on so that ops in a chain do not. */
int cs_column_cached_meta(const cs_column* col, int64_t out[4]);
int cs_column_get_view(const cs_column* col, cs_column_view* view);
/* NVStrings::create_offsets (NVStrings.h:207): int32 offsets (rows+1), chars,
 * optional bitmask.  CS_ERR_RANGE when nbytes >= 2^31. */
int cs_column_export_offsets32(const cs_column* col, char* chars, int32_t* offsets,
                               uint8_t* validity, int on_device, cs_stream stream);
/* Native egress, int64 offsets. */
int cs_column_export_offsets64(const cs_column* col, uint8_t* chars, int64_t* offsets,
                               uint8_t* validity, int on_device, cs_stream stream);
/* NVStrings::byte_count (NVStrings.h:354): bytes per row, -1 for null rows;
 * *total receives the sum over non-null rows. */
int cs_column_byte_count(const cs_column* col, int32_t* lengths, int on_device,
                         cs_stream stream, int64_t* total);
/* NVStrings::set_null_bitarray (NVStrings.h:225): bit=1 valid, LSB first;
 * *null_count receives the number of cleared bits. */
int cs_column_null_bitarray(const cs_column* col, uint8_t* bitarray, int empty_is_null,
                            int on_device, cs_stream stream, int64_t* null_count);

/* ---- re-arrangement / combination -------------- */
/* NVStrings::create_from_index (NVStrings.h:98; NVStringsImpl.cu:209-325): `pairs`
 * is an array of `count` std::pair<const char*, size_t> (pointer, byte length;
 * NULL pointer = null row, zero length = empty string).  The pointers address
 * device-visible memory; on_device says where the PAIR ARRAY lives (the
 * reference's `devmem`).  sorttype: NVStrings::sorttype bits (0 none, 1 length,
 * 2 name): ascending, nulls first.  An unreadable pointer surfaces as
 * CS_ERR_INVALID_ARG ("bad_device_ptr"). */
int cs_column_from_index(const void* pairs, int64_t count, int on_device, int sorttype,
                         cs_stream stream, cs_column** out);
/* NVStrings::create_from_csv (NVStrings.h:146; util.cu:42-169): one column of a CSV text as a strings column.  The
 * text is `nbytes` bytes up to their first NUL byte, in host or device memory (on_device; device bytes are read where
 * they are and never written); the first line is the header and yields no row; a line ends at '\r' or '\n' and every
 * byte 1..31 behind it; `column` is 0-based, fields are cut at ',' outside double quotes; `lines` > 0 limits the rows;
 * flags: 1 sort by length, 2 sort by name, 8 an empty field is an empty string, not a null row (util.h:27-29).  Both
 * the line scan and the field walk run on the device.  A text with no line end in front of its first NUL gives an
 * empty column; a row of 2^31 - 1 bytes or more gives CS_ERR_RANGE. */
int cs_column_from_csv_buffer(const void* bytes, int64_t nbytes, int on_device, unsigned column, unsigned lines,
                              unsigned flags, cs_stream stream, cs_column** out);
/* The same from a file: read whole, one copy to the device.  A file that cannot be opened or holds fewer than 2 bytes
 * gives CS_OK and *out = NULL (the reference returns a null instance). */
int cs_column_from_csv(const char* path, unsigned column, unsigned lines, unsigned flags, cs_stream stream,
                       cs_column** out);
/* Bytes of the text one workgroup of the line scan takes (tests place their edge cases around multiples of it). */
int cs_csv_tile_bytes(void);
/* NVStrings::create_index (NVStrings.h:180; NVStrings.cu:348-400): one (pointer,
 * byte length) pair per row, the pointers addressing the column's own device
 * chars (valid until the handle is destroyed); null row = (NULL, 0). */
int cs_column_create_index(const cs_column* col, void* pairs, int on_device, cs_stream stream);
/* NVStrings::len (NVStrings.h:343; attrs.cu:32-69): characters per row, -1 for
 * null rows; *total = sum over non-null rows (the row count when `lengths` is
 * NULL, as in the reference). */
int cs_len(const cs_column* col, int32_t* lengths, int on_device, cs_stream stream,
           int64_t* total);
/* NVStrings::gather(pos, count) (NVStrings.h:278; array.cu:73-118): rows in the
 * given order, repeats allowed; a position outside [0, rows) -> CS_ERR_RANGE
 * (std::out_of_range in the reference). */
int cs_gather(const cs_column* col, const int32_t* pos, int64_t n, int on_device,
              cs_stream stream, cs_column** out);
/* NVStrings::gather(mask) (NVStrings.h:288; array.cu:121-146): rows whose mask
 * byte is non-zero. */
int cs_gather_mask(const cs_column* col, const uint8_t* mask, int on_device,
                   cs_stream stream, cs_column** out);
/* NVStrings::sublist(start, end, step) (NVStrings.h:261; array.cu:238-260). */
int cs_sublist(const cs_column* col, int64_t start, int64_t end, int64_t step,
               cs_stream stream, cs_column** out);
/* NVStrings::scatter(strs, pos) / scatter(str, pos, count) (NVStrings.h:302,318;
 * array.cu:157-236): a copy of `col` with row pos[j] replaced by row j of
 * `strs` (or by the scalar; NULL = null row).  Positions outside the column are
 * ignored; when a row is named more than once the last entry wins. */
int cs_scatter(const cs_column* col, const cs_column* strs, const int32_t* pos, int on_device,
               cs_stream stream, cs_column** out);
int cs_scatter_scalar(const cs_column* col, const char* str, const int32_t* pos, int64_t n,
                      int on_device, cs_stream stream, cs_column** out);
/* NVStrings::sort / order (NVStrings.h:1102,1114; array.cu:303-360): sorttype
 * bits 1 = byte length, 2 = name (unsigned bytewise, custring.inl:240-261);
 * nulls first or last regardless of direction.  Equal rows keep their index
 * order (the reference's comparator sort leaves their order unspecified). */
int cs_sort(const cs_column* col, int sorttype, int ascending, int nullfirst, cs_stream stream,
            cs_column** out);
int cs_order(const cs_column* col, int sorttype, int ascending, int nullfirst, uint32_t* indexes,
             int on_device, cs_stream stream);
/* NVStrings::cat(others, separator, narep) (NVStrings.h:384,397; combine.cu:31-291):
 * row-wise concatenation of `col` and up to 15 other columns of the same row
 * count; a null element is replaced by narep, or makes the row null when narep
 * is NULL. */
int cs_cat(const cs_column* col, const cs_column* const* others, int nothers,
           const char* separator, const char* narep, cs_stream stream, cs_column** out);
/* NVStrings::join(delimiter, narep) (NVStrings.h:561; combine.cu:293-420): all
 * rows joined into a column of ONE row; a null row contributes narep, or nothing
 * (and no delimiter) when narep is NULL.  delimiter NULL -> CS_ERR_INVALID_ARG. */
int cs_join(const cs_column* col, const char* delimiter, const char* narep, cs_stream stream,
            cs_column** out);

/* ---- per-row string ops ------------------------------------------------ */
/* NVStrings::lower / upper (NVStrings.h:815,822; case.cu:31-97,100-170). */
int cs_lower(const cs_column* col, cs_stream stream, cs_column** out);
int cs_upper(const cs_column* col, cs_stream stream, cs_column** out);
/* NVStrings::lstrip / strip / rstrip (NVStrings.h:796-808; strip.cu:30-199).
 * to_strip NULL = " \n\t".  side: 0 both, 1 left, 2 right. */
int cs_strip(const cs_column* col, const char* to_strip, int side, cs_stream stream,
             cs_column** out);
/* NVStrings::find (NVStrings.h:861; find.cu:75-120): char position of the
 * first occurrence in [start,end), -1 not found, -2 null row.
 * *found = number of rows with result != -1 (null rows included, as in the
 * reference). */
int cs_find(const cs_column* col, const char* str, int start, int end, int32_t* results,
            int on_device, cs_stream stream, int64_t* found);
/* NVStrings::contains (NVStrings.h:907; find.cu:237-272): 1 byte per row. */
/* The rest of NVStrings' find family (NVStrings.h:837-934; find.cu:36-72, 123-236, 276-387).  Positions are character
 * positions; null rows give -2 (positions), -1 (compare), false (predicates); the count out is what the reference returns. */
/* NVStrings::rfind: the last occurrence inside characters [start, end) (end < 0: to the end). */
int cs_rfind(const cs_column* col, const char* str, int start, int end, int32_t* results, int on_device, cs_stream stream, int64_t* found);
/* NVStrings::find_from: per-row windows; `starts` / `ends` hold one int32 per row (host memory unless bounds_on_device), either may be null. */
int cs_find_from(const cs_column* col, const char* str, const int32_t* starts, const int32_t* ends, int bounds_on_device, int32_t* results,
                 int on_device, cs_stream stream, int64_t* found);
/* NVStrings::find_multiple: results[row * targets + j] = position of targets[j] in the row. */
int cs_find_multiple(const cs_column* col, const cs_column* targets, int32_t* results, int on_device, cs_stream stream, int64_t* found);
/* NVStrings::compare: bytewise difference (custring.inl:240-261); *matches = rows equal to `str`.  An empty `str` is
 * compared like any other (1 for a non-empty row, 0 for an empty one) -- the reference returns without writing its
 * results (find.cu) and its callers hand back an uninitialised buffer. */
int cs_compare(const cs_column* col, const char* str, int32_t* results, int on_device, cs_stream stream, int64_t* matches);
/* NVStrings::match_strings: row-wise equality of two columns of the same size (two nulls are equal). */
int cs_match_strings(const cs_column* col, const cs_column* other, uint8_t* results, int on_device, cs_stream stream, int64_t* matches);
/* NVStrings::startswith / endswith. */
int cs_startswith(const cs_column* col, const char* str, uint8_t* results, int on_device, cs_stream stream, int64_t* matches);
int cs_endswith(const cs_column* col, const char* str, uint8_t* results, int on_device, cs_stream stream, int64_t* matches);
int cs_contains(const cs_column* col, const char* str, uint8_t* results, int on_device,
                cs_stream stream, int64_t* found);
/* NVStrings::replace (NVStrings.h:714; modify.cu:109-192). str NULL/empty ->
 * CS_ERR_INVALID_ARG. */
int cs_replace(const cs_column* col, const char* str, const char* repl, int maxrepl,
               cs_stream stream, cs_column** out);
/* NVStrings::split(delimiter,maxsplit,results) and split(maxsplit,results)
 * (NVStrings.h:504,524; split.cu:734-956). delimiter NULL = whitespace.
 * Column-major result: *out_cols is a malloc'd array of *ncols handles
 * (release each handle, then cs_free the array). */
int cs_split(const cs_column* col, const char* delimiter, int maxsplit, cs_stream stream,
             cs_column*** out_cols, int* ncols);
/* NVStrings::rsplit(delimiter,maxsplit,results) and rsplit(maxsplit,results)
 * (NVStrings.h:514,534; split.cu:960-1148): as cs_split with the tokens
 * located from the right (the per-row token count is split's).  Same
 * ownership of *out_cols. */
int cs_rsplit(const cs_column* col, const char* delimiter, int maxsplit, cs_stream stream,
              cs_column*** out_cols, int* ncols);
void cs_free(void* p);

/* ---- regex -------------------------------------------------------------- */
/* Reprog::create_from + dreprog::create_from (regcomp.cpp:954-960,
 * regexec.cpp:12-73). Host-only compile; usable without a GPU.  The library keeps
 * the last 32 compiled patterns: a handle is a counted reference to an immutable
 * object that several handles (and host threads) may share; every handle is
 * released with cs_regex_destroy.  CS_REGEX_NO_CACHE=1 compiles afresh per call. */
int cs_regex_compile(const char* pattern, cs_regex** out);
int cs_regex_destroy(cs_regex* re);
int cs_regex_inst_count(const cs_regex* re);
/* Which executor runs the pattern (no reference counterpart: the reference has one executor, regexec.inl:204-442).
 * Bit 0: the tagged DFA (otherwise the ordered-list simulator); bit 1: the unit decomposition is offered; bit 2: capture
 * groups are tracked on the DFA; bits 8..11: live threads the automaton keeps at most; bits 16..31: DFA states. */
int cs_regex_engine(const cs_regex* re);
/* Flat int32 program image (layout: custrings_amd/csrc/regex_program.h). */
int cs_regex_blob(const cs_regex* re, const int32_t** words, int* nwords);
/* NVStrings::contains_re / match / count_re (NVStrings.h:963,975,988;
 * count.cu:59-250). */
int cs_contains_re(const cs_column* col, const cs_regex* re, uint8_t* results, int on_device,
                   cs_stream stream, int64_t* found);
int cs_match_re(const cs_column* col, const cs_regex* re, uint8_t* results, int on_device,
                cs_stream stream, int64_t* found);
int cs_count_re(const cs_column* col, const cs_regex* re, int32_t* results, int on_device,
                cs_stream stream, int64_t* found);
/* NVStrings::replace_re (NVStrings.h:766; replace.cu:110-189). */
int cs_replace_re(const cs_column* col, const cs_regex* re, const char* repl, int maxrepl,
                  cs_stream stream, cs_column** out);
/* NVStrings::replace_re(patterns, repls) (NVStrings.h:777; replace_multi.cu:110-189):
 * at every character position the patterns are tried in order, anchored there;
 * the first that matches is replaced by repls[its index] (or by repls[0] when
 * `repls` holds one row; a null replacement removes the match) and the walk
 * continues behind the match.  A pattern that can match the empty string is
 * refused with CS_ERR_INVALID_ARG (the reference does not terminate on it). */
int cs_replace_re_multi(const cs_column* col, const cs_regex* const* patterns, int npatterns,
                        const cs_column* repls, cs_stream stream, cs_column** out);
/* NVStrings::replace_with_backrefs(pattern, repl) (NVStrings.h:788;
 * replace_backref.cu:36-207): every match is replaced by `repl` with \N
 * (backslash + digits) standing for capture group N of that match (0 = the
 * whole match; a group that took no part contributes nothing).  repl NULL ->
 * all rows null.  At most 16 references.  A pattern that can match the empty
 * string is refused with CS_ERR_INVALID_ARG (the reference does not terminate
 * on it). */
int cs_replace_with_backrefs(const cs_column* col, const cs_regex* re, const char* repl,
                             cs_stream stream, cs_column** out);
/* NVStrings::extract(pattern, results) (NVStrings.h:682; extract.cu:69-151):
 * column-major, one column per capture group; a row is null unless the
 * pattern matches and the group's span is non-empty.  *out_cols is a malloc'd
 * array of *ncols handles (release each, then cs_free the array); a pattern
 * without capture groups or a column of zero rows yields *ncols = 0. */
int cs_extract(const cs_column* col, const cs_regex* re, cs_stream stream,
               cs_column*** out_cols, int* ncols);
/* NVStrings::findall(pattern, results) (NVStrings.h:943; findall.cu:99-179):
 * column-major, column k holds every row's k-th match in count_re order; rows
 * with fewer matches (and null rows) are null, an empty match is an empty
 * string.  No match in any row yields one all-null column; a column of zero
 * rows yields *ncols = 0.  Same ownership as cs_extract. */
int cs_findall(const cs_column* col, const cs_regex* re, cs_stream stream,
               cs_column*** out_cols, int* ncols);

/* Record (row-major) forms -- NVStrings::split_record / rsplit_record /
 * extract_record / findall_record (NVStrings.h:443-494,693,952;
 * extract_record.cu:146-152, findall_record.cu:144-151) return one instance
 * per row.  Natively a record result is ONE column holding the records'
 * strings in row-major order plus rows+1 list offsets (record r = flat rows
 * [list_offsets[r], list_offsets[r+1])).  This call transposes a column-major
 * result (`ncols` columns of equal row count): ragged = 0 keeps
 * every column per record, nulls included (extract_record); ragged = 1 keeps
 * each row's leading non-null columns (findall_record, split_record: a null
 * row or a row without matches has an empty record).  list_offsets: rows+1
 * int64, device memory when on_device. */
int cs_records_from_columns(const cs_column* const* cols, int ncols, int ragged,
                            int64_t* list_offsets, int on_device, cs_stream stream,
                            cs_column** out);

/* NVStrings::split_record / rsplit_record (NVStrings.h:443-494; split.cu:125-700)
 * natively: ONE flat column of every row's tokens in row-major order plus rows+1
 * list offsets (record r = flat rows [list_offsets[r], list_offsets[r+1]); a
 * null row has no entries, where the reference pushes a null instance).
 * delimiter NULL (or "") = whitespace: a valid row without tokens then yields one
 * empty string (split.cu:393-397).  list_offsets: int64, device memory when
 * on_device. */
int cs_split_record(const cs_column* col, const char* delimiter, int maxsplit,
                    int64_t* list_offsets, int on_device, cs_stream stream, cs_column** out);
int cs_rsplit_record(const cs_column* col, const char* delimiter, int maxsplit,
                     int64_t* list_offsets, int on_device, cs_stream stream, cs_column** out);
/* split_re / rsplit_re: split every row at the matches of a compiled pattern (no
 * member of the reference; pandas / Spark semantics).  A row's matches are those
 * cs_count_re counts and cs_findall returns.  With m matches a row has s = m cuts
 * (maxsplit <= 0) or min(m, maxsplit): cs_split_re cuts at the first s matches,
 * cs_rsplit_re at the last s; the row has s + 1 tokens, empty strings where two
 * cuts are adjacent or a cut touches an end of the row.  Column-major result as
 * cs_split (same ownership): column k holds token k, null from a row's token count
 * on and for null rows; zero rows and only null rows answer as cs_split.  The
 * record forms return the flat column and list offsets of cs_split_record (a null
 * row has no entries).  The empty pattern and a pattern that can match the empty
 * string are CS_ERR_INVALID_ARG. */
int cs_split_re(const cs_column* col, const cs_regex* re, int maxsplit, cs_stream stream,
                cs_column*** out_cols, int* ncols);
int cs_rsplit_re(const cs_column* col, const cs_regex* re, int maxsplit, cs_stream stream,
                 cs_column*** out_cols, int* ncols);
int cs_split_record_re(const cs_column* col, const cs_regex* re, int maxsplit,
                       int64_t* list_offsets, int on_device, cs_stream stream, cs_column** out);
int cs_rsplit_record_re(const cs_column* col, const cs_regex* re, int maxsplit,
                        int64_t* list_offsets, int on_device, cs_stream stream, cs_column** out);
/* NVStrings::partition / rpartition (NVStrings.h:537,549; split.cu:1165-1361):
 * three strings per row -- head, delimiter, tail around the first (last)
 * occurrence; no occurrence: (row, "", "") / ("", "", row); a null row: three
 * nulls.  Flat column of 3 * rows entries (row r = entries 3r .. 3r+2).  A NULL
 * or empty delimiter yields *out = NULL (the reference returns no results). */
int cs_partition(const cs_column* col, const char* delimiter, int from_right, cs_stream stream,
                 cs_column** out);

/* ---- category (dictionary encoding) ------------------------------------ */
/* NVCategory::create_from_strings (NVCategory.h:107; NVCategory.cu:220-304):
 * keys = sorted unique rows (null first, then unsigned bytewise order,
 * custring.inl:240-261), codes[r] = index of row r's key. */
int cs_category_build(const cs_column* col, cs_stream stream, cs_category** out);
/* NVCategory::create_from_categories (NVCategory.h:121; NVCategory.cu:430-514):
 * merged sorted-unique key set, concatenated remapped codes. */
int cs_category_merge(const cs_category* const* cats, int ncats, cs_stream stream,
                      cs_category** out);
/* The merge step of a distributed category build (one process per GPU): after the ranks all-gathered their key sets --
 * the transport is the caller's: RCCL, MPI, torch.distributed -- every rank merges them and maps its local codes into the
 * merged key set.  keysets[r] = rank r's key set (this rank's own at index `rank`); *merged_keys is the same column on every
 * rank; values = device memory for cs_category_size(local) int32 codes.  Composes NVCategory::create_from_categories
 * (NVCategory.cu:430-514); the reference itself is single-GPU. */
int cs_category_merge_gathered(const cs_category* local, const cs_column* const* keysets, int nranks, int rank, cs_stream stream,
                               cs_column** merged_keys, int32_t* values);
/* The whole distributed build behind the C ABI (BASELINE.json north_star; what custrings_amd/dist.py does through
 * torch.distributed): local build (NVCategory.cu:220-304), all-gather of the ranks' sorted key sets, merge
 * (NVCategory::create_from_categories, NVCategory.cu:430-514), remap.  One process per GPU.  `nccl_comm`: the caller's
 * ncclComm_t of `nranks` ranks (RCCL is resolved in the process at run time: dlsym, else dlopen of librccl.so);
 * *out: keys = the same column on every rank, values = this rank's rows' codes.  nranks == 1 is the local build. */
int cs_category_build_distributed(const cs_column* col, void* nccl_comm, int nranks, int rank, cs_stream stream, cs_category** out);
/* The same over a caller-supplied all-gather (another transport, a test harness): `allgather(ctx, send, recv, bytes,
 * stream)` puts every rank's `bytes` bytes at `send` (device memory) behind each other, in rank order, at `recv`
 * (device memory, nranks * bytes), ordered after the work queued on `stream`; returns 0 on success. */
typedef int (*cs_allgather_fn)(void* ctx, const void* send, void* recv, size_t bytes, void* stream);
int cs_category_build_distributed_with(const cs_column* col, cs_allgather_fn allgather, void* ctx, int nranks, int rank, cs_stream stream,
                                       cs_category** out);
/* ... and a caller-supplied all-to-all of variable pieces, which opens the second route: from 2^21 keys in all (K close to
 * N) the merge is partitioned by key RANGE -- splitters from a sample of every rank's keys, every key to its range's
 * owner, the merged ranges all-gathered: every rank merges 1/nranks of the keys instead of all of them.
 * `alltoallv(ctx, send, send_bytes, send_off, recv, recv_bytes, recv_off, nranks, stream)`: this rank's piece for rank d
 * is send_bytes[d] bytes at send + send_off[d] (device memory); what rank d sent to this rank arrives at recv + recv_off[d]
 * (recv_bytes[d] bytes: the library exchanged the sizes beforehand); ordered after the work queued on `stream`; 0 on
 * success.  cs_category_build_distributed passes grouped ncclSend / ncclRecv.  NULL: the all-gather route only.
 * A rank whose local build fails still takes part in the first exchange and every rank returns an error together. */
typedef int (*cs_alltoallv_fn)(void* ctx, const void* send, const size_t* send_bytes, const size_t* send_off, void* recv, const size_t* recv_bytes,
                               const size_t* recv_off, int nranks, void* stream);
int cs_category_build_distributed_with2(const cs_column* col, cs_allgather_fn allgather, cs_alltoallv_fn alltoallv, void* ctx, int nranks, int rank,
                                        cs_stream stream, cs_category** out);
int cs_category_destroy(cs_category* cat);
/* NVCategory::create_ipc_transfer / create_from_ipc (NVCategory.h:128,176; ipc_transfer.h:109-200): the key column
 * as above plus the handle of the int32 values. */
typedef struct cs_ipc_category {
  cs_ipc_column keys;
  unsigned char values[64]; /* hipIpcMemHandle_t */
  int64_t rows;
} cs_ipc_category;
int cs_category_ipc_export(const cs_category* cat, cs_ipc_category* out);
int cs_category_ipc_import(const cs_ipc_category* ipc, cs_category** out);
int64_t cs_category_size(const cs_category* cat);      /* NVCategory::size      */
int64_t cs_category_keys_size(const cs_category* cat); /* NVCategory::keys_size */
/* NVCategory::get_keys (new handle on the shared key column). */
int cs_category_keys(const cs_category* cat, cs_column** out);
/* NVCategory::values_cptr: borrowed device pointer to the int32 codes. */
const int32_t* cs_category_values_ptr(const cs_category* cat);
/* NVCategory::get_values (NVCategory.h:225). */
int cs_category_get_values(const cs_category* cat, int32_t* out, int on_device,
                           cs_stream stream);
/* NVCategory::get_indexes_for: the rows whose value is `key`, ascending, into `results` (host or device memory with room
 * for that many int32; NULL: the count alone); *count = how many. */
int cs_category_indexes_for(const cs_category* cat, int32_t key, int32_t* results, int on_device, cs_stream stream,
                            int64_t* count);
/* The remap family (NVCategory.h:247-420; NVCategory.cu:926-1822).  Keys stay
 * sorted unique (merge_category alone appends the new keys behind the old ones);
 * values of keys that disappear become -1. */
int cs_category_to_strings(const cs_category* cat, cs_stream stream, cs_column** out);
int cs_category_gather_strings(const cs_category* cat, const int32_t* pos, int64_t n, int on_device,
                               cs_stream stream, cs_column** out); /* CS_ERR_RANGE: std::out_of_range */
int cs_category_gather(const cs_category* cat, const int32_t* pos, int64_t n, int on_device,
                       cs_stream stream, cs_category** out);
int cs_category_gather_and_remap(const cs_category* cat, const int32_t* pos, int64_t n, int on_device,
                                 cs_stream stream, cs_category** out);
int cs_category_add_strings(const cs_category* cat, const cs_column* strs, cs_stream stream,
                            cs_category** out);
int cs_category_remove_strings(const cs_category* cat, const cs_column* strs, cs_stream stream,
                               cs_category** out);
int cs_category_merge_category(const cs_category* cat, const cs_category* cat2, cs_stream stream,
                               cs_category** out);
int cs_category_add_keys(const cs_category* cat, const cs_column* strs, cs_stream stream,
                         cs_category** out); /* add_keys_and_remap */
int cs_category_remove_keys(const cs_category* cat, const cs_column* strs, cs_stream stream,
                            cs_category** out); /* remove_keys_and_remap */
int cs_category_remove_unused_keys(const cs_category* cat, cs_stream stream, cs_category** out);
int cs_category_set_keys(const cs_category* cat, const cs_column* strs, cs_stream stream,
                         cs_category** out); /* set_keys_and_remap */
/* Multi-GPU key-set merge helper: out[i] = table[codes[i]] (codes < 0 kept). */
int cs_remap_codes(const int32_t* codes, int64_t n, const int32_t* table, int32_t* out,
                   cs_stream stream);

/* ---- text --------------------------------------------------------------- */
/* NVText::tokenize(strs, delimiter) (NVText.h:40; tokens.cu:123-155):
 * delimiter NULL = whitespace (char <= ' '), else any char of `delimiter`. */
int cs_tokenize(const cs_column* col, const char* delimiter, cs_stream stream,
                cs_column** out);
/* NVText::tokenize(strs, delimiters) (NVText.h:48; tokens.cu:158-260): every row of
 * `delimiters` is a whole-string delimiter (tried in order at each byte; null and
 * empty rows skipped); empty tokens are dropped.  No delimiters = whitespace. */
int cs_tokenize_multi(const cs_column* col, const cs_column* delimiters, cs_stream stream,
                      cs_column** out);
/* NVText::create_ngrams (NVText.h:153; ngram.cu:32-110). */
int cs_ngrams(const cs_column* tokens, unsigned ngrams, const char* separator,
              cs_stream stream, cs_column** out);

/* NVText counters (NVText.h:51-141; tokens.cu:262-716).  delimiter NULL (or "")
 * = whitespace, else any character of the string. */
int cs_token_count(const cs_column* col, const char* delimiter, uint32_t* results, int on_device,
                   cs_stream stream); /* tokens per row, 0 for a null row */
int cs_unique_tokens(const cs_column* col, const char* delimiter, cs_stream stream,
                     cs_column** out); /* sorted distinct tokens */
/* results[r * tokens_rows + t] = how many of row r's tokens equal tokens[t]. */
int cs_tokens_counts(const cs_column* col, const cs_column* tokens, const char* delimiter,
                     uint32_t* results, int on_device, cs_stream stream);
/* Every token equal to targets[t] becomes repls[t] (repls[0] when `repls` has one
 * row; a null replacement removes the token).  *out = NULL when the result holds
 * no bytes at all (tokens.cu:612-613). */
int cs_replace_tokens(const cs_column* col, const cs_column* targets, const cs_column* repls,
                      const char* delimiter, cs_stream stream, cs_column** out);
/* Tokens of each row joined by one space; *out = NULL when no row holds a token
 * (tokens.cu:703-704). */
int cs_normalize_spaces(const cs_column* col, cs_stream stream, cs_column** out);

/* ---- synthetic workloads (bench / parity inputs) -- */
/* kind: 2 = C2 word rows, 3 = C3 log lines, 4 = C4 16-char tokens,
 * 5 = C5 tweet-like text.  Row r is a pure function of (seed, first_row + r). */
int cs_synth_column(int kind, int64_t first_row, int64_t rows, uint64_t seed,
                    int64_t param, cs_stream stream, cs_column** out);
/* Order-sensitive 64-bit digest of a column (offsets, chars, validity);
 * used for full-size parity ("checksum of checksums"). */
int cs_column_digest(const cs_column* col, cs_stream stream, uint64_t* digest);

/* ---- measurement -------------------------------------------------------- */
/* Device time (ms, HIP events on `stream`) and launch count of the dominant
 * kernel accumulated since the last reset; see bench.py "roofline". */
int cs_prof_reset(void);
int cs_prof_enable(int on);
int cs_prof_get(const char* kernel, double* total_ms, int64_t* launches);
/* Test aid: `blocks` workgroups of 256 threads and `lds_bytes` of LDS each that do nothing for `milliseconds`, queued on
 * `stream` -- a co-tenant that keeps part of the GPU occupied while another stream's call runs (the persistent kernels
 * size their grids for an empty device). */
int cs_debug_spin(int blocks, int lds_bytes, int milliseconds, cs_stream stream);

/* ---- numeric and boolean conversions (reference: cpp/src/strings/convert.cu; per-row logic in
 * custrings_amd/csrc/convert_ops.h) ---------------------------------------------------------------------
 * Parse ops: one value per row into `results` (rows entries; device memory when on_device).  A null row
 * gives 0.  `count` receives the number of non-zero results, or -1 for an empty column or a NULL
 * `results` (then nothing is written) -- the reference's return value. */
int cs_hash(const cs_column* col, uint32_t* results, int on_device, cs_stream stream, int64_t* count); /* NVStrings::hash, NVStrings.h:1031: MurmurHash3_x86_32, seed 31 */
int cs_stoi(const cs_column* col, int32_t* results, int on_device, cs_stream stream, int64_t* count);  /* NVStrings::stoi, NVStrings.h:991 */
int cs_stol(const cs_column* col, int64_t* results, int on_device, cs_stream stream, int64_t* count);  /* NVStrings::stol, NVStrings.h:999 */
int cs_stof(const cs_column* col, float* results, int on_device, cs_stream stream, int64_t* count);    /* NVStrings::stof, NVStrings.h:1015 */
int cs_stod(const cs_column* col, double* results, int on_device, cs_stream stream, int64_t* count);   /* NVStrings::stod, NVStrings.h:1023 */
int cs_htoi(const cs_column* col, uint32_t* results, int on_device, cs_stream stream, int64_t* count); /* NVStrings::htoi, NVStrings.h:1007 */
int cs_ip2int(const cs_column* col, uint32_t* results, int on_device, cs_stream stream, int64_t* count); /* NVStrings::ip2int, NVStrings.h:1113 */
/* NVStrings::to_bools, NVStrings.h:1092: 1 where the row equals `true_string`; a null row gives
 * (true_string == NULL).  `count` = rows minus the false results (nulls count as false). */
int cs_to_bools(const cs_column* col, const char* true_string, uint8_t* results, int on_device, cs_stream stream,
                int64_t* count);
/* Format ops: a new column of `count` rows from `count` values; `nulls` (optional, (count + 7) / 8 bytes,
 * LSB-first, bit = 1 valid) makes the cleared rows null.  `values` and `nulls` live on the device when
 * on_device.  values == NULL or count == 0: CS_ERR_INVALID_ARG (std::invalid_argument in the reference). */
int cs_itos(const int32_t* values, int64_t count, const uint8_t* nulls, int on_device, cs_stream stream, cs_column** out);  /* NVStrings::itos, NVStrings.h:1042 */
int cs_ltos(const int64_t* values, int64_t count, const uint8_t* nulls, int on_device, cs_stream stream, cs_column** out);  /* NVStrings::ltos, NVStrings.h:1053 */
int cs_ftos(const float* values, int64_t count, const uint8_t* nulls, int on_device, cs_stream stream, cs_column** out);    /* NVStrings::ftos, NVStrings.h:1067 */
int cs_dtos(const double* values, int64_t count, const uint8_t* nulls, int on_device, cs_stream stream, cs_column** out);   /* NVStrings::dtos, NVStrings.h:1081 */
int cs_int2ip(const uint32_t* values, int64_t count, const uint8_t* nulls, int on_device, cs_stream stream, cs_column** out); /* NVStrings::int2ip, NVStrings.h:1124 */
/* NVStrings::create_from_bools, NVStrings.h:1105: `true_string` / `false_string` (both required) per value
 * (one byte each, non-zero = true). */
int cs_from_bools(const uint8_t* values, int64_t count, const char* true_string, const char* false_string,
                  const uint8_t* nulls, int on_device, cs_stream stream, cs_column** out);

/* ---- timestamp conversions (reference: cpp/src/strings/datetime.cu; per-row logic in
 * custrings_amd/csrc/datetime_ops.h) ---------------------------------------------------------------------
 * `format` holds strptime / strftime specifiers (%Y %y %m %d %j %H %I %M %S %f %p %z %Z; %% is a literal
 * '%'); NULL means "%Y-%m-%dT%H:%M:%SZ".  A '%' at the end, an unknown specifier or units outside the enum
 * are CS_ERR_INVALID_ARG (std::invalid_argument in the reference). */
typedef enum cs_timestamp_units { /* NVStrings::timestamp_units, NVStrings.h:1128 */
  CS_TS_YEARS = 0,
  CS_TS_MONTHS = 1,
  CS_TS_DAYS = 2,
  CS_TS_HOURS = 3,
  CS_TS_MINUTES = 4,
  CS_TS_SECONDS = 5,
  CS_TS_MS = 6,
  CS_TS_US = 7,
  CS_TS_NS = 8
} cs_timestamp_units;
/* NVStrings::timestamp2long, NVStrings.h:1153: one int64 per row since the epoch, in `units` (a
 * cs_timestamp_units), into `results` (device memory when on_device).  A null, empty or unparsable row gives
 * 0.  `count` receives the number of non-zero results, or -1 for an empty column or a NULL `results` (checked
 * before the format is read; nothing is written). */
int cs_timestamp2long(const cs_column* col, const char* format, int units, int64_t* results, int on_device, cs_stream stream,
                      int64_t* count);
/* NVStrings::long2timestamp, NVStrings.h:1171: a column of `count` rows from int64 `values` in `units`; `nulls`
 * (optional, (count + 7) / 8 bytes, LSB-first, bit = 1 valid) makes the cleared rows null.  Every other row has
 * the same width.  values == NULL or count == 0: CS_ERR_INVALID_ARG (checked before the format is read). */
int cs_long2timestamp(const int64_t* values, int64_t count, int units, const char* format, const uint8_t* nulls, int on_device,
                      cs_stream stream, cs_column** out);

/* ---- substrings, padding, wrapping (reference: cpp/src/strings/substr.cu, pad.cu, modify.cu:35-106,494-552;
 * per-row logic in custrings_amd/csrc/pad_ops.h) -------------------------------------------------------------
 * Null rows stay null (the output shares the input's validity).  Character positions are unsigned as in the
 * reference: a negative start is past the end of every row.  An output row of 2^31 bytes or more is
 * CS_ERR_RANGE. */
/* NVStrings::slice / get (NVStrings.h:650-658; substr.cu:32-83): characters [start, stop) of every row,
 * stop <= 0 meaning the row's end; step > 1 takes characters start, start + step, ... below stop.
 * stop > 0 && start > stop: CS_ERR_INVALID_ARG (std::invalid_argument). */
int cs_slice(const cs_column* col, int start, int stop, int step, cs_stream stream, cs_column** out);
/* NVStrings::slice_from (NVStrings.h:671; substr.cu:85-130): slice with one int32 start / stop per row
 * (device memory when on_device, else host); a NULL array means 0 / -1 for every row. */
int cs_slice_from(const cs_column* col, const int32_t* starts, const int32_t* stops, int on_device, cs_stream stream,
                  cs_column** out);
/* NVStrings::slice_replace (NVStrings.h:704; modify.cu:35-106): characters [start, stop) replaced with
 * `repl`, stop < 0 meaning the row's end; a start at or past the character count (a negative one included)
 * appends.  repl NULL: CS_ERR_INVALID_ARG. */
int cs_slice_replace(const cs_column* col, const char* repl, int start, int stop, cs_stream stream, cs_column** out);
/* NVStrings::insert (NVStrings.h:754; modify.cu:494-552): `repl` inserted at character position `start`
 * (-1 = the end; a row with fewer characters than `start` is left as it is).  repl NULL: CS_ERR_INVALID_ARG. */
int cs_insert(const cs_column* col, const char* repl, int start, cs_stream stream, cs_column** out);
/* NVStrings::repeat (NVStrings.h:561; pad.cu:28-85): every row repeated max(count, 1) times. */
int cs_repeat(const cs_column* col, unsigned count, cs_stream stream, cs_column** out);
/* NVStrings::pad / rjust / ljust / center (NVStrings.h:566-620; pad.cu:87-287): rows shorter than `width`
 * characters filled to it with the first UTF-8 character of `fillchar` (NULL or empty = " ").
 * side: 0 fill on the left (rjust), 1 on the right (ljust), 2 both (center: the odd one on the right). */
int cs_pad(const cs_column* col, unsigned width, int side, const char* fillchar, cs_stream stream, cs_column** out);
/* NVStrings::zfill (NVStrings.h:630; pad.cu:290-353): '0' fill to `width` characters after a leading '+' / '-'
 * (every row, numeric or not). */
int cs_zfill(const cs_column* col, unsigned width, cs_stream stream, cs_column** out);
/* NVStrings::wrap (NVStrings.h:640; pad.cu:355-436): every character <= ' ' becomes ' ' and some become '\n',
 * so that lines hold about `width` characters.  The output has the input's extents. */
int cs_wrap(const cs_column* col, unsigned width, cs_stream stream, cs_column** out);

/* ---- character types and the other case ops (reference: cpp/src/strings/attrs.cu:115-438, case.cu:169-397; per-row
 * logic in custrings_amd/csrc/chartype_ops.h) -----------------------------------------------------------------
 * Predicates: one byte per row (1 / 0) into `results` (rows entries; device memory when on_device); `count`
 * receives the number of true rows.  A column of no rows or a NULL `results`: count 0, nothing written.
 * Flag bits of the Unicode table: decimal 1, numeric 2, digit 4, alpha 8, space 16, upper 32, lower 64; a
 * character above U+FFFF has none.
 *   isalnum (bits 15), isalpha (8), isdigit (4), isspace (16), isdecimal (1), isnumeric (2): the row is not
 *     empty and every character has one of the bits; a null row is false
 *   islower / isupper: the row is not empty and every character is not alphabetic, or lower / upper
 *   is_empty: the row is null or has no bytes */
typedef enum cs_chartype_pred {
  CS_IS_ALNUM = 0,
  CS_IS_ALPHA = 1,
  CS_IS_DIGIT = 2,
  CS_IS_SPACE = 3,
  CS_IS_DECIMAL = 4,
  CS_IS_NUMERIC = 5,
  CS_IS_LOWER = 6,
  CS_IS_UPPER = 7,
  CS_IS_EMPTY = 8
} cs_chartype_pred;
int cs_chartype(const cs_column* col, int pred, uint8_t* results, int on_device, cs_stream stream, int64_t* count);
int cs_isalnum(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count);   /* NVStrings::isalnum, attrs.cu:115 */
int cs_isalpha(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count);   /* NVStrings::isalpha, attrs.cu:152 */
int cs_isdigit(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count);   /* NVStrings::isdigit, attrs.cu:190 */
int cs_isspace(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count);   /* NVStrings::isspace, attrs.cu:227 */
int cs_isdecimal(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count); /* NVStrings::isdecimal, attrs.cu:264 */
int cs_isnumeric(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count); /* NVStrings::isnumeric, attrs.cu:301 */
int cs_islower(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count);   /* NVStrings::islower, attrs.cu:338 */
int cs_isupper(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count);   /* NVStrings::isupper, attrs.cu:375 */
int cs_is_empty(const cs_column* col, uint8_t* results, int on_device, cs_stream stream, int64_t* count);  /* NVStrings::is_empty, attrs.cu:412 */
/* NVStrings::swapcase (case.cu:169): every cased character becomes its opposite-case one.
 * NVStrings::capitalize (case.cu:238): the first character to upper, the others to lower case -- only
 * characters up to U+0FFF are mapped (the reference's bound); later cased ones pass through.
 * NVStrings::title (case.cu:314): a letter that follows a non-letter (or starts the row) to upper, a letter
 * that follows a letter to lower case.  Null rows stay null. */
int cs_swapcase(const cs_column* col, cs_stream stream, cs_column** out);
int cs_capitalize(const cs_column* col, cs_stream stream, cs_column** out);
int cs_title(const cs_column* col, cs_stream stream, cs_column** out);

/* ---- column statistics (NVStrings::compute_statistics, NVStrings.cu:604; per-row logic in
 * custrings_amd/csrc/stats_ops.h; kernels cs_stats.hip) ----------------------------------------------
 * One read of the chars gives every length, memory and class figure and the character histogram.
 * Per row: bytes and chars (what cs_len reports) are 0 for a null row; mem is 0 for a null row, else
 * 8 + bytes + 1 + (chars != bytes ? (chars + 3) / 4 : 0) -- the reference's per-row object, 9 for an empty row.
 * The *_avg are sums / rows (chars_avg divides the BYTES, as the reference does), the *_max maxima over all rows, the
 * *_min minima over the rows whose value is not 0 (0 when there is none), the *_95 always 0.  total_memory is the
 * column's own footprint (NVStrings::memsize).  unique_strings counts the distinct rows, all nulls as one value.
 * The class counts are the characters <= U+FFFF of non-null rows whose flag-table byte has the space / digit / upper /
 * lower bit.  A column of no rows gives all zeros and no pair. */
typedef struct cs_statistics {
  uint64_t total_bytes, total_chars;
  uint64_t bytes_avg, bytes_max, bytes_min, bytes_95;
  uint64_t chars_avg, chars_max, chars_min, chars_95;
  uint64_t total_memory;
  uint64_t mem_avg, mem_max, mem_min, mem_95;
  uint64_t total_strings, total_nulls, total_empty, unique_strings;
  uint64_t whitespace_count, digits_count, uppercase_count, lowercase_count;
} cs_statistics;
/* what to compute: a bit set.  Fields outside it stay 0 (total_strings and total_memory are always set).  LENGTHS: the
 * totals, averages, minima and maxima, total_nulls and total_empty; UNIQUE builds a category and drops it. */
enum { CS_STATS_LENGTHS = 1, CS_STATS_CLASSES = 2, CS_STATS_HISTOGRAM = 4, CS_STATS_UNIQUE = 8, CS_STATS_ALL = 15 };
/* With CS_STATS_HISTOGRAM: `pairs` (device memory when on_device) receives one (character, count) pair of uint32 per code
 * point 1 .. 0xFFFF that occurs in a non-null row, in code-point order -- the character as packed UTF-8 bytes (U+00E9 ->
 * 0xC3A9), the count modulo 2^32 -- and *npairs their number.  CS_ERR_INVALID_ARG for a null `col` / `out` / `npairs`
 * and when there are more pairs than `pairs_cap`: *npairs then holds the number needed and `pairs` is untouched. */
int cs_column_statistics(const cs_column* col, int what, cs_statistics* out, uint32_t* pairs, int64_t pairs_cap, int64_t* npairs, int on_device,
                         cs_stream stream);
/* Code points below this are counted in LDS, the others straight in device memory (tests put a character on each side). */
int cs_stats_lds_bins(void);

/* ---- the rest of NVText: string matches, edit distance, stemmer measure, scatter (per-row logic in
 * custrings_amd/csrc/text_ops.h; kernels cs_textops.hip) ---------------------------------------------
 * Matrix results are row-major: results[r * targets_rows + j] (device memory when on_device).  A column of no rows, no
 * targets or a NULL `results` writes nothing. */
/* NVText::contains_strings (NVText.cu:32): 1 when target j occurs in row r -- bytes compared at every byte offset.  A null
 * row, a null target and an empty target give 0. */
int cs_contains_strings(const cs_column* col, const cs_column* targets, uint8_t* results, int on_device, cs_stream stream);
/* NVText::strings_counts (NVText.cu:77): occurrences of target j in row r, each search starting chars(target) characters
 * behind the character position of the last match. */
int cs_strings_counts(const cs_column* col, const cs_column* targets, uint32_t* results, int on_device, cs_stream stream);
typedef enum cs_distance_type { CS_LEVENSHTEIN = 0 } cs_distance_type; /* NVText::distance_type, NVText.h:121 */
/* NVText::edit_distance (edit_distance.cu:119): the Levenshtein distance, in characters, of every row to `target`.  A null
 * or empty row gives chars(target).  algo != CS_LEVENSHTEIN, target NULL or results NULL: CS_ERR_INVALID_ARG.  A row or a
 * target of more than 32767 characters: CS_ERR_RANGE (the reference's 16-bit table wraps there). */
int cs_edit_distance(const cs_column* col, const char* target, int algo, uint32_t* results, int on_device, cs_stream stream);
/* NVText::edit_distance (edit_distance.cu:172): row r of `col` against row r of `targets`; a null or empty side gives the
 * other side's characters (0 when both are).  Columns of different sizes: CS_ERR_INVALID_ARG. */
int cs_edit_distance_column(const cs_column* col, const cs_column* targets, int algo, uint32_t* results, int on_device, cs_stream stream);
/* NVText::porter_stemmer_measure (stemmer.cu:69): vowel-run -> consonant transitions per row; vowels NULL = "aeiou",
 * y_char NULL = "y" (its first character).  A null row gives 0 (the reference leaves its entry unwritten). */
int cs_porter_stemmer_measure(const cs_column* col, const char* vowels, const char* y_char, uint32_t* results, int on_device, cs_stream stream);
/* NVText::scatter_count (NVText.cu:126): row i repeated counts[i] times, in order (counts: rows entries, device memory when
 * on_device); null rows stay null.  *out = NULL for a column of no rows or NULL counts; a total of 0 gives an empty column;
 * a total of 2^31 or more: CS_ERR_RANGE. */
int cs_scatter_count(const cs_column* col, const uint32_t* counts, int on_device, cs_stream stream, cs_column** out);

/* ---- minhash: MinHash signatures of a column and LSH band keys (no reference member; the definition and the per-row logic
 * are custrings_amd/csrc/minhash_ops.h; kernels cs_minhash.hip) ----------------------------------------------------
 * results[r * nperm + i] = the minimum, over the n-grams of `width` characters of row r, of
 * ((MurmurHash3_x86_32(n-gram bytes, seed) * a[i] + b[i]) mod (2^61 - 1)) & 0xFFFFFFFF.  A character starts at every byte
 * that is no continuation byte; a row of fewer than `width` characters (and one at least) is one n-gram; a row of none
 * -- null, empty, continuation bytes only -- gives 0xFFFFFFFF everywhere.  `a` and `b` are host arrays of nperm values;
 * `results` is device memory when on_device.  A null `col` / `a` / `b`, width < 1 or nperm < 1: CS_ERR_INVALID_ARG;
 * width > 255, nperm > 4096 or some a[i] == 0: CS_ERR_RANGE.  A column of no rows or a NULL `results` writes nothing. */
int cs_minhash(const cs_column* col, int width, uint32_t seed, const uint32_t* a, const uint32_t* b, int nperm, uint32_t* results, int on_device,
               cs_stream stream);
/* keys[r * bands + j] = (int64)j << 32 | MurmurHash3_x86_32(the nperm / bands values of band j of signature r as
 * little-endian bytes, seed j): equal keys mean two rows agree on a whole band, keys of different bands never collide.
 * `signatures` (rows x nperm) and `keys` are both device memory when on_device, both host memory otherwise.  nperm < 1,
 * bands < 1, nperm % bands != 0, rows < 0 or a NULL `signatures` with rows > 0: CS_ERR_INVALID_ARG; nperm > 4096:
 * CS_ERR_RANGE.  rows == 0 or a NULL `keys` writes nothing. */
int cs_minhash_bands(const uint32_t* signatures, int64_t rows, int nperm, int bands, int64_t* keys, int on_device, cs_stream stream);

/* ---- WordPiece: a column of text to the int32 ids of a vocabulary (no reference member; the definition and the per-word
 * logic are custrings_amd/csrc/wordpiece_ops.h; kernels cs_wordpiece.hip) ------------------------------------------------
 * The vocabulary is a strings column whose row index is the id: null and empty rows are no entry, among equal rows the
 * lowest index wins.  A row's words are its maximal runs of bytes > 0x20; with `punct` every ASCII punctuation byte is a
 * word of its own.  A word of more than max_word_chars characters is the id of `unk`; any other word is cut greedily,
 * longest match first, into entries -- behind the word's front: entries that start with `prefix`, matched without it --,
 * and is the id of `unk` alone when some piece has no match.  A null row has no ids.  A character starts at every byte
 * that is no continuation byte. */
typedef struct cs_wordpiece_vocab cs_wordpiece_vocab;
/* The vocabulary's hash table on the device; the handle does not refer to `vocab` afterwards.  prefix NULL = "##", unk NULL =
 * "[UNK]".  A null `vocab` / `out`, a prefix of no or more than 8 bytes, or an `unk` that is no entry: CS_ERR_INVALID_ARG;
 * more than 2^24 rows or an entry of more than 255 bytes: CS_ERR_RANGE.  *out = NULL when anything fails. */
int cs_wordpiece_vocab_create(const cs_column* vocab, const char* prefix, const char* unk, cs_stream stream, cs_wordpiece_vocab** out);
void cs_wordpiece_vocab_destroy(cs_wordpiece_vocab* v);
/* the distinct entries, the id of `unk` and the longest entry's bytes (any of the three may be NULL) */
int cs_wordpiece_vocab_info(const cs_wordpiece_vocab* v, int64_t* entries, int32_t* unk_id, int32_t* max_entry_bytes);
/* *id = the id of the entry token[0, nbytes), -1 when it is none */
int cs_wordpiece_vocab_find(const cs_wordpiece_vocab* v, const char* token, int64_t nbytes, int32_t* id, cs_stream stream);
/* size pass: offsets[rows + 1] (the exclusive scan of the rows' id counts; device memory when on_device) and the total.
 * 1 <= max_word_chars <= 1024, else CS_ERR_RANGE (all three calls). */
int cs_wordpiece_count(const cs_column* col, const cs_wordpiece_vocab* v, int max_word_chars, int punct, int64_t* offsets, int on_device, cs_stream stream,
                       int64_t* total);
/* write pass: ids[total] at the offsets cs_wordpiece_count gave (`offsets` and `ids` are both device memory when on_device).
 * A row writes inside its own offsets only.  A NULL `ids` or a column of no rows writes nothing. */
int cs_wordpiece_ids(const cs_column* col, const cs_wordpiece_vocab* v, int max_word_chars, int punct, const int64_t* offsets, int32_t* ids, int on_device,
                     cs_stream stream);
/* model input in one pass: rows x max_length ids and a rows x max_length mask (1 = token, 0 = padding; may be NULL).  A
 * negative cls_id / sep_id means "none".  A row's ids are cut to max_length minus the specials present, cls_id goes in
 * front of them, sep_id behind, then pad_id; a null row is the specials and padding.  max_length < 1 or less than the
 * specials present: CS_ERR_INVALID_ARG. */
int cs_wordpiece_encode(const cs_column* col, const cs_wordpiece_vocab* v, int max_word_chars, int punct, int max_length, int32_t cls_id, int32_t sep_id,
                        int32_t pad_id, int32_t* ids, uint8_t* mask, int on_device, cs_stream stream);

/* ---- the URL codec, translate and fillna (reference: cpp/src/strings/urlencode.cu, modify.cu:302-489; per-row logic in
 * custrings_amd/csrc/recode_ops.h; kernels cs_recode.hip) --------------------------------------------------------
 * url_encode, url_decode and translate keep null rows null (the output shares the input's validity); an output row of
 * 2^31 bytes or more is CS_ERR_RANGE. */
/* NVStrings::url_encode (NVStrings.h:1181; urlencode.cu:44-164): the ASCII bytes 0-9 A-Z a-z . _ ~ - are copied, every
 * other byte becomes '%' and two upper-case hex digits.  Rows that are not valid UTF-8 follow the same byte rule. */
int cs_url_encode(const cs_column* col, cs_stream stream, cs_column** out);
/* NVStrings::url_decode (NVStrings.h:1188; urlencode.cu:179-277): a '%' with at least two bytes behind it in the row
 * consumes them and emits one byte -- a digit is 0-9, A-Z (value c - 55) or a-z (c - 87), anything else 0, the byte
 * taken modulo 256; every other byte is copied. */
int cs_url_decode(const cs_column* col, cs_stream stream, cs_column** out);
/* NVStrings::translate (NVStrings.h:733; modify.cu:302-390): every character that is a key of the table becomes its
 * target, a target of 0 drops it; `from` / `to` are HOST arrays of n code points.  Of several pairs with one key the
 * last wins.  A sequence that is not one well-formed UTF-8 character (an encoded surrogate included) matches no key and is copied.  A code point above
 * U+10FFFF, n < 0 or a missing array: CS_ERR_INVALID_ARG. */
int cs_translate(const cs_column* col, const uint32_t* from, const uint32_t* to, int n, cs_stream stream, cs_column** out);
/* NVStrings::fillna(const char*) (NVStrings.h:739; modify.cu:395-439): null rows take `str`, the result has no nulls.
 * str NULL: CS_ERR_INVALID_ARG. */
int cs_fillna(const cs_column* col, const char* str, cs_stream stream, cs_column** out);
/* NVStrings::fillna(NVStrings&) (NVStrings.h:747; modify.cu:444-489): a null row takes the same row of `repl` (and stays
 * null where that is null too).  Another row count: CS_ERR_INVALID_ARG. */
int cs_fillna_column(const cs_column* col, const cs_column* repl, cs_stream stream, cs_column** out);

/* ---- numeric categories (numeric_category.h) ---------------------------- */
/* Sorted unique keys of one numeric type and an int32 value per row.  -0.0 and +0.0 are one key; all NaN are one key,
 * behind +inf.  The number kept for a key is that of the lowest-indexed row of its class.  `nulls` is an LSB-first bitmask,
 * a 0 bit is a null item; when an item is null, key 0 is the null key and null rows have value 0.  A row is null exactly
 * when the key set includes the null key and the row's value is 0: the bitmask of a category follows from its values.
 * `on_device` says where the caller's arrays (items, nulls, indexes, results) live.  Outputs own their buffers. */
typedef struct cs_numcat cs_numcat;
typedef enum cs_numtype { CS_NUM_I8 = 0, CS_NUM_I32 = 1, CS_NUM_I64 = 2, CS_NUM_F32 = 3, CS_NUM_F64 = 4 } cs_numtype;
/* numeric_category<T>(items, count, nulls).  items NULL or n == 0: an empty category.  n >= 2^31 - 1: CS_ERR_RANGE. */
int cs_numcat_build(const void* items, int64_t n, const uint8_t* nulls, cs_numtype type, int on_device, cs_stream stream,
                    cs_numcat** out);
int cs_numcat_destroy(cs_numcat* cat);
int64_t cs_numcat_size(const cs_numcat* cat);
int64_t cs_numcat_keys_size(const cs_numcat* cat);
int cs_numcat_type(const cs_numcat* cat);              /* cs_numtype */
const void* cs_numcat_keys_ptr(const cs_numcat* cat);  /* device memory; NULL without keys */
const int32_t* cs_numcat_values_ptr(const cs_numcat* cat);
const uint8_t* cs_numcat_nulls_ptr(const cs_numcat* cat); /* NULL unless the key set includes the null key */
int cs_numcat_has_nulls(const cs_numcat* cat);            /* some row is null */
int cs_numcat_keys_have_null(const cs_numcat* cat);
int cs_numcat_get_keys(const cs_numcat* cat, void* out, int on_device, cs_stream stream);
int cs_numcat_get_values(const cs_numcat* cat, int32_t* out, int on_device, cs_stream stream);
/* to_type: results[i] = keys[values[i]] (0 where the value is -1); `nulls`, when given, is always written ((size + 7) / 8
 * bytes, all rows' bits 1 when none is null). */
int cs_numcat_to_type(const cs_numcat* cat, void* results, uint8_t* nulls, int on_device, cs_stream stream);
/* gather_type: keys[indexes[i]]; an index outside [0, keys_size): CS_ERR_RANGE.  The bit of an index that names the null key is 0. */
int cs_numcat_gather_type(const cs_numcat* cat, const int32_t* indexes, int64_t n, void* results, uint8_t* nulls, int on_device,
                          cs_stream stream);
/* `key`: HOST pointer to one number of the category's type, NULL = the null key.  An absent key: -1 / no rows. */
int cs_numcat_index_for(const cs_numcat* cat, const void* key, cs_stream stream, int32_t* out);
/* the rows whose value is the key's index, ascending; `results` may be NULL (count only) */
int cs_numcat_indexes_for(const cs_numcat* cat, const void* key, int32_t* results, int on_device, cs_stream stream, int64_t* count);
/* The key-set family: a new category every time.  Values of removed keys become -1; removing the null key leaves no null rows. */
int cs_numcat_add_keys(const cs_numcat* cat, const void* items, int64_t n, const uint8_t* nulls, int on_device, cs_stream stream,
                       cs_numcat** out);
int cs_numcat_remove_keys(const cs_numcat* cat, const void* items, int64_t n, const uint8_t* nulls, int on_device, cs_stream stream,
                          cs_numcat** out);
int cs_numcat_set_keys(const cs_numcat* cat, const void* items, int64_t n, const uint8_t* nulls, int on_device, cs_stream stream,
                       cs_numcat** out);
int cs_numcat_remove_unused_keys(const cs_numcat* cat, cs_stream stream, cs_numcat** out);
/* merged sorted key set; this category's values followed by cat2's, renumbered.  Different types: CS_ERR_INVALID_ARG. */
int cs_numcat_merge(const cs_numcat* cat, const cs_numcat* cat2, cs_stream stream, cs_numcat** out);
/* gather: same keys, the indexes (each in [0, keys_size)) as values; gather_and_remap: only the keys they name;
 * gather_values: values[indexes[i]], each index in [0, size).  Otherwise CS_ERR_RANGE. */
int cs_numcat_gather(const cs_numcat* cat, const int32_t* indexes, int64_t n, int on_device, cs_stream stream, cs_numcat** out);
int cs_numcat_gather_and_remap(const cs_numcat* cat, const int32_t* indexes, int64_t n, int on_device, cs_stream stream,
                               cs_numcat** out);
int cs_numcat_gather_values(const cs_numcat* cat, const int32_t* indexes, int64_t n, int on_device, cs_stream stream,
                            cs_numcat** out);
int cs_numcat_copy(const cs_numcat* cat, cs_stream stream, cs_numcat** out);
/* A yardstick for tools/bench_ops.py, not a route of the library: the images of all n rows with their row numbers through
 * the radix sort (the reference's algorithm -- sort every row -- on this project's sort).  Nothing is returned; the call
 * waits for the sort.  UNSUPPORTED: a cs_debug_* entry point is not part of the interface a caller may rely on. */
int cs_debug_numcat_sort_rows(const void* items, int64_t n, cs_numtype type, int on_device, cs_stream stream);
/* For the tests of the scan under every output column: runs ONE of the library's lengths-to-offsets routes over `lens`
 * (device, segs * n int32, negative = null row -> 0 bytes) into `offsets` (device, segs * (n + 1) int64), and waits.
 * route 0: the chunk scan with metadata; 1: the same with the validity mask of the fused pass, copied to `validity`
 * (device, (n + 63) / 64 * 8 bytes; may be null, must be null on the other routes); 2: the workgroup scan (what
 * CS_SCAN_BY_WORKGROUPS selects); 3: the scan that reads nothing back; 4: the segmented scan (the only route with segs > 1).
 * out (host, 3 per segment): total bytes, longest row, largest 64-row span; -1 where the route does not report the number.
 * Routes 0 and 2 call the two scans themselves: which of them offsets_from_lengths picks (its reading of CS_SCAN_BY_WORKGROUPS)
 * is not what this entry point covers.  No chars are allocated.  UNSUPPORTED, as every cs_debug_* entry point. */
int cs_debug_offsets_from_lengths(const int32_t* lens, int64_t n, int segs, int route, int64_t* offsets, uint8_t* validity, int64_t* out,
                                  cs_stream stream);
/* For the tests of the stable radix sort under order, sort and both category builds: sorts the n pairs (keys[i], items[i])
 * (both device) by key, unsigned ascending, equal keys in input order, in place, with the library's own sort, and waits.
 * n < 0, or a null pointer with n > 0: CS_ERR_INVALID_ARG; n of 0 or 1 touches nothing.  UNSUPPORTED, as every cs_debug_*
 * entry point. */
int cs_debug_radix_sort_pairs64(uint64_t* keys, int32_t* items, int64_t n, cs_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* CUSTRINGS_AMD_H */
