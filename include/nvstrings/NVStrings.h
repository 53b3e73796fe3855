/* NVStrings -- host C++ class of the custrings API over the MI355X back-end.
 *
 * Same class name, nested types, method names, argument types / defaults and ownership rules as
 * the reference's /root/reference/cpp/include/NVStrings.h (line cited per method), so that code
 * compiled against EITHER header links against libNVStrings.so built from this repository
 * (custrings_amd/host/NVStrings.cpp): the members are out-of-line and exported under the same
 * mangled names.  Instances are immutable; every transforming method returns a new heap instance
 * that the caller frees with NVStrings::destroy (NVStrings.h:52-57,156).
 * Error mapping: CS_ERR_INVALID_ARG -> std::invalid_argument, CS_ERR_RANGE ->
 * std::out_of_range where the reference throws that (gather), else std::invalid_argument; anything
 * else -> std::runtime_error; integer returns where the reference returns integers.
 * Members of the reference outside SURVEY.md section 8 are not declared.
 */
#ifndef NVSTRINGS_AMD_NVSTRINGS_H
#define NVSTRINGS_AMD_NVSTRINGS_H

#include <cstddef>
#include <utility>
#include <vector>

struct cs_column;
struct nvstrings_ipc_transfer; /* nvstrings/ipc_transfer.h */
struct StringsStatistics;      /* nvstrings/StringsStatistics.h */

class NVStrings {
  cs_column* m_col; /* (the reference holds an NVStringsImpl* here; one pointer either way) */

  /* ctors / dtor are private to control allocation (NVStrings.h:52-57) */
  NVStrings();
  NVStrings(unsigned int count);
  NVStrings(const NVStrings&);
  NVStrings& operator=(const NVStrings&) = delete;
  ~NVStrings();

 public:
  /* NVStrings.h:66-70 */
  enum sorttype { none = 0, length = 1, name = 2 };

  /* ---- construction (NVStrings.h:86-156) ---- */
  static NVStrings* create_from_array(const char** strs, unsigned int count);
  static NVStrings* create_from_index(std::pair<const char*, size_t>* strs, unsigned int count, bool devmem = true, sorttype stype = none);
  // one column of a CSV file (NVStrings.h:146); null when the file cannot be opened or holds fewer than 2 bytes
  static NVStrings* create_from_csv(const char* csvfile, unsigned int column, unsigned int lines = 0, sorttype stype = none, bool nullIsEmpty = false);
  static NVStrings* create_from_offsets(const char* strs, int count, const int* offsets, const unsigned char* nullbitmask = 0, int nulls = 0,
                                        bool devmem = true);
  static NVStrings* create_from_strings(std::vector<NVStrings*> strs);
  static NVStrings* create_from_ipc(nvstrings_ipc_transfer& ipc); /* NVStrings.h:132: maps the exporter's buffers, no copy */
  static void destroy(NVStrings* inst);

  /* ---- attributes / export (NVStrings.h:162-354) ---- */
  size_t memsize() const;
  unsigned int size() const;
  int create_index(std::pair<const char*, size_t>* strs, bool devmem = true);
  int create_offsets(char* strs, int* offsets, unsigned char* nullbitmask = 0, bool devmem = true);
  int create_ipc_transfer(nvstrings_ipc_transfer& ipc); /* NVStrings.h:214 */
  unsigned int set_null_bitarray(unsigned char* bitarray, bool emptyIsNull = false, bool devmem = true);
  NVStrings* copy();
  int to_host(char** list, int start, int end);
  unsigned int len(int* lengths, bool devmem = true);
  size_t byte_count(int* lengths, bool devmem = true);
  /* NVStrings.h:1203 -- every length, memory and class figure, the distinct count and the character histogram, from one
   * read of the chars and one category build (cs_column_statistics, include/custrings_amd.h) */
  void compute_statistics(StringsStatistics& stats);

  /* ---- re-arrangement (NVStrings.h:261-334; array.cu) ---- */
  NVStrings* sublist(unsigned int start, unsigned int end, int step = 0);
  NVStrings* gather(const int* pos, unsigned int count, bool devmem = true);
  NVStrings* gather(const bool* mask, bool devmem = true);
  NVStrings* scatter(NVStrings& strs, const int* pos, bool devmem = true);
  NVStrings* scatter(const char* str, const int* pos, unsigned int count, bool devmem = true);
  NVStrings* remove_strings(const int* pos, unsigned int count, bool devmem = true);
  NVStrings* sort(sorttype stype = sorttype::name, bool ascending = true, bool nullfirst = true);
  int order(sorttype stype, bool ascending, unsigned int* indexes, bool nullfirst = true, bool devmem = true);

  /* ---- combine (NVStrings.h:437-452; combine.cu) ---- */
  NVStrings* cat(NVStrings* others, const char* separator, const char* narep = nullptr);
  NVStrings* cat(std::vector<NVStrings*>& others, const char* separator, const char* narep = nullptr);
  NVStrings* join(const char* separator = "", const char* narep = nullptr);

  /* ---- split family (NVStrings.h:464-552; split.cu) ---- */
  int split_record(const char* delimiter, int maxsplit, std::vector<NVStrings*>& results);
  int rsplit_record(const char* delimiter, int maxsplit, std::vector<NVStrings*>& results);
  int split_record(int maxsplit, std::vector<NVStrings*>& results);
  int rsplit_record(int maxsplit, std::vector<NVStrings*>& results);
  unsigned int split(const char* delimiter, int maxsplit, std::vector<NVStrings*>& results);
  unsigned int rsplit(const char* delimiter, int maxsplit, std::vector<NVStrings*>& results);
  unsigned int split(int maxsplit, std::vector<NVStrings*>& results);
  unsigned int rsplit(int maxsplit, std::vector<NVStrings*>& results);
  int partition(const char* delimiter, std::vector<NVStrings*>& results);
  int rpartition(const char* delimiter, std::vector<NVStrings*>& results);

  /* ---- regex extraction (NVStrings.h:682-693,943-952) ---- */
  int extract(const char* pattern, std::vector<NVStrings*>& results);
  int extract_record(const char* pattern, std::vector<NVStrings*>& results);
  int findall(const char* pattern, std::vector<NVStrings*>& results);
  int findall_record(const char* pattern, std::vector<NVStrings*>& results);

  /* ---- replace / strip / case (NVStrings.h:714-820) ---- */
  NVStrings* replace(const char* str, const char* repl, int maxrepl = -1);
  NVStrings* replace_re(const char* pattern, const char* repl, int maxrepl = -1);
  NVStrings* replace_re(std::vector<const char*>& patterns, NVStrings& repls);
  NVStrings* replace_with_backrefs(const char* pattern, const char* repl);
  NVStrings* lstrip(const char* to_strip);
  NVStrings* strip(const char* to_strip);
  NVStrings* rstrip(const char* to_strip);
  NVStrings* lower();
  NVStrings* upper();
  /* swapcase / capitalize / title (NVStrings.h:825-835; case.cu:169-397).  capitalize maps only characters up to U+0FFF
   * (the reference's bound); title treats every non-letter as a word break. */
  NVStrings* capitalize();
  NVStrings* swapcase();
  NVStrings* title();

  /* ---- character types (NVStrings.h:362-427; attrs.cu:115-438): one bool per row, the count of true rows returned
   * (0 for an empty instance or a null `results`).  A null row is false (true for is_empty); an empty row is false
   * (true for is_empty).  islower / isupper look at alphabetic characters only. ---- */
  unsigned int isalnum(bool* results, bool devmem = true);
  unsigned int isalpha(bool* results, bool devmem = true);
  unsigned int isdigit(bool* results, bool devmem = true);
  unsigned int isspace(bool* results, bool devmem = true);
  unsigned int isdecimal(bool* results, bool devmem = true);
  unsigned int isnumeric(bool* results, bool devmem = true);
  unsigned int islower(bool* results, bool devmem = true);
  unsigned int isupper(bool* results, bool devmem = true);
  unsigned int is_empty(bool* results, bool devmem = true);

  /* ---- substrings, padding, wrapping (NVStrings.h:561-754; substr.cu, pad.cu, modify.cu).  padside's enumerators and
   * their order are the reference's: they are part of the mangled names.  slice with stop > 0 && start > stop, a null
   * repl and an output row of 2^31 bytes or more throw std::invalid_argument. ---- */
  NVStrings* repeat(unsigned int count);
  enum padside {
    left,   ///< Add padding to the left.
    right,  ///< Add padding to the right.
    both    ///< Add padding equally to the right and left.
  };
  NVStrings* pad(unsigned int width, padside side, const char* fillchar = nullptr);
  NVStrings* ljust(unsigned int width, const char* fillchar = nullptr);
  NVStrings* center(unsigned int width, const char* fillchar = nullptr);
  NVStrings* rjust(unsigned int width, const char* fillchar = nullptr);
  NVStrings* zfill(unsigned int width);
  NVStrings* wrap(unsigned int width);
  NVStrings* get(unsigned int pos);
  NVStrings* slice(int start = 0, int stop = -1, int step = 1);
  NVStrings* slice_from(const int* starts = nullptr, const int* ends = nullptr);  // device memory, size() values each
  NVStrings* slice_replace(const char* repl, int start = 0, int stop = -1);
  NVStrings* insert(const char* repl, int pos = 0);

  /* ---- the URL codec, translate and fillna (NVStrings.h:733-747,1181-1188; urlencode.cu, modify.cu:302-489).  The table
   * is `count` (code point, code point) pairs, a target of 0 dropping the character; of several pairs with one key the
   * last wins.  A null `str`, another row count and a code point above U+10FFFF throw std::invalid_argument. ---- */
  NVStrings* translate(std::pair<unsigned, unsigned>* table, unsigned int count);
  NVStrings* fillna(const char* str);
  NVStrings* fillna(NVStrings& strs);
  NVStrings* url_encode();
  NVStrings* url_decode();

  /* ---- search (NVStrings.h:861-981) ---- */
  unsigned int find(const char* str, int start, int end, int* results, bool devmem = true);
  int contains(const char* str, bool* results, bool devmem = true);
  // the rest of the find family (reference NVStrings.h:849-934; find.cu)
  unsigned int compare(const char* str, int* results, bool devmem = true);
  unsigned int rfind(const char* str, int start, int end, int* results, bool devmem = true);
  unsigned int find_from(const char* str, int* starts, int* ends, int* results, bool devmem = true);
  unsigned int find_multiple(NVStrings& strs, int* results, bool devmem = true);
  int match_strings(NVStrings& strs, bool* results, bool devmem = true);
  unsigned int startswith(const char* str, bool* results, bool devmem = true);
  unsigned int endswith(const char* str, bool* results, bool devmem = true);
  int contains_re(const char* pattern, bool* results, bool devmem = true);
  int match(const char* pattern, bool* results, bool devmem = true);
  int count_re(const char* pattern, int* results, bool devmem = true);

  /* ---- conversions (NVStrings.h:991-1124; convert.cu).  Parse members return the count of non-zero results,
   * -1 for an empty instance or a null `results`; `long*` stays `long*` so the mangled names match. ---- */
  int stoi(int* results, bool devmem = true);
  int stol(long* results, bool devmem = true);
  int htoi(unsigned int* results, bool devmem = true);
  int stof(float* results, bool devmem = true);
  int stod(double* results, bool devmem = true);
  int hash(unsigned int* results, bool devmem = true);
  static NVStrings* itos(const int* values, unsigned int count, const unsigned char* nullbitmask = nullptr, bool devmem = true);
  static NVStrings* ltos(const long* values, unsigned int count, const unsigned char* nullbitmask = nullptr, bool devmem = true);
  static NVStrings* ftos(const float* values, unsigned int count, const unsigned char* nullbitmask = nullptr, bool devmem = true);
  static NVStrings* dtos(const double* values, unsigned int count, const unsigned char* nullbitmask = nullptr, bool devmem = true);
  int to_bools(bool* results, const char* true_string, bool devmem = true);
  static NVStrings* create_from_bools(const bool* values, unsigned int count, const char* true_string, const char* false_string,
                                      const unsigned char* nullbitmask = nullptr, bool devmem = true);
  int ip2int(unsigned int* results, bool devmem = true);
  static NVStrings* int2ip(const unsigned int* values, unsigned int count, const unsigned char* nullbitmask = nullptr, bool devmem = true);

  /* ---- timestamps (NVStrings.h:1126-1171; datetime.cu).  The enumerators and their order are the reference's: they are
   * part of the mangled names.  Format errors and a null `values` / zero `count` throw std::invalid_argument. ---- */
  enum timestamp_units {
    years,    ///< precision is years
    months,   ///< precision is months
    days,     ///< precision is days
    hours,    ///< precision is hours
    minutes,  ///< precision is minutes
    seconds,  ///< precision is seconds
    ms,       ///< precision is milliseconds
    us,       ///< precision is microseconds
    ns        ///< precision is nanoseconds
  };
  int timestamp2long(const char* format, timestamp_units units, unsigned long* results, bool devmem = true);
  static NVStrings* long2timestamp(const unsigned long* values, unsigned int count, timestamp_units units, const char* format,
                                   const unsigned char* nullbitmask = nullptr, bool devmem = true);

  /* ---- not in the reference: the bridge to the C ABI (used by libNVCategory / libNVText and by callers that
   * want the native record form or the engine's handles) ---- */
  static NVStrings* adopt(cs_column* column); /* takes ownership of a handle produced by the C ABI */
  cs_column* handle() const;
  cs_column* release();              /* gives the handle back to the caller: the instance is empty afterwards */
  static void check(int status);     /* cs_status -> the exceptions listed above */
  static void ensure_device();       /* binds the process to a GPU once (the device cs_init chose, else LOCAL_RANK, else 0) */
};

#endif
