/* StringsStatistics -- what NVStrings::compute_statistics fills (include/nvstrings/NVStrings.h).
 *
 * Field names, types and order are those of the reference's StringsStatistics.h, so that a caller compiled against either
 * header reads the same object.  Declarations only.  What each figure means on this back-end -- the minima over the
 * non-zero values, total_memory as NVStrings::memsize(), the *_95 left 0 -- is in include/custrings_amd.h at
 * cs_column_statistics and in INTEGRATION.md.
 */
#ifndef NVSTRINGS_AMD_STRINGSSTATISTICS_H
#define NVSTRINGS_AMD_STRINGSSTATISTICS_H

#include <cstddef>
#include <utility>
#include <vector>

struct StringsStatistics {
  size_t total_bytes, total_chars;
  size_t bytes_avg, bytes_max, bytes_min, bytes_95;
  size_t chars_avg, chars_max, chars_min, chars_95;
  size_t total_memory;
  size_t mem_avg, mem_max, mem_min, mem_95;
  size_t total_strings;
  size_t total_nulls;
  size_t total_empty;
  size_t unique_strings;
  size_t whitespace_count;
  size_t digits_count;
  size_t uppercase_count, lowercase_count;
  /* (character as packed UTF-8 bytes, count) in code-point order */
  std::vector<std::pair<unsigned int, unsigned int> > char_counts;
};

#endif
