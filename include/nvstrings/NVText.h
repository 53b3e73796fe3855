/* NVText -- tokenize, n-grams, the token counters, string matches, edit distance and stemmer measure of /root/reference/cpp/include/NVText.h over the C ABI.
 * Out-of-line, exported by libNVText.so (custrings_amd/host/NVText.cpp) under the reference's mangled names. */
#ifndef NVSTRINGS_AMD_NVTEXT_H
#define NVSTRINGS_AMD_NVTEXT_H

class NVStrings;

class NVText {
 public:
  /* NVText.h:40 -- delimiter nullptr = whitespace, else ANY character of `delimiter` separates */
  static NVStrings* tokenize(NVStrings& strs, const char* delimiter = nullptr);
  /* NVText.h:48 -- every row of `delimiters` is a whole-string delimiter */
  static NVStrings* tokenize(NVStrings& strs, NVStrings& delimiters);
  /* NVText.h:56-116 (tokens.cu:262-716) */
  static NVStrings* unique_tokens(NVStrings& strs, const char* delimiter = nullptr);
  static unsigned int token_count(NVStrings& strs, const char* delimiter, unsigned int* results, bool devmem = true);
  static unsigned int tokens_counts(NVStrings& strs, NVStrings& tokens, const char* delimiter, unsigned int* results, bool devmem = true);
  static NVStrings* replace_tokens(NVStrings& strs, NVStrings& tgts, NVStrings& repls, const char* delimiter = nullptr);
  static NVStrings* normalize_spaces(NVStrings& strs);
  /* NVText.h:76,86 (NVText.cu:32-123) -- results[row * tokens.size() + token]: does / how often does the token occur in the row */
  static unsigned int contains_strings(NVStrings& strs, NVStrings& tokens, bool* results, bool devmem = true);
  static unsigned int strings_counts(NVStrings& strs, NVStrings& tokens, unsigned int* results, bool devmem = true);
  /* NVText.h:121-144 (edit_distance.cu:119-228) -- Levenshtein distance in characters to one string, or row by row to strs2;
   * std::invalid_argument for another algorithm, a null `str` / `results`, columns of different sizes */
  enum distance_type { levenshtein };
  static unsigned int edit_distance(distance_type algo, NVStrings& strs, const char* str, unsigned int* results, bool devmem = true);
  static unsigned int edit_distance(distance_type algo, NVStrings& strs1, NVStrings& strs2, unsigned int* results, bool devmem = true);
  /* NVText.h:153 */
  static NVStrings* create_ngrams(NVStrings& strs, unsigned int ngrams, const char* separator);
  /* NVText.h:164 (stemmer.cu:69) -- vowels nullptr = "aeiou", y_char nullptr = "y" */
  static unsigned int porter_stemmer_measure(NVStrings& strs, const char* vowels, const char* y_char, unsigned int* results, bool devmem = true);
  /* NVText.h:173 (NVText.cu:126) -- row i repeated counts[i] times; nullptr for no rows or no counts */
  static NVStrings* scatter_count(NVStrings& strs, unsigned int* counts, bool devmem = true);
};

#endif
