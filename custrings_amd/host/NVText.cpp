// libNVText.so -- the NVText class (include/nvstrings/NVText.h), out of line, over the C ABI.
#include "nvstrings/NVText.h"

#include <stdexcept>

#include "custrings_amd.h"
#include "nvstrings/NVStrings.h"

NVStrings* NVText::tokenize(NVStrings& strs, const char* delimiter) {
  cs_column* c = nullptr;
  NVStrings::check(cs_tokenize(strs.handle(), delimiter, nullptr, &c));
  return NVStrings::adopt(c);
}
NVStrings* NVText::tokenize(NVStrings& strs, NVStrings& delimiters) {
  cs_column* c = nullptr;
  NVStrings::check(cs_tokenize_multi(strs.handle(), delimiters.handle(), nullptr, &c));
  return NVStrings::adopt(c);
}
NVStrings* NVText::unique_tokens(NVStrings& strs, const char* delimiter) {
  cs_column* c = nullptr;
  NVStrings::check(cs_unique_tokens(strs.handle(), delimiter, nullptr, &c));
  return NVStrings::adopt(c);
}
unsigned int NVText::token_count(NVStrings& strs, const char* delimiter, unsigned int* results, bool devmem) {
  NVStrings::check(cs_token_count(strs.handle(), delimiter, results, devmem ? 1 : 0, nullptr));
  return 0;  // tokens.cu:360
}
unsigned int NVText::tokens_counts(NVStrings& strs, NVStrings& tokens, const char* delimiter, unsigned int* results, bool devmem) {
  NVStrings::check(cs_tokens_counts(strs.handle(), tokens.handle(), delimiter, results, devmem ? 1 : 0, nullptr));
  return 0;
}
NVStrings* NVText::replace_tokens(NVStrings& strs, NVStrings& tgts, NVStrings& repls, const char* delimiter) {
  cs_column* c = nullptr;
  NVStrings::check(cs_replace_tokens(strs.handle(), tgts.handle(), repls.handle(), delimiter, nullptr, &c));
  return c ? NVStrings::adopt(c) : nullptr;
}
NVStrings* NVText::normalize_spaces(NVStrings& strs) {
  cs_column* c = nullptr;
  NVStrings::check(cs_normalize_spaces(strs.handle(), nullptr, &c));
  return c ? NVStrings::adopt(c) : nullptr;
}
NVStrings* NVText::create_ngrams(NVStrings& strs, unsigned int ngrams, const char* separator) {
  cs_column* c = nullptr;
  NVStrings::check(cs_ngrams(strs.handle(), ngrams, separator, nullptr, &c));
  return NVStrings::adopt(c);
}
unsigned int NVText::contains_strings(NVStrings& strs, NVStrings& tokens, bool* results, bool devmem) {
  NVStrings::check(cs_contains_strings(strs.handle(), tokens.handle(), reinterpret_cast<uint8_t*>(results), devmem ? 1 : 0, nullptr));
  return 0;  // NVText.cu:67
}
unsigned int NVText::strings_counts(NVStrings& strs, NVStrings& tokens, unsigned int* results, bool devmem) {
  NVStrings::check(cs_strings_counts(strs.handle(), tokens.handle(), results, devmem ? 1 : 0, nullptr));
  return 0;
}
unsigned int NVText::edit_distance(distance_type algo, NVStrings& strs, const char* str, unsigned int* results, bool devmem) {
  if (algo != levenshtein || !str || !results) throw std::invalid_argument("invalid algorithm");  // edit_distance.cu:121
  NVStrings::check(cs_edit_distance(strs.handle(), str, CS_LEVENSHTEIN, results, devmem ? 1 : 0, nullptr));
  return 0;
}
unsigned int NVText::edit_distance(distance_type algo, NVStrings& strs1, NVStrings& strs2, unsigned int* results, bool devmem) {
  if (algo != levenshtein) throw std::invalid_argument("invalid algorithm");            // edit_distance.cu:174
  if (strs1.size() != strs2.size()) throw std::invalid_argument("sizes must match");  // edit_distance.cu:177
  NVStrings::check(cs_edit_distance_column(strs1.handle(), strs2.handle(), CS_LEVENSHTEIN, results, devmem ? 1 : 0, nullptr));
  return 0;
}
unsigned int NVText::porter_stemmer_measure(NVStrings& strs, const char* vowels, const char* y_char, unsigned int* results, bool devmem) {
  NVStrings::check(cs_porter_stemmer_measure(strs.handle(), vowels, y_char, results, devmem ? 1 : 0, nullptr));
  return 0;
}
NVStrings* NVText::scatter_count(NVStrings& strs, unsigned int* counts, bool devmem) {
  cs_column* c = nullptr;
  NVStrings::check(cs_scatter_count(strs.handle(), counts, devmem ? 1 : 0, nullptr, &c));
  return c ? NVStrings::adopt(c) : nullptr;
}
