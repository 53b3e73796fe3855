// numeric_category<T> over the C ABI (include/nvstrings/numeric_category.h), part of libNVCategory.so: five explicit
// instantiations -- int, long, float, double, char -- under the reference's mangled names.
#include "nvstrings/numeric_category.h"

#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "custrings_amd.h"

namespace {
template <class T> struct TypeOf;
template <> struct TypeOf<char> { static constexpr cs_numtype code = CS_NUM_I8; static const char* name() { return "int8"; } };
template <> struct TypeOf<int> { static constexpr cs_numtype code = CS_NUM_I32; static const char* name() { return "int32"; } };
template <> struct TypeOf<long> { static constexpr cs_numtype code = CS_NUM_I64; static const char* name() { return "int64"; } };
template <> struct TypeOf<float> { static constexpr cs_numtype code = CS_NUM_F32; static const char* name() { return "float32"; } };
template <> struct TypeOf<double> { static constexpr cs_numtype code = CS_NUM_F64; static const char* name() { return "float64"; } };
static_assert(sizeof(long) == 8, "long is the 64-bit key type");

void check(int status) {
  if (status == CS_OK) return;
  const char* m = cs_last_error();
  const std::string msg = m ? m : "numeric_category: the operation failed";
  if (status == CS_ERR_RANGE) throw std::out_of_range(msg);
  if (status == CS_ERR_INVALID_ARG) throw std::invalid_argument(msg);
  throw std::runtime_error(msg);
}
void ready() {
  if (cs_current_device() < 0) check(cs_init(0));
}
}  // namespace

template <typename T>
numeric_category<T>::numeric_category() : handle_(nullptr) {}
template <typename T>
numeric_category<T>::numeric_category(const numeric_category&) : handle_(nullptr) {}
template <typename T>
numeric_category<T>::numeric_category(const T* items, size_t count, const BYTE* nulls) : handle_(nullptr) {
  ready();
  check(cs_numcat_build(items, (int64_t)count, nulls, TypeOf<T>::code, 1, nullptr, &handle_));
}
template <typename T>
numeric_category<T>::~numeric_category() {
  if (handle_) cs_numcat_destroy(handle_);
}
template <typename T>
numeric_category<T>* numeric_category<T>::adopt(cs_numcat* cat) {
  numeric_category<T>* c = new numeric_category<T>;
  c->handle_ = cat;
  return c;
}
template <typename T>
cs_numcat* numeric_category<T>::handle() const { return handle_; }
template <typename T>
cs_numcat* numeric_category<T>::release() {
  cs_numcat* h = handle_;
  handle_ = nullptr;
  return h;
}
template <typename T>
const char* numeric_category<T>::get_type_name() { return TypeOf<T>::name(); }

template <typename T>
numeric_category<T>* numeric_category<T>::copy() {
  cs_numcat* out = nullptr;
  check(cs_numcat_copy(handle_, nullptr, &out));
  return adopt(out);
}
template <typename T>
size_t numeric_category<T>::size() { return (size_t)cs_numcat_size(handle_); }
template <typename T>
size_t numeric_category<T>::keys_size() { return (size_t)cs_numcat_keys_size(handle_); }
template <typename T>
const T* numeric_category<T>::keys() { return static_cast<const T*>(cs_numcat_keys_ptr(handle_)); }
template <typename T>
const int* numeric_category<T>::values() { return cs_numcat_values_ptr(handle_); }
template <typename T>
const BYTE* numeric_category<T>::nulls_bitmask() { return cs_numcat_nulls_ptr(handle_); }
template <typename T>
bool numeric_category<T>::has_nulls() { return cs_numcat_has_nulls(handle_) != 0; }
template <typename T>
bool numeric_category<T>::keys_have_null() { return cs_numcat_keys_have_null(handle_) != 0; }

template <typename T>
void numeric_category<T>::print(const char* prefix, const char* delimiter) {
  std::vector<T> k(keys_size() ? keys_size() : 1);
  std::vector<int> v(size() ? size() : 1);
  check(cs_numcat_get_keys(handle_, k.data(), 0, nullptr));
  check(cs_numcat_get_values(handle_, v.data(), 0, nullptr));
  const bool hn = keys_have_null();
  std::printf("%s", prefix);
  if (!keys_size()) std::printf("<no keys>");
  for (size_t i = 0; i < keys_size(); ++i) {
    if (i == 0 && hn) std::printf("-%s", delimiter);
    else std::printf("%s%s", std::to_string(k[i]).c_str(), delimiter);
  }
  std::printf("\n%s", prefix);
  if (!size()) std::printf("<no values>");
  for (size_t i = 0; i < size(); ++i) {
    if (hn && v[i] == 0) std::printf("-%s", delimiter);
    else std::printf("%d%s", v[i], delimiter);
  }
  std::printf("\n");
}

template <typename T>
const T numeric_category<T>::get_key_for(int idx) {
  if (idx < 0 || (size_t)idx >= keys_size()) throw std::out_of_range("get_key_for: invalid index value");
  std::vector<T> k(keys_size());
  check(cs_numcat_get_keys(handle_, k.data(), 0, nullptr));
  return k[(size_t)idx];
}
template <typename T>
bool numeric_category<T>::is_value_null(int idx) {
  if (idx < 0 || (size_t)idx >= size()) throw std::out_of_range("is_value_null: invalid index value");
  if (!keys_have_null()) return false;
  std::vector<int> v(size());
  check(cs_numcat_get_values(handle_, v.data(), 0, nullptr));
  return v[(size_t)idx] == 0;
}
template <typename T>
int numeric_category<T>::get_index_for(T key) {
  int32_t out = -1;
  check(cs_numcat_index_for(handle_, &key, nullptr, &out));
  return out;
}
template <typename T>
size_t numeric_category<T>::get_indexes_for(T key, int* result) {
  int64_t n = 0;
  check(cs_numcat_indexes_for(handle_, &key, result, 1, nullptr, &n));
  return (size_t)n;
}
template <typename T>
size_t numeric_category<T>::get_indexes_for_null_key(int* result) {
  int64_t n = 0;
  check(cs_numcat_indexes_for(handle_, nullptr, result, 1, nullptr, &n));
  return (size_t)n;
}

#define KEY_SET(NAME)                                                                                    \
  template <typename T>                                                                                  \
  numeric_category<T>* numeric_category<T>::NAME(const T* items, size_t count, const BYTE* nulls) {      \
    cs_numcat* out = nullptr;                                                                            \
    check(cs_numcat_##NAME(handle_, items, (int64_t)count, nulls, 1, nullptr, &out));                    \
    return adopt(out);                                                                                   \
  }
KEY_SET(add_keys)
KEY_SET(remove_keys)
KEY_SET(set_keys)
#undef KEY_SET
template <typename T>
numeric_category<T>* numeric_category<T>::remove_unused_keys() {
  cs_numcat* out = nullptr;
  check(cs_numcat_remove_unused_keys(handle_, nullptr, &out));
  return adopt(out);
}
template <typename T>
numeric_category<T>* numeric_category<T>::merge(numeric_category<T>& cat) {
  cs_numcat* out = nullptr;
  check(cs_numcat_merge(handle_, cat.handle_, nullptr, &out));
  return adopt(out);
}
#define BY_INDEXES(NAME)                                                                 \
  template <typename T>                                                                  \
  numeric_category<T>* numeric_category<T>::NAME(const int* indexes, size_t count) {     \
    cs_numcat* out = nullptr;                                                            \
    check(cs_numcat_##NAME(handle_, indexes, (int64_t)count, 1, nullptr, &out));         \
    return adopt(out);                                                                   \
  }
BY_INDEXES(gather)
BY_INDEXES(gather_and_remap)
BY_INDEXES(gather_values)
#undef BY_INDEXES
template <typename T>
void numeric_category<T>::to_type(T* results, BYTE* nulls) {
  check(cs_numcat_to_type(handle_, results, nulls, 1, nullptr));
}
template <typename T>
void numeric_category<T>::gather_type(const int* indexes, size_t count, T* results, BYTE* nulls) {
  check(cs_numcat_gather_type(handle_, indexes, (int64_t)count, results, nulls, 1, nullptr));
}

template class __attribute__((visibility("default"))) numeric_category<int>;
template class __attribute__((visibility("default"))) numeric_category<long>;
template class __attribute__((visibility("default"))) numeric_category<float>;
template class __attribute__((visibility("default"))) numeric_category<double>;
template class __attribute__((visibility("default"))) numeric_category<char>;
