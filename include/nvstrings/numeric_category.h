/* numeric_category<T> -- a category whose keys are numbers: sorted unique keys of type T and an int32 value per item.
 * The members, their order and their signatures are those of the reference's class (cpp/include/numeric_category.h), so a
 * caller built against that header links against libNVCategory.so; the text and everything behind it are this project's
 * (the C ABI's cs_numcat, include/custrings_amd.h).
 *
 * T is one of int, long, float, double, char (get_type_name(): "int32", "int64", "float32", "float64", "int8"); those five
 * are instantiated in the library.  Every array argument -- items, nulls, indexes, results -- is DEVICE memory, as in the
 * reference; `nulls` is an LSB-first bitmask where a 0 bit marks a null item.  When an item is null, key 0 is the null key
 * and null items have value 0.  gather* and gather_type throw std::out_of_range on an index outside the keys (the values
 * for gather_values); other failures throw std::runtime_error or std::invalid_argument. */
#ifndef NVSTRINGS_AMD_NUMERIC_CATEGORY_H
#define NVSTRINGS_AMD_NUMERIC_CATEGORY_H

#include <cstddef>

#include "base_category.h"

typedef unsigned char BYTE;
struct cs_numcat;

template <typename T>
class numeric_category : base_category_type { /* the object begins with the vtable pointer, like NVCategory */
  cs_numcat* handle_;

  numeric_category();
  numeric_category(const numeric_category&);

 public:
  numeric_category(const T* items, size_t count, const BYTE* nulls = nullptr);
  ~numeric_category();

  numeric_category<T>* copy();

  size_t size();      /* items */
  size_t keys_size(); /* keys, the null key included */

  const T* keys();             /* device memory */
  const int* values();         /* device memory */
  const BYTE* nulls_bitmask(); /* device memory; nullptr unless the key set includes the null key */
  bool has_nulls();            /* some item is null */
  bool keys_have_null();

  void print(const char* prefix = "", const char* delimiter = " ");
  const char* get_type_name();

  const T get_key_for(int idx);
  bool is_value_null(int idx);

  int get_index_for(T key);                      /* -1 when the key is absent */
  size_t get_indexes_for(T key, int* result);    /* result may be nullptr: the count alone */
  size_t get_indexes_for_null_key(int* result);

  /* each returns a new instance; values of keys that go away become -1 */
  numeric_category<T>* add_keys(const T* items, size_t count, const BYTE* nulls = nullptr);
  numeric_category<T>* remove_keys(const T* items, size_t count, const BYTE* nulls = nullptr);
  numeric_category<T>* remove_unused_keys();
  numeric_category<T>* set_keys(const T* items, size_t count, const BYTE* nulls = nullptr);
  numeric_category<T>* merge(numeric_category<T>& cat);

  numeric_category<T>* gather(const int* indexes, size_t count);
  numeric_category<T>* gather_and_remap(const int* indexes, size_t count);
  numeric_category<T>* gather_values(const int* indexes, size_t count);

  /* results holds size() (count) numbers, nulls (size() + 7) / 8 bytes; a nulls buffer that is passed is always written */
  void to_type(T* results, BYTE* nulls = nullptr);
  void gather_type(const int* indexes, size_t count, T* results, BYTE* nulls = nullptr);

  /* ---- this project's additions: the C-ABI handle behind the instance ---- */
  static numeric_category<T>* adopt(cs_numcat* cat);
  cs_numcat* handle() const;
  cs_numcat* release(); /* gives the handle back to the caller: the instance is empty afterwards */
};

#endif
