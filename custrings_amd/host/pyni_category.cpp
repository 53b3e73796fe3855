// pyniNVCategory -- CPython glue of the nvcategory Python class (python/cpp/pycategory.cpp in the reference,
// method table :900-930) over libNVCategory.so.  A handle is a string category (NVCategory) or a numeric one
// (numeric_category<T>, python/cpp/numeric_category.cpp): every entry point the reference routes through the latter asks
// the handle for get_type_name() first (num_of) and takes the numeric path for anything but "custring".
#include <cstring>

#include "custrings_amd.h"
#include "nvstrings/NVCategory.h"
#include "nvstrings/numeric_category.h"
#include "pyni_common.h"

using namespace pyni;

namespace pyni {
template <>
struct Bridge<NVCategory> {
  static NVCategory* wrap(void* h) { return NVCategory::adopt(static_cast<cs_category*>(h)); }
  static void drop(NVCategory* c) {
    c->release();
    NVCategory::destroy(c);
  }
};
}  // namespace pyni

#define SELF(args) ptr_arg<NVCategory>(args, 0)

static PyObject* n_createCategoryFromHostStrings(PyObject*, PyObject* args) {  // pycategory.cpp:89-130
  PyObject* strs = arg(args, 0);
  std::vector<const char*> list;
  if (PyUnicode_Check(strs)) list.push_back(PyUnicode_AsUTF8(strs));
  else if (PyList_Check(strs)) list_strings(strs, list);
  else {
    PyErr_SetString(PyExc_ValueError, "nvcategory: a list of str is required");
    return nullptr;
  }
  return make_instance([&] { return NVCategory::create_from_array(list.data(), (unsigned int)list.size()); });
}
static PyObject* n_createCategoryFromNVStrings(PyObject*, PyObject* args) {  // one nvstrings object or a list of them
  PyObject* o = arg(args, 0);
  std::vector<NVStrings*> all;
  if (PyList_Check(o))
    for (Py_ssize_t i = 0; i < PyList_Size(o); ++i) all.push_back(handle_of<NVStrings>(PyList_GetItem(o, i)));
  else all.push_back(handle_of<NVStrings>(o));
  for (auto* p : all)
    if (!p) {
      PyErr_SetString(PyExc_ValueError, "nvcategory: argument must be nvstrings object(s)");
      return nullptr;
    }
  return make_instance([&] { return all.size() == 1 ? NVCategory::create_from_strings(*all[0]) : NVCategory::create_from_strings(all); });
}
static PyObject* n_createFromOffsets(PyObject*, PyObject* args) {  // (sbuf, obuf, scount, nbuf, ncount, bdevmem)
  Region chars(arg(args, 0)), offs(arg(args, 1)), nulls(arg(args, 3));
  const unsigned int count = (unsigned int)int_arg(args, 2, 0);
  const int ncount = (int)int_arg(args, 4, 0);
  const bool dev = bool_arg(args, 5);
  return make_instance(
      [&] { return NVCategory::create_from_offsets((const char*)chars.p, count, (const int*)offs.p, (const unsigned char*)nulls.p, ncount, dev); });
}
// ---- numeric categories ----------------------------------------------------------------------------------------------------
namespace {
const char* const kNumNames[] = {"int8", "int32", "int64", "float32", "float64"};  // cs_numtype order
struct Num {
  cs_numcat* h = nullptr;
  int code = -1;
};
// The numeric category behind an argument, if it is one: an integer is a C++ pointer and is asked for its type name through
// base_category_type; an object marked `_numeric` (custrings_amd/nvcategory.py) carries the C-ABI handle in m_cptr.
bool num_of(PyObject* o, Num& out) {
  if (!o || o == Py_None) return false;
  if (PyLong_Check(o)) {
    void* p = PyLong_AsVoidPtr(o);
    if (!p) return false;
    const char* name = reinterpret_cast<base_category_type*>(p)->get_type_name();
    for (int c = 0; c < 5; ++c)
      if (!std::strcmp(name, kNumNames[c])) {
        out.code = c;
        switch (c) {
          case CS_NUM_I8: out.h = reinterpret_cast<numeric_category<char>*>(p)->handle(); break;
          case CS_NUM_I32: out.h = reinterpret_cast<numeric_category<int>*>(p)->handle(); break;
          case CS_NUM_I64: out.h = reinterpret_cast<numeric_category<long>*>(p)->handle(); break;
          case CS_NUM_F32: out.h = reinterpret_cast<numeric_category<float>*>(p)->handle(); break;
          default: out.h = reinterpret_cast<numeric_category<double>*>(p)->handle(); break;
        }
        return true;
      }
    return false;
  }
  if (!PyObject_HasAttrString(o, "_numeric")) return false;
  PyObject* a = PyObject_GetAttrString(o, "m_cptr");
  if (!a) {
    PyErr_Clear();
    return false;
  }
  out.h = static_cast<cs_numcat*>(a == Py_None ? nullptr : PyLong_AsVoidPtr(a));
  Py_DECREF(a);
  out.code = cs_numcat_type(out.h);
  return out.h != nullptr;
}
PyObject* num_instance(cs_numcat* h, int code) {  // the C++ instance a new handle is returned as
  switch (code) {
    case CS_NUM_I8: return from_ptr(numeric_category<char>::adopt(h));
    case CS_NUM_I32: return from_ptr(numeric_category<int>::adopt(h));
    case CS_NUM_I64: return from_ptr(numeric_category<long>::adopt(h));
    case CS_NUM_F32: return from_ptr(numeric_category<float>::adopt(h));
    default: return from_ptr(numeric_category<double>::adopt(h));
  }
}
void num_delete(void* p, int code) {
  switch (code) {
    case CS_NUM_I8: delete reinterpret_cast<numeric_category<char>*>(p); break;
    case CS_NUM_I32: delete reinterpret_cast<numeric_category<int>*>(p); break;
    case CS_NUM_I64: delete reinterpret_cast<numeric_category<long>*>(p); break;
    case CS_NUM_F32: delete reinterpret_cast<numeric_category<float>*>(p); break;
    default: delete reinterpret_cast<numeric_category<double>*>(p); break;
  }
}
bool num_ok(int status) {  // a C-ABI status as the ValueError every failure of the glue is
  if (status == CS_OK) return true;
  const char* m = cs_last_error();
  PyErr_SetString(PyExc_ValueError, m && *m ? m : "nvcategory: the operation failed");
  return false;
}
// A numeric array argument: a typed buffer (numpy array: host memory, the dtype read from its format; datetime64 is taken
// as int64) or an integer address (device memory, of the type the caller already knows).
struct NumBuf {
  Py_buffer view{};
  bool has_view = false, none = false, bad = false;
  PyObject* viewed = nullptr;
  void* p = nullptr;
  int64_t n = -1;  // -1: an address, the length is not known
  int code = -1, on_device = 0;
  NumBuf(PyObject* o, int known_code) {
    if (!o || o == Py_None) {
      none = true;
      return;
    }
    if (PyLong_Check(o)) {
      p = PyLong_AsVoidPtr(o);
      none = p == nullptr;
      on_device = 1;
      code = known_code;
      return;
    }
    if (PyObject* dt = PyObject_GetAttrString(o, "dtype")) {
      PyObject* s = PyObject_Str(dt);
      const char* name = s ? PyUnicode_AsUTF8(s) : nullptr;
      if (name && !std::strncmp(name, "datetime64", 10)) viewed = PyObject_CallMethod(o, "view", "s", "int64");
      Py_XDECREF(s);
      Py_DECREF(dt);
    }
    PyErr_Clear();
    if (PyObject_GetBuffer(viewed ? viewed : o, &view, PyBUF_FORMAT | PyBUF_ND | PyBUF_C_CONTIGUOUS) != 0) {
      PyErr_Clear();
      bad = true;
      return;
    }
    has_view = true;
    const char* f = view.format ? view.format : "B";
    if (*f == '<' || *f == '=' || *f == '@') ++f;
    const size_t isz = (size_t)view.itemsize;
    if (f[1] == 0) {
      if (*f == 'b' && isz == 1) code = CS_NUM_I8;
      else if ((*f == 'i' || *f == 'l') && isz == 4) code = CS_NUM_I32;
      else if ((*f == 'l' || *f == 'q') && isz == 8) code = CS_NUM_I64;
      else if (*f == 'f' && isz == 4) code = CS_NUM_F32;
      else if (*f == 'd' && isz == 8) code = CS_NUM_F64;
    }
    bad = code < 0;
    p = view.buf;
    n = isz ? (int64_t)(view.len / (Py_ssize_t)isz) : 0;
  }
  ~NumBuf() {
    if (has_view) PyBuffer_Release(&view);
    Py_XDECREF(viewed);
  }
  NumBuf(const NumBuf&) = delete;
};
bool bad_dtype(const NumBuf& b) {
  if (!b.bad) return false;
  PyErr_Format(PyExc_ValueError, "invalid dtype in nvcategory dispatcher: %s", b.has_view && b.view.format ? b.view.format : "not an array");
  return true;
}
// an array that must hold the category's type (code) -- or, with want = CS_NUM_I32, int32 indexes -- and at least `need` items
bool typed(const NumBuf& b, int want, int64_t need, const char* what) {
  if (bad_dtype(b)) return false;
  if (b.none) {
    PyErr_Format(PyExc_ValueError, "%s: an array is required", what);
    return false;
  }
  if (b.code != want) {
    PyErr_Format(PyExc_ValueError, "%s: array of %s given where %s is required", what, b.code >= 0 ? kNumNames[b.code] : "?", kNumNames[want]);
    return false;
  }
  if (b.n >= 0 && b.n < need) {
    PyErr_Format(PyExc_ValueError, "%s: the array holds %lld items, %lld are required", what, (long long)b.n, (long long)need);
    return false;
  }
  return true;
}
// a bitmask argument: any one-byte buffer (host) or an address (device); must be on the side `on_device` names
struct MaskBuf {
  Py_buffer view{};
  bool has_view = false, bad = false;
  void* p = nullptr;
  int64_t bytes = -1;
  int on_device = -1;
  explicit MaskBuf(PyObject* o) {
    if (!o || o == Py_None) return;
    if (PyLong_Check(o)) {
      p = PyLong_AsVoidPtr(o);
      on_device = p ? 1 : -1;
      return;
    }
    if (PyObject_GetBuffer(o, &view, PyBUF_ND | PyBUF_C_CONTIGUOUS) != 0) {
      PyErr_Clear();
      bad = true;
      return;
    }
    has_view = true;
    p = view.buf;
    bytes = (int64_t)view.len;
    on_device = 0;
  }
  ~MaskBuf() {
    if (has_view) PyBuffer_Release(&view);
  }
  MaskBuf(const MaskBuf&) = delete;
  bool fits(int on_dev, int64_t items, const char* what) const {
    if (bad || (p && on_device != on_dev) || (p && bytes >= 0 && bytes < (items + 7) / 8)) {
      PyErr_Format(PyExc_ValueError, "%s: the nulls must be a byte array of (count + 7) / 8 bytes in the same memory as the numbers", what);
      return false;
    }
    return true;
  }
};
// A Python number as one item of the category's type.  `absent`: the number is none of an integer type's values (300 for
// int8, 1.5 for int32), so no key can equal it.  A float category takes the nearest float, as the caller's own array would.
bool key_of(PyObject* key, int code, unsigned char out[8], bool& is_null, bool& absent) {
  is_null = key == Py_None;
  absent = false;
  if (is_null) return true;
  const bool is_float = PyFloat_Check(key);
  if (code == CS_NUM_F32 || code == CS_NUM_F64) {
    const double d = PyFloat_AsDouble(key);  // (an int converts; one beyond a double's range raises)
    if (PyErr_Occurred()) return false;
    if (code == CS_NUM_F32) {
      const float v = (float)d;
      std::memcpy(out, &v, 4);
    } else {
      std::memcpy(out, &d, 8);
    }
    return true;
  }
  long long i = 0;
  if (is_float) {
    const double d = PyFloat_AsDouble(key);
    if (!(d >= -9223372036854775808.0 && d < 9223372036854775808.0) || d != (double)(long long)d) {
      absent = true;  // not an integer, NaN, or beyond 64 bits
      return true;
    }
    i = (long long)d;
  } else {
    int overflow = 0;
    i = PyLong_AsLongLongAndOverflow(key, &overflow);
    if (PyErr_Occurred()) return false;
    if (overflow) {
      absent = true;
      return true;
    }
  }
  if (code == CS_NUM_I8) {
    const signed char v = (signed char)i;
    absent = v != i;
    std::memcpy(out, &v, 1);
  } else if (code == CS_NUM_I32) {
    const int v = (int)i;
    absent = v != i;
    std::memcpy(out, &v, 4);
  } else {
    std::memcpy(out, &i, 8);
  }
  return true;
}
PyObject* number_list(const void* p, int code, int64_t n, bool first_is_none) {
  PyObject* ret = PyList_New((Py_ssize_t)n);
  for (int64_t i = 0; i < n; ++i) {
    PyObject* v;
    if (i == 0 && first_is_none) v = none();
    else if (code == CS_NUM_I8) v = PyLong_FromLong(((const signed char*)p)[i]);
    else if (code == CS_NUM_I32) v = PyLong_FromLong(((const int*)p)[i]);
    else if (code == CS_NUM_I64) v = PyLong_FromLongLong(((const long long*)p)[i]);
    else if (code == CS_NUM_F32) v = PyFloat_FromDouble(((const float*)p)[i]);
    else v = PyFloat_FromDouble(((const double*)p)[i]);
    PyList_SetItem(ret, (Py_ssize_t)i, v);
  }
  return ret;
}
PyObject* refuse_numeric(const char* what) {
  PyErr_Format(PyExc_ValueError, "%s: a category of numbers where a category of strings is required", what);
  return nullptr;
}

PyObject* num_get_keys(const Num& c, PyObject* args) {  // numeric_category.cpp:317-345
  const int64_t nk = cs_numcat_keys_size(c.h);
  NumBuf out(arg(args, 1), c.code);
  if (!out.none) {
    if (!typed(out, c.code, nk, "keys") || !num_ok(cs_numcat_get_keys(c.h, out.p, out.on_device, nullptr))) return nullptr;
    return none();
  }
  std::vector<unsigned char> k((size_t)(nk ? nk : 1) * 8);
  if (!num_ok(cs_numcat_get_keys(c.h, k.data(), 0, nullptr))) return nullptr;
  return number_list(k.data(), c.code, nk, cs_numcat_keys_have_null(c.h) != 0);
}
PyObject* num_get_values(const Num& c, PyObject* args) {  // numeric_category.cpp:424-453
  const int64_t n = cs_numcat_size(c.h);
  NumBuf out(arg(args, 1), CS_NUM_I32);
  if (!out.none) {
    if (!typed(out, CS_NUM_I32, n, "values") || !num_ok(cs_numcat_get_values(c.h, (int32_t*)out.p, out.on_device, nullptr))) return nullptr;
    return none();
  }
  std::vector<int> v((size_t)(n ? n : 1));
  if (!num_ok(cs_numcat_get_values(c.h, v.data(), 0, nullptr))) return nullptr;
  const bool hn = cs_numcat_keys_have_null(c.h) != 0;
  PyObject* ret = PyList_New((Py_ssize_t)n);
  for (int64_t i = 0; i < n; ++i) PyList_SetItem(ret, (Py_ssize_t)i, hn && v[(size_t)i] == 0 ? none() : PyLong_FromLong(v[(size_t)i]));
  return ret;
}
PyObject* num_indexes_for_key(const Num& c, PyObject* args) {  // (self, key, devptr) -> count
  unsigned char key[8];
  bool is_null = false, absent = false;
  if (!key_of(arg(args, 1), c.code, key, is_null, absent)) return nullptr;
  if (absent) return PyLong_FromLong(0);
  const void* k = is_null ? nullptr : key;
  int64_t count = 0;
  NumBuf out(arg(args, 2), CS_NUM_I32);
  if (out.none) {  // the count alone (one counting pass)
    if (!num_ok(cs_numcat_indexes_for(c.h, k, nullptr, 0, nullptr, &count))) return nullptr;
    return PyLong_FromLongLong(count);
  }
  if (!typed(out, CS_NUM_I32, 0, "indexes_for_key")) return nullptr;
  if (out.n >= 0 && out.n < cs_numcat_size(c.h)) {  // an array that may be too short: count first
    if (!num_ok(cs_numcat_indexes_for(c.h, k, nullptr, 0, nullptr, &count)) || !typed(out, CS_NUM_I32, count, "indexes_for_key")) return nullptr;
  }
  if (!num_ok(cs_numcat_indexes_for(c.h, k, (int32_t*)out.p, out.on_device, nullptr, &count))) return nullptr;
  return PyLong_FromLongLong(count);
}
PyObject* num_to_numbers(const Num& c, PyObject* args) {  // (self, narr, nulls)
  const int64_t n = cs_numcat_size(c.h);
  NumBuf out(arg(args, 1), c.code);
  MaskBuf nulls(arg(args, 2));
  if (!typed(out, c.code, n, "to_numbers") || !nulls.fits(out.on_device, n, "to_numbers")) return nullptr;
  if (!num_ok(cs_numcat_to_type(c.h, out.p, (uint8_t*)nulls.p, out.on_device, nullptr))) return nullptr;
  return none();
}
PyObject* num_gather_numbers(const Num& c, PyObject* args) {  // (self, indexes, narr, nulls)
  NumBuf idx(arg(args, 1), CS_NUM_I32);
  if (!typed(idx, CS_NUM_I32, 0, "gather_numbers")) return nullptr;
  if (idx.n < 0) {
    PyErr_SetString(PyExc_ValueError, "gather_numbers: the indexes need a length");
    return nullptr;
  }
  NumBuf out(arg(args, 2), c.code);
  MaskBuf nulls(arg(args, 3));
  if (!typed(out, c.code, idx.n, "gather_numbers") || !nulls.fits(out.on_device, idx.n, "gather_numbers")) return nullptr;
  if (out.on_device != idx.on_device) {
    PyErr_SetString(PyExc_ValueError, "gather_numbers: the arrays must all be host memory or all device memory");
    return nullptr;
  }
  if (!num_ok(cs_numcat_gather_type(c.h, (const int32_t*)idx.p, idx.n, out.p, (uint8_t*)nulls.p, out.on_device, nullptr))) return nullptr;
  return none();
}
typedef int (*IndexesFn)(const cs_numcat*, const int32_t*, int64_t, int, cs_stream, cs_numcat**);
PyObject* num_by_indexes(const Num& c, PyObject* args, IndexesFn fn, const char* what) {  // (self, indexes, count)
  NumBuf idx(arg(args, 1), CS_NUM_I32);
  if (!typed(idx, CS_NUM_I32, 0, what)) return nullptr;
  const int64_t n = idx.n >= 0 ? idx.n : (int64_t)int_arg(args, 2, 0);
  cs_numcat* out = nullptr;
  if (!num_ok(fn(c.h, (const int32_t*)idx.p, n, idx.on_device, nullptr, &out))) return nullptr;
  return num_instance(out, c.code);
}
typedef int (*KeysFn)(const cs_numcat*, const void*, int64_t, const uint8_t*, int, cs_stream, cs_numcat**);
PyObject* num_by_keys(const Num& c, PyObject* args, KeysFn fn, const char* what) {  // (self, keys, nulls)
  NumBuf keys(arg(args, 1), c.code);
  if (!typed(keys, c.code, 0, what)) return nullptr;
  if (keys.n < 0) {
    PyErr_Format(PyExc_ValueError, "%s: the keys need a dtype and a length", what);
    return nullptr;
  }
  MaskBuf nulls(arg(args, 2));
  if (!nulls.fits(keys.on_device, keys.n, what)) return nullptr;
  cs_numcat* out = nullptr;
  if (!num_ok(fn(c.h, keys.p, keys.n, (const uint8_t*)nulls.p, keys.on_device, nullptr, &out))) return nullptr;
  return num_instance(out, c.code);
}
}  // namespace

static PyObject* n_createCategoryFromNumbers(PyObject*, PyObject* args) {  // (narr, nulls); numeric_category.cpp:190-236
  NumBuf items(arg(args, 0), -1);
  if (bad_dtype(items)) return nullptr;
  if (items.none || items.n < 0) {
    PyErr_SetString(PyExc_ValueError, "invalid dtype in nvcategory dispatcher: an array with a dtype is required");
    return nullptr;
  }
  MaskBuf nulls(arg(args, 1));
  if (!nulls.fits(0, items.n, "from_numbers")) return nullptr;
  if (cs_current_device() < 0 && !num_ok(cs_init(0))) return nullptr;
  cs_numcat* out = nullptr;
  if (!num_ok(cs_numcat_build(items.p, items.n, (const uint8_t*)nulls.p, (cs_numtype)items.code, 0, nullptr, &out))) return nullptr;
  return num_instance(out, items.code);
}
// the numeric path of an entry point both kinds of category share
#define NUMERIC_FIRST(args, CALL)        \
  {                                      \
    Num num_;                            \
    if (num_of(arg(args, 0), num_)) CALL; \
  }
static PyObject* n_to_numbers(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, return num_to_numbers(num_, args));
  PyErr_SetString(PyExc_ValueError, "to_numbers: a category of strings has no numbers");
  return nullptr;
}
static PyObject* n_gather_numbers(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, return num_gather_numbers(num_, args));
  PyErr_SetString(PyExc_ValueError, "gather_numbers: a category of strings has no numbers");
  return nullptr;
}
static PyObject* n_gather_values(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, return num_by_indexes(num_, args, cs_numcat_gather_values, "gather_values"));
  PyErr_SetString(PyExc_ValueError, "gather_values: a category of numbers is required");
  return nullptr;
}

static PyObject* n_destroyCategory(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, {
    if (!PyLong_Check(arg(args, 0))) return refuse_numeric("destroyCategory (the object owns its handle)");
    num_delete(PyLong_AsVoidPtr(arg(args, 0)), num_.code);
    return PyLong_FromLong(0);
  });
  NVCategory* c = SELF(args);
  guarded([&] { NVCategory::destroy(c); });
  return PyLong_FromLong(0);
}
static PyObject* n_size(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, return PyLong_FromLongLong(cs_numcat_size(num_.h)));
  return PyLong_FromLong((long)SELF(args)->size());
}
static PyObject* n_keys_size(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, return PyLong_FromLongLong(cs_numcat_keys_size(num_.h)));
  return PyLong_FromLong((long)SELF(args)->keys_size());
}
static PyObject* n_keys_type(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, return PyUnicode_FromString(kNumNames[num_.code]));
  return PyUnicode_FromString("str");
}
static PyObject* n_get_keys(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, return num_get_keys(num_, args));
  NVCategory* c = SELF(args);
  return make_instance([&] { return c->get_keys(); });
}
static PyObject* n_get_value_for_index(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, return refuse_numeric("get_value_for_index"));
  NVCategory* c = SELF(args);
  const unsigned int i = (unsigned int)int_arg(args, 1, 0);
  int v = -1;
  if (!guarded([&] { v = c->get_value(i); })) return PyErr_Occurred() ? nullptr : none();
  return PyLong_FromLong(v);
}
static PyObject* n_get_value_for_string(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, return refuse_numeric("get_value_for_string"));
  NVCategory* c = SELF(args);
  const char* s = str_arg(args, 1);
  int v = -1;
  if (!guarded([&] { v = c->get_value(s); })) return PyErr_Occurred() ? nullptr : none();
  return PyLong_FromLong(v);
}
static PyObject* n_get_values(PyObject*, PyObject* args) {  // (self, devptr) -> devptr | list
  NUMERIC_FIRST(args, return num_get_values(num_, args));
  NVCategory* c = SELF(args);
  int* devptr = ptr_arg<int>(args, 1);
  if (devptr) {
    if (!guarded([&] { c->get_values(devptr, true); })) return PyErr_Occurred() ? nullptr : none();
    return PyLong_FromVoidPtr(devptr);
  }
  const unsigned int n = c->size();
  std::vector<int> v(n ? n : 1);
  if (n && !guarded([&] { c->get_values(v.data(), false); })) return nullptr;
  PyObject* ret = PyList_New(n);
  for (unsigned int i = 0; i < n; ++i) PyList_SetItem(ret, i, PyLong_FromLong(v[i]));
  return ret;
}
static PyObject* n_get_values_cpointer(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, return from_ptr(cs_numcat_values_ptr(num_.h)));
  return from_ptr(SELF(args)->values_cptr());
}
static PyObject* n_get_indexes_for_key(PyObject*, PyObject* args) {  // (self, key, devptr) -> list of rows
  NUMERIC_FIRST(args, return num_indexes_for_key(num_, args));
  NVCategory* c = SELF(args);
  const char* key = str_arg(args, 1);
  const unsigned int n = c->size();
  std::vector<int> rows(n ? n : 1);
  int found = 0;
  if (!guarded([&] { found = c->get_indexes_for(key, rows.data(), false); })) return PyErr_Occurred() ? nullptr : none();
  if (found < 0) found = 0;
  PyObject* ret = PyList_New(found);
  for (int i = 0; i < found; ++i) PyList_SetItem(ret, i, PyLong_FromLong(rows[(size_t)i]));
  return ret;
}
#define WITH_STRINGS(NAME, CALL)                                                          \
  static PyObject* NAME(PyObject*, PyObject* args) {                                      \
    NUMERIC_FIRST(args, return num_##NAME(num_, args));                                   \
    NVCategory* c = SELF(args);                                                           \
    NVStrings* s = handle_of<NVStrings>(arg(args, 1));                                    \
    if (!s) {                                                                             \
      PyErr_SetString(PyExc_ValueError, "nvcategory: parameter must be nvstrings object"); \
      return nullptr;                                                                     \
    }                                                                                     \
    return make_instance([&] { return c->CALL(*s); });                                    \
  }
static PyObject* num_n_add_strings(const Num&, PyObject*) { return refuse_numeric("add_strings"); }
static PyObject* num_n_remove_strings(const Num&, PyObject*) { return refuse_numeric("remove_strings"); }
static PyObject* num_n_add_keys(const Num& c, PyObject* a) { return num_by_keys(c, a, cs_numcat_add_keys, "add_keys"); }
static PyObject* num_n_remove_keys(const Num& c, PyObject* a) { return num_by_keys(c, a, cs_numcat_remove_keys, "remove_keys"); }
static PyObject* num_n_set_keys(const Num& c, PyObject* a) { return num_by_keys(c, a, cs_numcat_set_keys, "set_keys"); }
WITH_STRINGS(n_add_strings, add_strings)
WITH_STRINGS(n_remove_strings, remove_strings)
WITH_STRINGS(n_add_keys, add_keys_and_remap)
WITH_STRINGS(n_remove_keys, remove_keys_and_remap)
WITH_STRINGS(n_set_keys, set_keys_and_remap)
#define WITH_CATEGORY(NAME, CALL)                                                          \
  static PyObject* NAME(PyObject*, PyObject* args) {                                       \
    NUMERIC_FIRST(args, return num_##NAME(num_, args));                                    \
    {                                                                                      \
      Num other_;                                                                          \
      if (num_of(arg(args, 1), other_)) return refuse_numeric(#NAME);                      \
    }                                                                                      \
    NVCategory* c = SELF(args);                                                            \
    NVCategory* o = handle_of<NVCategory>(arg(args, 1));                                   \
    if (!o) {                                                                              \
      PyErr_SetString(PyExc_ValueError, "nvcategory: parameter must be nvcategory object"); \
      return nullptr;                                                                      \
    }                                                                                      \
    return make_instance([&] { return c->CALL(*o); });                                     \
  }
static PyObject* num_n_merge_category(const Num&, PyObject*) { return refuse_numeric("merge_category"); }
static PyObject* num_n_merge_and_remap(const Num& c, PyObject* args) {  // numeric_category.cpp:847-851: the types must match
  Num o;
  if (!num_of(arg(args, 1), o) || o.code != c.code) {
    PyErr_SetString(PyExc_ValueError, "merge_and_remap: the categories hold different types");
    return nullptr;
  }
  cs_numcat* out = nullptr;
  if (!num_ok(cs_numcat_merge(c.h, o.h, nullptr, &out))) return nullptr;
  return num_instance(out, c.code);
}
WITH_CATEGORY(n_merge_category, merge_category)
WITH_CATEGORY(n_merge_and_remap, merge_and_remap)
static PyObject* n_remove_unused_keys(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, {
    cs_numcat* out = nullptr;
    if (!num_ok(cs_numcat_remove_unused_keys(num_.h, nullptr, &out))) return nullptr;
    return num_instance(out, num_.code);
  });
  NVCategory* c = SELF(args);
  return make_instance([&] { return c->remove_unused_keys_and_remap(); });
}
static PyObject* n_to_strings(PyObject*, PyObject* args) {
  NUMERIC_FIRST(args, return refuse_numeric("to_strings"));
  NVCategory* c = SELF(args);
  return make_instance([&] { return c->to_strings(); });
}
#define WITH_INDEXES(NAME, CALL)                                                                     \
  static PyObject* NAME(PyObject*, PyObject* args) {                                                 \
    NUMERIC_FIRST(args, return num_##NAME(num_, args));                                              \
    NVCategory* c = SELF(args);                                                                      \
    Array<int> a(arg(args, 1));                                                                      \
    const unsigned int count = a.on_device ? (unsigned int)int_arg(args, 2, 0) : (unsigned int)a.count; \
    return make_instance([&] { return c->CALL(a.data, count, a.on_device); });                       \
  }
static PyObject* num_n_gather_strings(const Num&, PyObject*) { return refuse_numeric("gather_strings"); }
static PyObject* num_n_gather(const Num& c, PyObject* a) { return num_by_indexes(c, a, cs_numcat_gather, "gather"); }
static PyObject* num_n_gather_and_remap(const Num& c, PyObject* a) { return num_by_indexes(c, a, cs_numcat_gather_and_remap, "gather_and_remap"); }
WITH_INDEXES(n_gather_strings, gather_strings)
WITH_INDEXES(n_gather, gather)
WITH_INDEXES(n_gather_and_remap, gather_and_remap)

static PyObject* n_dropWrapper(PyObject*, PyObject* args) { return drop_wrapper<NVCategory>(args); }

static PyMethodDef s_Methods[] = {
#define M(n) {#n, n, METH_VARARGS, ""}
    M(n_dropWrapper),
    M(n_createCategoryFromNumbers), M(n_to_numbers), M(n_gather_numbers), M(n_gather_values),
    M(n_createCategoryFromHostStrings), M(n_createCategoryFromNVStrings), M(n_createFromOffsets), M(n_destroyCategory), M(n_size), M(n_keys_size),
    M(n_keys_type), M(n_get_keys), M(n_get_indexes_for_key), M(n_get_value_for_index), M(n_get_value_for_string), M(n_get_values),
    M(n_get_values_cpointer), M(n_add_strings), M(n_remove_strings), M(n_to_strings), M(n_gather_strings), M(n_gather), M(n_gather_and_remap),
    M(n_merge_category), M(n_merge_and_remap), M(n_add_keys), M(n_remove_keys), M(n_remove_unused_keys), M(n_set_keys),
#undef M
    {NULL, NULL, 0, NULL}};
static struct PyModuleDef s_Module = {PyModuleDef_HEAD_INIT, "pyniNVCategory", "CPython glue of nvcategory over the MI355X back-end", -1, s_Methods};
PyMODINIT_FUNC PyInit_pyniNVCategory(void) { return PyModule_Create(&s_Module); }
