// pyniNVText -- CPython glue of the nvtext Python module (python/cpp/pytext.cpp in the reference, method
// table :653-666) for tokenize, n-grams, the token counters, the string matches, edit distance and scatter_count, over
// libNVText.so.  The strings arguments
// are nvstrings Python objects (their m_cptr is read), as in the reference.
#include "nvstrings/NVText.h"
#include "nvstrings/NVStrings.h"
#include "pyni_common.h"

using namespace pyni;

static NVStrings* strs_arg(PyObject* args, int i) {
  NVStrings* s = handle_of<NVStrings>(arg(args, i));
  if (!s) PyErr_SetString(PyExc_ValueError, "nvtext: parameter must be nvstrings object");
  return s;
}
static PyObject* n_tokenize(PyObject*, PyObject* args) {
  NVStrings* s = strs_arg(args, 0);
  if (!s) return nullptr;
  const char* d = str_arg(args, 1);
  return make_instance([&] { return NVText::tokenize(*s, d); });
}
static PyObject* n_tokenize_multi(PyObject*, PyObject* args) {  // (strs, delimiters: nvstrings object)
  NVStrings *s = strs_arg(args, 0), *d = s ? strs_arg(args, 1) : nullptr;
  if (!s || !d) return nullptr;
  return make_instance([&] { return NVText::tokenize(*s, *d); });
}
static PyObject* n_unique_tokens(PyObject*, PyObject* args) {
  NVStrings* s = strs_arg(args, 0);
  if (!s) return nullptr;
  const char* d = str_arg(args, 1);
  return make_instance([&] { return NVText::unique_tokens(*s, d); });
}
static PyObject* n_token_count(PyObject*, PyObject* args) {  // (strs, delimiter, devptr)
  NVStrings* s = strs_arg(args, 0);
  if (!s) return nullptr;
  const char* d = str_arg(args, 1);
  return int_results<unsigned int>(s, ptr_arg<unsigned int>(args, 2), 0, [&](unsigned int* out, bool dev) { NVText::token_count(*s, d, out, dev); });
}
static PyObject* n_tokens_counts(PyObject*, PyObject* args) {  // (strs, tgts, delimiter, devptr) -> list of rows
  NVStrings *s = strs_arg(args, 0), *t = s ? strs_arg(args, 1) : nullptr;
  if (!s || !t) return nullptr;
  const char* d = str_arg(args, 2);
  unsigned int* devptr = ptr_arg<unsigned int>(args, 3);
  if (devptr) {
    if (!guarded([&] { NVText::tokens_counts(*s, *t, d, devptr, true); })) return PyErr_Occurred() ? nullptr : none();
    return PyLong_FromVoidPtr(devptr);
  }
  const unsigned int rows = s->size(), tc = t->size();
  std::vector<unsigned int> host((size_t)rows * tc + 1);
  if (!guarded([&] { NVText::tokens_counts(*s, *t, d, host.data(), false); })) return PyErr_Occurred() ? nullptr : none();
  PyObject* ret = PyList_New(rows);
  for (unsigned int r = 0; r < rows; ++r) {
    PyObject* row = PyList_New(tc);
    for (unsigned int k = 0; k < tc; ++k) PyList_SetItem(row, k, PyLong_FromLong((long)host[(size_t)r * tc + k]));
    PyList_SetItem(ret, r, row);
  }
  return ret;
}
static PyObject* n_replace_tokens(PyObject*, PyObject* args) {  // (strs, tgts, repls, delimiter)
  NVStrings *s = strs_arg(args, 0), *t = s ? strs_arg(args, 1) : nullptr, *r = t ? strs_arg(args, 2) : nullptr;
  if (!s || !t || !r) return nullptr;
  const char* d = str_arg(args, 3);
  return make_instance([&] { return NVText::replace_tokens(*s, *t, *r, d); });
}
static PyObject* n_normalize_spaces(PyObject*, PyObject* args) {
  NVStrings* s = strs_arg(args, 0);
  if (!s) return nullptr;
  return make_instance([&] { return NVText::normalize_spaces(*s); });
}
static PyObject* n_create_ngrams(PyObject*, PyObject* args) {  // (strs, N, sep)
  NVStrings* s = strs_arg(args, 0);
  if (!s) return nullptr;
  const unsigned int n = (unsigned int)int_arg(args, 1, 2);
  const char* sep = str_arg(args, 2);
  return make_instance([&] { return NVText::create_ngrams(*s, n, sep ? sep : "_"); });
}

// a `tgts` argument: an nvstrings object (borrowed) or a list of str / None (an instance made here and destroyed with this)
struct Targets {
  NVStrings* p = nullptr;
  bool own = false;
  explicit Targets(PyObject* o) {
    if (PyList_Check(o)) {
      std::vector<const char*> rows;
      list_strings(o, rows);
      guarded([&] { p = NVStrings::create_from_array(rows.data(), (unsigned int)rows.size()); });
      own = p != nullptr;
    } else if (o != Py_None && !PyUnicode_Check(o)) {
      p = handle_of<NVStrings>(o);
    }
  }
  ~Targets() {
    if (own) guarded([&] { NVStrings::destroy(p); });
  }
};
// pytext.cpp:172-345 -- (strs, tgts: list or nvstrings, devptr) -> a list of `columns` values per row, or the device pointer
template <class T, class Call, class Item>
static PyObject* match_results(PyObject* args, Call&& call, Item&& item) {
  NVStrings* s = strs_arg(args, 0);
  if (!s) return nullptr;
  if (arg(args, 1) == Py_None) {
    PyErr_SetString(PyExc_ValueError, "tgts argument must be specified");
    return nullptr;
  }
  Targets t(arg(args, 1));
  if (PyErr_Occurred()) return nullptr;
  if (!t.p) {
    PyErr_SetString(PyExc_ValueError, "invalid tgts parameter");
    return nullptr;
  }
  if (t.p->size() == 0) {
    PyErr_SetString(PyExc_ValueError, "tgts argument is empty");
    return nullptr;
  }
  if (T* devptr = ptr_arg<T>(args, 2)) {
    if (!guarded([&] { call(*s, *t.p, devptr, true); })) return nullptr;
    return PyLong_FromVoidPtr(devptr);
  }
  const size_t rows = s->size(), columns = t.p->size();
  PyObject* ret = PyList_New((Py_ssize_t)rows);
  if (rows == 0) return ret;
  std::vector<unsigned char> host(rows * columns * sizeof(T));
  if (!guarded([&] { call(*s, *t.p, reinterpret_cast<T*>(host.data()), false); })) {
    Py_DECREF(ret);
    return nullptr;
  }
  const T* v = reinterpret_cast<const T*>(host.data());
  for (size_t r = 0; r < rows; ++r) {
    PyObject* row = PyList_New((Py_ssize_t)columns);
    for (size_t k = 0; k < columns; ++k) PyList_SetItem(row, (Py_ssize_t)k, item(v[r * columns + k]));
    PyList_SetItem(ret, (Py_ssize_t)r, row);
  }
  return ret;
}
static PyObject* n_contains_strings(PyObject*, PyObject* args) {
  return match_results<bool>(
      args, [](NVStrings& s, NVStrings& t, bool* out, bool dev) { NVText::contains_strings(s, t, out, dev); },
      [](bool v) { return PyBool_FromLong(v); });
}
static PyObject* n_strings_counts(PyObject*, PyObject* args) {
  return match_results<unsigned int>(
      args, [](NVStrings& s, NVStrings& t, unsigned int* out, bool dev) { NVText::strings_counts(s, t, out, dev); },
      [](unsigned int v) { return PyLong_FromLong((long)v); });
}
static PyObject* n_edit_distance(PyObject*, PyObject* args) {  // pytext.cpp:495-589 -- (strs, tgt: str / list / nvstrings, algo, devptr)
  NVStrings* s = strs_arg(args, 0);
  if (!s) return nullptr;
  PyObject* tgt = arg(args, 1);
  if (tgt == Py_None) {
    PyErr_SetString(PyExc_ValueError, "tgt argument must be specified");
    return nullptr;
  }
  if (int_arg(args, 2, (long)NVText::levenshtein) != (long)NVText::levenshtein) {
    PyErr_SetString(PyExc_ValueError, "unrecognized edit-distance algorithm");
    return nullptr;
  }
  unsigned int* devptr = ptr_arg<unsigned int>(args, 3);
  if (PyUnicode_Check(tgt)) {
    const char* str = PyUnicode_AsUTF8(tgt);
    if (!str) return nullptr;
    return int_results<unsigned int>(s, devptr, 0, [&](unsigned int* out, bool dev) { NVText::edit_distance(NVText::levenshtein, *s, str, out, dev); });
  }
  Targets t(tgt);
  if (PyErr_Occurred()) return nullptr;
  if (!t.p) {
    PyErr_SetString(PyExc_ValueError, "invalid tgt parameter");
    return nullptr;
  }
  if (t.p->size() != s->size()) {
    PyErr_SetString(PyExc_ValueError, "strs and tgt must have the same number of strings");
    return nullptr;
  }
  return int_results<unsigned int>(s, devptr, 0, [&](unsigned int* out, bool dev) { NVText::edit_distance(NVText::levenshtein, *s, *t.p, out, dev); });
}
static PyObject* n_scatter_count(PyObject*, PyObject* args) {  // pytext.cpp:616-650 -- (strs, counts: list (None = 0) or device pointer)
  NVStrings* s = strs_arg(args, 0);
  if (!s) return nullptr;
  Array<unsigned int> counts(arg(args, 1));
  if (counts.bad || !counts.data) {
    PyErr_SetString(PyExc_ValueError, "counts must be a list or a device pointer");
    return nullptr;
  }
  if (!counts.on_device && counts.count != s->size()) {
    PyErr_SetString(PyExc_ValueError, "counts must have one entry per string");
    return nullptr;
  }
  return make_instance([&] { return NVText::scatter_count(*s, counts.data, counts.on_device); });
}

static PyMethodDef s_Methods[] = {
#define M(n) {#n, n, METH_VARARGS, ""}
    M(n_tokenize), M(n_tokenize_multi), M(n_unique_tokens), M(n_token_count), M(n_tokens_counts), M(n_replace_tokens), M(n_normalize_spaces), M(n_create_ngrams),
    M(n_contains_strings), M(n_strings_counts), M(n_edit_distance), M(n_scatter_count),
#undef M
    {NULL, NULL, 0, NULL}};
static struct PyModuleDef s_Module = {PyModuleDef_HEAD_INIT, "pyniNVText", "CPython glue of nvtext over the MI355X back-end", -1, s_Methods};
PyMODINIT_FUNC PyInit_pyniNVText(void) { return PyModule_Create(&s_Module); }
