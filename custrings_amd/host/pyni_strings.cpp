// pyniNVStrings -- CPython glue of the nvstrings Python class (python/cpp/pystrings.cpp in the reference,
// method table :3860-3973) for the members SURVEY.md section 8 names, over libNVStrings.so.
#include "pyni_common.h"
#include "nvstrings/StringsStatistics.h"
#include "nvstrings/ipc_transfer.h"
#include <cstring>
#include <memory>
#include <type_traits>

using namespace pyni;

#define SELF(args) ptr_arg<NVStrings>(args, 0)

// ---- construction / export ----------------------------------------------------------------------------
static PyObject* n_createFromHostStrings(PyObject*, PyObject* args) {  // pystrings.cpp:212-250
  PyObject* strs = arg(args, 0);
  std::vector<const char*> list;
  if (PyUnicode_Check(strs)) list.push_back(PyUnicode_AsUTF8(strs));
  else if (PyList_Check(strs)) list_strings(strs, list);
  else {
    PyErr_SetString(PyExc_ValueError, "nvstrings: a list of str is required");
    return nullptr;
  }
  return make_instance([&] { return NVStrings::create_from_array(list.data(), (unsigned int)list.size()); });
}
static PyObject* n_destroyStrings(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  guarded([&] { NVStrings::destroy(s); });
  return PyLong_FromLong(0);
}
static PyObject* n_createHostStrings(PyObject*, PyObject* args) { return host_strings(SELF(args)); }
static PyObject* n_createFromOffsets(PyObject*, PyObject* args) {  // (sbuf, obuf, scount, nbuf, ncount, bdevmem)
  if (arg(args, 0) == Py_None || arg(args, 1) == Py_None) {
    PyErr_SetString(PyExc_ValueError, "nvstrings: missing parameter");
    return nullptr;
  }
  Region chars(arg(args, 0)), offs(arg(args, 1)), nulls(arg(args, 3));
  const int count = (int)int_arg(args, 2, 0), ncount = (int)int_arg(args, 4, 0);
  const bool dev = bool_arg(args, 5);
  return make_instance([&] {
    return NVStrings::create_from_offsets((const char*)chars.p, count, (const int*)offs.p, (const unsigned char*)nulls.p, ncount, dev);
  });
}
static PyObject* n_createFromCSV(PyObject*, PyObject* args) {  // pystrings.cpp:359-374: (csv, column, lines, flags) -> instance or None
  const char* path = str_arg(args, 0);
  if (!path) {
    PyErr_SetString(PyExc_ValueError, "nvstrings: missing parameter");
    return nullptr;
  }
  const std::string csv = path;
  const unsigned int column = (unsigned int)int_arg(args, 1, 0), lines = (unsigned int)int_arg(args, 2, 0), flags = (unsigned int)int_arg(args, 3, 0);
  return make_instance([&] { return NVStrings::create_from_csv(csv.c_str(), column, lines, (NVStrings::sorttype)(flags & 3), (flags & 8) != 0); });
}
static PyObject* n_create_offsets(PyObject*, PyObject* args) {  // (self, sbuf, obuf, nbuf, bdevmem)
  NVStrings* s = SELF(args);
  if (arg(args, 1) == Py_None || arg(args, 2) == Py_None) {
    PyErr_SetString(PyExc_ValueError, "nvstrings: missing parameter");
    return nullptr;
  }
  Region chars(arg(args, 1)), offs(arg(args, 2)), nulls(arg(args, 3));
  const bool dev = bool_arg(args, 4);
  if (!guarded([&] { s->create_offsets((char*)chars.p, (int*)offs.p, (unsigned char*)nulls.p, dev); })) return nullptr;
  return none();
}
static PyObject* n_createFromNVStrings(PyObject*, PyObject* args) {  // one instance or a list of them -> their rows in order
  PyObject* o = arg(args, 0);
  std::vector<NVStrings*> all;
  if (PyList_Check(o))
    for (Py_ssize_t i = 0; i < PyList_Size(o); ++i) all.push_back(handle_of<NVStrings>(PyList_GetItem(o, i)));
  else all.push_back(handle_of<NVStrings>(o));
  for (auto* p : all)
    if (!p) {
      PyErr_SetString(PyExc_ValueError, "nvstrings: argument list must contain nvstrings objects");
      return nullptr;
    }
  return make_instance([&] { return NVStrings::create_from_strings(all); });
}
static PyObject* n_getIPCData(PyObject*, PyObject* args) {  // pystrings.cpp: n_getIPCData -- here the transfer record as bytes
  NVStrings* s = SELF(args);
  nvstrings_ipc_transfer rec;
  if (!guarded([&] { s->create_ipc_transfer(rec); })) return nullptr;
  return PyBytes_FromStringAndSize(reinterpret_cast<const char*>(&rec), (Py_ssize_t)sizeof(rec));
}
static PyObject* n_createFromIPC(PyObject*, PyObject* args) {  // pystrings.cpp: n_createFromIPC
  PyObject* o = arg(args, 0);
  char* data = nullptr;
  Py_ssize_t len = 0;
  if (!PyBytes_Check(o) || PyBytes_AsStringAndSize(o, &data, &len) != 0 || len != (Py_ssize_t)sizeof(nvstrings_ipc_transfer)) {
    PyErr_SetString(PyExc_ValueError, "nvstrings: the bytes of get_ipc_data() are required");
    return nullptr;
  }
  nvstrings_ipc_transfer rec;
  memcpy(&rec, data, sizeof(rec));
  return make_instance([&] { return NVStrings::create_from_ipc(rec); });
}
static PyObject* n_size(PyObject*, PyObject* args) { return PyLong_FromLong((long)SELF(args)->size()); }
static PyObject* n_len(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  return int_results<int>(s, ptr_arg<int>(args, 1), 0, [&](int* out, bool dev) { s->len(out, dev); });
}
static PyObject* n_byte_count(PyObject*, PyObject* args) {  // (self, memptr, bdevmem) -> total bytes
  NVStrings* s = SELF(args);
  int* mem = ptr_arg<int>(args, 1);
  const bool dev = bool_arg(args, 2);
  size_t total = 0;
  if (!guarded([&] { total = s->byte_count(mem, dev); })) return PyErr_Occurred() ? nullptr : none();
  return PyLong_FromLong((long)total);
}
static PyObject* n_null_count(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const bool empty_is_null = bool_arg(args, 1);
  unsigned int n = 0;
  std::vector<unsigned char> bits(((size_t)s->size() + 7) / 8 + 1);
  if (!guarded([&] { n = s->set_null_bitarray(bits.data(), empty_is_null, false); })) return PyErr_Occurred() ? nullptr : none();
  return PyLong_FromLong((long)n);
}
static PyObject* n_set_null_bitmask(PyObject*, PyObject* args) {  // (self, nbuf, bdevmem) -> null count
  NVStrings* s = SELF(args);
  Region nulls(arg(args, 1));
  const bool dev = bool_arg(args, 2);
  unsigned int n = 0;
  if (!guarded([&] { n = s->set_null_bitarray((unsigned char*)nulls.p, false, dev); })) return PyErr_Occurred() ? nullptr : none();
  return PyLong_FromLong((long)n);
}
static PyObject* n_copy(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  return make_instance([&] { return s->copy(); });
}

// ---- split family ---------------------------------------------------------------------------------------------
template <class F>
static PyObject* columns_of(F&& f) {
  std::vector<NVStrings*> results;
  if (!guarded([&] { f(results); })) return PyErr_Occurred() ? nullptr : none();
  return instance_list(results);
}
static PyObject* n_split(PyObject*, PyObject* args) {  // pystrings.cpp:1619-1642: (self, delimiter|None, n|None)
  NVStrings* s = SELF(args);
  const char* d = str_arg(args, 1);
  const int n = (int)int_arg(args, 2, -1);
  return columns_of([&](std::vector<NVStrings*>& r) { s->split(d, n, r); });
}
static PyObject* n_rsplit(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* d = str_arg(args, 1);
  const int n = (int)int_arg(args, 2, -1);
  return columns_of([&](std::vector<NVStrings*>& r) { s->rsplit(d, n, r); });
}
static PyObject* n_split_record(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* d = str_arg(args, 1);
  const int n = (int)int_arg(args, 2, -1);
  return columns_of([&](std::vector<NVStrings*>& r) { s->split_record(d, n, r); });
}
static PyObject* n_rsplit_record(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* d = str_arg(args, 1);
  const int n = (int)int_arg(args, 2, -1);
  return columns_of([&](std::vector<NVStrings*>& r) { s->rsplit_record(d, n, r); });
}
static PyObject* n_partition(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* d = str_arg(args, 1);
  return columns_of([&](std::vector<NVStrings*>& r) { s->partition(d, r); });
}
static PyObject* n_rpartition(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* d = str_arg(args, 1);
  return columns_of([&](std::vector<NVStrings*>& r) { s->rpartition(d, r); });
}

// ---- replace / strip / case -------------------------------------------------------------------------------------
static PyObject* n_replace(PyObject*, PyObject* args) {  // pystrings.cpp:1902-1931: "Oszip"
  PyObject* vo = nullptr;
  const char *pat = nullptr, *repl = nullptr;
  int maxrepl = -1, regex = 1;
  if (!PyArg_ParseTuple(args, "Oszip", &vo, &pat, &repl, &maxrepl, &regex)) {
    PyErr_Clear();
    PyErr_SetString(PyExc_ValueError, "nvstrings.replace: invalid parameters");
    return nullptr;
  }
  NVStrings* s = reinterpret_cast<NVStrings*>(PyLong_AsVoidPtr(vo));
  return make_instance([&] { return regex ? s->replace_re(pat, repl, maxrepl) : s->replace(pat, repl, maxrepl); });
}
static std::string quote_literal(const char* t) {  // a literal as a pattern of the regex dialect (regcomp.cpp:314-539)
  std::string out;
  for (; *t; ++t) {
    if (strchr("\\^$.|?*+()[]{}", *t)) out.push_back('\\');
    out.push_back(*t);
  }
  return out;
}
static PyObject* n_replace_multi(PyObject*, PyObject* args) {  // (self, pats: list of str | nvstrings, repls ptr, regex)
  NVStrings* s = SELF(args);
  PyObject* pats = arg(args, 1);
  NVStrings* repls = handle_of<NVStrings>(arg(args, 2));
  const bool regex = bool_arg(args, 3);
  std::vector<std::string> owned;
  std::vector<const char*> list;
  if (PyList_Check(pats)) {
    list_strings(pats, list);
  } else if (NVStrings* p = handle_of<NVStrings>(pats)) {  // literal targets held on the device
    PyObject* host = host_strings(p);
    if (host == Py_None) return host;
    list_strings(host, list);
    for (auto& q : list) owned.push_back(q ? q : "");
    Py_DECREF(host);
    for (size_t i = 0; i < list.size(); ++i) list[i] = list[i] ? owned[i].c_str() : nullptr;
  } else {
    PyErr_SetString(PyExc_ValueError, "nvstrings.replace_multi: pats must be list of str");
    return nullptr;
  }
  std::vector<std::string> quoted;
  if (!regex) {
    quoted.reserve(list.size());
    for (auto& q : list) {
      quoted.push_back(q ? quote_literal(q) : std::string());
      if (q) q = quoted.back().c_str();
    }
  }
  return make_instance([&] { return s->replace_re(list, *repls); });
}
static PyObject* n_replace_with_backrefs(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char *pat = str_arg(args, 1), *repl = str_arg(args, 2);
  return make_instance([&] { return s->replace_with_backrefs(pat, repl); });
}
#define STRIP_FN(NAME, CALL)                                  \
  static PyObject* NAME(PyObject*, PyObject* args) {          \
    NVStrings* s = SELF(args);                                \
    const char* t = str_arg(args, 1);                         \
    return make_instance([&] { return s->CALL(t); });         \
  }
STRIP_FN(n_lstrip, lstrip)
STRIP_FN(n_strip, strip)
STRIP_FN(n_rstrip, rstrip)
static PyObject* n_lower(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  return make_instance([&] { return s->lower(); });
}
static PyObject* n_upper(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  return make_instance([&] { return s->upper(); });
}

// ---- search -----------------------------------------------------------------------------------------------------------
static PyObject* n_find(PyObject*, PyObject* args) {  // (self, str, start, end|None, devptr): values < -1 -> None
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  const int start = (int)int_arg(args, 2, 0), end = (int)int_arg(args, 3, -1);
  return int_results<int>(s, ptr_arg<int>(args, 4), -1, [&](int* out, bool dev) { s->find(str, start, end, out, dev); });
}
// the rest of the find family (pystrings.cpp:1005-1044, 2234-2360, 2738-2916)
static PyObject* n_compare(PyObject*, PyObject* args) {  // (self, str, devptr): None for null rows in the host list
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  int* devptr = ptr_arg<int>(args, 2);
  if (devptr) return int_results<int>(s, devptr, 0, [&](int* out, bool dev) { s->compare(str, out, dev); });
  const unsigned int count = s->size();
  if (count == 0) return PyList_New(0);
  std::vector<int> host(count);
  std::vector<unsigned char> nulls((count + 7) / 8, 0);
  unsigned int ncount = 0;
  if (!guarded([&] {
        s->compare(str, host.data(), false);
        ncount = s->set_null_bitarray(nulls.data(), false, false);
      }))
    return nullptr;
  PyObject* ret = PyList_New(count);
  for (unsigned int i = 0; i < count; ++i) {
    if (ncount && !((nulls[i / 8] >> (i % 8)) & 1)) {
      Py_INCREF(Py_None);
      PyList_SetItem(ret, i, Py_None);
    } else {
      PyList_SetItem(ret, i, PyLong_FromLong((long)host[i]));
    }
  }
  return ret;
}
static PyObject* n_rfind(PyObject*, PyObject* args) {  // (self, str, start, end|None, devptr)
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  const int start = (int)int_arg(args, 2, 0), end = (int)int_arg(args, 3, -1);
  return int_results<int>(s, ptr_arg<int>(args, 4), -1, [&](int* out, bool dev) { s->rfind(str, start, end, out, dev); });
}
static PyObject* n_find_from(PyObject*, PyObject* args) {  // (self, str, starts devptr, ends devptr, devptr)
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  int *starts = ptr_arg<int>(args, 2), *ends = ptr_arg<int>(args, 3);
  return int_results<int>(s, ptr_arg<int>(args, 4), -1, [&](int* out, bool dev) { s->find_from(str, starts, ends, out, dev); });
}
static PyObject* n_startswith(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  return bool_results(s, ptr_arg<bool>(args, 2), [&](bool* out, bool dev) { return (int)s->startswith(str, out, dev); });
}
static PyObject* n_endswith(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  return bool_results(s, ptr_arg<bool>(args, 2), [&](bool* out, bool dev) { return (int)s->endswith(str, out, dev); });
}
// the other column: an nvstrings object or a list of str / None
struct OtherStrings {
  NVStrings* p = nullptr;
  bool own = false;
  OtherStrings(PyObject* o, const char* what) {
    if (o == Py_None) {
      PyErr_Format(PyExc_ValueError, "nvstrings.%s: parameter required", what);
    } else if (PyList_Check(o)) {
      if (PyList_Size(o) == 0) {
        PyErr_Format(PyExc_ValueError, "nvstrings.%s empty argument list", what);
        return;
      }
      std::vector<const char*> list;
      list_strings(o, list);
      guarded([&] { p = NVStrings::create_from_array(list.data(), (unsigned int)list.size()); });
      own = p != nullptr;
    } else {
      p = handle_of<NVStrings>(o);
      if (!p) PyErr_Format(PyExc_ValueError, "nvstrings.%s: argument must be nvstrings object", what);
    }
  }
  ~OtherStrings() {
    if (own) guarded([&] { NVStrings::destroy(p); });
  }
};
static PyObject* n_match_strings(PyObject*, PyObject* args) {  // (self, strs, devptr): plain bools (two nulls are equal)
  NVStrings* s = SELF(args);
  OtherStrings other(arg(args, 1), "match_strings");
  if (!other.p) return nullptr;
  if (other.p->size() != s->size()) {
    PyErr_SetString(PyExc_ValueError, "nvstrings.match_strings list size must match");
    return nullptr;
  }
  bool* devptr = ptr_arg<bool>(args, 2);
  if (devptr) {
    if (!guarded([&] { s->match_strings(*other.p, devptr, true); })) return nullptr;
    return PyLong_FromVoidPtr(devptr);
  }
  const unsigned int count = s->size();
  if (count == 0) return PyList_New(0);
  std::vector<unsigned char> host(count);
  if (!guarded([&] { s->match_strings(*other.p, reinterpret_cast<bool*>(host.data()), false); })) return nullptr;
  PyObject* ret = PyList_New(count);
  for (unsigned int i = 0; i < count; ++i) PyList_SetItem(ret, i, PyBool_FromLong(host[i]));
  return ret;
}
static PyObject* n_find_multiple(PyObject*, PyObject* args) {  // (self, strs, devptr): a list of positions per row
  NVStrings* s = SELF(args);
  OtherStrings other(arg(args, 1), "find_multiple");
  if (!other.p) return nullptr;
  int* devptr = ptr_arg<int>(args, 2);
  if (devptr) {
    if (!guarded([&] { s->find_multiple(*other.p, devptr, true); })) return nullptr;
    return PyLong_FromVoidPtr(devptr);
  }
  const unsigned int rows = s->size(), tc = other.p->size();
  PyObject* ret = PyList_New(rows);
  if (rows == 0) return ret;
  std::vector<int> host((size_t)rows * tc);
  if (!guarded([&] { s->find_multiple(*other.p, host.data(), false); })) {
    Py_DECREF(ret);
    return nullptr;
  }
  for (unsigned int r = 0; r < rows; ++r) {
    PyObject* row = PyList_New(tc);
    for (unsigned int j = 0; j < tc; ++j) {
      const int v = host[(size_t)r * tc + j];
      if (v < -1) {
        Py_INCREF(Py_None);
        PyList_SetItem(row, j, Py_None);
      } else {
        PyList_SetItem(row, j, PyLong_FromLong((long)v));
      }
    }
    PyList_SetItem(ret, r, row);
  }
  return ret;
}
static PyObject* n_contains(PyObject*, PyObject* args) {  // pystrings.cpp:2588-2666: (self, str, regex, devptr)
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  const bool regex = bool_arg(args, 2);
  return bool_results(s, ptr_arg<bool>(args, 3), [&](bool* out, bool dev) { return regex ? s->contains_re(str, out, dev) : s->contains(str, out, dev); });
}
static PyObject* n_match(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  return bool_results(s, ptr_arg<bool>(args, 2), [&](bool* out, bool dev) { return s->match(str, out, dev); });
}
static PyObject* n_count(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  int* devptr = ptr_arg<int>(args, 2);
  if (devptr) return int_results<int>(s, devptr, 0, [&](int* out, bool dev) { s->count_re(str, out, dev); });
  // host list: None for null rows (pystrings.cpp:2949-2968)
  const unsigned int count = s->size();
  if (count == 0) return PyList_New(0);
  std::vector<int> host(count);
  std::vector<unsigned char> nulls((count + 7) / 8, 0);
  unsigned int ncount = 0;
  if (!guarded([&] {
        s->count_re(str, host.data(), false);
        ncount = s->set_null_bitarray(nulls.data(), false, false);
      }))
    return nullptr;
  PyObject* ret = PyList_New(count);
  for (unsigned int i = 0; i < count; ++i) {
    if (ncount && !((nulls[i / 8] >> (i % 8)) & 1)) {
      Py_INCREF(Py_None);
      PyList_SetItem(ret, i, Py_None);
    } else {
      PyList_SetItem(ret, i, PyLong_FromLong(host[i]));
    }
  }
  return ret;
}
#define PATTERN_COLUMNS(NAME, CALL)                                                   \
  static PyObject* NAME(PyObject*, PyObject* args) {                                  \
    NVStrings* s = SELF(args);                                                        \
    const char* pat = str_arg(args, 1);                                               \
    return columns_of([&](std::vector<NVStrings*>& r) { s->CALL(pat, r); });          \
  }
PATTERN_COLUMNS(n_findall, findall)
PATTERN_COLUMNS(n_findall_record, findall_record)
PATTERN_COLUMNS(n_extract, extract)
PATTERN_COLUMNS(n_extract_record, extract_record)

// ---- re-arrangement / combine ---------------------------------------------------------------------------------------------
static PyObject* n_sort(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const NVStrings::sorttype st = (NVStrings::sorttype)int_arg(args, 1, 2);
  const bool asc = bool_arg(args, 2), nf = bool_arg(args, 3);
  return make_instance([&] { return s->sort(st, asc, nf); });
}
static PyObject* n_order(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const NVStrings::sorttype st = (NVStrings::sorttype)int_arg(args, 1, 2);
  const bool asc = bool_arg(args, 2), nf = bool_arg(args, 3);
  return int_results<unsigned int>(s, ptr_arg<unsigned int>(args, 4), 0, [&](unsigned int* out, bool dev) { s->order(st, asc, out, nf, dev); });
}
static PyObject* n_gather(PyObject*, PyObject* args) {  // (self, indexes: list of int | list of bool | address, count)
  NVStrings* s = SELF(args);
  PyObject* idx = arg(args, 1);
  if (PyList_Check(idx) && PyList_Size(idx) > 0 && PyBool_Check(PyList_GetItem(idx, 0))) {
    Array<unsigned char> mask(idx);
    if (mask.count != s->size()) {
      PyErr_SetString(PyExc_ValueError, "nvstrings.gather: the mask must have one entry per string");
      return nullptr;
    }
    return make_instance([&] { return s->gather(reinterpret_cast<const bool*>(mask.data), false); });
  }
  Array<int> a(idx);
  if (a.bad) {
    PyErr_SetString(PyExc_ValueError, "nvstrings.gather: unknown type of indexes");
    return nullptr;
  }
  if (a.all_bool && !a.on_device) {  // (a numpy bool array: the mask form, as a list of bool)
    if (a.count != s->size()) {
      PyErr_SetString(PyExc_ValueError, "nvstrings.gather: the mask must have one entry per string");
      return nullptr;
    }
    std::vector<unsigned char> m(a.count);
    for (size_t i = 0; i < a.count; ++i) m[i] = a.data[i] != 0;
    return make_instance([&] { return s->gather(reinterpret_cast<const bool*>(m.data()), false); });
  }
  const unsigned int count = a.on_device ? (unsigned int)int_arg(args, 2, 0) : (unsigned int)a.count;
  return make_instance([&] { return s->gather(a.data, count, a.on_device); });
}
static PyObject* n_sublist(PyObject*, PyObject* args) {  // (self, start|None, end|None, step|None)
  NVStrings* s = SELF(args);
  const unsigned int start = (unsigned int)int_arg(args, 1, 0), end = (unsigned int)int_arg(args, 2, (long)s->size());
  const int step = (int)int_arg(args, 3, 1);
  return make_instance([&] { return s->sublist(start, end, step); });
}
static PyObject* n_scatter(PyObject*, PyObject* args) {  // (self, nvstrings object, indexes)
  NVStrings* s = SELF(args);
  NVStrings* strs = handle_of<NVStrings>(arg(args, 1));
  if (!strs) {
    PyErr_SetString(PyExc_ValueError, "nvstrings.scatter: parameter must be nvstrings object");
    return nullptr;
  }
  Array<int> a(arg(args, 2));
  if (!a.on_device && a.count < strs->size()) {
    PyErr_SetString(PyExc_ValueError, "nvstrings.scatter: number of indexes must match the number of strings");
    return nullptr;
  }
  return make_instance([&] { return s->scatter(*strs, a.data, a.on_device); });
}
static PyObject* n_scalar_scatter(PyObject*, PyObject* args) {  // (self, str, indexes, count)
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  Array<int> a(arg(args, 2));
  const unsigned int count = a.on_device ? (unsigned int)int_arg(args, 3, 0) : (unsigned int)a.count;
  return make_instance([&] { return s->scatter(str, a.data, count, a.on_device); });
}
static PyObject* n_remove_strings(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  Array<int> a(arg(args, 1));
  const unsigned int count = a.on_device ? (unsigned int)int_arg(args, 2, 0) : (unsigned int)a.count;
  return make_instance([&] { return s->remove_strings(a.data, count, a.on_device); });
}
static PyObject* n_add_strings(PyObject*, PyObject* args) {  // (self, nvstrings | list of nvstrings)
  std::vector<NVStrings*> all{SELF(args)};
  PyObject* o = arg(args, 1);
  if (PyList_Check(o))
    for (Py_ssize_t i = 0; i < PyList_Size(o); ++i) all.push_back(handle_of<NVStrings>(PyList_GetItem(o, i)));
  else all.push_back(handle_of<NVStrings>(o));
  for (auto* p : all)
    if (!p) {
      PyErr_SetString(PyExc_ValueError, "nvstrings.add_strings: argument must be nvstrings object(s)");
      return nullptr;
    }
  return make_instance([&] { return NVStrings::create_from_strings(all); });
}
static PyObject* n_cat(PyObject*, PyObject* args) {  // (self, others: None | nvstrings | list of nvstrings, sep|None, na_rep|None)
  NVStrings* s = SELF(args);
  PyObject* others = arg(args, 1);
  const char *sep = str_arg(args, 2), *narep = str_arg(args, 3);
  if (others == Py_None)  // no others: all rows joined into one string (pystrings.cpp:1454-1473)
    return make_instance([&] { return s->join(sep ? sep : "", narep); });
  if (PyList_Check(others)) {
    std::vector<NVStrings*> list;
    for (Py_ssize_t i = 0; i < PyList_Size(others); ++i) list.push_back(handle_of<NVStrings>(PyList_GetItem(others, i)));
    return make_instance([&] { return s->cat(list, sep, narep); });
  }
  NVStrings* one = handle_of<NVStrings>(others);
  return make_instance([&] { return s->cat(one, sep, narep); });
}
static PyObject* n_join(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* sep = str_arg(args, 1);
  return make_instance([&] { return s->join(sep ? sep : ""); });
}
static PyObject* n_device_memory(PyObject*, PyObject* args) { return PyLong_FromLong((long)SELF(args)->memsize()); }
// pystrings.cpp:3780-3832: (self) -> the dict of NVStrings::compute_statistics; chars_histogram maps a one-character str to its
// count (a pair whose bytes are no valid UTF-8 -- a lone surrogate -- has no str and is left out; the C++ vector keeps it)
static PyObject* n_get_info(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  StringsStatistics st;
  if (!guarded([&] { s->compute_statistics(st); })) return nullptr;
  PyObject* d = PyDict_New();
  auto put = [&](const char* key, size_t v) {
    PyObject* o = PyLong_FromUnsignedLongLong((unsigned long long)v);
    PyDict_SetItemString(d, key, o);
    Py_DECREF(o);
  };
  put("total_strings", st.total_strings);
  put("null_strings", st.total_nulls);
  put("empty_strings", st.total_empty);
  put("unique_strings", st.unique_strings);
  put("total_bytes", st.total_bytes);
  put("total_chars", st.total_chars);
  put("device_memory", st.total_memory);
  put("bytes_avg", st.bytes_avg);
  put("bytes_min", st.bytes_min);
  put("bytes_max", st.bytes_max);
  put("chars_avg", st.chars_avg);
  put("chars_min", st.chars_min);
  put("chars_max", st.chars_max);
  put("memory_avg", st.mem_avg);
  put("memory_min", st.mem_min);
  put("memory_max", st.mem_max);
  put("whitespace", st.whitespace_count);
  put("digits", st.digits_count);
  put("uppercase", st.uppercase_count);
  put("lowercase", st.lowercase_count);
  PyObject* hist = PyDict_New();
  for (const auto& pr : st.char_counts) {
    char text[4];
    int w = 0;
    for (int shift = 24; shift >= 0; shift -= 8)
      if (w || (pr.first >> shift) & 0xFF || shift == 0) text[w++] = (char)((pr.first >> shift) & 0xFF);
    PyObject* key = PyUnicode_DecodeUTF8(text, w, "strict");
    if (!key) {
      PyErr_Clear();
      continue;
    }
    PyObject* n = PyLong_FromUnsignedLong(pr.second);
    PyDict_SetItem(hist, key, n);
    Py_DECREF(key);
    Py_DECREF(n);
  }
  PyDict_SetItemString(d, "chars_histogram", hist);
  Py_DECREF(hist);
  return d;
}

static PyObject* n_dropWrapper(PyObject*, PyObject* args) { return drop_wrapper<NVStrings>(args); }

// ---- conversions (pystrings.cpp:451-880, 1047-1440; convert.cu) ----------------------------------------------------------
// (self, devptr): the results go to the device pointer when one is given; else a host list with None for the null rows
// (pystrings.cpp:1088-1128).  An empty instance gives an empty list.
template <class T, class Call, class Py>
static PyObject* conv_results(PyObject* args, int devarg, Call&& call, Py&& to_py) {
  NVStrings* s = SELF(args);
  const unsigned int count = s->size();
  if (count == 0) return PyList_New(0);
  T* devptr = ptr_arg<T>(args, devarg);
  if (devptr) {
    if (!guarded([&] { call(s, devptr, true); })) return nullptr;
    return PyLong_FromVoidPtr(devptr);
  }
  std::unique_ptr<T[]> host(new T[count]);  // (not a vector: vector<bool> has no data())
  if (!guarded([&] { call(s, host.get(), false); })) return nullptr;
  std::vector<unsigned char> nulls((count + 7) / 8, 0);
  unsigned int ncount = 0;
  if (!guarded([&] { ncount = s->set_null_bitarray(nulls.data(), false, false); })) return nullptr;
  PyObject* ret = PyList_New(count);
  for (unsigned int i = 0; i < count; ++i) {
    if (ncount && !((nulls[i / 8] >> (i % 8)) & 1)) {
      Py_INCREF(Py_None);
      PyList_SetItem(ret, i, Py_None);
    } else {
      PyList_SetItem(ret, i, to_py(host[i]));
    }
  }
  return ret;
}
static PyObject* py_long(long v) { return PyLong_FromLong(v); }
static PyObject* py_ulong(unsigned long v) { return PyLong_FromUnsignedLong(v); }
static PyObject* n_hash(PyObject*, PyObject* args) {
  return conv_results<unsigned int>(args, 1, [](NVStrings* s, unsigned int* o, bool d) { s->hash(o, d); }, py_ulong);
}
static PyObject* n_stoi(PyObject*, PyObject* args) {
  return conv_results<int>(args, 1, [](NVStrings* s, int* o, bool d) { s->stoi(o, d); }, py_long);
}
static PyObject* n_stol(PyObject*, PyObject* args) {
  return conv_results<long>(args, 1, [](NVStrings* s, long* o, bool d) { s->stol(o, d); }, py_long);
}
static PyObject* n_stof(PyObject*, PyObject* args) {
  return conv_results<float>(args, 1, [](NVStrings* s, float* o, bool d) { s->stof(o, d); }, [](float v) { return PyFloat_FromDouble((double)v); });
}
static PyObject* n_stod(PyObject*, PyObject* args) {
  return conv_results<double>(args, 1, [](NVStrings* s, double* o, bool d) { s->stod(o, d); }, [](double v) { return PyFloat_FromDouble(v); });
}
static PyObject* n_htoi(PyObject*, PyObject* args) {
  return conv_results<unsigned int>(args, 1, [](NVStrings* s, unsigned int* o, bool d) { s->htoi(o, d); }, py_ulong);
}
static PyObject* n_ip2int(PyObject*, PyObject* args) {
  return conv_results<unsigned int>(args, 1, [](NVStrings* s, unsigned int* o, bool d) { s->ip2int(o, d); }, py_ulong);
}
static PyObject* n_to_bools(PyObject*, PyObject* args) {  // (self, true, devptr)
  const char* t = str_arg(args, 1);
  return conv_results<bool>(args, 2, [t](NVStrings* s, bool* o, bool d) { s->to_bools(o, t, d); }, [](bool v) { return PyBool_FromLong(v); });
}

// (values, count, nulls, bdevmem): values / nulls are a list, a host buffer or an address (device memory when bdevmem,
// as the reference's DataBuffer has it); `count` is needed for an address only.
template <class T>
struct Values {
  std::unique_ptr<T[]> own;  // (not a vector: vector<bool> has no data())
  Py_buffer view{};
  bool has_view = false;
  const T* data = nullptr;
  size_t count = 0;
  const char* error = nullptr;
  explicit Values(PyObject* o) {
    if (o == Py_None) {
      error = "values required";
    } else if (PyList_Check(o)) {
      count = (size_t)PyList_Size(o);
      own.reset(new T[count ? count : 1]);
      for (size_t i = 0; i < count; ++i) {
        PyObject* e = PyList_GetItem(o, (Py_ssize_t)i);
        if (e == Py_None) own[i] = T(0);
        else if (std::is_floating_point<T>::value) own[i] = T(PyFloat_AsDouble(e));
        else if (PyBool_Check(e)) own[i] = T(e == Py_True);
        else own[i] = T(PyLong_AsLongLong(e));
      }
      if (PyErr_Occurred()) {
        PyErr_Clear();
        error = "values must be numbers";
      }
      data = own.get();
    } else if (PyLong_Check(o)) {
      data = static_cast<const T*>(PyLong_AsVoidPtr(o));
    } else if (PyObject_CheckBuffer(o) && PyObject_GetBuffer(o, &view, PyBUF_FORMAT | PyBUF_ND | PyBUF_C_CONTIGUOUS) == 0) {
      has_view = true;
      if ((size_t)view.itemsize != sizeof(T)) {
        error = "values are not of the expected width";
      } else {
        data = static_cast<const T*>(view.buf);
        count = (size_t)view.len / sizeof(T);
      }
    } else {
      PyErr_Clear();
      error = "values must be a list, a buffer or a memory address";
    }
  }
  ~Values() {
    if (has_view) PyBuffer_Release(&view);
  }
};
template <class T, class Make>
static PyObject* from_values(PyObject* args, const char* what, int nulls_arg, int dev_arg, Make&& make) {
  Values<T> vals(arg(args, 0));
  if (vals.error) {
    PyErr_Format(PyExc_TypeError, "nvstrings.%s(): %s", what, vals.error);
    return nullptr;
  }
  unsigned int count = (unsigned int)vals.count;
  if (count == 0) count = (unsigned int)int_arg(args, 1, 0);
  Values<unsigned char> nulls(arg(args, nulls_arg));
  if (arg(args, nulls_arg) != Py_None && nulls.error) {
    PyErr_Format(PyExc_TypeError, "nvstrings.%s(): nulls: %s", what, nulls.error);
    return nullptr;
  }
  const bool dev = bool_arg(args, dev_arg);
  return make_instance([&] { return make(vals.data, count, arg(args, nulls_arg) == Py_None ? nullptr : nulls.data, dev); });
}
static PyObject* n_createFromInt32s(PyObject*, PyObject* args) {
  return from_values<int>(args, "itos", 2, 3, [](const int* v, unsigned n, const unsigned char* m, bool d) { return NVStrings::itos(v, n, m, d); });
}
static PyObject* n_createFromInt64s(PyObject*, PyObject* args) {
  return from_values<long>(args, "ltos", 2, 3, [](const long* v, unsigned n, const unsigned char* m, bool d) { return NVStrings::ltos(v, n, m, d); });
}
static PyObject* n_createFromFloat32s(PyObject*, PyObject* args) {
  return from_values<float>(args, "ftos", 2, 3, [](const float* v, unsigned n, const unsigned char* m, bool d) { return NVStrings::ftos(v, n, m, d); });
}
static PyObject* n_createFromFloat64s(PyObject*, PyObject* args) {
  return from_values<double>(args, "dtos", 2, 3, [](const double* v, unsigned n, const unsigned char* m, bool d) { return NVStrings::dtos(v, n, m, d); });
}
static PyObject* n_createFromIPv4Integers(PyObject*, PyObject* args) {
  return from_values<unsigned int>(args, "int2ip", 2, 3,
                                   [](const unsigned int* v, unsigned n, const unsigned char* m, bool d) { return NVStrings::int2ip(v, n, m, d); });
}
static PyObject* n_createFromBools(PyObject*, PyObject* args) {  // (values, count, nulls, true, false, bdevmem)
  if (arg(args, 3) == Py_None || arg(args, 4) == Py_None) {
    PyErr_SetString(PyExc_ValueError, "nvstrings.from_bools(): true and false must not be null");
    return nullptr;
  }
  const char* t = str_arg(args, 3);
  const char* f = str_arg(args, 4);
  return from_values<bool>(args, "from_bools", 2, 5, [t, f](const bool* v, unsigned n, const unsigned char* m, bool d) {
    return NVStrings::create_from_bools(v, n, t, f, m, d);
  });
}

// ---- timestamps (pystrings.cpp:707-780, 1335-1388; datetime.cu) ---------------------------------------------------------
// the unit names of the Python API; an unknown name is a ValueError
static bool units_arg(PyObject* args, int i, NVStrings::timestamp_units* units) {
  static const struct {
    const char* name;
    NVStrings::timestamp_units units;
  } names[] = {{"Y", NVStrings::years}, {"M", NVStrings::months}, {"D", NVStrings::days},  {"h", NVStrings::hours}, {"m", NVStrings::minutes},
               {"s", NVStrings::seconds}, {"ms", NVStrings::ms},  {"us", NVStrings::us}, {"ns", NVStrings::ns}};
  const char* u = str_arg(args, i);
  for (const auto& n : names) {
    if (u && !strcmp(u, n.name)) {
      *units = n.units;
      return true;
    }
  }
  if (!PyErr_Occurred()) PyErr_SetString(PyExc_ValueError, "nvstrings: units parameter value unrecognized");
  return false;
}
static PyObject* n_timestamp2int(PyObject*, PyObject* args) {  // (self, format, units, devptr)
  const char* format = str_arg(args, 1);
  NVStrings::timestamp_units units;
  if (!units_arg(args, 2, &units)) return nullptr;
  return conv_results<unsigned long>(args, 3, [&](NVStrings* s, unsigned long* o, bool d) { s->timestamp2long(format, units, o, d); },
                                     [](unsigned long v) { return PyLong_FromLong((long)v); });
}
static PyObject* n_createFromTimestamp(PyObject*, PyObject* args) {  // (values, count, nulls, format, units, bdevmem)
  const char* format = str_arg(args, 3);
  NVStrings::timestamp_units units;
  if (!units_arg(args, 4, &units)) return nullptr;
  PyObject* v = arg(args, 0);
  if (PyObject_CheckBuffer(v)) {  // (pystrings.cpp:743-747: the values must be 8 bytes wide)
    Py_buffer view;
    if (PyObject_GetBuffer(v, &view, PyBUF_FORMAT | PyBUF_ND) == 0) {
      const bool wide = view.itemsize == (Py_ssize_t)sizeof(long) && (!view.format || strchr("qlQL", view.format[strlen(view.format) - 1]));
      PyBuffer_Release(&view);
      if (!wide) {
        PyErr_SetString(PyExc_TypeError, "nvstrings.int2timestamp(): values must be of type int64");
        return nullptr;
      }
    } else {
      PyErr_Clear();
    }
  }
  return from_values<long>(args, "int2timestamp", 2, 5, [&](const long* p, unsigned n, const unsigned char* m, bool d) {
    return NVStrings::long2timestamp(reinterpret_cast<const unsigned long*>(p), n, units, format, m, d);
  });
}

// ---- substrings / padding / wrapping (pystrings.cpp:1671-1899, 2053-2072; substr.cu, pad.cu, modify.cu) -------------
static PyObject* n_get(PyObject*, PyObject* args) {  // (self, position)
  NVStrings* s = SELF(args);
  const unsigned pos = (unsigned)int_arg(args, 1, 0);
  return make_instance([&] { return s->get(pos); });
}
static PyObject* n_repeat(PyObject*, PyObject* args) {  // (self, count)
  NVStrings* s = SELF(args);
  const unsigned count = (unsigned)int_arg(args, 1, 0);
  return make_instance([&] { return s->repeat(count); });
}
// the fill character of the pad family: None is the default (" "), an empty string a ValueError
static bool fill_arg(PyObject* args, int i, const char** fill) {
  *fill = str_arg(args, i);
  if (PyErr_Occurred()) return false;
  if (*fill && !**fill) {
    PyErr_SetString(PyExc_ValueError, "fillchar cannot be empty");
    return false;
  }
  return true;
}
static PyObject* n_pad(PyObject*, PyObject* args) {  // (self, width, side, fillchar): side "left" / "right" / "both"
  NVStrings* s = SELF(args);
  const unsigned width = (unsigned)int_arg(args, 1, 0);
  const char* side = str_arg(args, 2);
  const char* fill = nullptr;
  if (!fill_arg(args, 3, &fill)) return nullptr;
  NVStrings::padside ps = NVStrings::left;
  if (side && !strcmp(side, "right")) ps = NVStrings::right;
  else if (side && !strcmp(side, "both")) ps = NVStrings::both;
  return make_instance([&] { return s->pad(width, ps, fill); });
}
#define JUST_FN(NAME, CALL)                                          \
  static PyObject* NAME(PyObject*, PyObject* args) { /* (self, width, fillchar) */ \
    NVStrings* s = SELF(args);                                       \
    const unsigned width = (unsigned)int_arg(args, 1, 0);            \
    const char* fill = nullptr;                                      \
    if (!fill_arg(args, 2, &fill)) return nullptr;                   \
    return make_instance([&] { return s->CALL(width, fill); });      \
  }
JUST_FN(n_ljust, ljust)
JUST_FN(n_center, center)
JUST_FN(n_rjust, rjust)
static PyObject* n_zfill(PyObject*, PyObject* args) {  // (self, width)
  NVStrings* s = SELF(args);
  const unsigned width = (unsigned)int_arg(args, 1, 0);
  return make_instance([&] { return s->zfill(width); });
}
static PyObject* n_wrap(PyObject*, PyObject* args) {  // (self, width)
  NVStrings* s = SELF(args);
  const unsigned width = (unsigned)int_arg(args, 1, 0);
  return make_instance([&] { return s->wrap(width); });
}
static PyObject* n_slice(PyObject*, PyObject* args) {  // (self, start, stop, step): stop None = -1, step None = 1
  NVStrings* s = SELF(args);
  const int start = (int)int_arg(args, 1, 0), stop = (int)int_arg(args, 2, -1), step = (int)int_arg(args, 3, 1);
  return make_instance([&] { return s->slice(start, stop, step); });
}
static PyObject* n_slice_from(PyObject*, PyObject* args) {  // (self, starts, stops): device addresses, 0 / None = none
  NVStrings* s = SELF(args);
  const int* starts = ptr_arg<const int>(args, 1);
  const int* stops = ptr_arg<const int>(args, 2);
  return make_instance([&] { return s->slice_from(starts, stops); });
}
static PyObject* n_slice_replace(PyObject*, PyObject* args) {  // (self, start, stop, repl): None = 0 / -1 / null
  NVStrings* s = SELF(args);
  const int start = (int)int_arg(args, 1, 0), stop = (int)int_arg(args, 2, -1);
  const char* repl = str_arg(args, 3);
  return make_instance([&] { return s->slice_replace(repl, start, stop); });
}
static PyObject* n_insert(PyObject*, PyObject* args) {  // (self, start, repl)
  NVStrings* s = SELF(args);
  const int start = (int)int_arg(args, 1, 0);
  const char* repl = str_arg(args, 2);
  return make_instance([&] { return s->insert(repl, start); });
}

// ---- character types and swapcase / capitalize / title (pystrings.cpp:3419-3456 and its eight siblings) -------------------
// (self, devptr): with a device address the bools are written there and the address comes back; without, a list in
// which null rows are None -- for is_empty as well
#define CHARTYPE_FN(NAME, CALL)                                                                                      \
  static PyObject* NAME(PyObject*, PyObject* args) {                                                                 \
    NVStrings* s = SELF(args);                                                                                       \
    return bool_results(s, ptr_arg<bool>(args, 1), [&](bool* out, bool dev) { return (int)s->CALL(out, dev); });     \
  }
CHARTYPE_FN(n_isalnum, isalnum)
CHARTYPE_FN(n_isalpha, isalpha)
CHARTYPE_FN(n_isdigit, isdigit)
CHARTYPE_FN(n_isspace, isspace)
CHARTYPE_FN(n_isdecimal, isdecimal)
CHARTYPE_FN(n_isnumeric, isnumeric)
CHARTYPE_FN(n_islower, islower)
CHARTYPE_FN(n_isupper, isupper)
CHARTYPE_FN(n_is_empty, is_empty)
#define CASE_FN(NAME, CALL)                            \
  static PyObject* NAME(PyObject*, PyObject* args) {   \
    NVStrings* s = SELF(args);                         \
    return make_instance([&] { return s->CALL(); });   \
  }
CASE_FN(n_swapcase, swapcase)
CASE_FN(n_capitalize, capitalize)
CASE_FN(n_title, title)

// ---- index / rindex, the URL codec, translate, fillna (pystrings.cpp:2015-2050, 2426-2530, 3044-3104, 3834-3856) ------------
// find / rfind that raise on a miss: (self, str, start, end|None, devptr).  With a device address the results are written
// there either way and a miss raises "not found in N elements" (null rows count as found, as cs_find has it); the host
// list has None for a null row and raises at the first -1.
template <class Find>
static PyObject* index_results(NVStrings* s, const char* name, const char* str, int* devptr, Find&& find) {
  const unsigned int count = s->size();
  if (devptr) {
    unsigned int found = 0;
    if (!guarded([&] { found = find(devptr, true); })) return nullptr;
    if (found != count) {
      PyErr_Format(PyExc_ValueError, "nvstrings.%s: [%s] not found in %d elements", name, str ? str : "", (int)(count - found));
      return nullptr;
    }
    return PyLong_FromVoidPtr(devptr);
  }
  if (count == 0) return PyList_New(0);
  std::vector<int> host(count);
  if (!guarded([&] { find(host.data(), false); })) return nullptr;
  for (unsigned int i = 0; i < count; ++i)
    if (host[i] == -1) {
      PyErr_Format(PyExc_ValueError, "nvstrings.%s: [%s] not found in element %d", name, str ? str : "", (int)i);
      return nullptr;
    }
  PyObject* ret = PyList_New(count);
  for (unsigned int i = 0; i < count; ++i) {
    if (host[i] < -1) {
      Py_INCREF(Py_None);
      PyList_SetItem(ret, i, Py_None);
    } else {
      PyList_SetItem(ret, i, PyLong_FromLong((long)host[i]));
    }
  }
  return ret;
}
static PyObject* n_index(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  const int start = (int)int_arg(args, 2, 0), end = (int)int_arg(args, 3, -1);
  return index_results(s, "index", str, ptr_arg<int>(args, 4), [&](int* out, bool dev) { return s->find(str, start, end, out, dev); });
}
static PyObject* n_rindex(PyObject*, PyObject* args) {
  NVStrings* s = SELF(args);
  const char* str = str_arg(args, 1);
  const int start = (int)int_arg(args, 2, 0), end = (int)int_arg(args, 3, -1);
  return index_results(s, "rindex", str, ptr_arg<int>(args, 4), [&](int* out, bool dev) { return s->rfind(str, start, end, out, dev); });
}
CASE_FN(n_url_encode, url_encode)
CASE_FN(n_url_decode, url_decode)
// one side of a translate pair: an ordinal, a str (its first character) or, for a target, None (0: drop the character)
static bool code_point(PyObject* o, bool none_ok, unsigned* out) {
  if (o == Py_None && none_ok) {
    *out = 0;
    return true;
  }
  if (PyUnicode_Check(o) && PyUnicode_GetLength(o) >= 1) {
    *out = (unsigned)PyUnicode_ReadChar(o, 0);
    return true;
  }
  if (PyLong_Check(o)) {
    const unsigned long v = PyLong_AsUnsignedLong(o);
    if (PyErr_Occurred() || v > 0xFFFFFFFFul) {
      PyErr_Clear();
      return false;
    }
    *out = (unsigned)v;
    return true;
  }
  return false;
}
static PyObject* n_translate(PyObject*, PyObject* args) {  // (self, table): a dict of ordinal -> ordinal | None, or a list of [char, char | None]
  NVStrings* s = SELF(args);
  PyObject* t = arg(args, 1);
  std::vector<std::pair<unsigned, unsigned>> table;
  bool ok = true;
  if (PyList_Check(t)) {
    for (Py_ssize_t i = 0; ok && i < PyList_Size(t); ++i) {
      PyObject* e = PyList_GetItem(t, i);
      const bool seq = PyList_Check(e) || PyTuple_Check(e);
      std::pair<unsigned, unsigned> p;
      ok = seq && PySequence_Size(e) == 2;
      if (ok) {
        PyObject *k = PySequence_GetItem(e, 0), *v = PySequence_GetItem(e, 1);
        ok = code_point(k, false, &p.first) && code_point(v, true, &p.second);
        Py_XDECREF(k);
        Py_XDECREF(v);
      }
      table.push_back(p);
    }
    if (!ok) {
      PyErr_SetString(PyExc_ValueError, "nvstrings.translate: invalid map entry");
      return nullptr;
    }
  } else if (PyDict_Check(t)) {
    PyObject *k = nullptr, *v = nullptr;
    Py_ssize_t pos = 0;
    while (ok && PyDict_Next(t, &pos, &k, &v)) {
      std::pair<unsigned, unsigned> p;
      ok = code_point(k, false, &p.first) && code_point(v, true, &p.second);
      table.push_back(p);
    }
    if (!ok) {
      PyErr_SetString(PyExc_ValueError, "nvstrings.translate: invalid map entry");
      return nullptr;
    }
  } else {
    PyErr_SetString(PyExc_ValueError, "nvstrings.translate: invalid argument type");
    return nullptr;
  }
  return make_instance([&] { return s->translate(table.data(), (unsigned int)table.size()); });
}
static PyObject* n_fillna(PyObject*, PyObject* args) {  // (self, repl): a str, or an nvstrings object of the same size
  NVStrings* s = SELF(args);
  PyObject* r = arg(args, 1);
  if (r == Py_None) {
    PyErr_SetString(PyExc_ValueError, "nvstrings.fillna repl argument must be specified");
    return nullptr;
  }
  if (PyUnicode_Check(r)) {
    const char* str = PyUnicode_AsUTF8(r);
    return make_instance([&] { return s->fillna(str); });
  }
  NVStrings* other = PyLong_Check(r) ? nullptr : handle_of<NVStrings>(r);
  if (!other) {
    PyErr_SetString(PyExc_ValueError, "nvstrings.fillna repl argument must be a str or an nvstrings object");
    return nullptr;
  }
  if (other->size() != s->size()) {
    PyErr_SetString(PyExc_ValueError, "nvstrings.fillna repl argument must be same size");
    return nullptr;
  }
  return make_instance([&] { return s->fillna(*other); });
}

static PyMethodDef s_Methods[] = {
#define M(n) {#n, n, METH_VARARGS, ""}
    M(n_dropWrapper), M(n_getIPCData), M(n_createFromIPC),
    M(n_createFromHostStrings), M(n_destroyStrings), M(n_createHostStrings), M(n_createFromOffsets), M(n_createFromCSV), M(n_createFromNVStrings), M(n_create_offsets),
    M(n_size), M(n_len), M(n_byte_count), M(n_null_count), M(n_set_null_bitmask), M(n_copy), M(n_split), M(n_rsplit), M(n_split_record),
    M(n_rsplit_record), M(n_partition), M(n_rpartition), M(n_replace), M(n_replace_multi), M(n_replace_with_backrefs), M(n_lstrip), M(n_strip),
    M(n_rstrip), M(n_lower), M(n_upper), M(n_find), M(n_rfind), M(n_find_from), M(n_find_multiple), M(n_compare), M(n_match_strings), M(n_startswith), M(n_endswith), M(n_contains), M(n_match), M(n_count), M(n_findall), M(n_findall_record), M(n_extract),
    M(n_extract_record), M(n_sort), M(n_order), M(n_gather), M(n_sublist), M(n_scatter), M(n_scalar_scatter), M(n_remove_strings),
    M(n_add_strings), M(n_cat), M(n_join), M(n_device_memory), M(n_get_info),
    M(n_hash), M(n_stoi), M(n_stol), M(n_stof), M(n_stod), M(n_htoi), M(n_ip2int), M(n_to_bools), M(n_createFromInt32s),
    M(n_createFromInt64s), M(n_createFromFloat32s), M(n_createFromFloat64s), M(n_createFromIPv4Integers), M(n_createFromBools),
    M(n_timestamp2int), M(n_createFromTimestamp),
    M(n_get), M(n_slice), M(n_slice_from), M(n_slice_replace), M(n_insert), M(n_repeat), M(n_pad), M(n_ljust), M(n_center),
    M(n_rjust), M(n_zfill), M(n_wrap),
    M(n_isalnum), M(n_isalpha), M(n_isdigit), M(n_isspace), M(n_isdecimal), M(n_isnumeric), M(n_islower), M(n_isupper), M(n_is_empty),
    M(n_swapcase), M(n_capitalize), M(n_title),
    M(n_index), M(n_rindex), M(n_url_encode), M(n_url_decode), M(n_translate), M(n_fillna),
#undef M
    {NULL, NULL, 0, NULL}};
static struct PyModuleDef s_Module = {PyModuleDef_HEAD_INIT, "pyniNVStrings", "CPython glue of nvstrings over the MI355X back-end", -1, s_Methods};
PyMODINIT_FUNC PyInit_pyniNVStrings(void) { return PyModule_Create(&s_Module); }
