"""Writes tests/golden/reference_numcat.json and tests/golden/relink_numcat_symbols.json: the known answers of the reference's tests of the numeric categories
(python/tests/test_category_numeric.py, 15 cases) and of four docstring examples of its nvcategory.py.

The cases are transcribed below as data; every one names its file and a literal that must stand there, which is looked up
in the reference tree (the line it is found on is recorded).  A case: dtype, items, optional nulls (the bitmask's bytes),
op, arg, expected.  Ops: size, keys_size, keys, values, keys_values (both, of the category the op produces),
indexes_for_key, to_numbers, gather_numbers, keys_type.


The symbol file holds the mangled names a caller of every public member of numeric_category<T>, T = int, long, float,
double, char (CALLER below), leaves undefined when it is compiled against the reference's header: names only.

    python3 tools/make_numcat_golden.py <reference tree> tests/golden
"""
import json
import os
import subprocess
import sys
import tempfile

CALLER = r"""
#include "numeric_category.h"
template <typename T>
long use(const T* items, const int* idx, T* out, unsigned char* bits, int* rows) {
  numeric_category<T>* c = new numeric_category<T>(items, 4, bits);
  numeric_category<T>* d = c->copy();
  long n = (long)(c->size() + c->keys_size()) + (c->keys() != 0) + (c->values() != 0) + (c->nulls_bitmask() != 0) + c->has_nulls() + c->keys_have_null();
  c->print("", " ");
  n += c->get_type_name()[0] + (long)c->get_key_for(0) + c->is_value_null(0) + c->get_index_for(items[0]);
  n += (long)c->get_indexes_for(items[0], rows) + (long)c->get_indexes_for_null_key(rows);
  numeric_category<T>* r[] = {c->add_keys(items, 1, bits), c->remove_keys(items, 1, bits), c->remove_unused_keys(), c->set_keys(items, 1, bits),
                              c->merge(*d), c->gather(idx, 1), c->gather_and_remap(idx, 1), c->gather_values(idx, 1)};
  c->to_type(out, bits);
  c->gather_type(idx, 1, out, bits);
  for (numeric_category<T>* x : r) delete x;
  delete d;
  delete c;
  return n;
}
template long use<int>(const int*, const int*, int*, unsigned char*, int*);
template long use<long>(const long*, const int*, long*, unsigned char*, int*);
template long use<float>(const float*, const int*, float*, unsigned char*, int*);
template long use<double>(const double*, const int*, double*, unsigned char*, int*);
template long use<char>(const char*, const int*, char*, unsigned char*, int*);
int main() { return 0; }
"""


def caller_symbols(include_dir):
    """The numeric_category symbols CALLER leaves undefined when compiled against the header in include_dir."""
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "caller.cpp"), os.path.join(d, "caller.o")
        with open(src, "w") as f:
            f.write(CALLER)
        subprocess.run(["g++", "-std=c++14", "-c", "-I", include_dir, src, "-o", obj], check=True)
        out = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
        return sorted({ln.split()[-1] for ln in out.splitlines() if "numeric_category" in ln})


T = "python/tests/test_category_numeric.py"
D = "python/nvcategory.py"
I9 = [4, 1, 2, 3, 2, 1, 4, 1, 1]
F9 = [2, 1, 1.25, 1.5, 1, 1.25, 1, 1, 2]
CASES = [
    (T, "def test_size():", dict(name="size", dtype="int64", items=I9, op="size", expected=9)),
    (T, "def test_keys_size():", dict(name="keys_size", dtype="int32", items=I9, op="keys_size", expected=4)),
    (T, "expected = [1.0, 1.25, 1.5, 2.0]", dict(name="keys", dtype="float64", items=F9, op="keys", expected=[1.0, 1.25, 1.5, 2.0])),
    (T, "expected = [3, 0, 1, 2, 1, 0, 3, 0, 0]", dict(name="values", dtype="int64", items=I9, op="values", expected=[3, 0, 1, 2, 1, 0, 3, 0, 0])),
    (T, "expected = [1, 5, 7, 8]", dict(name="indexes_for_key", dtype="int64", items=I9, op="indexes_for_key", arg=1, expected=[1, 5, 7, 8])),
    (T, "def test_to_numbers():", dict(name="to_numbers", dtype="float64", items=F9, op="to_numbers", expected=F9)),
    (T, "expected = [1.0, 1.5, 1.0]",
     dict(name="gather_numbers", dtype="float64", items=[1, 1.25, 1.5, 1, 1.25, 1, 1, 2], op="gather_numbers", arg=[0, 2, 0], expected=[1.0, 1.5, 1.0])),
    (T, "expected_values = [4, 1, 2, 3, 2, 1, 4, 1, 1, 2, 4, 3, 0]",
     dict(name="merge_category", dtype="int64", items=I9, op="merge_and_remap", arg=[2, 4, 3, 0],
          expected=dict(keys=[0, 1, 2, 3, 4], values=[4, 1, 2, 3, 2, 1, 4, 1, 1, 2, 4, 3, 0]))),
    (T, "expected_keys = [0, 1, 1.25, 1.5, 1.75, 2]",
     dict(name="add_keys", dtype="float64", items=F9, op="add_keys", arg=[2, 1, 1.75, 0],
          expected=dict(keys=[0, 1, 1.25, 1.5, 1.75, 2], values=[5, 1, 2, 3, 1, 2, 1, 1, 5]))),
    (T, "expected_values = [2, 0, 1, -1, 1, 0, 2, 0, 0]",
     dict(name="remove_keys", dtype="int64", items=I9, op="remove_keys", arg=[3, 0], expected=dict(keys=[1, 2, 4], values=[2, 0, 1, -1, 1, 0, 2, 0, 0]))),
    (T, "expected_values = [3, -1, 1, 2, 1, -1, 3, -1, -1]",
     dict(name="set_keys", dtype="int8", items=I9, op="set_keys", arg=[2, 4, 3, 0], expected=dict(keys=[0, 2, 3, 4], values=[3, -1, 1, 2, 1, -1, 3, -1, -1]))),
    (T, "ncat = ncat.remove_unused_keys()",
     dict(name="remove_unused_keys", dtype="int32", items=I9, op="add_keys_then_remove_unused", arg=[2, 4, 3, 0],
          expected=dict(keys=[1, 2, 3, 4], values=[3, 0, 1, 2, 1, 0, 3, 0, 0]))),
    (T, "expected_values = [1, 3, 2, 3, 1, 2]",
     dict(name="gather", dtype="float32", items=F9, op="gather", arg=[1, 3, 2, 3, 1, 2], expected=dict(keys=[1.0, 1.25, 1.5, 2.0], values=[1, 3, 2, 3, 1, 2]))),
    (T, "expected_values = [0, 2, 1, 2, 0, 1]",
     dict(name="gather_and_remap", dtype="float32", items=I9, op="gather_and_remap", arg=[1, 3, 2, 3, 1, 2],
          expected=dict(keys=[2.0, 3.0, 4.0], values=[0, 2, 1, 2, 0, 1]))),
    (T, "expected_keys = [2, 1, 3, 4]",
     dict(name="nulls", dtype="int64", items=I9, nulls=[1 + 2 + 8 + 32 + 64 + 128, 1], op="keys_values",
          expected=dict(keys=[2, 1, 3, 4], values=[3, 1, 0, 2, 0, 1, 3, 1, 1]))),
    (D, "[1, 2, 3, 4] [3, 0, 1, 2, 1, 0, 3, 0, 0]",
     dict(name="doc_from_numbers", dtype="int64", items=I9, op="keys_values", expected=dict(keys=[1, 2, 3, 4], values=[3, 0, 1, 2, 1, 0, 3, 0, 0]))),
    (D, "'float64'", dict(name="doc_keys_type", dtype="float64", items=F9, op="keys_type", expected="float64")),
    (D, "[1, 4, 6, 7]", dict(name="doc_indexes_for_key", dtype="float64", items=F9, op="indexes_for_key", arg=1, expected=[1, 4, 6, 7])),
    (D, "[2.0, 1.0, 1.25, 1.5, 1.0, 1.25, 1.0, 1.0, 2.0]", dict(name="doc_to_numbers", dtype="float64", items=F9, op="to_numbers", expected=F9)),
]


def main(ref, out_dir):
    cases = []
    for path, literal, case in CASES:
        with open(os.path.join(ref, path), encoding="utf8") as f:
            lines = f.read().split("\n")
        hits = [i + 1 for i, ln in enumerate(lines) if literal in ln]
        if not hits:
            sys.exit("%s: no line holds %r" % (path, literal))
        cases.append(dict(case, source="%s:%d" % (path, hits[0]), literal=literal))
    doc = {"about": "known answers of the reference's numeric-category tests and docstring examples (tools/make_numcat_golden.py)", "cases": cases}
    with open(os.path.join(out_dir, "reference_numcat.json"), "w", encoding="utf8") as f:
        json.dump(doc, f, indent=1, ensure_ascii=False)
        f.write("\n")
    print("wrote %d cases" % len(cases))
    symbols = caller_symbols(os.path.join(ref, "cpp", "include"))
    doc = {"about": "numeric_category<T> symbols, T = int / long / float / double / char, that a caller of every public member (tools/make_numcat_golden.py "
                    "CALLER) leaves undefined when compiled against the reference's numeric_category.h", "symbols": symbols}
    with open(os.path.join(out_dir, "relink_numcat_symbols.json"), "w", encoding="utf8") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote %d symbols" % len(symbols))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
