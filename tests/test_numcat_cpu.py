"""Numeric categories without a GPU: the model against the reference's known answers, the per-item header under g++, and
the public surface."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import numcat_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_numcat.json")
with open(GOLDEN) as f:
    CASES = json.load(f)["cases"]


def model_answer(case):
    dt = np.dtype(case["dtype"])
    nulls = np.array(case["nulls"], dtype=np.uint8) if "nulls" in case else None
    cat = M.build(np.array(case["items"], dtype=dt), nulls)
    op, arg = case["op"], case.get("arg")
    kv = lambda c: dict(keys=c.keys.tolist(), values=c.values.tolist())
    if op == "size":
        return cat.values.size
    if op == "keys_size":
        return cat.keys.size
    if op == "keys":
        return cat.keys.tolist()
    if op == "values":
        return cat.values.tolist()
    if op == "keys_values":
        return kv(cat)
    if op == "keys_type":
        return cat.dtype.name
    if op == "indexes_for_key":
        return M.indexes_for(cat, arg)
    if op == "to_numbers":
        return M.to_type(cat)[0].tolist()
    if op == "gather_numbers":
        return M.gather_type(cat, arg)[0].tolist()
    if op == "merge_and_remap":
        return kv(M.merge(cat, M.build(np.array(arg, dtype=dt))))
    if op == "add_keys_then_remove_unused":
        return kv(M.remove_unused_keys(M.add_keys(cat, np.array(arg, dtype=dt))))
    return kv(getattr(M, op)(cat, np.array(arg, dtype=dt) if op.endswith("_keys") else arg))


def test_golden_file_has_the_19_cases():
    assert len(CASES) == 19 and len({c["name"] for c in CASES}) == 19
    assert sum(c["source"].startswith("python/tests/test_category_numeric.py:") for c in CASES) == 15


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_model_reproduces_reference(case):
    assert model_answer(case) == case["expected"]


def test_model_rules():
    z = np.array([-0.0, 0.0, np.nan, 1.0, float.fromhex("0x1.8p+0"), np.inf], dtype=np.float64)
    z[4] = np.frombuffer(np.uint64(0x7FF8000000000001).tobytes(), dtype=np.float64)[0]  # a second NaN payload
    c = M.build(z)
    assert c.values.tolist() == [0, 0, 3, 1, 3, 2]
    assert M.bits(c.keys).tolist() == M.bits(z[[0, 3, 5, 2]]).tolist()  # -0.0 and the first NaN are the numbers kept
    c = M.build(np.array([5, 7, 5, 9], dtype=np.int32), np.array([0b0101], dtype=np.uint8))
    assert c.keys.tolist() == [7, 5] and c.values.tolist() == [1, 0, 1, 0] and c.have_null
    r = M.remove_keys(c, np.array([0], dtype=np.int32), np.array([0], dtype=np.uint8))  # removing the null key
    assert r.keys.tolist() == [5] and r.values.tolist() == [0, -1, 0, -1] and not r.have_null and r.mask() is None


# ---- numcat_ops.h under g++ ----------------------------------------------------------------------------------------------------
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include "numcat_ops.h"
template <class T> int run(const char* path, long n) {
  FILE* f = fopen(path, "rb");
  T* v = (T*)malloc(sizeof(T) * n);
  if (!f || fread(v, sizeof(T), n, f) != (size_t)n) return 2;
  for (long i = 0; i < n; ++i) {
    const uint64_t m = csnum::Image<T>::of(v[i]);
    T b = csnum::Image<T>::back(m);
    printf("%llu %llu\n", (unsigned long long)m, (unsigned long long)csnum::Image<T>::of(b));
  }
  return 0;
}
int main(int argc, char** argv) {
  const int type = atoi(argv[1]);
  const long n = atol(argv[3]);
  switch (type) {
    case 0: return run<int8_t>(argv[2], n);
    case 1: return run<int32_t>(argv[2], n);
    case 2: return run<int64_t>(argv[2], n);
    case 3: return run<float>(argv[2], n);
    default: return run<double>(argv[2], n);
  }
}
"""
TYPES = ["int8", "int32", "int64", "float32", "float64"]


@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "h.cpp"), os.path.join(d, "h")
        open(src, "w").write(HARNESS)
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "custrings_amd", "csrc"), src, "-o", exe], check=True)

        def images(values):
            path = os.path.join(d, "in.bin")
            values.tofile(path)
            out = subprocess.run([exe, str(TYPES.index(values.dtype.name)), path, str(values.size)], capture_output=True, text=True, check=True).stdout
            rows = [ln.split() for ln in out.splitlines()]
            return np.array([int(r[0]) for r in rows], dtype=np.uint64), np.array([int(r[1]) for r in rows], dtype=np.uint64)

        yield images


def edge_values(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(20241018)
    raw = np.frombuffer(rng.bytes(10000 * dt.itemsize), dtype=dt)
    if dt.kind == "i":
        info = np.iinfo(dt)
        edges = np.array([info.min, info.max, -1, 0, 1, info.min + 1, info.max - 1], dtype=dt)
    else:
        u = {4: np.uint32, 8: np.uint64}[dt.itemsize]
        info = np.finfo(dt)
        sign = 1 << (8 * dt.itemsize - 1)
        nan1 = int(np.array([np.nan], dtype=dt).view(u)[0])
        pats = np.array([1, sign | 1, (1 << (info.nmant)) - 1, sign | ((1 << info.nmant) - 1), nan1 | 1, nan1 | sign | 5], dtype=u).view(dt)  # denormals, two NaN payloads
        edges = np.concatenate([np.array([info.min, info.max, -1, 0.0, -0.0, 1, np.inf, -np.inf, np.nan, info.tiny, -info.tiny], dtype=dt), pats])
    return np.concatenate([edges, raw])


@pytest.mark.parametrize("dt", TYPES)
def test_image_order_and_equality(harness, dt):
    v = edge_values(dt)
    img, again = harness(v)
    assert np.array_equal(img, again)  # image -> number -> image comes back
    # order: sort by image, then every neighbouring pair must be in value order (NaN last, the zeros equal)
    o = np.argsort(img, kind="stable")
    sv, si = v[o], img[o]
    a, b, ia, ib = sv[:-1], sv[1:], si[:-1], si[1:]
    if np.dtype(dt).kind == "f":
        nan_a, nan_b = np.isnan(a), np.isnan(b)
        eq = (a == b) | (nan_a & nan_b)
        lt = (a < b) | (~nan_a & nan_b)
        assert np.isnan(sv[-1]) and img.max() == img[np.isnan(v)][0]  # NaN sorts last, behind +inf
        z = img[(v == 0)]
        assert z.size >= 2 and (z == z[0]).all()  # -0.0 and +0.0 are merged
        assert len(set(img[np.isnan(v)].tolist())) == 1
    else:
        eq, lt = a == b, a < b
    assert np.array_equal(ia == ib, eq)
    assert np.array_equal(ia < ib, lt)
    assert (eq | lt).all()
    if np.dtype(dt).itemsize <= 4:
        assert int(img.max()) < (1 << (8 * np.dtype(dt).itemsize))  # the narrow types sit in the low bits


# ---- the public surface -----------------------------------------------------------------------------------------------------------
def test_from_numbers_in_both_modules():
    from custrings_amd import nvcategory as N

    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import nvcategory as top

    assert callable(N.from_numbers) and callable(top.from_numbers) and "from_numbers" in N.__all__
    for n in ("keys_type", "to_numbers", "gather_numbers", "gather_values"):
        assert callable(getattr(N.numeric_nvcategory, n)), n
    assert callable(N.nvcategory.__dict__["keys_type"])


def test_not_built_is_empty():
    from custrings_amd import nvcategory as N

    assert list(N._NOT_BUILT) == []
    assert "__getattr__" not in N.nvcategory.__dict__


def test_c_abi_declares_the_entry_points():
    from custrings_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "custrings_amd.h")).read()
    names = [n for n in _lib._PROTOS if n.startswith("cs_numcat_")]
    assert len(names) == 25 and "cs_debug_numcat_sort_rows" in _lib._PROTOS
    for n in names:
        assert hasattr(_lib.lib, n) and (" %s(" % n) in hdr, n


def test_dtype_dispatch_refuses_other_types():
    from custrings_amd import nvcategory as N

    for bad in (np.array([1, 2], dtype=np.uint16), np.array([True]), np.array(["a"])):
        with pytest.raises(ValueError, match="invalid dtype in nvcategory dispatcher"):
            N._numbers(bad)
    assert N._numbers(np.array(["2020-01-01"], dtype="datetime64[ms]"))[3] == N._NUM_NAMES.index("int64")


# ---- the C++ class: the reference's mangled names, from libNVCategory.so ------------------------------------------------------
SYMBOLS = os.path.join(ROOT, "tests", "golden", "relink_numcat_symbols.json")
REF_INCLUDE = "/root/reference/cpp/include"


def golden_tool():
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_numcat_golden", os.path.join(ROOT, "tools", "make_numcat_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def wanted_symbols():
    with open(SYMBOLS) as f:
        return json.load(f)["symbols"]


def test_symbol_file_covers_the_five_types():
    wanted = wanted_symbols()
    for t in "ilfdc":  # int, long, float, double, char
        mine = [s for s in wanted if s.startswith("_ZN16numeric_categoryI%sE" % t)]
        assert len(mine) == 25, (t, len(mine))  # the constructor and 24 members (the destructor and get_type_name are virtual: reached through the vtable, no symbol in the caller)


def test_recorded_symbols_match_reference_header():
    if not os.path.isdir(REF_INCLUDE):
        pytest.skip("the reference headers are not on this machine")
    assert golden_tool().caller_symbols(REF_INCLUDE) == wanted_symbols()


def test_our_header_gives_the_recorded_symbols():
    assert golden_tool().caller_symbols(os.path.join(ROOT, "include", "nvstrings")) == wanted_symbols()


def test_numeric_category_members_are_defined_in_libnvcategory():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host"), "libs"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "custrings_amd", "libNVCategory.so")], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    wanted = set(wanted_symbols())
    assert not (wanted - have), sorted(wanted - have)


@pytest.mark.parametrize("include", ["reference", "ours"])
def test_caller_links_against_libnvcategory(include):
    inc = REF_INCLUDE if include == "reference" else os.path.join(ROOT, "include", "nvstrings")
    if not os.path.isdir(inc):
        pytest.skip("the reference headers are not on this machine")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host"), "libs"], check=True)
    pkg = os.path.join(ROOT, "custrings_amd")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "caller.cpp"), os.path.join(d, "caller")
        open(src, "w").write(golden_tool().CALLER)
        subprocess.run(["g++", "-std=c++14", "-I", inc, src, "-o", exe, "-L", pkg, "-lNVCategory", "-lNVStrings", "-lcustrings_amd",
                        "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
        assert subprocess.run([exe]).returncode == 0  # (main calls nothing: loading resolves every symbol)


def test_pyni_exports_the_numeric_names():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host")], check=True)
    names = ["n_createCategoryFromNumbers", "n_to_numbers", "n_gather_numbers", "n_gather_values", "n_keys_type"]
    code = "import pyniNVCategory as P; print(' '.join(n for n in %r if not hasattr(P, n)))" % names
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "custrings_amd") + os.pathsep + ROOT)
    out = subprocess.run(["python3", "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == ""


def test_string_side_refuses_a_numeric_category():
    from custrings_amd import nvcategory as N

    class Fake:
        _numeric = True
        m_cptr = 1

    with pytest.raises(ValueError):
        N.from_categories([Fake()])
    with pytest.raises(ValueError):
        N.nvcategory(0).merge_category(Fake())
    with pytest.raises(ValueError):
        N.nvcategory(0).merge_and_remap(Fake())
    with pytest.raises(ValueError):
        N._room(3, 4, "keys")
    assert not hasattr(N.numeric_nvcategory, "_nv_wrap")
