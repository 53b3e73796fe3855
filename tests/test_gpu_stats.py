"""compute_statistics / get_info on the MI355X against the model of tests/stats_model.py (checked against stats_ops.h by
tests/test_stats_cpu.py): the worked example through the Python API, the pyni glue and a C++ program built against
include/nvstrings; every tile edge on the tile route and a long row on the rows route, routes asserted; the histogram's hot
bin, its LDS boundary and its ends; cross-checks against len / byte_count / null_count / is_empty / the category build /
device_memory; a borrowed column whose null rows have bytes; int32 and int64 offsets; degenerate columns; the `what` subsets;
a pair buffer that is too small; repeatability and the bytes in use."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import borrowedutil as bu
import cpulibs
import gpuutil
import stats_model as m
from test_stats_cpu import EXAMPLE, EXAMPLE_FIGURES, EXAMPLE_HISTOGRAM

pytestmark = pytest.mark.gpu

ROOT = cpulibs.ROOT
LENGTHS, CLASSES, HISTOGRAM, UNIQUE, ALL = 1, 2, 4, 8, 15


def _L():
    return gpuutil.lib()


def _route():
    return _L().lib.cs_debug_last_route().decode()


def column(rows, narrow=False):
    """rows of bytes / None -> a device column with int64 offsets (`narrow`: int32)"""
    from custrings_amd import nvstrings

    chars, offs, nulls = m.ctm.to_arrow(rows)
    valid = np.concatenate([np.packbits(1 - nulls, bitorder="little"), np.zeros(8, dtype=np.uint8)])
    chars = chars if chars.size else np.zeros(1, dtype=np.uint8)
    if narrow:
        return nvstrings.from_offsets(chars, offs.astype(np.int32), len(rows), valid)
    return nvstrings.from_offsets64(chars, offs, len(rows), valid)


def stats(g, what=ALL):
    from custrings_amd import nvstrings

    return nvstrings.column_statistics(g, what)


def check_against_model(g, rows, route=None):
    if route:
        stats(g, ALL & ~UNIQUE)  # (the pass alone: what the category build notes is its own business)
        assert _route() == route, _route()
    st, pairs = stats(g)
    want, want_pairs = m.model(rows)
    bad = [k for k in want if st[k] != want[k]]
    assert not bad, [(k, st[k], want[k]) for k in bad]
    assert pairs == want_pairs
    return st, pairs


# ---- the worked example, three ways -------------------------------------------------------------------------------------------
def _example_info(device_memory):
    d = {k: EXAMPLE_FIGURES[v] for k, v in m.INFO_OF.items()}
    d["device_memory"] = device_memory
    d["chars_histogram"] = dict(EXAMPLE_HISTOGRAM)
    return d


def test_worked_example_python_api():
    from custrings_amd import nvstrings

    s = nvstrings.to_device(EXAMPLE)
    info = s.get_info()
    assert list(info) == m.INFO_KEYS
    assert info == _example_info(s.device_memory())
    assert list(info["chars_histogram"].items()) == EXAMPLE_HISTOGRAM  # (code-point order)
    assert nvstrings.get_info(s) == info
    st, pairs = stats(s)
    assert {k: st[k] for k in EXAMPLE_FIGURES} == EXAMPLE_FIGURES and pairs[-1] == (0xC3A9, 1)


def test_worked_example_pyni_glue():
    import pyniNVStrings as P

    h = P.n_createFromHostStrings(EXAMPLE)
    try:
        info = P.n_get_info(h)
        assert sorted(info) == sorted(m.INFO_KEYS)
        assert info == _example_info(P.n_device_memory(h))
        assert list(info["chars_histogram"].items()) == EXAMPLE_HISTOGRAM
    finally:
        P.n_destroyStrings(h)


CPP = r"""
#include <cstdio>
#include "nvstrings/NVStrings.h"
#include "nvstrings/StringsStatistics.h"
int main() {
  const char* a[] = {"hello", "World 42", nullptr, "", "h\xc3\xa9llo"};
  NVStrings* s = NVStrings::create_from_array(a, 5);
  StringsStatistics st;
  st.char_counts.emplace_back(1u, 1u);  // (what the call finds there goes)
  s->compute_statistics(st);
#define P(f) printf(#f " %zu\n", st.f)
  P(total_bytes); P(total_chars); P(bytes_avg); P(bytes_max); P(bytes_min); P(bytes_95); P(chars_avg); P(chars_max); P(chars_min); P(chars_95);
  P(mem_avg); P(mem_max); P(mem_min); P(mem_95); P(total_strings); P(total_nulls); P(total_empty); P(unique_strings);
  P(whitespace_count); P(digits_count); P(uppercase_count); P(lowercase_count);
  printf("memory_is_memsize %d\n", (int)(st.total_memory == s->memsize()));
  for (size_t i = 0; i < st.char_counts.size(); ++i) printf("pair %u %u\n", st.char_counts[i].first, st.char_counts[i].second);
  NVStrings::destroy(s);
  s = NVStrings::create_from_array(a, 0);
  s->compute_statistics(st);
  printf("empty %zu %zu %zu %zu\n", st.total_strings, st.total_memory, st.mem_min, st.char_counts.size());
  NVStrings::destroy(s);
  return 0;
}
"""


def test_worked_example_cpp_program():
    lib = os.path.join(ROOT, "custrings_amd")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "stats_kat.cpp"), os.path.join(d, "stats_kat")
        open(src, "w").write(CPP)
        subprocess.run(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", lib, "-lNVStrings",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.splitlines()]
    got = {ln[0]: int(ln[1]) for ln in lines if len(ln) == 2}
    assert {k: got[k] for k in EXAMPLE_FIGURES} == EXAMPLE_FIGURES
    assert got["memory_is_memsize"] == 1
    assert [(int(ln[1]), int(ln[2])) for ln in lines if ln[0] == "pair"] == [(int.from_bytes(ch.encode(), "big"), n) for ch, n in EXAMPLE_HISTOGRAM]
    assert ["empty", "0", "0", "0", "0"] in lines


# ---- routes ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_rows():
    return m.random_bytes_rows(70_000, seed=11)  # rows of 0..40 random bytes; every 7th null, every 11th empty


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 70_000])
def test_tile_edges(random_rows, n):
    rows = random_rows[:n] if n > 1 else [b"one r\xc3\xb6w"]
    st, _ = check_against_model(column(rows), rows, route="tile")
    if n >= 63:
        assert st["total_nulls"] == n // 7 and st["total_empty"] >= n // 11 - n // 77 - 1


def test_rows_route_long_row(random_rows):
    base = random_rows[100:165]
    long_one = bu.long_row(7000, 6)
    rows = base[:30] + [long_one] + base[31:]
    assert len(rows) == 65
    st, pairs = check_against_model(column(rows), rows, route="rows")
    # the same rows without the long one on the tile route, plus that row's own figures
    short = base[:30] + [b""] + base[31:]
    st_t, pairs_t = check_against_model(column(short), short, route="tile")
    own, own_pairs = m.model([long_one])
    for k in ("total_bytes", "total_chars", "whitespace_count", "digits_count", "uppercase_count", "lowercase_count"):
        assert st[k] == st_t[k] + own[k], k
    assert st["total_empty"] == st_t["total_empty"] - 1 and st["bytes_max"] == len(long_one)
    summed = dict(pairs_t)
    for p, c in own_pairs:
        summed[p] = summed.get(p, 0) + c
    assert dict(pairs) == summed


# ---- the histogram on the device ------------------------------------------------------------------------------------------------
def test_histogram_every_lane_on_one_bin():
    rows = [b"a"] * 64_000
    st, pairs = check_against_model(column(rows), rows, route="tile")
    assert pairs == [(ord("a"), 64_000)] and st["lowercase_count"] == 64_000 and st["unique_strings"] == 1


def test_histogram_spread_over_printable_ascii():
    alphabet = bytes(range(0x20, 0x7F))
    rows = [(alphabet * 2)[i % 95:i % 95 + 19] for i in range(9_500)]
    _, pairs = check_against_model(column(rows), rows, route="tile")
    assert [p for p, _ in pairs] == list(alphabet) and {c for _, c in pairs} == {9_500 * 19 // 95}


def test_histogram_lds_boundary_and_ends():
    edge = int(_L().lib.cs_stats_lds_bins())
    assert 0x80 <= edge <= 0x10000
    enc = lambda cp: chr(cp).encode("utf-8", "surrogatepass")  # noqa: E731
    below, above = enc(edge - 1), enc(edge) if edge < 0x10000 else b""
    rows = [below * 3 + above * 5, above + b"x" + below] * 300 + m.edge_rows()
    _, pairs = check_against_model(column(rows), rows, route="tile")
    got = dict(pairs)
    base = dict(m.model(m.edge_rows())[1])
    assert got[m.packed(edge - 1)] == 4 * 300 + base.get(m.packed(edge - 1), 0)
    if edge < 0x10000:
        assert got[m.packed(edge)] == 6 * 300 + base.get(m.packed(edge), 0)
    assert got[m.packed(0xFFFF)] == 5 and 0 not in got and max(got) == m.packed(0xFFFF)  # U+0000 and U+10000 up: counted in chars, never listed


@pytest.mark.parametrize("layout", [2, 3])
def test_measured_histogram_layouts_give_the_same_pairs(random_rows, layout):
    """CS_STATS_HIST: the per-wave bins and the leader-match step that DESIGN.md section 4j measures against the product's layout"""
    L = _L()
    rows = random_rows[:3_000] + [b"a"] * 2_000 + [None if r is None else r.encode() for r in m.text_rows(2_000, seed=23)]
    L.lib.cs_config_set(b"CS_STATS_HIST", str(layout).encode())
    try:
        check_against_model(column(rows), rows, route="tile")
        long_rows = rows[:64] + [bu.long_row(7000, 6)]
        check_against_model(column(long_rows), long_rows, route="rows")
    finally:
        L.lib.cs_config_set(b"CS_STATS_HIST", None)


# ---- cross-checks against ops that have their own tests -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["text", "malformed"])
def test_cross_checks(kind, random_rows):
    L = _L()
    if kind == "text":
        rows = [None if r is None else r.encode() for r in m.text_rows(5_000, seed=21)]
    else:
        rows = m.malformed_rows() * 30 + random_rows[:3_000]
    g = column(rows)
    n = len(rows)
    info = g.get_info()
    lens = np.zeros(n, dtype=np.int32)
    total = C.c_int64()
    L.check(L.lib.cs_len(g.m_cptr, lens.ctypes.data, 0, None, C.byref(total)))
    assert info["total_chars"] == total.value == int(lens[lens > 0].sum())
    assert info["chars_max"] == int(lens.max()) and info["chars_min"] == int(lens[lens > 0].min())
    L.check(L.lib.cs_column_byte_count(g.m_cptr, lens.ctypes.data, 0, None, C.byref(total)))
    assert info["total_bytes"] == total.value and info["bytes_max"] == int(lens.max())
    assert info["null_strings"] == int(L.lib.cs_column_null_count(g.m_cptr)) == g.null_count()
    empty = np.zeros(n, dtype=np.uint8)
    L.check(L.lib.cs_is_empty(g.m_cptr, empty.ctypes.data, 0, None, C.byref(total)))
    assert info["empty_strings"] == total.value - info["null_strings"] and info["empty_strings"] > 0
    cat = C.c_void_p()
    L.check(L.lib.cs_category_build(g.m_cptr, None, C.byref(cat)))
    try:
        assert info["unique_strings"] == int(L.lib.cs_category_keys_size(cat))
    finally:
        L.lib.cs_category_destroy(cat)
    assert info["device_memory"] == g.device_memory()
    check_against_model(g, rows)


# ---- a borrowed column: odd address, hostile bytes around, null rows with bytes of their own --------------------------------
@pytest.mark.parametrize("poison", bu.POISONS)
@pytest.mark.parametrize("shift", [1, 15])
def test_borrowed_column_null_rows_with_bytes(poison, shift):
    import torch
    from custrings_amd import nvstrings

    pz = bu.poison_for(poison, "text")
    rows = bu.body_rows(300, seed=31)
    hidden = "Ünï 12 HIDDEN\t".encode()  # what a null row's extent holds: it must count nowhere
    held = [hidden if r is None else r for r in rows]
    chars, offs, _ = m.ctm.to_arrow(held)
    valid = np.packbits(np.array([r is not None for r in rows] + [True] * ((-len(rows)) % 8), dtype=np.uint8), bitorder="little")
    assert any(r is None for r in rows)
    cb, _, cat_ = bu.place(chars, shift, pz, "cuda:0")
    ob, ov, _ = bu.place(offs, 8, pz, "cuda:0", align=8)
    vb, vv, _ = bu.place(valid, 5, pz, "cuda:0")
    ptr = cb.data_ptr() + cat_
    assert ptr % 16 == shift
    g = nvstrings.from_offsets64(ptr, ov.view(torch.int64), len(rows), vv, bdevmem=True, copy=False)
    g._keep = (cb, ob, vb)
    st, pairs = check_against_model(g, rows, route="tile")
    assert st["total_nulls"] == sum(r is None for r in rows)
    before = cb.cpu().numpy().copy()
    stats(g)
    assert np.array_equal(cb.cpu().numpy(), before)


def test_int32_and_int64_offsets_agree(random_rows):
    from custrings_amd import nvstrings

    rows = random_rows[:5_000]
    wide, narrow = column(rows), column(rows, narrow=True)
    a, b_ = stats(wide), stats(narrow)
    a[0].pop("total_memory"), b_[0].pop("total_memory")
    assert a == b_
    assert nvstrings.get_info(narrow)["device_memory"] == narrow.device_memory()
    check_against_model(narrow, rows, route="tile")


# ---- degenerate columns ---------------------------------------------------------------------------------------------------------
def test_degenerate_columns():
    from custrings_amd import nvstrings

    st, pairs = stats(nvstrings.to_device([]))
    assert not any(st.values()) and pairs == []
    info = nvstrings.to_device([]).get_info()
    assert info["chars_histogram"] == {} and not any(v for k, v in info.items() if k != "chars_histogram")
    rows = [None] * 130
    st, pairs = check_against_model(column(rows), rows)
    assert st["unique_strings"] == 1 and st["bytes_min"] == st["chars_min"] == st["mem_min"] == 0 and pairs == []
    rows = [b""] * 130
    st, pairs = check_against_model(column(rows), rows)
    assert st["mem_min"] == st["mem_max"] == 9 and st["total_empty"] == 130 and pairs == []


# ---- `what` ---------------------------------------------------------------------------------------------------------------------
def _launches(name):
    L = _L()
    n = C.c_int64()
    ms = C.c_double()
    L.check(L.lib.cs_prof_get(name.encode(), C.byref(ms), C.byref(n)))
    return n.value


def test_what_subsets(random_rows):
    L = _L()
    rows = random_rows[:2_000] + [b"Ab 1\tz"]
    g = column(rows)
    want, want_pairs = m.model(rows)
    lengths = ("total_bytes total_chars bytes_avg bytes_max bytes_min chars_avg chars_max chars_min mem_avg mem_max mem_min total_nulls "
               "total_empty").split()
    classes = "whitespace_count digits_count uppercase_count lowercase_count".split()
    L.lib.cs_prof_enable(1)
    try:
        L.lib.cs_prof_reset()
        st, pairs = stats(g, LENGTHS)
        assert _route() == "tile"
        assert _launches("k_stats") == 1 and _launches("k_cat_insert") == 0  # no category build
        assert {k: st[k] for k in lengths} == {k: want[k] for k in lengths} and pairs == []
        assert st["unique_strings"] == 0 and not any(st[k] for k in classes) and st["total_strings"] == len(rows)
        st, pairs = stats(g, CLASSES)
        assert {k: st[k] for k in classes} == {k: want[k] for k in classes} and any(st[k] for k in classes)
        assert not any(st[k] for k in lengths) and pairs == [] and st["unique_strings"] == 0
        st, pairs = stats(g, HISTOGRAM)
        assert pairs == want_pairs and not any(st[k] for k in lengths + classes)
        assert _launches("k_cat_insert") == 0
        L.lib.cs_prof_reset()
        st, pairs = stats(g, UNIQUE)
        assert st["unique_strings"] == want["unique_strings"] and not any(st[k] for k in lengths + classes) and pairs == []
        assert _launches("k_stats") == 0 and _launches("k_cat_insert") >= 1
    finally:
        L.lib.cs_prof_enable(0)
        L.lib.cs_prof_reset()


def test_pairs_cap_too_small_and_null_pointers():
    from custrings_amd import nvstrings

    L = _L()
    g = nvstrings.to_device(EXAMPLE)
    st = (C.c_uint64 * 23)()
    pairs = np.full((16, 2), 0xA5A5A5A5, dtype=np.uint32)
    n = C.c_int64(-1)
    bad = 1  # CS_ERR_INVALID_ARG
    assert L.lib.cs_column_statistics(g.m_cptr, ALL, st, pairs.ctypes.data, 10, C.byref(n), 0, None) == bad
    assert n.value == len(EXAMPLE_HISTOGRAM) == 11 and np.all(pairs == 0xA5A5A5A5)
    assert L.lib.cs_column_statistics(g.m_cptr, HISTOGRAM, st, None, 0, C.byref(n), 0, None) == bad and n.value == 11
    assert L.lib.cs_column_statistics(g.m_cptr, ALL, st, pairs.ctypes.data, 11, C.byref(n), 0, None) == 0
    assert n.value == 11 and pairs[10].tolist() == [0xC3A9, 1] and np.all(pairs[11:] == 0xA5A5A5A5)
    assert L.lib.cs_column_statistics(None, ALL, st, pairs.ctypes.data, 16, C.byref(n), 0, None) == bad
    assert L.lib.cs_column_statistics(g.m_cptr, ALL, None, pairs.ctypes.data, 16, C.byref(n), 0, None) == bad
    assert L.lib.cs_column_statistics(g.m_cptr, ALL, st, pairs.ctypes.data, 16, None, 0, None) == bad
    assert L.lib.cs_column_statistics(g.m_cptr, ALL, st, None, 16, C.byref(n), 0, None) == bad
    assert L.lib.cs_column_statistics(g.m_cptr, LENGTHS | UNIQUE, st, None, 0, None, 0, None) == 0  # (no histogram: no pair arguments needed)


def test_pairs_to_device_memory():
    import torch
    from custrings_amd import nvstrings

    L = _L()
    g = nvstrings.to_device(EXAMPLE)
    out = bu.Guarded(np.uint32, 22)
    st = (C.c_uint64 * 23)()
    n = C.c_int64()
    torch.cuda.synchronize()
    L.check(L.lib.cs_column_statistics(g.m_cptr, HISTOGRAM, st, out.ptr, 11, C.byref(n), 1, None))
    assert n.value == 11
    assert out.values().reshape(11, 2).tolist() == [[int.from_bytes(ch.encode(), "big"), c] for ch, c in EXAMPLE_HISTOGRAM]


def test_repeatable_and_nothing_stays_in_use(random_rows):
    L = _L()
    rows = random_rows[:20_000]
    g = column(rows)
    first = stats(g)  # (the column's cached metadata is made here)
    before = int(L.lib.cs_device_bytes_in_use())
    second = stats(g)
    assert int(L.lib.cs_device_bytes_in_use()) == before
    assert first == second
    info = g.get_info()
    assert int(L.lib.cs_device_bytes_in_use()) == before
    assert info == g.get_info()
