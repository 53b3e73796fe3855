"""contains_strings / strings_counts / edit_distance / porter_stemmer_measure / scatter_count on the MI355X: the reference's
known answers through the Python API, the pyni glue and a C++ program built against include/nvstrings; every op against the
CPU harness of text_ops.h (checked against the model by tests/test_text_cpu.py) on both routes, with the routes asserted;
the bounds of the target staging, the out-tile and the bit-vector form straddled; arbitrary bytes; empty and all-null columns;
one full-size check of the two routes per op family."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cpulibs
import gpuutil
import text_model as m

pytestmark = pytest.mark.gpu

ROOT = cpulibs.ROOT
ROUTES = ["tile", "rows"]


def cases():
    with open(os.path.join(ROOT, "tests", "golden", "reference_text.json")) as f:
        return json.load(f)["cases"]


def _ids(c):
    return "%s-%s" % (c["op"], c["src"].split("/")[-1])


def _L():
    return gpuutil.lib()


def _route():
    return _L().lib.cs_debug_last_route().decode()


def column(rows):
    """rows of str / bytes / None -> a device column"""
    from custrings_amd import nvstrings

    chars, offs, nulls = m.to_arrow(rows)
    valid = np.packbits(1 - nulls, bitorder="little")
    valid = np.concatenate([valid, np.zeros(8, dtype=np.uint8)])
    return nvstrings.from_offsets64(chars if chars.size else np.zeros(1, dtype=np.uint8), offs, len(rows), valid)


def set_route(monkeypatch, route):
    if route == "rows":
        monkeypatch.setenv("CS_TEXT_ROWWISE", "1")
    else:
        monkeypatch.delenv("CS_TEXT_ROWWISE", raising=False)


@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


def run_api(case):
    import nvtext
    from custrings_amd import nvstrings

    s = nvstrings.to_device(case["input"])
    op = case["op"]
    if op == "contains_strings":
        return nvtext.contains_strings(s, case["targets"])
    if op == "strings_counts":
        return nvtext.strings_counts(s, nvstrings.to_device(case["targets"]))
    if op in ("edit_distance", "edit_distance_column"):
        return nvtext.edit_distance(s, case["targets"], algo=0)
    if op == "porter_stemmer_measure":
        return nvtext.porter_stemmer_measure(s)
    return nvtext.scatter_count(s, case["counts"]).to_host()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", cases(), ids=_ids)
def test_known_answers_python_api(case, route, monkeypatch):
    set_route(monkeypatch, route)
    assert run_api(case) == case["expected"], case["src"]
    if case["op"] not in ("scatter_count", "edit_distance_column"):
        assert _route() == route


@pytest.mark.parametrize("case", [c for c in cases() if c["op"] != "porter_stemmer_measure"], ids=_ids)
def test_known_answers_pyni_glue(case):
    import torch

    import pyniNVStrings as PS
    import pyniNVText as P
    from custrings_amd import nvstrings

    s = nvstrings.to_device(case["input"])
    op, n = case["op"], len(case["input"])
    if op == "scatter_count":
        r = P.n_scatter_count(s, case["counts"])
        try:
            assert PS.n_createHostStrings(r) == case["expected"], case["src"]
        finally:
            PS.n_destroyStrings(r)
        dev = torch.tensor([0 if c is None else c for c in case["counts"]], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r = P.n_scatter_count(s, dev.data_ptr())
        try:
            assert PS.n_createHostStrings(r) == case["expected"], case["src"]
        finally:
            PS.n_destroyStrings(r)
        return
    if op in ("contains_strings", "strings_counts"):
        fn = getattr(P, "n_" + op)
        assert fn(s, case["targets"], 0) == case["expected"]  # a list
        assert fn(s, nvstrings.to_device(case["targets"]), 0) == case["expected"]  # an nvstrings
        dtype = torch.uint8 if op == "contains_strings" else torch.int32
        t = torch.full((n, len(case["targets"])), 7, dtype=dtype, device="cuda")
        torch.cuda.synchronize()
        assert fn(s, case["targets"], t.data_ptr()) == t.data_ptr()
        assert t.cpu().numpy().astype(np.int64).tolist() == np.array(case["expected"]).astype(np.int64).tolist()
        with pytest.raises(ValueError):
            fn(s, None, 0)
        with pytest.raises(ValueError):
            fn(s, [], 0)
        return
    tg = case["targets"]
    assert P.n_edit_distance(s, tg, 0, 0) == case["expected"]
    if isinstance(tg, list):
        assert P.n_edit_distance(s, nvstrings.to_device(tg), None, 0) == case["expected"]
    t = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    P.n_edit_distance(s, tg, 0, t.data_ptr())
    assert t.cpu().tolist() == case["expected"]
    with pytest.raises(ValueError):
        P.n_edit_distance(s, tg, 1, 0)
    with pytest.raises(ValueError):
        P.n_edit_distance(s, None, 0, 0)
    with pytest.raises(ValueError):
        P.n_edit_distance(s, ["x"] * (n + 1), 0, 0)


CPP = r"""
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "nvstrings/NVStrings.h"
#include "nvstrings/NVText.h"
static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
template <class T, size_t N> static bool eq(const std::vector<T>& got, const T (&want)[N]) {
  bool ok = got.size() >= N;
  for (size_t i = 0; ok && i < N; ++i) ok = got[i] == want[i];
  return ok;
}
int main() {
  const char* t[] = {"the fox jumped over the dog", "the dog chased the cat", "the cat chased the mouse", nullptr, "", "the mouse ate the cheese"};
  NVStrings* strs = NVStrings::create_from_array(t, 6);
  {
    const char* h[] = {"the", "cat"};
    NVStrings* tg = NVStrings::create_from_array(h, 2);
    bool got[12];
    NVText::contains_strings(*strs, *tg, got, false);
    const bool want[] = {true, false, true, true, true, true, false, false, false, false, true, false};
    for (int i = 0; i < 12; ++i) CHECK(got[i] == want[i]);
    NVStrings::destroy(tg);
  }
  {
    const char* h[] = {"cat ", "dog "};
    NVStrings* tg = NVStrings::create_from_array(h, 2);
    std::vector<unsigned int> got(12, 9);
    NVText::strings_counts(*strs, *tg, got.data(), false);
    const unsigned int want[] = {0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0};
    CHECK(eq(got, want));
    NVStrings::destroy(tg);
  }
  {
    const char* h[] = {"dog", nullptr, "cat", "mouse", "pup", "", "puppy"};
    NVStrings* s = NVStrings::create_from_array(h, 7);
    std::vector<unsigned int> got(7, 9);
    NVText::edit_distance(NVText::levenshtein, *s, "puppy", got.data(), false);
    const unsigned int want[] = {5, 5, 5, 5, 2, 5, 0};
    CHECK(eq(got, want));
    const char* g[] = {"hog", "not", "cake", "house", "fox", nullptr, "puppy"};
    NVStrings* tg = NVStrings::create_from_array(g, 7);
    NVText::edit_distance(NVText::levenshtein, *s, *tg, got.data(), false);
    const unsigned int want2[] = {1, 3, 2, 1, 3, 0, 0};
    CHECK(eq(got, want2));
    bool threw = false;
    try { NVText::edit_distance(NVText::levenshtein, *s, *strs, got.data(), false); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { NVText::edit_distance(NVText::levenshtein, *s, (const char*)nullptr, got.data(), false); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { NVText::edit_distance((NVText::distance_type)1, *s, "x", got.data(), false); } catch (const std::invalid_argument&) { threw = true; }
    CHECK(threw);
    NVStrings::destroy(tg);
    NVStrings::destroy(s);
  }
  {
    const char* h[] = {"abandon", nullptr, "abbey", "cleans", "trouble", "", "yearly"};
    NVStrings* s = NVStrings::create_from_array(h, 7);
    std::vector<unsigned int> got(7, 9);
    NVText::porter_stemmer_measure(*s, nullptr, nullptr, got.data(), false);
    const unsigned int want[] = {3, 0, 2, 1, 1, 0, 1};
    CHECK(eq(got, want));
    NVStrings::destroy(s);
  }
  {
    const char* h[] = {"Larry", "Curly", "Moe"};
    NVStrings* s = NVStrings::create_from_array(h, 3);
    unsigned int counts[] = {3, 0, 1};
    NVStrings* got = NVText::scatter_count(*s, counts, false);
    CHECK(got && got->size() == 4);
    if (got) {
      std::vector<std::vector<char>> bufs(4, std::vector<char>(16, 0));
      std::vector<char*> rows(4);
      for (int i = 0; i < 4; ++i) rows[i] = bufs[i].data();
      got->to_host(rows.data(), 0, 4);
      const char* want[] = {"Larry", "Larry", "Larry", "Moe"};
      for (int i = 0; i < 4; ++i) CHECK(!strcmp(rows[i], want[i]));
      NVStrings::destroy(got);
    }
    CHECK(NVText::scatter_count(*s, nullptr, false) == nullptr);
    NVStrings::destroy(s);
  }
  NVStrings::destroy(strs);
  printf(bad ? "%d FAILED\n" : "cpp text ok\n", bad);
  return bad ? 1 : 0;
}
"""


def test_known_answers_cpp_program():
    pkg = os.path.join(ROOT, "custrings_amd")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cpp"), os.path.join(d, "t")
        with open(src, "w") as f:
            f.write(CPP)
        subprocess.run(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", pkg, "-lNVText", "-lNVStrings",
                        "-lcustrings_amd", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "cpp text ok" in out.stdout, out.stdout + out.stderr


# ---- every op against the harness, both routes ---------------------------------------------------------------------------------
def _len_rows(count, seed):
    """`count` rows cycling through 0 / 1 / 63 / 64 / 65 / 200 characters, null rows and rows with multi-byte characters among them"""
    rng = np.random.default_rng(seed)
    letters = ["a", "e", "y", "b", " ", "t", "é", "日", "aa"]
    lens = [0, 1, 63, 64, 65, 200, 5, 9]
    rows = []
    for i in range(count):
        if i % 11 == 7:
            rows.append(None)
            continue
        n = lens[i % len(lens)]
        pick = rng.integers(0, len(letters) if i % 3 else 6, size=n).tolist()  # (two rows in three are ASCII)
        rows.append("".join(letters[k] for k in pick))
    return rows


def _matrix(fn, dtype, col, tcol):
    res = np.full(max(col.size() * tcol.size(), 1), 7, dtype=dtype)
    _L().check(fn(col.m_cptr, tcol.m_cptr, res.ctypes.data, 0, None))
    return res[: col.size() * tcol.size()]


def _values(call, col):
    res = np.full(max(col.size(), 1), 7, dtype=np.uint32)
    _L().check(call(res.ctypes.data))
    return res[: col.size()]


def _targets(M):
    base = ["a", "aa", "e ", "é", "日", "yt", "", None, "b" * 70, "ab", "t", " "]
    return [base[j % len(base)] if j < len(base) else "aeybt "[j % 6] + "aeybt "[(j // 6) % 6] + "aeybt "[(j // 36) % 6] for j in range(M)]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097])
def test_ops_match_harness(harness, monkeypatch, route, count):
    set_route(monkeypatch, route)
    L = _L().lib
    rows = _len_rows(count, seed=count)
    col, arrow = column(rows), m.to_arrow(rows)
    for M in (2, 33):  # (33 uint32 values a row are beyond the out-tile at 64 rows a tile)
        tg = _targets(M)
        tcol, tarrow = column(tg), m.to_arrow(tg)
        got = _matrix(L.cs_contains_strings, np.uint8, col, tcol)
        assert _route() == route
        assert np.array_equal(got, harness.run_arrow("contains", arrow, tarrow, dtype=np.uint8)), M
        got = _matrix(L.cs_strings_counts, np.uint32, col, tcol)
        assert _route() == route
        assert np.array_equal(got, harness.run_arrow("counts", arrow, tarrow)), M
    for vowels, y in (("aeiou", "y"), ("aeé日", "t")):
        got = _values(lambda p: L.cs_porter_stemmer_measure(col.m_cptr, vowels.encode(), y.encode(), p, 0, None), col)
        assert _route() == route
        assert np.array_equal(got, harness.run_arrow("measure", arrow, a1=vowels, a2=y))
    for target in ("a", "ate by a bee", "日é a"):
        got = _values(lambda p: L.cs_edit_distance(col.m_cptr, target.encode(), 0, p, 0, None), col)
        assert _route() == route
        assert np.array_equal(got, harness.run_arrow("edit_scalar", arrow, m.to_arrow([target]), "dp")), target
    other = _len_rows(count, seed=count + 1)[::-1]
    ocol = column(other)
    got = _values(lambda p: L.cs_edit_distance_column(col.m_cptr, ocol.m_cptr, 0, p, 0, None), col)
    assert _route() == "rows"
    assert np.array_equal(got, harness.run_arrow("edit_pairs", arrow, m.to_arrow(other), "dp"))
    cnt = (np.arange(count) % 4).astype(np.uint32)
    out = C.c_void_p()
    _L().check(L.cs_scatter_count(col.m_cptr, cnt.ctypes.data, 0, None, C.byref(out)))
    from custrings_amd import nvstrings

    got = nvstrings.nvstrings(out.value).to_host()
    assert got == m.scatter_count(rows, cnt.tolist())


@pytest.mark.parametrize("route", ROUTES)
def test_a_long_row_among_short_ones(harness, monkeypatch, route):
    """a row of 5000 bytes fits a 16-row tile; one of 7000 fits no tile: the column goes row-wise whatever the switch says"""
    L = _L().lib
    for big, want_route in ((5000, route), (7000, "rows")):
        set_route(monkeypatch, route)
        rows = [r if r is None else r[:40] for r in _len_rows(130, seed=3)]  # (16 of them stay far below 1 KB)
        rows[77] = ("the cat ate " * 600)[:big]
        col, arrow = column(rows), m.to_arrow(rows)
        tg = ["cat", "e a", "zz"]
        got = _matrix(L.cs_strings_counts, np.uint32, col, column(tg))
        assert _route() == want_route
        assert np.array_equal(got, harness.run_arrow("counts", arrow, m.to_arrow(tg)))
        got = _values(lambda p: L.cs_porter_stemmer_measure(col.m_cptr, None, None, p, 0, None), col)
        assert _route() == want_route
        assert np.array_equal(got, harness.run_arrow("measure", arrow, a1="aeiou", a2="y"))
        got = _values(lambda p: L.cs_edit_distance(col.m_cptr, b"the cat ate the rat", 0, p, 0, None), col)
        assert _route() == want_route
        assert np.array_equal(got, harness.run_arrow("edit_scalar", arrow, m.to_arrow(["the cat ate the rat"]), "dp"))


def test_edit_distance_route_switches_at_65_characters(harness):
    L = _L().lib
    rows = _len_rows(300, seed=8)
    col, arrow = column(rows), m.to_arrow(rows)
    letters = "abey t"
    for chars, want_route in ((1, "tile"), (63, "tile"), (64, "tile"), (65, "rows"), (0, "rows")):
        target = "".join(letters[(i * 7 + i // 5) % 6] for i in range(chars))
        got = _values(lambda p: L.cs_edit_distance(col.m_cptr, target.encode(), 0, p, 0, None), col)
        assert _route() == want_route, chars
        assert np.array_equal(got, harness.run_arrow("edit_scalar", arrow, m.to_arrow([target]), "dp")), chars
    target = "é" + "ab日" * 21  # 64 characters, 107 bytes, non-ASCII ones among them
    got = _values(lambda p: L.cs_edit_distance(col.m_cptr, target.encode(), 0, p, 0, None), col)
    assert _route() == "tile"
    assert np.array_equal(got, harness.run_arrow("edit_scalar", arrow, m.to_arrow([target]), "dp"))


def test_edit_distance_column_nulls_sizes_and_range():
    import nvtext
    from custrings_amd import nvstrings

    a = nvstrings.to_device([None, "abc", None, "", "añb"])
    b_ = nvstrings.to_device(["xy", None, None, None, "anb"])
    assert nvtext.edit_distance(a, b_) == [2, 3, 0, 0, 1]
    assert nvtext.edit_distance(a, [None, "abc", "q", "", "añb"]) == [0, 0, 1, 0, 0]
    with pytest.raises(ValueError):
        nvtext.edit_distance(a, ["x"])
    with pytest.raises(ValueError):
        nvtext.edit_distance(a, "x", algo=1)
    long_row = nvstrings.to_device(["ab", "é" * 32768])  # 65536 bytes, 32768 characters
    for tgt in ("abc", ["ab", "x"], "x" * 70):
        with pytest.raises(ValueError):
            nvtext.edit_distance(long_row, tgt)
    with pytest.raises(ValueError):
        nvtext.edit_distance(nvstrings.to_device(["ab"]), "x" * 32768)
    ok = nvstrings.to_device(["ab", "é" * 32767])  # 65534 bytes, 32767 characters: taken
    assert nvtext.edit_distance(ok, "é") == [2, 32766]
    assert nvtext.edit_distance(ok, ["b", "éz"]) == [1, 32766]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("M", [1, 2, 33, 65])
def test_match_bounds(harness, monkeypatch, route, M):
    """M = 1 / 2: the results are assembled in LDS; 33: the uint32 block is beyond the out-tile, the uint8 one inside; 65: both
    beyond.  A target longer than every row; a target set beyond the LDS budget (bytes, then count) read from memory."""
    set_route(monkeypatch, route)
    L = _L().lib
    rows = _len_rows(200, seed=M)
    col, arrow = column(rows), m.to_arrow(rows)
    sets = [_targets(M), _targets(M)[:-1] + ["ab" * 150]]
    if M == 65:
        sets.append(_targets(M)[:-1] + ["ay " * 3000])  # 9000 bytes of targets: beyond the staged bytes
        sets.append(_targets(600))  # beyond the staged count
    for tg in sets:
        tcol, tarrow = column(tg), m.to_arrow(tg)
        got = _matrix(L.cs_contains_strings, np.uint8, col, tcol)
        assert _route() == route
        assert np.array_equal(got, harness.run_arrow("contains", arrow, tarrow, dtype=np.uint8))
        got = _matrix(L.cs_strings_counts, np.uint32, col, tcol)
        assert np.array_equal(got, harness.run_arrow("counts", arrow, tarrow))


def test_scatter_count_counts_and_nulls():
    import torch

    import nvtext
    from custrings_amd import nvstrings

    rows = [None if i % 9 == 4 else "row%d" % i for i in range(65)]
    s = nvstrings.to_device(rows)
    counts = [(0, 1, 1000)[(i * 5) % 3] for i in range(65)]
    want = m.scatter_count(rows, counts)
    assert nvtext.scatter_count(s, counts).to_host() == want
    dev = torch.tensor(counts, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got = nvtext.scatter_count(s, dev.data_ptr())
    assert got.to_host() == want and got.null_count() == sum(1 for r in want if r is None)
    zero = nvtext.scatter_count(s, [0] * 65)
    assert zero is not None and zero.size() == 0
    assert nvtext.scatter_count(s, [None] * 64 + [2]).to_host() == ["row64", "row64"]
    with pytest.raises(ValueError):
        nvtext.scatter_count(s, [1] * 64)
    with pytest.raises(ValueError):
        nvtext.scatter_count(nvstrings.to_device(["a", "b"]), [1 << 30, 1 << 30])  # 2^31 rows


@pytest.mark.parametrize("seed", [1, 2])
def test_routes_agree_on_arbitrary_bytes(harness, monkeypatch, seed):
    """invalid UTF-8 and NUL bytes: parity with the reference is claimed on valid UTF-8 only, but the two routes and the
    harness (which reads rows copied to the end of its buffer) must agree"""
    L = _L().lib
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(1500):
        n = int(rng.integers(0, 40))
        pool = np.array([0, 0x61, 0x62, 0x80, 0xA9, 0xC3, 0xE6, 0xF0, 0xFF, 0x20], dtype=np.uint8)
        rows.append(None if i % 50 == 9 else bytes(pool[rng.integers(0, len(pool), size=n)].tolist()))
    tg = [b"a", b"\xa9", b"\xc3\xa9", b"\x00", b"ab", b"\xff\xff", b"\x80\x80", b" a"]
    col, arrow, tcol, tarrow = column(rows), m.to_arrow(rows), column(tg), m.to_arrow(tg)
    other = rows[::-1]
    ocol = column(other)
    results = {}
    for route in ROUTES:
        set_route(monkeypatch, route)
        r = [_matrix(L.cs_contains_strings, np.uint8, col, tcol), _matrix(L.cs_strings_counts, np.uint32, col, tcol),
             _values(lambda p: L.cs_porter_stemmer_measure(col.m_cptr, b"a\xc3\xa9", b"b", p, 0, None), col),
             _values(lambda p: L.cs_edit_distance(col.m_cptr, b"a\xc3\xa9b\xff a", 0, p, 0, None), col),
             _values(lambda p: L.cs_edit_distance_column(col.m_cptr, ocol.m_cptr, 0, p, 0, None), col)]
        results[route] = r
    for a, b_ in zip(results["tile"], results["rows"]):
        assert np.array_equal(a, b_)
    assert np.array_equal(results["tile"][0], harness.run_arrow("contains", arrow, tarrow, dtype=np.uint8))
    assert np.array_equal(results["tile"][1], harness.run_arrow("counts", arrow, tarrow))
    assert np.array_equal(results["tile"][3], harness.run_arrow("edit_scalar", arrow, m.to_arrow([b"a\xc3\xa9b\xff a"]), "bits"))
    assert np.array_equal(results["tile"][4], harness.run_arrow("edit_pairs", arrow, m.to_arrow(other), "dp"))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("rows", [[], [None] * 70], ids=["empty", "all-null"])
def test_empty_and_all_null_columns(monkeypatch, route, rows):
    import nvtext

    set_route(monkeypatch, route)
    s = column(rows)
    n = len(rows)
    assert nvtext.contains_strings(s, ["a", "b"]) == [[False, False]] * n
    assert nvtext.strings_counts(s, ["a", "b"]) == [[0, 0]] * n
    assert nvtext.edit_distance(s, "abc") == [3] * n
    assert nvtext.edit_distance(s, "x" * 70) == [70] * n
    if n:
        assert nvtext.edit_distance(s, [None if i % 2 else "ab" for i in range(n)]) == [0 if i % 2 else 2 for i in range(n)]
    assert nvtext.porter_stemmer_measure(s) == [0] * n
    got = nvtext.scatter_count(s, [2] * n)
    if n == 0:
        assert got is None
    else:
        assert got.size() == 2 * n and got.null_count() == 2 * n


# ---- full size: both routes, equal digests -------------------------------------------------------------------------------------
FULL = 10_000_000


def _digest(t):
    import torch

    v = t.to(torch.int64)
    idx = torch.arange(1, v.numel() + 1, device=v.device, dtype=torch.int64)
    return int(((v + 1) * (idx % 1000003 + 1)).sum().item()), int(v.sum().item())


@pytest.mark.parametrize("family", ["match", "edit", "measure", "scatter"])
def test_full_size_routes_agree(monkeypatch, family):
    import torch

    L = _L().lib
    col = gpuutil.synth(2, 0, FULL)  # C2 word rows
    digests = []
    for route in ROUTES:
        set_route(monkeypatch, route)
        if family == "match":
            tcol = column(["a", "th"])
            for fn, dt in ((L.cs_contains_strings, torch.uint8), (L.cs_strings_counts, torch.int32)):
                t = torch.zeros(FULL * 2, dtype=dt, device="cuda")
                torch.cuda.synchronize()
                _L().check(fn(col.m_cptr, tcol.m_cptr, t.data_ptr(), 1, None))
                assert _route() == route
                digests.append(_digest(t))
        elif family == "edit":
            for target in (b"banana", b"x" * 65):
                t = torch.zeros(FULL, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                _L().check(L.cs_edit_distance(col.m_cptr, target, 0, t.data_ptr(), 1, None))
                assert _route() == (route if len(target) <= 64 else "rows")
                digests.append(_digest(t))
        elif family == "measure":
            t = torch.zeros(FULL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            _L().check(L.cs_porter_stemmer_measure(col.m_cptr, None, None, t.data_ptr(), 1, None))
            assert _route() == route
            digests.append(_digest(t))
        else:  # (one route: the scatter against the gather it restates)
            if route == "rows":
                continue
            cnt = torch.arange(FULL, device="cuda", dtype=torch.int32) % 3
            idx = torch.repeat_interleave(torch.arange(FULL, device="cuda", dtype=torch.int32), cnt.to(torch.int64))
            torch.cuda.synchronize()
            out, ref = C.c_void_p(), C.c_void_p()
            _L().check(L.cs_scatter_count(col.m_cptr, cnt.data_ptr(), 1, None, C.byref(out)))
            _L().check(L.cs_gather(col.m_cptr, idx.data_ptr(), idx.numel(), 1, None, C.byref(ref)))
            from custrings_amd import nvstrings

            got, want = nvstrings.nvstrings(out.value), nvstrings.nvstrings(ref.value)
            assert got.size() == idx.numel() == int(cnt.sum().item())
            digests += [(got.digest(), 1), (want.digest(), 1)]
    half = len(digests) // 2
    assert digests[:half] == digests[half:]
    assert all(d[1] > 0 for d in digests)
