"""compute_statistics / get_info without a GPU: the model (tests/stats_model.py) on the worked example and against a second
restatement over Python str; stats_ops.h (the text the kernels compile) built with g++ against the model on generated rows
-- ASCII, 2-, 3- and 4-byte characters, NUL bytes, truncated lead bytes, lone continuation bytes, null and empty rows -- and
on the code points at every edge of the histogram; the relink of NVStrings::compute_statistics; the pyni name and the Python
surface."""
import json
import os
import subprocess
import tempfile

import pytest

import cpulibs
import stats_model as m

ROOT = cpulibs.ROOT

EXAMPLE = ["hello", "World 42", None, "", "héllo"]
EXAMPLE_FIGURES = dict(total_strings=5, total_nulls=1, total_empty=1, unique_strings=5, total_bytes=19, total_chars=18, bytes_avg=3, chars_avg=3,
                       bytes_min=5, bytes_max=8, chars_min=5, chars_max=8, mem_min=9, mem_max=17, mem_avg=11, whitespace_count=1, digits_count=2,
                       uppercase_count=1, lowercase_count=14, bytes_95=0, chars_95=0, mem_95=0)
EXAMPLE_HISTOGRAM = [(" ", 1), ("2", 1), ("4", 1), ("W", 1), ("d", 1), ("e", 1), ("h", 2), ("l", 5), ("o", 3), ("r", 1), ("é", 1)]


def _enc(rows):
    return [None if r is None else r.encode("utf-8", "surrogatepass") for r in rows]


def _example_pairs():
    return [(int.from_bytes(ch.encode(), "big"), n) for ch, n in EXAMPLE_HISTOGRAM]


def test_worked_example_model():
    st, pairs = m.model(_enc(EXAMPLE))
    assert st == EXAMPLE_FIGURES
    assert pairs == _example_pairs() and pairs[-1][0] == 0xC3A9
    assert sum(n for _, n in pairs) == 18
    assert [m.row_mem(r) for r in _enc(EXAMPLE)] == [14, 17, 0, 9, 17]
    assert m.model_from_str(EXAMPLE) == (st, pairs)


def test_model_degenerate_columns():
    st, pairs = m.model([])
    assert not any(st.values()) and pairs == []
    st, pairs = m.model([None] * 9)
    assert st["unique_strings"] == 1 and st["total_nulls"] == 9 and pairs == []
    assert st["bytes_min"] == st["chars_min"] == st["mem_min"] == 0 == st["mem_max"]
    st, pairs = m.model([b""] * 9)
    assert st["mem_min"] == st["mem_max"] == 9 and st["total_empty"] == 9 and st["unique_strings"] == 1 and st["bytes_min"] == 0


def test_model_over_bytes_agrees_with_model_over_str():
    rows = m.text_rows(20_000, seed=5)
    assert any(r is not None and any(ord(ch) > 0xFFFF for ch in r) for r in rows)
    assert m.model(_enc(rows)) == m.model_from_str(rows)


def test_model_histogram_edges():
    st, pairs = m.model(m.edge_rows())
    listed = {p for p, _ in pairs}
    for cp in (0x7F, 0x80, 0x7FF, 0x800, 0xFFFF):
        assert m.packed(cp) in listed, hex(cp)
    assert 0 not in listed and all(p <= 0xEFBFBF for p in listed)  # U+0000 and everything above U+FFFF: never listed
    assert dict(pairs)[m.packed(0xFFFF)] == 5
    # counted in chars all the same
    assert st["total_chars"] == sum(m.count_chars(r) for r in m.edge_rows() if r is not None)
    assert m.model([b"\0\0x\0"])[0]["total_chars"] == 4 and m.model([b"\0\0x\0"])[1] == [(ord("x"), 1)]
    assert m.model(["\U00010000".encode()])[0]["total_chars"] == 1 and m.model(["\U00010000".encode()])[1] == []


# ---- the harness (stats_ops.h) against the model ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


def _same(harness, rows):
    got, want = harness.figures(rows), m.model(rows)
    bad = [k for k in want[0] if got[0][k] != want[0][k]]
    assert not bad, [(k, got[0][k], want[0][k]) for k in bad]
    assert got[1] == want[1]
    per_row, _ = harness.run(rows)
    chars = [0 if r is None else m.count_chars(r) for r in rows]  # (cs_len's rule, row by row)
    assert per_row[:, 0].tolist() == chars
    assert per_row[:, 1].tolist() == [m.row_mem(r) for r in rows]


def test_harness_worked_example(harness):
    got = harness.figures(_enc(EXAMPLE))
    assert got[0] == EXAMPLE_FIGURES and got[1] == _example_pairs()


def test_harness_matches_model_on_text(harness):
    _same(harness, _enc(m.text_rows(200_000, seed=3)))


def test_harness_matches_model_on_malformed_bytes(harness):
    _same(harness, m.malformed_rows() + [None, b""])
    for r in m.malformed_rows():  # each row alone: its own characters, nothing of a neighbour
        _same(harness, [r])
    _same(harness, m.random_bytes_rows(100_000, seed=4))


def test_harness_histogram_edges(harness):
    rows = m.edge_rows()
    _same(harness, rows)
    _, hist = harness.run(rows)
    for cp in (0x7F, 0x80, 0x7FF, 0x800, 0xFFFF):
        assert hist[cp] > 0, hex(cp)
    assert hist[0] == 3 + 2  # (U+0000 is counted; the compaction leaves it out)
    one = harness.figures(["\U00010000".encode()])
    assert one[0]["total_chars"] == 1 and one[1] == [] and not any(one[0][k] for k in ("whitespace_count", "digits_count", "uppercase_count", "lowercase_count"))


# ---- relink: a caller of compute_statistics, compiled against the reference's headers ----------------------------------------
CALLER = r"""
#include "NVStrings.h"
#include "StringsStatistics.h"
void calls(NVStrings* s, StringsStatistics& st) { s->compute_statistics(st); }
"""
REF_INCLUDE = "/root/reference/cpp/include"
SYMBOLS = os.path.join(ROOT, "tests", "golden", "relink_stats_symbols.json")


def caller_symbols(include_dir):
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "caller.cpp"), os.path.join(d, "caller.o")
        open(src, "w").write(CALLER)
        subprocess.run(["g++", "-std=c++14", "-c", "-I", include_dir, src, "-o", obj], check=True)
        out = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
        return sorted({ln.split()[-1] for ln in out.splitlines() if "NVStrings" in ln})


def wanted_symbols():
    with open(SYMBOLS) as f:
        return json.load(f)["symbols"]


def test_recorded_symbol_matches_reference_headers():
    assert len(wanted_symbols()) == 1
    if not os.path.isdir(REF_INCLUDE):
        pytest.skip("the reference headers are not on this machine")
    assert caller_symbols(REF_INCLUDE) == wanted_symbols()


def test_our_headers_give_the_recorded_symbol():
    assert caller_symbols(os.path.join(ROOT, "include", "nvstrings")) == wanted_symbols()


def test_struct_layout_matches_reference_headers():
    """field names and order: a program that prints every field's offset, built against either header"""
    if not os.path.isdir(REF_INCLUDE):
        pytest.skip("the reference headers are not on this machine")
    fields = ("total_bytes total_chars bytes_avg bytes_max bytes_min bytes_95 chars_avg chars_max chars_min chars_95 total_memory mem_avg "
              "mem_max mem_min mem_95 total_strings total_nulls total_empty unique_strings whitespace_count digits_count uppercase_count "
              "lowercase_count char_counts").split()
    prog = '#include <cstdio>\n#include <cstddef>\n#include "StringsStatistics.h"\nint main() {\n' + \
        "".join('  printf("%s %%zu\\n", offsetof(StringsStatistics, %s));\n' % (f, f) for f in fields) + \
        '  printf("size %zu\\n", sizeof(StringsStatistics));\n}\n'
    outs = []
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.cpp"), os.path.join(d, "layout")
        open(src, "w").write(prog)
        for inc in (REF_INCLUDE, os.path.join(ROOT, "include", "nvstrings")):
            subprocess.run(["g++", "-std=c++14", "-Wno-invalid-offsetof", "-I", inc, src, "-o", exe], check=True)
            outs.append(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert outs[0] == outs[1] and "char_counts 184" in outs[0]


def test_member_relinks_against_libnvstrings():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host"), "libs"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "custrings_amd", "libNVStrings.so")],
                         capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not (set(wanted_symbols()) - have), sorted(set(wanted_symbols()) - have)


# ---- the pyni glue name and the Python surface ------------------------------------------------------------------------------
def test_pyni_name_is_what_the_reference_python_calls():
    with open(os.path.join(ROOT, "tests", "golden", "reference_python_calls.json")) as f:
        assert '"n_get_info"' in json.dumps(json.load(f))


def test_pyni_exports_n_get_info():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host")], check=True)
    code = "import pyniNVStrings as P; print(hasattr(P, 'n_get_info'))"
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "custrings_amd") + os.pathsep + ROOT)
    out = subprocess.run(["python3", "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "True"


def test_python_surface():
    import inspect

    import nvstrings as top
    from custrings_amd import nvstrings as N

    assert callable(N.get_info) and "get_info" not in N.__all__ and "get_info" not in N._NOT_BUILT
    # handed out by __getattr__, bound to the instance: no member of the class (tests/test_gpu_metadata.py lists those)
    assert not hasattr(N.nvstrings, "get_info") and not hasattr(top.nvstrings, "get_info")
    assert "get_info" not in {n for n, _ in inspect.getmembers(N.nvstrings, inspect.isfunction)}
    s = N.nvstrings(0, own=False)
    assert hasattr(s, "get_info") and callable(s.get_info)
    assert s.get_info.func is N.get_info and s.get_info.args == (s,)
    with pytest.raises(AttributeError):
        s.no_such_member
    assert set(m.INFO_OF) | {"device_memory", "chars_histogram"} == set(m.INFO_KEYS) and len(m.INFO_KEYS) == 21
