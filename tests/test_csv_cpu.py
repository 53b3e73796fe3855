"""from_csv without a GPU: the Python model (tests/csv_model.py) against the reference's known answers and the documented
quirks; csv_ops.h (the text the kernels compile) behind a sequential line scan, built with g++ and the address /
undefined-behaviour sanitizers and run as a child process, against the model on about 200k generated lines; the relink of
NVStrings::create_from_csv; the pyni name the reference's Python layer calls; the public API."""
import json
import os
import subprocess
import tempfile

import pytest

import cpulibs
import csv_model as m

ROOT = cpulibs.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden")


def cases():
    with open(os.path.join(GOLDEN, "reference_csv.json")) as f:
        return json.load(f)["cases"]


def case_bytes(case):
    if "file" in case:
        with open(os.path.join(GOLDEN, case["file"]), "rb") as f:
            return f.read()
    return case["text"].encode()


def col(text, column=0, lines=0, flags=0):
    return m.from_csv_buffer(text, column, lines, flags)


# ---- the model against the known answers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases(), ids=lambda c: c["src"].split("/")[-1])
def test_model_reproduces_known_answers(case):
    got = col(case_bytes(case), case["column"], case["lines"], case["flags"])
    want = [e.encode() for e in case["expected"]]
    assert got[:case.get("first", len(want))] == want and (len(got) == len(want) or "first" in case), case["src"]


def test_fixture_file_is_what_the_issue_describes():
    with open(os.path.join(GOLDEN, "tweets_head.csv"), "rb") as f:
        head = f.read()
    assert head.count(b"\n") == 64 and b"\r" not in head and b"\0" not in head and b'""' in head and len(head) < 16 * 1024
    assert len(col(head, 7)) == 63 and None not in col(head, 7)


# ---- quirks, one assertion each ------------------------------------------------------------------------------------------------
def test_crlf_is_one_line_end():
    assert col(b"h\r\na\r\nb\r\n") == [b"a", b"b"]


def test_lf_cr_lf_is_one_line_end():
    assert col(b"h\na\n\r\nb\n") == [b"a", b"b"]


def test_tabs_behind_a_terminator_are_skipped():
    assert col(b"h\na\n\t\tb\n") == [b"a", b"b"]


def test_a_tab_inside_a_line_is_kept():
    assert col(b"h\na\tb\tc\n") == [b"a\tb\tc"]


def test_quote_then_content_behind_the_closing_quote():
    assert col(b'h\n"abc"def,x\n') == [b'abc"de']


def test_doubled_quotes_stay():
    assert col(b'h\n"a ""b"" c",x\n') == [b'a ""b"" c']


def test_a_quote_behind_content_opens_no_field():
    assert col(b'h\nab"c,d",e\n') == [b'ab"']  # (three bytes counted, a b c; the quote stays in the span, so the c falls off the end; the comma ends the field)


def test_a_comma_inside_quotes():
    assert col(b'h\nx,"a,b",y\n', 1) == [b"a,b"]


def test_too_few_columns_runs_into_the_skipped_bytes():
    assert col(b"h\r\na,b\r\nc,d,e\r\n", 2) == [b"\n", b"e"]


def test_column_zero():
    assert col(b"h\na,b,c\n", 0) == [b"a"]


def test_column_last():
    assert col(b"h\na,b,c\n", 2) == [b"c"]


def test_column_past_last():
    assert col(b"h\na,b,c\nd\n", 3) == [None, b"\r"]  # (the second row's walk ends in the '\r' the loader appends)


def test_an_empty_field_is_null():
    assert col(b"h\na,,c\n", 1) == [None]


def test_an_empty_field_is_empty_with_flag_8():
    assert col(b"h\na,,c\n", 1, flags=m.NULL_IS_EMPTY) == [b""]


def test_lines_one():
    assert col(b"h\na\nb\nc\n", lines=1) == [b"a"]


def test_lines_equal_to_rows():
    assert col(b"h\na\nb\nc\n", lines=3) == [b"a", b"b", b"c"]


def test_lines_beyond_rows():
    assert col(b"h\na\nb\nc\n", lines=9) == [b"a", b"b", b"c"]


def test_a_nul_drops_the_tail():
    assert col(b"h\na\nb\0c\nd\n") == [b"a"]  # (the partial line in front of the NUL has no line end: no row)


def test_no_terminator_before_a_nul_is_empty():
    assert col(b"abc\0\nd\n") == []


@pytest.mark.parametrize("data", [b"", b"x"])
def test_a_file_below_two_bytes_is_none(data, tmp_path):
    p = tmp_path / "tiny.csv"
    p.write_bytes(data)
    assert m.from_csv(str(p), 0) is None


def test_a_missing_file_is_none(tmp_path):
    assert m.from_csv(str(tmp_path / "none.csv"), 0) is None


def test_high_bytes_pass_through():
    assert col(b"h\n\xff\x80,\xc3\xa9\n", 1) == [b"\xc3\xa9"]


def test_last_line_without_a_terminator_is_a_row():
    assert col(b"h\na") == [b"a"]


def test_sort_flags():
    text = b"h\nbb\n\nc\n,\nab\n"
    assert col(text, flags=m.SORT_NAME) == [None, b"ab", b"bb", b"c"]
    assert col(text, flags=m.SORT_LENGTH) == [None, b"c", b"bb", b"ab"]
    assert col(text, flags=m.SORT_LENGTH | m.SORT_NAME) == [None, b"c", b"ab", b"bb"]


# ---- the harness (csv_ops.h) against the model ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    with tempfile.TemporaryDirectory() as d:
        yield m.Harness(d, ROOT)


LINES = 200_000
COLUMNS = [0, 1, 3]


@pytest.fixture(scope="module")
def generated():
    per = LINES // len(COLUMNS)
    return m.gen_buffers(per - 8000, seed=5) + [m.gen_lines(4000, seed=6, shape="mixed"), m.gen_lines(2000, seed=7, shape="tweets"),
                                                 m.gen_lines(2000, seed=8, shape="log")]


def test_harness_reproduces_known_answers(harness):
    for case in cases():
        got = harness.run([case_bytes(case)], case["column"], case["lines"], case["flags"])[0]
        want = [e.encode() for e in case["expected"]]
        assert got[:len(want)] == want, case["src"]


def test_generated_files_hold_what_the_walk_must_survive(generated):
    blob = b"".join(generated)
    for needle in (b'"', b",", b"\r", b"\n", b"\t", b"\x01", b"\r\n", b'""', b"\xff"):
        assert blob.count(needle) > 1000, needle
    assert sum(b"\0" in g for g in generated) >= 50  # (a file ends at its first NUL: a few per file, in many files)
    assert sum(len(m.line_starts(g)) for g in generated) * len(COLUMNS) > LINES * 0.9


@pytest.mark.parametrize("column", COLUMNS)
@pytest.mark.parametrize("flags", [0, m.NULL_IS_EMPTY])
def test_harness_matches_model_on_generated_lines(harness, generated, column, flags):
    got = harness.run(generated, column, 0, flags)  # (the starts by 16-byte pieces against the sequential scan: its own exit code)
    nulls = quoted = 0
    for g, data in zip(got, generated):
        spans = m.spans_of(data)
        want = [m.field_of(s, column, bool(flags)) for s in spans]
        assert g == [w[0] for w in want], (column, flags, data[:80])
        nulls += sum(w[0] is None or w[0] == b"" for w in want)
        quoted += sum(w[1] for w in want)
    assert nulls >= 1000, nulls  # (rows whose field is empty: null rows without flag 8)
    assert quoted >= 1000, quoted


@pytest.mark.parametrize("lines", [1, 7, 10 ** 6])
def test_harness_matches_model_with_a_lines_limit(harness, generated, lines):
    few = generated[:20] + generated[-3:]
    got = harness.run(few, 1, lines, 0)
    assert got == [m.from_csv_buffer(d, 1, lines) for d in few]


# ---- relink: a caller of the member, compiled against the reference's headers ------------------------------------------------
CALLER = r"""
#include "NVStrings.h"
NVStrings* calls(const char* path) { return NVStrings::create_from_csv(path, 7, 100, NVStrings::name, true); }
"""
REF_INCLUDE = "/root/reference/cpp/include"
SYMBOLS = os.path.join(GOLDEN, "relink_csv_symbols.json")


def wanted_symbols():
    with open(SYMBOLS) as f:
        return json.load(f)["symbols"]


def caller_symbols(include_dir):
    with tempfile.TemporaryDirectory() as d:
        src, obj = os.path.join(d, "caller.cpp"), os.path.join(d, "caller.o")
        open(src, "w").write(CALLER)
        subprocess.run(["g++", "-std=c++14", "-c", "-I", include_dir, src, "-o", obj], check=True)
        out = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout
        return sorted({ln.split()[-1] for ln in out.splitlines() if "NVStrings" in ln})


def test_recorded_symbol_matches_reference_headers():
    assert len(wanted_symbols()) == 1
    if not os.path.isdir(REF_INCLUDE):
        pytest.skip("the reference headers are not on this machine")
    assert caller_symbols(REF_INCLUDE) == wanted_symbols()


def test_our_headers_give_the_recorded_symbol():
    assert caller_symbols(os.path.join(ROOT, "include", "nvstrings")) == wanted_symbols()


def test_create_from_csv_relinks_against_libnvstrings():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host"), "libs"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "custrings_amd", "libNVStrings.so")],
                         capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not (set(wanted_symbols()) - have)


# ---- the pyni glue name and the public API -------------------------------------------------------------------------------------
def test_pyni_name_is_what_the_reference_python_calls():
    with open(os.path.join(GOLDEN, "reference_python_calls.json")) as f:
        assert '"n_createFromCSV"' in json.dumps(json.load(f))


def test_pyni_exports_n_createFromCSV():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "custrings_amd", "host")], check=True)
    code = "import pyniNVStrings as P; print(hasattr(P, 'n_createFromCSV'))"
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "custrings_amd") + os.pathsep + ROOT)
    out = subprocess.run(["python3", "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "True"


def test_c_abi_declares_the_entry_points():
    from custrings_amd import _lib

    for n in ("cs_column_from_csv", "cs_column_from_csv_buffer", "cs_csv_tile_bytes"):
        assert n in _lib._PROTOS and hasattr(_lib.lib, n), n
    assert _lib.lib.cs_csv_tile_bytes() > 0 and _lib.lib.cs_csv_tile_bytes() % 16 == 0


def test_python_api_has_from_csv():
    import sys

    from custrings_amd import nvstrings as N

    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import nvstrings as top

    for n in ("from_csv", "from_csv_buffer"):
        assert callable(getattr(N, n)) and callable(getattr(top, n)), n
