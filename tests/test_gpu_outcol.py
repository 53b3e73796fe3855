"""The shared host tail that turns per-row lengths into an output column (cs_internal.h: Built), once per converted
family at the row counts where it can go wrong -- 1, the 256-row workgroup of the size kernels and of blocks_for, the
2048-length chunk of the offsets scan, each with its neighbours -- on columns of nulls only, of empty rows only (no
chars at all) and with a null in the last row (the tail bits of the last validity word).  Results against the oracle
and the pad model, the families' own references; the null count of every result, and int32 offsets where promised."""
import contextlib
import functools

import pytest

import engines
import gpuutil
import pad_model

pytestmark = pytest.mark.gpu

ROWS = [1, 255, 256, 257, 2047, 2048, 2049]
CONTENTS = ["all-null", "all-empty", "null-last"]
EVERY = pytest.mark.parametrize("content", CONTENTS)
EVERY_N = pytest.mark.parametrize("n", ROWS)

IP = r"\d+\.\d+"
GROUPS = r"(\d+)\.(\d+)"


def rows_of(n, content):
    if content == "all-null":
        return [None] * n
    if content == "all-empty":
        return [""] * n
    # (words, digits, an accent, spaces either end; every seventh row empty, the last one null)
    rows = ["" if i % 7 == 3 else "  Ab%d 10.%d.%d xé aeiou " % (i % 5, i % 251, i % 3) for i in range(n)]
    rows[-1] = None
    return rows


@functools.lru_cache(maxsize=None)
def oracle():
    return engines.OracleEngine()


@functools.lru_cache(maxsize=None)
def column(n, content):
    from custrings_amd import nvstrings

    rows = rows_of(n, content)
    return rows, nvstrings.to_device(rows)


@contextlib.contextmanager
def switched(*names):
    L = gpuutil.lib()
    for v in names:
        L.check(L.lib.cs_config_set(v.encode(), b"1"))
    try:
        yield
    finally:
        for v in names:
            L.check(L.lib.cs_config_set(v.encode(), None))


def route():
    return gpuutil.lib().lib.cs_debug_last_route().decode()


def same(g, want, what, width=None):
    L = gpuutil.lib()
    assert g.to_host() == want, what
    assert int(L.lib.cs_column_null_count(g.m_cptr)) == sum(r is None for r in want), what + ": null count"
    if width:
        assert int(L.lib.cs_column_offset_width(g.m_cptr)) == width, what + ": offset width"


def same_columns(gcols, wcols, what, width=None):
    assert len(gcols) == len(wcols), what + ": column count"
    for k, (g, w) in enumerate(zip(gcols, wcols)):
        same(g, w, "%s: column %d" % (what, k), width)


@EVERY
@EVERY_N
def test_case_strip_and_two_pass(n, content):
    rows, g = column(n, content)
    o = oracle()
    same(g.lower(), o.lower(rows), "lower")
    same(g.strip(), o.strip(rows), "strip")
    with switched("CS_STRIP_ROWWISE"):
        same(g.strip(), o.strip(rows), "strip, row-wise")
    with switched("CS_REPLACE_ROWWISE"):  # (the literal replace on its own size / write kernels: two_pass)
        same(g.replace("b", "BBB", regex=False), o.replace(rows, "b", "BBB"), "replace")


@EVERY
@EVERY_N
def test_pad_family(n, content):
    rows, g = column(n, content)
    for op, args, got in (("slice", [1, 6], g.slice(1, 6)), ("repeat", [3], g.repeat(3))):
        same(got, [pad_model.apply(op, r, args) for r in rows], op)


@EVERY
@EVERY_N
def test_replace_re_routes(n, content):
    rows, g = column(n, content)
    o = oracle()
    with switched("CS_REGEX_TWO_PASS"):
        same(g.replace(IP, "<ip>"), o.replace_re(rows, IP, "<ip>"), "replace_re, two-pass")
    with switched("CS_CLASS_RUNS_ALWAYS"):
        got = g.replace("[aeiou]+", "*")
        if content == "null-last" and n > 1:
            assert route() == "runs"
        same(got, o.replace_re(rows, "[aeiou]+", "*"), "replace_re, class runs")
    want = o.replace_with_backrefs(rows, GROUPS, r"\2-\1")
    same(g.replace_with_backrefs(GROUPS, r"\2-\1"), want, "replace_with_backrefs")
    with switched("CS_BACKREFS_TWO_PASS"):
        same(g.replace_with_backrefs(GROUPS, r"\2-\1"), want, "replace_with_backrefs, two-pass")
    same(g.replace_multi([r"\d+", "é"], ["#", "e"]), o.replace_multi(rows, [r"\d+", "é"], ["#", "e"]), "replace_re, two patterns")


@EVERY
@EVERY_N
def test_extract_and_findall(n, content):
    rows, g = column(n, content)
    o = oracle()
    same_columns(g.extract(GROUPS), o.extract(rows, GROUPS), "extract")
    same_columns(g.findall(r"\d+"), o.findall(rows, r"\d+"), "findall")
    with switched("CS_REGEX_ROWWISE"):  # (spans by a thread a row, lengths scanned with the validity fused in)
        same_columns(g.extract(GROUPS), o.extract(rows, GROUPS), "extract, row-wise")
        same_columns(g.findall(r"\d+"), o.findall(rows, r"\d+"), "findall, row-wise")


@EVERY
@EVERY_N
def test_tokens_ngrams_split(n, content):
    from custrings_amd import nvtext

    rows, g = column(n, content)
    o = oracle()
    want = o.tokenize(rows)
    if content != "null-last":
        assert want == []  # no token anywhere: a column of no rows
    same(nvtext.tokenize(g), want, "tokenize")
    with switched("CS_TOKENIZE_ROWWISE"):
        same(nvtext.tokenize(g), want, "tokenize, row-wise")
    same(nvtext.ngrams(g, 2, "_"), o.ngrams(rows, 2, "_"), "ngrams")  # (null and empty rows are dropped: the row-wise tail)
    # split promises int32 offsets for columns below 2 GiB; a column of nulls only splits into one all-null column
    width = 4 if content == "null-last" and n > 1 else None
    same_columns(g.split(" "), o.split(rows, " "), "split", width)
    with switched("CS_SPLIT_GENERIC"):
        same_columns(g.split(" "), o.split(rows, " "), "split, row-wise")


@EVERY
@EVERY_N
def test_category_keys_concat_records(n, content):
    from custrings_amd import nvcategory, nvstrings

    rows, g = column(n, content)
    o = oracle()
    same(nvcategory.from_strings(g).keys(), o.category(rows)[0], "category keys")
    other = ["tail", None, ""]
    same(g.add_strings(nvstrings.to_device(other)), rows + other, "concat")
    flat, loff = g.extract_record(GROUPS, flat=True)
    want = o.extract_record(rows, GROUPS)
    same(flat, [x for rec in want for x in rec], "extract_record")
    assert loff.tolist() == [2 * r for r in range(n + 1)]
    flat, loff = g.findall_record("@@", flat=True)  # no match in any row: a records column of no rows
    assert flat.size() == 0 and not loff.any()
    same(flat, [], "findall_record without a match")


def test_metadata_from_the_scan_serves_a_tile_op():
    """concat and the records entry now take the longest row and the largest 64-row span from their scan, as the other
    ops do: a tile-route op on their output plans its tiles from them and computes what the model does"""
    rows, g = column(2049, "null-last")
    both = g.add_strings(g)
    flat, _ = g.findall_record(r"\w+", flat=True)
    for col, want in ((both, rows + rows), (flat, [x for rec in oracle().findall_record(rows, r"\w+") for x in rec])):
        got = col.slice(1, 6)
        assert route() == "tile"
        same(got, [pad_model.apply("slice", r, [1, 6]) for r in want], "slice of the output")
