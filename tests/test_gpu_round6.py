"""Round 6: the buffer pool's size classes (no hipMalloc for a column a little larger than the last one), regression
tests for the two malformed-UTF-8 parity bugs the round-5 soak found, a fixed-seed slice of tools/soak_gpu.py inside
the suite -- once per forced regex route, the ORACLE as the witness on valid UTF-8 / ASCII columns and the row-wise
kernels on arbitrary bytes --, rows beyond 93 bytes on the fast split / regex forms."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import cpulibs
import engines
import gpuutil

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IPV4 = r"\d+\.\d+\.\d+\.\d+"


def last_route():
    return gpuutil.lib().lib.cs_debug_last_route().decode()


def blob_of(pat):
    b = engines.reference_blob(pat)
    return np.ascontiguousarray(b if b is not None else engines.product_blob(pat), dtype=np.int32)


def col_of(rows):
    chars = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return cpulibs.Col(chars, offs, None)


_soak = None


def soak():
    """tools/soak_gpu.py as a module (its column generator, op snapshot and oracle leg are the suite's too)."""
    global _soak
    if _soak is None:
        spec = importlib.util.spec_from_file_location("soak_gpu", os.path.join(ROOT, "tools", "soak_gpu.py"))
        _soak = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_soak)
    return _soak


# ---- the buffer pool (reference: the RMM pool behind device_alloc, cpp/src/util.inl:90-106) ----------------------------

def test_gpu_pool_serves_columns_of_slightly_different_sizes():
    """The headline step on five columns whose sizes differ by up to +-1 % (other seeds, other row counts): after the first
    column every buffer -- the column's own and all 21 outputs -- comes out of the pool (cs_core.hip: size_class: 3 % of
    headroom, eight classes an octave).  Until round 5 a column a few KB larger than the last one paid a hipMalloc per
    buffer (120-134 ms at 100M rows: VERDICT r05 missing 4)."""
    L = gpuutil.lib()
    from custrings_amd import nvstrings

    re = gpuutil.compile_re(IPV4)

    def step(rows, seed):
        g = gpuutil.synth(3, 0, rows, seed=seed)
        cols = g.split(" ")
        o = C.c_void_p()
        L.check(L.lib.cs_replace_re(g.m_cptr, re, b"<IP>", -1, None, C.byref(o)))
        out = nvstrings.nvstrings(o.value)
        n = (len(cols), out.size())
        del cols, out, g
        return n

    base = 3_000_000
    try:
        step(int(base * 1.01), 11)  # (the largest first: what the pool holds afterwards serves every smaller request within 20 %)
        m0 = int(L.lib.cs_debug_malloc_count())
        L.check(L.lib.cs_config_set(b"CS_POOL_TRACE", b"1"))  # (a miss says which request it was, on stderr)
        for i, f in enumerate((0.99, 1.0, 0.995, 1.008, 1.01)):
            step(int(base * f), 12 + i)
        assert int(L.lib.cs_debug_malloc_count()) == m0, "a column within 1 %% of the last one allocated %d new block(s)" % (int(L.lib.cs_debug_malloc_count()) - m0)
        # growing by 2 % a step: the headroom of a class (3 %) absorbs a step, a new class is entered at most every second step
        m0 = int(L.lib.cs_debug_malloc_count())
        rows = base
        for i in range(6):
            rows = int(rows * 1.02)
            step(rows, 30 + i)
        grown = int(L.lib.cs_debug_malloc_count()) - m0
        assert grown <= 3 * 70, "growing columns: %d allocations" % grown  # (about 66 buffers a step; at most every second step allocates)
    finally:
        L.lib.cs_regex_destroy(re)
        L.check(L.lib.cs_config_set(b"CS_POOL_TRACE", None))
    assert int(L.lib.cs_pool_cached_bytes()) > 0
    L.check(L.lib.cs_pool_trim(0))
    assert int(L.lib.cs_pool_cached_bytes()) == 0


# ---- malformed UTF-8: what the round-5 soak found ------------------------------------------------------------------------

LEAD_ROWS = [b"4\xc3b", b"ab b", b"\xc3b", b"b\xc3", b"a\xe2bb", b"\xf0abcb", b"\xc3\xa9b", b"b\x80b", b"\xe2\x82b ab", b"4\xc3b" * 9, b"", b"b"]
# what the reference's executor sees (regexec.inl:204-442 walks custring_view::iterator, whose operator++ advances by the
# LEAD byte's width -- custring_view.inl:48-57,361-366 -- so the bytes behind a lead are swallowed whatever they are; a stray
# continuation byte has width 0 there, the product treats it as a character of its own): matches of b|ab per row
LEAD_COUNTS = [0, 2, 0, 1, 0, 1, 1, 2, 1, 0, 0, 1]


def test_gpu_unit_route_lead_byte_swallows_the_ascii_byte_behind_it():
    """count_re / contains_re / replace_re of `b|ab` (a unit-route program) on rows where a lead byte >= 0xC0 stands without its
    continuation bytes: the byte behind it belongs to the 'character' and is no match.  Round 5's last soak (seed 70058) found
    the unit route counting the `b` of `4\\xc3b`: its whole-character check ran only for patterns that look flags up
    (regex_stream.h: reclassify_high; fix 35b5107, which landed without a test)."""
    L = gpuutil.lib()
    pat = r"b|ab"
    re = gpuutil.compile_re(pat)
    rng = np.random.default_rng(70058)
    filler = [bytes(rng.choice(list(b"ab4 .x"), int(rng.integers(0, 60))).astype(np.uint8)) for _ in range(4000)]
    # the malformed rows in the middle of plain ones (the tile's other rows stay on the fast form) and in tiles of their own
    rows = filler[:1000] + LEAD_ROWS + filler[1000:2000] + LEAD_ROWS * 20 + filler[2000:]
    col = col_of(rows)
    g = gpuutil.from_col(col)
    try:
        cnt = np.zeros(col.rows, dtype=np.int32)
        found = C.c_int64()
        L.check(L.lib.cs_count_re(g.m_cptr, re, cnt.ctypes.data, 0, None, C.byref(found)))
        assert last_route() in ("units", "bits", "chain", "plain"), last_route()
        got_rep = gpuutil.to_col(g.replace(pat, "_"))
        got_has, _ = gpuutil.bools(g, "cs_contains_re", re)
        # witness 1: the hand-derived counts of the explicit rows
        assert cnt[1000:1000 + len(LEAD_ROWS)].tolist() == LEAD_COUNTS
        assert (got_has[1000:1000 + len(LEAD_ROWS)] != 0).tolist() == [c > 0 for c in LEAD_COUNTS]
        # witness 2: the row-wise kernels on the whole column
        for v in ("CS_REGEX_ROWWISE", "CS_REGEX_TWO_PASS"):
            L.check(L.lib.cs_config_set(v.encode(), b"1"))
        try:
            cnt2 = np.zeros(col.rows, dtype=np.int32)
            L.check(L.lib.cs_count_re(g.m_cptr, re, cnt2.ctypes.data, 0, None, C.byref(found)))
            want_rep = gpuutil.to_col(g.replace(pat, "_"))
            want_has, _ = gpuutil.bools(g, "cs_contains_re", re)
        finally:
            for v in ("CS_REGEX_ROWWISE", "CS_REGEX_TWO_PASS"):
                L.check(L.lib.cs_config_set(v.encode(), None))
        assert np.array_equal(cnt, cnt2), np.flatnonzero(cnt != cnt2)[:8]
        assert np.array_equal(got_has, want_has)
        assert got_rep.same_as(want_rep)
        # witness 3: the oracle on the rows that ARE valid UTF-8 (the reference's contract)
        valid = [i for i, r in enumerate(rows) if _is_utf8(r)]
        ocnt, _ = cpulibs.Oracle().count_re(col, blob_of(pat))
        assert np.array_equal(cnt[valid], ocnt[valid])
    finally:
        L.lib.cs_regex_destroy(re)


def _is_utf8(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def test_gpu_soak_seed_70058_and_its_neighbours():
    """The soak column that exposed the unit-route bug, and the class-runs one (findall([a-c]+) on random bytes), replayed."""
    s = soak()
    bad = 0
    for seed in (70058, 70056):
        bad += s.check_column(seed, pats=[(r"b|ab", ""), (r"[a-c]+", "xyz__"), (r"(a|b)c", "-"), (r"\w+", "<w>")], regex_only=True, category=False)
    assert bad == 0


# ---- a slice of the soak inside the suite, once per forced route -----------------------------------------------------------

ROUTE_SLICES = {
    # forced switches, (pattern, replacement) pairs the route converts, seeds: [valid UTF-8 (oracle), ASCII (oracle), arbitrary bytes (row-wise)]
    "default": ((), None, (21 + 28 * 3, 9 + 28 * 5, 3 + 28 * 7)),
    "bits": (("CS_BITS_ALWAYS",), [(r"(\bab\b)|(\bc\b)|(\bxyz\b)", "="), (r"[abc1]+", "*"), (r"ab|a1|bc", "#"), (r"x?y?z", "Q"), (r"b|ab", ""), (r"\d\.|\.\d", "~")],
             (22 + 28 * 2, 7 + 28 * 4, 0 + 28 * 6)),
    "class-runs": (("CS_CLASS_RUNS_ALWAYS",), [(r"[a-c]+", "xyz__"), (r"\w+", "<w>"), (r"\S+", "s"), (r"[^\w]", "_"), (r".", "?"), (r"\d", "9"), (r"[^ ]+", "_")],
                   (27 + 28 * 1, 10 + 28 * 2, 34 + 28 * 3)),
    "chain-tables-in-memory": (("CS_CHAIN_TABLES_IN_MEMORY",), [(IPV4, "<IP>"), (r"\b\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}\b", "<IP>"), (r"[a-c]+=>", ""), (r"\d+\.\d+ ", "<n>"),
                                                                (r"\b\d+\.\d+\b", ""), (r"\d+\.\d{2}\.\d+", "#")],
                               (23 + 28 * 9, 8 + 28 * 3, 5 + 28 * 2)),
}


@pytest.mark.parametrize("route", sorted(ROUTE_SLICES))
def test_gpu_soak_slice(route):
    """tools/soak_gpu.py, fixed seeds, inside the suite: the fast kernels with one regex route forced
    against the CPU oracle on the columns of valid UTF-8 / ASCII text and against the row-wise kernels on every column
    (the only witness on arbitrary bytes: the reference is undefined there).  The default slice runs every op of the path."""
    s = soak()
    assert s.ORC is not None, "the oracle library is the witness of this test"
    forced, pats, seeds = ROUTE_SLICES[route]
    bad = 0
    lines = []
    for seed in seeds:
        bad += s.check_column(seed, pats=pats, regex_only=pats is not None, max_rows=6000, forced=forced, category=pats is None, log=lines.append)
    assert bad == 0, lines[:10]


# ---- rows beyond 93 bytes on the fast split kernels (split.cu:751-816, custring_view.cuh:36-42: any row length) ---------------

def _random_rows(rng, n, lo, hi, tokens_hi=40, alphabet=b"abcdefghijklmnop0123456789.-_/", wide=("é", "€", "😀", "ß")):
    """rows of lo..hi BYTES: words of 1..12 characters joined by single spaces (now and then two, or a leading / trailing one)."""
    wide_b = [w.encode() for w in wide]
    out = []
    for _ in range(n):
        target = int(rng.integers(lo, hi + 1))
        parts, size, toks = [], 0, 0
        while size < target and toks < tokens_hi:
            k = int(rng.integers(1, 13))
            if rng.random() < 0.08:
                w = b"".join(wide_b[int(i)] for i in rng.integers(0, len(wide_b), max(1, k // 3)))
            else:
                w = bytes(rng.choice(list(alphabet), k).astype(np.uint8))
            sep = b"  " if rng.random() < 0.05 else b" "
            parts.append(w + sep)
            size += len(w) + len(sep)
            toks += 1
        row = b"".join(parts)[:target]
        if rng.random() < 0.05:
            row = b" " + row[:-1] if row else row
        out.append(row)
    return out


def _with_nulls(rows, rng, share=0.02):
    col = col_of(rows)
    keep = rng.random(len(rows)) >= share
    keep[-8:] = True  # (the rows a test appends by hand stay)
    lens = np.array([len(r) if k else 0 for r, k in zip(rows, keep)], dtype=np.int64)
    chars = np.frombuffer(b"".join(r for r, k in zip(rows, keep) if k), dtype=np.uint8).copy()
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return cpulibs.Col(chars, offs, np.packbits(keep, bitorder="little"))


@pytest.mark.parametrize("lo,hi,longest,route", [(40, 150, 150, "split-tiles-188"), (0, 170, 188, "split-tiles-188"), (94, 128, 188, "split-tiles-188"),
                                                 (0, 92, 92, "split-tiles-92"), (0, 92, 93, "split-tiles-188"), (60, 120, 189, "split-first-generation")])
def test_gpu_split_rows_beyond_93_bytes_vs_oracle(lo, hi, longest, route):
    """split(' ') on rows of up to 188 bytes -- BASELINE's C5 lengths and the edges of the six-word masks -- through
    k_split_measure2<0, true, 6> + k_split_emit4<.., 6, 8>, against the oracle: every column bit for bit, non-ASCII rows and
    null rows included.  A column whose longest row has 189 bytes keeps the first-generation kernels."""
    rng = np.random.default_rng(9300 + lo + hi + longest)
    rows = _random_rows(rng, 20_000, lo, hi)
    # the longest row, delimiters only (as many tokens as the walk's columns allow), three-byte tokens, an empty row
    rows += [b"x" * longest, b" " * (28 if route == "split-tiles-92" else 60), b"a b" * (min(longest, 186) // 3), b"", b"z" * (longest - 1) + b" "]
    col = _with_nulls(rows, rng)
    g = gpuutil.from_col(col)
    got = g.split(" ")
    assert last_route() == route, last_route()
    want = cpulibs.Oracle().split(col, " ")
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        gpuutil.assert_same(a, b, "split(' ') column %d of %d, rows %d..%d bytes" % (k, len(want), lo, hi))


def test_gpu_split_long_rows_many_columns_and_the_fallbacks():
    """More than 64 tokens in a row (the six-word walk holds 64 columns) or a 64-row span beyond 8 KB: the column leaves the
    tile kernels for the first-generation / row-wise ones -- same columns as the oracle either way."""
    rng = np.random.default_rng(9377)
    orc = cpulibs.Oracle()
    base = _random_rows(rng, 5000, 40, 150)
    for extra, route in (([b"a " * 70], ("split-first-generation", "split-rowwise")),          # 71 tokens in one row
                         ([b"y" * 188] * 64, ("split-first-generation", "split-rowwise", "split-tiles-188")),  # a sub-tile of 12 KB
                         ([b"q " * 32], ("split-tiles-188",))):                                  # 33 columns: beyond the 96-bit kernels' 32
        col = col_of(base[:2000] + extra + base[2000:])
        g = gpuutil.from_col(col)
        got = g.split(" ")
        assert last_route() in route, (last_route(), route)
        want = orc.split(col, " ")
        assert len(got) == len(want)
        for a, b in zip(got, want):
            gpuutil.assert_same(a, b, "split(' ') with %r..." % extra[0][:8])


def test_gpu_split_c5_column_on_the_long_row_kernels():
    """BASELINE's C5 column (tweet-like rows of 40-150 bytes): split(' ') takes the six-word tile kernels and equals the oracle;
    split with a limit and whitespace splitting (96-bit token walker only) still answer through the older kernels."""
    rows = 200_000
    g = gpuutil.synth(5, 0, rows)
    o = cpulibs.Oracle().synth(5, 0, rows)
    got = g.split(" ")
    assert last_route() == "split-tiles-188", last_route()
    want = cpulibs.Oracle().split(o, " ")
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        gpuutil.assert_same(a, b, "C5 split(' ') column %d" % k)
    for d, n in ((" ", 3), (None, -1)):
        got = g.split(d, n)
        want = cpulibs.Oracle().split(o, d, n)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            gpuutil.assert_same(a, b, "C5 split(%r, %d)" % (d, n))



# ---- forms the suite did not reach until round 6 (profiles/r06/kernel_coverage.txt) ----------------------------------------------

def test_gpu_split_with_int64_offsets(monkeypatch):
    """The split tile kernels' int64-offsets forms (a column of 2 GiB or more; CS_SPLIT_OFF64 forces them on a small one):
    k_split_emit4<.., OFF32 = false, ..> in its three walks, against the oracle."""
    monkeypatch.setenv("CS_SPLIT_OFF64", "1")
    orc = cpulibs.Oracle()
    rng = np.random.default_rng(6464)
    for rows_b, delim, n, route in ((_random_rows(rng, 9000, 0, 92), " ", -1, "split-tiles-92"), (_random_rows(rng, 9000, 40, 150), " ", -1, "split-tiles-188"),
                                    (_random_rows(rng, 9000, 0, 92), None, -1, "split-tiles"), (_random_rows(rng, 9000, 0, 92), "  ", -1, "split-tiles"),
                                    (_random_rows(rng, 9000, 0, 92), " ", 3, "split-tiles")):
        col = _with_nulls(rows_b, rng)
        g = gpuutil.from_col(col)
        got = g.split(delim, n)
        assert last_route() == route, (last_route(), route)
        assert all(int(gpuutil.lib().lib.cs_column_offset_width(c.m_cptr)) == 8 for c in got)
        want = orc.split(col, delim, n)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            gpuutil.assert_same(a, b, "split(%r, %d) with int64 offsets" % (delim, n))


@pytest.mark.parametrize("pat,repl", [(IPV4, "<IP>"), (r"(\bab\b)|(\bc\b)", "="), (r"\w+@\w+", "<m>"), (r"#\w+", "<a-longer-tag>")])
def test_gpu_regex_with_the_dfa_tables_in_memory(pat, repl, monkeypatch):
    """A DFA beyond the LDS budget keeps its tables in memory (CS_TDFA_GLOBAL_TABLE forces that for any pattern): replace_re
    then takes the two-pass kernels (the stream forms with the tables in memory left the library in round 6), the scans
    their table-in-memory forms -- all against the oracle."""
    monkeypatch.setenv("CS_TDFA_GLOBAL_TABLE", "1")
    L = gpuutil.lib()
    orc = cpulibs.Oracle()
    blob = blob_of(pat)
    for kind, rows in ((3, 30_011), (5, 20_000)):
        g, o = gpuutil.synth(kind, 0, rows), orc.synth(kind, 0, rows)
        gpuutil.assert_same(g.replace(pat, repl), orc.replace_re(o, blob, repl), "replace_re(%r), tables in memory" % pat)
        re = gpuutil.compile_re(pat)
        try:
            has, n = gpuutil.bools(g, "cs_contains_re", re)
            want_has, want_n = orc.contains_re(o, blob)
            assert np.array_equal(has, want_has) and n == want_n
            cnt = np.zeros(rows, dtype=np.int32)
            found = C.c_int64()
            L.check(L.lib.cs_count_re(g.m_cptr, re, cnt.ctypes.data, 0, None, C.byref(found)))
            want_cnt, _ = orc.count_re(o, blob)
            assert np.array_equal(cnt, want_cnt)
        finally:
            L.lib.cs_regex_destroy(re)
        got = g.findall(pat)
        want = orc.findall(o, blob)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            gpuutil.assert_same(a, b, "findall(%r), tables in memory" % pat)


@pytest.mark.parametrize("pat,repl", [(IPV4, "<IP>"), (r"#\w+", "<tag>"), (r"\w+@\w+", "<m>"), (r"(\bin\b)|(\ba\b)|(\bthe\b)", "="), (r"\d", "##"), (r"[a-z]+ing\b", "")])
def test_gpu_replace_re_on_rows_of_94_to_188_bytes(pat, repl):
    """replace_re on rows beyond the 96-bit masks (BASELINE's C5 lengths; the stream kernel's long-row form on tiles of 32 rows),
    sparse and dense patterns, growing and shrinking replacements, against the oracle -- and no launch gives up."""
    L = gpuutil.lib()
    orc = cpulibs.Oracle()
    blob = blob_of(pat)
    rng = np.random.default_rng(8800)
    rows_b = _random_rows(rng, 30_000, 40, 150, alphabet=b"abcdefghijklmnop0123456789.-_/#@ing the a in") + [b"1.2.3.4 " * 20, b"x" * 188, b"#tag@mail.com " * 13]
    cases = [(gpuutil.synth(5, 0, 150_000), orc.synth(5, 0, 150_000), "C5"), (None, _with_nulls(rows_b, rng), "random long rows")]
    for g, o, what in cases:
        if g is None:
            g = gpuutil.from_col(o)
        f0 = int(L.lib.cs_fallback_count())
        gpuutil.assert_same(g.replace(pat, repl), orc.replace_re(o, blob, repl), "replace_re(%r) on %s" % (pat, what))
        assert int(L.lib.cs_fallback_count()) == f0, "a single-pass kernel gave up"


# ---- rows beyond the masks as PIECES (cs_virtual.hip) -----------------------------------------------------------------------------

# (pattern, replacement, does replace_re take the pieces too?  None: not asserted -- a program that would take the unit scan stays
# on the long-row form when the column's sample holds bytes >= 0x80: cs_regex_pattern.hip, pieces_for)
PIECE_PATTERNS = [(IPV4, "<IP>", True), (r"(\bin\b)|(\ba\b)|(\bthe\b)", "=", None), (r"\w+@\w+", "<m>", None), (r"#\w+", "<a-longer-tag>", True),
                  (r"\b\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}\b", "", True), (r"\d+$", "N", None), (r"[a-z]+ing\b", "ING", None), (r"GET|POST|the", "V", True)]


@pytest.mark.parametrize("pat,repl,replace_on_pieces", PIECE_PATTERNS)
def test_gpu_regex_on_long_rows_as_pieces(pat, repl, replace_on_pieces):
    """A column with rows beyond 93 bytes, a program for which white space is a safe cut (regex_tdfa.cpp: header word 31 bit 25):
    contains_re / count_re / replace_re run on the column's PIECES -- every long row cut behind a space / tab / LF / CR into
    pieces of at most 92 bytes, a second column over the same chars -- on the kernels of short rows, and the rows' results
    follow from the pieces'.  Against the oracle on the ROWS: BASELINE's C5 column, random long rows with nulls and non-ASCII
    words, rows of tabs and line feeds, a row whose only cut byte sits at the 92nd position."""
    L = gpuutil.lib()
    orc = cpulibs.Oracle()
    blob = blob_of(pat)
    rng = np.random.default_rng(9200)
    # (well-formed text: a row cut inside a character would leave a lead byte in front of the next row's first byte, and such a
    # column -- like one with NUL bytes -- keeps the long-row kernels: test_gpu_regex_on_long_rows_not_as_pieces)
    rows_b = [r.decode("utf-8", "ignore").encode() for r in _random_rows(rng, 20_000, 40, 220, alphabet=b"abcdefghijklmnop0123456789.-_/#@ing the a in")]
    rows_b += [b"1.2.3.4 " * 30, b"x" * 91 + b" " + b"y" * 92, b"a\tb\nc\rd " * 25, b" " * 200, b"the in a " * 40, b"#tag@mail.com\n" * 20, b"", b"short"]
    cases = [(gpuutil.synth(5, 0, 120_000), orc.synth(5, 0, 120_000), "C5"), (None, _with_nulls(rows_b, rng), "random long rows")]
    for g, o, what in cases:
        if g is None:
            g = gpuutil.from_col(o)
        f0 = int(L.lib.cs_fallback_count())
        got = g.replace(pat, repl)
        if replace_on_pieces:
            assert last_route().startswith("pieces:"), (what, last_route())
        gpuutil.assert_same(got, orc.replace_re(o, blob, repl), "replace_re(%r) on %s" % (pat, what))
        re = gpuutil.compile_re(pat)
        try:
            has, n = gpuutil.bools(g, "cs_contains_re", re)
            assert last_route().startswith("pieces:"), (what, last_route())
            want_has, want_n = orc.contains_re(o, blob)
            assert np.array_equal(has, want_has) and n == want_n, what
            cnt = np.zeros(o.rows, dtype=np.int32)
            found = C.c_int64()
            L.check(L.lib.cs_count_re(g.m_cptr, re, cnt.ctypes.data, 0, None, C.byref(found)))
            want_cnt, want_found = orc.count_re(o, blob)
            assert np.array_equal(cnt, want_cnt), (what, np.flatnonzero(cnt != want_cnt)[:5])
            assert found.value == want_found
        finally:
            L.lib.cs_regex_destroy(re)
        assert int(L.lib.cs_fallback_count()) == f0


@pytest.mark.parametrize("pat,repl", [(r"^\d+", "N"), (r"\s+", " "), (r"(\d+) (\d+)", "x"), (r"[^a]+", "-"), (r"\w+\s\w+", "2")])
def test_gpu_regex_on_long_rows_not_as_pieces(pat, repl):
    """Programs that can tell a piece from a row -- `^`, white space inside a match, a class that holds it -- and a column with a
    92-byte stretch without white space keep the long-row kernels; same answers as the oracle."""
    orc = cpulibs.Oracle()
    blob = blob_of(pat)
    g, o = gpuutil.synth(5, 0, 60_000), orc.synth(5, 0, 60_000)
    gpuutil.assert_same(g.replace(pat, repl), orc.replace_re(o, blob, repl), "replace_re(%r)" % pat)
    assert not last_route().startswith("pieces:"), last_route()
    rng = np.random.default_rng(9201)
    plain = [r.decode("utf-8", "ignore").encode() for r in _random_rows(rng, 5000, 40, 150)]
    for extra, why in (([b"z" * 150], "a stretch of 92 bytes without white space"), ([b"a b\x00c d " * 12], "a NUL byte: the executor ends the row's scan there"),
                       ([b"word \xc3 word " * 10], "a lead byte in front of a space: the executor swallows the space")):
        col = col_of(plain + extra)
        g2 = gpuutil.from_col(col)
        got = g2.replace(IPV4, "<IP>")
        assert not last_route().startswith("pieces:"), (why, last_route())
        L = gpuutil.lib()
        for v in ("CS_REGEX_ROWWISE", "CS_REGEX_TWO_PASS"):
            L.check(L.lib.cs_config_set(v.encode(), b"1"))
        try:
            want = gpuutil.to_col(g2.replace(IPV4, "<IP>"))
        finally:
            for v in ("CS_REGEX_ROWWISE", "CS_REGEX_TWO_PASS"):
                L.check(L.lib.cs_config_set(v.encode(), None))
        gpuutil.assert_same(got, want, "a column without a view (%s): against the row-wise kernels" % why)


@pytest.mark.parametrize("pat,repl", [(r"\d+", "<number>"), (r"\d", "##"), (r" ", "  "), (r"[a-z]", "<x>"), (r"\.", "[dot]")])
def test_gpu_growing_replacement_sized_from_count_re(pat, repl, monkeypatch):
    """A replacement longer than a one- or two-byte match: count_re runs first and the stream kernel's out tile and output are
    sized from the matches the column and its busiest tile hold (cs_regex.hip: k_match_stats) instead of the worst case
    (three times the in tile, twice the column).  Same column as the oracle's, no launch given up; the worst-case sizing
    (CS_NO_COUNT_SIZING) gives the same."""
    L = gpuutil.lib()
    orc = cpulibs.Oracle()
    blob = blob_of(pat)
    for kind, rows in ((3, 200_003), (2, 100_000)):
        g, o = gpuutil.synth(kind, 0, rows), orc.synth(kind, 0, rows)
        want = orc.replace_re(o, blob, repl)
        f0 = int(L.lib.cs_fallback_count())
        gpuutil.assert_same(g.replace(pat, repl), want, "replace_re(%r -> %r), sized from the count" % (pat, repl))
        assert int(L.lib.cs_fallback_count()) == f0
        monkeypatch.setenv("CS_NO_COUNT_SIZING", "1")
        gpuutil.assert_same(g.replace(pat, repl), want, "replace_re(%r -> %r), worst-case sizing" % (pat, repl))
        monkeypatch.delenv("CS_NO_COUNT_SIZING")


@pytest.mark.parametrize("pat", [r"\w+@\w+", r"[a-z]+\.[a-z]+", r"\w+-\w+"])
def test_gpu_contains_re_of_a_dense_unit_program_by_its_counts(pat, monkeypatch):
    """contains_re of a program with a unit decomposition whose candidate bytes are most of the column runs count_re's unit scan
    and turns the counts into flags (cs_regex_scan.hip: scan<0>): flags and the number of rows that hold a match against the oracle,
    null rows included, and the row lanes' scan (CS_NO_CONTAINS_BY_COUNT) says the same."""
    orc = cpulibs.Oracle()
    blob = blob_of(pat)
    rng = np.random.default_rng(77)
    rows_b = [bytes(rng.choice(list(b"abcdefghij  ..@-"), int(n)).astype(np.uint8)) for n in rng.integers(0, 91, 30_000)]
    # (every fourth row with two-byte characters: the unit scan's tiles that hold bytes >= 0x80)
    glyphs = list("abcdefgh  .@-") + ["\u00e9", "\u00fc", "\u0416"]
    for i in range(0, len(rows_b), 4):
        rows_b[i] = "".join(rng.choice(glyphs, int(rng.integers(0, 40)))).encode()
    col = _with_nulls(rows_b, rng)
    g = gpuutil.from_col(col)
    re = gpuutil.compile_re(pat)
    try:
        has, n = gpuutil.bools(g, "cs_contains_re", re)
        assert last_route() in (("units",) if "@" in pat else ("units", "bits", "plain")), last_route()
        want, want_n = orc.contains_re(col, blob)
        assert np.array_equal(has, want) and n == want_n
        monkeypatch.setenv("CS_NO_CONTAINS_BY_COUNT", "1")
        has2, n2 = gpuutil.bools(g, "cs_contains_re", re)
        assert np.array_equal(has2, want) and n2 == want_n
    finally:
        gpuutil.lib().lib.cs_regex_destroy(re)


# ---- rows with bytes >= 0x80 put off to a second launch (regex_stream.h: ScanStreamArgs::deferred; cs_regex_scan.hip: k_tdfa_scan_list) ----
LATER_PATTERNS = [r"\w+@\w+", r"(\bin\b)|(\ba\b)|(\bthe\b)", r"[aeiou]+", r"\d+\.\d+\.\d+\.\d+", r"[a-z]+ing\b", r"\d+", r"#\w+"]


def _mostly_ascii_rows(rng, count, odd_share, lo=0, hi=90):
    glyphs = list("abcdefghing the in a 0123456789.@#-")
    rows = []
    for i in range(count):
        n = int(rng.integers(lo, hi + 1))
        row = "".join(rng.choice(glyphs, n))
        if rng.random() < odd_share and n >= 4:
            k = int(rng.integers(0, n - 2))
            row = row[:k] + str(rng.choice(["é", "Ж", "€", "\x00"])) + row[k + 2:]
        rows.append(row.encode()[:hi])
    # (a row cut inside a character by the [:hi] above is made whole again)
    return [r.decode("utf-8", "ignore").encode() for r in rows]


@pytest.mark.parametrize("pat", LATER_PATTERNS)
def test_gpu_scan_puts_rows_with_high_bytes_off(pat, monkeypatch):
    """contains_re / count_re on a column whose sample holds a FEW bytes >= 0x80: the rows that hold them (and rows with a NUL)
    go to a list and are scanned by k_tdfa_scan_list, the other rows of their sub-tiles keep the bit form / the chain arithmetic /
    the unit scan -- flags, counts and the number of rows with a match against the oracle, nulls and empty rows included; the
    same with nothing put off (CS_NO_DEFERRED_ROWS)."""
    L = gpuutil.lib()
    orc = cpulibs.Oracle()
    blob = blob_of(pat)
    rng = np.random.default_rng(4100)
    rows_b = _mostly_ascii_rows(rng, 40_000, 0.01)
    rows_b[0] = "é first window".encode()  # (the sample's first window sees such a byte whatever the draw)
    col = _with_nulls(rows_b, rng)
    g = gpuutil.from_col(col)
    re = gpuutil.compile_re(pat)
    try:
        want_has, want_n = orc.contains_re(col, blob)
        want_cnt = orc.count_re(col, blob)
        for env in (None, "1"):
            if env:
                monkeypatch.setenv("CS_NO_DEFERRED_ROWS", env)
            f0 = int(L.lib.cs_fallback_count())
            has, n = gpuutil.bools(g, "cs_contains_re", re)
            r1 = last_route()
            cnt = np.zeros(col.rows, dtype=np.int32)
            found = C.c_int64()
            L.check(L.lib.cs_count_re(g.m_cptr, re, cnt.ctypes.data, 0, None, C.byref(found)))
            r2 = last_route()
            assert np.array_equal(has, want_has) and n == want_n, (pat, env, r1)
            assert np.array_equal(cnt, want_cnt[0] if isinstance(want_cnt, tuple) else want_cnt), (pat, env, r2)
            assert int(L.lib.cs_fallback_count()) == f0
            if env is None:
                assert r1.endswith("+later") and r2.endswith("+later"), (r1, r2)
            else:
                assert "+later" not in r1 + r2
    finally:
        L.lib.cs_regex_destroy(re)


def test_gpu_scan_with_more_such_rows_than_the_list_holds():
    """The sample's three windows see one byte >= 0x80, the column between them is full of such rows: the list overflows, the op
    says so (a counted fallback) and scans the column again with nothing put off -- the result is the oracle's."""
    L = gpuutil.lib()
    orc = cpulibs.Oracle()
    pat = r"\w+@\w+"
    blob = blob_of(pat)
    rng = np.random.default_rng(4101)
    rows_b = _mostly_ascii_rows(rng, 60_000, 0.0, lo=30, hi=80)
    rows_b[0] = "é first window".encode()
    for i in range(6_000, 24_000):  # (the windows are 64 KiB at the start, the middle and the end of ~3.3 MB of chars)
        rows_b[i] = ("é" + rows_b[i].decode()[2:]).encode()
    col = _with_nulls(rows_b, rng)
    g = gpuutil.from_col(col)
    re = gpuutil.compile_re(pat)
    try:
        f0 = int(L.lib.cs_fallback_count())
        has, n = gpuutil.bools(g, "cs_contains_re", re)
        want_has, want_n = orc.contains_re(col, blob)
        assert np.array_equal(has, want_has) and n == want_n
        assert int(L.lib.cs_fallback_count()) == f0 + 1
    finally:
        L.lib.cs_regex_destroy(re)


@pytest.mark.parametrize("pat,repl", [(r"\w+@\w+", "<m>"), (r"(\bin\b)|(\ba\b)|(\bthe\b)", "="), (r"\d+\.\d+\.\d+\.\d+", "<IP>"), (r"[a-z]+ing\b", ""),
                                      (r"#\w+", "<a longer tag>"), (r"\d+", "<number>"), (r"\bthe\b", "THE"),
                                      # (replacements of 9-16 bytes: the four-register variants of every form)
                                      (r"\w+@\w+", "<mail-address>"), (r"(\bin\b)|(\ba\b)|(\bthe\b)", "<stop-word>"), (r"\d+\.\d+\.\d+\.\d+", "<ip-address>")])
def test_gpu_replace_re_leaves_rows_with_high_bytes_holes(pat, repl, monkeypatch):
    """replace_re on a column whose sample holds a FEW bytes >= 0x80 (cs_regex.hip: StreamArgs::hole_mask): the rows that hold
    them (cs_virtual.hip: OddRows -- rows with a NUL too) are sized beforehand and written afterwards, a thread a row; the
    single pass leaves them holes and runs its unit forms on the others.  Against the oracle: shrinking, equal and growing
    replacements, such rows first and last in their 64-row tile, next to nulls and empty rows; and with the holes off."""
    L = gpuutil.lib()
    orc = cpulibs.Oracle()
    blob = blob_of(pat)
    rng = np.random.default_rng(4200)
    rows_b = _mostly_ascii_rows(rng, 50_000, 0.01)
    rows_b[0] = "é in the first window a@b 1.2.3.4 #tag".encode()
    for r in (63, 64, 127, 128, 4095, 4096, 49_999):
        rows_b[r] = ("the ünïcode a@b in " + str(r) + " 10.0.0.1 #x testing").encode()
    rows_b[200] = b"nul \x00 in the middle a@b 1.2.3.4"
    rows_b[201] = b""
    col = _with_nulls(rows_b, rng)
    g = gpuutil.from_col(col)
    want = orc.replace_re(col, blob, repl)
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("CS_NO_DEFERRED_ROWS", env)
        f0 = int(L.lib.cs_fallback_count())
        got = g.replace(pat, repl)
        route = last_route()
        gpuutil.assert_same(got, want, "replace_re(%r) route %s" % (pat, route))
        assert int(L.lib.cs_fallback_count()) == f0
        if env:
            assert "+later" not in route


def test_gpu_replace_re_with_holes_on_the_pieces_of_long_rows():
    """BASELINE's C5 column (rows of 40-150 bytes, one in 170 with an accent): replace_re runs on the column's pieces, and the
    pieces with a byte >= 0x80 are the single pass's holes -- against the oracle on the rows."""
    L = gpuutil.lib()
    orc = cpulibs.Oracle()
    g, o = gpuutil.synth(5, 0, 150_000), orc.synth(5, 0, 150_000)
    for pat, repl in ((r"(\bin\b)|(\ba\b)|(\bthe\b)", "="), (r"\w+@\w+", "<m>"), (r"#\w+", "<tag>"), (r"#\w+", "#"), (r"[a-z]+ing\b", "")):
        f0 = int(L.lib.cs_fallback_count())
        got = g.replace(pat, repl)
        assert last_route().startswith("pieces:") and last_route().endswith("+later"), last_route()
        gpuutil.assert_same(got, orc.replace_re(o, blob_of(pat), repl), "replace_re(%r) on C5 (%s)" % (pat, last_route()))
        assert int(L.lib.cs_fallback_count()) == f0


@pytest.mark.parametrize("pat,repl", [(r"[^ ]+$", "LAST"), (r"\w+\b", "w"), (r"[a-z]+\b", ""), (r"#\w+$", "<tag>"), (r"\d+$", "N"), (r"[a-e]+\B", "=")])
def test_gpu_bit_form_with_assertions_behind_the_plus_loop(pat, repl, monkeypatch):
    """A path that ends in a greedy `+` loop with assertions behind it (regex_bits.h: the TAIL -- the loop's exits are tried
    longest first, a start whose run has no exit that passes matches nothing): contains_re / count_re / replace_re on the bit
    form (forced: CS_BITS_ALWAYS) against the oracle -- log lines, rows that end in a space, a newline, a digit, nulls."""
    monkeypatch.setenv("CS_BITS_ALWAYS", "1")
    L = gpuutil.lib()
    orc = cpulibs.Oracle()
    blob = blob_of(pat)
    rng = np.random.default_rng(4300)
    base = orc.synth(3, 0, 30_000).to_list()
    extra = ["the last word", "ends in space ", "ends in newline\n", "two\nlines here", "abc1", "abc_", "a_b c-d", "#tag", "x #tag", "#tag x", "", "42", "x 42", "42 x", "abcde", "abcdef x"]
    for k, e in enumerate(extra):
        base[1000 + 37 * k] = e
    col = _with_nulls([r.encode() if r is not None else b"" for r in base], rng)
    g = gpuutil.from_col(col)
    re = gpuutil.compile_re(pat)
    try:
        f0 = int(L.lib.cs_fallback_count())
        has, n = gpuutil.bools(g, "cs_contains_re", re)
        want_has, want_n = orc.contains_re(col, blob)
        assert np.array_equal(has, want_has) and n == want_n, (pat, last_route())
        cnt = np.zeros(col.rows, dtype=np.int32)
        found = C.c_int64()
        L.check(L.lib.cs_count_re(g.m_cptr, re, cnt.ctypes.data, 0, None, C.byref(found)))
        assert last_route() in ("bits", "chain"), last_route()  # (a chain -- `[a-z]+\b` -- keeps the chain arithmetic)
        assert np.array_equal(cnt, orc.count_re(col, blob)[0]), pat
        got = g.replace(pat, repl)
        assert last_route() in ("bits", "chain"), last_route()
        gpuutil.assert_same(got, orc.replace_re(col, blob, repl), "replace_re(%r)" % pat)
        assert int(L.lib.cs_fallback_count()) == f0
    finally:
        L.lib.cs_regex_destroy(re)


@pytest.mark.parametrize("switch", [None, "CS_REGEX_ROWWISE", "CS_CLASS_RUNS_ALWAYS", "CS_REGEX_NO_TDFA", "CS_NO_DEFERRED_ROWS"])
def test_gpu_regex_on_rows_with_nul_bytes(switch, monkeypatch):
    """Embedded NUL bytes (tests/test_nul_bytes.py: the reference ends a call at a NUL met by a live thread, but its search for the
    next start of a program whose first instruction is a literal jumps over them): contains_re / count_re / replace_re against
    the oracle on a column where one row in fifty holds a NUL -- short rows (the mask forms put such rows off / leave them holes)
    and rows beyond the masks; every executor (the stream kernels' generic scan, the row-wise kernels, cs_runs.hip, the list
    simulator)."""
    if switch:
        monkeypatch.setenv(switch, "1")
    L = gpuutil.lib()
    orc = cpulibs.Oracle()
    rng = np.random.default_rng(4400)
    for lo, hi in ((0, 60), (20, 200)):
        rows_b = []
        for i in range(12_000):
            n = int(rng.integers(lo, hi + 1))
            r = bytes(rng.choice(list(b"ab1 a.b  xa"), n).astype(np.uint8))
            if rng.random() < 0.02 and n >= 3:
                k = int(rng.integers(0, n))
                r = r[:k] + b"\x00" + r[k + 1:]
            rows_b.append(r)
        rows_b[0] = b"\x00a first window"
        rows_b[77] = b"a\x00a"
        rows_b[78] = b"\x00\x00a\x00"
        for k, r in enumerate((b"x\x00\na", b"\x00\na", b"a\x00\na", b"x\n\x00a", b"xa\x00\nab\nab", b"\n\x00\na", b"ab\nab", b"x\nab\n\nab x\x00y\nab")):
            rows_b[100 + 3 * k] = r
        col = _with_nulls(rows_b, rng)
        g = gpuutil.from_col(col)
        for pat, repl in (("a", "aa"), ("a+", "-"), ("ab", ""), (r"a\d", "<>"), ("[ab]+", "="), (r"\d", "##"), (r"a\b", "A"), ("b a", "_"), ("^a", "<"), (r"^\w", "W"), ("^ab", "")):
            blob = blob_of(pat)
            re = gpuutil.compile_re(pat)
            try:
                has, n = gpuutil.bools(g, "cs_contains_re", re)
                want_has, want_n = orc.contains_re(col, blob)
                assert np.array_equal(has, want_has) and n == want_n, (pat, switch, last_route())
                cnt = np.zeros(col.rows, dtype=np.int32)
                found = C.c_int64()
                L.check(L.lib.cs_count_re(g.m_cptr, re, cnt.ctypes.data, 0, None, C.byref(found)))
                assert np.array_equal(cnt, orc.count_re(col, blob)[0]), (pat, switch, last_route())
            finally:
                L.lib.cs_regex_destroy(re)
            gpuutil.assert_same(g.replace(pat, repl), orc.replace_re(col, blob, repl), "replace_re(%r) %s %s" % (pat, switch, last_route()))


def test_gpu_put_off_rows_on_a_column_with_int32_offsets():
    """A split's output column (int32 offsets, nulls where a row had fewer tokens) with a few tokens that hold a two-byte character:
    contains_re / count_re put those rows off, replace_re leaves them holes -- against the oracle on the oracle's own split."""
    L = gpuutil.lib()
    orc = cpulibs.Oracle()
    rng = np.random.default_rng(4500)
    rows_b = _mostly_ascii_rows(rng, 60_000, 0.03, lo=10, hi=90)
    rows_b[0] = "é in the first window".encode()
    col = _with_nulls(rows_b, rng)
    g = gpuutil.from_col(col)
    gcols = g.split(" ", 3)
    ocols = orc.split(col, " ", 3)
    assert len(gcols) == len(ocols)
    for gc, oc in zip(gcols, ocols):
        for pat, repl in ((r"[a-z]+ing\b", "-"), (r"\d+", "<n>"), (r"(\bin\b)|(\ba\b)|(\bthe\b)", "=")):
            blob = blob_of(pat)
            re = gpuutil.compile_re(pat)
            try:
                has, n = gpuutil.bools(gc, "cs_contains_re", re)
                want_has, want_n = orc.contains_re(oc, blob)
                assert np.array_equal(has, want_has) and n == want_n, (pat, last_route())
            finally:
                L.lib.cs_regex_destroy(re)
            gpuutil.assert_same(gc.replace(pat, repl), orc.replace_re(oc, blob, repl), "replace_re(%r) %s" % (pat, last_route()))


def test_gpu_generated_patterns_against_the_oracle():
    """A slice of tools/fuzz_patterns_gpu.py: sixty generated patterns (alternations, classes, counted items, assertions, `+` tails)
    on columns of ASCII text with a few rows of two-byte characters and NUL bytes -- contains_re, count_re, replace_re against the
    oracle (1359 patterns, 0 mismatches in the round's long run)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_patterns_gpu", os.path.join(ROOT, "tools", "fuzz_patterns_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    done, bad = mod.run(120.0, 606, max_patterns=60)
    assert done == 60 and bad == 0


def test_gpu_random_arguments_of_the_other_ops_against_the_oracle():
    """A slice of tools/fuzz_ops_gpu.py: random delimiters and limits for split / rsplit, character sets for strip, needles and
    replacements for the literal replace, delimiter sets for tokenize -- on columns with a few two-byte characters and NUL bytes,
    against the oracle (10 328 rounds, 0 mismatches in the round's long run)."""
    import importlib.util
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location("fuzz_ops_gpu", os.path.join(ROOT, "tools", "fuzz_ops_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    done, bad = mod.run(120.0, 707, max_rounds=150)
    assert done == 150 and bad == 0
