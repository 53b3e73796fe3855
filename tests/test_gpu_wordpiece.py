"""WordPiece on the MI355X, bit for bit against the model of tests/wordpiece_model.py (checked against the reference fixture
and against wordpiece_ops.h by tests/test_wordpiece_cpu.py), through the C ABI and through custrings_amd/wordpiece.py: the wave
and workgroup edges of the row count with null rows at the ends of a tile, both forms with the route asserted (the long form
forced on short rows and reached by plan on rows of a few KB), words at and beyond max_word_chars, a word whose last piece
fails, a word as long as the longest entry, a last character of four bytes, rows of blanks, words on and across the long
form's 64-byte segments, a vocabulary with probe chains and the vocabulary of unk alone, both punct settings, a borrowed column
at an odd address, results to host and to device memory with the words beside them watched, encode at its edges, the
reference fixture itself, and every argument error."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import borrowedutil as bu
import gpuutil
import wordpiece_model as m

pytestmark = pytest.mark.gpu

TILE, LONG = "wordpiece tile", "wordpiece long"
CAN32, CAN64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def _L():
    return gpuutil.lib()


def _route():
    return _L().lib.cs_debug_last_route().decode()


def column(rows):
    from custrings_amd import nvstrings

    _L()
    chars, offs, nulls = m.to_arrow(rows)
    valid = np.concatenate([np.packbits(1 - nulls, bitorder="little"), np.zeros(8, dtype=np.uint8)])
    chars = chars if chars.size else np.zeros(1, dtype=np.uint8)
    return nvstrings.from_offsets64(chars, offs, len(rows), valid)


class Vocab:
    """a vocabulary on the device and its model"""

    def __init__(self, entries, **kw):
        from custrings_amd import wordpiece

        self.entries = entries
        self.dev = wordpiece.vocabulary(column(entries), **{k: v.decode() for k, v in kw.items()})
        self.model = m.Vocab(entries, **kw)


_vocabs = {}


def vocab(name):
    if name not in _vocabs:
        if name == "small":  # the fixture's 300 entries
            entries = m.make_vocab(300, 11)
        elif name == "large":  # probe chains exist: 5 000 rows, ~6 400 keys in 32 768 slots
            entries = m.make_vocab(5000, 21, max_chars=4)
        elif name == "unk":
            entries = [b"[UNK]"]
        _vocabs[name] = Vocab(entries)
    return _vocabs[name]


def long_form():
    class Forced:
        def __enter__(self):
            _L().lib.cs_config_set(b"CS_WORDPIECE_LONG", b"1")

        def __exit__(self, *exc):
            _L().lib.cs_config_set(b"CS_WORDPIECE_LONG", None)

    return Forced()


def abi_tokenize(g, v, nrows, max_word_chars=100, punct=0, guard=4):
    """cs_wordpiece_count and cs_wordpiece_ids into host memory with `guard` canary words on either side -> (ids, offsets)"""
    L = _L()
    offs = np.full(nrows + 1 + 2 * guard, CAN64, dtype=np.int64)
    total = C.c_int64(-1)
    L.check(L.lib.cs_wordpiece_count(g.m_cptr, v.dev.m_cptr, max_word_chars, punct, offs[guard:].ctypes.data, 0, None, C.byref(total)))
    first = _route()
    assert np.all(offs[:guard] == CAN64) and np.all(offs[guard + nrows + 1:] == CAN64), "words beside the offsets were written"
    assert total.value == offs[guard + nrows]
    ids = np.full(total.value + 2 * guard, CAN32, dtype=np.int32)
    L.check(L.lib.cs_wordpiece_ids(g.m_cptr, v.dev.m_cptr, max_word_chars, punct, offs[guard:].ctypes.data, ids[guard:].ctypes.data, 0, None))
    assert np.all(ids[:guard] == CAN32) and np.all(ids[guard + total.value:] == CAN32), "words beside the ids were written"
    assert total.value == 0 or _route() == first
    return ids[guard:guard + total.value], offs[guard:guard + nrows + 1]


def check_tokenize(rows, v, route, max_word_chars=100, punct=0, want=None):
    ids, offs = abi_tokenize(column(rows), v, len(rows), max_word_chars, punct)
    assert _route() == route, _route()
    want_ids, want_offs = want if want is not None else m.tokenize(rows, v.model, max_word_chars, punct)
    bad = np.nonzero(np.diff(offs) != np.diff(want_offs))[0]
    assert bad.size == 0, (bad[:5].tolist(), rows[bad[0]])
    assert np.array_equal(offs, want_offs)
    wrong = np.nonzero(ids != want_ids)[0]
    assert wrong.size == 0, (wrong[:5].tolist(), rows[int(np.searchsorted(want_offs, wrong[0], side="right")) - 1])


def with_nulls_at_tile_ends(rows):
    rows = list(rows)
    for at in (0, 31, 63, 64, len(rows) - 1):
        if at < len(rows):
            rows[at] = None
    return rows


_want = {}


def short_case(nrows, vname, punct):
    """the rows of a short-form case and the model's answer, computed once"""
    key = (nrows, vname, punct)
    if key not in _want:
        rows = m.make_rows(nrows, 100 + nrows) if nrows > 1 else [b"ab ##ab, a\xf0\x9f\x98\x80"]
        if nrows >= 63:
            rows = with_nulls_at_tile_ends(rows)
        _want[key] = (rows, m.tokenize(rows, vocab(vname).model, 100, punct))
    return _want[key]


# ---- the tile form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows,vname,punct", [(1, "small", 1), (63, "large", 0), (64, "small", 1), (65, "large", 1), (257, "large", 0), (257, "small", 1)])
def test_short_rows_take_the_tile_form(nrows, vname, punct):
    rows, want = short_case(nrows, vname, punct)
    check_tokenize(rows, vocab(vname), TILE, punct=punct, want=want)


@pytest.mark.parametrize("nrows,vname,punct", [(63, "large", 0), (64, "small", 1), (257, "large", 0)])
def test_the_long_form_on_short_rows_gives_the_same(nrows, vname, punct):
    rows, want = short_case(nrows, vname, punct)
    with long_form():
        check_tokenize(rows, vocab(vname), LONG, punct=punct, want=want)


def word_cases(v):
    """what a word can be, around the limits (the small vocabulary: single letters a-e and more are entries, "x" is none)"""
    longest = max(v.model.ids, key=len)
    rows = [b"abcde", b"abcdef", b"abcdea", b"a" * 6, b"a" * 7,  # characters at, and one beyond, max_word_chars = 6 below
            "語語語語語語".encode(), "語語語語語語語".encode(),
            b"abx", b"aabx cd", b"ab abx ab",  # the last piece fails behind pieces that matched
            longest, longest + b"a", b"a" + longest,
            "ab😀".encode(), "ab 😀".encode(), "x😀".encode(), "a𐍈".encode(),  # a four-byte last character
            b" ", b" \t\n\r\x0b\x0c  ", b"", None,
            b"##ab", b"##", b"###", b"####", b"##a#", b"a##b", b"a##a#", b"#", b"[UNK]", b"[UNK],[UNK]"]
    return rows + m.hostile_rows()


@pytest.mark.parametrize("punct", [0, 1])
@pytest.mark.parametrize("forced", [False, True])
def test_words_at_the_limits_on_both_forms(punct, forced):
    v = vocab("small")
    rows = word_cases(v)
    assert m.row_ids(b"aabx", v.model) == [v.model.unk] and v.model.unk not in m.row_ids(b"aab", v.model)
    for mwc in (6, 100):
        if forced:
            with long_form():
                check_tokenize(rows, v, LONG, mwc, punct)
        else:
            check_tokenize(rows, v, TILE, mwc, punct)


def test_max_word_chars_at_its_ends():
    v = vocab("small")
    rows = [b"a", b"ab a", b"a" * 1024 + b" b", b"a" * 1025 + b" b", b"ab" * 600]
    check_tokenize(rows, v, TILE, 1)
    check_tokenize(rows, v, TILE, 1024)
    assert m.row_ids(rows[2], v.model, 1024) != m.row_ids(rows[3], v.model, 1024)


@pytest.mark.parametrize("punct", [0, 1])
def test_the_vocabulary_of_unk_alone(punct):
    v = vocab("unk")
    assert v.dev.entries == 1 and v.dev.unk_id == 0 and v.dev.max_entry_bytes == 5
    rows = with_nulls_at_tile_ends(m.make_rows(70, 3)) + m.hostile_rows()
    check_tokenize(rows, v, TILE, punct=punct)
    with long_form():
        check_tokenize(rows, v, LONG, punct=punct)


# ---- the long form -------------------------------------------------------------------------------------------------------------------
def long_rows():
    text = [r for r in m.make_rows(1800, 77) if r]
    rows = [b" ".join(text[i:i + 80]) for i in range(0, 1600, 80)]  # 20 rows of a few KB
    rows[3] = None
    rows += [b"a " * 30 + b"abcdeabcde ab",  # a word from byte 60 to 70: across the first segment's edge
             b"a " * 29 + b"abcdea ab",  # a word from byte 58 that ends exactly on the edge, the next starts behind it
             b"a " * 32 + b"ab cd",  # a word that starts exactly on the edge
             b"a " * 29 + b"abcde,ab",  # punctuation as byte 63, a word from byte 64
             b"ab" * 100 + b" ab",  # one word over three segments (more characters than max_word_chars = 100)
             b"abx" * 30 + b" " * 70 + b"ab",  # a segment of blanks only
             b" " * 200, b"", b"\x80" * 130 + b" a",
             b"ab " * 300 + "語😀".encode()]  # a four-byte last character
    rows.append(b" ".join(text[:200]))  # > 6 KB: no tile size takes this column
    return rows


@pytest.fixture(scope="module")
def long_case():
    rows = long_rows()
    assert len(rows[-1]) > 6144 and all(r is None or 1500 < len(r) < 6000 for r in rows[:20])
    return rows, {p: m.tokenize(rows, vocab("large").model, 100, p) for p in (0, 1)}


@pytest.mark.parametrize("punct", [0, 1])
def test_long_rows_take_the_long_form(long_case, punct):
    rows, want = long_case
    check_tokenize(rows, vocab("large"), LONG, punct=punct, want=want[punct])


def test_long_rows_without_the_oversize_one_take_the_long_form_by_plan(long_case):
    rows = long_case[0][:20]  # rows of a few KB only: 16 of them do not fit a tile
    check_tokenize(rows, vocab("small"), LONG, punct=1)


# ---- memory ----------------------------------------------------------------------------------------------------------------------------
def test_borrowed_column_at_an_odd_address_into_device_memory():
    import torch

    from custrings_amd import wordpiece

    rows, (want_ids, want_offs) = short_case(257, "large", 0)
    v = vocab("large")
    col = bu.Borrowed(rows, 13, 8, b"\xff")
    offs = bu.Guarded(np.int64, 258)
    ids = bu.Guarded(np.int32, len(want_ids))
    total, _ = wordpiece.tokenize(col.col, v.dev, devptrs=(ids.ptr, offs.ptr))
    assert _route() == TILE and total == len(want_ids)
    assert np.array_equal(offs.values(), want_offs) and np.array_equal(ids.values(), want_ids)
    assert col.caller_memory_intact()
    t_ids = torch.zeros(len(want_ids), dtype=torch.int32, device="cuda:0")
    t_offs = torch.zeros(258, dtype=torch.int64, device="cuda:0")
    with long_form():
        assert wordpiece.tokenize(col.col, v.dev, devptrs=(t_ids, t_offs))[0] == total and _route() == LONG
    assert np.array_equal(t_ids.cpu().numpy(), want_ids) and np.array_equal(t_offs.cpu().numpy(), want_offs)
    with pytest.raises(ValueError):
        wordpiece.tokenize(col.col, v.dev, devptrs=(t_ids[:-1], t_offs))
    # a vocabulary over borrowed memory keeps nothing of it
    vcol = bu.Borrowed(v.entries, 7, 8, b"\xff")
    borrowed_vocab = wordpiece.vocabulary(vcol.col)
    vcol.chars_back.fill_(0x61)  # (the caller's memory changes behind the handle's back)
    torch.cuda.synchronize()
    got, got_offs = wordpiece.tokenize(column(rows), borrowed_vocab)
    assert np.array_equal(got, want_ids) and np.array_equal(got_offs, want_offs)


# ---- encode ------------------------------------------------------------------------------------------------------------------------------
def encode_rows(v):
    rows = with_nulls_at_tile_ends(m.make_rows(70, 9))
    by_count = {}
    for r in m.make_rows(200, 10, marks_every=0):
        by_count.setdefault(len(m.row_ids(r, v.model, punct=1)), r)
    rows += [by_count[n] for n in (0, 1, 5, 6, 7, 8, 9) if n in by_count]  # cut exactly at the limit for max_length 8, and around it
    assert {0, 6, 7, 8} <= set(by_count)
    return rows + [b"", b"  ", None, b"x" * 200 + b" ab"]


def abi_encode(g, v, nrows, max_length, cls, sep, pad, punct, want_mask=True, guard=8):
    L = _L()
    ids = np.full(nrows * max_length + 2 * guard, CAN32, dtype=np.int32)
    mask = np.full(nrows * max_length + 2 * guard, 0x5A, dtype=np.uint8)
    L.check(L.lib.cs_wordpiece_encode(g.m_cptr, v.dev.m_cptr, 100, punct, max_length, cls, sep, pad, ids[guard:].ctypes.data,
                                      mask[guard:].ctypes.data if want_mask else None, 0, None))
    n = nrows * max_length
    assert np.all(ids[:guard] == CAN32) and np.all(ids[guard + n:] == CAN32), "words beside the ids were written"
    assert np.all(mask[:guard] == 0x5A) and np.all(mask[guard + n:] == 0x5A), "bytes beside the mask were written"
    if not want_mask:
        assert np.all(mask == 0x5A)
    return ids[guard:guard + n].reshape(nrows, max_length), mask[guard:guard + n].reshape(nrows, max_length)


@pytest.mark.parametrize("max_length,cls,sep", [(1, -1, -1), (1, 1, -1), (1, -1, 2), (2, 1, 2), (2, -1, -1), (8, 1, 2), (8, -1, -1), (8, 1, -1)])
def test_encode_on_both_forms(max_length, cls, sep):
    v = vocab("small")
    rows = encode_rows(v)
    g = column(rows)
    want_ids, want_mask = m.encode(rows, v.model, max_length, cls, sep, 3, punct=1)
    ids, mask = abi_encode(g, v, len(rows), max_length, cls, sep, 3, 1)
    assert _route() == TILE
    assert np.array_equal(ids, want_ids) and np.array_equal(mask, want_mask)
    with long_form():
        ids, mask = abi_encode(g, v, len(rows), max_length, cls, sep, 3, 1, want_mask=max_length != 8)
        assert _route() == LONG
    assert np.array_equal(ids, want_ids) and (max_length == 8 or np.array_equal(mask, want_mask))


def test_encode_long_rows_into_device_memory_through_the_module(long_case):
    from custrings_amd import wordpiece

    rows, _ = long_case
    v = vocab("small")
    cls, sep, pad = v.model.id_of(b"[CLS]"), v.model.id_of(b"[SEP]"), v.model.id_of(b"[PAD]")
    want_ids, want_mask = m.encode(rows, v.model, 128, cls, sep, pad)
    ids, mask = wordpiece.encode(column(rows), v.dev, 128, cls="[CLS]", sep="[SEP]", pad="[PAD]")
    assert _route() == LONG and ids.dtype == np.int32 and mask.dtype == np.uint8
    assert np.array_equal(ids, want_ids) and np.array_equal(mask, want_mask)
    d_ids, d_mask = bu.Guarded(np.int32, len(rows) * 128), bu.Guarded(np.uint8, len(rows) * 128)
    wordpiece.encode(column(rows), v.dev, 128, cls=cls, sep=sep, pad=pad, devptrs=(d_ids.ptr, d_mask.ptr))
    assert np.array_equal(d_ids.values().reshape(-1, 128), want_ids) and np.array_equal(d_mask.values().reshape(-1, 128), want_mask)
    d_ids = bu.Guarded(np.int32, len(rows) * 128)
    wordpiece.encode(column(rows), v.dev, 128, cls=cls, sep=sep, pad=pad, devptrs=(d_ids.ptr, None))
    assert np.array_equal(d_ids.values().reshape(-1, 128), want_ids)


# ---- the module ------------------------------------------------------------------------------------------------------------------------------
def test_the_reference_fixture_through_the_module():
    from custrings_amd import nvstrings, nvtext, wordpiece

    assert nvtext.wordpiece_tokenize is wordpiece.tokenize and nvtext.wordpiece_encode is wordpiece.encode
    d = json.load(open(os.path.join(m.ROOT, "tests", "golden", "reference_wordpiece.json")))
    strs = nvstrings.to_device(d["rows"])
    v = nvtext.wordpiece_vocabulary(nvstrings.to_device(d["vocab"]), prefix=d["prefix"], unk=d["unk"])
    assert v.entries == len(d["vocab"]) and v.unk_id == d["vocab"].index(d["unk"]) and v.max_entry_bytes == max(len(e.encode()) for e in d["vocab"])
    for e in ("##", "#", "###", "##a#", "a##b", "[UNK]", "😀"):
        assert v.id_of(e) == d["vocab"].index(e)
    assert v.id_of("no such entry") is None and v.id_of("") is None and v.id_of("##a##") is None
    for c in d["cases"]:
        ids, offs = wordpiece.tokenize(strs, v, max_word_chars=c["max_word_chars"], punct=bool(c["punct"]))
        assert ids.dtype == np.int32 and offs.dtype == np.int64 and _route() == TILE
        assert [ids[offs[r]:offs[r + 1]].tolist() for r in range(len(d["rows"]))] == c["ids"], (c["punct"], c["max_word_chars"])


def test_duplicate_null_and_empty_vocabulary_rows_and_other_prefixes():
    from custrings_amd import wordpiece

    entries = [None, b"", b"ab", b"<unk>", b"ab", b"@@c", None, b"@@c", b"<unk>", b"", b"c", b"ab", b"@@", b"##c"]
    v = Vocab(entries, prefix=b"@@", unk=b"<unk>")
    assert v.dev.entries == 6 and v.dev.unk_id == 3 and v.dev.id_of(b"ab") == 2 and v.dev.id_of("@@c") == 5 and v.dev.id_of("c") == 10
    rows = [b"ab abc c", b"cc", None, b"x", b"@@c @@ c@@ c##c ab@@c"]
    check_tokenize(rows, v, TILE)
    empty = column([])
    ids, offs = wordpiece.tokenize(empty, v.dev)
    assert ids.size == 0 and offs.tolist() == [0]
    assert wordpiece.encode(empty, v.dev, 4)[0].shape == (0, 4)


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from custrings_amd import wordpiece

    L = _L()
    INVALID, RANGE = L.CS_ERR_INVALID_ARG, L.CS_ERR_RANGE
    g = column([b"ab cd"])
    v = vocab("small")
    create, count, ids_fn, encode = L.lib.cs_wordpiece_vocab_create, L.lib.cs_wordpiece_count, L.lib.cs_wordpiece_ids, L.lib.cs_wordpiece_encode
    handle = C.c_void_p(1)
    entries = column([b"a", b"b", b"[UNK]"])
    assert create(entries.m_cptr, b"##", b"[unk]", None, C.byref(handle)) == INVALID and handle.value is None  # unk is no entry
    assert "unknown token" in L.last_error()
    assert create(entries.m_cptr, b"", b"[UNK]", None, C.byref(handle)) == INVALID  # an empty prefix
    assert create(entries.m_cptr, b"123456789", b"[UNK]", None, C.byref(handle)) == INVALID
    assert create(None, b"##", b"[UNK]", None, C.byref(handle)) == INVALID
    assert create(entries.m_cptr, b"##", b"[UNK]", None, None) == INVALID
    assert create(column([b"[UNK]", b"a" * 256]).m_cptr, None, None, None, C.byref(handle)) == RANGE  # an entry over 255 bytes
    assert create(column([b"[UNK]", b"a" * 255]).m_cptr, None, None, None, C.byref(handle)) == 0 and handle.value
    L.lib.cs_wordpiece_vocab_destroy(handle)
    L.lib.cs_wordpiece_vocab_destroy(None)
    assert create(column([]).m_cptr, None, None, None, C.byref(handle)) == INVALID  # (no rows: unk is no entry)
    offs = np.full(2, 7, dtype=np.int64)
    out = np.full(8, 7, dtype=np.int32)
    total = C.c_int64()
    po, pi = offs.ctypes.data, out.ctypes.data
    assert count(None, v.dev.m_cptr, 100, 0, po, 0, None, C.byref(total)) == INVALID  # a null column
    assert count(g.m_cptr, None, 100, 0, po, 0, None, C.byref(total)) == INVALID
    assert count(g.m_cptr, v.dev.m_cptr, 100, 0, None, 0, None, C.byref(total)) == INVALID
    assert count(g.m_cptr, v.dev.m_cptr, 100, 0, po, 0, None, None) == INVALID
    assert count(g.m_cptr, v.dev.m_cptr, 0, 0, po, 0, None, C.byref(total)) == RANGE  # max_word_chars out of range
    assert count(g.m_cptr, v.dev.m_cptr, 1025, 0, po, 0, None, C.byref(total)) == RANGE
    assert ids_fn(None, v.dev.m_cptr, 100, 0, po, pi, 0, None) == INVALID
    assert ids_fn(g.m_cptr, v.dev.m_cptr, 100, 0, None, pi, 0, None) == INVALID
    assert ids_fn(g.m_cptr, v.dev.m_cptr, 1025, 0, po, pi, 0, None) == RANGE
    assert ids_fn(g.m_cptr, v.dev.m_cptr, 100, 0, po, pi, 0, None) == INVALID  # offsets that do not start at 0
    assert encode(None, v.dev.m_cptr, 100, 0, 4, -1, -1, 0, pi, None, 0, None) == INVALID
    assert encode(g.m_cptr, v.dev.m_cptr, 100, 0, 1, 1, 2, 0, pi, None, 0, None) == INVALID  # max_length too small for the specials
    assert encode(g.m_cptr, v.dev.m_cptr, 100, 0, 0, -1, -1, 0, pi, None, 0, None) == INVALID
    assert encode(g.m_cptr, v.dev.m_cptr, 0, 0, 4, -1, -1, 0, pi, None, 0, None) == RANGE
    assert np.all(offs == 7) and np.all(out == 7)
    assert encode(g.m_cptr, v.dev.m_cptr, 100, 0, 2, 1, 2, 0, pi, None, 0, None) == 0 and out[:3].tolist() == [1, 2, 7]  # (the specials alone fit)
    with pytest.raises(ValueError):
        wordpiece.vocabulary(entries, unk="[unk]")
    with pytest.raises(ValueError):
        wordpiece.encode(g, v.dev, 8, cls="no such token")
    with pytest.raises(ValueError):
        wordpiece.encode(g, v.dev, 1, cls="[CLS]", sep="[SEP]")
    with pytest.raises(ValueError):
        wordpiece.tokenize(g, v.dev, max_word_chars=0)
