"""WordPiece without a GPU: the model of tests/wordpiece_model.py against the reference fixture
(tests/golden/reference_wordpiece.json: the ids of the `tokenizers` library, written by tools/make_wordpiece_golden.py);
custrings_amd/csrc/wordpiece_ops.h (the text the kernels compile), built with g++, against the model on the fixture and on
what the fixture may not hold -- malformed bytes, continuation bytes only, control and NUL bytes, duplicate, null and empty
vocabulary rows, words that start with the prefix, a vocabulary of unk alone; and the table with keys that meet in it."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wordpiece_model as m

GOLDEN = os.path.join(m.ROOT, "tests", "golden", "reference_wordpiece.json")


@pytest.fixture(scope="module")
def golden():
    d = json.load(open(GOLDEN))
    d["vocab_bytes"] = [e.encode() for e in d["vocab"]]
    d["row_bytes"] = [r.encode() for r in d["rows"]]
    d["model"] = m.Vocab(d["vocab_bytes"], d["prefix"].encode(), d["unk"].encode())
    return d


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return m.Harness(str(tmp_path_factory.mktemp("wordpiece")))


def same_as_model(harness, vocab, rows, max_word_chars=100, punct=0, **kw):
    """the header's ids of `rows` against the model's; returns the harness's answer"""
    v = m.Vocab(vocab, kw.get("prefix", b"##"), kw.get("unk", b"[UNK]"))
    got = harness.run(vocab, rows, max_word_chars=max_word_chars, punct=punct, **kw)
    ids, offs = m.tokenize(rows, v, max_word_chars, punct)
    assert got["unk"] == v.unk and got["entries"] == v.entries and got["max_entry_bytes"] == v.max_entry_bytes
    bad = [r for r in range(len(rows)) if got["counts"][r] != offs[r + 1] - offs[r]]
    assert not bad, (bad[:5], rows[bad[0]])
    assert np.array_equal(got["ids"], ids)
    return got


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_what_the_issue_asks_for(golden):
    assert {"##", "#", "###", "##a#", "a##b", "[UNK]"} <= set(golden["vocab"]) and 250 <= len(golden["vocab"]) <= 350
    assert 450 <= len(golden["rows"]) <= 550
    assert {(c["punct"], c["max_word_chars"]) for c in golden["cases"]} >= {(0, 100), (1, 100), (0, 5), (0, 6)}
    widths = {len(ch.encode()) for e in golden["vocab"] for ch in e}
    assert widths == {1, 2, 3, 4}
    for c in golden["cases"][:2]:
        assert 0.02 <= c["unk_share"] <= 0.30
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_model_equals_the_fixture(golden):
    for c in golden["cases"]:
        for row, want in zip(golden["row_bytes"], c["ids"]):
            assert m.row_ids(row, golden["model"], c["max_word_chars"], c["punct"]) == want, (row, c["punct"], c["max_word_chars"])


def test_words_and_pieces_of_the_definition():
    v = m.Vocab([b"[UNK]", b"ab", b"##cd", b"##", b"##ab", b"a", b"##b", None, b"", b"ab", b"#", b","])
    assert v.entries == 9 and v.unk == 0 and v.id_of(b"ab") == 1 and v.id_of(b"") == -1 and v.max_entry_bytes == 5
    assert m.words(b" ab\tcd,e ", 0) == [(1, 3), (4, 8)] and m.words(b" ab\tcd,e ", 1) == [(1, 3), (4, 6), (6, 7), (7, 8)]
    assert m.words(None, 0) == [] and m.words(b" \n", 1) == []
    assert m.row_ids(b"abcd", v) == [1, 2]
    assert m.row_ids(b"abcdx", v) == [0]  # the last piece fails: ab and ##cd are dropped
    assert m.row_ids(b"##ab", v) == [4]  # a word that starts with the prefix finds the whole entry
    assert m.row_ids(b"a##ab", v) == [0]  # ... which is NOT the continuation "##ab" (that would be the entry "####ab")
    assert m.row_ids(b"aab", v) == [5, 4]  # the same entry "##ab" as the continuation "ab"
    assert m.row_ids(b"ab", v) == [1] and m.row_ids(b"abb", v) == [1, 6] and m.row_ids(b"ba", v) == [0]
    assert m.row_ids(b"##", v) == [3] and m.row_ids(b"#", v) == [10] and m.row_ids(b"###", v) == [0]
    assert m.row_ids(b"##,ab", v, punct=1) == [10, 10, 11, 1] and m.row_ids(b"##,ab", v, punct=0) == [0]
    assert m.row_ids(b"abcd", v, max_word_chars=4) == [1, 2] and m.row_ids(b"abcd", v, max_word_chars=3) == [0]
    assert m.boundaries(b"\x80a\x80b") == [0, 1, 3, 4] and m.boundaries(b"\x80\x80") == [0, 2]


# ---- the header against the model ------------------------------------------------------------------------------------------------------
def test_header_equals_the_model_on_the_fixture(golden, harness):
    for c in golden["cases"]:
        got = same_as_model(harness, golden["vocab_bytes"], golden["row_bytes"], c["max_word_chars"], c["punct"])
        assert got["ids"].tolist() == [i for row in c["ids"] for i in row]


@pytest.mark.parametrize("punct", [0, 1])
def test_header_equals_the_model_on_hostile_rows(harness, punct):
    vocab = m.make_vocab(300, 11)
    vocab += [b"\x80", b"##\x80", b"a\x80", b"\xc3", b"a\0b", b"\0", b"##\0", b"\x7f", b"ab\x01cd", b"\xff", b"##b\xfe", b"ab", b"##ab"]
    rows = m.hostile_rows() + m.make_rows(150, 5, null_every=9)
    rows += [bytes(np.random.default_rng(7).integers(0, 256, size=n, dtype=np.uint8)) for n in (1, 5, 33, 64, 65, 200)]
    for mwc in (100, 2, 1):
        same_as_model(harness, vocab, rows, mwc, punct)


def test_duplicate_null_and_empty_vocabulary_rows(harness):
    vocab = [None, b"", b"ab", b"[UNK]", b"ab", b"##c", None, b"##c", b"[UNK]", b"", b"c", b"ab"]
    got = same_as_model(harness, vocab, [b"ab abc c", b"cc", None, b"x"], queries=[b"ab", b"##c", b"[UNK]", b"c", b"", b"x"])
    assert got["entries"] == 4 and got["unk"] == 3
    assert got["found"].tolist() == [2, 5, 3, 10, -1, -1]  # the lowest row of equal ones
    assert got["ids"].tolist() == [2, 2, 5, 10, 10, 5, 3]


def test_a_vocabulary_of_unk_alone(harness):
    rows = m.hostile_rows() + m.make_rows(40, 6)
    for punct in (0, 1):
        got = same_as_model(harness, [b"[UNK]"], rows, 100, punct)
        assert got["entries"] == 1 and set(got["ids"].tolist()) == {0}
    got = same_as_model(harness, [b"<unk>"], rows, unk=b"<unk>")
    assert got["unk"] == 0
    assert harness.run([b"a", b"b"], [b"a"])["unk"] == -1  # unk is no entry: nothing is tokenized


def test_other_prefixes(harness):
    for prefix in (b"_", b"@@", b"12345678"):
        vocab = [b"[UNK]", b"ab", prefix + b"cd", prefix, prefix + prefix, b"cd", prefix + b"ab", b"##cd"]
        rows = [b"abcd", b"cdab", prefix + b"cd", prefix, prefix + prefix, b"ab" + prefix + b"cd", b"ab" + prefix, b"cd##cd", b"abab cdcd"]
        same_as_model(harness, vocab, rows, prefix=prefix)


def test_the_longest_entry_bounds_the_walk(harness):
    long_entry = b"abcdefghij" * 25 + b"abcde"  # 255 bytes
    vocab = [b"[UNK]", long_entry, b"##" + long_entry[:253], b"a", b"##x"]
    rows = [long_entry, long_entry + b"x", b"a" + long_entry[:253], b"a" + long_entry[:253] + b"x", long_entry[:254], b"a" + long_entry[:252]]
    got = same_as_model(harness, vocab, rows, max_word_chars=1024)
    assert got["max_entry_bytes"] == 255 and got["ids"].tolist() == [1, 1, 4, 3, 2, 3, 2, 4, 0, 0]


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def test_the_colliding_pairs_collide():
    a, b = m.SAME_HASH_WHOLE
    assert a != b and len(a) == len(b) and m.murmur3_32(a, m.SEED_WHOLE) == m.murmur3_32(b, m.SEED_WHOLE)
    a, b = m.SAME_HASH_CONT
    assert a != b and len(a) == len(b) and m.murmur3_32(a, m.SEED_CONT) == m.murmur3_32(b, m.SEED_CONT)


def test_every_entry_is_found_and_a_key_that_shares_a_hash_is_not(harness):
    vocab = m.make_vocab(300, 11) + [m.SAME_HASH_WHOLE[0], b"##" + m.SAME_HASH_CONT[0], b"x"]
    v = m.Vocab(vocab)
    queries = list(vocab) + [m.SAME_HASH_WHOLE[1], b"##" + m.SAME_HASH_CONT[1]]
    rows = [m.SAME_HASH_WHOLE[0], m.SAME_HASH_WHOLE[1], b"x" + m.SAME_HASH_CONT[0], b"x" + m.SAME_HASH_CONT[1]]
    got = same_as_model(harness, vocab, rows, queries=queries)
    assert got["found"].tolist() == [v.id_of(q) for q in queries] and got["found"][-2:].tolist() == [-1, -1]
    assert got["ids"].tolist() == [len(vocab) - 3, v.unk, len(vocab) - 1, len(vocab) - 2, v.unk]


def test_keys_that_share_a_slot_of_a_small_table(harness):
    """16 slots and 7 keys (load < 0.5): probe chains exist; for every entry a non-entry that starts at its slot"""
    vocab = [b"[UNK]", b"ab", b"cd", b"##ef", b"gh", b"ij"]
    taken = set(vocab)
    sharers = [m.slot_sharer(e, 16, taken) for e in vocab]
    assert all(len(s) == len(e) and m.murmur3_32(s, m.SEED_WHOLE) % 16 == m.murmur3_32(e, m.SEED_WHOLE) % 16 for s, e in zip(sharers, vocab))
    got = same_as_model(harness, vocab, [b" ".join(vocab), b" ".join(sharers)], queries=vocab + sharers, slots=16)
    assert got["slots"] == 16 and got["found"].tolist() == list(range(6)) + [-1] * 6
    assert harness.run(vocab, [b"ab"])["slots"] == 32  # what the library sizes it to: four slots a row, 16 at least


# ---- encode's helpers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_length,cls,sep", [(1, -1, -1), (1, 1, -1), (2, 1, 2), (2, -1, 2), (8, 1, 2), (8, -1, -1), (3, 1, 2)])
def test_encoded_rows(harness, max_length, cls, sep):
    vocab = m.make_vocab(300, 11)
    v = m.Vocab(vocab)
    rows = m.make_rows(60, 8, null_every=7) + m.hostile_rows()
    got = harness.run(vocab, rows, max_length=max_length, cls=cls, sep=sep, pad=3, punct=1)
    ids, mask = m.encode(rows, v, max_length, cls, sep, 3, punct=1)
    assert np.array_equal(got["encoded"], ids) and np.array_equal(got["mask"], mask)


# ---- the fixture is what the library gives now -----------------------------------------------------------------------------------------------
@pytest.mark.skipif(importlib.util.find_spec("tokenizers") is None, reason="the tokenizers library is not installed")
def test_the_committed_fixture_is_what_the_generator_writes():
    tool = os.path.join(m.ROOT, "tools", "make_wordpiece_golden.py")
    done = subprocess.run([sys.executable, tool, "--check"], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
