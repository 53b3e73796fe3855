"""minhash without a GPU: the model of tests/minhash_model.py on the published MurmurHash3_x86_32 vectors and the worked
example; the fold against `%` at its edges; the permutations pinned; custrings_amd/csrc/minhash_ops.h (the text the kernels
compile), built with g++, against the model on generated rows."""
import itertools

import numpy as np
import pytest

import minhash_model as m

A4 = [1390851129, 4071050725, 647892280, 1695753999]
B4 = [2795742288, 2301595691, 2179419893, 161042648]
EXAMPLE = [("the quick brown fox", "03aa9506 0e0d4976 11f94195 14709336"),
           ("héllo wörld", "07bd58f6 07693d29 5df6240d 0682f785"),
           ("ab", "25236478 dc8bcb2a 58703ebd dab3686a"),
           ("abcd", "907232ea 5ecdf3ff fb825025 ae21860e"),
           ("", "ffffffff ffffffff ffffffff ffffffff")]
# the first three (a, b) of permutations(n, seed=0): pinned once computed
PINNED = [(3793791033, 1853398634), (113532185, 4169906344), (456755563, 1405853452)]


def test_murmur_vectors():
    assert m.murmur3_32(b"", 0) == 0
    assert m.murmur3_32(b"", 1) == 0x514e28b7
    assert m.murmur3_32(b"hello", 0) == 0x248bfa47
    assert m.murmur3_32(b"The quick brown fox jumps over the lazy dog", 0) == 0x2e4ff723


def test_worked_example():
    for text, want in EXAMPLE:
        got = m.signature(text.encode(), 4, 0, A4, B4)
        assert " ".join("%08x" % v for v in got) == want, text
    assert m.signature(None, 4, 0, A4, B4) == [m.NO_GRAM] * 4


def test_ngrams_of_the_definition():
    assert m.ngrams("héllo".encode(), 4) == ["héll".encode(), "éllo".encode()]
    assert m.ngrams(b"ab", 4) == [b"ab"]
    assert m.ngrams(b"\x80\x80", 1) == [] and m.ngrams(b"", 3) == [] and m.ngrams(None, 3) == []
    assert m.ngrams(b"\x80a\x80b\x80", 1) == [b"a\x80", b"b\x80"]  # (bytes in front of the first character belong to no n-gram)
    assert m.ngrams(b"\x80a\x80b\x80", 3) == [b"\x80a\x80b\x80"]  # ... but the whole row is the whole row


def test_fold_against_modulo_at_the_edges():
    edge = [0, 1, 1 << 31, (1 << 32) - 1]
    for h, a, b in itertools.product(edge, repeat=3):
        v = h * a + b
        assert v < 1 << 64 and m.fold61(v) == v % m.P, (h, a, b)
    top = ((1 << 32) - 1) ** 2 + (1 << 32) - 1  # the largest h a + b
    seen = 0
    for centre in (m.P, 2 * m.P, 1 << 61, (1 << 64) - 1):
        for v in range(centre - 2, centre + 3):
            if 0 <= v <= top:
                assert m.fold61(v) == v % m.P, v
                seen += 1
    assert seen == 15  # (2^64 - 1 and its neighbours lie above the largest sum: not reachable)


def test_permutations_are_pinned_and_odd():
    from custrings_amd import minhash

    a, b = minhash.permutations(300, 0)
    assert a.dtype == np.uint32 and b.dtype == np.uint32 and a.shape == (300,) and b.shape == (300,)
    assert list(zip(a[:3].tolist(), b[:3].tolist())) == PINNED
    assert np.all(a & 1 == 1)
    a2, b2 = minhash.permutations(5, 0)
    assert np.array_equal(a2, a[:5]) and np.array_equal(b2, b[:5])
    a3, _ = minhash.permutations(5, 1)
    assert not np.array_equal(a3, a2)


def test_jaccard_estimate_counts_equal_positions():
    from custrings_amd import minhash

    sig = np.array([[1, 2, 3, 4], [1, 9, 3, 8], [1, 2, 3, 4]], dtype=np.uint32)
    assert minhash.jaccard_estimate(sig, 0, 1) == 0.5 and minhash.jaccard_estimate(sig, 0, 2) == 1.0


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return m.Harness(str(tmp_path_factory.mktemp("minhash")))


def _perms(nperm, seed):
    from custrings_amd import minhash

    return minhash.permutations(nperm, seed)


@pytest.mark.parametrize("width", [1, 4, 5, 255])
def test_header_matches_the_model(harness, width):
    rows = m.boundary_rows(min(width, 6)) + m.malformed_rows() + m.mixed_rows(120, 11 + width)
    if width == 255:
        rows += [m.text_row(n, n) for n in (254, 255, 256, 257, 300)]
    a, b = _perms(8, 5)
    a[0], b[0] = 0xFFFFFFFF, 0xFFFFFFFF
    sig, keys, counts, _ = harness.run(rows, width, 77, a, b, 4)
    want = m.signatures(rows, width, 77, a, b)
    assert counts.tolist() == [len(m.ngrams(r, width)) for r in rows]
    assert np.array_equal(sig, want)
    assert np.array_equal(keys, m.band_keys(want, 4))


def test_header_on_the_worked_example_and_hash_row(harness):
    rows = [t.encode() for t, _ in EXAMPLE] + [None, b"hello", b"The quick brown fox jumps over the lazy dog"]
    sig, _, _, hashes = harness.run(rows, 4, 0, A4, B4, 1)
    for got, (_, want) in zip(sig, EXAMPLE):
        assert " ".join("%08x" % v for v in got) == want
    assert hashes.tolist() == [m.murmur3_32(r or b"", 31) for r in rows]  # (NVStrings::hash keeps its seed)
