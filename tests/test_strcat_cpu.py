"""tests/strcat_model.py checked without a GPU: against the reference's own category vectors (tests/golden), against the C++
oracle's category entries at the key counts the GPU tests use, for the invariants of every result, and the share of the
committed op chains that end in an IndexError."""
import random

import pytest

import cpulibs
import engines
import strcat_model as M
from cpulibs import Col

KS = [0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 5000]
FAMILY = ["to_strings", "gather_strings", "gather", "gather_and_remap", "add_strings", "remove_strings", "merge_category", "merge_and_remap",
          "add_keys", "remove_keys", "set_keys", "remove_unused_keys", "value", "value_for_index", "indexes_for_key"]
GOLDEN = [c for c in engines.load_cases("reference_tests.json") if c["op"] == "category" or c["op"].startswith("cat_")]


def lists(cat):
    return {"keys": M.dec(cat[0]), "values": list(cat[1])}


@pytest.mark.parametrize("case", GOLDEN, ids=[c["id"] for c in GOLDEN])
def test_model_gives_the_reference_vectors(case):
    """python/tests/test_category.py as recorded in tests/golden/reference_tests.json."""
    cat, a = M.from_strings(case["input"]), case["args"].get("arg")
    op = case["op"]
    if op == "category":
        got = lists(cat)
    elif op == "cat_to_strings":
        got = M.dec(M.to_strings(cat))
    elif op == "cat_gather_strings":
        got = M.dec(M.gather_strings(cat, a))
    elif op in ("cat_merge_category", "cat_merge_and_remap"):
        got = lists(getattr(M, op[4:])(cat, M.from_strings(a)))
    else:
        got = lists(getattr(M, op[4:])(cat, a))
    assert got == case["expect"]


def test_golden_covers_what_it_did():
    assert len(GOLDEN) == 13 and {c["op"] for c in GOLDEN} >= {"cat_merge_category", "cat_gather_and_remap", "cat_remove_strings"}


def test_model_has_every_method_of_the_reference_class():
    """tests/golden/reference_python_calls.json lists the methods of the reference's nvcategory.py."""
    calls = {name for name, _ in engines.golden_json("reference_python_calls.json")["calls"]["nvcategory.py"]}
    assert set(FAMILY) <= calls
    for name in FAMILY:
        assert callable(getattr(M, name)) and ":" in getattr(M, name).__doc__, name  # (each names its reference lines)


def test_reference_examples_of_the_key_ops():
    """The key-only expectations of python/tests/test_category.py:191-220 and the worked examples in NVCategory.cu."""
    cat = M.from_strings(["a", "b", "b", "f", "c", "f"])
    assert lists(M.add_keys(cat, ["a", "b", "c", "d"])) == {"keys": ["a", "b", "c", "d", "f"], "values": [0, 1, 1, 4, 2, 4]}  # :1351-1373
    assert lists(M.remove_keys(cat, ["b", "d"])) == {"keys": ["a", "c", "f"], "values": [0, -1, -1, 2, 1, 2]}  # :1457-1479
    assert lists(M.set_keys(cat, ["b", "c", "e", "d"])) == {"keys": ["b", "c", "d", "e"], "values": [-1, 0, 0, -1, 1, -1]}  # :1676-1685
    assert lists(M.remove_unused_keys(M.set_keys(cat, ["b", "c", "e", "d"])))["keys"] == ["b", "c"]
    merged = M.merge_category(cat, M.from_strings(list("aadcce")))  # :1180-1191
    assert lists(merged) == {"keys": list("abcfde"), "values": [0, 1, 1, 3, 2, 3, 0, 0, 4, 2, 2, 5]}
    assert M.value(cat, "c") == 2 and M.value(cat, None) == -1 and M.value(M.from_strings([None, "a"]), None) == 0
    assert M.indexes_for_key(cat, "f") == [3, 5] and M.value_for_index(cat, -1) == -1 and M.value_for_index(cat, 5) == 3
    with pytest.raises(ValueError):
        M.indexes_for_key(cat, "zz")


def state(K, null, rnd, minus_one=False):
    keys = M.key_pool(K, 3, "k")
    cat = M.from_strings(M.rows_over(keys, 3 * K + 37 if K else 0, rnd, null))
    if minus_one and cat[0]:
        cat = M.gather(cat, [rnd.randrange(-1, len(cat[0])) for _ in range(2 * K + 5)])
    return cat


def col(rows):
    return Col.from_list(M.dec(rows))


@pytest.fixture(scope="module")
def oracle():
    return cpulibs.Oracle()


@pytest.mark.parametrize("null", [False, True], ids=["", "null"])
@pytest.mark.parametrize("K", KS)
def test_model_against_the_oracle(oracle, K, null):
    rnd = random.Random(K * 2 + null)
    cat = state(K, null, rnd)
    rows = M.to_strings(cat) or []
    k, v = oracle.category(col(rows))
    assert (k.to_bytes_list(), v.tolist()) == (cat[0], cat[1])
    neg = state(K, null, rnd, minus_one=True)  # -1 values, repeats, unused keys
    nk = len(neg[0])
    # to_strings == the lenient gather of the values; gather_strings the strict one
    assert oracle.cat_gather_strings(col(neg[0]), neg[1], strict=False).to_bytes_list() == (M.to_strings(neg) or [])
    pos = [rnd.randrange(nk) for _ in range(nk // 2 + 3)] if nk else []
    assert oracle.cat_gather_strings(col(neg[0]), pos, strict=True).to_bytes_list() == M.gather_strings(neg, pos)
    gk, gv = oracle.cat_gather_and_remap(col(neg[0]), pos)
    assert (gk.to_bytes_list(), gv.tolist()) == tuple(M.gather_and_remap(neg, pos))
    for bad in ([-1], [nk]):
        for fn, mfn in ((lambda p: oracle.cat_gather_strings(col(neg[0]), p), M.gather_strings),
                        (lambda p: oracle.cat_gather_and_remap(col(neg[0]), p), M.gather_and_remap)):
            with pytest.raises(IndexError):
                fn(pos + bad)
            with pytest.raises(IndexError):
                mfn(neg, pos + bad)
    # add_keys takes -1 values; new keys from the other side of the same edge, about half of them known
    other = M.key_pool({255: 257, 257: 255, 2047: 2049, 2049: 2047}.get(K, K + 1), 4, "n")
    strs = [x for x in M.dec(neg[0]) if rnd.random() < 0.5] + other[: len(other) // 2] + [None]
    ak, av = oracle.cat_add_keys_and_remap(col(neg[0]), neg[1], Col.from_list(strs))
    assert (ak.to_bytes_list(), av.tolist()) == tuple(M.add_keys(neg, strs))


def every_result(cat, rnd):
    """(op, result, keys must be sorted) for every category-returning op on `cat`, with arguments that hit, miss and are empty."""
    keys = M.dec(cat[0])
    nk = len(keys)
    half = [k for k in keys if rnd.random() < 0.5]
    new = M.key_pool(7, 9, "z") + [None]
    other = M.merge_category(M.from_strings(half[:3] + new[:2]), M.from_strings(new + half))  # unsorted argument
    unsorted_in = not M.is_sorted(cat[0])
    yield "copy", M.copy(cat), not unsorted_in
    for strs in ([], half, new, half + new, keys):
        yield "add_strings", M.add_strings(cat, strs), True
        yield "remove_strings", M.remove_strings(cat, strs), True
        yield "add_keys", M.add_keys(cat, strs), bool(strs) or not unsorted_in
        yield "remove_keys", M.remove_keys(cat, strs), (bool(strs) and nk > 0) or not unsorted_in
        yield "set_keys", M.set_keys(cat, strs), True
    yield "remove_unused_keys", M.remove_unused_keys(cat), None  # (a copy when nothing is unused: the order stays)
    for arg in (M.from_strings(half), M.from_strings(new), other, ([], []), ([], [-1, -1])):
        yield "merge_category", M.merge_category(cat, arg), None
        yield "merge_category", M.merge_category(arg, cat), None
        yield "merge_and_remap", M.merge_and_remap(cat, arg), True
    yield "from_categories", M.from_categories([cat, other, cat, ([], [-1])]), True
    pos = [rnd.randrange(nk) for _ in range(nk + 3)] if nk else []
    yield "gather", M.gather(cat, pos + [-1]), not unsorted_in
    yield "gather_and_remap", M.gather_and_remap(cat, pos), not unsorted_in


@pytest.mark.parametrize("K", [0, 1, 2, 40, 257])
def test_every_result_is_a_category(K):
    """Distinct keys, values in [-1, keys), and sorted keys (null first) from every op that does not keep the order it is
    given (M.KEEPS_KEY_ORDER, and the copies add_keys / remove_keys / remove_unused_keys return when they have nothing to do)."""
    rnd = random.Random(K)
    fresh = state(K, True, rnd)
    starts = [fresh, state(K, False, rnd, minus_one=True), M.merge_category(fresh, M.from_strings(M.key_pool(K + 3, 5, "A"))),
              M.set_keys(fresh, []), M.remove_keys(fresh, M.dec(fresh[0])), M.add_keys(fresh, ["zzz unused", None])]
    seen_unsorted = False
    for start in starts:
        seen_unsorted |= not M.is_sorted(start[0])
        for op, res, must_be_sorted in every_result(start, rnd):
            M.check(res, op)
            if must_be_sorted:
                assert M.is_sorted(res[0]), op
    assert seen_unsorted or K < 2  # (keys that sort before "k...": the merged keys are unsorted)


def test_an_emptied_category():
    """The early exits: what each op makes of a category without keys, with rows (all -1) and without."""
    rows3 = ([], [-1, -1, -1])
    assert M.merge_category(rows3, ([], [])) == ([], []) and M.merge_category(([], []), rows3) == ([], [])  # :1230-1231
    full = M.from_strings(["b", "a"])
    assert M.merge_category(rows3, full) == full and M.merge_category(full, rows3) == full  # the three rows are lost
    assert M.add_keys(rows3, []) == ([], []) and M.add_keys(rows3, ["b", "a", "b"]) == ([b"a", b"b"], [-1, -1, -1])
    assert M.set_keys(rows3, []) == ([], []) and M.set_keys(full, []) == ([], [-1, -1])
    assert M.set_keys(rows3, ["x"]) == ([b"x"], [-1, -1, -1])
    assert M.from_categories([rows3, rows3]) == ([], []) and M.from_categories([rows3, full]) == ([b"a", b"b"], [-1, -1, -1, 1, 0])
    assert M.to_strings(([b"a"], [])) is None and M.to_strings(rows3) == [None] * 3
    assert M.remove_unused_keys(([b"a", b"b"], [])) == ([b"a", b"b"], [])  # no rows: nothing counts as unused
    assert M.remove_unused_keys(([b"a", b"b"], [-1, -1])) == ([], [-1, -1])
    assert M.add_strings(rows3, ["q"]) == ([None, b"q"], [0, 0, 0, 1])  # product's rule: -1 is a null row


def test_chains_meet_every_handover_and_seldom_stop_early():
    chains, counts, stopped = M.all_chains()
    assert len(chains) >= 40 and all(6 <= len(steps) <= 10 or steps[-1][2] == "raises" for steps in chains.values())
    assert {M.CHAIN_KS[s % 3] for s in chains} == {40, 300, 2100}
    missing = [h for h in M.HANDOVERS if counts[h] == 0]
    assert not missing, missing
    assert 10 * len(stopped) <= len(chains), stopped
    for steps in chains.values():
        for op, args, kind, want in steps:
            if kind == "cat":
                M.check(want, op)
