"""Numeric categories on the GPU, bit for bit against tests/numcat_model.py."""
import json
import os

import numpy as np
import pytest

import numcat_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "reference_numcat.json")) as f:
    CASES = json.load(f)["cases"]
TYPES = ["int8", "int32", "int64", "float32", "float64"]
SIZES = [0, 1, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097, 70000]


@pytest.fixture(scope="module")
def N():
    from custrings_amd import _lib, nvcategory

    _lib.ensure_init()
    return nvcategory


def got(cat):
    """What the library holds, as a model Cat plus the bitmask and flags it reports."""
    from custrings_amd import _lib

    dt = np.dtype(cat.keys_type())
    keys = np.zeros(cat.keys_size(), dtype=dt)
    vals = np.zeros(cat.size(), dtype=np.int32)
    if keys.size:
        cat.keys(keys)
    if vals.size:
        cat.values(vals)
    c = M.Cat(dt, keys, vals, cat.keys_have_null())
    mask = None
    if cat.nulls_cpointer():
        import ctypes

        mask = np.zeros((vals.size + 7) // 8, dtype=np.uint8)
        hip = _lib.loaded_hip()
        assert hip.hipMemcpy(ctypes.c_void_p(mask.ctypes.data), ctypes.c_void_p(cat.nulls_cpointer()), ctypes.c_size_t(mask.size), 2) == 0
    return c, mask


def same(cat, want):
    c, mask = got(cat)
    assert c.dtype == want.dtype
    assert c.have_null == want.have_null
    assert c.values.tolist() == want.values.tolist()
    assert M.bits(c.keys).tolist() == M.bits(want.keys).tolist()
    wm = want.mask()
    assert (mask is None) == (wm is None)
    if wm is not None:
        assert mask.tolist() == wm.tolist()
    assert cat.has_nulls() == (want.null_rows() > 0)


# ---- the reference's known answers ------------------------------------------------------------------------------------------
def library_answer(N, case):
    dt = np.dtype(case["dtype"])
    nulls = np.array(case["nulls"], dtype=np.uint8).view(np.int8) if "nulls" in case else None
    cat = N.from_numbers(np.array(case["items"], dtype=dt), nulls)
    op, arg = case["op"], case.get("arg")

    def kv(c):
        k = np.empty(c.keys_size(), dtype=dt)
        v = np.empty(c.size(), dtype=np.int32)
        c.keys(k)
        c.values(v)
        return dict(keys=k.tolist(), values=v.tolist())

    if op == "size":
        return cat.size()
    if op == "keys_size":
        return cat.keys_size()
    if op == "keys":
        return kv(cat)["keys"]
    if op == "values":
        return kv(cat)["values"]
    if op == "keys_values":
        return kv(cat)
    if op == "keys_type":
        return cat.keys_type()
    if op == "indexes_for_key":
        idx = np.empty(cat.indexes_for_key(arg), dtype=np.int32)
        assert cat.indexes_for_key(arg, idx) == idx.size
        return idx.tolist()
    if op == "to_numbers":
        out = np.empty(cat.size(), dtype=dt)
        cat.to_numbers(out)
        return out.tolist()
    if op == "gather_numbers":
        out = np.empty(len(arg), dtype=dt)
        cat.gather_numbers(np.array(arg, dtype=np.int32), out)
        return out.tolist()
    if op == "merge_and_remap":
        return kv(cat.merge_and_remap(N.from_numbers(np.array(arg, dtype=dt))))
    if op == "add_keys_then_remove_unused":
        return kv(cat.add_keys(np.array(arg, dtype=dt)).remove_unused_keys())
    if op.endswith("_keys"):
        return kv(getattr(cat, op)(np.array(arg, dtype=dt)))
    return kv(getattr(cat, op)(np.array(arg, dtype=np.int32)))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden(N, case):
    assert library_answer(N, case) == case["expected"]


# three of them through the CPython glue, on C++ instances (what the reference's nvcategory.py does with its m_cptr)
def glue_answer(P, case):
    dt = np.dtype(case["dtype"])
    c = P.n_createCategoryFromNumbers(np.array(case["items"], dtype=dt), np.array(case["nulls"], dtype=np.uint8).view(np.int8) if "nulls" in case else None)
    made = [c]

    def kv(h):
        k, v = np.empty(P.n_keys_size(h), dtype=dt), np.empty(P.n_size(h), dtype=np.int32)
        P.n_get_keys(h, k)
        P.n_get_values(h, v)
        return dict(keys=k.tolist(), values=v.tolist())

    try:
        assert P.n_keys_type(c) == dt.name
        op, arg = case["op"], case.get("arg")
        if op == "keys_values":
            return kv(c)
        if op == "merge_and_remap":
            made.append(P.n_createCategoryFromNumbers(np.array(arg, dtype=dt), None))
            made.append(P.n_merge_and_remap(c, made[-1]))
            return kv(made[-1])
        if op == "gather_numbers":
            out = np.empty(len(arg), dtype=dt)
            P.n_gather_numbers(c, np.array(arg, dtype=np.int32), out, None)
            return out.tolist()
        made.append(getattr(P, "n_" + op)(c, np.array(arg, dtype=dt), None))
        return kv(made[-1])
    finally:
        for h in made:
            P.n_destroyCategory(h)


@pytest.mark.parametrize("name", ["nulls", "merge_category", "set_keys", "gather_numbers"])
def test_golden_through_the_glue(N, name):
    import pyniNVCategory as P

    case = [c for c in CASES if c["name"] == name][0]
    assert glue_answer(P, case) == case["expected"]


def test_glue_takes_the_python_object_and_keeps_strings_apart(N):
    import pyniNVCategory as P

    cat = N.from_numbers(np.array([5, 7, 5, 9], dtype=np.int32), np.array([0b0101], dtype=np.int8))
    assert P.n_keys_type(cat) == "int32" and P.n_size(cat) == 4 and P.n_keys_size(cat) == 2
    assert P.n_get_keys(cat, None) == [None, 5] and P.n_get_values(cat, None) == [1, None, 1, None]
    assert P.n_get_indexes_for_key(cat, 5, 0) == 2 and P.n_get_indexes_for_key(cat, None, 0) == 2
    rows = np.full(3, -7, dtype=np.int32)
    assert P.n_get_indexes_for_key(cat, 5, rows) == 2 and rows.tolist() == [0, 2, -7]
    with pytest.raises(ValueError):
        P.n_get_indexes_for_key(cat, 5, np.zeros(1, dtype=np.int32))  # too short
    small = N.from_numbers(np.array([44, 1, 44], dtype=np.int8))
    for key in (300, 1.5, float("nan"), 2 ** 70):
        assert P.n_get_indexes_for_key(small, key, 0) == 0, key  # none of int8's values: absent, not truncated to 44
    assert P.n_get_indexes_for_key(small, 44, 0) == 2 and P.n_get_indexes_for_key(small, 44.0, 0) == 2
    strs = N.to_device(["b", "a", "b"])
    h = P.n_createCategoryFromHostStrings(["b", "a", "b"])  # (a string category's own entry points take the C++ pointer)
    assert P.n_keys_type(h) == "str" and P.n_size(h) == 3 and P.n_keys_size(h) == 2  # the string path, as before
    with pytest.raises(ValueError):
        P.n_merge_and_remap(h, cat)
    P.n_destroyCategory(h)
    with pytest.raises(ValueError):
        P.n_to_strings(cat)
    with pytest.raises(ValueError):
        P.n_get_keys(cat, np.zeros(1, dtype=np.int32))  # too short
    with pytest.raises(ValueError):
        P.n_get_keys(cat, np.zeros(2, dtype=np.int64))  # another type
    with pytest.raises(ValueError, match="invalid dtype in nvcategory dispatcher"):
        P.n_createCategoryFromNumbers(np.array([1, 2], dtype=np.uint16), None)
    for short in (lambda: cat.to_numbers(np.zeros(3, dtype=np.int32)), lambda: cat.keys(np.zeros(1, dtype=np.int32)),
                  lambda: cat.gather_numbers(np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32)),
                  lambda: cat.indexes_for_key(5, np.zeros(1, dtype=np.int32)), lambda: strs.merge_and_remap(cat)):
        with pytest.raises(ValueError):
            short()


def test_lists_hold_none_for_nulls(N):
    cat = N.from_numbers(np.array([5, 7, 5, 9], dtype=np.int32), np.array([0b0101], dtype=np.int8))
    assert cat.keys() == [None, 5] and cat.values() == [1, None, 1, None]
    assert N.from_numbers(np.array([2, 1], dtype=np.int64)).keys() == [1, 2]
    assert N.to_device(["b", "a"]).keys_type() == "str"


# ---- build shapes ---------------------------------------------------------------------------------------------------------------
def columns(dt, n):
    """name -> items for one type and row count."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(n * 7 + dt.itemsize)
    cols = {"equal": np.full(n, 3, dtype=dt), "k3": rng.integers(-1, 2, n).astype(dt)}
    if dt.name != "int8" or n <= 256:
        cols["distinct"] = rng.permutation(n).astype(np.int64).astype(dt) if dt.name == "int8" else (rng.permutation(n) - n // 2).astype(dt)
        if dt.name == "int8":
            cols["distinct"] = (rng.permutation(256)[:n] - 128).astype(dt)
    cols["negatives"] = rng.integers(-100, 100, n).astype(dt)
    if dt.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[dt.itemsize]
        nan = int(np.array([np.nan], dtype=dt).view(u)[0])
        sign = 1 << (8 * dt.itemsize - 1)
        pool = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -1.5], dtype=dt), np.array([1, sign | 1, 2, nan, nan | 3, nan | sign | 9], dtype=u).view(dt)])
        cols["specials"] = pool[rng.integers(0, pool.size, n)]
        cols["minus_zero_first"] = np.concatenate([np.array([-0.0], dtype=dt), np.zeros(max(n - 1, 0), dtype=dt)])[:n]
    if dt.name == "int64":
        cols["top_byte"] = (rng.integers(-128, 128, n).astype(np.int64) << 56)
        cols["bottom_byte"] = (np.int64(0x0102030405060700) + rng.integers(0, 256, n).astype(np.int64))
        cols["extremes"] = np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min, -1, 0], dtype=np.int64)[rng.integers(0, 4, n)]
    return cols


@pytest.mark.parametrize("dt", TYPES)
def test_build_shapes(N, dt):
    for n in SIZES:
        for name, items in columns(dt, n).items():
            try:
                same(N.from_numbers(items), M.build(items))
            except AssertionError as e:
                raise AssertionError("%s n=%d %s: %s" % (dt, n, name, e))


def masks(n):
    rng = np.random.default_rng(n)
    out = {"all_ones": np.ones(n, dtype=bool), "all_null": np.zeros(n, dtype=bool), "random": rng.random(n) < 0.7}
    first, last = np.ones(n, dtype=bool), np.ones(n, dtype=bool)
    first[0], last[-1] = False, False
    out["first_null"], out["last_null"] = first, last
    return {k: np.packbits(v, bitorder="little") for k, v in out.items()}


@pytest.mark.parametrize("dt", ["int32", "int64", "float64"])
def test_nulls(N, dt):
    for n in (1, 8, 9, 65, 4097):
        items = np.arange(n).astype(dt) % 5  # the null rows hold different numbers: the null key's number is the first one's
        items[::2] += 100
        for name, mask in masks(n).items():
            try:
                same(N.from_numbers(items, mask.view(np.int8)), M.build(items, mask))
            except AssertionError as e:
                raise AssertionError("%s n=%d %s: %s" % (dt, n, name, e))


# ---- the read side -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", TYPES)
def test_to_numbers_round_trip(N, dt):
    items = columns(dt, 4097)["specials" if np.dtype(dt).kind == "f" else "negatives"]
    mask = masks(4097)["random"]
    for nulls in (None, mask):
        cat = N.from_numbers(items, None if nulls is None else nulls.view(np.int8))
        want, wmask = M.to_type(M.build(items, nulls))
        out, omask = np.full(items.size, 9, dtype=dt), np.full((items.size + 7) // 8, 0x55, dtype=np.uint8)
        cat.to_numbers(out, omask)
        assert M.bits(out).tolist() == M.bits(want).tolist() and omask.tolist() == wmask.tolist()
        ok = M.valid_rows(items.size, nulls) & ~(np.isnan(items) | (items == 0) if np.dtype(dt).kind == "f" else np.zeros(items.size, dtype=bool))
        assert M.bits(out[ok]).tolist() == M.bits(items[ok]).tolist()  # bitwise but for NaN payloads and zero signs
        if nulls is None:
            assert (omask[:-1] == 0xFF).all()  # a passed null buffer is written even when no row is null


def test_gather_numbers(N):
    items = np.array([4.5, 1, 2, 3, 2, 1], dtype=np.float64)
    cat = N.from_numbers(items, np.array([0b111101], dtype=np.int8))
    m = M.build(items, np.array([0b111101], dtype=np.uint8))
    idx = np.array([0, 4, 1, 0, 2, 2, 3, 1, 0], dtype=np.int32)
    out, mask = np.zeros(idx.size), np.zeros(2, dtype=np.uint8)
    cat.gather_numbers(idx, out, mask)
    want, wmask = M.gather_type(m, idx)
    assert out.tolist() == want.tolist() and mask.tolist() == wmask.tolist()
    for bad in (-1, cat.keys_size()):
        with pytest.raises(IndexError):
            cat.gather_numbers(np.array([0, bad], dtype=np.int32), np.zeros(2))
        for fn in (cat.gather, cat.gather_and_remap):
            with pytest.raises(IndexError):
                fn(np.array([0, bad], dtype=np.int32))
    for bad in (-1, cat.size()):
        with pytest.raises(IndexError):
            cat.gather_values(np.array([bad], dtype=np.int32))


def test_indexes_for_key(N):
    items = (np.arange(5000) % 7).astype(np.int32)
    mask = masks(5000)["random"]
    cat, m = N.from_numbers(items, mask.view(np.int8)), M.build(items, mask)
    for key in (3, 99, None, 0):
        want = M.indexes_for(m, key)
        assert cat.value(key) == M.index_for(m, key)
        n = cat.indexes_for_key(key)
        idx = np.full(n + 1, -7, dtype=np.int32)
        assert cat.indexes_for_key(key, idx) == n == len(want)
        assert idx[:n].tolist() == want and idx[n] == -7
    # a number that is none of the type's values is absent, never truncated to one that is
    small = N.from_numbers(np.array([44, 1, 44], dtype=np.int8))
    for key in (300, 44 + 256, 1.5, float("nan"), float("inf"), 2 ** 70):
        assert small.value(key) == -1 and small.indexes_for_key(key) == 0, key
    assert small.value(44) == 1 and small.value(44.0) == 1 and small.indexes_for_key(44) == 2
    wide = N.from_numbers(np.array([7, 2 ** 32 + 7], dtype=np.int64))
    assert N.from_numbers(np.array([7], dtype=np.int32)).value(2 ** 32 + 7) == -1 and wide.value(2 ** 32 + 7) == 1
    plain = N.from_numbers(items)
    assert plain.value(None) == -1 and plain.indexes_for_key(None) == 0 and plain.value(99) == -1 and plain.indexes_for_key(99) == 0


# ---- the key-set family ---------------------------------------------------------------------------------------------------------
def key_arguments(keys, dt):
    """empty, disjoint, overlapping, identical -- each without and with a null item."""
    k = np.asarray(keys)
    lo = k.min() if k.size else 0
    disjoint = (np.arange(max(k.size, 2)) + 1000).astype(dt)[::-1]
    args = {"empty": np.array([], dtype=dt), "disjoint": disjoint, "overlapping": np.concatenate([disjoint[:2], k[::2], k[:1]]).astype(dt), "identical": k.astype(dt)[::-1].copy()}
    out = {}
    for name, a in args.items():
        out[name] = (a, None)
        if a.size:
            bitsv = np.ones(a.size, dtype=bool)
            bitsv[a.size // 2] = False
            out[name + "+null"] = (a, np.packbits(bitsv, bitorder="little"))
    return out


@pytest.mark.parametrize("nkeys", [1, 64, 4097])
@pytest.mark.parametrize("with_null", [False, True])
def test_key_set_family(N, nkeys, with_null):
    dt = np.dtype("float64" if nkeys == 64 else "int64")
    rng = np.random.default_rng(nkeys)
    items = (rng.integers(0, nkeys, nkeys * 2) * 3 - 40).astype(dt)
    items[:nkeys] = (np.arange(nkeys) * 3 - 40).astype(dt)  # every key is there
    mask = None
    if with_null:
        b = np.ones(items.size, dtype=bool)
        b[nkeys::5] = False
        mask = np.packbits(b, bitorder="little")
    cat, m = N.from_numbers(items, None if mask is None else mask.view(np.int8)), M.build(items, mask)
    same(cat, m)
    assert m.keys.size == nkeys + (1 if with_null else 0)
    nonnull = m.keys[1 if with_null else 0:]
    for name, (a, nl) in key_arguments(nonnull, dt).items():
        gl = None if nl is None else nl.view(np.int8)
        try:
            same(cat.add_keys(a, gl), M.add_keys(m, a, nl))
            same(cat.remove_keys(a, gl), M.remove_keys(m, a, nl))
            same(cat.set_keys(a, gl), M.set_keys(m, a, nl))
            other, mo = N.from_numbers(a, gl), M.build(a, nl)
            same(cat.merge_and_remap(other), M.merge(m, mo))
            same(other.merge_and_remap(cat), M.merge(mo, m))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
    grown, mg = cat.add_keys(np.array([7777, 8888], dtype=dt)), M.add_keys(m, np.array([7777, 8888], dtype=dt))
    same(grown.remove_unused_keys(), M.remove_unused_keys(mg))
    same(cat.remove_unused_keys(), M.remove_unused_keys(m))
    same(cat.copy(), m)
    idx = rng.integers(0, m.keys.size, 300).astype(np.int32)
    idx[:3] = 0
    same(cat.gather(idx), M.gather(m, idx))
    same(cat.gather_and_remap(idx), M.gather_and_remap(m, idx))
    no_zero = np.maximum(idx, 1) if m.keys.size > 1 else idx  # key 0 (the null key, when there is one) is not named
    same(cat.gather_and_remap(no_zero), M.gather_and_remap(m, no_zero))
    rows = rng.integers(0, items.size, 300).astype(np.int32)
    same(cat.gather_values(rows), M.gather_values(m, rows))
    # a null key that no row uses is removed with the unused keys
    unused = cat.add_keys(np.array([5], dtype=dt), np.array([0], dtype=np.int8)) if not with_null else cat.gather_values(np.flatnonzero(m.values != 0).astype(np.int32)[:50])
    mu = M.add_keys(m, np.array([5], dtype=dt), np.array([0], dtype=np.uint8)) if not with_null else M.gather_values(m, np.flatnonzero(m.values != 0).astype(np.int32)[:50])
    same(unused, mu)
    same(unused.remove_unused_keys(), M.remove_unused_keys(mu))


def test_types_must_match(N):
    a, b = N.from_numbers(np.array([1, 2], dtype=np.int32)), N.from_numbers(np.array([1.0, 2.0], dtype=np.float64))
    with pytest.raises(ValueError):
        a.merge_and_remap(b)
    for fn in (a.add_keys, a.remove_keys, a.set_keys):
        with pytest.raises(ValueError):
            fn(np.array([1.0]))
    with pytest.raises(ValueError):
        a.to_numbers(np.zeros(2, dtype=np.int64))
    with pytest.raises(ValueError, match="invalid dtype in nvcategory dispatcher"):
        N.from_numbers(np.array([1, 2], dtype=np.uint8))
    d = N.from_numbers(np.array(["2020-01-02", "2020-01-01", "2020-01-02"], dtype="datetime64[D]"))
    assert d.keys_type() == "int64" and d.values() == [1, 0, 1]


# ---- inputs and outputs on the device ---------------------------------------------------------------------------------------
def test_device_tensors(N):
    import torch

    items = columns("float64", 4097)["specials"]
    m = M.build(items)
    big = torch.zeros(items.size + 11, dtype=torch.float64, device="cuda")
    big[:] = float("nan")
    big[3:3 + items.size] = torch.from_numpy(items).cuda()  # a borrowed input at an odd element offset inside a larger buffer
    cat = N.from_numbers(big[3:3 + items.size])
    big.zero_()  # the category owns its buffers
    torch.cuda.synchronize()
    same(cat, m)
    out = torch.full((items.size + 2,), 5.0, dtype=torch.float64, device="cuda")
    omask = torch.full(((items.size + 7) // 8 + 1,), 0x11, dtype=torch.uint8, device="cuda")
    cat.to_numbers(out[1:1 + items.size], omask[1:])
    want, wmask = M.to_type(m)
    assert M.bits(out[1:-1].cpu().numpy()).tolist() == M.bits(want).tolist() and out[0].item() == 5.0 and out[-1].item() == 5.0
    assert omask[1:].cpu().numpy().tolist() == wmask.tolist() and omask[0].item() == 0x11
    keys = torch.zeros(cat.keys_size(), dtype=torch.float64, device="cuda")
    vals = torch.zeros(cat.size(), dtype=torch.int32, device="cuda")
    cat.keys(keys)
    cat.values(vals)
    assert M.bits(keys.cpu().numpy()).tolist() == M.bits(m.keys).tolist() and vals.cpu().numpy().tolist() == m.values.tolist()
    i8 = torch.from_numpy(np.array([3, -3, 3, 0], dtype=np.int8)).cuda()
    same(N.from_numbers(i8), M.build(np.array([3, -3, 3, 0], dtype=np.int8)))
    idx = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    same(cat.gather(idx), M.gather(m, [1, 0, 1]))
