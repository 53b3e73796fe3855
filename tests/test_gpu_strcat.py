"""-m gpu: the string categories' key and remap family (cs_catops.hip, cs_category_merge, the kernels of cat_remap.h) against
tests/strcat_model.py -- at key counts around one block of 256 and one 2048-row scan chunk, with arguments from the other
side of the same edge, on categories the family itself makes (unsorted keys, -1 values, unused keys, no keys), in seeded
op chains, at every early exit, and the accessors.  Every comparison is exact: the keys byte for byte, both sizes, the
values as int32."""
import random

import numpy as np
import pytest

import gpuutil
import strcat_model as M
from cpulibs import Col

pytestmark = pytest.mark.gpu

KS = [0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 5000]
OTHER_SIDE = {0: 1, 1: 2, 2: 1, 255: 257, 256: 255, 257: 255, 2047: 2049, 2048: 2047, 2049: 2047, 5000: 2049}


class Lib:
    def __init__(self):
        from custrings_amd import _lib, nvcategory, nvstrings

        _lib.ensure_init()
        self.nvc, self.nvs = nvcategory, nvstrings

    def strs(self, rows):
        return self.nvs.to_device(M.dec(M.enc(rows)))

    def cat(self, rows):
        return self.nvc.from_strings(self.strs(rows))

    def recipe(self, r):
        if r[0] == "rows":
            return self.cat(r[1])
        return self.cat(r[1]).merge_category(self.cat(r[2])).gather(r[3])


@pytest.fixture(scope="module")
def L():
    return Lib()


def same(cat, want, what=""):
    keys, values = want
    assert cat.keys_size() == len(keys), what
    assert cat.size() == len(values), what
    gpuutil.assert_same(cat.keys(), Col.from_list(keys), what + ": keys")
    got = np.full(len(values), 7, dtype=np.int32)
    if len(values):
        cat.values(got)
    assert np.array_equal(got, np.asarray(values, dtype=np.int32).reshape(-1)), what + ": values"
    return cat


def same_strings(col, rows, what=""):
    if rows is None:
        assert col is None, what
    else:
        gpuutil.assert_same(col, Col.from_list(rows), what)


def both_raise(fn, mfn):
    with pytest.raises(IndexError):
        mfn()
    with pytest.raises(IndexError):
        fn()


def arguments(K, keys, rnd):
    """Strings with OTHER_SIDE[K] distinct values that overlap the category's keys by about half, not at all, completely."""
    k2 = OTHER_SIDE[K]
    new = M.key_pool(k2, 4, "n")
    own = list(keys)
    rnd.shuffle(own)
    half = own[: k2 // 2] + new[: k2 - len(own[: k2 // 2])]
    out = {"half": half, "none": new, "all": own[:k2] or new[:1]}
    return {name: M.rows_over(M.dec(M.enc(v)), len(v) + 11, rnd) for name, v in out.items()}


@pytest.mark.parametrize("null", [False, True], ids=["nonull", "null"])
@pytest.mark.parametrize("K", KS)
def test_two_argument_ops_at_key_count_edges(L, K, null):
    rnd = random.Random(K * 2 + null)
    rows = M.rows_over(M.key_pool(K, 3, "k"), 3 * K + 37 if K else 0, rnd, null)
    m = M.from_strings(rows)
    g = same(L.cat(rows), m, "from_strings")
    for name, strs in arguments(K, [k for k in m[0] if k is not None], rnd).items():
        if null and name != "none":
            strs = strs + [None]
        s = L.strs(strs)
        for op in ("add_strings", "remove_strings", "add_keys", "remove_keys", "set_keys"):
            same(getattr(g, op)(s), getattr(M, op)(m, strs), "%s(%s)" % (op, name))
        m2, g2 = M.from_strings(strs), L.cat(strs)
        merged = same(g.merge_category(g2), M.merge_category(m, m2), "merge_category(%s)" % name)
        same(g2.merge_category(g), M.merge_category(m2, m), "merge_category(%s) reversed" % name)
        same(g.merge_and_remap(g2), M.merge_and_remap(m, m2), "merge_and_remap(%s)" % name)
        # the merged (unsorted) category into each key op, with the same strings
        mm = M.merge_category(m, m2)
        for op in ("add_keys", "remove_keys", "set_keys"):
            same(getattr(merged, op)(s), getattr(M, op)(mm, strs), "%s(%s) after merge_category" % (op, name))
        same(merged.merge_category(g2.merge_category(g)), M.merge_category(mm, M.merge_category(m2, m)), "merge_category of two merged")


@pytest.mark.parametrize("null", [False, True], ids=["nonull", "null"])
@pytest.mark.parametrize("K", KS)
def test_gathers_at_key_count_edges(L, K, null):
    import torch

    rnd = random.Random(K * 2 + null + 100)
    rows = M.rows_over(M.key_pool(K, 3, "k"), 3 * K + 37 if K else 0, rnd, null)
    m, g = M.from_strings(rows), L.cat(rows)
    nk = len(m[0])
    same_strings(g.to_strings(), M.to_strings(m), "to_strings")
    lists = {"repeats": [rnd.randrange(nk) for _ in range(2 * nk + 3)] if nk else [],
             "every key": rnd.sample(range(nk), nk),
             "one unused": [i for i in range(nk) if i != nk // 2] * 2,
             "key 0 only": [0] * (nk + 5) if nk else [],
             "fewer rows than keys": [rnd.randrange(nk) for _ in range(nk // 2 + 1)] if nk else []}
    for name, pos in lists.items():
        for form, p in (("host", pos), ("device", torch.tensor(pos, dtype=torch.int32, device="cuda"))):
            if form == "device" and not pos:
                continue
            what = "%s, %s" % (name, form)
            same_strings(g.gather_strings(p), M.gather_strings(m, pos), "gather_strings " + what)
            same(g.gather_and_remap(p), M.gather_and_remap(m, pos), "gather_and_remap " + what)
            gg = same(g.gather(p), M.gather(m, pos), "gather " + what)
        # what the gathered category (repeats, unused keys, maybe fewer rows than keys) gives the next op
        mg = M.gather(m, pos)
        same(gg.remove_unused_keys(), M.remove_unused_keys(mg), "remove_unused_keys after gather, " + name)
        same_strings(gg.to_strings(), M.to_strings(mg), "to_strings after gather, " + name)
        same(gg.add_keys(L.strs(["zz new", None])), M.add_keys(mg, ["zz new", None]), "add_keys after gather, " + name)
    if nk:
        pos = lists["repeats"] + [-1, nk - 1, -1]
        for p in (pos, torch.tensor(pos, dtype=torch.int32, device="cuda")):
            gm = same(g.gather(p), M.gather(m, pos), "gather with -1")
        mm = M.gather(m, pos)
        same_strings(gm.to_strings(), M.to_strings(mm), "to_strings with -1")
        strs = M.dec(m[0][: nk // 2 + 1]) + ["zz new"]
        for op in ("add_strings", "remove_strings", "add_keys", "remove_keys", "set_keys"):
            same(getattr(gm, op)(L.strs(strs)), getattr(M, op)(mm, strs), op + " with -1")
        same(gm.remove_unused_keys(), M.remove_unused_keys(mm), "remove_unused_keys with -1")
        same(gm.merge_and_remap(gm), M.merge_and_remap(mm, mm), "merge_and_remap with -1 on both sides")
        same(gm.merge_category(g), M.merge_category(mm, m), "merge_category with -1")
    for bad in ([-1], [nk], [0, -2]):
        both_raise(lambda: g.gather_strings(bad), lambda: M.gather_strings(m, bad))
        both_raise(lambda: g.gather_and_remap(bad), lambda: M.gather_and_remap(m, bad))
    for bad in ([-2], [nk]):
        both_raise(lambda: g.gather(bad), lambda: M.gather(m, bad))


def step(L, g, op, args):
    """One chain step on the product: a category, a strings column (or None), or the accessors' answers."""
    if op == "merge_category_right":
        return L.recipe(args[0]).merge_category(g)
    if op in ("merge_category", "merge_and_remap"):
        return getattr(g, op)(L.recipe(args[0]))
    if op in ("add_keys", "remove_keys", "set_keys", "add_strings", "remove_strings"):
        return getattr(g, op)(L.strs(args[0]))
    if op == "value":
        k = g.value(args[0])
        return k, (g.indexes_for_key(args[0]) if k >= 0 else None), g.value_for_index(args[1])
    return getattr(g, op)(*args)


@pytest.mark.parametrize("seed", M.CHAIN_SEEDS)
def test_chain(L, seed):
    """tests/strcat_model.py chain(seed): the product and the model step by step, compared after every step."""
    steps = M.all_chains()[0][seed]
    rnd = random.Random(1000 + seed)  # chain() draws its first rows with this generator before anything else
    K = M.CHAIN_KS[seed % 3]
    rows = M.rows_over(M.key_pool(K, seed, "k"), 3 * K + 37, rnd, null=seed % 2 == 0)
    g = same(L.cat(rows), M.from_strings(rows), "start")
    for i, (op, args, kind, want) in enumerate(steps):
        what = "seed %d step %d %s" % (seed, i, op)
        if kind == "raises":
            assert i == len(steps) - 1
            with pytest.raises(IndexError):
                step(L, g, op, args)
        elif kind == "cat":
            g = same(step(L, g, op, args), want, what)
        elif kind == "strings":
            same_strings(step(L, g, op, args), want, what)
        else:
            assert step(L, g, op, args) == want, what


def test_chains_meet_every_handover():
    """(the chains test_chain replays; the same counts are asserted on the CPU in test_strcat_cpu.py)"""
    chains, counts, stopped = M.all_chains()
    assert len(chains) >= 40 and all(counts[h] > 0 for h in M.HANDOVERS), counts
    assert 10 * len(stopped) <= len(chains)


FULL = ["b", "a", None, "b", "é"]
NOKEYS3 = ("emptied", FULL[:3])  # three rows of -1 over no keys


def build(L, spec):
    """(model, product) for: a list of rows | ("emptied", rows) = set_keys([]) of them | ("gathered", rows, pos)"""
    if isinstance(spec, list):
        return M.from_strings(spec), L.cat(spec)
    if spec[0] == "emptied":
        return M.set_keys(M.from_strings(spec[1]), []), L.cat(spec[1]).set_keys(L.strs([]))
    return M.gather(M.from_strings(spec[1]), spec[2]), L.cat(spec[1]).gather(spec[2])


EXITS = {
    # merge_category: k1 == 0 || k2 == 0
    "merge_category no keys left": ("merge_category", NOKEYS3, FULL),
    "merge_category no keys right": ("merge_category", FULL, NOKEYS3),
    "merge_category no keys on both sides": ("merge_category", NOKEYS3, ("emptied", ["x"])),
    "merge_category empty left": ("merge_category", [], FULL),
    "merge_category empty right": ("merge_category", FULL, []),
    "merge_category empty both": ("merge_category", [], []),
    "merge_category nothing new": ("merge_category", FULL, ["a", None]),
    "merge_and_remap no keys left": ("merge_and_remap", NOKEYS3, FULL),
    "merge_and_remap no keys right": ("merge_and_remap", FULL, NOKEYS3),
    "merge_and_remap no keys on both sides": ("merge_and_remap", NOKEYS3, NOKEYS3),
    # strs->rows == 0 and cat->keys->rows == 0
    "add_keys no strings": ("add_keys", FULL, []),
    "add_keys no keys": ("add_keys", NOKEYS3, ["q", "p", "q", None]),
    "add_keys no keys, no strings": ("add_keys", NOKEYS3, []),
    "add_keys empty category": ("add_keys", [], ["q", "p"]),
    "remove_keys no strings": ("remove_keys", FULL, []),
    "remove_keys no keys": ("remove_keys", NOKEYS3, ["a"]),
    "remove_keys nothing hit": ("remove_keys", FULL, ["zz", "y"]),
    "remove_keys everything hit": ("remove_keys", FULL, ["é", None, "a", "b", "zz"]),
    "set_keys no strings": ("set_keys", FULL, []),
    "set_keys no strings, no keys": ("set_keys", NOKEYS3, []),
    "set_keys no strings, empty category": ("set_keys", [], []),
    "set_keys no keys": ("set_keys", NOKEYS3, ["q", None, "p"]),
    "add_strings no keys": ("add_strings", NOKEYS3, ["q"]),
    "add_strings nothing": ("add_strings", [], []),
    "remove_strings everything": ("remove_strings", FULL, ["a", "b", "é", None]),
    "remove_strings no rows": ("remove_strings", ("gathered", FULL, []), ["a"]),
    # remove_unused_keys: c.n == nk, c.n == 0, no rows, no keys
    "remove_unused_keys nothing unused": ("remove_unused_keys", FULL),
    "remove_unused_keys everything unused": ("remove_unused_keys", ("gathered", FULL, [-1, -1, -1])),
    "remove_unused_keys one unused": ("remove_unused_keys", ("gathered", FULL, [0, 1, 3, 3, -1])),
    "remove_unused_keys no rows": ("remove_unused_keys", ("gathered", FULL, [])),
    "remove_unused_keys no keys": ("remove_unused_keys", NOKEYS3),
    "gather_and_remap no positions": ("gather_and_remap", FULL, []),
    "gather no positions": ("gather", FULL, []),
    "gather of no keys": ("gather", NOKEYS3, [-1, -1]),
}


@pytest.mark.parametrize("name", list(EXITS))
def test_early_exit(L, name):
    op, left, *rest = EXITS[name]
    m, g = build(L, left)
    if op in ("merge_category", "merge_and_remap"):
        m2, g2 = build(L, rest[0])
        same(getattr(g, op)(g2), getattr(M, op)(m, m2), name)
    elif op in ("gather", "gather_and_remap"):
        same(getattr(g, op)(rest[0]), getattr(M, op)(m, rest[0]), name)
    elif rest:
        same(getattr(g, op)(L.strs(rest[0])), getattr(M, op)(m, rest[0]), name)
    else:
        same(getattr(g, op)(), getattr(M, op)(m), name)


def test_to_strings_and_gather_strings_exits(L):
    m, g = build(L, ("gathered", FULL, []))
    assert g.to_strings() is None and M.to_strings(m) is None  # no rows: no instance
    m, g = build(L, NOKEYS3)
    same_strings(g.to_strings(), M.to_strings(m), "to_strings over no keys")
    same_strings(g.gather_strings([]), [], "gather_strings of nothing")
    both_raise(lambda: g.gather_strings([0]), lambda: M.gather_strings(m, [0]))
    both_raise(lambda: g.gather_and_remap([0]), lambda: M.gather_and_remap(m, [0]))


@pytest.mark.parametrize("null", [False, True], ids=["nonull", "null"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_from_categories_and_from_strings_list(L, n, null):
    rnd = random.Random(n)
    pool = M.key_pool(300, 6, "k")
    lists = [[rnd.choice(pool[40 * i: 40 * i + 90] + ([None] if null else [])) for _ in range(257 + 64 * i)] for i in range(n)]
    same(L.nvc.from_strings_list([L.strs(x) for x in lists]), M.from_strings([r for x in lists for r in x]), "from_strings_list")
    same(L.nvc.from_strings(*[L.strs(x) for x in lists]), M.from_strings([r for x in lists for r in x]), "from_strings")
    same(L.nvc.from_categories([L.cat(x) for x in lists]), M.from_categories([M.from_strings(x) for x in lists]), "from_categories")
    # categories the family made: unsorted keys, -1, no keys
    ms = [M.from_strings(x) for x in lists]
    gs = [L.cat(x) for x in lists]
    ms = [M.merge_category(ms[0], M.from_strings(["A first", "zz"]))] + ms[1:] + [M.set_keys(ms[-1], [])]
    gs = [gs[0].merge_category(L.cat(["A first", "zz"]))] + gs[1:] + [gs[-1].set_keys(L.strs([]))]
    same(L.nvc.from_categories(gs), M.from_categories(ms), "from_categories of made categories")


@pytest.mark.parametrize("null", [False, True], ids=["nonull", "null"])
def test_accessors(L, null):
    import torch

    rnd = random.Random(5 + null)
    rows = M.rows_over(M.key_pool(300, 8, "k"), 937, rnd, null)
    m, g = M.from_strings(rows), L.cat(rows)
    for made_m, made_g in ((m, g), (M.merge_category(m, M.from_strings(["A first", None])), g.merge_category(L.cat(["A first", None]))),
                           (M.gather(m, [5, -1, 5, 0, 299, -1]), g.gather([5, -1, 5, 0, 299, -1]))):
        keys = M.dec(made_m[0])
        for k in keys + [None, "no such key", ""]:
            assert made_g.value(k) == M.value(made_m, k), k
        n = len(made_m[1])
        for idx in (0, n - 1, -1, -n, n, n + 5):
            assert made_g.value_for_index(idx) == M.value_for_index(made_m, idx), idx
        for k in rnd.sample(keys, 25) + [keys[0], keys[-1]]:
            want = M.indexes_for_key(made_m, k)
            assert made_g.indexes_for_key(k) == want, k
            assert made_g.indexes_for_key(k) == [i for i, r in enumerate(M.to_strings(made_m)) if r == M.enc([k])[0] and made_m[1][i] >= 0]
            host = np.full(n + 1, -7, dtype=np.int32)
            assert made_g.indexes_for_key(k, host) == len(want)
            assert host.tolist() == want + [-7] * (n + 1 - len(want))
            dev = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
            assert made_g.indexes_for_key(k, dev) == len(want)
            assert dev.cpu().tolist() == want + [-7] * (n + 1 - len(want))
        for absent in ("no such key",) + (() if None in made_m[0] else (None,)):
            with pytest.raises(ValueError):
                M.indexes_for_key(made_m, absent)
            with pytest.raises(ValueError):
                made_g.indexes_for_key(absent)
    with pytest.raises(ValueError):
        g.indexes_for_key(M.dec(m[0])[-1], np.zeros(0, dtype=np.int32))  # no room for the rows
