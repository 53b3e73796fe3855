"""A numpy model of the numeric categories (custrings_amd/csrc/cs_numcat.hip), written from the rules and not from the
kernels: the build is np.unique plus the null rule and the lowest-index rule, the key-set family is plain Python over
sorted lists.

A category is a Cat: dtype, keys (array), values (int32 array), have_null.  With have_null key 0 is the null key and a row
is null exactly when its value is 0.  Rules: -0.0 and +0.0 are one key, all NaN are one key behind
+inf, and the number kept for a key is that of the lowest-indexed member of its class (old keys before new items)."""
import math

import numpy as np


class Cat:
    def __init__(self, dtype, keys, values, have_null):
        self.dtype = np.dtype(dtype)
        self.keys = np.asarray(keys, dtype=self.dtype).reshape(-1)
        self.values = np.asarray(values, dtype=np.int32).reshape(-1)
        self.have_null = bool(have_null)

    def mask(self):
        """The bitmask the invariant gives (LSB first, 0 = null), or None without a null key / without rows."""
        if not self.have_null or self.values.size == 0:
            return None
        return np.packbits(self.values != 0, bitorder="little")

    def null_rows(self):
        return int((self.values == 0).sum()) if self.have_null else 0


def bits(a):
    """The array's bytes as unsigned integers: what "bit for bit" compares."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def is_null(nulls, i):
    return nulls is not None and ((int(np.asarray(nulls).view(np.uint8)[i >> 3]) >> (i & 7)) & 1) == 0


def valid_rows(n, nulls):
    if nulls is None:
        return np.ones(n, dtype=bool)
    return np.unpackbits(np.asarray(nulls).view(np.uint8), bitorder="little")[:n].astype(bool)


def canon(a):
    """One representative per equality class: +0.0 for the zeros (x + 0.0), one NaN for the NaNs."""
    a = np.asarray(a)
    if a.dtype.kind != "f":
        return a
    c = a + a.dtype.type(0)
    c[np.isnan(a)] = np.nan
    return c


def build(items, nulls=None):
    items = np.asarray(items)
    n = items.size
    if n == 0:
        return Cat(items.dtype, [], [], False)
    ok = valid_rows(n, nulls)
    rows = np.flatnonzero(ok)
    _, first, inverse = np.unique(canon(items[rows]), return_index=True, return_inverse=True, equal_nan=True)
    keys = items[rows[first]]
    values = np.zeros(n, dtype=np.int32)
    have_null = not ok.all()
    values[rows] = inverse.reshape(-1) + (1 if have_null else 0)
    if have_null:
        keys = np.concatenate([items[np.flatnonzero(~ok)[:1]], keys])
    return Cat(items.dtype, keys, values, have_null)


def _order(x):
    """Sort key of a number's class: NaN behind everything, the zeros together."""
    x = x.item() if hasattr(x, "item") else x
    if isinstance(x, float):
        return (1, 0.0) if math.isnan(x) else (0, x + 0.0)
    return (0, x)


def _old(cat):
    """(null key's number or None, [(class, number)] of the other keys, in order)."""
    ks = list(cat.keys)
    null = ks[0] if cat.have_null else None
    return null, [(_order(k), k) for k in ks[1 if cat.have_null else 0:]]


def _new(items, nulls, dtype):
    items = np.asarray(items, dtype=dtype).reshape(-1)
    seen, out, null = set(), [], None
    for i, x in enumerate(items):
        if is_null(nulls, i):
            if null is None:
                null = x
        elif _order(x) not in seen:
            seen.add(_order(x))
            out.append((_order(x), x))
    return null, out


def _remapped(cat, null, pairs, extra_values=None, extra_table=None):
    """The category with keys [null] + pairs (sorted here) and cat's values sent to them by class; -1 where the class is gone."""
    pairs = sorted(pairs, key=lambda p: p[0])
    base = 0 if null is None else 1
    where = {c: base + j for j, (c, _) in enumerate(pairs)}
    old_null, old = _old(cat)
    table = ([0 if null is not None else -1] if cat.have_null else []) + [where.get(c, -1) for c, _ in old]
    values = [v if v < 0 else table[v] for v in cat.values.tolist()]
    if extra_values is not None:
        values += [v if v < 0 else extra_table(where)[v] for v in extra_values]
    keys = ([null] if null is not None else []) + [k for _, k in pairs]
    return Cat(cat.dtype, keys, values, null is not None)


def add_keys(cat, items, nulls=None):
    if np.asarray(items).size == 0:
        return Cat(cat.dtype, cat.keys, cat.values, cat.have_null)
    old_null, old = _old(cat)
    new_null, new = _new(items, nulls, cat.dtype)
    have = {c for c, _ in old}
    return _remapped(cat, old_null if old_null is not None else new_null, old + [p for p in new if p[0] not in have])


def remove_keys(cat, items, nulls=None):
    if np.asarray(items).size == 0:
        return Cat(cat.dtype, cat.keys, cat.values, cat.have_null)
    old_null, old = _old(cat)
    new_null, new = _new(items, nulls, cat.dtype)
    gone = {c for c, _ in new}
    return _remapped(cat, None if new_null is not None else old_null, [p for p in old if p[0] not in gone])


def set_keys(cat, items, nulls=None):
    old_null, old = _old(cat)
    new_null, new = _new(items, nulls, cat.dtype)
    mine = dict(old)
    null = None if new_null is None else (old_null if old_null is not None else new_null)
    return _remapped(cat, null, [(c, mine.get(c, k)) for c, k in new])


def merge(cat, cat2):
    assert cat.dtype == cat2.dtype
    old_null, old = _old(cat)
    null2, keys2 = _old(cat2)
    have = {c for c, _ in old}

    def table2(where):
        return ([0] if cat2.have_null else []) + [where[c] for c, _ in keys2]

    return _remapped(cat, old_null if old_null is not None else null2, old + [p for p in keys2 if p[0] not in have], cat2.values.tolist(), table2)


def _keep_used(cat, vals):
    vals = [int(v) for v in vals]
    used = sorted({v for v in vals if v >= 0})
    table = {k: j for j, k in enumerate(used)}
    return Cat(cat.dtype, cat.keys[used] if used else [], [v if v < 0 else table[v] for v in vals], cat.have_null and 0 in table)


def remove_unused_keys(cat):
    return _keep_used(cat, cat.values.tolist())


def _check(indexes, limit):
    idx = np.asarray(indexes, dtype=np.int32).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= limit):
        raise IndexError("invalid index value")
    return idx


def gather(cat, indexes):
    return Cat(cat.dtype, cat.keys, _check(indexes, cat.keys.size), cat.have_null)


def gather_and_remap(cat, indexes):
    return _keep_used(cat, _check(indexes, cat.keys.size).tolist())


def gather_values(cat, indexes):
    return Cat(cat.dtype, cat.keys, cat.values[_check(indexes, cat.values.size)], cat.have_null)


def to_type(cat):
    """(numbers, bitmask): a value of -1 reads as 0; the bitmask is all ones (within the rows) without null rows."""
    out = np.zeros(cat.values.size, dtype=cat.dtype)
    ok = cat.values >= 0
    out[ok] = cat.keys[cat.values[ok]]
    null = (cat.values == 0) if cat.have_null else np.zeros(cat.values.size, dtype=bool)
    return out, np.packbits(~null, bitorder="little")


def gather_type(cat, indexes):
    idx = _check(indexes, cat.keys.size)
    null = (idx == 0) if cat.have_null else np.zeros(idx.size, dtype=bool)
    return cat.keys[idx], np.packbits(~null, bitorder="little")


def index_for(cat, key):
    if key is None:
        return 0 if cat.have_null else -1
    want = _order(np.asarray([key]).astype(cat.dtype)[0])
    for j, (c, _) in enumerate(_old(cat)[1]):
        if c == want:
            return j + (1 if cat.have_null else 0)
    return -1


def indexes_for(cat, key):
    k = index_for(cat, key)
    return [] if k < 0 else np.flatnonzero(cat.values == k).tolist()
