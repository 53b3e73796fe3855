"""A plain-Python model of the string categories' key and remap family (custrings_amd/csrc/cs_catops.hip, cs_category_merge
in cs_category.hip), written from the rules of the reference (cpp/src/category/NVCategory.cu; the line numbers in the
docstrings are that file's) and not from the kernels.

A category is a pair (keys, values): keys a list of bytes with None for the null key, values a list of int.  Nothing here
assumes that the keys are sorted or that the values are non-negative: merge_category returns unsorted keys, remove_keys and
set_keys return values of -1, gather takes -1 and repeats, add_keys returns keys no row uses -- and every function takes such
a category as well as a fresh one.

The reference keeps two facts about a category that (keys, values) does not show: whether it has a key list at all (pList)
and whether it has a value list (pMap).  They differ only for categories without keys or without rows.  Where the
reference's result depends on them, or on memory it never wrote, the function says so, follows the product and is listed
in PRODUCTS_RULE; no test may depend on the reference there."""

# op -> the inputs on which the reference's result is undefined or depends on state (keys, values) does not show
PRODUCTS_RULE = {
    "add_strings": "a value of -1 (create_index :694 reads keys[-1]); the product takes such a row as a null row",
    "remove_strings": "a value of -1 (create_index :694 reads keys[-1]); the product keeps such a row, as a null row, whatever "
                      "strs holds: a row without a key matches no string",
    "copy": "a category without keys (NVCategoryImpl_copy :524 drops the rows when there is no key list, keeps them when the "
            "list is there and empty: set_keys([]) makes the first kind, remove_keys of every key the second); the "
            "product keeps the rows.  Reached through add_keys([]), remove_keys, remove_unused_keys and merge_category",
    "indexes_for_key": "a key whose index is not below the number of rows (get_indexes_for :887-889 compares the KEY index "
                       "with the ROW count and reports the key as absent); the product returns the rows",
}


def sort_key(k):
    """Null first, then unsigned bytewise order, a prefix before the longer string: the comparator every sort of the
    reference uses, `(lhs && rhs) ? lhs->compare(*rhs) < 0 : rhs != 0` (:250-255, :1262, :1423)."""
    return (k is not None, b"" if k is None else k)


def sorted_keys(keys):
    return sorted(set(keys), key=sort_key)


def is_sorted(keys):
    return all(sort_key(a) < sort_key(b) for a, b in zip(keys, keys[1:]))


def enc(strs):
    """list of str / bytes / None -> list of bytes / None"""
    return [None if x is None else (x.encode("utf8") if isinstance(x, str) else bytes(x)) for x in strs]


def dec(rows):
    return [None if x is None else x.decode("utf8") for x in rows]


def remap(keys, values, new_keys):
    """Each value through old key -> place in new_keys; a key that is gone gives -1, a negative value stays
    (`v < 0 ? v : d_y[v]`, :1446, :1557, :1664, :1816)."""
    where = {k: i for i, k in enumerate(new_keys)}
    table = [where.get(k, -1) for k in keys]
    return list(new_keys), [v if v < 0 else table[v] for v in values]


def from_strings(rows):
    """NVCategoryImpl_init :220-304: keys = the distinct rows sorted (null first), values = each row's place."""
    rows = enc(rows)
    keys = sorted_keys(rows)
    where = {k: i for i, k in enumerate(keys)}
    return keys, [where[r] for r in rows]


def copy(cat):
    """NVCategoryImpl_copy :522-558: the same keys in the same order, the same values.  Product's rule for a category
    without keys (PRODUCTS_RULE["copy"]): the rows stay."""
    return list(cat[0]), list(cat[1])


def to_strings(cat):
    """:977-1009.  No rows: no instance (None, :981-982).  A value of -1 gives a null row (:992-993 read the key only for
    `stridx >= 0`), and so does the null key."""
    keys, values = cat
    if not values:
        return None
    return [None if v < 0 else keys[v] for v in values]


def _rows(cat):
    return to_strings(cat) or []


def gather_strings(cat, pos):
    """:1011-1059.  keys[pos[i]]; a position below 0 (-1 too) or not below the key count raises (:1032-1036, :1055-1056)."""
    keys, _ = cat
    if any(p < 0 or p >= len(keys) for p in pos):
        raise IndexError("gather_strings: position out of range")
    return [keys[p] for p in pos]


def gather(cat, pos):
    """:1142-1172.  The same keys in the same order, the positions as values; -1 is allowed, below -1 or not below the key
    count raises (:1157-1164)."""
    keys, _ = cat
    if any(p < -1 or p >= len(keys) for p in pos):
        raise IndexError("gather: position out of range")
    return list(keys), list(pos)


def gather_and_remap(cat, pos):
    """:1084-1139.  Only the keys the positions name, IN THE ORDER THEY HAVE (copy_if over the key indexes, :1127), values
    renumbered; any position below 0 raises, -1 included (:1096-1103)."""
    keys, _ = cat
    if any(p < 0 or p >= len(keys) for p in pos):
        raise IndexError("gather_and_remap: position out of range")
    used = set(pos)
    return remap(keys, pos, [k for i, k in enumerate(keys) if i in used])


def add_strings(cat, strs):
    """:926-938: the category of (this category's rows ++ strs), so sorted keys and no unused key.  Product's rule for a
    value of -1 (PRODUCTS_RULE["add_strings"]): a null row."""
    return from_strings(_rows(cat) + enc(strs))


def remove_strings(cat, strs):
    """:942-974: the category of this category's rows without those equal to a row of strs; null equals null (:961).
    Product's rule for a value of -1 (PRODUCTS_RULE["remove_strings"]): the row has no key, so no string removes it, and it
    stays as a null row."""
    keys, values = cat
    gone = set(enc(strs))
    return from_strings([None if v < 0 else keys[v] for v in values if v < 0 or keys[v] not in gone])


def merge_category(cat, cat2):
    """:1223-1336.  Neither side has keys: an empty category, NO rows (:1230-1231).  One side has no keys: a copy of the
    other alone, the rows of the side without keys are lost (:1235-1239).  Else keys = this category's keys as they are,
    then cat2's keys that are new in SORTED order whatever order cat2 holds them in (they are taken from the sorted
    concatenation, :1260, :1284-1291); values = these values, then cat2's renumbered, a negative value as it is
    (:1326-1331).  Both sides may hold unsorted keys; the result is unsorted unless the new keys all sort behind."""
    (k1, v1), (k2, v2) = cat, cat2
    if not k1 and not k2:
        return [], []
    if not k1 or not k2:
        return copy(cat2 if not k1 else cat)
    have = set(k1)
    merged = list(k1) + sorted_keys(k for k in k2 if k not in have)
    return merged, list(v1) + remap(k2, v2, merged)[1]


def from_categories(cats):
    """create_from_categories :430-514 (merge_and_remap :1339-1345 is this with two).  No key anywhere: an empty category,
    no rows (:443-444).  Else keys = the sorted union (null first), values = all the values in order, renumbered; a negative
    value stays as it is on either side (:505)."""
    if not any(k for k, _ in cats):
        return [], []
    keys = sorted_keys(k for ks, _ in cats for k in ks)
    values = []
    for ks, vs in cats:
        values += remap(ks, vs, keys)[1]
    return keys, values


def merge_and_remap(cat, cat2):
    """:1339-1345: create_from_categories of the two, so a value of -1 stays -1 on either side (:505)."""
    return from_categories([cat, cat2])


def add_keys(cat, strs):
    """add_keys_and_remap :1375-1452.  No keys and no strs: an empty category, NO rows (:1380-1381).  No strs: a copy, the
    keys in the order they have (:1382-1383).  No keys: sorted distinct strs, the values as they are (:1390-1406).  Else the
    sorted union -- the stable sort of :1423 sorts the old keys too, so unsorted keys come out sorted -- and the values
    follow their keys."""
    keys, values = cat
    strs = enc(strs)
    if not keys and not strs:
        return [], []
    if not strs:
        return copy(cat)
    if not keys:
        return sorted_keys(strs), list(values)
    return remap(keys, values, sorted_keys(list(keys) + strs))


def remove_keys(cat, strs):
    """remove_keys_and_remap :1482-1563.  No keys or no strs: a copy, the keys in the order they have (:1486-1487).  Else
    the keys that are in no row of strs, SORTED (they are picked from the sorted concatenation, :1510, :1528-1543), values
    of removed keys -1."""
    keys, values = cat
    gone = set(enc(strs))
    if not keys or not strs:
        return copy(cat)
    return remap(keys, values, sorted_keys(k for k in keys if k not in gone))


def remove_unused_keys(cat):
    """remove_unused_keys_and_remap :1567-1669.  No keys: a copy (:1571-1572).  No rows: a copy too, every key stays
    (:1581-1594: without a value list nothing is counted as unused).  Every key used: a copy, the keys in the order they
    have (:1593-1594).  Else the used keys SORTED (:1622, :1639-1654); negative values stay."""
    keys, values = cat
    used = {v for v in values if v >= 0}
    if not keys or not values or len(used) == len(keys):
        return copy(cat)
    return remap(keys, values, sorted_keys(k for i, k in enumerate(keys) if i in used))


def set_keys(cat, strs):
    """set_keys_and_remap :1708-1822.  No keys and no strs: an empty category, NO rows (:1714-1715).  No strs: no keys, as
    many rows as before, every value -1 (:1716-1720).  No keys: sorted distinct strs, the values as they are (:1726-1742).
    Else keys = sorted distinct strs, values of keys that are gone -1; unsorted old keys change nothing."""
    keys, values = cat
    strs = enc(strs)
    if not keys and not strs:
        return [], []
    if not strs:
        return [], [-1] * len(values)
    if not keys:
        return sorted_keys(strs), list(values)
    return remap(keys, values, sorted_keys(strs))


def value(cat, s):
    """get_value(const char*) :766-793: the index of the key equal to s, -1 when there is none; None finds the null key
    (:785 "only true if both are null"), which is index 0 of sorted keys."""
    s = enc([s])[0]
    return cat[0].index(s) if s in cat[0] else -1


def value_for_index(cat, idx):
    """get_value(unsigned) :754-763: the row's value; -1 for an index not below the row count, and for a negative one
    (pycategory.cpp:279 casts it to unsigned, which is not below any count)."""
    return cat[1][idx] if 0 <= idx < len(cat[1]) else -1


def indexes_for_key(cat, s):
    """get_indexes_for :885-923 and pycategory.cpp:353-397: the rows whose value is the key's index, ascending; a string that
    is no key raises ValueError (:919-921, pycategory.cpp:371-372), None asks for the null key.  Product's rule for a key
    index not below the row count (PRODUCTS_RULE["indexes_for_key"])."""
    k = value(cat, s)
    if k < 0:
        raise ValueError("nvcategory: string not found in keys")
    return [i for i, v in enumerate(cat[1]) if v == k]


# ops whose result keeps the order the keys came in (so unsorted in, unsorted out); every other result has sorted keys
KEEPS_KEY_ORDER = {"copy", "gather", "gather_and_remap", "merge_category"}


def check(cat, what=""):
    """What every category of the family satisfies: distinct keys, values in [-1, keys)."""
    keys, values = cat
    assert len(set(keys)) == len(keys), what + ": a key twice"
    assert all(-1 <= v < len(keys) for v in values), what + ": a value outside [-1, keys)"


# ---- test data: key pools and op chains, shared by test_strcat_cpu.py (model alone) and test_gpu_strcat.py ------------------
def key_pool(n, seed=0, tag=""):
    """n distinct valid-UTF-8 strings of 0..40 bytes: the empty string, multi-byte ones, some that share a 16-byte prefix."""
    import random

    rnd = random.Random("%s/%d/%d" % (tag, n, seed))
    out, seen = [], set()
    fixed = ["", "é", "ß" * 20, "😀" * 10, "sixteen-byte-pfx", "sixteen-byte-pfxa", "sixteen-byte-pfxb", "sixteen-byte-pfxé", "a", "b"]
    for x in fixed:
        x = tag + x if x else x
        if len(out) < n and x not in seen and len(x.encode("utf8")) <= 40:
            seen.add(x)
            out.append(x)
    alphabet = ["a", "b", "c", "Z", "0", " ", "_", "é", "ü", "😀"]
    while len(out) < n:
        x = tag + ("shared-prefix-16b" if rnd.random() < 0.1 else "") + "".join(rnd.choice(alphabet) for _ in range(rnd.randint(1, 12)))
        if x not in seen and len(x.encode("utf8")) <= 40:
            seen.add(x)
            out.append(x)
    return out


def rows_over(keys, n, rnd, null=False):
    """n rows that use every one of `keys` at least once (n >= len(keys)), shuffled, with a null row or without."""
    rows = list(keys) + [rnd.choice(keys) for _ in range(n - len(keys))] if keys else []
    if null and rows:
        rows += [None, None]
    rnd.shuffle(rows)
    return rows


CHAIN_KS = (40, 300, 2100)
CHAIN_SEEDS = tuple(range(42))  # seed s runs at K = CHAIN_KS[s % 3]
FOLLOWERS = ["add_keys", "remove_keys", "set_keys", "remove_unused_keys", "gather_and_remap", "to_strings", "add_strings", "remove_strings",
             "merge_and_remap", "value"]
HANDOVERS = ([("unsorted", f) for f in FOLLOWERS] + [("neg", f) for f in FOLLOWERS]
             + [("unused", f) for f in ("remove_unused_keys", "gather_and_remap", "merge_category")]
             + [("emptied", f) for f in ("add_keys", "merge_category", "merge_category_right", "add_strings")])
_PRODUCERS = {"unsorted": ("merge_category", "merge_category_right"), "neg": ("remove_keys", "set_keys", "gather"), "unused": ("add_keys",),
              "emptied": ("remove_keys", "set_keys")}


def _holds(prop, cat):
    keys, values = cat
    if prop == "unsorted":
        return not is_sorted(keys)
    if prop == "neg":
        return -1 in values
    if prop == "unused":
        return len({v for v in values if v >= 0}) < len(keys)
    return not keys  # emptied


def from_recipe(recipe):
    """An argument category: ("rows", rows) = from_strings(rows); ("merged", rows_a, rows_b, pos) = the categories of
    rows_a and rows_b merged (unsorted keys), then gather(pos) (repeats, -1)."""
    if recipe[0] == "rows":
        return from_strings(recipe[1])
    return gather(merge_category(from_strings(recipe[1]), from_strings(recipe[2])), recipe[3])


def apply(op, cat, args):
    """The model's answer for one chain step: ("cat", category) | ("strings", rows or None) | ("value", anything)."""
    if op == "merge_category_right":
        return "cat", merge_category(from_recipe(args[0]), cat)
    if op in ("merge_category", "merge_and_remap"):
        return "cat", globals()[op](cat, from_recipe(args[0]))
    if op in ("to_strings", "gather_strings"):
        return "strings", globals()[op](cat, *args)
    if op == "value":  # value and indexes_for_key of one string
        k = value(cat, args[0])
        return "value", (k, indexes_for_key(cat, args[0]) if k >= 0 else None, value_for_index(cat, args[1]))
    return "cat", globals()[op](cat, *args)


def chain(seed, counts=None):
    """One seeded sequence of 6..10 ops over a category of CHAIN_KS[seed % 3] keys.  Yields (op, args, kind, expected) per
    step with the model's state moving along; `expected` is IndexError where the model says the op raises, and the chain
    ends there.  An argument category travels as a recipe (from_recipe).  counts[(property, follower)] += 1 for each
    hand-over of HANDOVERS that occurs; the follower is chosen from them, so a replay needs the same counts."""
    import random

    rnd = random.Random(1000 + seed)
    K = CHAIN_KS[seed % len(CHAIN_KS)]
    pool = key_pool(K, seed, "k")
    spare = key_pool(K // 2 + 3, seed, "n")  # strings that are no key at the start
    cat = from_strings(rows_over(pool, 3 * K + 37, rnd, null=seed % 2 == 0))
    prev = None
    for step in range(rnd.randint(6, 10)):
        keys, values = cat
        props = [p for p in ("emptied", "unsorted", "neg", "unused") if prev in _PRODUCERS[p] and _holds(p, cat)]
        if props and counts is not None and rnd.random() < 0.9:  # the follower this property has met least often
            p = props[0]
            op = min((f for q, f in HANDOVERS if q == p), key=lambda f: (counts.get((p, f), 0), rnd.random()))
        else:
            op = rnd.choice(FOLLOWERS + ["merge_category", "merge_category", "merge_category_right", "gather", "gather", "gather_strings",
                                         "remove_keys", "set_keys", "add_keys"])
        if counts is not None:
            for p in props:
                if (p, op) in counts:
                    counts[(p, op)] += 1
        known = [k.decode("utf8") if k is not None else None for k in keys]
        some = lambda share: [k for k in known if rnd.random() < share]  # noqa: E731
        fresh = lambda n: [rnd.choice(spare + [None]) for _ in range(n)]  # noqa: E731
        if op in ("add_keys", "add_strings", "remove_strings"):
            args = (some(0.3) + fresh(rnd.randint(0, K // 3)),)
        elif op == "remove_keys":
            r = rnd.random()
            args = (list(known),) if r < 0.2 else (some(0.4) + fresh(3),)
        elif op == "set_keys":
            r = rnd.random()
            args = ([],) if r < 0.15 else (some(0.6) + fresh(rnd.randint(0, K // 4)),)
        elif op in ("merge_category", "merge_category_right", "merge_and_remap"):
            r = rnd.random()
            base = [] if r < 0.1 else some(0.5) + fresh(rnd.randint(1, K // 2))
            recipe = ("rows", base * 2)
            if r > 0.7 and base:  # an argument that is itself merged (unsorted keys) and holds a -1
                a, b = base[: len(base) // 2 + 1], base
                nk = len(merge_category(from_strings(a), from_strings(b))[0])
                recipe = ("merged", a, b, [rnd.randrange(-1, nk) for _ in range(len(base) + 5)])
            args = (recipe,)
        elif op in ("gather", "gather_and_remap", "gather_strings"):
            lo = -1 if op == "gather" else 0
            n = rnd.choice([len(keys) // 2 + 1, 2 * len(keys) + 5])
            args = ([rnd.randrange(lo, len(keys)) for _ in range(n)] if keys else ([-1] * 5 if op == "gather" else []),)
            if rnd.random() < 0.012:
                args[0].append(len(keys))  # out of range: both must raise
        elif op == "value":
            args = (rnd.choice(known + [None, "no such key"]), rnd.choice([0, len(values) - 1, -1, len(values)]))
        else:
            args = ()
        try:
            kind, want = apply(op, cat, args)
        except IndexError:
            yield op, args, "raises", IndexError
            return
        yield op, args, kind, want
        if kind == "cat":
            cat = want
            prev = op
        # (a step that returns no category leaves the hand-over open for the next op)


_ALL = None


def all_chains():
    """Every committed chain, materialised once: ({seed: [step, ...]}, hand-over counts, seeds that end in IndexError)."""
    global _ALL
    if _ALL is None:
        counts = {h: 0 for h in HANDOVERS}
        chains = {s: list(chain(s, counts)) for s in CHAIN_SEEDS}
        _ALL = chains, counts, [s for s, steps in chains.items() if steps[-1][2] == "raises"]
    return _ALL
