"""Borrowed (zero-copy) columns for tests/test_gpu_borrowed.py: the rows, the poison, the placement of a column's bytes,
offsets and validity at chosen addresses inside larger poisoned tensors, guarded result buffers, and the op matrix --
per op the call on a device column and the CPU answer from the row list (the models of tests/*_model.py, the oracle for
the regex / find / combine ops).

Everything a test places lies at least GUARD bytes inside one allocation, so a kernel that reads a 16-byte piece too
many -- or a few -- reads poison, never unmapped memory."""
import numpy as np

import chartype_model as ctm
import convert_model as cm
import cpulibs
import datetime_model as dm
import pad_model as pm
import text_model as tm

GUARD = 256
SHIFTS = [0, 1, 7, 13, 15]
# (shift of the chars past a 16-byte boundary, address of the int64 offsets mod 16)
PLACES = [(0, 0), (0, 8), (1, 8), (7, 0), (7, 8), (13, 8), (15, 0), (15, 8)]
# The ASCII poison, one repeating pattern: digits, both letter cases, space, '.', ':', '-' and every delimiter, fill
# character and target of the matrix below ('*' pad fill, '0' zfill, ' ' / ',' delimiters, "e" / "fox" / "12" / "."
# targets, 'T' 'Z' of the timestamps, "True").  It is laid so that the byte in front of a column is the pattern's LAST byte
# and the byte behind a column its FIRST: the neighbours are known.  Which two bytes those are is the pattern's phase, and
# a group of ops takes the phase at which one neighbour alone changes its answers (isupper needs a lower-case letter
# beside an upper-case row, islower the opposite, isalnum neither): ROTATE[group] is the index the pattern starts at.
ASCII_POISON = b"12.5:30-True,*0ae fox\tQy+9E T1Z:7"
ROTATE = {
    "num": 0,                                 # '7' in front, '1' behind
    "int": 0,
    "bool": 0,
    "ts": 0,
    "text": ASCII_POISON.index(b"ae") + 1,    # 'a' in front, 'e' behind
    "lower": ASCII_POISON.rindex(b":"),       # 'Z' in front
    "upper": ASCII_POISON.index(b"fox"),      # 'f' behind
    "alpha": ASCII_POISON.index(b":") + 1,    # ':' in front
    "digit": ASCII_POISON.index(b":") + 1,
    "space": ASCII_POISON.index(b":") + 1,
}
POISONS = ["ff", "ascii"]


def poison_for(name, group):
    if name == "ff":
        return b"\xff"
    r = ROTATE[group]
    return ASCII_POISON[r:] + ASCII_POISON[:r]


TS_FRACTION = b"%Y-%m-%dT%H:%M:%S.%fZ"


def poison_front(poison, k):
    """the k bytes in front of a column"""
    reps = poison * (k // len(poison) + 1)
    return reps[len(reps) - k:]


def poison_behind(poison, k):
    return (poison * (k // len(poison) + 1))[:k]


# ---- rows ------------------------------------------------------------------------------------------------------------
PIECES = ["12", "-7", "3.5e2", "ff", "CAFE", "10.0.0.1", "192.168.1.20", "True", "true", "2019-03-20T12:34:56Z",
          "1969-12-31T23:59:59.250Z", "the fox", "Hello wORLD", "yearly", "abbey", "x:y-z", "a b", " ", "\t", "é", "ñandú", "Ünï",
          "€uro", "日本", "語", "😀", "ß", "Ω", "¼", "٣", "e", ".", ",", "fox"]
# The first and the last row of a column, per group of ops: what the poison in front of the first or behind the last
# one must change (tests/test_gpu_borrowed.py::test_ascii_poison_changes_every_answer holds every op to it).
ENDS = {
    "num": (".5", "10.0.0.1"),
    "int": ("12", "12"),
    "bool": ("True", "True"),
    "ts": ("1969-12-31T23:59:59.250Z", "2019-03-20T12:34:56Z"),
    "alpha": ("fox", "FOX"),
    "lower": ("fox", "fox"),
    "upper": ("FOX", "FOX"),
    "digit": ("12", "٣"),
    "space": (" ", "\t "),
    "text": ("the fox", "wORLD é"),
}
SHAPES = ["one", "sub_tile_plus_one", "ragged_tiles", "row_5000", "row_7000", "no_bytes"]


def body_rows(n, seed):
    rng = np.random.default_rng(seed)
    kinds = rng.integers(0, 12, size=n)
    counts = rng.integers(1, 5, size=n)
    picks = rng.integers(0, len(PIECES), size=(n, 4))
    rows = []
    for k, c, pk in zip(kinds.tolist(), counts.tolist(), picks.tolist()):
        if k == 0:
            rows.append(None)
        elif k == 1:
            rows.append(b"")
        else:
            rows.append("".join(PIECES[p] for p in pk[:c]).encode())
    return rows


def long_row(nbytes, seed):
    rng = np.random.default_rng(seed)
    out = []
    size = 0
    while size < nbytes - 8:
        p = PIECES[int(rng.integers(0, len(PIECES)))] + " "
        out.append(p)
        size += len(p.encode())
    return ("".join(out).encode() + b"x" * nbytes)[:nbytes - 1].decode("utf-8", "ignore").encode()


def make_rows(shape, group):
    """the rows of `shape` (bytes, None = null) with the group's first and last row"""
    first, last = (e.encode() for e in ENDS[group])
    if shape == "one":
        return [first]
    if shape == "no_bytes":
        return [None if i % 3 == 1 else b"" for i in range(130)]
    n = 65 if shape == "sub_tile_plus_one" else 1100
    rows = body_rows(n, 7 + n)
    if shape == "row_5000":
        rows[417] = long_row(5000, 5)
    if shape == "row_7000":
        rows[830] = long_row(7000, 6)
    rows[0], rows[-1] = first, last
    return rows


def arrow(rows):
    """-> chars uint8, offsets int64, validity bytes whose padding bits are SET (Arrow allows them)"""
    chars, offs, nulls = tm.to_arrow(rows)
    bits = (1 - nulls).astype(np.uint8)
    pad = (-len(rows)) % 8
    valid = np.packbits(np.concatenate([bits, np.ones(pad, dtype=np.uint8)]), bitorder="little")
    return chars, offs, valid


# ---- placement -------------------------------------------------------------------------------------------------------
def place(data, at_mod16, poison, device, align=1):
    """`data` (numpy, any dtype) inside a poisoned uint8 tensor, its first byte at an address that is `at_mod16` mod 16,
    GUARD bytes of poison at least on either side -> (backing tensor, view of the data's bytes as uint8, first index)"""
    import torch

    raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    size = 2 * GUARD + 32 + raw.size
    backing = torch.empty(size, dtype=torch.uint8, device=device)
    at = GUARD + (at_mod16 - (backing.data_ptr() + GUARD)) % 16
    assert at % align == 0 or backing.data_ptr() % 16 == 0
    host = np.empty(size, dtype=np.uint8)
    front = poison_front(poison, at)
    behind = poison_behind(poison, size - at - raw.size)
    host[:at] = np.frombuffer(front, dtype=np.uint8)
    host[at:at + raw.size] = raw
    host[at + raw.size:] = np.frombuffer(behind, dtype=np.uint8)
    backing.copy_(torch.from_numpy(host))
    view = backing[at:at + raw.size]
    assert (backing.data_ptr() + at) % 16 == at_mod16 % 16
    assert at >= GUARD and size - at - raw.size >= GUARD
    return backing, view, at


class Borrowed:
    """A column over caller memory: chars at `shift` past a 16-byte boundary, int64 offsets at `offs_mod` mod 16, validity at
    an odd address, poison all around; `.col` is from_offsets64(copy=False), `.copied()` the same bytes through the copying
    ingest with int32 offsets at 4 mod 16."""

    def __init__(self, rows, shift, offs_mod, poison, device="cuda:0"):
        from custrings_amd import nvstrings

        self.rows = rows
        self.poison = poison
        self.device = device
        chars, offs, valid = arrow(rows)
        self.np_chars, self.np_offs, self.np_valid = chars, offs, valid
        self.has_nulls = any(r is None for r in rows)
        self.chars_back, self.chars, self.chars_at = place(chars, shift, poison, device)
        self.offs_back, offs_u8, self.offs_at = place(offs, offs_mod, poison, device, align=8)
        self.offs = offs_u8.view(__import__("torch").int64)
        self.valid_back, self.valid, _ = place(valid, 5, poison, device)
        self.chars_ptr = self.chars_back.data_ptr() + self.chars_at
        assert self.chars_ptr % 16 == shift and self.offs.data_ptr() % 16 == offs_mod and self.valid.data_ptr() % 2 == 1
        # (a column without bytes still hands over its odd chars address)
        self.col = nvstrings.from_offsets64(self.chars_ptr, self.offs, len(rows), self.valid if self.has_nulls else None,
                                            bdevmem=True, copy=False)
        self.col._keep = (self.chars_back, self.offs_back, self.valid_back)

    def copied(self):
        from custrings_amd import nvstrings
        import torch

        self.o32_back, o32, _ = place(self.np_offs.astype(np.int32), 4, self.poison, self.device, align=4)
        g = nvstrings.from_offsets(self.chars_ptr, o32.view(torch.int32), len(self.rows), self.valid if self.has_nulls else None,
                                   bdevmem=True)
        return g

    def caller_memory_intact(self):
        """the library wrote nothing into the caller's tensors"""
        import torch

        for back, data, at in ((self.chars_back, self.np_chars, self.chars_at), (self.offs_back, self.np_offs, self.offs_at)):
            raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            host = back.cpu().numpy()
            want = np.concatenate([np.frombuffer(poison_front(self.poison, at), dtype=np.uint8), raw,
                                   np.frombuffer(poison_behind(self.poison, len(host) - at - raw.size), dtype=np.uint8)])
            if not np.array_equal(host, want):
                return False
        return True


CANARY = 0xA5


class Guarded:
    """A caller's device buffer of n elements of `dtype` at an address aligned to the element size only (odd for one byte,
    4 mod 16 for four, 8 mod 16 for eight) inside a tensor of canary bytes."""

    def __init__(self, dtype, n, device="cuda:0", fill=None):
        import torch

        self.dtype = np.dtype(dtype)
        self.n = n
        nbytes = self.dtype.itemsize * n
        self.back = torch.full((2 * GUARD + 32 + nbytes,), CANARY, dtype=torch.uint8, device=device)
        mod = self.dtype.itemsize if self.dtype.itemsize > 1 else 1
        self.at = GUARD + (mod - (self.back.data_ptr() + GUARD)) % 16
        self.nbytes = nbytes
        self.ptr = self.back.data_ptr() + self.at
        assert self.ptr % 16 == mod
        if fill is not None:
            raw = np.ascontiguousarray(fill, dtype=self.dtype).view(np.uint8).reshape(-1)
            assert raw.size == nbytes
            self.back[self.at:self.at + nbytes] = torch.from_numpy(raw.copy()).to(device)

    def values(self):
        """the region's values; raises when a byte beside it changed"""
        host = self.back.cpu().numpy()
        assert np.all(host[:self.at] == CANARY), "bytes in FRONT of the caller's buffer were written"
        assert np.all(host[self.at + self.nbytes:] == CANARY), "bytes BEHIND the caller's buffer were written"
        return host[self.at:self.at + self.nbytes].copy().view(self.dtype)


# ---- the op matrix -----------------------------------------------------------------------------------------------------
def dec(rows):
    return [None if r is None else r.decode("utf-8") for r in rows]


def col_bytes(g):
    import gpuutil

    return gpuutil.to_col(g).to_bytes_list()


_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        _oracle = cpulibs.Oracle()
    return _oracle


_blobs = {}


def blob(pat):
    import engines

    if pat not in _blobs:
        bl = engines.reference_blob(pat)
        _blobs[pat] = np.ascontiguousarray(bl if bl is not None else engines.product_blob(pat), dtype=np.int32)
    return _blobs[pat]


def ocol(rows):
    return cpulibs.Col.from_list(rows)


def obytes(c):
    return c.to_bytes_list()


class Op:
    def __init__(self, name, group, switch, gpu, cpu):
        self.name, self.group, self.switch, self.gpu, self.cpu = name, group, switch, gpu, cpu


def _dev(dtype, per_row=1):
    """a member with a devptr: its values through a guarded caller buffer"""
    def wrap(call):
        def run(g, ctx):
            buf = Guarded(dtype, max(g.size() * per_row, 1))
            call(g, buf.ptr, ctx)
            return cm.bits(buf.values()[:g.size() * per_row]).tolist()
        return run
    return wrap


CONV, PAD, CASE, TEXT = "CS_CONVERT_ROWWISE", "CS_PAD_ROWWISE", "CS_CASE_ROWWISE", "CS_TEXT_ROWWISE"
IPV4 = r"\d+\.\d+\.\d+\.\d+"
GROUPS_PAT = r"(\d+)\.(\d+)"
TARGETS = {1: ["e"], 3: ["e", "fox", "é"], 5: ["e", "fox", "é", "12", "."]}


def slice_args(n):
    i = np.arange(n)
    return (i % 3).astype(np.int32), (3 + i % 5).astype(np.int32)


def edit_targets(rows):
    """a target per row: the row's first characters, turned round (null and empty targets included)"""
    out = []
    for i, r in enumerate(dec(rows)):
        out.append(None if i % 11 == 4 else "" if r is None else r[:6][::-1])
    return out


def counts_for(n):
    return [(i + 1) % 3 for i in range(n)]


def _parse(op):
    member = {"to_bools": "to_booleans"}.get(op, op)
    gpu = _dev(cm.PARSE_DTYPE[op])(lambda g, p, ctx: getattr(g, member)(devptr=p))
    if op == "to_bools":
        return Op("to_booleans", "bool", CONV, gpu, lambda rows: cm.parse_column(op, rows, true=b"True").tolist())
    return Op(op, "int" if op in ("stoi", "stol") else "num", CONV, gpu, lambda rows: cm.bits(cm.parse_column(op, rows)).tolist())


def _pred(op, group):
    return Op(op, group, CONV, _dev(np.uint8)(lambda g, p, ctx: getattr(g, op)(devptr=p)),
              lambda rows: [int(ctm.predicate(op, r)) for r in dec(rows)])


def _pad(name, member, model_op, args, kwargs=None):
    return Op(name, "text", PAD, lambda g, ctx: col_bytes(getattr(g, member)(*args, **(kwargs or {}))),
              lambda rows: pm.apply_column(model_op, rows, list(args) + list((kwargs or {}).values())))


def _matrix(name, M, dtype):
    from_model = tm.contains_strings if name == "contains_strings" else tm.strings_counts

    def gpu(g, ctx):
        buf = Guarded(dtype, max(g.size() * M, 1))
        getattr(_nvtext(), name)(g, ctx.targets(M), devptr=buf.ptr)
        return buf.values()[:g.size() * M].astype(np.int64).tolist()

    return Op("%s_M%d" % (name, M), "text", TEXT, gpu,
              lambda rows: [int(v) for row in from_model(dec(rows), TARGETS[M]) for v in row])


def _nvtext():
    from custrings_amd import nvtext

    return nvtext


def _text_dev(name, call, cpu):
    return Op(name, "text", TEXT, _dev(np.uint32)(call), cpu)


def build_ops():
    ops = [_parse(op) for op in ("hash", "stoi", "stol", "stof", "stod", "htoi", "ip2int", "to_bools")]
    ops.append(Op("timestamp2int", "ts", CONV, _dev(np.int64)(lambda g, p, ctx: g.timestamp2int(devptr=p)),
                  lambda rows: dm.parse_column(rows).tolist()))
    ops.append(Op("timestamp2int_fraction", "ts", CONV,
                  _dev(np.int64)(lambda g, p, ctx: g.timestamp2int(TS_FRACTION.decode(), units="ms", devptr=p)),
                  lambda rows: dm.parse_column(rows, TS_FRACTION, dm.UNITS["ms"]).tolist()))
    for op, group in (("isalnum", "alpha"), ("isalpha", "alpha"), ("islower", "lower"), ("isupper", "upper"), ("isdigit", "digit"),
                      ("isdecimal", "digit"), ("isnumeric", "digit"), ("isspace", "space"), ("is_empty", "space")):
        ops.append(_pred(op, group))
    ops.append(Op("lower", "text", CASE, lambda g, ctx: col_bytes(g.lower()), lambda rows: obytes(oracle().lower(ocol(rows)))))
    ops.append(Op("upper", "text", CASE, lambda g, ctx: col_bytes(g.upper()), lambda rows: obytes(oracle().upper(ocol(rows)))))
    for op in ctm.CASE_OPS:
        ops.append(Op(op, "text", CASE, (lambda op: lambda g, ctx: col_bytes(getattr(g, op)()))(op),
                      (lambda op: lambda rows: [None if r is None else ctm.case_op(op, r).encode() for r in dec(rows)])(op)))
    ops += [
        _pad("get", "get", "get", (1,)),
        _pad("slice", "slice", "slice", (1, 5)),
        _pad("slice_step", "slice", "slice", (1, 9, 2)),
        _pad("slice_replace", "slice_replace", "slice_replace", (1, 3, "+-")),
        _pad("insert", "insert", "insert", (1, "::")),
        _pad("repeat", "repeat", "repeat", (2,)),
        _pad("pad_left", "pad", "pad", (9, "left", "*")),
        _pad("pad_right", "pad", "pad", (9, "right", "*")),
        _pad("pad_both", "pad", "pad", (9, "both", "é")),
        _pad("zfill", "zfill", "zfill", (8,)),
        _pad("wrap", "wrap", "wrap", (10,)),
    ]
    # slice_replace / insert take (start, stop, repl) / (start, repl) as members, (repl, start, stop) / (repl, start) in the model
    for o in ops:
        if o.name == "slice_replace":
            o.cpu = lambda rows: pm.apply_column("slice_replace", rows, ["+-", 1, 3])
        if o.name == "insert":
            o.cpu = lambda rows: pm.apply_column("insert", rows, ["::", 1])
    ops.append(Op("slice_from", "text", PAD, lambda g, ctx: col_bytes(g.slice_from(*slice_args(g.size()))),
                  lambda rows: pm.apply_column("slice_from", rows, [], *slice_args(len(rows)))))
    for M in (1, 3, 5):
        ops.append(_matrix("contains_strings", M, np.uint8))
        ops.append(_matrix("strings_counts", M, np.uint32))
    ops.append(_text_dev("edit_distance", lambda g, p, ctx: _nvtext().edit_distance(g, "fox", devptr=p),
                         lambda rows: tm.edit_distance(dec(rows), "fox")))
    ops.append(_text_dev("edit_distance_column", lambda g, p, ctx: _nvtext().edit_distance(g, ctx.edit_targets(), devptr=p),
                         lambda rows: tm.edit_distance(dec(rows), edit_targets(rows))))
    ops.append(_text_dev("porter_stemmer_measure", lambda g, p, ctx: _nvtext().porter_stemmer_measure(g, devptr=p),
                         lambda rows: tm.porter_stemmer_measure(dec(rows))))
    ops.append(Op("scatter_count", "text", TEXT, lambda g, ctx: (lambda r: [] if r is None else col_bytes(r))(_nvtext().scatter_count(g, counts_for(g.size()))),
                  lambda rows: tm.scatter_count(rows, counts_for(len(rows)))))
    # the older ops the zero-copy test of test_gpu_parity.py leaves out
    ops.append(Op("rsplit", "text", None, lambda g, ctx: [col_bytes(c) for c in g.rsplit(" ", 3)],
                  lambda rows: [obytes(c) for c in oracle().rsplit(ocol(rows), " ", 3)]))
    ops.append(Op("extract", "num", None, lambda g, ctx: [col_bytes(c) for c in g.extract(GROUPS_PAT)],
                  lambda rows: [obytes(c) for c in oracle().extract(ocol(rows), blob(GROUPS_PAT))]))
    ops.append(Op("findall", "num", None, lambda g, ctx: [col_bytes(c) for c in g.findall(IPV4)],
                  lambda rows: [obytes(c) for c in oracle().findall(ocol(rows), blob(IPV4))]))
    ops.append(Op("count", "num", None, _dev(np.int32)(lambda g, p, ctx: g.count(r"\d+", devptr=p)),
                  lambda rows: oracle().count_re(ocol(rows), blob(r"\d+"))[0].tolist()))
    ops.append(Op("replace_with_backrefs", "num", None, lambda g, ctx: col_bytes(g.replace_with_backrefs(GROUPS_PAT, r"\2.\1")),
                  lambda rows: obytes(oracle().replace_with_backrefs(ocol(rows), blob(GROUPS_PAT), r"\2.\1"))))
    ops.append(Op("rfind", "text", None, _dev(np.int32)(lambda g, p, ctx: g.rfind("o", devptr=p)),
                  lambda rows: oracle().rfind(ocol(rows), "o")[0].tolist()))
    ops.append(Op("len", "text", None, _dev(np.int32)(lambda g, p, ctx: g.len(devptr=p)), lambda rows: oracle().len(ocol(rows))[0].tolist()))
    ops.append(Op("cat", "text", None, lambda g, ctx: col_bytes(g.cat(ctx.others(), sep=",", na_rep="-")),
                  lambda rows: obytes(oracle().cat(ocol(rows), [ocol(rows[::-1])], ",", "-"))))
    return ops


class Expect:
    """CPU answers, computed once per (op, shape) and left unchanged"""

    def __init__(self):
        self.memo = {}

    def __call__(self, op, shape):
        key = (op.name, shape)
        if key not in self.memo:
            self.memo[key] = op.cpu(make_rows(shape, op.group))
        return self.memo[key]
