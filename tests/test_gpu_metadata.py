"""No producer of a string column under-estimates the sizing numbers it caches.

A column carries its longest row (`max_row`) and its largest 64-row span (`max_span64`), exact or as upper bounds, so that
an op in a chain pays no pass over its input.  Two consumers trust them with no check in the kernel: the staged tile walk
(cstile::walk_staged_tiles<Oversize::kHostChecked>, the parse ops and edit_distance) sizes its LDS buffer from the span, and
edit_distance skips its 32767-character guard when the longest row is short.  So for every producer, on its default route and
on its row-wise switch:

  1. each cached number is -1 (not known) or at least the measured one; equal to it where the column's offsets came out
     of cs::Built::scan, whose pass over the lengths measures both; the span alone equal to it where the extents are the
     input's own or a single-pass kernel reports the largest tile it wrote;
  2. stoi and edit_distance of the column are those of the same strings ingested afresh (whose numbers are measured when
     first asked for), and stoi is convert_model's.  Only a column that passed 1 is handed to these kernels.

The input column puts two 3000-byte rows at rows 63 and 64: its widest 64-row window is not the widest of an output whose
rows moved (gather, sublist, split columns, tokens)."""
import ctypes as C
import inspect
import random

import numpy as np
import pytest

import convert_model
import gpuutil
from gpuutil import cached_meta, measured_meta


ROWS = 1500
# exact: the offsets went through Built::scan, both numbers are the measured ones; span: the largest 64-row span is the measured
# one (the input's own where the extents are shared, the largest tile total a single-pass kernel wrote), the longest row a bound
# or unknown; bound: each number a bound computed from the input's, or unknown (-1)
E, S, B = "exact", "span", "bound"


def input_rows(ascii_only):
    rnd = random.Random(20240607 if not ascii_only else 20240608)
    alphabet = list("abcXYZ  _-,.%+019") + ([] if ascii_only else ["é", "ß", "Σ", "😀"])
    out = []
    for r in range(ROWS):
        u = rnd.random()
        if u < 0.03:
            out.append(None)
        elif u < 0.35:  # something for stoi, ip2int and the regex ops to find
            out.append(rnd.choice(["", " ", "-", "+", "x "]) + ".".join(str(rnd.randint(0, 300)) for _ in range(rnd.randint(1, 4))))
        else:
            out.append("".join(rnd.choice(alphabet) for _ in range(rnd.randint(0, 20)))[:20])
    for r in (63, 64):  # five long words (a split makes a handful of columns, not hundreds), a few numbers in each
        words = []
        for _ in range(5):
            w = "".join(rnd.choice("abcXYZ_-,") for _ in range(599))
            for at in (40, 300):
                w = w[:at] + "%d.%d" % (rnd.randint(0, 300), rnd.randint(0, 99)) + w[at:]
            words.append(w)
        out[r] = " ".join(words)[:3000]
        assert len(out[r]) == 3000
    return out


class World:
    """The inputs, made once: nothing below changes them (columns are immutable)."""

    def __init__(self):
        from custrings_amd import nvstrings

        self.rows = input_rows(False)
        self.col = nvstrings.to_device(self.rows)
        self.ascii = nvstrings.to_device(input_rows(True))
        rnd = random.Random(5)
        self.other = nvstrings.to_device(["%d:%s" % (r, "é" * (r % 7)) if r % 11 else None for r in range(ROWS)])
        self.few = nvstrings.to_device(["one", None, "", "thrée" * 40, "4"])
        self.positions = [rnd.randrange(ROWS) for _ in range(1000)] + [64, 63, 64]
        self.mask = [r % 3 != 1 for r in range(ROWS)]
        self.starts = np.array([r % 5 for r in range(ROWS)], dtype=np.int32)
        self.stops = np.array([r % 5 + r % 13 for r in range(ROWS)], dtype=np.int32)
        self.counts = [r % 3 for r in range(ROWS)]
        self.ints = np.array([rnd.randint(-2 ** 31, 2 ** 31 - 1) if r % 4 else r for r in range(ROWS)], dtype=np.int64)
        self.floats = np.array([rnd.uniform(-1e6, 1e6) if r % 4 else r * 0.25 for r in range(ROWS)], dtype=np.float64)
        self.nulls = np.packbits(np.array([r % 9 != 0 for r in range(ROWS)]), bitorder="little")


@pytest.fixture(scope="module")
def world():
    return World()


def _category(w):
    from custrings_amd import nvcategory

    return nvcategory.from_strings(w.col)


def _from_index(w):
    """create_from_index over the input's own device buffers, rows in reverse order (the long rows move to another window)"""
    from custrings_amd import _lib, nvstrings

    _, offs, _ = w.col._export64()
    v = _lib.ColumnView()
    _lib.check(_lib.lib.cs_column_get_view(w.col.m_cptr, C.byref(v)))
    pairs = np.zeros((ROWS, 2), dtype=np.uint64)
    for j, r in enumerate(range(ROWS - 1, -1, -1)):
        if w.rows[r] is not None:
            pairs[j, 0] = v.chars + int(offs[r])
            pairs[j, 1] = int(offs[r + 1] - offs[r])
    out = C.c_void_p()
    _lib.check(_lib.lib.cs_column_from_index(pairs.ctypes.data, ROWS, 0, 0, None, C.byref(out)))
    return nvstrings.nvstrings(out.value)


def _nvs():
    from custrings_amd import nvstrings

    return nvstrings


def _nvt():
    from custrings_amd import nvtext

    return nvtext


IPV4ISH = r"(\d+)\.(\d+)"
CASE, PAD, RECODE, STRIP = {"CS_CASE_ROWWISE": "1"}, {"CS_PAD_ROWWISE": "1"}, {"CS_RECODE_ROWWISE": "1"}, {"CS_STRIP_ROWWISE": "1"}

# (name, what it pins, switches, producer: World -> a column or a list of columns, method names it covers)
PRODUCERS = []


def producer(name, kind, fn, covers=None, switches=(None,), on=("col",)):
    """One entry per switch setting and input column: `fn(column, world)`.  `kind`: one for all of them, or a dict from the
    switch's name (None: the default route) to the kind on that route."""
    for sw in switches:
        for which in on:
            k = kind[next(iter(sw)) if sw else None] if isinstance(kind, dict) else kind
            label = name + ("[" + ",".join(sorted(sw)) + "]" if sw else "") + ("@" + which if which != "col" else "")
            PRODUCERS.append((label, k, sw or {}, which, fn, covers if covers is not None else [name.split("(")[0]]))


for op in ("lower", "upper", "swapcase", "capitalize", "title"):
    # (a column with multi-byte characters takes the two-pass kernels; an ASCII one the tile kernel, whose output shares the
    # input's extents and inherits its numbers)
    # (lower keeps to the tile kernel on the mixed column too: it patches the rows that hold multi-byte characters)
    producer(op, S if op == "lower" else E, lambda c, w, op=op: getattr(c, op)(), on=("col",))
    producer(op, S, lambda c, w, op=op: getattr(c, op)(), on=("ascii",))
    producer(op, E, lambda c, w, op=op: getattr(c, op)(), switches=(CASE,), on=("ascii",))
for op in ("strip", "lstrip", "rstrip"):
    producer(op, E, lambda c, w, op=op: getattr(c, op)(), switches=(None, STRIP), on=("col", "ascii"))
    producer(op + "(chars)", E, lambda c, w, op=op: getattr(c, op)(" .-x0a"), switches=(None, STRIP))
producer("slice", E, lambda c, w: c.slice(2, 12), switches=(None, PAD))
producer("slice(step)", E, lambda c, w: c.slice(1, None, 2), switches=(None, PAD))
producer("get", E, lambda c, w: c.get(3), switches=(None, PAD))
producer("slice_from", E, lambda c, w: c.slice_from(w.starts, w.stops), switches=(None, PAD))
producer("slice_replace", E, lambda c, w: c.slice_replace(2, 5, "héé"), switches=(None, PAD))
producer("insert", E, lambda c, w: c.insert(3, "<é>"), switches=(None, PAD))
producer("pad", E, lambda c, w: c.pad(30, "both", "*"), switches=(None, PAD))
producer("ljust", E, lambda c, w: c.ljust(25), switches=(None, PAD))
producer("center", E, lambda c, w: c.center(25, "é"), switches=(None, PAD))
producer("rjust", E, lambda c, w: c.rjust(25, "-"), switches=(None, PAD))
producer("zfill", E, lambda c, w: c.zfill(12), switches=(None, PAD))
producer("repeat", E, lambda c, w: c.repeat(3), switches=(None, PAD))
producer("wrap", S, lambda c, w: c.wrap(10), switches=(None, PAD))  # (no length changes: the input's extents, shared)
producer("url_encode", E, lambda c, w: c.url_encode(), switches=(None, RECODE))
producer("url_decode", E, lambda c, w: c.url_decode(), switches=(None, RECODE))
producer("url_decode(encoded)", E, lambda c, w: c.url_encode().url_decode(), switches=(None, RECODE))
producer("translate", E, lambda c, w: c.translate({ord("a"): "é", ord("1"): None, ord("é"): "e"}), switches=(None, RECODE))
producer("fillna(str)", E, lambda c, w: c.fillna("missing"), covers=["fillna"])
producer("fillna(column)", E, lambda c, w: c.fillna(w.other), covers=["fillna"])
# (the single-pass literal kernel reports the largest span it wrote and no longest row)
producer("replace(literal)", S, lambda c, w: c.replace("a", "XYZ", regex=False), covers=["replace"], on=("col", "ascii"))
producer("replace(literal)", E, lambda c, w: c.replace("a", "XYZ", regex=False), covers=["replace"], switches=({"CS_REPLACE_ROWWISE": "1"},), on=("col", "ascii"))
# (single-pass replace_re: the span is the largest sub-tile total the kernel wrote; CS_REGEX_ROWWISE does not move it off that
# kernel; the two-pass form sizes, then scans.  replace_with_backrefs tries the single pass first, which hands a column with rows
# this long back to the two-pass form, as CS_BACKREFS_TWO_PASS does outright.)
producer("replace(regex)", {None: S, "CS_REGEX_TWO_PASS": E, "CS_REGEX_ROWWISE": S}, lambda c, w: c.replace(r"\d+", "#"), covers=["replace"], on=("col", "ascii"),
         switches=(None, {"CS_REGEX_TWO_PASS": "1"}, {"CS_REGEX_ROWWISE": "1"}))
producer("replace(regex,growing)", {None: S, "CS_REGEX_TWO_PASS": E}, lambda c, w: c.replace(r"\d+", "<NUMBER>"), covers=["replace"], on=("col", "ascii"),
         switches=(None, {"CS_REGEX_TWO_PASS": "1"}))
producer("replace_with_backrefs", E, lambda c, w: c.replace_with_backrefs(IPV4ISH, r"\2.<\1>"), on=("col", "ascii"),
         switches=(None, {"CS_BACKREFS_TWO_PASS": "1"}, {"CS_REGEX_ROWWISE": "1"}))
producer("replace_multi", E, lambda c, w: c.replace_multi([r"\d+", "a", r"\bX"], ["<N>", "", "é"]))
producer("replace_multi(literals)", E, lambda c, w: c.replace_multi(["a", "."], ["AA", ""], regex=False), covers=["replace_multi"])
for op in ("split", "rsplit"):
    producer(op, B, lambda c, w, op=op: getattr(c, op)(" "),
             switches=(None, {"CS_SPLIT_GENERIC": "1"}, {"CS_SPLIT_OFF64": "1"}, {"CS_RSPLIT_ROWWISE": "1"}))
    producer(op + "(n=3)", B, lambda c, w, op=op: getattr(c, op)(".", 3), covers=[op])
    producer(op + "(whitespace)", B, lambda c, w, op=op: getattr(c, op)(None), covers=[op])
    producer(op + "_record", E, lambda c, w, op=op: getattr(c, op + "_record")(" ", -1, flat=True)[0])
producer("partition", E, lambda c, w: c.partition(" ", flat=True))
producer("rpartition", E, lambda c, w: c.rpartition(".", flat=True))
# (the thread-a-row route of extract and findall scans each column's lengths; the tile route cuts its columns out of one
# segmented scan and hands them bounds)
producer("extract", {None: B, "CS_REGEX_ROWWISE": E, "CS_SPANS_ROWWISE": B}, lambda c, w: c.extract(IPV4ISH), on=("col", "ascii"), switches=(None, {"CS_REGEX_ROWWISE": "1"}, {"CS_SPANS_ROWWISE": "1"}))
producer("findall", {None: B, "CS_REGEX_ROWWISE": E, "CS_SPANS_ROWWISE": B}, lambda c, w: c.findall(r"\d+"), on=("col", "ascii"), switches=(None, {"CS_REGEX_ROWWISE": "1"}, {"CS_SPANS_ROWWISE": "1"}))
producer("extract_record", E, lambda c, w: c.extract_record(IPV4ISH, flat=True)[0])
producer("findall_record", E, lambda c, w: c.findall_record(r"\d+", flat=True)[0])
producer("gather", E, lambda c, w: c.gather(w.positions))
producer("gather(mask)", E, lambda c, w: c.gather(w.mask), covers=["gather"])
# (consecutive rows are a view of the input's buffers: nothing is cached)
producer("sublist(step 1)", B, lambda c, w: c.sublist(1, ROWS, 1), covers=["sublist"])
producer("sublist(step 3)", E, lambda c, w: c.sublist(1, ROWS, 3), covers=["sublist"])
producer("copy", B, lambda c, w: c.copy())
producer("remove_strings", E, lambda c, w: c.remove_strings([0, 5, 62, 1400]))
producer("scatter", E, lambda c, w: c.scatter(w.few, [70, 3, 64, 1499, 0]))
producer("scalar_scatter", E, lambda c, w: c.scalar_scatter("é+" * 50, [1, 63, 640], 3))
producer("add_strings", E, lambda c, w: c.add_strings(w.other))
producer("cat", E, lambda c, w: c.cat(w.other, ":", "_"))
producer("cat(two)", E, lambda c, w: c.cat([w.other, w.ascii], None, None), covers=["cat"])
producer("cat(all rows)", B, lambda c, w: c.cat(None, ",", "?"), covers=["cat"])
producer("join", B, lambda c, w: c.join("-"))
for stype in (1, 2, 3):
    producer("sort(%d)" % stype, E, lambda c, w, stype=stype: c.sort(stype), covers=["sort"])
producer("sort(desc)", E, lambda c, w: c.sort(2, False, False), covers=["sort"])
# (the tile route of tokenize writes its offsets itself and caches nothing; the row-wise one sizes, then scans)
producer("nvtext.tokenize", B, lambda c, w: _nvt().tokenize(c))
producer("nvtext.tokenize", E, lambda c, w: _nvt().tokenize(c), switches=({"CS_TOKENIZE_ROWWISE": "1"},))
producer("nvtext.tokenize(delimiter)", B, lambda c, w: _nvt().tokenize(c, " ."), covers=["nvtext.tokenize"])
producer("nvtext.tokenize(delimiter)", E, lambda c, w: _nvt().tokenize(c, " ."), covers=["nvtext.tokenize"], switches=({"CS_TOKENIZE_ROWWISE": "1"},))
producer("nvtext.tokenize(list)", E, lambda c, w: _nvt().tokenize(c, [" ", "..", "a"]), covers=["nvtext.tokenize"])
producer("nvtext.ngrams", E, lambda c, w: _nvt().ngrams(_nvt().tokenize(c), 2, "_"), switches=(None, {"CS_NGRAM_ROWWISE": "1"}))
producer("nvtext.ngrams(rows)", E, lambda c, w: _nvt().ngrams(c, 3, "é"), covers=["nvtext.ngrams"], switches=(None, {"CS_NGRAM_ROWWISE": "1"}))
producer("nvtext.unique_tokens", E, lambda c, w: _nvt().unique_tokens(c))
producer("nvtext.replace_tokens", E, lambda c, w: _nvt().replace_tokens(c, ["a", "10", "abc"], ["<A>", "", "é"]))
producer("nvtext.normalize_spaces", E, lambda c, w: _nvt().normalize_spaces(c))
producer("nvtext.scatter_count", E, lambda c, w: _nvt().scatter_count(c, w.counts))
producer("nvcategory.keys", E, lambda c, w: _category(w).keys())
producer("nvcategory.to_strings", E, lambda c, w: _category(w).to_strings())
producer("nvcategory.gather_strings", E, lambda c, w: _category(w).gather_strings([k % 40 for k in range(900)]))
for fn, dtype in (("itos", np.int32), ("ltos", np.int64), ("ftos", np.float32), ("dtos", np.float64), ("int2ip", np.uint32)):
    def formatted(c, w, fn=fn, dtype=dtype, nulls=False):
        vals = (w.floats if dtype in (np.float32, np.float64) else w.ints).astype(dtype)
        return getattr(_nvs(), fn)(vals, nulls=w.nulls if nulls else None)
    producer("nvstrings." + fn, E, formatted, switches=(None, {"CS_CONVERT_ROWWISE": "1"}))
    producer("nvstrings." + fn + "(nulls)", E, lambda c, w, f=formatted: f(c, w, nulls=True), covers=["nvstrings." + fn])
producer("nvstrings.from_booleans", E, lambda c, w: _nvs().from_booleans((w.ints % 2).astype(np.uint8), nulls=w.nulls, true="yes", false="never"))
producer("nvstrings.int2timestamp", B, lambda c, w: _nvs().int2timestamp(w.ints), switches=(None, {"CS_CONVERT_ROWWISE": "1"}))
producer("nvstrings.int2timestamp(nulls,format)", B, lambda c, w: _nvs().int2timestamp(w.ints, nulls=w.nulls, format="%d/%m/%y %I:%M %p", units="ms"),
         covers=["nvstrings.int2timestamp"], switches=(None, {"CS_CONVERT_ROWWISE": "1"}))
# (ingest caches nothing: the numbers are measured when an op first asks for them)
producer("nvstrings.to_device", B, lambda c, w: _nvs().to_device(w.rows))
producer("nvstrings.from_strings", B, lambda c, w: _nvs().from_strings(w.few, [c, w.few]))
producer("nvstrings.from_offsets", B, lambda c, w: _from_offsets32(c), covers=["nvstrings.from_offsets"])
producer("nvstrings.from_offsets64", B, lambda c, w: gpuutil.from_col(gpuutil.to_col(c)))
producer("cs_column_from_index", E, lambda c, w: _from_index(w), covers=[])


def _bound(c):
    made = c.upper()
    wrapped = _nvs().bind_cpointer(made.get_cpointer(), own=False)
    wrapped._keep = made
    return wrapped


producer("nvstrings.bind_cpointer", E, lambda c, w: _bound(c))  # (a second handle on a produced column: what that column cached)


def _from_offsets32(c):
    chars, offs, valid = c._export64()
    return _nvs().from_offsets(chars, offs.astype(np.int32), c.size(), np.concatenate([valid, np.zeros(8, dtype=np.uint8)]))


# ---- the assertions -----------------------------------------------------------------------------------------------------
def host_rows(col):
    chars, offs, valid = col._export64()
    rows = len(offs) - 1
    bits = np.unpackbits(valid, bitorder="little")[:rows]
    data, o = chars.tobytes(), offs.tolist()
    return [data[o[i]: o[i + 1]] if bits[i] else None for i in range(rows)]


def reingested(rows):
    lens = np.array([0 if r is None else len(r) for r in rows], dtype=np.int64)
    offs = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(lens)])
    chars = np.frombuffer(b"".join(r for r in rows if r is not None) or b"\0", dtype=np.uint8)
    valid = np.concatenate([np.packbits(np.array([r is not None for r in rows], dtype=np.uint8), bitorder="little"), np.zeros(8, dtype=np.uint8)])
    return _nvs().from_offsets64(chars, offs, len(rows), valid)


def check_column(col, kind, what):
    """Assertion 1 on what the producer cached (read before anything else touches the column), then, only if it held,
    assertion 2: the kHostChecked consumers on this column and on the same strings ingested afresh."""
    span, longest = cached_meta(col)[:2]
    mspan, mlong = measured_meta(col)
    print("%-60s cached (span, row) = (%d, %d) measured (%d, %d)" % (what, span, longest, mspan, mlong))
    assert span == -1 or span >= mspan, "%s: cached max_span64 %d is below the measured %d" % (what, span, mspan)
    assert longest == -1 or longest >= mlong, "%s: cached max_row %d is below the measured %d" % (what, longest, mlong)
    if kind == S:
        assert span == mspan, "%s: cached max_span64 %d, measured %d" % (what, span, mspan)
    if kind == E:
        assert (span, longest) == (mspan, mlong), "%s: through Built::scan, yet (max_span64, max_row) = (%d, %d), measured (%d, %d)" % (
            what, span, longest, mspan, mlong)
    if col.size() == 0:
        return
    rows = host_rows(col)
    fresh = reingested(rows)
    assert all(v in (-1, m) for v, m in zip(cached_meta(fresh)[:2], (mspan, mlong))), what + ": the re-ingested column's own numbers"
    got = col.stoi()
    assert got == fresh.stoi(), what + ": stoi differs from the re-ingested column's"
    assert got == [None if r is None else convert_model.stoi(r) for r in rows], what + ": stoi differs from the model's"
    assert _nvt().edit_distance(col, "10.0.0.1") == _nvt().edit_distance(fresh, "10.0.0.1"), what + ": edit_distance differs from the re-ingested column's"


@pytest.mark.gpu
@pytest.mark.parametrize("label,kind,switches,which,fn,covers", PRODUCERS, ids=[p[0] for p in PRODUCERS])
def test_gpu_producer_does_not_underestimate(world, monkeypatch, label, kind, switches, which, fn, covers):
    for name, value in switches.items():
        monkeypatch.setenv(name, value)
    out = fn(getattr(world, which), world)
    for name in switches:  # (the consumers below run as they do by default)
        monkeypatch.delenv(name)
    cols = out if isinstance(out, list) else [out]
    assert cols and all(c is not None for c in cols), label
    for k, c in enumerate(cols):
        check_column(c, kind, "%s%s" % (label, " column %d" % k if len(cols) > 1 else ""))


def _ipc_child(record, q):
    import os
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    for p in (here, os.path.dirname(here)):
        sys.path.insert(0, p)
    try:
        from custrings_amd import nvstrings, nvtext
        import gpuutil as g

        col = nvstrings.create_from_ipc(record)
        cached, measured = g.cached_meta(col)[:2], g.measured_meta(col)
        if not all(c == -1 or c >= m for c, m in zip(cached, measured)):  # (an under-estimate is reported, not handed to a kernel)
            q.put(("ok", cached, measured, None, None))
            return
        q.put(("ok", cached, measured, col.stoi(), nvtext.edit_distance(col, "10.0.0.1")))
    except Exception as e:  # the parent reports it
        q.put(("error", repr(e)))


@pytest.mark.gpu
def test_gpu_imported_column_does_not_underestimate(world):
    """A column after an IPC export and an import in a second process: what the importer knows of its sizes, and the
    consumers there against this process's."""
    import multiprocessing as mp

    exported = world.col.sublist(1, ROWS, 1)  # (a produced column, its long rows at 62 and 63)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_ipc_child, args=(exported.get_ipc_data(), q))
    p.start()
    got = q.get(timeout=180)
    p.join(timeout=60)
    assert got[0] == "ok", got
    (span, longest), (mspan, mlong) = got[1], got[2]
    assert (mspan, mlong) == measured_meta(exported)
    assert span == -1 or span >= mspan
    assert longest == -1 or longest >= mlong
    rows = host_rows(exported)
    fresh = reingested(rows)
    assert got[3] == fresh.stoi() and got[4] == _nvt().edit_distance(fresh, "10.0.0.1")
    assert got[3] == [None if r is None else convert_model.stoi(r) for r in rows]


# ---- completeness --------------------------------------------------------------------------------------------------------
# What returns no strings column (numbers, booleans, host data, handles), or takes one apart without making one.
NO_STRINGS = {
    "nvstrings": """get_ipc_data get_cpointer to_host to_offsets order len size byte_count set_null_bitmask null_count device_memory
                    find rfind find_from find_multiple compare match_strings startswith endswith contains match count hash stoi stol stof
                    stod htoi ip2int to_booleans isalnum isalpha isdigit isspace isdecimal isnumeric islower isupper is_empty index rindex
                    timestamp2int digest""".split(),
    "nvtext": "token_count tokens_counts contains_strings strings_counts edit_distance porter_stemmer_measure".split(),
    "nvstrings.": ["free"],
}


def test_the_table_leaves_out_no_producer():
    """Every public method of nvstrings, and every public function of the nvstrings and nvtext modules, either makes
    strings and is in the table, or is named above as making none: a new op cannot join the library without joining this
    file."""
    from custrings_amd import nvstrings, nvtext

    covered = {name for p in PRODUCERS for name in p[5]} | {"nvstrings.create_from_ipc"}  # (test_gpu_imported_column_does_not_underestimate)
    methods = {n for n, f in inspect.getmembers(nvstrings.nvstrings, inspect.isfunction) if not n.startswith("_")}
    module = {"nvstrings." + n for n in nvstrings.__all__ if inspect.isfunction(getattr(nvstrings, n))}
    text = {"nvtext." + n for n in nvtext.__all__}
    skipped = set(NO_STRINGS["nvstrings"]) | {"nvstrings." + n for n in NO_STRINGS["nvstrings."]} | {"nvtext." + n for n in NO_STRINGS["nvtext"]}
    everything = methods | module | text
    assert not (skipped - everything), "named as making no strings, but not there: %s" % sorted(skipped - everything)
    assert not (skipped & covered), sorted(skipped & covered)
    missing = everything - covered - skipped
    assert not missing, "string producers that tests/test_gpu_metadata.py does not look at: %s" % sorted(missing)
    assert len(PRODUCERS) == len({p[0] for p in PRODUCERS})
