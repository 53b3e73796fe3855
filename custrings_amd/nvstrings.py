"""`nvstrings` -- host-side mirror of the reference's Python module for the hot path.

Same function / method names, argument defaults and None<->null mapping as
/root/reference/python/nvstrings.py (cited per method), implemented over the
C ABI in include/custrings_amd.h via ctypes.  Every method is one C call on the
MI355X back-end; there is no Python or CPU implementation of any string op
here.  Reference methods outside the hot path raise NotImplementedError.
"""
import ctypes as C
import functools

import numpy as np

from . import _lib
from ._lib import lib, check, b, addr

__all__ = ["to_device", "from_strings", "from_offsets", "free", "bind_cpointer", "create_from_ipc", "nvstrings",
           "itos", "ltos", "ftos", "dtos", "int2ip", "from_booleans", "int2timestamp"]


def to_device(strs):
    """nvstrings.py:4-24 -- list of str/None -> device column (NVStrings::create_from_array)."""
    _lib.ensure_init()
    if isinstance(strs, str) or strs is None:
        strs = [strs]
    strs = list(strs)
    n = len(strs)
    enc = [None if s is None else (s.encode("utf8") if isinstance(s, str) else bytes(s)) for s in strs]
    if any(e is not None and b"\0" in e for e in enc):
        # a NUL inside a string: the C-string ingest would cut it there; the offsets ingest is binary safe
        lens = np.array([0 if e is None else len(e) for e in enc], dtype=np.int64)
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=offs[1:])
        chars = np.frombuffer(b"".join(e for e in enc if e is not None), dtype=np.uint8)
        valid = np.packbits(np.array([e is not None for e in enc], dtype=np.uint8), bitorder="little")
        valid = np.concatenate([valid, np.zeros(8, dtype=np.uint8)])
        return from_offsets64(chars if chars.size else np.zeros(1, dtype=np.uint8), offs, n, valid)
    arr = (C.c_char_p * max(n, 1))(*enc)
    out = C.c_void_p()
    check(lib.cs_column_from_host_strings(arr, n, None, C.byref(out)))
    return nvstrings(out.value)


def from_strings(*args):
    """nvstrings.py:27-56 -- concatenate instances / lists of instances into one (row-wise)."""
    cols = []
    for a in args:
        if isinstance(a, (list, tuple)):
            cols.extend(a)
        else:
            cols.append(a)
    hosts = []
    for c in cols:
        hosts.extend(c.to_host())
    return to_device(hosts)


def from_offsets(sbuf, obuf, scount, nbuf=None, ncount=0, bdevmem=False):
    """nvstrings.py:103-150 -- Arrow chars + int32 offsets (+ bitmask) -> instance
    (NVStrings::create_from_offsets, NVStrings.h:116)."""
    _lib.ensure_init()
    pc, k1 = addr(sbuf)
    po, k2 = addr(obuf)
    pn, k3 = addr(nbuf)
    out = C.c_void_p()
    check(lib.cs_column_from_offsets32(pc, int(scount), po, pn, 1 if bdevmem else 0, None, C.byref(out)))
    del k1, k2, k3
    return nvstrings(out.value)


def from_csv(csv, column, lines=0, flags=0):
    """nvstrings.py:59-100 -- one column (0-based) of a CSV file as an instance (NVStrings::create_from_csv, NVStrings.h:146).
    The first line is the header; `lines` > 0 limits the rows; flags: 1 sort by length, 2 sort by name, 8 an empty field is an
    empty string, not a null.  None when the file cannot be opened or holds fewer than 2 bytes."""
    _lib.ensure_init()
    out = C.c_void_p()
    check(lib.cs_column_from_csv(b(str(csv)), int(column), int(lines), int(flags), None, C.byref(out)))
    return nvstrings(out.value) if out.value else None


def from_csv_buffer(buf, column, lines=0, flags=0, count=0):
    """from_csv over CSV text in memory: a bytes object or numpy uint8 array on the host, or a device tensor / device address
    (an address needs `count`, its bytes); device text is read where it is, not copied."""
    _lib.ensure_init()
    on_device = isinstance(buf, int) or hasattr(buf, "data_ptr")
    if isinstance(buf, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(buf, dtype=np.uint8)
    if isinstance(buf, int):
        n = int(count)
    elif on_device:
        n = int(buf.numel()) * int(buf.element_size())
    else:
        buf = np.ascontiguousarray(buf)
        n = int(buf.nbytes)
    p, keep = addr(buf) if n else (None, None)
    out = C.c_void_p()
    check(lib.cs_column_from_csv_buffer(p, n, 1 if on_device else 0, int(column), int(lines), int(flags), None, C.byref(out)))
    del keep
    return nvstrings(out.value)


STATS_LENGTHS, STATS_CLASSES, STATS_HISTOGRAM, STATS_UNIQUE, STATS_ALL = 1, 2, 4, 8, 15  # include/custrings_amd.h
_STATS_FIELDS = ("total_bytes total_chars bytes_avg bytes_max bytes_min bytes_95 chars_avg chars_max chars_min chars_95 total_memory "
                 "mem_avg mem_max mem_min mem_95 total_strings total_nulls total_empty unique_strings whitespace_count digits_count "
                 "uppercase_count lowercase_count").split()  # struct cs_statistics, in order


def column_statistics(strs, what=STATS_ALL):
    """cs_column_statistics: (the fields of cs_statistics as a dict, the histogram as a list of (packed UTF-8 character,
    count) pairs in code-point order).  `what`: the STATS_* bits; figures outside it are 0."""
    st = (C.c_uint64 * len(_STATS_FIELDS))()
    pairs = np.zeros((0xFFFF, 2), dtype=np.uint32)
    n = C.c_int64()
    check(lib.cs_column_statistics(strs.m_cptr, int(what), st, pairs.ctypes.data, len(pairs), C.byref(n), 0, None))
    return dict(zip(_STATS_FIELDS, (int(v) for v in st))), [(int(a), int(c)) for a, c in pairs[:n.value].tolist()]


def get_info(strs):
    """nvstrings.py:2579-2587 -- the column's statistics as a dict (NVStrings::compute_statistics): row, null, empty and
    distinct counts, byte / character / per-row memory totals, averages, minima (over the non-zero values) and maxima, the
    white-space / digit / upper / lower character counts and `chars_histogram`, one entry per character up to U+FFFF that
    occurs.  One read of the chars and one category build.  `device_memory` is device_memory()."""
    st, pairs = column_statistics(strs)
    info = {"total_strings": st["total_strings"], "null_strings": st["total_nulls"], "empty_strings": st["total_empty"],
            "unique_strings": st["unique_strings"], "total_bytes": st["total_bytes"], "total_chars": st["total_chars"],
            "device_memory": strs.device_memory() if st["total_strings"] else 0,
            "bytes_avg": st["bytes_avg"], "bytes_min": st["bytes_min"], "bytes_max": st["bytes_max"],
            "chars_avg": st["chars_avg"], "chars_min": st["chars_min"], "chars_max": st["chars_max"],
            "memory_avg": st["mem_avg"], "memory_min": st["mem_min"], "memory_max": st["mem_max"],
            "whitespace": st["whitespace_count"], "digits": st["digits_count"], "uppercase": st["uppercase_count"],
            "lowercase": st["lowercase_count"]}
    hist = {}
    for packed, count in pairs:
        try:
            hist[packed.to_bytes(4, "big").lstrip(b"\0").decode("utf-8")] = count
        except UnicodeDecodeError:  # (a lone surrogate has no str: left out, as the CPython glue does)
            pass
    info["chars_histogram"] = hist
    return info


def from_offsets64(chars, offsets, rows, validity=None, bdevmem=False, copy=True):
    """Native ingest (int64 offsets); copy=False wraps caller-owned device buffers."""
    _lib.ensure_init()
    pc, k1 = addr(chars)
    po, k2 = addr(offsets)
    pn, k3 = addr(validity)
    out = C.c_void_p()
    check(lib.cs_column_from_offsets64(pc, int(rows), po, pn, 1 if bdevmem else 0, 1 if copy else 0, None, C.byref(out)))
    r = nvstrings(out.value)
    if not copy:
        r._keep = (k1, k2, k3, chars, offsets)
    return r


IPC_COLUMN_BYTES = 3 * 64 + 3 * 8 + 4 * 4  # sizeof(cs_ipc_column), include/custrings_amd.h


def create_from_ipc(ipc_data):
    """nvstrings.py:348-360 -- an instance over the buffers another process of this node exported with
    get_ipc_data() (NVStrings::create_from_ipc, NVStrings.h:132): mapped through HIP IPC, no copy.  The
    exporting instance must stay alive while this one is in use."""
    _lib.ensure_init()
    rec = C.create_string_buffer(bytes(ipc_data), IPC_COLUMN_BYTES)
    out = C.c_void_p()
    check(lib.cs_column_ipc_import(rec, C.byref(out)))
    return nvstrings(out.value)


def free(dstrs):
    """nvstrings.py:363-367."""
    if dstrs is not None:
        dstrs._destroy()


def bind_cpointer(cptr, own=True):
    """nvstrings.py:370-377 -- wrap an existing cs_column* handle."""
    if cptr == 0 or cptr is None:
        return None
    return nvstrings(cptr, own)


# (inert: all six are methods of the class now, found before __getattr__ is asked; the list keeps its value for the
# assertion in tests/test_chartype_cpu.py and goes with it)
_NOT_BUILT = "fillna index rindex translate url_encode url_decode".split()


# ---- numbers / booleans -> strings (nvstrings.py:153-340; convert.cu) ---------------------------------------------------
def _values(values, count, dtype, bdevmem):
    """values argument of the format functions -> (address, count, keepalive): a list or numpy array on the host, or
    (bdevmem=True) a device address / torch tensor; `count` is needed for a bare address."""
    if isinstance(values, int):
        return values, int(count), None
    if hasattr(values, "data_ptr"):
        return values.data_ptr(), int(count) or values.numel(), values
    if bdevmem:
        raise ValueError("bdevmem=True needs a device address or a device tensor")
    if isinstance(values, (list, tuple)):
        values = [0 if v is None else v for v in values]
    a = np.ascontiguousarray(values, dtype=dtype)
    return a.ctypes.data, int(count) or len(a), a


def _nulls(nulls):
    """the Arrow validity bitmask (bit = 1 valid, LSB first): list of bytes, numpy array, address or tensor."""
    if nulls is None:
        return None, None
    if isinstance(nulls, int):
        return nulls, None
    if hasattr(nulls, "data_ptr"):
        return nulls.data_ptr(), nulls
    a = np.ascontiguousarray(nulls, dtype=np.uint8)
    return a.ctypes.data, a


def _format(fn, values, count, nulls, bdevmem, dtype):
    _lib.ensure_init()
    pv, n, k1 = _values(values, count, dtype, bdevmem)
    pn, k2 = _nulls(nulls)
    out = C.c_void_p()
    check(fn(pv, n, pn, 1 if bdevmem else 0, None, C.byref(out)))
    del k1, k2
    return nvstrings(out.value)


def itos(values, count=0, nulls=None, bdevmem=False):
    """nvstrings.py:153-174 -- strings from int32 values (NVStrings::itos, NVStrings.h:1042)."""
    return _format(lib.cs_itos, values, count, nulls, bdevmem, np.int32)


def ltos(values, count=0, nulls=None, bdevmem=False):
    """nvstrings.py:177-198 -- strings from int64 values (NVStrings::ltos, NVStrings.h:1053)."""
    return _format(lib.cs_ltos, values, count, nulls, bdevmem, np.int64)


def ftos(values, count=0, nulls=None, bdevmem=False):
    """nvstrings.py:201-223 -- strings from float32 values, up to 10 significant digits (NVStrings::ftos, NVStrings.h:1067)."""
    return _format(lib.cs_ftos, values, count, nulls, bdevmem, np.float32)


def dtos(values, count=0, nulls=None, bdevmem=False):
    """nvstrings.py:226-248 -- strings from float64 values, up to 10 significant digits (NVStrings::dtos, NVStrings.h:1081)."""
    return _format(lib.cs_dtos, values, count, nulls, bdevmem, np.float64)


def int2ip(values, count=0, nulls=None, bdevmem=False):
    """nvstrings.py:251-271 -- dotted-quad strings from uint32 values (NVStrings::int2ip, NVStrings.h:1124)."""
    return _format(lib.cs_int2ip, values, count, nulls, bdevmem, np.uint32)


def from_booleans(values, count=0, nulls=None, true="True", false="False", bdevmem=False):
    """nvstrings.py:313-345 -- `true` / `false` per bool value (NVStrings::create_from_bools, NVStrings.h:1105)."""
    if true is None or false is None:
        raise ValueError("nvstrings.from_booleans: true and false must not be None")
    return _format(lambda pv, n, pn, dev, st, out: lib.cs_from_bools(pv, n, b(true), b(false), pn, dev, st, out),
                   values, count, nulls, bdevmem, np.uint8)


# ---- timestamps (nvstrings.py:275-310, 849-879; datetime.cu) -----------------------------------------------------------
_TS_UNITS = {"Y": 0, "M": 1, "D": 2, "h": 3, "m": 4, "s": 5, "ms": 6, "us": 7, "ns": 8}  # NVStrings::timestamp_units


def _ts_units(units):
    if units not in _TS_UNITS:
        raise ValueError("nvstrings: units parameter value unrecognized")
    return _TS_UNITS[units]


def int2timestamp(values, count=0, nulls=None, format=None, units="s", bdevmem=False):
    """
    Create date/time strings from an array of int64 values.
    The values must be in units as specified by the units parameter.
    The values is expected to be from epoch time and in UTC.

    Parameters
    ----------
    values : list, memory address or buffer
        Array of int64 values to convert to date-time strings.
    count : int
        Number of integers in values.
        This is only required if values is a memory pointer.
    nulls : list, memory address or buffer
        Bit array indicating which values should be considered null.
        Uses the arrow format for valid bitmask.
    format : str
        May include the following strftime specifiers only:
        %Y,%y,%m,%d,%H,%I,%p,%M,%S,%f,%z
        Default format is "%Y-%m-%dT%H:%M:%SZ"
    units : str
        The units of the values and must be one of the following:
        Y,M,D,h,m,s,ms,us,ns
        Default is 's' for seconds
    bdevmem : boolean
        Default (False) interprets memory pointers as CPU memory.

    """
    u = _ts_units(units)
    fmt = None if format is None else b(format)
    if isinstance(values, np.ndarray) and (values.dtype.kind not in "iu" or values.dtype.itemsize != 8):
        raise TypeError("nvstrings.int2timestamp(): values must be of type int64")
    return _format(lambda pv, n, pn, dev, st, out: lib.cs_long2timestamp(pv, n, u, fmt, pn, dev, st, out),
                   values, count, nulls, bdevmem, np.int64)


def _int_array(values, count=0):
    """list of ints | numpy array | device address (+ count) -> (address, n, on_device, keepalive)"""
    if isinstance(values, int):
        return values, int(count), 1, None
    if hasattr(values, "data_ptr"):  # torch tensor on the device
        return values.data_ptr(), int(count) or values.numel(), 1, values
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a.ctypes.data, len(a), 0, a


def _escape_literal(text):
    """A literal as a pattern of the reference's regex dialect (regcomp.cpp:314-539): metacharacters quoted."""
    return "".join("\\" + ch if ch in "\\^$.|?*+()[]{}" else ch for ch in text)


class nvstrings:
    """Immutable device strings column (reference class: nvstrings.py:380-402).

    Holds a `cs_column*`; every transforming method returns a new instance.
    """

    def __init__(self, cptr, own=True):
        self.m_cptr = cptr
        self._own = own
        self._keep = None

    _cs_abi = True  # m_cptr is a cs_column* (the pyni glue wraps it on demand, see host/pyni_common.h)
    _nv_cptr = None

    def get_ipc_data(self):
        """nvstrings.py:447-462 -- the record another process hands to create_from_ipc (NVStrings::create_ipc_transfer,
        NVStrings.h:214): the HIP IPC handles of this column's buffers, as bytes."""
        rec = C.create_string_buffer(IPC_COLUMN_BYTES)
        check(lib.cs_column_ipc_export(self.m_cptr, rec))
        return rec.raw

    def _destroy(self):
        if self._nv_cptr:  # the C++ instance the glue wrapped around this handle
            import pyniNVStrings

            pyniNVStrings.n_dropWrapper(self._nv_cptr)
            self._nv_cptr = None
        if getattr(self, "m_cptr", None) and self._own:
            lib.cs_column_destroy(self.m_cptr)
        self.m_cptr = 0

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def __getattr__(self, name):
        # get_info is handed out here, bound to the instance, and is no plain method of the class: it makes no strings, and
        # tests/test_gpu_metadata.py lists every plain-function member of the class against its table of string producers.
        # A change that may add "get_info" to that file's NO_STRINGS table can turn this into an ordinary method.
        if name == "get_info":
            return functools.partial(get_info, self)
        if name in _NOT_BUILT:
            raise NotImplementedError("nvstrings.%s is outside the accelerated hot path (SURVEY.md section 8)" % name)
        raise AttributeError(name)

    def __str__(self):
        return str(self.to_host())

    def __repr__(self):
        return "<nvstrings count={}>".format(self.size())

    def __len__(self):
        return self.size()

    def __iter__(self):
        raise TypeError("iterable not supported by nvstrings")

    def get_cpointer(self):
        return self.m_cptr

    # ---- egress -------------------------------------------------------------
    def _export64(self):
        rows = self.size()
        nbytes = lib.cs_column_nbytes(self.m_cptr)
        chars = np.empty(max(nbytes, 1), dtype=np.uint8)
        offs = np.zeros(rows + 1, dtype=np.int64)
        valid = np.zeros((rows + 7) // 8 + 1, dtype=np.uint8)
        if rows:
            check(lib.cs_column_export_offsets64(self.m_cptr, chars.ctypes.data, offs.ctypes.data, valid.ctypes.data, 0, None))
        return chars[:nbytes], offs, valid[: (rows + 7) // 8]

    def to_host(self):
        """nvstrings.py:464-482 -- list of str, None for null rows."""
        chars, offs, valid = self._export64()
        rows = len(offs) - 1
        bits = np.unpackbits(valid, bitorder="little")[:rows] if rows else np.zeros(0, dtype=np.uint8)
        data = chars.tobytes()
        o = offs.tolist()
        return [data[o[i] : o[i + 1]].decode("utf8", "surrogateescape") if bits[i] else None for i in range(rows)]

    def to_offsets(self, sbuf, obuf, nbuf=0, bdevmem=False):
        """nvstrings.py:484-517 -- NVStrings::create_offsets (int32 offsets, LSB-first bitmask)."""
        pc, k1 = addr(sbuf)
        po, k2 = addr(obuf)
        pn, k3 = addr(nbuf)
        check(lib.cs_column_export_offsets32(self.m_cptr, pc, po, pn, 1 if bdevmem else 0, None))
        del k1, k2, k3

    def sublist(self, start, end=0, step=0):
        """NVStrings::sublist(start, end, step) (NVStrings.h:261; array.cu:238-260): rows start, start+step, ...
        before `end`.  A list as the first argument is the Python module's form (nvstrings.py:2390): gather."""
        if not isinstance(start, int):
            return self.gather(start, end)
        out = C.c_void_p()
        check(lib.cs_sublist(self.m_cptr, int(start), int(end), int(step), None, C.byref(out)))
        return nvstrings(out.value)

    # ---- re-arrangement (nvstrings.py:2326-2540; array.cu) --------------------------------------------
    def gather(self, indexes, count=0):
        """nvstrings.py:2394-2418 -- rows at the given positions (ints) or where the mask is true (bools)."""
        out = C.c_void_p()
        if not isinstance(indexes, int) and not hasattr(indexes, "data_ptr") and len(indexes) and isinstance(indexes[0], (bool, np.bool_)):
            m = np.ascontiguousarray(indexes, dtype=np.uint8)
            if len(m) != self.size():
                raise ValueError("gather: the mask must have one entry per string")
            check(lib.cs_gather_mask(self.m_cptr, m.ctypes.data, 0, None, C.byref(out)))
            return nvstrings(out.value)
        p, n, dev, keep = _int_array(indexes, count)
        st = lib.cs_gather(self.m_cptr, p, n, dev, None, C.byref(out))
        if st == _lib.CS_ERR_RANGE:
            raise IndexError(_lib.last_error())  # std::out_of_range in the reference
        check(st)
        del keep
        return nvstrings(out.value)

    def scatter(self, strs, indexes):
        """nvstrings.py:2420-2448 -- a copy with row indexes[j] replaced by row j of strs."""
        p, n, dev, keep = _int_array(indexes, strs.size())
        if n != strs.size():
            raise ValueError("scatter: one index per string of strs")
        out = C.c_void_p()
        check(lib.cs_scatter(self.m_cptr, strs.m_cptr, p, dev, None, C.byref(out)))
        del keep
        return nvstrings(out.value)

    def scalar_scatter(self, str, indexes, count):
        """nvstrings.py:2450-2478 -- a copy with the given rows replaced by one string."""
        p, n, dev, keep = _int_array(indexes, count)
        out = C.c_void_p()
        check(lib.cs_scatter_scalar(self.m_cptr, b(str), p, n if not dev else int(count), dev, None, C.byref(out)))
        del keep
        return nvstrings(out.value)

    def remove_strings(self, indexes, count=0):
        """nvstrings.py:2480-2505 -- the rows NOT named by indexes (array.cu:262-300)."""
        p, n, dev, keep = _int_array(indexes, count)
        if dev:
            raise NotImplementedError("remove_strings with a device pointer")
        mask = np.ones(self.size(), dtype=np.uint8)
        idx = np.asarray(keep, dtype=np.int64)
        mask[idx[(idx >= 0) & (idx < self.size())]] = 0
        out = C.c_void_p()
        check(lib.cs_gather_mask(self.m_cptr, mask.ctypes.data, 0, None, C.byref(out)))
        return nvstrings(out.value)

    def add_strings(self, strs):
        """nvstrings.py:2507-2530 -- these rows followed by those of strs."""
        arr = (C.c_void_p * 2)(self.m_cptr, strs.m_cptr)
        out = C.c_void_p()
        check(lib.cs_column_concat(arr, 2, None, C.byref(out)))
        return nvstrings(out.value)

    def copy(self):
        """nvstrings.py:2532-2540."""
        return self.sublist(0, self.size(), 1) if self.size() else to_device([])

    def sort(self, stype=2, asc=True, nullfirst=True):
        """nvstrings.py:2326-2355 -- by name (2), byte length (1) or both (3)."""
        out = C.c_void_p()
        check(lib.cs_sort(self.m_cptr, int(stype), 1 if asc else 0, 1 if nullfirst else 0, None, C.byref(out)))
        return nvstrings(out.value)

    def order(self, stype=2, asc=True, nullfirst=True, devptr=0):
        """nvstrings.py:2357-2388 -- the row indexes in sorted order."""
        rows = self.size()
        if devptr:
            check(lib.cs_order(self.m_cptr, int(stype), 1 if asc else 0, 1 if nullfirst else 0, devptr, 1, None))
            return devptr
        res = np.zeros(max(rows, 1), dtype=np.uint32)
        check(lib.cs_order(self.m_cptr, int(stype), 1 if asc else 0, 1 if nullfirst else 0, res.ctypes.data, 0, None))
        return [int(v) for v in res[:rows]]

    def len(self, devptr=0):
        """nvstrings.py:538-565 -- characters per row; None for null rows in the host list."""
        rows = self.size()
        total = C.c_int64()
        if devptr:
            check(lib.cs_len(self.m_cptr, devptr, 1, None, C.byref(total)))
            return devptr
        res = np.zeros(max(rows, 1), dtype=np.int32)
        check(lib.cs_len(self.m_cptr, res.ctypes.data, 0, None, C.byref(total)))
        return [None if v < 0 else int(v) for v in res[:rows]]

    # ---- combine (nvstrings.py:881-934; combine.cu) ---------------------------------------------------
    def cat(self, others=None, sep=None, na_rep=None):
        """nvstrings.py:881-911 -- row-wise concatenation with one or several other instances; without `others`
        all rows are joined into one string (pystrings.cpp n_cat: join(sep or "", na_rep))."""
        out = C.c_void_p()
        if others is None:
            check(lib.cs_join(self.m_cptr, b(sep if sep is not None else ""), b(na_rep), None, C.byref(out)))
            return nvstrings(out.value)
        if not isinstance(others, (list, tuple)):
            others = [others]
        arr = (C.c_void_p * max(len(others), 1))(*[o.m_cptr for o in others])
        check(lib.cs_cat(self.m_cptr, arr, len(others), b(sep), b(na_rep), None, C.byref(out)))
        return nvstrings(out.value)

    def join(self, sep=""):
        """nvstrings.py:913-934 -- all rows joined into a single string (null rows contribute nothing)."""
        out = C.c_void_p()
        check(lib.cs_join(self.m_cptr, b(sep), None, None, C.byref(out)))
        return nvstrings(out.value)

    def _export_window(self, first, rows):
        return self.sublist(first, first + rows)._export64()

    def size(self):
        """nvstrings.py:519-536."""
        return int(lib.cs_column_rows(self.m_cptr))

    def byte_count(self, vals=0, bdevmem=False):
        """nvstrings.py:567-596 -- per-row byte length (-1 null); returns the total."""
        pv, k = addr(vals)
        total = C.c_int64()
        check(lib.cs_column_byte_count(self.m_cptr, pv, 1 if bdevmem else 0, None, C.byref(total)))
        del k
        return total.value

    def set_null_bitmask(self, nbuf, bdevmem=False):
        """nvstrings.py:598-620 -- returns the number of nulls."""
        pn, k = addr(nbuf)
        cnt = C.c_int64()
        check(lib.cs_column_null_bitarray(self.m_cptr, pn, 0, 1 if bdevmem else 0, None, C.byref(cnt)))
        del k
        return cnt.value

    def null_count(self, emptyisnull=False):
        """nvstrings.py:622-645."""
        rows = self.size()
        tmp = np.zeros((rows + 7) // 8 + 1, dtype=np.uint8)
        cnt = C.c_int64()
        if rows == 0:
            return 0
        check(lib.cs_column_null_bitarray(self.m_cptr, tmp.ctypes.data, 1 if emptyisnull else 0, 0, None, C.byref(cnt)))
        return cnt.value

    def _null_flags(self):
        rows = self.size()
        tmp = np.zeros((rows + 7) // 8 + 1, dtype=np.uint8)
        cnt = C.c_int64()
        if rows:
            check(lib.cs_column_null_bitarray(self.m_cptr, tmp.ctypes.data, 0, 0, None, C.byref(cnt)))
        return np.unpackbits(tmp, bitorder="little")[:rows] == 0

    def device_memory(self):
        """nvstrings.py:2628 -- bytes of device memory held by this column."""
        rows = self.size()
        return int(lib.cs_column_nbytes(self.m_cptr)) + 8 * (rows + 1) + (rows + 7) // 8

    # ---- split ----------------------------------------------------------------
    def split(self, delimiter=None, n=-1):
        """nvstrings.py:1069-1097 -- column-major split; list of nvstrings."""
        arr = C.POINTER(C.c_void_p)()
        ncols = C.c_int()
        check(lib.cs_split(self.m_cptr, b(delimiter), int(n), None, C.byref(arr), C.byref(ncols)))
        out = [nvstrings(arr[i]) for i in range(ncols.value)]
        lib.cs_free(arr)
        return out

    def rsplit(self, delimiter=None, n=-1):
        """nvstrings.py:1099-1127 -- column-major split with the tokens located from the right."""
        arr = C.POINTER(C.c_void_p)()
        ncols = C.c_int()
        check(lib.cs_rsplit(self.m_cptr, b(delimiter), int(n), None, C.byref(arr), C.byref(ncols)))
        out = [nvstrings(arr[i]) for i in range(ncols.value)]
        lib.cs_free(arr)
        return out

    def _record_call(self, fn, delimiter, n, flat):
        rows = self.size()
        loff = np.zeros(rows + 1, dtype=np.int64)
        out = C.c_void_p()
        check(fn(self.m_cptr, b(delimiter), int(n), loff.ctypes.data, 0, None, C.byref(out)))
        f = nvstrings(out.value)
        if flat:
            return f, loff
        nulls = self._null_flags() if rows else []
        return [None if nulls[r] else f.sublist(int(loff[r]), int(loff[r + 1]), 1) for r in range(rows)]

    def split_record(self, delimiter=None, n=-1, flat=False):
        """nvstrings.py:936-967 -- one nvstrings per row holding that row's tokens (None for a null row).
        flat=True returns the native form: (all tokens in row-major order, rows+1 list offsets)."""
        return self._record_call(lib.cs_split_record, delimiter, n, flat)

    def rsplit_record(self, delimiter=None, n=-1, flat=False):
        """nvstrings.py:969-1001 -- split_record with the tokens located from the right."""
        return self._record_call(lib.cs_rsplit_record, delimiter, n, flat)

    def _partition(self, delimiter, from_right, flat):
        out = C.c_void_p()
        check(lib.cs_partition(self.m_cptr, b(delimiter), from_right, None, C.byref(out)))
        if not out.value:
            return []
        f = nvstrings(out.value)
        if flat:
            return f
        return [f.sublist(3 * r, 3 * r + 3, 1) for r in range(self.size())]

    def partition(self, delimiter=" ", flat=False):
        """nvstrings.py:1003-1034 -- per row (head, delimiter, tail) around the first occurrence."""
        return self._partition(delimiter, 0, flat)

    def rpartition(self, delimiter=" ", flat=False):
        """nvstrings.py:1036-1067 -- per row (head, delimiter, tail) around the last occurrence."""
        return self._partition(delimiter, 1, flat)

    # ---- replace ----------------------------------------------------------------
    def replace_multi(self, pats, repls, regex=True):
        """nvstrings.py:1487-1530 -- several patterns (list of str; regex) or literals (list / nvstrings) at once:
        at each position the first that matches is replaced by its replacement (or the single one)."""
        if regex:
            if not isinstance(pats, list):
                raise ValueError("pats must be list of str")
            pats = list(pats)
        else:
            pats = [None if p is None else _escape_literal(p) for p in (pats.to_host() if isinstance(pats, nvstrings) else pats)]
        if isinstance(repls, str):
            repls = to_device([repls])
        if isinstance(repls, list):
            repls = to_device(repls)
        res = [_compile(p) if p is not None else None for p in pats]
        arr = (C.c_void_p * max(len(res), 1))(*[r for r in res])
        out = C.c_void_p()
        try:
            check(lib.cs_replace_re_multi(self.m_cptr, arr, len(res), repls.m_cptr, None, C.byref(out)))
        finally:
            for r in res:
                if r is not None:
                    lib.cs_regex_destroy(r)
        return nvstrings(out.value)

    def replace(self, pat, repl, n=-1, regex=True):
        """nvstrings.py:1460-1485 -- replace_re when regex (default) else literal replace."""
        out = C.c_void_p()
        if regex:
            re = _compile(pat)
            try:
                check(lib.cs_replace_re(self.m_cptr, re, b(repl), int(n), None, C.byref(out)))
            finally:
                lib.cs_regex_destroy(re)
        else:
            check(lib.cs_replace(self.m_cptr, b(pat), b(repl), int(n), None, C.byref(out)))
        return nvstrings(out.value)

    def replace_with_backrefs(self, pat, repl):
        """nvstrings.py:1532-1557 -- regex replace with \\N in repl standing for capture group N of the match."""
        if not pat:
            raise ValueError("nvstrings::replace_with_backrefs parameter cannot be null or empty")
        re = _compile(pat)
        out = C.c_void_p()
        try:
            check(lib.cs_replace_with_backrefs(self.m_cptr, re, b(repl), None, C.byref(out)))
        finally:
            lib.cs_regex_destroy(re)
        return nvstrings(out.value)

    # ---- extract ------------------------------------------------------------------
    def extract(self, pat):
        """nvstrings.py:2127-2157 -- one nvstrings per capture group (column-major)."""
        re = _compile(pat)
        arr = C.POINTER(C.c_void_p)()
        ncols = C.c_int()
        try:
            check(lib.cs_extract(self.m_cptr, re, None, C.byref(arr), C.byref(ncols)))
        finally:
            lib.cs_regex_destroy(re)
        out = [nvstrings(arr[i]) for i in range(ncols.value)]
        if ncols.value:
            lib.cs_free(arr)
        return out

    def findall(self, pat):
        """nvstrings.py:1921-1948 -- column k holds every row's k-th match (column-major)."""
        re = _compile(pat)
        arr = C.POINTER(C.c_void_p)()
        ncols = C.c_int()
        try:
            check(lib.cs_findall(self.m_cptr, re, None, C.byref(arr), C.byref(ncols)))
        finally:
            lib.cs_regex_destroy(re)
        out = [nvstrings(arr[i]) for i in range(ncols.value)]
        if ncols.value:
            lib.cs_free(arr)
        return out

    # ---- record (row-major) forms ---------------------------------------------------
    @staticmethod
    def _records(cols, ragged):
        """Column-major result -> (flat nvstrings in row-major order, list offsets as a host numpy int64 array):
        the native record form (cs_records_from_columns)."""
        import numpy as np

        rows = cols[0].size() if cols else 0
        arr = (C.c_void_p * max(len(cols), 1))(*[c.m_cptr for c in cols])
        loff = np.zeros(rows + 1, dtype=np.int64)
        out = C.c_void_p()
        check(lib.cs_records_from_columns(arr, len(cols), int(ragged), loff.ctypes.data, 0, None, C.byref(out)))
        return nvstrings(out.value), loff

    @staticmethod
    def _rows_of(flat, loff):
        return [flat.sublist(int(loff[r]), int(loff[r + 1])) for r in range(len(loff) - 1)]

    def extract_record(self, pat, flat=False):
        """nvstrings.py:2097-2125 -- per row the capture groups of its first match (null where there is none).
        flat=True returns the native form instead: (one nvstrings in row-major order, list offsets)."""
        cols = self.extract(pat)
        if not cols:
            return []
        f, loff = self._records(cols, False)
        return (f, loff) if flat else self._rows_of(f, loff)

    def findall_record(self, pat, flat=False):
        """nvstrings.py:1891-1919 -- per row all its matches (an empty instance where there is none)."""
        f, loff = self._records(self.findall(pat), True)
        return (f, loff) if flat else self._rows_of(f, loff)

    # ---- strip --------------------------------------------------------------------
    def _strip(self, to_strip, side):
        out = C.c_void_p()
        check(lib.cs_strip(self.m_cptr, b(to_strip), side, None, C.byref(out)))
        return nvstrings(out.value)

    def lstrip(self, to_strip=None):
        """nvstrings.py:1583-1603."""
        return self._strip(to_strip, 1)

    def strip(self, to_strip=None):
        """nvstrings.py:1605-1625."""
        return self._strip(to_strip, 0)

    def rstrip(self, to_strip=None):
        """nvstrings.py:1627-1647."""
        return self._strip(to_strip, 2)

    # ---- case -----------------------------------------------------------------------
    def lower(self):
        """nvstrings.py:1649-1665."""
        out = C.c_void_p()
        check(lib.cs_lower(self.m_cptr, None, C.byref(out)))
        return nvstrings(out.value)

    def upper(self):
        """nvstrings.py:1667-1683."""
        out = C.c_void_p()
        check(lib.cs_upper(self.m_cptr, None, C.byref(out)))
        return nvstrings(out.value)

    # ---- find / contains ----------------------------------------------------------------
    def find(self, sub, start=0, end=None, devptr=0):
        """nvstrings.py:1796-1823 -- char position, -1 miss; host list has None for null rows
        (pystrings.cpp n_find: values < -1 become None)."""
        rows = self.size()
        end = -1 if end is None else int(end)
        found = C.c_int64()
        if devptr:
            check(lib.cs_find(self.m_cptr, b(sub), int(start), end, devptr, 1, None, C.byref(found)))
            return devptr
        res = np.zeros(max(rows, 1), dtype=np.int32)
        check(lib.cs_find(self.m_cptr, b(sub), int(start), end, res.ctypes.data, 0, None, C.byref(found)))
        return [None if v < -1 else int(v) for v in res[:rows]]

    # ---- the rest of the find family (nvstrings.py:647, 1825-1890, 2005-2095, 2550; find.cu) -----------------------
    def _positions(self, call, devptr, n=None):
        rows = self.size() if n is None else n
        found = C.c_int64()
        if devptr:
            check(call(devptr, 1, C.byref(found)))
            return devptr
        res = np.zeros(max(rows, 1), dtype=np.int32)
        check(call(res.ctypes.data, 0, C.byref(found)))
        return res[:rows]

    def rfind(self, sub, start=0, end=None, devptr=0):
        """nvstrings.py:1861-1890 -- the LAST occurrence inside characters [start, end); None for null rows."""
        end = -1 if end is None else int(end)
        res = self._positions(lambda out, dev, f: lib.cs_rfind(self.m_cptr, b(sub), int(start), end, out, dev, None, f), devptr)
        return res if devptr else [None if v < -1 else int(v) for v in res]

    def find_from(self, sub, starts=0, ends=0, devptr=0):
        """nvstrings.py:1825-1859 -- `starts` / `ends`: device pointers to one int32 per row (0 = from the start / to the end)."""
        res = self._positions(lambda out, dev, f: lib.cs_find_from(self.m_cptr, b(sub), starts or None, ends or None, 1, out, dev, None, f), devptr)
        return res if devptr else [None if v < -1 else int(v) for v in res]

    def find_multiple(self, strs, devptr=0):
        """nvstrings.py:2550-2580 -- a row of positions per string, one per target."""
        if strs is None:
            raise ValueError("nvstrings.find_multiple: parameter required")
        targets = strs if isinstance(strs, nvstrings) else to_device(list(strs))
        tc = targets.size()
        if tc == 0:
            raise ValueError("nvstrings.find_multiple empty argument list")
        rows = self.size()
        res = self._positions(lambda out, dev, f: lib.cs_find_multiple(self.m_cptr, targets.m_cptr, out, dev, None, f), devptr, rows * tc)
        if devptr:
            return res
        return [[None if v < -1 else int(v) for v in res[r * tc:(r + 1) * tc]] for r in range(rows)]

    def compare(self, str, devptr=0):
        """nvstrings.py:647-672 -- bytewise difference to `str` (0 = equal); None for null rows in the host list."""
        rows = self.size()
        res = self._positions(lambda out, dev, f: lib.cs_compare(self.m_cptr, b(str), out, dev, None, f), devptr)
        if devptr:
            return res
        nulls = self._null_flags()
        return [None if nulls[i] else int(res[i]) for i in range(rows)]

    def match_strings(self, strs, devptr=0):
        """nvstrings.py:2005-2047 -- row-wise equality with another instance (or list) of the same size."""
        if strs is None:
            raise ValueError("nvstrings.match_strings: parameter required")
        other = strs if isinstance(strs, nvstrings) else to_device(list(strs))
        if other.size() != self.size():
            raise ValueError("nvstrings.match_strings list size must match")
        rows = self.size()
        found = C.c_int64()
        if devptr:
            check(lib.cs_match_strings(self.m_cptr, other.m_cptr, devptr, 1, None, C.byref(found)))
            return devptr
        if rows == 0:
            return []
        res = np.zeros(rows, dtype=np.uint8)
        check(lib.cs_match_strings(self.m_cptr, other.m_cptr, res.ctypes.data, 0, None, C.byref(found)))
        return [bool(v) for v in res]

    def startswith(self, pat, devptr=0):
        """nvstrings.py:2049-2071; null rows -> None in the host list."""
        return self._bools(lambda out, dev, f: lib.cs_startswith(self.m_cptr, b(pat), out, dev, None, f), devptr)

    def endswith(self, pat, devptr=0):
        """nvstrings.py:2073-2095."""
        return self._bools(lambda out, dev, f: lib.cs_endswith(self.m_cptr, b(pat), out, dev, None, f), devptr)

    def _bools(self, call, devptr):
        rows = self.size()
        found = C.c_int64()
        if devptr:
            check(call(devptr, 1, C.byref(found)))
            return devptr
        if rows == 0:
            return []
        res = np.zeros(rows, dtype=np.uint8)
        check(call(res.ctypes.data, 0, C.byref(found)))
        nulls = self._null_flags()
        return [None if nulls[i] else bool(res[i]) for i in range(rows)]

    def contains(self, pat, regex=True, devptr=0):
        """nvstrings.py:1951-1978; null rows -> None in the host list (pystrings.cpp:2654-2662)."""
        if regex:
            re = _compile(pat)
            try:
                return self._bools(lambda p, d, f: lib.cs_contains_re(self.m_cptr, re, p, d, None, f), devptr)
            finally:
                lib.cs_regex_destroy(re)
        return self._bools(lambda p, d, f: lib.cs_contains(self.m_cptr, b(pat), p, d, None, f), devptr)

    def match(self, pat, devptr=0):
        """nvstrings.py:1980-2003."""
        re = _compile(pat)
        try:
            return self._bools(lambda p, d, f: lib.cs_match_re(self.m_cptr, re, p, d, None, f), devptr)
        finally:
            lib.cs_regex_destroy(re)

    def count(self, pat, devptr=0):
        """nvstrings.py:2033-2047 -- occurrences of the pattern per row."""
        rows = self.size()
        found = C.c_int64()
        re = _compile(pat)
        try:
            if devptr:
                check(lib.cs_count_re(self.m_cptr, re, devptr, 1, None, C.byref(found)))
                return devptr
            if rows == 0:
                return []
            res = np.zeros(rows, dtype=np.int32)
            check(lib.cs_count_re(self.m_cptr, re, res.ctypes.data, 0, None, C.byref(found)))
        finally:
            lib.cs_regex_destroy(re)
        nulls = self._null_flags()
        return [None if nulls[i] else int(res[i]) for i in range(rows)]

    # ---- strings -> numbers / booleans (nvstrings.py:675-850; convert.cu) -----------------------------------------------
    def _convert(self, fn, dtype, devptr, to_py):
        """one value per row: to `devptr` (device address or tensor) when given, else a host list, None for null rows."""
        rows = self.size()
        cnt = C.c_int64()
        if devptr:
            p = devptr.data_ptr() if hasattr(devptr, "data_ptr") else int(devptr)
            check(fn(p, 1, C.byref(cnt)))
            return devptr
        if rows == 0:
            return []
        res = np.zeros(rows, dtype=dtype)
        check(fn(res.ctypes.data, 0, C.byref(cnt)))
        nulls = self._null_flags()
        return [None if nulls[i] else to_py(v) for i, v in enumerate(res.tolist())]

    def hash(self, devptr=0):
        """nvstrings.py:675-694 -- MurmurHash3 (seed 31) of every row as uint32 (NVStrings::hash)."""
        return self._convert(lambda p, d, f: lib.cs_hash(self.m_cptr, p, d, None, f), np.uint32, devptr, int)

    def stoi(self, devptr=0):
        """nvstrings.py:696-715 -- int32 per row (NVStrings::stoi)."""
        return self._convert(lambda p, d, f: lib.cs_stoi(self.m_cptr, p, d, None, f), np.int32, devptr, int)

    def stol(self, devptr=0):
        """nvstrings.py:717-736 -- int64 per row (NVStrings::stol)."""
        return self._convert(lambda p, d, f: lib.cs_stol(self.m_cptr, p, d, None, f), np.int64, devptr, int)

    def stof(self, devptr=0):
        """nvstrings.py:738-758 -- float32 per row (NVStrings::stof)."""
        return self._convert(lambda p, d, f: lib.cs_stof(self.m_cptr, p, d, None, f), np.float32, devptr, float)

    def stod(self, devptr=0):
        """nvstrings.py:760-780 -- float64 per row (NVStrings::stod)."""
        return self._convert(lambda p, d, f: lib.cs_stod(self.m_cptr, p, d, None, f), np.float64, devptr, float)

    def htoi(self, devptr=0):
        """nvstrings.py:782-802 -- hexadecimal strings to uint32 (NVStrings::htoi)."""
        return self._convert(lambda p, d, f: lib.cs_htoi(self.m_cptr, p, d, None, f), np.uint32, devptr, int)

    def ip2int(self, devptr=0):
        """nvstrings.py:827-848 -- dotted-quad strings to uint32 (NVStrings::ip2int)."""
        return self._convert(lambda p, d, f: lib.cs_ip2int(self.m_cptr, p, d, None, f), np.uint32, devptr, int)

    def to_booleans(self, true="True", devptr=0):
        """nvstrings.py:804-825 -- True where the row equals `true`; a null row is None in the host list
        (on the device: 1 when `true` is None, else 0)."""
        return self._convert(lambda p, d, f: lib.cs_to_bools(self.m_cptr, b(true), p, d, None, f), np.uint8, devptr, bool)

    # ---- substrings / padding / wrapping (nvstrings.py:1129-1460; substr.cu, pad.cu, modify.cu) ----------------
    def _made(self, fn):
        out = C.c_void_p()
        check(fn(C.byref(out)))
        return nvstrings(out.value)

    def get(self, i):
        """nvstrings.py:1129-1151 -- the character at position i of every row (an empty row past the end)."""
        return self.slice(i & 0xFFFFFFFF, (i + 1) & 0xFFFFFFFF)

    def repeat(self, repeats):
        """nvstrings.py:1153-1175 -- every row repeated; a count of 0 or 1 gives a copy."""
        return self._made(lambda o: lib.cs_repeat(self.m_cptr, repeats & 0xFFFFFFFF, None, o))

    def _pad(self, width, side, fillchar):
        if fillchar is not None and len(fillchar) == 0:
            raise ValueError("fillchar cannot be empty")
        return self._made(lambda o: lib.cs_pad(self.m_cptr, width & 0xFFFFFFFF, side, b(fillchar), None, o))

    def pad(self, width, side="left", fillchar=" "):
        """nvstrings.py:1177-1205 -- fill rows shorter than width characters; side 'left', 'right' or 'both'."""
        return self._pad(width, {"right": 1, "both": 2}.get(side, 0), fillchar)

    def ljust(self, width, fillchar=" "):
        """nvstrings.py:1207-1233 -- fill on the right to width characters."""
        return self._pad(width, 1, fillchar)

    def center(self, width, fillchar=" "):
        """nvstrings.py:1235-1261 -- fill on both sides to width characters (the odd one on the right)."""
        return self._pad(width, 2, fillchar)

    def rjust(self, width, fillchar=" "):
        """nvstrings.py:1263-1289 -- fill on the left to width characters."""
        return self._pad(width, 0, fillchar)

    def zfill(self, width):
        """nvstrings.py:1291-1315 -- '0' fill on the left to width characters, after a leading sign."""
        return self._made(lambda o: lib.cs_zfill(self.m_cptr, width & 0xFFFFFFFF, None, o))

    def wrap(self, width):
        """nvstrings.py:1317-1340 -- lines of about width characters: whitespace becomes ' ', some of it '\\n'."""
        return self._made(lambda o: lib.cs_wrap(self.m_cptr, width & 0xFFFFFFFF, None, o))

    def slice(self, start, stop=None, step=None):
        """nvstrings.py:1342-1369 -- characters [start, stop) of every row (stop None or <= 0: to the end), every
        step-th one.  start > stop > 0 is a ValueError."""
        stop = -1 if stop is None else stop
        step = 1 if step is None else step
        return self._made(lambda o: lib.cs_slice(self.m_cptr, start, stop, step, None, o))

    def slice_from(self, starts=0, stops=0):
        """nvstrings.py:1371-1403 -- slice with a start and a stop per row: int32 device addresses (0 = none: 0 / -1),
        device tensors, or host lists / numpy arrays."""
        def arr(v):
            if v is None or (isinstance(v, int) and v == 0):
                return None, 0, None
            if isinstance(v, int):
                return v, 1, None
            if hasattr(v, "data_ptr"):
                if v.dtype.itemsize != 4 or v.dtype.is_floating_point:
                    raise TypeError("nvstrings.slice_from(): starts / stops must be int32")
                if v.numel() < self.size():
                    raise ValueError("nvstrings.slice_from(): starts / stops need size() values")
                return v.data_ptr(), 1 if v.is_cuda else 0, v
            a = np.ascontiguousarray(v, dtype=np.int32)
            if a.size < self.size():
                raise ValueError("nvstrings.slice_from(): starts / stops need size() values")
            return a.ctypes.data, 0, a
        ps, ds, k1 = arr(starts)
        pe, de, k2 = arr(stops)
        if ps and pe and ds != de:  # (one on the host, the other on the device: both to the host)
            raise ValueError("nvstrings.slice_from(): starts and stops must both be on the host or both on the device")
        dev = ds or de
        r = self._made(lambda o: lib.cs_slice_from(self.m_cptr, ps, pe, dev, None, o))
        del k1, k2
        return r

    def slice_replace(self, start=None, stop=None, repl=None):
        """nvstrings.py:1405-1432 -- characters [start, stop) replaced with repl (start None = 0, stop None = the end); a
        start past the end appends."""
        start = 0 if start is None else start
        stop = -1 if stop is None else stop
        return self._made(lambda o: lib.cs_slice_replace(self.m_cptr, b(repl), start, stop, None, o))

    def insert(self, start=0, repl=None):
        """nvstrings.py:1434-1460 -- repl inserted at character position start (-1 = the end)."""
        start = 0 if start is None else start
        return self._made(lambda o: lib.cs_insert(self.m_cptr, b(repl), start, None, o))

    # ---- character types (attrs.cu:115-438) and swapcase / capitalize / title (case.cu:169-397) ----------------------
    def _chartype(self, pred, devptr):
        return self._bools(lambda out, dev, f: lib.cs_chartype(self.m_cptr, pred, out, dev, None, f), devptr)

    def isalnum(self, devptr=0):
        """True where the row is not empty and every character is a letter or a digit of any kind (decimal, digit,
        numeric); a null row is None in the host list, False on the device."""
        return self._chartype(0, devptr)

    def isalpha(self, devptr=0):
        """True where the row is not empty and every character is alphabetic."""
        return self._chartype(1, devptr)

    def isdigit(self, devptr=0):
        """True where the row is not empty and every character is a digit (superscripts included)."""
        return self._chartype(2, devptr)

    def isspace(self, devptr=0):
        """True where the row is not empty and every character is white space."""
        return self._chartype(3, devptr)

    def isdecimal(self, devptr=0):
        """True where the row is not empty and every character is a decimal digit."""
        return self._chartype(4, devptr)

    def isnumeric(self, devptr=0):
        """True where the row is not empty and every character is numeric (fractions included)."""
        return self._chartype(5, devptr)

    def islower(self, devptr=0):
        """True where the row is not empty and none of its alphabetic characters is upper case ("123" is True)."""
        return self._chartype(6, devptr)

    def isupper(self, devptr=0):
        """True where the row is not empty and none of its alphabetic characters is lower case ("123" is True)."""
        return self._chartype(7, devptr)

    def is_empty(self, devptr=0):
        """True where the row has no bytes; a null row is None in the host list, True on the device."""
        return self._chartype(8, devptr)

    def swapcase(self):
        """Every cased character becomes its opposite-case one."""
        return self._made(lambda o: lib.cs_swapcase(self.m_cptr, None, o))

    def capitalize(self):
        """The first character to upper, the others to lower case (characters up to U+0FFF only, as the reference)."""
        return self._made(lambda o: lib.cs_capitalize(self.m_cptr, None, o))

    def title(self):
        """A letter after a non-letter (or at the start) to upper, a letter after a letter to lower case."""
        return self._made(lambda o: lib.cs_title(self.m_cptr, None, o))

    # ---- index / rindex, the URL codec, translate, fillna (nvstrings.py:1558, 1740-1794, 2303, 2589-2627) ------------
    def _index(self, name, fn, sub, start, end, devptr):
        end = -1 if end is None else int(end)
        rows = self.size()
        found = C.c_int64()
        if devptr:
            check(fn(self.m_cptr, b(sub), int(start), end, devptr, 1, None, C.byref(found)))
            if found.value != rows:  # (null rows count as found; the results are in the caller's buffer either way)
                raise ValueError("nvstrings.%s: [%s] not found in %d elements" % (name, sub, rows - found.value))
            return devptr
        res = np.zeros(max(rows, 1), dtype=np.int32)
        check(fn(self.m_cptr, b(sub), int(start), end, res.ctypes.data, 0, None, C.byref(found)))
        out = []
        for i, v in enumerate(res[:rows]):
            if v == -1:
                raise ValueError("nvstrings.%s: [%s] not found in element %d" % (name, sub, i))
            out.append(None if v < -1 else int(v))
        return out

    def index(self, sub, start=0, end=None, devptr=0):
        """nvstrings.py:1740-1766 -- find that raises ValueError when some row does not hold `sub`; None for null rows."""
        return self._index("index", lib.cs_find, sub, start, end, devptr)

    def rindex(self, sub, start=0, end=None, devptr=0):
        """nvstrings.py:1768-1794 -- rfind that raises ValueError when some row does not hold `sub`."""
        return self._index("rindex", lib.cs_rfind, sub, start, end, devptr)

    def url_encode(self):
        """nvstrings.py:2589-2607 -- every byte but 0-9 A-Z a-z . _ ~ - becomes '%' and two upper-case hex digits."""
        return self._made(lambda o: lib.cs_url_encode(self.m_cptr, None, o))

    def url_decode(self):
        """nvstrings.py:2609-2627 -- '%' and the two bytes behind it become one byte."""
        return self._made(lambda o: lib.cs_url_decode(self.m_cptr, None, o))

    def translate(self, table):
        """nvstrings.py:2303-2330 -- every character that is a key of `table` becomes its target, None drops it: a dict
        of ordinal -> ordinal | None (str.maketrans), or a list of [char, char | None].  Of several entries with one
        key the last wins."""
        def cp(v, none_ok):
            if v is None and none_ok:
                return 0
            if isinstance(v, str) and len(v) >= 1:
                return ord(v[0])
            if isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= 0xFFFFFFFF:
                return v
            raise ValueError("nvstrings.translate: invalid map entry")
        if isinstance(table, dict):
            pairs = [(cp(k, False), cp(v, True)) for k, v in table.items()]
        elif isinstance(table, list):
            for e in table:
                if not isinstance(e, (list, tuple)) or len(e) != 2:
                    raise ValueError("nvstrings.translate: invalid map entry")
            pairs = [(cp(e[0], False), cp(e[1], True)) for e in table]
        else:
            raise ValueError("nvstrings.translate: invalid argument type")
        keys = np.array([p[0] for p in pairs], dtype=np.uint32)
        vals = np.array([p[1] for p in pairs], dtype=np.uint32)
        return self._made(lambda o: lib.cs_translate(self.m_cptr, keys.ctypes.data if len(pairs) else None,
                                                     vals.ctypes.data if len(pairs) else None, len(pairs), None, o))

    def fillna(self, repl):
        """nvstrings.py:1558-1582 -- null rows take `repl`: a str, or the same row of another nvstrings of this size."""
        if repl is None:
            raise ValueError("nvstrings.fillna repl argument must be specified")
        if isinstance(repl, str):
            return self._made(lambda o: lib.cs_fillna(self.m_cptr, b(repl), None, o))
        if not isinstance(repl, nvstrings):
            raise ValueError("nvstrings.fillna repl argument must be a str or an nvstrings object")
        if repl.size() != self.size():
            raise ValueError("nvstrings.fillna repl argument must be same size")
        return self._made(lambda o: lib.cs_fillna_column(self.m_cptr, repl.m_cptr, None, o))

    def timestamp2int(self, format=None, units="s", devptr=0):
        """
        Returns integer value represented by each string.
        String is interpretted using the format provided.
        The values are returned in the units specified based
        on epoch time and in UTC.

        Parameters
        ----------
        format : str
            May include the following strptime specifiers only:
            %Y,%y,%m,%d,%H,%I,%p,%M,%S,%f,%z
            Default format is "%Y-%m-%dT%H:%M:%SZ"
        units : str
            The units of the values and must be one of the following:
            Y,M,D,h,m,s,ms,us,ns
            Default is 's' for seconds
        devptr : GPU memory pointer
            Where resulting integer values will be written.
            Memory must be able to hold at least size() of int64 values.

        Examples
        --------
        >>> import nvstrings
        >>> s = nvstrings.to_device(["2019-03-20T12:34:56Z"])
        >>> print(s.timestamp2int())
        [1553085296]

        """
        u = _ts_units(units)
        fmt = None if format is None else b(format)
        return self._convert(lambda p, d, f: lib.cs_timestamp2long(self.m_cptr, fmt, u, p, d, None, f), np.int64, devptr, int)

    # ---- parity helper ---------------------------------------------------------------------
    def digest(self):
        d = C.c_uint64()
        check(lib.cs_column_digest(self.m_cptr, None, C.byref(d)))
        return d.value


def _compile(pat):
    if pat is None:
        raise ValueError("pattern cannot be null")
    re = C.c_void_p()
    check(lib.cs_regex_compile(b(pat), C.byref(re)))
    return re
