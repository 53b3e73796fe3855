"""`nvcategory` -- host-side mirror of /root/reference/python/nvcategory.py for the
hot path (dictionary encoding: sorted unique keys + int32 values), over the C ABI.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import nvstrings as _nvs
from ._lib import lib, check

__all__ = ["to_device", "from_offsets", "from_strings", "from_strings_list", "from_numbers", "bind_cpointer", "nvcategory"]


def _build(col_ptr):
    out = C.c_void_p()
    check(lib.cs_category_build(col_ptr, None, C.byref(out)))
    return nvcategory(out.value)


def to_device(strs):
    """nvcategory.py:5-25 -- category straight from a host list."""
    s = _nvs.to_device(strs)
    return _build(s.m_cptr)


def from_offsets(sbuf, obuf, scount, nbuf=None, ncount=0, bdevmem=False):
    """nvcategory.py:28-75 (NVCategory::create_from_offsets, NVCategory.h:101)."""
    s = _nvs.from_offsets(sbuf, obuf, scount, nbuf, ncount, bdevmem)
    return _build(s.m_cptr)


def from_strings(*args):
    """nvcategory.py:78-103 -- one category over the rows of 1..n nvstrings, in order
    (NVCategory::create_from_strings, NVCategory.h:107,114)."""
    return from_strings_list(list(args))


def from_strings_list(list):
    """nvcategory.py:106-128."""
    _lib.ensure_init()
    if len(list) == 1:
        return _build(list[0].m_cptr)
    arr = (C.c_void_p * max(len(list), 1))(*[s.m_cptr for s in list])
    out = C.c_void_p()
    check(lib.cs_column_concat(arr, len(list), None, C.byref(out)))
    allrows = _nvs.nvstrings(out.value)
    return _build(allrows.m_cptr)


def from_categories(cats):
    """NVCategory::create_from_categories (NVCategory.h:121; NVCategory.cu:430-514):
    merged key set, concatenated remapped values."""
    _strings_only(cats, "from_categories")
    arr = (C.c_void_p * max(len(cats), 1))(*[c.m_cptr for c in cats])
    out = C.c_void_p()
    check(lib.cs_category_merge(arr, len(cats), None, C.byref(out)))
    return nvcategory(out.value)


IPC_CATEGORY_BYTES = (3 * 64 + 3 * 8 + 4 * 4) + 64 + 8  # sizeof(cs_ipc_category)


def create_from_ipc(ipc_data):
    """A category over the buffers another process exported with get_ipc_data() (NVCategory::create_from_ipc,
    NVCategory.h:128; the reference exposes it in C++ only)."""
    _lib.ensure_init()
    rec = C.create_string_buffer(bytes(ipc_data), IPC_CATEGORY_BYTES)
    out = C.c_void_p()
    check(lib.cs_category_ipc_import(rec, C.byref(out)))
    return nvcategory(out.value)


def _strings_only(cats, what):
    for c in cats:
        if getattr(c, "_numeric", False):
            raise ValueError("%s: a category of numbers where a category of strings is required" % what)


def bind_cpointer(cptr, own=True):
    """nvcategory.py:157-163."""
    if not cptr:
        return None
    return nvcategory(cptr, own)


_NOT_BUILT = []  # every method of the reference's class is built


def _ints(values, count=0):
    if isinstance(values, int):
        return values, int(count), 1, None
    if hasattr(values, "data_ptr"):
        return values.data_ptr(), int(count) or values.numel(), 1, values
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a.ctypes.data, len(a), 0, a


def _checked(status):
    if status == _lib.CS_ERR_RANGE:
        raise IndexError(_lib.last_error())  # std::out_of_range in the reference
    check(status)


class nvcategory:
    """Reference class: nvcategory.py:166-192."""

    def __init__(self, cptr, own=True):
        self.m_cptr = cptr
        self._own = own

    def get_ipc_data(self):
        """The record for create_from_ipc in another process (NVCategory::create_ipc_transfer, NVCategory.h:176)."""
        rec = C.create_string_buffer(IPC_CATEGORY_BYTES)
        check(lib.cs_category_ipc_export(self.m_cptr, rec))
        return rec.raw

    _cs_abi = True  # m_cptr is a cs_category* (the pyni glue wraps it on demand, see host/pyni_common.h)
    _nv_cptr = None

    def __del__(self):
        try:
            if self._nv_cptr:
                import pyniNVCategory

                pyniNVCategory.n_dropWrapper(self._nv_cptr)
                self._nv_cptr = None
            if self.m_cptr and self._own:
                lib.cs_category_destroy(self.m_cptr)
            self.m_cptr = 0
        except Exception:
            pass

    def keys_type(self):
        """nvcategory.py:276-290 -- "str" for a category of strings."""
        return "str"

    def __str__(self):
        return "keys: " + str(self.keys()) + "\nvalues: " + str(self.values())

    def __repr__(self):
        return "<nvcategory keys={},values={}>".format(self.keys_size(), self.size())

    def get_cpointer(self):
        return self.m_cptr

    def size(self):
        """nvcategory.py:200-219."""
        return int(lib.cs_category_size(self.m_cptr))

    def keys_size(self):
        """nvcategory.py:221-240."""
        return int(lib.cs_category_keys_size(self.m_cptr))

    def keys(self, narr=None):
        """nvcategory.py:242-274 -- the sorted unique keys as an nvstrings."""
        out = C.c_void_p()
        check(lib.cs_category_keys(self.m_cptr, C.byref(out)))
        return _nvs.nvstrings(out.value)

    def values(self, devptr=0, bdevmem=None):
        """nvcategory.py:364-389 -- int32 key index per row.  `devptr`: an int address or a tensor with
        data_ptr() is device memory, a numpy array host memory (bdevmem overrides)."""
        if devptr is not None and not (isinstance(devptr, int) and devptr == 0):
            p, keep = _lib.addr(devptr)
            on_device = 1 if (isinstance(devptr, int) or hasattr(devptr, "data_ptr") or hasattr(devptr, "__cuda_array_interface__")) else 0
            if bdevmem is not None:
                on_device = 1 if bdevmem else 0
            check(lib.cs_category_get_values(self.m_cptr, p, on_device, None))
            return devptr
        n = self.size()
        res = np.zeros(max(n, 1), dtype=np.int32)
        if n:
            check(lib.cs_category_get_values(self.m_cptr, res.ctypes.data, 0, None))
        return res[:n].tolist()

    def values_cpointer(self):
        """nvcategory.py:391-396."""
        return lib.cs_category_values_ptr(self.m_cptr)

    def value_for_index(self, idx):
        """nvcategory.py:324-341 -- the row's value; -1 for an index outside the rows, a negative one too
        (NVCategory::get_value, NVCategory.cu:754-763, takes it as unsigned)."""
        return self.values()[idx] if 0 <= idx < self.size() else -1

    def value(self, str):
        """nvcategory.py:343-362 -- index of a key (None: the null key), -1 when absent."""
        k = self.keys().to_host()
        return k.index(str) if str in k else -1

    def indexes_for_key(self, str, devptr=0):
        """nvcategory.py:292-322 -- the rows whose value is the given key, as a list; with `devptr` (a numpy int32 array, a
        device tensor or a device address) they are written there and their number is returned.  A string that is no
        key raises ValueError (pycategory.cpp:371-372)."""
        k = self.value(str)
        if k < 0:
            raise ValueError("nvcategory: string not found in keys")
        count = C.c_int64()
        if isinstance(devptr, int) and devptr == 0:
            check(lib.cs_category_indexes_for(self.m_cptr, k, None, 0, None, C.byref(count)))
            res = np.zeros(max(count.value, 1), dtype=np.int32)
            if count.value:
                check(lib.cs_category_indexes_for(self.m_cptr, k, res.ctypes.data, 0, None, C.byref(count)))
            return res[: count.value].tolist()
        rp, n, dev, keep = _typed(devptr, 1, "indexes_for_key")
        if n is not None and n < self.size():  # an array that may be too short: count first
            check(lib.cs_category_indexes_for(self.m_cptr, k, None, 0, None, C.byref(count)))
            _room(n, count.value, "indexes_for_key")
        check(lib.cs_category_indexes_for(self.m_cptr, k, rp, dev, None, C.byref(count)))
        return int(count.value)

    def _cat_call(self, fn, *args):
        out = C.c_void_p()
        _checked(fn(self.m_cptr, *args, None, C.byref(out)))
        return nvcategory(out.value)

    def to_strings(self):
        """nvcategory.py:419-436 -- the original strings back (NVCategory::to_strings)."""
        out = C.c_void_p()
        check(lib.cs_category_to_strings(self.m_cptr, None, C.byref(out)))
        return _nvs.nvstrings(out.value) if out.value else None

    def gather_strings(self, indexes, count=0):
        """nvcategory.py:438-470 -- keys[indexes[i]] as strings; an index outside the keys raises."""
        p, n, dev, keep = _ints(indexes, count)
        out = C.c_void_p()
        _checked(lib.cs_category_gather_strings(self.m_cptr, p, n, dev, None, C.byref(out)))
        return _nvs.nvstrings(out.value)

    def gather(self, indexes, count=0):
        """nvcategory.py:510-545 -- same keys, the given indexes as values."""
        p, n, dev, keep = _ints(indexes, count)
        return self._cat_call(lib.cs_category_gather, p, n, dev)

    def gather_and_remap(self, indexes, count=0):
        """nvcategory.py:472-508 -- only the keys the indexes name, values renumbered."""
        p, n, dev, keep = _ints(indexes, count)
        return self._cat_call(lib.cs_category_gather_and_remap, p, n, dev)

    def add_strings(self, nvs):
        """nvcategory.py:547-574."""
        return self._cat_call(lib.cs_category_add_strings, nvs.m_cptr)

    def remove_strings(self, nvs):
        """nvcategory.py:576-603."""
        return self._cat_call(lib.cs_category_remove_strings, nvs.m_cptr)

    def merge_category(self, nvcat):
        """nvcategory.py:669-685 -- the other category's new keys are appended behind these keys (NVCategory.cu:1223-1337)."""
        _strings_only([nvcat], "merge_category")
        return self._cat_call(lib.cs_category_merge_category, nvcat.m_cptr)

    def merge_and_remap(self, nvcat):
        """nvcategory.py:687-715 -- merged sorted key set, both value lists renumbered."""
        return from_categories([self, nvcat])

    def add_keys(self, strs):
        """nvcategory.py:605-624 (NVCategory::add_keys_and_remap)."""
        return self._cat_call(lib.cs_category_add_keys, strs.m_cptr)

    def remove_keys(self, strs):
        """nvcategory.py:626-645 (NVCategory::remove_keys_and_remap)."""
        return self._cat_call(lib.cs_category_remove_keys, strs.m_cptr)

    def remove_unused_keys(self):
        """nvcategory.py:717-733 (NVCategory::remove_unused_keys_and_remap)."""
        return self._cat_call(lib.cs_category_remove_unused_keys)

    def set_keys(self, strs):
        """nvcategory.py:647-667 (NVCategory::set_keys_and_remap)."""
        return self._cat_call(lib.cs_category_set_keys, strs.m_cptr)


# ---- numeric categories (numeric_category.h; python/cpp/numeric_category.cpp) -------------------------------------------
_NUM_NAMES = ["int8", "int32", "int64", "float32", "float64"]  # cs_numtype order


def _numtype(dtype_name):
    name = str(dtype_name).replace("torch.", "")
    if name.startswith("datetime64"):
        name = "int64"  # numeric_category.cpp: datetime64[*] is taken as int64
    if name not in _NUM_NAMES:
        raise ValueError("invalid dtype in nvcategory dispatcher: %s" % dtype_name)
    return _NUM_NAMES.index(name)


def _numbers(arr):
    """numpy array or device tensor -> (address, count, on_device, cs_numtype, keepalive)."""
    if hasattr(arr, "data_ptr") and hasattr(arr, "dtype"):
        t = arr.contiguous()
        return t.data_ptr(), t.numel(), 1 if t.is_cuda else 0, _numtype(t.dtype), t
    if isinstance(arr, np.ndarray):
        code = _numtype(arr.dtype)
        a = np.ascontiguousarray(arr)
        return a.ctypes.data, a.size, 0, code, a
    raise ValueError("invalid dtype in nvcategory dispatcher: %s" % type(arr).__name__)


def _typed(arr, code, what):
    """The same for an array that must hold the category's type; a bare address is device memory of that type."""
    if isinstance(arr, int):
        return arr, None, 1, None
    p, n, dev, got, keep = _numbers(arr)
    if got != code:
        raise ValueError("%s: array of %s given to a category of %s" % (what, _NUM_NAMES[got], _NUM_NAMES[code]))
    return p, n, dev, keep


def _room(n, need, what):
    """An output array of known length must hold what is written to it."""
    if n is not None and n < need:
        raise ValueError("%s: the array holds %d items, %d are required" % (what, n, need))


def _mask_room(nulls, items, what):
    n = nulls.numel() * nulls.element_size() if hasattr(nulls, "numel") else getattr(nulls, "nbytes", None)
    _room(n, (items + 7) // 8, what + " (nulls)")


def _bytes_arg(arr):
    """A bitmask: numpy array of a one-byte type, device tensor or device address -> (address, on_device, keepalive)."""
    if arr is None:
        return None, None, None
    if isinstance(arr, int):
        return arr or None, 1, None
    if hasattr(arr, "data_ptr"):
        return arr.data_ptr(), 1 if arr.is_cuda else 0, arr
    a = np.ascontiguousarray(arr)
    return a.ctypes.data, 0, a


def _same_side(dev, other, what):
    if other is not None and other != dev:
        raise ValueError("%s: the arrays must all be host memory or all device memory" % what)


def from_numbers(narr, nulls=None):
    """nvcategory.py:131-154 -- a category over an array of numbers (numpy, or a device tensor); `nulls`: LSB-first
    bitmask, a 0 bit is a null item."""
    _lib.ensure_init()
    p, n, dev, code, keep = _numbers(narr)
    np_, ndev, nkeep = _bytes_arg(nulls)
    _same_side(dev, ndev, "from_numbers")
    out = C.c_void_p()
    check(lib.cs_numcat_build(p, n, np_, code, dev, None, C.byref(out)))
    return numeric_nvcategory(out.value)


class numeric_nvcategory(nvcategory):
    """An nvcategory whose keys are numbers: m_cptr is a cs_numcat*.  The pyniNVCategory glue knows such an object by
    `_numeric` and takes the handle as it is (no C++ instance is wrapped around it)."""

    _numeric = True

    def __del__(self):
        try:
            if self.m_cptr and self._own:
                lib.cs_numcat_destroy(self.m_cptr)
            self.m_cptr = 0
        except Exception:
            pass

    def get_ipc_data(self):
        raise ValueError("get_ipc_data: a category of numbers has no IPC record")

    @property
    def _code(self):
        return lib.cs_numcat_type(self.m_cptr)

    @property
    def _dtype(self):
        return np.dtype(_NUM_NAMES[self._code])

    def keys_type(self):
        """nvcategory.py:276-290."""
        return _NUM_NAMES[self._code]

    def size(self):
        return int(lib.cs_numcat_size(self.m_cptr))

    def keys_size(self):
        return int(lib.cs_numcat_keys_size(self.m_cptr))

    def keys_have_null(self):
        return bool(lib.cs_numcat_keys_have_null(self.m_cptr))

    def has_nulls(self):
        return bool(lib.cs_numcat_has_nulls(self.m_cptr))

    def keys_cpointer(self):
        return lib.cs_numcat_keys_ptr(self.m_cptr)

    def values_cpointer(self):
        return lib.cs_numcat_values_ptr(self.m_cptr)

    def nulls_cpointer(self):
        return lib.cs_numcat_nulls_ptr(self.m_cptr)

    def keys(self, narr=None):
        """The keys into `narr`, or as a list with None for the null key (numeric_category.cpp:317-345)."""
        if narr is not None:
            p, n, dev, keep = _typed(narr, self._code, "keys")
            _room(n, self.keys_size(), "keys")
            check(lib.cs_numcat_get_keys(self.m_cptr, p, dev, None))
            return narr
        k = np.zeros(max(self.keys_size(), 1), dtype=self._dtype)
        check(lib.cs_numcat_get_keys(self.m_cptr, k.ctypes.data, 0, None))
        res = k[: self.keys_size()].tolist()
        if res and self.keys_have_null():
            res[0] = None
        return res

    def values(self, devptr=0, bdevmem=None):
        """The int32 values into `devptr`, or as a list with None for null rows (numeric_category.cpp:424-453)."""
        if devptr is not None and not (isinstance(devptr, int) and devptr == 0):
            p, keep = _lib.addr(devptr)
            on_device = 1 if (isinstance(devptr, int) or getattr(devptr, "is_cuda", False)) else 0
            if not isinstance(devptr, int):
                _typed(devptr, 1, "values")
                _room(devptr.numel() if hasattr(devptr, "numel") else getattr(devptr, "size", None), self.size(), "values")
            if bdevmem is not None:
                on_device = 1 if bdevmem else 0
            check(lib.cs_numcat_get_values(self.m_cptr, p, on_device, None))
            return devptr
        n = self.size()
        v = np.zeros(max(n, 1), dtype=np.int32)
        check(lib.cs_numcat_get_values(self.m_cptr, v.ctypes.data, 0, None))
        res = v[:n].tolist()
        if self.keys_have_null():
            res = [None if x == 0 else x for x in res]
        return res

    def _key(self, key):
        """A number as one item of the keys' type -> (address or None for the null key, keepalive, absent).  `absent`: the
        number is none of the type's values (300 for int8, 1.5 for int32), so no key can equal it."""
        if key is None:
            return None, None, False
        dt = self._dtype
        if dt.kind == "i":
            try:
                whole = int(key)
            except (OverflowError, ValueError):  # inf, NaN
                return None, None, True
            info = np.iinfo(dt)
            if whole != key or whole < info.min or whole > info.max:
                return None, None, True
            a = np.array([whole], dtype=dt)
        else:
            a = np.array([key]).astype(dt)
        return a.ctypes.data, a, False

    def value(self, key):
        """Index of a key (None: the null key), -1 when absent."""
        p, keep, absent = self._key(key)
        if absent:
            return -1
        out = C.c_int32()
        check(lib.cs_numcat_index_for(self.m_cptr, p, None, C.byref(out)))
        return out.value

    def indexes_for_key(self, key, devptr=0):
        """nvcategory.py:292-322 -- how many rows hold the key; with `devptr` their indexes are written there."""
        p, keep, absent = self._key(key)
        if absent:
            return 0
        count = C.c_int64()
        if isinstance(devptr, int) and devptr == 0:  # the count alone: one counting pass
            check(lib.cs_numcat_indexes_for(self.m_cptr, p, None, 0, None, C.byref(count)))
            return int(count.value)
        rp, n, dev, rkeep = _typed(devptr, 1, "indexes_for_key")
        if n is not None and n < self.size():  # an array that may be too short: count first
            check(lib.cs_numcat_indexes_for(self.m_cptr, p, None, 0, None, C.byref(count)))
            _room(n, count.value, "indexes_for_key")
        check(lib.cs_numcat_indexes_for(self.m_cptr, p, rp, dev, None, C.byref(count)))
        return int(count.value)

    def to_numbers(self, narr, nulls=None):
        """nvcategory.py:489-516."""
        p, n, dev, keep = _typed(narr, self._code, "to_numbers")
        _room(n, self.size(), "to_numbers")
        np_, ndev, nkeep = _bytes_arg(nulls)
        _mask_room(nulls, self.size(), "to_numbers")
        _same_side(dev, ndev, "to_numbers")
        check(lib.cs_numcat_to_type(self.m_cptr, p, np_, dev, None))
        return narr

    def gather_numbers(self, indexes, narr, nulls=None):
        """nvcategory.py:552-582 -- keys[indexes[i]]; an index outside the keys raises IndexError."""
        ip, n, idev, ikeep = _typed(indexes, 1, "gather_numbers")
        p, room, dev, keep = _typed(narr, self._code, "gather_numbers")
        np_, ndev, nkeep = _bytes_arg(nulls)
        _same_side(dev, idev, "gather_numbers")
        _same_side(dev, ndev, "gather_numbers")
        if n is None:
            raise ValueError("gather_numbers: the indexes need a length")
        _room(room, n, "gather_numbers")
        _mask_room(nulls, n, "gather_numbers")
        _checked(lib.cs_numcat_gather_type(self.m_cptr, ip, n, p, np_, dev, None))
        return narr

    def _num_call(self, fn, *args):
        out = C.c_void_p()
        _checked(fn(self.m_cptr, *args, None, C.byref(out)))
        return numeric_nvcategory(out.value)

    def _by_indexes(self, fn, indexes, count):
        p, n, dev, keep = _ints(indexes, count)
        return self._num_call(fn, p, n, dev)

    def gather(self, indexes, count=0):
        return self._by_indexes(lib.cs_numcat_gather, indexes, count)

    def gather_and_remap(self, indexes, count=0):
        return self._by_indexes(lib.cs_numcat_gather_and_remap, indexes, count)

    def gather_values(self, indexes, count=0):
        return self._by_indexes(lib.cs_numcat_gather_values, indexes, count)

    def _by_keys(self, fn, what, narr, nulls):
        p, n, dev, keep = _typed(narr, self._code, what)
        if n is None:
            raise ValueError("%s: the keys need a dtype" % what)
        np_, ndev, nkeep = _bytes_arg(nulls)
        _same_side(dev, ndev, what)
        return self._num_call(fn, p, n, np_, dev)

    def add_keys(self, narr, nulls=None):
        return self._by_keys(lib.cs_numcat_add_keys, "add_keys", narr, nulls)

    def remove_keys(self, narr, nulls=None):
        return self._by_keys(lib.cs_numcat_remove_keys, "remove_keys", narr, nulls)

    def set_keys(self, narr, nulls=None):
        return self._by_keys(lib.cs_numcat_set_keys, "set_keys", narr, nulls)

    def remove_unused_keys(self):
        return self._num_call(lib.cs_numcat_remove_unused_keys)

    def merge_and_remap(self, nvcat):
        """Merged sorted key set, both value lists renumbered; a category of another type raises (numeric_category.cpp:847-851)."""
        if not getattr(nvcat, "_numeric", False) or nvcat._code != self._code:
            raise ValueError("merge_and_remap: the categories hold different types")
        return self._num_call(lib.cs_numcat_merge, nvcat.m_cptr)

    def copy(self):
        return self._num_call(lib.cs_numcat_copy)

    def value_for_index(self, idx):
        return self.values()[idx]

    def _strings_only(self, *args, **kwargs):
        raise ValueError("a category of %s has no strings" % self.keys_type())

    to_strings = gather_strings = add_strings = remove_strings = merge_category = _strings_only
