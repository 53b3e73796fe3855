"""`splitre` -- rows of a strings column split at the matches of a regex (cs_split_re, cs_rsplit_re and the record
entries).  The definition is custrings_amd/csrc/splitre_ops.h: the matches are those findall returns; empty tokens are kept;
with n > 0 split_re cuts at a row's first n matches, rsplit_re at its last n; a pattern that can match the empty string is
refused (ValueError).

    cols = splitre.split_re(strs, r"\\s*[,;]\\s*")              # column-major: cols[k] holds every row's token k
    head, tail = splitre.rsplit_re(strs, r"\\d+", 1)            # cut at the last match only
    flat, offsets = splitre.split_record_re(strs, r"\\s+", flat=True)
"""
import ctypes as C

import numpy as np

from ._lib import lib, check
from .nvstrings import nvstrings, _compile

__all__ = ["split_re", "rsplit_re", "split_record_re", "rsplit_record_re"]


def _columns(fn, strs, pat, n):
    re = _compile(pat)
    arr = C.POINTER(C.c_void_p)()
    ncols = C.c_int()
    try:
        check(fn(strs.m_cptr, re, int(n), None, C.byref(arr), C.byref(ncols)))
    finally:
        lib.cs_regex_destroy(re)
    out = [nvstrings(arr[i]) for i in range(ncols.value)]
    if ncols.value:
        lib.cs_free(arr)
    return out


def _records(fn, strs, pat, n, flat):
    rows = strs.size()
    loff = np.zeros(rows + 1, dtype=np.int64)
    out = C.c_void_p()
    re = _compile(pat)
    try:
        check(fn(strs.m_cptr, re, int(n), loff.ctypes.data, 0, None, C.byref(out)))
    finally:
        lib.cs_regex_destroy(re)
    f = nvstrings(out.value)
    if flat:
        return f, loff
    nulls = strs._null_flags() if rows else []
    return [None if nulls[r] else f.sublist(int(loff[r]), int(loff[r + 1]), 1) for r in range(rows)]


def split_re(strs, pat, n=-1):
    """Column-major split at the matches of `pat`: a list of nvstrings, null where a row has fewer tokens."""
    return _columns(lib.cs_split_re, strs, pat, n)


def rsplit_re(strs, pat, n=-1):
    """split_re cutting at the LAST n matches of a row (the matches are still found left to right)."""
    return _columns(lib.cs_rsplit_re, strs, pat, n)


def split_record_re(strs, pat, n=-1, flat=False):
    """split_re in the record form of nvstrings.split_record: one nvstrings per row holding its tokens (None for a null
    row); flat=True returns the native form: (all tokens in row-major order, rows+1 list offsets)."""
    return _records(lib.cs_split_record_re, strs, pat, n, flat)


def rsplit_record_re(strs, pat, n=-1, flat=False):
    """rsplit_re in the record form."""
    return _records(lib.cs_rsplit_record_re, strs, pat, n, flat)
