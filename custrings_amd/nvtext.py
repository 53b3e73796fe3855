"""`nvtext` -- host-side mirror of /root/reference/python/nvtext.py over the C ABI."""
import ctypes as C

import numpy as np

from . import nvstrings as _nvs
from ._lib import lib, check, b
from .wordpiece import vocabulary as wordpiece_vocabulary, tokenize as wordpiece_tokenize, encode as wordpiece_encode  # noqa: F401

__all__ = ["tokenize", "ngrams", "unique_tokens", "token_count", "tokens_counts", "replace_tokens", "normalize_spaces",
           "contains_strings", "strings_counts", "edit_distance", "scatter_count", "porter_stemmer_measure"]
# (wordpiece_vocabulary / wordpiece_tokenize / wordpiece_encode, imported above from wordpiece.py, are not in __all__: that
# list is the reference module's functions, which tests/test_gpu_metadata.py holds against its table of string producers)


def tokenize(strs, delimiter=None):
    """nvtext.py:7-43 -- every token of every row, in row order, as one column.
    delimiter None = whitespace; otherwise ANY character of `delimiter` separates
    (NVText::tokenize, NVText.h:40; tokens.cu:45-50)."""
    out = C.c_void_p()
    if isinstance(delimiter, (list, _nvs.nvstrings)):  # nvtext.py:38-40: several whole-string delimiters
        d = _nvs.to_device(delimiter) if isinstance(delimiter, list) else delimiter
        check(lib.cs_tokenize_multi(strs.m_cptr, d.m_cptr, None, C.byref(out)))
        return _nvs.nvstrings(out.value)
    check(lib.cs_tokenize(strs.m_cptr, b(delimiter), None, C.byref(out)))
    return _nvs.nvstrings(out.value)


def ngrams(tokens, N=2, sep="_"):
    """nvtext.py:290-319 -- n-grams over the whole token column
    (NVText::create_ngrams, NVText.h:153; ngram.cu:32-110)."""
    out = C.c_void_p()
    check(lib.cs_ngrams(tokens.m_cptr, int(N), b(sep), None, C.byref(out)))
    return _nvs.nvstrings(out.value)


def unique_tokens(strs, delimiter=" "):
    """nvtext.py:46-73 -- the sorted distinct tokens of all rows (NVText::unique_tokens, tokens.cu:262-304)."""
    out = C.c_void_p()
    check(lib.cs_unique_tokens(strs.m_cptr, b(delimiter), None, C.byref(out)))
    return _nvs.nvstrings(out.value)


def token_count(strs, delimiter=" ", devptr=0):
    """nvtext.py:76-101 -- tokens per row (0 for a null row)."""
    rows = strs.size()
    if devptr:
        check(lib.cs_token_count(strs.m_cptr, b(delimiter), devptr, 1, None))
        return devptr
    res = np.zeros(max(rows, 1), dtype=np.uint32)
    check(lib.cs_token_count(strs.m_cptr, b(delimiter), res.ctypes.data, 0, None))
    return [int(v) for v in res[:rows]]


def tokens_counts(strs, tgts, delimiter=" ", devptr=0):
    """nvtext.py:162-191 -- per row, how many of its tokens equal each of tgts (a list per row)."""
    if isinstance(tgts, list):
        tgts = _nvs.to_device(tgts)
    rows, tc = strs.size(), tgts.size()
    if devptr:
        check(lib.cs_tokens_counts(strs.m_cptr, tgts.m_cptr, b(delimiter), devptr, 1, None))
        return devptr
    res = np.zeros(max(rows * tc, 1), dtype=np.uint32)
    check(lib.cs_tokens_counts(strs.m_cptr, tgts.m_cptr, b(delimiter), res.ctypes.data, 0, None))
    return [[int(v) for v in res[r * tc : (r + 1) * tc]] for r in range(rows)]


def replace_tokens(strs, tgts, repls, delimiter=None):
    """nvtext.py:194-233 -- every token equal to one of tgts is replaced by the matching repl (or the single one)."""
    if isinstance(repls, str):
        repls = _nvs.to_device([repls])
    if isinstance(repls, list):
        repls = _nvs.to_device(repls)
    if isinstance(tgts, list):
        tgts = _nvs.to_device(tgts)
    out = C.c_void_p()
    check(lib.cs_replace_tokens(strs.m_cptr, tgts.m_cptr, repls.m_cptr, b(delimiter), None, C.byref(out)))
    return _nvs.nvstrings(out.value) if out.value else None


def normalize_spaces(strs):
    """nvtext.py:236-258 -- tokens of each row joined by single spaces."""
    out = C.c_void_p()
    check(lib.cs_normalize_spaces(strs.m_cptr, None, C.byref(out)))
    return _nvs.nvstrings(out.value) if out.value else None


def _targets(tgts, what):
    """pytext.cpp:179-207 -- a list or an nvstrings, not empty"""
    if tgts is None:
        raise ValueError("%s argument must be specified" % what)
    if isinstance(tgts, list):
        tgts = _nvs.to_device(tgts)
    if not isinstance(tgts, _nvs.nvstrings):
        raise ValueError("invalid %s parameter" % what)
    return tgts


def _matrix(fn, dtype, strs, tgts, devptr, item):
    tgts = _targets(tgts, "tgts")
    rows, tc = strs.size(), tgts.size()
    if tc == 0:
        raise ValueError("tgts argument is empty")
    if devptr:
        check(fn(strs.m_cptr, tgts.m_cptr, devptr, 1, None))
        return devptr
    res = np.zeros(max(rows * tc, 1), dtype=dtype)
    check(fn(strs.m_cptr, tgts.m_cptr, res.ctypes.data, 0, None))
    return [[item(v) for v in res[r * tc : (r + 1) * tc]] for r in range(rows)]


def contains_strings(strs, tgts, devptr=0):
    """nvtext.py:104-130 -- per row, whether each of tgts occurs in it (a list of bools per row)."""
    return _matrix(lib.cs_contains_strings, np.uint8, strs, tgts, devptr, bool)


def strings_counts(strs, tgts, devptr=0):
    """nvtext.py:133-159 -- per row, how often each of tgts occurs in it (a list of ints per row)."""
    return _matrix(lib.cs_strings_counts, np.uint32, strs, tgts, devptr, int)


def edit_distance(strs, tgt, algo=0, devptr=0):
    """nvtext.py:261-287 -- the Levenshtein distance of every row to `tgt` (a str), or row by row to a list / nvstrings
    of the same size; algo 0 is the only one."""
    if tgt is None:
        raise ValueError("tgt argument must be specified")
    if algo not in (0, None):
        raise ValueError("unrecognized edit-distance algorithm")
    rows = strs.size()
    res = None if devptr else np.zeros(max(rows, 1), dtype=np.uint32)
    out = devptr if devptr else res.ctypes.data
    if isinstance(tgt, str):
        check(lib.cs_edit_distance(strs.m_cptr, b(tgt), 0, out, 1 if devptr else 0, None))
    else:
        tgts = _targets(tgt, "tgt")
        if tgts.size() != rows:
            raise ValueError("strs and tgt must have the same number of strings")
        check(lib.cs_edit_distance_column(strs.m_cptr, tgts.m_cptr, 0, out, 1 if devptr else 0, None))
    return None if devptr else [int(v) for v in res[:rows]]


def porter_stemmer_measure(strs, vowels="aeiou", y_char="y", devptr=0):
    """NVText::porter_stemmer_measure (NVText.h:164; the reference's Python module has no such function) -- the
    vowel-run -> consonant transitions of every row; 0 for a null row."""
    rows = strs.size()
    if devptr:
        check(lib.cs_porter_stemmer_measure(strs.m_cptr, b(vowels), b(y_char), devptr, 1, None))
        return devptr
    res = np.zeros(max(rows, 1), dtype=np.uint32)
    check(lib.cs_porter_stemmer_measure(strs.m_cptr, b(vowels), b(y_char), res.ctypes.data, 0, None))
    return [int(v) for v in res[:rows]]


def scatter_count(strs, counts):
    """nvtext.py:322-346 -- row i repeated counts[i] times (a list, None = 0, or a device pointer to uint32 values)."""
    out = C.c_void_p()
    if isinstance(counts, int):
        check(lib.cs_scatter_count(strs.m_cptr, counts, 1, None, C.byref(out)))
    else:
        vals = np.array([0 if c is None else int(c) for c in counts], dtype=np.uint32)
        if len(vals) != strs.size():
            raise ValueError("counts must have one entry per string")
        check(lib.cs_scatter_count(strs.m_cptr, vals.ctypes.data if len(vals) else None, 0, None, C.byref(out)))
    return _nvs.nvstrings(out.value) if out.value else None
