"""`minhash` -- near-duplicate detection over a strings column: MinHash signatures (cs_minhash) and LSH band keys
(cs_minhash_bands).  The definition is custrings_amd/csrc/minhash_ops.h.

    sig = minhash.minhash(strs, width=5, nperm=128)          # rows x 128 uint32
    keys = minhash.band_keys(sig, bands=32)                  # rows x 32 int64
    cat = nvcategory.from_numbers(keys.reshape(-1))          # rows that share a key are candidates
    minhash.jaccard_estimate(sig, i, j)                      # the estimate of two rows' n-gram set similarity
"""
import numpy as np

from . import _lib
from ._lib import lib, check

__all__ = ["permutations", "minhash", "band_keys", "jaccard_estimate"]

_MASK64 = (1 << 64) - 1


def _splitmix64(state):
    """the splitmix64 sequence from `state`: a generator of 64-bit values"""
    while True:
        state = (state + 0x9E3779B97F4A7C15) & _MASK64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
        yield z ^ (z >> 31)


def permutations(nperm, seed=0):
    """(a, b): the multipliers (odd, so never 0) and addends of `nperm` permutations, uint32 arrays; the same for the same
    seed everywhere: a[i] = (next() >> 32) | 1, b[i] = next() >> 32 over splitmix64 started at `seed`."""
    nxt = _splitmix64(int(seed) & _MASK64)
    a = np.empty(int(nperm), dtype=np.uint32)
    b_ = np.empty(int(nperm), dtype=np.uint32)
    for i in range(int(nperm)):
        a[i] = (next(nxt) >> 32) | 1
        b_[i] = next(nxt) >> 32
    return a, b_


def _address(devptr):
    return devptr.data_ptr() if hasattr(devptr, "data_ptr") else int(devptr)


def minhash(strs, width=5, seed=0, a=None, b=None, nperm=128, devptr=0):
    """The rows x nperm uint32 signatures of `strs` over its n-grams of `width` characters.  Without `a` / `b` the
    permutations are permutations(nperm, seed).  With `devptr` (an address or a tensor in device memory, rows x nperm
    uint32) the signatures are written there and `devptr` is returned."""
    if (a is None) != (b is None):
        raise ValueError("minhash: a and b go together")
    if a is None:
        if int(nperm) < 1:
            raise ValueError("minhash: nperm must be 1 at least")
        a, b = permutations(nperm, seed)
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    if a.ndim != 1 or a.shape != b.shape:
        raise ValueError("minhash: a and b must be one-dimensional and of one length")
    n, rows = int(a.size), strs.size()
    if hasattr(devptr, "data_ptr") or devptr:
        check(lib.cs_minhash(strs.m_cptr, int(width), int(seed) & 0xFFFFFFFF, a.ctypes.data, b.ctypes.data, n, _address(devptr), 1, None))
        return devptr
    res = np.empty((rows, n), dtype=np.uint32)
    check(lib.cs_minhash(strs.m_cptr, int(width), int(seed) & 0xFFFFFFFF, a.ctypes.data, b.ctypes.data, n, res.ctypes.data if rows else None, 0, None))
    return res


def band_keys(signatures, bands, devptr=0):
    """rows x bands int64 keys of rows x nperm signatures (a numpy array, or a tensor in device memory): key j of a row is
    j << 32 | a hash of its band j.  A device tensor needs `devptr` (rows x bands int64 in device memory), which is
    returned; a numpy array gives a numpy array.  keys.reshape(-1) goes straight into nvcategory.from_numbers."""
    if signatures.ndim != 2:
        raise ValueError("band_keys: signatures are rows x nperm")
    rows, nperm = int(signatures.shape[0]), int(signatures.shape[1])
    _lib.ensure_init()
    if hasattr(signatures, "data_ptr"):
        if not signatures.is_contiguous() or signatures.element_size() != 4:
            raise ValueError("band_keys: a contiguous tensor of 32-bit values")
        if not hasattr(devptr, "data_ptr") and not devptr:
            raise ValueError("band_keys: signatures in device memory need devptr")
        check(lib.cs_minhash_bands(signatures.data_ptr(), rows, nperm, int(bands), _address(devptr), 1, None))
        return devptr
    sig = np.ascontiguousarray(signatures, dtype=np.uint32)
    keys = np.empty((rows, max(int(bands), 0)), dtype=np.int64)
    check(lib.cs_minhash_bands(sig.ctypes.data if rows else None, rows, nperm, int(bands), keys.ctypes.data if rows else None, 0, None))
    return keys


def jaccard_estimate(sig, i, j):
    """the share of positions at which rows i and j of the signatures agree: the MinHash estimate of the Jaccard similarity
    of their n-gram sets (numpy, on the host)"""
    sig = np.asarray(sig)
    return float(np.count_nonzero(sig[i] == sig[j])) / sig.shape[1]
