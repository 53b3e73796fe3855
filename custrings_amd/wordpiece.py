"""`wordpiece` -- a column of text to the integer ids of a vocabulary, on the device: the BERT family's sub-word tokenizer
(cs_wordpiece_*).  The definition is custrings_amd/csrc/wordpiece_ops.h.

    vocab = wordpiece.vocabulary(nvstrings.to_device(tokens))            # row index = id; owns the device table
    ids, offsets = wordpiece.tokenize(strs.lower(), vocab)               # row r: ids[offsets[r]:offsets[r + 1]]
    ids, mask = wordpiece.encode(strs.lower(), vocab, 128, cls="[CLS]", sep="[SEP]", pad="[PAD]", punct=True)

Lower-casing and accent stripping are not part of it: chain lower() in front.
"""
import ctypes as C

import numpy as np

from ._lib import lib, check, b

__all__ = ["Vocabulary", "vocabulary", "tokenize", "encode"]


def _address(devptr):
    return devptr.data_ptr() if hasattr(devptr, "data_ptr") else int(devptr)


class Vocabulary:
    """The device hash table of a vocabulary column (cs_wordpiece_vocab); freed with the object."""

    def __init__(self, strs, prefix="##", unk="[UNK]"):
        self.m_cptr = None
        handle = C.c_void_p()
        check(lib.cs_wordpiece_vocab_create(strs.m_cptr, b(prefix), b(unk), None, C.byref(handle)))
        self.m_cptr = handle.value
        entries, unk_id, longest = C.c_int64(), C.c_int(), C.c_int()
        check(lib.cs_wordpiece_vocab_info(self.m_cptr, C.byref(entries), C.byref(unk_id), C.byref(longest)))
        self.entries, self.unk_id, self.max_entry_bytes = entries.value, unk_id.value, longest.value
        self.prefix, self.unk = prefix, unk

    def __del__(self):
        if getattr(self, "m_cptr", None):
            lib.cs_wordpiece_vocab_destroy(self.m_cptr)
            self.m_cptr = None

    def id_of(self, token):
        """the id of the entry `token` (a str or bytes), None when it is none"""
        text = b(token)
        found = C.c_int()
        check(lib.cs_wordpiece_vocab_find(self.m_cptr, text, len(text), C.byref(found), None))
        return found.value if found.value >= 0 else None

    def _special(self, token, what):
        """an id as it is, a token through the vocabulary, None as -1"""
        if token is None:
            return -1
        if isinstance(token, (str, bytes)):
            found = self.id_of(token)
            if found is None:
                raise ValueError("wordpiece: the %s token %r is no entry of the vocabulary" % (what, token))
            return found
        if int(token) < 0:
            raise ValueError("wordpiece: the %s id is negative" % what)
        return int(token)


def vocabulary(strs, prefix="##", unk="[UNK]"):
    """The vocabulary of the column `strs`: the row index is the id, null and empty rows are no entry, the lowest of equal
    rows wins.  `unk` must be an entry."""
    return Vocabulary(strs, prefix, unk)


def tokenize(strs, vocab, max_word_chars=100, punct=False, devptrs=None):
    """(ids int32[total], offsets int64[rows + 1]) as numpy arrays: row r's ids are ids[offsets[r]:offsets[r + 1]].  With
    `devptrs` = (ids, offsets), addresses or tensors in device memory (offsets: rows + 1 int64; ids: int32, room for every
    id -- a tensor says how many it holds, an address is trusted), both are written there and (total, offsets) is returned;
    more ids than a tensor holds is a ValueError and `ids` is left alone."""
    rows, total = strs.size(), C.c_int64()
    args = (strs.m_cptr, vocab.m_cptr, int(max_word_chars), 1 if punct else 0)
    if devptrs is not None:
        d_ids, d_offsets = devptrs
        check(lib.cs_wordpiece_count(*args, _address(d_offsets), 1, None, C.byref(total)))
        if hasattr(d_ids, "numel") and d_ids.numel() < total.value:
            raise ValueError("wordpiece: %d ids do not fit the tensor's %d" % (total.value, d_ids.numel()))
        check(lib.cs_wordpiece_ids(*args, _address(d_offsets), _address(d_ids) if total.value else None, 1, None))
        return total.value, d_offsets
    offsets = np.zeros(rows + 1, dtype=np.int64)
    check(lib.cs_wordpiece_count(*args, offsets.ctypes.data, 0, None, C.byref(total)))
    ids = np.empty(total.value, dtype=np.int32)
    check(lib.cs_wordpiece_ids(*args, offsets.ctypes.data, ids.ctypes.data if total.value else None, 0, None))
    return ids, offsets


def encode(strs, vocab, max_length, cls=None, sep=None, pad=None, max_word_chars=100, punct=False, devptrs=None):
    """(ids int32[rows, max_length], mask uint8[rows, max_length]) as numpy arrays: per row cls, the row's ids cut to what
    fits, sep, then pad; mask 1 on all but the padding.  cls / sep / pad are token strings (looked up in the vocabulary),
    ids, or None (no cls, no sep; pad None = id 0).  With `devptrs` = (ids, mask), addresses or tensors in device memory
    (mask may be None), they are written there and returned."""
    rows, length = strs.size(), int(max_length)
    cls_id, sep_id = vocab._special(cls, "cls"), vocab._special(sep, "sep")
    pad_id = 0 if pad is None else vocab._special(pad, "pad")
    args = (strs.m_cptr, vocab.m_cptr, int(max_word_chars), 1 if punct else 0, length, cls_id, sep_id, pad_id)
    if devptrs is not None:
        d_ids, d_mask = devptrs
        check(lib.cs_wordpiece_encode(*args, _address(d_ids), None if d_mask is None else _address(d_mask), 1, None))
        return d_ids, d_mask
    ids = np.empty((rows, max(length, 0)), dtype=np.int32)
    mask = np.empty((rows, max(length, 0)), dtype=np.uint8)
    check(lib.cs_wordpiece_encode(*args, ids.ctypes.data if rows else None, mask.ctypes.data if rows else None, 0, None))
    return ids, mask
