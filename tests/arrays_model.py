"""A plain model of the array, combine, record and partition ops (cs_array.hip, cs_records.hip) over Python lists.

A column is a list of `bytes` (a row) or `None` (a null row).  Each function states what the op returns, from the op's
description in NVStrings.h (gather, scatter, sublist, sort / order, cat, join, partition, the *_record forms) -- no scans, no
offsets, no kernels.  split_record / rsplit_record are not here: their reference restatement is the oracle
(oracle/oracle_round2.inc) and is not said a third time.

Record results are (flat column in row-major order, rows + 1 list offsets): record r is flat[list[r]:list[r + 1]].
"""

CAT_MAX_COLUMNS = 16  # the library's own bound on cat: this column and 15 others (the reference has none)


def gather(rows, pos):
    """The rows at `pos`, in that order.  A position outside [0, rows) is an IndexError; an empty column or an empty list
    gives an empty column without looking at the positions."""
    if not rows or not pos:
        return []
    for p in pos:
        if not 0 <= p < len(rows):
            raise IndexError("gather position %d outside [0, %d)" % (p, len(rows)))
    return [rows[p] for p in pos]


def gather_mask(rows, mask):
    """The rows whose mask entry is true."""
    assert len(mask) == len(rows)
    return [r for r, m in zip(rows, mask) if m]


def remove_strings(rows, pos):
    """The rows NOT named by `pos`; positions outside the column name nothing."""
    gone = set(pos)
    return [r for i, r in enumerate(rows) if i not in gone]


def sublist(rows, start, end, step):
    """Rows start, start + step, ... before `end` (after it, for a negative step).  start and end are clamped into
    [0, rows]; step 0 is step 1; a range that runs the wrong way is empty.  With a negative step `start` itself is the first
    row taken, so start == rows is a position outside the column."""
    count = len(rows)
    start = min(max(start, 0), count)
    end = min(max(end, 0), count)
    step = step or 1
    if start == end or (step > 0 and start > end) or (step < 0 and start < end):
        return []
    return gather(rows, list(range(start, end, step)))


def scatter(rows, src, pos):
    """A copy of `rows` with row pos[j] replaced by src[j] (a null src row makes a null row).  Positions outside the
    column are ignored; of several entries naming one row the last in list order wins."""
    assert len(src) == len(pos)
    out = list(rows)
    for j, p in enumerate(pos):
        if 0 <= p < len(out):
            out[p] = src[j]
    return out


def scalar_scatter(rows, scalar, pos):
    """A copy of `rows` with the rows at `pos` replaced by `scalar` (None: null rows)."""
    return scatter(rows, [scalar] * len(pos), pos)


def cat(cols, sep, narep):
    """Row-wise concatenation of the columns, `sep` between neighbours.  A null element is replaced by `narep`; without a
    `narep` it makes the whole row null.  Columns of different row counts are a ValueError."""
    if any(len(c) != len(cols[0]) for c in cols):
        raise ValueError("cat: sizes do not match")
    out = []
    for parts in zip(*cols):
        if narep is None and any(p is None for p in parts):
            out.append(None)
        else:
            out.append((sep or b"").join(narep if p is None else p for p in parts))
    return out


def join(rows, sep, narep):
    """All rows as ONE string.  A null row stands as `narep`, or without one is left out together with the separator that
    would follow it.  The separator follows every other row but the column's last -- so a column that ends in left-out
    rows ends in a separator (combine.cu:293-420 writes the separator with the row before it knows what follows)."""
    out = b""
    for r, row in enumerate(rows):
        if row is None and narep is None:
            continue
        out += narep if row is None else row
        if r + 1 < len(rows):
            out += sep
    return [out]


def order(rows, stype, asc, nullfirst):
    """Row indexes in sorted order: by byte length (stype & 1), then by bytes (stype & 2); nulls first or last whatever the
    direction; equal rows keep their index order (a stable sort -- one of the orders the reference's sort may give)."""
    null_class = 0 if nullfirst == asc else 1

    def key(i):
        if rows[i] is None:
            return (null_class, 0, b"")
        return (1 - null_class, len(rows[i]) if stype & 1 else 0, rows[i] if stype & 2 else b"")

    return sorted(range(len(rows)), key=key, reverse=not asc)


def sort(rows, stype, asc, nullfirst):
    return [rows[i] for i in order(rows, stype, asc, nullfirst)]


def records(cols, ragged):
    """Column-major -> row-major.  Fixed form: record r is row r of every column, nulls kept.  Ragged form: record r is
    row r of the leading columns up to, not including, the first in which row r is null."""
    if any(len(c) != len(cols[0]) for c in cols):
        raise ValueError("records: columns of different row counts")
    flat, lst = [], [0]
    for r in range(len(cols[0]) if cols else 0):
        for c in cols:
            if ragged and c[r] is None:
                break
            flat.append(c[r])
        lst.append(len(flat))
    return flat, lst


def partition(rows, delim, from_right):
    """Three strings per row -- head, delimiter, tail -- around the first (last, from the right) occurrence of `delim`;
    without one the whole row comes first (last, from the right) and the other two are empty.  A null row gives three
    nulls.  Without a delimiter there is no result at all (None)."""
    if not delim:
        return None
    flat = []
    for row in rows:
        if row is None:
            flat += [None, None, None]
        else:
            flat += list(row.rpartition(delim) if from_right else row.partition(delim))
    return flat, list(range(0, 3 * len(rows) + 1, 3))


def metadata(rows):
    """(size, null_count, byte_count total) of a column"""
    return len(rows), sum(r is None for r in rows), sum(len(r) for r in rows if r is not None)
