"""The numpy statement of the sparse form of a vector (include/pprhip.h "sparse results"): the entries with
x(v) > threshold as (id, value) pairs, by id ascending or by value descending with ties by id ascending; the CSR over many
vectors; the cap truncation.  The GPU tests compare the engine against these on the dense vector the same handle returns."""
import numpy as np

BY_ID, BY_VALUE = 0, 1


def sparse_ref(x, threshold=0.0, order=BY_ID):
    """(ids int32, vals float64) of the kept entries in the chosen order; the values are x's own."""
    x = np.asarray(x, dtype=np.float64)
    ids = np.flatnonzero(x > threshold)
    vals = x[ids]
    if order == BY_VALUE:
        p = np.lexsort((ids, -vals))      # last key first: value descending, then id ascending
        ids, vals = ids[p], vals[p]
    return ids.astype(np.int32), vals


def sparse_ref_all(rows, threshold=0.0, order=BY_ID):
    """(offsets uint64[len(rows) + 1], ids, vals) of the rows' sparse forms, one behind the other."""
    parts = [sparse_ref(x, threshold, order) for x in rows]
    offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        offsets[1:] = np.cumsum([p[0].size for p in parts])
        return offsets, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return offsets, np.empty(0, dtype=np.int32), np.empty(0)


def truncate(ids, vals, cap):
    """What a call with `cap` writes: the first min(cap, count) entries; the count stays the whole."""
    k = min(int(cap), ids.size)
    return ids[:k], vals[:k], ids.size


def same_bits(a, b):
    """float64 arrays equal bit for bit (0.0 and -0.0 differ, NaNs compare by payload)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
