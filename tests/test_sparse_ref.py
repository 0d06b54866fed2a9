"""The reference of the sparse results (tests/sparse_ref.py) on hand-made vectors."""
import numpy as np

from sparse_ref import BY_ID, BY_VALUE, same_bits, sparse_ref, sparse_ref_all, truncate


def test_by_id_is_flatnonzero_over_the_threshold():
    x = np.array([0.0, 0.5, 0.0, 0.25, 1e-300, 0.5])
    ids, vals = sparse_ref(x)
    assert ids.dtype == np.int32 and vals.dtype == np.float64
    assert list(ids) == [1, 3, 4, 5] and same_bits(vals, x[[1, 3, 4, 5]])
    ids, vals = sparse_ref(x, 0.25)            # strict: the entry equal to the threshold drops out
    assert list(ids) == [1, 5]


def test_by_value_breaks_ties_by_id():
    x = np.array([0.1, 0.3, 0.1, 0.3, 0.2, 0.3, 0.0])
    ids, vals = sparse_ref(x, 0.0, BY_VALUE)
    assert list(ids) == [1, 3, 5, 4, 0, 2]
    assert list(vals) == [0.3, 0.3, 0.3, 0.2, 0.1, 0.1]
    ids, _ = sparse_ref(np.full(7, 0.125), 0.0, BY_VALUE)    # all tie: id order
    assert list(ids) == list(range(7))


def test_empty_results():
    for order in (BY_ID, BY_VALUE):
        for x, thr in ((np.zeros(5), 0.0), (np.array([0.5, 0.25]), 1.0), (np.empty(0), 0.0)):
            ids, vals = sparse_ref(x, thr, order)
            assert ids.size == 0 and vals.size == 0 and ids.dtype == np.int32


def test_threshold_equal_to_the_maximum_keeps_nothing():
    x = np.array([0.125, 0.75, 0.5, 0.75])
    for order in (BY_ID, BY_VALUE):
        assert sparse_ref(x, x.max(), order)[0].size == 0
        assert list(sparse_ref(x, np.nextafter(x.max(), 0.0), order)[0]) == [1, 3]


def test_negative_zero_and_nan_are_never_kept():
    x = np.array([-0.0, 0.0, np.nan, 2.0 ** -1074, -1.0])
    with np.errstate(invalid="ignore"):
        ids, vals = sparse_ref(x)
    assert list(ids) == [3] and same_bits(vals, [2.0 ** -1074])
    assert not same_bits([0.0], [-0.0]) and same_bits([-0.0], [-0.0])


def test_csr_concatenation_and_offsets():
    rows = [np.array([0.0, 0.5, 0.25]), np.zeros(3), np.array([0.125, 0.0, 0.125])]
    offs, ids, vals = sparse_ref_all(rows)
    assert offs.dtype == np.uint64 and list(offs) == [0, 2, 2, 4]
    assert list(ids) == [1, 2, 0, 2] and list(vals) == [0.5, 0.25, 0.125, 0.125]
    offs, ids, vals = sparse_ref_all(rows, 0.125, BY_VALUE)
    assert list(offs) == [0, 2, 2, 2] and list(ids) == [1, 2]
    offs, ids, vals = sparse_ref_all([])
    assert list(offs) == [0] and ids.size == 0 and vals.size == 0


def test_truncation_keeps_the_count():
    ids, vals = sparse_ref(np.array([0.1, 0.4, 0.2, 0.3]), 0.0, BY_VALUE)
    for cap, want in ((0, []), (1, [1]), (3, [1, 3, 2]), (4, [1, 3, 2, 0]), (9, [1, 3, 2, 0])):
        i, v, count = truncate(ids, vals, cap)
        assert list(i) == want and v.size == len(want) and count == 4
