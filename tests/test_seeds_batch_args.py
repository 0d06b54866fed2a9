"""Batched seed sets without a device: the C symbols, and how the binding packs q seed sets into the CSR-like arrays the
batched calls take (_seed_set_arrays).  The GPU half is tests/test_gpu_seeds_batch.py."""
import numpy as np
import pytest

BATCH_SEED_SYMBOLS = ["pprhip_fora_batch_seeds", "pprhip_fora_batch_topk_seeds"]


def test_symbols_exported_and_bound(pkg):
    L = pkg.lib()
    for s in BATCH_SEED_SYMBOLS:
        assert s in pkg.EXPORTS and hasattr(L, s), s
        assert getattr(L, s).argtypes, s
    assert hasattr(pkg.Graph, "fora_batch_seeds") and hasattr(pkg.Graph, "fora_batch_topk_seeds")


def test_offsets_dtypes_and_slices(pkg):
    sets = [[3, 1], np.array([7], dtype=np.int64), (0, 2, 2, 5)]
    s, w, off = pkg._seed_set_arrays(sets, None)
    assert s.dtype == np.int32 and s.flags["C_CONTIGUOUS"]
    assert off.dtype == np.uint64 and list(off) == [0, 2, 3, 7]
    assert w is None
    assert list(s) == [3, 1, 7, 0, 2, 2, 5]
    for i, x in enumerate(sets):
        assert list(s[int(off[i]):int(off[i + 1])]) == list(np.asarray(x))


def test_weights_per_set_with_uniform_fill(pkg):
    sets = [[3, 1], [7], [0, 2, 5]]
    s, w, off = pkg._seed_set_arrays(sets, [[0.5, 2.0], None, np.array([1, 2, 3], dtype=np.int32)])
    assert w.dtype == np.float64 and w.flags["C_CONTIGUOUS"] and w.size == s.size
    assert list(w) == [0.5, 2.0, 1.0, 1.0, 2.0, 3.0]
    _, w2, _ = pkg._seed_set_arrays(sets, [None, None, None])
    assert list(w2) == [1.0] * 6


def test_length_mismatches_raise(pkg):
    with pytest.raises(ValueError):
        pkg._seed_set_arrays([[1, 2], [3]], [[1.0, 1.0]])  # one weight entry for two sets
    with pytest.raises(ValueError):
        pkg._seed_set_arrays([[1, 2], [3]], [[1.0], None])  # set 0: one weight for two seeds
    with pytest.raises(ValueError):
        pkg._seed_set_arrays([[1]], [[1.0, 2.0]])


def test_empty_list_and_empty_sets(pkg):
    s, w, off = pkg._seed_set_arrays([], None)
    assert list(off) == [0] and s.size == 0 and s.dtype == np.int32 and w is None
    s, w, off = pkg._seed_set_arrays([], [])
    assert list(off) == [0] and w.size == 0
    s, _, off = pkg._seed_set_arrays([[4], [], [5, 6]], None)  # an empty set packs (the C call rejects it)
    assert list(off) == [0, 1, 1, 3] and list(s) == [4, 5, 6]
