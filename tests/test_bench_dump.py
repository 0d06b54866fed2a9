"""CPU test of bench.py's --dump-outputs writer: float64 .npy files, the byte cap, the fixed node sample."""
import os

import numpy as np
import pytest

from bench import DUMP_BYTES, dump_outputs


class _FakeStore:
    """Stands in for pkg.Results: slot i holds a vector whose entries encode (i, node)."""

    def __init__(self, q, n):
        self.q, self.n = q, n

    def fetch(self, i):
        return i + np.arange(self.n) / self.n

    def sum(self, i):
        return float(self.fetch(i).sum())


def _last(q, k=4):
    ids = np.arange(q * k, dtype=np.int32).reshape(q, k)
    return {"step": 9, "ids": ids, "vals": ids / 100.0, "nsel": np.full(q, k, dtype=np.int32)}


def test_dump_outputs_small_graph_writes_whole_vectors(tmp_path):
    q, n = 3, 50
    srcs = np.array([4, 7, 11], dtype=np.int32)
    info = dump_outputs(str(tmp_path / "d"), srcs, _last(q), _FakeStore(q, n), n)
    names = {"sources", "topk_ids", "topk_vals", "topk_count", "vector_sample_nodes", "vector_sample", "vector_mass"}
    assert set(info["files"]) == {x + ".npy" for x in names} and info["step"] == 9
    for x in names:
        a = np.load(os.path.join(info["dir"], x + ".npy"))
        assert a.dtype == np.float64, x
    assert np.array_equal(np.load(tmp_path / "d" / "sources.npy"), srcs)
    assert np.array_equal(np.load(tmp_path / "d" / "topk_ids.npy"), _last(q)["ids"])
    assert np.array_equal(np.load(tmp_path / "d" / "vector_sample_nodes.npy"), np.arange(n))
    vs = np.load(tmp_path / "d" / "vector_sample.npy")
    assert vs.shape == (q, n) and np.array_equal(vs[2], _FakeStore(q, n).fetch(2))
    last = _last(q)
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "topk_vals.npy"), last["vals"])
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "topk_count.npy"), last["nsel"])
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "vector_mass.npy"),
                                  [_FakeStore(q, n).sum(i) for i in range(q)])


def test_dump_outputs_large_graph_is_a_fixed_sample_under_the_cap(tmp_path):
    q, n = 64, 1 << 20
    store = _FakeStore(q, n)
    a = dump_outputs(str(tmp_path / "a"), np.zeros(q, dtype=np.int32), _last(q), store, n)
    b = dump_outputs(str(tmp_path / "b"), np.zeros(q, dtype=np.int32), _last(q), store, n)
    sizes = sum(os.path.getsize(os.path.join(a["dir"], f)) for f in a["files"])
    assert a["bytes"] == sizes <= DUMP_BYTES
    nodes = np.load(tmp_path / "a" / "vector_sample_nodes.npy")
    assert nodes.size < n and np.all(np.diff(nodes) > 0) and nodes[-1] < n
    assert np.array_equal(nodes, np.load(tmp_path / "b" / "vector_sample_nodes.npy"))
    vs = np.load(tmp_path / "a" / "vector_sample.npy")
    assert np.array_equal(vs[5], store.fetch(5)[nodes.astype(np.int64)])


def test_dump_outputs_without_store_writes_the_topk_blocks(tmp_path):
    q = 2
    info = dump_outputs(str(tmp_path), np.array([1, 2], dtype=np.int32), _last(q), None, 10)
    assert set(info["files"]) == {"sources.npy", "topk_ids.npy", "topk_vals.npy", "topk_count.npy"}


@pytest.mark.parametrize("q", [1, 2, 3, 128])
def test_dump_outputs_cap_holds_for_any_batch_size(tmp_path, q):
    """The 64 MB covers every file, the node list of the sample included, also when a step has one to three queries."""
    n = 1 << 22  # bench.py's default graph (scale 22)
    info = dump_outputs(str(tmp_path), np.arange(q, dtype=np.int32), _last(q), _FakeStore(q, n), n)
    sizes = sum(os.path.getsize(os.path.join(info["dir"], f)) for f in info["files"])
    assert info["bytes"] == sizes <= DUMP_BYTES
    assert sizes > DUMP_BYTES - (64 << 10) * (q + 1)  # (the sample uses what the cap leaves)


def test_dump_outputs_writes_the_gathered_blocks(tmp_path):
    q, world, k = 3, 2, 4
    gi = np.arange(world * q * k, dtype=np.int32).reshape(world, q, k)
    info = dump_outputs(str(tmp_path), np.arange(q, dtype=np.int32), _last(q, k), _FakeStore(q, 20), 20,
                        gathered={"ids": gi, "vals": gi / 7.0})
    assert {"gathered_topk_ids.npy", "gathered_topk_vals.npy"} <= set(info["files"])
    np.testing.assert_array_equal(np.load(tmp_path / "gathered_topk_ids.npy"), gi)
    np.testing.assert_array_equal(np.load(tmp_path / "gathered_topk_vals.npy"), gi / 7.0)
