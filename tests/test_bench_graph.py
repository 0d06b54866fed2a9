"""CPU tests of bench.py's graph source: a plain run generates its graph, a --full run shares one copy with its
child processes."""
import os

import numpy as np

from bench import GRAPH_DIR_ENV, load_host


def _same_csr(a, b):
    return a.n == b.n and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("out_rp", "out_ci", "in_rp", "in_ci"))


def test_load_host_without_a_graph_dir_generates_the_graph(monkeypatch, pkg_product):
    monkeypatch.delenv(GRAPH_DIR_ENV, raising=False)
    saved = []
    monkeypatch.setattr(np, "savez", lambda *a, **k: saved.append(a))
    assert _same_csr(load_host(pkg_product, 10), pkg_product.HostCsr.rmat(10, 16, seed=1))
    assert not saved


def test_load_host_shares_one_copy_through_the_graph_dir(monkeypatch, tmp_path, pkg_product):
    monkeypatch.setenv(GRAPH_DIR_ENV, str(tmp_path))
    first = load_host(pkg_product, 10)
    assert os.listdir(tmp_path) == ["rmat10_seed1.npz"]

    def no_generation(*a, **k):
        raise AssertionError("the graph was generated again")

    monkeypatch.setattr(pkg_product.HostCsr, "rmat", no_generation)
    assert _same_csr(load_host(pkg_product, 10), first)
