"""The sweep cut without a device: the numpy reference of tests/sweep_ref.py against closed forms and brute force (the GPU
tests compare the engine with it bit for bit), and the argument checks of the three entry points, which run before the
handle is looked at (include/pprhip.h "local clustering", "Parameter ranges")."""
import ctypes as C

import numpy as np
import pytest

from sweep_ref import cut_of, degrees, edges_of, sweep_ref


def barbell_edges():
    """Triangles {0, 1, 2} and {3, 4, 5} joined by the bridge 2 - 3, every undirected edge as two relationships."""
    und = [(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3)]
    e = und + [(b, a) for a, b in und]
    return np.array([a for a, _ in e], dtype=np.int64), np.array([b for _, b in e], dtype=np.int64)


BARBELL_X = np.array([0.30, 0.25, 0.20, 0.10, 0.05, 0.04])  # x / deg ranks 0, 1, 2, 3, 4, 5


def test_barbell_closed_form():
    src, dst = barbell_edges()
    assert src.size == 14
    r = sweep_ref(6, src, dst, BARBELL_X)
    assert list(r["order"]) == [0, 1, 2, 3, 4, 5] and r["support"] == r["profiled"] == 6 and r["total_vol"] == 28
    assert list(r["vol"][:3]) == [4, 8, 14] and r["cut"][2] == 2
    assert (r["best_size"], r["best_cut"], r["best_vol"]) == (3, 2, 14) and r["best_conductance"] == 2.0 / 14.0
    assert (r["cut"][3], r["vol"][3]) == (4, 20) and 4.0 / 8.0 == float(r["cut"][3]) / min(20, 28 - 20)
    # the last prefix covers every edge-bearing node: denominator 0, not a candidate
    assert r["vol"][5] == 28 and r["cut"][5] == 0 and r["best_size"] != 6
    one = sweep_ref(6, src, dst, BARBELL_X, max_size=1)
    assert one["profiled"] == 1 and one["support"] == 6 and one["best_size"] == 1 and one["best_cut"] == 4 and one["best_conductance"] == 1.0
    small = sweep_ref(6, src, dst, BARBELL_X, max_vol=8)
    assert small["profiled"] == 6 and small["best_size"] == 2 and small["best_cut"] == 4 and small["best_conductance"] == 0.5
    none = sweep_ref(6, src, dst, BARBELL_X, max_vol=3)
    assert none["best_size"] == 0 and none["best_conductance"] == float("inf")


def test_raw_scores_and_ties():
    src, dst = barbell_edges()
    x = np.array([0.1, 0.1, 0.3, 0.3, 0.0, 0.2])
    r = sweep_ref(6, src, dst, x, normalize=0)
    assert list(r["order"]) == [2, 3, 5, 0, 1] and r["support"] == 5   # ties by id, x = 0 is not ranked
    for i in range(r["profiled"]):
        assert r["cut"][i] == cut_of(6, src, dst, r["order"][:i + 1])


def test_loops_multi_edges_and_isolated_nodes(toy_graphs):
    host = toy_graphs["isolated_mix"]
    src, dst = edges_of(host)
    assert list(degrees(host.n, src, dst)) == [4, 3, 4, 1, 0, 0]       # the self loop of 0 adds 2, 1 -> 2 counts twice
    x = np.array([0.2, 0.3, 0.1, 0.05, 0.2, 0.0])
    for normalize in (0, 1):
        r = sweep_ref(host.n, src, dst, x, normalize=normalize)
        assert r["support"] == 4 and 4 not in r["order"]               # an isolated node is never ranked
        assert list(r["vol"]) == list(np.cumsum(degrees(host.n, src, dst)[r["order"]]))
        for i in range(r["profiled"]):
            assert r["cut"][i] == cut_of(host.n, src, dst, r["order"][:i + 1])
        assert r["vol"][-1] == 12 == r["total_vol"] and r["best_size"] < 4
    assert sweep_ref(host.n, src, dst, np.zeros(6))["support"] == 0


def test_reference_against_brute_force_on_random_graphs():
    rng = np.random.default_rng(11)
    for n, m in ((9, 30), (40, 90), (64, 400)):
        src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
        x = rng.random(n) * (rng.random(n) < 0.7)
        x[rng.integers(0, n, 3)] = 0.125                                # a few exact ties
        r = sweep_ref(n, src, dst, x)
        phis = []
        for i in range(r["profiled"]):
            c = cut_of(n, src, dst, r["order"][:i + 1])
            assert r["cut"][i] == c
            den = min(int(r["vol"][i]), 2 * m - int(r["vol"][i]))
            phis.append(c / den if den > 0 else float("inf"))
        if r["profiled"] and min(phis) < float("inf"):
            assert r["best_size"] == int(np.argmin(phis)) + 1 and r["best_conductance"] == min(phis)


def test_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for s in ("pprhip_sweep_cut", "pprhip_results_sweep_cut", "pprhip_local_cluster_seeds"):
        assert s in pkg.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    assert pkg.Graph.RELEASE_SWEEP == 8
    assert C.sizeof(pkg.Sweep) == 11 * 8 and set(pkg.Sweep().as_dict()) == {k for k, _ in pkg.Sweep._fields_}


def test_arguments_are_checked_before_the_handle(pkg):
    """normalize outside {0, 1}, a null info and a buffer with cap == 0 are refused without a device: the message
    names the argument, not the (null) handle."""
    L = pkg.lib()
    info = pkg.Sweep()
    buf = np.zeros(4, dtype=np.int32)
    seeds = np.zeros(1, dtype=np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    sp = seeds.ctypes.data_as(C.c_void_p)

    def refused(rc, what):
        assert rc == pkg.ERR_INVALID
        assert what in L.pprhip_last_error().decode(), L.pprhip_last_error().decode()

    for bad in (2, -1):
        refused(L.pprhip_sweep_cut(None, bad, 0, 0, None, None, None, 0, C.byref(info)), "normalize")
        refused(L.pprhip_results_sweep_cut(None, 0, bad, 0, 0, None, None, None, 0, C.byref(info)), "normalize")
        refused(L.pprhip_local_cluster_seeds(None, sp, None, 1, 0.15, 1e-4, bad, 0, 0, None, 0, C.byref(info), None),
                "normalize")
    refused(L.pprhip_sweep_cut(None, 1, 0, 0, None, None, None, 0, None), "null info")
    refused(L.pprhip_results_sweep_cut(None, 0, 1, 0, 0, None, None, None, 0, None), "null info")
    refused(L.pprhip_local_cluster_seeds(None, sp, None, 1, 0.15, 1e-4, 1, 0, 0, None, 0, None, None), "null info")
    for args in ((p, None, None), (None, p, None), (None, None, p)):
        refused(L.pprhip_sweep_cut(None, 1, 0, 0, *args, 0, C.byref(info)), "cap = 0")
        refused(L.pprhip_results_sweep_cut(None, 0, 1, 0, 0, *args, 0, C.byref(info)), "cap = 0")
    refused(L.pprhip_local_cluster_seeds(None, sp, None, 1, 0.15, 1e-4, 1, 0, 0, p, 0, C.byref(info), None), "cap = 0")
    # alpha and rmax by the existing rules, before the handle as well
    refused(L.pprhip_local_cluster_seeds(None, sp, None, 1, 1.5, 1e-4, 1, 0, 0, None, 0, C.byref(info), None), "alpha")
    refused(L.pprhip_local_cluster_seeds(None, sp, None, 1, 0.15, -1.0, 1, 0, 0, None, 0, C.byref(info), None), "rmax")
    # and with good arguments the null handle is what is left to refuse
    refused(L.pprhip_sweep_cut(None, 1, 0, 0, None, None, None, 0, C.byref(info)), "null graph")
    refused(L.pprhip_results_sweep_cut(None, 0, 1, 0, 0, None, None, None, 0, C.byref(info)), "no result")


def test_release_keeps_refusing_unknown_bits(pkg):
    with pytest.raises(pkg.PprhipError):
        pkg._check(pkg.lib().pprhip_graph_release(None, 8))            # a null handle, whatever the flag
