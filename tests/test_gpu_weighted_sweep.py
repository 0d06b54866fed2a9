"""The sweep cut by relationship weight on the GPU (pprhip_weighted_sweep_cut, pprhip_results_weighted_sweep_cut,
pprhip_weighted_local_cluster_seeds; include/pprhip.h "weighted local clustering", DESIGN.md 2 "Weighted sweep cut")
against the numpy reference of tests/weighted_sweep_ref.py applied to the vector the handle returns.  Every comparison
is exact: order, vol_q, cut_q, the shift, the total volume and the best prefix as integers, the conductance bit for bit -
the weights enter as integer quanta and the score is one correctly rounded division, so no tolerance exists."""
import struct

import numpy as np
import pytest

from conftest import edges_to_host
from sweep_ref import edges_of, sweep_ref
from test_sweep_ref import barbell_edges
from weighted_sweep_ref import quanta, shift_of, weighted_sweep_ref

ALPHA = 0.15
WEIGHT_SETS = ["uniform", "pareto", "ones", "spread"]
pytestmark = pytest.mark.gpu


def bits(d):
    return struct.pack("<d", float(d))


def weights_of(name, m, seed=7):
    """The weight sets of the issue.  "spread": 1e-30 .. 1e30, so that most relationships fall below half a quantum and
    the clamp to one quantum happens on the device."""
    rng = np.random.default_rng(seed)
    if name == "uniform":
        return rng.uniform(0.5, 1.5, m)
    if name == "pareto":
        return rng.pareto(1.5, m) + 0.01
    if name == "ones":
        return np.ones(m)
    w = 10.0 ** rng.uniform(-30, 30, m)
    w[m // 3], w[m // 2] = 1e30, 1e-30
    return w


def same(got, ref, cap=None):
    """(order, vol_q, cut_q, WeightedSweep) of the engine against weighted_sweep_ref's dict."""
    order, vol, cut, info = got
    k = ref["profiled"] if cap is None else min(cap, ref["profiled"])
    assert order.dtype == np.int32 and vol.dtype == np.uint64 and cut.dtype == np.uint64
    assert (info.shift, info.total_vol_q) == (ref["shift"], ref["total_vol_q"])
    assert (info.support, info.profiled) == (ref["support"], ref["profiled"])
    assert order.size == vol.size == cut.size == k
    assert np.array_equal(order, ref["order"][:k]), "order differs at %s" % np.nonzero(order != ref["order"][:k])[0][:5]
    assert np.array_equal(vol, ref["vol_q"][:k]), "vol_q differs at %s" % np.nonzero(vol != ref["vol_q"][:k])[0][:5]
    assert np.array_equal(cut, ref["cut_q"][:k]), "cut_q differs at %s" % np.nonzero(cut != ref["cut_q"][:k])[0][:5]
    assert (info.best_size, info.best_cut_q, info.best_vol_q) == (ref["best_size"], ref["best_cut_q"], ref["best_vol_q"])
    assert bits(info.best_conductance) == bits(ref["best_conductance"]), (info.best_conductance, ref["best_conductance"])
    assert info.edge_slots == ref["edge_slots"]


def check(g, edges, w, x=None, cap=None, **kw):
    """One weighted sweep of the handle's vector with the arguments kw against the reference on that vector."""
    x = g.reserve() if x is None else x
    ref = weighted_sweep_ref(g.n, edges[0], edges[1], w, x, normalize=int(kw.get("normalize", True)),
                             max_size=kw.get("max_size", 0), max_vol=kw.get("max_vol", 0.0))
    got = g.weighted_sweep_cut(cap=cap, **kw)
    same(got, ref, cap)
    return ref, got


def words(got):
    order, vol, cut, info = got
    return (order.tobytes(), vol.tobytes(), cut.tobytes(),
            tuple(sorted((k, bits(v) if isinstance(v, float) else v) for k, v in info.as_dict().items()
                         if not k.endswith("_ms"))))


def barbell(pkg):
    src, dst = barbell_edges()
    return edges_to_host(pkg, 6, list(zip(src.tolist(), dst.tolist())))


# ------------------------------------------------------------------ toy graphs
@pytest.mark.parametrize("name", ["two_node", "cycle5", "star_dead_leaves", "isolated_mix", "line", "barbell"])
def test_toy_graphs_after_a_weighted_push(pkg, toy_graphs, name):
    host = barbell(pkg) if name == "barbell" else toy_graphs[name]
    edges = edges_of(host)
    with pkg.Graph(host, device=0) as g:
        for wname in WEIGHT_SETS:
            w = weights_of(wname, host.m)
            g.set_weights(w)
            g.weighted_forward_push(0, ALPHA, 1e-9, fetch=False)
            for normalize in (True, False):
                ref, _ = check(g, edges, w, normalize=normalize)
                assert ref["support"] > 0
        if name == "barbell":      # a bridge heavier than a triangle is not cut
            w = np.ones(host.m)
            g.set_weights(w)
            g.weighted_forward_push(0, ALPHA, 1e-9, fetch=False)
            ref, _ = check(g, edges, w)
            assert ref["best_size"] == 3 and bits(ref["best_conductance"]) == bits(2.0 / 14.0)
            w[(edges[0] == 2) & (edges[1] == 3)] = 8.0
            w[(edges[0] == 3) & (edges[1] == 2)] = 8.0
            g.set_weights(w)
            ref, _ = check(g, edges, w, normalize=False)
            assert ref["best_size"] != 3
        if name == "isolated_mix":  # a push from an isolated node leaves x = 1 on a node without edges
            g.weighted_forward_push(4, ALPHA, 1e-9, fetch=False)
            ref, (order, vol, cut, info) = check(g, edges, w)
            assert info.support == 0 and info.profiled == 0 and info.best_size == 0 and order.size == 0
            assert info.best_conductance == float("inf") and info.edge_slots == 0


# ------------------------------------------------------------------ GOT
@pytest.mark.parametrize("wname", WEIGHT_SETS)
def test_got_sources_seed_sets_and_bounds(pkg, got, wname):
    edges = edges_of(got)
    w = weights_of(wname, got.m)
    by_deg = np.argsort(-np.diff(got.out_rp.astype(np.int64)), kind="stable")
    srcs = [int(by_deg[0]), int(by_deg[7]), int(by_deg[40])]
    seed_set, sw = [srcs[1], srcs[2], int(by_deg[3])], [0.5, 0.2, 0.3]
    with pkg.Graph(got, device=0) as g:
        g.set_weights(w)
        runs = [lambda s=s, r=r: g.weighted_forward_push(s, ALPHA, r, fetch=False) for s in srcs for r in (1e-4, 1e-7)]
        runs += [lambda r=r: g.weighted_forward_push_seeds(seed_set, ALPHA, r, weights=sw, fetch=False) for r in (1e-4, 1e-7)]
        runs += [lambda s=s: g.weighted_fora(s, 0.5, ALPHA, seed=3, fetch=False) for s in srcs]
        runs += [lambda: g.weighted_fora_seeds(seed_set, 0.5, ALPHA, seed=3, weights=sw, fetch=False)]
        # the sweep reads any vector: an unweighted push
        runs += [lambda s=s: g.forward_push(s, ALPHA, 1e-6, fetch=False) for s in srcs]
        runs += [lambda: g.forward_push_seeds(seed_set, ALPHA, 1e-6, weights=sw, fetch=False)]
        one_quantum, half = float(np.ldexp(1.0, -shift_of(w))), float(np.sum(w)) / 2
        clamped = int(np.count_nonzero(np.ldexp(w, shift_of(w)) < 0.5))
        assert (clamped > got.m // 2) == (wname == "spread")
        for run in runs:
            run()
            x = g.reserve()
            for normalize in (True, False):
                ref, _ = check(g, edges, w, x=x, normalize=normalize)
                support = ref["support"]
                assert support > 5
                for max_size in (1, 5, support):
                    check(g, edges, w, x=x, normalize=normalize, max_size=max_size)
                for max_vol in (one_quantum, half):
                    check(g, edges, w, x=x, normalize=normalize, max_vol=max_vol)
                check(g, edges, w, x=x, normalize=normalize, max_size=5, max_vol=half)
                check(g, edges, w, x=x, normalize=normalize, cap=3)
                _, _, _, info = g.weighted_sweep_cut(normalize=normalize, cap=0)
                assert info.best_size == ref["best_size"] and bits(info.best_conductance) == bits(ref["best_conductance"])
            assert np.array_equal(g.reserve(), x)          # the vector is not modified


def test_a_bound_below_one_quantum_admits_nothing(pkg, got):
    edges = edges_of(got)
    w = weights_of("uniform", got.m)
    with pkg.Graph(got, device=0) as g:
        g.set_weights(w)
        g.weighted_forward_push(0, ALPHA, 1e-6, fetch=False)
        ref, (order, _, _, info) = check(g, edges, w, max_vol=1e-30)
        assert info.best_size == 0 and info.best_conductance == float("inf") and order.size == ref["support"] > 0
        check(g, edges, w, max_vol=1e300)                  # the limit saturates at 2^63 - 1: no bound in effect


# ------------------------------------------------------------------ R-MAT: more than one tile, hubs, many workgroups
def test_rmat12_against_the_reference(pkg, rmat12):
    edges = edges_of(rmat12)
    src = int(np.argmax(np.diff(rmat12.out_rp.astype(np.int64))))
    with pkg.Graph(rmat12, device=0) as g:
        for wname in ("pareto", "spread"):
            w = weights_of(wname, rmat12.m)
            g.set_weights(w)
            for rmax in (1e-3, 1e-8):
                g.weighted_forward_push(src, ALPHA, rmax, fetch=False)
                x = g.reserve()
                ref, got = check(g, edges, w, x=x)
                check(g, edges, w, x=x, normalize=False)
                check(g, edges, w, x=x, max_size=ref["support"] // 2, max_vol=float(np.sum(w)) / 4)
                assert words(g.weighted_sweep_cut()) == words(got)       # the same words every run
            assert ref["edge_slots"] > 8 * 4096


# ------------------------------------------------------------------ state
def test_no_weights_is_err_state(pkg, got):
    with pkg.Graph(got, device=0) as g:
        g.forward_push(0, ALPHA, 1e-4, fetch=False)
        for call in (lambda: g.weighted_sweep_cut(), lambda: g.weighted_local_cluster([0], ALPHA, 1e-4)):
            with pytest.raises(pkg.PprhipError) as e:
                call()
            assert e.value.code == pkg.ERR_STATE and "no relationship weights" in str(e.value)
        w = weights_of("uniform", got.m)
        g.set_weights(w)
        check(g, edges_of(got), w)
        g.release(g.RELEASE_WEIGHTS)
        with pytest.raises(pkg.PprhipError) as e:
            g.weighted_sweep_cut()
        assert e.value.code == pkg.ERR_STATE
        assert g.sweep_cut(cap=0)[3].support > 0           # the unweighted sweep does not need them
        g.set_weights(w)
        check(g, edges_of(got), w)


def test_open_stream_refuses_the_weighted_sweep(pkg, rmat12):
    live = np.nonzero(np.diff(rmat12.out_rp) > 0)[0][:4].astype(np.int32)
    with pkg.Graph(rmat12, device=0) as g:
        g.set_weights(weights_of("uniform", rmat12.m))
        g.weighted_forward_push(int(live[0]), ALPHA, 1e-4, fetch=False)
        g.set_tuning(pkg.tuning_batch())
        with pkg.QueryStream(g, 0.5, ALPHA, k=4):
            for call in (lambda: g.weighted_sweep_cut(), lambda: g.weighted_local_cluster([int(live[0])], ALPHA, 1e-4)):
                with pytest.raises(pkg.PprhipError) as e:
                    call()
                assert e.value.code == pkg.ERR_STATE
        g.weighted_forward_push(int(live[0]), ALPHA, 1e-4, fetch=False)
        assert g.weighted_sweep_cut(cap=0)[3].support > 0


def test_a_second_weight_set_rebuilds_the_quanta(pkg, got):
    edges = edges_of(got)
    w1, w2 = weights_of("uniform", got.m), weights_of("pareto", got.m) * 1024.0
    assert shift_of(w1) != shift_of(w2)
    with pkg.Graph(got, device=0) as g, pkg.Graph(got, device=0) as fresh:
        g.set_weights(w1)
        g.weighted_forward_push(3, ALPHA, 1e-6, fetch=False)
        check(g, edges, w1)
        g.set_weights(w2)
        g.weighted_forward_push(3, ALPHA, 1e-6, fetch=False)
        _, got2 = check(g, edges, w2)
        fresh.set_weights(w2)
        fresh.weighted_forward_push(3, ALPHA, 1e-6, fetch=False)
        assert words(fresh.weighted_sweep_cut()) == words(got2)
        assert got2[3].shift == shift_of(w2) and got2[3].total_vol_q == 2 * sum(quanta(w2).tolist())


def test_weighted_and_unweighted_sweeps_interleaved(pkg, rmat12):
    edges = edges_of(rmat12)
    w = weights_of("pareto", rmat12.m)
    src = int(np.argmax(np.diff(rmat12.out_rp.astype(np.int64))))
    with pkg.Graph(rmat12, device=0) as g:
        g.set_weights(w)
        g.weighted_forward_push(src, ALPHA, 1e-6, fetch=False)
        x = g.reserve()
        uref = sweep_ref(g.n, edges[0], edges[1], x)
        for kw in (dict(), dict(normalize=False), dict(max_size=100)):
            _, a = check(g, edges, w, x=x, **kw)
            order, vol, cut, info = g.sweep_cut()
            assert np.array_equal(order, uref["order"]) and np.array_equal(vol, uref["vol"]) and np.array_equal(cut, uref["cut"])
            assert (info.best_size, info.best_cut, info.best_vol) == (uref["best_size"], uref["best_cut"], uref["best_vol"])
            assert bits(info.best_conductance) == bits(uref["best_conductance"])
            assert words(g.weighted_sweep_cut(**kw)) == words(a)
        assert np.array_equal(g.reserve(), x)


# ------------------------------------------------------------------ memory
def big_host(pkg):
    """Three hubs with 2^17 leaves each, hub <-> leaf in both directions: 393 K nodes, 786 K relationships."""
    c = 1 << 17
    src, dst = [], []
    for h in range(3):
        lv = np.arange(3 + h * c, 3 + (h + 1) * c)
        src += [np.full(c, h), lv]
        dst += [lv, np.full(c, h)]
    return pkg.HostCsr(3 + 3 * c, np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32))


def test_accounting_and_release(pkg):
    host = big_host(pkg)
    edges = edges_of(host)
    w = weights_of("uniform", host.m)
    n = host.n
    with pkg.Graph(host, device=0) as g:
        def cycle():
            g.set_weights(w)
            present, b0 = g.weights_info()
            assert present and b0 >= 24 * host.m + 8 * n
            g.weighted_forward_push_seeds([0, 1, 2, 5], ALPHA, 1e-6, fetch=False)
            g.sweep_cut(cap=0)                             # the unweighted workspace first: no weighted bytes yet
            assert g.weights_info() == (True, b0)
            free_a, _ = g.device_memory()
            got = g.weighted_sweep_cut()
            free_b, _ = g.device_memory()
            assert g.weights_info() == (True, b0 + 8 * n)  # qdeg, counted while it exists
            assert free_a - free_b >= 16 * n               # qdeg and the volume in quanta
            g.weighted_sweep_cut(cap=0)
            assert g.weights_info() == (True, b0 + 8 * n)
            return got

        free0, _ = g.device_memory()
        first = cycle()
        same(first, weighted_sweep_ref(n, edges[0], edges[1], w, g.reserve()))
        g.release(g.RELEASE_SWEEP | g.RELEASE_WEIGHTS)
        assert g.weights_info() == (False, 0)
        free1, _ = g.device_memory()
        again = cycle()
        same(again, weighted_sweep_ref(n, edges[0], edges[1], w, g.reserve()))
        g.release(g.RELEASE_SWEEP | g.RELEASE_WEIGHTS)
        free2, _ = g.device_memory()
        print("free before %d, after one cycle %d, after two %d" % (free0, free1, free2))
        # The first cycle is the warm-up, as in test_gpu_lifecycle.py: it also holds what the handle's first seeded push
        # allocates and keeps (the seed tables).  A cycle holds 16 n bytes (6 MB) for the weighted sweep alone and 50 MB
        # more: nothing of that stays behind the second one (2 MB: one allocation granule of slack)
        assert free1 - free2 <= 2 << 20, "a cycle of set_weights, sweeps and release kept %d bytes" % (free1 - free2)
        # the weights alone go: the sweep workspace stays, and the next weighted sweep rebuilds qdeg
        g.set_weights(w)
        g.weighted_forward_push_seeds([0, 1, 2, 5], ALPHA, 1e-6, fetch=False)
        a = g.weighted_sweep_cut()
        g.set_weights(None)
        assert g.weights_info() == (False, 0)
        g.set_weights(2.0 * w)
        b = g.weighted_sweep_cut()                         # the same vector; scaling by 2 moves the shift alone
        assert words(b)[:3] == words(a)[:3] and b[3].shift == a[3].shift - 1 and b[3].total_vol_q == a[3].total_vol_q
