"""The sweep cut on the GPU (pprhip_sweep_cut, pprhip_results_sweep_cut, pprhip_local_cluster_seeds; include/pprhip.h
"local clustering", DESIGN.md 2 "Sweep cut") against the numpy reference of tests/sweep_ref.py applied to the vector the
handle returns.  Every comparison is exact: order, vol, cut and the best prefix as integers, the conductance bit for bit -
the profile is integer arithmetic and the score one correctly rounded division, so no tolerance exists."""
import gc
import struct

import numpy as np
import pytest

from conftest import edges_to_host, shared_graph
from sweep_ref import cut_of, edges_of, sweep_ref
from test_sweep_ref import barbell_edges

ALPHA = 0.15
pytestmark = pytest.mark.gpu


def bits(d):
    return struct.pack("<d", float(d))


def same(got, ref, cap=None):
    """(order, vol, cut, Sweep) of the engine against sweep_ref's dict."""
    order, vol, cut, info = got
    k = ref["profiled"] if cap is None else min(cap, ref["profiled"])
    assert order.dtype == np.int32 and vol.dtype == np.uint64 and cut.dtype == np.uint64
    assert (info.support, info.profiled) == (ref["support"], ref["profiled"])
    assert order.size == vol.size == cut.size == k
    assert np.array_equal(order, ref["order"][:k]), "order differs at %s" % np.nonzero(order != ref["order"][:k])[0][:5]
    assert np.array_equal(vol, ref["vol"][:k]), "vol differs at %s" % np.nonzero(vol != ref["vol"][:k])[0][:5]
    assert np.array_equal(cut, ref["cut"][:k]), "cut differs at %s" % np.nonzero(cut != ref["cut"][:k])[0][:5]
    assert (info.best_size, info.best_cut, info.best_vol) == (ref["best_size"], ref["best_cut"], ref["best_vol"])
    assert bits(info.best_conductance) == bits(ref["best_conductance"]), (info.best_conductance, ref["best_conductance"])
    assert info.total_vol == ref["total_vol"] and info.edge_slots == ref["edge_slots"]


def check(g, edges, x=None, cap=None, **kw):
    """One sweep of the handle's vector with the arguments kw against the reference on that vector."""
    x = g.reserve() if x is None else x
    ref = sweep_ref(g.n, edges[0], edges[1], x, normalize=int(kw.get("normalize", True)), max_size=kw.get("max_size", 0),
                    max_vol=kw.get("max_vol", 0))
    got = g.sweep_cut(cap=cap, **kw)
    same(got, ref, cap)
    return ref, got


def barbell(pkg):
    src, dst = barbell_edges()
    return edges_to_host(pkg, 6, list(zip(src.tolist(), dst.tolist())))


# ------------------------------------------------------------------ toy graphs
@pytest.mark.parametrize("name", ["two_node", "cycle5", "star_dead_leaves", "isolated_mix", "line", "barbell"])
def test_toy_graphs_after_a_push(pkg, toy_graphs, name):
    host = barbell(pkg) if name == "barbell" else toy_graphs[name]
    edges = edges_of(host)
    with pkg.Graph(host, device=0) as g:
        g.forward_push(0, ALPHA, 1e-9)
        for normalize in (True, False):
            ref, _ = check(g, edges, normalize=normalize)
            assert ref["support"] > 0
        ref, _ = check(g, edges)
        if name == "star_dead_leaves":   # the five leaves tie: id order
            assert list(ref["order"]) == [0, 1, 2, 3, 4, 5]
        if name == "barbell":
            assert (ref["best_size"], ref["best_cut"], ref["best_vol"]) == (3, 2, 14) and sorted(ref["order"][:3]) == [0, 1, 2]
        if name == "isolated_mix":       # a push from an isolated node leaves x = 1 on a node without edges
            g.forward_push(4, ALPHA, 1e-9)
            ref, (order, vol, cut, info) = check(g, edges)
            assert info.support == 0 and info.profiled == 0 and info.best_size == 0 and order.size == 0
            assert info.best_conductance == float("inf") and info.edge_slots == 0 and info.total_vol == 12


# ------------------------------------------------------------------ GOT
def test_got_sources_seed_sets_and_bounds(pkg, got, dev_cache):
    g = shared_graph(dev_cache, pkg, "got", lambda: pkg.Graph(got, device=0))
    edges = edges_of(got)
    by_deg = np.argsort(-np.diff(got.out_rp.astype(np.int64)), kind="stable")
    srcs = [int(by_deg[0]), int(by_deg[7]), int(by_deg[40])]
    seed_set, weights = [srcs[1], srcs[2], int(by_deg[3])], [0.5, 0.2, 0.3]
    runs = [lambda s=s, r=r: g.forward_push(s, ALPHA, r, fetch=False) for s in srcs for r in (1e-4, 1e-7)]
    runs += [lambda r=r: g.forward_push_seeds(seed_set, ALPHA, r, weights=weights, fetch=False) for r in (1e-4, 1e-7)]
    runs += [lambda s=s: g.fora_single_source(s, 0.5, ALPHA, seed=3, fetch=False) for s in srcs]
    for run in runs:
        run()
        x = g.reserve()
        for normalize in (True, False):
            ref, _ = check(g, edges, x=x, normalize=normalize)
            support = ref["support"]
            assert support > 5
            for max_size in (1, 5, support):
                check(g, edges, x=x, normalize=normalize, max_size=max_size)
            for max_vol in (1, got.m):
                check(g, edges, x=x, normalize=normalize, max_vol=max_vol)
            check(g, edges, x=x, normalize=normalize, max_size=5, max_vol=got.m)
            check(g, edges, x=x, normalize=normalize, cap=3)
            _, _, _, info = g.sweep_cut(normalize=normalize, cap=0)
            assert info.best_size == ref["best_size"] and bits(info.best_conductance) == bits(ref["best_conductance"])


# ------------------------------------------------------------------ tile edges without knowing the tile
# (graphs built for the tile, the turns and the stride loops: test_gpu_sweep_cut_designs.py)
def stars_host(pkg, j):
    """A 3-cycle (ids 0, 1, 2), then three hubs (3, 4, 5) with 2^j - 1, 2^j and 2^j + 1 leaves each, hub <-> leaf in both
    directions: in slot space some hub ends before, on and after every power-of-two boundary up to 2^(j + 1)."""
    leaves = [(1 << j) - 1, 1 << j, (1 << j) + 1]
    n = 6 + sum(leaves)
    src = [np.array([0, 1, 2])]
    dst = [np.array([1, 2, 0])]
    first = 6
    for h, c in enumerate(leaves):
        lv = np.arange(first, first + c)
        hub = np.full(c, 3 + h)
        src += [hub, lv]
        dst += [lv, hub]
        first += c
    return pkg.HostCsr(n, np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32))


@pytest.mark.parametrize("j", list(range(5, 18)))
def test_hubs_around_every_tile_boundary(pkg, j):
    host = stars_host(pkg, j)
    edges = edges_of(host)
    with pkg.Graph(host, device=0) as g:
        g.forward_push_seeds([3, 4, 5, 1], ALPHA, 1e-12, fetch=False)
        x = g.reserve()
        for normalize in (True, False):
            ref, _ = check(g, edges, x=x, normalize=normalize)
            assert ref["support"] == host.n and ref["edge_slots"] == 2 * host.m
        check(g, edges, x=x, max_size=(1 << j) + 7)


# ------------------------------------------------------------------ R-MAT
@pytest.mark.parametrize("which", ["rmat12", "rmat15"])
def test_rmat_small_and_full_support(pkg, request, dev_cache, which):
    host = request.getfixturevalue(which)
    g = shared_graph(dev_cache, pkg, which, lambda: pkg.Graph(host, device=0))
    edges = edges_of(host)
    src = int(np.argmax(np.diff(host.out_rp.astype(np.int64))))
    sizes = []
    for rmax in (1e-3, 1e-8):
        g.forward_push(src, ALPHA, rmax, fetch=False)
        x = g.reserve()
        ref, (order, vol, cut, info) = check(g, edges, x=x)
        sizes.append(ref["support"])
        for i in np.unique(np.linspace(0, ref["profiled"] - 1, 8).astype(np.int64)):
            assert int(cut[i]) == cut_of(host.n, edges[0], edges[1], order[:i + 1]), "prefix %d" % i
        check(g, edges, x=x, normalize=False)
        check(g, edges, x=x, max_size=ref["support"] // 2, max_vol=host.m // 2)
    live = int(np.count_nonzero(np.bincount(np.concatenate(edges), minlength=host.n)))
    assert sizes[0] < sizes[1] and sizes[1] > 0.5 * live   # a small support, then most of the edge-bearing nodes


# ------------------------------------------------------------------ one-call form, result store
def test_local_cluster_is_push_then_sweep(pkg, got, dev_cache):
    g = shared_graph(dev_cache, pkg, "got", lambda: pkg.Graph(got, device=0))
    seeds, weights = [5, 17, 42], [1.0, 2.0, 1.0]
    for kw in (dict(), dict(normalize=False), dict(max_size=20), dict(max_vol=got.m // 4)):
        g.forward_push_seeds(seeds, ALPHA, 1e-6, weights=weights, fetch=False)
        x = g.reserve()
        order, _, _, info = g.sweep_cut(**kw)
        members, info2, st = g.local_cluster(seeds, ALPHA, 1e-6, weights=weights, **kw)
        assert np.array_equal(g.reserve(), x) and st.levels > 0
        assert info.best_size > 0 and np.array_equal(members, order[:info.best_size])
        a, b = info.as_dict(), info2.as_dict()
        assert {k: v for k, v in a.items() if not k.endswith("_ms")} == {k: v for k, v in b.items() if not k.endswith("_ms")}
        few, info3, _ = g.local_cluster(seeds, ALPHA, 1e-6, weights=weights, cap=2, **kw)
        assert np.array_equal(few, members[:2]) and info3.best_size == info.best_size
    with pytest.raises(pkg.PprhipError) as e:
        g.local_cluster([got.n], ALPHA, 1e-6)
    assert e.value.code == pkg.ERR_INVALID
    assert np.array_equal(g.reserve(), x)   # a bad seed set leaves the handle untouched


def test_local_cluster_on_the_barbell_is_the_seeds_triangle(pkg):
    with pkg.Graph(barbell(pkg), device=0) as g:
        for seed, want in ((0, [0, 1, 2]), (4, [3, 4, 5])):
            members, info, _ = g.local_cluster([seed], ALPHA, 1e-9)
            assert sorted(members) == want and (info.best_cut, info.best_vol) == (2, 14)
            assert bits(info.best_conductance) == bits(2.0 / 14.0)


def test_results_store_entries(pkg, rmat12, dev_cache):
    g = shared_graph(dev_cache, pkg, "rmat12", lambda: pkg.Graph(rmat12, device=0))
    edges = edges_of(rmat12)
    live = np.nonzero(np.diff(rmat12.out_rp) > 0)[0]
    sets = [live[3 * i: 3 * i + 1 + i % 3] for i in range(20)]
    store = pkg.Results(g, 20)
    try:
        g.fora_batch_seeds(sets, 0.5, ALPHA, seed=5, keep=store)
        for i in (0, 7, 19):
            x = store.fetch(i)
            for kw in (dict(), dict(normalize=False, max_size=100)):
                ref = sweep_ref(rmat12.n, edges[0], edges[1], x, normalize=int(kw.get("normalize", True)),
                                max_size=kw.get("max_size", 0))
                same(store.sweep_cut(i, **kw), ref)
            assert np.array_equal(store.fetch(i), x)
        with pytest.raises(pkg.PprhipError):
            store.sweep_cut(20)
    finally:
        store.close()
        g.release(g.RELEASE_BATCH)


# ------------------------------------------------------------------ stability, lifecycle
def test_sweep_is_repeatable_and_leaves_the_vector_alone(pkg, rmat12, dev_cache):
    g = shared_graph(dev_cache, pkg, "rmat12", lambda: pkg.Graph(rmat12, device=0))
    src = int(np.argmax(np.diff(rmat12.out_rp.astype(np.int64))))
    g.forward_push(src, ALPHA, 1e-6, fetch=False)
    x, r = g.reserve(), g.residue()
    top = g.topk_select(8)
    a = g.sweep_cut()
    b = g.sweep_cut()
    assert all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3]))
    assert {k: v for k, v in a[3].as_dict().items() if not k.endswith("_ms")} == \
           {k: v for k, v in b[3].as_dict().items() if not k.endswith("_ms")}
    assert a[3].total_ms > 0 and a[3].scan_ms > 0 and a[3].sort_ms > 0
    top2 = g.topk_select(8)
    assert np.array_equal(g.reserve(), x) and np.array_equal(g.residue(), r)
    assert top[0] == top2[0] and np.array_equal(top[1], top2[1]) and np.array_equal(top[2], top2[2]) and top[3] == top2[3]
    # after a top-k call the vector is the estimate of the last round: the sweep reads what reserve() returns
    g.fora_topk(src, 0.5, ALPHA, 10, seed=3)
    check(g, edges_of(rmat12))


def test_open_stream_refuses_the_sweep(pkg, rmat12):
    live = np.nonzero(np.diff(rmat12.out_rp) > 0)[0][:4].astype(np.int32)
    with pkg.Graph(rmat12, device=0) as g:
        g.forward_push(int(live[0]), ALPHA, 1e-4, fetch=False)
        g.set_tuning(pkg.tuning_batch())
        with pkg.QueryStream(g, 0.5, ALPHA, k=4):
            with pytest.raises(pkg.PprhipError) as e:
                g.sweep_cut()
            assert e.value.code == pkg.ERR_STATE
            with pytest.raises(pkg.PprhipError) as e:
                g.local_cluster([int(live[0])], ALPHA, 1e-4)
            assert e.value.code == pkg.ERR_STATE
        g.forward_push(int(live[0]), ALPHA, 1e-4, fetch=False)
        assert g.sweep_cut(cap=0)[3].support > 0


def test_release_returns_the_workspace(pkg):
    host = stars_host(pkg, 17)   # 393 K nodes: a workspace of 30 MB
    edges = edges_of(host)
    with pkg.Graph(host, device=0) as g:
        g.forward_push_seeds([3, 4, 5, 1], ALPHA, 1e-6, fetch=False)
        free0, _ = g.device_memory()
        first = g.sweep_cut()
        free1, _ = g.device_memory()
        assert free0 - free1 >= 64 * host.n, "the sweep's workspace took %d bytes" % (free0 - free1)
        g.release(g.RELEASE_SWEEP)
        free2, _ = g.device_memory()
        assert free2 - free1 >= 64 * host.n, "release gave %d bytes back" % (free2 - free1)
        g.release(g.RELEASE_SWEEP)   # nothing to release: a no-op
        with pytest.raises(pkg.PprhipError) as e:
            g.release(64)
        assert e.value.code == pkg.ERR_INVALID
        again = g.sweep_cut()
        assert all(np.array_equal(p, q) for p, q in zip(first[:3], again[:3]))
        same(again, sweep_ref(host.n, edges[0], edges[1], g.reserve()))


def test_closed_handles_leave_no_bytes(pkg, rmat12):
    host = stars_host(pkg, 17)

    def one_life():
        with pkg.Graph(host, device=0) as g:
            g.forward_push_seeds([3, 4, 5, 1], ALPHA, 1e-6, fetch=False)
            assert g.sweep_cut(cap=0)[3].support == host.n
            g.local_cluster([3], ALPHA, 1e-6, cap=4)
        gc.collect()

    with pkg.Graph(rmat12, device=0) as probe:   # a small handle that stays: pprhip_device_memory needs one
        one_life()
        one_life()
        free0, _ = probe.device_memory()
        for _ in range(4):
            one_life()
        free1, _ = probe.device_memory()
    print("four more lives: device %+.1f MB" % ((free0 - free1) / 1e6))
    assert free0 - free1 <= 64 << 20, "device memory not returned: %.1f MB after four more lives" % ((free0 - free1) / 1e6)
