"""Sparse results on the GPU (pprhip_get_reserve_sparse, pprhip_get_residue_sparse, pprhip_results_fetch_sparse,
pprhip_results_fetch_sparse_all; include/pprhip.h "sparse results", DESIGN.md 2 "Sparse results") against the numpy
reference of tests/sparse_ref.py applied to the dense vector the same handle returns.  Every comparison is exact: ids
equal, values bit for bit - the compaction copies values and the orders are total, so no tolerance exists."""
import gc

import numpy as np
import pytest

from conftest import edges_to_host, shared_graph
from sparse_ref import BY_ID, BY_VALUE, same_bits, sparse_ref, sparse_ref_all, truncate

ALPHA = 0.15
ORDERS = (("id", BY_ID), ("value", BY_VALUE))
pytestmark = pytest.mark.gpu


def same(got, ref_ids, ref_vals, cap=None):
    """(ids, vals, count) of the engine against the reference's entries cut at cap."""
    ids, vals, count = got
    want_ids, want_vals, want_count = truncate(ref_ids, ref_vals, ref_ids.size if cap is None else cap)
    assert ids.dtype == np.int32 and vals.dtype == np.float64
    assert count == want_count, (count, want_count)
    assert ids.size == vals.size == want_ids.size, (ids.size, vals.size, want_ids.size)
    assert np.array_equal(ids, want_ids), "ids differ at %s" % np.nonzero(ids != want_ids)[0][:5]
    assert same_bits(vals, want_vals), "values differ at %s" % np.nonzero(vals != want_vals)[0][:5]


def caps_of(count):
    return sorted({c for c in (0, 1, count - 1, count, count + 5) if c >= 0})


def check(fetch, x, thresholds, caps=True):
    """fetch(threshold=, order=, cap=) over the dense vector x: both orders at every threshold, whole and cut at the
    caps {0, 1, count - 1, count, count + 5}.  Returns the counts, one per threshold."""
    counts = []
    for thr in thresholds:
        for name, order in ORDERS:
            ref_ids, ref_vals = sparse_ref(x, thr, order)
            same(fetch(threshold=thr, order=name), ref_ids, ref_vals)
            for cap in (caps_of(ref_ids.size) if caps else ()):
                same(fetch(threshold=thr, order=name, cap=cap), ref_ids, ref_vals, cap)
        counts.append(int(ref_ids.size))
    return counts


def kept_thresholds(x):
    """0, the median kept value, the maximum (strict: the maximum itself drops out), 1.0 (nothing is kept)."""
    kept = x[x > 0]
    return [0.0, float(np.sort(kept)[kept.size // 2]), float(kept.max()), 1.0]


# ------------------------------------------------------------------ toy graphs, GOT
@pytest.mark.parametrize("name", ["two_node", "cycle5", "star_dead_leaves", "isolated_mix", "line", "got"])
def test_toy_graphs_after_a_push(pkg, toy_graphs, got, name):
    host = got if name == "got" else toy_graphs[name]
    with pkg.Graph(host, device=0) as g:
        g.forward_push(0, ALPHA, 1e-9, fetch=False)
        for fetch, x in ((g.reserve_sparse, g.reserve()), (g.residue_sparse, g.residue())):
            if not np.any(x > 0):      # (a converged push may leave no residue at all)
                assert fetch()[2] == 0
                continue
            thresholds = kept_thresholds(x)
            counts = check(fetch, x, thresholds)
            assert counts[0] == np.count_nonzero(x > 0) > 0 and counts[3] == 0
            assert counts[2] < counts[0]          # the maximum dropped out
        assert g.reserve_sparse()[2] > 0


# ------------------------------------------------------------------ tile edges without knowing the tile
N_TILE = (1 << 18) + 3


def cycle_and_isolated(pkg):
    """A 3-cycle on the ids 0, 1, 2 and isolated nodes up to n = 2^18 + 3.  A seed set of isolated nodes - dead ends -
    leaves reserve = p, so forward_push_seeds over a designed set yields a designed support."""
    return edges_to_host(pkg, N_TILE, [(0, 1), (1, 2), (2, 0)])


def around(j):
    return [(1 << j) - 1, 1 << j, (1 << j) + 1]


def designed_supports():
    n = N_TILE
    out = [("last", [n - 1], None), ("first_isolated", [3], None)]
    for j in range(5, 18):
        out.append(("around_2^%d" % j, around(j), [1.0, 2.0, 3.0]))
    every = sorted({v for j in range(5, 18) for v in around(j)})
    out.append(("around_all", every, [float(1 + i) for i in range(len(every))]))
    block = list(range((1 << 12) - 70, (1 << 12) + 71))
    out.append(("block_at_2^12", block, [float(1 + (7 * i) % len(block)) for i in range(len(block))]))
    return out


def test_designed_supports_at_every_power_of_two(pkg, dev_cache):
    g = shared_graph(dev_cache, pkg, "tile", lambda: pkg.Graph(cycle_and_isolated(pkg), device=0))
    for name, support, weights in designed_supports():
        g.forward_push_seeds(support, ALPHA, 1e-9, weights=weights, fetch=False)
        x = g.reserve()
        assert np.array_equal(np.flatnonzero(x > 0), np.array(support)), name     # the design holds: not vacuous
        if weights is not None:
            assert np.unique(x[support]).size == len(support), name               # distinct values
        counts = check(g.reserve_sparse, x, [0.0], caps=len(support) > 1)
        assert counts == [len(support)], name
        check(g.residue_sparse, g.residue(), [0.0], caps=False)


def test_full_and_tied_supports(pkg, dev_cache):
    g = shared_graph(dev_cache, pkg, "tile", lambda: pkg.Graph(cycle_and_isolated(pkg), device=0))
    n = N_TILE
    isolated = np.arange(3, n, dtype=np.int32)
    # all isolated nodes, uniform weights: every value ties, so by value is by id
    g.forward_push_seeds(isolated, ALPHA, 1e-9, fetch=False)
    x = g.reserve()
    assert np.array_equal(np.flatnonzero(x > 0), isolated) and np.unique(x[3:]).size == 1
    assert check(g.reserve_sparse, x, [0.0]) == [n - 3]
    by_id, by_value = g.reserve_sparse(order="id"), g.reserve_sparse(order="value")
    assert by_id[2] == by_value[2] == n - 3
    assert np.array_equal(by_id[0], isolated) and np.array_equal(by_value[0], isolated)
    # ... plus node 0, pushed until the cycle holds reserve everywhere: full support
    g.forward_push_seeds(np.arange(n, dtype=np.int32)[np.r_[0, 3:n]], ALPHA, 1e-12, fetch=False)
    x = g.reserve()
    assert np.count_nonzero(x > 0) == n
    assert check(g.reserve_sparse, x, [0.0, float(x[1])], caps=False)[0] == n
    r = g.residue()
    check(g.residue_sparse, r, [0.0])
    # weights cycling through 1, 2, 3: runs of ties in every tile
    w = 1.0 + (np.arange(isolated.size) % 3)
    g.forward_push_seeds(isolated, ALPHA, 1e-9, weights=w, fetch=False)
    x = g.reserve()
    assert np.array_equal(np.flatnonzero(x > 0), isolated) and np.unique(x[3:]).size == 3
    levels = np.unique(x[3:])
    counts = check(g.reserve_sparse, x, [0.0, float(levels[0]), float(levels[1])])
    assert counts[0] == n - 3 and counts[0] > counts[1] > counts[2] > 0
    ids, vals, _ = g.reserve_sparse(order="value")
    assert np.all(np.diff(vals) <= 0)
    for lv in levels:       # inside a run of ties the ids ascend
        assert np.all(np.diff(ids[vals == lv]) > 0)


# ------------------------------------------------------------------ R-MAT
@pytest.mark.parametrize("which", ["rmat12", "rmat15"])
def test_rmat_small_and_full_support(pkg, request, dev_cache, which):
    host = request.getfixturevalue(which)
    g = shared_graph(dev_cache, pkg, which, lambda: pkg.Graph(host, device=0))
    src = int(np.argmax(np.diff(host.out_rp.astype(np.int64))))
    thresholds = [0.0, 1.0 / host.n, 1e-3]
    sizes = []
    for rmax in (1e-3, 1e-8):
        g.forward_push(src, ALPHA, rmax, fetch=False)
        sizes.append(check(g.reserve_sparse, g.reserve(), thresholds)[0])
        check(g.residue_sparse, g.residue(), thresholds)
    edge_bearing = int(np.count_nonzero((np.diff(host.out_rp.astype(np.int64)) + np.diff(host.in_rp.astype(np.int64))) > 0))
    assert sizes[0] < sizes[1] and sizes[1] > 0.5 * edge_bearing   # a small support, then most of the edge-bearing nodes
    assert sizes[0] < 0.25 * edge_bearing
    g.fora_single_source(src, 0.5, ALPHA, seed=3, fetch=False)
    counts = check(g.reserve_sparse, g.reserve(), thresholds)
    assert counts[0] >= counts[1] >= counts[2] > 0


def test_internal_order_is_invisible(pkg, rmat15, monkeypatch):
    """PPRHIP_RELABEL=0 keeps the caller's ids as the internal order: the compaction then reads x[v] and not
    x[old2new[v]].  A seed set of dead ends leaves reserve = p on either handle, the same bits: so the same sparse result."""
    dead = np.flatnonzero(np.diff(rmat15.out_rp.astype(np.int64)) == 0)
    assert dead.size > 2000
    seeds = dead[:: max(1, dead.size // 1500)].astype(np.int32)
    weights = 1.0 + (np.arange(seeds.size) * 37) % 101
    g_def = pkg.Graph(rmat15)
    monkeypatch.setenv("PPRHIP_RELABEL", "0")
    g_ids = pkg.Graph(rmat15)
    try:
        out = []
        for g in (g_def, g_ids):
            g.forward_push_seeds(seeds, ALPHA, 1e-9, weights=weights, fetch=False)
            x = g.reserve()
            assert np.array_equal(np.flatnonzero(x > 0), seeds)
            thr = float(np.median(x[seeds]))
            check(g.reserve_sparse, x, [0.0, thr])
            out.append([g.reserve_sparse(threshold=t, order=o) for t in (0.0, thr) for o in ("id", "value")])
        for a, b in zip(*out):
            assert a[2] == b[2] and np.array_equal(a[0], b[0]) and same_bits(a[1], b[1])
    finally:
        g_def.close()
        g_ids.close()


# ------------------------------------------------------------------ result store
def check_store(store, count):
    rows = [store.fetch(i) for i in range(count)]
    maxima = np.array([x.max() for x in rows])
    assert np.all(maxima > 0)
    distinct = np.unique(maxima)
    mid = float(distinct[(distinct.size - 1) // 2])   # some row's maximum, a larger one above it when there is any
    for thr in (0.0, 1.0 / rows[0].size, mid):
        for name, order in ORDERS:
            for i, x in enumerate(rows):
                ref_ids, ref_vals = sparse_ref(x, thr, order)
                same(store.fetch_sparse(i, threshold=thr, order=name), ref_ids, ref_vals)
                if i in (0, count - 1):
                    for cap in caps_of(ref_ids.size):
                        same(store.fetch_sparse(i, threshold=thr, order=name, cap=cap), ref_ids, ref_vals, cap)
            ref_offs, ref_ids, ref_vals = sparse_ref_all(rows, thr, order)
            offs, ids, vals, total = store.fetch_sparse_all(threshold=thr, order=name)
            assert offs.dtype == np.uint64 and np.array_equal(offs, ref_offs) and total == ref_ids.size
            same((ids, vals, total), ref_ids, ref_vals)
            sizes = np.diff(ref_offs.astype(np.int64))
            if thr == mid:     # that row and every row with a smaller maximum are empty, the others are not
                assert np.array_equal(sizes == 0, maxima <= mid) and np.any(sizes == 0)
                assert np.any(sizes > 0) == (distinct.size > 1)
            wide = np.flatnonzero(sizes > 1)
            k = int(wide[wide.size // 2]) if wide.size else 0
            for cap in (0, int(ref_offs[k]) + int(sizes[k]) // 2, total, total + 5):   # one ends in the middle of row k
                offs, ids, vals, total2 = store.fetch_sparse_all(threshold=thr, order=name, cap=cap)
                assert np.array_equal(offs, ref_offs) and total2 == total
                same((ids, vals, total2), ref_ids, ref_vals, cap)
    for i in range(count):
        assert same_bits(store.fetch(i), rows[i])


def test_results_store(pkg, rmat12, dev_cache):
    g = shared_graph(dev_cache, pkg, "rmat12", lambda: pkg.Graph(rmat12, device=0))
    live = np.nonzero(np.diff(rmat12.out_rp) > 0)[0]
    store = pkg.Results(g, 17)
    try:
        offs, ids, vals, total = store.fetch_sparse_all()                        # an empty store
        assert list(offs) == [0] and total == 0 and ids.size == 0 and vals.size == 0
        offs, ids, vals, total = store.fetch_sparse_all(order="value", cap=4)
        assert list(offs) == [0] and total == 0 and ids.size == 0
        with pytest.raises(pkg.PprhipError) as e:
            store.fetch_sparse(0)
        assert e.value.code == pkg.ERR_INVALID
        srcs = live[np.linspace(0, live.size - 1, 17).astype(np.int64)]           # more than BATCH queries
        assert srcs.size > pkg.BATCH
        g.fora_batch_single_source(srcs, 0.5, ALPHA, seed=5, keep=store)
        assert store.info()[1] == 17
        check_store(store, 17)
        assert np.unique([store.fetch(i).max() for i in range(17)]).size > 1
        with pytest.raises(pkg.PprhipError) as e:
            store.fetch_sparse(17)
        assert e.value.code == pkg.ERR_INVALID
        has_in = np.nonzero(np.diff(rmat12.in_rp) > 0)[0]
        targets = has_in[np.linspace(0, has_in.size - 1, 4).astype(np.int64)]
        g.ppr_targets(targets, ALPHA, 1e-4, keep=store, fetch=False)
        assert store.info()[1] == 4
        check_store(store, 4)
    finally:
        store.close()
        g.release(g.RELEASE_BATCH)


# ------------------------------------------------------------------ behaviour
def test_repeatable_and_leaves_the_vector_alone(pkg, rmat12, dev_cache):
    g = shared_graph(dev_cache, pkg, "rmat12", lambda: pkg.Graph(rmat12, device=0))
    src = int(np.argmax(np.diff(rmat12.out_rp.astype(np.int64))))
    g.forward_push(src, ALPHA, 1e-6, fetch=False)
    x, r = g.reserve(), g.residue()
    top = g.topk_select(8)
    cut = g.sweep_cut()
    for order in ("id", "value"):
        for fetch in (g.reserve_sparse, g.residue_sparse):
            a, b = fetch(threshold=1e-7, order=order), fetch(threshold=1e-7, order=order)
            assert a[2] == b[2] > 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert same_bits(g.reserve(), x) and same_bits(g.residue(), r)
    top2, cut2 = g.topk_select(8), g.sweep_cut()
    assert top[0] == top2[0] and np.array_equal(top[1], top2[1]) and same_bits(top[2], top2[2]) and top[3] == top2[3]
    assert all(np.array_equal(p, q) for p, q in zip(cut[:3], cut2[:3]))
    assert cut[3].best_size == cut2[3].best_size and cut[3].support == cut2[3].support
    # the cap largest: by value with a small cap is the head of the top-k order
    ids, vals, count = g.reserve_sparse(order="value", cap=8)
    k = min(8, top[1].size)
    assert count == np.count_nonzero(x > 0) and np.array_equal(ids[:k], top[1][:k]) and same_bits(vals[:k], top[2][:k])
    # after a top-k call the vector is the estimate of the last round: the sparse getter reads what reserve() returns
    g.fora_topk(src, 0.5, ALPHA, 10, seed=3)
    check(g.reserve_sparse, g.reserve(), [0.0, 1e-3])


def test_open_stream_refuses_every_sparse_call(pkg, rmat12):
    live = np.nonzero(np.diff(rmat12.out_rp) > 0)[0][:4].astype(np.int32)
    with pkg.Graph(rmat12, device=0) as g:
        g.set_tuning(pkg.tuning_batch())
        store = pkg.Results(g, 4)
        try:
            g.fora_batch_single_source(live, 0.5, ALPHA, seed=5, keep=store)
            g.forward_push(int(live[0]), ALPHA, 1e-4, fetch=False)
            with pkg.QueryStream(g, 0.5, ALPHA, k=4):
                for call in (g.reserve_sparse, g.residue_sparse, lambda **kw: store.fetch_sparse(0, **kw),
                             store.fetch_sparse_all):
                    for kw in (dict(), dict(order="value", cap=3), dict(cap=0)):
                        with pytest.raises(pkg.PprhipError) as e:
                            call(**kw)
                        assert e.value.code == pkg.ERR_STATE
            g.forward_push(int(live[0]), ALPHA, 1e-4, fetch=False)
            assert g.reserve_sparse(cap=0)[2] > 0 and store.fetch_sparse_all(cap=0)[3] > 0
        finally:
            store.close()


def full_support_push(g):
    g.forward_push_seeds(np.arange(g.n, dtype=np.int32)[np.r_[0, 3:g.n]], ALPHA, 1e-12, fetch=False)


def test_release_returns_the_workspace(pkg):
    """By value over a full support of n = 2^18 + 3: 36 bytes per kept entry (include/pprhip.h), 9 MB."""
    with pkg.Graph(cycle_and_isolated(pkg), device=0) as g:
        full_support_push(g)
        x = g.reserve()
        free0, _ = g.device_memory()
        first = g.reserve_sparse(order="value")
        assert first[2] == g.n
        free1, _ = g.device_memory()
        assert free0 - free1 >= 36 * g.n, "the workspace took %d bytes" % (free0 - free1)
        g.release(g.RELEASE_SPARSE)
        free2, _ = g.device_memory()
        assert free2 - free1 >= 36 * g.n, "release gave %d bytes back" % (free2 - free1)
        g.release(pkg.RELEASE_SPARSE)   # nothing to release: a no-op
        with pytest.raises(pkg.PprhipError) as e:
            g.release(32)
        assert e.value.code == pkg.ERR_INVALID
        again = g.reserve_sparse(order="value")
        assert again[2] == first[2] and np.array_equal(again[0], first[0]) and same_bits(again[1], first[1])
        same(again, *sparse_ref(x, 0.0, BY_VALUE))
        assert same_bits(g.reserve(), x)


def test_closed_handles_leave_no_bytes(pkg, rmat12):
    host = cycle_and_isolated(pkg)

    def one_life():
        with pkg.Graph(host, device=0) as g:
            full_support_push(g)
            assert g.reserve_sparse(order="value", cap=4)[2] == host.n
            assert g.residue_sparse(cap=0)[2] >= 0
            store = pkg.Results(g, 2)
            assert store.fetch_sparse_all()[3] == 0
            store.close()
        gc.collect()

    with pkg.Graph(rmat12, device=0) as probe:   # a small handle that stays: pprhip_device_memory needs one
        one_life()
        one_life()
        free0, _ = probe.device_memory()
        for _ in range(4):
            one_life()
        free1, _ = probe.device_memory()
    print("four more lives: device %+.1f MB" % ((free0 - free1) / 1e6))
    assert free0 - free1 <= 16 << 20, "device memory not returned: %.1f MB after four more lives" % ((free0 - free1) / 1e6)
