"""Single-target PPR on the device (pprhip_ppr_targets; include/pprhip.h "single targets", DESIGN.md §2 "Single
targets"): the deterministic bound 0 <= pi - value <= rmax against the exact solve, every vector against its own parts
(backward push, survival), invariance of a target's vector under the call it is in, weighted target sets and the start
kernel's tile edges, top-k / result store / delivery, arguments and state."""
import ctypes as C

import numpy as np
import pytest

from conftest import shared_graph
from targets_ref import ppr_exact, set_exact, topk_rows, topk_rule

pytestmark = pytest.mark.gpu
A = 0.15
SLACK = 1e-12  # rounding of the dense solve and of the push's fp64 sums


# ------------------------------------------------------------------ fixtures
@pytest.fixture
def dev_got(pkg, got, dev_cache):
    return shared_graph(dev_cache, pkg, "got", lambda: pkg.Graph(got))


@pytest.fixture
def dev_r12(pkg, rmat12, dev_cache):
    return shared_graph(dev_cache, pkg, "r12", lambda: pkg.Graph(rmat12))


@pytest.fixture(scope="module")
def exact_cache():
    """Dense exact solves, one per (graph, alpha) and module."""
    return {}


def exact(cache, name, host, alpha):
    key = (name, alpha)
    if key not in cache:
        cache[key] = ppr_exact(host, alpha)
    return cache[key]


def hub_and_no_in(host):
    """The largest in-degree node and the first node without in-edges (but with out-edges)."""
    od, idg = np.diff(host.out_rp.astype(np.int64)), np.diff(host.in_rp.astype(np.int64))
    return int(np.argmax(idg)), int(np.flatnonzero((idg == 0) & (od > 0))[0])


def special_targets(host, rng, count):
    """`count` targets that include the largest in-degree node, a node without in-edges (but with out-edges), a dead
    end, a node with a self loop and an isolated node."""
    od, idg = np.diff(host.out_rp.astype(np.int64)), np.diff(host.in_rp.astype(np.int64))
    loops = [u for u in range(host.n) if u in host.out_ci[int(host.out_rp[u]):int(host.out_rp[u + 1])]]
    picks = [*hub_and_no_in(host), int(np.flatnonzero((od == 0) & (idg > 0))[0]),
             int(loops[0]), int(np.flatnonzero((od == 0) & (idg == 0))[0])]
    rest = [int(v) for v in rng.permutation(host.n) if int(v) not in picks][:count - len(picks)]
    return np.array(picks + rest, dtype=np.int32), picks


def assert_bound(values, ref, rmax, what):
    """values[i, s] against ref[s, i]: -1e-12 <= exact - value <= rmax + 1e-12 for all (s, t)."""
    gap = ref.T - values
    print(what, "min gap %.3e max gap %.3e (rmax %.1e)" % (gap.min(), gap.max(), rmax))
    assert gap.min() >= -SLACK and gap.max() <= rmax + SLACK, (what, gap.min(), gap.max())


# ------------------------------------------------------------------ 1. the bound against the exact solve
@pytest.mark.parametrize("alpha", [0.05, 0.15, 0.5])
def test_bound_every_got_target(pkg, got, dev_got, exact_cache, alpha):
    pi = exact(exact_cache, "got", got, alpha)
    dev_got.set_tuning(pkg.tuning_default())
    for rmax in (1e-2, 1e-5):
        values, _, st, pq = dev_got.ppr_targets(np.arange(got.n), alpha, rmax)
        assert values.shape == (got.n, got.n) and len(pq) == got.n
        assert_bound(values, pi, rmax, ("got", alpha, rmax))
        assert st.rmax_final == rmax and st.rounds == got.n and st.walks == 0 and st.walk_steps == 0
        assert all(s.rounds == 1 and s.rmax_final == rmax for s in pq)
        assert st.pops == sum(s.pops for s in pq) and st.levels == sum(s.levels for s in pq)


@pytest.mark.parametrize("alpha", [0.05, 0.15, 0.5])
def test_bound_rmat12_special_targets(pkg, rmat12, dev_r12, exact_cache, alpha):
    pi = exact(exact_cache, "r12", rmat12, alpha)
    targets, picks = special_targets(rmat12, np.random.default_rng(12), 64)
    assert targets.size == 64 and len(set(picks)) == 5
    dev_r12.set_tuning(pkg.tuning_default())
    for rmax in (1e-2, 1e-5):
        values, _, _, _ = dev_r12.ppr_targets(targets, alpha, rmax)
        assert_bound(values, pi[:, targets], rmax, ("rmat12", alpha, rmax))


# ------------------------------------------------------------------ 2. equals its parts
def test_targets_equal_their_parts(pkg, rmat12, dev_r12):
    g, host = dev_r12, rmat12
    g.set_tuning(pkg.tuning_default())
    targets, _ = special_targets(host, np.random.default_rng(5), 24)
    idg = np.diff(host.in_rp.astype(np.int64))
    rmax = 1e-4
    values, _, _, pq = g.ppr_targets(targets, A, rmax)
    S = g.walk_survival(A)
    seen = set()
    for i, t in enumerate(targets):
        if idg[t] > 0:
            p, _, _ = g.backward_push(int(t), A, rmax)
            assert np.allclose(values[i] * S, p, rtol=1e-12, atol=0), t
            assert pq[i].pops > 0 and pq[i].levels > 0
            seen.add("in")
        else:  # the definition, not Backward_Search.java:46-49: p(t) = alpha, nothing else
            ref = np.zeros(host.n)
            ref[t] = A / S[t]
            assert np.array_equal(values[i], ref), t
            assert pq[i].pops == 0 and pq[i].levels == 0
            seen.add("noin")
    assert seen == {"in", "noin"}


def test_backward_kinds_share_their_push(pkg, got, dev_got, rmat12, dev_r12, monkeypatch):
    """The backward kinds share their push and differ only at a target without in-edges.  For a target without in-edges,
    the hub and an ordinary target of each graph: (a) backward_push(t), (b) all_pair_backward over [t, t + 1) started at
    tier 3, a kBackward job on the batch slots, (c) ppr_targets([t]) multiplied back by the survival vector.  With
    in-edges (b) holds (a)'s reserve entries at or above the threshold and (c) * S is (a)'s reserve, both to the
    tolerance of test_targets_equal_their_parts; without, (a) and (b) hold reserve(t) = 1.0 (Backward_Search.java:46-49)
    and (c) holds alpha / S(t), and nothing else.  That is the exact statement after the kernel's division; "(c) * S is
    exactly alpha" is asserted as |value * S(t) - alpha| <= 2^-52 alpha, a rounding for the division and one for the
    product.  (Pairs: test_pairs_equal_host_recomputation_from_parts.)"""
    rmax, rtol = 1e-4, 1e-12
    for g, host in ((dev_got, got), (dev_r12, rmat12)):
        g.set_tuning(pkg.tuning_default())
        idg = np.diff(host.in_rp.astype(np.int64))
        picks = list(hub_and_no_in(host))  # (special_targets' first two; GOT has neither a self loop nor an isolated node)
        picks.append(next(int(v) for v in np.random.default_rng(12).permutation(host.n)
                          if int(v) not in picks and idg[v] > 0))
        S = g.walk_survival(A)
        for t in picks:
            p, r, _ = g.backward_push(t, A, rmax)
            monkeypatch.setenv("PPRHIP_APBS_TIER", "3")
            ix, st = g.all_pair_backward(A, rmax, -1, t_begin=t, t_end=t + 1)
            monkeypatch.delenv("PPRHIP_APBS_TIER")
            off, tg, vl = ix.arrays()
            ix.close()
            assert st.dense_nodes == 1 and np.all(tg == t) and np.all(np.diff(off) <= 1)  # the batch tier; one target
            entries = np.zeros(host.n)
            entries[np.flatnonzero(np.diff(off))] = vl
            values, _, _, pq = g.ppr_targets([t], A, rmax)
            if idg[t] > 0:
                held = entries > 0
                assert np.allclose(entries[held], p[held], rtol=rtol, atol=0), t
                assert np.all(p[held] >= rmax * (1 - rtol)) and np.all(held[p >= rmax * (1 + rtol)]), t
                assert np.allclose(values[0] * S, p, rtol=rtol, atol=0), t
                assert pq[0].pops > 0
            else:
                e_t = np.zeros(host.n)
                e_t[t] = 1.0
                assert np.array_equal(p, e_t) and not r.any(), t
                assert np.array_equal(entries, e_t), t
                assert np.array_equal(values[0], A / S[t] * e_t), t  # alpha, divided by S(t) once ...
                assert abs(values[0][t] * S[t] - A) <= 2.0 ** -52 * A  # ... and multiplied back: a rounding each
                assert pq[0].pops == 0 and pq[0].levels == 0


# ------------------------------------------------------------------ 3. batch invariance
def _invariance_case(g, host, rmax):
    idg = np.diff(host.in_rp.astype(np.int64))
    hubs = np.argsort(-idg)[:34].astype(np.int32)
    pool = np.concatenate([hubs, hubs[:6]])  # 40 targets, six of them twice
    alone = {}
    for t in np.unique(pool):
        v, _, _, pq = g.ppr_targets([t], A, rmax)
        alone[int(t)] = (v[0], pq[0])
    dense = 0
    for q in (1, 16, 17, 40):
        values, _, st, pq = g.ppr_targets(pool[:q] if q < 40 else pool, A, rmax)
        dense += st.dense_levels
        for i in range(q):
            ref, sref = alone[int(pool[i])]
            assert np.allclose(values[i], ref, rtol=1e-12, atol=0), (q, i)
            assert pq[i].levels == sref.levels and pq[i].pops == sref.pops, (q, i)
    return dense


def test_targets_batch_invariance(pkg, rmat12, dev_r12, monkeypatch):
    g = dev_r12
    g.set_tuning(pkg.tuning_default())
    _invariance_case(g, rmat12, 1e-4)
    monkeypatch.setenv("PPRHIP_BATCH_THREADS", "0")  # the single-thread driver
    _invariance_case(g, rmat12, 1e-4)
    monkeypatch.delenv("PPRHIP_BATCH_THREADS")
    t_ = pkg.tuning_batch()
    t_.dense_frac = 0.002  # the dense tuning of test_pairs_equal_parts_under_a_dense_tuning: shared dense levels run
    g.set_tuning(t_)
    try:
        assert _invariance_case(g, rmat12, 1e-4) > 0
    finally:
        g.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 4. target sets
def test_sets_reduce_sum_and_scale(pkg, rmat12, dev_r12, exact_cache):
    g, host = dev_r12, rmat12
    g.set_tuning(pkg.tuning_default())
    pi = exact(exact_cache, "r12", host, A)
    idg = np.diff(host.in_rp.astype(np.int64))
    a, b = (int(v) for v in np.argsort(-idg)[:2])
    noin = int(np.flatnonzero(idg == 0)[0])
    rmax = 1e-4
    single, _, _, pqs = g.ppr_targets([a, noin], A, rmax)
    # a set of one with weight 1 is the single target
    one, _, _, pq1 = g.ppr_target_sets([[a], [noin]], A, rmax, weights=[[1.0], None])
    assert np.allclose(one, single, rtol=1e-12, atol=0)
    assert [s.pops for s in pq1] == [s.pops for s in pqs] and [s.levels for s in pq1] == [s.levels for s in pqs]
    # duplicates sum
    dup, _, _, _ = g.ppr_target_sets([[a, b, a], [a, b]], A, rmax, weights=[[0.5, 1.0, 0.5], [1.0, 1.0]])
    assert np.allclose(dup[0], dup[1], rtol=1e-12, atol=0)
    assert_bound(dup[:1], set_exact(pi, [a, b])[:, None], rmax, "duplicates")
    # weights are not normalized: {a} at weight 2 is twice {a} at rmax / 2, up to the bound
    two, _, _, _ = g.ppr_target_sets([[a]], A, rmax, weights=[[2.0]])
    half, _, _, _ = g.ppr_targets([a], A, rmax / 2)
    assert np.max(np.abs(two[0] - 2.0 * half[0])) <= rmax + SLACK
    assert_bound(two, 2.0 * pi[:, [a]], rmax, "weight 2")


def test_sets_within_the_bound(pkg, rmat12, dev_r12, exact_cache):
    g, host = dev_r12, rmat12
    g.set_tuning(pkg.tuning_default())
    pi = exact(exact_cache, "r12", host, A)
    rng = np.random.default_rng(41)
    big = rng.choice(host.n, 300, replace=False)
    rmax = 1e-4
    hub = int(np.argmax(np.diff(host.in_rp)))
    mixed = np.array([hub, int(big[0]), int(big[1])])
    mixed_w = np.array([1.0, rmax / 4, rmax])  # two members at or below the threshold: they start as residue
    sets = [big, big, mixed]
    weights = [None, np.full(300, 1.0 / 300), mixed_w]
    values, _, st, pq = g.ppr_target_sets(sets, A, rmax, weights=weights)
    refs = np.stack([set_exact(pi, big), set_exact(pi, big, weights[1]), set_exact(pi, mixed, mixed_w)], axis=1)
    assert_bound(values, refs, rmax, "sets")
    # every member of the uniform set at rmax 1e-2 lies below the threshold: only members without in-edges move
    low, _, _, pql = g.ppr_target_sets([big], A, 1e-2, weights=[np.full(300, 1.0 / 300)])
    assert pql[0].pops == 0
    assert_bound(low, refs[:, 1:2], 1e-2, "all below")


@pytest.mark.parametrize("size", [1, 63, 64, 65, 2049])
def test_set_sizes_at_tile_and_wave_edges(pkg, rmat12, dev_r12, exact_cache, size):
    g, host = dev_r12, rmat12
    g.set_tuning(pkg.tuning_default())
    pi = exact(exact_cache, "r12", host, A)
    rng = np.random.default_rng(size)
    members = rng.choice(host.n, size, replace=False)
    w = rng.uniform(0.5, 1.5, size)
    values, _, _, _ = g.ppr_target_sets([members], A, 1e-9, weights=[w])
    assert_bound(values, set_exact(pi, members, w)[:, None], 1e-9, ("size", size))


# ------------------------------------------------------------------ 5. top-k, store, delivery
def test_topk_store_and_delivery(pkg, got, dev_got, toy_graphs):
    g = dev_got
    g.set_tuning(pkg.tuning_default())
    n = got.n
    targets = np.argsort(-np.diff(got.in_rp.astype(np.int64)))[:20].astype(np.int32)
    rmax = 1e-5
    for k in (1, 8, n + 5):
        store = pkg.Results(g, 20)
        try:
            values, (ids, vals, nsel), _, _ = g.ppr_targets(targets, A, rmax, k=k, keep=store)
            for i in range(20):
                cnt, row_i, row_v = topk_rows(values[i], k)
                assert nsel[i] == cnt and np.array_equal(ids[i], row_i) and np.array_equal(vals[i], row_v), (k, i)
                assert np.array_equal(store.fetch(i), values[i]), (k, i)
            none, (ids2, vals2, nsel2), _, _ = g.ppr_targets(targets, A, rmax, k=k, fetch=False)
            assert none is None and np.array_equal(nsel2, nsel)
            assert np.array_equal(ids2, ids) and np.allclose(vals2, vals, rtol=1e-12, atol=0)
            # a kept slot serves a sweep cut like any stored vector
            assert store.sweep_cut(0, cap=0)[3].support == np.count_nonzero(values[0])
        finally:
            store.close()
    # ties: every leaf of the star is its own only source, so the set of all leaves ties five ways at the top
    star = toy_graphs["star_dead_leaves"]
    with pkg.Graph(star) as gs:
        values, (ids, vals, nsel), _, _ = gs.ppr_target_sets([[1, 2, 3, 4, 5]], A, 1e-6, k=2)
        cnt, row_i, row_v = topk_rows(values[0], 2)
        assert cnt == 5 and nsel[0] == 5 and np.array_equal(ids[0], row_i) and np.array_equal(vals[0], row_v)
        assert list(topk_rule(values[0], 2)[1]) == [1, 2, 3, 4, 5] and np.all(values[0][1:] == 1.0)
        assert 0.0 < values[0][0] < 1.0


# ------------------------------------------------------------------ 6. arguments and state
def _raw(pkg, g, targets, weights, offsets, q, alpha, rmax, k=0, with_topk_buffers=True):
    L = pkg.lib()
    t = None if targets is None else np.ascontiguousarray(targets, dtype=np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    o = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    ids = np.zeros(max(1, abs(q) * max(k, 1)), dtype=np.int32) if with_topk_buffers else None
    vals = np.zeros(max(1, abs(q) * max(k, 1))) if with_topk_buffers else None
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    st = pkg.Stats()
    rc = L.pprhip_ppr_targets(g.h, ptr(t), ptr(w), ptr(o), q, alpha, rmax, None, None, k, ptr(ids), ptr(vals), None, None,
                              C.byref(st))
    return rc, L.pprhip_last_error().decode()


def test_refusals_name_the_set_and_leave_the_handle(pkg, got, dev_got):
    g, n = dev_got, got.n
    src = int(np.argmax(np.diff(got.out_rp)))
    before, _, _, _ = g.forward_push(src, A, 1e-6)
    nan, inf = float("nan"), float("inf")
    per_set = [  # (targets, weights, offsets, the set the message names)
        ([0, 1, n], None, [0, 2, 3], 1), ([0, -1, 2], None, [0, 1, 2, 3], 1), ([0, 1, 2], [1, 1, -0.5], [0, 1, 3], 1),
        ([0, 1, 2], [1, nan, 1], [0, 1, 2, 3], 1), ([0, 1, 2], [1, 1, inf], [0, 1, 2, 3], 2),
        ([0, 1, 2], [1, 0, 0], [0, 1, 3], 1), ([0, 1, 2], None, [0, 2, 2, 3], 1), ([0, 1, 2], None, [0, 2, 1, 3], 1),
    ]
    for t, w, o, bad in per_set:
        rc, msg = _raw(pkg, g, t, w, o, len(o) - 1, A, 1e-4)
        assert rc == pkg.ERR_INVALID and "set %d" % bad in msg, (t, w, o, msg)
    rc, msg = _raw(pkg, g, [0, n + 3, 1], None, None, 3, A, 1e-4)  # single targets: set i = {targets[i]}
    assert rc == pkg.ERR_INVALID and "set 1" in msg
    whole_call = [
        dict(targets=[0, 1], weights=None, offsets=[1, 2], q=1, alpha=A, rmax=1e-4),            # offsets[0] != 0
        dict(targets=[0], weights=None, offsets=None, q=-1, alpha=A, rmax=1e-4),
        dict(targets=[0], weights=None, offsets=None, q=1, alpha=A, rmax=1e-4, k=-1),
        dict(targets=[0], weights=None, offsets=None, q=1, alpha=A, rmax=1e-4, k=4, with_topk_buffers=False),
        dict(targets=None, weights=None, offsets=None, q=1, alpha=A, rmax=1e-4),
    ]
    whole_call += [dict(targets=[0], weights=None, offsets=None, q=1, alpha=A, rmax=r) for r in (0.0, -1e-3, 1.5, nan, inf)]
    whole_call += [dict(targets=[0], weights=None, offsets=None, q=1, alpha=a, rmax=1e-4) for a in (0.0, 1.0, -0.1, nan)]
    for kw in whole_call:
        rc, msg = _raw(pkg, g, kw.pop("targets"), kw.pop("weights"), kw.pop("offsets"), kw.pop("q"), kw.pop("alpha"),
                       kw.pop("rmax"), **kw)
        assert rc == pkg.ERR_INVALID and "pprhip_ppr_targets" in msg, msg
    assert np.array_equal(g.reserve(), before)  # nothing ran: the result before is still there
    rc, _ = _raw(pkg, g, None, None, None, 0, A, 1e-4)  # an empty call
    assert rc == pkg.OK
    values, sel, st, pq = g.ppr_targets(np.zeros(0, dtype=np.int32), A, 1e-4, k=3)
    assert values.shape == (0, n) and sel[0].shape == (0, 3) and pq == [] and st.pops == 0


def test_targets_refused_while_a_stream_is_open(pkg, dev_got):
    qs = pkg.QueryStream(dev_got, 0.5, A)
    try:
        with pytest.raises(pkg.PprhipError) as e:
            dev_got.ppr_targets([0], A, 1e-4)
        assert e.value.code == pkg.ERR_STATE
    finally:
        qs.close()


def test_other_paths_unchanged_after_a_target_call(pkg, got):
    src = int(np.argmax(np.diff(got.out_rp)))

    def run(g):
        f, _ = g.fora_single_source(src, 0.5, A, seed=3)
        pv, _ = g.ppr_pairs(np.arange(30), np.arange(30)[::-1], 0.5, A, 9)
        g.forward_push(src, A, 1e-7, fetch=False)
        sw = g.sweep_cut(cap=0)[3]
        return f, pv, np.array([sw.support, sw.best_size, sw.best_cut, sw.best_vol], dtype=np.int64)

    with pkg.Graph(got) as g:
        ref = run(g)
        g.ppr_targets(np.arange(40), A, 1e-5, k=4)
        g.ppr_target_sets([np.arange(100), [5, 6]], A, 1e-5)
        again = run(g)
    # (the same computation twice; walks and pushes add with fp64 atomics, so the bits may differ in the last places)
    for a, b in zip(ref, again):
        if a.dtype.kind == "f":
            assert np.allclose(a, b, rtol=1e-12, atol=1e-15)
        else:
            assert np.array_equal(a, b)


def test_targets_memory_steady(pkg, rmat12, dev_r12):
    g = dev_r12
    g.set_tuning(pkg.tuning_default())
    rng = np.random.default_rng(1)
    t = rng.integers(0, rmat12.n, 48)
    sets = [rng.integers(0, rmat12.n, 70) for _ in range(20)]
    g.ppr_targets(t, A, 1e-4, k=8)
    g.ppr_target_sets(sets, A, 1e-4, fetch=False, k=8)
    free0, _ = g.device_memory()
    for i in range(20):
        if i % 2:
            g.ppr_targets(t, A, 1e-4, k=8)
        else:
            g.ppr_target_sets(sets, A, 1e-4, fetch=False, k=8)
    free1, _ = g.device_memory()
    assert free1 == free0
