"""Batched weighted targets on the GPU (include/pprhip.h "weighted relationships", the backward direction;
csrc/weighted_bwd_batch.cpp): a pprhip_weighted_ppr_targets call of two or more queries runs 16 in flight, the queries
at a dense level sharing one sweep.  Query i takes the decisions of the call of that one query (which keeps the serial
path) and of the numpy reference tests/weighted_bwd_ref.py; the sweeps are the host model's
(tests/weighted_bwd_batch_ref.py).  1e-12 is the project's bar for "same arithmetic, other addition order".  Levels and
pops are compared for every query: tests/test_weighted_bwd_batch_ref.py pins that no input here puts a value closer
to rmax than 1e-9 (relative), and the tests assert it again."""
import numpy as np
import pytest

import targets_ref
import weighted_bwd_batch_ref as bb
import weighted_bwd_ref as br
from conftest import shared_graph
from test_gpu_weighted_backward import _rmat_targets
from weighted_bwd_designs import design_weights, reversed_dense_design

ALPHA = 0.15
TOL = 1e-12
EPS = 0.5
pytestmark = pytest.mark.gpu

ALL_SPARSE, ALL_DENSE = 1e9, 1e-12  # dense_frac: no level reaches it / every level does
SIZES = (2, 3, 15, 16, 17, 40)


def _indeg(host):
    return np.diff(host.in_rp.astype(np.int64))


def _outdeg(host):
    return np.diff(host.out_rp.astype(np.int64))


def _rand_w(host, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, host.m)


def _frac(name, host, mode):
    """dense_frac of a tuning: no level dense, every level dense, or mixed - 0.25 on R-MAT 12 (the pinned case); on the
    others the rule of tests/test_gpu_weighted_batch.py mirrored for a backward push: the largest in-degree target's
    first level (1 node + d in-edges) just below the threshold, wider levels above."""
    if mode == "sparse":
        return ALL_SPARSE
    if mode == "dense":
        return ALL_DENSE
    if mode == "default":
        return None
    return 0.25 if name == "rmat12" else (int(_indeg(host).max()) + 1.5) / host.m


def _graph(dev_cache, pkg, name, host, w, dense_frac=None):
    g = shared_graph(dev_cache, pkg, name, lambda: pkg.Graph(host, device=0))
    t = pkg.tuning_default()
    if dense_frac is not None:
        t.dense_frac = dense_frac
    g.set_tuning(t)
    g.set_weights(w)
    return g


_S = {}


def _survival(name, host, w):
    if name not in _S:
        _S[name] = (w.copy(), br.survival_exact(host, w, ALPHA))
    assert np.array_equal(_S[name][0], w)
    return _S[name][1]


_ONE = {}


def _one(g, key, ids, sw, rmax):
    """The call of one query (the serial path) under the tuning `key` names, run once per module: (vector, Stats)."""
    k = (key, tuple(int(x) for x in np.atleast_1d(ids)), None if sw is None else tuple(float(x) for x in sw), rmax)
    if k not in _ONE:
        if sw is None and np.ndim(ids) == 0:
            v, _, _, pq = g.weighted_ppr_targets([int(ids)], ALPHA, rmax)
        else:
            v, _, _, pq = g.weighted_ppr_target_sets([ids], ALPHA, rmax, weights=None if sw is None else [sw])
        assert pq[0].class_launches[5] == 0  # the call of one shares no sweep
        _ONE[k] = (v[0], pq[0])
    return _ONE[k]


def _check_query(tag, name, host, w, g, key, ids, sw, rmax, value, st, mode):
    """Query (ids, sw) of a batched call against its call of one and against bpush_sync / S_w."""
    single = np.ndim(ids) == 0
    rkey = (name, int(ids)) if single else (name, tuple(int(x) for x in ids), tuple(float(x) for x in sw))
    ref_p, levels, pops, margin, _ = bb.push_ref(rkey, host, w, int(ids) if single else ids, sw, ALPHA, rmax)
    # Single targets: no value next to rmax, asserted.  The sets hold members whose weight IS rmax (the same double on
    # both sides of the comparison, which the margin cannot tell from a near miss): their levels are compared with the
    # reference's where the margin allows, as tests/test_gpu_weighted_backward.py does, and with the call of one's always.
    assert margin >= bb.MARGIN or not single, ("the inputs put a value next to rmax", tag, margin)
    alone, st1 = _one(g, key, ids, sw, rmax)
    S = _survival(name, host, w)
    e1, e2 = float(np.max(np.abs(value - alone))), float(np.max(np.abs(value - ref_p / S)))
    assert e1 <= TOL and e2 <= TOL, (tag, e1, e2)
    if margin >= bb.MARGIN:
        assert st.levels == levels and st.pops + st.dense_nodes == pops, (tag, st.levels, levels, st.pops, st.dense_nodes, pops)
    assert (st.levels, st.dense_levels, st.pops, st.dense_nodes, st.enqueues) == \
        (st1.levels, st1.dense_levels, st1.pops, st1.dense_nodes, st1.enqueues), tag
    assert st.rounds == 1 and st.rmax_final == rmax and st.push_ms >= 0.0 and st.total_ms >= st.push_ms
    if mode == "dense":
        assert st.dense_levels == st.levels, tag
    if mode == "sparse":
        assert st.dense_levels == 0, tag


# ---------------------------------------------------------------------------------------------- 1. query i is the call of one
def _case(pkg, got, rmat12, name):
    if name == "got":
        return got, _rand_w(got, 21), list(range(got.n)), (1e-3, 1e-6)
    if name == "rmat12":
        return rmat12, _rand_w(rmat12, 22), [int(t) for t in _rmat_targets(rmat12)], (1e-4,)
    host, d = reversed_dense_design(pkg)
    pool = [d["pool"][0], d["pool"][511], d["pool"][512], d["pool"][1099], d["A"], d["B"], d["C"], d["Z"], d["small"][3],
            d["isolated"]]
    return host, design_weights(host, 43), pool, (1e-7,)


@pytest.mark.parametrize("mode", ["sparse", "dense", "mixed"])
@pytest.mark.parametrize("name", ["got", "rmat12", "rdense"])
def test_query_i_is_the_call_of_one(pkg, dev_cache, got, rmat12, name, mode):
    """Calls of 2, 3, 15, 16, 17 and 40 targets (the pool cycled from where the call before stopped; GOT also in one
    call of all its targets): every vector, level count and pop count is the call of one's and the reference's."""
    host, w, pool, rmaxes = _case(pkg, got, rmat12, name)
    g = _graph(dev_cache, pkg, name, host, w, _frac(name, host, mode))
    key = (name, mode)
    for rmax in rmaxes:
        at = 0
        for q in SIZES + ((len(pool),) if name == "got" else ()):
            targets = [pool[(at + i) % len(pool)] for i in range(q)]
            at += q
            values, _, st, pq = g.weighted_ppr_targets(targets, ALPHA, rmax)
            assert len(pq) == q and st.rmax_final == rmax
            for i, t in enumerate(targets):
                _check_query((name, mode, rmax, q, i, t), name, host, w, g, key, np.int64(t), None, rmax, values[i], pq[i], mode)
            assert st.levels == sum(s.levels for s in pq) and st.dense_levels == sum(s.dense_levels for s in pq)
            if mode == "sparse":
                assert st.class_launches[5] == 0, (name, rmax, q)
            if mode == "dense" and st.levels:
                # the shared sweep ran: fails on a build that runs the weighted targets one after another
                assert st.class_launches[5] > 0, (name, rmax, q)
                assert st.class_launches[5] <= st.dense_levels


# ---------------------------------------------------------------------------------------------- 2. sweep counts
def test_sweep_counts_are_the_host_models(pkg, dev_cache, rmat12, monkeypatch):
    """R-MAT 12, the 64 targets, dense_frac 0.25, rmax 1e-4: 36 sweeps with 16 workspaces, 104 on a fresh handle under
    PPRHIP_BATCH_WORKSPACES=4 (the forward driver's rule would run 55 and 180), the same vectors."""
    host, w, rmax = rmat12, _rand_w(rmat12, 22), 1e-4
    targets = _rmat_targets(host)
    kinds = []
    for t in targets:
        _, levels, _, margin, trace = bb.push_ref(("rmat12", int(t)), host, w, int(t), None, ALPHA, rmax)
        assert margin >= bb.MARGIN
        kinds.append(bb.kinds_of(trace, host, 0.25))
    want16, want4 = bb.lockstep_sweeps(kinds, 16), bb.lockstep_sweeps(kinds, 4)
    assert (want16, want4) == (36, 104)
    g = _graph(dev_cache, pkg, "rmat12", host, w, 0.25)
    full, _, st, pq = g.weighted_ppr_targets(targets, ALPHA, rmax)
    print("16 workspaces: %d sweeps for %d dense levels" % (st.class_launches[5], st.dense_levels))
    assert st.class_launches[5] == want16 and st.dense_levels == sum(sum(k) for k in kinds)
    assert [s.dense_levels for s in pq] == [sum(k) for k in kinds]
    monkeypatch.setenv("PPRHIP_BATCH_WORKSPACES", "4")
    with pkg.Graph(host, device=0) as g4:
        t = pkg.tuning_default()
        t.dense_frac = 0.25
        g4.set_tuning(t)
        g4.set_weights(w)
        out, _, st4, pq4 = g4.weighted_ppr_targets(targets, ALPHA, rmax)
    err = float(np.max(np.abs(out - full)))
    print("4 workspaces against 16: max |diff| %.2e, sweeps %d" % (err, st4.class_launches[5]))
    assert st4.class_launches[5] == want4 and err <= TOL
    assert [(s.levels, s.dense_levels) for s in pq4] == [(s.levels, s.dense_levels) for s in pq]


# ---------------------------------------------------------------------------------------------- 3. sets and leftovers
def _check_sets(tag, name, host, w, g, key, sets, ws, rmax, mode):
    values, _, st, pq = g.weighted_ppr_target_sets(sets, ALPHA, rmax, weights=ws)
    for i, (ids, sw) in enumerate(zip(sets, ws)):
        if len(ids) == 1 and sw[0] == 1.0:
            ids, sw = np.int64(ids[0]), None
        _check_query((tag, i), name, host, w, g, key, ids, sw, rmax, values[i], pq[i], mode)
    return st


@pytest.mark.parametrize("mode", ["default", "dense"])
def test_sets_and_single_targets_in_one_call(pkg, dev_cache, got, rmat12, mode):
    """GOT: weights, duplicates, zero weights, members at or below rmax, members without in-edges, with single targets
    between the sets.  R-MAT 12: sets of 2 047 / 2 048 / 2 049 members (the start kernel's tile edge), singles between."""
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w, _frac("got", got, mode))
    rmax = 1e-3
    lone = np.flatnonzero(_indeg(got) == 0)
    dead = np.flatnonzero((_outdeg(got) == 0) & (_indeg(got) > 0))
    sets = [[3, 5, 3, 9], [int(np.argmax(_indeg(got)))], [1, 2, 4], [int(lone[0])], [int(lone[0]), 7, int(lone[-1])],
            [int(dead[0])] if dead.size else [11], list(range(40)), [17]]
    ws = [[0.5, 1.0, 0.25, 2.0], [1.0], [1.0, 0.0, rmax], [1.0], [0.7, rmax * 0.5, 1.3], [1.0], np.linspace(0.1, 1.0, 40),
          [1.0]]
    st = _check_sets(("got", mode), "got", got, w, g, ("got", mode), sets, ws, rmax, mode)
    assert mode != "dense" or st.class_launches[5] > 0
    host, w12 = rmat12, _rand_w(rmat12, 22)
    g12 = _graph(dev_cache, pkg, "rmat12", host, w12, _frac("rmat12", host, mode))
    perm = np.random.default_rng(12).permutation(host.n)
    sets, ws = [], []
    for size in (2047, 2048, 2049):
        sets += [perm[:size], [int(perm[size])]]
        ws += [np.random.default_rng(size).uniform(0.0, 2e-4, size), [1.0]]  # about half the members at or below rmax
    st = _check_sets(("rmat12", mode), "rmat12", host, w12, g12, ("rmat12", mode), sets, ws, 1e-4, mode)
    assert mode != "dense" or st.class_launches[5] > 0


def test_a_refilled_column_inherits_nothing(pkg, dev_cache):
    """The reversed dense design, every level dense, 33 queries: the first 16 are the pool as a weighted set and
    dead-end targets - members without out-edges, which enter a column through the scatter and are never rewritten by
    a sweep - the next 17, which take over their columns, are A, B, C, Z and small nodes."""
    host, d = reversed_dense_design(pkg)
    w = design_weights(host, 43)
    g = _graph(dev_cache, pkg, "rdense", host, w, ALL_DENSE)
    pool = np.array(d["pool"])
    assert (_outdeg(host)[pool] == 0).all() and (_indeg(host)[pool] > 0).all()
    sw = np.random.default_rng(44).uniform(0.2, 1.0, pool.size)
    first = [(pool, sw)] + [([int(p)], [1.0]) for p in pool[[0, 1, 2, 510, 511, 512, 513, 1023, 1024, 1098, 1099, 7, 77, 777, 999]]]
    later = [([d[k]], [1.0]) for k in "ABCZ"] + [([int(s)], [1.0]) for s in d["small"][:13]]
    assert len(first) == 16 and len(later) == 17
    sets, ws = [x[0] for x in first + later], [x[1] for x in first + later]
    st = _check_sets("rdense", "rdense", host, w, g, ("rdense", "dense"), sets, ws, 1e-7, "dense")
    assert st.class_launches[5] > 0


def test_calls_of_other_kinds_leave_nothing_behind(pkg, rmat12):
    """weighted_fora_batch, weighted_ppr_targets, ppr_targets, weighted_ppr_targets on one handle, every call with
    shared sweeps: the two weighted target calls agree, the unweighted one is a fresh handle's; then a batched FORA call
    (forward sweeps behind backward ones) is a fresh handle's as well."""
    host, w = rmat12, _rand_w(rmat12, 22)
    targets = _rmat_targets(host)[:24]
    srcs = [int(np.argmax(_outdeg(host))), 1, 2, 3, 5, 8]
    tun = pkg.tuning_batch()  # dense levels from 2 % of m

    def unweighted(g):
        v, _, st, _ = g.ppr_targets(targets, ALPHA, 1e-4)
        out, _, _, _, _, bst = g.fora_batch_single_source(srcs, EPS, ALPHA, seed=3, fetch=True)
        print("unweighted sweeps: targets %d, FORA %d" % (st.class_launches[5], bst.class_launches[5]))
        assert bst.class_launches[5] > 0
        return v, out

    with pkg.Graph(host, device=0) as g, pkg.Graph(host, device=0) as fresh:
        for x in (g, fresh):
            x.set_tuning(tun)
        g.set_weights(w)
        _, _, _, _, _, fst = g.weighted_fora_batch(srcs, EPS, ALPHA, 3, fetch=True)
        a, _, sa, _ = g.weighted_ppr_targets(targets, ALPHA, 1e-4)
        v, _, sv, _ = g.ppr_targets(targets, ALPHA, 1e-4)
        b, _, sb, _ = g.weighted_ppr_targets(targets, ALPHA, 1e-4)
        assert min(fst.class_launches[5], sa.class_launches[5], sb.class_launches[5]) > 0
        assert float(np.max(np.abs(a - b))) <= TOL and sa.class_launches[5] == sb.class_launches[5]
        out, _, _, _, _, _ = g.fora_batch_single_source(srcs, EPS, ALPHA, seed=3, fetch=True)
        ref_v, ref_out = unweighted(fresh)
        assert float(np.max(np.abs(v - ref_v))) <= TOL
        # the same pushes and the same walks on both handles; the additions of the pushes in another order
        assert float(np.max(np.abs(out - ref_out))) <= 1e-9


# ---------------------------------------------------------------------------------------------- 4. delivery
def test_delivery_topk_store_and_sums(pkg, dev_cache, got):
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w)
    ind = _indeg(got)
    t = np.array([0, 5, int(np.argmax(ind)), int(np.flatnonzero(ind == 0)[0]), 17, 42] + list(range(60, 74)), dtype=np.int32)
    assert t.size == 20
    k = 8
    keep = pkg.Results(g, t.size)
    try:
        values, sel, st, pq = g.weighted_ppr_targets(t, ALPHA, 1e-5, k=k, keep=keep)
        ids, vals, n_sel = sel
        assert keep.info()[1] == t.size
        for i in range(t.size):
            cnt, row_i, row_v = targets_ref.topk_rows(values[i], k)
            assert n_sel[i] == cnt and np.array_equal(ids[i], row_i) and np.array_equal(vals[i], row_v), i
            assert np.array_equal(keep.fetch(i), values[i])
        assert st.levels == sum(s.levels for s in pq) and st.pops == sum(s.pops for s in pq)
        assert st.rmax_final == 1e-5 and st.total_ms > 0.0
        # without values_out the kept vectors are the only delivery
        none, _, _, _ = g.weighted_ppr_targets(t[:3], ALPHA, 1e-5, keep=keep, fetch=False)
        assert none is None and keep.info()[1] == 3
        for i in range(3):
            assert np.array_equal(keep.fetch(i), values[i])
    finally:
        keep.close()


# ---------------------------------------------------------------------------------------------- 5. life on the handle
def test_release_gives_the_memory_back_and_three_lives_leave_nothing(pkg, rmat12):
    w = _rand_w(rmat12, 22)
    tun = pkg.tuning_default()
    tun.dense_frac = 0.25

    def life(g):
        g.set_tuning(tun)
        g.set_weights(w)
        _, _, st, _ = g.weighted_ppr_targets([1, 2, 3], ALPHA, 1e-4, k=4)
        assert st.class_launches[5] > 0
        g.weighted_ppr_targets([5], ALPHA, 1e-4)

    both = pkg.Graph.RELEASE_BATCH | pkg.Graph.RELEASE_WEIGHTS
    with pkg.Graph(rmat12, device=0) as probe:
        with pkg.Graph(rmat12, device=0) as g:
            life(g)  # first round: the allocator's own pools, the sweep layout over the out-CSR, the selection scratch
            g.release(both)
            free0, _ = g.device_memory()
            life(g)
            busy, _ = g.device_memory()
            assert busy < free0  # the batch state and the weights are there again
            g.release(both)
            free1, _ = g.device_memory()
            assert free1 == free0 and g.weights_info() == (False, 0)
        base, _ = probe.device_memory()
        for _ in range(3):
            with pkg.Graph(rmat12, device=0) as g:
                life(g)
            left, _ = probe.device_memory()
            assert left == base


def test_a_refused_call_runs_nothing(pkg, got):
    n = got.n
    with pkg.Graph(got, device=0) as g:
        g.set_weights(_rand_w(got, 21))
        before, _, _, _ = g.weighted_ppr_targets([3, 4], ALPHA, 1e-4)
        kept = g.reserve()
        free0, _ = g.device_memory()
        for call in (lambda: g.weighted_ppr_target_sets([[0], [1, n], [2]], ALPHA, 1e-4),
                     lambda: g.weighted_ppr_targets([0, n + 3, 1], ALPHA, 1e-4)):
            with pytest.raises(pkg.PprhipError) as e:
                call()
            assert e.value.code == pkg.ERR_INVALID and "set 1" in str(e.value) and "pprhip_weighted_ppr_targets" in str(e.value)
        assert np.array_equal(g.reserve(), kept) and g.device_memory()[0] == free0
        after, _, _, _ = g.weighted_ppr_targets([3, 4], ALPHA, 1e-4)
        assert np.array_equal(after, before) or float(np.max(np.abs(after - before))) <= TOL
