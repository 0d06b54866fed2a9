"""Batched weighted FORA on the GPU (include/pprhip.h "batched weighted FORA"): query i of weighted_fora_batch /
weighted_fora_batch_seeds against the single call it stands for - vectors within 1e-12 ("same arithmetic, other addition
order") and the same decisions level by level -, against the numpy references of tests/weighted_ref.py and
tests/weighted_query_ref.py, the designed graphs of tests/weighted_designs.py at the edges of the batched sweep, the
weighted walk index, delivery, and the call's life on the handle."""
import numpy as np
import pytest

import weighted_query_ref as wqr
import weighted_ref as wr
from conftest import shared_graph
from weighted_designs import dense_design, sparse_design

ALPHA = 0.15
EPS = 0.5
TOL = 1e-12
pytestmark = pytest.mark.gpu

ALL_SPARSE, ALL_DENSE = 1e9, 1e-12  # dense_frac: no level reaches it / every level does
SIZES = (1, 3, 15, 16, 17, 40)


def _deg(host):
    return np.diff(host.out_rp.astype(np.int64))


def _indeg(host):
    return np.diff(host.in_rp.astype(np.int64))


def _rand_w(host, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, host.m)


def _graph(dev_cache, pkg, name, host, w=None, dense_frac=None):
    """The module's handle of `host` with the given weights (None: left as they are) and tuning (None: the default)."""
    g = shared_graph(dev_cache, pkg, name, lambda: pkg.Graph(host, device=0))
    t = pkg.tuning_default()
    if dense_frac is not None:
        t.dense_frac = dense_frac
    g.set_tuning(t)
    if w is not None:
        g.set_weights(w)
    return g


def _frac(host, mode):
    """dense_frac of a tuning: no level dense, every level dense, or the hub's first level (1 node + d edges) just below
    the threshold and its wide levels above."""
    if mode == "sparse":
        return ALL_SPARSE
    if mode == "dense":
        return ALL_DENSE
    return (int(_deg(host).max()) + 1.5) / host.m


def _source_pool(host):
    """The hub, a dead end, a node without in-edges that has out-edges, the hub again, a leaf-like node of out-degree 1
    (or the smallest there is), then fixed others; small graphs: every node."""
    if host.n <= 8:
        return list(range(host.n))
    deg, ind = _deg(host), _indeg(host)
    hub = int(np.argmax(deg))
    pool = [hub]
    dead = np.flatnonzero(deg == 0)
    if dead.size:
        pool.append(int(dead[0]))
    noin = np.flatnonzero((ind == 0) & (deg > 0))
    if noin.size:
        pool.append(int(noin[0]))
    pool.append(hub)  # the same source twice
    live = np.flatnonzero(deg > 0)
    pool.append(int(live[np.argmin(deg[live])]))
    rng = np.random.default_rng(5)
    pool += [int(x) for x in rng.choice(host.n, 7, replace=False)]
    return pool


def _cycled(pool, q):
    return [pool[i % len(pool)] for i in range(q)]


_SINGLE = {}


def _single(g, key, s, seed, rmax=0.0):
    """weighted_fora(s) on g under the tuning `key` names, run once per module."""
    k = (key, s, seed, rmax)
    if k not in _SINGLE:
        _SINGLE[k] = g.weighted_fora(s, EPS, ALPHA, seed, rmax=rmax)
    return _SINGLE[k]


def _decisions(st):
    return (st.levels, st.dense_levels, st.pops + st.dense_nodes, st.walks, st.walk_steps, st.dead_end_pops,
            st.rmax_final, st.omega, st.rounds)


def _check_batch(g, key, srcs, seed, rmax=0.0, mode=None, **kw):
    """One call of `srcs`; every query against its single call.  Returns (vectors, per-query stats, summed stats)."""
    singles = [_single(g, key, s, seed, rmax) for s in srcs]
    out, _, _, _, pq, st = g.weighted_fora_batch(srcs, EPS, ALPHA, seed, rmax=rmax, fetch=True, per_query=True, **kw)
    assert out.shape == (len(srcs), g.n) and len(pq) == len(srcs)
    worst = 0.0
    for i, s in enumerate(srcs):
        est, sst = singles[i]
        err = float(np.max(np.abs(out[i] - est)))
        worst = max(worst, err)
        assert err <= TOL, (key, len(srcs), i, s, err)
        assert _decisions(pq[i]) == _decisions(sst), (key, len(srcs), i, s, _decisions(pq[i]), _decisions(sst))
        if mode == "sparse":
            assert pq[i].dense_levels == 0
        elif mode == "dense":
            assert pq[i].dense_levels == pq[i].levels
    print("%s q=%d: worst |batch - single| %.2e, sweeps %d" % (key, len(srcs), worst, st.class_launches[5]))
    return out, pq, st


# ------------------------------------------------------------------------------------- query i is the single call
def _cases(pkg, got, rmat12, toy_graphs):
    dd, d = dense_design(pkg)
    sd, by_deg = sparse_design(pkg)
    dd_srcs = [d["pool"][0], d["pool"][511], d["pool"][512], d["pool"][1099], d["A"], d["B"], d["C"], d["small"][1],
               d["dead"]]
    sd_srcs = [int(v) for v in by_deg.values()] + _source_pool(sd)[:4]
    return {
        "got": (got, _rand_w(got, 21), _source_pool(got), 0.0),
        "rmat12": (rmat12, _rand_w(rmat12, 22), _source_pool(rmat12), 0.0),
        "dense_design": (dd, _rand_w(dd, 41), dd_srcs, 1e-9),
        "sparse_design": (sd, _rand_w(sd, 42), sd_srcs, 0.0),
        "two_node": (toy_graphs["two_node"], _rand_w(toy_graphs["two_node"], 2), [0, 1], 0.0),
        "star_dead_leaves": (toy_graphs["star_dead_leaves"], _rand_w(toy_graphs["star_dead_leaves"], 1),
                             list(range(6)), 0.0),
        "isolated_mix": (toy_graphs["isolated_mix"], np.linspace(0.75, 3.0, toy_graphs["isolated_mix"].m),
                         list(range(6)), 0.0),
    }


@pytest.mark.parametrize("mode", ["sparse", "dense", "mixed"])
@pytest.mark.parametrize("name", ["got", "rmat12", "dense_design", "sparse_design", "two_node", "star_dead_leaves",
                                  "isolated_mix"])
def test_query_i_is_the_single_call(pkg, dev_cache, got, rmat12, toy_graphs, name, mode):
    """Calls of 1, 3, 15, 16, 17 and 40 queries - one column, a few, one short of all, all, one refill, slots refilled
    while other columns are in mid-push - under a tuning without dense levels, with dense levels only, and with both.
    The sources: the hub, a dead end, a node without in-edges, the same source twice; dense_design's at rmax = 1e-9 (a
    row that starts on a chunk boundary, rows crossing one and two, a last chunk shorter than 512 edges); got: 352
    in-edges, fewer chunks than waves."""
    host, w, pool, rmax = _cases(pkg, got, rmat12, toy_graphs)[name]
    g = _graph(dev_cache, pkg, name, host, w, dense_frac=_frac(host, mode))
    key = (name, mode)
    deg = _deg(host)
    sweeps = 0
    for q in SIZES:
        srcs = _cycled(pool, q)
        _, pq, st = _check_batch(g, key, srcs, 3, rmax, mode)
        sweeps += st.class_launches[5]
        if q == 40 and host.n > 8:
            # queries of clearly different lengths share the call: the dead end runs no level, the hub's push is long
            levels = [p.levels for p in pq]
            print("levels of the 40:", levels)
            assert min(levels) == 0 or not (deg == 0).any()
            assert len(set(levels)) >= 3 and max(levels) >= min(levels) + 3
    if mode == "sparse":
        assert sweeps == 0
    elif mode == "dense":
        assert sweeps > 0, "the batched sweep did not run"
    if mode == "mixed" and name == "rmat12":  # the hub of R-MAT 12: its first level sparse, its wide levels dense
        hub = _single(g, key, int(np.argmax(deg)), 3, rmax)[1]
        assert 0 < hub.dense_levels < hub.levels


# ------------------------------------------------------------------------------------- numpy and the bound
# (graph, weight seed, sources, walk seed): the triples tests/test_gpu_weighted.py keeps because weighted_ref.fora itself
# meets the bound on them; the last source of each graph is a dead end
NUMPY_CASES = [("got", 21, [63, 35, 71], 3), ("rmat12", 22, [1803, 2025, 3], 4)]


@pytest.mark.parametrize("name,wseed,srcs,seed", NUMPY_CASES)
def test_against_numpy_and_the_bound(pkg, dev_cache, got, rmat12, name, wseed, srcs, seed):
    host = got if name == "got" else rmat12
    w = _rand_w(host, wseed)
    pi = wr.ppr_exact(host, w, ALPHA)
    g = _graph(dev_cache, pkg, name, host, w)
    out, _, _, _, pq, _ = g.weighted_fora_batch(srcs, EPS, ALPHA, seed, fetch=True, per_query=True)
    rmax0, omega = wr.whole_params(host.n, host.m, ALPHA, EPS)
    for i, s in enumerate(srcs):
        bound = EPS * np.maximum(pi[s], 1.0 / host.n)
        ref, ref_walks, ref_steps = wr.fora(host, w, s, EPS, ALPHA, seed)
        assert np.all(np.abs(ref - pi[s]) <= bound), "the reference misses the bound: not a triple to test with"
        err = float(np.max(np.abs(out[i] - ref)))
        worst = float(np.max(np.abs(out[i] - pi[s]) / bound))
        print("%s src %d: |batch - ref| %.2e, worst |est - pi| / bound %.3f, walks %d" % (name, s, err, worst, pq[i].walks))
        assert err <= TOL, (name, s, err)
        assert np.all(np.abs(out[i] - pi[s]) <= bound), (name, s, worst)
        assert pq[i].walks == ref_walks and pq[i].walk_steps == ref_steps and pq[i].rounds == 1
        assert pq[i].rmax_final == rmax0 and pq[i].omega == omega


# ------------------------------------------------------------------------------------- column isolation
def test_columns_do_not_leak(pkg, dev_cache, rmat12):
    """Sixteen queries, every level dense: fifteen columns carry the hub's push, one another source's."""
    w = _rand_w(rmat12, 22)
    g = _graph(dev_cache, pkg, "rmat12", rmat12, w, dense_frac=ALL_DENSE)
    hub = int(np.argmax(_deg(rmat12)))
    for odd_at in (0, 9, 15):
        srcs = [hub] * 16
        srcs[odd_at] = 1803
        out, _, _ = _check_batch(g, ("rmat12", "dense"), srcs, 3, mode="dense")
        sums = out.sum(axis=1)
        print("odd column %d: max |sum - 1| %.2e" % (odd_at, float(np.max(np.abs(sums - 1.0)))))
        assert np.all(np.abs(sums - 1.0) <= TOL)


# ------------------------------------------------------------------------------------- the weighted walk index
def test_served_from_the_weighted_walk_index(pkg, dev_cache, rmat12):
    w = _rand_w(rmat12, 22)
    g = _graph(dev_cache, pkg, "rmat12", rmat12, w, dense_frac=_frac(rmat12, "mixed"))
    seed = 6
    srcs = _cycled(_source_pool(rmat12), 20)
    plain, _, _, _, plain_pq, _ = g.weighted_fora_batch(srcs, EPS, ALPHA, seed, fetch=True, per_query=True)
    g.build_weighted_walk_index(ALPHA, seed=seed)
    try:
        g.weighted_walk_index_usage(reset=True)
        singles = [g.weighted_fora(s, EPS, ALPHA, seed) for s in srcs]
        used_single = g.weighted_walk_index_usage(reset=True)
        out, _, _, _, pq, _ = g.weighted_fora_batch(srcs, EPS, ALPHA, seed, fetch=True, per_query=True)
        used_batch = g.weighted_walk_index_usage(reset=True)
        print("index usage (served, walked): singles %s, batch %s" % (used_single, used_batch))
        assert used_batch == used_single and used_batch[0] > 0
        for i in range(len(srcs)):
            assert pq[i].walks == singles[i][1].walks == plain_pq[i].walks
            assert np.max(np.abs(out[i] - singles[i][0])) <= TOL, i
            assert np.max(np.abs(out[i] - plain[i])) <= TOL, i
        g.weighted_fora_batch(srcs, EPS, ALPHA, seed + 1)  # another seed: nothing is served
        assert g.weighted_walk_index_usage(reset=True) == (0, 0)
    finally:
        g.drop_weighted_walk_index()


# ------------------------------------------------------------------------------------- seed sets
def _seed_sets(host):
    """A single member, non-uniform weights, a dead-end seed among live ones, a live seed without in-edges, only
    dead-end seeds."""
    deg, ind = _deg(host), _indeg(host)
    live = np.flatnonzero(deg > 0)
    dead = np.flatnonzero(deg == 0)
    noin = np.flatnonzero((ind == 0) & (deg > 0))
    hub = int(np.argmax(deg))
    a, b, c = (int(x) for x in live[[1, live.size // 2, live.size - 1]])
    sets = [([hub], None), ([hub, a, b], [3.0, 1.0, 0.5]), ([a, int(dead[0]), c], [1.0, 2.0, 1.0]),
            ([int(dead[0]), int(dead[-1])], [1.0, 3.0]), ([b, c, hub, a], None)]
    if noin.size:
        sets.append(([int(noin[0]), a], [2.0, 1.0]))
        sets.append(([int(noin[-1])], None))
    return sets


@pytest.mark.parametrize("mode", ["mixed", "dense"])
@pytest.mark.parametrize("name", ["got", "rmat12"])
def test_seed_sets(pkg, dev_cache, got, rmat12, name, mode):
    host = got if name == "got" else rmat12
    w = _rand_w(host, 21 if name == "got" else 22)
    g = _graph(dev_cache, pkg, name, host, w, dense_frac=_frac(host, mode))
    base = _seed_sets(host)
    assert name != "rmat12" or len(base) == 7, "R-MAT 12 has live nodes without in-edges"
    picked = _cycled(base, 18)
    sets, sws = [p[0] for p in picked], [p[1] for p in picked]
    singles = [g.weighted_fora_seeds(s, EPS, ALPHA, 3, weights=sw) for s, sw in base]
    out, _, _, _, pq, st = g.weighted_fora_batch_seeds(sets, EPS, ALPHA, 3, weights=sws, fetch=True, per_query=True)
    worst = 0.0
    for i in range(18):
        est, sst = singles[i % len(base)]
        err = float(np.max(np.abs(out[i] - est)))
        worst = max(worst, err)
        assert err <= TOL, (name, mode, i, sets[i], err)
        assert _decisions(pq[i]) == _decisions(sst), (name, mode, i, sets[i])
        if mode == "dense":
            assert pq[i].dense_levels == pq[i].levels
    print("%s %s: worst |batch - single| over 18 sets %.2e, sweeps %d" % (name, mode, worst, st.class_launches[5]))
    assert st.class_launches[5] > 0
    all_dead = [i for i, s in enumerate(sets) if (_deg(host)[s] == 0).all()]
    assert all_dead and all(pq[i].levels == 0 and pq[i].walks == 0 for i in all_dead)
    for i in all_dead:
        assert np.max(np.abs(out[i] - wqr.seed_p(host.n, sets[i], sws[i]))) <= TOL
    if name == "got":  # ... and against the numpy restatement
        for i in range(min(4, len(base))):
            ref, walks, steps = wqr.fora_seeds(host, w, sets[i], sws[i], EPS, ALPHA, 3)
            err = float(np.max(np.abs(out[i] - ref)))
            print("got set %s: |batch - numpy| %.2e" % (sets[i], err))
            assert err <= TOL and pq[i].walks == walks and pq[i].walk_steps == steps, (i, err)


# ------------------------------------------------------------------------------------- delivery
def _n_sel(vec, k):
    """What the selection reports (pprhip_topk_select): the entries >= the k-th largest, or every positive entry when
    there are fewer than k."""
    pos = np.sort(vec[vec > 0.0])[::-1]
    return int(pos.size) if pos.size < k else int(np.count_nonzero(vec >= pos[k - 1]))


def test_delivery_topk_keep_and_out(pkg, dev_cache, rmat12):
    w = _rand_w(rmat12, 22)
    g = _graph(dev_cache, pkg, "rmat12", rmat12, w, dense_frac=_frac(rmat12, "mixed"))
    srcs = _cycled(_source_pool(rmat12), 19)
    k = 10
    keep = pkg.Results(g, len(srcs))
    mine = np.full((len(srcs), g.n), -1.0)
    out, ids, vals, nsel, pq, _ = g.weighted_fora_batch(srcs, EPS, ALPHA, 3, k=k, fetch=True, per_query=True, keep=keep,
                                                       out=mine)
    assert out is mine and mine.min() >= 0.0
    assert keep.info() == (len(srcs), len(srcs), g.n)
    # the unweighted batch reports n_sel the same way
    uo, _, _, unsel, _, _ = g.fora_batch_single_source(srcs[:3], EPS, ALPHA, 3, k=k, fetch=True)
    for i in range(3):
        assert unsel[i] == _n_sel(uo[i], k)
    for i, s in enumerate(srcs):
        order = np.lexsort((np.arange(g.n), -out[i]))[:k]
        order = order[out[i][order] > 0.0]
        m = order.size
        assert np.array_equal(ids[i][:m], order) and np.array_equal(vals[i][:m], out[i][order]), (i, s)
        assert (ids[i][m:] == -1).all() and (vals[i][m:] == 0.0).all()
        assert nsel[i] == _n_sel(out[i], k), (i, s, nsel[i])
        assert np.array_equal(keep.fetch(i), out[i]), (i, s)
    sid, sval, cnt = keep.fetch_sparse(4, 0.0, "id")
    assert np.array_equal(sid, np.flatnonzero(out[4] > 0)) and np.array_equal(sval, out[4][out[4] > 0]) and cnt == sid.size
    # without fetch nothing comes back but the selection and the statistics
    none, ids2, vals2, nsel2, pq2, _ = g.weighted_fora_batch(srcs, EPS, ALPHA, 3, k=k)
    assert none is None and pq2 is None and np.array_equal(ids2, ids) and np.array_equal(nsel2, nsel)
    assert np.max(np.abs(vals2 - vals)) <= TOL


# ------------------------------------------------------------------------------------- life on the handle
def test_needs_weights_and_checks_before_anything_runs(pkg, dev_cache, got):
    with pkg.Graph(got, device=0) as g0:
        for call in (lambda: g0.weighted_fora_batch([63, 35], EPS, ALPHA, 3),
                     lambda: g0.weighted_fora_batch_seeds([[63], [35, 17]], EPS, ALPHA, 3)):
            with pytest.raises(pkg.PprhipError, match="no relationship weights") as ei:
                call()
            assert ei.value.code == pkg.ERR_STATE
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w)
    g.weighted_fora(63, EPS, ALPHA, 3)
    before = g.reserve()
    srcs = [63] * 20
    srcs[7] = got.n
    keep = pkg.Results(g, 20)
    with pytest.raises(pkg.PprhipError) as ei:
        g.weighted_fora_batch(srcs, EPS, ALPHA, 3, keep=keep)
    assert ei.value.code == pkg.ERR_INVALID
    with pytest.raises(pkg.PprhipError) as ei:
        g.weighted_fora_batch_seeds([[63]] * 7 + [[63, -1]] + [[35]] * 12, EPS, ALPHA, 3)
    assert ei.value.code == pkg.ERR_INVALID
    for bad in (dict(eps=0.0), dict(eps=EPS, rmax=-1.0)):
        with pytest.raises(pkg.PprhipError) as ei:
            g.weighted_fora_batch([63], bad["eps"], ALPHA, 3, rmax=bad.get("rmax", 0.0))
        assert ei.value.code == pkg.ERR_INVALID
    assert np.array_equal(g.reserve(), before)
    # an empty call
    out, ids, vals, nsel, pq, st = g.weighted_fora_batch([], EPS, ALPHA, 3, k=5, fetch=True, per_query=True, keep=keep)
    assert out.shape == (0, g.n) and st.levels == 0 and st.walks == 0 and keep.info()[1] == 0
    out, _, _, _, _, st = g.weighted_fora_batch_seeds([], EPS, ALPHA, 3, fetch=True)
    assert out.shape == (0, g.n) and st.levels == 0
    # the handle is as usable as before
    _check_batch(g, ("got", "default"), [63, 35, 71], 3)


def test_unweighted_batches_around_a_weighted_one(pkg, dev_cache, rmat12):
    """The weighted call borrows the batch workspaces and the shared arrays of the unweighted batched calls and hands
    them back as it found them."""
    w = _rand_w(rmat12, 22)
    g = _graph(dev_cache, pkg, "rmat12", rmat12, w)
    srcs = _cycled(_source_pool(rmat12), 21)
    counters = lambda st: (st.levels, st.dense_levels, st.pops, st.dense_nodes, st.edge_pushes, st.walks, st.walk_steps,
                           st.dead_end_pops, st.rounds)
    try:
        g.set_tuning(pkg.tuning_batch())  # (dense levels from 1 % of m: the unweighted sweeps run)
        a, _, _, _, apq, ast = g.fora_batch_single_source(srcs, EPS, ALPHA, 3, fetch=True, per_query=True)
        wout, _, _ = _check_batch(g, ("rmat12", "batch tuning"), srcs, 3)
        b, _, _, _, bpq, bst = g.fora_batch_single_source(srcs, EPS, ALPHA, 3, fetch=True, per_query=True)
        # ... and behind a backward call, which leaves its own layout in the shared row sums
        g.ppr_targets([5, 9, 1803], ALPHA, 1e-6)
        _check_batch(g, ("rmat12", "batch tuning"), srcs, 3)
        c, _, _, _, cpq, _ = g.fora_batch_single_source(srcs, EPS, ALPHA, 3, fetch=True, per_query=True)
    finally:
        g.set_tuning(pkg.tuning_default())
    assert ast.class_launches[5] > 0 and bst.class_launches[5] > 0
    print("unweighted batch before / after a weighted one: max |diff| %.2e" % float(np.max(np.abs(a - b))))
    assert np.max(np.abs(a - b)) <= TOL and np.max(np.abs(a - c)) <= TOL
    for i in range(len(srcs)):
        assert counters(apq[i]) == counters(bpq[i]) == counters(cpq[i]), i
    assert np.max(np.abs(wout - a)) > 1e-6  # (the weighted vectors are other vectors)


def test_a_second_set_of_weights_rules(pkg, dev_cache, got):
    w1, w2 = _rand_w(got, 21), _rand_w(got, 52)
    srcs = [63, 35, 17, 71, 63]
    g = _graph(dev_cache, pkg, "got", got, w1, dense_frac=ALL_DENSE)
    o1, _, _, _, _, _ = g.weighted_fora_batch(srcs, EPS, ALPHA, 3, fetch=True)
    g.set_weights(w2)
    try:
        o2, _, _, _, _, _ = g.weighted_fora_batch(srcs, EPS, ALPHA, 3, fetch=True)
        for i, s in enumerate(srcs):
            est, _ = g.weighted_fora(s, EPS, ALPHA, 3)
            assert np.max(np.abs(o2[i] - est)) <= TOL, s
            ref, _, _ = wr.fora(got, w2, s, EPS, ALPHA, 3)
            assert np.max(np.abs(o2[i] - ref)) <= TOL, s
        assert np.max(np.abs(o1 - o2)) > 1e-6
    finally:
        g.set_weights(w1)


def test_fewer_workspaces(pkg, dev_cache, rmat12, monkeypatch):
    """PPRHIP_BATCH_WORKSPACES=4: four columns in flight, the same queries."""
    w = _rand_w(rmat12, 22)
    frac = _frac(rmat12, "mixed")
    g = _graph(dev_cache, pkg, "rmat12", rmat12, w, dense_frac=frac)
    srcs = _cycled(_source_pool(rmat12), 13)
    full, _, _ = _check_batch(g, ("rmat12", "mixed"), srcs, 3)
    monkeypatch.setenv("PPRHIP_BATCH_WORKSPACES", "4")
    with pkg.Graph(rmat12, device=0) as g4:
        t = pkg.tuning_default()
        t.dense_frac = frac
        g4.set_tuning(t)
        g4.set_weights(w)
        out, _, _, _, pq, st = g4.weighted_fora_batch(srcs, EPS, ALPHA, 3, fetch=True, per_query=True)
    err = float(np.max(np.abs(out - full)))
    print("4 workspaces against 16: max |diff| %.2e, sweeps %d" % (err, st.class_launches[5]))
    assert err <= TOL and st.class_launches[5] > 0
    for i, s in enumerate(srcs):
        assert _decisions(pq[i]) == _decisions(_single(g, ("rmat12", "mixed"), s, 3)[1]), (i, s)
