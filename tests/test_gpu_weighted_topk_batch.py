"""Batched weighted FORA top-k on the GPU (include/pprhip.h "batched weighted top-k"): query i of a call IS
weighted_fora_topk(srcs[i], ..., seed + i) - the same rounds, levels and walks, vectors within 1e-12 - under tunings
without dense levels, with dense levels only and the default; the calls against the numpy reference of
tests/weighted_query_ref.py; the merged walk launch on the designed graph of tests/weighted_topk_batch_designs.py,
whose walk phases the host places in their launches before any device result is looked at; seed sets; columns that do
not leak; delivery and checks.  Graphs: GoT, R-MAT 12 and designed ones, never larger."""
import numpy as np
import pytest

import test_gpu_weighted_batch as tb
import test_gpu_weighted_query as tq
import weighted_query_ref as wq
import weighted_topk_batch_designs as dsg
from weighted_query_designs import collect_design, exact_eps

ALPHA, EPS, TOL = 0.15, 0.5, 1e-12
pytestmark = pytest.mark.gpu
SIZES = (1, 3, 16, 17, 40)
MODES = ("sparse", "dense", "default")
BASE_WAVES = 256 * 16  # the merged launch's base grid, n_cus * 16, on an MI355X (the design's shares hold from 3 CUs up)


def _frac(host, mode):
    return None if mode == "default" else tb._frac(host, mode)


def _pool(host):
    """tb._source_pool: the hub, a dead end, a node without in-edges, the hub again, a node of out-degree 1, others."""
    deg = tq._deg(host)
    pool = tb._source_pool(host)
    assert int(np.argmax(deg)) in pool and any(deg[s] == 0 for s in pool) and any(deg[s] == 1 for s in pool)
    return pool


_SINGLE = {}


def _single(g, key, s, k, seed, conf=None, sw=None):
    """weighted_fora_topk(s) / weighted_fora_topk_seeds(s) on g under the tuning `key` names, run once per module."""
    kk = (key, tuple(np.atleast_1d(s).tolist()), None if sw is None else tuple(sw), k, seed)
    if kk not in _SINGLE:
        if np.ndim(s) == 0:
            _SINGLE[kk] = g.weighted_fora_topk(int(s), EPS, ALPHA if conf is None else conf.alpha, k, seed, conf=conf, fetch=True)
        else:
            _SINGLE[kk] = g.weighted_fora_topk_seeds(s, EPS, ALPHA if conf is None else conf.alpha, k, seed, weights=sw,
                                                     conf=conf, fetch=True)
    return _SINGLE[kk]


def _decisions(st):
    return (st.rounds, st.levels, st.dense_levels, st.pops + st.dense_nodes, st.walks, st.walk_steps, st.mc_sources,
            st.rmax_final, st.omega)


def _near(vals, est, k):
    """positions of a row whose neighbouring values are within 1e-9 (relative): there the ids may differ"""
    cnt = vals.size
    near = np.zeros(cnt, dtype=bool)
    if cnt > 1:
        gap = np.abs(np.diff(vals)) <= 1e-9 * vals[:-1]
        near[:-1] |= gap
        near[1:] |= gap
    if cnt == k:  # the last position against the first one left out
        rest = np.sort(est)[::-1]
        near[-1] |= bool(rest.size > k and abs(vals[-1] - rest[k]) <= 1e-9 * vals[-1])
    return near


def _same_query(tag, k, row, single, cap_near=True):
    """(ids, vals, n_out, stats, kept vector) of query i against its single call's (nsel, ids, vals, est, st).
    cap_near: the near-tie rule may excuse one position of the row at most (single sources, chosen so; a seed set's p
    ties its seeds exactly)."""
    ids, vals, n_out, st, vec = row
    nsel, sids, svals, est, sst = single
    assert _decisions(st) == _decisions(sst), (tag, _decisions(st), _decisions(sst))
    assert abs(st.rsum - sst.rsum) <= TOL and abs(st.kth_value - sst.kth_value) <= TOL, (tag, st.rsum, sst.rsum)
    assert n_out == nsel, (tag, n_out, nsel)
    cnt = min(nsel, k)
    assert np.max(np.abs(vals[:cnt] - svals[:cnt]), initial=0.0) <= TOL, tag
    assert (ids[cnt:] == -1).all() and (vals[cnt:] == 0.0).all(), tag
    near = _near(svals[:cnt], est, k)
    assert near.sum() <= 1 or not cap_near, (tag, int(near.sum()))
    assert np.array_equal(ids[:cnt][~near], sids[:cnt][~near]), (tag, ids, sids)
    err = float(np.max(np.abs(vec - est)))
    assert err <= TOL, (tag, err)
    return err


def _check_call(pkg, g, key, srcs, k, seed, mode=None, conf=None):
    q = len(srcs)
    keep = pkg.Results(g, q)
    try:
        ids, vals, n_out, st, pq = g.weighted_fora_batch_topk(srcs, k, EPS, ALPHA if conf is None else conf.alpha, seed,
                                                               conf=conf, per_query=True, keep=keep)
        assert ids.shape == (q, k) and vals.shape == (q, k) and len(pq) == q
        worst = 0.0
        for i, s in enumerate(srcs):
            single = _single(g, key, s, k, seed + i, conf)
            worst = max(worst, _same_query((key, q, i, s), k, (ids[i], vals[i], int(n_out[i]), pq[i], keep.fetch(i)), single))
            if mode == "sparse":
                assert pq[i].dense_levels == 0
            elif mode == "dense":
                assert pq[i].dense_levels == pq[i].levels
        assert st.rounds == sum(p.rounds for p in pq) and st.walks == sum(p.walks for p in pq)
        print("%s q=%d: worst |batch - single| %.2e, sweeps %d (%.1f columns), walk launches %d (%.1f columns)" %
              (key, q, worst, st.class_launches[5], st.dense_levels / max(1, st.class_launches[5]), st.class_launches[3],
               st.rounds / max(1, st.class_launches[3])))
        return ids, vals, pq, st
    finally:
        keep.close()


# ------------------------------------------------------------------------------------- 1. query i is the single call
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["got", "rmat12"])
def test_query_i_is_the_single_call(pkg, dev_cache, got, rmat12, name, mode):
    host = got if name == "got" else rmat12
    w = tq._rand_w(host, 21 if name == "got" else 22)
    g = tq._graph(dev_cache, pkg, name, host, w, dense_frac=_frac(host, mode))
    pool, k = _pool(host), 8
    sweeps = merged = 0
    for q in SIZES:
        _, _, pq, st = _check_call(pkg, g, (name, mode), tb._cycled(pool, q), k, 3, mode)
        sweeps += st.class_launches[5]
        if q > 1:
            merged += st.class_launches[3]
            assert st.class_launches[3] <= st.rounds  # (a merged launch serves at least one round)
        if q >= 16:  # walk phases did share launches, and a dead end ran no round beside queries of several
            assert st.class_launches[3] < st.rounds
            assert min(p.rounds for p in pq) == 0 and max(p.rounds for p in pq) >= 2
    assert merged > 0 and (mode != "sparse" or sweeps == 0) and (mode != "dense" or sweeps > 0)


# ------------------------------------------------------------------------------------- 2. against numpy
_REF = {}


def _ref(key, *args):
    if key not in _REF:
        _REF[key] = wq.topk(*args)
    return _REF[key]


@pytest.mark.parametrize("case", range(len(tq.TOPK_CASES)))
def test_against_numpy(pkg, dev_cache, got, rmat12, case):
    name, wseed, seeds, sw, k, seed = tq.TOPK_CASES[case]
    host = got if name == "got" else rmat12
    w = tq._rand_w(host, wseed)
    conf = pkg.conf_topk(host.n, host.m, k, ALPHA)
    g = tq._graph(dev_cache, pkg, name, host, w)
    keep = pkg.Results(g, 3)
    if len(seeds) == 1:
        out = g.weighted_fora_batch_topk(seeds * 3, k, EPS, ALPHA, seed, conf=conf, per_query=True, keep=keep)
    else:
        out = g.weighted_fora_batch_topk_seeds([seeds] * 3, k, EPS, ALPHA, seed, weights=[sw] * 3, conf=conf,
                                               per_query=True, keep=keep)
    ids, vals, n_out, _, pq = out
    for i in range(3):
        ref = _ref((case, i), host, w, seeds, sw, EPS, conf, seed + i)
        st = pq[i]
        assert (st.rounds, st.levels, st.walks, st.walk_steps) == (ref["rounds"], ref["levels"], ref["walks"], ref["steps"]), (case, i)
        assert st.pops + st.dense_nodes == ref["pops"] and st.rmax_final == ref["rmax"] and st.omega == ref["omega"]
        err = float(np.max(np.abs(keep.fetch(i) - ref["est"])))
        assert err <= TOL, (case, i, err)
        cnt = ref["vals"].size
        assert min(int(n_out[i]), k) == cnt and np.max(np.abs(vals[i][:cnt] - ref["vals"])) <= TOL
        # (the ids too, by the near-tie rule, without the cap of one excused position that holds for the sources of
        # test_query_i_is_the_single_call: GoT's seed set at seed + 1 has one near-tied pair, which marks two positions)
        near = _near(ref["vals"], ref["est"], k)
        assert np.array_equal(ids[i][:cnt][~near], ref["ids"][~near]), (case, i)
    keep.close()


# ------------------------------------------------------------------------------------- 3. designed walk phases
# the call on walk_design: (source, why).  Column = position (q < 16, no query ends before the launch in question).
DESIGN_SRCS = [(dsg.CHAIN0 + 1, "a single walk"), (dsg.RAND0, "in its levels when the others walk: an idle column between"),
               (dsg.RAND0 + 8, "fewer than 64 walks"), (dsg.HUB, "one walk per leaf: many"), (dsg.RAND0 + 2, "more than a wave"),
               (dsg.CYCLE0, "the cycle: rounds that plan no walk"), (dsg.CHAIN0 + 2, "a single walk, in its second round")]


def test_designed_walk_phases_share_one_launch(pkg, dev_cache):
    """The design, on the host first: with wq.topk's round_levels and walks_round and the driver's lockstep
    (weighted_topk_batch_designs.launches) one merged launch holds a column of exactly one walk, one of fewer than 64, one
    of 2 000 (32 waves of walk_multi_shares), and idle columns between and behind them.  A plan of a weighted top-k round
    never holds a dead-end start: a dead end with mass is active at every threshold, so no round ends with residue on
    one (asserted below); that branch of the kernel is k_w_walk_plan's, kept for the same reason it is there.  Dead-end
    restarts are walked (the pair and the line end in dead ends)."""
    host, w, _ = dsg.walk_design(pkg)
    srcs = [s for s, _ in DESIGN_SRCS]
    conf = pkg.conf_topk(host.n, host.m, dsg.K, dsg.ALPHA)
    refs = [_ref(("design", i), host, w, [s], None, dsg.EPS, conf, dsg.SEED + i) for i, s in enumerate(srcs)]
    assert all(r["rounds"] >= 2 for r in refs)
    L = dsg.launches(refs)
    hit = [t for t, cols in L.items()
           if any(x == 1 for _, _, x in cols) and any(1 < x < 64 for _, _, x in cols) and any(x >= 2000 for _, _, x in cols)]
    assert hit, L
    cols = L[min(hit)]
    counts = np.zeros(16, dtype=np.uint64)
    for c, _, x in cols:
        counts[c] = x
    busy = np.flatnonzero(counts)
    assert np.count_nonzero(counts[busy[0]:busy[-1]] == 0) >= 1 and len(cols) >= 4, counts  # an idle column between
    # the launch's 2 128 walks are 34 groups of 64: every base grid of 34 waves or more - the launcher's n_cus * 16 on any
    # device of three CUs or more - deals the same shares, one group per wave
    per, first = pkg.walk_multi_shares(counts, BASE_WAVES)
    groups = (int(counts.sum()) + 63) // 64
    per_min, first_min = pkg.walk_multi_shares(counts, groups)
    assert groups <= 3 * 16 and per_min == per and np.array_equal(first_min, first)
    nw = np.diff(first.astype(np.int64))
    assert per == 64 and nw[np.flatnonzero(counts == 1)[0]] == 1 and nw.max() == 32 and first[16] == nw.sum() <= BASE_WAVES + 15
    assert any(x == 0 for cs in L.values() for _, _, x in cs)  # a phase that plans no walk rides a launch too
    assert sum(dsg.dead_end_starts(host, r, j) for r in refs for j in range(r["rounds"])) == 0
    print("design: launch %d holds %s" % (min(hit), cols))
    for mode in ("default", "dense", "sparse"):
        frac = {"default": None, "dense": tq.ALL_DENSE, "sparse": tq.ALL_SPARSE}[mode]
        g = tq._graph(dev_cache, pkg, "walk_design", host, w, dense_frac=frac)
        keep = pkg.Results(g, len(srcs))
        ids, vals, n_out, st, pq = g.weighted_fora_batch_topk(srcs, dsg.K, dsg.EPS, dsg.ALPHA, dsg.SEED, conf=conf,
                                                               per_query=True, keep=keep)
        assert st.class_launches[3] == len(L), (mode, st.class_launches[3], len(L))  # the launches the host model places
        for i, ref in enumerate(refs):
            p = pq[i]
            assert (p.rounds, p.levels, p.walks, p.walk_steps) == (ref["rounds"], ref["levels"], ref["walks"], ref["steps"]), (mode, i)
            err = float(np.max(np.abs(keep.fetch(i) - ref["est"])))
            assert err <= TOL, (mode, i, err)
            cnt = ref["vals"].size
            assert np.max(np.abs(vals[i][:cnt] - ref["vals"])) <= TOL and abs(p.kth_value - ref["kth"]) <= TOL
        keep.close()


def test_collect_design_as_three_of_a_call(pkg, dev_cache):
    """tests/weighted_query_designs.py: collect_design (residues exactly on a round's threshold, active nodes at tile
    edges) as 3 of a call's queries, in all three dense modes; seed + i: the walks differ, the pushes do not."""
    host, w, d = collect_design(pkg)
    conf = pkg.conf_topk(host.n, host.m, 4, 0.5)
    eps = exact_eps(conf, d["rmax1"])
    other = int(np.flatnonzero(tq._deg(host) > 0)[-1])
    srcs = [d["S"], other, d["S"], d["G"], d["S"]]
    refs = {i: _ref(("collect", i), host, w, [d["S"]], None, eps, conf, 5 + i) for i in (0, 2, 4)}
    assert all(r["frontier"][:2] == [1, 1 + d["chosen"].size] for r in refs.values())
    for frac in (tq.ALL_SPARSE, None, tq.ALL_DENSE):
        g = tq._graph(dev_cache, pkg, "collect_design", host, w, dense_frac=frac)
        keep = pkg.Results(g, len(srcs))
        _, vals, _, _, pq = g.weighted_fora_batch_topk(srcs, 4, eps, 0.5, 5, conf=conf, per_query=True, keep=keep)
        for i, ref in refs.items():
            p = pq[i]
            assert (p.rounds, p.levels, p.pops + p.dense_nodes, p.walks, p.walk_steps) == \
                (ref["rounds"], ref["levels"], ref["pops"], ref["walks"], ref["steps"]), (frac, i)
            assert p.rmax_final == ref["rmax"] and np.max(np.abs(keep.fetch(i) - ref["est"])) <= TOL, (frac, i)
            assert (p.dense_levels == 0) == (frac == tq.ALL_SPARSE)
        keep.close()


# ------------------------------------------------------------------------------------- 4. seed sets
@pytest.mark.parametrize("mode", ["default", "dense"])
@pytest.mark.parametrize("name", ["got", "rmat12"])
def test_seed_sets(pkg, dev_cache, got, rmat12, name, mode):
    host = got if name == "got" else rmat12
    w = tq._rand_w(host, 21 if name == "got" else 22)
    g = tq._graph(dev_cache, pkg, name, host, w, dense_frac=_frac(host, mode))
    sets, k, seed = tq._sets(host), 6, 7
    keys = list(sets) * 2  # (more queries than kinds of sets: every kind at two seeds)
    keep = pkg.Results(g, len(keys))
    ids, vals, n_out, st, pq = g.weighted_fora_batch_topk_seeds([sets[x][0] for x in keys], k, EPS, ALPHA, seed,
                                                                weights=[sets[x][1] for x in keys], per_query=True, keep=keep)
    for i, x in enumerate(keys):
        single = _single(g, (name, mode), np.asarray(sets[x][0]), k, seed + i, sw=sets[x][1])
        _same_query((name, mode, x, i), k, (ids[i], vals[i], int(n_out[i]), pq[i], keep.fetch(i)), single, cap_near=False)
        if x == "dead":  # no live seed: rounds 0, the row is the top-k of p
            p = wq.seed_p(host.n, *sets[x])
            rid, rv, _ = wq.select(p, k)
            assert pq[i].rounds == 0 and pq[i].walks == 0 and pq[i].levels == 0
            assert np.max(np.abs(keep.fetch(i) - p)) <= 1e-16 and n_out[i] == rid.size
            assert np.array_equal(ids[i][:rid.size], rid) and np.max(np.abs(vals[i][:rid.size] - rv)) <= 1e-16
    keep.close()


# ------------------------------------------------------------------------------------- 5. columns and neighbours
def test_columns_do_not_leak(pkg, dev_cache, rmat12):
    w = tq._rand_w(rmat12, 22)
    g = tq._graph(dev_cache, pkg, "rmat12", rmat12, w, dense_frac=tq.ALL_DENSE)
    pool, k, s = _pool(rmat12), 8, 1803
    keep = pkg.Results(g, 16)
    alone = _single(g, ("rmat12", "dense"), s, k, 11 + 9)
    srcs = tb._cycled(pool, 16)
    srcs[9] = s
    ids, vals, n_out, _, pq = g.weighted_fora_batch_topk(srcs, k, EPS, ALPHA, 11, per_query=True, keep=keep)
    _same_query("among 15 others", k, (ids[9], vals[9], int(n_out[9]), pq[9], keep.fetch(9)), alone)
    keep.close()


def test_neighbours_are_untouched_and_new_weights_rule(pkg, dev_cache, rmat12):
    w = tq._rand_w(rmat12, 22)
    g = tq._graph(dev_cache, pkg, "rmat12", rmat12, w, dense_frac=_frac(rmat12, "mixed"))
    srcs = tb._cycled(_pool(rmat12), 6)

    def neighbours():
        a = g.fora_batch_topk(srcs, 8, EPS, ALPHA, 5)
        b = g.weighted_fora_batch(srcs, EPS, ALPHA, 5, fetch=True)
        return a[0], a[1], b[0]

    before = neighbours()
    _check_call(pkg, g, ("rmat12", "mixed"), srcs, 8, 3)
    after = neighbours()
    for x, y in zip(before, after):
        assert np.array_equal(x, y) or np.max(np.abs(x - y)) <= TOL
    w2 = tq._rand_w(rmat12, 99)
    g.set_weights(w2)
    _check_call(pkg, g, ("rmat12", "mixed", "w2"), srcs, 8, 3)
    conf = pkg.conf_topk(rmat12.n, rmat12.m, 8, ALPHA)
    ref = _ref(("w2", 1803), rmat12, w2, [1803], None, EPS, conf, 4)
    keep = pkg.Results(g, 2)
    _, _, _, _, pq = g.weighted_fora_batch_topk([1803, 1803], 8, EPS, ALPHA, 4, per_query=True, keep=keep)
    assert (pq[0].rounds, pq[0].walks, pq[0].walk_steps) == (ref["rounds"], ref["walks"], ref["steps"])
    assert np.max(np.abs(keep.fetch(0) - ref["est"])) <= TOL
    keep.close()
    g.set_weights(w)


def test_fewer_workspaces(pkg, dev_cache, rmat12, monkeypatch):
    w = tq._rand_w(rmat12, 22)
    g = tq._graph(dev_cache, pkg, "rmat12", rmat12, w, dense_frac=_frac(rmat12, "mixed"))
    srcs = tb._cycled(_pool(rmat12), 17)
    monkeypatch.setenv("PPRHIP_BATCH_WORKSPACES", "3")
    _, _, _, st = _check_call(pkg, g, ("rmat12", "mixed"), srcs, 8, 3)
    assert st.dense_levels <= 3 * st.class_launches[5] and st.rounds <= 3 * st.class_launches[3]  # three columns at most


# ------------------------------------------------------------------------------------- 6. delivery and checks
def test_delivery_keep_and_padding(pkg, dev_cache, got):
    w = tq._rand_w(got, 21)
    g = tq._graph(dev_cache, pkg, "got", got, w)
    dead = int(np.flatnonzero(tq._deg(got) == 0)[0])
    srcs, k = [63, dead, 35], 5
    keep = pkg.Results(g, 4)
    ids, vals, n_out, st, pq = g.weighted_fora_batch_topk(srcs, k, EPS, ALPHA, 3, per_query=True, keep=keep)
    # a dead-end source: rounds 0, the estimate is e_s, one entry and a padded row
    assert pq[1].rounds == 0 and n_out[1] == 1 and ids[1].tolist() == [dead] + [-1] * (k - 1)
    assert vals[1].tolist() == [1.0] + [0.0] * (k - 1)
    for i, s in enumerate(srcs):
        _, _, _, est, _ = _single(g, ("got", "default"), s, k, 3 + i)
        vec = keep.fetch(i)
        assert np.max(np.abs(vec - est)) <= TOL
        sid, sval, scnt = keep.fetch_sparse(i, 0.0, "id")
        assert np.array_equal(sid, np.flatnonzero(vec > 0)) and np.array_equal(sval, vec[vec > 0]) and scnt == sid.size
        order, vol, cut, info = keep.sweep_cut(i)
        g.weighted_fora_topk(s, EPS, ALPHA, k, 3 + i)
        order1, vol1, cut1, info1 = g.sweep_cut()
        assert info.best_size == info1.best_size and np.array_equal(order[:info.best_size], order1[:info1.best_size])
    with pytest.raises(pkg.PprhipError):  # the store holds 4: a call of 5 is refused before anything runs
        g.weighted_fora_batch_topk([63] * 5, k, EPS, ALPHA, 3, keep=keep)
    ids0, vals0, n0, st0 = g.weighted_fora_batch_topk([], k, EPS, ALPHA, 3, keep=keep)  # q = 0
    assert ids0.shape == (0, k) and st0.rounds == 0 and st0.walks == 0
    keep.close()


def test_needs_weights_and_a_bad_query_leaves_the_handle_untouched(pkg, dev_cache, got):
    with pkg.Graph(got, device=0) as g0:
        for call in (lambda: g0.weighted_fora_batch_topk([63, 35], 5, EPS, ALPHA, 3),
                     lambda: g0.weighted_fora_batch_topk_seeds([[63], [35, 3]], 5, EPS, ALPHA, 3)):
            with pytest.raises(pkg.PprhipError, match="no relationship weights") as ei:
                call()
            assert ei.value.code == pkg.ERR_STATE
    w = tq._rand_w(got, 21)
    g = tq._graph(dev_cache, pkg, "got", got, w)
    usual = _single(g, ("got", "default"), 63, 5, 3)
    with pytest.raises(pkg.PprhipError, match="pprhip_weighted_fora_batch_topk") as ei:
        g.weighted_fora_batch_topk([63, got.n, 35], 5, EPS, ALPHA, 3)
    assert ei.value.code == pkg.ERR_INVALID
    with pytest.raises(pkg.PprhipError, match="set 1") as ei:
        g.weighted_fora_batch_topk_seeds([[63], [35, -1], [3]], 5, EPS, ALPHA, 3)
    assert ei.value.code == pkg.ERR_INVALID
    with pytest.raises(pkg.PprhipError, match="set 2") as ei:
        g.weighted_fora_batch_topk_seeds([[63], [35], [3, 4]], 5, EPS, ALPHA, 3, weights=[None, None, [1.0, -2.0]])
    assert ei.value.code == pkg.ERR_INVALID
    nsel, ids, vals, est, st = g.weighted_fora_topk(63, EPS, ALPHA, 5, 3, fetch=True)
    assert nsel == usual[0] and np.array_equal(ids, usual[1]) and np.max(np.abs(est - usual[3])) <= TOL
    assert _decisions(st) == _decisions(usual[4])
