"""The weighted backward direction on the GPU (include/pprhip.h "weighted relationships", the backward direction): the
weighted backward push (sparse and dense levels), the survival vector, single targets / target sets and single pairs
over P(u, v) = w / W(u) against the numpy references of tests/weighted_bwd_ref.py, the designed graphs of
tests/weighted_bwd_designs.py at the kernels' edges, and the state of the handle around the calls.  1e-12 is the
project's bar for "same arithmetic, other addition order".  Levels and pops are compared only where the reference
compared no value closer to rmax than 1e-9 (relative): a condition on the inputs, asserted here."""
import ctypes as C

import numpy as np
import pytest

import targets_ref
import weighted_bwd_ref as br
import weighted_ref as wr
from conftest import shared_graph, to_oracle
from weighted_bwd_designs import (PAIR_EPS, PAIR_RMAX, PAIR_SEED, PAIR_W_SEED, design_weights, guarantee_pairs,
                                  reversed_dense_design, reversed_sparse_design)

ALPHA = 0.15
TOL = 1e-12
MARGIN = 1e-9
pytestmark = pytest.mark.gpu

ALL_SPARSE, ALL_DENSE = 1e9, 1e-12  # dense_frac: no level reaches it / every level does
MODES = {"sparse": (ALL_SPARSE, "none"), "dense": (ALL_DENSE, "all"), "default": (None, None)}


def _indeg(host):
    return np.diff(host.in_rp.astype(np.int64))


def _outdeg(host):
    return np.diff(host.out_rp.astype(np.int64))


def _rand_w(host, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, host.m)


def _graph(dev_cache, pkg, name, host, w=None, dense_frac=None, gs_blocks=None):
    """The module's handle of `host` with the given weights (None: left as they are) and tuning (None: the default)."""
    g = shared_graph(dev_cache, pkg, name, lambda: pkg.Graph(host, device=0))
    t = pkg.tuning_default()
    if dense_frac is not None:
        t.dense_frac = dense_frac
    if gs_blocks is not None:
        t.gs_blocks = gs_blocks
    g.set_tuning(t)
    if w is not None:
        g.set_weights(w)
    return g


_EXACT = {}


def _exact(name, host, w, alpha=ALPHA):
    """(pi, S_w) of (graph, weights, alpha), computed once per module run and left unchanged."""
    key = (name, alpha)
    if key not in _EXACT:
        leak = br.leaking_exact(host, w, alpha)
        S = leak.sum(axis=1)
        _EXACT[key] = (w.copy(), leak / S[:, None], S)
    assert np.array_equal(_EXACT[key][0], w)
    return _EXACT[key][1], _EXACT[key][2]


def _special_targets(host, need_all=False):
    """Largest in-degree, a node without in-edges, a dead end with in-edges, an isolated node, a self loop - those the
    graph has (need_all: all five)."""
    ind, outd = _indeg(host), _outdeg(host)
    src = np.repeat(np.arange(host.n), outd)
    kinds = [np.array([np.argmax(ind)]), np.flatnonzero((ind == 0) & (outd > 0)), np.flatnonzero((outd == 0) & (ind > 0)),
             np.flatnonzero((ind == 0) & (outd == 0)), src[src == host.out_ci[:host.m]]]
    assert not need_all or all(k.size for k in kinds)
    return [int(k[0]) for k in kinds if k.size]


def _check_bpush(g, host, w, t, rmax, tag, expect_dense=None):
    ref_p, ref_r, levels, pops, margin = br.bpush_sync(host, w, t, None, ALPHA, rmax, "push")
    assert margin >= MARGIN, ("the inputs put a value next to rmax", tag, t, rmax, margin)
    p, r, st = g.weighted_backward_push(t, ALPHA, rmax)
    assert st.levels == levels and st.pops + st.dense_nodes == pops, (tag, t, rmax, st.levels, levels, st.pops, pops)
    ep, er = float(np.max(np.abs(p - ref_p))), float(np.max(np.abs(r - ref_r)))
    assert ep <= TOL and er <= TOL, (tag, t, rmax, ep, er)
    assert st.rounds == 1 and st.rmax_final == rmax
    if expect_dense == "none":
        assert st.dense_levels == 0, (tag, t)
    elif expect_dense == "all":
        assert st.dense_levels == st.levels, (tag, t)
    if _indeg(host)[t] == 0:
        assert p[t] == 1.0 and p.sum() == 1.0 and not r.any() and st.levels == 0
    return p, r, st


# ---------------------------------------------------------------------------------------------- 1. push
@pytest.mark.parametrize("mode", list(MODES))
def test_backward_push_against_the_level_reference(pkg, dev_cache, got, toy_graphs, rmat12, mode):
    frac, expect = MODES[mode]
    cases = [(name, host, _rand_w(host, 3 + i)) for i, (name, host) in enumerate(sorted(toy_graphs.items()))]
    cases += [("got", got, _rand_w(got, 21)), ("rmat12", rmat12, _rand_w(rmat12, 22))]
    for name, host, w in cases:
        g = _graph(dev_cache, pkg, name, host, w, dense_frac=frac)
        targets = _special_targets(host, need_all=True) if name == "rmat12" else range(host.n)
        for t in targets:
            for rmax in (1e-2, 1e-5):
                _check_bpush(g, host, w, t, rmax, (name, mode), expect)


def test_results_of_a_backward_push_stay_on_the_handle(pkg, dev_cache, got):
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w)
    t = int(np.argmax(_indeg(got)))
    p, r, _ = g.weighted_backward_push(t, ALPHA, 1e-5)
    assert np.array_equal(g.reserve(), p) and np.array_equal(g.residue(), r)
    ids, vals, cnt = g.reserve_sparse(0.0, "id")
    assert cnt == np.count_nonzero(p) and np.array_equal(vals, p[ids])
    n_sel, sel_ids, sel_vals = g.topk_select(5)[:3]
    cnt5, row_i, row_v = targets_ref.topk_rows(p, 5)
    m5 = min(cnt5, 5)
    assert n_sel == cnt5 and np.array_equal(sel_ids[:m5], row_i[:m5]) and np.array_equal(sel_vals[:m5], row_v[:m5])
    assert g.sweep_cut(cap=0)[3].support == np.count_nonzero(p)


# ---------------------------------------------------------------------------------------------- 2. designed graphs
@pytest.mark.parametrize("mode", list(MODES))
def test_designed_dense_rows_at_chunk_edges(pkg, dev_cache, mode):
    """Out-rows on, across one and across two chunk boundaries, the last chunk not full: pushes from pool nodes (the
    rows A, B, C, Z receive), from the rows themselves and from small nodes; then the whole pool as one weighted target
    set, so that every edge of the long rows carries a contribution in the first level."""
    frac, expect = MODES[mode]
    host, d = reversed_dense_design(pkg)
    w = design_weights(host, 43)
    g = _graph(dev_cache, pkg, "rdense", host, w, dense_frac=frac)
    for t in [d["pool"][0], d["pool"][511], d["pool"][512], d["pool"][1099], d["A"], d["B"], d["C"], d["Z"], d["small"][3],
              d["isolated"]]:
        _check_bpush(g, host, w, t, 1e-7, ("rdense", mode), expect)
    pool = np.array(d["pool"])
    sw = np.random.default_rng(44).uniform(0.2, 1.0, pool.size)
    rmax = 1e-6
    ref_p, _, levels, pops, margin = br.bpush_sync(host, w, pool, sw, ALPHA, rmax, "pair")
    assert margin >= MARGIN
    S = br.survival_exact(host, w, ALPHA)
    values, _, st, pq = g.weighted_ppr_target_sets([pool], ALPHA, rmax, weights=[sw])
    assert pq[0].levels == levels and pq[0].pops + pq[0].dense_nodes == pops
    assert np.max(np.abs(values[0] - ref_p / S)) <= TOL
    if expect == "all":
        assert pq[0].dense_levels == levels


@pytest.mark.parametrize("mode", list(MODES))
def test_designed_sparse_targets_at_wave_stage_and_tile_edges(pkg, dev_cache, mode):
    """Targets of in-degree 1, 2, 3, 63, 64, 65, 1 500 and 2 500; the hub's second level has more than one LDS stage of
    nodes and more than one tile of in-edges (pinned in tests/test_weighted_bwd_ref.py)."""
    frac, expect = MODES[mode]
    host, by_deg = reversed_sparse_design(pkg)
    w = design_weights(host, 41)
    g = _graph(dev_cache, pkg, "rsparse", host, w, dense_frac=frac)
    for deg, t in sorted(by_deg.items()):
        assert _indeg(host)[t] == deg
        _check_bpush(g, host, w, t, 1e-7, ("rsparse", mode, deg), expect)


# ---------------------------------------------------------------------------------------------- 3. anchors
@pytest.mark.parametrize("weight", [0.5, 4.0])
def test_power_of_two_weights_are_the_unweighted_backward_push(pkg, orc, dev_cache, got, rmat12, weight):
    """Every weight one power of two: (c * w) / W is bit for bit c / d_out, so the weighted push is backward_push under
    gs_blocks = 1 and the oracle's sync schedule: same levels and pops, vectors within 1e-12."""
    for name, host in (("got", got), ("rmat12", rmat12)):
        g = _graph(dev_cache, pkg, name, host, np.full(host.m, weight), gs_blocks=1)
        og = to_oracle(orc, host)
        for t in _special_targets(host):
            for rmax in (1e-4, 1e-7):
                p0, r0, st0 = g.backward_push(t, ALPHA, rmax)
                p1, r1, st1 = g.weighted_backward_push(t, ALPHA, rmax)
                po, ro, sto = og.backward_push(t, ALPHA, rmax)
                assert st1.levels == st0.levels == sto.levels, (name, t, rmax)
                assert st1.pops + st1.dense_nodes == st0.pops + st0.dense_nodes == sto.pops + sto.dense_nodes
                for a, b in ((p1, p0), (r1, r0), (p1, po), (r1, ro)):
                    assert np.max(np.abs(a - b)) <= TOL, (name, t, rmax)


def test_integer_weights_are_the_multigraph(pkg, dev_cache, got, rmat12):
    """Integer weights against backward_push on the handle of the expanded multigraph."""
    for name, host in (("got", got), ("rmat12", rmat12)):
        w = np.random.default_rng(31).integers(1, 4, host.m).astype(np.float64)
        src = np.repeat(np.arange(host.n), _outdeg(host))
        rep = w.astype(np.int64)
        multi = pkg.HostCsr(host.n, np.repeat(src, rep).astype(np.int32),
                            np.repeat(host.out_ci[:host.m], rep).astype(np.int32))
        g = _graph(dev_cache, pkg, name, host, w)
        with pkg.Graph(multi, device=0) as gm:
            for t in _special_targets(host):
                a, ra, _ = g.weighted_backward_push(t, ALPHA, 1e-6)
                b, rb, _ = gm.backward_push(t, ALPHA, 1e-6)
                assert np.max(np.abs(a - b)) <= TOL and np.max(np.abs(ra - rb)) <= TOL, (name, t)


# ---------------------------------------------------------------------------------------------- 4. survival
def test_survival_against_the_exact_solve(pkg, dev_cache, got, toy_graphs, rmat12):
    host_d, _ = reversed_dense_design(pkg)
    cases = [(name, host, _rand_w(host, 3 + i)) for i, (name, host) in enumerate(sorted(toy_graphs.items()))]
    cases += [("got", got, _rand_w(got, 21)), ("rmat12", rmat12, _rand_w(rmat12, 22)),
              ("rdense", host_d, design_weights(host_d, 43))]
    for name, host, w in cases:
        g = _graph(dev_cache, pkg, name, host, w)
        S = g.weighted_walk_survival(ALPHA)
        ref = _exact(name, host, w)[1] if name == "rmat12" else br.survival_exact(host, w, ALPHA)
        err = float(np.max(np.abs(S - ref)))
        print("%s: |S_w - exact| %.2e" % (name, err))
        assert err <= TOL, name
        assert (S[_outdeg(host) == 0] == ALPHA).all()


def test_survival_is_kept_per_alpha_and_goes_with_the_weights(pkg, got):
    w = _rand_w(got, 21)
    with pkg.Graph(got, device=0) as g, pkg.Graph(got, device=0) as plain:
        g.set_weights(w)
        s1 = g.weighted_walk_survival(ALPHA)
        s2 = g.weighted_walk_survival(ALPHA)  # the kept vector: the same bits
        assert np.array_equal(s1, s2)
        s5 = g.weighted_walk_survival(0.5)    # another alpha recomputes
        assert np.max(np.abs(s5 - br.survival_exact(got, w, 0.5))) <= TOL and not np.array_equal(s5, s1)
        assert np.max(np.abs(g.weighted_walk_survival(ALPHA) - s1)) <= 1e-14
        w2 = _rand_w(got, 77)
        g.set_weights(w2)                     # other weights recompute
        s3 = g.weighted_walk_survival(ALPHA)
        assert np.max(np.abs(s3 - br.survival_exact(got, w2, ALPHA))) <= TOL and np.max(np.abs(s3 - s1)) > 1e-6
        # the unweighted survival is a vector of its own, beside the weighted one
        assert np.array_equal(g.walk_survival(ALPHA), plain.walk_survival(ALPHA))
        assert np.array_equal(g.weighted_walk_survival(ALPHA), s3)
        assert pkg.lib().pprhip_weighted_walk_survival(g.h, ALPHA, None) == pkg.OK  # survival_out may be NULL


# ---------------------------------------------------------------------------------------------- 5. targets
class _closing:
    def __init__(self, obj):
        self.obj = obj

    def __enter__(self):
        return self.obj

    def __exit__(self, *a):
        self.obj.close()


def _bound(pi_col, value, rmax, tag):
    diff = pi_col - value
    assert diff.min() >= -TOL and diff.max() <= rmax + TOL, (tag, float(diff.min()), float(diff.max()))


def test_targets_bound_on_got(pkg, dev_cache, got):
    """-1e-12 <= pi - value <= rmax + 1e-12 for every GOT target at three alphas and two thresholds."""
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w)
    for alpha in (0.05, 0.15, 0.5):
        pi, _ = _exact("got", got, w, alpha)
        for rmax in (1e-2, 1e-5):
            values, _, st, pq = g.weighted_ppr_targets(np.arange(got.n), alpha, rmax)
            assert st.rmax_final == rmax and len(pq) == got.n and all(s.rounds == 1 for s in pq)
            for t in range(got.n):
                _bound(pi[:, t], values[t], rmax, (alpha, rmax, t))


def _rmat_targets(host):
    ind, outd = _indeg(host), _outdeg(host)
    rng = np.random.default_rng(8)
    t = list(np.argsort(-ind)[:8]) + _special_targets(host) + list(np.flatnonzero((ind == 0) & (outd > 0))[:6]) + \
        list(np.flatnonzero((outd == 0) & (ind > 0))[:6])
    t = list(dict.fromkeys(int(x) for x in t + list(rng.permutation(host.n))))  # distinct, the special ones first
    return np.array(t[:64], dtype=np.int32)


def test_targets_bound_on_rmat12_and_reserve_identity(pkg, dev_cache, rmat12):
    host, w = rmat12, _rand_w(rmat12, 22)
    g = _graph(dev_cache, pkg, "rmat12", host, w)
    pi, S = _exact("rmat12", host, w)
    t = _rmat_targets(host)
    rmax = 1e-4
    values, _, _, _ = g.weighted_ppr_targets(t, ALPHA, rmax)
    Sd = g.weighted_walk_survival(ALPHA)
    for i, ti in enumerate(t):
        _bound(pi[:, ti], values[i], rmax, int(ti))
    for i in (0, 3, 20, 40):  # value * S_w is the backward push's reserve for a target with in-edges
        if _indeg(host)[t[i]] > 0:
            p, _, _ = g.weighted_backward_push(int(t[i]), ALPHA, rmax)
            assert np.max(np.abs(values[i] * Sd - p)) <= TOL
    # a target's vector is the same alone and inside a call of 20
    for i in (1, 9, 19):
        alone, _, _, _ = g.weighted_ppr_targets([int(t[i])], ALPHA, rmax)
        assert np.max(np.abs(alone[0] - values[i])) <= TOL
    lone = int(np.flatnonzero((_indeg(host) == 0) & (_outdeg(host) > 0))[0])
    v, _, _, pq = g.weighted_ppr_targets([lone], ALPHA, rmax)
    assert np.count_nonzero(v[0]) == 1 and abs(v[0][lone] - ALPHA / S[lone]) <= TOL and pq[0].levels == 0


def test_target_sets(pkg, dev_cache, got, rmat12):
    """Weights, duplicates, zero weights, members at or below rmax, members without in-edges; sets of 2 047 / 2 048 /
    2 049 members (the tile edge of the start kernel)."""
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w)
    pi, S = _exact("got", got, w)
    rmax = 1e-3
    ind = _indeg(got)
    lone = np.flatnonzero(ind == 0)
    sets = [[3, 5, 3, 9], [1, 2, 4], [int(lone[0]), 7, int(lone[-1])], list(range(40))]
    ws = [[0.5, 1.0, 0.25, 2.0], [1.0, 0.0, rmax], [0.7, rmax * 0.5, 1.3], np.linspace(0.1, 1.0, 40)]
    values, _, _, pq = g.weighted_ppr_target_sets(sets, ALPHA, rmax, weights=ws)
    for i, (ids, sw) in enumerate(zip(sets, ws)):
        _bound(targets_ref.set_exact(pi, ids, sw), values[i], rmax, i)
        ref_p, _, levels, pops, margin = br.bpush_sync(got, w, ids, sw, ALPHA, rmax, "pair")
        assert np.max(np.abs(values[i] - ref_p / S)) <= TOL
        if margin >= MARGIN:
            assert pq[i].levels == levels and pq[i].pops + pq[i].dense_nodes == pops
    host, w12 = rmat12, _rand_w(rmat12, 22)
    g12 = _graph(dev_cache, pkg, "rmat12", host, w12)
    pi12, S12 = _exact("rmat12", host, w12)
    perm = np.random.default_rng(12).permutation(host.n)
    for size in (2047, 2048, 2049):
        ids = perm[:size]
        sw = np.random.default_rng(size).uniform(0.0, 2e-4, size)  # about half the members at or below rmax = 1e-4
        v, _, _, _ = g12.weighted_ppr_target_sets([ids], ALPHA, 1e-4, weights=[sw])
        _bound(targets_ref.set_exact(pi12, ids, sw), v[0], 1e-4, size)
        ref_p = br.bpush_sync(host, w12, ids, sw, ALPHA, 1e-4, "pair")[0]
        assert np.max(np.abs(v[0] - ref_p / S12)) <= TOL, size


def test_targets_topk_and_kept_vectors(pkg, dev_cache, got):
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w)
    t = np.array([0, 5, int(np.argmax(_indeg(got))), int(np.flatnonzero(_indeg(got) == 0)[0]), 17, 42], dtype=np.int32)
    k = 8
    with _closing(pkg.Results(g, t.size)) as keep:
        values, sel, _, _ = g.weighted_ppr_targets(t, ALPHA, 1e-5, k=k, keep=keep)
        ids, vals, n_sel = sel
        assert keep.info()[1] == t.size
        for i in range(t.size):
            cnt, row_i, row_v = targets_ref.topk_rows(values[i], k)
            assert n_sel[i] == cnt and np.array_equal(ids[i], row_i) and np.array_equal(vals[i], row_v), i
            assert np.array_equal(keep.fetch(i), values[i])
            sid, sval, scnt = keep.fetch_sparse(i, 0.0, "id")
            assert scnt == np.count_nonzero(values[i]) and np.array_equal(sval, values[i][sid])
            assert keep.sweep_cut(i, cap=0)[3].support == np.count_nonzero(values[i])
        # without values_out the kept vectors are the only delivery
        none, _, _, _ = g.weighted_ppr_targets(t[:2], ALPHA, 1e-5, keep=keep, fetch=False)
        assert none is None and keep.info()[1] == 2 and np.array_equal(keep.fetch(1), values[1])


# ---------------------------------------------------------------------------------------------- 6. pairs
def _omega(conf, eps):
    return 3.0 * np.log(2.0 / conf.pfail) / (eps * eps) / conf.delta


def _device_pair_values(g, host, ss, tt, n_walks, rmax, seed):
    """pair_value from the device's own parts: weighted_backward_push, weighted_walk_survival and
    weighted_random_walks at the pair stream."""
    S = g.weighted_walk_survival(ALPHA)
    ind, outd = _indeg(host), _outdeg(host)
    out = np.zeros(ss.size)
    term_of = {}
    for t in np.unique(tt):
        if ind[t] == 0:  # the pair rule: p(t) = alpha, no residue, no walks
            p, r = np.zeros(host.n), np.zeros(host.n)
            p[t] = ALPHA
        else:
            p, r, _ = g.weighted_backward_push(int(t), ALPHA, rmax)
        for i in np.flatnonzero(tt == t):
            s = int(ss[i])
            v = p[s] / S[s]
            if ind[t] > 0 and n_walks:
                if s not in term_of:
                    term_of[s], _ = g.weighted_random_walks(np.full(n_walks, s, dtype=np.int32),
                                                            np.arange(n_walks, dtype=np.uint64), ALPHA, seed,
                                                            stream=br.PAIR_WALK_STREAM, no_zero_hop=False)
                v += r[term_of[s]].sum() / float(n_walks)
            out[i] = v
    return out


@pytest.mark.parametrize("n_walks", [1, 63, 64, 65, 2500])
def test_pairs_identity_at_every_walk_count(pkg, dev_cache, got, n_walks):
    """value = p_t(s) / S_w(s) + (1 / w) sum r_t(V_i), from the device's own push, survival and walks, to 1e-12: walk
    counts at the wave's edges and one that spans several work items; shared targets, shared sources, duplicate pairs,
    a dead-end source, a target without in-edges."""
    host, w = got, _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", host, w)
    conf = pkg.conf_whole_graph(host.n, host.m, ALPHA)
    eps = 0.5
    rmax = (n_walks - 0.5) / _omega(conf, eps)
    assert pkg.pair_params(conf, eps, rmax)[1] == n_walks
    ind, outd = _indeg(host), _outdeg(host)
    dead, lone, hub = int(np.flatnonzero(outd == 0)[0]), int(np.flatnonzero(ind == 0)[0]), int(np.argmax(ind))
    ss = np.array([0, 1, 2, 0, 0, dead, 5, 5, 9, 11, hub, 3], dtype=np.int32)
    tt = np.array([hub, hub, hub, 7, 7, hub, 8, 8, lone, lone, 12, dead], dtype=np.int32)
    seed = 17
    vals, st = g.weighted_ppr_pairs(ss, tt, eps, ALPHA, seed, rmax=rmax)
    want = _device_pair_values(g, host, ss, tt, n_walks, rmax, seed)
    assert np.max(np.abs(vals - want)) <= TOL, (n_walks, float(np.max(np.abs(vals - want))))
    walked = int((ind[tt] > 0).sum())
    assert st.walks == n_walks * walked and st.rmax_final == rmax and abs(st.omega - _omega(conf, eps)) <= 1e-9 * st.omega
    assert st.rounds == np.unique(tt).size and st.push_ms >= 0.0 and st.mc_ms >= 0.0
    assert vals[6] == vals[7] and vals[3] == vals[4]  # duplicate pairs: the same bits (no atomics on a pair's value)
    # a pair's value is the same alone and in the call
    for i in (0, 5, 10):
        one, _ = g.weighted_ppr_pairs([int(ss[i])], [int(tt[i])], eps, ALPHA, seed, rmax=rmax)
        assert abs(one[0] - vals[i]) <= TOL
    # a target without in-edges: exact, no walks
    only, st0 = g.weighted_ppr_pairs([lone, 4], [lone, lone], eps, ALPHA, seed, rmax=rmax)
    S = g.weighted_walk_survival(ALPHA)
    assert st0.walks == 0 and abs(only[0] - ALPHA / S[lone]) <= TOL and only[1] == 0.0


def test_pairs_more_than_one_launch_block(pkg, dev_cache, got):
    """One target with more pairs than one walk launch takes (2^19 chunk sums at one work item per pair)."""
    host, w = got, _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", host, w)
    conf = pkg.conf_whole_graph(host.n, host.m, ALPHA)
    rmax = 0.5 / _omega(conf, 0.5)  # w = 1
    q = (1 << 19) + 1000
    hub = int(np.argmax(_indeg(host)))
    ss = (np.arange(q) % host.n).astype(np.int32)
    tt = np.full(q, hub, dtype=np.int32)
    vals, st = g.weighted_ppr_pairs(ss, tt, 0.5, ALPHA, 5, rmax=rmax)
    assert st.walks == q
    want = _device_pair_values(g, host, np.arange(host.n, dtype=np.int32), np.full(host.n, hub, dtype=np.int32), 1, rmax, 5)
    assert np.max(np.abs(vals - want[ss])) <= TOL


def test_pairs_guarantee_on_got(pkg, dev_cache, got):
    """|value - pi| <= eps * max(pi, delta) at the inputs for which the numpy reference alone meets it
    (tests/test_weighted_bwd_ref.py), and the device's values are the reference's."""
    host = got
    w = design_weights(host, PAIR_W_SEED)
    g = _graph(dev_cache, pkg, "got_pairs", host, w)
    conf = pkg.conf_whole_graph(host.n, host.m, ALPHA)
    rmax, n_walks = pkg.pair_params(conf, PAIR_EPS, PAIR_RMAX)
    assert n_walks <= 2000
    pi = br.ppr_exact(host, w, ALPHA)
    ss, tt = guarantee_pairs(host)
    vals, st = g.weighted_ppr_pairs(ss, tt, PAIR_EPS, ALPHA, PAIR_SEED, rmax=PAIR_RMAX)
    assert st.rmax_final == rmax
    exact = pi[ss, tt]
    ratio = np.abs(vals - exact) / (PAIR_EPS * np.maximum(exact, conf.delta))
    print("pair guarantee on the device: worst |err| / bound = %.3f" % float(ratio.max()))
    assert (ratio <= 1.0).all()
    S = br.survival_exact(host, w, ALPHA)
    tab = wr.table(host, w)
    for i in range(0, ss.size, 7):
        p, r, _, _, _ = br.bpush_sync(host, w, int(tt[i]), None, ALPHA, rmax, "pair")
        ref = br.pair_value(host, w, p, r, S, int(ss[i]), int(n_walks), ALPHA, PAIR_SEED, tab)
        assert abs(vals[i] - ref) <= TOL, i


# ---------------------------------------------------------------------------------------------- 7. state
def _new_calls(g):
    return [lambda: g.weighted_backward_push(0, ALPHA, 1e-4), lambda: g.weighted_walk_survival(ALPHA),
            lambda: g.weighted_ppr_targets([0, 1], ALPHA, 1e-4), lambda: g.weighted_ppr_target_sets([[0, 1]], ALPHA, 1e-4),
            lambda: g.weighted_ppr_pairs([0], [1], 0.5, ALPHA, 3)]


def test_state_errors_leave_the_handle(pkg, got):
    n = got.n
    src = int(np.argmax(_outdeg(got)))
    with pkg.Graph(got, device=0) as g:
        before, _, _, _ = g.forward_push(src, ALPHA, 1e-6)
        for call in _new_calls(g):  # no weights
            with pytest.raises(pkg.PprhipError) as e:
                call()
            assert e.value.code == pkg.ERR_STATE and "no relationship weights" in str(e.value)
        g.set_weights(_rand_w(got, 21))
        qs = pkg.QueryStream(g, 0.5, ALPHA)
        try:
            for call in _new_calls(g):  # a query stream open
                with pytest.raises(pkg.PprhipError) as e:
                    call()
                assert e.value.code == pkg.ERR_STATE
        finally:
            qs.close()
        bad = [lambda: g.weighted_backward_push(n, ALPHA, 1e-4), lambda: g.weighted_backward_push(-1, ALPHA, 1e-4),
               lambda: g.weighted_ppr_targets([0, n + 3, 1], ALPHA, 1e-4),
               lambda: g.weighted_ppr_target_sets([[0], [1, n]], ALPHA, 1e-4),
               lambda: g.weighted_ppr_target_sets([[0], [1, 2]], ALPHA, 1e-4, weights=[[1.0], [1.0, -0.5]]),
               lambda: g.weighted_ppr_target_sets([[0], [1, 2]], ALPHA, 1e-4, weights=[[1.0], [0.0, 0.0]]),
               lambda: g.weighted_ppr_pairs([0, n], [1, 1], 0.5, ALPHA, 3), lambda: g.weighted_ppr_pairs([0, 1], [1, -2], 0.5, ALPHA, 3)]
        for i, call in enumerate(bad):
            with pytest.raises(pkg.PprhipError) as e:
                call()
            assert e.value.code == pkg.ERR_INVALID, i
            if 2 <= i <= 5:
                assert "set 1" in str(e.value) and "pprhip_weighted_ppr_targets" in str(e.value), str(e.value)
            if i >= 6:
                assert "pair 1" in str(e.value)
        # offsets that do not ascend name the set as well
        L = pkg.lib()
        t = np.array([0, 1, 2], dtype=np.int32)
        o = np.array([0, 2, 1, 3], dtype=np.uint64)
        st = pkg.Stats()
        rc = L.pprhip_weighted_ppr_targets(g.h, t.ctypes.data_as(C.c_void_p), None, o.ctypes.data_as(C.c_void_p), 3, ALPHA,
                                           1e-4, None, None, 0, None, None, None, None, C.byref(st))
        assert rc == pkg.ERR_INVALID and "set 1" in L.pprhip_last_error().decode()
        assert np.array_equal(g.reserve(), before)  # nothing ran: the result before is still there
        # empty calls
        v, sel, st, pq = g.weighted_ppr_targets(np.zeros(0, dtype=np.int32), ALPHA, 1e-4, k=3)
        assert v.shape == (0, n) and pq == [] and st.pops == 0
        pv, st = g.weighted_ppr_pairs([], [], 0.5, ALPHA, 3)
        assert pv.size == 0 and st.walks == 0


def test_bad_input_is_refused_alike_by_the_weighted_and_the_unweighted_call(pkg, got):
    """pprhip_weighted_ppr_targets / _ppr_pairs refuse what pprhip_ppr_targets / _ppr_pairs refuse, on one handle that
    has weights: the same return code, and the same message once the entry point's name is replaced.  Without weights
    every weighted call is PPRHIP_ERR_STATE and the unweighted one succeeds."""
    L = pkg.lib()
    n = got.n
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    i32 = lambda *x: np.array(x, dtype=np.int32)
    u64 = lambda *x: np.array(x, dtype=np.uint64)
    f64 = lambda *x: np.array(x, dtype=np.float64)

    def both(name, call):
        """call(entry point) for the unweighted and the weighted one: ((rc, message), (rc, message))."""
        res = []
        for fn_name in ("pprhip_" + name, "pprhip_weighted_" + name):
            rc = call(getattr(L, fn_name))
            res.append((rc, L.pprhip_last_error().decode() if rc != pkg.OK else ""))
        return res

    def targets(t, w, off, q, k=0, ids=None, vals=None, keep=None, values=None):
        st = pkg.Stats()
        return lambda fn: fn(g.h, vp(t), vp(w), vp(off), q, ALPHA, 1e-4, keep, vp(values), k, vp(ids), vp(vals), None, None,
                             C.byref(st))

    def pairs(s, t, q, out, conf, rmax=0.0):
        st = pkg.Stats()
        return lambda fn: fn(g.h, vp(s), vp(t), q, 0.5, C.byref(conf), rmax, 3, vp(out), C.byref(st))

    with pkg.Graph(got, device=0) as g, pkg.Graph(got, device=0) as other:
        g.set_weights(_rand_w(got, 21))
        conf = pkg.conf_whole_graph(got.n, got.m, ALPHA)
        many = pkg.conf_whole_graph(got.n, got.m, ALPHA)
        many.delta = 1e-16  # omega = 3 ln(2 / pfail) / (eps^2 delta) > 1e17 > 2^48 walks at rmax = 1
        out4 = np.zeros(4)
        with _closing(pkg.Results(other, 1)) as foreign:
            bad = [
                ("ppr_targets", "q < 0", targets(i32(0), None, None, -1), None),
                ("ppr_targets", "k > 0 without ids_out", targets(i32(0), None, None, 1, k=3), None),
                ("ppr_targets", "offsets[0] != 0", targets(i32(0, 1, 2), None, u64(1, 2, 3), 2), None),
                ("ppr_targets", "descending offsets", targets(i32(0, 1, 2), None, u64(0, 2, 1, 3), 3), "set 1"),
                ("ppr_targets", "an empty set", targets(i32(0, 1), None, u64(0, 1, 1, 2), 3), "set 1"),
                ("ppr_targets", "id n", targets(i32(0, 1, n), None, u64(0, 1, 2, 3), 3), "set 2"),
                ("ppr_targets", "negative weight", targets(i32(0, 1), f64(1.0, -0.5), None, 2), "set 1"),
                ("ppr_targets", "NaN weight", targets(i32(0, 1), f64(1.0, np.nan), None, 2), "set 1"),
                ("ppr_targets", "weights sum to 0", targets(i32(0, 1, 2), f64(1.0, 0.0, 0.0), u64(0, 1, 3), 2), "set 1"),
                ("ppr_targets", "keep of another graph", targets(i32(0), None, None, 1, keep=foreign.h), None),
                ("ppr_pairs", "NULL values_out", pairs(i32(0), i32(1), 1, None, conf), None),
                ("ppr_pairs", "source -1", pairs(i32(-1, 0), i32(1, 1), 2, out4, conf), "pair 0"),
                ("ppr_pairs", "target n", pairs(i32(0, 1, 2, 3), i32(1, 1, 1, n), 4, out4, conf), "pair 3"),
                ("ppr_pairs", "more than 2^48 walks", pairs(i32(0), i32(1), 1, out4, many, rmax=1.0), "2^48"),
            ]
            for name, what, call, names in bad:
                (rc_u, msg_u), (rc_w, msg_w) = both(name, call)
                assert rc_u == rc_w == pkg.ERR_INVALID, (what, rc_u, rc_w, msg_u, msg_w)
                assert msg_u.startswith("pprhip_%s: " % name), (what, msg_u)
                assert msg_w.replace("pprhip_weighted_" + name, "pprhip_" + name) == msg_u, (what, msg_u, msg_w)
                assert names is None or names in msg_u, (what, msg_u)
        g.release(pkg.Graph.RELEASE_WEIGHTS)
        values = np.zeros((1, n))
        for name, call in (("ppr_targets", targets(i32(0), None, None, 1, values=values)),
                           ("ppr_pairs", pairs(i32(0), i32(1), 1, out4, conf))):
            (rc_u, _), (rc_w, msg_w) = both(name, call)
            assert rc_u == pkg.OK and rc_w == pkg.ERR_STATE, (name, rc_u, rc_w, msg_w)
            assert msg_w.startswith("pprhip_weighted_%s: " % name) and "no relationship weights" in msg_w


def test_unweighted_backward_calls_ignore_the_weights(pkg, got):
    """backward_push, ppr_targets and ppr_pairs give what a weight-free handle gives, before and after weighted calls."""
    t = int(np.argmax(_indeg(got)))

    def run(g):
        p, r, _ = g.backward_push(t, ALPHA, 1e-6)
        v, _, _, _ = g.ppr_targets(np.arange(20), ALPHA, 1e-5)
        pv, _ = g.ppr_pairs(np.arange(30), np.arange(30)[::-1], 0.5, ALPHA, 9)
        return p, r, v, pv, g.walk_survival(ALPHA)

    with pkg.Graph(got, device=0) as plain, pkg.Graph(got, device=0) as g:
        ref = run(plain)
        g.set_weights(_rand_w(got, 21))
        g.weighted_ppr_targets([t], ALPHA, 1e-5)
        g.weighted_ppr_pairs([0], [t], 0.5, ALPHA, 9)
        during = run(g)
    for a, b in zip(ref, during):
        assert np.max(np.abs(a - b)) <= TOL
    assert np.array_equal(ref[4], during[4])


def test_release_gives_the_survival_back_and_three_lives_leave_nothing(pkg, rmat12):
    w = _rand_w(rmat12, 22)

    def life(g):
        g.set_weights(w)
        g.weighted_walk_survival(ALPHA)
        g.weighted_ppr_targets([1, 2], ALPHA, 1e-4, k=4)
        g.weighted_ppr_pairs([1, 2], [3, 4], 0.5, ALPHA, 3)
        g.weighted_backward_push(5, ALPHA, 1e-5)

    with pkg.Graph(rmat12, device=0) as probe:
        with pkg.Graph(rmat12, device=0) as g:
            life(g)  # first round: the allocator's own pools, the sweep layout over the out-CSR, the selection scratch
            g.release(pkg.Graph.RELEASE_WEIGHTS)
            free0, _ = g.device_memory()
            life(g)
            assert g.weights_info()[0]
            g.release(pkg.Graph.RELEASE_WEIGHTS)
            free1, _ = g.device_memory()
            assert free1 == free0 and g.weights_info() == (False, 0)
            life(g)
            g.set_weights(None)  # the drop frees the survival as well
            free2, _ = g.device_memory()
            assert free2 == free0
        base, _ = probe.device_memory()
        for _ in range(3):
            with pkg.Graph(rmat12, device=0) as g:
                life(g)
            left, _ = probe.device_memory()
            assert left == base
