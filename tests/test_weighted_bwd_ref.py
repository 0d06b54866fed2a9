"""The weighted backward direction's host references (tests/weighted_bwd_ref.py) pinned on the CPU, independently of
the engine: the exact push invariant against the weighted leaking inverse, powers of two against the oracle's
unweighted backward push level for level, integer weights against the expanded multigraph, the designed graphs'
placement on the host lift, and the pair guarantee of the reference alone at the inputs the GPU test uses."""
import numpy as np
import pytest

import weighted_bwd_ref as br
import weighted_ref as wr
from conftest import edges_to_host, to_oracle
from weighted_bwd_designs import (CHUNK, FILL, PAIR_EPS, PAIR_RMAX, PAIR_SEED, PAIR_W_SEED, STAGE, TILE, design_weights,
                                  guarantee_pairs, reversed_dense_design, reversed_sparse_design)

ALPHA = 0.15


def _graphs(got, toy_graphs):
    g = dict(toy_graphs)
    g["got"] = got
    return g


def _indeg(host):
    return np.diff(host.in_rp.astype(np.int64))


@pytest.mark.parametrize("rmax", [1e-2, 1e-5])
def test_push_invariant_against_the_leaking_inverse(got, toy_graphs, rmax):
    """pi'(., t) = p + sum_v pi'(., v) r(v) to 1e-13, for single targets (both start rules where they agree) and
    weighted sets; every residue <= rmax at the end."""
    rng = np.random.default_rng(5)
    for name, host in _graphs(got, toy_graphs).items():
        w = rng.uniform(0.5, 1.5, host.m)
        leak = br.leaking_exact(host, w, ALPHA)
        assert np.max(np.abs(leak.sum(axis=1) - br.survival_exact(host, w, ALPHA))) == 0.0
        assert np.max(np.abs(leak / leak.sum(axis=1, keepdims=True) - br.ppr_exact(host, w, ALPHA))) <= 1e-13
        indeg = _indeg(host)
        for t in range(host.n) if host.n <= 8 else range(0, host.n, 5):
            p, r, levels, pops, _ = br.bpush_sync(host, w, t, None, ALPHA, rmax, "pair")
            assert np.max(np.abs(leak[:, t] - (p + leak @ r))) <= 1e-13, (name, t)
            assert (r <= rmax).all()
            p2, r2, l2, q2, _ = br.bpush_sync(host, w, t, None, ALPHA, rmax, "push")
            if indeg[t] == 0:
                assert p2[t] == 1.0 and p2.sum() == 1.0 and not r2.any() and l2 == 0 and q2 == 0
                assert p[t] == ALPHA and p.sum() == ALPHA and not r.any() and levels == 0
            else:
                assert np.array_equal(p, p2) and np.array_equal(r, r2) and (levels, pops) == (l2, q2)
        ids = rng.integers(0, host.n, 9)
        ws = rng.uniform(0.0, 2.0, 9)
        ws[2] = 0.0            # dropped
        ids[4] = ids[1]        # a duplicate: summed
        ws[6] = rmax * 0.5     # stays residue unless a push lifts it
        p, r, _, _, _ = br.bpush_sync(host, w, ids, ws, ALPHA, rmax, "pair")
        assert np.max(np.abs(leak[:, ids] @ ws - (p + leak @ r))) <= 1e-13, name
        assert (r[indeg > 0] <= rmax).all()


@pytest.mark.parametrize("weight", [0.5, 4.0])
def test_power_of_two_weights_are_the_oracles_backward_push(orc, got, toy_graphs, rmat12, weight):
    """Every weight one power of two: (c * w) / W is bit for bit c / d_out, so bpush_sync is the oracle's
    frontier-synchronous backward push, level for level, with vectors equal."""
    t_ = orc.tuning_default()
    t_.gs_blocks = 1
    orc.set_sync_tuning(t_)
    try:
        graphs = _graphs(got, toy_graphs)
        graphs["rmat12"] = rmat12
        for name, host in graphs.items():
            og = to_oracle(orc, host)
            indeg = _indeg(host)
            w = np.full(host.m, weight)
            for t in sorted({0, host.n - 1, int(np.argmax(indeg)), int(np.argmin(indeg))}):
                for rmax in (1e-3, 1e-6):
                    p, r, st = og.backward_push(t, ALPHA, rmax)
                    reserve, residue, levels, pops, _ = br.bpush_sync(host, w, t, None, ALPHA, rmax, "push")
                    assert levels == st.levels and pops == st.pops + st.dense_nodes, (name, t, rmax)
                    assert np.max(np.abs(reserve - p)) <= 1e-15 and np.max(np.abs(residue - r)) <= 1e-15, (name, t, rmax)
    finally:
        orc.set_sync_tuning(None)


def test_integer_weights_are_the_multigraph(pkg, orc, got, toy_graphs):
    """Integer weights 1 .. 3 against the oracle's backward push on the graph with each relationship repeated."""
    rng = np.random.default_rng(11)
    for name, host in _graphs(got, toy_graphs).items():
        w = rng.integers(1, 4, host.m).astype(np.float64)
        src = np.repeat(np.arange(host.n), np.diff(host.out_rp.astype(np.int64)))
        rep = w.astype(np.int64)
        multi = edges_to_host(pkg, host.n, list(zip(np.repeat(src, rep).tolist(),
                                                    np.repeat(host.out_ci[:host.m], rep).tolist())))
        og = to_oracle(orc, multi)
        for t in range(host.n) if host.n <= 8 else range(0, host.n, 9):
            p, r, _ = og.backward_push(t, ALPHA, 1e-6)
            reserve, residue, _, _, _ = br.bpush_sync(host, w, t, None, ALPHA, 1e-6, "push")
            assert np.max(np.abs(reserve - p)) <= 1e-12 and np.max(np.abs(residue - r)) <= 1e-12, (name, t)


def test_designed_graphs_have_their_designed_layout(pkg):
    """The reversed dense design's out-rows sit at the chunk edges they are meant for (internal edge order of the host
    lift); the reversed sparse design's targets have the in-degrees they are named by, and the push from its hub has a
    level of more than one LDS stage of nodes and more than one tile of in-edges."""
    host, d = reversed_dense_design(pkg)
    L = pkg.lift_host(host)
    o2n, orp = L["old2new"], L["out_rp"].astype(np.int64)
    assert [int(o2n[d[k]]) for k in ("C", "Z", "B", "A")] == [0, 1, 2, 3]
    assert orp[1] == 1100 and orp[2] == 1100 + FILL and orp[3] == orp[2] + 513 and orp[4] == orp[3] + 512
    assert (orp[1] - 1) // CHUNK == 2                                     # C crosses two boundaries
    assert orp[2] % CHUNK == CHUNK - 1 and orp[3] % CHUNK == 0            # B: one edge before a boundary, ends on the next
    assert orp[3] % CHUNK == 0 and orp[4] % CHUNK == 0 and orp[4] - orp[3] == CHUNK  # A: exactly one chunk
    assert host.m % CHUNK != 0 and host.m // CHUNK >= 6                   # the last chunk is not full
    indeg, outdeg = _indeg(host), np.diff(host.out_rp.astype(np.int64))
    assert all(indeg[d[k]] > 0 for k in "ABCZ")
    assert outdeg[d["dead"]] == 0 and indeg[d["dead"]] > 0                # a dead end with in-edges
    assert outdeg[d["isolated"]] == 0 and indeg[d["isolated"]] == 0
    assert (indeg[outdeg > 0] == 0).any()                                 # a node without in-edges that has out-edges
    hs, by_deg = reversed_sparse_design(pkg)
    ind = _indeg(hs)
    assert all(ind[u] == k for k, u in by_deg.items()) and sorted(by_deg) == [1, 2, 3, 63, 64, 65, 1500, 2500]
    trace = []
    br.bpush_sync(hs, design_weights(hs, 41), by_deg[2500], None, ALPHA, 1e-7, "push", trace=trace)
    assert trace[0] == (1, 2500) and any(nf > STAGE and ef > TILE for nf, ef in trace)


def test_reference_meets_the_pair_guarantee_at_the_gpu_tests_inputs(pkg, got):
    """|value - pi| <= eps * max(pi, delta) for every pair of the GPU test, by the numpy reference alone, with
    w <= 2 000 walks per pair."""
    host = got
    w = design_weights(host, PAIR_W_SEED)
    conf = pkg.conf_whole_graph(host.n, host.m, ALPHA)
    rmax, n_walks = pkg.pair_params(conf, PAIR_EPS, PAIR_RMAX)
    assert 0 < n_walks <= 2000
    pi = br.ppr_exact(host, w, ALPHA)
    S = br.survival_exact(host, w, ALPHA)
    tab = wr.table(host, w)
    ss, tt = guarantee_pairs(host)
    assert ss.size >= 100
    worst = 0.0
    for t in np.unique(tt):
        p, r, _, _, _ = br.bpush_sync(host, w, int(t), None, ALPHA, rmax, "pair")
        for s in ss[tt == t]:
            v = br.pair_value(host, w, p, r, S, int(s), int(n_walks), ALPHA, PAIR_SEED, tab)
            err, bound = abs(v - pi[s, t]), PAIR_EPS * max(pi[s, t], conf.delta)
            worst = max(worst, err / bound)
            assert err <= bound, (int(s), int(t), v, pi[s, t])
    print("pair guarantee of the reference: worst |err| / bound = %.3f at w = %d, rmax = %.4g" % (worst, n_walks, rmax))
