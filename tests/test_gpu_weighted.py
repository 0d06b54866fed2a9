"""Weighted relationships on the GPU (include/pprhip.h "weighted relationships"): the power method, the forward push
(sparse and dense levels), the walks and FORA over P(u, v) = w / W(u) against the numpy references of
tests/weighted_ref.py, the designed graphs of tests/weighted_designs.py at the kernels' edges, and the weights' life on
the handle.  1e-12 is the project's bar for "same arithmetic, other addition order"."""
import numpy as np
import pytest

import weighted_ref as wr
from conftest import edges_to_host, shared_graph
from weighted_designs import dense_design, sparse_design

ALPHA = 0.15
TOL = 1e-12
pytestmark = pytest.mark.gpu

ALL_SPARSE, ALL_DENSE = 1e9, 1e-12  # dense_frac: no level reaches it / every level does


def _deg(host):
    return np.diff(host.out_rp.astype(np.int64))


def _rand_w(host, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, host.m)


def _isolated_mix_w(host):
    """isolated_mix: the parallel relationships 1 -> 2 carry different weights, the self loop 0 -> 0 a heavy one."""
    w = np.linspace(0.75, 3.0, host.m)
    return w


_EXACT = {}


def _exact(name, host, w):
    """ppr_exact of (graph, weights), computed once per module run (R-MAT 12 is a 4096 x 4096 solve); a name always
    comes with the same weights."""
    if name not in _EXACT:
        _EXACT[name] = (w.copy(), wr.ppr_exact(host, w, ALPHA))
    assert np.array_equal(_EXACT[name][0], w)
    return _EXACT[name][1]


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


def _restart_matrix(host, w, s, alpha):
    """Row v: the PPR vector of the walk from v that restarts at s on a dead end (tests/test_weighted_ref.py)."""
    Q = wr.transition(host, w)
    Q[_deg(host) == 0, s] = 1.0
    return alpha * np.linalg.inv(np.eye(host.n) - (1.0 - alpha) * Q)


def _sources(host, extra=()):
    deg = _deg(host)
    dead = np.flatnonzero(deg == 0)
    s = {int(np.argmax(deg)), int(np.flatnonzero(deg > 0)[0])} | set(extra)
    if dead.size:
        s.add(int(dead[0]))
    return sorted(s)


# ---------------------------------------------------------------------------------------------- power method
def _power_cases(got, toy_graphs, rmat12):
    return [("isolated_mix", toy_graphs["isolated_mix"], _isolated_mix_w(toy_graphs["isolated_mix"])),
            ("star_dead_leaves", toy_graphs["star_dead_leaves"], _rand_w(toy_graphs["star_dead_leaves"], 1)),
            ("got", got, _rand_w(got, 21)), ("rmat12", rmat12, _rand_w(rmat12, 22))]


def test_power_method_against_the_iteration_and_the_exact_solve(pkg, dev_cache, got, toy_graphs, rmat12):
    iters = 200
    for name, host, w in _power_cases(got, toy_graphs, rmat12):
        g = _graph(dev_cache, pkg, name, host, w)
        pi = _exact(name, host, w)
        srcs = range(host.n) if host.n <= 8 else _sources(host)
        for s in srcs:
            out, st = g.weighted_power_method(s, ALPHA, iters)
            ref = wr.power_iter(host, w, s, ALPHA, iters)
            err_it, err_pi = float(np.max(np.abs(out - ref))), float(np.max(np.abs(out - pi[s])))
            print("%s src %d: |gpu - power_iter| %.2e, |gpu - exact| %.2e" % (name, s, err_it, err_pi))
            assert err_it <= TOL, (name, s)
            assert err_pi <= (1.0 - ALPHA) ** iters + TOL, (name, s)
            assert st.rounds == iters and st.dense_levels == iters - 1


def test_power_method_few_iterations(pkg, dev_cache, got):
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w)
    s = _sources(got)[0]
    for iters in (0, 1, 2, 3):
        out, _ = g.weighted_power_method(s, ALPHA, iters)
        assert np.max(np.abs(out - wr.power_iter(got, w, s, ALPHA, iters))) <= TOL, iters


def test_power_method_integer_weights_are_the_multigraph(pkg, dev_cache, got, rmat12):
    """Integer weights against the existing power_method on the handle of the expanded multigraph."""
    for name, host in (("got", got), ("rmat12", rmat12)):
        w = np.random.default_rng(31).integers(1, 4, host.m).astype(np.float64)
        src = np.repeat(np.arange(host.n), _deg(host))
        rep = w.astype(np.int64)
        multi = pkg.HostCsr(host.n, np.repeat(src, rep).astype(np.int32),
                            np.repeat(host.out_ci[:host.m], rep).astype(np.int32))
        g = _graph(dev_cache, pkg, name, host, w)
        with pkg.Graph(multi, device=0) as gm:
            for s in _sources(host):
                a, _ = g.weighted_power_method(s, ALPHA, 100)
                b, _ = gm.power_method(s, ALPHA, 100)
                assert np.max(np.abs(a - b)) <= TOL, (name, s)


# ---------------------------------------------------------------------------------------------- forward push
def _check_push(g, host, w, s, rmax, tag, expect_dense=None):
    ref_p, ref_r, levels, pops = wr.push_sync(host, w, s, ALPHA, rmax)
    p, r, rsum, st = g.weighted_forward_push(s, ALPHA, rmax)
    assert st.levels == levels and st.pops + st.dense_nodes == pops, (tag, s, rmax, st.levels, levels)
    ep, er = float(np.max(np.abs(p - ref_p))), float(np.max(np.abs(r - ref_r)))
    assert ep <= TOL and er <= TOL, (tag, s, rmax, ep, er)
    assert abs(rsum - ref_r.sum()) <= TOL and st.rsum == rsum
    assert st.dead_end_pops == 0 or (_deg(host) == 0).any()
    if expect_dense == "none":
        assert st.dense_levels == 0, (tag, s)
    elif expect_dense == "all":
        assert st.dense_levels == st.levels, (tag, s)
    return p, r, st


@pytest.mark.parametrize("mode", ["sparse", "dense", "mixed"])
def test_forward_push_against_the_level_reference(pkg, dev_cache, got, toy_graphs, rmat12, mode):
    """Levels and pops equal, vectors within 1e-12 - with dense_frac so large that no level runs dense, so small that
    every one does, and at a value at which the first level (the source alone) runs sparse and wide levels dense: the
    sparse / dense equivalence and both changes of shape.  two_node: source 0's only neighbour is a dead end, source 1
    is one; star_dead_leaves: every neighbour is."""
    cases = [("two_node", toy_graphs["two_node"], _rand_w(toy_graphs["two_node"], 2)),
             ("star_dead_leaves", toy_graphs["star_dead_leaves"], _rand_w(toy_graphs["star_dead_leaves"], 1)),
             ("isolated_mix", toy_graphs["isolated_mix"], _isolated_mix_w(toy_graphs["isolated_mix"])),
             ("got", got, _rand_w(got, 21)), ("rmat12", rmat12, _rand_w(rmat12, 22))]
    hub_dense = 0
    for name, host, w in cases:
        deg = _deg(host)
        srcs = range(host.n) if host.n <= 8 else _sources(host)
        for s in srcs:
            if mode == "sparse":
                frac, expect = ALL_SPARSE, "none"
            elif mode == "dense":
                frac, expect = ALL_DENSE, "all"
            else:  # the first level (1 node + d edges) stays just below the threshold
                frac, expect = (deg[s] + 1.5) / host.m, None
            g = _graph(dev_cache, pkg, name, host, w, dense_frac=frac)
            for rmax in ((1e-2, 1e-7) if host.n <= 8 else (1e-4, 1e-7)):
                _, _, st = _check_push(g, host, w, s, rmax, (name, mode), expect)
                if mode == "mixed" and deg[s] > 0:
                    assert st.dense_levels < st.levels
                if name == "rmat12" and s == int(np.argmax(deg)):
                    hub_dense = max(hub_dense, st.dense_levels)
    if mode == "mixed":  # the hub of R-MAT 12: its second level is wide
        assert hub_dense > 0


def test_forward_push_exact_invariant(pkg, dev_cache, got, toy_graphs):
    """pi_s = reserve + sum_v r(v) pi_v against the dense solve (pi_v: the walk from v that restarts at s)."""
    for name, host, w in (("isolated_mix", toy_graphs["isolated_mix"], _isolated_mix_w(toy_graphs["isolated_mix"])),
                          ("got", got, _rand_w(got, 21))):
        pi = _exact(name, host, w)
        for frac in (ALL_SPARSE, ALL_DENSE):
            g = _graph(dev_cache, pkg, name, host, w, dense_frac=frac)
            for s in (range(host.n) if host.n <= 8 else _sources(host, extra=(17, 42))):
                M = _restart_matrix(host, w, s, ALPHA)
                for rmax in (1e-3, 1e-6):
                    p, r, _, _ = g.weighted_forward_push(s, ALPHA, rmax)
                    assert np.max(np.abs(pi[s] - (p + r @ M))) <= TOL, (name, s, rmax)
                    assert not wr.active(r, _deg(host), rmax).any() or _deg(host)[s] == 0


@pytest.mark.parametrize("weight", [4.0, 0.25])
def test_forward_push_power_of_two_weights_are_the_unweighted_push(pkg, dev_cache, got, rmat12, weight):
    """Weights all 4.0 / all 0.25: every product is exact, the weighted push is forward_push under gs_blocks = 1."""
    for name, host in (("got", got), ("rmat12", rmat12)):
        g = _graph(dev_cache, pkg, name, host, np.full(host.m, weight), gs_blocks=1)
        for s in _sources(host):
            for rmax in (1e-4, 1e-7):
                p0, r0, rsum0, st0 = g.forward_push(s, ALPHA, rmax)
                p1, r1, rsum1, st1 = g.weighted_forward_push(s, ALPHA, rmax)
                assert st1.levels == st0.levels and st1.pops + st1.dense_nodes == st0.pops + st0.dense_nodes, (name, s, rmax)
                assert st1.dense_levels == st0.dense_levels and st1.dead_end_pops == st0.dead_end_pops
                assert np.max(np.abs(p1 - p0)) <= TOL and np.max(np.abs(r1 - r0)) <= TOL, (name, s, rmax)
                assert abs(rsum1 - rsum0) <= TOL


# ---------------------------------------------------------------------------------------------- designed graphs
def test_dense_kernel_on_the_designed_graph(pkg, dev_cache):
    """tests/weighted_designs.py: dense_design - a row that starts on a chunk boundary, rows crossing one and two
    boundaries, a last chunk of fewer than 512 edges, sources without in-edges, dead ends.  Every level dense."""
    host, d = dense_design(pkg)
    w = _rand_w(host, 41)
    g = _graph(dev_cache, pkg, "dense_design", host, w, dense_frac=ALL_DENSE)
    srcs = [d["pool"][0], d["pool"][511], d["pool"][512], d["pool"][1099], d["A"], d["B"], d["C"], d["small"][1], d["dead"]]
    for s in srcs:
        _check_push(g, host, w, s, 1e-9, "dense_design", "all")
        out, _ = g.weighted_power_method(s, ALPHA, 40)
        assert np.max(np.abs(out - wr.power_iter(host, w, s, ALPHA, 40))) <= TOL, s
    # mass on every pool node at once: every edge of the three long rows carries a contribution
    g2 = _graph(dev_cache, pkg, "dense_design", host, w, dense_frac=ALL_DENSE)
    for s in (d["A"], d["pool"][3]):
        _check_push(g2, host, w, s, 1e-15, "dense_design tiny rmax", "all")


def test_dense_levels_with_fewer_chunks_than_waves(pkg, dev_cache, got):
    """GOT: 352 in-edges, one chunk."""
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w, dense_frac=ALL_DENSE)
    for s in _sources(got, extra=(5,)):
        _check_push(g, got, w, s, 1e-8, "got dense", "all")


def test_sparse_kernel_on_the_designed_sources(pkg, dev_cache):
    """Sources of out-degree 1, 63, 64, 65 and more than 2 048 (and 2, 3, 1 500): rows shorter and longer than a wave,
    than the staged window and than a tile of the push kernel.  No level dense."""
    host, by_deg = sparse_design(pkg)
    w = _rand_w(host, 42)
    g = _graph(dev_cache, pkg, "sparse_design", host, w, dense_frac=ALL_SPARSE)
    for dgr, s in by_deg.items():
        for rmax in (1e-3, 1e-6):
            _, _, st = _check_push(g, host, w, s, rmax, ("sparse_design", dgr), "none")
            assert st.edge_pushes >= dgr


# ---------------------------------------------------------------------------------------------- walks
def _walk_weights(host, by_deg):
    """Random weights; on the rows of degree 3, 65 and 1 500 one weight dominates so far that the small ones behind it
    vanish from the prefix (equal consecutive entries)."""
    w = _rand_w(host, 43)
    rp = host.out_rp.astype(np.int64)
    for dgr, pos in ((3, 1), (65, 10), (1500, 700)):
        u = by_deg[dgr]
        w[rp[u]:rp[u + 1]] = 1e-3
        w[rp[u] + pos] = 1e16
    return w


@pytest.mark.parametrize("no_zero_hop", [False, True])
def test_walks_are_bit_identical_to_the_reference(pkg, dev_cache, no_zero_hop):
    """Terminals and step counts of weighted_random_walks = weighted_ref.walks: starts on rows of degree 1, 2, 3, 63, 64,
    65, 1 500 and 2 500, dominated rows, dead-end starts and restarts, walk indices beyond 2^32, two streams."""
    host, by_deg = sparse_design(pkg)
    w = _walk_weights(host, by_deg)
    cum, W = wr.table(host, w)
    u = by_deg[1500]
    b = int(host.out_rp[u])
    assert cum[b + 701] == cum[b + 700] and cum[b + 699] < cum[b + 700]  # the small weights vanish behind the heavy one
    g = _graph(dev_cache, pkg, "sparse_design", host, w)
    deg = _deg(host)
    rng = np.random.default_rng(6)
    dead = np.flatnonzero(deg == 0)[:4]
    starts = np.concatenate([np.repeat(np.array(list(by_deg.values())), 300), rng.integers(0, host.n, 1500), dead])
    starts = starts.astype(np.int32)
    idx = rng.integers(0, 1 << 20, starts.size).astype(np.uint64)
    idx[::3] += np.uint64(1 << 32) * rng.integers(1, 200, idx[::3].size).astype(np.uint64)  # beyond 2^32
    for stream, seed in ((0, 99), (7, 0xABCDEF0123456789)):
        term, steps = g.weighted_random_walks(starts, idx, ALPHA, seed, stream, no_zero_hop)
        rt, rs = wr.walks(host, (cum, W), starts, idx, ALPHA, seed, stream, no_zero_hop)
        assert np.array_equal(term, rt) and np.array_equal(steps, rs), (stream, int((term != rt).sum()))
        assert (deg[starts[steps == 0]] == 0).all() or not no_zero_hop
    # the heavy relationship takes (nearly) every first hop of its row
    heavy = int(host.out_ci[b + 700])
    t1, s1 = g.weighted_random_walks(np.full(64, u, dtype=np.int32), np.arange(64, dtype=np.uint64), 0.999999, 5, 0, True)
    assert (s1 == 1).all() and (t1 == heavy).all()


def test_walks_with_unit_weights_on_power_of_two_rows_are_the_unweighted_walks(pkg, dev_cache):
    """Unit weights, out-degrees 1, 2, 4, ... : word * d is exact and the weighted pick is (word * d) >> 32, so the
    weighted walk is random_walks' walk."""
    rng = np.random.default_rng(7)
    n = 96
    degs = rng.choice([0, 1, 2, 4, 8, 16, 32], n)
    degs[:7] = [0, 1, 2, 4, 8, 16, 32]
    host = edges_to_host(pkg, n, [(u, int(v)) for u in range(n) for v in rng.integers(0, n, degs[u])])
    g = _graph(dev_cache, pkg, "pow2", host, np.ones(host.m))
    starts = np.tile(np.arange(n, dtype=np.int32), 30)
    idx = np.arange(starts.size, dtype=np.uint64) * np.uint64(7919)
    for nzh in (False, True):
        a = g.weighted_random_walks(starts, idx, 0.2, 11, 2, nzh)
        b = g.random_walks(starts, idx, 0.2, 11, 2, nzh)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------- FORA
# (graph, weight seed, source, walk seed): fixed after running weighted_ref.fora on them on the CPU - it draws the very
# walks the device draws - and keeping triples for which the reference itself meets the bound on every node (the bound
# holds with probability 1 - pfail only).  The last source of each graph is a dead end.
FORA_CASES = [("got", 21, 63, 3), ("got", 21, 35, 3), ("got", 21, 71, 3),
              ("rmat12", 22, 1803, 4), ("rmat12", 22, 2025, 4), ("rmat12", 22, 3, 4)]


@pytest.mark.parametrize("name,wseed,src,seed", FORA_CASES)
def test_fora_meets_its_bound_and_the_reference(pkg, dev_cache, got, rmat12, name, wseed, src, seed):
    eps = 0.5
    host = got if name == "got" else rmat12
    w = _rand_w(host, wseed)
    pi = _exact(name, host, w)[src]
    bound = eps * np.maximum(pi, 1.0 / host.n)
    ref, ref_walks, ref_steps = wr.fora(host, w, src, eps, ALPHA, seed)
    assert np.all(np.abs(ref - pi) <= bound), "the reference misses the bound: not a triple to test with"
    g = _graph(dev_cache, pkg, name, host, w)
    est, st = g.weighted_fora(src, eps, ALPHA, seed)
    worst = float(np.max(np.abs(est - pi) / bound))
    err = float(np.max(np.abs(est - ref)))
    print("%s src %d: worst |est - pi| / bound %.3f, |est - ref| %.2e, walks %d" % (name, src, worst, err, st.walks))
    assert np.all(np.abs(est - pi) <= bound), (name, src, worst)
    assert err <= TOL, (name, src, err)
    assert st.walks == ref_walks and st.walk_steps == ref_steps and st.rounds == 1
    rmax0, omega = wr.whole_params(host.n, host.m, ALPHA, eps)
    assert st.rmax_final == rmax0 and st.omega == omega
    if _deg(host)[src] == 0:
        assert st.walks == 0 and est[src] == 1.0 and np.count_nonzero(est) == 1
    # the estimate stays in HBM: the getters and the selection read it
    assert np.array_equal(g.reserve(), est)
    ids, vals, cnt = g.reserve_sparse(0.0, "id")
    assert np.array_equal(ids, np.flatnonzero(est > 0)) and np.array_equal(vals, est[est > 0]) and cnt == ids.size
    k = min(10, int(cnt))
    nsel, tid, tval, kth, _ = g.topk_select(k, cap=k)
    order = np.lexsort((np.arange(host.n), -est))[:k]
    assert nsel >= k and np.array_equal(tid, order) and np.array_equal(tval, est[order]) and kth == est[order[-1]]


def test_fora_at_a_given_threshold(pkg, dev_cache, got):
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w)
    est, st = g.weighted_fora(63, 0.5, ALPHA, 8, rmax=1e-3)
    ref, walks, _ = wr.fora(got, w, 63, 0.5, ALPHA, 8, rmax=1e-3)
    assert st.rmax_final == 1e-3 and st.walks == walks and np.max(np.abs(est - ref)) <= TOL


# ---------------------------------------------------------------------------------------------- lifecycle
def test_weighted_calls_need_weights(pkg, rmat12):
    with pkg.Graph(rmat12, device=0) as g:
        assert g.weights_info() == (False, 0)
        calls = [lambda: g.weighted_power_method(0, ALPHA, 3), lambda: g.weighted_forward_push(0, ALPHA, 1e-4),
                 lambda: g.weighted_random_walks([0], [0], ALPHA, 1), lambda: g.weighted_fora(0, 0.5, ALPHA, 1)]
        for c in calls:
            with pytest.raises(pkg.PprhipError, match="no relationship weights") as ei:
                c()
            assert ei.value.code == pkg.ERR_STATE
        g.set_weights(np.ones(rmat12.m))
        for c in calls:
            c()
        g.set_weights(None)
        with pytest.raises(pkg.PprhipError) as ei:
            calls[1]()
        assert ei.value.code == pkg.ERR_STATE


def test_second_set_of_weights_rules_and_a_bad_one_changes_nothing(pkg, dev_cache, got):
    w1, w2 = _rand_w(got, 51), _rand_w(got, 52)
    s = _sources(got)[0]
    g = _graph(dev_cache, pkg, "got", got, w1)
    a1, _ = g.weighted_power_method(s, ALPHA, 50)
    g.set_weights(w2)
    a2, _ = g.weighted_power_method(s, ALPHA, 50)
    assert np.max(np.abs(a1 - wr.power_iter(got, w1, s, ALPHA, 50))) <= TOL
    assert np.max(np.abs(a2 - wr.power_iter(got, w2, s, ALPHA, 50))) <= TOL and np.max(np.abs(a1 - a2)) > 1e-6
    info = g.weights_info()
    for bad in (np.nan, np.inf, 0.0, -1.0):
        wb = w1.copy()
        wb[100] = bad
        with pytest.raises(pkg.PprhipError, match="edge 100") as ei:
            g.set_weights(wb)
        assert ei.value.code == pkg.ERR_INVALID
    wb = w1.copy()
    b, e = int(got.out_rp[s]), int(got.out_rp[s + 1])
    wb[b:e] = 1e308
    with pytest.raises(pkg.PprhipError, match="node %d" % s):
        g.set_weights(wb)
    assert g.weights_info() == info
    a3, _ = g.weighted_power_method(s, ALPHA, 50)
    assert np.array_equal(a3, a2) or np.max(np.abs(a3 - a2)) <= TOL  # the second set is still in force


def test_in_row_weights_follow_a_caller_ordered_in_adjacency(pkg, got):
    """The lifted in-row keeps the order of the caller's in-adjacency: with the in-rows reversed the weights must still
    find their sources (dense levels read the in-row copy, sparse levels the out-row weights)."""
    class Host:
        pass
    h = Host()
    h.n, h.m, h.out_rp, h.out_ci, h.in_rp = got.n, got.m, got.out_rp, got.out_ci, got.in_rp
    h.in_ci = got.in_ci.copy()
    for v in range(got.n):
        b, e = int(got.in_rp[v]), int(got.in_rp[v + 1])
        h.in_ci[b:e] = got.in_ci[b:e][::-1]
    w = _rand_w(got, 21)
    with pkg.Graph(h, device=0) as g:
        g.set_weights(w)
        for frac in (ALL_SPARSE, ALL_DENSE):
            t = pkg.tuning_default()
            t.dense_frac = frac
            g.set_tuning(t)
            for s in _sources(got):
                _check_push(g, got, w, s, 1e-7, "reversed in-rows")


def test_drop_and_release_give_the_bytes_back(pkg, rmat15, rmat12):
    """24 m + 8 n bytes come with set_weights and go with the drop, with the release and with the handle."""
    w = _rand_w(rmat15, 61)
    expect = 24 * rmat15.m + 8 * rmat15.n
    with pkg.Graph(rmat12, device=0) as probe:  # a small handle that stays: pprhip_device_memory needs one
        with pkg.Graph(rmat15, device=0) as g:
            g.set_weights(w)  # first round: the allocator's own pools
            g.set_weights(None)
            free0, _ = probe.device_memory()
            g.set_weights(w)
            present, nbytes = g.weights_info()
            assert present and expect <= nbytes <= expect + 8 * 1024
            free1, _ = probe.device_memory()
            g.set_weights(w)  # a second call replaces the first: no second copy stays
            free1b, _ = probe.device_memory()
            g.set_weights(None)
            free2, _ = probe.device_memory()
            assert g.weights_info() == (False, 0)
            g.set_weights(w)
            g.release(pkg.Graph.RELEASE_WEIGHTS)
            free3, _ = probe.device_memory()
            assert g.weights_info() == (False, 0)
            g.set_weights(w)
        free4, _ = probe.device_memory()
    slack = 8 << 20
    print("weights: %d bytes; device memory taken %d, after drop %+d, after release %+d" %
          (nbytes, free0 - free1, free0 - free2, free0 - free3))
    assert free0 - free1 >= nbytes - slack and abs(free1b - free1) <= slack
    assert abs(free0 - free2) <= slack and abs(free0 - free3) <= slack
    assert free4 >= free0  # the handle's end frees them with everything else


def test_unweighted_calls_ignore_the_weights(pkg, rmat12):
    """forward_push, fora_single_source and power_method give the same results before set_weights, while weights are
    present, and after the drop."""
    s = int(np.argmax(_deg(rmat12)))

    def run(g):
        p, r, _, _ = g.forward_push(s, ALPHA, 1e-6)
        f, _ = g.fora_single_source(s, 0.5, ALPHA, seed=3, n_rounds=1)
        q, _ = g.power_method(s, ALPHA, 60)
        return p, r, f, q

    with pkg.Graph(rmat12, device=0) as g:
        before = run(g)
        g.set_weights(_rand_w(rmat12, 22))
        g.weighted_forward_push(s, ALPHA, 1e-6)
        during = run(g)
        g.set_weights(None)
        after = run(g)
    for a, b, c in zip(before, during, after):
        assert np.max(np.abs(a - b)) <= TOL and np.max(np.abs(a - c)) <= TOL
