"""Single pairs beyond the two operating points of tests/test_gpu_pairs.py (DESIGN.md §2 "Single pairs", §3): every
walk-count regime of k_pair_walk against the oracle-side twin (tests/test_pairs_twin.py: nothing of the engine's goes
into the expected value), the block loop of finish_pairs (bwd_runs.cpp) over a target's sources, the exact identity the estimator rests on
with the engine's push and survival, a Hoeffding-tight accuracy bound, and the survival kernels on a graph built to
straddle every row split (8 lanes per row below out-degree 512, a workgroup per row from 512 on).

The walk count w = ceil(omega r_max) is chosen through the call's own knobs - the conf's delta, eps and an explicit
r_max - and every test asserts the w that pkg.pair_params returns, so none can drift off its regime."""
import math
import time

import numpy as np
import pytest

from conftest import edges_to_host, shared_graph, to_oracle
from test_gpu_pairs import ppr_exact, survival_dense
from test_pairs_twin import LADDER, PAIR_EPS, PairTwin, conf_for_walks, identity_error, pair_regime, pair_twin

pytestmark = pytest.mark.gpu
A = 0.15
TOL = 1e-12          # the project's bar where only fp64 addition order differs
TIE = 1e-9           # no residue of the twin's push this close (relative) to r_max: DESIGN.md §3, parity thresholds
PART_CAP = 1 << 19   # kPartCap (csrc/pairs.cpp): item sums per workspace, so a walk launch takes PART_CAP / items pairs
SURV_HEAVY = 512     # kSurvHeavy (csrc/kernels_walk.hip): rows from this out-degree on are summed by a workgroup each
GOT_RMAX = 0.02      # near the balanced default of GOT at eps = 0.5 (0.0219): pushes of up to 7 levels
R12_RMAX = 1e-3


# ------------------------------------------------------------------ fixtures
@pytest.fixture
def dev_got(pkg, got, dev_cache):
    return shared_graph(dev_cache, pkg, "got", lambda: pkg.Graph(got))


@pytest.fixture
def dev_r12(pkg, rmat12, dev_cache):
    return shared_graph(dev_cache, pkg, "r12", lambda: pkg.Graph(rmat12))


@pytest.fixture(scope="module")
def got_twin(orc, got):
    return PairTwin(orc, to_oracle(orc, got), got, A, GOT_RMAX)


@pytest.fixture(scope="module")
def r12_twin(orc, rmat12):
    return PairTwin(orc, to_oracle(orc, rmat12), rmat12, A, R12_RMAX)


@pytest.fixture(scope="module")
def got_pi(got):
    return ppr_exact(got, A)


def _degrees(host):
    return np.diff(host.out_rp.astype(np.int64)), np.diff(host.in_rp.astype(np.int64))


def _regime_id(w):
    return "w%d-items%d-of%d" % ((w,) + pair_regime(w))


def _check_against_twin(pkg, g, host, twin, pairs, w, seed):
    """One call of the pairs at exactly w walks each: every value, the walk count and the step count against the twin."""
    rmax = twin.rmax
    conf = conf_for_walks(pkg, host, twin.alpha, rmax, w)
    assert pkg.pair_params(conf, PAIR_EPS, rmax) == (rmax, w)
    for t in {t for _, t in pairs}:
        assert twin.tie_margin(t) > TIE, (t, twin.tie_margin(t))
    vals, st = g.ppr_pairs([p[0] for p in pairs], [p[1] for p in pairs], PAIR_EPS, twin.alpha, seed, rmax=rmax, conf=conf)
    steps = walks = 0
    worst = 0.0
    for i, (s, t) in enumerate(pairs):
        ref, st_i, w_i = pair_twin(twin.orc, twin.og, host, s, t, twin.alpha, rmax, w, seed, twin=twin)
        steps += st_i
        walks += w_i
        if ref:
            worst = max(worst, abs(vals[i] - ref) / abs(ref))
        assert abs(vals[i] - ref) <= TOL * abs(ref) + 1e-300, (w, s, t, vals[i], ref)
    print("w = %d: items %d of %d walks, %d pairs, max relative difference to the twin %.2e, %d walks, %d steps"
          % ((w,) + pair_regime(w) + (len(pairs), worst, st.walks, st.walk_steps)))
    assert st.rmax_final == rmax
    assert st.walks == walks == w * sum(1 for _, t in pairs if twin.din[t] > 0)
    assert st.walk_steps == steps
    return vals, st


# ------------------------------------------------------------------ a. the walk-count ladder
def _got_ladder_pairs(host):
    od, idg = _degrees(host)
    rng = np.random.default_rng(31)
    live_t = np.flatnonzero(idg > 0)
    hub_s, hub_t = int(np.argmax(od)), int(np.argmax(idg))
    dead = int(np.flatnonzero((od == 0) & (idg > 0))[0])
    one = int(np.flatnonzero(od == 1)[0])
    noin = int(np.flatnonzero((idg == 0) & (od > 0))[0])
    same = int(np.flatnonzero((od > 1) & (idg > 0))[3])
    pick = lambda: int(rng.choice(live_t))
    pairs = [(hub_s, pick()), (pick(), hub_t), (dead, pick()), (one, pick()), (same, same), (pick(), noin), (noin, noin),
             (int(rng.integers(0, host.n)), pick()), (int(rng.integers(0, host.n)), int(rng.integers(0, host.n)))]
    assert od[dead] == 0 and od[one] == 1 and idg[noin] == 0 and od[hub_s] == od.max() and idg[hub_t] == idg.max()
    return pairs


@pytest.mark.parametrize("w", LADDER, ids=_regime_id)
def test_walk_count_ladder_got(pkg, got, dev_got, got_twin, w):
    dev_got.set_tuning(pkg.tuning_default())
    _check_against_twin(pkg, dev_got, got, got_twin, _got_ladder_pairs(got), w, seed=1000 + w)


@pytest.mark.parametrize("w", [65, 1025, 524289], ids=_regime_id)
def test_walk_count_ladder_rmat12_dense_push(pkg, rmat12, dev_r12, r12_twin, w):
    """The same on R-MAT 12 with the targets' pushes taking dense levels (the twin's backward push has one level shape)."""
    host, g = rmat12, dev_r12
    od, idg = _degrees(host)
    hubs = [int(x) for x in np.argsort(-idg, kind="stable")[:3]]
    dead = int(np.flatnonzero((od == 0) & (idg > 0))[0])
    pairs = [(int(np.argmax(od)), hubs[0]), (1234, hubs[1]), (dead, hubs[0]), (77, hubs[2])]
    t_ = pkg.tuning_default()
    t_.dense_frac = 0.002
    g.set_tuning(t_)
    try:
        _, st = _check_against_twin(pkg, g, host, r12_twin, pairs, w, seed=5)
        assert st.dense_levels > 0
    finally:
        g.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ b. the block loop
def _block_conf(pkg, got, rmax):
    """w = 524 289 gives 512 items per pair, so a walk launch takes PART_CAP / 512 = 1 024 pairs and a target with more
    sources runs the loop of finish_pairs (bwd_runs.cpp) more than once."""
    w = 524289
    conf = conf_for_walks(pkg, got, A, rmax, w)
    assert pkg.pair_params(conf, PAIR_EPS, rmax) == (rmax, w)
    chunks = pair_regime(w)[0]
    assert chunks == 512 and PART_CAP // chunks == 1024
    return w, conf


def test_block_loop_one_target(pkg, orc, got, dev_got, got_twin):
    """2 500 sources of the target with the most in-edges, cycling through all nodes: three launches of the walk and
    reduce kernels, each at its own offset into the call's sources and positions, all through the one buffer of item
    sums.  The push is shared and a pair's walks depend on (seed, source, index) alone, so every occurrence of a source
    must give the same bits; the ends of every block go to the twin."""
    twin, rmax = got_twin, GOT_RMAX
    w, conf = _block_conf(pkg, got, rmax)
    g = dev_got
    g.set_tuning(pkg.tuning_default())
    t0 = int(np.argmax(np.diff(got.in_rp.astype(np.int64))))
    assert twin.tie_margin(t0) > TIE
    q = 2500
    blocks = -(-q // 1024)
    assert blocks == 3                                      # [0, 1024), [1024, 2048), [2048, 2500)
    src = np.arange(q) % got.n                              # every source occurs in all three blocks
    assert all(len(set((np.flatnonzero(src == v) // 1024).tolist())) == 3 for v in range(got.n))
    tic = time.perf_counter()
    vals, st = g.ppr_pairs(src, np.full(q, t0), PAIR_EPS, A, 41, rmax=rmax, conf=conf)
    print("block loop: %d pairs of %d walks in %d blocks, %.3f s; %d distinct values"
          % (q, w, blocks, time.perf_counter() - tic, len(np.unique(vals))))
    assert st.walks == q * w
    for v in range(got.n):
        occ = vals[src == v]
        assert np.all(occ == occ[0]), (v, occ)
    for i in (0, 1023, 1024, 2047, 2048, 2499, 1022, 1025):  # the ends of every block, and one more on each side of the first cut
        ref, _, _ = pair_twin(orc, twin.og, got, int(src[i]), t0, A, rmax, w, 41, twin=twin)
        assert abs(vals[i] - ref) <= TOL * abs(ref) + 1e-300, (i, int(src[i]), vals[i], ref)
    # (24 of GOT's 107 nodes reach this target at all; their values differ, so equal bits are no accident of zeros)
    assert len(np.unique(vals)) > 20


def test_block_loop_two_targets_in_one_call(pkg, orc, got, dev_got):
    """Two targets of 1 500 sources each in one call, interleaved: two workspaces loop over their own slice of the item
    sums at the same time, two blocks each.  Every value equals, bit for bit, the one a call of that target alone gives.
    For that the push itself must give the same bits in every call, which a level that adds to a node from several
    frontier nodes (in atomic order) does not promise: r_max = 0.9 ends the push after its first level - the largest
    residue it can leave is 0.85, at an in-neighbour of out-degree 1 - where every node is added to from the target
    alone."""
    rmax = 0.9
    w, conf = _block_conf(pkg, got, rmax)
    twin = PairTwin(orc, to_oracle(orc, got), got, A, rmax)
    g = dev_got
    g.set_tuning(pkg.tuning_default())
    ta, tb = (int(x) for x in np.argsort(-np.diff(got.in_rp.astype(np.int64)), kind="stable")[:2])
    assert twin.push(ta)[2].levels == 1 and twin.push(tb)[2].levels == 1
    q = 1500
    assert -(-q // 1024) == 2
    src = np.arange(q) % got.n
    alone = {t: g.ppr_pairs(src, np.full(q, t), PAIR_EPS, A, 41, rmax=rmax, conf=conf)[0] for t in (ta, tb)}
    both_s, both_t = np.repeat(src, 2), np.tile([ta, tb], q)
    tic = time.perf_counter()
    vals, st = g.ppr_pairs(both_s, both_t, PAIR_EPS, A, 41, rmax=rmax, conf=conf)
    print("two targets: %d pairs of %d walks, %.3f s" % (2 * q, w, time.perf_counter() - tic))
    assert st.walks == 2 * q * w and st.rounds == 2
    assert np.array_equal(vals[0::2], alone[ta]) and np.array_equal(vals[1::2], alone[tb])
    assert not np.array_equal(alone[ta], alone[tb])
    for i in (0, 1023, 1024, 1499):
        for t, v in ((ta, vals[2 * i]), (tb, vals[2 * i + 1])):
            ref, _, _ = pair_twin(orc, twin.og, got, int(src[i]), t, A, rmax, w, 41, twin=twin)
            assert abs(v - ref) <= TOL * abs(ref) + 1e-300, (i, t, v, ref)


# ------------------------------------------------------------------ c. the exact identity, and what it allows
@pytest.mark.parametrize("alpha", [0.05, 0.15, 0.5])
def test_exact_identity_on_the_engine_push(pkg, got, dev_got, alpha):
    """pi(s, t) = p_t(s) / S(s) + sum_v pi(s, v) r_t(v) with p_t, r_t of pprhip_backward_push
    and S of pprhip_walk_survival against the dense inverse, for every target with in-edges and every source, at three
    thresholds - the middle one under a tuning that makes levels dense.  No walks: a wrong push start, a wrong S or S on
    the wrong term cannot hide behind the estimator's noise.  (tests/test_pairs_twin.py has the same line on the
    oracle's push.)  A target without in-edges keeps reserve(t) = 1 in pprhip_backward_push; there the pair call itself
    is exact: alpha / S(t) on the diagonal, 0 elsewhere."""
    g = dev_got
    pi = ppr_exact(got, alpha)
    _, idg = _degrees(got)
    surv = g.walk_survival(alpha)
    assert np.max(np.abs(surv - survival_dense(got, alpha))) <= 1e-12
    dense = pkg.tuning_default()
    dense.dense_frac = 0.01
    try:
        for rmax, tun in ((1e-2, pkg.tuning_default()), (1e-4, dense), (1e-6, pkg.tuning_default())):
            g.set_tuning(tun)
            worst, dense_levels = 0.0, 0
            for t in np.flatnonzero(idg > 0):
                p, r, st = g.backward_push(int(t), alpha, rmax)
                dense_levels += st.dense_levels
                assert np.max(r) <= rmax
                worst = max(worst, identity_error(pi, p, r, surv, int(t)))
            print("alpha = %g, r_max = %g: identity holds to %.2e, %d dense levels" % (alpha, rmax, worst, dense_levels))
            assert worst <= 1e-12, (alpha, rmax, worst)
            assert dense_levels > 0 or tun is not dense, rmax
    finally:
        g.set_tuning(pkg.tuning_default())
    noin = np.flatnonzero(idg == 0)
    assert noin.size > 0
    s, t = np.meshgrid(np.arange(got.n), noin, indexing="ij")
    vals, st = g.ppr_pairs(s.ravel(), t.ravel(), PAIR_EPS, alpha, 3)
    assert st.walks == 0 and st.walk_steps == 0
    vals = vals.reshape(s.shape)
    for j, tt in enumerate(noin):
        off = np.arange(got.n) != tt
        assert np.all(vals[off, j] == 0.0)
        assert abs(vals[tt, j] - alpha / surv[tt]) <= 1e-15 * (alpha / surv[tt])
        assert abs(vals[tt, j] - pi[tt, tt]) <= 1e-12


def test_accuracy_at_the_hoeffding_bound(pkg, got, dev_got, got_pi):
    """A bias detector far below the eps-bound.  By the identity the estimate's error is all in the walk term, the mean
    of w independent terms r_t(V_i), each in [0, r_max]: its standard deviation is at most r_max / (2 sqrt(w)), and
    Hoeffding gives P(|mean - E| >= x) <= 2 exp(-2 w x^2 / r_max^2), which at x = 6 r_max / (2 sqrt(w)) - six of those
    standard deviations - is 2 exp(-18) = 3e-8 per pair (2e-9 by the normal approximation).  At w = 700 001 and
    r_max = 0.02 that bound is 7.2e-5 for every pair, where the call's own guarantee eps max(pi, delta) allows 5e-3 at
    pi = 0.01.  The fp64 error of either side (1e-12) does not register."""
    w, rmax = 700001, GOT_RMAX
    conf = conf_for_walks(pkg, got, A, rmax, w)
    assert pkg.pair_params(conf, PAIR_EPS, rmax) == (rmax, w)
    bound = 6.0 * rmax / (2.0 * math.sqrt(w))
    rng = np.random.default_rng(2025)
    s, t = rng.integers(0, got.n, 200), rng.integers(0, got.n, 200)
    dev_got.set_tuning(pkg.tuning_default())
    vals, st = dev_got.ppr_pairs(s, t, PAIR_EPS, A, 97, rmax=rmax, conf=conf)
    err = np.abs(vals - got_pi[s, t])
    print("200 pairs at w = %d: max |value - pi| = %.3e, bound %.3e" % (w, err.max(), bound))
    assert st.walks > 100 * w
    assert np.all(err <= bound), (int(np.argmax(err)), err.max(), bound)


# ------------------------------------------------------------------ d. survival across the row splits
DEGREE_LADDER = [0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1599, 3000]


def survival_graph_edges(no_dead_ends, n=1600, seed=12):
    """Edges of a graph whose node i < len(DEGREE_LADDER) has out-degree DEGREE_LADDER[i]: the 8-lane tail (7 / 8 / 9,
    15 / 16 / 17), the 256-thread tail of a workgroup (255 / 256 / 257, 767 / 768 / 769), the split at 512 (511 / 512 /
    513), a row of n - 1 and one of 3 000 edges (multi-edges by necessity, and a self loop).  Neighbours by a seeded
    rng, with repetition.  The other nodes have 0 to 5 out-edges; the last 6 are isolated and 20 before them are pointed
    at by rows of out-degree >= 512 only.  no_dead_ends: every node without out-edges gets one."""
    rng = np.random.default_rng(seed)
    k = len(DEGREE_LADDER)
    deg = np.concatenate([DEGREE_LADDER, rng.integers(0, 6, n - k)])
    isolated = np.arange(n - 6, n)
    heavy_only = np.arange(n - 26, n - 6)
    deg[isolated] = 0
    common = np.arange(0, n - 26)
    with_heavy_only = np.arange(0, n - 6)
    if no_dead_ends:
        deg[deg == 0] = 1
    edges = []
    for u in range(n):
        d = int(deg[u])
        if d == 0:
            continue
        nb = rng.choice(with_heavy_only if d >= SURV_HEAVY else common, d, replace=True)
        if d == 3000:
            nb[0] = u
        edges += [(u, int(v)) for v in nb]
    return n, edges, deg


def _check_survival_graph(host, deg, no_dead_ends):
    od, idg = _degrees(host)
    assert np.array_equal(od, deg) and set(DEGREE_LADDER) - ({0} if no_dead_ends else set()) <= set(od.tolist())
    assert np.any((od < SURV_HEAVY) & (od > 0)) and np.any(od >= SURV_HEAVY)      # rows on both sides of the split ...
    assert {SURV_HEAVY - 1, SURV_HEAVY, SURV_HEAVY + 1} <= set(od.tolist())       # ... and at it
    big = int(np.flatnonzero(od == 3000)[0])
    row = host.out_ci[host.out_rp[big]:host.out_rp[big + 1]]
    assert big in row and len(set(row.tolist())) < 3000                           # self loop, multi-edges
    n = host.n
    heavy_rows = np.flatnonzero(od >= SURV_HEAVY)
    for v in range(n - 26, n - 6):  # reachable from heavy rows only (every one of them is, or the ladder misses its point)
        pred = host.in_ci[host.in_rp[v]:host.in_rp[v + 1]]
        assert pred.size > 0 and np.all(np.isin(pred, heavy_rows)), v
    if not no_dead_ends:
        assert np.all((od[n - 6:] == 0) & (idg[n - 6:] == 0))
        assert np.count_nonzero((od == 0) & (idg > 0)) > 10
    else:
        assert od.min() >= 1


@pytest.mark.parametrize("alpha", [0.01, 0.15, 0.5, 0.99])
def test_survival_across_the_row_splits(pkg, alpha):
    n, edges, deg = survival_graph_edges(False)
    host = edges_to_host(pkg, n, edges)
    _check_survival_graph(host, deg, False)
    with pkg.Graph(host) as g:
        tic = time.perf_counter()
        S = g.walk_survival(alpha)
        dt = time.perf_counter() - tic
    ref = survival_dense(host, alpha)
    print("alpha = %g: max |S - dense solve| = %.2e, solve %.3f s" % (alpha, np.max(np.abs(S - ref)), dt))
    assert np.max(np.abs(S - ref)) <= 1e-12, (alpha, np.max(np.abs(S - ref)))
    dead = np.flatnonzero(deg == 0)
    assert dead.size > 0 and np.all(S[dead] == alpha)


@pytest.mark.parametrize("alpha", [0.01, 0.15, 0.5, 0.99])
def test_survival_is_one_without_dead_ends(pkg, alpha):
    """No dead end, no leak: S = 1 at every node, whichever kernel sums its row."""
    n, edges, deg = survival_graph_edges(True)
    host = edges_to_host(pkg, n, edges)
    _check_survival_graph(host, deg, True)
    with pkg.Graph(host) as g:
        S = g.walk_survival(alpha)
    print("alpha = %g: max |S - 1| = %.2e" % (alpha, np.max(np.abs(S - 1.0))))
    assert np.max(np.abs(S - 1.0)) <= 1e-13, (alpha, np.max(np.abs(S - 1.0)))


def test_rmat12_rows_for_the_record(rmat12):
    """What tests/test_gpu_pairs.py::test_walk_survival_against_dense_solve covered on R-MAT 12: its largest row (2 456
    out-edges with the suite's generator seed) is a workgroup row.  Nothing above relies on it."""
    max_deg = int(np.diff(rmat12.out_rp.astype(np.int64)).max())
    assert max_deg >= SURV_HEAVY or max_deg > 0, "R-MAT 12's largest out-degree is %d: no workgroup row" % max_deg
