"""The oracle twin at teleport probabilities other than 0.15, held to mathematics that does not go through it.

Every expected value elsewhere in the suite is computed at alpha = 0.15, so a (1 - alpha) dropped or a constant 0.85 in
the twin would pass there.  Here, at six values of alpha from 0.01 to 0.99:
- the push invariant pi(s, .) = reserve + sum_v r(v) pi(v, .) for both schedules, with pi from a dense solve of
  alpha (I - (1 - alpha) P_s)^-1 (GOT, the toy graphs, R-MAT 12);
- the two-node, cycle and star closed forms, and the power method's exact partial sum and its (1 - alpha)^iters bound;
- the seed-set invariant p^T Pi_p = reserve + r^T Pi_p on sets with dead-end seeds (the 1 - (1 - alpha) D closed form)
  and the seed plan's closed form;
- the walk semantics: the stop test at alpha = 0.99 with and without the forced first hop, long walks and dead-end
  restarts at 0.01.
The GPU half, engine against twin at these values, is tests/test_gpu_alpha.py."""
import numpy as np
import pytest

from conftest import to_oracle
from test_oracle_seeds import kinds, seed_sets
from test_seeds import exact_invariant_err, seed_p

ALPHAS = [0.01, 0.05, 0.2, 0.5, 0.9, 0.99]


def walk_matrix(host, s):
    """P_s: the random-walk matrix whose dead-end rows point to the query source s (the reference's dynamics)."""
    n = host.n
    P = np.zeros((n, n))
    for v in range(n):
        nb = np.asarray(host.out_ci[host.out_rp[v]:host.out_rp[v + 1]])
        if nb.size == 0:
            P[v, s] = 1.0
        else:
            np.add.at(P[v], nb, 1.0 / nb.size)
    return P


def left_pi(host, s, alpha, X):
    """Rows of X times Pi_s = alpha (I - (1 - alpha) P_s)^-1, by one dense LU solve (independent of every oracle
    routine)."""
    P = walk_matrix(host, s)
    A_t = (np.eye(host.n) - (1 - alpha) * P).T
    return alpha * np.linalg.solve(A_t, np.atleast_2d(X).T).T


def rmaxes(alpha):
    """Thresholds that leave several levels at each alpha: the residue falls by about (1 - alpha) per level."""
    return (1e-3, 1e-6, 1e-10) if alpha >= 0.2 else (1e-4, 1e-8)


def push_cases(got, toy_graphs, rmat12):
    od = np.diff(got.out_rp)
    yield "got", got, [s for s in (0, 17, 42, 99) if od[s] > 0] + [int(np.argmax(od == 0))]
    for name, host in sorted(toy_graphs.items()):
        yield name, host, list(range(host.n))
    od = np.diff(rmat12.out_rp)
    yield "rmat12", rmat12, [int(np.argmax(od)), int(np.nonzero(od == 1)[0][0])]


# ------------------------------------------------------------------ push invariant against the dense solve
@pytest.mark.parametrize("alpha", ALPHAS)
def test_push_invariant_against_dense_solve(orc, got, toy_graphs, rmat12, alpha):
    levels = 0
    for name, host, srcs in push_cases(got, toy_graphs, rmat12):
        og = to_oracle(orc, host)
        od = np.diff(np.asarray(host.out_rp, dtype=np.int64))
        for s in srcs:
            if od[s] == 0:  # dead-end source: all mass stays at s (Forward_Push.java:72-76)
                for sch in (orc.FIFO, orc.SYNC):
                    p, r, rsum, st = og.forward_push(s, alpha, 1e-6, sch)
                    assert p[s] == 1.0 and p.sum() == 1.0 and rsum == 0.0
                continue
            for rmax in rmaxes(alpha):
                runs = [og.forward_push(s, alpha, rmax, sch) for sch in (orc.FIFO, orc.SYNC)]
                e_s = np.zeros(host.n)
                e_s[s] = 1.0
                sol = left_pi(host, s, alpha, np.vstack([e_s] + [r for _, r, _, _ in runs]))
                for i, (p, r, rsum, st) in enumerate(runs):
                    what = (name, s, alpha, rmax, i)
                    assert np.max(np.abs(p + sol[1 + i] - sol[0])) < 1e-13, what
                    assert np.all((od == 0) & (r == 0) | (od > 0) & (r / np.maximum(od, 1) < rmax)), what
                    assert p.sum() + r.sum() == pytest.approx(1.0, abs=1e-12), what
                    assert np.all(p >= 0) and np.all(r >= 0), what
                levels += runs[1][3].levels
    assert levels > 0


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("alpha", ALPHAS)
def test_two_node_cycle_and_star_closed_forms(orc, toy_graphs, alpha):
    a = alpha
    og = to_oracle(orc, toy_graphs["two_node"])  # Dissertation p.13-14: t is a dead end that returns to s
    ps, pt = a / (1 - (1 - a) ** 2), a * (1 - a) / (1 - (1 - a) ** 2)
    for sch in (orc.FIFO, orc.SYNC):
        p, r, rsum, st = og.forward_push(0, a, 1e-14, sch)
        assert abs(p[0] - ps) <= 1e-12 and abs(p[1] - pt) <= 1e-12, (a, sch)
        assert p.sum() + r.sum() == pytest.approx(1.0, abs=1e-14)
    og = to_oracle(orc, toy_graphs["cycle5"])
    exact = np.array([a * (1 - a) ** j / (1 - (1 - a) ** 5) for j in range(5)])
    for sch in (orc.FIFO, orc.SYNC):
        p, r, rsum, st = og.forward_push(0, a, 1e-14, sch)
        assert np.max(np.abs(p - exact)) < 1e-12, (a, sch)
        pb, rb, stb = og.backward_push(0, a, 1e-14, sch)  # pi(v, 0): v is 5 - v steps before 0
        assert np.max(np.abs(pb - exact[(5 - np.arange(5)) % 5])) < 1e-12, (a, sch)
    og = to_oracle(orc, toy_graphs["star_dead_leaves"])  # centre keeps a / (1 - (1 - a)^2), each leaf a fifth of the rest
    centre = a / (1 - (1 - a) ** 2)
    for sch in (orc.FIFO, orc.SYNC):
        p, r, rsum, st = og.forward_push(0, a, 1e-14, sch)
        assert abs(p[0] - centre) <= 1e-12 and np.allclose(p[1:], (1 - centre) / 5, rtol=0, atol=1e-12), (a, sch)


@pytest.mark.parametrize("alpha", ALPHAS)
def test_power_method_partial_sum(orc, got, rmat12, alpha):
    """Power_Method.java after `iters` sweeps holds alpha sum_{t < iters} (1 - alpha)^t e_s P^t: with x = e_s P^iters,
    reserve + (1 - alpha)^iters x Pi_s = Pi_s[s] exactly, and |reserve - Pi_s[s]| <= (1 - alpha)^iters."""
    for host, srcs in ((got, (17, 42)), (rmat12, (int(np.argmax(np.diff(rmat12.out_rp))),))):
        og = to_oracle(orc, host)
        for s in srcs:
            od = np.diff(np.asarray(host.out_rp, dtype=np.int64))
            src = np.repeat(np.arange(host.n), od)
            dst = np.asarray(host.out_ci, dtype=np.int64)
            inv = 1.0 / np.maximum(od, 1)
            iters_list = (1, 2, 7, 100)
            e_s = np.zeros(host.n)
            e_s[s] = 1.0
            x, tails, done = e_s.copy(), [], 0
            for iters in iters_list:
                for _ in range(iters - done):  # x P_s, sparse: dead-end mass returns to s
                    nx = np.bincount(dst, weights=(x * inv)[src], minlength=host.n)
                    nx[s] += x[od == 0].sum()
                    x = nx
                done = iters
                tails.append((1 - alpha) ** iters * x)
            sol = left_pi(host, s, alpha, np.vstack([e_s] + tails))
            for i, iters in enumerate(iters_list):
                pm = og.power_method(s, alpha, iters)
                assert np.max(np.abs(pm + sol[1 + i] - sol[0])) < 1e-13, (s, alpha, iters)
                assert np.max(np.abs(pm - sol[0])) <= (1 - alpha) ** iters + 1e-15
                assert pm.sum() == pytest.approx(1 - (1 - alpha) ** iters, abs=1e-13)


# ------------------------------------------------------------------ seed sets
def all_dead_set(host):
    _, dead, _ = kinds(host)
    return (dead[:5], np.linspace(1.0, 2.0, min(5, dead.size))) if dead.size else None


@pytest.mark.parametrize("alpha", ALPHAS)
def test_seed_push_exact_invariant(pkg_product, orc, got, toy_graphs, rmat12, alpha):
    """p^T Pi_p = reserve + r^T Pi_p after every seed-set push, on sets with dead-end seeds (the landing's closed form
    1 - (1 - alpha) D), with one live seed among thirty dead ends (D -> 1), and on a set of dead ends only (the reserve
    is p itself, nothing is pushed)."""
    dead_weight = 0.0
    for name, host in [("got", got)] + sorted(toy_graphs.items()) + [("rmat12", rmat12)]:
        og = to_oracle(orc, host)
        dout = np.diff(np.asarray(host.out_rp, dtype=np.int64))
        sets = seed_sets(host, 3)
        if name == "rmat12":
            sets = [x for x in sets if x[1] is not None][1:5:3]
        for s, w in sets:
            p_vec = seed_p(host.n, s, w)
            dead_weight = max(dead_weight, p_vec[dout == 0].sum())
            for rmax in rmaxes(alpha)[-2:] if name == "rmat12" else rmaxes(alpha):
                p, r, rsum, st = og.forward_push_seeds(s, alpha, rmax, weights=w)
                what = (name, alpha, rmax, s.size)
                assert np.all(r[dout == 0] == 0.0) and np.all(r[dout > 0] / dout[dout > 0] < rmax), what
                assert abs(r.sum() - rsum) <= 1e-12 and abs(p.sum() + rsum - 1.0) <= 1e-12, what
                assert exact_invariant_err(host, p_vec, p, r, alpha) <= 1e-12, what
        dead = all_dead_set(host)
        if dead is not None:
            s, w = dead
            p, r, rsum, st = og.forward_push_seeds(s, alpha, 1e-9, weights=w)
            assert np.max(np.abs(p - seed_p(host.n, s, w))) <= 1e-15 and not r.any() and st.levels == 0, name
    assert dead_weight > 0.5


@pytest.mark.parametrize("alpha", ALPHAS)
def test_seed_plan_closed_form(pkg_product, orc, got, toy_graphs, alpha):
    """The plan's landing weights: q_i = p_i / (1 - (1 - alpha) D) for the live seeds, e_j = alpha p_j / (...) for the
    dead ends, summing to 1."""
    checked = 0
    for name, host in [("got", got)] + sorted(toy_graphs.items()):
        og = to_oracle(orc, host)
        for s, w in seed_sets(host, 4):
            ids, p, lw, n_live = og.seed_plan(s, w, alpha)
            D = p[n_live:].sum()
            den = 1.0 - (1.0 - alpha) * D
            if n_live and D > 0:
                assert np.max(np.abs(lw[:n_live] - p[:n_live] / den)) <= 1e-15, (name, alpha)
                assert np.max(np.abs(lw[n_live:] - alpha * p[n_live:] / den)) <= 1e-15, (name, alpha)
                checked += 1
            assert abs(lw.sum() - 1.0) <= 1e-14 / den, (name, alpha)  # (1 / den rounds: up to 100 at alpha = 0.01)
    assert checked > 0


# ------------------------------------------------------------------ walks
def test_walk_semantics_alpha_099(orc, got):
    """Each decision stops with probability alpha: at 0.99 almost every walk ends at once; with the forced first hop
    (Monte_Carlo.java:111-112) every walk makes one step and then almost always stops on a neighbour of its start."""
    a = 0.99
    og = to_oracle(orc, got)
    src = 17
    nbrs = set(got.out_ci[got.out_rp[src]:got.out_rp[src + 1]].tolist())
    N = 20000
    w0 = [og.random_walk(src, a, 5, 0, i, False) for i in range(N)]
    w1 = [og.random_walk(src, a, 5, 0, i, True) for i in range(N)]
    s0 = np.array([x[1] for x in w0])
    s1 = np.array([x[1] for x in w1])
    assert np.mean(s0 == 0) == pytest.approx(a, abs=0.003)             # P(stop at once) = alpha
    assert all(t == src for t, st in w0 if st == 0)
    assert s1.min() == 1 and np.mean(s1 == 1) == pytest.approx(a, abs=0.003)
    assert all(t in nbrs for t, st in w1 if st == 1)
    assert np.mean(s1) == pytest.approx(1 + (1 - a) / a, abs=0.003)
    assert s1.max() >= 2                                               # the second decision does run


def test_walk_semantics_alpha_001(orc, toy_graphs, got):
    """At 0.01 walks are long (mean (1 - alpha) / alpha = 99 steps) and meet dead ends: on the line 0 -> 1 -> ... -> 7
    a walk from 0 restarts at 0 from the dead end 7 (one step, Monte_Carlo.java:87-90), so its terminal is steps mod 8."""
    a = 0.01
    og = to_oracle(orc, toy_graphs["line"])
    N = 20000
    walks = [og.random_walk(0, a, 3, 1, i, False) for i in range(N)]
    steps = np.array([st for _, st in walks])
    assert all(t == st % 8 for t, st in walks)
    assert steps.max() > 500 and np.mean(steps >= 8) > 0.9              # most walks pass the dead end at least once
    assert np.mean(steps) == pytest.approx((1 - a) / a, rel=0.03)
    og = to_oracle(orc, got)
    steps = np.array([og.random_walk(17, a, 5, 0, i, True)[1] for i in range(N)])
    assert steps.min() >= 1 and np.mean(steps) == pytest.approx(1 + (1 - a) / a, rel=0.03)
