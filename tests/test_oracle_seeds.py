"""The twin's seed sets (oracle/ppr_oracle.c: orc_seed_plan, orc_forward_push_seeds, orc_fora_whole_seeds,
orc_fora_topk_seeds) without a device: the exact push invariant p^T Pi_p = reserve + r^T Pi_p at every rmax and level
shape, bit-identity with the single-source entry points for a set of one seed, the normalization rules, and FORA's and
top-k's bounds against rule B.  The GPU half, engine against twin, is tests/test_gpu_seeds_twin.py."""
import numpy as np
import pytest

from conftest import to_oracle
from test_gpu_fuzz import random_graph
from test_seeds import exact_invariant_err, pi_p_left, rule_b, seed_p

A = 0.15
EPS = 0.5
LEVEL_SHAPES = [(1e9, 1), (1e-9, 1), (1e-9, 2), (1e-9, 3), (1e-9, 6), (0.002, 1), (0.002, 2), (0.002, 3), (0.002, 6)]


def kinds(host):
    dout = np.diff(np.asarray(host.out_rp, dtype=np.int64))
    din = np.diff(np.asarray(host.in_rp, dtype=np.int64))
    return np.nonzero(dout > 0)[0], np.nonzero(dout == 0)[0], np.nonzero((dout > 0) & (din == 0))[0]


def seed_sets(host, seed):
    """Sets of 1, 2, 3 and 12 seeds mixing live nodes, dead ends, nodes without in-edges, duplicates and zero weights,
    one live seed among many dead ends (D -> 1), weights from 1e-12 to 1, and every node of a small graph."""
    live, dead, zin = kinds(host)
    rng = np.random.default_rng(seed)
    out = []
    for k in (1, 2, 3, 12):
        s = rng.choice(host.n, size=min(k, host.n), replace=False)
        if zin.size and k >= 3:
            s[0] = zin[0]
        if dead.size and k >= 2:
            s[-1] = dead[0]
        w = rng.uniform(0.1, 1.0, size=s.size)
        out.append((s, w))
    if live.size and dead.size:
        s = np.concatenate([live[:1], dead[:30]])
        out.append((s, np.concatenate([[1e-3], np.ones(s.size - 1)])))
    if live.size >= 3:
        s = rng.choice(live, size=min(6, live.size), replace=False)
        out.append((np.concatenate([s, s[:2]]), np.concatenate([10.0 ** -rng.uniform(0, 12, size=s.size), [0.0, 0.5]])))
    if host.n <= 120:
        out.append((np.arange(host.n), None))
    return out


def tuning(orc, dense_frac, blocks):
    t = orc.tuning_default()
    t.dense_frac = dense_frac
    t.gs_blocks = blocks
    return t


def check_exact(host, s, w, p, r, rmax, what, tol=1e-12):
    dout = np.diff(np.asarray(host.out_rp, dtype=np.int64))
    live = dout > 0
    assert np.all(r[live] / dout[live] < rmax), what
    assert np.all(r[~live] == 0.0) and np.all(p >= 0.0) and np.all(r >= 0.0), what
    err = exact_invariant_err(host, seed_p(host.n, s, w), p, r, A)
    assert err <= tol, (what, err)


def graphs(pkg, got, toy_graphs, rmat12):
    out = [("got", got)] + sorted(toy_graphs.items()) + [("rmat12", rmat12)]
    out += [("fuzz%d" % i, random_graph(pkg, i)) for i in range(12)]
    return out


# ------------------------------------------------------------------ the Pi_p statement itself
def test_pi_p_series_is_the_dense_solve(pkg_product, got, toy_graphs):
    """pi_p_left's Neumann series equals alpha (I - (1 - alpha) P_p)^-1 from a dense solve, and p^T Pi_p is rule B."""
    for name, host in [("got", got)] + sorted(toy_graphs.items()):
        n = host.n
        rng = np.random.default_rng(n)
        _, dead, _ = kinds(host)
        s = rng.choice(n, size=min(4, n), replace=False)
        if dead.size:
            s[0] = dead[0]
        w = rng.uniform(0.1, 1.0, size=s.size)
        p = seed_p(n, s, w)
        P = np.zeros((n, n))
        dout = np.diff(np.asarray(host.out_rp, dtype=np.int64))
        for v in range(n):
            if dout[v] == 0:
                P[v] = p
            for e in range(host.out_rp[v], host.out_rp[v + 1]):
                P[v, host.out_ci[e]] += 1.0 / dout[v]
        Pi = A * np.linalg.inv(np.eye(n) - (1 - A) * P)
        x = rng.uniform(0.0, 1.0, size=n)
        assert np.max(np.abs(pi_p_left(host, p, x, A) - x @ Pi)) <= 1e-13, name
        assert np.max(np.abs(pi_p_left(host, p, p, A) - p @ Pi)) <= 1e-14, name
        assert np.max(np.abs(rule_b(host, s, w, A) - p @ Pi)) <= 1e-13, name


# ------------------------------------------------------------------ 1. the exact invariant
def test_twin_seed_push_exact_invariant(pkg_product, orc, got, toy_graphs, rmat12):
    """After any seed-set push: p^T Pi_p = reserve + r^T Pi_p to 1e-12, every r/d < rmax.  Every level shape: sparse
    only, dense only and mixed, Jacobi and 2-, 3- and 6-block Gauss-Seidel sweeps."""
    dense_seen = gs_seen = 0
    try:
        for name, host in graphs(pkg_product, got, toy_graphs, rmat12):
            og = to_oracle(orc, host)
            sets = seed_sets(host, 5)
            if name == "rmat12":
                sets = sets[1:5:2] + sets[-1:]
            for frac, B in LEVEL_SHAPES:
                orc.set_sync_tuning(tuning(orc, frac, B))
                for i, (s, w) in enumerate(sets):
                    for rmax in (1e-3, 1e-6, 1e-9):
                        p, r, rsum, st = og.forward_push_seeds(s, A, rmax, weights=w)
                        check_exact(host, s, w, p, r, rmax, (name, frac, B, i, rmax))
                        assert abs(r.sum() - rsum) <= 1e-12
                        dense_seen += st.dense_levels
                        gs_seen += st.dense_levels if B > 1 else 0
                        if frac == 1e9:
                            assert st.dense_levels == 0
    finally:
        orc.set_sync_tuning(None)
    assert dense_seen > 0 and gs_seen > 0


# ------------------------------------------------------------------ 2. a set of one seed is the single-source call
def single_sources(host):
    live, dead, zin = kinds(host)
    out = [int(x) for x in live[:2]]
    out += [int(dead[0])] if dead.size else []
    out += [int(zin[0])] if zin.size else []
    return out


def test_twin_one_seed_is_bit_identical(pkg_product, orc, got, toy_graphs, rmat12):
    """orc_*_seeds([s]) against orc_forward_push, orc_fora_whole and orc_fora_topk on s: the same doubles and the same
    counters, for a live source, a dead-end source and a source without in-edges, over sparse, dense and Gauss-Seidel
    level shapes."""
    try:
        for name, host in [("got", got)] + sorted(toy_graphs.items()) + [("rmat12", rmat12)]:
            og = to_oracle(orc, host)
            for frac, B in ((0.05, 2), (1e-9, 1), (1e-9, 3), (1e9, 1)):
                t = tuning(orc, frac, B)
                orc.set_sync_tuning(t)
                for s in single_sources(host):
                    what = (name, frac, B, s)
                    for rmax in (1e-3, 1e-7):
                        p0, r0, rs0, st0 = og.forward_push(s, A, rmax, orc.SYNC)
                        p1, r1, rs1, st1 = og.forward_push_seeds([s], A, rmax)
                        assert np.array_equal(p0, p1) and np.array_equal(r0, r1) and rs0 == rs1, what
                        assert st0.as_dict() == st1.as_dict(), what
                    for n_rounds in (0, 1, 3):
                        e0, st0 = og.fora_whole(s, EPS, A, seed=3, n_rounds=n_rounds, schedule=orc.SYNC, tuning=t)
                        e1, st1 = og.fora_whole_seeds([s], EPS, A, seed=3, n_rounds=n_rounds, tuning=t)
                        assert np.array_equal(e0, e1) and st0.as_dict() == st1.as_dict(), (what, n_rounds)
                    for k in (1, 5):
                        e0, st0 = og.fora_topk(s, EPS, A, k, seed=4, schedule=orc.SYNC)
                        e1, st1 = og.fora_topk_seeds([s], EPS, A, k, seed=4)
                        assert np.array_equal(e0, e1) and st0.as_dict() == st1.as_dict(), (what, k)
    finally:
        orc.set_sync_tuning(None)


# ------------------------------------------------------------------ 3. normalization
def test_seed_plan_closed_form(pkg_product, orc, got, toy_graphs):
    """orc_seed_plan from DESIGN §2: p, live seeds first, q_i = p_i / (1 - (1 - alpha) D), e_j = alpha p_j / (...), the
    shares adding up to 1; every seed a dead end: p itself."""
    for name, host in [("got", got)] + sorted(toy_graphs.items()):
        og = to_oracle(orc, host)
        dout = np.diff(np.asarray(host.out_rp, dtype=np.int64))
        for s, w in seed_sets(host, 9):
            ids, p, lw, n_live = og.seed_plan(s, w, A)
            want = seed_p(host.n, s, w)
            assert np.max(np.abs(want[ids] - p)) <= 1e-16 and np.count_nonzero(want) == ids.size, name
            assert np.all(dout[ids[:n_live]] > 0) and np.all(dout[ids[n_live:]] == 0)
            assert np.all(np.diff(ids[:n_live]) > 0) and np.all(np.diff(ids[n_live:]) > 0)
            D = p[n_live:].sum()
            den = 1.0 - (1.0 - A) * D
            if n_live:
                assert np.max(np.abs(lw[:n_live] - p[:n_live] / den)) <= 1e-15
                assert np.max(np.abs(lw[n_live:] - A * p[n_live:] / den), initial=0) <= 1e-15
            else:
                assert np.array_equal(lw, p)
            assert abs(lw.sum() - 1.0) <= 1e-14, (name, lw.sum())


def test_twin_normalization_is_invariant(pkg_product, orc, got, rmat12):
    """Permuting the set, splitting a weight across duplicates, adding zero weights or scaling every weight by 1e-100 or
    1e100 gives the same vectors to 1e-15; the inputs the rule rejects are rejected."""
    orc.set_sync_tuning(tuning(orc, 0.002, 3))
    try:
        for host in (got, rmat12):
            og = to_oracle(orc, host)
            live, dead, _ = kinds(host)
            rng = np.random.default_rng(3)
            s = np.concatenate([rng.choice(live, size=9, replace=False), dead[:3]])
            w = rng.uniform(0.1, 1.0, size=s.size)
            base = og.forward_push_seeds(s, A, 1e-7, weights=w)
            fbase = og.fora_whole_seeds(s, EPS, A, seed=2, weights=w, n_rounds=0, tuning=tuning(orc, 0.002, 3))
            perm = rng.permutation(s.size)
            split_s = np.concatenate([s, s[:4]])
            split_w = np.concatenate([w[:4] / 2, w[4:], w[:4] / 2])
            zero_s = np.concatenate([s, rng.choice(host.n, size=5)])
            zero_w = np.concatenate([w, np.zeros(5)])
            for what, (s2, w2) in {"permuted": (s[perm], w[perm]), "split": (split_s, split_w),
                                   "zeros": (zero_s, zero_w), "1e-100": (s, w * 1e-100),
                                   "1e100": (s, w * 1e100)}.items():
                p, r, rsum, st = og.forward_push_seeds(s2, A, 1e-7, weights=w2)
                assert np.max(np.abs(p - base[0])) <= 1e-15 and np.max(np.abs(r - base[1])) <= 1e-15, what
                assert st.levels == base[3].levels and st.pops == base[3].pops, what
                est, stf = og.fora_whole_seeds(s2, EPS, A, seed=2, weights=w2, n_rounds=0,
                                               tuning=tuning(orc, 0.002, 3))
                assert stf.walks == fbase[1].walks and np.max(np.abs(est - fbase[0])) <= 1e-15, what
            bad = [([], None), ([host.n], None), ([-1], None), ([1, 2], [1.0, -0.5]), ([1], [np.nan]),
                   ([1], [np.inf]), ([1, 2], [0.0, 0.0]), ([1, 2], [1e308, 1e308])]
            for s2, w2 in bad:
                for call in (lambda: og.forward_push_seeds(s2, A, 1e-4, weights=w2),
                             lambda: og.fora_whole_seeds(s2, EPS, A, seed=1, weights=w2),
                             lambda: og.fora_topk_seeds(s2, EPS, A, 3, seed=1, weights=w2),
                             lambda: og.seed_plan(s2, w2, A)):
                    with pytest.raises(orc.SeedSetError):
                        call()
    finally:
        orc.set_sync_tuning(None)


# ------------------------------------------------------------------ 4. FORA and top-k against rule B
def test_twin_fora_seeds_bound(pkg_product, orc, got, rmat12):
    """The twin's FORA over seed sets meets the (eps, 1/n) bound against rule B; every seed a dead end gives p."""
    for host in (got, rmat12):
        og = to_oracle(orc, host)
        rng = np.random.default_rng(11)
        delta = 1.0 / host.n
        live, dead, _ = kinds(host)
        for k in (2, 10, 100, host.n // 2):
            s = rng.choice(host.n, size=k, replace=False)
            s[0] = live[0]
            for w in (None, rng.uniform(0.0, 2.0, size=k)):
                pi = rule_b(host, s, w, A)
                for n_rounds, frac in ((0, 0.05), (2, 0.05), (0, 0.002)):
                    t = tuning(orc, frac, 2)
                    est, st = og.fora_whole_seeds(s, EPS, A, seed=5, weights=w, n_rounds=n_rounds, tuning=t)
                    assert abs(est.sum() - 1.0) < 1e-9
                    big = pi > delta
                    assert np.all(np.abs(est[big] - pi[big]) <= EPS * pi[big]), (host.n, k, n_rounds, frac)
        est, st = og.fora_whole_seeds(dead[:5], EPS, A, seed=1, weights=np.arange(1.0, 6.0))
        want = seed_p(host.n, dead[:5], np.arange(1.0, 6.0))
        assert np.max(np.abs(est - want)) <= 1e-15 and st.walks == 0 and st.rounds == 1


def test_twin_fora_topk_seeds_against_rule_b(pkg_product, orc, got, rmat12):
    """The twin's top-k over seed sets: ordered output, the eps/2 bound on the reported entries, set identity where the
    exact values around the k-th place are further apart than that bound (as test_gpu_seeds.topk_ok for the engine)."""
    decided = 0
    for host, k in ((got, 10), (rmat12, 32)):
        og = to_oracle(orc, host)
        rng = np.random.default_rng(8)
        # (not the set of one live seed among many dead ends: walks restart at their start node at a dead end, the
        # walk quirk of DESIGN §2, which rule B's bound does not allow for once D is close to 1)
        sets = seed_sets(host, 21)
        for s, w in sets[1:4] + sets[5:6]:
            for eps in (EPS, 0.05):
                est, st = og.fora_topk_seeds(s, eps, A, k, seed=5, weights=w)
                pi = rule_b(host, s, w, A)
                n_sel, ids, vals = orc.topk(est, k)
                assert np.all(np.diff(vals) <= 0) and est.sum() <= 1.0 + 1e-9
                order = np.lexsort((np.arange(host.n), -pi))
                v = pi[order]
                kk = min(k, n_sel, int((pi > 0).sum()))
                kth = v[kk - 1]
                top = ids[:kk]
                assert np.all(np.abs(vals[:kk] - pi[top]) <= 0.5 * eps * np.maximum(pi[top], kth)), (host.n, eps)
                if v.size > k and v[k] > 0 and (v[k - 1] - v[k]) > 2 * 0.5 * eps * v[k - 1]:
                    assert set(ids[:k].tolist()) == set(order[:k].tolist())
                    decided += 1
        _, dead, _ = kinds(host)
        est, st = og.fora_topk_seeds(dead[:3], EPS, A, 3, seed=1)
        assert np.max(np.abs(est - seed_p(host.n, dead[:3], None))) <= 1e-15 and st.walks == 0 and st.rounds == 0
    assert decided > 0
