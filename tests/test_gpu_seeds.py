"""Seed sets on the GPU: forward push, FORA and FORA top-k personalized to a weighted node set, against the single-source calls
(a set of one seed), the push invariant, and the numpy rule-B oracle of tests/test_seeds.py."""
import numpy as np
import pytest

from conftest import shared_graph
from test_seeds import exact_invariant_err, rule_b, seed_p

pytestmark = pytest.mark.gpu

A = 0.15
EPS = 0.5
STAT_FIELDS = ("rounds", "levels", "dense_levels", "walks", "mc_sources")


@pytest.fixture
def dev_got(pkg, got, dev_cache):
    return shared_graph(dev_cache, pkg, "dev_got", lambda: pkg.Graph(got))


@pytest.fixture
def dev_rmat12(pkg, rmat12, dev_cache):
    return shared_graph(dev_cache, pkg, "dev_rmat12", lambda: pkg.Graph(rmat12))


def degrees(host):
    return np.diff(np.asarray(host.out_rp, dtype=np.int64)), np.diff(np.asarray(host.in_rp, dtype=np.int64))


def kinds(host):
    """(live nodes, dead ends, live nodes without in-edges)"""
    dout, din = degrees(host)
    live = np.nonzero(dout > 0)[0]
    dead = np.nonzero(dout == 0)[0]
    zin = np.nonzero((dout > 0) & (din == 0))[0]
    return live, dead, zin


def one_seed_sources(host, count=3, seed=4):
    live, dead, zin = kinds(host)
    rng = np.random.default_rng(seed)
    out = [int(x) for x in rng.choice(live, size=count, replace=False)]
    out.append(int(np.argmax(np.diff(np.asarray(host.out_rp)))))  # the hub
    if dead.size:
        out.append(int(dead[0]))
    if zin.size:
        out.append(int(zin[0]))
    return out


def mixed_set(host, k, seed):
    """k seeds that mix live nodes, dead ends, live nodes without in-edges and duplicates, with random weights"""
    live, dead, zin = kinds(host)
    rng = np.random.default_rng(seed)
    parts = [rng.choice(live, size=min(live.size, max(1, k - 4)), replace=False)]
    if dead.size:
        parts.append(rng.choice(dead, size=min(2, dead.size), replace=False))
    if zin.size:
        parts.append(zin[:1])
    s = np.concatenate(parts)
    s = np.concatenate([s, s[:1]])  # a duplicate
    return s.astype(np.int32), rng.uniform(0.1, 1.0, size=s.size)


def same_stats(a, b, what):
    for f in STAT_FIELDS:
        assert getattr(a, f) == getattr(b, f), (what, f, getattr(a, f), getattr(b, f))


def check_invariant(host, p, r, rsum, rmax, pi=None, tol=1e-12, seeds=None, weights=None):
    """The band 0 <= pi_p - reserve <= rsum, and - given the set, on graphs up to R-MAT 12 - the exact invariant
    p^T Pi_p = reserve + r^T Pi_p (tests/test_seeds.py), which a landing error smaller than rsum breaks as well."""
    dout, _ = degrees(host)
    assert abs(p.sum() + rsum - 1.0) <= tol
    assert abs(r.sum() - rsum) <= tol
    live = dout > 0
    assert np.all(r[live] / dout[live] < rmax)
    assert np.all(r[~live] == 0.0)
    assert np.all(p >= 0.0) and np.all(r >= 0.0)
    if pi is not None:
        gap = pi - p
        assert np.all(gap >= -tol) and np.all(gap <= rsum + tol)
    if seeds is not None and host.n <= 4096:
        err = exact_invariant_err(host, seed_p(host.n, seeds, weights), p, r, A)
        assert err <= tol, ("exact invariant", err)


def topk_ok(host, seeds, weights, eps, k, n_sel, ids, vals, est, what):
    """what test_fora_topk_vs_cpu_power_method asserts, against rule B: ordered output, the eps/2 bound on the reported
    entries, and set identity where the exact values around the k-th place are further apart than that bound"""
    pi = rule_b(host, seeds, weights, A)
    assert np.all(np.diff(vals) <= 0) and np.array_equal(est[ids], vals), what
    order = np.lexsort((np.arange(host.n), -pi))
    v = pi[order]
    kk = min(k, n_sel, int((pi > 0).sum()))
    kth = v[kk - 1]
    top = ids[:kk]
    assert np.all(np.abs(vals[:kk] - pi[top]) <= 0.5 * eps * np.maximum(pi[top], kth)), what
    if v.size > k and v[k] > 0 and (v[k - 1] - v[k]) > 2 * 0.5 * eps * v[k - 1]:
        assert set(ids[:k].tolist()) == set(order[:k].tolist()), what
        return True
    return False


def fora_bound_ok(est, exact, eps, delta):
    big = exact > delta
    return np.all(np.abs(est[big] - exact[big]) <= eps * exact[big])


def lowered(pkg, frac):
    t = pkg.tuning_default()
    t.dense_frac = frac
    return t


# ------------------------------------------------------------------ 1. a set of one seed is the single-source call
@pytest.mark.parametrize("dense_frac", [None, 0.002])
def test_one_seed_equals_single_source(pkg, got, dev_got, rmat12, dev_rmat12, dense_frac):
    for host, dev in ((got, dev_got), (rmat12, dev_rmat12)):
        if dense_frac is not None:
            dev.set_tuning(lowered(pkg, dense_frac))
        try:
            for s in one_seed_sources(host):
                for rmax in (1e-4, 1e-7):
                    p0, r0, rs0, st0 = dev.forward_push(s, A, rmax)
                    p1, r1, rs1, st1 = dev.forward_push_seeds([s], A, rmax)
                    same_stats(st0, st1, ("push", s, rmax))
                    assert np.max(np.abs(p0 - p1)) <= 1e-12 and np.max(np.abs(r0 - r1)) <= 1e-12
                    assert abs(rs0 - rs1) <= 1e-12
                for n_rounds in (0, 3):
                    e0, st0 = dev.fora_single_source(s, EPS, A, seed=3, n_rounds=n_rounds)
                    e1, st1 = dev.fora_seeds([s], EPS, A, seed=3, n_rounds=n_rounds)
                    same_stats(st0, st1, ("fora", s, n_rounds))
                    assert np.max(np.abs(e0 - e1)) <= 1e-12, (s, n_rounds)
                    assert np.array_equal(dev.reserve(), e1)
                k = 10 if host is got else 32
                n0, i0, v0, e0, st0 = dev.fora_topk(s, EPS, A, k, seed=5, cap=host.n, fetch=True)
                n1, i1, v1, e1, st1 = dev.fora_topk_seeds([s], EPS, A, k, seed=5, cap=host.n, fetch=True)
                same_stats(st0, st1, ("topk", s))
                assert np.max(np.abs(e0 - e1)) <= 1e-12, s
                assert n0 == n1 and np.array_equal(i0, i1), s
                assert np.array_equal(dev.reserve(), e1)
        finally:
            dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 2. the forward-push invariant
@pytest.mark.parametrize("dense_frac", [None, 0.002])
def test_push_invariant_mixed_sets(pkg, got, dev_got, rmat12, dev_rmat12, dense_frac):
    dense_seen = 0
    for host, dev in ((got, dev_got), (rmat12, dev_rmat12)):
        if dense_frac is not None:
            dev.set_tuning(lowered(pkg, dense_frac))
        try:
            for k, sd in ((3, 1), (12, 2), (60, 3)):
                s, w = mixed_set(host, k, sd)
                pi = rule_b(host, s, w, A)
                for rmax in (1e-3, 1e-6, 1e-9):
                    p, r, rsum, st = dev.forward_push_seeds(s, A, rmax, weights=w)
                    check_invariant(host, p, r, rsum, rmax, pi, seeds=s, weights=w)
                    assert np.array_equal(dev.residue(), r)
                    dense_seen += st.dense_levels
                # the same sets through the top-k push (parking, arming and landing in top-k mode)
                n_sel, ids, vals, est, st = dev.fora_topk_seeds(s, EPS, A, 10, seed=2, weights=w, cap=host.n, fetch=True)
                topk_ok(host, s, w, EPS, 10, n_sel, ids, vals, est, ("topk", k, sd))
                assert est.sum() <= 1.0 + 1e-9
                dense_seen += st.dense_levels
        finally:
            dev.set_tuning(pkg.tuning_default())
    if dense_frac is not None:
        assert dense_seen > 0


# ------------------------------------------------------------------ 3. FORA's (eps, 1/n) bound against rule B
def test_fora_seeds_bound(pkg, got, dev_got, rmat12, dev_rmat12):
    for host, dev in ((got, dev_got), (rmat12, dev_rmat12)):
        live, _, _ = kinds(host)
        rng = np.random.default_rng(11)
        delta = 1.0 / host.n
        for k in (2, 10, 100, host.n // 2):
            s = rng.choice(host.n, size=k, replace=False).astype(np.int32)
            if not np.isin(s, live).any():
                s[0] = live[0]
            for w in (None, rng.uniform(0.0, 2.0, size=k)):
                pi = rule_b(host, s, w, A)
                for n_rounds in (0, 2):
                    est, st = dev.fora_seeds(s, EPS, A, seed=5, weights=w, n_rounds=n_rounds)
                    assert abs(est.sum() - 1.0) < 1e-9 or (st.walks == 0 and abs(est.sum() + st.rsum - 1.0) < 1e-12)
                    assert fora_bound_ok(est, pi, EPS, delta), (k, n_rounds, w is None)
    # dense levels from a seed set
    dev_rmat12.set_tuning(lowered(pkg, 0.002))
    try:
        s, w = mixed_set(rmat12, 40, 9)
        pi = rule_b(rmat12, s, w, A)
        est, st = dev_rmat12.fora_seeds(s, EPS, A, seed=6, weights=w)
        assert st.dense_levels > 0
        assert fora_bound_ok(est, pi, EPS, 1.0 / rmat12.n)
    finally:
        dev_rmat12.set_tuning(pkg.tuning_default())


def test_fora_seeds_at_scale(pkg):
    """R-MAT 18 (as in test_fora_at_scale_vs_cpu_power_method): sparse and sliced dense levels, large sets"""
    host = pkg.HostCsr.rmat(18, 16, seed=1)
    rng = np.random.default_rng(3)
    with pkg.Graph(host) as g:
        for k in (100, host.n // 2):
            s = rng.choice(host.n, size=k, replace=False).astype(np.int32)
            w = rng.uniform(0.0, 1.0, size=k)
            pi = rule_b(host, s, w, A)
            est, st = g.fora_seeds(s, EPS, A, seed=7, weights=w)
            assert fora_bound_ok(est, pi, EPS, 1.0 / host.n), k
            p, r, rsum, st = g.forward_push_seeds(s, A, 1e-9, weights=w)
            check_invariant(host, p, r, rsum, 1e-9, pi, seeds=s, weights=w)
            assert st.dense_levels > 0


# ------------------------------------------------------------------ 4. every seed a dead end
def test_all_seeds_dead_ends_give_p(got, dev_got, rmat12, dev_rmat12):
    for host, dev in ((got, dev_got), (rmat12, dev_rmat12)):
        _, dead, _ = kinds(host)
        s = dead[:7].astype(np.int32)
        w = np.arange(1.0, s.size + 1.0)
        want = np.zeros(host.n)
        want[s] = w / w.sum()
        p, r, rsum, st = dev.forward_push_seeds(s, A, 1e-6, weights=w)
        assert np.max(np.abs(p - want)) <= 1e-15 and rsum == 0.0 and not r.any() and st.levels == 0
        est, st = dev.fora_seeds(s, EPS, A, seed=1, weights=w)
        assert np.max(np.abs(est - want)) <= 1e-15 and st.walks == 0
        assert np.max(np.abs(rule_b(host, s, w, A) - want)) <= 1e-13


# ------------------------------------------------------------------ 5. top-k against rule B
def test_fora_topk_seeds_against_rule_b(pkg, got, dev_got, rmat12, dev_rmat12):
    decided = 0
    for host, dev, k in ((got, dev_got, 10), (rmat12, dev_rmat12, 32)):
        rng = np.random.default_rng(8)
        for kk in (2, 10, 100):
            s, w = mixed_set(host, kk, int(rng.integers(1 << 30)))
            for weights in (None, w):
                for eps in (EPS, 0.05):
                    n_sel, ids, vals, est, _ = dev.fora_topk_seeds(s, eps, A, k, seed=5, weights=weights, cap=host.n,
                                                                   fetch=True)
                    decided += topk_ok(host, s, weights, eps, k, n_sel, ids, vals, est, (host.n, kk, eps))
                    n2, i2, _, _, _ = dev.topk_select(k, cap=host.n)
                    assert n2 == n_sel and np.array_equal(i2, ids)
    assert decided > 0  # (the set identity was decidable somewhere)
    _, dead, _ = kinds(got)
    n_sel, ids, vals, est, st = dev_got.fora_topk_seeds(dead[:3], EPS, A, 3, seed=1, cap=8, fetch=True)
    assert n_sel == 3 and set(ids.tolist()) == set(dead[:3].tolist()) and st.walks == 0
    assert np.max(np.abs(vals - 1.0 / 3)) <= 1e-15


# ------------------------------------------------------------------ 6. the row-panel sweep (graphs of 2^26 edges)
def test_seeds_row_panel_rmat22(pkg):
    host = pkg.HostCsr.rmat(22, 16, seed=1)
    assert host.m >= 1 << 26
    with pkg.Graph(host) as g:
        s, w = mixed_set(host, 1000, 5)
        p, r, rsum, st = g.forward_push_seeds(s, A, 1e-9, weights=w)
        check_invariant(host, p, r, rsum, 1e-9)
        assert st.dense_levels > 0
        src = int(np.argmax(np.diff(np.asarray(host.out_rp))))
        for rmax in (1e-9,):
            p0, r0, _, st0 = g.forward_push(src, A, rmax)
            p1, r1, _, st1 = g.forward_push_seeds([src], A, rmax)
            same_stats(st0, st1, "push")
            assert st1.dense_levels > 0
            assert np.max(np.abs(p0 - p1)) <= 1e-12 and np.max(np.abs(r0 - r1)) <= 1e-12
        e0, st0 = g.fora_single_source(src, EPS, A, seed=2)
        e1, st1 = g.fora_seeds([src], EPS, A, seed=2)
        same_stats(st0, st1, "fora")
        assert np.max(np.abs(e0 - e1)) <= 1e-12
        n0, i0, _, e0, st0 = g.fora_topk(src, EPS, A, 32, seed=2, cap=64, fetch=True)
        n1, i1, _, e1, st1 = g.fora_topk_seeds([src], EPS, A, 32, seed=2, cap=64, fetch=True)
        same_stats(st0, st1, "topk")
        assert n0 == n1 and np.array_equal(i0, i1) and np.max(np.abs(e0 - e1)) <= 1e-12
        g.set_tuning(lowered(pkg, 0.002))  # (top-k rounds push little: dense levels from 0.2 % of m)
        n_sel, ids, vals, est, st = g.fora_topk_seeds(s, EPS, A, 32, seed=3, weights=w, cap=64, fetch=True)
        assert st.dense_levels > 0 and n_sel >= 32
        assert np.all(np.diff(vals) <= 0) and np.array_equal(est[ids], vals) and est.sum() <= 1.0 + 1e-9
        g.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 7. arguments and state
def test_invalid_arguments(pkg, got, dev_got):
    bad = [([], None), ([got.n], None), ([-1], None), ([1, 2], [1.0, -1.0]), ([1], [np.nan]), ([1], [np.inf]),
           ([1, 2], [0.0, 0.0])]
    for s, w in bad:
        with pytest.raises(pkg.PprhipError) as e:
            dev_got.forward_push_seeds(s, A, 1e-4, weights=w)
        assert e.value.code == pkg.ERR_INVALID
        with pytest.raises(pkg.PprhipError) as e:
            dev_got.fora_seeds(s, EPS, A, seed=1, weights=w)
        assert e.value.code == pkg.ERR_INVALID
        with pytest.raises(pkg.PprhipError) as e:
            dev_got.fora_topk_seeds(s, EPS, A, 5, seed=1, weights=w)
        assert e.value.code == pkg.ERR_INVALID


def test_no_seed_state_leaks_into_single_source(pkg, rmat12):
    rng = np.random.default_rng(2)
    s = rng.choice(rmat12.n, size=rmat12.n // 2, replace=False).astype(np.int32)
    src = one_seed_sources(rmat12)[:3]
    with pkg.Graph(rmat12) as fresh:
        want = [fresh.fora_single_source(x, EPS, A, seed=4)[0] for x in src]
        want_push = [fresh.forward_push(x, A, 1e-7)[0] for x in src]
        want_topk = [fresh.fora_topk(x, EPS, A, 32, seed=4, cap=64, fetch=True)[3] for x in src]
    with pkg.Graph(rmat12) as g:
        for t in (pkg.tuning_default(), lowered(pkg, 0.002)):
            g.set_tuning(t)
            g.fora_seeds(s, EPS, A, seed=4)
            g.forward_push_seeds(s, A, 1e-7)
            g.fora_topk_seeds(s, EPS, A, 32, seed=4, cap=64)
        g.set_tuning(pkg.tuning_default())
        for x, e, pp, tk in zip(src, want, want_push, want_topk):
            assert np.max(np.abs(g.fora_single_source(x, EPS, A, seed=4)[0] - e)) <= 1e-12
            assert np.max(np.abs(g.forward_push(x, A, 1e-7)[0] - pp)) <= 1e-12
            g.fora_topk_seeds(s, EPS, A, 32, seed=4, cap=64)
            assert np.max(np.abs(g.fora_topk(x, EPS, A, 32, seed=4, cap=64, fetch=True)[3] - tk)) <= 1e-12
        g.fora_topk_seeds(s, EPS, A, 32, seed=4, cap=64)
        with pytest.raises(pkg.PprhipError) as e:  # a seed-set top-k session is not continued round by round
            g.topk_push_round(1e-6, 1e-5)
        assert e.value.code == pkg.ERR_STATE
