"""Single-pair PPR on the device (pprhip_walk_survival, pprhip_ppr_pairs; include/pprhip.h "single pairs", DESIGN.md §2
"Single pairs"): the survival vector against a dense solve, every value against a host recomputation from the engine's
own parts (backward push, survival, walk terminals), the accuracy guarantee against the exact PPR, invariance of a
pair's value under the call it is in, call shapes, arguments and state, and a full-size check at R-MAT 22."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import edges_to_host, shared_graph

pytestmark = pytest.mark.gpu
A = 0.15


# ------------------------------------------------------------------ host references
def _transition(host):
    """Row-stochastic P over the out-CSR (parallel edges counted), dead-end rows zero."""
    n = host.n
    P = np.zeros((n, n))
    for u in range(n):
        b, e = int(host.out_rp[u]), int(host.out_rp[u + 1])
        for v in host.out_ci[b:e]:
            P[u, int(v)] += 1.0 / (e - b)
    return P


def survival_dense(host, alpha):
    P = _transition(host)
    return np.linalg.solve(np.eye(host.n) - (1.0 - alpha) * P, np.full(host.n, alpha))


def ppr_exact(host, alpha):
    """pi[s, t] of the restarting walk (the engine's pi): the leaking PPR divided by the survival of its source."""
    P = _transition(host)
    leak = alpha * np.linalg.inv(np.eye(host.n) - (1.0 - alpha) * P)
    return leak / leak.sum(axis=1, keepdims=True)


def pair_reference(pkg, g, host, s, t, alpha, rmax, walks, seed, surv):
    """The estimate of pair (s, t) from the engine's parts: the push of pprhip_backward_push at the call's r_max (under
    the handle's tuning, as the pair call), S, and the terminals of the pair walks."""
    if host.in_rp[t + 1] == host.in_rp[t]:  # no in-edges: p_t(t) = alpha, no residue (pprhip_backward_push differs)
        return alpha / surv[t] if s == t else 0.0
    p, r, _ = g.backward_push(t, alpha, rmax)
    term, _ = g.random_walks(np.full(walks, s, dtype=np.int32), np.arange(walks, dtype=np.uint64), alpha, seed,
                             stream=pkg.PAIR_WALK_STREAM, no_zero_hop=False)
    return p[s] / surv[s] + float(np.sum(r[term])) / walks


# ------------------------------------------------------------------ fixtures
@pytest.fixture
def dev_got(pkg, got, dev_cache):
    return shared_graph(dev_cache, pkg, "got", lambda: pkg.Graph(got))


@pytest.fixture
def dev_r12(pkg, rmat12, dev_cache):
    return shared_graph(dev_cache, pkg, "r12", lambda: pkg.Graph(rmat12))


def _special_nodes(host):
    od, idg = np.diff(host.out_rp), np.diff(host.in_rp)
    return (np.flatnonzero(od == 0), np.flatnonzero(idg == 0), np.flatnonzero((od == 0) & (idg == 0)))


# ------------------------------------------------------------------ 1. survival
@pytest.mark.parametrize("alpha", [0.05, 0.15, 0.5])
def test_walk_survival_against_dense_solve(pkg, got, rmat12, toy_graphs, alpha):
    iso = edges_to_host(pkg, 9, [(0, 1), (1, 2), (2, 0), (2, 3), (5, 6)])  # 4, 7, 8 isolated; 3, 6 dead ends
    graphs = {"got": got, "rmat12": rmat12, "cycle5": toy_graphs["cycle5"],
              "star_dead_leaves": toy_graphs["star_dead_leaves"], "isolated_mix": toy_graphs["isolated_mix"],
              "isolated": iso}
    for name, host in graphs.items():
        with pkg.Graph(host) as g:
            S = g.walk_survival(alpha)
            ref = survival_dense(host, alpha)
            assert np.max(np.abs(S - ref)) <= 1e-12, (name, alpha, np.max(np.abs(S - ref)))
            if name == "cycle5":
                assert np.max(np.abs(S - 1.0)) <= 1e-12
            dead = np.flatnonzero(np.diff(host.out_rp) == 0)
            assert np.all(S[dead] == alpha), name
            # kept per alpha, rebuilt when alpha changes
            S2 = g.walk_survival(0.3)
            assert np.max(np.abs(S2 - survival_dense(host, 0.3))) <= 1e-12
            assert np.array_equal(g.walk_survival(alpha), S)


# ------------------------------------------------------------------ 2. exact against its own parts
def _sample_pairs(host, rng, count):
    dead, noin, iso = _special_nodes(host)
    n = host.n
    pairs = [(int(s), int(t)) for s, t in zip(rng.integers(0, n, count), rng.integers(0, n, count))]
    pairs += [(int(s), int(rng.integers(0, n))) for s in dead[:6]]          # dead-end sources
    pairs += [(int(t), int(t)) for t in noin[:4]] + [(int(rng.integers(0, n)), int(t)) for t in noin[:4]]
    pairs += [(int(v), int(v)) for v in rng.integers(0, n, 4)]            # s = t
    pairs += [(int(v), int(rng.integers(0, n))) for v in iso[:3]] + [(int(rng.integers(0, n)), int(v)) for v in iso[:3]]
    return pairs


@pytest.mark.parametrize("which", ["got", "rmat12"])
def test_pairs_equal_host_recomputation_from_parts(pkg, got, rmat12, dev_got, dev_r12, which):
    host, g = (got, dev_got) if which == "got" else (rmat12, dev_r12)
    rng = np.random.default_rng(7)
    pairs = _sample_pairs(host, rng, 40)
    if which == "rmat12":
        assert len(_special_nodes(host)[2]) > 0  # the sample holds isolated nodes
    s, t = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    eps, seed = 0.5, 11
    conf = pkg.conf_whole_graph(host.n, host.m, A)
    rmax, walks = pkg.pair_params(conf, eps)
    g.set_tuning(pkg.tuning_default())
    vals, st = g.ppr_pairs(s, t, eps, A, seed)
    assert st.rmax_final == rmax and st.walks > 0 and st.walk_steps > 0
    surv = g.walk_survival(A)
    for i, (a, b) in enumerate(pairs):
        ref = pair_reference(pkg, g, host, a, b, A, rmax, walks, seed, surv)
        assert abs(vals[i] - ref) <= 1e-12 * abs(ref) + 1e-300, (which, a, b, vals[i], ref)


def test_pairs_equal_parts_under_a_dense_tuning(pkg, rmat12, dev_r12):
    """The push runs under the handle's tuning: with dense levels (low dense_frac) the values still equal the parts
    computed by pprhip_backward_push under the same tuning."""
    g, host = dev_r12, rmat12
    t_ = pkg.tuning_batch()
    t_.dense_frac = 0.002
    g.set_tuning(t_)
    try:
        rng = np.random.default_rng(3)
        idg = np.diff(host.in_rp.astype(np.int64))
        hubs = np.argsort(-idg)[:6]
        pairs = [(int(rng.integers(0, host.n)), int(h)) for h in hubs]
        conf = pkg.conf_whole_graph(host.n, host.m, A)
        rmax, walks = pkg.pair_params(conf, 0.5, 1e-4)
        vals, st = g.ppr_pairs([p[0] for p in pairs], [p[1] for p in pairs], 0.5, A, 5, rmax=1e-4)
        assert st.dense_levels > 0
        surv = g.walk_survival(A)
        for i, (a, b) in enumerate(pairs):
            ref = pair_reference(pkg, g, host, a, b, A, rmax, walks, 5, surv)
            assert abs(vals[i] - ref) <= 1e-12 * abs(ref) + 1e-300, (a, b, vals[i], ref)
    finally:
        g.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 3. accuracy
def test_pairs_accuracy_all_got_pairs(pkg, got, dev_got):
    eps = 0.2
    n = got.n
    conf = pkg.conf_whole_graph(n, got.m, A)
    delta, pfail = conf.delta, conf.pfail
    s, t = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    vals, st = dev_got.ppr_pairs(s.ravel(), t.ravel(), eps, A, 2024)
    pi = ppr_exact(got, A).ravel()
    bad = np.abs(vals - pi) > eps * np.maximum(pi, delta)
    # the guarantee is per pair with probability >= 1 - pfail: the expected failures are at most pfail * n^2 (= n);
    # the Chernoff bound is loose, so the count lies far below that in practice - slack 5 covers a rare cluster of
    # failures among pairs that share a target (their walks are independent, their residue vector is not)
    assert int(bad.sum()) <= pfail * n * n + 5, int(bad.sum())
    assert np.max(np.abs(vals - pi)) <= eps * max(np.max(pi), delta)


# ------------------------------------------------------------------ 4. batch invariance
def _invariance_case(pkg, g, host, monkeypatch):
    rng = np.random.default_rng(99)
    q = 1000
    s = rng.integers(0, host.n, q).astype(np.int32)
    t = rng.integers(0, host.n, q).astype(np.int32)
    t[:200] = t[0]  # one target with many sources in the mix
    probe = [0, 1, 5, 250, 999]
    alone = np.array([g.ppr_pairs([s[i]], [t[i]], 0.5, A, 17)[0][0] for i in probe])
    base, _ = g.ppr_pairs(s, t, 0.5, A, 17)
    assert np.allclose(base[probe], alone, rtol=1e-12, atol=0)
    perm = rng.permutation(q)
    pv, _ = g.ppr_pairs(s[perm], t[perm], 0.5, A, 17)
    assert np.allclose(pv[np.argsort(perm)], base, rtol=1e-12, atol=0)
    for ws in ("16", "32"):
        monkeypatch.setenv("PPRHIP_BATCH_WORKSPACES", ws)
        wv, _ = g.ppr_pairs(s, t, 0.5, A, 17)
        assert np.allclose(wv, base, rtol=1e-12, atol=0), ws
    monkeypatch.delenv("PPRHIP_BATCH_WORKSPACES")
    monkeypatch.setenv("PPRHIP_BATCH_THREADS", "0")  # the single-thread driver
    sv, _ = g.ppr_pairs(s, t, 0.5, A, 17)
    monkeypatch.delenv("PPRHIP_BATCH_THREADS")
    assert np.allclose(sv, base, rtol=1e-12, atol=0)
    return base


def test_pairs_batch_invariance(pkg, rmat12, dev_r12, monkeypatch):
    g = dev_r12
    g.set_tuning(pkg.tuning_default())
    _invariance_case(pkg, g, rmat12, monkeypatch)
    t_ = pkg.tuning_default()
    t_.dense_frac = 0.002  # the targets' pushes take shared dense levels
    g.set_tuning(t_)
    try:
        _, st = g.ppr_pairs(np.arange(64), np.argsort(-np.diff(rmat12.in_rp.astype(np.int64)))[:64], 0.5, A, 17)
        assert st.dense_levels > 0
        _invariance_case(pkg, g, rmat12, monkeypatch)
    finally:
        g.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 5. shapes
def test_pairs_shapes(pkg, rmat12, dev_r12):
    g, host = dev_r12, rmat12
    g.set_tuning(pkg.tuning_default())
    rng = np.random.default_rng(5)
    t0 = int(np.argmax(np.diff(host.in_rp)))
    srcs = rng.integers(0, host.n, 600)
    v1, st1 = g.ppr_pairs(srcs, np.full(600, t0), 0.5, A, 3)
    assert st1.walks == 600 * pkg.pair_params(pkg.conf_whole_graph(host.n, host.m, A), 0.5)[1]
    s0 = int(np.argmax(np.diff(host.out_rp)))
    tg = rng.integers(0, host.n, 300)
    v2, _ = g.ppr_pairs(np.full(300, s0), tg, 0.5, A, 3)
    for i in (0, 17, 599):
        assert v1[i] == pytest.approx(g.ppr_pairs([srcs[i]], [t0], 0.5, A, 3)[0][0], rel=1e-12, abs=0)
    for i in (0, 33, 299):
        assert v2[i] == pytest.approx(g.ppr_pairs([s0], [tg[i]], 0.5, A, 3)[0][0], rel=1e-12, abs=0)
    dup_s, dup_t = np.array([s0, 7, s0, 7, s0]), np.array([t0, 9, t0, 9, t0])
    vd, _ = g.ppr_pairs(dup_s, dup_t, 0.5, A, 3)
    assert vd[0] == vd[2] == vd[4] and vd[1] == vd[3]
    v0, st0 = g.ppr_pairs(np.zeros(0), np.zeros(0), 0.5, A, 3)
    assert v0.size == 0 and st0.walks == 0


# ------------------------------------------------------------------ 6. arguments and state
def test_pairs_bad_ids_write_nothing(pkg, dev_got, got):
    L = pkg.lib()
    conf = pkg.conf_whole_graph(got.n, got.m, A)
    for s_, t_ in (([0, got.n], [1, 2]), ([0, 1], [2, -1]), ([-5, 1], [2, 3])):
        s = np.array(s_, dtype=np.int32)
        t = np.array(t_, dtype=np.int32)
        out = np.full(2, 123.0)
        st = pkg.Stats()
        rc = L.pprhip_ppr_pairs(dev_got.h, s.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), 2, 0.5,
                                C.byref(conf), 0.0, 1, out.ctypes.data_as(C.c_void_p), C.byref(st))
        assert rc == pkg.ERR_INVALID and "pair" in L.pprhip_last_error().decode()
        assert np.all(out == 123.0)


def test_pairs_refused_while_a_stream_is_open(pkg, dev_got):
    qs = pkg.QueryStream(dev_got, 0.5, A)
    try:
        with pytest.raises(pkg.PprhipError) as e:
            dev_got.ppr_pairs([0], [1], 0.5, A, 1)
        assert e.value.code == pkg.ERR_STATE
        with pytest.raises(pkg.PprhipError):
            dev_got.walk_survival(A)
    finally:
        qs.close()


def test_other_paths_unchanged_after_a_pair_call(pkg, got):
    src = int(np.argmax(np.diff(got.out_rp)))
    def run(g):
        f, _ = g.fora_single_source(src, 0.5, A, seed=3)
        p, r, _ = g.backward_push(src, A, 1e-4)
        ids, vals, _ = g.fora_batch_topk([src, 0, 17], 10, 0.5, A, 4)
        return f, p, r, ids, vals
    with pkg.Graph(got) as fresh:
        ref = run(fresh)
    with pkg.Graph(got) as g:
        g.ppr_pairs(np.arange(50), np.arange(50)[::-1], 0.5, A, 9)
        got_ = run(g)
    # (the same computation on both handles; walks add with fp64 atomics, so the bits may differ in the last places)
    for a, b in zip(ref, got_):
        if a.dtype.kind == "f":
            assert np.allclose(a, b, rtol=1e-12, atol=1e-15)
        else:
            assert np.array_equal(a, b)


def test_pairs_memory_steady(pkg, rmat12, dev_r12):
    g = dev_r12
    rng = np.random.default_rng(1)
    s, t = rng.integers(0, rmat12.n, 300), rng.integers(0, rmat12.n, 300)
    g.ppr_pairs(s, t, 0.5, A, 1)
    free0, _ = g.device_memory()
    for i in range(20):
        g.ppr_pairs(s, t, 0.5, A, 1 + i)
    free1, _ = g.device_memory()
    assert free1 == free0


# ------------------------------------------------------------------ 7. full size
@pytest.mark.timeout(1200)
def test_full_size_rmat22_pairs_against_power_method(pkg):
    host = pkg.HostCsr.rmat(22, 16, seed=1)
    eps = 0.5
    rng = np.random.default_rng(22)
    od = np.diff(host.out_rp)
    with pkg.Graph(host) as g:
        conf = pkg.conf_whole_graph(host.n, host.m, A)
        delta = conf.delta
        srcs = rng.integers(0, host.n, 64)
        tgts = rng.integers(0, host.n, 64)
        live = np.flatnonzero(od > 0)
        four = rng.choice(live, 4, replace=False)
        pis = {}
        pairs_s, pairs_t = list(srcs), list(tgts)
        for s in four:
            pi, _ = g.power_method(int(s), A, 200)
            pis[int(s)] = pi
            top = np.argsort(-pi, kind="stable")[:16]
            pairs_s += [int(s)] * 16
            pairs_t += [int(x) for x in top]
        vals, st = g.ppr_pairs(pairs_s, pairs_t, eps, A, 77)
        assert st.walks > 0
        bad = 0
        for i, (s, t) in enumerate(zip(pairs_s, pairs_t)):
            s = int(s)
            if s not in pis:
                pis[s] = g.power_method(s, A, 200)[0]
            pi = pis[s][int(t)]
            if abs(vals[i] - pi) > eps * max(pi, delta):
                bad += 1
        assert bad == 0, bad
