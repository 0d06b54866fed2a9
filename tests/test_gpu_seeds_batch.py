"""Batched seed sets on the GPU (pprhip_fora_batch_seeds, pprhip_fora_batch_topk_seeds): query i of a call is the
single-query seeded call on set i - the same rounds, levels, dense levels and walks, the vector to 1e-12 - whatever the
batch driver does around it; sets of one seed are the single-source batched calls; a sample meets the twin.  Then the
result store, state left on a handle, argument checks, memory and R-MAT 22."""
import ctypes as C

import numpy as np
import pytest

from conftest import shared_graph, to_oracle
from test_gpu_fuzz import check_fora, orc_tuning
from test_gpu_seeds import mixed_set, one_seed_sources, same_stats
from test_gpu_seeds_twin import SHAPES, seed_sets, set_shape

pytestmark = pytest.mark.gpu

A = 0.15
EPS = 0.5


@pytest.fixture
def dev_got(pkg, got, dev_cache):
    return shared_graph(dev_cache, pkg, "dev_got", lambda: pkg.Graph(got))


@pytest.fixture
def dev_rmat12(pkg, rmat12, dev_cache):
    return shared_graph(dev_cache, pkg, "dev_rmat12", lambda: pkg.Graph(rmat12))


@pytest.fixture
def dev_rmat15(pkg, rmat15, dev_cache):
    return shared_graph(dev_cache, pkg, "dev_rmat15", lambda: pkg.Graph(rmat15))


def lowered(pkg, frac):
    t = pkg.tuning_default()
    t.dense_frac = frac
    return t


def batch_sets(host, seed, extra=3):
    """seed_sets() of the twin test, twice (the second pass reversed: workspaces take sets of other sizes after one
    another), and a few mixed sets: more than one round of 16 columns."""
    named = list(seed_sets(host, seed).items())
    out = named + [(n + "'", sw) for n, sw in reversed(named)]
    for j in range(extra):
        out.append(("mixed%d" % j, mixed_set(host, 5 + 7 * j, seed + j)))
    return [n for n, _ in out], [s for _, (s, _) in out], [w for _, (_, w) in out]


def same_topk_rows(ids, vals, nsel_ids, nsel_vals, nsel, k, what):
    m = min(nsel, k)
    assert list(ids[:m]) == list(nsel_ids[:m]), what
    assert np.max(np.abs(vals[:m] - nsel_vals[:m]), initial=0) <= 1e-12, what
    assert np.all(ids[m:] == -1) and np.all(vals[m:] == 0.0), what


# ------------------------------------------------------------------ 1. sets of one seed are the single-source batch
@pytest.mark.parametrize("dense_frac", [None, 0.002])
def test_one_seed_sets_equal_single_source_batch(pkg, got, dev_got, rmat12, dev_rmat12, dense_frac):
    shared = 0
    for host, dev in ((got, dev_got), (rmat12, dev_rmat12)):
        rng = np.random.default_rng(5)
        srcs = one_seed_sources(host) + [int(x) for x in rng.integers(0, host.n, size=14)]  # >= 19: two rounds of 16
        dev.set_tuning(pkg.tuning_default() if dense_frac is None else lowered(pkg, dense_frac))
        try:
            for n_rounds in (2, 0):
                o0, i0, v0, n0, pq0, st0 = dev.fora_batch_single_source(srcs, EPS, A, seed=3, n_rounds=n_rounds, k=10,
                                                                         fetch=True, per_query=True)
                o1, i1, v1, n1, pq1, st1 = dev.fora_batch_seeds([[s] for s in srcs], EPS, A, seed=3,
                                                                n_rounds=n_rounds, k=10, fetch=True, per_query=True)
                for i, s in enumerate(srcs):
                    same_stats(pq0[i], pq1[i], ("one-seed batch", s, n_rounds))
                    assert np.max(np.abs(o0[i] - o1[i])) <= 1e-12, (s, n_rounds)
                assert np.array_equal(i0, i1) and np.array_equal(n0, n1)
                assert st1.dense_levels == st0.dense_levels
                if st1.dense_levels > 0:
                    assert 0 < st1.class_launches[5] <= st1.dense_levels
                    shared += st1.class_launches[5] < st1.dense_levels
            k = 10 if host is got else 32
            ti0, tv0, _ = dev.fora_batch_topk(srcs, k, EPS, A, seed=11)
            ti1, tv1, _ = dev.fora_batch_topk_seeds([[s] for s in srcs], k, EPS, A, seed=11)
            assert np.array_equal(ti0, ti1)
            assert np.max(np.abs(tv0 - tv1)) <= 1e-12
        finally:
            dev.set_tuning(pkg.tuning_default())
    if dense_frac is not None:
        assert shared > 0  # the batched sweep served several seeded queries per launch


# ------------------------------------------------------------------ 2. mixed sets are the single-query seed path
@pytest.mark.parametrize("graph", ["got", "rmat12", "rmat15"])
def test_mixed_sets_equal_single_query_path(pkg, orc, got, dev_got, rmat12, dev_rmat12, rmat15, dev_rmat15, graph):
    host, dev = {"got": (got, dev_got), "rmat12": (rmat12, dev_rmat12), "rmat15": (rmat15, dev_rmat15)}[graph]
    og = to_oracle(orc, host)
    names, sets, weights = batch_sets(host, seed=21)
    k = 10
    sweeps = 0
    try:
        for frac, B in SHAPES:
            t = set_shape(pkg, dev, frac, B)
            for n_rounds in (2, 0):
                out, _, _, _, pq, st = dev.fora_batch_seeds(sets, EPS, A, seed=7, weights=weights, n_rounds=n_rounds,
                                                            fetch=True, per_query=True)
                sweeps += st.class_launches[5]
                for i, (s, w) in enumerate(zip(sets, weights)):
                    what = (graph, frac, B, n_rounds, names[i])
                    est, sts = dev.fora_seeds(s, EPS, A, seed=7, weights=w, n_rounds=n_rounds)
                    same_stats(sts, pq[i], what)
                    assert np.max(np.abs(out[i] - est)) <= 1e-12, (what, float(np.max(np.abs(out[i] - est))))
                for i in (0, len(sets) // 2, len(sets) - 1):  # a sample against the twin
                    ref, sto = og.fora_whole_seeds(sets[i], EPS, A, seed=7, weights=weights[i], n_rounds=n_rounds,
                                                   tuning=orc_tuning(orc, t))
                    check_fora(out[i], pq[i], ref, sto, (graph, frac, B, n_rounds, names[i], "twin"))
            ids, vals, _ = dev.fora_batch_topk_seeds(sets, k, EPS, A, seed=9, weights=weights)
            for i, (s, w) in enumerate(zip(sets, weights)):
                nsel, sids, svals, _, _ = dev.fora_topk_seeds(s, EPS, A, k, seed=9 + i, weights=w, cap=k)
                same_topk_rows(ids[i], vals[i], sids, svals, nsel, k, (graph, frac, B, "topk", names[i]))
            for i in (1, len(sets) - 2):  # the twin's selection, up to nodes whose estimates tie within 1e-9
                ref, _ = og.fora_topk_seeds(sets[i], EPS, A, k, seed=9 + i, weights=weights[i])
                cnt, oids, _ = orc.topk(ref, k, cap=k)
                m = min(cnt, k)
                for j in range(m):
                    assert ids[i][j] == oids[j] or abs(ref[ids[i][j]] - ref[oids[j]]) <= 1e-9, \
                        (graph, frac, B, "topk twin", names[i], j)
    finally:
        dev.set_tuning(pkg.tuning_default())
    if graph != "got":
        assert sweeps > 0


# ------------------------------------------------------------------ 3. every driver gives the same queries
@pytest.mark.parametrize("env", [{"PPRHIP_BATCH_WORKSPACES": "16"}, {"PPRHIP_BATCH_WORKSPACES": "19"},
                                 {"PPRHIP_BATCH_WORKSPACES": "48"}, {"PPRHIP_BATCH_THREADS": "1"},
                                 {"PPRHIP_BATCH_THREADS": "0"},
                                 {"PPRHIP_BATCH_WORKSPACES": "16", "PPRHIP_BATCH_NO_TAIL": "1"}])
def test_driver_variants(pkg, rmat15, env, monkeypatch):
    rng = np.random.default_rng(13)
    t = pkg.tuning_batch()
    sets45 = [mixed_set(rmat15, int(rng.integers(1, 40)), 100 + j) for j in range(45)]
    sets45[7] = (np.arange(0, rmat15.n, 3, dtype=np.int32), None)
    ref_g = pkg.Graph(rmat15)
    ref_g.set_tuning(t)
    g = None
    try:
        ref = {}
        for q in (35, 45):
            s, w = [x for x, _ in sets45[:q]], [y for _, y in sets45[:q]]
            ref[q] = (ref_g.fora_batch_seeds(s, EPS, A, seed=6, weights=w, fetch=True, per_query=True),
                      ref_g.fora_batch_topk_seeds(s, 16, EPS, A, seed=8, weights=w))
        for key, v in env.items():
            monkeypatch.setenv(key, v)
        g = pkg.Graph(rmat15)
        g.set_tuning(t)
        for q in (35, 45):
            s, w = [x for x, _ in sets45[:q]], [y for _, y in sets45[:q]]
            out, _, _, _, pq, st = g.fora_batch_seeds(s, EPS, A, seed=6, weights=w, fetch=True, per_query=True)
            (out0, _, _, _, pq0, st0), (ids0, vals0, _) = ref[q]
            assert st.dense_levels == st0.dense_levels and st.class_launches[5] > 0
            for i in range(q):
                same_stats(pq0[i], pq[i], (env, q, i))
            assert np.max(np.abs(out - out0)) <= 1e-12
            ids, vals, _ = g.fora_batch_topk_seeds(s, 16, EPS, A, seed=8, weights=w)
            assert np.array_equal(ids, ids0) and np.max(np.abs(vals - vals0)) <= 1e-12
    finally:
        if g is not None:
            g.close()
        ref_g.close()


# ------------------------------------------------------------------ 4. resident store and delivery
def test_resident_store_equals_delivery(pkg, rmat12, dev_rmat12):
    names, sets, weights = batch_sets(rmat12, seed=3)
    dev_rmat12.set_tuning(pkg.tuning_batch())
    store = pkg.Results(dev_rmat12, len(sets))
    try:
        out, ids, _, nsel, _, _ = dev_rmat12.fora_batch_seeds(sets, EPS, A, seed=4, weights=weights, k=8, keep=store,
                                                              fetch=True)
        assert store.info()[1] == len(sets)
        for i in range(len(sets)):
            assert np.array_equal(store.fetch(i), out[i]), names[i]
            assert abs(store.sum(i) - out[i].sum()) <= 1e-12
        assert ids.shape == (len(sets), 8) and nsel.shape == (len(sets),)
    finally:
        store.close()
        dev_rmat12.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 5. nothing of a seeded batch stays on the handle
def test_no_state_leaks(pkg, rmat12):
    rng = np.random.default_rng(8)
    srcs = [int(x) for x in rng.integers(0, rmat12.n, size=20)]
    names, sets, weights = batch_sets(rmat12, seed=17)
    sets.append(np.arange(rmat12.n, dtype=np.int32))  # every node
    weights.append(None)
    lone, lone_w = mixed_set(rmat12, 40, 5)
    with pkg.Graph(rmat12) as fresh:
        want_lone = fresh.fora_seeds(lone, EPS, A, seed=2, weights=lone_w)[0]
    with pkg.Graph(rmat12) as g:
        g.set_tuning(pkg.tuning_batch())
        a0 = g.fora_batch_single_source(srcs, EPS, A, seed=1, fetch=True)[0]
        t0 = g.fora_batch_topk(srcs, 16, EPS, A, seed=2)
        for _ in range(2):
            g.fora_batch_seeds(sets, EPS, A, seed=3, weights=weights, k=4)
            g.fora_batch_topk_seeds(sets, 16, EPS, A, seed=4, weights=weights)
        a1 = g.fora_batch_single_source(srcs, EPS, A, seed=1, fetch=True)[0]
        t1 = g.fora_batch_topk(srcs, 16, EPS, A, seed=2)
        assert np.max(np.abs(a0 - a1)) <= 1e-12
        assert np.array_equal(t0[0], t1[0]) and np.max(np.abs(t0[1] - t1[1])) <= 1e-12
        g.set_tuning(pkg.tuning_default())
        got_lone = g.fora_seeds(lone, EPS, A, seed=2, weights=lone_w)[0]
        assert np.max(np.abs(got_lone - want_lone)) <= 1e-12


# ------------------------------------------------------------------ 6. argument checks
def test_invalid_arguments(pkg, got, dev_got):
    rng = np.random.default_rng(4)
    sets = [rng.choice(got.n, size=3, replace=False).astype(np.int32) for _ in range(10)]
    ref_set = sets[0]
    dev_got.fora_seeds(ref_set, EPS, A, seed=1)
    before = dev_got.reserve().copy()

    def rejected(call, what, code=pkg.ERR_INVALID):
        with pytest.raises(pkg.PprhipError) as e:
            call()
        assert e.value.code == code, what
        return str(e.value)

    bad_id = [s.copy() for s in sets]
    bad_id[7][1] = got.n
    bad_w = [np.ones(3) for _ in sets]
    bad_w[7][2] = -1.0
    empty = [s for s in sets]
    empty[7] = np.zeros(0, dtype=np.int32)
    for what, ss, ww in (("bad id", bad_id, None), ("negative weight", sets, bad_w), ("empty set", empty, None)):
        msg = rejected(lambda: dev_got.fora_batch_seeds(ss, EPS, A, seed=1, weights=ww), what)
        assert "set 7" in msg, (what, msg)
        msg = rejected(lambda: dev_got.fora_batch_topk_seeds(ss, 5, EPS, A, seed=1, weights=ww), what)
        assert "set 7" in msg, (what, msg)
    # offsets that do not describe sets, and q < 0, through the C call itself
    seeds = np.concatenate(sets).astype(np.int32)
    conf = pkg.conf_whole_graph(got.n, got.m, A)
    L = pkg.lib()
    st = pkg.Stats()
    for off, q in ((np.array([0, 3, 2, 6], dtype=np.uint64), 3), (np.array([1, 3, 6], dtype=np.uint64), 2),
                   (np.array([0], dtype=np.uint64), -1)):
        rc = L.pprhip_fora_batch_seeds(dev_got.h, seeds.ctypes.data_as(C.c_void_p), None, off.ctypes.data_as(C.c_void_p),
                                       q, EPS, C.byref(conf), 1, 0, None, None, 0, None, None, None, None, C.byref(st))
        assert rc == pkg.ERR_INVALID, (off, q)
        ids = np.empty((max(q, 1), 5), dtype=np.int32)
        vals = np.empty((max(q, 1), 5))
        rc = L.pprhip_fora_batch_topk_seeds(dev_got.h, seeds.ctypes.data_as(C.c_void_p), None,
                                            off.ctypes.data_as(C.c_void_p), q, 5, EPS, A, 1,
                                            ids.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), C.byref(st))
        assert rc == pkg.ERR_INVALID, (off, q)
    assert np.array_equal(dev_got.reserve(), before)  # the handle is untouched
    out, _, _, _, _, st0 = dev_got.fora_batch_seeds([], EPS, A, seed=1, fetch=True)  # q == 0: an empty call
    assert out.shape == (0, got.n) and st0.levels == 0
    with pkg.QueryStream(dev_got, EPS, A) as qs:
        rejected(lambda: dev_got.fora_batch_seeds(sets, EPS, A, seed=1), "stream open", pkg.ERR_STATE)
        rejected(lambda: dev_got.fora_batch_topk_seeds(sets, 5, EPS, A, seed=1), "stream open", pkg.ERR_STATE)
        qs.wait(qs.submit([1, 2], 3))


# ------------------------------------------------------------------ 7. memory comes back
def test_memory_given_back(pkg, rmat12, rmat15):
    names, sets, weights = batch_sets(rmat15, seed=9)
    sets.append(np.arange(0, rmat15.n, 2, dtype=np.int32))  # grows the workspaces' tables past 1 024 entries
    weights.append(None)

    def life():
        with pkg.Graph(rmat15) as g:
            g.set_tuning(pkg.tuning_batch())
            for _ in range(2):
                g.fora_batch_seeds(sets, EPS, A, seed=3, weights=weights, k=4)
                g.fora_batch_topk_seeds(sets, 8, EPS, A, seed=5, weights=weights)
            g.release(pkg.Graph.RELEASE_BATCH)
            g.fora_batch_seeds(sets[:5], EPS, A, seed=3, weights=weights[:5])

    with pkg.Graph(rmat12) as probe:
        life()
        free0, _ = probe.device_memory()
        for _ in range(3):
            life()
        free1, _ = probe.device_memory()
    assert free0 - free1 <= 64 << 20, "device memory not returned: %.1f MB" % ((free0 - free1) / 1e6)


# ------------------------------------------------------------------ 8. R-MAT 22
def test_rmat22_scale(pkg):
    host = pkg.HostCsr.rmat(22, 16, seed=1)
    sets, weights = [], []
    for j in range(20):
        for k in (32, 1000):
            s, w = mixed_set(host, k, 300 + 2 * j + (k > 32))
            sets.append(s)
            weights.append(w)
    with pkg.Graph(host) as g:
        g.set_tuning(pkg.tuning_batch())
        out, _, _, _, pq, st = g.fora_batch_seeds(sets, EPS, A, seed=5, weights=weights, fetch=True, per_query=True)
        assert st.class_launches[5] > 0 and st.class_launches[5] < st.dense_levels
        sums = out.sum(axis=1)
        assert np.max(np.abs(sums - 1.0)) <= 1e-9, float(np.max(np.abs(sums - 1.0)))
        for i in (3, 36):
            est, sts = g.fora_seeds(sets[i], EPS, A, seed=5, weights=weights[i])
            same_stats(sts, pq[i], ("rmat22", i))
            assert np.max(np.abs(est - out[i])) <= 1e-9, i
        ids, vals, _ = g.fora_batch_topk_seeds(sets[:18], 32, EPS, A, seed=7, weights=weights[:18])
        nsel, sids, svals, _, _ = g.fora_topk_seeds(sets[5], EPS, A, 32, seed=12, weights=weights[5], cap=32)
        same_topk_rows(ids[5], vals[5], sids, svals, nsel, 32, ("rmat22 topk", 5))
