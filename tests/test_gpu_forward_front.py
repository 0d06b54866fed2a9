"""The front end of the forward single-query calls on the GPU (csrc/forward_calls.cpp): what the shared bodies write into
the statistics and the arrays for each of the eight push and FORA calls from a live source, a dead-end source and a
seed set of dead ends; the two walk-batch calls; the order of refusals of the weighted calls on a live handle; and
the refusal of a bad top-k output row (topk_args_ok), which stands behind the handle in all four top-k calls.
The vectors themselves are checked against the references elsewhere (test_gpu_parity, test_gpu_seeds_twin,
test_gpu_weighted, test_gpu_weighted_query); here 1e-12 where two runs of one query are compared (same arithmetic, the
fp64 atomics in another order), exact otherwise."""
import numpy as np
import pytest

import weighted_query_ref as wq
import weighted_ref as wr
from conftest import shared_graph, to_oracle

ALPHA, EPS, SEED = 0.15, 0.5, 3
TOL = 1e-12
pytestmark = pytest.mark.gpu

PUSH = ["forward_push", "forward_push_seeds", "weighted_forward_push", "weighted_forward_push_seeds"]
FORA = ["fora_single_source", "fora_seeds", "weighted_fora", "weighted_fora_seeds"]
WEIGHTED_ENTRIES = ["pprhip_weighted_forward_push", "pprhip_weighted_forward_push_seeds", "pprhip_weighted_fora",
                    "pprhip_weighted_fora_seeds", "pprhip_weighted_random_walk_batch", "pprhip_weighted_fora_topk",
                    "pprhip_weighted_fora_topk_seeds"]


def _deg(host):
    return np.diff(host.out_rp.astype(np.int64))


def _rand_w(host, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, host.m)


def _hosts(got, toy_graphs):
    return {"got": got, "two_node": toy_graphs["two_node"], "cycle5": toy_graphs["cycle5"]}


def _graph(dev_cache, pkg, name, host, w):
    g = shared_graph(dev_cache, pkg, name, lambda: pkg.Graph(host, device=0))
    g.set_tuning(pkg.tuning_default())
    g.set_weights(w)
    return g


def _starts(host):
    """kind -> (source, seed set): a live start, a dead-end start, and (sets only) every seed a dead end"""
    deg = _deg(host)
    live, dead = np.flatnonzero(deg > 0), np.flatnonzero(deg == 0)
    hub = int(np.argmax(deg))
    s = {"live": (hub, [hub, int(live[-1])])}
    if dead.size:
        s["dead"] = (int(dead[0]), [int(dead[0])])
        s["dead_set"] = (None, [int(x) for x in dead[:3]])
    return s


def _weighted_dead_pops(host, w, src, seeds, alpha, rmax):
    """Dead-end pops of the weighted push from src (seeds None) or from the uniform seed set: the levels of
    weighted_ref.push_sync / weighted_query_ref.SeededPush with the frontier's dead ends counted, checked against them."""
    deg = _deg(host)
    _, W = wr.table(host, w)
    rp, dst = host.out_rp.astype(np.int64), host.out_ci[:host.m].astype(np.int64)
    reserve, residue = np.zeros(host.n), np.zeros(host.n)
    if seeds is None:
        if deg[src] == 0:
            return 0
        residue[src] = 1.0
        F = np.array([src], dtype=np.int64)
        ref = wr.push_sync(host, w, src, alpha, rmax)
    else:
        t = wq.SeedTable(host, seeds, None, alpha)
        residue[t.live], reserve[t.dead] = t.q, t.e
        F = t.live
        ref = wq.push_sync_seeds(host, w, seeds, None, alpha, rmax)
    count = 0
    while F.size:
        rc = residue[F].copy()
        residue[F] = 0.0
        reserve[F] = reserve[F] + rc * alpha
        is_dead = deg[F] == 0
        count += int(is_dead.sum())
        x = float((rc[is_dead] * (1.0 - alpha)).sum())
        old = residue.copy()
        lv = F[~is_dead]
        if lv.size:
            cnt = deg[lv]
            e = np.repeat(rp[lv], cnt) + np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            c = ((1.0 - alpha) * rc[~is_dead]) / W[lv]
            residue += np.bincount(dst[e], weights=np.repeat(c, cnt) * w[e], minlength=host.n)
        if x > 0.0 and seeds is None:
            residue[src] += x
        elif x > 0.0:
            residue[t.live] = residue[t.live] + x * t.q
            reserve[t.dead] = reserve[t.dead] + x * t.e
        F = np.flatnonzero(~wr.active(old, deg, rmax) & wr.active(residue, deg, rmax) & (residue != old))
    assert np.array_equal(reserve, ref[0]) and np.array_equal(residue, ref[1])
    return count


_REF = {}  # (graph, call, kind, rmax) -> the CPU reference's dead-end pops, computed once


def _ref_dead_pops(orc, host, w, name, call, src, seeds, rmax, rmax0):
    key = (name, call, src, tuple(seeds), rmax)
    if key not in _REF:
        og = to_oracle(orc, host)
        if call == "forward_push":
            _REF[key] = og.forward_push(src, ALPHA, rmax, orc.SYNC)[3].dead_end_pops
        elif call == "forward_push_seeds":
            _REF[key] = og.forward_push_seeds(seeds, ALPHA, rmax)[3].dead_end_pops
        elif call == "fora_single_source":
            _REF[key] = og.fora_whole(src, EPS, ALPHA, SEED, n_rounds=1, schedule=orc.SYNC)[1].dead_end_pops
        elif call == "fora_seeds":
            _REF[key] = og.fora_whole_seeds(seeds, EPS, ALPHA, SEED, n_rounds=1)[1].dead_end_pops
        else:
            _REF[key] = _weighted_dead_pops(host, w, src, None if call in ("weighted_forward_push", "weighted_fora")
                                            else seeds, ALPHA, rmax if rmax else rmax0)
    return _REF[key]


def _run(g, call, src, seeds, rmax, fetch):
    """(reserve | estimate, residue | None, Stats)"""
    start = seeds if call.endswith("_seeds") else src
    f = getattr(g, call)
    if call in PUSH:
        p, r, rsum, st = f(start, ALPHA, rmax, fetch=fetch)
        assert st.rsum == rsum
        return p, r, st
    if call.startswith("weighted"):
        est, st = f(start, EPS, ALPHA, SEED, rmax=rmax, fetch=fetch)
    else:
        est, st = f(start, EPS, ALPHA, SEED, n_rounds=1, fetch=fetch)
    return est, None, st


# ---------------------------------------------------------------------------------------------- stats and arrays per call
@pytest.mark.parametrize("call", PUSH + FORA)
@pytest.mark.parametrize("name", ["got", "two_node", "cycle5"])
def test_what_the_front_end_writes(pkg, orc, dev_cache, got, toy_graphs, name, call):
    host = _hosts(got, toy_graphs)[name]
    w = _rand_w(host, 21)
    g = _graph(dev_cache, pkg, name, host, w)
    deg = _deg(host)
    rmax0, omega = wr.whole_params(host.n, host.m, ALPHA, EPS)
    seeded, fora = call.endswith("_seeds"), call in FORA
    for kind, (src, seeds) in _starts(host).items():
        if not seeded and src is None:
            continue
        # (the unweighted FORA calls take no threshold: one round runs at rmax0)
        for rmax in ((0.0,) if fora and not call.startswith("weighted") else (1e-2, 1e-7) + ((0.0,) if fora else ())):
            tag = (name, call, kind, rmax)
            x, r, st = _run(g, call, src, seeds, rmax, True)
            assert np.array_equal(g.reserve(), x), tag
            res = g.residue()
            assert r is None or np.array_equal(res, r), tag
            live = bool((deg[seeds] > 0).any()) if seeded else deg[src] > 0
            print(tag, "rsum %.17g residue sum %.17g walks %d dead-end pops %d push_ms %.3f mc_ms %.3f" %
                  (st.rsum, res.sum(), st.walks, st.dead_end_pops, st.push_ms, st.mc_ms))
            assert st.rounds == 1, tag
            assert st.rmax_final == (rmax if rmax else rmax0), tag
            assert abs(st.rsum - res.sum() * ((1.0 - ALPHA) if fora else 1.0)) <= TOL, tag
            assert st.push_ms >= 0.0 and st.mc_ms >= 0.0, tag
            if fora:
                assert st.omega == omega, tag
            if not live:
                assert st.walks == 0 and st.levels == 0 and st.rsum == 0.0 and not res.any(), tag
                e = wq.seed_p(host.n, seeds, None) if seeded else np.bincount([src], minlength=host.n).astype(float)
                assert np.max(np.abs(x - e)) <= (1e-16 if seeded else 0.0), tag
            if not fora:
                assert st.walks == 0, tag
            assert st.dead_end_pops == _ref_dead_pops(orc, host, w, name, call, src, seeds, rmax, rmax0), tag
            # fetch=False: no arrays, and the getters read the same vectors
            x2, r2, st2 = _run(g, call, src, seeds, rmax, False)
            assert x2 is None and r2 is None, tag
            assert np.max(np.abs(g.reserve() - x)) <= TOL and np.max(np.abs(g.residue() - res)) <= TOL, tag
            assert (st2.levels, st2.dead_end_pops, st2.walks, st2.rounds) == (st.levels, st.dead_end_pops, st.walks, 1), tag


# ---------------------------------------------------------------------------------------------- walk batch
def _walk_case(host, count=8):
    rng = np.random.default_rng(7)
    starts = np.repeat(rng.integers(0, host.n, count), 2).astype(np.int32)
    idx = np.tile(np.array([0, 5], dtype=np.uint64), count)
    return starts, idx


@pytest.mark.parametrize("name", ["cycle5", "got"])
def test_walk_batches_return_original_ids_and_steps(pkg, orc, dev_cache, got, toy_graphs, name):
    host = _hosts(got, toy_graphs)[name]
    w = _rand_w(host, 21)
    g = _graph(dev_cache, pkg, name, host, w)
    starts, idx = _walk_case(host)
    for hop in (False, True):
        t0, s0 = g.random_walks(starts, idx, ALPHA, SEED, 1, hop)
        rt, rs = to_oracle(orc, host).random_walks(starts, idx, ALPHA, SEED, 1, hop)
        assert np.array_equal(t0, rt) and np.array_equal(s0, rs), (name, hop)
        t1, s1 = g.weighted_random_walks(starts, idx, ALPHA, SEED, 1, hop)
        wt, ws = wr.walks(host, wr.table(host, w), starts, idx, ALPHA, SEED, 1, hop)
        assert np.array_equal(t1, wt) and np.array_equal(s1, ws), (name, hop)
        assert t0.dtype == t1.dtype == np.int32 and s0.dtype == s1.dtype == np.uint32
        assert 0 <= t1.min() and t1.max() < host.n


def test_unit_weights_on_degree_one_rows_walk_alike(pkg, dev_cache, toy_graphs):
    host = toy_graphs["cycle5"]
    assert (_deg(host) == 1).all()
    g = _graph(dev_cache, pkg, "cycle5", host, np.ones(host.m))
    starts, idx = _walk_case(host)
    for hop in (False, True):
        t0, s0 = g.random_walks(starts, idx, ALPHA, SEED, 0, hop)
        t1, s1 = g.weighted_random_walks(starts, idx, ALPHA, SEED, 0, hop)
        assert np.array_equal(t0, t1) and np.array_equal(s0, s1), hop


@pytest.mark.parametrize("call,entry", [("random_walks", "pprhip_random_walk_batch"),
                                        ("weighted_random_walks", "pprhip_weighted_random_walk_batch")])
def test_walk_batch_edges(pkg, dev_cache, toy_graphs, call, entry):
    host = toy_graphs["cycle5"]
    g = _graph(dev_cache, pkg, "cycle5", host, np.ones(host.m))
    t, s = getattr(g, call)(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint64), ALPHA, SEED)
    assert t.size == 0 and s.size == 0
    for bad in (host.n, -1):
        with pytest.raises(pkg.PprhipError) as ei:
            getattr(g, call)([0, bad], [0, 1], ALPHA, SEED)
        assert ei.value.code == pkg.ERR_INVALID and "node id %d" % bad in str(ei.value)
        assert (entry + ":") in str(ei.value) and str(ei.value).count("pprhip_") == 1


# ---------------------------------------------------------------------------------------------- order of refusals
@pytest.mark.parametrize("entry", WEIGHTED_ENTRIES)
def test_weights_are_asked_for_before_ids_and_sets(pkg, toy_graphs, entry):
    host = toy_graphs["cycle5"]
    bad = host.n
    with pkg.Graph(host, device=0) as g:
        call = {"pprhip_weighted_forward_push": lambda: g.weighted_forward_push(bad, ALPHA, 1e-4),
                "pprhip_weighted_forward_push_seeds": lambda: g.weighted_forward_push_seeds([0, bad], ALPHA, 1e-4),
                "pprhip_weighted_fora": lambda: g.weighted_fora(bad, EPS, ALPHA, SEED),
                "pprhip_weighted_fora_seeds": lambda: g.weighted_fora_seeds([0, bad], EPS, ALPHA, SEED),
                "pprhip_weighted_random_walk_batch": lambda: g.weighted_random_walks([0, bad], [0, 1], ALPHA, SEED),
                "pprhip_weighted_fora_topk": lambda: g.weighted_fora_topk(bad, EPS, ALPHA, 2, SEED),
                "pprhip_weighted_fora_topk_seeds": lambda: g.weighted_fora_topk_seeds([0, bad], EPS, ALPHA, 2, SEED)}[entry]
        with pytest.raises(pkg.PprhipError, match="no relationship weights") as ei:
            call()
        assert ei.value.code == pkg.ERR_STATE and (entry + ":") in str(ei.value)
        g.set_weights(np.ones(host.m))
        with pytest.raises(pkg.PprhipError, match="node id %d" % bad) as ei:
            call()
        assert ei.value.code == pkg.ERR_INVALID and (entry + ":") in str(ei.value)


# ---------------------------------------------------------------------------------------------- the top-k output row
TOPK_ENTRIES = ["pprhip_fora_topk", "pprhip_fora_topk_seeds", "pprhip_weighted_fora_topk", "pprhip_weighted_fora_topk_seeds"]
BAD_ROWS = [dict(cap=-1), dict(k=0), dict(row=False)]


def _topk_raw(pkg, g, entry, n, start_ok=True, k=2, cap=4, row=True):
    """entry on the live handle through the C ABI: (rc, message); start_ok False: a node id outside the graph"""
    import ctypes as C
    conf = pkg.conf_topk(n, n, 2, ALPHA)
    conf.k = k
    seeds = (C.c_int32 * 2)(0, 1 if start_ok else n)
    start = (seeds, None, 2) if entry.endswith("_seeds") else (0 if start_ok else n,)
    ids, vals, n_out, st = (C.c_int32 * 8)(), (C.c_double * 8)(), C.c_int(0), pkg.Stats()
    rc = getattr(pkg.lib(), entry)(g.h, *start, EPS, C.byref(conf), SEED, ids if row else None, vals if row else None, cap,
                                   C.byref(n_out), None, C.byref(st))
    return rc, (pkg.lib().pprhip_last_error() or b"").decode()


@pytest.mark.parametrize("entry", TOPK_ENTRIES)
def test_a_bad_topk_row_on_a_live_handle(pkg, toy_graphs, entry):
    """k < 1, cap < 0 and a row of cap > 0 without ids / vals: PPRHIP_ERR_INVALID, "<entry>: bad arguments" and no other
    name.  Where the refusal stands: behind the handle's weights; behind the node id of a single source; in front of
    the parse of a seed set."""
    host = toy_graphs["cycle5"]
    weighted, seeded = "weighted" in entry, entry.endswith("_seeds")
    with pkg.Graph(host, device=0) as g:
        if weighted:
            for bad in BAD_ROWS:
                rc, msg = _topk_raw(pkg, g, entry, host.n, **bad)
                assert rc == pkg.ERR_STATE and "no relationship weights" in msg and msg.startswith(entry + ":"), (bad, rc, msg)
            g.set_weights(np.ones(host.m))
        rc, msg = _topk_raw(pkg, g, entry, host.n)
        assert rc == pkg.OK, (rc, msg)
        for bad in BAD_ROWS:
            rc, msg = _topk_raw(pkg, g, entry, host.n, **bad)
            assert rc == pkg.ERR_INVALID and msg == entry + ": bad arguments", (bad, rc, msg)
            rc, msg = _topk_raw(pkg, g, entry, host.n, start_ok=False, **bad)
            assert rc == pkg.ERR_INVALID and msg.startswith(entry + ":"), (bad, rc, msg)
            if seeded:
                assert msg == entry + ": bad arguments", (bad, msg)
            else:
                assert "node id %d" % host.n in msg and "bad arguments" not in msg, (bad, msg)
