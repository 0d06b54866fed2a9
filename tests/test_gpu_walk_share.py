"""The call-scoped terminal cache of the batched whole-graph FORA paths (engine.hpp: WalkShare; DESIGN.md 2 "Terminals
shared inside a call").

Every query of a batched call walks with the call's seed, so walk (v, j) has one terminal whichever query draws it; from
32 queries per call on the first query to walk it leaves the terminal in a cell and later ones only deposit there.  The
cache changes no terminal and no increment, only the order of the fp64 additions on a vector: TOL_MC, the bar
tests/test_gpu_parity.py uses for two runs of the same walks.  The tests run on libpprhip_hooks.so: the accessors
pprhip_hook_walk_share_* and the switch PPRHIP_WALK_SHARE=0 (no cache) exist there only."""
import ctypes as C

import numpy as np
import pytest

from conftest import to_oracle

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]
ALPHA = 0.15
EPS = 0.5
TOL_SPEC = 1e-6
TOL_MC = 1e-9
Q = 40  # queries per call: above the threshold of 32


def assert_close(a, b, tol, what):
    err = float(np.max(np.abs(a - b))) if a.size else 0.0
    print("%s: max abs diff %.3e" % (what, err))
    assert err <= tol, "%s: max abs diff %.3e > %.1e" % (what, err, tol)
    assert err <= TOL_SPEC


def live_sources(host, count, seed):
    live = np.nonzero(np.diff(host.out_rp) > 0)[0]
    rng = np.random.default_rng(seed)
    return [int(x) for x in live[rng.integers(0, live.size, count)]]


def hooks(pkg):
    L = pkg.lib()
    u64p, ip = C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    L.pprhip_hook_walk_share_info.argtypes = [C.c_void_p, ip, ip, u64p, u64p, u64p]
    L.pprhip_hook_walk_share_usage.argtypes = [C.c_void_p, u64p, u64p, C.c_int]
    L.pprhip_hook_walk_share_fetch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, u64p]
    return L


def share_info(pkg, g):
    present, on, seed, cells, nbytes = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    pkg._check(hooks(pkg).pprhip_hook_walk_share_info(g.h, C.byref(present), C.byref(on), C.byref(seed), C.byref(cells),
                                                      C.byref(nbytes)))
    return dict(present=bool(present.value), on=bool(on.value), seed=seed.value, cells=cells.value, bytes=nbytes.value)


def share_usage(pkg, g, reset=True):
    s, w = C.c_uint64(), C.c_uint64()
    pkg._check(hooks(pkg).pprhip_hook_walk_share_usage(g.h, C.byref(s), C.byref(w), int(reset)))
    return s.value, w.value


def share_cells(pkg, g, node):
    cnt = C.c_uint64()
    L = hooks(pkg)
    pkg._check(L.pprhip_hook_walk_share_fetch(g.h, node, None, 0, C.byref(cnt)))
    out = np.empty(cnt.value, dtype=np.int32)
    if cnt.value:
        pkg._check(L.pprhip_hook_walk_share_fetch(g.h, node, out.ctypes.data_as(C.c_void_p), cnt.value, C.byref(cnt)))
    return out


def batch(g, srcs, seed, n_rounds=0, k=8):
    out, ids, vals, nsel, pq, st = g.fora_batch_single_source(srcs, EPS, ALPHA, seed=seed, n_rounds=n_rounds, k=k,
                                                              fetch=True, per_query=True)
    return out, ids, nsel, pq


def same_results(a, b, what):
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[1], b[1]), what + ": top-k id lists differ"
    for i in range(len(a[3])):
        assert a[3][i].walks == b[3][i].walks and a[3][i].rounds == b[3][i].rounds, (what, i)
        assert_close(a[0][i], b[0][i], TOL_MC, "%s query %d" % (what, i))


# ------------------------------------------------------------------ 1. the cells are the walks
@pytest.mark.parametrize("name", ["got", "rmat12", "rmat15"])
def test_cells_hold_the_walks_bit_exact(pkg, got, rmat12, rmat15, name):
    """Every filled cell (v, j) is the terminal of walk (seed, stream 0, v, j) with the forced first hop, as
    pprhip_random_walk_batch draws it; with one push per query (n_rounds = 1, so the residue a query plans from is the
    forward push's at the call's threshold) every node with out-edges that a query planned has its walk 0 in the cache."""
    host = {"got": got, "rmat12": rmat12, "rmat15": rmat15}[name]
    srcs = live_sources(host, Q, seed=23)
    d = np.diff(host.out_rp)
    with pkg.Graph(host) as g:
        g.set_tuning(pkg.tuning_batch())
        out, ids, nsel, pq = batch(g, srcs, seed=11, n_rounds=1)
        info = share_info(pkg, g)
        served, stored = share_usage(pkg, g)
        print("%s: cells %d bytes %d, walks %d served %d stored %d" % (name, info["cells"], info["bytes"],
                                                                       sum(x.walks for x in pq), served, stored))
        assert info["present"] and info["seed"] == 11 and not info["on"]      # the cache lives for one call
        assert served > 0 and stored > 0
        assert sum(x.walk_steps for x in pq) > 0
        planned = np.zeros(host.n, dtype=bool)
        for i in sorted(set([0, Q // 2, Q - 1])):
            _, res, _, _ = g.forward_push(srcs[i], ALPHA, pq[i].rmax_final)
            planned |= (res > 0) & (d > 0)
        filled = compared = 0
        for v in range(host.n):
            cells = share_cells(pkg, g, v)
            if d[v] == 0:
                assert cells.size == 0
                continue
            assert cells.size >= 1
            have = np.nonzero(cells >= 0)[0]
            if planned[v]:
                assert cells[0] >= 0, "node %d was planned and its walk 0 is not in the cache" % v
            if have.size == 0:
                continue
            filled += 1
            live, _ = g.random_walks(np.full(have.size, v, dtype=np.int32), have.astype(np.uint64), ALPHA, seed=11,
                                     stream=0, no_zero_hop=True)
            assert np.array_equal(cells[have], live), "node %d: cached terminals differ from random_walks" % v
            compared += have.size
        print("%s: %d nodes with cells filled, %d terminals compared, %d planned nodes" % (name, filled, compared,
                                                                                          int(planned.sum())))
        assert compared > 0 and filled >= int(planned.sum())


# ------------------------------------------------------------------ 2. the vectors are what they were
@pytest.mark.parametrize("name", ["got", "rmat12", "rmat15"])
def test_vectors_equal_the_unshared_call(pkg, orc, got, rmat12, rmat15, name, monkeypatch):
    host = {"got": got, "rmat12": rmat12, "rmat15": rmat15}[name]
    srcs = live_sources(host, Q, seed=5)
    t = pkg.tuning_batch()
    with pkg.Graph(host) as g:
        g.set_tuning(t)
        for n_rounds in (2, 0):
            monkeypatch.setenv("PPRHIP_WALK_SHARE", "0")
            off = batch(g, srcs, seed=7, n_rounds=n_rounds)
            assert share_usage(pkg, g) == (0, 0)
            monkeypatch.delenv("PPRHIP_WALK_SHARE")
            on = batch(g, srcs, seed=7, n_rounds=n_rounds)
            served, stored = share_usage(pkg, g)
            assert served > 0 and stored > 0
            same_results(on, off, "%s rounds=%d" % (name, n_rounds))
            # the cache walks less, and never more than the call without it
            assert sum(x.walk_steps for x in on[3]) < sum(x.walk_steps for x in off[3])
        if name != "rmat15":
            og = to_oracle(orc, host)
            ot = orc.tuning_default()
            for f, _ in ot._fields_:
                setattr(ot, f, getattr(t, f))
            for i in (0, Q - 1):
                ref, sto = og.fora_whole(srcs[i], EPS, ALPHA, seed=7, n_rounds=0, schedule=orc.SYNC, tuning=ot)
                assert on[3][i].walks == sto.walks
                assert_close(on[0][i], ref, TOL_MC, "%s vs twin query %d" % (name, i))
        # a call below the threshold runs without the cache: its statistics are the single query's
        small = batch(g, srcs[:19], seed=7)
        assert share_usage(pkg, g) == (0, 0)
        for i in range(19):
            assert small[3][i].walk_steps == off[3][i].walk_steps


# ------------------------------------------------------------------ 3. a change of seed
def test_seed_change_between_calls_and_in_a_stream(pkg, rmat15, monkeypatch):
    """Two calls with different seeds on one handle, and a query stream with two submissions of different seeds: each
    equals the call without the cache (terminals of the other seed left in the cells would not)."""
    srcs = live_sources(rmat15, Q, seed=31)
    with pkg.Graph(rmat15) as g:
        g.set_tuning(pkg.tuning_batch())
        monkeypatch.setenv("PPRHIP_WALK_SHARE", "0")
        off = {sd: batch(g, srcs, seed=sd) for sd in (3, 4)}
        monkeypatch.delenv("PPRHIP_WALK_SHARE")
        for sd in (3, 4, 3):
            on = batch(g, srcs, seed=sd)
            assert share_usage(pkg, g)[0] > 0 and share_info(pkg, g)["seed"] == sd
            same_results(on, off[sd], "seed %d" % sd)
        store = pkg.Results(g, 2 * Q)
        try:
            with pkg.QueryStream(g, EPS, ALPHA, k=8) as qs:
                t1 = qs.submit(np.array(srcs, dtype=np.int32), 3, keep=store, keep_first=0)
                t2 = qs.submit(np.array(srcs, dtype=np.int32), 4, keep=store, keep_first=Q)
                r1, r2 = qs.wait(t1), qs.wait(t2)
            assert share_usage(pkg, g)[0] > 0
            for (ids, vals, nsel, st), sd, first in ((r1, 3, 0), (r2, 4, Q)):
                assert np.array_equal(nsel, off[sd][2]) and np.array_equal(ids, off[sd][1])
                for i in range(Q):
                    assert_close(store.fetch(first + i), off[sd][0][i], TOL_MC, "stream seed %d query %d" % (sd, i))
        finally:
            store.close()


# ------------------------------------------------------------------ 4. no memory for the cache
def test_allocation_failure_is_soft(pkg, rmat12, monkeypatch):
    srcs = live_sources(rmat12, Q, seed=9)
    with pkg.Graph(rmat12) as g:
        g.set_tuning(pkg.tuning_batch())
        monkeypatch.setenv("PPRHIP_WALK_SHARE", "0")
        off = batch(g, srcs, seed=2)     # (builds the batch state: the next call's first allocation is the cache's)
        monkeypatch.delenv("PPRHIP_WALK_SHARE")
        assert not share_info(pkg, g)["present"]
        for nth in ("1", "2", "3"):      # the cells, the offsets, the counters
            pkg.Results(g, 1).close()    # (an allocation without the switch starts its count over)
            monkeypatch.setenv("PPRHIP_FAIL_ALLOC_AFTER", nth)
            on = batch(g, srcs, seed=2)  # PPRHIP_OK: a failure would have raised
            monkeypatch.delenv("PPRHIP_FAIL_ALLOC_AFTER")
            assert not share_info(pkg, g)["present"] and share_usage(pkg, g) == (0, 0)
            same_results(on, off, "allocation %s fails" % nth)
            for i in range(Q):
                assert on[3][i].walk_steps == off[3][i].walk_steps
        on = batch(g, srcs, seed=2)      # and the next call gets its cache
        assert share_info(pkg, g)["present"] and share_usage(pkg, g)[0] > 0
        same_results(on, off, "after the failures")
