"""The engine against the twin at teleport probabilities other than 0.15.

Everything else on the GPU runs at alpha = 0.15, so a kernel that read another slot's alpha, a cached alpha that
outlived its query or a (1 - alpha) dropped on one path would agree with every expected value there.  Here every path
that takes alpha - walks, forward push at every level shape and layout, FORA whole-graph (single, batched, streamed),
FORA top-k (push-ahead on and off, batched, the resumable push called round by round), backward push, All-Pair, the
power method and seed sets - is held to the twin at the tolerances and counter equalities of test_gpu_parity.py and
test_gpu_seeds_twin.py, one handle runs them all with alpha changing on every call, and FORA is held to the CPU power
method under its own bound.  The twin itself is pinned at these values by tests/test_oracle_alpha.py."""
import math

import numpy as np
import pytest

from conftest import shared_graph, to_oracle
from test_gpu_fuzz import check_fora, orc_tuning
from test_gpu_reference import fora_bound_ok, live_sources
from test_gpu_seeds_twin import kinds

pytestmark = pytest.mark.gpu

ALPHAS = [0.05, 0.2, 0.5, 0.9]
EPS = 0.5
TOL_PUSH = 1e-12
TOL_MC = 1e-9


@pytest.fixture
def dev_got(pkg, got, dev_cache):
    return shared_graph(dev_cache, pkg, "dev_got", lambda: pkg.Graph(got))


@pytest.fixture
def dev_rmat12(pkg, rmat12, dev_cache):
    return shared_graph(dev_cache, pkg, "dev_rmat12", lambda: pkg.Graph(rmat12))


@pytest.fixture
def dev_rmat15(pkg, rmat15, dev_cache):
    return shared_graph(dev_cache, pkg, "dev_rmat15", lambda: pkg.Graph(rmat15))


def shape(pkg, dev, dense_frac=None, blocks=None, base=None):
    t = base if base is not None else pkg.tuning_default()
    if dense_frac is not None:
        t.dense_frac = dense_frac
    if blocks is not None:
        t.gs_blocks = blocks
    dev.set_tuning(t)  # (the conftest patch hands it to the twin's push and top-k as well)
    return t


def same_push(dev, og, orc, s, alpha, rmax, what):
    p, r, rsum, st = dev.forward_push(s, alpha, rmax)
    po, ro, rso, sto = og.forward_push(s, alpha, rmax, orc.SYNC)
    assert np.max(np.abs(p - po)) <= TOL_PUSH, (what, "reserve", float(np.max(np.abs(p - po))))
    assert np.max(np.abs(r - ro)) <= TOL_PUSH, (what, "residue", float(np.max(np.abs(r - ro))))
    assert abs(rsum - rso) <= TOL_PUSH, what
    assert (st.levels, st.dense_levels, st.pops + st.dense_nodes, st.dead_end_pops, st.enqueues) == \
           (sto.levels, sto.dense_levels, sto.pops + sto.dense_nodes, sto.dead_end_pops, sto.enqueues), what
    return st


def same_ids(ids, oids, ref, what):
    """Identical id lists in the same order; where the twin's estimate holds two values within TOL_MC of each other
    (symmetric nodes), their order is fp64 addition order and either is accepted."""
    assert len(ids) == len(oids), (what, len(ids), len(oids))
    for i, (a, b) in enumerate(zip(ids, oids)):
        assert a == b or abs(ref[a] - ref[b]) <= TOL_MC, (what, i, a, b)


def same_topk(host, dev, og, orc, s, alpha, k, what, seed=4):
    nsel, ids, vals, est, st = dev.fora_topk(s, EPS, alpha, k, seed=seed, cap=host.n, fetch=True)
    ref, sto = og.fora_topk(s, EPS, alpha, k, seed=seed, schedule=orc.SYNC)
    assert (st.rounds, st.walks, st.levels, st.pops, st.dead_end_pops) == \
           (sto.rounds, sto.walks, sto.levels, sto.pops, sto.dead_end_pops), what
    assert np.max(np.abs(est - ref)) <= TOL_MC, (what, float(np.max(np.abs(est - ref))))
    cnt, oids, _ = orc.topk(ref, k, cap=host.n)
    assert nsel == cnt, (what, nsel, cnt)
    same_ids(list(ids), list(oids), ref, what)
    return nsel, ids, est


# ------------------------------------------------------------------ walks
@pytest.mark.parametrize("alpha", [0.01, 0.05, 0.2, 0.5, 0.9, 0.99])
def test_walks_bit_exact(pkg, orc, got, dev_got, rmat12, dev_rmat12, alpha):
    """walker_step's stop test ws * 2^-32 < alpha: terminals and step counts of every walk equal the twin's.  At 0.01
    enough walks run that some exceed 1 000 steps (and pass dead ends many times)."""
    for host, dev in ((got, dev_got), (rmat12, dev_rmat12)):
        og = to_oracle(orc, host)
        n_walks = 200000 if alpha == 0.01 and host is got else 3000
        rng = np.random.default_rng(int(alpha * 1000) + host.n)
        starts = rng.integers(0, host.n, size=n_walks).astype(np.int32)
        idx = rng.integers(0, 1 << 40, size=n_walks).astype(np.uint64)
        for nzh in (False, True):
            term, steps = dev.random_walks(starts, idx, alpha, seed=3, stream=5, no_zero_hop=nzh)
            for i in range(n_walks):
                t, st = og.random_walk(int(starts[i]), alpha, 3, 5, int(idx[i]), nzh)
                assert t == term[i] and st == steps[i], (alpha, nzh, i, (t, st), (term[i], steps[i]))
            if alpha == 0.01 and host is got:
                assert steps.max() > 1000
            if alpha == 0.99 and nzh:
                assert np.mean(steps[np.diff(host.out_rp)[starts] > 0] == 1) > 0.95


# ------------------------------------------------------------------ forward push
RMAX = {0.05: (3.7e-5, 2.9e-8), 0.2: (3.7e-5, 2.9e-8), 0.5: (3.7e-5, 2.9e-9), 0.9: (3.7e-6, 2.9e-10)}


@pytest.mark.parametrize("alpha", ALPHAS)
def test_forward_push(pkg, orc, got, dev_got, toy_graphs, rmat12, dev_rmat12, rmat15, dev_rmat15, alpha):
    """Reserve and residue to 1e-12, level counters equal: GOT, the toys, R-MAT 12 at every level shape (default,
    dense only, sparse only) with 1-, 2- and 3-block Gauss-Seidel sweeps, R-MAT 15 at the default shape."""
    og = to_oracle(orc, got)
    for s in (0, 17, 42, 99):
        for rmax in RMAX[alpha]:
            same_push(dev_got, og, orc, s, alpha, rmax, ("got", alpha, s, rmax))
    for name, host in sorted(toy_graphs.items()):
        og = to_oracle(orc, host)
        with pkg.Graph(host) as g:
            for s in range(host.n):
                for rmax in (1.3e-2, 1.3e-7):
                    same_push(g, og, orc, s, alpha, rmax, (name, alpha, s, rmax))
    og = to_oracle(orc, rmat12)
    srcs = [int(np.argmax(np.diff(rmat12.out_rp)))] + live_sources(rmat12, 2, 5)
    seen = {}
    try:
        for frac in (None, 1e-9, 1e9):
            for B in (1, 2, 3):
                shape(pkg, dev_rmat12, frac, B)
                for s in srcs:
                    for rmax in RMAX[alpha]:
                        st = same_push(dev_rmat12, og, orc, s, alpha, rmax, ("rmat12", alpha, frac, B, s, rmax))
                        seen[frac] = seen.get(frac, 0) + (st.dense_levels if frac != 1e9 else st.levels)
                        if frac == 1e9:
                            assert st.dense_levels == 0
                        if frac == 1e-9:
                            assert st.dense_levels == st.levels
    finally:
        dev_rmat12.set_tuning(pkg.tuning_default())
    assert seen[1e-9] > 0 and seen[1e9] > 0, seen
    og = to_oracle(orc, rmat15)
    for s in live_sources(rmat15, 2, 8):
        st = same_push(dev_rmat15, og, orc, s, alpha, RMAX[alpha][1], ("rmat15", alpha, s))
        assert st.levels >= 3


@pytest.mark.parametrize("layout", ["panel", "sliced"])
def test_forward_push_rmat15_layouts(pkg, orc, rmat15, layout, monkeypatch):
    """The single-query sweep over the row-panel copy of the in-CSR (PPRHIP_SWEEP1_PANELS=1) and over the sliced copy
    (PPRHIP_SLICE_IDS=1000), Jacobi and 2- and 3-block Gauss-Seidel, against the twin at three values of alpha."""
    if layout == "panel":
        monkeypatch.setenv("PPRHIP_SWEEP1_PANELS", "1")
    else:
        monkeypatch.setenv("PPRHIP_SLICE_IDS", "1000")
    og = to_oracle(orc, rmat15)
    od = np.diff(rmat15.out_rp)
    srcs = [s for s in live_sources(rmat15, 12, 41) if od[s] > 0][:2]
    g = pkg.Graph(rmat15)
    try:
        for alpha in (0.05, 0.5, 0.9):
            dense = 0
            for B in (1, 2, 3):
                t = pkg.tuning_batch()
                t.gs_blocks = B
                g.set_tuning(t)
                for s in srcs:
                    dense += same_push(g, og, orc, s, alpha, RMAX[alpha][1], (layout, alpha, B, s)).dense_levels
            assert dense > 0, alpha
    finally:
        g.close()


# ------------------------------------------------------------------ FORA whole graph
@pytest.mark.parametrize("alpha", ALPHAS)
def test_fora_whole_graph(pkg, orc, got, dev_got, rmat12, dev_rmat12, alpha):
    """n_rounds 1, 2 and auto: the cost model and the a-priori start carry (1 - alpha), so the round counts are the
    twin's; vectors under check_fora's rule."""
    for host, dev, srcs in ((got, dev_got, [0, 17, 42, 106]), (rmat12, dev_rmat12, live_sources(rmat12, 3, 5))):
        og = to_oracle(orc, host)
        for s in srcs:
            for n_rounds in (1, 2, 0):
                est, st = dev.fora_single_source(s, EPS, alpha, seed=3, n_rounds=n_rounds)
                ref, sto = og.fora_whole(s, EPS, alpha, seed=3, n_rounds=n_rounds, schedule=orc.SYNC)
                check_fora(est, st, ref, sto, (alpha, s, n_rounds))
                assert st.walks == sto.walks and st.walk_steps == sto.walk_steps, (alpha, s, n_rounds)


@pytest.mark.parametrize("threads", ["0", "1"])
def test_fora_batch_and_stream(pkg, orc, rmat12, dev_rmat12, threads, monkeypatch):
    """16 queries in flight (worker threads on and off) and the query stream: each query equals the single call at its
    alpha (rounds, levels, walks; vector to the addition order), a sample equals the twin."""
    monkeypatch.setenv("PPRHIP_BATCH_THREADS", threads)
    og = to_oracle(orc, rmat12)
    srcs = live_sources(rmat12, 16, 31)
    t = shape(pkg, dev_rmat12, base=pkg.tuning_batch())
    try:
        for alpha in ALPHAS:
            out, _, _, _, pq, _ = dev_rmat12.fora_batch_single_source(srcs, EPS, alpha, seed=6, fetch=True, per_query=True)
            singles = [dev_rmat12.fora_single_source(s, EPS, alpha, seed=6) for s in srcs]
            for i, (est, st) in enumerate(singles):
                check_fora(out[i], pq[i], est, st, (alpha, "batch", i))
                assert (pq[i].levels, pq[i].walks) == (st.levels, st.walks), (alpha, i)
            for i in (0, 9):
                ref, sto = og.fora_whole(srcs[i], EPS, alpha, seed=6, n_rounds=0, schedule=orc.SYNC,
                                         tuning=orc_tuning(orc, t))
                check_fora(out[i], pq[i], ref, sto, (alpha, "batch twin", i))
            store = pkg.Results(dev_rmat12, len(srcs))
            try:
                with pkg.QueryStream(dev_rmat12, EPS, alpha, k=0) as qs:
                    qs.wait(qs.submit(np.array(srcs[:7], dtype=np.int32), 6, keep=store, keep_first=0))
                    qs.wait(qs.submit(np.array(srcs[7:], dtype=np.int32), 6, keep=store, keep_first=7))
                for i, (est, st) in enumerate(singles):
                    assert np.max(np.abs(store.fetch(i) - out[i])) <= 1e-12, (alpha, "stream", i)
            finally:
                store.close()
    finally:
        dev_rmat12.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ FORA top-k and the resumable push
@pytest.mark.parametrize("ahead", ["1", "0"])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_fora_topk(pkg, orc, got, dev_got, rmat12, dev_rmat12, alpha, ahead, monkeypatch):
    """k = 1, 10, 50 with the push-ahead on and off (PPRHIP_TOPK_AHEAD): rounds, walks, level counters, estimate and
    selection are the twin's."""
    monkeypatch.setenv("PPRHIP_TOPK_AHEAD", ahead)
    for host, dev, srcs in ((got, dev_got, [0, 17, 42]), (rmat12, dev_rmat12, live_sources(rmat12, 2, 8))):
        og = to_oracle(orc, host)
        for s in srcs:
            for k in (1, 10, 50):
                same_topk(host, dev, og, orc, s, alpha, k, (alpha, ahead, s, k))


@pytest.mark.parametrize("alpha", ALPHAS)
def test_fora_batch_topk_and_rounds(pkg, orc, got, dev_got, rmat12, dev_rmat12, alpha):
    """pprhip_fora_batch_topk (query i with seed + i) against the twin's top-k, and pprhip_fwdpush_topk_reset /
    _round called with Fora_Topk's thresholds, round by round against the twin's resumable push."""
    for host, dev, k, srcs in ((got, dev_got, 10, [0, 17, 42, 90, 106]), (rmat12, dev_rmat12, 32,
                                                                          live_sources(rmat12, 6, 6))):
        og = to_oracle(orc, host)
        ids, vals, st = dev.fora_batch_topk(srcs, k, EPS, alpha, seed=11)
        for i, s in enumerate(srcs):
            ref, sto = og.fora_topk(s, EPS, alpha, k, seed=11 + i, schedule=orc.SYNC)
            cnt, oids, _ = orc.topk(ref, k, cap=k)
            m = min(cnt, k)
            same_ids(list(ids[i][:m]), list(oids[:m]), ref, (alpha, "batch", s))
            assert np.all(ids[i][m:] == -1)
        conf = pkg.conf_topk(host.n, host.m, k, alpha)
        for s in srcs[:3]:
            dev.topk_push_reset(s, alpha)
            tw = og.topk_push(s, alpha, orc.SYNC)
            delta, rounds = 1.0 / k, 0
            while True:
                min_rmax, rmax, _ = pkg.fora_topk_params(conf, EPS, delta)
                rsum, st = dev.topk_push_round(min_rmax, rmax)
                rs_t, st_t = tw.round(min_rmax, rmax)
                p, r = dev.reserve(), dev.residue()
                assert np.max(np.abs(p - tw.reserve)) <= TOL_PUSH and np.max(np.abs(r - tw.residue)) <= TOL_PUSH
                assert abs(rsum - rs_t) <= TOL_PUSH and st.levels == st_t.levels, (alpha, s, rounds)
                rounds += 1
                if delta <= conf.min_delta or rounds >= 5:
                    break
                delta = max(conf.min_delta, delta / 4)


# ------------------------------------------------------------------ backward push, All-Pair, power method
@pytest.mark.parametrize("alpha", ALPHAS)
def test_backward_push_and_power_method(pkg, orc, got, dev_got, rmat12, dev_rmat12, alpha):
    og = to_oracle(orc, got)
    for t in (0, 3, 17, 42):
        p, r, st = dev_got.backward_push(t, alpha, 5e-6)
        po, ro, sto = og.backward_push(t, alpha, 5e-6, orc.SYNC)
        assert np.max(np.abs(p - po)) <= TOL_PUSH and np.max(np.abs(r - ro)) <= TOL_PUSH, (alpha, t)
        assert st.levels == sto.levels
    og = to_oracle(orc, rmat12)
    hub = int(np.argmax(np.diff(rmat12.in_rp)))
    try:
        for frac in (0.01, 0.05, 1e9):
            shape(pkg, dev_rmat12, frac)
            for t in [hub] + live_sources(rmat12, 2, 12):
                p, r, st = dev_rmat12.backward_push(t, alpha, 1e-7)
                po, ro, sto = og.backward_push(t, alpha, 1e-7, orc.SYNC)
                assert st.levels == sto.levels, (alpha, frac, t)
                assert np.max(np.abs(p - po)) <= TOL_PUSH and np.max(np.abs(r - ro)) <= TOL_PUSH, (alpha, frac, t)
                if frac == 0.01 and t == hub:
                    assert st.dense_levels > 0
    finally:
        dev_rmat12.set_tuning(pkg.tuning_default())
    for host, dev in ((got, dev_got), (rmat12, dev_rmat12)):
        og = to_oracle(orc, host)
        for s in live_sources(host, 2, 19):
            for iters in (1, 2, 100):
                p, _ = dev.power_method(s, alpha, iters)
                assert np.max(np.abs(p - og.power_method(s, alpha, iters))) <= TOL_PUSH, (alpha, s, iters)


@pytest.mark.parametrize("tier", ["1", "2", "3"])
def test_all_pair_tiers(pkg, orc, rmat12, dev_rmat12, tier, monkeypatch):
    """The All-Pair index through the LDS hash tier, the dense-vector tier and the whole-vector tier
    (PPRHIP_APBS_TIER) at alpha = 0.05 and 0.5.  Thresholds and k keep away from ties: at alpha = 0.5 many
    values are exactly equal, and the twin has entries on 2e-4 itself and rows that tie at their 8th value, so there
    the k rule runs on a target range where no row ties at its 7th value."""
    monkeypatch.setenv("PPRHIP_APBS_TIER", tier)
    og = to_oracle(orc, rmat12)
    lo, hi = 100, 100 + (40 if tier == "3" else 300)
    cases = {0.05: ((1e-3, -1, hi), (2e-4, 8, hi)), 0.5: ((2.3e-4, -1, hi), (3.1e-4, 7, min(hi, 140)))}
    for alpha in (0.05, 0.5):
        for thr, k, hi in cases[alpha]:
            ix, st = dev_rmat12.all_pair_backward(alpha, thr, k, lo, hi)
            off, tg, vl = ix.arrays()
            ooff, otg, ovl = og.all_pair_backward(alpha, thr, k, lo, hi, schedule=orc.SYNC)
            assert np.array_equal(off, ooff) and np.array_equal(tg, otg), (alpha, thr, k)
            assert np.max(np.abs(vl - ovl), initial=0) <= TOL_PUSH
            assert off[-1] > 0
            ix.close()


# ------------------------------------------------------------------ seed sets
def alpha_seed_sets(host, seed):
    live, dead, zin = kinds(host)
    rng = np.random.default_rng(seed)
    s = rng.choice(live, size=min(6, live.size), replace=False)
    out = {"mixed": (np.concatenate([s, dead[:3]]).astype(np.int32), rng.uniform(0.1, 1.0, size=s.size + min(3, dead.size))),
           "all_dead": (dead[:4].astype(np.int32), np.linspace(1.0, 2.0, min(4, dead.size))),
           "D~1": (np.concatenate([live[:1], dead[:40]]).astype(np.int32), None)}
    if host.n > 1200:
        big = rng.choice(host.n, size=1300, replace=False).astype(np.int32)
        out["big"] = (big, rng.uniform(0.1, 1.0, size=big.size))
    return out


@pytest.mark.parametrize("alpha", [0.05, 0.5, 0.9])
def test_seed_sets(pkg, orc, got, dev_got, rmat12, dev_rmat12, alpha):
    """Push, FORA and top-k from seed sets with dead-end seeds (the landing closed form 1 - (1 - alpha) D), a set of
    dead ends only, and a set of more than 1 024 seeds, against orc_forward_push_seeds, orc_fora_whole_seeds and
    orc_fora_topk_seeds."""
    for name, host, dev in (("got", got, dev_got), ("rmat12", rmat12, dev_rmat12)):
        og = to_oracle(orc, host)
        for frac, B in ((None, 2), (1e-9, 3)):
            t = shape(pkg, dev, frac, B)
            try:
                for sname, (s, w) in alpha_seed_sets(host, 4).items():
                    what = (name, alpha, frac, sname)
                    for rmax in RMAX[alpha]:
                        p, r, rsum, st = dev.forward_push_seeds(s, alpha, rmax, weights=w)
                        po, ro, rso, sto = og.forward_push_seeds(s, alpha, rmax, weights=w)
                        for f in ("levels", "dense_levels", "pops", "dead_end_pops", "enqueues"):
                            assert getattr(st, f) == getattr(sto, f), (what, rmax, f)
                        assert np.max(np.abs(p - po)) <= TOL_PUSH and np.max(np.abs(r - ro)) <= TOL_PUSH, (what, rmax)
                    for n_rounds in (2, 0):
                        est, st = dev.fora_seeds(s, EPS, alpha, seed=7, weights=w, n_rounds=n_rounds)
                        ref, sto = og.fora_whole_seeds(s, EPS, alpha, seed=7, weights=w, n_rounds=n_rounds,
                                                       tuning=orc_tuning(orc, t))
                        check_fora(est, st, ref, sto, what + (n_rounds,))
                    nsel, ids, vals, est, st = dev.fora_topk_seeds(s, EPS, alpha, 10, seed=9, weights=w, cap=host.n,
                                                                   fetch=True)
                    ref, sto = og.fora_topk_seeds(s, EPS, alpha, 10, seed=9, weights=w)
                    assert st.rounds == sto.rounds, what
                    if st.walks == sto.walks:
                        assert np.max(np.abs(est - ref)) <= TOL_MC, what
                        cnt, oids, _ = orc.topk(ref, 10, cap=host.n)
                        assert nsel == cnt, what
                        same_ids(list(ids), list(oids), ref, what)
            finally:
                dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ one handle, alpha changing on every call
def history_steps(host):
    live = live_sources(host, 8, 44)
    _, dead, _ = kinds(host)
    seeds = (np.concatenate([np.array(live[:4]), dead[:2]]).astype(np.int32), None)
    return [("push", 0.9, live[0]), ("topk_rounds", 0.05, live[1]), ("fora", 0.5, live[2]), ("batch", 0.2, live[:5]),
            ("batch_topk", 0.9, live[3:8]), ("stream", 0.05, live[:6]), ("seeds", 0.5, seeds), ("seeds_topk", 0.2, seeds),
            ("backward", 0.9, live[4]), ("fora", 0.05, live[2]), ("topk", 0.5, live[5]), ("push", 0.2, live[0])]


def run_step(pkg, dev, kind, alpha, arg, host):
    """One call; returns the vectors and id lists it produced (FORA steps: the estimate and its Stats last)."""
    if kind == "push":
        p, r, _, _ = dev.forward_push(arg, alpha, 2.9e-8)
        return [p, r], []
    if kind == "topk_rounds":
        conf = pkg.conf_topk(host.n, host.m, 10, alpha)
        dev.topk_push_reset(arg, alpha)
        out, delta = [], 0.1
        for _ in range(3):
            min_rmax, rmax, _ = pkg.fora_topk_params(conf, EPS, delta)
            dev.topk_push_round(min_rmax, rmax)
            out += [dev.reserve(), dev.residue()]
            delta /= 4
        return out, []
    if kind == "fora":
        est, st = dev.fora_single_source(arg, EPS, alpha, seed=3)
        return [est, st], []
    if kind == "topk":
        nsel, ids, _, est, _ = dev.fora_topk(arg, EPS, alpha, 10, seed=4, cap=host.n, fetch=True)
        return [est], [list(ids)]
    if kind == "batch":
        out, ids, _, _, _, _ = dev.fora_batch_single_source(arg, EPS, alpha, seed=6, k=8, fetch=True)
        return list(out), [list(x) for x in ids]
    if kind == "batch_topk":
        ids, _, _ = dev.fora_batch_topk(arg, 10, EPS, alpha, seed=11)
        return [], [list(x) for x in ids]
    if kind == "stream":
        with pkg.QueryStream(dev, EPS, alpha, k=8) as qs:
            ids, _, _, _ = qs.wait(qs.submit(np.array(arg, dtype=np.int32), 5))
        return [], [list(x) for x in ids]
    if kind == "seeds":
        s, w = arg
        p, r, _, _ = dev.forward_push_seeds(s, alpha, 2.9e-8, weights=w)
        est, st = dev.fora_seeds(s, EPS, alpha, seed=7, weights=w)
        return [p, r, est, st], []
    if kind == "seeds_topk":
        s, w = arg
        nsel, ids, _, est, _ = dev.fora_topk_seeds(s, EPS, alpha, 10, seed=9, weights=w, cap=host.n, fetch=True)
        return [est], [list(ids)]
    if kind == "backward":
        p, r, _ = dev.backward_push(arg, alpha, 1e-7)
        return [p, r], []
    raise AssertionError(kind)


def twin_step(orc, og, kind, alpha, arg, host):
    """The twin's values for the deterministic steps (push, resumable push, backward, single-source FORA and top-k)."""
    if kind == "push":
        p, r, _, _ = og.forward_push(arg, alpha, 2.9e-8, orc.SYNC)
        return [p, r]
    if kind == "backward":
        p, r, _ = og.backward_push(arg, alpha, 1e-7, orc.SYNC)
        return [p, r]
    if kind == "topk_rounds":
        conf = orc_conf_topk(og, host, alpha)
        tw = og.topk_push(arg, alpha, orc.SYNC)
        out, delta = [], 0.1
        for _ in range(3):
            min_rmax, rmax, _ = orc.fora_topk_params(conf, EPS, delta)
            tw.round(min_rmax, rmax)
            out += [tw.reserve.copy(), tw.residue.copy()]
            delta /= 4
        return out
    if kind == "fora":
        return list(og.fora_whole(arg, EPS, alpha, seed=3, n_rounds=0, schedule=orc.SYNC))
    if kind == "topk":
        return [og.fora_topk(arg, EPS, alpha, 10, seed=4, schedule=orc.SYNC)[0]]
    if kind == "seeds":
        s, w = arg
        p, r, _, _ = og.forward_push_seeds(s, alpha, 2.9e-8, weights=w)
        return [p, r] + list(og.fora_whole_seeds(s, EPS, alpha, seed=7, weights=w, n_rounds=0))
    return None


def orc_conf_topk(og, host, alpha):
    return og.conf_topk(10, alpha)


def test_handle_history(pkg, orc, rmat12):
    """One R-MAT 12 handle runs forward push, the resumable top-k push, FORA, batched FORA, batched top-k, a stream,
    seed sets and backward push with alpha changing on every call: each result equals the same call on a fresh handle
    (vectors to 1e-12, id lists identical) and, where the twin computes the same thing, the twin's.  An alpha cached in
    topk_alpha, in a slot workspace or in the seed table would show."""
    og = to_oracle(orc, rmat12)
    with pkg.Graph(rmat12) as dev:
        for i, (kind, alpha, arg) in enumerate(history_steps(rmat12)):
            vecs, ids = run_step(pkg, dev, kind, alpha, arg, rmat12)
            with pkg.Graph(rmat12) as fresh:
                vecs0, ids0 = run_step(pkg, fresh, kind, alpha, arg, rmat12)
            arrays = [v for v in vecs if isinstance(v, np.ndarray)]
            for a, b in zip(arrays, [v for v in vecs0 if isinstance(v, np.ndarray)]):
                assert np.max(np.abs(a - b)) <= TOL_PUSH, (i, kind, alpha, float(np.max(np.abs(a - b))))
            assert ids == ids0, (i, kind, alpha)
            twin = twin_step(orc, og, kind, alpha, arg, rmat12)
            if twin is None:
                continue
            if kind in ("fora", "seeds"):  # the estimate under check_fora's rule, with the rounds and walks
                check_fora(vecs[-2], vecs[-1], twin[-2], twin[-1], (i, kind, alpha))
                vecs, twin = vecs[:-2], twin[:-2]
            tol = TOL_MC if kind == "topk" else TOL_PUSH
            for a, b in zip(vecs, twin):
                assert np.max(np.abs(a - b)) <= tol, (i, kind, alpha, float(np.max(np.abs(a - b))))


# ------------------------------------------------------------------ against the CPU power method
@pytest.mark.parametrize("alpha", [0.05, 0.5])
def test_fora_against_cpu_power_method(pkg, orc, got, dev_got, rmat12, dev_rmat12, alpha):
    """FORA single and batched under their (eps, delta) bound, and Fora_Topk's reported entries within eps of the CPU
    power method run until (1 - alpha)^iters < 1e-13 - the chain that does not go through the twin.  (Fora_Topk's eps/2
    rule is not a bound here: the scaled threshold of Fora_Topk.java:133 voids it, and at alpha = 0.5 on GOT source 1
    one entry misses eps/2 by 1.5 % with the twin's own, identical, estimate.)"""
    iters = int(math.ceil(math.log(1e-13) / math.log(1 - alpha)))
    for host, dev, srcs, k in ((got, dev_got, [63, 1, 5, 17], 10), (rmat12, dev_rmat12, live_sources(rmat12, 3, 3), 32)):
        og = to_oracle(orc, host)
        exact = {s: og.power_method(s, alpha, iters) for s in srcs}
        delta = 1.0 / host.n
        for s in srcs:
            est, st = dev.fora_single_source(s, EPS, alpha, seed=3)
            assert fora_bound_ok(est, exact[s], EPS, delta), (alpha, s)
        out, _, _, _, _, _ = dev.fora_batch_single_source(srcs, EPS, alpha, seed=3, fetch=True)
        for i, s in enumerate(srcs):
            assert fora_bound_ok(out[i], exact[s], EPS, delta), (alpha, "batch", s)
        for s in srcs:
            pm = exact[s]
            cnt, oids, ovals = orc.topk(pm, k, cap=host.n)
            n_sel, ids, vals, est, _ = dev.fora_topk(s, EPS, alpha, k, seed=5, cap=host.n, fetch=True)
            ref, _ = og.fora_topk(s, EPS, alpha, k, seed=5, schedule=orc.SYNC)
            assert np.max(np.abs(est - ref)) <= TOL_MC, (alpha, s)
            kk = min(cnt, k)
            kth = ovals[kk - 1]
            top = ids[:kk]
            assert np.all(np.abs(vals[:kk] - pm[top]) <= EPS * np.maximum(pm[top], kth)), (alpha, s)
