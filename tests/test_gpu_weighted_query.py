"""Weighted seed sets and weighted FORA top-k on the GPU (include/pprhip.h "weighted seed sets and top-k") against the
numpy reference of tests/weighted_query_ref.py: the seeded push with dead-end mass landing on p (sparse and dense
levels), weighted FORA from a seed set, the round-start collect kernel on the designed graph of
tests/weighted_query_designs.py, the top-k rounds, and the calls' life beside the unweighted ones on one handle.
Vectors within 1e-12 (same arithmetic, other addition order); level, pop and walk counters exactly."""
import ctypes as C
import math

import numpy as np
import pytest

import weighted_query_ref as wq
import weighted_ref as wr
from conftest import shared_graph
from weighted_query_designs import PUSH_TILE, TILE, collect_design, exact_eps, landing_design

ALPHA = 0.15
TOL = 1e-12
pytestmark = pytest.mark.gpu

ALL_SPARSE, ALL_DENSE = 1e9, 1e-12  # dense_frac: no level reaches it / every level does


def _deg(host):
    return np.diff(host.out_rp.astype(np.int64))


def _in_deg(host):
    return np.diff(host.in_rp.astype(np.int64))


def _rand_w(host, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, host.m)


def _graph(dev_cache, pkg, name, host, w=None, dense_frac=None, gs_blocks=None):
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


def _sets(host):
    """name -> (seeds, seed weights): live seeds only; live and dead-end seeds mixed; with a live seed that has no
    in-edges (an extra row of the dense apply); duplicates and zero weights; every seed a dead end."""
    deg, din = _deg(host), _in_deg(host)
    live, dead = np.flatnonzero(deg > 0), np.flatnonzero(deg == 0)
    zin = np.flatnonzero((deg > 0) & (din == 0))
    hub = int(np.argmax(deg))
    s = {"live": ([hub, int(live[1]), int(live[live.size // 2])], [3.0, 1.0, 2.0]),
         "mixed": ([int(live[2]), int(dead[0]), hub, int(dead[-1])], [1.0, 2.0, 2.0, 0.5]),
         "dups": ([hub, int(live[5]), hub, int(live[7]), int(dead[0]), int(live[5])], [1.0, 2.0, 1.5, 0.0, 1.0, 0.5]),
         "dead": ([int(dead[0]), int(dead[1]), int(dead[-1])], None)}
    if zin.size:
        s["zin"] = ([int(zin[0]), hub, int(dead[0]), int(zin[-1])], [2.0, 1.0, 1.0, 1.0])
    return s


def _check_push(g, host, w, seeds, sw, rmax, tag, alpha=ALPHA):
    ref_p, ref_r, levels, pops = wq.push_sync_seeds(host, w, seeds, sw, alpha, rmax)
    p, r, rsum, st = g.weighted_forward_push_seeds(seeds, alpha, rmax, weights=sw)
    assert st.levels == levels and st.pops + st.dense_nodes == pops, (tag, rmax, st.levels, levels, st.pops, pops)
    ep, er = float(np.max(np.abs(p - ref_p))), float(np.max(np.abs(r - ref_r)))
    assert ep <= TOL and er <= TOL, (tag, rmax, ep, er)
    assert abs(rsum - ref_r.sum()) <= TOL and st.rsum == rsum and st.rounds == 1 and st.rmax_final == rmax
    assert np.array_equal(g.reserve(), p) and np.array_equal(g.residue(), r)
    return p, r, st


# ---------------------------------------------------------------------------------------------- seeded push
@pytest.mark.parametrize("mode", ["default", "dense", "sparse"])
@pytest.mark.parametrize("name", ["got", "rmat12"])
def test_seeded_push_against_the_level_reference(pkg, dev_cache, got, rmat12, name, mode):
    host = got if name == "got" else rmat12
    w = _rand_w(host, 21 if name == "got" else 22)
    frac = {"default": None, "dense": ALL_DENSE, "sparse": ALL_SPARSE}[mode]
    g = _graph(dev_cache, pkg, name, host, w, dense_frac=frac)
    sets = _sets(host)
    assert "zin" in sets or name == "got"
    dense_seen = 0
    for key, (seeds, sw) in sets.items():
        for rmax in (1e-4, 1e-7):
            p, r, st = _check_push(g, host, w, seeds, sw, rmax, (name, mode, key))
            dense_seen += st.dense_levels
            if mode == "dense":
                assert st.dense_levels == st.levels
            if mode == "sparse":
                assert st.dense_levels == 0
            if key == "dead":
                assert st.levels == 0 and np.max(np.abs(p - wq.seed_p(host.n, seeds, sw))) <= 1e-16 and not r.any()
            else:
                assert not wr.active(r, _deg(host), rmax).any()
    assert dense_seen > 0 or mode == "sparse" or name == "got"


def test_a_set_of_one_seed_is_the_weighted_push(pkg, dev_cache, got, rmat12):
    for name, host, wseed in (("got", got, 21), ("rmat12", rmat12, 22)):
        w = _rand_w(host, wseed)
        deg = _deg(host)
        for frac in (None, ALL_DENSE):
            g = _graph(dev_cache, pkg, name, host, w, dense_frac=frac)
            for s in (int(np.argmax(deg)), int(np.flatnonzero(deg > 0)[3]), int(np.flatnonzero(deg == 0)[0])):
                for rmax in (1e-4, 1e-7):
                    p0, r0, rsum0, st0 = g.weighted_forward_push(s, ALPHA, rmax)
                    p1, r1, rsum1, st1 = g.weighted_forward_push_seeds([s], ALPHA, rmax, weights=[2.5])
                    assert (st1.levels, st1.pops, st1.dense_nodes, st1.dense_levels, st1.dead_end_pops) == \
                        (st0.levels, st0.pops, st0.dense_nodes, st0.dense_levels, st0.dead_end_pops), (name, s, rmax)
                    assert np.max(np.abs(p1 - p0)) <= TOL and np.max(np.abs(r1 - r0)) <= TOL and abs(rsum1 - rsum0) <= TOL


def test_dead_end_mass_lands_in_a_dense_and_in_a_sparse_level_of_one_push(pkg, dev_cache):
    host, seeds, sw, d = landing_design(pkg)
    w = _rand_w(host, 5)
    frac, rmax = 0.25, 1e-3
    thresh = math.ceil(frac * host.m)
    ref = wq.SeededPush(host, w, seeds, sw, ALPHA)
    ref.run(ref.t.live, rmax)
    dense = [nf + ef >= thresh for nf, ef, _ in ref.level_info]
    assert any(dn and x > 0 for dn, (_, _, x) in zip(dense, ref.level_info)), "no landing in a dense level"
    assert any(not dn and x > 0 for dn, (_, _, x) in zip(dense, ref.level_info)), "no landing in a sparse level"
    assert _in_deg(host)[d["B"]] == 0 and d["dz"] in ref.t.dead and d["B"] in ref.t.live
    g = _graph(dev_cache, pkg, "landing_design", host, w, dense_frac=frac)
    _, _, st = _check_push(g, host, w, seeds, sw, rmax, "landing_design")
    assert st.dense_levels == sum(dense) and 0 < st.dense_levels < st.levels
    for f in (ALL_SPARSE, ALL_DENSE):  # and with every landing in one kind of level
        g = _graph(dev_cache, pkg, "landing_design", host, w, dense_frac=f)
        for rm in (1e-3, 1e-6):
            _check_push(g, host, w, seeds, sw, rm, ("landing_design", f))


@pytest.mark.parametrize("weight", [4.0, 0.25])
def test_power_of_two_weights_are_the_unweighted_seeded_push(pkg, dev_cache, got, rmat12, weight):
    for name, host in (("got", got), ("rmat12", rmat12)):
        g = _graph(dev_cache, pkg, name, host, np.full(host.m, weight), gs_blocks=1)
        for key, (seeds, sw) in _sets(host).items():
            for rmax in (1e-4, 1e-7):
                p0, r0, rsum0, st0 = g.forward_push_seeds(seeds, ALPHA, rmax, weights=sw)
                p1, r1, rsum1, st1 = g.weighted_forward_push_seeds(seeds, ALPHA, rmax, weights=sw)
                assert np.max(np.abs(p1 - p0)) <= TOL and np.max(np.abs(r1 - r0)) <= TOL, (name, key, rmax)
                assert abs(rsum1 - rsum0) <= TOL and st1.dead_end_pops == st0.dead_end_pops


# ---------------------------------------------------------------------------------------------- FORA from a seed set
def test_fora_seeds_against_the_reference(pkg, dev_cache, got, rmat12):
    eps = 0.5
    for name, host, wseed, seed in (("got", got, 21, 3), ("rmat12", rmat12, 22, 4)):
        w = _rand_w(host, wseed)
        g = _graph(dev_cache, pkg, name, host, w)
        rmax0, omega = wr.whole_params(host.n, host.m, ALPHA, eps)
        for key, (seeds, sw) in _sets(host).items():
            ref, walks, steps = wq.fora_seeds(host, w, seeds, sw, eps, ALPHA, seed)
            est, st = g.weighted_fora_seeds(seeds, eps, ALPHA, seed, weights=sw)
            assert np.max(np.abs(est - ref)) <= TOL, (name, key)
            assert st.walks == walks and st.walk_steps == steps and st.rounds == 1, (name, key)
            assert st.rmax_final == rmax0 and st.omega == omega and np.array_equal(g.reserve(), est)
            if key == "dead":
                assert st.walks == 0 and np.max(np.abs(est - wq.seed_p(host.n, seeds, sw))) <= 1e-16
    est, st = g.weighted_fora_seeds(*_sets(rmat12)["mixed"][:1], eps, ALPHA, 4, weights=_sets(rmat12)["mixed"][1], rmax=1e-4)
    ref, walks, _ = wq.fora_seeds(rmat12, w, *_sets(rmat12)["mixed"], eps, ALPHA, 4, rmax=1e-4)
    assert st.rmax_final == 1e-4 and st.walks == walks and np.max(np.abs(est - ref)) <= TOL


# ---------------------------------------------------------------------------------------------- top-k
def _check_topk(g, host, w, seeds, sw, eps, conf, seed, tag, single=False, ref=None):
    ref = ref or wq.topk(host, w, seeds, sw, eps, conf, seed)
    if single:
        nsel, ids, vals, est, st = g.weighted_fora_topk(seeds[0], eps, conf.alpha, conf.k, seed, conf=conf, fetch=True)
    else:
        nsel, ids, vals, est, st = g.weighted_fora_topk_seeds(seeds, eps, conf.alpha, conf.k, seed, weights=sw, conf=conf,
                                                              fetch=True)
    print("%s: rounds %d (ref %d), levels %d (%d), walks %d (%d), steps %d (%d)" %
          (tag, st.rounds, ref["rounds"], st.levels, ref["levels"], st.walks, ref["walks"], st.walk_steps, ref["steps"]))
    assert st.rounds == ref["rounds"] and st.levels == ref["levels"] and st.pops + st.dense_nodes == ref["pops"], tag
    assert st.walks == ref["walks"] and st.walk_steps == ref["steps"], tag
    err = float(np.max(np.abs(est - ref["est"])))
    assert err <= TOL, (tag, err)
    assert np.max(np.abs(g.residue() - ref["residue"])) <= TOL, tag
    if ref["rounds"]:
        assert st.rmax_final == ref["rmax"] and st.omega == ref["omega"], tag
        assert abs(st.rsum - ref["residue"].sum()) <= TOL and abs(st.kth_value - ref["kth"]) <= TOL
    return ref, nsel, ids, vals, est, st


def test_collect_kernel_on_the_designed_graph(pkg, dev_cache):
    """tests/weighted_query_designs.py: collect_design - residues exactly on the round's threshold (>= decides), active
    nodes at the first and last position of a tile and of the array, a tile with none, n no multiple of the tile, a hub
    whose edges cross tiles of the push kernel."""
    host, w, d = collect_design(pkg)
    alpha = 0.5
    conf = pkg.conf_topk(host.n, host.m, 4, alpha)
    eps = exact_eps(conf, d["rmax1"])
    ref = wq.topk(host, w, [d["S"]], None, eps, conf, 5)
    # the design, on the host: internal ids, the two rounds, the second round's first frontier
    o2n = pkg.lift_host(host)["old2new"]
    assert host.n % TILE != 0 and o2n[d["G"]] == 0 and np.array_equal(o2n[3:], np.arange(3, host.n))
    assert ref["rounds"] == 2 and ref["rmax"] == d["rmax1"] and ref["round_levels"][0] == 1
    assert ref["frontier"] == [1, 1 + d["chosen"].size]
    pos = sorted(int(o2n[v]) for v in [d["G"]] + list(d["chosen"]))
    assert pos == [0, TILE - 1, 2 * TILE, 3 * TILE - 1, host.n - 1]
    assert _deg(host)[d["G"]] > 2 * PUSH_TILE and ref["level_sizes"][2] > 3000  # (joined on equality after G's pushes)
    for name, frac in (("sparse", ALL_SPARSE), ("default", None), ("dense", ALL_DENSE)):
        g = _graph(dev_cache, pkg, "collect_design", host, w, dense_frac=frac)
        _, _, _, _, _, st = _check_topk(g, host, w, [d["S"]], None, eps, conf, 5, ("collect_design", name), single=True,
                                        ref=ref)
        assert (st.dense_levels == 0) == (name == "sparse")


@pytest.mark.parametrize("graph,alpha,k", [("two_node", 0.5, 1), ("cycle5", 0.6, 2)])
def test_a_round_whose_first_frontier_is_empty(pkg, dev_cache, toy_graphs, graph, alpha, k):
    host = toy_graphs[graph]
    w = np.full(host.m, 2.0)
    conf = pkg.conf_topk(host.n, host.m, k, alpha)
    ref = wq.topk(host, w, [0], None, 0.5, conf, 3)
    assert ref["rounds"] == 2 and ref["frontier"] == [1, 0] and ref["round_levels"][1] == 0 and ref["walks_round"][1] == 1
    g = _graph(dev_cache, pkg, graph, host, w)
    _check_topk(g, host, w, [0], None, 0.5, conf, 3, graph, single=True, ref=ref)


# (graph, weight seed, seeds, seed weights, k, walk seed): the cases of tests/test_weighted_query_ref.py
TOPK_CASES = [("got", 21, [63], None, 5, 3), ("got", 21, [3, 17, 42, 90], [1.0, 2.0, 1.0, 4.0], 10, 3),
              ("rmat12", 22, [1803], None, 8, 4), ("rmat12", 22, [5, 77, 1803, 2025], None, 32, 4)]
_REF = {}


@pytest.mark.parametrize("case", range(len(TOPK_CASES)))
def test_topk_against_the_reference_and_the_ways_to_read_the_result(pkg, dev_cache, got, rmat12, case):
    name, wseed, seeds, sw, k, seed = TOPK_CASES[case]
    host = got if name == "got" else rmat12
    w = _rand_w(host, wseed)
    eps = 0.5
    conf = pkg.conf_topk(host.n, host.m, k, ALPHA)
    if case not in _REF:
        _REF[case] = wq.topk(host, w, seeds, sw, eps, conf, seed)
    g = _graph(dev_cache, pkg, name, host, w)
    ref, nsel, ids, vals, est, st = _check_topk(g, host, w, seeds, sw, eps, conf, seed, (name, seeds, k),
                                                single=len(seeds) == 1, ref=_REF[case])
    # ids: equal wherever the reference's neighbouring values are more than 1e-9 (relative) apart
    rv = ref["vals"]
    cnt = rv.size
    assert min(nsel, k) == cnt and ids.size >= cnt
    near = np.zeros(cnt, dtype=bool)
    gap = np.abs(np.diff(rv)) <= 1e-9 * rv[:-1]
    near[:-1] |= gap
    near[1:] |= gap
    if cnt == k:  # the last position against the first one left out
        rest = np.sort(ref["est"])[::-1]
        near[-1] |= rest.size > k and abs(rv[-1] - rest[k]) <= 1e-9 * rv[-1]
    assert near.sum() <= 1, (name, near.sum())
    assert np.array_equal(ids[:cnt][~near], ref["ids"][~near]) and np.max(np.abs(vals[:cnt] - rv)) <= TOL
    # reserve_out, get_reserve, topk_select and reserve_sparse read the same estimate
    assert np.array_equal(g.reserve(), est)
    n2, ids2, vals2, kth2, _ = g.topk_select(k, cap=k)
    assert n2 == nsel and np.array_equal(ids2, ids) and np.array_equal(vals2, vals)
    assert kth2 == (vals[k - 1] if cnt == k else 0.0) and st.kth_value == kth2
    sid, sval, scnt = g.reserve_sparse(0.0, "id")
    assert np.array_equal(sid, np.flatnonzero(est > 0)) and np.array_equal(sval, est[est > 0]) and scnt == sid.size


def test_topk_without_a_live_seed_is_p(pkg, dev_cache, got):
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w)
    dead = np.flatnonzero(_deg(got) == 0)
    conf = pkg.conf_topk(got.n, got.m, 5, ALPHA)
    nsel, ids, vals, est, st = g.weighted_fora_topk(int(dead[0]), 0.5, ALPHA, 5, 3, fetch=True)
    assert st.rounds == 0 and st.walks == 0 and st.levels == 0 and est[dead[0]] == 1.0 and np.count_nonzero(est) == 1
    assert nsel == 1 and ids.tolist() == [int(dead[0])] and vals.tolist() == [1.0]
    seeds, sw = [int(dead[1]), int(dead[0])], [1.0, 3.0]
    ref = wq.topk(got, w, seeds, sw, 0.5, conf, 3)
    ref, nsel, ids, vals, est, st = _check_topk(g, got, w, seeds, sw, 0.5, conf, 3, "all dead", ref=ref)
    assert st.rounds == 0 and nsel == 2 and ids.tolist() == [int(dead[0]), int(dead[1])]
    assert np.max(np.abs(est - wq.seed_p(got.n, seeds, sw))) <= 1e-16 and np.array_equal(g.reserve(), est)


def test_topk_rows_are_padded(pkg, dev_cache, got):
    """cap < k: the first cap entries, n_out says how many there are; cap > k: the unused entries are -1 / 0."""
    w = _rand_w(got, 21)
    g = _graph(dev_cache, pkg, "got", got, w)
    k = 5
    conf = pkg.conf_topk(got.n, got.m, k, ALPHA)
    nsel, ids, vals, _, _ = g.weighted_fora_topk(63, 0.5, ALPHA, k, 3, conf=conf)
    L = pkg.lib()
    for cap in (2, 9):
        i = np.full(cap, 77, dtype=np.int32)
        v = np.full(cap, 7.0)
        n_out, st = C.c_int(0), pkg.Stats()
        rc = L.pprhip_weighted_fora_topk(g.h, 63, 0.5, C.byref(conf), 3, i.ctypes.data, v.ctypes.data, cap, C.byref(n_out),
                                         None, C.byref(st))
        assert rc == 0 and n_out.value == nsel
        m = min(cap, nsel)
        assert np.array_equal(i[:m], ids[:m]) and np.array_equal(v[:m], vals[:m])
        assert (i[m:] == -1).all() and (v[m:] == 0.0).all()
    s = (C.c_int32 * 2)(63, 35)
    i = np.full(9, 77, dtype=np.int32)
    v = np.full(9, 7.0)
    n_out = C.c_int(0)
    assert L.pprhip_weighted_fora_topk_seeds(g.h, s, None, 2, 0.5, C.byref(conf), 3, i.ctypes.data, v.ctypes.data, 9,
                                             C.byref(n_out), None, None) == 0
    assert k <= n_out.value <= 9 and (i[n_out.value:] == -1).all() and (v[n_out.value:] == 0.0).all()


def test_one_round_in_isolation_draws_the_batch_walks(pkg, dev_cache, rmat12):
    """delta == min_delta: exactly one round; its walks are weighted_random_walks(starts, idx, stream 0, no forced hop)
    of the plan its residues give, and the estimate is the push reserve plus their deposits."""
    host, k, seed = rmat12, 8, 11
    w = _rand_w(host, 22)
    g = _graph(dev_cache, pkg, "rmat12", host, w)
    conf = pkg.conf_topk(host.n, host.m, k, ALPHA)
    conf.delta = conf.min_delta = 1.0 / 64
    ref = wq.topk(host, w, [1803], None, 0.5, conf, seed)
    assert ref["rounds"] == 1 and ref["walks"] > 1000
    _, _, _, _, est, st = _check_topk(g, host, w, [1803], None, 0.5, conf, seed, "one round", single=True, ref=ref)
    r = g.residue()
    nrw = float(int(st.omega * ((1.0 - ALPHA) * st.rsum)))
    v = np.flatnonzero(r > 0.0)
    x = r[v] * nrw
    oi = np.ceil(x).astype(np.int64)
    starts = np.repeat(v, oi).astype(np.int32)
    idx = (np.arange(int(oi.sum()), dtype=np.int64) - np.repeat(np.cumsum(oi) - oi, oi)).astype(np.uint64)
    assert starts.size == st.walks and np.array_equal(starts, ref["starts"][0]) and np.array_equal(idx, ref["idx"][0])
    term, steps = g.weighted_random_walks(starts, idx, ALPHA, seed, 0, False)
    rt, rs = wr.walks(host, wr.table(host, w), starts, idx, ALPHA, seed, 0, False)
    assert np.array_equal(term, rt) and np.array_equal(steps, rs) and int(steps.sum()) == st.walk_steps
    expect = ref["reserve"] + np.bincount(term, weights=np.repeat((x / oi) / nrw, oi), minlength=host.n)
    assert np.max(np.abs(est - expect)) <= TOL


# ---------------------------------------------------------------------------------------------- isolation
def test_unweighted_calls_are_untouched_by_the_new_calls(pkg, rmat12):
    deg = _deg(rmat12)
    s = int(np.argmax(deg))
    seeds = [s, int(np.flatnonzero(deg == 0)[0]), 77]

    def run(g):
        a = g.fora_topk(s, 0.5, ALPHA, 8, 5, fetch=True)
        b = g.fora_seeds(seeds, 0.5, ALPHA, 5)
        return a[1], a[2], a[3], b[0]

    with pkg.Graph(rmat12, device=0) as g:
        before = run(g)
        g.set_weights(_rand_w(rmat12, 22))
        g.weighted_fora_topk(s, 0.5, ALPHA, 8, 5)
        g.weighted_forward_push_seeds(seeds, ALPHA, 1e-5)
        between = run(g)
        g.weighted_fora_topk_seeds(seeds, 0.5, ALPHA, 8, 5)
        g.weighted_fora_seeds(seeds, 0.5, ALPHA, 5)
        after = run(g)
    for a, b, c in zip(before, between, after):
        assert np.array_equal(a, b) or np.max(np.abs(a - b)) <= TOL
        assert np.array_equal(a, c) or np.max(np.abs(a - c)) <= TOL


def test_the_new_calls_need_weights_and_check_their_sets(pkg, rmat12):
    with pkg.Graph(rmat12, device=0) as g:
        calls = [lambda: g.weighted_forward_push_seeds([0, 5], ALPHA, 1e-4), lambda: g.weighted_fora_seeds([0, 5], 0.5, ALPHA, 1),
                 lambda: g.weighted_fora_topk(0, 0.5, ALPHA, 4, 1), lambda: g.weighted_fora_topk_seeds([0, 5], 0.5, ALPHA, 4, 1)]
        ref = g.forward_push_seeds([0, 5], ALPHA, 1e-4)
        for c in calls:
            with pytest.raises(pkg.PprhipError, match="no relationship weights") as ei:
                c()
            assert ei.value.code == pkg.ERR_STATE
        again = g.forward_push_seeds([0, 5], ALPHA, 1e-4)
        assert np.max(np.abs(ref[0] - again[0])) <= TOL and np.max(np.abs(ref[1] - again[1])) <= TOL  # still usable
        g.set_weights(np.ones(rmat12.m))
        for c in calls:
            c()
        # ids and sets after the weights check, before any device work: the unweighted calls' refusals and messages
        for bad, msg in (([0, rmat12.n], "seed"), ([3, -1], "seed")):
            for call in (lambda b: g.weighted_forward_push_seeds(b, ALPHA, 1e-4), lambda b: g.weighted_fora_seeds(b, 0.5, ALPHA, 1),
                         lambda b: g.weighted_fora_topk_seeds(b, 0.5, ALPHA, 4, 1)):
                with pytest.raises(pkg.PprhipError, match=msg) as ei:
                    call(bad)
                assert ei.value.code == pkg.ERR_INVALID
        with pytest.raises(pkg.PprhipError, match="pprhip_weighted_fora_topk") as ei:
            g.weighted_fora_topk(rmat12.n, 0.5, ALPHA, 4, 1)
        assert ei.value.code == pkg.ERR_INVALID
        with pytest.raises(pkg.PprhipError, match="negative|weight") as ei:
            g.weighted_fora_topk_seeds([0, 5], 0.5, ALPHA, 4, 1, weights=[1.0, -1.0])
        assert ei.value.code == pkg.ERR_INVALID
