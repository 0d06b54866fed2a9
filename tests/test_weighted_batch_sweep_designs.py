"""The designs of tests/weighted_batch_sweep_designs.py held to their claims, without a device: every feature by name on
the inspector's output (both sides), the lifted weights against the library's table and the host's relationships, the
through-layout references against weighted_ref / weighted_query_ref / weighted_bwd_ref, every mutant caught by the very
queries the GPU file runs (tests/test_gpu_weighted_batch_sweep_designs.py), and no value of those queries next to a
threshold."""
import numpy as np
import pytest

import batch_sweep_designs as D
import weighted_batch_sweep_designs as WD
import weighted_bwd_batch_ref as bb
import weighted_bwd_ref as br
import weighted_query_ref as wqr
import weighted_ref as wr

TOL = 1e-12  # the project's bar for "same arithmetic, other addition order": what the GPU file holds every vector to
MARGIN = 1000 * TOL  # a mutant has to miss it by 1 000 x

_E1A, _E1B = "E1_group_of_128_single_edge_rows", "E1_group_with_short_rows_and_the_end_of_a_longer_one"
_E2A, _E2B = "E2_row_into_next_group", "E2_row_through_two_startless_groups"
_E3A, _E3B = "E3_row_starts_on_group_first_edge", "E3_row_ends_on_group_last_edge"
_E4A, _E4B = "E4_row_ends_on_chunk_last_edge_then_row_on_chunk_first_edge", "E4_row_fills_one_chunk"
_E5A, _E5B = "E5_row_crosses_one_chunk_boundary", "E5_long_row_over_a_chunk_without_row_start"
_E6, _E7, _E7S = "E6_m_not_multiple_of_chunk", "E7_row_gathers_ids_255_and_256", "E7_fewer_nodes_than_table_lines"
_A4 = "A4_tile_with_cross_and_plain_rows"
_DESIGNED = [_E1A, _E1B, _E2A, _E2B, _E3A, _E3B, _E4A, _E4B, _E5A, _E5B, _E6, _E7, _A4]  # the rows of `edges`, as in-rows
_POOL_SIDE = [_E1A, _E1B, _E2A, _E3A, _E3B, _E4A, _E5A, _E6, _E7, _A4]  # the pool's and the H rows' out-rows
_BY_LENGTH = [_E1B, _E2A, _E3A, _E3B, _E5A, _E6, _A4]  # the designed rows as out-rows, ordered by their length
_SMALL = [_E1B, _E2A, _E3A, _E3B, _E6, _E7S, _A4]
# (design, transposed) -> the features the forward side (the in-rows: k_wbat_edges) carries
FWD_CLAIMS = {("edges", False): _DESIGNED, ("edges", True): _POOL_SIDE, ("tail", False): _DESIGNED,
              ("tail", True): _POOL_SIDE, ("small", False): _SMALL}
# ... and the backward side (the out-rows: k_wbb_edges)
BWD_CLAIMS = {("edges", False): _POOL_SIDE, ("edges", True): _BY_LENGTH, ("tail", False): _POOL_SIDE,
              ("tail", True): _BY_LENGTH, ("small", False): _SMALL, ("small", True): _SMALL}

_cache = {}


def laid(pkg, name, transposed=False):
    """(host, w, forward side, backward side, in_w, out_w) of a design or its transpose, lifted once."""
    key = (name, transposed)
    if key not in _cache:
        host = WD.host_of(pkg, name, transposed)
        lift = pkg.lift_host(host)
        w = WD.weights_of(host, name, transposed)
        in_w, out_w = WD.lifted_weights(host, lift, w)
        _cache[key] = (host, w, D.inspect_forward(pkg, host, lift), D.inspect_backward(pkg, host, lift), in_w, out_w)
    return _cache[key]


def forward_runs():
    """Every forward query of the GPU file: (design, tag, keyword arguments of push_fwd_w)."""
    runs = [(name, ("source", s), dict(src=s)) for name, srcs in WD.forward_queries().items() for s in srcs]
    have = set(WD.forward_queries()["edges"])
    runs += [("edges", ("source", s), dict(src=s)) for s in WD.count_sources() if s not in have]
    runs += [("edges", ("set", i), dict(seeds=ids, sw=sw)) for i, (ids, sw) in enumerate(WD.seed_set_queries())]
    return runs


def backward_runs():
    """Every backward query of the GPU file: (design, transposed, ids, weights, rmax)."""
    return [(name, tr, ids, sw, rmax) for name, tr, targets, sets, rmax in WD.backward_queries()
            for ids, sw in [(t, None) for t in targets] + list(sets)]


_true = {}


def true_fwd(pkg, name, tag, kw):
    if (name, tag) not in _true:
        host, w, fwd, _, in_w, _ = laid(pkg, name)
        _true[(name, tag)] = WD.push_fwd_w(host, w, fwd, in_w, WD.ALPHA, WD.fora_rmax(host), **kw)
    return _true[(name, tag)]


def true_bwd(pkg, name, tr, ids, sw, rmax):
    key = (name, tr, "bwd", tuple(np.atleast_1d(ids).tolist()), rmax)
    if key not in _true:
        host, w, _, bwd, _, out_w = laid(pkg, name, tr)
        _true[key] = WD.push_bwd_w(host, w, bwd, out_w, ids, sw, WD.ALPHA, rmax)
    return _true[key]


# ------------------------------------------------------------------ 1. the designs carry their features
def _features(side):
    return {**D.edge_features(side), **D.apply_features(side)}


def test_sizes_the_gpu_file_promises(pkg):
    for key in BWD_CLAIMS:
        host = laid(pkg, *key)[0]
        assert host.n <= 1554 and host.m <= 3779, key
    assert max(len(s) for s in WD.forward_queries().values()) <= 33 and len(WD.seed_set_queries()) == 18
    assert all(len(t) + len(s) <= 33 for _, _, t, s, _ in WD.backward_queries())


@pytest.mark.parametrize("name,transposed,feature", [(n, t, f) for (n, t), fs in FWD_CLAIMS.items() for f in fs])
def test_forward_side_carries(pkg, name, transposed, feature):
    fwd = laid(pkg, name, transposed)[2]
    assert _features(fwd)[feature], (name, transposed, feature)


@pytest.mark.parametrize("name,transposed,feature", [(n, t, f) for (n, t), fs in BWD_CLAIMS.items() for f in fs])
def test_backward_side_carries(pkg, name, transposed, feature):
    bwd = laid(pkg, name, transposed)[3]
    assert _features(bwd)[feature], (name, transposed, feature)


def test_features_found(pkg):
    """What the inspector finds per design and side (A1 and A2 are about tiles that mix rows with and without edges:
    the weighted apply kernels have none)."""
    for key in BWD_CLAIMS:
        _, _, fwd, bwd, _, _ = laid(pkg, *key)
        for what, side in (("forward ", fwd), ("backward", bwd)):
            found = sorted(k.split("_")[0] + ":" + "_".join(k.split("_")[1:]) for k, v in _features(side).items()
                           if v and not k.startswith(("A1", "A2")))
            print("%s%s %s side (m %d, m %% 8 = %d, %d rows): %s" % (key[0], "^T" if key[1] else "", what, side.m,
                                                                    side.m % WD.LANE_EDGES, side.n_nz, ", ".join(found)))


def test_tail_puts_designed_rows_in_the_straddling_lane(pkg):
    """m % 8 == 3 on both sides; on the backward side the last row ends at m, and the lane whose eight edges straddle m
    holds exactly the three single-edge rows of the new nodes, which gather R7."""
    nm = WD.all_designs()["tail"].names
    for tr in (False, True):
        host, _, fwd, bwd, _, _ = laid(pkg, "tail", tr)
        assert host.m % WD.LANE_EDGES == 3 and fwd.m == bwd.m == host.m
        assert bwd.last[-1] + 1 == bwd.m and bwd.m % WD.LANE_EDGES != 0
        assert fwd.last[-1] + 1 == fwd.m
    host, _, _, bwd, _, _ = laid(pkg, "tail")
    t = WD.LANE_EDGES * (bwd.m // WD.LANE_EDGES)
    rows = bwd.row_of_edge[t:]
    assert rows.size == 3 and np.array_equal(rows, [bwd.n_nz - 3, bwd.n_nz - 2, bwd.n_nz - 1])
    assert (bwd.length[rows] == 1).all() and bwd.first[rows[0]] == t
    assert np.array_equal(bwd.new2old[bwd.rows[rows]], nm["new"])
    assert (bwd.new2old[bwd.ci[t:]] == nm["R7"]).all()
    assert nm["R7"] in [tg for n, tr, tgs, _, _ in WD.backward_queries() if (n, tr) == ("tail", False) for tg in tgs]
    # the designs reused as they are would skip that lane's path
    for name in ("edges", "small"):
        assert laid(pkg, name)[0].m % WD.LANE_EDGES == 0


def test_seed_sets_walk_the_extra_rows_in_several_trips(pkg):
    """The seed sets pass the library's parsing rules (distinct positive weights summed: weighted_query_ref.SeedTable)
    and hold what the GPU file says: 600 live seeds without in-edges (three trips of 256), 300 mixed with dead ends and
    rows with in-edges, a single member, dead ends only; the sets of 600 finish first, so the queries behind the
    sixteenth take over their columns."""
    host, w, fwd, _, in_w, _ = laid(pkg, "edges")
    deg, ind = np.diff(host.out_rp.astype(np.int64)), np.diff(host.in_rp.astype(np.int64))
    sets = WD.seed_set_queries()
    extra = []
    for ids, sw in sets:
        assert len(set(ids)) == len(ids) and min(ids) >= 0 and max(ids) < host.n and (sw is None or min(sw) > 0.0)
        t = wqr.SeedTable(host, ids, sw, WD.ALPHA)
        extra.append(int(np.count_nonzero(ind[t.live] == 0)))
    assert extra[0] == extra[1] == 600 and extra[2] == 300 and 600 > 2 * 256
    ids2 = np.array(sets[2][0])
    assert (deg[ids2] == 0).sum() == 5 and ((ind[ids2] > 0) & (deg[ids2] > 0)).sum() == 4
    assert len(sets[3][0]) == 1 and (deg[sets[17][0]] == 0).all()
    levels = [true_fwd(pkg, "edges", ("set", i), dict(seeds=ids, sw=sw))[2] for i, (ids, sw) in enumerate(sets)]
    print("levels of the 18 seed sets:", levels)
    assert levels[0] < min(levels[1:16]) and levels[1] <= min(levels[2:16]) and levels[17] == 0
    assert len(sets[16][0]) == 1  # what takes over the first column


# ------------------------------------------------------------------ 2. the lifted weights
@pytest.mark.parametrize("name,transposed", sorted(BWD_CLAIMS))
def test_lifted_weights(pkg, name, transposed):
    host, w, fwd, bwd, in_w, out_w = laid(pkg, name, transposed)
    L = fwd.lift
    assert np.unique(w).size == host.m  # every relationship its own weight
    new2old = L["new2old"].astype(np.int64)
    # out-rows: the library's table over the lifted rows is the table over the caller's rows, bit for bit
    _, ws_lift = pkg.weight_table_host(L["out_rp"], out_w)
    _, ws_host = pkg.weight_table_host(host.out_rp, w)
    assert np.array_equal(ws_lift, ws_host[new2old]) and np.array_equal(ws_host, wr.table(host, w)[1])
    hrp, lrp = host.out_rp.astype(np.int64), L["out_rp"].astype(np.int64)
    for v in range(host.n):
        o = new2old[v]
        assert np.array_equal(out_w[lrp[v]:lrp[v + 1]], w[hrp[o]:hrp[o + 1]])
    # in-rows: every lifted in-edge holds the weight of a relationship from its source to its row; per row the multiset
    src = np.repeat(np.arange(host.n, dtype=np.int64), np.diff(hrp))
    dst = host.out_ci[:host.m].astype(np.int64)
    want = sorted(zip(dst.tolist(), src.tolist(), w.tolist()))
    irow = new2old[np.repeat(np.arange(host.n, dtype=np.int64), np.diff(L["in_rp"].astype(np.int64)))]
    isrc = new2old[L["in_ci"][:host.m].astype(np.int64)]
    assert sorted(zip(irow.tolist(), isrc.tolist(), in_w.tolist())) == want
    # ... and the sides index them as the references do
    assert np.array_equal(fwd.new2old[fwd.rows[fwd.row_of_edge]], irow) and np.array_equal(fwd.new2old[fwd.ci], isrc)
    orow = new2old[np.repeat(np.arange(host.n, dtype=np.int64), np.diff(lrp))]
    assert np.array_equal(bwd.new2old[bwd.rows[bwd.row_of_edge]], orow)


def test_small_has_parallel_relationships(pkg):
    host = laid(pkg, "small")[0]
    src = np.repeat(np.arange(host.n, dtype=np.int64), np.diff(host.out_rp.astype(np.int64)))
    pairs = src * host.n + host.out_ci[:host.m].astype(np.int64)
    assert np.unique(pairs).size < host.m


# ------------------------------------------------------------------ 3. the references through the layout
def test_forward_reference_is_push_sync(pkg):
    worst, longest, dead_src = {}, {}, 0
    for name, tag, kw in forward_runs():
        host, w, _, _, _, _ = laid(pkg, name)
        rmax = WD.fora_rmax(host)
        p, r, levels, pops, _ = true_fwd(pkg, name, tag, kw)
        if tag[0] == "source":
            p0, r0, l0, n0 = wr.push_sync(host, w, kw["src"], WD.ALPHA, rmax)
        else:
            p0, r0, l0, n0 = wqr.push_sync_seeds(host, w, kw["seeds"], kw["sw"], WD.ALPHA, rmax)
        err = max(float(np.max(np.abs(p - p0))), float(np.max(np.abs(r - r0))))
        worst[name] = max(worst.get(name, 0.0), err)
        longest[name] = max(longest.get(name, 0), levels)
        assert err <= TOL and (levels, pops) == (l0, n0), (name, tag, err, levels, l0, pops, n0)
    for name in worst:
        print("forward reference against push_sync, %s: largest difference %.3e, longest push %d levels"
              % (name, worst[name], longest[name]))
    assert longest["edges"] >= 10
    assert rmax == pkg.fora_whole_params(pkg.conf_whole_graph(host.n, host.m, WD.ALPHA), WD.EPS)[0]


def test_backward_reference_is_bpush_sync(pkg):
    worst, deepest = {}, {}
    for name, tr, ids, sw, rmax in backward_runs():
        host, w, _, _, _, _ = laid(pkg, name, tr)
        p, r, levels, pops, _ = true_bwd(pkg, name, tr, ids, sw, rmax)
        p0, r0, l0, n0, _ = br.bpush_sync(host, w, ids, sw, WD.ALPHA, rmax, "pair")
        err = max(float(np.max(np.abs(p - p0))), float(np.max(np.abs(r - r0))))
        worst[(name, tr)] = max(worst.get((name, tr), 0.0), err)
        deepest[(name, tr)] = max(deepest.get((name, tr), 0), levels)
        assert err <= TOL and (levels, pops) == (l0, n0), (name, tr, ids, err, levels, l0, pops, n0)
    for (name, tr), e in worst.items():
        print("backward reference against bpush_sync, %s%s: largest difference %.3e, deepest push %d levels"
              % (name, "^T" if tr else "", e, deepest[(name, tr)]))
        assert deepest[(name, tr)] >= 3, (name, tr)  # several consecutive sweeps at BWD_RMAX


# ------------------------------------------------------------------ 4. every mutant is caught by the GPU file's queries
def _mutant_margin(pkg, mutant, direction, name, tr, only=None):
    host, w, fwd, bwd, in_w, out_w = laid(pkg, name, tr)
    best, where = 0.0, None
    if direction == "fwd":
        assert not tr
        rmax = WD.fora_rmax(host)
        for s in WD.forward_queries()[name]:
            if only is not None and s != only:
                continue
            true = true_fwd(pkg, name, ("source", s), dict(src=s))[0]
            wrong = WD.push_fwd_w(host, w, fwd, in_w, WD.ALPHA, rmax, src=s, mutant=mutant)[0]
            diff = float(np.max(np.abs(true - wrong)))
            if diff > best:
                best, where = diff, s
    else:
        for n2, t2, ids, sw, rmax in backward_runs():
            if (n2, t2) != (name, tr) or (only is not None and (np.ndim(ids) != 0 or ids != only)):
                continue
            true = true_bwd(pkg, name, tr, ids, sw, rmax)[0]
            wrong = WD.push_bwd_w(host, w, bwd, out_w, ids, sw, WD.ALPHA, rmax, mutant=mutant)[0]
            diff = float(np.max(np.abs(true - wrong)))
            if diff > best:
                best, where = diff, ids if np.ndim(ids) == 0 else "a set"
    return best, where


def test_every_mutant_is_caught(pkg):
    """Per mutant and direction: the queries the GPU file runs on its design; the largest difference of the mutant's
    reserve from the true one over them must be at least MARGIN.  No mutant is left out."""
    assert set(WD.MUTANT_CASES) == set(WD.MUTANTS)
    for m in WD.KEPT + WD.WEIGHT_MUTANTS:
        assert (m, "fwd") in WD.MUTANTS and (m, "bwd") in WD.MUTANTS
    margins = {}
    for mutant, direction in WD.MUTANTS:
        name, tr = WD.MUTANT_CASES[(mutant, direction)]
        best, where = _mutant_margin(pkg, mutant, direction, name, tr)
        margins[(mutant, direction)] = best
        print("mutant %-27s %s on %-7s: reserve off by %.3e (query %s)" % (mutant, direction, name + ("^T" if tr else ""),
                                                                           best, where))
    low = min(margins, key=margins.get)
    print("smallest mutant margin: %.3e (%s %s), required %.1e" % (margins[low], low[0], low[1], MARGIN))
    for key, best in margins.items():
        assert best >= MARGIN, (key, best)


def test_weight_mutants_bite_where_they_are_aimed(pkg):
    """A weight mutant is exposed by the query placed beside the position it misreads (and not only by another one)."""
    nm = WD.all_designs()["tail"].names
    pool = nm["pool"]
    aimed = [("weight_of_next_edge", "fwd", "edges", False, pool[199]),     # b's last edge takes the next row's weight
             ("weight_from_group_0", "fwd", "edges", False, pool[199]),     # ... group 3's edge takes group 0's
             ("weight_of_lanes_first_edge", "fwd", "edges", False, pool[29]),
             ("pad_weight_one", "fwd", "edges", False, nm["hub"]),          # internal vertex 0 holds a contribution
             ("weight_of_next_edge", "bwd", "edges", True, pool[199]),
             ("weight_from_group_0", "bwd", "edges", True, pool[700]),
             ("weight_of_lanes_first_edge", "bwd", "edges", True, pool[0]),
             ("pad_weight_one", "bwd", "edges", False, nm["hub"]),
             ("tail_lane_weights_zero", "bwd", "tail", False, nm["R7"]),    # the straddling lane's rows gather R7
             ("tail_lane_reads_on", "bwd", "tail", False, nm["R7"])]
    assert {a[0] for a in aimed} == set(WD.WEIGHT_MUTANTS) | {"tail_lane_weights_zero", "tail_lane_reads_on"}
    for mutant, direction, name, tr, q in aimed:
        best, where = _mutant_margin(pkg, mutant, direction, name, tr, only=q)
        print("aimed %-27s %s, query %d: %.3e" % (mutant, direction, q, best))
        assert where == q and best >= MARGIN, (mutant, direction, q, best)
    # the tail mutants touch nothing but the last lane: a target that does not reach R7's in-rows does not see them
    host, w, _, bwd, _, out_w = laid(pkg, "tail")
    true = true_bwd(pkg, "tail", False, nm["f"], None, WD.BWD_RMAX)[0]
    wrong = WD.push_bwd_w(host, w, bwd, out_w, nm["f"], None, WD.ALPHA, WD.BWD_RMAX, mutant="tail_lane_weights_zero")[0]
    assert np.array_equal(true, wrong)


# ------------------------------------------------------------------ 5. no value next to a threshold
def test_threshold_margins(pkg):
    """The GPU file compares levels and pops, so no query may compare a value closer to its threshold than 1e-9
    (relative), the convention of weighted_bwd_batch_ref.MARGIN: pinned for every query, through the layout and for the
    plain reference alone."""
    smallest, where = np.inf, None
    for name, tag, kw in forward_runs():
        mg = true_fwd(pkg, name, tag, kw)[4]
        assert mg >= bb.MARGIN, (name, tag, mg)
        if mg < smallest:
            smallest, where = mg, (name, "forward") + tag
    for name, tr, ids, sw, rmax in backward_runs():
        host, w, _, _, _, _ = laid(pkg, name, tr)
        mg = true_bwd(pkg, name, tr, ids, sw, rmax)[4]
        mg0 = br.bpush_sync(host, w, ids, sw, WD.ALPHA, rmax, "pair")[4]
        assert mg >= bb.MARGIN and mg0 >= bb.MARGIN, (name, tr, ids, mg, mg0)
        if min(mg, mg0) < smallest:
            smallest, where = min(mg, mg0), (name + ("^T" if tr else ""), "backward", ids if np.ndim(ids) == 0 else "set")
    print("smallest threshold margin: %.3e (%s), required %.1e" % (smallest, where, bb.MARGIN))
