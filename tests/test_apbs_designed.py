"""The designed All-Pair searches of tests/apbs_designed.py before any of them reaches a device: every design's claims
(nodes touched, frontier sizes and E per level) hold on the reference; the reference on fractions.Fraction gives what
it gives on binary64, entry for entry (the designs are exact); the reference equals the oracle's twin on offsets,
targets and values; the collider ids hash where they are said to; and every threshold tie a design promises occurs."""
from fractions import Fraction

import numpy as np
import pytest

import apbs_designed as ad
from conftest import to_oracle

CASES = [(name, i) for name in ad.DESIGNS for i in range(len(ad.cases(ad.design(name))))]


def case_id(c):
    name, i = c
    label, lo, hi, rmax, _ = ad.cases(ad.design(name))[i]
    return "%s-%s-%g" % (name, label, rmax)


@pytest.fixture(scope="module")
def twin_graph(orc, pkg_product):
    made = {}

    def get(D):
        if D.name not in made:
            made[D.name] = to_oracle(orc, D.G.host(pkg_product))
        return made[D.name]

    return get


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_design(orc, twin_graph, case):
    D = ad.design(case[0])
    label, lo, hi, rmax, claims = ad.cases(D)[case[1]]
    G = D.G
    runs = ad.run(G, lo, hi, rmax)
    # ---- the claims
    for S in runs:
        touched, frontiers, edges = claims[S.t]
        assert (S.touched, S.frontiers, S.edges) == (touched, frontiers, edges), (D, label, S.t)
        assert S.pops == sum(frontiers) and S.pushes == sum(edges)
    # ---- exactness: the same search on fractions (crowds: the first eight targets, every kind of gadget among them -
    # the others are copies on the same sources)
    for S in runs[:8] if D.name.startswith("crowd") else runs:
        Q = ad.search(G, S.t, Fraction(rmax), num=Fraction)
        assert set(Q.entries) == set(S.entries), (D, label, S.t)
        assert all(Fraction(S.entries[u]) == Q.entries[u] for u in Q.entries), (D, label, S.t)
        assert (Q.pops, Q.pushes, Q.frontiers, Q.edges, Q.touched) == (S.pops, S.pushes, S.frontiers, S.edges, S.touched)
        assert (Q.ties_res, Q.ties_rsv) == (S.ties_res, S.ties_rsv)
    # ---- the ties the design promises at this threshold
    res_ties, rsv_ties = sum(S.ties_res for S in runs), sum(S.ties_rsv for S in runs)
    print("%s %s rmax %g: %d targets, %d residue ties, %d reserve ties" % (D, label, rmax, len(runs), res_ties, rsv_ties))
    want = D.ties[rmax]
    if isinstance(want, dict):
        want = want[label]
    assert (res_ties > 0) == (want in ("residue", "both")) and (rsv_ties > 0) == (want in ("reserve", "both"))
    # ---- the twin, exactly
    off, tg, vl = ad.index_of(G, runs)
    ooff, otg, ovl = twin_graph(D).all_pair_backward(ad.ALPHA, rmax, -1, lo, hi, schedule=orc.SYNC)
    assert np.array_equal(off, ooff) and np.array_equal(tg, otg)
    assert np.array_equal(vl.view(np.uint64), ovl.view(np.uint64))


def test_sizes_sit_on_the_constants():
    """The sizes the designs are built at, against the constants of kernels_apbs.hip as restated in the helper."""
    assert (ad.SMALL_LIMIT, ad.LARGE_LIMIT) == (ad.SMALL_CAP - ad.SMALL_CAP // 4, ad.LARGE_CAP - ad.LARGE_CAP // 4)
    for limit in (ad.SMALL_LIMIT, ad.LARGE_LIMIT):
        assert {limit - 1, limit, limit + 1} <= set(ad.FAN_SIZES)
    for front in (ad.SMALL_FRONT, ad.LARGE_FRONT, ad.DN_STAGE):
        assert {front - 1, front, front + 1} <= set(ad.FAN_FRONTIERS)
    assert 2 * ad.SMALL_FRONT + 1 in ad.FAN_FRONTIERS
    for F, trip in ((128, ad.SMALL_TRIP), (129, ad.SMALL_TRIP), (512, ad.LARGE_TRIP), (1025, ad.LARGE_TRIP)):
        assert {(F, trip - 1), (F, trip), (F, trip + 1)} <= set(ad.TWO_LEVELS)
        assert 1 + F + len(ad.powers(trip + 1)) < (ad.SMALL_LIMIT if trip == ad.SMALL_TRIP else ad.LARGE_LIMIT)
    chunks = [-(-E // ad.DN_CHUNK_TEST) for _, E in ad.TWO_LEVELS_DENSE]
    assert chunks[:2] == [ad.DN_SHARE_MIN - 1, ad.DN_SHARE_MIN] and ad.TWO_LEVELS_DENSE[2][0] > ad.DN_STAGE
    assert {ad.DEG_BIG - 1, ad.DEG_BIG, ad.DEG_DENSE - 1, ad.DEG_DENSE, ad.DEG_DENSE + 1, 0, 1} <= set(ad.ROUTING_DEGREES)
    assert sorted(d for d, _ in ad.ROUTING_DEEP.values()) == [ad.DEG_BIG - 1, ad.DEG_BIG, ad.DEG_DENSE - 1, ad.DEG_DENSE]
    # the in-degree-0 targets of the routing design sit among the others in every wave of k_apbs_split
    D = ad.design("routing")
    din = D.G.din[:ad.ROUTING_TARGETS]
    for w in range(0, ad.ROUTING_TARGETS, 64):
        assert 0 < int((din[w:w + 64] == 0).sum()) < din[w:w + 64].size
    assert ad.ROUTING_TARGETS > 256                                            # more than one workgroup of the split
    # crowds: more targets in the kernel's list than its largest grid
    assert ad.design("crowd_small").T > 8 * ad.MAX_CUS and ad.design("crowd_large").T > 2 * ad.MAX_CUS
    assert max(ad.design(n).G.m for n in ad.DESIGNS) <= 1_000_000
    # ... and fewer entries than the smallest record buffer of a call (65 536): no search waits for room and runs again
    for name in ("crowd_small", "crowd_large"):
        C = ad.design(name)
        entries = sum(len(S.entries) for S in ad.run(C.G, 0, C.T, C.rmaxes[0]))
        assert C.T < entries < 65536 // 4
    # a two_level's level 2 really holds parallel edges and entries of in-degree 0
    L = ad.design("levels")
    t = L.targets["two129_256"]
    a = L.G.innbrs(t)
    assert len(a) == 129 and sorted(int(L.G.din[x]) for x in a)[:3] == [0, 0, 0]
    assert any(len(set(L.G.innbrs(x))) < int(L.G.din[x]) for x in a)


def test_collider_hash():
    """The Python restatement of ap_slot's hash against two values worked out by hand, and the chains it is used for."""
    # u = 1: 2654435761 >> 7 = 20737779 = 40503 * 512 + 243 = 10125 * 2048 + 1779
    assert ad.slot(1, 512) == 243 and ad.slot(1, 2048) == 1779
    # u = 2: 2 * 2654435761 mod 2^32 = 1013904226; >> 7 = 7921126 = 15470 * 512 + 486
    assert ad.slot(2, 512) == 486
    D = ad.design("colliders")
    for cap, t in ((ad.LARGE_CAP, 0), (ad.SMALL_CAP, 1)):
        ids = D.ids[cap]
        assert len(ids) == ad.COLLIDER_COUNT and sorted(D.G.innbrs(t)) == sorted(ids)
        assert all(ad.slot(u, cap) in (cap - 2, cap - 1) for u in ids)
        assert {ad.slot(u, cap) for u in ids} == {cap - 2, cap - 1}
        used = ad.probe_occupancy([t] + ids, cap)
        # the chain runs from slot cap - 2 over cap - 1 to 0 and on: all of the table's end and its first slots are full
        assert {cap - 2, cap - 1} | set(range(ad.COLLIDER_COUNT - 2)) <= used
        # the large table's target is node 0, whose home is slot 0: the wrapped chain steps over it; the small table's
        # is node 1 (home 243), so there the chain wraps into an empty slot 0
        assert ad.slot(t, cap) == (0 if t == 0 else 243) and 0 in used
    assert not set(D.ids[ad.LARGE_CAP]) & set(D.ids[ad.SMALL_CAP])


def test_counters_of_a_search_run_twice():
    """counters(): what the kernels count when a table hands a search on - the worked figures of a fan of 385 (1 pop
    and 384 edges in the small table, all of it again in the large one) and of 1537."""
    D = ad.design("fans")
    for N, mode, want in ((384, "tables", (384, 383, 0)), (385, "tables", (1 + 385, 2 * 384, 0)),
                          (1536, "tables", (1 + 1536, 2 * 1535, 0)), (1537, "tables", (2 + 1537, 3 * 1536, 1)),
                          (1537, "large", (1 + 1537, 2 * 1536, 1)), (1537, "default", (1537, 1536, 1)),
                          (385, "dense", (385, 384, 1))):
        t = D.targets["fan%d" % N]
        assert ad.counters(D.G, ad.run(D.G, t, t + 1, ad.R_FAN), mode) == want, (N, mode)
