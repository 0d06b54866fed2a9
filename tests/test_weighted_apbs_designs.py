"""The weighted designed All-Pair searches of tests/weighted_apbs_designs.py before any of them reaches a device: on every
design and threshold the device tests use, the reference on binary64 equals the reference on fractions.Fraction entry
for entry, for every target of every queried range (no design had to be given uniform weights or left out); with all
weights 1.0 it is apbs_designed.search; the weights change the index where the helper's docstring says they do and nowhere else; the sizes the designs were built
for - nodes touched, frontier sizes, edges per level, and from them the tiers that run each search - are re-derived
from the weighted searches; and the Game-of-Thrones case of the device tests keeps every compared value away from the
threshold.

On "the weighted index differs from the unweighted one": with the exact weights (0.5, 1.5, ... on rows of degree >= 2,
2.0 on rows of degree 1) p = 1 on every row of degree 1, so fans, routing, capf and colliders - whose rows all have
degree 1 - CANNOT differ, and in `levels` every source's whole row lands on one frontier of equal contributions, so its
residue is the unweighted one.  This file asserts those equalities as what they are.  A kernel that ignored the weights
is caught by hot (dense tier, posted level), crowd_small and crowd_large (both tables and the dense tier) and by the
random weights of the Game-of-Thrones case."""
from fractions import Fraction

import numpy as np
import pytest

import apbs_designed as ad
import weighted_apbs_designs as wd
import weighted_bwd_ref as br

DIFFER = {"hot", "crowd_small", "crowd_large"}
SAME = {"fans", "routing", "capf", "colliders", "levels"}
CASES = [(name, i) for name in wd.GPU_DESIGNS for i in range(len(wd.gpu_cases(name)))]


def case_id(c):
    label, lo, hi, rmax = wd.gpu_cases(c[0])[c[1]]
    return "%s-%s-%g" % (c[0], label.replace(" ", "_"), rmax)


def same_search(A, B):
    return (A.entries == B.entries and (A.pops, A.pushes, A.frontiers, A.edges, A.touched, A.touched_after) ==
            (B.pops, B.pushes, B.frontiers, B.edges, B.touched, B.touched_after))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_float_equals_fraction_and_unit_weights_equal_unweighted(case):
    name = case[0]
    label, lo, hi, rmax = wd.gpu_cases(name)[case[1]]
    D = ad.design(name)
    G, w = D.G, wd.design_weights(name)
    runs = wd.run_w(name, lo, hi, rmax)
    ones = wd.uniform_weights(G)
    for S in runs:                                            # every target of every range the device tests query
        Q = wd.search_w(G, w, S.t, Fraction(rmax), num=Fraction)
        assert set(Q.entries) == set(S.entries), (D, label, S.t)
        assert all(Fraction(S.entries[u]) == Q.entries[u] for u in Q.entries), (D, label, S.t)
        assert (Q.pops, Q.pushes, Q.frontiers, Q.edges, Q.touched) == (S.pops, S.pushes, S.frontiers, S.edges, S.touched)
        assert (Q.ties_res, Q.ties_rsv) == (S.ties_res, S.ties_rsv)
        assert same_search(wd.search_w(G, ones, S.t, rmax), ad.search(G, S.t, rmax)), (D, label, S.t)


def test_weights_are_the_stated_ones(pkg_product):
    """Aligned with HostCsr.out_ci; W = d on every row, p = 1 on rows of degree 1."""
    for name in wd.GPU_DESIGNS:
        G, w = ad.design(name).G, wd.design_weights(name)
        host = G.host(pkg_product)
        rp = host.out_rp.astype(np.int64)
        assert np.array_equal(host.out_ci[:G.m], G.dst[np.argsort(G.src, kind="stable")])
        for u in np.flatnonzero(G.dout > 0)[:2000]:
            row = w[rp[u]:rp[u + 1]]
            assert row.sum() == (2.0 if row.size == 1 else row.size)
            assert row.size == 1 or (np.all(row[0::2] == 0.5) and np.all(row[1::2] == 1.5))
        X = wd.weighted(G, w)
        assert all(X.W[u] == (2.0 if G.dout[u] == 1 else float(G.dout[u])) for u in range(G.n) if G.dout[u])


@pytest.mark.parametrize("name", wd.GPU_DESIGNS)
def test_where_the_weights_change_the_index(name):
    D = ad.design(name)
    differ = 0
    for label, lo, hi, rmax in wd.gpu_cases(name):
        for S, B in zip(wd.run_w(name, lo, hi, rmax), ad.run(D.G, lo, hi, rmax)):
            differ += S.entries != B.entries
    print("%s: %d searches differ from their unweighted ones" % (name, differ))
    if name in DIFFER:
        assert differ > 0
    else:
        assert name in SAME and differ == 0
        if name != "levels":
            assert set(D.G.dout.tolist()) <= {0, 1}          # why: p = 1 on every edge
    if name == "levels":
        # the running sums differ all the same: the first add of a source of four or more edges is 0.25 * 0.5 / d
        t = D.targets["two128_256"]
        S = wd.search_w(D.G, wd.design_weights(name), t, ad.R_STRICT, keep=True)
        B = ad.search(D.G, t, ad.R_STRICT, keep=True)
        assert S.residue == B.residue and S.reserve == B.reserve


# ------------------------------------------------------------------ the sizes the designs sit on, from the weighted runs
def claims_of(name):
    """(label, lo, hi, rmax) -> {target: (touched, frontiers, E per level)} expected of the WEIGHTED searches."""
    D = ad.design(name)
    unweighted = {(label, lo, hi, rmax): c for label, lo, hi, rmax, c in ad.cases(D)}
    out = {}
    for label, lo, hi, rmax in wd.gpu_cases(name):
        if name.startswith("crowd"):
            pos = wd.crowd_positions(D)
            out[(label, lo, hi, rmax)] = {t: wd.crowd_claim_w(D, t, pos[t], rmax) for t in range(D.T)}
        elif name == "hot" and hi - lo > 1:
            c = D.gadgets[0].claims[rmax]
            out[(label, lo, hi, rmax)] = {t: (c if t in ad.HOT_TARGETS else (1, [], [])) for t in range(lo, hi)}
        else:
            # every other design: the topology decides which nodes cross, and every node that crossed without weights
            # still does (it ends its level on the same residue, or - hot - above rmax all the same)
            out[(label, lo, hi, rmax)] = unweighted[(label, lo, hi, rmax)]
    return out


@pytest.mark.parametrize("name", wd.GPU_DESIGNS)
def test_sizes_from_the_weighted_searches(name):
    D = ad.design(name)
    for (label, lo, hi, rmax), claims in claims_of(name).items():
        for S in wd.run_w(name, lo, hi, rmax):
            assert (S.touched, S.frontiers, S.edges) == claims[S.t], (name, label, S.t)
            assert S.pops == sum(S.frontiers) and S.pushes == sum(S.edges)


def path(name, label, mode, rmax=None):
    D = ad.design(name)
    lo, hi, rmax = [(a, b, r) for lb, a, b, r in wd.gpu_cases(name) if lb == label and rmax in (None, r)][0]
    S = wd.run_w(name, lo, hi, rmax)[0]
    return ad.tiers(S, int(D.G.din[S.t]), mode)


def test_tiers_from_the_weighted_searches():
    """The tier every edge case is meant for, stated from the weighted Search objects (nodes touched, in-degree)."""
    # fans on the give-up loads: exactly `limit` nodes stay in a table, limit + 1 are handed on
    assert path("fans", "fan384", "tables") == ["small"] and path("fans", "fan385", "tables") == ["small", "large"]
    assert path("fans", "fan1536", "tables") == ["small", "large"]
    assert path("fans", "fan1537", "tables") == ["small", "large", "dense"]
    assert path("fans", "fan1536", "large") == ["large"] and path("fans", "fan1537", "large") == ["large", "dense"]
    assert path("fans", "fan385", "default") == ["dense"] and path("fans", "fan385", "dense") == ["dense"]
    # two levels on the trips: F <= 129 stays in the small table (4 * 64 edges one below, on, one above), F >= 512 is
    # handed to the large one in level 1 and runs its level 2 (4 * 256 edges) there
    L = ad.design("levels")
    for F, E in ad.TWO_LEVELS:
        lb = "two%d_%d" % (F, E)
        for rmax in L.rmaxes:
            S = wd.run_w("levels", L.targets[lb], L.targets[lb] + 1, rmax)[0]
            assert S.frontiers[:2] == [1, F] and S.edges[:2] == [F, E]
            assert path("levels", lb, "tables", rmax) == (["small"] if F <= 129 else ["small", "large"])
            assert S.touched <= ad.LARGE_LIMIT
    assert {E for F, E in ad.TWO_LEVELS if F <= 129} == {ad.SMALL_TRIP - 1, ad.SMALL_TRIP, ad.SMALL_TRIP + 1}
    assert {E for F, E in ad.TWO_LEVELS if F >= 512} == {ad.LARGE_TRIP - 1, ad.LARGE_TRIP, ad.LARGE_TRIP + 1}
    # dense tier, chunks of 16 edges: level 2 of kDnShareMin - 1 chunks (stays), kDnShareMin (posted), and a frontier
    # above kDnStage (posted whatever its chunks)
    for (F, E), chunks in zip(ad.TWO_LEVELS_DENSE, (ad.DN_SHARE_MIN - 1, ad.DN_SHARE_MIN, 2)):
        lb = "two%d_%d" % (F, E)
        S = wd.run_w("levels", L.targets[lb], L.targets[lb] + 1, ad.R_STRICT)[0]
        assert S.frontiers[1] == F and S.edges[1] == E and -(-E // ad.DN_CHUNK_TEST) == chunks
    assert ad.TWO_LEVELS_DENSE[2][0] > ad.DN_STAGE
    # capf: the frontier the lists are sized for
    C = ad.design("capf")
    for g in C.gadgets:
        t = C.targets[g.name]
        S = wd.run_w("capf", t, t + 1, ad.R_FAN)[0]
        assert max(S.frontiers) == ad.CAPF_FRONT
    # hot: level 1 stays on its workgroup (two chunks of 16), level 2 is posted (kDnShareMin chunks); ids hot_n - 1 and
    # hot_n cross in it
    for t in ad.HOT_TARGETS:
        S = wd.search_w(ad.design("hot").G, wd.design_weights("hot"), t, ad.R_HOT, keep=True)
        assert S.edges[:2] == [20, ad.DN_SHARE_MIN * ad.DN_CHUNK_TEST] and S.frontiers[2] == len(ad.HOT_SOURCES)
        assert all(S.reserve[b] > 0 for b in ad.HOT_SOURCES)
    # crowds: more targets than workgroups; the big fans outgrow their table whether or not their sources cross
    for name, mode, limit, want in (("crowd_small", "tables", ad.SMALL_LIMIT, ["small", "large"]),
                                    ("crowd_large", "large", ad.LARGE_LIMIT, ["large", "dense"])):
        D = ad.design(name)
        r_full, r_fit = wd.crowd_rmaxes(D)
        for rmax in (r_full, r_fit):
            runs = wd.run_w(name, 0, D.T, rmax)
            big = [S for S in runs if D.kinds[S.t][0] > 5]
            assert big and all(S.touched == limit + 1 and ad.tiers(S, int(D.G.din[S.t]), mode) == want for S in big)
            assert {len(S.frontiers) for S in big} == {1, 2}  # even positions of the largest group stop after level 1
            assert all(ad.tiers(S, int(D.G.din[S.t]), mode) == want[:1] for S in runs if D.kinds[S.t][0] == 5)
        # at apbs_designed's threshold the sources of the searches that cross end on a reserve equal to rmax, which is
        # emitted (>=): more entries than the smallest record buffer holds, so some searches wait for room and run
        # again, and the device test holds pops and edge pushes to >= there
        full = wd.run_w(name, 0, D.T, r_full)
        assert sum(S.ties_rsv for S in full) > 0 and sum(len(S.entries) for S in full) > wd.RECORD_BUFFER_MIN
        # at 0.5 / (largest group's size) the same searches cross (same frontiers and edges, so the same counters), the
        # reserve 0.375 / size is below the threshold, and the entries fit a quarter of the buffer: no search is run
        # again and the device test holds (pops, edge pushes, rounds) to == in every counter mode
        fit = wd.run_w(name, 0, D.T, r_fit)
        assert [(S.frontiers, S.edges, S.touched) for S in fit] == [(S.frontiers, S.edges, S.touched) for S in full]
        assert D.T < sum(len(S.entries) for S in fit) < wd.RECORD_BUFFER_MIN // 4
        # (crowd_large's group of 128 leaves its sources 0.125 / 128 = rmax at even positions: a few hundred emitted ties)
        assert sum(S.ties_rsv for S in fit) < D.T
        for m in wd.COUNTER_MODES:
            assert ad.counters(D.G, fit, m) == ad.counters(D.G, full, m)


# ------------------------------------------------------------------ Game of Thrones, pinned
from weighted_apbs_designs import GOT_ALPHA, GOT_MARGIN, GOT_THRESHOLDS, GOT_W_SEED  # noqa: E402


def test_got_values_keep_their_distance_from_the_threshold(got):
    """weights default_rng(21).uniform(0.5, 1.5, m) in HostCsr.out_ci order: over all targets and both thresholds the
    numpy reference compares no residue (before or after a deposit) and emits or drops no reserve closer to the threshold
    than 1e-6 (relative).  The device forms c * (w / W) where the reference forms (c * w) / W - an ulp, ten orders of
    magnitude below the margin - so membership in a frontier and in the index is the same on both."""
    w = np.random.default_rng(GOT_W_SEED).uniform(0.5, 1.5, got.m)
    assert got.n == 107
    for thr in GOT_THRESHOLDS:
        m_res = m_rsv = np.inf
        for t in range(got.n):
            p, r, _, _, margin = br.bpush_sync(got, w, [t], None, GOT_ALPHA, thr, "push")
            m_res = min(m_res, margin)
            if np.any(p > 0):
                m_rsv = min(m_rsv, float(np.min(np.abs(p[p > 0] - thr) / thr)))
        print("threshold %g: residues >= %.3g, reserves >= %.3g (relative) from it" % (thr, m_res, m_rsv))
        assert m_res >= GOT_MARGIN and m_rsv >= GOT_MARGIN, (thr, m_res, m_rsv)
