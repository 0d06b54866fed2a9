"""The designs of tests/sparse_level_designs.py on the CPU: every design's float run equals its Fraction run entry by
entry (so the device has to equal it bit for bit), every feature a design claims is present in the reference's trace,
every feature is claimed, and the reference agrees with the oracle twin level for level."""
import math
from fractions import Fraction

import numpy as np
import pytest

import sparse_level_designs as D
from conftest import to_oracle

ALL = list(D.all_designs().values())


@pytest.mark.parametrize("d", ALL, ids=repr)
def test_float_run_is_exact(d):
    fl, fr = D.run(d, float), D.run(d, Fraction)
    for which in ("reserve", "residue"):
        a, b = getattr(fl, which), getattr(fr, which)
        assert a.keys() == b.keys(), (d, which)
        bad = [v for v in a if Fraction(a[v]) != b[v]]
        assert not bad, (d, which, bad[:5])
    assert [(L.nf, L.ef, L.dead, L.enq, L.dense) for L in fl.trace] == [(L.nf, L.ef, L.dead, L.enq, L.dense) for L in fr.trace]
    total = sum(fr.residue.values(), Fraction(0))
    assert Fraction(float(total)) == total          # rsum is exact too
    assert d.n <= 140000 and (d.m <= 400000 or d.name.endswith("edges_2pow20")), (d.n, d.m)
    print("%s: n %d m %d rmax %g, levels (nf, ef): %s" % (d.name, d.n, d.m, d.rmax, [(L.nf, L.ef) for L in fl.trace]))


@pytest.mark.parametrize("d", ALL, ids=repr)
def test_claimed_features_are_present(d):
    assert d.claims, d
    for f in d.claims:
        assert D.FEATURES[f](d), (d, f, [(L.nf, L.ef) for L in D.run(d).trace])


def test_every_feature_is_claimed():
    claimed = {f for d in ALL for f in d.claims}
    assert claimed == set(D.FEATURES)
    assert {f[0] for f in D.FEATURES} == set("BWGTSNCD")
    # the transposed designs put every tile, staging, crossing and table feature on the backward search as well
    assert {f for d in ALL if not d.fwd for f in d.claims} >= set(D.BWD_FEATURES)
    assert {f for d in ALL if d.fwd for f in d.claims} == set(D.FEATURES)
    # every backward out-degree that divides a value is a power of two
    for d in ALL:
        if not d.fwd:
            o = d.dout[d.dout > 0]
            assert np.all(o & (o - 1) == 0), d


def test_schedule_restates_the_two_rules():
    """The batch positions on hand-made traces: eight levels per batch; a level of 4 096 behind small ones ends the
    one-workgroup kernel and starts a batch; behind a first level of 65 536 one level more runs whatever its size."""
    def trace(sizes):
        out = []
        for s in sizes:
            L = D.Level()
            L.nf, L.ef, L.dense = 1, s - 1, False
            out.append(L)
        return out
    pos = lambda sizes: [(S.pos, S.wg_from, S.cut) for S in D.schedule(trace(sizes))]
    assert [p for p, _, _ in pos([2] * 9)] == [0, 1, 2, 3, 4, 5, 6, 7, 0]
    assert pos([2, 4095, 2]) == [(0, 0, False), (1, 0, False), (2, 0, False)]
    assert pos([2, 4096, 2]) == [(0, 0, False), (0, 1, True), (1, 1, False)]
    assert pos([65535, 5000, 2]) == [(0, 1, False), (0, 1, True), (1, 1, False)]
    assert pos([65536, 70000, 4096, 2]) == [(0, 2, False), (1, 2, False), (0, 1, True), (1, 1, False)]


@pytest.mark.parametrize("d", ALL, ids=repr)
def test_reference_agrees_with_the_twin(orc, pkg_product, d):
    """Levels, pops, dead-end pops, edge pushes, enqueues and both vectors, bit for bit, at the designs' alpha.  The
    twin's backward search has one level shape and counts no dead ends; the D designs run under their dense_frac."""
    ref = D.run(d)
    og = to_oracle(orc, d.host(pkg_product))
    tot = ref.totals()
    if d.fwd:
        t = orc.tuning_default()
        t.dense_frac, t.gs_blocks = d.dense_frac, 1
        orc.set_sync_tuning(t)
        try:
            p, r, rsum, st = og.forward_push(d.start, D.ALPHA, d.rmax, orc.SYNC)
        finally:
            orc.set_sync_tuning(None)
        assert rsum == float(sum(D.run(d, Fraction).residue.values(), Fraction(0)))
        assert st.dead_end_pops == tot["dead_end_pops"] and st.dense_levels == tot["dense_levels"]
        assert st.dense_nodes == tot["dense_nodes"]
    else:
        p, r, st = og.backward_push(d.start, D.ALPHA, d.rmax, orc.SYNC)
    assert (st.levels, st.pops, st.edge_pushes, st.enqueues) == \
        (tot["levels"], tot["pops"], tot["edge_pushes"], tot["enqueues"]), d
    assert np.array_equal(p, ref.vector("reserve", d.n)) and np.array_equal(r, ref.vector("residue", d.n)), d


@pytest.mark.parametrize("d", [d for d in ALL if d.K], ids=repr)
def test_dense_frac_gives_the_designed_size(d):
    assert math.ceil(d.dense_frac * float(d.m)) == d.K
    assert float(d.K - 1) < d.dense_frac * float(d.m) <= float(d.K)     # K - 1 runs sparse, K dense (level_cost)
