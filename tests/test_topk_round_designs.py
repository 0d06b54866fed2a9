"""The designs of tests/topk_round_designs.py on the CPU: every scenario a design claims holds as a predicate over the
reference's trace, the float run equals the Fraction run entry by entry (so the device has to equal it bit for bit), the
dense size is what dense_frac gives, the plain reference equals the oracle twin's topk_push round by round, and every
wrong reference (MUTANTS) is told apart - by every design where it is about arming."""
import math
from fractions import Fraction

import numpy as np
import pytest

import topk_round_designs as T
from conftest import to_oracle
from sparse_ref import same_bits

ALL = list(T.all_designs().values())


def outcome(rs):
    """What a device run can be compared on: the vectors, the residue sum and the counters of every round."""
    return [(R.reserve, R.residue, R.rsum, R.totals()) for R in rs]


@pytest.mark.parametrize("d", ALL, ids=repr)
def test_claimed_scenarios_hold(d):
    print(T.summary(d))
    assert d.claims, d
    for f in d.claims:
        assert T.FEATURES[f](d), (d, f)
    r = T.run(d)
    assert len(r) >= 4 and sum(1 for R in r if R.below) >= 2, d
    assert all(R.armed_joins == 0 and not R.armed for R in r if not R.below), d     # a round at or above min_rmax arms nothing
    assert any(R.below and R.armed_joins > 0 for R in r), d
    assert d.n <= 2 * T.SEED_TILE + 5 and max((L.ef for R in r for L in R.trace)) < 10000, d
    assert d.keep_ids, d
    o = d.dout[d.dout > 0]
    assert np.all(o & (o - 1) == 0), d     # every out-degree a power of two


def test_every_scenario_is_claimed():
    claimed = {f for d in ALL for f in d.claims}
    assert claimed == set(T.FEATURES)
    assert {f[0] for f in T.FEATURES} == set("PASKRL")   # positions, armed once, source, parking, dropping, level shapes
    sizes = sorted(d.n for d in ALL if d.name.startswith("pos_") and not d.K)
    assert sizes == sorted(T.POSITION_SIZES) == [13, 2049, 4096, 4101]
    # every positions design has a variant whose armed round runs dense
    assert {d.name + "_dense" for d in ALL if d.name.startswith("pos_") and not d.K} == {d.name for d in ALL if d.K}


@pytest.mark.parametrize("d", ALL, ids=repr)
def test_float_run_is_exact(d):
    fl, fr = T.run(d, float), T.run(d, Fraction)
    assert len(fl) == len(fr) == len(d.rounds)
    for i, (a, b) in enumerate(zip(fl, fr)):
        for which in ("reserve", "residue"):
            x, y = getattr(a, which), getattr(b, which)
            assert x.keys() == y.keys(), (d, i, which)
            bad = [v for v in x if Fraction(x[v]) != y[v]]
            assert not bad, (d, i, which, bad[:5])
        assert Fraction(a.rsum) == b.rsum, (d, i)          # rsum is exact too
        assert (a.start, a.dropped, a.stayed, a.armed, a.armed_joins) == (b.start, b.dropped, b.stayed, b.armed, b.armed_joins)
        assert [(L.nf, L.ef, L.dead, L.enq, L.dense) for L in a.trace] == [(L.nf, L.ef, L.dead, L.enq, L.dense) for L in b.trace]


@pytest.mark.parametrize("d", [d for d in ALL if d.K], ids=repr)
def test_dense_frac_gives_the_designed_size(d):
    assert math.ceil(d.dense_frac * float(d.m)) == d.K
    assert float(d.K - 1) < d.dense_frac * float(d.m) <= float(d.K)


@pytest.mark.parametrize("d", ALL, ids=repr)
def test_reference_equals_the_twin(orc, pkg_product, d):
    """Round by round: both vectors bit for bit, the residue sum, levels, pops, enqueues (and the dense and dead-end
    counters), under the design's dense_frac with one Gauss-Seidel block."""
    ref = T.run(d)
    og = to_oracle(orc, d.host(pkg_product))
    t = orc.tuning_default()
    t.dense_frac, t.gs_blocks = d.dense_frac, 1
    orc.set_sync_tuning(t)
    try:
        tw = og.topk_push(d.start, T.ALPHA, orc.SYNC)
        for i, ((mn, rm), R) in enumerate(zip(d.rounds, ref)):
            rsum, st = tw.round(mn, rm)
            tot = R.totals()
            assert rsum == R.rsum, (d, i, rsum, R.rsum)
            assert {k: int(getattr(st, k)) for k in T.COUNTERS} == tot, (d, i, tot)
            assert same_bits(tw.reserve, R.vector("reserve", d.n)), (d, i)
            assert same_bits(tw.residue, R.vector("residue", d.n)), (d, i)
    finally:
        orc.set_sync_tuning(None)


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_every_mutant_is_caught(mutant):
    caught = [d.name for d in ALL if outcome(T.rounds(d, mutant=mutant)) != outcome(T.run(d))]
    print("%s: caught by %s" % (mutant, caught))
    assert caught, mutant


@pytest.mark.parametrize("d", ALL, ids=repr)
def test_every_design_tells_the_arming_mutants_apart(d):
    ref = T.run(d)
    pops = lambda rs: [R.totals()["pops"] + R.totals()["dense_nodes"] for R in rs]
    seen = {m: pops(T.rounds(d, mutant=m)) for m in ("no_arm", "arm_twice")}
    print("%s pops per round: %s, never armed %s, armed twice %s" % (d.name, pops(ref), seen["no_arm"], seen["arm_twice"]))
    assert any(seen[m] != pops(ref) for m in seen), d
