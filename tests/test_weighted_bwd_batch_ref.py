"""The host model of the batched weighted target call (tests/weighted_bwd_batch_ref.py) pinned on the CPU: the sweep
counts of the lockstep rounds on R-MAT 12, the round rule on hand-made level sequences, and the margin of every input
the GPU tests (tests/test_gpu_weighted_targets_batch.py) compare decisions on."""
import numpy as np
import pytest

import weighted_bwd_batch_ref as bb
from test_gpu_weighted_backward import _rmat_targets
from weighted_bwd_designs import design_weights, reversed_dense_design

ALPHA = 0.15
D, S = True, False


def rmat12_case(host):
    return np.random.default_rng(22).uniform(0.5, 1.5, host.m), _rmat_targets(host)


def design_targets(d):
    return [d["pool"][0], d["pool"][511], d["pool"][512], d["pool"][1099], d["A"], d["B"], d["C"], d["Z"], d["small"][3],
            d["isolated"]]


def test_round_rule_on_hand_made_sequences():
    # one column: every dense level is a sweep of its own
    assert bb.lockstep([[D, S, D], [D]], 1) == (3, 4, 3)
    # two columns: the dense column waits while the other runs its sparse levels, then both share the sweeps
    assert bb.lockstep([[D, D], [S, S, D, D]], 2) == (2, 4, 4)
    assert bb.eager_sweeps([[D, D], [S, S, D, D]], 2) == 4
    # a query without levels finishes at once and its column takes the next one in the same round
    assert bb.lockstep([[], [], [D], [S]], 2) == (1, 2, 1)
    # a refill: the third query begins when the first has finished, and the second waits for its sparse level
    assert bb.lockstep([[D], [D, D], [S, D]], 2) == (2, 3, 4)
    # all sparse: no sweep; rounds = the longest query
    assert bb.lockstep([[S, S, S], [S]], 16) == (0, 3, 0)
    assert bb.lockstep([], 4) == (0, 0, 0)
    # the rounds never exceed the levels the queries run one after another
    rng = np.random.default_rng(1)
    for _ in range(50):
        kinds = [list(rng.random(rng.integers(0, 9)) < 0.5) for _ in range(rng.integers(1, 40))]
        for cols in (1, 3, 16):
            sweeps, rounds, busy = bb.lockstep(kinds, cols)
            dense = sum(sum(k) for k in kinds)
            assert rounds <= sum(len(k) for k in kinds) and busy == dense
            assert sweeps <= bb.eager_sweeps(kinds, cols) or cols > 1
            if cols == 1:
                assert sweeps == dense == bb.eager_sweeps(kinds, 1)


@pytest.mark.parametrize("rmax, s16, s4, dense_all, dense_max, e16, e4",
                         [(1e-4, 36, 104, 401, 36, 55, 180), (1e-6, 110, 371, 1465, None, None, None)])
def test_sweep_counts_on_rmat12(rmat12, rmax, s16, s4, dense_all, dense_max, e16, e4):
    w, targets = rmat12_case(rmat12)
    assert targets.size == 64
    kinds, margins = [], []
    for t in targets:
        _, levels, _, margin, trace = bb.push_ref(("rmat12", int(t)), rmat12, w, int(t), None, ALPHA, rmax)
        kinds.append(bb.kinds_of(trace, rmat12, 0.25))
        assert len(kinds[-1]) == levels
        margins.append(margin)
    assert kinds[0] == bb.level_kinds(rmat12, w, int(targets[0]), ALPHA, rmax, 0.25)
    assert bb.lockstep_sweeps(kinds, 16) == s16 and bb.lockstep_sweeps(kinds, 4) == s4
    assert sum(sum(k) for k in kinds) == dense_all
    if dense_max is not None:
        assert max(sum(k) for k in kinds) == dense_max
        assert bb.eager_sweeps(kinds, 16) == e16 and bb.eager_sweeps(kinds, 4) == e4
    print("rmax %g: smallest margin %.2g" % (rmax, min(margins)))
    assert min(margins) >= bb.MARGIN


def test_margins_of_the_gpu_tests_inputs(pkg, got):
    """No value next to rmax: the GPU tests compare levels and pops for every query."""
    w = np.random.default_rng(21).uniform(0.5, 1.5, got.m)
    for rmax in (1e-3, 1e-6):
        worst = min(bb.push_ref(("got", t), got, w, t, None, ALPHA, rmax)[3] for t in range(got.n))
        print("got, rmax %g: smallest margin %.2g" % (rmax, worst))
        assert worst >= 1e-4
    host, d = reversed_dense_design(pkg)
    assert host.m % 512 == 46  # the last chunk's lanes read their weights one by one
    wd = design_weights(host, 43)
    worst = min(bb.push_ref(("rdense", t), host, wd, t, None, ALPHA, 1e-7)[3] for t in design_targets(d))
    print("reversed dense design, rmax 1e-7: smallest margin %.2g" % worst)
    assert worst >= 1e-2
