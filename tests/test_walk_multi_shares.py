"""The dealing rule of the batched weighted top-k's merged walk launch without a device (pprhip_walk_multi_shares,
walk_multi_shares) against a numpy restatement written here, at its edges: nothing to walk, a single walk, fewer walks
than a wave has lanes, counts that are an exact multiple of a wave's share and one more, idle columns at the ends and
between busy ones, sixteen columns of one walk on a base grid of one wave (the case that reaches the W + 15 bound),
one column holding everything."""
import numpy as np
import pytest

B = 16


def _restated(counts, base_waves):
    c = [int(x) for x in counts]
    groups = (sum(c) + 63) // 64
    per = (groups + base_waves - 1) // base_waves * 64
    nw = [(x + per - 1) // per if per else 0 for x in c]
    return per, np.concatenate(([0], np.cumsum(nw))).astype(np.int64)


def _cols(d):
    c = np.zeros(B, dtype=np.uint64)
    for k, v in d.items():
        c[k] = v
    return c


# "a multiple of per and per + 1": T = 1408 + 705 + 500 + 3 = 2616 -> 41 groups of 64, W = 4 -> per = 11 * 64 = 704
CASES = {
    "all zero": (_cols({}), 4096),
    "one column, one walk": (_cols({5: 1}), 4096),
    "fewer walks than lanes": (_cols({0: 7, 3: 20, 9: 1}), 4096),
    "a multiple of per and per + 1": (_cols({1: 2 * 704, 2: 705, 6: 500, 7: 3}), 4),
    "idle between, first and last idle": (_cols({1: 1000, 2: 3, 7: 50000, 14: 64}), 64),
    "sixteen single walks, one base wave": (np.ones(B, dtype=np.uint64), 1),
    "one column holds everything": (_cols({15: 5_000_000}), 4096),
    "base_waves = 1": (_cols({0: 100, 4: 1, 8: 1000, 12: 65}), 1),
    "many, few, one": (_cols({0: 1, 2: 40, 3: 3_000_000, 5: 129}), 4096),
    "the largest counts": (np.full(B, (1 << 36) - 1, dtype=np.uint64), 4096),
}


@pytest.mark.parametrize("case", list(CASES))
def test_shares_against_the_restatement(pkg, case):
    counts, base = CASES[case]
    per, first = pkg.walk_multi_shares(counts, base)
    rper, rfirst = _restated(counts, base)
    assert per == rper and np.array_equal(first.astype(np.int64), rfirst), (case, per, rper, first, rfirst)
    assert first.size == B + 1 and first[0] == 0 and (np.diff(first.astype(np.int64)) >= 0).all()
    # no more waves than the launch has, and the bound is reached by sixteen single walks on one base wave
    assert int(first[B]) <= base + B - 1, (case, first[B], base)
    if case == "sixteen single walks, one base wave":
        assert int(first[B]) == base + B - 1 and per == 64
    total = int(counts.astype(object).sum())
    if total == 0:
        assert per == 0 and not first.any()
        return
    assert per % 64 == 0 and per * base >= total
    # the shares partition every column's [0, c) exactly once; a wave belongs to one column (the ranges of waves are
    # disjoint by construction of first: wave b lies in exactly one [first[c], first[c + 1]))
    for c in range(B):
        lo, hi, cnt = int(first[c]), int(first[c + 1]), int(counts[c])
        assert (hi > lo) == (cnt > 0), (case, c)
        if cnt == 0:
            continue
        starts = [(b - lo) * per for b in range(lo, min(hi, lo + 4))] + [(hi - 1 - lo) * per]
        assert starts[0] == 0 and all(s < cnt for s in starts), (case, c)  # every wave of the column has walks
        assert (hi - lo - 1) * per < cnt <= (hi - lo) * per, (case, c)     # and the last one ends at cnt exactly
    if case == "a multiple of per and per + 1":
        assert per == 704 and first[2] - first[1] == 2 and first[3] - first[2] == 2 and first[7] - first[6] == 1


def test_small_cases_wave_by_wave(pkg):
    """Every wave's range written out: each walk of each column lies in exactly one wave."""
    rng = np.random.default_rng(7)
    for base in (1, 2, 5, 16):
        for _ in range(6):
            counts = rng.integers(0, 300, B).astype(np.uint64) * rng.integers(0, 2, B).astype(np.uint64)
            per, first = pkg.walk_multi_shares(counts, base)
            owner = np.full(int(first[B]), -1)
            for c in range(B):
                seen = np.zeros(int(counts[c]), dtype=np.int64)
                for b in range(int(first[c]), int(first[c + 1])):
                    assert owner[b] == -1
                    owner[b] = c
                    lo = (b - int(first[c])) * per
                    hi = min(lo + per, int(counts[c]))
                    assert lo < hi
                    seen[lo:hi] += 1
                assert (seen == 1).all(), (base, c)
            assert (owner >= 0).all() and int(first[B]) <= base + B - 1


def test_refusals(pkg):
    with pytest.raises(pkg.PprhipError, match="base_waves"):
        pkg.walk_multi_shares(np.zeros(B, dtype=np.uint64), 0)
    with pytest.raises(pkg.PprhipError, match="walk limit"):
        pkg.walk_multi_shares(_cols({3: 1 << 36}), 8)
    with pytest.raises(ValueError):
        pkg.walk_multi_shares(np.zeros(B - 1, dtype=np.uint64), 8)
