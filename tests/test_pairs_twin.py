"""The oracle-side twin of the single-pair estimator (DESIGN.md §2 "Single pairs", §3), without a device: pair_twin and
its helpers, which tests/test_gpu_pairs_regimes.py holds pprhip_ppr_pairs to, and the exact identity the estimator rests
on,  pi(s, t) = p_t(s) / S(s) + sum_v pi(s, v) r_t(v),  checked here on the oracle's own backward push - so that a
mistake in the test's algebra shows on the CPU, before the engine is held to the same line."""
import math

import numpy as np
import pytest

from conftest import to_oracle
from test_gpu_pairs import ppr_exact, survival_dense

PAIR_EPS = 0.5  # the eps every regime test calls with: the walk count is steered through the conf's delta
# w < 64: a refill finds fewer walks left than free lanes; 63 / 64 / 65: one wave's width; 1023 / 1024 / 1025: one item
# and the first cut into two; 2049: three items; 524 288 = 512 x 1024: the item cap, reached exactly; 524 289: items of
# 1 025 walks, the last one of 514; 700 001 = 511 x 1 368 + 953.
LADDER = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 524288, 524289, 700001]


def pair_regime(w):
    """(items per pair, walks per item) of a pair's w walks: min(512, ceil(w / 1024)) items of ceil(w / items) walks
    (DESIGN.md §2 "Single pairs", driver)."""
    chunks = min(512, -(-w // 1024)) if w else 0
    return chunks, (-(-w // chunks) if chunks else 0)


def conf_for_walks(pkg, host, alpha, rmax, w, eps=PAIR_EPS):
    """The whole-graph conf of host with delta moved so that a pair call at (eps, rmax) takes exactly w walks per pair:
    w = ceil(omega rmax), omega = 3 ln(2 / pfail) / (eps^2 delta), and delta puts omega rmax at w - 1/2.  The caller
    asserts pkg.pair_params(conf, eps, rmax) == (rmax, w)."""
    conf = pkg.conf_whole_graph(host.n, host.m, alpha)
    conf.delta = 3.0 * math.log(2.0 / conf.pfail) / (eps * eps) * rmax / (w - 0.5)
    return conf


class PairTwin:
    """pair_twin's parts for one graph, alpha and r_max, each computed once: S by the dense solve, the oracle's backward
    push (SYNC schedule) per target, the walk sums per (source, target, walks, seed)."""

    def __init__(self, orc, og, host, alpha, rmax):
        self.orc, self.og, self.host, self.alpha, self.rmax = orc, og, host, alpha, rmax
        self.surv = survival_dense(host, alpha)
        self.din = np.diff(host.in_rp.astype(np.int64))
        self._push, self._walk = {}, {}

    def push(self, t):
        if t not in self._push:
            self._push[t] = self.og.backward_push(t, self.alpha, self.rmax, self.orc.SYNC)
        return self._push[t]

    def tie_margin(self, t):
        """The smallest |r / rmax - 1| over the residues the push from t left (inf without residue)."""
        r = self.push(t)[1]
        r = r[r > 0.0]
        return float(np.min(np.abs(r / self.rmax - 1.0))) if r.size else math.inf

    def pair(self, s, t, walks, seed):
        """(value, steps of its walks, walks it ran)."""
        if self.din[t] == 0:  # the pair start rule: t popped without in-edges, p_t(t) = alpha, no residue, no walks
            return (self.alpha / self.surv[t] if s == t else 0.0), 0, 0
        p, r, _ = self.push(t)
        key = (s, t, walks, seed)
        if key not in self._walk:
            self._walk[key] = self.og.pair_walk_sum(s, self.alpha, seed, walks, r)
        total, steps = self._walk[key]
        return p[s] / self.surv[s] + total / walks, steps, walks


def pair_twin(orc, og, host, s, t, alpha, rmax, walks, seed, twin=None):
    """The value of pair (s, t) from the oracle's parts, nothing of the engine's: p_t, r_t of the oracle's backward push
    (SYNC) under the pair start rule, S by the dense solve, the walk term by orc_pair_walk_sum.  Returns (value, steps,
    walks); twin: a PairTwin of the same graph, alpha and r_max whose parts are re-used."""
    twin = twin or PairTwin(orc, og, host, alpha, rmax)
    assert twin.alpha == alpha and twin.rmax == rmax and twin.host is host
    return twin.pair(s, t, walks, seed)


def identity_error(pi, p, r, surv, t):
    """max_s |p_t(s) / S(s) + sum_v pi(s, v) r_t(v) - pi(s, t)|"""
    return float(np.max(np.abs(p / surv + pi @ r - pi[:, t])))


# ------------------------------------------------------------------ the twin's own checks (no device)
@pytest.mark.parametrize("w", LADDER)
def test_conf_for_walks_hits_the_walk_count(pkg, got, w):
    for rmax in (0.02, 1e-3, 0.9):
        conf = conf_for_walks(pkg, got, 0.15, rmax, w)
        assert pkg.pair_params(conf, PAIR_EPS, rmax) == (rmax, w)


def test_pair_regime_table():
    assert [pair_regime(w) for w in (0, 1, 64, 1024, 1025, 2049, 524288, 524289, 700001)] == [
        (0, 0), (1, 1), (1, 64), (1, 1024), (2, 513), (3, 683), (512, 1024), (512, 1025), (512, 1368)]


def test_ladder_reaches_every_regime():
    """The ladder as the driver cuts it: one item below and at 1 024 walks, the cut into 2 and 3 items with a shorter
    last one, the cap of 512 items exactly, and items longer than 1 024 walks under the cap."""
    reg = {w: pair_regime(w) for w in LADDER}
    assert all(reg[w] == (1, w) for w in (1, 2, 63, 64, 65, 1023, 1024))
    assert reg[1025] == (2, 513) and 2 * 513 > 1025 and reg[2049] == (3, 683)
    assert reg[524288] == (512, 1024) and reg[524289] == (512, 1025) and 524289 - 511 * 1025 == 514
    assert reg[700001] == (512, 1368) and 700001 % 512 != 0 and 0 < 700001 - 511 * 1368 < 1368


@pytest.mark.parametrize("alpha", [0.05, 0.15, 0.5])
def test_exact_identity_on_the_oracle_push(orc, got, toy_graphs, alpha):
    """pi(s, t) = p_t(s) / S(s) + sum_v pi(s, v) r_t(v) for every source at once, any r_max, both schedules (the
    identity does not care how far the push went).  A target without in-edges is left out: orc_backward_push keeps
    Backward_Search.java:46-49's reserve(t) = 1 there, which is not the pair start rule."""
    for name, host in (("got", got), ("isolated_mix", toy_graphs["isolated_mix"]), ("line", toy_graphs["line"])):
        og = to_oracle(orc, host)
        pi, surv = ppr_exact(host, alpha), survival_dense(host, alpha)
        assert np.max(np.abs(pi.sum(axis=1) - 1.0)) <= 1e-12
        din = np.diff(host.in_rp.astype(np.int64))
        for rmax in (1e-2, 1e-4, 1e-6):
            for schedule in (orc.FIFO, orc.SYNC):
                worst = 0.0
                for t in np.flatnonzero(din > 0):
                    p, r, _ = og.backward_push(int(t), alpha, rmax, schedule)
                    assert np.max(r) <= rmax
                    worst = max(worst, identity_error(pi, p, r, surv, int(t)))
                assert worst <= 1e-12, (name, alpha, rmax, schedule, worst)


def test_pair_twin_estimates_pi(orc, got):
    """The twin is an estimator of the exact pi: at 20 000 walks and r_max = 0.02 every term lies in [0, r_max], so
    Hoeffding puts |twin - pi| <= 6 r_max / (2 sqrt(w)) (failure probability 2 exp(-18) per pair); and a target without
    in-edges is exact."""
    og = to_oracle(orc, got)
    pi = ppr_exact(got, 0.15)
    tw = PairTwin(orc, og, got, 0.15, 0.02)
    rng = np.random.default_rng(4)
    w = 20000
    for s, t in zip(rng.integers(0, got.n, 12), rng.integers(0, got.n, 12)):
        v, steps, ran = pair_twin(orc, og, got, int(s), int(t), 0.15, 0.02, w, 9, twin=tw)
        if tw.din[t] == 0:
            assert ran == 0 and v == (0.15 / tw.surv[t] if s == t else 0.0)
            assert v == pytest.approx(pi[s, t], rel=1e-12, abs=0.0)
        else:
            assert ran == w and abs(v - pi[s, t]) <= 6 * 0.02 / (2 * math.sqrt(w)), (s, t, v, pi[s, t])
