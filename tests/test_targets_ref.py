"""The mathematics of the single-target queries (include/pprhip.h "single targets", DESIGN.md §2 "Single targets"),
pinned on the CPU independently of the engine: with p and r from the oracle's backward search and S from a dense solve,
the push invariant reproduces the leaking PPR, and p / S is a lower bound of the engine's restarting PPR that misses it
by at most rmax, for every (s, t)."""
import numpy as np
import pytest

from conftest import to_oracle
from targets_ref import leaking_exact, ppr_exact

RMAX = (1e-2, 1e-5)


def _graphs(got, toy_graphs):
    g = dict(toy_graphs)
    g["got"] = got
    return g


@pytest.mark.parametrize("alpha", [0.15, 0.5])
def test_invariant_and_bound_on_every_pair(orc, got, toy_graphs, alpha):
    for name, host in _graphs(got, toy_graphs).items():
        og = to_oracle(orc, host)
        leak = leaking_exact(host, alpha)
        S = leak.sum(axis=1)
        pi = ppr_exact(host, alpha)
        assert np.all(S >= alpha - 1e-15) and np.all(S <= 1.0 + 1e-12)
        idg = np.diff(host.in_rp.astype(np.int64))
        for rmax in RMAX:
            for t in range(host.n):
                if idg[t] == 0:
                    # The oracle follows Backward_Search.java:46-49 here (reserve(t) = 1, nothing pushed); the query is
                    # held to the definition instead: r(t) = 1 and t popped leaves p(t) = alpha and no residue.
                    po, _, _ = og.backward_push(t, alpha, rmax)
                    assert po[t] == 1.0 and np.count_nonzero(po) == 1
                    p, r = np.zeros(host.n), np.zeros(host.n)
                    p[t] = alpha
                else:
                    p, r, _ = og.backward_push(t, alpha, rmax)
                assert np.all(r >= 0.0) and np.max(r) <= rmax, (name, t, rmax, np.max(r))
                # pi'(s, t) = p_t(s) + sum_v pi'(s, v) r_t(v)
                assert np.max(np.abs(p + leak @ r - leak[:, t])) <= 1e-12, (name, t, rmax)
                # 0 <= pi(s, t) - p_t(s) / S(s) <= rmax (1e-12: the rounding of the dense solve and of the push's sums)
                gap = pi[:, t] - p / S
                assert np.min(gap) >= -1e-12 and np.max(gap) <= rmax + 1e-12, (name, t, rmax, np.min(gap), np.max(gap))


def test_bound_is_linear_in_the_start(orc, got):
    """A weighted set: sum_t w_t p_t / S misses pi(., T) by at most sum_t w_t rmax_t - the linearity the set start rests
    on (one push from r = w at rmax has every residue <= rmax, so its own bound is rmax)."""
    alpha, rmax = 0.15, 1e-3
    og = to_oracle(orc, got)
    pi = ppr_exact(got, alpha)
    S = leaking_exact(got, alpha).sum(axis=1)
    idg = np.diff(got.in_rp.astype(np.int64))
    members = np.flatnonzero(idg > 0)[:7]
    w = np.array([0.5, 2.0, 1.0, 0.25, 3.0, 1.0, 0.125])
    acc = np.zeros(got.n)
    for t, wt in zip(members, w):
        p, _, _ = og.backward_push(int(t), alpha, rmax)
        acc += wt * p
    gap = pi[:, members] @ w - acc / S
    assert np.min(gap) >= -1e-12 and np.max(gap) <= rmax * w.sum() + 1e-12
