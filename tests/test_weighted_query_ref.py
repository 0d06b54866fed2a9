"""tests/weighted_query_ref.py pinned on its own, without a device: the seeded weighted push against the unweighted
seed-set target and against the exact push invariant over the weighted P, its two degenerate sets, and the weighted
top-k rounds against the exact pi of their p."""
import numpy as np
import pytest

import weighted_query_ref as wq
import weighted_ref as wr
from test_seeds import pi_p_left, rule_b

ALPHA = 0.15


def _deg(host):
    return np.diff(host.out_rp.astype(np.int64))


def _rand_w(host, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, host.m)


def _mixed_set(host, n_live=3, n_dead=2):
    deg = _deg(host)
    live, dead = np.flatnonzero(deg > 0), np.flatnonzero(deg == 0)
    seeds = np.concatenate([live[[1, live.size // 2, live.size - 1]][:n_live], dead[:n_dead]])
    sw = np.arange(1, seeds.size + 1, dtype=np.float64)
    return seeds, sw


def pi_p_exact(host, w, p, alpha):
    """p^T Pi_p, Pi_p = alpha (I - (1 - alpha) P_p)^-1 with P_p the weighted transition matrix whose dead-end rows are p."""
    P = wr.transition(host, w)
    P[_deg(host) == 0] = p
    return alpha * np.linalg.solve((np.eye(host.n) - (1.0 - alpha) * P).T, p)


def _Pi_p(host, w, p, alpha):
    P = wr.transition(host, w)
    P[_deg(host) == 0] = p
    return alpha * np.linalg.inv(np.eye(host.n) - (1.0 - alpha) * P)


@pytest.mark.parametrize("weight", [4.0, 0.25])
def test_power_of_two_weights_give_the_unweighted_seed_set_target(got, toy_graphs, weight):
    """Every weight one power of two: P is the unweighted P and every product is exact.  Run to convergence (rmax so
    small that rsum <= rmax m is below the bar), the reserve is rule_b's pi_p; at any rmax the unweighted invariant
    p^T Pi_p = reserve + r^T Pi_p (pi_p_left) holds."""
    for host in (got, toy_graphs["star_dead_leaves"], toy_graphs["isolated_mix"]):
        w = np.full(host.m, weight)
        deg = _deg(host)
        live, dead = np.flatnonzero(deg > 0), np.flatnonzero(deg == 0)
        seeds = np.concatenate([live[:2], dead[:2]])
        sw = np.arange(1, seeds.size + 1, dtype=np.float64)
        target = rule_b(host, seeds, sw, ALPHA)
        rmax = 1e-16
        reserve, residue, levels, pops = wq.push_sync_seeds(host, w, seeds, sw, ALPHA, rmax)
        assert residue.sum() <= rmax * host.m + 1e-18 and levels > 1 and pops >= levels
        assert np.max(np.abs(reserve - target)) <= 1e-12
        p = wq.seed_p(host.n, seeds, sw)
        for rmax in (1e-2, 1e-5):
            reserve, residue, _, _ = wq.push_sync_seeds(host, w, seeds, sw, ALPHA, rmax)
            assert not wr.active(residue, deg, rmax).any()
            err = np.max(np.abs(pi_p_left(host, p, p, ALPHA) - (reserve + pi_p_left(host, p, residue, ALPHA))))
            assert err <= 1e-13, (host.n, rmax, err)


def test_exact_push_invariant_over_the_weighted_transition_for_a_mixed_set(got, toy_graphs):
    for host, wseed in ((got, 21), (toy_graphs["star_dead_leaves"], 1)):
        w = _rand_w(host, wseed)
        seeds, sw = _mixed_set(host) if host.n > 8 else (np.array([0, 2, 4]), np.array([2.0, 1.0, 3.0]))
        deg = _deg(host)
        assert (deg[seeds] > 0).any() and (deg[seeds] == 0).any()
        p = wq.seed_p(host.n, seeds, sw)
        Pi = _Pi_p(host, w, p, ALPHA)
        for rmax in (1e-2, 1e-4, 1e-8):
            reserve, residue, levels, _ = wq.push_sync_seeds(host, w, seeds, sw, ALPHA, rmax)
            err = float(np.max(np.abs(p @ Pi - (reserve + residue @ Pi))))
            assert err <= 1e-13, (host.n, rmax, err)
            assert not wr.active(residue, deg, rmax).any() and levels >= 1


def test_a_set_of_one_seed_is_push_sync(got, rmat12):
    for host, wseed in ((got, 21), (rmat12, 22)):
        w = _rand_w(host, wseed)
        deg = _deg(host)
        for s in (int(np.argmax(deg)), int(np.flatnonzero(deg > 0)[3]), int(np.flatnonzero(deg == 0)[0])):
            for rmax in (1e-4, 1e-7):
                a = wr.push_sync(host, w, s, ALPHA, rmax)
                b = wq.push_sync_seeds(host, w, [s], [2.5], ALPHA, rmax)
                assert a[2:] == b[2:], (s, rmax)
                assert np.max(np.abs(a[0] - b[0])) <= 1e-15 and np.max(np.abs(a[1] - b[1])) <= 1e-15


def test_a_set_of_dead_ends_gives_p(got):
    dead = np.flatnonzero(_deg(got) == 0)[:3]
    sw = np.array([1.0, 2.0, 5.0])
    reserve, residue, levels, pops = wq.push_sync_seeds(got, _rand_w(got, 21), dead, sw, ALPHA, 1e-6)
    assert np.array_equal(reserve, wq.seed_p(got.n, dead, sw)) and not residue.any() and levels == 0 and pops == 0
    est, walks, steps = wq.fora_seeds(got, _rand_w(got, 21), dead, sw, 0.5, ALPHA, 3)
    assert np.array_equal(est, reserve) and walks == 0 and steps == 0


def test_duplicates_are_summed_and_zero_weights_dropped(got):
    w = _rand_w(got, 21)
    a = wq.push_sync_seeds(got, w, [5, 9, 5, 30, 12], [1.0, 2.0, 3.0, 0.0, 2.0], ALPHA, 1e-5)
    b = wq.push_sync_seeds(got, w, [5, 9, 12], [4.0, 2.0, 2.0], ALPHA, 1e-5)
    assert a[2:] == b[2:] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# (graph, weight seed, seeds, seed weights, k, walk seed): fixed, not searched
TOPK_CASES = [("got", 21, [63], None, 5, 3), ("got", 21, [3, 17, 42, 90], [1.0, 2.0, 1.0, 4.0], 10, 3),
              ("rmat12", 22, [1803], None, 8, 4), ("rmat12", 22, [5, 77, 1803, 2025], None, 32, 4)]


def test_topk_rounds_against_the_exact_pi(pkg, got, rmat12):
    eps = 0.5
    rounds = []
    for name, wseed, seeds, sw, k, seed in TOPK_CASES:
        host = got if name == "got" else rmat12
        w = _rand_w(host, wseed)
        conf = pkg.conf_topk(host.n, host.m, k, ALPHA)
        r = wq.topk(host, w, seeds, sw, eps, conf, seed)  # (asserts that every round ends with no active node)
        rounds.append(r["rounds"])
        assert not wr.active(r["residue"], _deg(host), r["rmax"]).any()
        pi = pi_p_exact(host, w, wq.seed_p(host.n, seeds, sw), ALPHA)
        bound = eps * np.maximum(pi[r["ids"]], r["delta"])
        worst = float(np.max(np.abs(r["vals"] - pi[r["ids"]]) / bound))
        print("%s %s k %d: rounds %d, walks %d, delta %.3g, worst |val - pi| / bound %.3f" %
              (name, seeds, k, r["rounds"], r["walks"], r["delta"], worst))
        assert r["ids"].size == min(k, np.count_nonzero(r["est"] > 0.0)) and worst <= 1.0, (name, seeds, worst)
        # the push invariant of the last round's state
        p = wq.seed_p(host.n, seeds, sw)
        assert abs(r["reserve"].sum() + r["residue"].sum() - 1.0) <= 1e-12 and p.sum() == pytest.approx(1.0, abs=1e-15)
    assert max(rounds) >= 2, rounds


def test_topk_without_a_live_seed_is_p(pkg, got):
    dead = np.flatnonzero(_deg(got) == 0)[:2]
    conf = pkg.conf_topk(got.n, got.m, 5, ALPHA)
    r = wq.topk(got, _rand_w(got, 21), dead, [1.0, 3.0], 0.5, conf, 3)
    assert r["rounds"] == 0 and r["walks"] == 0 and np.array_equal(r["est"], wq.seed_p(got.n, dead, [1.0, 3.0]))
    assert r["ids"].tolist() == [int(dead[1]), int(dead[0])] and r["kth"] == 0.0
