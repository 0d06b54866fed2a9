"""The sweep cut by relationship weight without a device: the numpy reference of tests/weighted_sweep_ref.py against
brute force and against the unweighted reference, and the quantum rule of include/pprhip.h "weighted local clustering"
against pprhip_weight_quantum (a pure host function).  Every comparison is exact: quanta are integers, the conductance
is compared by its bits."""
import struct

import numpy as np
import pytest

from sweep_ref import edges_of, sweep_ref
from test_sweep_ref import BARBELL_X, barbell_edges
from weighted_sweep_ref import cut_of, qdegrees, quanta, shift_of, vol_limit, weighted_sweep_ref

SIZES = [1, 2, 3, 4, 1000, 1 << 16, (1 << 16) + 1]


def bits(d):
    return struct.pack("<d", float(d))


def weight_sets(m, rng):
    """The weight sets of the issue, by name."""
    spread = np.full(m, 1e-30)
    spread[m // 2] = 1e30
    return {"ones": np.ones(m), "halves": np.full(m, 0.5), "uniform": rng.uniform(0.5, 1.5, m),
            "pareto": rng.pareto(1.5, m) + 0.01, "huge": np.full(m, 1e300), "tiny": np.full(m, 1e-300), "spread": spread}


def multigraph(rng, n, m):
    """A random multigraph with self loops and parallel relationships."""
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    src[:4], dst[:4] = [0, 0, 1, 1], [0, 1, 2, 2]        # a self loop, a pair of parallel relationships
    return src.astype(np.int64), dst.astype(np.int64)


def brute(n, src, dst, w, r, max_vol=0.0):
    """Every word of a reference result from brute force over its own order."""
    q = quanta(w)
    qdeg = qdegrees(n, src, dst, q)
    total = 2 * sum(int(c) for c in q)
    assert r["total_vol_q"] == total and r["shift"] == shift_of(w)
    vol, best = 0, (float("inf"), 0, 0, 0)
    for i in range(r["profiled"]):
        vol += int(qdeg[r["order"][i]])
        cut = cut_of(n, src, dst, q, r["order"][:i + 1])
        assert (int(r["vol_q"][i]), int(r["cut_q"][i])) == (vol, cut), i
        den = min(vol, total - vol)
        if den > 0 and (max_vol <= 0 or vol <= vol_limit(max_vol, r["shift"])):
            phi = float(np.float64(np.uint64(cut)) / np.float64(np.uint64(den)))
            if phi < best[0]:
                best = (phi, i + 1, cut, vol)
    assert (r["best_size"], r["best_cut_q"], r["best_vol_q"]) == best[1:]
    assert bits(r["best_conductance"]) == bits(best[0])


# ------------------------------------------------------------------ the reference against brute force
def test_barbell_with_a_heavy_bridge():
    src, dst = barbell_edges()
    w = np.ones(14)
    r = weighted_sweep_ref(6, src, dst, w, BARBELL_X)
    u = sweep_ref(6, src, dst, BARBELL_X)
    q0 = 1 << r["shift"]
    assert r["shift"] == 61 - 1 - 4 and list(r["order"]) == list(u["order"]) and r["best_size"] == 3
    assert list(r["vol_q"]) == [int(v) * q0 for v in u["vol"]] and list(r["cut_q"]) == [int(c) * q0 for c in u["cut"]]
    w[(src == 2) & (dst == 3)] = 8.0       # the bridge weighs more than a triangle: the best cut leaves it inside
    w[(src == 3) & (dst == 2)] = 8.0
    h = weighted_sweep_ref(6, src, dst, w, BARBELL_X, normalize=0)
    assert list(h["order"]) == [0, 1, 2, 3, 4, 5] and h["best_size"] != 3
    brute(6, src, dst, w, h)


def test_toy_graphs_against_brute_force(toy_graphs):
    rng = np.random.default_rng(5)
    for name, host in toy_graphs.items():
        src, dst = edges_of(host)
        for wname, w in weight_sets(host.m, rng).items():
            x = rng.random(host.n) * (rng.random(host.n) < 0.8)
            for normalize in (0, 1):
                r = weighted_sweep_ref(host.n, src, dst, w, x, normalize=normalize)
                brute(host.n, src, dst, w, r)
                assert r["edge_slots"] == sum(np.bincount(np.concatenate([src, dst]), minlength=host.n)[r["order"]])
    host = toy_graphs["isolated_mix"]
    src, dst = edges_of(host)
    q = quanta(np.arange(1, 7, dtype=np.float64))
    qdeg = qdegrees(host.n, src, dst, q)
    loop = int(np.nonzero((src == 0) & (dst == 0))[0][0])
    assert int(qdeg[0]) == sum(int(q[e]) for e in range(6) if src[e] == 0 or dst[e] == 0) + int(q[loop])   # twice
    assert int(qdeg[4]) == int(qdeg[5]) == 0
    assert weighted_sweep_ref(host.n, src, dst, np.ones(6), np.array([0, 0, 0, 0, 1.0, 0]))["support"] == 0


@pytest.mark.parametrize("n,m", [(9, 30), (40, 90), (64, 400)])
def test_random_multigraphs_against_brute_force(n, m):
    rng = np.random.default_rng(11 + n)
    src, dst = multigraph(rng, n, m)
    for wname, w in weight_sets(m, rng).items():
        x = rng.random(n) * (rng.random(n) < 0.7)
        x[rng.integers(0, n, 3)] = 0.125                                # a few exact ties
        for normalize in (0, 1):
            r = weighted_sweep_ref(n, src, dst, w, x, normalize=normalize)
            brute(n, src, dst, w, r)
            half = float(np.sum(w)) / 2
            brute(n, src, dst, w, weighted_sweep_ref(n, src, dst, w, x, normalize=normalize, max_vol=half), max_vol=half)
            k = weighted_sweep_ref(n, src, dst, w, x, normalize=normalize, max_size=5)
            assert k["profiled"] == min(5, r["support"]) and np.array_equal(k["vol_q"], r["vol_q"][:k["profiled"]])
            brute(n, src, dst, w, k)


# ------------------------------------------------------------------ the quantum rule
@pytest.mark.parametrize("m", SIZES)
def test_weight_quantum_is_the_rule_and_the_bound_holds(pkg, m):
    rng = np.random.default_rng(m)
    L = 0
    while (1 << L) < m:
        L += 1
    for name, w in weight_sets(m, rng).items():
        s = pkg.weight_quantum(w)
        assert s == shift_of(w), name
        q = quanta(w, s)
        assert int(q.min()) >= 1 and int(q.max()) <= 1 << (61 - L), name
        total = 2 * sum(q.tolist())
        assert total <= 1 << 62, (name, m, total)
        if name in ("ones", "halves", "huge", "tiny") and m & (m - 1) == 0:
            assert total > 1 << 60, (name, m)                           # and the bits are used


@pytest.mark.parametrize("k", [1, 2, 5, 10, 16])
def test_bound_at_powers_of_two_and_one_more(pkg, k):
    for m in (1 << k, (1 << k) + 1):
        for w in (np.ones(m), np.full(m, np.nextafter(2.0, 0.0)), np.full(m, 1e300)):
            s = pkg.weight_quantum(w)
            assert s == shift_of(w)
            assert 2 * sum(quanta(w, s).tolist()) <= 1 << 62


def test_a_weight_below_half_a_quantum_is_one_quantum():
    # five weights, the largest 1.0: L = 3, e = 1, s = 57, one quantum is worth 2^-57
    w = np.array([1.0, 2.0 ** -70, 1e-300, 0.49 * 2.0 ** -57, 0.5 * 2.0 ** -57])
    assert shift_of(w) == 57
    assert quanta(w).tolist() == [1 << 57, 1, 1, 1, 1]
    assert quanta(np.array([1.0, 3.0 * 2.0 ** -57, 1.0, 1.0, 1.0])).tolist()[1] == 3
    # two weights: s = 59; ties go to even
    assert quanta(np.array([1.0, 1.5 * 2.0 ** -59])).tolist() == [1 << 59, 2]
    assert quanta(np.array([1.0, 2.5 * 2.0 ** -59])).tolist() == [1 << 59, 2]
    assert quanta(np.array([1.0, 3.5 * 2.0 ** -59])).tolist() == [1 << 59, 4]


def same_value(a, b):
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    return bits(a) == bits(b) if isinstance(a, float) else a == b


def test_scaling_by_a_power_of_two_moves_the_shift_alone():
    rng = np.random.default_rng(3)
    n, m = 50, 300
    src, dst = multigraph(rng, n, m)
    w = rng.pareto(1.5, m) + 0.01
    x = rng.random(n)
    a = weighted_sweep_ref(n, src, dst, w, x)
    for k in (-40, -1, 3, 200):
        b = weighted_sweep_ref(n, src, dst, np.ldexp(w, k), x)
        assert b["shift"] == a["shift"] - k
        assert np.array_equal(quanta(np.ldexp(w, k)), quanta(w))
        for key in a:
            assert key == "shift" or same_value(a[key], b[key]), key


@pytest.mark.parametrize("w0", [1.0, 0.5, 2.0 ** -10, 2.0 ** 40])
def test_equal_power_of_two_weights_give_the_unweighted_sweep(w0):
    rng = np.random.default_rng(8)
    n, m = 200, 3000
    src, dst = multigraph(rng, n, m)
    x = rng.random(n) * (rng.random(n) < 0.8)
    for normalize in (0, 1):
        for kw in (dict(), dict(max_size=40)):
            u = sweep_ref(n, src, dst, x, normalize=normalize, **kw)
            r = weighted_sweep_ref(n, src, dst, np.full(m, w0), x, normalize=normalize, **kw)
            q0 = int(quanta(np.full(m, w0))[0])
            assert q0 == 1 << 48 and r["shift"] == 61 - (int(np.log2(w0)) + 1) - 12      # 3000 <= 2^12
            assert np.array_equal(r["order"], u["order"]) and (r["support"], r["profiled"]) == (u["support"], u["profiled"])
            assert np.array_equal(r["vol_q"], u["vol"] * np.uint64(q0)) and np.array_equal(r["cut_q"], u["cut"] * np.uint64(q0))
            assert (r["best_size"], r["best_cut_q"], r["best_vol_q"]) == (u["best_size"], u["best_cut"] * q0, u["best_vol"] * q0)
            assert bits(r["best_conductance"]) == bits(u["best_conductance"])
            assert r["total_vol_q"] == u["total_vol"] * q0 and r["edge_slots"] == u["edge_slots"]
        # max_vol in weight units against the unweighted bound in relationships
        u = sweep_ref(n, src, dst, x, max_vol=m // 3)
        r = weighted_sweep_ref(n, src, dst, np.full(m, w0), x, max_vol=(m // 3) * w0)
        assert r["best_size"] == u["best_size"] and bits(r["best_conductance"]) == bits(u["best_conductance"])


def test_max_vol_limit_in_quanta():
    assert vol_limit(1.0, 10) == 1024 and vol_limit(1.5, 1) == 3 and vol_limit(0.75, 1) == 1
    assert vol_limit(1e300, 60) == (1 << 63) - 1 and vol_limit(1.0, 63) == (1 << 63) - 1 and vol_limit(1.0, 62) == 1 << 62
    assert vol_limit(1e-300, 5) == 0
    src, dst = barbell_edges()
    r = weighted_sweep_ref(6, src, dst, np.ones(14), BARBELL_X, max_vol=1e-30)    # below one quantum: no candidate
    assert r["best_size"] == 0 and r["best_conductance"] == float("inf") and r["profiled"] == 6
