"""Designed graphs of the weighted seed-set and top-k tests (tests/test_gpu_weighted_query.py).  Their properties are
asserted on the host - the lift's internal order and the numpy reference - by the tests that use them."""
import math

import numpy as np

from conftest import edges_to_host

import weighted_query_ref as wq

TILE = 1024  # nodes a workgroup of the round-start collect kernel compacts with one packed atomic (kWqTile)
PUSH_TILE = 2048  # edges per workgroup iteration of the sparse push kernel (kWTile)


def landing_design(pkg):
    """Dead-end mass that lands in a dense level and in a sparse level of the same push, on a set with a live seed that
    has in-edges (A), a live seed without (B: an extra row of the dense apply) and a dead-end seed (dz, isolated).
      level 0  {A, B}: A -> d0 (dead end), A -> H, B -> H                                   small
      level 1  {d0, H}: d0's mass lands; H -> 600 pool nodes                                 wide
      level 2  the pool: 100 of them dead ends (their mass lands), 500 -> T                  wide
      level 3  {T, ...}: T -> d1 (dead end), T -> A                                          small
      level 4  {d1, ...}: d1's mass lands                                                    small
    With dense_frac = 0.25 (277 of m = 1 106) the wide levels are dense, the others sparse.
    Returns (host, seeds, seed weights, dict of the named nodes)."""
    A, B, H, T, d0, d1, dz = 0, 1, 2, 3, 4, 5, 6
    pool = list(range(7, 607))
    n = pool[-1] + 1
    edges = [(A, d0), (A, H), (B, H), (T, d1), (T, A)]
    edges += [(H, p) for p in pool]
    edges += [(p, T) for p in pool[100:]]
    host = edges_to_host(pkg, n, edges)
    return host, np.array([A, B, dz, A]), np.array([1.0, 1.0, 1.0, 1.0]), dict(A=A, B=B, H=H, T=T, d0=d0, d1=d1, dz=dz)


def collect_design(pkg):
    """The first frontier of a top-k round at the edges of the collect kernel, with residues that sit EXACTLY on the
    threshold.  alpha = 0.5 and every weight sum a power of two (or a divisor that leaves one), so every product,
    quotient and sum of the push is exact: r / d == rmax is decided by `>=`, and the device's order of additions
    cannot change a decision.
      S = 0 (the source), G = 1 (out-degree 5 000), Z = 2 (out-degree 4 500), targets 3 .. n - 1 (out-degree 1, -> Z),
      n = 3 * 1 024 + 37.  S -> G, S -> Z, S -> every target; G and Z -> the targets in turn (parallel relationships),
      Z's last one -> S.
    Internal order = (has in-edges, out-degree descending, id): G, Z, S, then the targets by id - a target's internal id
    is its id, G's is 0.  W(S) = 2^15 and T = 3 * 2^-16 (a threshold inside a binade: the schedule's expression reaches
    it, exact_eps); w(S -> t) = 1.5 (r = T / 2 after S pops) except the CHOSEN targets 1 023, 2 048, 3 071 and n - 1, w =
    3 (r = T); w(S -> G) = 3 * 5 000 (r / d = T); S -> Z takes the rest (r / d < T).
    At a schedule whose second round runs at rmax = T and whose first round's rmax is above every r / d, round 0 is S's
    pop alone and round 1 starts from {G} + CHOSEN: active nodes at the first position of the array and of a tile, at
    the last position of a tile and of the array, a tile (1 024 .. 2 047) with none, n no multiple of the tile, and
    5 000 + 4 edges whose prefix crosses two tiles of the push kernel.  G's pushes (weights 1) then lift T / 2 to T:
    more nodes that join on equality.  Returns (host, weights, dict)."""
    n = 3 * TILE + 37
    S, G, Z = 0, 1, 2
    targets = np.arange(3, n)
    chosen = np.array([TILE - 1, 2 * TILE, 3 * TILE - 1, n - 1])
    dG, dZ = 5000, 4500
    src = np.concatenate([np.full(2 + targets.size, S), np.full(dG, G), np.full(dZ, Z), targets])
    zdst = targets[np.arange(dZ) % targets.size]
    zdst[-1] = S  # (S has an in-edge: it sorts with the other rows that have one)
    dst = np.concatenate([[G, Z], targets, targets[np.arange(dG) % targets.size], zdst, np.full(targets.size, Z)])
    wS = np.full(2 + targets.size, 1.5)
    wS[0] = 3.0 * dG
    wS[2 + (chosen - 3)] = 3.0
    wS[1] = 2.0 ** 15 - (wS.sum() - wS[1])
    assert wS[1] > 0 and wS.sum() == 2.0 ** 15
    w_edges = np.concatenate([wS, np.ones(dG + dZ + targets.size)])
    host = pkg.HostCsr(n, src.astype(np.int32), dst.astype(np.int32))
    w = w_edges[pkg.out_edge_order(src.astype(np.int32), False)]
    return host, w, dict(S=S, G=G, Z=Z, chosen=chosen, rmax1=3.0 * 2.0 ** -16, n=n)


def exact_eps(conf, target, lo=1e-3, hi=4.0):
    """An eps at which the push threshold of the SECOND round (delta = conf.delta / 4) is exactly `target` (a power of
    two): bisection on the schedule's own expression to the two doubles around the crossing; when neither hits (the
    expression steps by about two ulps there), conf.delta moves to its next double - which shifts the values a little -
    and the search starts over.  Changes conf.delta in place and sets conf.min_delta = conf.delta / 4: two rounds."""
    def f(eps):
        sc = wq.TopkSchedule(eps / 2.0, conf)
        return sc.push_rmax(sc.rmax(conf.delta / 4.0))
    for _ in range(4096):
        a, b = lo, hi
        assert f(a) < target < f(b)
        while float(np.nextafter(a, math.inf)) < b:
            mid = 0.5 * (a + b)
            if f(mid) < target:
                a = mid
            else:
                b = mid
        if f(b) == target:
            conf.min_delta = conf.delta / 4.0
            return b
        conf.delta = float(np.nextafter(conf.delta, math.inf))
    raise AssertionError("no eps gives the threshold %r exactly" % target)
