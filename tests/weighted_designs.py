"""Designed graphs of the weighted kernels' tests (tests/test_gpu_weighted.py); the properties they are built for are
checked on the host lift in tests/test_weighted_ref.py."""
import numpy as np

from conftest import edges_to_host

CHUNK = 512  # in-edges a wave of the dense sweep owns


def dense_design(pkg):
    """In-rows at the chunk edges of the dense pull sweep.  The internal order puts the nodes with in-edges first, by
    out-degree descending, so the in-rows lie in the order A, B, C, then the small ones:
      A (out-degree 6): 512 in-edges, the edges [0, 512) - B's row starts exactly on a chunk boundary;
      B (out-degree 5): 513 in-edges, [512, 1025) - crosses one boundary;
      C (out-degree 4): 1 100 in-edges, [1025, 2125) - crosses two;
      30 small nodes with out-degree 0 .. 2 (dead ends among them), a few parallel relationships and a self loop.
    The in-edges come from a pool of 1 100 nodes that nobody points to (rows without in-edges that have out-edges).
    m is no multiple of 512: the last chunk holds fewer than 512 edges.  Returns (host, dict of the named nodes)."""
    A, B, C = 0, 1, 2
    small = list(range(3, 33))
    pool = list(range(33, 33 + 1100))
    n = pool[-1] + 1 + 2  # two isolated nodes behind the pool
    edges = []
    for i, p in enumerate(pool):
        if i < 512:
            edges.append((p, A))
        if i < 513:
            edges.append((p, B))
        edges.append((p, C))
    edges += [(A, s) for s in small[:6]]
    edges += [(B, s) for s in small[6:11]]
    edges += [(C, s) for s in small[11:15]]
    for k, s in enumerate(small):  # out-degree k % 3: dead ends, single and double rows; parallel pairs, one self loop
        d = k % 3
        if d >= 1:
            edges.append((s, small[(k + 7) % len(small)]))
        if d == 2:
            edges.append((s, small[(k + 7) % len(small)] if k % 2 else s))
    host = edges_to_host(pkg, n, edges)
    return host, dict(A=A, B=B, C=C, small=small, pool=pool, dead=small[0], isolated=n - 1)


def sparse_design(pkg, seed=9):
    """Sources of out-degree 1, 2, 3, 63, 64, 65, 1 500 and 2 500 (rows 0 .. 7) over 3 000 nodes with a sparse random
    rest (out-degree 0 .. 4, dead ends among them).  Returns (host, {degree: node})."""
    rng = np.random.default_rng(seed)
    n = 3000
    degs = [1, 2, 3, 63, 64, 65, 1500, 2500]
    edges = []
    for u, d in enumerate(degs):
        edges += [(u, int(v)) for v in rng.integers(8, n, d)]
    for u in range(8, n):
        edges += [(u, int(v)) for v in rng.integers(0, n, rng.integers(0, 5))]
    return edges_to_host(pkg, n, edges), {d: u for u, d in enumerate(degs)}
