"""Designed graphs of the weighted backward kernels' tests (tests/test_gpu_weighted_backward.py), built by reversing the
edges of tests/weighted_designs.py; the properties they are built for are checked on the host lift in
tests/test_weighted_bwd_ref.py."""
import numpy as np

from conftest import edges_to_host
from weighted_designs import dense_design, sparse_design

CHUNK = 512    # out-edges a wave of the dense backward sweep owns (kChunkEdges)
STAGE = 512    # frontier entries the sparse kernel stages in LDS at a time (kWStage)
TILE = 2048    # in-edges per workgroup turn of the sparse kernel (kWTile)
FILL = 947     # out-degree of the filler row: 1 100 + 947 + 513 = 5 * 512


def _reversed_edges(host):
    src = np.repeat(np.arange(host.n), np.diff(host.out_rp.astype(np.int64)))
    return list(zip(host.out_ci[:host.m].astype(np.int64).tolist(), src.tolist()))


def reversed_dense_design(pkg):
    """dense_design with every edge reversed, plus one filler row.  A, B and C now have 512, 513 and 1 100 OUT-edges (to
    the pool, whose nodes become dead ends with one to three in-edges) and in-edges from small nodes.  The internal
    order puts the nodes with in-edges first, by out-degree descending: C, the filler Z (947 out-edges to the pool, one
    in-edge), B, A, then the small ones.  So the out-rows lie at
      C [0, 1 100): crosses two chunk boundaries;  Z [1 100, 2 047);
      B [2 047, 2 560): starts one edge before a boundary, crosses it and ends on the next;
      A [2 560, 3 072): exactly one chunk, boundary to boundary;
    and m is no multiple of 512.  Returns (host, dict of the named nodes)."""
    host, d = dense_design(pkg)
    edges = _reversed_edges(host)
    Z = host.n
    edges += [(Z, p) for p in d["pool"][:FILL]]
    edges.append((d["small"][1], Z))
    d = dict(d, Z=Z, dead=d["pool"][0], isolated=host.n - 1)
    return edges_to_host(pkg, host.n + 1, edges), d


def reversed_sparse_design(pkg, seed=9):
    """sparse_design with every edge reversed: targets of in-degree 1, 2, 3, 63, 64, 65, 1 500 and 2 500 (nodes 0 .. 7)
    over 3 000 nodes with a sparse rest.  Returns (host, {in-degree: node})."""
    host, by_deg = sparse_design(pkg, seed)
    return edges_to_host(pkg, host.n, _reversed_edges(host)), by_deg


def design_weights(host, seed):
    """Non-uniform weights in [0.5, 1.5)."""
    return np.random.default_rng(seed).uniform(0.5, 1.5, host.m)


# the pairs of the guarantee test on GOT: fixed inputs for which the numpy reference alone meets the guarantee
# (tests/test_weighted_bwd_ref.py pins that); w = ceil(omega * rmax) stays below 2 000 walks per pair
PAIR_EPS, PAIR_RMAX, PAIR_SEED, PAIR_W_SEED = 0.5, 0.0, 7, 21


def guarantee_pairs(host):
    """144 pairs: 12 sources x 12 targets drawn once, the hubs of either side among them."""
    rng = np.random.default_rng(3)
    outdeg = np.diff(host.out_rp.astype(np.int64))
    indeg = np.diff(host.in_rp.astype(np.int64))
    s = np.unique(np.concatenate([[int(np.argmax(outdeg))], rng.choice(host.n, 11, replace=False)]))
    t = np.unique(np.concatenate([[int(np.argmax(indeg))], rng.choice(host.n, 11, replace=False)]))
    ss, tt = np.meshgrid(s, t, indexing="ij")
    return ss.ravel().astype(np.int32), tt.ravel().astype(np.int32)
