"""Designed input for the merged walk launch of the batched weighted top-k (kernels_weighted_topk_batch.hip:
k_w_walk_plan_multi) and the host model of the driver's lockstep that says which walk phases share a launch.

walk_design: one graph of disjoint parts, so that queries of very different sizes run in one call -
  a cycle of five and a pair u -> dead end (the toy graphs on which a weighted top-k round starts from an empty frontier
  and plans a single walk), a line that ends in a dead end, and a random part with dead ends.
launches(refs): weighted_topk_batch.cpp's loop for a call of q <= 16 queries that all start in driver round 0.  A query
  runs one level per driver round; the round after its frontier has emptied it plans and walks; the next round's first
  frontier is counted in that same driver round, so round j walks in driver round t_j = t_(j-1) + 1 + levels_j, t_0 =
  levels_0.  Returns {driver round: [(column, query round, walks)]}: the columns of each merged launch."""
import numpy as np

from conftest import edges_to_host

CYCLE0, PAIR0, LINE0, LINE_N, RAND0, RAND_N = 0, 5, 7, 6, 13, 180
CHAIN0, CHAIN_N = RAND0 + RAND_N, 10      # a chain c0 -> c1 -> ... -> the hub: a source further up reaches the hub later
HUB = CHAIN0 + CHAIN_N                    # the hub -> LEAVES leaves -> the hub: one residue entry per leaf
LEAVES = 2000
ALPHA, EPS, K, SEED = 0.5, 0.5, 2, 3


def walk_design(pkg):
    """(host, weights, parts): parts names the first node of every part."""
    edges = [(i, (i + 1) % 5) for i in range(5)]                       # cycle5
    edges += [(PAIR0, PAIR0 + 1)]                                        # two_node: 6 is a dead end
    edges += [(LINE0 + i, LINE0 + i + 1) for i in range(LINE_N - 1)]    # a line; its last node is a dead end
    rng = np.random.default_rng(11)
    for u in range(RAND0, RAND0 + RAND_N):
        if (u - RAND0) % 9 == 4:                                         # every ninth node of the random part: a dead end
            continue
        for v in rng.choice(RAND_N, size=int(rng.integers(1, 7)), replace=False):
            edges.append((u, RAND0 + int(v)))
    edges += [(CHAIN0 + i, CHAIN0 + i + 1) for i in range(CHAIN_N)]
    for leaf in range(HUB + 1, HUB + 1 + LEAVES):
        edges += [(HUB, leaf), (leaf, HUB)]
    n = HUB + 1 + LEAVES
    host = edges_to_host(pkg, n, edges)
    w = np.full(host.m, 2.0)
    src_of = np.repeat(np.arange(n), np.diff(host.out_rp.astype(np.int64)))
    rnd = (src_of >= RAND0) & (src_of < CHAIN0)
    w[rnd] = np.random.default_rng(12).uniform(0.5, 1.5, int(rnd.sum()))
    return host, w, dict(cycle=CYCLE0, pair=PAIR0, line=LINE0, rand=RAND0, chain=CHAIN0, hub=HUB)


def launches(refs):
    out = {}
    for c, ref in enumerate(refs):
        t = -1
        for j in range(ref["rounds"]):
            t += 1 + ref["round_levels"][j]
            out.setdefault(t, []).append((c, j, ref["walks_round"][j]))
    return out


def dead_end_starts(host, ref, j):
    """walks of round j of a query that start at a dead end (the plan holds such an entry)"""
    deg = np.diff(host.out_rp.astype(np.int64))
    return int(np.count_nonzero(deg[ref["starts"][j]] == 0))
