"""The designed All-Pair searches of tests/apbs_designed.py over relationship weights (helper of
test_weighted_apbs_designs.py and test_gpu_weighted_allpair.py; nothing here needs a device).

The gadgets and designs are apbs_designed's own.  The weights keep every value exact: in HostCsr.out_ci order an out-row
of degree d >= 2 (a power of two in those designs) alternates 0.5, 1.5, ..., so W = d and p = w / W is a short dyadic
rational; a row of degree 1 gets 2.0, so p = 1.  With alpha = 0.5 every residue and reserve stays a short dyadic
rational, every sum is exact in any order, and c * (w / W) equals (c * w) / W: a device result has to equal the
reference bit for bit on every tier.

`search_w` is the weighted form of apbs_designed.search - tests/weighted_bwd_ref.py: bpush_sync(..., "push") followed
by the unweighted emission rule - on `float` and on `fractions.Fraction`, with the same `Search` fields, so
apbs_designed.tiers / counters / index_of work on its results.

What the weights change.  p = 1 on every row of degree 1, and a source whose whole out-row lands on one level's frontier
of equal pending contributions receives (sum of w) / W = 1 times that contribution whatever the single weights are.  So:
  fans, routing, capf, colliders   every out-degree is 1: the weighted index IS the unweighted one, bit for bit;
  levels                           a source b_j sends all its d edges to the a_i of level 2, which all hold 0.25: b_j
                                   ends the level on 0.25 as without weights (the running sums on the way differ);
  hot                              a source's row is split between two targets and node 400: every source's reserve differs;
  crowd_small, crowd_large         a source's row is spread over its group's targets: a target at an even position of its
                                   group takes 0.25 / size from every source, one at an odd position 0.75 / size.  In the
                                   largest group the former stays below rmax (level 1 is the whole search), the latter
                                   crosses.  The crowds run at two thresholds (crowd_rmaxes): apbs_designed's own
                                   0.375 / size leaves the crossing sources a reserve EQUAL to rmax, which is emitted -
                                   ~400 000 entries, more than the record buffer holds, so searches wait for room and
                                   run again; at 0.5 / size the same sources cross, their reserve 0.375 / size stays
                                   below the threshold, the entries fit, and the counters are exact.
That equality is arithmetic, not a choice of this file; test_weighted_apbs_designs.py asserts each line of it."""
import numpy as np

import apbs_designed as ad


def exact_weights(G):
    """The weights of the module docstring, aligned with HostCsr(G.n, G.src, G.dst).out_ci (stable by source)."""
    perm = np.argsort(G.src, kind="stable")
    s = G.src[perm]
    first = np.concatenate([[0], np.cumsum(G.dout)])[s]          # a row's first position in out_ci order
    pos = np.arange(G.m) - first
    return np.where(G.dout[s] == 1, 2.0, np.where(pos % 2 == 0, 0.5, 1.5))


def uniform_weights(G, value=1.0):
    return np.full(G.m, float(value))


class Weighted:
    """G with weights `w` (out_ci order): per in-edge of G.in_ci the weight, per node W."""

    def __init__(self, G, w):
        w = np.asarray(w, dtype=np.float64)
        assert w.size == G.m
        self.G, self.w = G, w
        perm = np.argsort(G.src, kind="stable")                   # out_ci order -> edge-list index
        w_edge = np.empty(G.m)
        w_edge[perm] = w
        self.in_w = w_edge[np.argsort(G.dst, kind="stable")].tolist()   # aligned with G.in_ci
        self.W = np.bincount(G.src, weights=w_edge, minlength=G.n).tolist()
        # (sums of 0.5 / 1.5 / 2.0 over at most a few thousand edges: exact in any order)

    def inedges(self, v):
        lo, hi = int(self.G.in_rp[v]), int(self.G.in_rp[v + 1])
        return zip(self.G.in_ci[lo:hi].tolist(), self.in_w[lo:hi])


_weighted = {}


def weighted(G, w):
    key = (id(G), id(w))
    if key not in _weighted:
        _weighted[key] = (G, w, Weighted(G, w))                   # (G and w kept alive: their ids are the key)
    return _weighted[key][2]


def search_w(G, w, t, rmax, num=float, alpha=ad.ALPHA, keep=False):
    """apbs_designed.search with the deposit c(v) * p(e), p(e) = w(e) / W(u) formed once per edge (the device's record)."""
    X = w if isinstance(w, Weighted) else weighted(G, w)
    a, one, zero, rm = num(alpha), num(1), num(0), num(rmax)
    S = ad.Search()
    S.t, S.pops, S.pushes, S.frontiers, S.edges, S.touched_after = t, 0, 0, [], [], []
    S.ties_res = 0
    res, rsv = {}, {}
    if G.din[t] == 0:
        rsv[t] = one
        res[t] = zero
    else:
        res[t] = one
        frontier = [t]
        while frontier:
            pend = []
            for v in frontier:
                r = res[v]
                res[v] = zero
                rsv[v] = rsv.get(v, zero) + a * r
                pend.append((one - a) * r)
            start = {}
            E = 0
            for v, c in zip(frontier, pend):
                for u, we in X.inedges(v):
                    E += 1
                    old = res.get(u, zero)
                    if u not in start:
                        start[u] = old
                    nw = old + c * (num(we) / num(X.W[u]))
                    res[u] = nw
                    if nw == rm:
                        S.ties_res += 1
            S.pops += len(frontier)
            S.pushes += E
            S.frontiers.append(len(frontier))
            S.edges.append(E)
            S.touched_after.append(len(res))
            frontier = [u for u, old in start.items() if old <= rm and res[u] > rm]
    S.touched = len(res)
    S.entries = {u: r for u, r in rsv.items() if r > zero and r >= rm}
    S.ties_rsv = sum(1 for r in rsv.values() if r == rm)
    S.reserve, S.residue = (rsv, res) if keep else (None, None)
    return S


_w = {}
_runs = {}


def design_weights(name):
    """The exact weights of design `name`, made once."""
    if name not in _w:
        _w[name] = exact_weights(ad.design(name).G)
    return _w[name]


def run_w(name, lo, hi, rmax):
    """The float weighted searches of the targets [lo, hi) of a design, computed once and never changed."""
    key = (name, lo, hi, rmax)
    if key not in _runs:
        G = ad.design(name).G
        X = weighted(G, design_weights(name))
        _runs[key] = [search_w(G, X, t, rmax) for t in range(lo, hi)]
    return _runs[key]


# ------------------------------------------------------------------ what the device tests run
FAN_SIZES_GPU = [384, 385, 1536, 1537]                    # the give-up loads of the two tables
# modes of test_gpu_weighted_allpair.py: the hook switches of each; "whole" sends every target to the whole-vector pushes
MODES = {"default": {}, "tables": {"PPRHIP_APBS_DEG": "0,0"}, "large": {"PPRHIP_APBS_DEG": "1,0"},
         "dense": {"PPRHIP_APBS_TIER": "2"}, "whole": {"PPRHIP_APBS_TIER": "3"}}
COUNTER_MODES = ("default", "tables", "large", "dense")   # where apbs_designed.counters applies
RECORD_BUFFER_MIN = 65536                                 # the driver's record buffer holds at least this many entries


def crowd_positions(D):
    """target -> its position among its group's targets (= the position of its edge in every source's out-row)."""
    seen, pos = {}, {}
    for t in range(D.T):
        pos[t] = seen.get(D.kinds[t], 0)
        seen[D.kinds[t]] = pos[t] + 1
    return pos


def crowd_rmaxes(D):
    """The thresholds a crowd is queried at: apbs_designed's 0.375 / (largest group's size), at which the entries outgrow
    the record buffer, and 0.5 / (largest group's size), at which they fit (module docstring)."""
    big = max(s for _, s in D.kinds.values())
    return [D.rmaxes[0], 0.5 / big]


def crowd_claim_w(D, t, pos, rmax):
    """Weighted claim of a crowd's target: (touched, frontiers, E per level).  A source adds 0.5 * w / size with
    w = 0.5 at even positions of the group, 1.5 at odd ones."""
    N, size = D.kinds[t]
    add = 0.5 * (0.5 if pos % 2 == 0 else 1.5) / size
    crosses = add > rmax
    return (N, [1, N - 1], [N - 1, 0]) if crosses else (N, [1], [N - 1])


def gpu_cases(name):
    """(label, lo, hi, rmax) the device tests query design `name` at."""
    D = ad.design(name)
    if name == "fans":
        return [("fan%d" % N, D.targets["fan%d" % N], D.targets["fan%d" % N] + 1, r) for N in FAN_SIZES_GPU for r in D.rmaxes]
    if name == "levels":
        return [("two%d_%d" % fe, D.targets["two%d_%d" % fe], D.targets["two%d_%d" % fe] + 1, r)
                for fe in ad.TWO_LEVELS + ad.TWO_LEVELS_DENSE for r in D.rmaxes]
    if name == "hot":
        return [("hot%d" % t, t, t + 1, ad.R_HOT) for t in ad.HOT_TARGETS] + [("hot range", 0, 128, ad.R_HOT)]
    if name.startswith("crowd"):
        return [("all", 0, D.T, rmax) for rmax in crowd_rmaxes(D)]
    return [(label, lo, hi, rmax) for label, lo, hi, rmax, _ in ad.cases(D)]


# Game of Thrones with random weights: default_rng(GOT_W_SEED).uniform(0.5, 1.5, m) in HostCsr.out_ci order
GOT_W_SEED = 21
GOT_ALPHA = 0.15
GOT_THRESHOLDS = (1e-3, 1e-4)
GOT_MARGIN = 1e-6                                         # no compared value closer to the threshold (relative)

GPU_DESIGNS = ["fans", "levels", "routing", "capf", "colliders", "hot", "crowd_small", "crowd_large"]
