"""Designed graphs, layout weights and numpy references (with mutants) for the batched WEIGHTED sweeps
(csrc/kernels_weighted_batch.hip: k_wbat_edges, k_wbat_apply, k_wbat_apply_extra, k_wbat_leave;
csrc/kernels_weighted_bwd_batch.hip: k_wbb_edges, k_wbb_apply, k_wbb_leave).  No device.

Both edge kernels are copies of k_dense_edges_b with a weight stream beside the index stream, so the positions that
make that kernel delicate are the same ones - lane groups of 128 edges in chunks of 512, row-start masks, the segmented
scan over the groups, the plain store against the atomic, the row left open at a chunk's end - and the layout inspector
and the designs of tests/batch_sweep_designs.py are used as they are:

  edges   E1-E7 of the unweighted module, on the forward side and (transposed) on the backward side
  small   fewer than 256 nodes, parallel relationships (a row keeps the multiset of its weights, in any assignment)
  tail    `edges` plus three nodes behind the isolated ones, each without in-edges and with one relationship to R7:
          m % 8 == 3 on both sides, and on the backward side three single-edge rows are the last three out-rows, inside
          the one lane whose eight edges straddle m (wbb_load_chunk's element-by-element path; out_w is not padded)

`blocks` is not needed: the weighted sweeps are plain Jacobi, they have no Gauss-Seidel blocks.  The weighted apply
kernels walk the rows with edges only (the forward rows without in-edges go through k_wbat_apply_extra), so the tile
features that mix both kinds of rows do not exist here; last_tile_skipped is the last tile of rows with edges.

Weights: uniform(0.5, 1.5) from a fixed seed per design and orientation, one per relationship, aligned with host.out_ci;
every edge has its own weight, so any mix-up moves a sum.  lifted_weights gives the weight of every lifted edge on either
side, as set_weights lays them out (csrc/weighted.cpp: build_weight_arrays).

The references, push_fwd_w and push_bwd_w, are the weighted Jacobi pulls of either direction as numpy level loops whose
row sums go over the inspected Side with the lifted weights: forward c = ((1 - alpha) r) / W, a term is c * w, dead-end
mass returns to the source (or lands on the seed set) - the rules of weighted_ref.push_sync and
weighted_query_ref.SeededPush; backward c = (1 - alpha) r, the sum is divided by W(u) once, strict threshold - the rules
of weighted_bwd_ref.bpush_sync.  A mutant reads the layout or its weights wrongly in one way (MUTANTS); MUTANT_CASES
names the design and direction that expose each; the queries are the ones the GPU file runs (forward_queries,
backward_queries, seed_set_queries, count_sources).

Not covered at these sizes: the grid-stride second trip of both edge kernels and of both apply kernels, which need
more than 4 096 chunks or about 260 000 rows (tests/test_gpu_scale.py runs graphs of that size), and the second trip
of k_wbat_leave, which needs a seed set of more than 16 384 live seeds without in-edges."""
import functools

import numpy as np

import batch_sweep_designs as D
import weighted_query_ref as wqr
import weighted_ref as wr
from batch_sweep_designs import CHUNK, GROUP, TILE

ALPHA = D.ALPHA
EPS = D.EPS
BWD_RMAX = D.BWD_RMAX
LANE_EDGES = 8  # edges a lane of the edge kernels loads
W_SEEDS = {("edges", False): 61, ("edges", True): 62, ("tail", False): 63, ("tail", True): 64, ("small", False): 65,
           ("small", True): 66}


# ------------------------------------------------------------------ designs
def tail_design():
    """`edges` and three more nodes behind its isolated ones: no in-edges, one relationship each, to R7.  m = 3 779."""
    e = D.all_designs()["edges"]
    new = [e.n, e.n + 1, e.n + 2]
    names = dict(e.names, new=new)
    edges = list(e.edges) + [(x, e.names["R7"]) for x in new]
    return D.Design("tail", e.n + 3, edges, names, list(e.sources) + [new[-1]])


@functools.lru_cache(maxsize=None)
def all_designs():
    d = D.all_designs()
    return {"edges": d["edges"], "small": d["small"], "tail": tail_design()}


def host_of(pkg, name, transposed=False):
    d = all_designs()[name]
    return d.transposed(pkg) if transposed else d.host(pkg)


def weights_of(host, name, transposed=False):
    """One weight per relationship, aligned with host.out_ci."""
    return np.random.default_rng(W_SEEDS[(name, transposed)]).uniform(0.5, 1.5, host.m)


def lifted_weights(host, lift, w):
    """(in_w, out_w): the weight of every edge of the lifted in-CSR and of the lifted out-CSR.  Out-rows move with their
    node and keep their order.  An in-row lists, by ascending internal source, the weights its sources' out-rows hold for
    it; parallel relationships take them in out-row order (a stable assignment: the row keeps the multiset)."""
    w = np.asarray(w, dtype=np.float64)
    new2old = lift["new2old"].astype(np.int64)
    lrp = lift["out_rp"].astype(np.int64)
    hrp = host.out_rp.astype(np.int64)
    deg = np.diff(lrp)
    within = np.arange(host.m, dtype=np.int64) - np.repeat(lrp[:-1], deg)
    out_w = w[np.repeat(hrp[new2old], deg) + within]
    out_src = np.repeat(np.arange(host.n, dtype=np.int64), deg)
    out_dst = lift["out_ci"][:host.m].astype(np.int64)
    in_row = np.repeat(np.arange(host.n, dtype=np.int64), np.diff(lift["in_rp"].astype(np.int64)))
    in_src = lift["in_ci"][:host.m].astype(np.int64)
    o_order = np.argsort(out_dst * host.n + out_src, kind="stable")
    i_order = np.argsort(in_row * host.n + in_src, kind="stable")
    assert np.array_equal(out_src[o_order], in_src[i_order]) and np.array_equal(out_dst[o_order], in_row[i_order])
    in_w = np.empty(host.m)
    in_w[i_order] = out_w[o_order]
    return in_w, out_w


# ------------------------------------------------------------------ the queries of the GPU tests
def forward_queries():
    """design -> sources of the forward batch (tests/test_gpu_weighted_batch_sweep_designs.py)."""
    return {name: list(d.sources) for name, d in all_designs().items()}


def count_sources():
    """33 sources of `edges` for the column-count cases, as the unweighted suite picks them."""
    d = all_designs()["edges"]
    nm = d.names
    cand = list(d.sources) + nm["pool"][3:9] + nm["pool"][1190:1196] + nm["T1"][1:4] + nm["H"][130:134] + nm["T0"][1:3]
    cand = cand[:33]
    assert len(cand) == 33 and len(set(cand)) == 33
    return cand


def seed_set_queries():
    """The 18 seed sets on `edges`, (ids, weights or None) in call order.  Pool nodes are live seeds without in-edges:
    rows outside the sweep, which k_wbat_apply_extra walks 256 at a time with one workgroup per column and k_wbat_leave
    clears in both arrays.  The two sets of 600 (three trips of that loop) come first and finish first (the CPU test pins
    that), so the first one's column is taken over by the single member that follows the sixteenth query; the set of
    dead ends, which finishes at once, comes last."""
    nm = all_designs()["edges"].names
    pool, T0 = nm["pool"], nm["T0"]
    rng = np.random.default_rng(77)
    big = [pool[i] for i in range(0, 1200, 2)]
    big2 = [pool[i] for i in range(1, 1200, 2)]
    mix = [pool[i] for i in range(0, 1200, 4)] + T0[:5] + [nm["hub"], nm["a"], nm["R7"], nm["H"][200]]
    sets = [(big, rng.uniform(0.2, 1.0, 600)), (big2, rng.uniform(0.2, 1.0, 600)), (mix, rng.uniform(0.2, 1.0, len(mix))),
            ([pool[29]], None), ([nm["hub"], nm["f"]], [2.0, 1.0]), ([pool[0], pool[1199]], None), ([nm["R7"]], None),
            ([nm["extra"][-1], nm["last_row"], nm["hub"]], [1.0, 2.0, 3.0]), ([pool[700], nm["extra"][0], nm["f"]], None),
            ([pool[199]], None), ([nm["c"], nm["d"], T0[3]], [0.5, 0.25, 0.25]), ([pool[511]], None),
            ([nm["e"], pool[2]], None), ([nm["b"], nm["T1"][3], nm["dead"]], None), ([nm["T1"][5]], None),
            ([nm["hub"]], None),
            ([pool[7]], None), (T0[3:8], [1.0, 2.0, 3.0, 4.0, 5.0])]
    assert len(sets) == 18 and len(big) == 600 and len(mix) == 309
    return [(list(ids), None if sw is None else [float(x) for x in sw]) for ids, sw in sets]


def backward_queries():
    """(design, transposed, targets, sets, rmax): the backward batches.  Targets of D.backward_cases(); on tail (its
    out-rows end with the three single-edge rows that gather R7) R7 and a dead end; on tail^T R7, the last new node (a
    dead end there) and the last row; `sets`: (ids, weights) target sets whose members include nodes without
    out-edges."""
    by = {(n, t): list(tg) for n, t, tg in D.backward_cases() if n != "blocks"}
    e, s = all_designs()["tail"].names, all_designs()["small"].names
    out = [("edges", False, by[("edges", False)], [(e["T0"][:6] + [e["R7"], e["hub"]], [1.0, 0.5, 0.25, 2.0, 1.0, 0.75, 1.5, 0.3])]),
           ("edges", True, by[("edges", True)], [(e["pool"][:5] + [e["hub"]], [1.0, 0.5, 2.0, 0.25, 1.0, 0.5])]),
           ("tail", False, [e["R7"], e["last_row"], e["dead"], e["f"]], []),
           ("tail", True, [e["R7"], e["new"][-1], e["last_row"], e["pool"][0], e["pool"][700], e["hub"]],
            [(e["new"] + [e["pool"][29]], [1.0, 2.0, 0.5, 1.0])]),
           ("small", False, by[("small", False)], [(s["dead"][:4] + [64], [1.0, 1.0, 0.5, 2.0, 1.0])]),
           ("small", True, by[("small", True)], [(s["pool"][:4] + [1], [1.0, 0.5, 2.0, 1.0, 1.0])])]
    return [(n, t, tg, sets, BWD_RMAX) for n, t, tg, sets in out]


def fora_rmax(host, alpha=ALPHA, eps=EPS):
    """The push threshold of a weighted whole-graph FORA query."""
    return wr.whole_params(host.n, host.m, alpha, eps)[0]


# ------------------------------------------------------------------ numpy references through the layout
KEPT = ("later_group", "later_chunk", "startless_chunk", "cross_rows_not_cleared", "last_tile_skipped")
WEIGHT_MUTANTS = ("weight_of_next_edge", "weight_from_group_0", "weight_of_lanes_first_edge", "pad_weight_one")
BWD_ONLY = ("tail_lane_weights_zero", "tail_lane_reads_on", "leave_skipped")
FWD_ONLY = ("extra_rows_skipped",)
MUTANTS = tuple([(m, d) for m in KEPT + WEIGHT_MUTANTS for d in ("fwd", "bwd")] + [(m, "bwd") for m in BWD_ONLY] +
                [(m, "fwd") for m in FWD_ONLY])

# (mutant, direction) -> (design, transposed): the graph whose queries of that direction expose it
MUTANT_CASES = {
    ("later_group", "fwd"): ("edges", False), ("later_group", "bwd"): ("edges", True),
    ("later_chunk", "fwd"): ("edges", False), ("later_chunk", "bwd"): ("edges", True),
    ("startless_chunk", "fwd"): ("edges", False), ("startless_chunk", "bwd"): ("edges", True),
    ("cross_rows_not_cleared", "fwd"): ("edges", False), ("cross_rows_not_cleared", "bwd"): ("edges", True),
    ("last_tile_skipped", "fwd"): ("small", False), ("last_tile_skipped", "bwd"): ("small", True),
    ("weight_of_next_edge", "fwd"): ("edges", False), ("weight_of_next_edge", "bwd"): ("edges", True),
    ("weight_from_group_0", "fwd"): ("edges", False), ("weight_from_group_0", "bwd"): ("edges", True),
    ("weight_of_lanes_first_edge", "fwd"): ("edges", False), ("weight_of_lanes_first_edge", "bwd"): ("edges", True),
    ("pad_weight_one", "fwd"): ("edges", False), ("pad_weight_one", "bwd"): ("edges", False),
    ("tail_lane_weights_zero", "bwd"): ("tail", False), ("tail_lane_reads_on", "bwd"): ("tail", False),
    ("leave_skipped", "bwd"): ("edges", False), ("extra_rows_skipped", "fwd"): ("edges", False),
}


class _Gather:
    """Row sums of one sweep over the inspected side `s` with the lifted weights `wl`: term = c[source] * w(e)."""

    def __init__(self, s, wl, mutant):
        self.s, self.mutant = s, mutant
        e = np.arange(s.m)
        self.src = s.new2old[s.ci]                 # original id of the vertex every edge gathers
        self.rows_old = s.new2old[s.rows]
        self.keep = np.ones(s.m, dtype=bool)
        w = np.array(wl[:s.m], dtype=np.float64)
        if mutant == "later_group":
            self.keep = e // GROUP == s.first[s.row_of_edge] // GROUP
        elif mutant == "later_chunk":
            self.keep = e // CHUNK == s.first_chunk[s.row_of_edge]
        elif mutant == "startless_chunk":
            self.keep = s.group_starts.sum(axis=1)[e // CHUNK] > 0
        elif mutant == "weight_of_next_edge":
            w = np.append(w[1:], 0.0)              # (behind m: the padding's 0.0)
        elif mutant == "weight_from_group_0":
            w = w[e - GROUP * ((e % CHUNK) // GROUP)]
        elif mutant == "weight_of_lanes_first_edge":
            w = w[e - e % LANE_EDGES]
        elif mutant == "tail_lane_weights_zero":
            w[LANE_EDGES * (s.m // LANE_EDGES):] = 0.0
        elif mutant == "tail_lane_reads_on":
            t = LANE_EDGES * (s.m // LANE_EDGES)
            w[t:] = w[t - LANE_EDGES:s.m - LANE_EDGES]
        self.w = w
        self.stale = np.zeros(s.n_nz)
        self.skip = np.zeros(0, dtype=np.int64)    # rows (original ids) the apply pass does not visit
        if mutant == "last_tile_skipped":
            self.skip = self.rows_old[(s.n_nz - 1) // TILE * TILE:]

    def sums(self, c):
        """c over original ids -> the row sums over original ids (rows without edges: 0)."""
        s = self.s
        val = c[self.src] * self.w
        acc = np.bincount(s.row_of_edge, weights=np.where(self.keep, val, 0.0), minlength=s.n_nz)
        if self.mutant == "pad_weight_one":
            acc[-1] += s.pad * (c[s.new2old[0]] * 1.0)
        if self.mutant == "cross_rows_not_cleared":
            acc += np.where(s.cross, self.stale, 0.0)
            self.stale = acc.copy()
        full = np.zeros(s.n)
        full[self.rows_old] = acc
        full[self.skip] = 0.0
        return full


def _dist(x, rmax):
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    return float(np.min(np.abs(x - rmax) / rmax)) if x.size and rmax > 0 else np.inf


def push_fwd_w(host, w, side, wl, alpha, rmax, src=None, seeds=None, sw=None, mutant=None, max_levels=400):
    """The weighted forward push from `src` (weighted_ref.push_sync) or from the seed set (seeds, sw)
    (weighted_query_ref.push_sync_seeds) where every level is a pull over the forward side.  A mutant may never come to
    rest: the push stops after max_levels.
    Returns (reserve, residue, levels, pops, margin): margin is the smallest |r / d - rmax| / rmax over every value the
    run compared with the threshold (inf when it compared none)."""
    n = host.n
    _, W = wr.table(host, w)
    deg = np.diff(host.out_rp.astype(np.int64))
    indeg = np.diff(host.in_rp.astype(np.int64))
    reserve, residue = np.zeros(n), np.zeros(n)
    margin = np.inf
    if seeds is None:
        if deg[src] == 0:
            reserve[src] = 1.0
            return reserve, residue, 0, 0, margin
        residue[src] = 1.0
        F = np.array([src], dtype=np.int64)
        live, q, dead_seeds, e_dead = np.array([src]), np.ones(1), np.zeros(0, dtype=np.int64), np.zeros(0)
    else:
        t = wqr.SeedTable(host, seeds, sw, alpha)
        residue[t.live] = t.q
        reserve[t.dead] = t.e
        F = t.live
        live, q, dead_seeds, e_dead = t.live, t.q, t.dead, t.e
    G = _Gather(side, wl, mutant)
    extra = live[indeg[live] == 0]  # the rows outside the sweep a column visits
    levels = pops = 0
    while F.size and levels < max_levels:
        levels += 1
        pops += int(F.size)
        rc = residue[F].copy()
        residue[F] = 0.0
        reserve[F] = reserve[F] + rc * alpha
        dead = deg[F] == 0
        x = float((rc[dead] * (1.0 - alpha)).sum())
        c = np.zeros(n)
        c[F[~dead]] = ((1.0 - alpha) * rc[~dead]) / W[F[~dead]]
        a = G.sums(c)
        if x > 0.0:
            a[live] = a[live] + x * q
            reserve[dead_seeds] = reserve[dead_seeds] + x * e_dead
        if mutant == "extra_rows_skipped":
            a[extra] = 0.0
        a[G.skip] = 0.0
        old = residue.copy()
        residue = old + a
        got = np.flatnonzero(residue != old)
        live_got = got[deg[got] > 0]
        if live_got.size:
            margin = min(margin, _dist(old[live_got] / deg[live_got], rmax), _dist(residue[live_got] / deg[live_got], rmax))
        F = got[~wr.active(old[got], deg[got], rmax) & wr.active(residue[got], deg[got], rmax)]
    return reserve, residue, levels, pops, margin


def push_bwd_w(host, w, side, wl, ids, weights, alpha, rmax, mutant=None, max_levels=400):
    """The weighted backward push with the start of targets and pairs (weighted_bwd_ref.bpush_sync, rule "pair") where
    every level is a pull over the backward side: a row sums c(v) * w(e) over its out-edges and takes the sum divided by
    W(u) once; strict threshold.  Returns (reserve, residue, levels, pops, margin) as bpush_sync does."""
    import weighted_bwd_ref as br
    n = host.n
    _, W = wr.table(host, w)
    deg = np.diff(host.out_rp.astype(np.int64))
    indeg = np.diff(host.in_rp.astype(np.int64))
    reserve, residue = np.zeros(n), np.zeros(n)
    margin = np.inf
    mid, mw = br.merge_set(ids, weights)
    if mid.size == 1 and mw[0] == 1.0:
        t = int(mid[0])
        if indeg[t] == 0:
            reserve[t] = alpha
            return reserve, residue, 0, 0, margin
        residue[t] = 1.0
        F = np.array([t], dtype=np.int64)
    else:
        lone = indeg[mid] == 0
        reserve[mid[lone]] = mw[lone] * alpha
        residue[mid[~lone]] = mw[~lone]
        margin = min(margin, _dist(mw[~lone], rmax))
        F = mid[~lone][mw[~lone] > rmax]
    G = _Gather(side, wl, mutant)
    Wd = np.where(deg > 0, W, 1.0)
    ghost = np.zeros(n)
    levels = pops = 0
    while F.size and levels < max_levels:
        rc = residue[F].copy()
        residue[F] = 0.0
        reserve[F] = reserve[F] + rc * alpha
        c = np.zeros(n)
        c[F] = (1.0 - alpha) * rc
        if mutant == "leave_skipped":  # the scattered members without out-edges stay in the array the even sweeps read
            if levels == 0:
                ghost = np.where(deg == 0, c, 0.0)
            elif levels % 2 == 0:
                c = c + ghost
        levels += 1
        pops += int(F.size)
        acc = G.sums(c)
        old = residue.copy()
        residue = old + acc / Wd
        got = np.flatnonzero(residue != old)
        if got.size:
            margin = min(margin, _dist(old[got], rmax), _dist(residue[got], rmax))
        F = got[~(old[got] > rmax) & (residue[got] > rmax)]
    return reserve, residue, levels, pops, margin
