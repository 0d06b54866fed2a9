"""Designed graphs for the sweep cut (csrc/kernels_sweep.hip: k_sweep_support, k_sweep_rank, k_sweep_tile_starts,
k_sweep_edges, k_sweep_best; csrc/sweep.cpp).  Helper of test_sweep_cut_designs.py (CPU) and
test_gpu_sweep_cut_designs.py; nothing in this file needs a device.

`slot_layout` is a plain numpy model of what k_sweep_edges sees: the profiled nodes' adjacencies (out-row, then in-row)
laid end to end in profile order and cut into tiles of SWEEP_TILE slots.  Every design states the edge it is built for
as a predicate over that layout (FEATURES), evaluated on the order tests/sweep_ref.py derives from a vector: the CPU
test evaluates it on the oracle twin's vector, the GPU test on the vector the handle returns.  A design whose vector
does not put it there fails; nothing passes vacuously.

Family A, dead-end sinks.  A few source nodes without in-edges point with parallel edges at sinks without out-edges; the
sinks are the seed set.  A dead-end seed keeps its mass (seed sets), so the vector is the normalized weights
and the push runs no level.  Weights deg * (2k - position) (normalize: the score is x / deg) or 2k - position make the
profile any chosen permutation of the ids, and vol the running sum of a degree sequence that is written down.  Every
slot of a sink names an unranked source: +1, so cut == vol, and a slot counted for the wrong node shows at that position.

Family B, feeder padding.  A graph without dead ends (communities, three hubs, self loops on a hub, parallel
relationships, every relationship with its reverse but for a gadget of two nodes with one-slot rows) is pushed from a
seed set to rmax 1e-12.  In-edges from an unseeded feeder without in-edges change no push; they lengthen the in-row of
the node they point to and shift every later node in slot space.  `_solve` pads one node so that a measured slot lands
on a wanted offset; the order comes from the twin's vector of the unpadded graph (the padded graph's is the same bit
for bit under one level schedule and within the push's own error under the library's, which picks a level's shape by
the edge count; the CPU test checks both, and the features are proved on the padded graph's own vector).
normalize = False leaves the order alone, normalize = True moves the padded node only, so a design is solved for one
value of normalize and claims its feature for that value.

The constant is restated from csrc/engine.hpp (kSweepTile); test_sweep_cut_designs.py checks it against the header."""
import functools

import numpy as np

from sweep_ref import degrees, sweep_ref

SWEEP_TILE = 4096          # kSweepTile (csrc/engine.hpp): adjacency slots one workgroup turn of k_sweep_edges covers
SWEEP_THREADS = 256        # a turn's lane l takes the slots l, l + 256, ... of its tile
ALPHA = 0.15
RMAX = 1e-12
T = SWEEP_TILE


# ------------------------------------------------------------------ the slot space
class Tile:
    """One tile of the slot space.  first / count: the profile positions it touches (k_sweep_edges' i0 and cnt);
    first_crosses / last_crosses: its first node began in an earlier tile / its last node ends in a later one; starts[j]:
    the first slot of node first + j relative to the tile (negative where the node began before it; the kernel keeps
    max(., 0)); splits[j]: the relative slot at which that node's out-row ends and its in-row begins; slots: how many
    slots the tile holds (the last tile may be short)."""
    __slots__ = ("t", "first", "count", "first_crosses", "last_crosses", "starts", "splits", "slots")


def slot_layout(order, d_out, d_in, tile=SWEEP_TILE):
    """The tiles of the profile `order` (node ids) over the degrees d_out / d_in (by node id)."""
    order = np.asarray(order, dtype=np.int64)
    do, di = np.asarray(d_out, dtype=np.int64)[order], np.asarray(d_in, dtype=np.int64)[order]
    volx = np.concatenate([[0], np.cumsum(do + di)])
    total = int(volx[-1])
    out = []
    for t in range((total + tile - 1) // tile):
        t0, t1 = t * tile, min((t + 1) * tile, total)
        L = Tile()
        L.t, L.slots = t, t1 - t0
        L.first = int(np.searchsorted(volx, t0, side="right")) - 1        # the largest i with volx[i] <= t0
        last = int(np.searchsorted(volx, t1 - 1, side="right")) - 1       # the node that holds slot t1 - 1
        L.count = last - L.first + 1
        L.first_crosses = bool(volx[L.first] < t0)
        L.last_crosses = bool(volx[last + 1] > t1)
        L.starts = volx[L.first:last + 1] - t0
        L.splits = L.starts + do[L.first:last + 1]
        out.append(L)
    return out


def slot_nodes(order, d_out, d_in):
    """Brute force: the profile position that owns every slot, and whether the slot lies in the node's in-row."""
    order = np.asarray(order, dtype=np.int64)
    do, di = np.asarray(d_out, dtype=np.int64)[order], np.asarray(d_in, dtype=np.int64)[order]
    pos = np.repeat(np.arange(order.size), do + di)
    first = np.concatenate([[0], np.cumsum(do + di)])[:-1]
    return pos, (np.arange(pos.size) - first[pos]) >= do[pos]


class View:
    """A vector's profile on a design, for the feature predicates: ref (sweep_ref's dict), deg and volx by position,
    tiles (slot_layout), rank by node id (-1: not profiled), normalize (the value the profile was ordered with)."""

    def __init__(self, d, x, normalize, **kw):
        self.d, self.x, self.normalize = d, np.asarray(x, dtype=np.float64), bool(normalize)
        self.ref = sweep_ref(d.n, d.src, d.dst, x, normalize=int(normalize), **kw)
        self.order = self.ref["order"].astype(np.int64)
        self.deg = (d.d_out + d.d_in)[self.order]
        self.volx = np.concatenate([[0], np.cumsum(self.deg)])
        self.total = int(self.volx[-1])
        self.tiles = slot_layout(self.order, d.d_out, d.d_in)
        self.rank = np.full(d.n, -1, dtype=np.int64)
        self.rank[self.order] = np.arange(self.order.size)

    def split_of(self, v):
        """The slot at which ranked node v's in-row begins."""
        return int(self.volx[self.rank[v]] + self.d.d_out[v])


# ------------------------------------------------------------------ features
def _start_at(off):
    return lambda V: bool(np.any(V.volx[1:-1] % T == off))      # (not the first node: slot 0 is no edge)


def _end_at(off):
    def f(V):
        end = V.volx[1:]
        if off == T + 1:   # one slot into the next tile
            return bool(np.any((end % T == 1) & (V.deg >= 2)))
        return bool(np.any(end % T == off % T))
    return f


def _hub(aligned):
    def f(V):
        s, e = V.volx[:-1], V.volx[1:]
        if aligned:
            return bool(np.any((s % T == 0) & (e % T == 0) & (V.deg >= 3 * T)))
        return bool(np.any((s % T == T - 1) & (e % T == 1) & (V.deg >= 3 * T + 2)))
    return f


def _tail_smalls_head(V):
    for L in V.tiles:
        if L.first_crosses and L.last_crosses and L.count >= 302 and L.starts[1] >= 64 and L.starts[-1] <= T - 64:
            inner = V.deg[L.first + 1:L.first + L.count - 1]
            if inner.max() <= 17 and V.deg[L.first] >= T and V.deg[L.first + L.count - 1] >= T:
                return True
    return False


def _run_changes_node(V):
    """Some lane's sixteen slots of one tile belong to three or more nodes: its run accumulator is flushed in between."""
    pos, _ = slot_nodes(V.order, V.d.d_out, V.d.d_in)
    for L in V.tiles:
        if L.slots == T:
            p = pos[L.t * T:(L.t + 1) * T].reshape(T // SWEEP_THREADS, SWEEP_THREADS)
            if np.any((np.diff(p, axis=0) != 0).sum(axis=0) >= 2):
                return True
    return False


def _wave_on_one_node_beside_others(V):
    """A tile of more than one node in which the 64 lanes of some wave all end on one node (the wave path) while another
    wave's lanes end on different nodes (the per-lane path)."""
    pos, _ = slot_nodes(V.order, V.d.d_out, V.d.d_in)
    for L in V.tiles:
        if L.slots == T and L.count > 1:
            last = pos[(L.t + 1) * T - SWEEP_THREADS:(L.t + 1) * T].reshape(4, 64)
            one = (last == last[:, :1]).all(axis=1)
            if one.any() and not one.all():
                return True
    return False


def _total(f):
    return lambda V: bool(f(V.total))


def _denormal(V):
    """Forty ranked nodes hold a denormal; equal scores among them; under normalize some scores round to 0, some do not."""
    x = V.x[V.order]
    tiny = (x > 0) & (x < 2.3e-308)
    score = (x / V.deg if V.normalize else x)[tiny]
    if tiny.sum() != 40 or x[0] != 1.0 or np.unique(score).size >= score.size or not np.any(score > 0):
        return False
    return bool(np.any(score == 0)) if V.normalize else True


def _split_at(off):
    def f(V):
        h = V.d.hub
        loops = int(np.count_nonzero((V.d.src == h) & (V.d.dst == h)))
        return V.rank[h] >= 0 and loops >= 2 and V.split_of(h) % T == off and V.d.d_out[h] > 2 and V.d.d_in[h] > 2
    return f


def _edge_slots(V):
    """The two slots of the relationship a -> b of the gadget: a's out-row and b's in-row are one slot each."""
    a, b = V.d.gadget
    assert V.d.d_out[a] == 1 and V.d.d_in[b] == 1
    return int(V.volx[V.rank[a]]), V.split_of(b)


def _edge(kind):
    def f(V):
        if min(V.rank[list(V.d.gadget)]) < 0:
            return False
        sa, sb = _edge_slots(V)
        if kind == "apart":
            return sa // T != sb // T
        if sa // T != sb // T:
            return False
        same_lane = sa % SWEEP_THREADS == sb % SWEEP_THREADS
        return same_lane if kind == "lane" else not same_lane
    return f


def _scanned(off):
    """max_size = d.cut_size ends the scanned slots on, one before and one behind a tile boundary."""
    return lambda V: V.d.cut_size is not None and V.d.cut_size < V.ref["support"] and \
        int(V.volx[V.d.cut_size]) % T == off and int(V.volx[V.d.cut_size]) > T


def _ties(V):
    """The least conductance (0) is taken by several hundred prefixes in different threads, waves and workgroups of
    k_sweep_best, and by none of the first 256."""
    r = V.ref
    vol = r["vol"].astype(np.int64)
    den = np.minimum(vol, r["total_vol"] - vol)
    at = np.nonzero((r["cut"] == 0) & (den > 0))[0]
    return at.size >= 300 and at[0] >= 512 and r["best_size"] == at[0] + 1 and r["best_conductance"] == 0.0 and \
        np.unique(at // 256).size >= 3 and np.unique(at % 256 // 64).size == 4 and np.unique(at % 256).size >= 100


FEATURES = {
    "A_tile_of_4096_nodes_aligned": lambda V: any(L.count == T and not L.first_crosses for L in V.tiles),
    "A_tile_of_4096_nodes_behind_a_hub_tail": lambda V: any(L.count == T and L.first_crosses for L in V.tiles),
    "A_start_at_0": _start_at(0), "A_start_at_1": _start_at(1), "A_start_at_T_minus_1": _start_at(T - 1),
    "A_end_at_T": _end_at(T), "A_end_at_T_minus_1": _end_at(T - 1), "A_end_at_T_plus_1": _end_at(T + 1),
    "A_hub_over_3_tiles_aligned": _hub(True), "A_hub_over_3_tiles_off_by_1_at_both_ends": _hub(False),
    "A_tile_inside_one_node": lambda V: any(L.count == 1 and L.first_crosses and L.last_crosses for L in V.tiles),
    "A_tail_smalls_head": _tail_smalls_head,
    "A_run_changes_node": _run_changes_node,
    "A_wave_path_beside_lane_path": _wave_on_one_node_beside_others,
    "A_degrees_256_257_in_a_row": lambda V: bool(np.any((V.deg[:-1] == 256) & (V.deg[1:] == 257))),
    "A_7_tiles": lambda V: len(V.tiles) >= 7,
    "A_total_1": _total(lambda s: s == 1), "A_total_T_minus_1": _total(lambda s: s == T - 1),
    "A_total_T": _total(lambda s: s == T), "A_total_T_plus_1": _total(lambda s: s == T + 1),
    "A_total_kT": _total(lambda s: s % T == 0 and s >= 2 * T),
    "A_total_kT_plus_1": _total(lambda s: s % T == 1 and s >= 2 * T),
    "A_denormal_scores": _denormal,
    "B_hub_split_at_0": _split_at(0), "B_hub_split_at_1": _split_at(1), "B_hub_split_at_T_minus_1": _split_at(T - 1),
    "B_edge_in_one_lane": _edge("lane"), "B_edge_in_one_tile": _edge("tile"), "B_edge_in_two_tiles": _edge("apart"),
    "B_scanned_kT_minus_1": _scanned(T - 1), "B_scanned_kT": _scanned(0), "B_scanned_kT_plus_1": _scanned(1),
    "C_best_prefix_ties": _ties,
}


# ------------------------------------------------------------------ designs
class Design:
    """A graph (n, src, dst), a seed set with weights (by the value of normalize the sweep will run with), the features
    it claims, and the values of normalize it claims them for."""
    hub = gadget = cut_size = None

    def __init__(self, name, n, src, dst, seeds, weights, claims, normalizes=(True, False)):
        self.name, self.n, self.claims, self.normalizes = name, int(n), list(claims), tuple(normalizes)
        self.src, self.dst = np.asarray(src, dtype=np.int32), np.asarray(dst, dtype=np.int32)
        self.m = int(self.src.size)
        self.seeds = np.asarray(seeds, dtype=np.int32)
        self._weights = weights
        self.d_out = np.bincount(self.src, minlength=self.n).astype(np.int64)
        self.d_in = np.bincount(self.dst, minlength=self.n).astype(np.int64)
        assert np.array_equal(self.d_out + self.d_in, degrees(self.n, self.src, self.dst))

    def __repr__(self):
        return self.name

    def weights(self, normalize):
        w = self._weights(bool(normalize)) if callable(self._weights) else self._weights
        return np.asarray(w, dtype=np.float64)

    def host(self, pkg):
        return pkg.HostCsr(self.n, self.src, self.dst)

    def view(self, x, normalize, **kw):
        return View(self, x, normalize, **kw)

    def prove(self, x, normalize):
        """Every claimed feature is present in the profile of x; returns the view."""
        V = self.view(x, normalize)
        assert self.claims, self
        for f in self.claims:
            assert FEATURES[f](V), "%s misses %s (normalize %s): %d nodes, %d slots" % (self, f, normalize, V.order.size,
                                                                                        V.total)
        return V


# ---------------------------------- family A
N_SOURCES = 3


def sinks(name, degs, claims, weights=None, seed=1):
    """Sinks of in-degree degs[i] at profile position i, their ids shuffled; the sources' edges in turn."""
    degs = np.asarray(degs, dtype=np.int64)
    k = int(degs.size)
    n_src = N_SOURCES
    while (k + n_src) % 256 == 0:
        n_src += 1
    ids = n_src + np.random.default_rng(seed).permutation(k)
    dst = np.repeat(ids, degs)
    src = np.arange(dst.size) % n_src
    if weights is None:
        level = (2 * k - np.arange(k)).astype(np.float64)
        weights = lambda normalize: level * degs if normalize else level
    d = Design(name, k + n_src, src, dst, ids, weights, claims)
    d.degs = degs
    return d


def _smalls(count):
    return [(1, 2, 3, 5, 7, 16, 17)[i % 7] for i in range(count)]


def _fill(degs, total):
    left = total - sum(degs)
    assert left >= 0
    return list(degs) + [3] * (left // 3) + [1] * (left % 3)


def sinks_denormal():
    """x = 1 on one sink and 1 to 4 times the smallest denormal on forty more, of degrees 1 to 5: x / deg rounds to 0 or to
    a denormal, and many scores are equal (order by id)."""
    degs = [1] + [1 + (j // 4) % 5 for j in range(40)]
    w = [1.0] + [(1 + j % 4) * 5e-324 for j in range(40)]
    return sinks("a_denormal", degs, ["A_denormal_scores"], weights=w, seed=3)


# ---------------------------------- family B
class Base:
    """The unpadded graph of family B."""

    def __init__(self):
        rng = np.random.default_rng(20)
        comms, size = 12, 120
        nc = comms * size
        a, b = [], []

        def both(u, v):
            a.extend([u, v])
            b.extend([v, u])

        for c in range(comms):
            lo = c * size
            for i in range(size):
                both(lo + i, lo + (i + 1) % size)
                for j in rng.choice(size, 4, replace=False):
                    if j != i:
                        both(lo + i, lo + int(j))
            for i in range(4):
                both(lo + 7 * i, (lo + size + 11 * i) % nc)
        for u in range(40):               # parallel relationships
            both(u, (u + 1) % size)
        hubs = [nc, nc + 1, nc + 2]
        for h, fan in zip(hubs, (500, 300, 200)):
            for v in rng.choice(nc, fan, replace=False):
                both(h, int(v))
        self.hub = hubs[0]
        a += [self.hub, self.hub]        # two self loops: a slot each in the hub's out-row and in its in-row
        b += [self.hub, self.hub]
        ga, gb = nc + 3, nc + 4          # the gadget: hub -> ga -> gb -> hub; ga's out-row and gb's in-row are one slot
        a += [self.hub, ga, gb]
        b += [ga, gb, self.hub]
        self.gadget = (ga, gb)
        self.n = nc + 5
        self.feeders = (self.n, self.n + 1)
        self.src, self.dst = np.array(a, dtype=np.int64), np.array(b, dtype=np.int64)
        self.seeds, self.weights = [5, 17, 130], [2.0, 1.0, 1.0]
        self.d_out = np.bincount(self.src, minlength=self.n + 2)
        self.d_in = np.bincount(self.dst, minlength=self.n + 2)

    def design(self, name, pad, claims, normalizes):
        """The graph with pad[v] feeder edges into v."""
        to = np.repeat(np.arange(self.n), pad)
        frm = np.asarray(self.feeders)[np.arange(to.size) % 2]
        d = Design(name, self.n + 2, np.concatenate([self.src, frm]), np.concatenate([self.dst, to]), self.seeds,
                   self.weights, claims, normalizes)
        d.hub, d.gadget, d.pad = self.hub, self.gadget, pad
        return d


@functools.lru_cache(maxsize=None)
def base():
    return Base()


@functools.lru_cache(maxsize=None)
def base_vector():
    """The twin's forward push of the unpadded graph from the seed set (feeders included as isolated ids)."""
    from oracle import oracle as orc
    orc.build()
    B = base()
    d = B.design("b_unpadded", np.zeros(B.n, dtype=np.int64), [], (True, False))
    return twin_vector(orc, d, True)


def twin_vector(orc, d, normalize):
    src, dst = d.src.astype(np.int64), d.dst.astype(np.int64)
    o1, o2 = np.argsort(src, kind="stable"), np.argsort(dst, kind="stable")
    rp = lambda key: np.concatenate([[0], np.cumsum(np.bincount(key, minlength=d.n))]).astype(np.uint32)
    og = orc.OracleGraph(d.n, rp(src), dst[o1].astype(np.int32), rp(dst), src[o2].astype(np.int32))
    return og.forward_push_seeds(d.seeds, ALPHA, RMAX, weights=d.weights(normalize))[0]


def _profile(B, x, pad, normalize):
    deg = (B.d_out + B.d_in).astype(np.int64)
    deg[:B.n] += pad
    ids = np.nonzero((x > 0) & (deg > 0))[0]
    score = x[ids] / deg[ids].astype(np.float64) if normalize else x[ids]
    order = ids[np.lexsort((ids, -score))]
    volx = np.concatenate([[0], np.cumsum(deg[order])])
    rank = np.full(x.size, -1, dtype=np.int64)
    rank[order] = np.arange(order.size)
    return order, volx, rank


def _solve(B, x, pad, normalize, measure, want, mod, also=None):
    """Pads one more node so that measure(order, volx, rank) -> (value, lo, hi) has value % mod == want; the node is
    taken from the profile positions lo .. hi - 1 (the gadget's second node keeps its one-slot in-row)."""
    order, volx, rank = _profile(B, x, pad, normalize)
    value, lo, hi = measure(order, volx, rank)
    need = (want - value) % mod
    if need == 0:
        return pad
    # normalize = True: the padded node's score falls and it moves down the profile, perhaps to where it counts
    # differently; so a first amount moves it, a second one (< mod) corrects what is measured then, and the result is
    # measured again
    for p in range(hi - 1, lo - 1, -1):
        v = int(order[p])
        if v == B.gadget[1]:
            continue
        for first in range(0, T + 1, SWEEP_THREADS) if normalize else (0,):
            trial = pad.copy()
            trial[v] += first
            trial[v] += (want - measure(*_profile(B, x, trial, normalize))[0]) % mod
            prof = _profile(B, x, trial, normalize)
            if measure(*prof)[0] % mod == want and (also is None or also(*prof)):
                return trial
    raise AssertionError("no node between positions %d and %d takes %d feeder edges" % (lo, hi, need))


def _family_b(normalize):
    B, x = base(), base_vector()
    tag = "n1" if normalize else "n0"
    none = np.zeros(B.n, dtype=np.int64)
    out = []

    def split(order, volx, rank):
        return int(volx[rank[B.hub]] + B.d_out[B.hub]), 0, int(rank[B.hub])

    for off, f in ((0, "B_hub_split_at_0"), (1, "B_hub_split_at_1"), (T - 1, "B_hub_split_at_T_minus_1")):
        pad = _solve(B, x, none, normalize, split, off, T)
        out.append(B.design("b_split_%d_%s" % (off, tag), pad, [f, "A_7_tiles"], (normalize,)))

    ga, gb = B.gadget

    def slots(volx, rank):
        return int(volx[rank[ga]]), int(volx[rank[gb]] + B.d_out[gb])

    def gap(order, volx, rank):
        sa, sb = slots(volx, rank)
        return abs(sb - sa), 0, int(max(rank[ga], rank[gb]))

    def low(order, volx, rank):
        return min(slots(volx, rank)), 0, int(min(rank[ga], rank[gb]))

    for kind, g_want, at, f in (("lane", 0, 100, "B_edge_in_one_lane"), ("tile", 128, 100, "B_edge_in_one_tile"),
                                ("apart", 128, T - 1, "B_edge_in_two_tiles")):
        pad = _solve(B, x, none, normalize, gap, g_want, SWEEP_THREADS)
        def gap_kept(o, v, r):   # the first padding's result survives the second one; one tile: the gap fits behind `at`
            g = gap(o, v, r)[0]
            return g % SWEEP_THREADS == g_want and (at == T - 1 or g < T - at)

        pad = _solve(B, x, pad, normalize, low, at, T, also=gap_kept)
        out.append(B.design("b_edge_%s_%s" % (kind, tag), pad, [f], (normalize,)))

    order, _, _ = _profile(B, x, none, normalize)
    q = int(order.size) * 2 // 3

    def scanned(order, volx, rank):
        return int(volx[q]), 0, q

    for off, f in ((T - 1, "B_scanned_kT_minus_1"), (0, "B_scanned_kT"), (1, "B_scanned_kT_plus_1")):
        pad = _solve(B, x, none, normalize, scanned, off, T)
        d = B.design("b_scanned_%d_%s" % (off, tag), pad, [f], (normalize,))
        d.cut_size = q
        out.append(d)
    return out


def extra_sweeps(d, V):
    """Bounded sweeps of a family B design, taken from the reference's profile: max_size at the designed cut, max_size
    between two adjacent ranked neighbours (the later one is ranked in the support and "none" in the profile), max_vol at
    the best prefix's volume and just below it."""
    kws = []
    if d.cut_size:
        kws.append(dict(max_size=d.cut_size))
    pos = V.rank
    keep = (pos[d.src] >= 0) & (pos[d.dst] >= 0) & (np.abs(pos[d.src] - pos[d.dst]) == 1)
    assert keep.any(), "%s: no relationship between adjacent profile positions" % d
    ks = np.maximum(pos[d.src][keep], pos[d.dst][keep])
    kws.append(dict(max_size=int(ks[ks.size // 2])))
    bv = V.ref["best_vol"]
    assert bv > 1
    kws += [dict(max_vol=bv), dict(max_vol=bv - 1)]
    return kws


# ---------------------------------- best-prefix ties
def pairs_with_ties(chained=300, free=420):
    """Two-node components (2i, 2i + 1), both members seeded with one weight: they tie in score and cut returns to 0
    behind every pair.  The first `chained` pairs are linked into one component, which the heaviest weights put first:
    no prefix inside it has cut 0."""
    k = chained + free
    u = 2 * np.arange(k)
    src = [u, u + 1]
    dst = [u + 1, u]
    c = u[:chained - 1]
    src += [c + 1, c + 2]
    dst += [c + 2, c + 1]
    w = np.repeat((4 * k - np.arange(k)).astype(np.float64), 2)
    w[:2 * chained] *= 64.0
    return Design("c_ties", 2 * k, np.concatenate(src), np.concatenate(dst), np.arange(2 * k), w, ["C_best_prefix_ties"])


# ---------------------------------- all of them
@functools.lru_cache(maxsize=None)
def family_a():
    hub = "A_tile_inside_one_node"
    return [
        sinks("a_aligned", [3 * T] + [1] * T + [T - 1, 1, 1, T + 1, T - 1] + [2] * 10 + [1],
              ["A_hub_over_3_tiles_aligned", hub, "A_tile_of_4096_nodes_aligned", "A_start_at_0", "A_start_at_1",
               "A_start_at_T_minus_1", "A_end_at_T", "A_end_at_T_minus_1", "A_end_at_T_plus_1", "A_7_tiles"]),
        sinks("a_off_by_1", [T - 1, 3 * T + 2] + [1] * (T - 1) + [2 * T],
              ["A_hub_over_3_tiles_off_by_1_at_both_ends", hub, "A_tile_of_4096_nodes_behind_a_hub_tail", "A_total_kT",
               "A_7_tiles"]),
        sinks("a_mixed", _fill([T + 100] + _smalls(400) + [2 * T + 50] + [256, 257, 257, 256, 255], 7 * T + 1),
              ["A_tail_smalls_head", "A_run_changes_node", "A_wave_path_beside_lane_path", "A_degrees_256_257_in_a_row",
               "A_total_kT_plus_1", "A_7_tiles"]),
        sinks("a_total_1", [1], ["A_total_1"]),
        sinks("a_total_T_minus_1", [2] * 2047 + [1], ["A_total_T_minus_1"]),
        sinks("a_total_T", [3] * 1365 + [1], ["A_total_T"]),
        sinks("a_total_T_plus_1", [2] * 2048 + [1], ["A_total_T_plus_1"]),
        sinks_denormal(),
    ]


@functools.lru_cache(maxsize=None)
def family_b():
    return _family_b(False) + _family_b(True)


@functools.lru_cache(maxsize=None)
def family_c():
    return [pairs_with_ties()]


# The designs' names, written down so that a test module is collected without building one of them (family B runs the
# twin); a test asks for its design by name.
NAMES_A = ["a_aligned", "a_off_by_1", "a_mixed", "a_total_1", "a_total_T_minus_1", "a_total_T", "a_total_T_plus_1",
           "a_denormal"]
NAMES_B = ["b_%s_%s" % (what, tag) for tag in ("n0", "n1")
           for what in ("split_0", "split_1", "split_4095", "edge_lane", "edge_tile", "edge_apart", "scanned_4095",
                        "scanned_0", "scanned_1")]
NAMES_C = ["c_ties"]
NAMES = NAMES_A + NAMES_B + NAMES_C


def all_designs():
    ds = family_a() + family_b() + family_c()
    assert [d.name for d in ds] == NAMES
    return ds


def design(name):
    family = {"a": family_a, "b": family_b, "c": family_c}[name[0]]()
    return next(d for d in family if d.name == name)
