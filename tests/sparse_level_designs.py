"""Designed graphs and a plain reference for the sparse frontier level (csrc/kernels_push.hip: k_sparse_prepare,
k_sparse_push, k_sparse_levels_wg; csrc/levels.cpp: run_sparse_batch).  Helper of test_sparse_level_designs.py (CPU) and
test_gpu_sparse_level_designs.py; nothing in this file needs a device.

The reference (`push`) is the frontier-synchronous push as the header of kernels_push.hip states it, over the caller's
ids, with no layout, tile or batch in it: every frontier node is popped at its residue at level start, alpha * r goes to
its reserve, the contributions land; forward, the level's dead-end mass lands on the source in the same level and a node
is active iff r / d >= rmax (a dead end iff r > 0); backward, every in-edge (u -> v) adds (1 - alpha) r(v) / d_out(u) and
u joins iff its residue was <= rmax when the level's adds began and is > rmax behind them.  It runs on `float` and on
`fractions.Fraction` and returns reserve, residue and a per-level trace (Level).

Exact arithmetic.  alpha = 0.5, the source's out-degree is a power of two and rmax = 2^-q.  Forward, a node of degree d
that is meant to push is fed d * rmax (a tie, which is active) through d parallel edges that carry rmax each, so its own
edges carry rmax / 2 whatever d is (5 000 included); backward, every out-degree is a power of two.  Every residue,
contribution and reserve is then a short dyadic rational, every sum is exact in any order - through the LDS table's
partial sums and the atomics' arrival order as well - and a device result equals the reference bit for bit.  Every design
proves this on the CPU: its float run equals its Fraction run entry by entry.

Absorbers.  Edges a design has to spare go where nothing can cross: forward into self loops (a node popped at
d * rmax gets at most half of it back), backward out of a node whose out-degree is padded, with edges into a node
nothing points away from, until its adds sum to rmax at the most.

Order.  The next frontier is appended by atomics, so a design fixes a level's nf, ef and the multiset of degrees in it,
never a position; every feature (FEATURES) is a predicate over the reference's trace that holds in every order.  Which
position of a batch a level takes, and whether the one-workgroup kernel meets it, follows from the sizes alone
(`schedule`, run_sparse_batch's two rules restated).

The constants the designs sit on are restated here from kernels_push.hip and levels.cpp."""
import functools
from collections import Counter

import numpy as np

ALPHA = 0.5
PUSH_TILE = 2048          # kPushTile: edges per workgroup turn
STAGE_CAP = 512           # kStageCap: frontier entries staged in LDS at a time
COMB_SLOTS, COMB_PROBES = 2048, 4   # kCombSlots, kCombProbes: the per-destination LDS table
MAX_BATCH = 8             # kMaxBatch: levels per host round trip
WG_CAP, WG_MID = 4096, 65536        # kWgCap and the size from which two levels run ahead of the one-workgroup kernel
GRID_ENTRIES, GRID_EDGES = 32768, 1 << 20   # grid bounds of the two-launch levels behind a batch's first
COMB_ON, COMB_OFF = "1", "1000000000000"    # PPRHIP_COMB_MIN_EDGES: the table on every level / on none


# ------------------------------------------------------------------ graphs
class Net:
    """An edge list under construction (parallel edges and self loops kept)."""

    def __init__(self):
        self.n, self._src, self._dst = 0, [], []

    def new(self, k=1):
        ids = np.arange(self.n, self.n + k, dtype=np.int64)
        self.n += k
        return ids

    def one(self):
        return int(self.new(1)[0])

    def add(self, u, v, times=1):
        u, v = np.broadcast_arrays(np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64))
        u, v = u.ravel(), v.ravel()
        if not (np.isscalar(times) and times == 1):
            u, v = np.repeat(u, times), np.repeat(v, times)
        self._src.append(u)
        self._dst.append(v)

    def arrays(self):
        return np.concatenate(self._src), np.concatenate(self._dst)


def home(u):
    """comb_insert's home slot of destination u (internal id)."""
    return ((int(u) * 2654435761) & 0xFFFFFFFF) >> 21


def same_home_ids(count, n, avoid=()):
    """`count` ids below n that share a home slot (as tests/apbs_designed.py:collider_ids finds its colliders)."""
    by = {}
    for u in range(n):
        if u in avoid:
            continue
        ids = by.setdefault(home(u), [])
        ids.append(u)
        if len(ids) == count:
            return ids
    raise AssertionError("no %d ids below %d share a home slot" % (count, n))


class Design:
    """A graph, the node the push starts from, rmax, the direction ("fwd": forward_push from `start`; "bwd":
    backward_push to `start`), the features it claims; K: the designed size ceil(dense_frac * m) (None: every level
    sparse); keep_ids: the claims name internal ids, the handle is made under PPRHIP_RELABEL=0; place: {node: id}."""

    def __init__(self, name, net, start, rmax, claims, mode="fwd", K=None, place=None, n=None):
        src, dst = net.arrays()
        self.n = max(net.n, n or 0)
        self.keep_ids = place is not None
        if place:
            perm = np.full(net.n, -1, dtype=np.int64)
            for node, to in place.items():
                perm[node] = to
            taken = set(place.values())
            assert len(taken) == len(place) and max(taken) < self.n
            free = (i for i in range(self.n) if i not in taken)
            for node in range(net.n):
                if perm[node] < 0:
                    perm[node] = next(free)
            src, dst, start = perm[src], perm[dst], int(perm[start])
            self.perm = perm
        self.name, self.start, self.rmax, self.claims, self.mode, self.K = name, int(start), rmax, list(claims), mode, K
        self.src, self.dst = src.astype(np.int32), dst.astype(np.int32)
        self.m = int(src.size)
        self.dout = np.bincount(src, minlength=self.n)
        self.din = np.bincount(dst, minlength=self.n)

    def __repr__(self):
        return self.name

    @property
    def fwd(self):
        return self.mode == "fwd"

    @property
    def dense_frac(self):
        """The tuning's dense_frac: ceil(dense_frac * m) == K (checked in float by the CPU tests); 1e9: never dense."""
        return 1e9 if self.K is None else (self.K - 0.5) / self.m

    @functools.cached_property
    def csr(self):
        """(row starts, neighbours) in the push direction: out-edges forward, in-edges backward."""
        key, val = (self.src, self.dst) if self.fwd else (self.dst, self.src)
        order = np.argsort(key, kind="stable")
        rp = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=self.n))])
        return rp.tolist(), val[order].tolist()

    def host(self, pkg):
        return pkg.HostCsr(self.n, self.src, self.dst)


# ------------------------------------------------------------------ the reference
class Level:
    """One level of the reference: nf entries with ef edges, `dead` dead-end pops among them, the multiset of their
    degrees (degs); enq distinct nodes joined the next frontier, tile_new bounds the distinct crossings any 2 048
    consecutive edges can hold; ndest distinct destinations (dest: their ids, kept up to 4 096); src_again: the dead-end
    mass landed on the source and the source crossed; runs: (adds, the add it crossed on, tie) of every crossing node
    that received two or more equal adds - tie: the running sum equalled the threshold right before (backward) or on
    (forward) the crossing add; stays_on_tie: nodes whose adds end exactly on rmax and that do not cross (backward)."""
    __slots__ = ("nf", "ef", "dead", "degs", "dense", "enq", "tile_new", "ndest", "dest", "src_again", "runs",
                 "ties", "stays_on_tie")

    @property
    def size(self):
        return self.nf + self.ef


class Run:
    def __init__(self, reserve, residue, trace):
        self.reserve, self.residue, self.trace = reserve, residue, trace

    def vector(self, which, n):
        out = np.zeros(n)
        for v, x in getattr(self, which).items():
            out[v] = float(x)
        return out

    def totals(self):
        """The whole-call counters of pprhip_stats_t a push with this trace reports."""
        t = self.trace
        sp = [L for L in t if not L.dense]
        return dict(levels=len(t), dense_levels=len(t) - len(sp), pops=sum(L.nf for L in sp),
                    dense_nodes=sum(L.nf for L in t if L.dense), edge_pushes=sum(L.ef for L in sp),
                    enqueues=sum(L.enq for L in t), dead_end_pops=sum(L.dead for L in t))


def push(D, num=float, alpha=ALPHA):
    """The frontier-synchronous push of design D from D.start in the number type `num`."""
    fwd = D.fwd
    rp, ci = D.csr
    dout = D.dout.tolist()
    a, one, zero, rm = num(alpha), num(1), num(0), num(D.rmax)
    s = D.start
    res, rsv, trace = {}, {}, []
    if rp[s + 1] == rp[s]:   # Forward_Push.java:72-76 / a target without in-edges
        return Run({s: one}, {}, [])

    def active(r, u):
        if not fwd:
            return r > rm
        d = dout[u]
        return r / num(d) >= rm if d else r > zero

    res[s] = one
    front = [s]
    while front:
        L = Level()
        L.nf = len(front)
        L.degs = Counter(rp[v + 1] - rp[v] for v in front)
        L.ef = sum(d * c for d, c in L.degs.items())
        L.dense = D.K is not None and L.size >= D.K
        L.dead = 0
        dead = zero
        pend = []
        for v in front:   # every frontier node gives up its residue at level start
            r = res[v]
            res[v] = zero
            rsv[v] = rsv.get(v, zero) + r * a
            d = rp[v + 1] - rp[v]
            if not fwd:
                pend.append((one - a) * r)
            elif d == 0:
                dead = dead + r * (one - a)
                L.dead += 1
                pend.append(None)
            else:
                pend.append(((one - a) * r) / num(d))
        seen = {}   # u -> [residue when the level's adds began, adds, the first add, all adds equal]
        for v, c in zip(front, pend):
            if c is None:
                continue
            for e in range(rp[v], rp[v + 1]):
                u = ci[e]
                add = c if fwd else c / num(dout[u])
                old = res.get(u, zero)
                res[u] = old + add
                rec = seen.get(u)
                if rec is None:
                    seen[u] = [old, 1, add, True]
                else:
                    rec[1] += 1
                    if add != rec[2]:
                        rec[3] = False
        L.ndest = len(seen)
        L.dest = np.fromiter(seen, dtype=np.int64, count=len(seen)) if len(seen) <= 2 * PUSH_TILE else None
        by_edge = set(seen)
        if fwd and dead > zero:   # the level's dead-end mass lands on the source
            old = res.get(s, zero)
            res[s] = old + dead
            if s not in seen:
                seen[s] = [old, 1, dead, False]
            else:
                seen[s][3] = False
        nxt, L.runs, L.ties, L.stays_on_tie = [], [], 0, 0
        for u, (old, cnt, add, equal) in seen.items():
            if not active(old, u) and active(res[u], u):
                nxt.append(u)
                if fwd and dout[u] and res[u] == rm * num(dout[u]):
                    L.ties += 1
                if equal and cnt >= 2:
                    j = next(j for j in range(1, cnt + 1) if active(old + add * num(j), u))
                    at = old + add * num(j if fwd else j - 1)
                    L.runs.append((cnt, j, at == (rm * num(dout[u]) if fwd else rm)))
            elif not fwd and res[u] == rm:
                L.stays_on_tie += 1
        L.enq = len(nxt)
        L.tile_new = min(PUSH_TILE, sum(1 for u in nxt if u in by_edge))
        L.src_again = fwd and dead > zero and s in nxt
        trace.append(L)
        front = nxt
    return Run(rsv, res, trace)


_runs = {}


def run(D, num=float):
    """The reference run of a design, computed once and never changed."""
    key = (D.name, num)
    if key not in _runs:
        _runs[key] = push(D, num)
    return _runs[key]


# ------------------------------------------------------------------ which batch position a level takes
class Slot:
    """pos: the level's position in its batch; wg_from: the batch's first position run by the one-workgroup kernel;
    cut: the level before it ran in the same batch and this one was too large for the one-workgroup kernel, which
    returned at it (the host breaks by the same rule), so the level is the first of a batch of its own."""
    __slots__ = ("pos", "wg_from", "cut", "dense")

    @property
    def in_wg(self):
        return not self.dense and self.pos >= self.wg_from


def schedule(trace):
    """run_sparse_batch's decisions for a trace (the one-workgroup kernel on, no round cut, no seed set)."""
    out, i, prepared, cut = [], 0, False, False
    while i < len(trace):
        if trace[i].dense:
            S = Slot()
            S.pos, S.wg_from, S.cut, S.dense = 0, 0, False, True
            out.append(S)
            prepared, cut, i = True, False, i + 1
            continue
        size0 = trace[i].size
        wg_from = 0 if (not prepared and size0 < WG_CAP) else 1 if size0 < WG_MID else 2
        prepared = False
        pos = 0
        while True:
            S = Slot()
            S.pos, S.wg_from, S.cut, S.dense = pos, wg_from, cut and pos == 0, False
            out.append(S)
            pos += 1
            cut = False
            if pos == MAX_BATCH or i + pos == len(trace) or trace[i + pos].dense:
                break
            if pos >= wg_from and trace[i + pos].size >= WG_CAP:
                cut = True
                break
        i += pos
    return out


# ------------------------------------------------------------------ features, by name
def _levels(D):
    t = run(D).trace
    return list(zip(range(len(t)), t, schedule(t)))


def _then_small(t, i):
    return i + 1 < len(t) and t[i + 1].size < WG_CAP


def _batch_levels(n):
    def f(D):
        t = run(D).trace
        return len(t) == n and all(not L.dense and 1 <= L.nf <= 3 for L in t)
    return f


def _first(size):
    def f(D):
        t = run(D).trace
        return any(L.size == size and S.pos == 0 and _then_small(t, i) for i, L, S in _levels(D))
    return f


def _later(size):
    def f(D):
        t = run(D).trace
        if size < WG_CAP:   # the one-workgroup kernel runs it and goes on
            return any(L.size == size and S.pos >= 1 and S.in_wg and _then_small(t, i) for i, L, S in _levels(D))
        return any(L.size == size and S.cut and _then_small(t, i) for i, L, S in _levels(D))
    return f


def _small_large_small(D):
    t = run(D).trace
    return any(t[i].size < WG_CAP <= t[i + 1].size and t[i + 2].size < WG_CAP for i in range(len(t) - 2))


def _edges(E):
    return lambda D: any(L.ef == E and not L.dense for L in run(D).trace)


def _entries_of_degree_one(n):
    return lambda D: any(L.nf == n and L.degs == {1: n} for L in run(D).trace)


def _adds(K):
    return lambda D: any(cnt == K and 1 < j < cnt for L in run(D).trace for cnt, j, tie in L.runs)


def _tie(D):
    t = run(D).trace
    if D.fwd:
        return any(L.ties for L in t)
    # the running sum equalled rmax behind an add, which is not active (strict), and the next add crossed
    return any(tie for L in t for cnt, j, tie in L.runs)


def _full_tile(L):
    return L.ef == PUSH_TILE and L.ndest == PUSH_TILE and L.tile_new == PUSH_TILE


def _homes(D, L):
    return Counter(home(u) for u in L.dest) if D.keep_ids and L.dest is not None else Counter()


def _probes_fail(D):
    # five destinations of one home slot can take its four probe slots only: one edge lands on its own in every order
    return any(L.ef == PUSH_TILE and L.ndest == PUSH_TILE and max(_homes(D, L).values(), default=0) > COMB_PROBES
               for L in run(D).trace)


def _colliders(L, D):
    h = _homes(D, L)
    return L.ef >= PUSH_TILE - 3 and len(h) >= 2 and max(h.values(), default=0) >= 6 and L.ndest >= 7


def _colliders_twice(D):
    # two tiles of one level, run one behind the other by the one workgroup of k_sparse_levels_wg
    return any(_colliders(L, D) and PUSH_TILE < L.ef and L.size < WG_CAP and S.in_wg for i, L, S in _levels(D))


def _dead_stage(D):
    return any(L.degs.get(0, 0) >= 1100 and L.degs.get(32, 0) == 64 and set(L.degs) == {0, 32} for L in run(D).trace)


def _sparse_dense_sparse(D):
    t = run(D).trace
    return any(not t[i].dense and t[i + 1].dense and not t[i + 2].dense and t[i + 2].ef == 0 and t[i + 2].nf > 0 and
               t[i + 2].dead == t[i + 2].nf and t[i + 2].src_again for i in range(len(t) - 2))


FEATURES = {
    **{"B_%d_levels" % n: _batch_levels(n) for n in (7, 8, 9, 15, 16, 17, 25)},
    "W_first_level_4095": _first(4095), "W_first_level_4096": _first(4096),
    "W_first_level_65535_then_small": _first(65535), "W_first_level_65536_then_small": _first(65536),
    "W_later_level_4095_then_small": _later(4095), "W_later_level_4096_then_small": _later(4096),
    "W_small_large_small": _small_large_small,
    "G_two_launch_level_above_32768_entries":
        lambda D: any(S.pos == 1 and S.wg_from == 2 and L.nf > GRID_ENTRIES for i, L, S in _levels(D)),
    "G_two_launch_level_above_2pow20_edges":
        lambda D: any(S.pos == 1 and S.wg_from == 2 and L.ef > GRID_EDGES for i, L, S in _levels(D)),
    **{"T_level_of_%d_edges" % E: _edges(E) for E in (2047, 2048, 2049, 4096, 4097)},
    "T_row_of_5000_among_rows_of_1_and_2":
        lambda D: any(L.degs.get(5000) == 1 and set(L.degs) == {1, 2, 5000} for L in run(D).trace),
    "T_one_row_of_2048": lambda D: any(L.nf == 1 and L.ef == PUSH_TILE for L in run(D).trace),
    **{"S_%d_entries_of_degree_1" % n: _entries_of_degree_one(n) for n in (511, 512, 513, 1025, 2048)},
    "S_stage_of_dead_ends": _dead_stage,
    "N_tile_of_2048_crossings": lambda D: any(_full_tile(L) for L in run(D).trace),
    "N_tile_of_2048_crossings_and_source_again":
        lambda D: any(_full_tile(L) and L.src_again and L.enq == PUSH_TILE + 1 for L in run(D).trace),
    "N_nothing_crosses": lambda D: any(L.ef >= PUSH_TILE - 1 and L.enq == 0 for L in run(D).trace),
    "N_4_adds_cross_inside": _adds(4), "N_64_adds_cross_inside": _adds(64), "N_2048_adds_cross_inside": _adds(2048),
    "N_tie": _tie,
    "C_2048_destinations_probes_fail": _probes_fail,
    "C_one_destination": lambda D: any(L.ef == PUSH_TILE and L.ndest == 1 for L in run(D).trace),
    "C_colliders_and_a_seventh": lambda D: any(_colliders(L, D) for L in run(D).trace),
    "C_colliders_two_tiles_in_a_row": _colliders_twice,
    "D_level_of_K_minus_1_sparse": lambda D: D.K and any(L.size == D.K - 1 and not L.dense for L in run(D).trace),
    "D_level_of_K_dense": lambda D: D.K and any(L.size == D.K and L.dense for L in run(D).trace),
    "D_sparse_dense_sparse_from_dead_ends": _sparse_dense_sparse,
}
# what the transposed designs put on the backward search (dead-end mass exists forward only)
BWD_FEATURES = sorted(f for f in FEATURES if f[0] in "TSNC" and f != "N_tile_of_2048_crossings_and_source_again")


# ------------------------------------------------------------------ forward designs
def _pow2_at_least(x):
    return 1 << max(0, int(x - 1).bit_length())


def _rows_summing_to(E, pattern=(1, 0, 2, 4, 0)):
    rows, left, i = [], E, 0
    while left:
        d = min(pattern[i % len(pattern)], left)
        rows.append(d)
        left -= d
        i += 1
    return rows


def _land(net, esrc, dest, fwd):
    """Where the level's E edges go (forward: their heads; backward: their tails).  Returns {node: id} placements."""
    E = esrc.size
    link = (lambda a, b, times=1: net.add(a, b, times)) if fwd else (lambda a, b, times=1: net.add(b, a, times))
    if dest == "self":            # forward only: nothing crosses
        net.add(esrc, esrc)
    elif dest == "pairs":         # two edges per node: the second add crosses (the last node of an odd E gets one)
        w = net.new((E + 1) // 2)
        link(esrc, w[np.arange(E) // 2])
        return w
    elif dest == "distinct":      # one edge per node, and it crosses
        w = net.new(E)
        link(esrc, w)
        return w
    else:                         # [(edges, node)]: runs of equal adds
        at = 0
        for K, w in dest:
            link(esrc[at:at + K], w)
            at += K
        assert at == E
    return None


def fwd_two_stage(name, rows, dest, claims, feed=1, place=None, n=None, groups=None):
    """source -> level 1: entries of out-degree rows[i] (0: a dead end), fed feed * rows[i] parallel edges of rmax each
    (a dead end one) -> level 2.  The source's spare edges are self loops; nodes of level 2 have one self loop."""
    net = Net()
    s = net.one()
    rows = np.asarray(rows, dtype=np.int64)
    ent = net.new(rows.size)
    k = np.where(rows > 0, feed * rows, 1)
    D = _pow2_at_least(int(k.sum()))
    net.add(s, ent, k)
    net.add(s, s, D - int(k.sum()))
    rmax = 0.5 / D                                 # what one edge of the source carries
    esrc = np.repeat(ent, rows)
    if groups:                                     # [(edges, out-degree of the node they share)]: its edges are self loops
        w = [net.one() for _ in groups]
        for (K, dw), u in zip(groups, w):
            net.add(u, u, dw)
        _land(net, esrc, [(K, u) for (K, dw), u in zip(groups, w)], True)
    else:
        w = _land(net, esrc, dest, True)
        if w is not None:
            net.add(w, w)
    if callable(place):
        place = place(w)
    return Design(name, net, s, rmax, claims, place=place, n=n)


def fwd_chain(L):
    """s -> a, b; a -> a; b -> b, c; c -> c: a holds 2^-(k + 1) in level k and pushes while that is >= rmax = 2^-L."""
    net = Net()
    s, a, b, c = net.new(4)
    net.add([s, s, a, b, b, c], [a, b, a, b, c, c])
    return Design("fwd_chain_%d" % L, net, s, 2.0 ** -L, ["B_%d_levels" % L])


def fwd_wg(name, P, entries, F, claims):
    """p0 -> ... -> p[P-1] (the feeder, out-degree F) -> entries [(out-degree, count)], one edge of the feeder each (the
    first entry takes the feeder's spare edges as well).  rmax is what the largest entries hold per edge, a tie; their
    edges are self loops, so half of it comes back and they stay; a smaller entry comes back once.  Sixteen edges of the
    first entry start a tail of single nodes, each of which holds half of what the one before it held."""
    net = Net()
    p = net.new(P)
    net.add(p[:-1], p[1:])
    dmax = max(d for d, _ in entries)
    q = net.new(12)
    net.add(q[:-1], q[1:])
    net.add(q[-1], q[-1])
    used = sum(count for _, count in entries)
    assert F >= used and F & (F - 1) == 0
    for i, (d, count) in enumerate(entries):
        e = net.new(count)
        net.add(p[-1], e)
        loops = np.full(count, d)
        if i == 0:
            net.add(p[-1], e[0], F - used)
            net.add(e[0], q[0], 16)
            loops[0] -= 16
        net.add(e, e, loops)
    rmax = 2.0 ** -(P - 1) / (2 * F) / dmax
    return Design(name, net, int(p[0]), rmax, claims)


def fwd_source_again():
    """s (4 edges) -> h three times and a dead end e once; level 1 pops h (2 048 edges to 2 048 nodes, 3 * 2^-15 >= rmax
    = 2^-14 each: all cross) and e, whose mass lands on s in the same level, and s crosses again."""
    net = Net()
    s, h, e = net.new(3)
    w = net.new(PUSH_TILE)
    net.add([s, s, s, s], [h, h, h, e])
    net.add(h, w)
    net.add(w, w)
    return Design("fwd_source_again", net, s, 2.0 ** -14, ["N_tile_of_2048_crossings_and_source_again"])


def fwd_edges_2pow20():
    """s (2^16 edges: the first level is 65 537) -> 32 entries of 32 768 self loops (1 024 edges of s each: 2^-7, a
    tie at rmax = 2^-22) and z (32 768 edges of s, one self loop): level 1 is 33 entries and 2^20 + 1 edges, run as two
    launches over 512 workgroups; z then halves for twenty levels more."""
    net = Net()
    s, z = net.new(2)
    ent = net.new(32)
    net.add(s, ent, 1024)
    net.add(s, z, 32768)
    net.add(ent, ent, 32768)
    net.add(z, z)
    return Design("fwd_edges_2pow20", net, s, 2.0 ** -22, ["G_two_launch_level_above_2pow20_edges"])


def fwd_dense(at_K):
    """K = 130.  Below: s -> e (128 self loops): level 1 is 129 = K - 1 and runs sparse.  At: s -> e1, e2 (64 edges each
    into eight dead ends): level 1 is 130 = K and runs dense; level 2 is the eight dead ends, compacted to an empty list,
    whose mass lands on s; s crosses and level 3 runs sparse.  Seventy edges nothing reaches make m differ from K."""
    net = Net()
    s = net.one()
    if at_K:
        e = net.new(2)
        dead = net.new(8)
        net.add(s, e)
        net.add(np.repeat(e, 64), np.tile(dead, 16))
        rmax, claims = 2.0 ** -8, ["D_level_of_K_dense", "D_sparse_dense_sparse_from_dead_ends"]
    else:
        e = net.one()
        net.add(s, e)
        net.add(e, e, 128)
        rmax, claims = 2.0 ** -8, ["D_level_of_K_minus_1_sparse"]
    far = net.new(70)
    net.add(far, np.roll(far, 1))
    return Design("fwd_dense_at_K" if at_K else "fwd_dense_below_K", net, s, rmax, claims, K=130)


def _colliders_place(n, count=6):
    ids = same_home_ids(count, n)
    other = next(u for u in range(n) if home(u) != home(ids[0]))
    return ids, other


def fwd_colliders():
    """Level 1: rows of 2 048 and 2 045 edges (4 095 with the two entries: two tiles of the one workgroup), every edge to
    one of seven nodes in turn: six share a home slot (256 self loops: they cross inside their run of ~585 adds of
    rmax / 2), the seventh (1 024 self loops) does not cross."""
    net = Net()
    s = net.one()
    rows = np.array([2048, 2045])
    ent = net.new(2)
    net.add(s, ent, rows)
    net.add(s, s, 8192 - 4093)
    w = net.new(7)
    net.add(w[:6], w[:6], 256)
    net.add(w[6], w[6], 1024)
    net.add(np.repeat(ent, rows), w[np.arange(4093) % 7])
    ids, other = _colliders_place(32768)
    place = {int(w[i]): ids[i] for i in range(6)}
    place[int(w[6])] = other
    return Design("fwd_colliders", net, s, 0.5 / 8192, ["C_colliders_and_a_seventh", "C_colliders_two_tiles_in_a_row",
                                                          "W_later_level_4095_then_small"], place=place, n=32768)


def _five_of_one_home(w):
    return {int(w[i]): u for i, u in enumerate(same_home_ids(5, 32768))}


# ------------------------------------------------------------------ backward designs
def bwd_two_stage(name, rows, dest, claims, place=None, n=None, groups=None):
    """target t <- level 1: entries of in-degree rows[i], each with the edges -> t and -> X (out-degree 2: they hold 1/4
    and hand on 1/8 per in-edge) <- level 2.  rmax = 1/16.  "pairs": nodes of out-degree 2, an add is 1/16 = rmax (a
    tie, not active) and the second crosses; "distinct": out-degree 1, the one add crosses; "absorb": one node whose
    out-degree is padded to 4 E; groups [(K, out-degree)]: K equal adds to one node.  X has no out-edge: it never
    receives."""
    net = Net()
    t, X = net.new(2)
    rows = np.asarray(rows, dtype=np.int64)
    ent = net.new(rows.size)
    net.add(ent, t)
    net.add(ent, X)
    edst = np.repeat(ent, rows)
    E = edst.size
    w = None
    if groups:
        dest, w = [], []
        for K, dw in groups:
            u = net.one()
            net.add(u, X, dw - K)
            dest.append((K, u))
            w.append(u)
        _land(net, edst, dest, False)
    elif dest == "absorb":
        A = net.one()
        net.add(A, edst)
        net.add(A, X, _pow2_at_least(4 * E) - E)
    else:
        w = _land(net, edst, dest, False)
        if dest == "pairs" and E % 2:
            net.add(w[-1], X)
    if callable(place):
        place = place(w)
    return Design(name, net, t, 1.0 / 16, claims, mode="bwd", place=place, n=n)


def bwd_chain(L):
    """t = p[0] <- p[1] <- ... <- p[L-1] and t <- q[0] <- ... <- q[L // 2 - 1], out-degree 1 each: level k pops p[k], which
    holds 2^-k, and q[k-1]; the last node of a chain has no in-edge."""
    net = Net()
    p = net.new(L)
    q = net.new(L // 2)
    net.add(p[1:], p[:-1])
    net.add(q, np.concatenate([p[:1], q[:-1]]))
    return Design("bwd_chain_%d" % L, net, int(p[0]), 2.0 ** -40, ["B_%d_levels" % L], mode="bwd")


def bwd_wg(name, P, entries, claims, shift=5):
    """t = p0 <- p1 <- ... <- p[P-1] (out-degree 1 each: p[k] holds 2^-k) <- entries [(in-degree, count)] of out-degree 1,
    whose in-edges come from one absorber (out-degree padded until its adds sum to rmax = 2^-(P + shift) at the most)
    and, one of them, from a tail of single nodes."""
    net = Net()
    p = net.new(P)
    X = net.one()
    net.add(p[1:], p[:-1])
    A = net.one()
    q = net.new(shift)          # the tail: q[j] holds 2^-(P + 1 + j); the last one ends on rmax, a tie, and stays
    net.add(q[1:], q[:-1])
    E = 0
    for d, count in entries:
        e = net.new(count)
        net.add(e, p[-1])
        to = np.repeat(e, d)
        if E == 0:              # the first entry's first in-edge comes from the tail
            net.add(q[0], to[0])
            to = to[1:]
        net.add(A, to)
        E += d * count
    net.add(A, X, _pow2_at_least(E << (shift - 1)) - (E - 1))
    return Design(name, net, int(p[0]), 2.0 ** -(P + shift), claims, mode="bwd")


def bwd_entries_above_32768():
    """t <- 40 000 nodes of out-degree 1 (they hold 1/2) and 25 536 edges of an absorber (out-degree 2^17): level 0 is
    65 537; level 1, 40 000 entries of in-degree 1 whose in-neighbours (out-degree 2) get 1/8 + 1/8 > rmax = 1/8."""
    net = Net()
    t, X, A = net.new(3)
    u = net.new(40000)
    net.add(u, t)
    net.add(A, t, 25536)
    net.add(A, X, (1 << 17) - 25536)
    w = net.new(20000)
    net.add(np.repeat(w, 2), u)
    return Design("bwd_entries_above_32768", net, t, 0.125, ["G_two_launch_level_above_32768_entries"], mode="bwd")


def bwd_edges_2pow20():
    """t <- 33 entries (-> t, -> X: they hold 1/4) and 65 503 edges of an absorber A2; 32 entries have 32 768 in-edges from
    the absorber A (out-degree 2^20: its adds sum to 1/8 = rmax, a tie that is not active), the last has one, from w."""
    net = Net()
    t, X, A, A2, w = net.new(5)
    u = net.new(33)
    net.add(u, t)
    net.add(u, X)
    net.add(A2, t, 65503)
    net.add(A2, X, (1 << 18) - 65503)
    net.add(A, np.repeat(u[:32], 32768))
    net.add(w, u[32])
    return Design("bwd_edges_2pow20", net, t, 0.125, ["G_two_launch_level_above_2pow20_edges"], mode="bwd")


def bwd_colliders():
    """fwd_colliders on the in-edges: two entries of in-degree 2 048 and 2 045, their in-neighbours seven nodes in turn; the
    six of one home slot have out-degree 1 024 (~585 adds of 2^-13: they cross inside the run), the seventh 2 048."""
    net = Net()
    t, X = net.new(2)
    rows = np.array([2048, 2045])
    ent = net.new(2)
    net.add(ent, t)
    net.add(ent, X)
    w = net.new(7)
    to = np.repeat(ent, rows)
    frm = w[np.arange(4093) % 7]
    net.add(frm, to)
    cnt = np.bincount(np.arange(4093) % 7, minlength=7)
    net.add(w[:6], X, 1024 - cnt[:6])
    net.add(w[6], X, 2048 - cnt[6])
    ids, other = _colliders_place(32768)
    place = {int(w[i]): ids[i] for i in range(6)}
    place[int(w[6])] = other
    return Design("bwd_colliders", net, t, 1.0 / 16, ["C_colliders_and_a_seventh", "C_colliders_two_tiles_in_a_row",
                                                        "W_later_level_4095_then_small"], mode="bwd", place=place, n=32768)


# ------------------------------------------------------------------ the designs
W_ENTRIES = {4095: ([(64, 63)], 64), 4096: ([(64, 62), (32, 2)], 64),
             65535: ([(256, 255)], 256), 65536: ([(256, 254), (128, 2)], 256)}
DEAD_STAGE_ROWS = [32] * 32 + [0] * 1100 + [32] * 32     # in id order 1 100 dead ends separate the live halves


@functools.lru_cache(maxsize=None)
def all_designs():
    ds = []
    for two, tag in ((fwd_two_stage, "fwd"), (bwd_two_stage, "bwd")):
        quiet = "self" if tag == "fwd" else "absorb"
        ds += [two("%s_edges_2047" % tag, _rows_summing_to(2047), quiet, ["T_level_of_2047_edges", "N_nothing_crosses"])]
        ds += [two("%s_edges_%d" % (tag, E), _rows_summing_to(E), "pairs", ["T_level_of_%d_edges" % E, "N_tie"])
               for E in (2049, 4096, 4097)]
        ds += [two("%s_row_5000" % tag, [1] * 100 + [5000] + [2] * 100, "pairs", ["T_row_of_5000_among_rows_of_1_and_2"])]
        ds += [two("%s_entries_%d" % (tag, k), [1] * k, "pairs", ["S_%d_entries_of_degree_1" % k])
               for k in (511, 512, 513, 1025)]
        kw = dict(feed=2) if tag == "fwd" else {}
        ds += [two("%s_tile_2048" % tag, [1] * PUSH_TILE, "distinct",
                   ["S_2048_entries_of_degree_1", "T_level_of_2048_edges", "N_tile_of_2048_crossings",
                    "C_2048_destinations_probes_fail"], place=_five_of_one_home, n=32768, **kw),
               two("%s_one_row_2048" % tag, [PUSH_TILE], "distinct", ["T_one_row_of_2048", "N_tile_of_2048_crossings"], **kw),
               two("%s_dead_stage" % tag, DEAD_STAGE_ROWS, "pairs", ["S_stage_of_dead_ends"])]
        # K equal adds to a node that crosses on add K / 2 (forward, out-degree K / 4: the sum is rmax * d on that add)
        # or K / 2 + 1 (backward, out-degree K: the sum is rmax on add K / 2)
        div = 4 if tag == "fwd" else 1
        ds += [two("%s_adds_4_64" % tag, [1] * 68, None, ["N_4_adds_cross_inside", "N_64_adds_cross_inside", "N_tie"],
                   groups=[(4, 4 // div), (64, 64 // div)]),
               two("%s_one_destination" % tag, [1] * PUSH_TILE, None, ["N_2048_adds_cross_inside", "C_one_destination"],
                   groups=[(PUSH_TILE, PUSH_TILE // div)])]
    ds += [fwd_colliders(), bwd_colliders(), fwd_source_again()]
    ds += [f(L) for f in (fwd_chain, bwd_chain) for L in (7, 8, 9, 15, 16, 17, 25)]
    for size, (entries, F) in W_ENTRIES.items():
        if size < WG_CAP:
            first = ["W_first_level_%d" % size]
            later = ["W_later_level_%d_then_small" % size]
        else:
            first = ["W_first_level_%d" % size]
            later = first + ["W_later_level_4096_then_small", "W_small_large_small"]
        if size in (4095, 4096):
            ds += [fwd_wg("fwd_wg_%d_first" % size, 8, entries, F, first),
                   fwd_wg("fwd_wg_%d_later" % size, 2, entries, F, later),
                   bwd_wg("bwd_wg_%d_first" % size, 8, entries, first),
                   bwd_wg("bwd_wg_%d_later" % size, 2, entries, later)]
        else:
            claim = ["W_first_level_%d_then_small" % size]
            ds += [fwd_wg("fwd_wg_%d" % size, 2, entries, F, claim), bwd_wg("bwd_wg_%d" % size, 2, entries, claim, shift=3)]
    ds += [fwd_two_stage("fwd_entries_above_32768", [1] * 40000, "pairs", ["G_two_launch_level_above_32768_entries"]),
           fwd_edges_2pow20(), bwd_entries_above_32768(), bwd_edges_2pow20(), fwd_dense(False), fwd_dense(True)]
    assert len({d.name for d in ds}) == len(ds)
    return {d.name: d for d in ds}


def designs(letters, mode=None):
    """The designs that claim a feature of one of the letters (B, W, G, T, S, N, C, D), in a fixed order."""
    out = []
    for d in all_designs().values():
        fam = {c[0] for c in d.claims}
        if fam & set(letters) and (mode is None or d.mode == mode):
            out.append(d)
    return out
