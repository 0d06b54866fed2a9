"""All-Pair backward searches designed node by node (helper of test_apbs_designed.py and test_gpu_apbs_designed.py).

The reference (`search`) is the frontier-synchronous backward search as kernels_apbs.hip's header and
Backward_Search.java:38-100 state it: the target is popped first whatever the threshold; per level every frontier node
gives alpha * r to its reserve and holds (1 - alpha) * r pending; every in-edge (u -> v) adds pending[v] / dout[u] to
res[u]; u joins the next frontier iff its residue was <= rmax when the level's edge phase began and is > rmax after it;
a target without in-edges yields {t: 1.0}; entries with reserve > 0 and reserve >= rmax are emitted.  It runs on any
number type: `float` (IEEE binary64, what numpy's float64 holds; the results go into float64 arrays) and
`fractions.Fraction`.

Every design uses alpha = 0.5 and out-degrees that are powers of two, so every residue and reserve is a short dyadic
rational, every sum is exact in any order, and a device result has to equal the reference bit for bit.  A residue or a
reserve equal to rmax is then something a design can arrange.

The constants the designs sit on are restated here from kernels_apbs.hip; nothing in this file needs a device."""
import numpy as np

ALPHA = 0.5
SMALL_CAP, LARGE_CAP = 512, 2048                 # slots of the two LDS tables
SMALL_LIMIT, LARGE_LIMIT = 384, 1536             # CAP - CAP / 4: a search of `limit` nodes stays, limit + 1 is handed on
SMALL_FRONT, LARGE_FRONT = 128, 512              # frontier entries staged per sub-batch
SMALL_TRIP, LARGE_TRIP = 4 * 64, 4 * 256         # edges per trip of the edge loop
DEG_BIG, DEG_DENSE = 4, 12                       # k_apbs_split: in-degrees from which a search starts further on
DN_STAGE = 1024                                  # dense tier: frontier entries of a one-tile level
DN_SHARE_MIN = 4                                 # dense tier: chunks from which a one-tile level is posted
DN_CHUNK_TEST = 16                               # the smallest PPRHIP_APBS_CHUNK the driver accepts
HOT_TEST = 64                                    # PPRHIP_APBS_HOT of the hot design
MAX_CUS = 512                                    # the crowd's pigeonhole bound holds for parts of at most this many CUs

R_FAN = 0.25                                     # fans: every add (0.5) crosses, the sources' reserve 0.25 == rmax
R_FAN_TIE = 0.5                                  # fans: every add equals rmax and nothing crosses; t's reserve 0.5 == rmax
R_STRICT = 5.0 / 32 + 2.0 ** -12                 # two_level: between two running sums of every run (adds >= 2^-9)
R_TIE = 0.125                                    # two_level: a running sum equals rmax after an add, the next add crosses


# ------------------------------------------------------------------ graphs
class Graph:
    """An edge list with its in-adjacency and out-degrees (parallel edges and self loops kept)."""

    def __init__(self, n, src, dst):
        self.n = int(n)
        self.src = np.asarray(src, dtype=np.int32)
        self.dst = np.asarray(dst, dtype=np.int32)
        self.m = int(self.src.size)
        assert self.src.size == self.dst.size
        assert self.m == 0 or (0 <= min(self.src.min(), self.dst.min()) and max(self.src.max(), self.dst.max()) < n)
        self.dout = np.bincount(self.src, minlength=self.n).astype(np.int64)
        self.din = np.bincount(self.dst, minlength=self.n).astype(np.int64)
        d = self.dout[self.dout > 0]
        assert np.all(d & (d - 1) == 0), "out-degrees must be powers of two"
        order = np.argsort(self.dst, kind="stable")
        self.in_rp = np.concatenate([[0], np.cumsum(self.din)]).astype(np.int64)
        self.in_ci = self.src[order]
        self._dout = self.dout.tolist()

    def innbrs(self, v):
        return self.in_ci[self.in_rp[v]:self.in_rp[v + 1]].tolist()

    def host(self, pkg):
        return pkg.HostCsr(self.n, self.src, self.dst)


class Search:
    """What one backward search did: the emitted entries {source: reserve}, the counters, and per level the frontier
    size, the edges E, and the distinct nodes touched once the level is over."""
    __slots__ = ("t", "entries", "reserve", "residue", "pops", "pushes", "frontiers", "edges", "touched_after",
                 "touched", "ties_res", "ties_rsv")


def search(G, t, rmax, num=float, alpha=ALPHA, keep=False):
    a, one, zero, rm = num(alpha), num(1), num(0), num(rmax)
    S = Search()
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
            for v, p in zip(frontier, pend):
                for u in G.innbrs(v):
                    E += 1
                    old = res.get(u, zero)
                    if u not in start:
                        start[u] = old
                    nw = old + p / num(G._dout[u])
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


_runs = {}


def run(G, lo, hi, rmax):
    """The float searches of the targets [lo, hi), kept per (graph, range, rmax): computed once, never changed."""
    key = (id(G), lo, hi, rmax)
    if key not in _runs:
        _runs[key] = [search(G, t, rmax) for t in range(lo, hi)]
    return _runs[key]


def index_of(G, searches):
    """The inverted index with k = -1: rows by source, entries in target order (offsets, targets, values)."""
    rows = sorted((u, S.t, r) for S in searches for u, r in S.entries.items())
    off = np.zeros(G.n + 1, dtype=np.uint64)
    if rows:
        np.add.at(off, np.array([x[0] for x in rows], dtype=np.int64) + 1, 1)
    return (np.cumsum(off).astype(np.uint64), np.array([x[1] for x in rows], dtype=np.int32),
            np.array([float(x[2]) for x in rows], dtype=np.float64))


# ------------------------------------------------------------------ the path a search takes, and what the counters hold
def partial(S, limit, front):
    """(pops, pushes) a table of `limit` nodes has counted when it hands the search on: the kernel adds a level's pops and
    a sub-batch's E before the edge loop in which the table overflows, and nothing after it.  Derived for levels of one
    sub-batch (the designs that overflow a table do so in such a level)."""
    for lv, touched in enumerate(S.touched_after):
        if touched > limit:
            assert S.frontiers[lv] <= front
            return sum(S.frontiers[:lv + 1]), sum(S.edges[:lv + 1])
    return None


def tiers(S, din, mode):
    """The tiers ("small", "large", "dense") that run the search, in order.  mode: "default" (k_apbs_split routes by
    in-degree), "tables" (PPRHIP_APBS_DEG=0,0: small table first), "large" (=1,0: large table first), "dense"
    (PPRHIP_APBS_TIER=2)."""
    if mode == "dense":
        return ["dense"]
    if din == 0:
        return []                                   # emitted by k_apbs_split
    first = {"tables": "small", "large": "large"}.get(mode) or \
        ("small" if din < DEG_BIG else "large" if din < DEG_DENSE else "dense")
    out = [first]
    if out[-1] == "small" and S.touched > SMALL_LIMIT:
        out.append("large")
    if out[-1] == "large" and S.touched > LARGE_LIMIT:
        out.append("dense")
    return out


def counters(G, searches, mode):
    """(pops, edge pushes, targets that reach the dense tier) of one call over `searches`, as the kernels count them: a
    tier that hands a search on has counted the part it ran, the tier that finishes it counts all of it."""
    pops = pushes = rounds = 0
    for S in searches:
        path = tiers(S, int(G.din[S.t]), mode)
        for tier in path[:-1]:
            p, e = partial(S, SMALL_LIMIT, SMALL_FRONT) if tier == "small" else partial(S, LARGE_LIMIT, LARGE_FRONT)
            pops, pushes = pops + p, pushes + e
        if path:
            pops, pushes = pops + S.pops, pushes + S.pushes
        rounds += "dense" in path
    return pops, pushes, rounds


# ------------------------------------------------------------------ gadgets: one target each, local ids, target = 0
class Gadget:
    def __init__(self, name, n, edges, claims):
        self.name, self.n, self.edges, self.claims = name, n, edges, claims   # claims: {rmax: (touched, frontiers, E)}


def fan(N):
    """Target 0 with N - 1 in-neighbours of out-degree 1: the search touches exactly N nodes; with rmax < 0.5 level 2 is
    a frontier of N - 1 entries, all of in-degree 0.  N = 1 is a target without in-edges."""
    edges = [(i, 0) for i in range(1, N)]
    if N == 1:
        return Gadget("fan1", 1, edges, {R_FAN: (1, [], []), R_FAN_TIE: (1, [], [])})
    return Gadget("fan%d" % N, N, edges, {R_FAN: (N, [1, N - 1], [N - 1, 0]), R_FAN_TIE: (N, [1], [N - 1])})


def fan_loop(F):
    """A fan whose target has its own edge as its only out-edge: level 2's frontier is the F - 1 sources and the target
    again, F entries, while only F distinct nodes are ever popped - the frontier list and the popped-node list of the
    dense tier (both of cap_f entries) fill up together, where a plain fan pops one node more than its frontier holds."""
    edges = [(i, 0) for i in range(1, F)] + [(0, 0)]
    return Gadget("fanloop%d" % F, F, edges, {R_FAN: (F, [1, F], [F, F])})


def powers(E, top=128):
    """E as a sum of powers of two, none above `top`."""
    out = [top] * (E // top)
    rest, p = E % top, top
    while rest:
        p //= 2
        if rest >= p:
            out.append(p)
            rest -= p
    return out


def two_level(F, E, zero_at=()):
    """Target 0 <- a_1 .. a_F (out-degree 1) <- sources b_j whose out-degrees are powers(E); b_j's edges go to a_i in turn
    (every second source with four or more edges sends two of them to the same a_i), never to the a_i listed in
    `zero_at`, which keep in-degree 0.  Level 2 is a frontier of F entries with E edges; b_j receives dout equal adds of
    0.25 / dout in that level: with R_STRICT the crossing falls strictly inside every run of four or more, with R_TIE the
    running sum equals rmax after an add and crosses on the next (runs of two or more), and b_j's reserve 0.125 equals
    rmax.  The frontier's order is the order of the appends, which the device does not promise: zero_at names positions
    in edge order."""
    fan_outs = powers(E)
    S = len(fan_outs)
    edges = [(i, 0) for i in range(1, F + 1)]
    ok = [i for i in range(1, F + 1) if (i - 1) not in set(zero_at)]
    cur = 0
    for j, d in enumerate(fan_outs):
        to = [ok[(cur + i) % len(ok)] for i in range(d)]
        if j % 2 == 1 and d >= 4:
            to[1] = to[0]
        cur += d
        edges += [(F + 1 + j, a) for a in to]
    n = 1 + F + S
    return Gadget("two%d_%d" % (F, E), n, edges, {R_STRICT: (n, [1, F, S], [F, E, 0]), R_TIE: (n, [1, F, S], [F, E, 0])})


def deep(d, W):
    """Target 0 <- a_1 .. a_d (out-degree 1), a_1 <- W sources of out-degree 1: a search of in-degree d that touches
    1 + d + W nodes, W of them in level 2 - what the in-degree routes to the wrong table.  With R_FAN the sources' adds
    (0.25) equal rmax and none crosses."""
    edges = [(i, 0) for i in range(1, d + 1)] + [(d + 1 + i, 1) for i in range(W)]
    return Gadget("deep%d_%d" % (d, W), 1 + d + W, edges, {R_FAN: (1 + d + W, [1, d], [d, W])})


class Design:
    """A graph, the gadgets in it (target ids are the gadgets' positions) and the thresholds it is run at."""

    def __init__(self, name, G, gadgets, rmaxes, ties):
        self.name, self.G, self.gadgets, self.rmaxes, self.ties = name, G, gadgets, rmaxes, ties
        self.targets = {g.name: i for i, g in enumerate(gadgets)}

    def __repr__(self):
        return self.name


def compose(name, gadgets, rmaxes, ties):
    """The gadgets side by side: gadget i's target is node i, its other nodes follow behind all targets."""
    K = len(gadgets)
    at = K
    src, dst = [], []
    for i, g in enumerate(gadgets):
        ids = [i] + list(range(at, at + g.n - 1))
        at += g.n - 1
        src += [ids[u] for u, _ in g.edges]
        dst += [ids[v] for _, v in g.edges]
    return Design(name, Graph(at, src, dst), gadgets, rmaxes, ties)


# ------------------------------------------------------------------ the designs
FAN_FRONTIERS = [127, 128, 129, 257, 511, 512, 513, 1023, 1024, 1025]        # N - 1: FRONT and kDnStage edges
FAN_SIZES = sorted(set([383, 384, 385, 1535, 1536, 1537] + [f + 1 for f in FAN_FRONTIERS]))   # N: give-up loads
TWO_LEVELS = [(128, 255), (128, 256), (128, 257), (129, 255), (129, 256), (129, 257),        # small table: 4 * 64
              (512, 1023), (512, 1024), (512, 1025), (1025, 1023), (1025, 1024), (1025, 1025)]  # large: 4 * 256
# dense tier, PPRHIP_APBS_CHUNK=16: level 2 of kDnShareMin - 1 and of kDnShareMin chunks, and one of two chunks whose
# frontier is above kDnStage (posted whatever its chunk count)
TWO_LEVELS_DENSE = [(129, 16 * (DN_SHARE_MIN - 1)), (129, 16 * (DN_SHARE_MIN - 1) + 1), (1025, 20)]
ROUTING_DEGREES = [0, 1, 0, 3, 4, 0, 0, 11, 12, 13, 0, 1, 3, 0, 4, 11, 0, 12, 0, 13, 0, 0]
ROUTING_DEEP = {37: (3, 400), 101: (4, 400), 200: (11, 1600), 290: (12, 1600)}   # position: (in-degree, W)
ROUTING_TARGETS = 300

_designs = {}


def _zero_at(F):
    front = SMALL_FRONT if F <= 129 else LARGE_FRONT
    return sorted({0, front - 1, front, F - 1} & set(range(F))) + ([front + 1] if front + 1 < F - 1 else [])


def design(name):
    if name in _designs:
        return _designs[name]
    if name == "fans":
        D = compose(name, [fan(N) for N in FAN_SIZES], [R_FAN, R_FAN_TIE], {R_FAN: "reserve", R_FAN_TIE: "both"})
    elif name == "levels":
        D = compose(name, [two_level(F, E, _zero_at(F)) for F, E in TWO_LEVELS + TWO_LEVELS_DENSE], [R_STRICT, R_TIE],
                    {R_STRICT: "none", R_TIE: "both"})
    elif name == "routing":
        gs = [deep(*ROUTING_DEEP[i]) if i in ROUTING_DEEP else fan(1 + ROUTING_DEGREES[i % len(ROUTING_DEGREES)])
              for i in range(ROUTING_TARGETS)]
        D = compose(name, gs, [R_FAN], {R_FAN: "both"})
    elif name == "capf":
        D = compose(name, [fan_loop(CAPF_FRONT), fan(CAPF_FRONT + 1)], [R_FAN],
                    {R_FAN: {"fanloop%d" % CAPF_FRONT: "both", "fan%d" % (CAPF_FRONT + 1): "reserve"}})
    elif name == "colliders":
        D = colliders()
    elif name == "hot":
        D = hot()
    elif name == "crowd_small":
        D = crowd(SMALL_LIMIT + 1, [(2048, "big"), (2048, "small"), (256, "small")])
    elif name == "crowd_large":
        D = crowd(LARGE_LIMIT + 1, [(512, "big"), (512, "small"), (128, "small")])
    else:
        raise KeyError(name)
    _designs[name] = D
    return D


CAPF_FRONT = 40   # the frontier of the cap_f cases
DESIGNS = ["fans", "levels", "routing", "capf", "colliders", "hot", "crowd_small", "crowd_large"]


# ------------------------------------------------------------------ colliders
def slot(u, cap):
    """ap_slot's home slot: ((u * 2654435761) >> 7) & (cap - 1) in uint32 arithmetic."""
    return (((u * 2654435761) & 0xFFFFFFFF) >> 7) & (cap - 1)


def probe_occupancy(ids, cap):
    """The slots linear probing (s + 1) & (cap - 1) fills with `ids`; the set does not depend on the insertion order."""
    used = set()
    for u in ids:
        s = slot(u, cap)
        while s in used:
            s = (s + 1) & (cap - 1)
        used.add(s)
    return used


COLLIDER_N = 65536
COLLIDER_COUNT = 40


def collider_ids(cap, count=COLLIDER_COUNT, avoid=()):
    ids = [u for u in range(COLLIDER_N) if slot(u, cap) >= cap - 2 and u not in avoid]
    assert len(ids) >= count
    return ids[:count]


def colliders():
    """65 536 nodes, nearly all isolated.  Target 0's in-neighbours have their home slot at 2046 or 2047 of the large
    table, target 1's at 510 or 511 of the small one (40 each, out-degree 1): the probe chains wrap through slot 0.
    Needs internal id == caller's id (PPRHIP_RELABEL=0)."""
    big = collider_ids(LARGE_CAP, avoid={0, 1})
    small = collider_ids(SMALL_CAP, avoid={0, 1} | set(big))
    G = Graph(COLLIDER_N, big + small, [0] * len(big) + [1] * len(small))
    c = {R_FAN: (COLLIDER_COUNT + 1, [1, COLLIDER_COUNT], [COLLIDER_COUNT, 0])}
    D = Design("colliders", G, [Gadget("collide%d" % LARGE_CAP, 0, [], c), Gadget("collide%d" % SMALL_CAP, 0, [], c)],
               [R_FAN], {R_FAN: "reserve"})
    D.ids = {LARGE_CAP: big, SMALL_CAP: small}
    return D


# ------------------------------------------------------------------ hot ids of the dense tier
HOT_TARGETS = (10, 100)
HOT_SOURCES = (HOT_TEST - 1, HOT_TEST, 20, 300)
R_HOT = 1.0 / 32


def hot():
    """512 nodes, ids kept (PPRHIP_RELABEL=0), for PPRHIP_APBS_HOT=64 and PPRHIP_APBS_CHUNK=16.  Targets 10 (hot) and
    100 (not hot), each <- 16 a_i (ids from 128 / 160, out-degree 1) <- the sources 63, 64, 20 and 300, whose 64
    out-edges are: one to each a_i of both targets, one to each target itself, the rest to node 400.
    Level 1 (20 edges, two chunks: stays on its workgroup) leaves 2^-7 on every source - in LDS for 63 and 20;
    level 2 (64 edges = kDnShareMin chunks: posted, hot residues spilled and filled) adds 16 times 2^-8: the running sum
    equals rmax = 1/32 after the sixth add and crosses on the seventh, for ids hot_n - 1 and hot_n in the same level."""
    src, dst = [], []
    for t, a0 in zip(HOT_TARGETS, (128, 160)):
        for i in range(16):
            src.append(a0 + i); dst.append(t)
            for b in HOT_SOURCES:
                src.append(b); dst.append(a0 + i)
        for b in HOT_SOURCES:
            src.append(b); dst.append(t)
    for b in HOT_SOURCES:
        src += [b] * 30
        dst += [400] * 30
    c = {R_HOT: (21, [1, 16, 4], [20, 64, 0])}
    D = Design("hot", Graph(512, src, dst), [], [R_HOT], {R_HOT: "residue"})
    D.targets = {"hot%d" % t: t for t in HOT_TARGETS}
    D.gadgets = [Gadget("hot%d" % t, 0, [], c) for t in HOT_TARGETS]
    return D


# ------------------------------------------------------------------ crowd
def crowd(big_n, groups):
    """Many gadgets in one range so that some workgroup of a table kernel runs one search after another and must find
    its table clean: fans of `big_n` nodes (they outgrow the table, which then clears every slot) between fans of 5 (cleared
    by the used list).  groups: (targets, kind) - the targets of a group share their sources, whose out-degree is the
    group's size (a power of two), so an add is 0.5 / size.  rmax is 3/4 of the smallest add: every source crosses and is
    popped, the sources of the largest groups keep a reserve (half an add) below rmax and are not emitted, those of a
    group of at most 2/3 that size are.  The call's entries - one per target and the small groups' sources - then stay
    far below the 65 536 records the driver's buffer holds at least, so no search is run again for want of room and the
    counters are exact.  The groups' targets are dealt out in turn.
    The small table's grid is at most 8 workgroups per CU, the large one's 2: with more than 8 * MAX_CUS = 4096 (2 *
    MAX_CUS = 1024) targets in the kernel's list some workgroup takes a second one on any part of at most MAX_CUS CUs
    (4096 targets would only equal the largest grid)."""
    T = sum(g[0] for g in groups)
    order, left = [], [g[0] for g in groups]
    while len(order) < T:
        for gi in range(len(groups)):
            if left[gi]:
                left[gi] -= 1
                order.append(gi)
    members = [[t for t, gi in enumerate(order) if gi == k] for k in range(len(groups))]
    src, dst, at = [], [], T
    kinds = {}
    for (size, kind), ts in zip(groups, members):
        nsrc = (big_n if kind == "big" else 5) - 1
        for s in range(at, at + nsrc):
            src += [s] * size
            dst += ts
        at += nsrc
        for t in ts:
            kinds[t] = (nsrc + 1, size)
    rmax = 0.375 / max(g[0] for g in groups)
    D = Design("crowd%d" % big_n, Graph(at, src, dst), [], [rmax], {rmax: "none"})
    D.kinds = kinds                                  # target -> (nodes its search touches, its group's size)
    D.targets = {"all": (0, T)}
    D.T = T
    return D


def crowd_claim(D, t):
    N, _ = D.kinds[t]
    return (N, [1, N - 1], [N - 1, 0])


# ------------------------------------------------------------------ cases of a design: (label, lo, hi, rmax, claims)
def cases(D):
    """Every (label, lo, hi, rmax, {target: (touched, frontier sizes, E per level)}) the design is queried at."""
    out = []
    for rmax in D.rmaxes:
        if D.name.startswith("crowd"):
            out.append(("all", 0, D.T, rmax, {t: crowd_claim(D, t) for t in range(D.T)}))
        elif D.name == "routing":
            out.append(("all", 0, len(D.gadgets), rmax, {i: g.claims[rmax] for i, g in enumerate(D.gadgets)}))
        else:
            for g in D.gadgets:
                t = D.targets[g.name]
                out.append((g.name, t, t + 1, rmax, {t: g.claims[rmax]}))
    return out
