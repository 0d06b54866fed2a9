"""Designed graphs and a plain reference for the resumable top-k push (pprhip_fwdpush_topk_reset / _round; the same code
runs under fora_topk, fora_batch_topk and the query stream) and the state it carries between rounds.  Helper of
test_topk_round_designs.py (CPU) and test_gpu_topk_round_designs.py; nothing in this file needs a device.

The reference (`rounds`) is Forward_Push.forward_push_topk in frontier-synchronous Jacobi levels over the caller's ids,
with no layout, tile or bit word in it.  Between rounds it keeps three things:

  the parked set   Q_next as a set.  An add that leaves a node at r / d >= min_rmax parks it (whether or not the node
                   joins the round's queue as well); the source is parked at reset.
  the round start  A parked node that is active at the round's rmax starts the round and leaves the set; a parked node
                   below min_rmax is dropped; every other parked node stays parked.
  the armed set    Only in a round with rmax < min_rmax: the nodes that meet rmax at round start without being parked.
                   An armed node joins the queue with its first mass, exactly once; every other node joins when an add
                   takes it across rmax.  A round with rmax >= min_rmax arms nothing.

A level pops every frontier node at its residue at level start (alpha * r to the reserve), lands the contributions, and
lands the level's dead-end mass on the source behind them.  A node is active at a threshold t iff r / d >= t (a dead
end iff r > 0).  Per round the reference returns both vectors, the residue sum, the start set, the dropped nodes, the
armed set, the armed joins and a per-level trace, from which `Round.totals` derives the counters of pprhip_stats_t as
sparse_level_designs.Run.totals does (a level of nf entries and ef edges runs dense iff nf + ef >= K).

Mutants (MUTANTS) are wrong references, used only to prove that the designs can tell them apart:
  no_arm       the crossing rule only
  arm_twice    an armed node joins again on its second mass of the same level
  arm_stale    the armed set of the previous round is kept
  keep_parked  a parked node below min_rmax is not dropped
  no_park      a push never parks

Exact arithmetic.  alpha = 0.5, every out-degree is a power of two and every threshold a dyadic rational, so every
residue, reserve and contribution is a short dyadic rational, every sum is exact in any order and a device result equals
the reference bit for bit; the CPU tests prove it per design (the float run equals the Fraction run entry by entry).

How the designs are made (Kit).  The source's 64 out-edges all enter a hub of out-degree 2^h that ties at the first
round's rmax, so every hub edge carries one unit u = 2^-(h + 2).  A node fed k hub edges with out-degree d holds k u and
sits at (k / d) u; with the rounds R1 = 2u, R2 = u/2 (both >= min_rmax = u/8), R3 = u/32, R4 = u/128 (both below) the
pair (k, d) decides what the node is at each round start (ROLES).  Hub edges a design has to spare go into absorbers of
out-degree 512 (self loops) that hold three units at the most and never meet a threshold.  Out-edges a node has to
spare are self loops.

The constants the designs sit on are restated here from kernels_frontier.hip (k_seed_list_topk), kernels_push.hip and
push_device.hpp (take_armed)."""
import functools
import math

import numpy as np

from sparse_level_designs import ALPHA, PUSH_TILE, WG_CAP, COMB_ON, COMB_OFF, Design, Net   # noqa: F401 (re-exported)

SEED_ITEMS = 8                    # kSeedItems: nodes per thread of k_seed_list_topk (one armed byte, one 8-byte flag word)
SEED_TILE = 256 * SEED_ITEMS      # nodes per workgroup turn of k_seed_list_topk
ARMED_WORD = 32                   # take_armed works on 32-bit words
BOUNDARIES = (8, 32, 64, 256, 2048)   # first ids of: a thread group, an armed word, a wave's 64 nodes, 256, a tile
SIDE = 6                          # ids on each side of a boundary that a positions design fills with roles
MUTANTS = ("no_arm", "arm_twice", "arm_stale", "keep_parked", "no_park")
COUNTERS = ("levels", "dense_levels", "pops", "dense_nodes", "edge_pushes", "enqueues", "dead_end_pops")


# ------------------------------------------------------------------ the reference
class Lv:
    """One level: nf entries (front, in order) with ef edges, `dead` dead-end pops, enq nodes joined the next frontier;
    recv: {node: adds it received}; joins: {node: (as an armed node, adds it received in the level, distinct frontier
    nodes they came from)}; parked: nodes an add of the level parked; park_ties: those left on r / d == min_rmax
    exactly; src_armed: the level's dead-end mass landed on the source and the source joined as an armed node."""
    __slots__ = ("nf", "ef", "dead", "enq", "dense", "front", "recv", "joins", "parked", "park_ties", "src_armed")


class Round:
    """One round: min_rmax, rmax, below (rmax < min_rmax); start, dropped, stayed: the three ways of the parked set at
    round start; armed: the armed set at round start; armed_joins; trace; reserve, residue: {node: value} behind the
    round; rsum."""

    def vector(self, which, n):
        out = np.zeros(n)
        for v, x in getattr(self, which).items():
            out[v] = float(x)
        return out

    def totals(self):
        """The counters of pprhip_stats_t a round with this trace reports."""
        t = self.trace
        sp = [L for L in t if not L.dense]
        return dict(levels=len(t), dense_levels=len(t) - len(sp), pops=sum(L.nf for L in sp),
                    dense_nodes=sum(L.nf for L in t if L.dense), edge_pushes=sum(L.ef for L in sp),
                    enqueues=sum(L.enq for L in t), dead_end_pops=sum(L.dead for L in t))

    def joined(self):
        return {u for L in self.trace for u in L.joins}

    def armed_joined(self):
        return {u for L in self.trace for u, j in L.joins.items() if j[0]}


def rounds(D, thresholds=None, num=float, mutant=None, alpha=ALPHA):
    """The resumable top-k push of design D from D.start over `thresholds` [(min_rmax, rmax)] (None: D.rounds) in the
    number type `num`; a list of Round."""
    assert mutant is None or mutant in MUTANTS
    thresholds = D.rounds if thresholds is None else thresholds
    rp, ci = D.csr
    dout = D.dout.tolist()
    a, one, zero = num(alpha), num(1), num(0)
    s = D.start
    res, rsv, parked, armed = {}, {}, {s}, set()
    out = []

    def active(r, u, t):
        d = dout[u]
        return r / num(d) >= t if d else r > zero

    for rnd, (mn, rm) in enumerate(thresholds):
        MN, RM = num(mn), num(rm)
        R = Round()
        R.min_rmax, R.rmax, R.below, R.trace, R.armed_joins = mn, rm, rm < mn, [], 0
        if dout[s] == 0:   # Forward_Push.java:149-153
            R.start, R.dropped, R.stayed, R.armed = [], [], [], set()
            R.reserve, R.residue, R.rsum = {s: one}, {}, zero
            out.append(R)
            continue
        if rnd == 0:
            res[s] = one
        was_parked = sorted(parked)
        R.start = [v for v in was_parked if active(res.get(v, zero), v, RM)]
        R.dropped = [v for v in was_parked if v not in R.start and not active(res.get(v, zero), v, MN)]
        R.stayed = [v for v in was_parked if v not in R.start and v not in R.dropped]
        now = {v for v, r in res.items() if v not in parked and active(r, v, RM)} if R.below else set()
        armed = (armed | now) if mutant == "arm_stale" else now
        if mutant == "no_arm":
            armed = set()
        R.armed = set(armed)
        parked -= set(R.start)
        if mutant != "keep_parked":
            parked -= set(R.dropped)
        front = list(R.start)
        while front:
            L = Lv()
            L.front = list(front)
            L.nf = len(front)
            L.ef = sum(rp[v + 1] - rp[v] for v in front)
            L.dense = D.K is not None and L.nf + L.ef >= D.K
            L.dead, L.joins, L.parked, L.park_ties, L.src_armed = 0, {}, set(), set(), False
            dead = zero
            pend = []
            for v in front:   # every frontier entry gives up its residue at level start
                r = res.get(v, zero)
                res[v] = zero
                rsv[v] = rsv.get(v, zero) + r * a
                d = rp[v + 1] - rp[v]
                if d == 0:
                    dead = dead + r * (one - a)
                    L.dead += 1
                    pend.append(None)
                else:
                    pend.append(((one - a) * r) / num(d))
            nxt, got, took = [], {}, {}

            def land(u, add, frm):
                old = res.get(u, zero)
                nw = old + add
                res[u] = nw
                g = got.setdefault(u, [0, set()])
                g[0] += 1
                g[1].add(frm)
                join = by_bit = False
                if not active(old, u, RM):
                    join = active(nw, u, RM)            # the crossing rule
                elif u in armed:
                    armed.discard(u)                    # the first mass of an armed node
                    join = by_bit = True
                    took[u] = 1
                elif mutant == "arm_twice" and took.get(u) == 1:
                    took[u] = 2
                    join = by_bit = True
                if join:
                    nxt.append(u)
                    if by_bit:
                        R.armed_joins += 1
                    L.joins.setdefault(u, by_bit)
                if mutant != "no_park" and active(nw, u, MN):
                    if u not in parked:
                        L.parked.add(u)
                    parked.add(u)
                return by_bit

            for v, c in zip(front, pend):
                if c is None:
                    continue
                for e in range(rp[v], rp[v + 1]):
                    land(ci[e], c, v)
            if dead > zero:   # Forward_Push.java:186-209: the level's dead-end mass lands on the source
                L.src_armed = land(s, dead, -1)
            L.recv = {u: g[0] for u, g in got.items()}
            L.joins = {u: (bit, got[u][0], len(got[u][1])) for u, bit in L.joins.items()}
            L.park_ties = {u for u in L.parked if dout[u] and res[u] == MN * num(dout[u])}
            L.enq = len(nxt)
            R.trace.append(L)
            front = nxt
        R.reserve = {v: x for v, x in rsv.items() if x != zero}
        R.residue = {v: x for v, x in res.items() if x != zero}
        R.rsum = math.fsum(R.residue.values()) if num is float else sum(R.residue.values(), zero)
        out.append(R)
    return out


_runs = {}


def run(D, num=float):
    """The reference rounds of a design, computed once and never changed."""
    key = (D.name, num)
    if key not in _runs:
        _runs[key] = rounds(D, None, num)
    return _runs[key]


def summary(D, rs=None):
    """One line per round for the tests' output."""
    out = []
    for i, R in enumerate(rs or run(D)):
        t = R.totals()
        out.append("%s round %d (min_rmax %.3g, rmax %.3g%s): start set %d, dropped %d, stayed %d, armed %d, armed joins %d,"
                   " levels %d (%d dense), pops %d, (nf, ef) %s"
                   % (D.name, i, R.min_rmax, R.rmax, ", below" if R.below else "", len(R.start), len(R.dropped),
                      len(R.stayed), len(R.armed), R.armed_joins, t["levels"], t["dense_levels"],
                      t["pops"] + t["dense_nodes"], [(L.nf, L.ef) for L in R.trace][:10]))
    return "\n".join(out)


# ------------------------------------------------------------------ building blocks
class Kit:
    """source (64 parallel edges; 16 where the hub has 16) -> hub -> nodes made by `node(k, d)`: k hub edges, out-degree d.  `link` spends
    out-edges; `finish` turns every out-edge left over into a self loop, rounds the hub up to a power of two with
    absorbers and fixes the unit."""

    def __init__(self, src_edges=64):
        self.net = Net()
        self.s, self.hub = self.net.one(), self.net.one()
        self.net.add(self.s, self.hub, src_edges)   # (1 / src_edges >= 2u: the source starts round 0)
        self.deg, self.used, self.fed, self.place = {}, {}, 0, {}

    def node(self, k, d, at=None):
        v = self.net.one()
        if k:
            self.net.add(self.hub, v, k)
            self.fed += k
        self.deg[v], self.used[v] = d, 0
        if at is not None:
            self.place[v] = at
        return v

    def link(self, v, to, times=1):
        self.net.add(v, to, times)
        self.used[v] += int(np.size(to)) * times
        assert self.used[v] <= self.deg[v], (v, self.used[v], self.deg[v])

    def finish(self, name, claims, n=None, K=None, rounds=None):
        for v, d in self.deg.items():
            if d > self.used[v]:
                self.net.add(v, v, d - self.used[v])
        h = (max(self.fed, 1) - 1).bit_length()
        spare = (1 << h) - self.fed
        while spare:
            k = min(3, spare)
            ab = self.net.one()
            self.net.add(self.hub, ab, k)
            self.net.add(ab, ab, 512)
            spare -= k
        u = 2.0 ** -(h + 2)
        D = Design(name, self.net, self.s, u, claims, K=K, place=dict(self.place), n=n)
        D.u = u
        D.rounds = rounds(u) if rounds else std_rounds(u)
        return D


def std_rounds(u):
    """R1 = 2u (the hub ties), R2 = u/2, both >= min_rmax = u/8; R3 = u/32, R4 = u/128, both below; R5 = u/64, below
    again behind a lower one: whatever is parked then lies below it, and the round is empty."""
    m = u / 8
    return [(m, 2 * u), (m, u / 2), (m, u / 32), (m, u / 128), (m, u / 64)]


# (k, d) of a node fed by the hub -> what it is at the start of the standard rounds (round numbers from 0)
ROLES = {
    "J": (2, 1),      # joins in round 0 (k/d >= 2), parked by the same add; popped, so dropped at round 1
    "S": (1, 1),      # parked in round 0 (1/2 <= k/d < 2): starts round 1
    "T": (1, 4),      # parked in round 0 (1/8 <= k/d < 1/2): stays at round 1, starts round 2
    "G": (0, 1),      # fed u/2 by S in round 1: parked and joined by that one add, popped; dropped at round 2; regains
                      # 11u/512 < R3 from A in round 2, so it is armed at round 3, and not in its start set
    "A": (1, 32),     # never parked: armed at round 2 (on a tie)
    "Q": (1, 512),    # quiet at every round start
}
SMALL_ROLES = dict(ROLES, J=(4, 1))   # (n = 13: the hub has no edge to spare)


def _side(kit, ids, order, roles=ROLES):
    """One side of a boundary: the roles of `order` on consecutive ids.  Returns {role: node}."""
    out = {}
    for role, at in zip(order, ids):
        k, d = roles[role]
        out[role] = kit.node(k, d, at=at)
    return out


def _wire(kit, sides, sink):
    """S -> its G; J, G -> the side's Q (or the sink); every T -> every A of the boundary (if there are two, the first
    over two parallel edges) and the rest to its Q; A -> its G, the rest self loops."""
    As = [sd["A"] for sd in sides if "A" in sd]
    for sd in sides:
        q = sd.get("Q", sink)
        if "S" in sd:
            kit.link(sd["S"], sd.get("G", q))
        for r in ("J", "G"):
            if r in sd:
                kit.link(sd[r], q)
        if "T" in sd:
            left = kit.deg[sd["T"]]
            for i, A in enumerate(As):
                t = 2 if i == 0 and len(As) == 2 else 1
                kit.link(sd["T"], A, t)
                left -= t
            kit.link(sd["T"], q, left)
        if "A" in sd and "G" in sd:
            kit.link(sd["A"], sd["G"])


def _engine(kit, G):
    """What the later rounds run on.
    T2 (1, 4) starts round 2 and hands u/4 to E over two edges and u/8 to the dead end L2, whose mass lands on the
    source in the next level.  The source holds 2u (from L1, a dead end fed 4 hub edges and popped in round 0): 2u / 64 =
    R3, so it is armed at round 2 and joins with L2's mass.
    E (d = 2: a self loop and Y) is parked on a tie and joined by T2's u/4, halves twice and is left parked at
    u/64 / 2 = R4: it starts round 3.  Y (d = 4) gathers 5u/64 in round 2, below R3, so it is armed at round 3, joins with
    E's u/256 and reaches X1 - an A node nobody reaches in round 2 - and G, dropped at round 2 and armed at round 3.
    X2 is armed at rounds 2, 3 and 4 and never reached.
    S3 (1, 1) starts round 1 and leaves P4 (d = 4) at u/8 / 4... = min_rmax exactly: parked on a tie without joining; it
    starts round 2."""
    T2, E, Y = kit.node(1, 4), kit.node(0, 2), kit.node(0, 4)
    X1, X2 = kit.node(1, 32), kit.node(1, 32)
    L1, L2 = kit.node(4, 0), kit.node(0, 0)
    S3, P4 = kit.node(1, 1), kit.node(0, 4)
    kit.link(T2, E, 2)
    kit.link(T2, L2)
    kit.link(E, Y)
    kit.link(Y, X1, 2)
    kit.link(Y, G)
    kit.link(S3, P4)
    return dict(T2=T2, E=E, Y=Y, X1=X1, X2=X2, L1=L1, L2=L2, S3=S3, P4=P4)


ORDERS = ("ATGSJQ", "QJSGTA", "TAQJSG", "GSJQAT", "SGATQJ", "JQTASG")


def positions(n, K=None):
    """Scenario 1: the six roles on both sides of every boundary that n leaves room for, so the role right below a
    boundary and the one right on it change from boundary to boundary; the last ids of n (n - 1 is an A node); an
    all-armed 32-bit word (96..127) fed in one level by the eight T nodes of one 8-byte flag word (128..135)."""
    small = n < 64
    kit = Kit(16 if small else 64)
    roles = SMALL_ROLES if small else ROLES
    sink = None if small else kit.node(1, 512)
    groups = []
    bounds = [b for b in BOUNDARIES if b <= n] + ([4096] if n >= 4096 else [])
    for k, b in enumerate(bounds):
        lo = list(range(b - SIDE, b))
        hi = list(range(b, min(b + SIDE, n)))
        lower, upper = ORDERS[k % 6], ORDERS[(k + 3) % 6]
        if len(hi) < SIDE:                      # a short upper side ends on the armed node
            upper = "TGSJ"[:len(hi) - 1] + "A"
        sides = [_side(kit, lo, lower, roles)]
        if hi:
            sides.append(_side(kit, hi, upper, dict(roles, T=(2, 8)) if small else roles))
        _wire(kit, sides, sink if sink is not None else sides[0]["Q"])
        groups.append((b, sides))
    word = flagword = eng = None
    if not small:
        word = [kit.node(1, 32, at=96 + i) for i in range(ARMED_WORD)]
        flagword = [kit.node(1, 4, at=128 + i) for i in range(SEED_ITEMS)]
        for i, t in enumerate(flagword):
            kit.link(t, np.array(word[4 * i:4 * i + 4]))
        eng = _engine(kit, groups[0][1][0]["G"])
    claims = ["P_roles_on_both_sides"]
    if not small:
        claims += ["P_all_armed_word", "P_all_parked_flag_word", "A_armed_joins_in_two_rounds_below",
                   "A_unreached_then_reached", "S_dead_end_mass_on_armed_source",
                   "K_parked_and_joined_by_one_add", "K_parked_without_joining_starts_next", "K_parked_on_tie",
                   "R_dropped_then_armed"]
    if n % SEED_ITEMS:
        claims += ["P_scalar_tail"]
    if n > SEED_TILE:
        claims += ["P_second_tile" if n >= SEED_TILE + SIDE else "P_tile_of_one_node"]
    if K:
        claims += ["L_armed_round_dense"]
    D = kit.finish("pos_%d%s" % (n, "_dense" if K else ""), claims, n=n, K=K)
    assert D.n == n, (D.n, n)
    at = lambda v: int(D.perm[v])
    D.groups = [(b, [{r: at(v) for r, v in sd.items()} for sd in sides]) for b, sides in groups]
    D.word = [at(v) for v in word] if word else None
    D.flagword = [at(v) for v in flagword] if flagword else None
    D.eng = {r: at(v) for r, v in eng.items()} if eng else None
    return D


def once():
    """Scenario 2 (n = 600).  Round 2 starts from T nodes (u/8 per edge) that reach A nodes (armed, (1, 32)):
    a2p by two parallel edges of one T, a2s by one edge each of two, a3 by two parallel edges and one more, a64 by four
    parallel edges each of sixteen (it ends at 9u / 32 >= min_rmax: an armed join that a later add of the level parks);
    the 32 nodes of the word 32..63 by one edge each of 32 different T nodes.
    The unreached: E (d = 2: a self loop and Y) is left parked at u/128 as in the positions designs; Y (d = 64) gathers
    5u/64; X (1, 32) is armed at round 2 and nobody reaches it.  Round 3 is (min_rmax, rmax) = (Rq / 2, Rq) with
    Rq = 21u / 16384: not below, so nothing is armed; E starts it, Y crosses Rq on the tie and pops, and X, which has met
    Rq all along without being parked or queued, receives Y's mass and must not join; the mass parks it (it meets that
    round's min_rmax), so it starts round 4, (u/8, u/128), instead of being armed there."""
    kit = Kit()
    sinks = []

    def sink():                      # a Q node takes the spare edges of at most eight T nodes
        if not sinks or sinks[-1][1] == 8:
            sinks.append([kit.node(1, 512), 0])
        sinks[-1][1] += 1
        return sinks[-1][0]

    def T(to, times):
        t = kit.node(1, 4)
        for x, k in zip(to, times):
            kit.link(t, x, k)
        left = 4 - sum(times)
        if left:
            kit.link(t, sink(), left)
        return t

    a2p, a2s, a3, a64 = (kit.node(1, 32, at=i) for i in (7, 8, 31, 64))
    word = [kit.node(1, 32, at=32 + i) for i in range(ARMED_WORD)]
    T([a2p, a3], [2, 2])
    T([a2s, a3], [1, 1])
    T([a2s], [1])
    for _ in range(16):
        T([a64], [4])
    for w in word:
        T([w], [1])
    T2, E, Y, X = kit.node(1, 4), kit.node(0, 2), kit.node(0, 64), kit.node(1, 32, at=95)
    kit.link(T2, E, 2)
    kit.link(T2, sink(), 2)
    kit.link(E, Y)
    kit.link(Y, X, 2)

    def rnds(u):
        m, rq = u / 8, 21 * u / 16384
        return [(m, 2 * u), (m, u / 2), (m, u / 32), (rq / 2, rq), (m, u / 128)]

    D = kit.finish("once", ["A_adds_2_parallel", "A_adds_2_several", "A_adds_3", "A_adds_64", "A_word_from_32_sources",
                            "A_armed_join_parked_by_a_later_add", "A_unreached_then_round_above_arms_nothing"],
                   n=600, rounds=rnds)
    at = lambda v: int(D.perm[v])
    D.ids = dict(a2p=at(a2p), a2s=at(a2s), a3=at(a3), a64=at(a64), X=at(X), Y=at(Y), E=at(E))
    D.word = [at(w) for w in word]
    return D


def tiles():
    """Scenario 6 (n = 2 300).  Round 2 (below min_rmax) starts from seven nodes (128, 1024) - parked on the tie
    k / d = 1/8 in round 0, staying at round 1 - and one T: 7 172 edges, more than two tiles of the two-launch level and
    too many for the one-workgroup kernel.  Each of the seven reaches the 32 armed nodes of the word 2048 + 32 .. + 63
    (the second tile of the round-start pass) over its first 32 edges, u/16 each, so every armed node is hit from four
    different tiles of the level and joins once."""
    kit = Kit()
    word = [kit.node(1, 32, at=SEED_TILE + 32 + i) for i in range(ARMED_WORD)]
    big = [kit.node(128, 1024, at=300 * i + 5) for i in range(7)]
    for b in big:
        kit.link(b, np.array(word))
    q = kit.node(1, 512)
    t = kit.node(1, 4)
    kit.link(t, word[0], 2)
    kit.link(t, q, 2)
    D = kit.finish("tiles", ["L_multi_tile_start_set"], n=2300)
    D.word = [int(D.perm[w]) for w in word]
    return D


# ------------------------------------------------------------------ features, by name
def _below(D):
    return [(i, R) for i, R in enumerate(run(D)) if R.below]


def _roles_on_both_sides(D):
    r = run(D)
    ok = True
    for b, sides in D.groups:
        if b + SIDE <= D.n:
            ok &= len(sides) == 2 and all(set(sd) == set(ROLES) for sd in sides)
        for sd in sides:
            ok &= all(lo < b for lo in sides[0].values()) and all(hi >= b for hi in sides[-1].values() if len(sides) == 2)
            if "S" in sd:
                ok &= sd["S"] in r[1].start
            if "J" in sd:
                ok &= sd["J"] in r[1].dropped and sd["J"] in r[0].joined()
            if "T" in sd:
                ok &= sd["T"] in r[1].stayed and sd["T"] in r[2].start
            if "G" in sd and "S" in sd:
                ok &= sd["G"] in r[2].dropped
            if "A" in sd:
                ok &= sd["A"] in r[2].armed and sd["A"] in r[2].armed_joined()
            if "Q" in sd:
                ok &= all(sd["Q"] not in x.start + x.dropped + x.stayed and sd["Q"] not in x.armed for x in r[:3])
    # the node right below a boundary and the node right on it: more than one role each
    return ok and (D.n < 64 or (len({next(k for k, v in s[0].items() if v == b - 1) for b, s in D.groups}) >= 3 and
                                len({next(k for k, v in s[1].items() if v == b) for b, s in D.groups if len(s) == 2}) >= 3))


def _all_armed_word(D):
    R = run(D)[2]
    return D.word == list(range(96, 128)) and any(
        all(u in L.joins and L.joins[u][0] for u in D.word) and
        len({v for v in L.front if set(D.csr[1][D.csr[0][v]:D.csr[0][v + 1]]) & set(D.word)}) >= 8 for L in R.trace)


def _scalar_tail(D):
    R = run(D)[2]
    last = [v for v in range(D.n - D.n % SEED_ITEMS, D.n)]
    return 0 < len(last) < SEED_ITEMS and D.n - 1 in R.armed_joined() and \
        (len(last) < 3 or (set(last) & set(R.start) and set(last) & set(R.dropped)))


def _adds(D, adds, srcs, node=None):
    return any(j[0] and j[1] == adds and j[2] == srcs and (node is None or u == node)
               for i, R in _below(D) for L in R.trace for u, j in L.joins.items())


def _unreached_then_reached(D):
    b = _below(D)
    return any(u in R1.armed and u not in R1.joined() and not any(u in L.recv for L in R1.trace) and i1 + 1 == i2 and
               u in R2.armed_joined() for (i1, R1), (i2, R2) in zip(b, b[1:]) for u in R1.armed)


def _round_above_arms_nothing(D):
    r = run(D)
    for i in range(1, len(r) - 1):
        if r[i - 1].below and not r[i].below and r[i].trace and not r[i].armed and r[i].armed_joins == 0:
            X = D.ids["X"]
            if X in r[i - 1].armed and not any(X in L.recv for L in r[i - 1].trace) and X not in r[i].joined() and \
                    any(X in L.recv for L in r[i].trace) and D.ids["Y"] in r[i].joined() and X in r[i + 1].start:
                return True
    return False


def _parked_then_joined_later_add(D):
    return any(j[0] and u in L.parked for i, R in _below(D) for L in R.trace for u, j in L.joins.items())


def _parked_and_joined(D):
    return any(u in L.parked and j[1] == 1 for R in run(D) for L in R.trace for u, j in L.joins.items())


def _parked_without_joining(D):
    r = run(D)
    return any(u not in R.joined() and u in r[i + 1].start
               for i, R in enumerate(r[:-1]) for L in R.trace for u in L.parked)


def _parked_on_tie(D):
    r = run(D)
    return any(u not in R.joined() and u in r[i + 1].start
               for i, R in enumerate(r[:-1]) for L in R.trace for u in L.park_ties)


def _dropped_then_armed(D):
    r = run(D)
    dout = D.dout
    for i in range(len(r) - 2):
        for g in r[i + 1].dropped:
            if any(g in L.parked and g in L.joins for L in r[i].trace) and g in r[i + 2].armed and \
                    g not in r[i + 2].start and \
                    r[i + 2].rmax * dout[g] <= r[i + 1].residue.get(g, 0.0) < r[i + 1].rmax * dout[g] and \
                    g in r[i + 2].armed_joined():
                return True
    return False


def _multi_tile(D):
    rp, ci = D.csr
    for i, R in _below(D):
        L = R.trace[0] if R.trace else None
        if L is None or L.ef < 2 * PUSH_TILE + 1 or L.nf + L.ef < WG_CAP:
            continue
        tiles_of, at = {}, 0
        for v in L.front:
            for e in range(rp[v], rp[v + 1]):
                tiles_of.setdefault(ci[e], set()).add(at // PUSH_TILE)
                at += 1
        if len({u >> 5 for u in D.word}) == 1 and min(D.word) >= SEED_TILE and \
                all(u in L.joins and L.joins[u][0] and len(tiles_of[u]) >= 3 for u in D.word):
            return True
    return False


def _armed_round_dense(D):
    R = run(D)[2]
    return bool(D.K) and R.below and R.armed_joins > 0 and R.trace and all(L.dense for L in R.trace) and \
        any(L.dense and any(j[0] for j in L.joins.values()) for L in R.trace)


FEATURES = {
    "P_roles_on_both_sides": _roles_on_both_sides,
    "P_all_armed_word": _all_armed_word,
    "P_all_parked_flag_word": lambda D: D.flagword == list(range(128, 136)) and set(D.flagword) <= set(run(D)[2].start),
    "P_scalar_tail": _scalar_tail,
    "P_second_tile": lambda D: any(v >= SEED_TILE for v in run(D)[2].start) and
    any(v >= SEED_TILE for v in run(D)[2].armed_joined()) and any(v >= SEED_TILE for v in run(D)[2].dropped),
    "P_tile_of_one_node": lambda D: D.n - 1 == SEED_TILE and D.n - 1 in run(D)[2].armed_joined(),
    "A_armed_joins_in_two_rounds_below": lambda D: sum(1 for i, R in _below(D) if R.armed_joins > 0) >= 2,
    "A_unreached_then_reached": _unreached_then_reached,
    "A_adds_2_parallel": lambda D: _adds(D, 2, 1, D.ids["a2p"]),
    "A_adds_2_several": lambda D: _adds(D, 2, 2, D.ids["a2s"]),
    "A_adds_3": lambda D: _adds(D, 3, 2, D.ids["a3"]),
    "A_adds_64": lambda D: _adds(D, 64, 16, D.ids["a64"]),
    "A_word_from_32_sources": lambda D: D.word == list(range(32, 64)) and any(
        all(u in L.joins and L.joins[u][0] for u in D.word) for i, R in _below(D) for L in R.trace),
    "A_armed_join_parked_by_a_later_add": _parked_then_joined_later_add,
    "A_unreached_then_round_above_arms_nothing": _round_above_arms_nothing,
    "S_dead_end_mass_on_armed_source": lambda D: any(L.src_armed and L.dead for i, R in _below(D) for L in R.trace),
    "K_parked_and_joined_by_one_add": _parked_and_joined,
    "K_parked_without_joining_starts_next": _parked_without_joining,
    "K_parked_on_tie": _parked_on_tie,
    "R_dropped_then_armed": _dropped_then_armed,
    "L_multi_tile_start_set": _multi_tile,
    "L_armed_round_dense": _armed_round_dense,
}

POSITION_SIZES = (2 * SEED_TILE + 5, 2 * SEED_TILE, SEED_TILE + 1, 13)
DENSE_K = 3      # every level but the source's own runs dense


@functools.lru_cache(maxsize=None)
def all_designs():
    ds = [positions(n) for n in POSITION_SIZES] + [positions(n, K=DENSE_K) for n in POSITION_SIZES] + [once(), tiles()]
    assert len({d.name for d in ds}) == len(ds)
    return {d.name: d for d in ds}


def whole_query_design():
    return all_designs()["pos_%d" % POSITION_SIZES[0]]
