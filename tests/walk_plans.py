"""Walk plans with every entry's walk count set from outside (helper of test_walk_plans_design.py and
test_gpu_walk_plans.py; DESIGN.md 3 "Designed walk plans").

A seeded FORA query with n_rounds = 1 pushes its live seeds once, whatever the threshold (the first frontier is the live
seeds, in the engine and in the twin alike), so a query never plans its walks straight from the seed weights.  The plans
here therefore go through one hop that is exact: the graph is an R-MAT body plus one seed node per body node with
out-edges (its carrier), the seed's single out-edge pointing at the carrier.  With a first threshold that no carrier
meets the push is that one level: seed i leaves alpha * q_i as its own reserve and (1 - alpha) * q_i - one addition to
zero - as the residue of carrier i, and the walk plan has one entry per carrier, in carrier order.  With weights
w_i = c_i - 0.5 (W = sum w_i an integer for an even number of seeds) and omega with omega * rsum in the middle of
[W, W + 1), entry i gets ceil(c_i - 0.5 +- rounding) = c_i walks.  A dead-end seed (a seed node without its edge) never
enters a frontier and makes no entry; it takes reserve by the closed form of DESIGN.md 2.5.

Nothing here needs a device."""
import math

import numpy as np

ALPHA = 0.15
TOL_MC = 1e-9
WALK_SEED = 3
N_DEAD = 4           # dead-end seed nodes per graph
GRID_REF = 4096      # 256 CUs x 16 waves: the grid the printed share refers to
GRID_SIDE = 1024     # ... x 4 waves: a walk phase of a batched call (fora.cpp: side_walk_waves), an inference - no
                     # counter shows a launch's grid, and the tests may not read the CU count
WIDE = 20            # "scale" of the built body graph (PlanGraph)


# ------------------------------------------------------------------ graphs
class PlanGraph:
    """R-MAT body of 2^scale nodes + a seed node per live body node + N_DEAD seed nodes without an edge."""

    def __init__(self, pkg, scale):
        self.scale = scale
        self.n0 = 1 << scale
        if scale == WIDE:
            # a built body for plans of more entries than an R-MAT of test size has live nodes: out-degrees 0..3 (a
            # quarter of the nodes are dead ends), uniform targets
            rng = np.random.default_rng(20)
            src = np.repeat(np.arange(self.n0, dtype=np.int32), rng.integers(0, 4, self.n0))
            dst = rng.integers(0, self.n0, src.size).astype(np.int32)
        else:
            src, dst = pkg.rmat_edges(scale, 16, 1)
        deg = np.bincount(src, minlength=self.n0)
        self.live = np.nonzero(deg > 0)[0].astype(np.int64)          # carriers, ascending
        self.n = self.n0 + self.live.size + N_DEAD
        self.host = pkg.HostCsr(self.n, np.concatenate([src, (self.n0 + np.arange(self.live.size)).astype(np.int32)]),
                                np.concatenate([dst, self.live.astype(np.int32)]))
        self.deg = np.diff(self.host.out_rp.astype(np.int64))
        assert np.array_equal(self.deg[:self.n0], deg) and np.all(self.deg[self.n0:self.n0 + self.live.size] == 1)
        assert np.all(self.deg[self.n - N_DEAD:] == 0)
        self.seed_of = np.full(self.n0, -1, dtype=np.int64)
        self.seed_of[self.live] = self.n0 + np.arange(self.live.size)
        self.dead_seeds = np.arange(self.n - N_DEAD, self.n, dtype=np.int64)

    def top(self, count):
        """The `count - 1` carriers of highest out-degree (ties by id) and the first one of a lower degree than all of
        them - the one entry a density can cut short alone -, ascending ids."""
        order = self.live[np.lexsort((self.live, -self.deg[self.live]))]
        d = self.deg[order]
        if count < 2 or not np.any(d[count - 1:] < d[count - 2]):     # (no lower degree left: the plain top `count`)
            return np.sort(order[:count])
        low = count - 1 + int(np.argmax(d[count - 1:] < d[count - 2]))
        return np.sort(np.concatenate([order[:count - 1], order[low:low + 1]]))

    def with_degrees(self, degrees):
        """Carriers of ascending ids whose out-degrees are `degrees`, entry by entry."""
        out, last = [], -1
        for want in degrees:
            cand = self.live[(self.live > last) & (self.deg[self.live] == want)]
            assert cand.size, "no carrier of degree %d behind node %d" % (want, last)
            last = int(cand[0])
            out.append(last)
        return np.array(out, dtype=np.int64)

    def equal_degree(self, count, d):
        c = self.live[self.deg[self.live] == d]
        assert c.size >= count
        return c[:count]


_graphs = {}


def plan_graph(pkg, scale):
    key = (pkg.__name__, scale)
    if key not in _graphs:
        _graphs[key] = PlanGraph(pkg, scale)
    return _graphs[key]


# ------------------------------------------------------------------ plans
class Plan:
    def __init__(self, name, scale, counts, carriers="top", n_dead=0, dup=False):
        self.name, self.scale, self.counts = name, scale, np.asarray(counts, dtype=np.int64)
        self.carriers, self.n_dead, self.dup = carriers, n_dead, dup
        assert self.counts.size % 2 == 0 and self.counts.min() >= 1
        self.total = int(self.counts.sum())

    def __repr__(self):
        return self.name


LARGE = 700_000        # walks of a large plan whose entries all have >= 63 walks (see sensitivity())
LARGE_ONES = 340_000   # ... of one that holds entries of a single walk beside larger ones
ONES_WIDE = 600_000    # entries of the widest all-ones plan


def _even(x):
    return x - x % 2


def _mixed(total, seed, run=130):
    """Family D: draws from the set, with runs of `run` ones directly behind and directly before a large entry; a
    plan that goes on to `total` gets such a run behind every 40 000 it draws."""
    rng = np.random.default_rng(seed)
    pool = np.array([1, 1, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 40000])
    out = [int(x) for x in rng.choice(pool[:-1], 24)] + [40000] + [1] * run + [1000] + [1] * (run + 1) + [40000, 2, 129]
    while sum(out) < total:
        out.append(int(rng.choice(pool if sum(out) + 40000 + run < total else pool[:-1])))
        if out[-1] == 40000:
            out += [1] * run
    if len(out) % 2:
        out.append(1)
    return out


def all_plans():
    p = []
    for s in (62, 64, 66, 126, 128, 130):
        p.append(Plan("A-ones-%d" % s, 12, [1] * s))
    for s in (4096, 4098, 20000):
        p.append(Plan("A-ones-%d" % s, 15, [1] * s))
    # 0.7225 / S >= 1000 * TOL_MC allows 722 500 entries of one walk: 600 000 give every wave of 4 096 a window of 128
    # one-walk entries with a window behind it, and every wave of 1 024 four such windows
    p.append(Plan("A-ones-%d" % ONES_WIDE, WIDE, [1] * ONES_WIDE))
    for w in (64, 65, 128, 129, 8193):
        p.append(Plan("B-giant-%d" % w, 12, [w - 1, 1]))
    p.append(Plan("B-giant-%d" % (LARGE_ONES + 1), 15, [LARGE_ONES, 1]))
    for c in (63, 64, 65, 127, 128, 129, 191, 192, 193):
        p.append(Plan("C-blocks-%d-small" % c, 12, [c] * 12, carriers=("equal", 2)))
        p.append(Plan("C-blocks-%d-large" % c, 15, [c] * _even(LARGE // c + 2)))
    p.append(Plan("D-mixed-small", 12, _mixed(0, 5)))
    p.append(Plan("D-mixed-large", 15, _mixed(LARGE_ONES, 6, run=300)))
    for name, c in (("2", [1, 1]), ("63", [30, 2, 30, 1]), ("64", [1, 31, 31, 1]), ("65", [33, 1, 1, 30]),
                    ("127", [100, 1, 25, 1])):
        p.append(Plan("E-tiny-" + name, 12, c))
    # capacity cases on purpose: the one entry a density cuts short ends on walk 64 / 128, a wave's first walk (equal
    # degrees, so the largest count is cut first and alone); two degree classes with ceil(d * rho) = c - 1 in both
    p.append(Plan("G-first-64", 12, [10, 55, 20, 3], carriers=("equal", 2)))
    p.append(Plan("G-first-128", 12, [28, 101, 6, 1], carriers=("equal", 2)))
    p.append(Plan("H-two-degrees", 12, [65, 129, 129, 65, 65, 129] * 4, carriers=("degrees", [2, 4, 4, 2, 2, 4] * 4)))
    p.append(Plan("F-dead-dup", 12, [5, 1, 64, 3, 129, 2], n_dead=2, dup=True))
    p.append(Plan("F-dead-dup-wide", 12, [65] * 40 + [1] * 130 + [700, 2], n_dead=3, dup=True))
    return p


PLANS = {p.name: p for p in all_plans()}
LARGE_PLANS = [n for n, p in PLANS.items() if p.total >= LARGE_ONES - 2000]


# ------------------------------------------------------------------ the designer
class Design:
    """Everything a query of plan `p` on graph `G` needs, and what it must give."""

    def __init__(self, orc, G, p):
        a = ALPHA
        c = p.counts
        S = c.size
        if p.carriers == "top":
            car = G.top(S)
        elif p.carriers[0] == "equal":
            car = G.equal_degree(S, p.carriers[1])
        elif p.carriers[0] == "degrees":
            car = G.with_degrees(p.carriers[1])
        else:                                      # ("ids", ascending carrier ids)
            car = np.asarray(p.carriers[1], dtype=np.int64)
            assert car.size == S and np.all(np.diff(car) > 0) and np.all(G.deg[car] > 0)
        self.plan, self.G, self.carriers, self.counts = p, G, car, c
        self.d = G.deg[car]
        w = c - 0.5
        W = float(w.sum())
        assert W == int(W)
        dead = G.dead_seeds[:p.n_dead]
        w_dead = np.full(dead.size, 1.5)
        total_w = W + float(w_dead.sum())
        p_live = w / total_w
        D = float(w_dead.sum()) / total_w
        den = 1.0 - (1.0 - a) * D
        self.seed_nodes, self.dead_nodes = G.seed_of[car], dead
        self.q = p_live / den                      # residue the live seeds start with
        self.dead_reserve = a * (w_dead / total_w) / den
        self.rsum = (1.0 - a) ** 2 * (1.0 - D) / den
        r_car = (1.0 - a) * self.q                 # residue of the carriers after the one level
        self.inc = (w / c) / W * self.rsum         # (p_i nrw / c_i) / nrw * rsum with nrw = W
        # the caller's list: seeds in a scrambled order, the first live seed (and the first dead one) listed twice
        ids = [int(x) for x in self.seed_nodes] + [int(x) for x in dead]
        ws = [float(x) for x in w] + [float(x) for x in w_dead]
        if p.dup:
            ids += [ids[0]]
            ws[0], extra = 0.25 * ws[0], 0.75 * ws[0]
            ws += [extra]
            if dead.size:
                ids += [int(dead[0])]
                ws[S], extra = 0.5, 1.0
                ws += [extra]
        perm = np.random.default_rng(S).permutation(len(ids))
        self.seeds = np.array(ids, dtype=np.int32)[perm]
        self.weights = np.array(ws)[perm]
        # omega * rsum in the middle of [W, W + 1); a first threshold twice what the fullest carrier holds per out-edge
        omega = (W + 0.5) / self.rsum
        rmax = 2.0 * float(np.max(r_car / self.d))
        self.pfail = 0.5
        L = math.log(2.0 / self.pfail)
        m = 1
        while 3.0 * m * omega * ((1.0 - a) * rmax) ** 2 - 2.0 < 1.0:
            m *= 2
        self.conf_m = m
        self.eps = 3.0 * m * omega * ((1.0 - a) * rmax) ** 2 - 2.0
        self.delta = (self.eps + 2.0) * L / self.eps / self.eps / omega
        self.rmax0, self.omega = orc.fora_whole_params(self.conf(orc.Conf), self.eps)
        assert abs(self.omega * self.rsum - (W + 0.5)) < 0.25, (self.omega * self.rsum, W)
        assert self.rmax0 > 1.5 * float(np.max(r_car / self.d)) and abs(self.rmax0 / rmax - 1.0) < 1e-9
        self.W = W
        self.woff = np.concatenate([[0], np.cumsum(c)])[:-1]
        self._walks = None
        self._twin = None

    def adopt(self, other):
        """The eps and conf of another design of the same W and dead-end weight (the queries of one batched call share
        them): its threshold must keep this plan's carriers out of the frontier as well."""
        assert other.W == self.W and other.rsum == self.rsum
        self.eps, self.delta, self.conf_m, self.pfail = other.eps, other.delta, other.conf_m, other.pfail
        self.rmax0, self.omega = other.rmax0, other.omega
        assert self.rmax0 > 1.5 * float(np.max((1.0 - ALPHA) * self.q / self.d))
        self._twin = None

    def conf(self, cls):
        cf = cls()
        cf.alpha, cf.delta, cf.pfail, cf.rsum, cf.min_delta, cf.k = ALPHA, self.delta, self.pfail, 1.0, 0.0, 0
        cf.n, cf.m = self.G.n, self.conf_m
        return cf

    # -- what the plan implies for the kernels
    def share(self, grid=GRID_REF):
        groups = (self.plan.total + 63) // 64
        return 64 * ((groups + grid - 1) // grid)

    def sensitivity(self):
        return float(self.inc.min()) / TOL_MC

    # -- references
    def walks(self, og):
        """(start, index, terminal, steps) of every walk of the plan, entry after entry, from the oracle's walker."""
        if self._walks is None:
            starts = np.repeat(self.carriers, self.counts).astype(np.int32)
            idx = (np.arange(self.plan.total, dtype=np.int64) - np.repeat(self.woff, self.counts)).astype(np.uint64)
            term, steps = og.random_walks(starts, idx, ALPHA, WALK_SEED, 0, True)
            self._walks = (starts, idx, term, steps)
        return self._walks

    def independent(self, og):
        """The expected vector rebuilt from the design alone (long double sums): alpha * q_i on seed i, the closed form
        on a dead-end seed, alpha * (1 - alpha) * q_i on carrier i, and inc_i at the terminal of each of its c_i walks."""
        ld = np.longdouble
        _, _, term, _ = self.walks(og)
        out = np.zeros(self.G.n, dtype=ld)
        out[self.seed_nodes] += ld(ALPHA) * self.q.astype(ld)
        out[self.dead_nodes] += self.dead_reserve.astype(ld)
        out[self.carriers] += ld(ALPHA) * (ld(1.0 - ALPHA) * self.q.astype(ld))
        order = np.argsort(term, kind="stable")
        ts = term[order]
        vals = np.repeat(self.inc, self.counts)[order].astype(ld)
        first = np.nonzero(np.concatenate([[True], ts[1:] != ts[:-1]]))[0]
        out[ts[first]] += np.add.reduceat(vals, first)
        assert abs(float(out.sum()) - 1.0) < 1e-12
        return out.astype(np.float64)

    def twin(self, orc, og):
        if self._twin is None:
            self._twin = og.fora_whole_seeds(self.seeds, self.eps, ALPHA, seed=WALK_SEED, weights=self.weights,
                                             n_rounds=1, conf=self.conf(orc.Conf))
        return self._twin

    # -- the walk index: densities that put cap(v) = ceil(d_out(v) * rho) where the plan wants it
    def caps(self, rho):
        return np.ceil(self.d.astype(np.float64) * rho).astype(np.int64)

    def usage(self, rho):
        cap = self.caps(rho)
        served = int(np.minimum(self.counts, cap).sum())
        return served, self.plan.total - served

    def overflow_steps(self, og, rho):
        _, idx, _, steps = self.walks(og)
        over = idx.astype(np.int64) >= np.repeat(self.caps(rho), self.counts)
        return int(steps[over].astype(np.int64).sum())

    def densities(self):
        """[(label, rho)]: everything served; one overflow walk - the last walk of entry z - in the whole phase (z the
        entry of the largest (c - 1.5) / d; named share-first-over when that walk sits at a multiple of 64, a wave's first walk); every
        entry over by one; everything over but each entry's first walk.  A case the plan's counts and degrees cannot
        produce with one density is left out (every entry of a single walk is always served: cap >= 1)."""
        c, d = self.counts, self.d.astype(np.float64)
        out = [("served", float(np.max(c / d)) * (1.0 + 1e-9))]
        assert self.usage(out[0][1])[1] == 0
        # the entry a falling density cuts short first; the case exists when it is cut short alone
        ratio = np.where(c >= 2, (c - 1.5) / d, -1.0)
        z = int(np.argmax(ratio))
        if ratio[z] > 0 and self.usage(float(ratio[z]))[1] == 1:
            at_share_start = (self.woff[z] + c[z] - 1) % 64 == 0
            out.append(("%s-entry-%d" % ("share-first-over" if at_share_start else "one-over", z), float(ratio[z])))
        if c.min() >= 2:
            rho = float(np.min((c - 1) / d)) * (1.0 - 1e-9)
            if np.all(self.caps(rho) == c - 1):
                out.append(("each-over-by-one", rho))
        out.append(("all-over", 1e-9))
        assert np.all(self.caps(1e-9) == 1)
        return out


def replay(counts, grid):
    """What the waves of a `grid` meet on a plan, from the kernels' share rule alone: (windows of k_mc_walk that hold 128
    entries - jl = 127, the S.woff[128] cell decides where e goes - and have a window staged behind them in the same
    wave; chunks of k_index_serve that hold 64 entries - jl = 63, the 65th offset - with a chunk behind them; the
    largest number of windows a wave stages)."""
    counts = np.asarray(counts, dtype=np.int64)
    total = int(counts.sum())
    ends = np.cumsum(counts)
    per = 64 * (((total + 63) // 64 + grid - 1) // grid)

    def full_with_next(width):
        off = np.arange(0, per, width, dtype=np.int64)       # a wave's windows start at its share's first walk
        start = (np.arange(0, total, per, dtype=np.int64)[:, None] + off[None, :]).ravel()
        start = start[start < total]
        hi = np.minimum((start // per + 1) * per, total)
        follows = start + width < hi
        first = np.searchsorted(ends, start, side="right")
        last = np.searchsorted(ends, np.minimum(start + width, hi) - 1, side="right")
        return int(np.sum(follows & (last - first == width - 1)))

    return full_with_next(128), full_with_next(64), -(-min(per, total) // 128)


_designs = {}


def design(orc, pkg, name):
    key = (pkg.__name__, name)
    if key not in _designs:
        p = PLANS[name]
        _designs[key] = Design(orc, plan_graph(pkg, p.scale), p)
    return _designs[key]


_oracle_graphs = {}


def oracle_graph(orc, G):
    if id(G) not in _oracle_graphs:
        h = G.host
        _oracle_graphs[id(G)] = orc.OracleGraph(h.n, h.out_rp, h.out_ci, h.in_rp, h.in_ci)
    return _oracle_graphs[id(G)]
