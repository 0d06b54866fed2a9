"""Host references of the weighted seed-set and top-k calls (include/pprhip.h "weighted seed sets and top-k"), numpy,
no device, built on tests/weighted_ref.py: the seed table (p resolved for the dead-end seeds), the seeded weighted push
on plain Jacobi levels with dead-end mass landing on p, weighted FORA from a seed set, and the weighted top-k rounds.
`w` is always aligned with host.out_ci; `seeds` / `sw` are the caller's seed ids and seed weights (None: uniform)."""
import math

import numpy as np

import weighted_ref as wr


def _deg(host):
    return np.diff(host.out_rp.astype(np.int64))


def seed_p(n, seeds, sw=None):
    """p: the seed weights over their sum, duplicates summed, zero weights dropped (they stay zero)."""
    seeds = np.atleast_1d(np.asarray(seeds, dtype=np.int64))
    sw = np.ones(seeds.size) if sw is None else np.atleast_1d(np.asarray(sw, dtype=np.float64))
    p = np.bincount(seeds, weights=sw, minlength=n).astype(np.float64)
    return p / p.sum()


class SeedTable:
    """with D = the weight of the dead-end seeds, mass x landing on p gives a live seed i the
    residue x q_i, q_i = p_i / (1 - (1 - alpha) D), and a dead-end seed j the reserve x e_j, e_j = alpha p_j / (1 -
    (1 - alpha) D).  Every seed a dead end: e = p.  Nothing here reads the relationship weights."""

    def __init__(self, host, seeds, sw, alpha):
        self.p = seed_p(host.n, seeds, sw)
        deg = _deg(host)
        ids = np.flatnonzero(self.p > 0.0)
        self.live = ids[deg[ids] > 0]
        self.dead = ids[deg[ids] == 0]
        den = 1.0 - (1.0 - alpha) * float(self.p[self.dead].sum())
        self.q = self.p[self.live] / den
        self.e = self.p[self.dead].copy() if self.live.size == 0 else alpha * self.p[self.dead] / den


class SeededPush:
    """The state of a seeded weighted push (reserve, residue) and its levels.  start: r = q on the live seeds, reserve =
    e on the dead-end seeds."""

    def __init__(self, host, w, seeds, sw, alpha):
        self.host, self.alpha = host, alpha
        self.w = np.asarray(w, dtype=np.float64)
        _, self.W = wr.table(host, self.w)
        self.deg = _deg(host)
        self.t = SeedTable(host, seeds, sw, alpha)
        self.reserve = np.zeros(host.n)
        self.residue = np.zeros(host.n)
        self.residue[self.t.live] = self.t.q
        self.reserve[self.t.dead] = self.t.e
        self.levels = self.pops = 0
        self.level_sizes = []
        self.level_info = []  # per level: (frontier nodes, their out-edges, the dead-end mass that landed on p)

    def run(self, F, rmax):
        """weighted_ref.push_sync's levels from the frontier F at rmax to their end, with one change: a level's dead-end
        mass x lands on p inside the level - r(i) += x q_i for every live seed (tested with the same crossing rule),
        reserve(j) += x e_j for every dead-end seed."""
        host, alpha, deg, W, w, t = self.host, self.alpha, self.deg, self.W, self.w, self.t
        rp = host.out_rp.astype(np.int64)
        dst = host.out_ci[:host.m].astype(np.int64)
        reserve, residue = self.reserve, self.residue
        F = np.asarray(F, dtype=np.int64)
        while F.size:
            self.levels += 1
            self.pops += int(F.size)
            self.level_sizes.append(int(F.size))
            rc = residue[F].copy()
            residue[F] = 0.0
            reserve[F] = reserve[F] + rc * alpha
            dead = deg[F] == 0
            x = float((rc[dead] * (1.0 - alpha)).sum())
            lv = F[~dead]
            c = ((1.0 - alpha) * rc[~dead]) / W[lv]
            old = residue.copy()
            if lv.size:
                cnt = deg[lv]
                starts = np.repeat(rp[lv], cnt)
                within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
                e = starts + within
                residue += np.bincount(dst[e], weights=np.repeat(c, cnt) * w[e], minlength=host.n)
            self.level_info.append((int(F.size), int(deg[F].sum()), x))
            if x > 0.0:
                residue[t.live] = residue[t.live] + x * t.q
                reserve[t.dead] = reserve[t.dead] + x * t.e
            F = np.flatnonzero(~wr.active(old, deg, rmax) & wr.active(residue, deg, rmax) & (residue != old))

    def active(self, rmax):
        return np.flatnonzero(wr.active(self.residue, self.deg, rmax))


def push_sync_seeds(host, w, seeds, sw, alpha, rmax):
    """pprhip_weighted_forward_push_seeds: the first frontier is the set of live seeds (they pop unconditionally); a set
    whose seeds are all dead ends leaves reserve = p and runs no push.  Returns (reserve, residue, levels, pops)."""
    s = SeededPush(host, w, seeds, sw, alpha)
    s.run(s.t.live, rmax)
    return s.reserve, s.residue, s.levels, s.pops


def fora_seeds(host, w, seeds, sw, eps, alpha, seed, rmax=0.0):
    """pprhip_weighted_fora_seeds: push_sync_seeds at rmax (0: rmax0), then weighted_ref.fora's walk phase unchanged
    (whole-graph plan, stream 0, forced first hop, a walk restarts at its own start node at a dead end).  No live seed:
    the estimate is p.  Returns (estimate, walks, walk steps)."""
    rmax0, omega = wr.whole_params(host.n, host.m, alpha, eps)
    s = SeededPush(host, w, seeds, sw, alpha)
    s.run(s.t.live, rmax if rmax else rmax0)
    est, residue = s.reserve.copy(), s.residue
    if s.t.live.size == 0:
        return est, 0, 0
    rsum = float(residue.sum()) * (1 - alpha)
    nrw = int(omega * rsum) if omega * rsum > 0 else 0
    v = np.flatnonzero(residue > 0.0)
    est[v] = est[v] + residue[v] * alpha
    if nrw <= 0 or not rsum > 0.0:
        return est, 0, 0
    r = residue[v] * (1.0 - alpha)
    x = r / rsum * float(nrw)
    omega_i = np.ceil(x).astype(np.int64)
    inc = (x / omega_i) / float(nrw) * rsum
    starts = np.repeat(v, omega_i)
    j = np.arange(int(omega_i.sum()), dtype=np.int64) - np.repeat(np.cumsum(omega_i) - omega_i, omega_i)
    term, steps = wr.walks(host, wr.table(host, w), starts, j.astype(np.uint64), alpha, seed, 0, True)
    est += np.bincount(term, weights=np.repeat(inc, omega_i), minlength=host.n)
    return est, int(starts.size), int(steps.sum())


class TopkSchedule:
    """Fora_Topk's schedule on delta (csrc/run.hpp: TopkSchedule): nothing in it depends on the weights."""

    def __init__(self, eps_half, conf):
        self.eps, self.min_delta, self.m = eps_half, conf.min_delta, float(conf.m)
        self.lg = math.log(2.0 / conf.pfail)

    def rmax(self, delta):
        return self.eps * math.sqrt(delta / 3.0 / self.m / self.lg)

    def omega(self, delta):
        return (self.eps + 2.0) * self.lg / self.eps / self.eps / delta

    def push_rmax(self, rmax):
        return rmax * (math.sqrt(self.m * rmax) * 3.0)

    def last(self, kth, delta):
        return kth >= (1 + self.eps) * delta or delta <= self.min_delta

    def next(self, delta):
        return max(self.min_delta, delta / 4.0)


def select(est, k):
    """(ids, values, kth): the k largest by value descending, ties by id ascending; kth is 0 when fewer than k entries
    are positive."""
    order = np.lexsort((np.arange(est.size), -est))[:k]
    order = order[est[order] > 0.0]
    kth = float(est[order[k - 1]]) if order.size >= k else 0.0
    return order, est[order], kth


def topk(host, w, seeds, sw, eps, conf, seed):
    """pprhip_weighted_fora_topk(_seeds) (a single source: seeds = [s]): plain rounds over the schedule.  Round j: the
    thresholds; the first frontier (round 0: the live seeds; later: every node active at rmax_j, possibly none); the
    levels of SeededPush.run at rmax_j; est := reserve, the unweighted top-k walk plan (rsum = (1 - alpha) sum r, nrw =
    int(omega_j rsum), an entry starts ceil(r nrw) walks, each adding (r nrw / omega_i) / nrw); weighted walks (seed,
    stream j, node, index) without the forced first hop; the selection.  No live seed: the estimate is p, rounds = 0.
    Returns a dict: est, ids, vals, kth, rounds, delta (the last round's), levels, pops, walks, steps, residue, and per
    round frontier (the first frontier's size), walks_round, starts / idx (the round's walks)."""
    alpha, k = conf.alpha, conf.k
    sc = TopkSchedule(eps / 2.0, conf)
    s = SeededPush(host, w, seeds, sw, alpha)
    out = dict(rounds=0, walks=0, steps=0, frontier=[], walks_round=[], round_levels=[], starts=[], idx=[],
               delta=conf.delta, rmax=0.0, omega=0.0)
    if s.t.live.size == 0:
        est = s.reserve.copy()
    else:
        tab = wr.table(host, w)
        delta = conf.delta
        while True:
            rmax_j, omega_j = sc.push_rmax(sc.rmax(delta)), sc.omega(delta)
            F = s.t.live if out["rounds"] == 0 else s.active(rmax_j)
            out["frontier"].append(int(F.size))
            lv0 = s.levels
            s.run(F, rmax_j)
            out["round_levels"].append(s.levels - lv0)
            assert s.active(rmax_j).size == 0
            est = s.reserve.copy()
            rsum = (1.0 - alpha) * float(s.residue.sum())
            nrw = float(int(omega_j * rsum)) if omega_j * rsum > 0 else 0.0
            v = np.flatnonzero(s.residue > 0.0)
            nw = 0
            starts = idx = np.zeros(0, dtype=np.int64)
            if nrw > 0.0 and v.size:
                x = s.residue[v] * nrw
                omega_i = np.ceil(x).astype(np.int64)
                keep = omega_i > 0
                v, x, omega_i = v[keep], x[keep], omega_i[keep]
                inc = (x / omega_i) / nrw
                starts = np.repeat(v, omega_i)
                idx = np.arange(int(omega_i.sum()), dtype=np.int64) - np.repeat(np.cumsum(omega_i) - omega_i, omega_i)
                term, steps = wr.walks(host, tab, starts, idx.astype(np.uint64), alpha, seed, out["rounds"], False)
                est += np.bincount(term, weights=np.repeat(inc, omega_i), minlength=host.n)
                nw = int(starts.size)
                out["steps"] += int(steps.sum())
            out["walks"] += nw
            out["walks_round"].append(nw)
            out["starts"].append(starts)
            out["idx"].append(idx)
            out["rounds"] += 1
            out.update(delta=delta, rmax=rmax_j, omega=omega_j)
            _, _, kth = select(est, k)
            if sc.last(kth, delta):
                break
            delta = sc.next(delta)
    ids, vals, kth = select(est, k)
    out.update(est=est, ids=ids, vals=vals, kth=kth, levels=s.levels, pops=s.pops, residue=s.residue.copy(),
               reserve=s.reserve.copy(), level_sizes=list(s.level_sizes), level_info=list(s.level_info))
    return out
