"""Host references of the weighted backward direction (include/pprhip.h "weighted relationships", the backward
direction), numpy, no device: the leaking inverse over P(u, v) = w(u -> v) / W(u), the survival vector S_w, the exact
restarting pi, the frontier-synchronous weighted backward push with both start rules, and a pair's value built from a
push, a survival vector and the weighted walks.  `w` is always aligned with host.out_ci.  Dense solves: small graphs."""
import numpy as np

import weighted_ref as wr

PAIR_WALK_STREAM = 0xFFFF


def leaking_exact(host, w, alpha):
    """pi'[s, t] of the leaking walk over the weighted P (a dead end's (1 - alpha) mass is lost)."""
    return alpha * np.linalg.inv(np.eye(host.n) - (1.0 - alpha) * wr.transition(host, w))


def survival_exact(host, w, alpha):
    """S_w(s) = sum_t pi'(s, t); alpha at dead ends."""
    return leaking_exact(host, w, alpha).sum(axis=1)


def ppr_exact(host, w, alpha):
    """pi[s, t] of the restarting walk over the weighted P; column t is the exact single-target vector."""
    return wr.ppr_exact(host, w, alpha)


def merge_set(ids, weights):
    """A target set as the engine parses it: distinct ids ascending, duplicates summed, zero weights dropped."""
    ids = np.atleast_1d(np.asarray(ids, dtype=np.int64))
    ws = np.ones(ids.size) if weights is None else np.atleast_1d(np.asarray(weights, dtype=np.float64))
    u = np.unique(ids)
    acc = np.array([ws[ids == x].sum() for x in u])
    keep = acc != 0.0
    return u[keep], acc[keep]


def bpush_sync(host, w, ids, weights, alpha, rmax, rule, trace=None):
    """The weighted backward push on plain frontier-synchronous Jacobi levels.  Every node of the frontier pops from the
    level-start residues (rc = r[v]; r[v] = 0; p[v] += rc * alpha; c(v) = (1 - alpha) * rc); every in-edge e = (u -> v)
    of a popped v deposits (c(v) * w(e)) / W(u) on r[u]; u joins the next level when !(old > rmax) and new > rmax.
    rule "push": pprhip_weighted_backward_push's start - `ids` is one target; without in-edges reserve(t) = 1 and no
      push, otherwise r(t) = 1 and t pops unconditionally first.
    rule "pair": the start of targets and pairs - one member of weight 1 starts with r(t) = 1 and pops (p(t) = alpha
      and no residue without in-edges); a set starts from r = w (merge_set): a member without in-edges takes alpha * w at
      once, a member with w <= rmax stays residue, the others are the first frontier.
    trace: a list that receives (nodes, in-edges) of every level's frontier.
    Returns (reserve, residue, levels, pops, margin): margin is the smallest |x - rmax| / rmax over every value the run
    compared with rmax (inf when it compared none)."""
    w = np.asarray(w, dtype=np.float64)
    _, W = wr.table(host, w)
    n = host.n
    indeg = np.diff(host.in_rp.astype(np.int64))
    esrc = np.repeat(np.arange(n, dtype=np.int64), np.diff(host.out_rp.astype(np.int64)))
    dst = host.out_ci[:host.m].astype(np.int64)
    reserve = np.zeros(n)
    residue = np.zeros(n)
    margin = np.inf

    def dist(x):
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
        return float(np.min(np.abs(x - rmax) / rmax)) if x.size and rmax > 0 else np.inf

    mid, mw = merge_set(ids, weights)
    if rule == "push":
        assert mid.size == 1 and weights is None
        t = int(mid[0])
        if indeg[t] == 0:
            reserve[t] = 1.0
            return reserve, residue, 0, 0, margin
        residue[t] = 1.0
        F = np.array([t], dtype=np.int64)
    elif rule == "pair":
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
            margin = min(margin, dist(mw[~lone]))
            F = mid[~lone][mw[~lone] > rmax]
    else:
        raise ValueError(rule)
    levels = pops = 0
    while F.size:
        levels += 1
        pops += int(F.size)
        if trace is not None:
            trace.append((int(F.size), int(indeg[F].sum())))
        rc = residue[F].copy()
        residue[F] = 0.0
        reserve[F] = reserve[F] + rc * alpha
        c = np.zeros(n)
        c[F] = (1.0 - alpha) * rc
        inF = np.zeros(n, dtype=bool)
        inF[F] = True
        sel = np.flatnonzero(inF[dst])
        old = residue.copy()
        if sel.size:
            u = esrc[sel]
            residue += np.bincount(u, weights=(c[dst[sel]] * w[sel]) / W[u], minlength=n)
        got = np.flatnonzero(residue != old)
        if got.size:
            margin = min(margin, dist(old[got]), dist(residue[got]))
        F = got[~(old[got] > rmax) & (residue[got] > rmax)]
    return reserve, residue, levels, pops, margin


def pair_value(host, w, reserve, residue, S, s, n_walks, alpha, seed, tab=None):
    """value(s, t) = p_t(s) / S_w(s) + (1 / w) sum_{i < w} r_t(V_i), V_i the terminal of the weighted walk (seed,
    PAIR_WALK_STREAM, s, i) without the forced first hop.  reserve / residue: a "pair"-rule push from t; n_walks = 0 (or
    an all-zero residue, the target without in-edges): the reserve term alone."""
    v = reserve[s] / S[s]
    if n_walks == 0 or not residue.any():
        return float(v)
    tab = tab if tab is not None else wr.table(host, w)
    term, _ = wr.walks(host, tab, np.full(n_walks, s, dtype=np.int64), np.arange(n_walks, dtype=np.uint64), alpha, seed,
                       stream=PAIR_WALK_STREAM, no_zero_hop=False)
    return float(v + residue[term].sum() / float(n_walks))
