"""Host references of the weighted calls (include/pprhip.h "weighted relationships"), numpy, no device: the exact pi
over P(u, v) = w(u -> v) / W(u), the power iteration, the frontier-synchronous weighted push, the weighted walk and the
weighted FORA built from them.  `w` is always aligned with host.out_ci.  Dense solves: small graphs only."""
import math

import numpy as np


def _deg(host):
    return np.diff(host.out_rp.astype(np.int64))


def _src_of_edges(host):
    return np.repeat(np.arange(host.n, dtype=np.int64), _deg(host))


def table(host, w):
    """(cum, W): the prefix rule - cum of a row is the sequential left-to-right fp64 sum in row order, W its last
    element (0 for a dead end)."""
    w = np.asarray(w, dtype=np.float64)
    cum = np.empty(host.m)
    W = np.zeros(host.n)
    rp = host.out_rp.astype(np.int64)
    for u in range(host.n):
        b, e = rp[u], rp[u + 1]
        if e > b:
            cum[b:e] = np.cumsum(w[b:e])
            W[u] = cum[e - 1]
    return cum, W


def transition(host, w):
    """Row-stochastic P over the out-CSR, P[u, v] = sum of w(u -> v) / W(u); dead-end rows zero."""
    w = np.asarray(w, dtype=np.float64)
    _, W = table(host, w)
    src = _src_of_edges(host)
    P = np.zeros((host.n, host.n))
    np.add.at(P, (src, host.out_ci[:host.m].astype(np.int64)), w / W[src])
    return P


def ppr_exact(host, w, alpha):
    """pi[s, t] of the restarting walk over the weighted P (targets_ref.ppr_exact with w / W): the leaking inverse, rows
    divided by their sums."""
    leak = alpha * np.linalg.inv(np.eye(host.n) - (1.0 - alpha) * transition(host, w))
    return leak / leak.sum(axis=1, keepdims=True)


def power_iter(host, w, src, alpha, iters):
    """Power_Method's iteration with the weighted deposit: every node with mass credits alpha r, a dead end returns
    (1 - alpha) r to src, every out-edge receives ((1 - alpha) r / W) * w."""
    w = np.asarray(w, dtype=np.float64)
    _, W = table(host, w)
    deg = _deg(host)
    esrc = _src_of_edges(host)
    dst = host.out_ci[:host.m].astype(np.int64)
    reserve = np.zeros(host.n)
    cur = np.zeros(host.n)
    cur[src] = 1.0
    live = deg > 0
    for _ in range(iters):
        reserve += cur * alpha
        remain = cur * (1.0 - alpha)
        c = np.zeros(host.n)
        c[live] = remain[live] / W[live]
        nxt = np.bincount(dst, weights=c[esrc] * w, minlength=host.n)
        nxt[src] += remain[~live].sum()
        cur = nxt
    return reserve


def active(r, d, rmax):
    """The push test, unchanged by the weights: r / d >= rmax with the relationship count d; a dead end with mass."""
    r = np.asarray(r, dtype=np.float64)
    d = np.asarray(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d > 0, r / np.maximum(d, 1) >= rmax, r > 0.0)


def push_sync(host, w, src, alpha, rmax):
    """The weighted forward push on plain frontier-synchronous Jacobi levels: every node active at level start pops from
    the level-start residues (reserve += alpha r; c = (1 - alpha) r / W; every out-edge deposits c * w; a dead end
    returns (1 - alpha) r to src within the level); a node joins the next level when it crosses the threshold.  The
    source pops unconditionally first; a dead-end source gets reserve 1 and no push (the unweighted conventions).
    Returns (reserve, residue, levels, pops)."""
    w = np.asarray(w, dtype=np.float64)
    _, W = table(host, w)
    deg = _deg(host)
    rp = host.out_rp.astype(np.int64)
    dst = host.out_ci[:host.m].astype(np.int64)
    reserve = np.zeros(host.n)
    residue = np.zeros(host.n)
    if deg[src] == 0:
        reserve[src] = 1.0
        return reserve, residue, 0, 0
    residue[src] = 1.0
    F = np.array([src], dtype=np.int64)
    levels = pops = 0
    while F.size:
        levels += 1
        pops += int(F.size)
        rc = residue[F].copy()
        residue[F] = 0.0
        reserve[F] = reserve[F] + rc * alpha
        dead = deg[F] == 0
        dead_mass = float((rc[dead] * (1.0 - alpha)).sum())
        lv = F[~dead]
        c = ((1.0 - alpha) * rc[~dead]) / W[lv]
        old = residue.copy()
        if lv.size:
            cnt = deg[lv]
            starts = np.repeat(rp[lv], cnt)
            within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            e = starts + within
            residue += np.bincount(dst[e], weights=np.repeat(c, cnt) * w[e], minlength=host.n)
        if dead_mass > 0.0:
            residue[src] += dead_mass
        F = np.flatnonzero(~active(old, deg, rmax) & active(residue, deg, rmax) & (residue != old))
    return reserve, residue, levels, pops


# ---------------------------------------------------------------------------------------------- walks
def walk(orc, host, tab, start, alpha, seed, stream, idx, no_zero_hop):
    """Walk (seed, stream, start, idx): oracle.random_walk's function (same Philox key and counter, word use, stop test,
    forced first hop, dead-end restart, step count) with the weighted neighbour pick: x = (word * 2^-32) * W(cur),
    j = the number of entries of the row's prefix that are <= x, clamped to d - 1.  tab = table(host, w).
    Returns (terminal, steps)."""
    cum, W = tab
    rp = host.out_rp
    if rp[start + 1] == rp[start]:
        return int(start), 0
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    c2 = ((idx >> 32) & 0xFFFF) | (stream << 16)
    cur, k, moves = int(start), 0, 0
    forced = bool(no_zero_hop)
    x4 = None
    while True:
        if (k & 1) == 0:
            x4 = orc.philox([start, idx & 0xFFFFFFFF, c2, k >> 1], key)
        w_stop, w_pick = int(x4[2 * (k & 1)]), int(x4[2 * (k & 1) + 1])
        k += 1
        if not forced and float(w_stop) * (1.0 / 4294967296.0) < alpha:
            break
        forced = False
        b, e = int(rp[cur]), int(rp[cur + 1])
        if e > b:
            x = (float(w_pick) * (1.0 / 4294967296.0)) * W[cur]
            j = min(int(np.searchsorted(cum[b:e], x, side="right")), e - b - 1)
            cur = int(host.out_ci[b + j])
        else:
            cur = int(start)
        moves += 1
    return cur, moves


_M32 = np.uint64(0xFFFFFFFF)


def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters (uint64 arrays holding 32-bit words); returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3))
    k0 = np.uint64(k0)
    k1 = np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & _M32, n2, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def walks(host, tab, starts, idx, alpha, seed, stream=0, no_zero_hop=False):
    """walk() for many walks at once (all of them advance one decision per turn); returns (terminals, steps)."""
    cum, W = tab
    rp = host.out_rp.astype(np.int64)
    ci = host.out_ci[:host.m].astype(np.int64)
    starts = np.asarray(starts, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.uint64)
    nw = starts.size
    cur = starts.copy()
    moves = np.zeros(nw, dtype=np.int64)
    forced = np.full(nw, bool(no_zero_hop))
    act = np.flatnonzero(rp[starts + 1] > rp[starts])
    c0 = starts.astype(np.uint64) & _M32
    c1 = idx & _M32
    c2 = ((idx >> np.uint64(32)) & np.uint64(0xFFFF)) | np.uint64(stream << 16)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    k = 0
    words = None
    while act.size:
        if (k & 1) == 0:
            words = philox_np(c0[act], c1[act], c2[act], np.full(act.size, k >> 1, dtype=np.uint64), k0, k1)
        w_stop = words[2 * (k & 1)].astype(np.float64)
        w_pick = words[2 * (k & 1) + 1].astype(np.float64)
        k += 1
        stop = ~forced[act] & (w_stop * (1.0 / 4294967296.0) < alpha)
        forced[act] = False
        go = ~stop
        a = act[go]
        c = cur[a]
        b, d = rp[c], rp[c + 1] - rp[c]
        x = (w_pick[go] * (1.0 / 4294967296.0)) * W[c]
        lo = np.zeros(a.size, dtype=np.int64)
        hi = d.copy()
        while True:  # lo = entries of the row's prefix that are <= x
            open_ = lo < hi
            if not open_.any():
                break
            mid = (lo + hi) >> 1
            le = np.zeros(a.size, dtype=bool)
            le[open_] = cum[(b + mid)[open_]] <= x[open_]
            lo = np.where(open_ & le, mid + 1, lo)
            hi = np.where(open_ & ~le, mid, hi)
        j = np.minimum(lo, np.maximum(d - 1, 0))
        nxt = np.where(d > 0, ci[np.minimum(b + j, host.m - 1)], starts[a])
        cur[a] = nxt
        moves[a] += 1
        words = tuple(x_[go] for x_ in words)
        act = a
    return cur.astype(np.int32), moves.astype(np.uint32)


# ---------------------------------------------------------------------------------------------- FORA
def whole_params(n, m, alpha, eps):
    """(rmax0, omega) of pprhip_fora_whole_params with delta = pfail = 1 / n."""
    delta = pfail = 1.0 / n
    rmax0 = eps * math.sqrt(delta / 3.0 / m / math.log(2.0 / pfail)) / (1.0 - alpha)
    omega = (eps + 2.0) * math.log(2.0 / pfail) / eps / eps / delta
    return rmax0, omega


def fora(host, w, src, eps, alpha, seed, rmax=0.0):
    """pprhip_weighted_fora: push_sync at rmax (0: rmax0), then the plan rule of the whole-graph FORA - rsum =
    (1 - alpha) * sum r, nrw = int(omega rsum); an entry r credits alpha r to itself and starts omega_i = ceil(x) walks,
    x = (1 - alpha) r / rsum * nrw, each adding (x / omega_i) / nrw * rsum at its terminal - with the weighted walks
    (seed, stream 0, node, j), forced first hop.  Returns (estimate, walks, walk steps)."""
    rmax0, omega = whole_params(host.n, host.m, alpha, eps)
    reserve, residue, _, _ = push_sync(host, w, src, alpha, rmax if rmax else rmax0)
    est = reserve.copy()
    if host.out_rp[src + 1] == host.out_rp[src]:
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
    term, steps = walks(host, table(host, w), starts, j.astype(np.uint64), alpha, seed, 0, True)
    est += np.bincount(term, weights=np.repeat(inc, omega_i), minlength=host.n)
    return est, int(starts.size), int(steps.sum())
