"""Numpy restatement of the sweep cut by relationship weight (include/pprhip.h "weighted local clustering"; DESIGN.md 2
"Weighted sweep cut"), in a form different from the kernel's: the kernel walks every ranked node's adjacency and adds
+q / -q per slot; here every relationship is looked at once and marks the two positions between which it cuts, as
tests/sweep_ref.py does.  All sums are over quanta, in Python ints or uint64; the quantum rule is written out below.
Shared by test_weighted_sweep_ref.py, test_gpu_weighted_sweep.py and test_gpu_weighted_sweep_designs.py."""
import math

import numpy as np

from sweep_ref import NONE

LIMIT_MAX = (1 << 63) - 1


def shift_of(weights):
    """s = 61 - e - L: e the exponent of frexp(wmax), L the smallest integer with m <= 2^L (no weights: 0)."""
    w = np.asarray(weights, dtype=np.float64).ravel()
    m = int(w.size)
    if m == 0:
        return 0
    _, e = math.frexp(float(w.max()))
    L = 0
    while (1 << L) < m:
        L += 1
    return 61 - e - L


def quanta(weights, shift=None):
    """q(e) = max(1, rint(ldexp(w(e), s))): to nearest, ties to even; below half a quantum: one quantum.  uint64."""
    w = np.asarray(weights, dtype=np.float64).ravel()
    s = shift_of(w) if shift is None else int(shift)
    with np.errstate(under="ignore"):
        scaled = np.rint(np.ldexp(w, s))
    assert np.all(scaled < 2.0 ** 62)
    return np.maximum(scaled.astype(np.int64), 1).astype(np.uint64)


def qdegrees(n, src, dst, q):
    """qdeg by node id (uint64; the total is at most 2^62): out-row plus in-row, a self loop twice."""
    deg = np.zeros(n, dtype=np.uint64)
    np.add.at(deg, np.asarray(src, dtype=np.int64), np.asarray(q, dtype=np.uint64))
    np.add.at(deg, np.asarray(dst, dtype=np.int64), np.asarray(q, dtype=np.uint64))
    return deg


def cut_of(n, src, dst, q, members):
    """Brute force: the quanta of the relationships (a -> b), a != b, with exactly one endpoint in `members`."""
    inside = set(int(v) for v in np.asarray(members).tolist())
    return sum(int(c) for a, b, c in zip(np.asarray(src).tolist(), np.asarray(dst).tolist(), np.asarray(q).tolist())
               if a != b and ((a in inside) != (b in inside)))


def vol_limit(max_vol, shift):
    """max_vol (weight units) in quanta: min(2^63 - 1, floor(ldexp(max_vol, s)))."""
    with np.errstate(over="ignore", under="ignore"):
        t = float(np.ldexp(np.float64(max_vol), shift))
    return LIMIT_MAX if t >= 2.0 ** 63 else int(math.floor(t))


def weighted_sweep_ref(n, src, dst, weights, x, normalize=1, max_size=0, max_vol=0.0):
    """Returns dict(order, vol_q, cut_q, support, profiled, best_size, best_cut_q, best_vol_q, best_conductance,
    total_vol_q, shift, edge_slots); order / vol_q / cut_q hold `profiled` entries (int32 / uint64 / uint64)."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    shift = shift_of(weights)
    q = quanta(weights, shift)
    qdeg = qdegrees(n, src, dst, q)
    slots = np.bincount(src, minlength=n) + np.bincount(dst, minlength=n)
    total = 2 * sum(q.tolist())
    assert total <= 1 << 62
    qdeg_u = qdeg
    assert sum(qdeg.tolist()) == total
    ids = np.nonzero((x > 0) & (slots > 0))[0]
    assert np.all(qdeg_u[ids] >= 1)
    score = x[ids] / qdeg_u[ids].astype(np.float64) if normalize else x[ids]   # uint64 -> fp64: to nearest
    order = ids[np.lexsort((ids, -score))]
    support = int(order.size)
    profiled = min(support, int(max_size)) if max_size > 0 else support
    order = order[:profiled]
    rank = np.full(n, NONE, dtype=np.int64)
    rank[order] = np.arange(profiled, dtype=np.int64)
    vol = np.cumsum(qdeg_u[order], dtype=np.uint64)
    # every relationship once: +q at the position that takes its first endpoint, -q where the second one is taken
    # (int64 holds every partial sum: the quanta of all relationships together are at most 2^61)
    keep = src != dst
    ra, rb, qs = rank[src[keep]], rank[dst[keep]], q[keep].astype(np.int64)
    lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
    delta = np.zeros(profiled, dtype=np.int64)
    np.add.at(delta, lo[lo != NONE], qs[lo != NONE])
    np.subtract.at(delta, hi[hi != NONE], qs[hi != NONE])
    cut = np.cumsum(delta)
    assert np.all(cut >= 0)
    cut = cut.astype(np.uint64)
    out = dict(order=order.astype(np.int32), vol_q=vol, cut_q=cut, support=support, profiled=profiled, best_size=0,
               best_cut_q=0, best_vol_q=0, best_conductance=float("inf"), total_vol_q=total, shift=shift,
               edge_slots=int(slots[order].sum()))
    if profiled:
        tot = np.uint64(total)
        den = np.minimum(vol, tot - vol)
        cand = den > 0
        if max_vol > 0:
            cand &= vol <= np.uint64(vol_limit(max_vol, shift))
        phi = np.full(profiled, np.inf)
        phi[cand] = cut[cand].astype(np.float64) / den[cand].astype(np.float64)
        if cand.any():
            b = int(np.argmin(phi))  # the first of the smallest: ties go to the shortest prefix
            out.update(best_size=b + 1, best_cut_q=int(cut[b]), best_vol_q=int(vol[b]), best_conductance=float(phi[b]))
    return out
