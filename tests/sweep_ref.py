"""Numpy restatement of the sweep cut (include/pprhip.h "local clustering"; DESIGN.md 2 "Sweep cut"), in a form different
from the kernel's: the kernel walks every ranked node's adjacency and adds +1 / -1 per slot; here every relationship is
looked at once and marks the two positions between which it cuts.  Shared by test_sweep_ref.py and test_gpu_sweep.py."""
import numpy as np

NONE = np.iinfo(np.int64).max  # rank of a node that is not profiled: greater than every position


def edges_of(host):
    """(src, dst) of a HostCsr's relationships, from its out-CSR."""
    src = np.repeat(np.arange(host.n, dtype=np.int64), np.diff(host.out_rp.astype(np.int64)))
    return src, host.out_ci[:host.m].astype(np.int64)


def degrees(n, src, dst):
    return np.bincount(src, minlength=n).astype(np.int64) + np.bincount(dst, minlength=n).astype(np.int64)


def cut_of(n, src, dst, members):
    """Brute force: relationships (a -> b), a != b, with exactly one endpoint in `members`."""
    inside = np.zeros(n, dtype=bool)
    inside[np.asarray(members, dtype=np.int64)] = True
    return int(np.count_nonzero((src != dst) & (inside[src] != inside[dst])))


def sweep_ref(n, src, dst, x, normalize=1, max_size=0, max_vol=0):
    """Returns dict(order, vol, cut, support, profiled, best_size, best_cut, best_vol, best_conductance, total_vol,
    edge_slots); order / vol / cut hold `profiled` entries (int32 / uint64 / uint64)."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    deg = degrees(n, src, dst)
    ids = np.nonzero((x > 0) & (deg > 0))[0]
    score = x[ids] / deg[ids].astype(np.float64) if normalize else x[ids]
    order = ids[np.lexsort((ids, -score))]
    support = int(order.size)
    profiled = min(support, int(max_size)) if max_size > 0 else support
    order = order[:profiled]
    rank = np.full(n, NONE, dtype=np.int64)
    rank[order] = np.arange(profiled, dtype=np.int64)
    vol = np.cumsum(deg[order]).astype(np.uint64)
    keep = src != dst
    ra, rb = rank[src[keep]], rank[dst[keep]]
    lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
    delta = np.zeros(profiled, dtype=np.int64)
    np.add.at(delta, lo[lo != NONE], 1)    # the relationship starts to cut at the prefix that takes its first endpoint
    np.add.at(delta, hi[hi != NONE], -1)   # ... and stops at the one that takes the second, where that is ranked
    cut = np.cumsum(delta).astype(np.uint64)
    total = 2 * int(src.size)
    out = dict(order=order.astype(np.int32), vol=vol, cut=cut, support=support, profiled=profiled, best_size=0, best_cut=0,
               best_vol=0, best_conductance=float("inf"), total_vol=total, edge_slots=int(vol[-1]) if profiled else 0)
    if profiled:
        v = vol.astype(np.int64)
        den = np.minimum(v, total - v)
        cand = den > 0
        if max_vol > 0:
            cand &= v <= int(max_vol)
        phi = np.full(profiled, np.inf)
        phi[cand] = cut[cand].astype(np.float64) / den[cand].astype(np.float64)
        if cand.any():
            b = int(np.argmin(phi))  # the first of the smallest: ties go to the shortest prefix
            out.update(best_size=b + 1, best_cut=int(cut[b]), best_vol=int(vol[b]), best_conductance=float(phi[b]))
    return out
