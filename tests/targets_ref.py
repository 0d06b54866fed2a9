"""Host references of the single-target queries (include/pprhip.h "single targets"), dense numpy: the exact pi(., t) of the
engine's restarting walk, pi(., T) of a weighted target set, the survival vector, and the top-k rule.  Small graphs only
(an n x n inverse)."""
import numpy as np


def transition(host):
    """Row-stochastic P over the out-CSR (parallel edges counted), dead-end rows zero."""
    n = host.n
    P = np.zeros((n, n))
    for u in range(n):
        b, e = int(host.out_rp[u]), int(host.out_rp[u + 1])
        for v in host.out_ci[b:e]:
            P[u, int(v)] += 1.0 / (e - b)
    return P


def leaking_exact(host, alpha):
    """pi'[s, t] of the leaking walk (a dead end's (1 - alpha) mass is lost): alpha (I - (1 - alpha) P)^-1."""
    return alpha * np.linalg.inv(np.eye(host.n) - (1.0 - alpha) * transition(host))


def survival_exact(host, alpha):
    """S(s) = sum_t pi'(s, t)."""
    return leaking_exact(host, alpha).sum(axis=1)


def ppr_exact(host, alpha):
    """pi[s, t] of the restarting walk (the engine's pi): the leaking inverse, rows divided by their sums.  Column t is
    the exact single-target vector pi(., t)."""
    leak = leaking_exact(host, alpha)
    return leak / leak.sum(axis=1, keepdims=True)


def set_exact(pi, ids, weights=None):
    """pi(., T) = sum_t w_t pi(., t) for the set `ids` (duplicates add up), weights None: 1 each, not normalized."""
    ids = np.atleast_1d(np.asarray(ids, dtype=np.int64))
    w = np.ones(ids.size) if weights is None else np.atleast_1d(np.asarray(weights, dtype=np.float64))
    return pi[:, ids] @ w


def topk_rule(v, k):
    """Algo_Util.kth_ppr's selection over the vector v: the positive entries ranked by value descending (ties by id
    ascending); every entry >= the k-th largest is selected, all of them when fewer than k are positive.  Returns
    (count, ids, vals); count may exceed k on ties."""
    v = np.asarray(v, dtype=np.float64)
    pos = np.flatnonzero(v > 0)
    order = pos[np.lexsort((pos, -v[pos]))]
    if k <= 0:
        return 0, order[:0].astype(np.int32), v[order[:0]]
    cnt = order.size if k > order.size else int((v[pos] >= v[order[k - 1]]).sum())
    return cnt, order[:cnt].astype(np.int32), v[order[:cnt]]


def topk_rows(v, k):
    """The row a batched call returns for v: the first min(count, k) selected entries, padded with id -1 / value 0."""
    cnt, ids, vals = topk_rule(v, k)
    row_i = np.full(k, -1, dtype=np.int32)
    row_v = np.zeros(k)
    m = min(cnt, k)
    row_i[:m] = ids[:m]
    row_v[:m] = vals[:m]
    return cnt, row_i, row_v
