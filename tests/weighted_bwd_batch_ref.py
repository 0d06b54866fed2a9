"""Host model of the batched weighted target call's driver (csrc/weighted_bwd_batch.cpp), numpy, no device: which
levels of a query are dense, and how many shared sweeps the lockstep rounds run for a call's queries on n_cols columns.
Built on the level reference of tests/weighted_bwd_ref.py."""
import math

import weighted_bwd_ref as br

MARGIN = 1e-9  # levels are compared only where the reference compared no value closer to rmax than this (relative)

_RUNS = {}


def push_ref(key, host, w, ids, weights, alpha, rmax):
    """bpush_sync(..., "pair") with its trace, computed once per `key` and left unchanged:
    (reserve, levels, pops, margin, trace)."""
    k = (key, alpha, rmax)
    if k not in _RUNS:
        trace = []
        p, _, levels, pops, margin = br.bpush_sync(host, w, ids, weights, alpha, rmax, "pair", trace=trace)
        p.setflags(write=False)
        _RUNS[k] = (p, levels, pops, margin, tuple(trace))
    return _RUNS[k]


def dense_threshold(host, dense_frac):
    """ceil(dense_frac * m): a level of nf nodes and ef in-edges is dense when nf + ef reaches it."""
    return int(math.ceil(dense_frac * float(host.m)))


def kinds_of(trace, host, dense_frac):
    thresh = dense_threshold(host, dense_frac)
    return [nf + ef >= thresh for nf, ef in trace]


def level_kinds(host, w, target, alpha, rmax, dense_frac, weights=None):
    """One bool per level of the push from `target` (one id, or a set with `weights`): True where the level is dense."""
    trace = []
    br.bpush_sync(host, w, target, weights, alpha, rmax, "pair", trace=trace)
    return kinds_of(trace, host, dense_frac)


def lockstep(kinds, n_cols):
    """The driver's rounds for the queries whose level kinds are kinds[i], in call order, on n_cols columns.  A round:
    in column order a column whose query has no level left finishes it and takes the call's next query (one without
    levels finishes at once); then, if any busy column's next level is sparse, every such column runs one level and the
    columns at a dense level wait; otherwise one sweep runs a level of every busy column.
    Returns (sweeps, rounds, busy columns summed over the sweeps)."""
    cols = [None] * n_cols  # [query, next level]
    nxt = sweeps = rounds = busy_sum = 0
    while True:
        for c in range(n_cols):
            while True:
                if cols[c] is not None and cols[c][1] == len(kinds[cols[c][0]]):
                    cols[c] = None
                if cols[c] is not None or nxt >= len(kinds):
                    break
                cols[c] = [nxt, 0]
                nxt += 1
        busy = [c for c in range(n_cols) if cols[c] is not None]
        if not busy:
            return sweeps, rounds, busy_sum
        rounds += 1
        sparse = [c for c in busy if not kinds[cols[c][0]][cols[c][1]]]
        if not sparse:
            sweeps += 1
            busy_sum += len(busy)
        for c in (sparse or busy):
            cols[c][1] += 1


def lockstep_sweeps(kinds, n_cols):
    return lockstep(kinds, n_cols)[0]


def eager_sweeps(kinds, n_cols):
    """The rule of the forward driver (csrc/weighted_batch.cpp), for comparison: every busy column runs a level in every
    round, the dense ones on one sweep."""
    cols = [None] * n_cols
    nxt = sweeps = 0
    while True:
        for c in range(n_cols):
            while True:
                if cols[c] is not None and cols[c][1] == len(kinds[cols[c][0]]):
                    cols[c] = None
                if cols[c] is not None or nxt >= len(kinds):
                    break
                cols[c] = [nxt, 0]
                nxt += 1
        busy = [c for c in range(n_cols) if cols[c] is not None]
        if not busy:
            return sweeps
        sweeps += 1 if any(kinds[cols[c][0]][cols[c][1]] for c in busy) else 0
        for c in busy:
            cols[c][1] += 1

