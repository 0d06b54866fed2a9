"""The batched weighted sweeps (csrc/kernels_weighted_batch.hip, csrc/kernels_weighted_bwd_batch.hip) on the designed
graphs of tests/weighted_batch_sweep_designs.py: every level of every query is a sweep (dense_frac = 1e-12) unless a
case says otherwise, so the rows placed at group, chunk and tail edges are summed by k_wbat_edges / k_wbb_edges with
their weights in every level.  References: the numpy restatements (weighted_ref.fora, weighted_query_ref.fora_seeds,
weighted_bwd_ref.bpush_sync over the exact survival) and the single calls on the same handle, which run other kernels;
1e-12 throughout, the project's bar for "same arithmetic, other addition order".  Levels and pops are compared too:
tests/test_weighted_batch_sweep_designs.py pins on the CPU that no query here compares a value closer to its threshold
than 1e-9 (relative), and that a wrong reading of any designed position or weight moves a reserve of these very queries
by at least 1e-9.  Every case prints the largest difference it saw."""
import numpy as np
import pytest

import weighted_batch_sweep_designs as WD
import weighted_bwd_ref as br
import weighted_query_ref as wqr
import weighted_ref as wr
from conftest import shared_graph

pytestmark = pytest.mark.gpu

ALPHA, EPS, TOL, SEED = WD.ALPHA, WD.EPS, 1e-12, 3
ALL_DENSE = 1e-12  # dense_frac: every level reaches it
_hosts, _single, _one, _push, _surv = {}, {}, {}, {}, {}


def _laid(pkg, name, tr=False):
    if (name, tr) not in _hosts:
        host = WD.host_of(pkg, name, tr)
        _hosts[(name, tr)] = (host, WD.weights_of(host, name, tr))
    return _hosts[(name, tr)]


def _graph(dev_cache, pkg, name, tr=False, dense_frac=ALL_DENSE):
    host, w = _laid(pkg, name, tr)
    key = name + ("^T" if tr else "")
    fresh = (key, pkg.__name__) not in dev_cache
    g = shared_graph(dev_cache, pkg, key, lambda: pkg.Graph(host, device=0))
    t = pkg.tuning_default()
    t.dense_frac = dense_frac
    g.set_tuning(t)
    if fresh:
        g.set_weights(w)
    return host, w, g


def _frac(host, direction):
    """The mixed tuning of tests/test_gpu_weighted_batch.py and tests/test_gpu_weighted_targets_batch.py: the widest
    node's first level (1 node + d edges) just below the threshold, wider levels above."""
    deg = np.diff((host.out_rp if direction == "fwd" else host.in_rp).astype(np.int64))
    return (int(deg.max()) + 1.5) / host.m


def _decisions(st):  # tests/test_gpu_weighted_batch.py
    return (st.levels, st.dense_levels, st.pops + st.dense_nodes, st.walks, st.walk_steps, st.dead_end_pops, st.rmax_final,
            st.omega, st.rounds)


def _diff(a, b):
    return float(np.max(np.abs(a - b)))


def _push_ref(pkg, name, s):
    """(levels, pops) of weighted_ref.push_sync at the FORA threshold, once per source."""
    if (name, s) not in _push:
        host, w = _laid(pkg, name)
        _push[(name, s)] = wr.push_sync(host, w, s, ALPHA, WD.fora_rmax(host))[2:]
    return _push[(name, s)]


def _single_fora(g, key, s):
    if (key, s) not in _single:
        _single[(key, s)] = g.weighted_fora(s, EPS, ALPHA, SEED)
    return _single[(key, s)]


def _forward_batch(pkg, g, name, mode, srcs, numpy_too):
    """One call of `srcs`: every query against its single call and (numpy_too) against weighted_ref.fora."""
    host, w = _laid(pkg, name)
    out, _, _, _, pq, st = g.weighted_fora_batch(srcs, EPS, ALPHA, SEED, fetch=True, per_query=True)
    assert out.shape == (len(srcs), host.n) and len(pq) == len(srcs)
    assert st.class_launches[5] > 0, "the batched weighted sweep did not run"
    w_single = w_numpy = 0.0
    for i, s in enumerate(srcs):
        est, sst = _single_fora(g, (name, mode), s)
        w_single = max(w_single, _diff(out[i], est))
        assert _diff(out[i], est) <= TOL, (name, mode, i, s, _diff(out[i], est))
        assert _decisions(pq[i]) == _decisions(sst), (name, mode, i, s, _decisions(pq[i]), _decisions(sst))
        levels, pops = _push_ref(pkg, name, s)
        assert pq[i].levels == levels and pq[i].pops + pq[i].dense_nodes == pops, (name, mode, i, s, pq[i].levels, levels)
        if mode == "dense":
            assert pq[i].dense_levels == pq[i].levels, (name, i, s)
        if numpy_too:
            ref, walks, steps = wr.fora(host, w, s, EPS, ALPHA, SEED)
            w_numpy = max(w_numpy, _diff(out[i], ref))
            assert _diff(out[i], ref) <= TOL, (name, mode, i, s, _diff(out[i], ref))
            assert pq[i].walks == walks and pq[i].walk_steps == steps, (name, mode, i, s)
    return out, pq, st, w_single, w_numpy


# ------------------------------------------------------------------ 1. forward against numpy
@pytest.mark.parametrize("name", ["edges", "tail", "small"])
def test_forward_against_numpy(pkg, dev_cache, name):
    _, _, g = _graph(dev_cache, pkg, name)
    srcs = WD.forward_queries()[name]
    _, pq, st, w_single, w_numpy = _forward_batch(pkg, g, name, "dense", srcs, True)
    if name == "edges":
        assert max(x.levels for x in pq) >= 10  # many consecutive sweeps: cleared rows feed the next level
    assert st.class_launches[5] < sum(x.dense_levels for x in pq)  # several queries per sweep
    print("forward %s: %d queries, %d sweeps, longest push %d levels, largest difference %.3e (numpy), %.3e (single call)"
          % (name, len(srcs), st.class_launches[5], max(x.levels for x in pq), w_numpy, w_single))


# ------------------------------------------------------------------ 2. idle, full and reused columns
def _ordered_sources(pkg, q):
    """q sources of `edges`, the longest pushes first, the two shortest (a dead end, an isolated node) last: a column
    is taken over after a long run, while its neighbours are in mid-push."""
    cand = WD.count_sources()
    order = sorted(cand, key=lambda s: -_push_ref(pkg, "edges", s)[0])
    return order[:q - 2] + order[-2:]


@pytest.mark.parametrize("q", [1, 2, 15, 16, 17, 33])
def test_forward_query_counts(pkg, dev_cache, q):
    _, _, g = _graph(dev_cache, pkg, "edges")
    srcs = _ordered_sources(pkg, q) if q > 2 else WD.forward_queries()["edges"][:q]
    out, pq, st, w_single, _ = _forward_batch(pkg, g, "edges", "dense", srcs, False)
    if q == 33:
        assert pq[0].levels >= pq[15].levels >= pq[32].levels == 0
    out2 = g.weighted_fora_batch(srcs, EPS, ALPHA, SEED, fetch=True)[0]
    assert _diff(out, out2) <= TOL, (q, _diff(out, out2))
    print("query count %d: %d sweeps, largest difference %.3e (single call), %.3e (second call)"
          % (q, st.class_launches[5], w_single, _diff(out, out2)))


# ------------------------------------------------------------------ 3. seed sets: the rows outside the sweep
def test_forward_seed_sets(pkg, dev_cache):
    """18 seed sets on `edges`: two of 600 live seeds without in-edges (k_wbat_apply_extra, one workgroup per column,
    takes three trips of 256; k_wbat_leave clears them with three workgroups), 300 of them mixed with dead ends and rows with in-edges, single members, dead ends only.
    The first set of 600 finishes first and its column is taken over by a single member: a row k_wbat_leave left behind
    in either array would be gathered into that query.  The numpy reference is quick enough for every set."""
    host, w, g = _graph(dev_cache, pkg, "edges")
    sets = WD.seed_set_queries()
    ids, sws = [s[0] for s in sets], [s[1] for s in sets]
    out, _, _, _, pq, st = g.weighted_fora_batch_seeds(ids, EPS, ALPHA, SEED, weights=sws, fetch=True, per_query=True)
    assert st.class_launches[5] > 0
    w_single = w_numpy = 0.0
    rmax = WD.fora_rmax(host)
    for i in range(len(sets)):
        est, sst = g.weighted_fora_seeds(ids[i], EPS, ALPHA, SEED, weights=sws[i])
        ref, walks, steps = wqr.fora_seeds(host, w, ids[i], sws[i], EPS, ALPHA, SEED)
        _, _, levels, pops = wqr.push_sync_seeds(host, w, ids[i], sws[i], ALPHA, rmax)
        w_single, w_numpy = max(w_single, _diff(out[i], est)), max(w_numpy, _diff(out[i], ref))
        assert _diff(out[i], est) <= TOL and _diff(out[i], ref) <= TOL, (i, _diff(out[i], est), _diff(out[i], ref))
        assert _decisions(pq[i]) == _decisions(sst), (i, _decisions(pq[i]), _decisions(sst))
        assert pq[i].walks == walks and pq[i].walk_steps == steps, i
        assert pq[i].levels == levels == pq[i].dense_levels and pq[i].pops + pq[i].dense_nodes == pops, (i, pq[i].levels, levels)
    assert pq[0].levels < min(x.levels for x in pq[1:16]) and pq[17].levels == 0
    print("seed sets: levels %s, %d sweeps, largest difference %.3e (numpy), %.3e (single call)"
          % ([x.levels for x in pq], st.class_launches[5], w_numpy, w_single))


# ------------------------------------------------------------------ 4. backward against numpy
def _survival(pkg, name, tr):
    if (name, tr) not in _surv:
        host, w = _laid(pkg, name, tr)
        _surv[(name, tr)] = br.survival_exact(host, w, ALPHA)
    return _surv[(name, tr)]


def _call_of_one(g, key, ids, sw, rmax):
    """The call of one query, which keeps the serial kernels: (vector, Stats), once per module."""
    k = (key, tuple(np.atleast_1d(ids).tolist()), rmax)
    if k not in _one:
        if sw is None:
            v, _, _, pq = g.weighted_ppr_targets([int(ids)], ALPHA, rmax)
        else:
            v, _, _, pq = g.weighted_ppr_target_sets([ids], ALPHA, rmax, weights=[sw])
        assert pq[0].class_launches[5] == 0  # the call of one shares no sweep
        _one[k] = (v[0], pq[0])
    return _one[k]


def _check_backward(pkg, g, name, tr, mode, ids, sw, rmax, value, st):
    """A query of a batched call against bpush_sync over the exact survival and against its call of one; returns the
    two differences."""
    host, w = _laid(pkg, name, tr)
    tag = (name, tr, mode, ids)
    k = (name, tr, tuple(np.atleast_1d(ids).tolist()), rmax)
    if k not in _push:
        _push[k] = br.bpush_sync(host, w, ids, sw, ALPHA, rmax, "pair")
    ref_p, _, levels, pops, _ = _push[k]
    alone, st1 = _call_of_one(g, (name, tr, mode), ids, sw, rmax)
    e_numpy, e_one = _diff(value, ref_p / _survival(pkg, name, tr)), _diff(value, alone)
    assert e_numpy <= TOL and e_one <= TOL, (tag, e_numpy, e_one)
    assert st.levels == levels and st.pops + st.dense_nodes == pops, (tag, st.levels, levels, st.pops, st.dense_nodes, pops)
    assert (st.levels, st.dense_levels, st.pops, st.dense_nodes, st.enqueues) == \
        (st1.levels, st1.dense_levels, st1.pops, st1.dense_nodes, st1.enqueues), tag
    assert st.rounds == 1 and st.rmax_final == rmax
    if mode == "dense":
        assert st.dense_levels == st.levels, tag
    return e_numpy, e_one


def _backward_batches(pkg, g, name, tr, mode, targets, sets, rmax):
    """weighted_ppr_targets over the targets, weighted_ppr_target_sets over the sets with two single targets between them."""
    w_numpy = w_one = 0.0
    values, _, st, pq = g.weighted_ppr_targets(targets, ALPHA, rmax)
    assert len(pq) == len(targets)
    for i, t in enumerate(targets):
        a, b = _check_backward(pkg, g, name, tr, mode, t, None, rmax, values[i], pq[i])
        w_numpy, w_one = max(w_numpy, a), max(w_one, b)
    assert st.levels == sum(x.levels for x in pq)
    assert 0 < st.class_launches[5] <= st.dense_levels  # the shared sweep ran
    sweeps, first_pq = st.class_launches[5], pq
    if sets:
        qs = [([targets[0]], [1.0])] + list(sets) + [([targets[1]], [1.0])]
        values, _, st, pq = g.weighted_ppr_target_sets([q[0] for q in qs], ALPHA, rmax, weights=[q[1] for q in qs])
        for i, (ids, sw) in enumerate(qs):
            one = len(ids) == 1 and sw[0] == 1.0
            a, b = _check_backward(pkg, g, name, tr, mode, ids[0] if one else ids, None if one else sw, rmax, values[i], pq[i])
            w_numpy, w_one = max(w_numpy, a), max(w_one, b)
        assert 0 < st.class_launches[5] <= st.dense_levels
        sweeps += st.class_launches[5]
    return w_numpy, w_one, sweeps, first_pq


@pytest.mark.parametrize("case", range(len(WD.backward_queries())))
def test_backward_against_numpy(pkg, dev_cache, case):
    name, tr, targets, sets, rmax = WD.backward_queries()[case]
    host, _, g = _graph(dev_cache, pkg, name, tr)
    deg = np.diff(host.out_rp.astype(np.int64))
    if sets:  # a set whose members include several nodes without out-edges: they enter by the scatter and must leave
        assert max(int((deg[np.array(ids)] == 0).sum()) for ids, _ in sets) >= 3
    w_numpy, w_one, sweeps, _ = _backward_batches(pkg, g, name, tr, "dense", targets, sets, rmax)
    print("backward %s%s: %d targets, %d sets, %d sweeps, largest difference %.3e (numpy), %.3e (call of one)"
          % (name, "^T" if tr else "", len(targets), len(sets), sweeps, w_numpy, w_one))


# ------------------------------------------------------------------ 5. both directions on one handle
def test_both_directions_on_one_handle(pkg, dev_cache):
    """`edges` has 309 in-rows and 1 525 out-rows: a forward batch, a backward batch, the same forward batch.  The rows
    the other direction summed with atomics in the shared row sums were cleared."""
    _, _, g = _graph(dev_cache, pkg, "edges")
    srcs = WD.forward_queries()["edges"]
    name, tr, targets, sets, rmax = WD.backward_queries()[0]
    assert (name, tr) == ("edges", False)
    first, pq1, _, w1, _ = _forward_batch(pkg, g, "edges", "dense", srcs, False)
    w_numpy, w_one, _, _ = _backward_batches(pkg, g, name, tr, "dense", targets, sets, rmax)
    third, pq3, _, w3, _ = _forward_batch(pkg, g, "edges", "dense", srcs, False)
    assert _diff(first, third) <= TOL, _diff(first, third)
    for a, b in zip(pq1, pq3):
        assert _decisions(a) == _decisions(b)
    again = _backward_batches(pkg, g, name, tr, "dense", targets, sets, rmax)
    print("forward, backward, forward: third against first %.3e; forward %.3e / %.3e (single call), backward %.3e / %.3e (numpy)"
          % (_diff(first, third), w1, w3, w_numpy, again[0]))


# ------------------------------------------------------------------ 6. mixed tuning: columns enter and leave
def test_mixed_tuning_forward(pkg, dev_cache):
    """The first level sparse, the wide ones dense: columns enter by k_wbat_scatter and leave by k_wbat_compact on the
    designed rows."""
    host, _, g = _graph(dev_cache, pkg, "edges", dense_frac=_frac(_laid(pkg, "edges")[0], "fwd"))
    srcs = WD.forward_queries()["edges"]
    _, pq, st, w_single, w_numpy = _forward_batch(pkg, g, "edges", "mixed", srcs, True)
    assert any(0 < x.dense_levels < x.levels for x in pq)
    print("mixed forward: dense / all levels %s, %d sweeps, largest difference %.3e (numpy), %.3e (single call)"
          % ([(x.dense_levels, x.levels) for x in pq], st.class_launches[5], w_numpy, w_single))


def test_mixed_tuning_backward(pkg, dev_cache):
    """The backward case under the same rule, on edges^T: there the designed rows are the out-rows the backward sweep
    walks, and the widest target's first level (pool[0]: 1 node + 269 in-edges) is sparse while its second is dense, so a
    column enters by k_wbb_scatter and leaves by k_wbb_compact.  (On `edges` itself the rule leaves every backward level
    sparse: its widest target, f, has 1 200 in-edges and no level is wider.)"""
    name, tr, targets, sets, rmax = WD.backward_queries()[1]
    assert (name, tr) == ("edges", True)
    _, _, g = _graph(dev_cache, pkg, name, tr, dense_frac=_frac(_laid(pkg, name, tr)[0], "bwd"))
    w_numpy, w_one, sweeps, pq = _backward_batches(pkg, g, name, tr, "mixed", targets, sets, rmax)
    assert any(0 < x.dense_levels < x.levels for x in pq), [(x.dense_levels, x.levels) for x in pq]
    print("mixed backward: dense / all levels %s, %d sweeps, largest difference %.3e (numpy), %.3e (call of one)"
          % ([(x.dense_levels, x.levels) for x in pq], sweeps, w_numpy, w_one))
