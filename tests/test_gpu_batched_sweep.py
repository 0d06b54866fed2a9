"""The batched dense sweep (csrc/kernels_dense_batch.hip) on the designed graphs of tests/batch_sweep_designs.py: every
level of every query is a sweep (dense_frac = 1e-9), so the rows placed at group, chunk, tile and block edges are summed
by the batched edge kernel and applied by the batched apply kernel in every level.  References: the oracle twin
(TOL_MC for FORA vectors, TOL_PUSH for pushes) and the single-query entry points on the same handle (TOL_PUSH), which run
other kernels.  tests/test_batch_sweep_designs.py shows on the CPU that a wrong reading of any designed position moves a
reserve of these very queries by far more than these tolerances.  Every case prints the largest difference it saw."""
import numpy as np
import pytest

import batch_sweep_designs as D
from conftest import shared_graph, to_oracle
from test_gpu_parity import TOL_MC, TOL_PUSH, to_orc_tuning

pytestmark = pytest.mark.gpu

A, EPS = D.ALPHA, D.EPS
STAT_FIELDS = ("levels", "dense_levels", "rounds", "walks", "walk_steps")
_hosts = {}
_singles = {}


def host_of(pkg, name, transposed=False):
    key = (name, transposed)
    if key not in _hosts:
        d = D.all_designs()[name]
        _hosts[key] = d.transposed(pkg) if transposed else d.host(pkg)
    return _hosts[key]


def dev_of(pkg, cache, name, transposed=False):
    return shared_graph(cache, pkg, name + ("^T" if transposed else ""), lambda: pkg.Graph(host_of(pkg, name, transposed)))


def sweep_tuning(pkg, B=1):
    t = pkg.tuning_batch()
    t.dense_frac, t.gs_frac, t.gs_blocks = 1e-9, 1e-9, B
    return t


def single(pkg, dev, name, B, s):
    """fora_single_source of one source under the sweep tuning, computed once per (library, design, blocks, source)."""
    key = (pkg.__name__, name, B, s)
    if key not in _singles:
        _singles[key] = dev.fora_single_source(s, EPS, A, seed=3, n_rounds=1)
    return _singles[key]


def diff(a, b):
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def swept(st, queries):
    assert st.class_launches[5] > 0  # the batched sweep ran
    if queries >= 2:
        assert st.class_launches[5] < st.dense_levels  # and served several queries per launch


def same(a, b, what, fields=STAT_FIELDS):
    for f in fields:
        assert getattr(a, f) == getattr(b, f), (what, f, getattr(a, f), getattr(b, f))


def batch_against_single(pkg, dev, name, B, srcs, what, fields=STAT_FIELDS):
    out, _, _, _, pq, st = dev.fora_batch_single_source(srcs, EPS, A, seed=3, n_rounds=1, fetch=True, per_query=True)
    swept(st, sum(1 for x in pq if x.levels > 0))
    worst = 0.0
    for i, s in enumerate(srcs):
        est, sts = single(pkg, dev, name, B, s)
        same(pq[i], sts, (what, i, s), fields)
        worst = max(worst, diff(out[i], est))
        assert diff(out[i], est) <= TOL_PUSH, (what, i, s, diff(out[i], est))
    return out, pq, worst


# ------------------------------------------------------------------ 1. whole-graph FORA on every design
@pytest.mark.parametrize("name", ["edges", "blocks", "small"])
def test_whole_graph_fora(pkg, orc, dev_cache, name):
    host, dev = host_of(pkg, name), dev_of(pkg, dev_cache, name)
    og = to_oracle(orc, host)
    srcs = D.all_designs()[name].sources
    t = sweep_tuning(pkg)
    dev.set_tuning(t)
    try:
        out, pq, w_single = batch_against_single(pkg, dev, name, 1, srcs, name)
        w_twin = 0.0
        for i, s in enumerate(srcs):
            ref, sto = og.fora_whole(s, EPS, A, seed=3, n_rounds=1, schedule=orc.SYNC, tuning=to_orc_tuning(orc, t))
            same(pq[i], sto, (name, "twin", s))
            w_twin = max(w_twin, diff(out[i], ref))
            assert diff(out[i], ref) <= TOL_MC, (name, s, diff(out[i], ref))
        assert max(x.levels for x in pq) >= 10  # many consecutive sweeps: cleared rows feed the next level
        print("whole-graph FORA %s: %d queries, largest difference %.3e (twin), %.3e (single query)"
              % (name, len(srcs), w_twin, w_single))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 2. idle, full and reused columns
def ordered_sources(pkg, q):
    """q sources of the edges design, the longest pushes first, dead-end and isolated sources last (a column is taken
    over after a long run)."""
    d = D.all_designs()["edges"]
    nm = d.names
    host = host_of(pkg, "edges")
    cand = list(d.sources) + nm["pool"][3:9] + nm["pool"][1190:1196] + nm["T1"][1:4] + nm["H"][130:134] + nm["T0"][1:3]
    cand = cand[:33]
    assert len(cand) == 33 and len(set(cand)) == 33
    if "order" not in _singles:
        rmax = D.fora_rmax(pkg, host)
        levels = {s: D.push_fwd(host, s, A, rmax)[2] for s in cand}
        _singles["order"] = sorted(cand, key=lambda s: -levels[s])
    order = _singles["order"]
    return order[:q - 2] + order[-2:]


@pytest.mark.parametrize("q", [1, 2, 15, 16, 17, 33])
def test_query_counts(pkg, dev_cache, q):
    dev = dev_of(pkg, dev_cache, "edges")
    srcs = ordered_sources(pkg, q) if q > 2 else D.all_designs()["edges"].sources[:q]
    dev.set_tuning(sweep_tuning(pkg))
    try:
        # (a call of more than a few queries walks a (start, index) once for all of them - tests/test_gpu_walk_share.py -
        # so a query's walk_steps count what it walked itself; the walks and the vector are the single query's)
        out, pq, worst = batch_against_single(pkg, dev, "edges", 1, srcs, ("count", q), STAT_FIELDS[:4])
        if q == 33:
            assert pq[0].levels >= pq[15].levels >= pq[32].levels == 0
        out2 = dev.fora_batch_single_source(srcs, EPS, A, seed=3, n_rounds=1, fetch=True)[0]
        assert diff(out, out2) <= TOL_PUSH, (q, diff(out, out2))
        print("query count %d: largest difference %.3e (single query), %.3e (second call)" % (q, worst, diff(out, out2)))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 3. holes in the active columns
def test_mixed_lengths(pkg, dev_cache):
    dev = dev_of(pkg, dev_cache, "blocks")
    nm = D.all_designs()["blocks"].names
    srcs = [nm["z"], nm["pool"][0], nm["trap"], nm["pool"][0], nm["pool"][300], nm["pool"][0], 255, nm["pool"][0]]
    dev.set_tuning(sweep_tuning(pkg))
    try:
        out, pq, worst = batch_against_single(pkg, dev, "blocks", 1, srcs, "mixed")
        levels = [x.levels for x in pq]
        assert min(levels) >= 1 and max(levels) >= 4 * min(levels), levels
        print("mixed lengths, levels %s: largest difference %.3e (single query)" % (levels, worst))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 4. Gauss-Seidel block sweeps
@pytest.mark.parametrize("B", [2, 3, 6, 5])
def test_block_sweeps(pkg, orc, dev_cache, B):
    host, dev = host_of(pkg, "blocks"), dev_of(pkg, dev_cache, "blocks")
    og = to_oracle(orc, host)
    srcs = D.all_designs()["blocks"].sources
    t = sweep_tuning(pkg, B)
    dev.set_tuning(t)
    try:
        out, pq, w_single = batch_against_single(pkg, dev, "blocks", B, srcs, ("blocks", B))
        w_twin = 0.0
        for i, s in enumerate(srcs):
            ref, sto = og.fora_whole(s, EPS, A, seed=3, n_rounds=1, schedule=orc.SYNC, tuning=to_orc_tuning(orc, t))
            same(pq[i], sto, ("blocks", B, "twin", s))
            w_twin = max(w_twin, diff(out[i], ref))
            assert diff(out[i], ref) <= TOL_MC, (B, s, diff(out[i], ref))
        print("block sweeps, gs_blocks %d: largest difference %.3e (twin), %.3e (single query)" % (B, w_twin, w_single))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 5. top-k: armed and flagged rows
@pytest.mark.parametrize("name", ["edges", "small"])
def test_topk(pkg, dev_cache, name):
    dev = dev_of(pkg, dev_cache, name)
    srcs = D.all_designs()[name].sources
    k = 8
    dev.set_tuning(sweep_tuning(pkg))
    try:
        ids, vals, st = dev.fora_batch_topk(srcs, k, EPS, A, seed=11)
        swept(st, len(srcs))
        worst, rounds = 0.0, 0
        for i, s in enumerate(srcs):
            nsel, sids, svals, _, sts = dev.fora_topk(s, EPS, A, k, seed=11 + i, cap=k)
            m = min(nsel, k)
            assert list(ids[i][:m]) == list(sids[:m]), (name, s)
            assert np.all(ids[i][m:] == -1) and np.all(vals[i][m:] == 0.0), (name, s)
            worst = max(worst, diff(vals[i][:m], svals[:m]))
            assert diff(vals[i][:m], svals[:m]) <= TOL_MC, (name, s)
            rounds += sts.rounds
        assert st.rounds == rounds
        print("top-k %s: largest difference %.3e (single query)" % (name, worst))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 6. seed sets: the landing branch
def test_seed_sets(pkg, orc, dev_cache):
    host, dev = host_of(pkg, "edges"), dev_of(pkg, dev_cache, "edges")
    og = to_oracle(orc, host)
    nm = D.all_designs()["edges"].names
    sets = [[nm["dead"], nm["pool"][0]], [nm["extra"][-1], nm["last_row"], nm["hub"]], [nm["last_row"]],
            nm["T0"][:5], [nm["pool"][29], nm["T0"][3], nm["R7"]], [nm["pool"][700], nm["extra"][0], nm["f"]],
            nm["T0"][20:] + [nm["pool"][199]]]
    weights = [None, [1.0, 2.0, 3.0], None, None, [0.5, 0.25, 0.25], None, None]
    t = sweep_tuning(pkg)
    dev.set_tuning(t)
    try:
        out, _, _, _, pq, st = dev.fora_batch_seeds(sets, EPS, A, seed=7, weights=weights, n_rounds=1, fetch=True,
                                                    per_query=True)
        swept(st, len(sets))
        w_twin = w_single = 0.0
        for i, (s, w) in enumerate(zip(sets, weights)):
            est, sts = dev.fora_seeds(s, EPS, A, seed=7, weights=w, n_rounds=1)
            same(pq[i], sts, ("seeds", i))
            w_single = max(w_single, diff(out[i], est))
            assert diff(out[i], est) <= TOL_PUSH, ("seeds", i, diff(out[i], est))
            ref, sto = og.fora_whole_seeds(s, EPS, A, seed=7, weights=w, n_rounds=1, tuning=to_orc_tuning(orc, t))
            same(pq[i], sto, ("seeds twin", i))
            w_twin = max(w_twin, diff(out[i], ref))
            assert diff(out[i], ref) <= TOL_MC, ("seeds twin", i, diff(out[i], ref))
        print("seed sets: largest difference %.3e (twin), %.3e (single query)" % (w_twin, w_single))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 7. the backward side, then forward again
@pytest.mark.parametrize("case", range(len(D.backward_cases())))
def test_backward(pkg, orc, dev_cache, case):
    name, transposed, targets = D.backward_cases()[case]
    host, dev = host_of(pkg, name, transposed), dev_of(pkg, dev_cache, name, transposed)
    og = to_oracle(orc, host)
    din = np.diff(host.in_rp.astype(np.int64))
    dev.set_tuning(sweep_tuning(pkg))
    try:
        values, _, st, pq = dev.ppr_targets(targets, A, D.BWD_RMAX)
        swept(st, sum(1 for t in targets if din[t] > 0))
        S = dev.walk_survival(A)
        w_twin = w_single = 0.0
        for i, t in enumerate(targets):
            if din[t] == 0:  # the definition: alpha at the target, nothing else
                ref = np.zeros(host.n)
                ref[t] = A
                assert diff(values[i] * S, ref) <= TOL_PUSH and pq[i].levels == 0, (name, transposed, t)
                continue
            p, _, _ = dev.backward_push(t, A, D.BWD_RMAX)
            po, _, sto = og.backward_push(t, A, D.BWD_RMAX, orc.SYNC)
            assert pq[i].levels == sto.levels, (name, transposed, t, pq[i].levels, sto.levels)
            w_single, w_twin = max(w_single, diff(values[i] * S, p)), max(w_twin, diff(values[i] * S, po))
            assert diff(values[i] * S, p) <= TOL_PUSH, (name, transposed, t, diff(values[i] * S, p))
            assert diff(values[i] * S, po) <= TOL_PUSH and diff(p, po) <= TOL_PUSH, (name, transposed, t)
        # the direction changes: the forward sweep finds the row sums of the backward one cleared
        srcs = [t for t in targets if host.out_rp[t + 1] > host.out_rp[t]][:4]
        out, _, _, _, pq2, st2 = dev.fora_batch_single_source(srcs, EPS, A, seed=3, n_rounds=1, fetch=True, per_query=True)
        swept(st2, len(srcs))
        w_fwd = 0.0
        for i, s in enumerate(srcs):
            est, sts = dev.fora_single_source(s, EPS, A, seed=3, n_rounds=1)
            same(pq2[i], sts, (name, transposed, "forward after", s))
            w_fwd = max(w_fwd, diff(out[i], est))
            assert diff(out[i], est) <= TOL_PUSH, (name, transposed, s, diff(out[i], est))
        print("backward %s%s: largest difference %.3e (twin), %.3e (backward_push); forward after it %.3e (single query)"
              % (name, "^T" if transposed else "", w_twin, w_single, w_fwd))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 8. without the LDS table
def test_no_table(pkg, dev_cache, monkeypatch):
    """PPRHIP_RELABEL=0 keeps the original ids: no hot table, the HOT = false edge kernel.  Blocks follow the internal
    order, so gs_blocks = 1."""
    host = host_of(pkg, "edges")
    dev = dev_of(pkg, dev_cache, "edges")
    srcs = D.all_designs()["edges"].sources
    monkeypatch.setenv("PPRHIP_RELABEL", "0")
    plain = pkg.Graph(host)
    monkeypatch.delenv("PPRHIP_RELABEL")
    t = sweep_tuning(pkg)
    try:
        dev.set_tuning(t)
        plain.set_tuning(t)
        out0, _, _, _, pq0, st0 = dev.fora_batch_single_source(srcs, EPS, A, seed=3, n_rounds=1, fetch=True, per_query=True)
        out1, _, _, _, pq1, st1 = plain.fora_batch_single_source(srcs, EPS, A, seed=3, n_rounds=1, fetch=True,
                                                                 per_query=True)
        swept(st0, len(srcs))
        swept(st1, len(srcs))
        for i, s in enumerate(srcs):
            same(pq0[i], pq1[i], ("no table", s))
        assert diff(out0, out1) <= TOL_PUSH, diff(out0, out1)
        print("no table: largest difference %.3e (handle with the table)" % diff(out0, out1))
    finally:
        plain.close()
        dev.set_tuning(pkg.tuning_default())
