"""The batched apply kernel (csrc/kernels_dense_batch.hip: k_dense_apply_batch) when a workgroup makes several trips.
A trip loads its row sums, its rows' records (BatchState::apply_meta) and its cross bits in one flight, clears the
cross rows' sums behind the loads and stages the rows' pending contributions in a second flight.  On the designed graphs
of tests/batch_sweep_designs.py a workgroup makes one trip (the grid is one workgroup per tile pair), so the test switch
PPRHIP_APPLY_GRID caps the grid of every launch at 1, 2 and 3 workgroups: with one workgroup the 25 tiles of `edges` are
13 trips, the last of them half empty, and every trip but the first follows another.  Every level of every query is a
sweep (dense_frac = 1e-9).  References and tolerances are those of tests/test_gpu_batched_sweep.py: the oracle twin
(TOL_MC for FORA vectors, TOL_PUSH for backward pushes, every per-query counter equal) and, for top-k, the single-query
entry point on the same handle.  A reference is computed once and shared by the grid sizes.

What the cases carry (asserted on the inspected layout in test_designs_carry_the_cases, so a design that loses one fails):
  edges   25 tiles (odd: the last trip's second tile lies beyond the end), tile 4 mixes rows with and without in-edges,
          seven cross rows in tiles that also hold plain rows, swept over ten and more consecutive levels - a sum that
          is not cleared comes back doubled in the next level -, sources among the rows without in-edges
  blocks  n_nz = 1 280 = 20 full tiles; 2 blocks cut at 512, 5 blocks at 256, 512 and 768 (the first sweep of a query
          is an entry sweep over all of them, the later ones run in place)
  small   3 tiles; the source pool[0] is a row without in-edges whose dead-end mass returns to it
and the backward cases of the designs, a top-k call, and PPRHIP_RELABEL=0, where a row's node is not its ordinal."""
import numpy as np
import pytest

import batch_sweep_designs as D
from conftest import shared_graph, to_oracle
from test_gpu_parity import TOL_MC, TOL_PUSH, to_orc_tuning

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]

A, EPS = D.ALPHA, D.EPS
STAT_FIELDS = ("levels", "dense_levels", "rounds", "walks", "walk_steps")
GRIDS = [1, 2, 3, None]
FORWARD = [("edges", 1), ("edges", 2), ("small", 1), ("small", 2), ("blocks", 1), ("blocks", 2), ("blocks", 5)]
_hosts = {}
_refs = {}


def host_of(pkg, name, transposed=False):
    key = (pkg.__name__, name, transposed)
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


def set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("PPRHIP_APPLY_GRID", raising=False)
    else:
        monkeypatch.setenv("PPRHIP_APPLY_GRID", str(grid))


def diff(a, b):
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def same(a, b, what):
    for f in STAT_FIELDS:
        assert getattr(a, f) == getattr(b, f), (what, f, getattr(a, f), getattr(b, f))


def twin_fora(pkg, orc, name, B, s):
    """The twin's FORA vector and counters of one source under the sweep tuning, once per (design, blocks, source)."""
    key = ("fora", name, B, s)
    if key not in _refs:
        og = to_oracle(orc, host_of(pkg, name))
        _refs[key] = og.fora_whole(s, EPS, A, seed=3, n_rounds=1, schedule=orc.SYNC,
                                   tuning=to_orc_tuning(orc, sweep_tuning(pkg, B)))
    return _refs[key]


def forward_against_twin(pkg, orc, dev, name, B, srcs, what):
    out, _, _, _, pq, st = dev.fora_batch_single_source(srcs, EPS, A, seed=3, n_rounds=1, fetch=True, per_query=True)
    assert st.class_launches[5] > 0  # the batched sweep ran
    assert st.class_launches[5] < st.dense_levels  # and served several queries per launch
    worst = 0.0
    for i, s in enumerate(srcs):
        ref, sto = twin_fora(pkg, orc, name, B, s)
        same(pq[i], sto, (what, s))
        worst = max(worst, diff(out[i], ref))
        assert diff(out[i], ref) <= TOL_MC, (what, s, diff(out[i], ref))
    return pq, worst


# ------------------------------------------------------------------ 0. the designs carry what the cases need
def test_designs_carry_the_cases(pkg):
    e, b, s = (D.inspect_forward(pkg, host_of(pkg, k)) for k in ("edges", "blocks", "small"))
    assert e.n_tiles % 2 == 1 and s.n_tiles % 2 == 1 and e.n_tiles >= 7  # three workgroups: trips behind trips, an odd end
    assert D.apply_features(e)["A1_tile_mixes_rows_with_and_without_edges_odd_tile_count"]
    assert D.apply_features(s)["A1_tile_mixes_rows_with_and_without_edges_odd_tile_count"]
    assert e.cross.sum() >= 3 and D.apply_features(e)["A4_tile_with_cross_and_plain_rows"]
    assert b.n_nz % D.TILE == 0 and D.apply_features(b)["A2_rows_fill_their_tiles"]
    assert [j for j, _, _, _ in b.blocks(5)][1:] == [0, 256, 512, 768]
    assert [j for j, _, _, _ in b.blocks(2)] == [0, 512]
    # sources among the rows without in-edges: in `small` pool[0]'s mass reaches dead ends and returns to it
    for side, name in ((e, "edges"), (s, "small")):
        z = set(int(x) for x in side.new2old[side.z_rows])
        assert D.all_designs()[name].names["pool"][0] in z and D.all_designs()[name].sources[0] in z


# ------------------------------------------------------------------ 1. forward sweeps, Jacobi and in blocks
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name,B", FORWARD)
def test_forward_trips(pkg, orc, dev_cache, monkeypatch, name, B, grid):
    dev = dev_of(pkg, dev_cache, name)
    srcs = D.all_designs()[name].sources
    dev.set_tuning(sweep_tuning(pkg, B))
    set_grid(monkeypatch, grid)
    try:
        pq, worst = forward_against_twin(pkg, orc, dev, name, B, srcs, (name, B, grid))
        # many consecutive sweeps: a cross row whose sum was not cleared comes back doubled in the next level
        assert max(x.dense_levels for x in pq) >= (10 if B == 1 else 3)
        if name == "small":  # the first source's dead-end mass came back to its row, which has no in-edges
            assert pq[0].levels >= 3
        print("forward %s, gs_blocks %d, grid %s: largest difference %.3e (twin)" % (name, B, grid, worst))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 2. the backward side
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", range(len(D.backward_cases())))
def test_backward_trips(pkg, orc, dev_cache, monkeypatch, case, grid):
    name, transposed, targets = D.backward_cases()[case]
    host, dev = host_of(pkg, name, transposed), dev_of(pkg, dev_cache, name, transposed)
    din = np.diff(host.in_rp.astype(np.int64))
    dev.set_tuning(sweep_tuning(pkg))
    set_grid(monkeypatch, grid)
    try:
        values, _, st, pq = dev.ppr_targets(targets, A, D.BWD_RMAX)
        assert st.class_launches[5] > 0
        S = dev.walk_survival(A)
        worst = 0.0
        for i, t in enumerate(targets):
            if din[t] == 0:  # the definition: alpha at the target, nothing else
                ref = np.zeros(host.n)
                ref[t] = A
                assert diff(values[i] * S, ref) <= TOL_PUSH and pq[i].levels == 0, (name, transposed, t)
                continue
            key = ("bwd", name, transposed, t)
            if key not in _refs:
                _refs[key] = to_oracle(orc, host).backward_push(t, A, D.BWD_RMAX, orc.SYNC)
            po, _, sto = _refs[key]
            assert pq[i].levels == sto.levels, (name, transposed, t, pq[i].levels, sto.levels)
            worst = max(worst, diff(values[i] * S, po))
            assert diff(values[i] * S, po) <= TOL_PUSH, (name, transposed, t, diff(values[i] * S, po))
        print("backward %s%s, grid %s: largest difference %.3e (twin)" % (name, "^T" if transposed else "", grid, worst))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 3. top-k: armed and flagged rows
@pytest.mark.parametrize("grid", GRIDS)
def test_topk_trips(pkg, dev_cache, monkeypatch, grid):
    dev = dev_of(pkg, dev_cache, "edges")
    srcs = D.all_designs()["edges"].sources
    k = 8
    dev.set_tuning(sweep_tuning(pkg))
    try:
        key = ("topk", pkg.__name__)
        if key not in _refs:  # the single-query entry point runs other kernels: the switch does not reach it
            _refs[key] = [dev.fora_topk(s, EPS, A, k, seed=11 + i, cap=k) for i, s in enumerate(srcs)]
        set_grid(monkeypatch, grid)
        ids, vals, st = dev.fora_batch_topk(srcs, k, EPS, A, seed=11)
        assert st.class_launches[5] > 0
        worst, rounds = 0.0, 0
        for i, s in enumerate(srcs):
            nsel, sids, svals, _, sts = _refs[key][i]
            m = min(nsel, k)
            assert list(ids[i][:m]) == list(sids[:m]), (grid, s)
            assert np.all(ids[i][m:] == -1) and np.all(vals[i][m:] == 0.0), (grid, s)
            worst = max(worst, diff(vals[i][:m], svals[:m]))
            assert diff(vals[i][:m], svals[:m]) <= TOL_MC, (grid, s)
            rounds += sts.rounds
        assert st.rounds == rounds
        print("top-k edges, grid %s: largest difference %.3e (single query)" % (grid, worst))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ 4. original ids: a row's node is not its ordinal
@pytest.mark.parametrize("grid", GRIDS)
def test_no_relabel_trips(pkg, orc, dev_cache, monkeypatch, grid):
    def make():
        monkeypatch.setenv("PPRHIP_RELABEL", "0")
        try:
            return pkg.Graph(host_of(pkg, "edges"))
        finally:
            monkeypatch.delenv("PPRHIP_RELABEL")

    plain = shared_graph(dev_cache, pkg, "edges/original ids", make)
    srcs = D.all_designs()["edges"].sources
    plain.set_tuning(sweep_tuning(pkg))
    set_grid(monkeypatch, grid)
    try:
        pq, worst = forward_against_twin(pkg, orc, plain, "edges", 1, srcs, ("original ids", grid))
        assert max(x.dense_levels for x in pq) >= 10
        print("original ids, grid %s: largest difference %.3e (twin)" % (grid, worst))
    finally:
        plain.set_tuning(pkg.tuning_default())
