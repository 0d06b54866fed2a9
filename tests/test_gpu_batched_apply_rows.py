"""The rows the batched apply kernel treats by class (csrc/kernels_dense_batch.hip: k_dense_apply_batch and its
launcher; engine.hpp: ApplyTileClass).  Dead-end tiles - rows with in-edges and out-degree 0 - are neither staged nor
stored and their residues count as zero without a load; the tiles of rows without in-edges are visited only where a
column's source lies, and in the two sweeps after.  What could go wrong is state that a skipped tile would have
rewritten: a stale entry of the contribution arrays shows as mass != 1, a stale prep_bits word as a counter, a cross
row's sum that was not cleared comes back doubled.

The graph is tests/apply_rows_designs.py's (tests/test_apply_rows_designs.py asserts on the CPU that it carries the
cases); tests/batch_sweep_designs.py's `small` and `edges`, whose sources lie among rows without in-edges too, run as
well.  Tuning, references and tolerances are those of tests/test_gpu_batched_apply_trips.py: dense_frac = gs_frac = 1e-9
(every level a sweep), the oracle twin at TOL_MC / TOL_PUSH with every per-query counter equal, top-k against the
single-query entry point; PPRHIP_APPLY_GRID 1, 2, 3 and unset.  A reference is computed once per (design, blocks,
source).  Every case runs three ways: as it is (test_case); with PPRHIP_APPLY_COUNT_RES=1, which loads the residues the
kernel otherwise takes for zero and counts the non-zero ones into class 7 of the call's statistics - 0 everywhere, of
a number of loads that is not 0 wherever the graph has dead-end tiles, so the counting ran
(test_no_residue_on_dead_ends; the same class carries the dead-end tiles that an entry sweep came by); and with
PPRHIP_APPLY_ALL_ROWS=1, every tile and every load, against the run without it (test_lean_equals_all_rows: the vectors
to TOL_PUSH - two runs of one build differ in the last bits of the walks' atomic sums - and every counter equal).

The contribution arrays are shared with backward calls, whose entry preparation leaves an entry on a target without
out-edges - a row of a dead-end tile; the forward sweeps behind a backward one store those tiles as plain ones
(case_stale_entry_of_a_backward_call)."""
import numpy as np
import pytest

import apply_rows_designs as R
import batch_sweep_designs as D
from conftest import to_oracle
from test_gpu_parity import TOL_MC, TOL_PUSH, to_orc_tuning

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]

A, EPS = D.ALPHA, D.EPS
STAT_FIELDS = ("levels", "dense_levels", "rounds", "walks", "walk_steps", "pops", "edge_pushes", "dead_end_pops")
GRIDS = [1, 2, 3, None]
_hosts, _refs, _sides = {}, {}, {}


def designs():
    d = dict(D.all_designs())
    d["rows"] = R.design()
    return d


def host_of(pkg, name, transposed=False):
    key = (pkg.__name__, name, transposed)
    if key not in _hosts:
        d = designs()[name]
        _hosts[key] = d.transposed(pkg) if transposed else d.host(pkg)
    return _hosts[key]


def sources(pkg, which):
    if "rows" not in _sides:
        _sides["rows"] = D.inspect_forward(pkg, host_of(pkg, "rows"))
    return R.source_sets(_sides["rows"])[which]


def sweep_tuning(pkg, B=1):
    t = pkg.tuning_batch()
    t.dense_frac, t.gs_frac, t.gs_blocks = 1e-9, 1e-9, B
    return t


def diff(a, b):
    return float(np.max(np.abs(a - b))) if a.size else 0.0


class Run:
    """One pass over a case: the handles it makes, what it returned (for the run-against-run comparison) and the
    residue counter of its calls."""

    def __init__(self, pkg, orc, monkeypatch):
        self.pkg, self.orc, self.mp = pkg, orc, monkeypatch
        self.vectors, self.counters, self.res_count, self.handles = [], [], 0, []
        self.res_loads, self.entry_tiles = 0, 0  # (with the counting switch: residues loaded, tiles of entry sweeps)

    def graph(self, name, transposed=False, relabel=True):
        if not relabel:
            self.mp.setenv("PPRHIP_RELABEL", "0")
        try:
            g = self.pkg.Graph(host_of(self.pkg, name, transposed))
        finally:
            if not relabel:
                self.mp.delenv("PPRHIP_RELABEL")
        self.handles.append(g)
        return g

    def close(self):
        for g in self.handles:
            g.close()

    def twin(self, name, B, s):
        key = ("fora", name, B, s)
        if key not in _refs:
            og = to_oracle(self.orc, host_of(self.pkg, name))
            _refs[key] = og.fora_whole(s, EPS, A, seed=3, n_rounds=1, schedule=self.orc.SYNC,
                                       tuning=to_orc_tuning(self.orc, sweep_tuning(self.pkg, B)))
        return _refs[key]

    def count(self, st):
        self.res_count += int(st.class_bytes[7])
        self.res_loads += int(st.class_launches[7])
        self.entry_tiles += int(st.class_ms[7])

    def keep(self, out, pq, st):
        self.vectors.append(np.array(out))
        self.counters += [tuple(getattr(x, f) for f in STAT_FIELDS) for x in pq]
        self.count(st)

    def forward(self, dev, name, B, srcs, what):
        """A batched whole-graph call against the twin, query by query."""
        dev.set_tuning(sweep_tuning(self.pkg, B))
        out, _, _, _, pq, st = dev.fora_batch_single_source(srcs, EPS, A, seed=3, n_rounds=1, fetch=True, per_query=True)
        assert st.class_launches[5] > 0, what  # the batched sweep ran
        for i, s in enumerate(srcs):
            ref, sto = self.twin(name, B, s)
            for f in ("levels", "dense_levels", "rounds", "walks", "walk_steps"):
                assert getattr(pq[i], f) == getattr(sto, f), (what, i, s, f, getattr(pq[i], f), getattr(sto, f))
            assert abs(float(out[i].sum()) - 1.0) <= TOL_MC, (what, i, s, float(out[i].sum()))
            assert diff(out[i], ref) <= TOL_MC, (what, i, s, diff(out[i], ref))
        self.keep(out, pq, st)
        return out, pq


# ------------------------------------------------------------------ the cases
def case_columns_reused(r):
    """48 queries over 16 columns: sources without in-edges from tile to tile whose mass comes back from the dead ends,
    ring rows, dead ends and rows of the boundary tile in between, so that a column changes hands while the tile of the
    source that left is still in the window, and after."""
    g = r.graph("rows")
    srcs = sources(r.pkg, "reuse")
    assert len(srcs) >= 40
    # (a call of 32 queries and more serves walks from the call's terminal cache, which the twin does not have: with
    # every walk walked, walk_steps is the twin's too)
    r.mp.setenv("PPRHIP_WALK_SHARE", "0")
    _, pq = r.forward(g, "rows", 1, srcs, "columns reused")
    assert max(x.dense_levels for x in pq) >= 30 and min(x.dense_levels for x in pq) == 0  # long and empty pushes


def case_two_calls(r):
    """The second call on a handle, with other sources, against the same call on a fresh handle."""
    g, fresh = r.graph("rows"), r.graph("rows")
    r.forward(g, "rows", 1, sources(r.pkg, "sixteen"), "first call")
    second, _ = r.forward(g, "rows", 1, sources(r.pkg, "second_call"), "second call")
    alone, _ = r.forward(fresh, "rows", 1, sources(r.pkg, "second_call"), "second call, fresh handle")
    assert diff(second, alone) <= TOL_PUSH, diff(second, alone)


def case_source_positions(r):
    """Sources in the boundary tile, the first and the last tile without in-edges (27 tiles: the last pair is half
    empty), two in one tile; then sixteen sources in sixteen tiles."""
    g = r.graph("rows")
    r.forward(g, "rows", 1, sources(r.pkg, "positions"), "source positions")
    r.forward(g, "rows", 1, sources(r.pkg, "sixteen"), "sixteen tiles")


def case_dead_end_tiles(B):
    def run(r):
        """Four dead-end tiles and two mixed ones; cross rows among them, cleared over 30 and more levels; with B > 1 an
        entry sweep and in-place sweeps over them, a block boundary at ordinal 512 inside the dead-end range."""
        g = r.graph("rows")
        _, pq = r.forward(g, "rows", B, sources(r.pkg, "dead_ends"), ("dead-end tiles", B))
        assert max(x.dense_levels for x in pq) >= 10, [x.dense_levels for x in pq]
    return run


def case_designs_of_the_sweep(r):
    """tests/batch_sweep_designs.py: `small` (a source without in-edges takes its dead-end mass back) and `edges`."""
    for name in ("small", "edges"):
        r.forward(r.graph(name), name, 1, designs()[name].sources, name)


def case_seeded_call(r):
    """A seeded call directly after a single-source call on one handle: seeds land on rows without in-edges that no
    source's tile covers, so the sweeps with a seeded column and the two behind them run over every tile; then single
    sources again."""
    g = r.graph("rows")
    r.forward(g, "rows", 1, sources(r.pkg, "sixteen"), "before the seeds")
    d = R.design().names
    sets = [[d["pool"][100 + 70 * i], d["pool"][900 - 50 * i], d["ring"][i], d["dead"][40 + i]] for i in range(6)]
    g.set_tuning(sweep_tuning(r.pkg))
    out, _, _, _, pq, st = g.fora_batch_seeds(sets, EPS, A, seed=3, n_rounds=1, fetch=True, per_query=True)
    assert st.class_launches[5] > 0
    og = to_oracle(r.orc, host_of(r.pkg, "rows"))
    for i, s in enumerate(sets):
        key = ("seeds", i)
        if key not in _refs:
            _refs[key] = og.fora_whole_seeds(s, EPS, A, seed=3, n_rounds=1,
                                             tuning=to_orc_tuning(r.orc, sweep_tuning(r.pkg)))
        ref, sto = _refs[key][0], _refs[key][1]
        assert pq[i].levels == sto.levels and pq[i].walks == sto.walks, (i, pq[i].levels, sto.levels)
        assert diff(out[i], ref) <= TOL_MC, (i, diff(out[i], ref))
    r.keep(out, pq, st)
    r.forward(g, "rows", 1, sources(r.pkg, "second_call"), "behind the seeds")


def case_backward_call(r):
    """A batched backward call between two forward calls on one handle (another layout of the shared arrays)."""
    host, g = host_of(r.pkg, "rows"), r.graph("rows")
    r.forward(g, "rows", 1, sources(r.pkg, "positions"), "before the backward call")
    d = R.design().names
    targets = [d["dead"][250], d["ring"][5], d["dead"][0]]
    g.set_tuning(sweep_tuning(r.pkg))
    values, _, st, pq = g.ppr_targets(targets, A, D.BWD_RMAX)
    assert st.class_launches[5] > 0
    S = g.walk_survival(A)
    for i, t in enumerate(targets):
        key = ("bwd", t)
        if key not in _refs:
            _refs[key] = to_oracle(r.orc, host).backward_push(t, A, D.BWD_RMAX, r.orc.SYNC)
        po, _, sto = _refs[key]
        assert pq[i].levels == sto.levels, (t, pq[i].levels, sto.levels)
        assert diff(values[i] * S, po) <= TOL_PUSH, (t, diff(values[i] * S, po))
    r.vectors.append(np.array(values))
    r.count(st)
    r.forward(g, "rows", 1, sources(r.pkg, "sixteen"), "behind the backward call")


def case_stale_entry_of_a_backward_call(r):
    """A backward call whose target is a dead end and whose threshold no in-neighbour reaches ends after one sweep: the
    target's entry (1 - alpha, written by the level's preparation) stays in the array that sweep read.  A forward call
    follows, of one query, so that it runs one sweep per dense level whatever the timing: one with an odd and one with
    an even number, so that the next backward call starts on either array; it has one target too, so it takes the same
    column in its first sweep, and must equal the same call on a fresh handle (an entry that survived is gathered by
    the dead end's in-neighbours in that sweep)."""
    d = R.design().names
    stale = [d["dead"][250]]  # 41 in-edges: (1 - alpha) / 3 at the most reaches an in-neighbour, below the 0.5
    targets = [d["ring"][5]]
    fresh = r.graph("rows")
    fresh.set_tuning(sweep_tuning(r.pkg))
    want, _, _, wpq = fresh.ppr_targets(targets, A, D.BWD_RMAX)
    # one source with an odd and one with an even number of dense levels (by the twin), past the two sweeps that run
    # over every tile
    between_srcs = {}
    for s in sources(r.pkg, "positions") + sources(r.pkg, "dead_ends"):
        n = r.twin("rows", 1, s)[1].dense_levels
        if n >= 3:
            between_srcs.setdefault(n % 2, s)
    assert sorted(between_srcs) == [0, 1], between_srcs
    parities = set()
    for between in between_srcs.values():
        g = r.graph("rows")
        r.forward(g, "rows", 1, sources(r.pkg, "sixteen"), "before the backward call")
        g.set_tuning(sweep_tuning(r.pkg))
        _, _, st, pq = g.ppr_targets(stale, A, 0.5)
        assert st.class_launches[5] == 1, (st.class_launches[5], [x.levels for x in pq])  # one sweep, and the call ends
        r.count(st)
        g.set_tuning(sweep_tuning(r.pkg))
        _, _, _, _, _, fst = g.fora_batch_single_source([between], EPS, A, seed=3, n_rounds=1, fetch=True, per_query=True)
        r.count(fst)
        assert fst.class_launches[5] >= 3, fst.class_launches[5]
        parities.add(fst.class_launches[5] % 2)
        got, _, st, pq = g.ppr_targets(targets, A, D.BWD_RMAX)
        r.count(st)
        assert [x.levels for x in pq] == [x.levels for x in wpq], between
        assert diff(got, want) <= TOL_PUSH, (between, diff(got, want))
        r.vectors.append(np.array(got))
    assert parities == {0, 1}, parities


def case_query_stream(r):
    """The query stream: two submissions through one driver, queries resumed from sweep to sweep with no call around
    them, against the batched call on a fresh handle."""
    g, fresh = r.graph("rows"), r.graph("rows")
    blocks = [sources(r.pkg, "positions") + sources(r.pkg, "dead_ends"), sources(r.pkg, "sixteen")]
    g.set_tuning(sweep_tuning(r.pkg))
    with r.pkg.QueryStream(g, EPS, A, k=8) as qs:
        tickets = [qs.submit(b, 5 + i) for i, b in enumerate(blocks)]
        got = [qs.wait(t) for t in tickets]
    fresh.set_tuning(sweep_tuning(r.pkg))
    for i, (b, (ids, vals, nsel, st)) in enumerate(zip(blocks, got)):
        _, ids2, vals2, nsel2, _, st2 = fresh.fora_batch_single_source(b, EPS, A, seed=5 + i, k=8)
        assert np.array_equal(nsel, nsel2) and np.array_equal(ids, ids2), i
        assert diff(vals, vals2) <= TOL_PUSH, (i, diff(vals, vals2))
        assert st.walks == st2.walks and st.levels == st2.levels
        r.vectors.append(np.array(vals))
        r.counters.append(tuple(int(x) for x in ids.ravel()))
        r.count(st)
        r.count(st2)


def case_topk_call(r):
    """A batched top-k call (rounds with their own thresholds, parked and armed rows) against the single-query entry
    point, which runs other kernels."""
    g = r.graph("rows")
    srcs = sources(r.pkg, "positions") + sources(r.pkg, "dead_ends")
    k = 8
    g.set_tuning(sweep_tuning(r.pkg))
    if "topk" not in _refs:
        _refs["topk"] = [g.fora_topk(s, EPS, A, k, seed=11 + i, cap=k) for i, s in enumerate(srcs)]
    ids, vals, st = g.fora_batch_topk(srcs, k, EPS, A, seed=11)
    assert st.class_launches[5] > 0
    rounds = 0
    for i, s in enumerate(srcs):
        nsel, sids, svals, _, sts = _refs["topk"][i]
        m = min(nsel, k)
        assert list(ids[i][:m]) == list(sids[:m]), (i, s)
        assert diff(vals[i][:m], svals[:m]) <= TOL_MC, (i, s)
        rounds += sts.rounds
    assert st.rounds == rounds
    r.vectors.append(np.array(vals))
    r.counters.append(tuple(int(x) for x in ids.ravel()))
    r.count(st)


def case_original_ids(r):
    """PPRHIP_RELABEL=0: a row's ordinal is not its node, every sweep runs over every tile; the dead-end tiles are found
    from the records all the same."""
    g = r.graph("rows", relabel=False)
    r.forward(g, "rows", 1, sources(r.pkg, "positions"), "original ids")


CASES = {"columns_reused": case_columns_reused, "two_calls": case_two_calls, "source_positions": case_source_positions,
         "dead_end_tiles_1": case_dead_end_tiles(1), "dead_end_tiles_2": case_dead_end_tiles(2),
         "dead_end_tiles_5": case_dead_end_tiles(5), "designs_of_the_sweep": case_designs_of_the_sweep,
         "seeded_call": case_seeded_call, "backward_call": case_backward_call, "topk_call": case_topk_call,
         "original_ids": case_original_ids, "stale_entry_of_a_backward_call": case_stale_entry_of_a_backward_call,
         "query_stream": case_query_stream}
# the cases whose graph has dead-end tiles and whose pushes reach them, and those with an entry sweep over them
DEAD_END_CASES = sorted(set(CASES) - {"designs_of_the_sweep"})
ENTRY_CASES = ("dead_end_tiles_2", "dead_end_tiles_5")


def run_case(pkg, orc, monkeypatch, case, grid=None, env=()):
    for k in ("PPRHIP_APPLY_GRID", "PPRHIP_APPLY_ALL_ROWS", "PPRHIP_APPLY_COUNT_RES"):
        monkeypatch.delenv(k, raising=False)
    if grid is not None:
        monkeypatch.setenv("PPRHIP_APPLY_GRID", str(grid))
    for k in env:
        monkeypatch.setenv(k, "1")
    r = Run(pkg, orc, monkeypatch)
    try:
        CASES[case](r)
    finally:
        r.close()
    return r


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_case(pkg, orc, monkeypatch, case, grid):
    r = run_case(pkg, orc, monkeypatch, case, grid)
    assert (r.res_count, r.res_loads, r.entry_tiles) == (0, 0, 0)  # (the counting is off)


@pytest.mark.parametrize("case", sorted(CASES))
def test_no_residue_on_dead_ends(pkg, orc, monkeypatch, case):
    """The residues of dead-end tiles, loaded and counted: none is non-zero on any path of the cases."""
    r = run_case(pkg, orc, monkeypatch, case, None, ("PPRHIP_APPLY_COUNT_RES",))
    print(case, "non-zero", r.res_count, "loads", r.res_loads, "entry tiles", r.entry_tiles)
    assert r.res_count == 0, r.res_count
    if case in DEAD_END_CASES:
        assert r.res_loads > 0  # the counting branch ran: so many residues were loaded and looked at
    if case in ENTRY_CASES:
        assert r.entry_tiles > 0  # an entry sweep came by dead-end tiles


@pytest.mark.parametrize("case", sorted(CASES))
def test_lean_equals_all_rows(pkg, orc, monkeypatch, case):
    lean = run_case(pkg, orc, monkeypatch, case)
    full = run_case(pkg, orc, monkeypatch, case, None, ("PPRHIP_APPLY_ALL_ROWS",))
    assert lean.counters == full.counters
    assert len(lean.vectors) == len(full.vectors)
    for a, b in zip(lean.vectors, full.vectors):
        assert diff(a, b) <= TOL_PUSH, diff(a, b)
