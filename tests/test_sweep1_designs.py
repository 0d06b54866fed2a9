"""The designs of tests/sweep1_designs.py held to their claims, without a device: every feature by name on the
inspectors' output, the host lift of every design against test_host's numpy restatement (its first graphs that are no
R-MAT, and its first folded panels at small size), the layout models against plain CSR gathers, the numpy reference
against the oracle twin on every query the GPU tests run (tests/test_gpu_sweep1_designs.py), and every mutant caught by
those queries."""
import numpy as np
import pytest

import sweep1_designs as D
from conftest import to_oracle
from test_host import _lift_expected

pytestmark = pytest.mark.hooks  # the layout switches exist in the hooks library only

TOL_PUSH = 1e-12  # tests/test_gpu_parity.py
MARGIN = 1000 * TOL_PUSH  # a mutant has to miss the tolerance the GPU tests hold by 1 000 x

HOT_CLAIMS = ["H1_one_lane_gathers_ids_16380_to_16387", "H2_source_with_internal_id_16383",
              "H2_source_with_internal_id_16384", "H2_ids_16383_and_16384_are_gathered"]
SLICED_CLAIMS = ["S1_row_with_a_segment_in_every_slice", "S2_row_in_first_and_last_slice_only",
                 "S3_segment_starts_on_lane_0_bit_0", "S3_segment_starts_on_lane_0_bit_0_behind_chunk_0",
                 "S4_segment_spans_two_whole_chunks", "S4_chunk_without_start_flag",
                 "S5_segment_ends_on_chunk_last_edge", "S10_ids_above_the_last_source_are_never_gathered",
                 "S11_last_chunk_partly_filled"]
SLICED_BLOCK_CLAIMS = {1: ["S8_neighbouring_ranges_joined"],
                       2: ["S6_window_begins_and_ends_mid_chunk", "S7_two_windows_share_a_chunk",
                           "S8_neighbouring_ranges_joined", "S9_slice_without_edge_of_the_block"],
                       3: ["S6_window_begins_and_ends_mid_chunk", "S7_two_windows_share_a_chunk",
                           "S8_neighbouring_ranges_joined", "S9_slice_without_edge_of_the_block"]}
PANEL_CLAIMS = (["P1_panel_of_%d_parts" % s for s in (1, 3, 4, 5, 16, 17, 33)] +   # (32 and 33 together pass the size
                ["P2_last_panel_short", "P2_last_panel_under_256_rows_and_folded",  # bound: 33 and 17 are kept)
                 "P3_item_last_turn_is_padding", "P3_item_edges_exact_multiple_of_8192", "P4_item_of_1_turn",
                 "P4_item_of_2_turns", "P4_item_of_3_or_more_turns", "P7_row_with_in_edges_in_every_part",
                 "P7_row_with_in_edges_in_one_part", "P9_self_loop_in_a_panel_row",
                 "P9_parallel_relationships_in_a_panel_row"])
PANEL_BLOCK_CLAIMS = {1: ["P6_range_starts_unfolded_and_holds_a_folded_panel"],
                      2: ["P5_bound_cuts_an_unfolded_panel", "P6_range_starts_unfolded_and_holds_a_folded_panel"],
                      3: ["P5_bound_cuts_a_folded_panel", "P5_bound_cuts_an_unfolded_panel",
                          "P6_range_starts_unfolded_and_holds_a_folded_panel"],
                      6: ["P5_bound_cuts_a_folded_panel", "P5_bound_cuts_an_unfolded_panel"]}
LAID = [(name, layout) for name, d in D.all_designs().items() for layout in d.layouts]


def sweep_tuning(orc, B=1):
    t = orc.tuning_default()
    t.dense_frac, t.gs_frac, t.gs_blocks = 1e-9, 1e-9, B
    return t


# ------------------------------------------------------------------ 1. the designs carry their features
def test_design_sizes_and_internal_order(pkg, monkeypatch):
    for name, d in D.all_designs().items():
        host, L, side, _ = D.laid(pkg, name, d.layouts[0], monkeypatch)
        assert host.m <= 2.5e6, name   # "about 2^21": 79 parts of 32 768 edges cannot be had below 2.36 M
        # rows with in-edges, then the pool, lie in id order: what the designs' docstrings say in ids holds in ordinals
        k = side.n_nz + len(d.names["pool"])
        assert np.array_equal(L["new2old"][:k], np.arange(k)), name
        assert set(d.block_sources) <= set(d.sources)
    assert D.host_of(pkg, "hot").n > D.HOT


@pytest.mark.parametrize("feature", HOT_CLAIMS)
def test_hot_design_carries(pkg, monkeypatch, feature):
    host, _, _, rm = D.laid(pkg, "hot", "rowmajor", monkeypatch)
    found = D.hot_features(rm, host)[feature]
    assert found, feature
    d = D.all_designs()["hot"]
    if feature.startswith("H2_source"):
        assert found[0] in d.sources and found[0] in d.one_level
    if feature.startswith("H1"):
        assert found == [d.names["X"]]


def test_hot_design_without_relabelling(pkg, monkeypatch):
    """H3: under PPRHIP_RELABEL=0 the ids stay, n_hot is 0; neither handle of this design has a sliced or a panel copy."""
    _, L, _, rm = D.laid(pkg, "hot", "norelabel", monkeypatch)
    assert np.array_equal(L["new2old"], np.arange(rm.n)) and rm.n_hot == 0
    _, L1, _, rm1 = D.laid(pkg, "hot", "rowmajor", monkeypatch)
    assert rm1.n_hot == D.HOT
    for x in (L, L1):
        assert x["sl_ci"].size == 0 and x["panel_src"].size == 0


@pytest.mark.parametrize("feature", SLICED_CLAIMS)
def test_sliced_design_carries(pkg, monkeypatch, feature):
    _, _, _, sl = D.laid(pkg, "sliced", "sliced", monkeypatch)
    assert sl.S >= 3
    assert D.sliced_features(sl)[feature], feature


@pytest.mark.parametrize("B", sorted(SLICED_BLOCK_CLAIMS))
def test_sliced_block_cuts_carry(pkg, monkeypatch, B):
    _, _, side, sl = D.laid(pkg, "sliced", "sliced", monkeypatch)
    found = D.sliced_block_features(sl, side.blocks(B))
    for feature in SLICED_BLOCK_CLAIMS[B]:
        assert found[feature], (B, feature)


def test_sliced_design_at_the_window_cap(pkg, monkeypatch):
    _, _, side, sl = D.laid(pkg, "sliced", "sliced16", monkeypatch)
    asked = int(D.LAYOUT_ENV["sliced16"]["PPRHIP_SLICE_IDS"])
    assert (sl.n_src + asked - 1) // asked > D.MAX_WINDOWS and sl.S == D.MAX_WINDOWS
    assert len(sl.windows(side.blocks(2)[0])) >= 8  # many windows in one launch


def test_named_rows_of_the_sliced_design(pkg, monkeypatch):
    d = D.all_designs()["sliced"]
    _, _, _, sl = D.laid(pkg, "sliced", "sliced", monkeypatch)
    f = D.sliced_features(sl)
    nm = d.names
    assert nm["A"] in f["S1_row_with_a_segment_in_every_slice"]
    assert nm["L"] in f["S2_row_in_first_and_last_slice_only"] and nm["L2"] in f["S2_row_in_first_and_last_slice_only"]
    # A's 120 edges of the last slice end on a chunk's last edge; the segment behind starts on lane 0
    a_last = int(np.flatnonzero((sl.seg_row == nm["A"]) & (sl.seg_slice == sl.S - 1))[0])
    assert a_last in f["S5_segment_ends_on_chunk_last_edge"] and sl.seg_end[a_last] - sl.seg_off[a_last] == 120
    assert a_last + 1 in f["S3_segment_starts_on_lane_0_bit_0_behind_chunk_0"]
    d_seg = f["S4_segment_spans_two_whole_chunks"]
    assert [int(sl.seg_row[g]) for g in d_seg] == [nm["D"]] and sl.seg_end[d_seg[0]] - sl.seg_off[d_seg[0]] == 1536


@pytest.mark.parametrize("feature", PANEL_CLAIMS)
def test_panels_design_carries(pkg, monkeypatch, feature):
    _, L, _, pn = D.laid(pkg, "panels", "panel", monkeypatch)
    assert D.panel_features(pn, L)[feature], feature


@pytest.mark.parametrize("B", sorted(PANEL_BLOCK_CLAIMS))
def test_panel_block_cuts_carry(pkg, monkeypatch, B):
    _, _, side, pn = D.laid(pkg, "panels", "panel", monkeypatch)
    found = D.panel_block_features(pn, side.blocks(B))
    for feature in PANEL_BLOCK_CLAIMS[B]:
        assert found[feature], (B, feature)


def test_named_rows_of_the_panels_design(pkg, monkeypatch):
    d = D.all_designs()["panels"]
    _, L, _, pn = D.laid(pkg, "panels", "panel", monkeypatch)
    assert list(pn.parts) == [3, 33, 16, 5, 1, 4, 1, 17] and pn.rows[-1] == 200
    assert list(pn.folded) == [False, True, False, False, False, False, False, True]
    edges = np.bincount(pn.items[:, 2], weights=pn.item_edges, minlength=pn.n_panels)
    assert tuple(int(x) for x in edges) == D.PANEL_EDGES
    f = D.panel_features(pn, L)
    nm = d.names
    assert nm["X1"] in f["P7_row_with_in_edges_in_every_part"] and nm["SL"] in f["P9_self_loop_in_a_panel_row"]
    assert nm["X1"] in f["P9_parallel_relationships_in_a_panel_row"]
    assert set(nm["dead"][1:]) <= set(f["P7_row_with_in_edges_in_one_part"])
    # the last pool node of a panel's feed lies in the panel's last part (and, of panel 1, in no other)
    for p in (1, 2, 7):
        v = nm["pool"][nm["last_feed"][p]]
        s0, s1 = int(pn.panel_slot0[p]), int(pn.panel_slot0[p + 1])
        hit = np.flatnonzero((pn.src[s0:s1] == v) & ~pn.pad[s0:s1]) + s0
        items = np.unique(pn.slot_item[hit])
        assert items.size and items[-1] == pn.item0[p + 1] - 1, p
        if p == 1:
            assert items.size == 1


# ------------------------------------------------------------------ 2. the lift and the inspectors
@pytest.mark.parametrize("name,layout", [x for x in LAID if x[1] != "norelabel"])
def test_lift_host_equals_numpy_restatement(pkg, monkeypatch, name, layout):
    host, L, _, _ = D.laid(pkg, name, layout, monkeypatch)
    width = int(D.LAYOUT_ENV[layout].get("PPRHIP_SLICE_IDS", 393216))
    exp = _lift_expected(host, width=width, panels=layout == "panel")
    for key, want in exp.items():
        assert L[key].shape == want.shape, (key, L[key].shape, want.shape)
        assert np.array_equal(L[key], want), key
    assert ("sl_ci" in exp) == (layout in ("sliced", "sliced16")) and ("panel_src" in exp) == (layout == "panel")
    if "sl_ci" not in exp:
        assert L["sl_ci"].size == 0 and L["seg_row"].size == 0
    if "panel_src" not in exp:
        assert L["panel_src"].size == 0


@pytest.mark.parametrize("name,layout", LAID)
def test_inspectors_read_the_layout_as_the_lift_wrote_it(pkg, monkeypatch, name, layout):
    host, L, side, x = D.laid(pkg, name, layout, monkeypatch)
    if isinstance(x, (D.RowMajor, D.Sliced)):
        per_chunk = np.bincount(np.flatnonzero(x.start) // D.CHUNK, minlength=(x.m + D.CHUNK - 1) // D.CHUNK)
        assert np.array_equal(np.diff(x.chunk_starts)[:per_chunk.size], per_chunk)
    if isinstance(x, D.RowMajor):
        assert np.array_equal(np.flatnonzero(x.start), side.first) and np.array_equal(x.row_of_edge, side.row_of_edge)
    elif isinstance(x, D.Sliced):
        assert np.array_equal(np.flatnonzero(x.start), x.seg_off)
        assert np.array_equal(x.edge_base[x.seg_slice] <= x.seg_off, np.ones(x.n_seg, dtype=bool))
        assert np.array_equal(np.sort(x.ci), np.sort(side.ci)) and x.edge_base[-1] == x.m
        lo = np.minimum(x.ci // (-(-x.n_src // x.S) if layout == "sliced16" else 512), x.S - 1)
        assert np.array_equal(lo, np.searchsorted(x.edge_base, np.arange(x.m), side="right") - 1)
    else:
        assert int((~x.pad).sum()) == x.m and x.n_slots == int(x.items[:, 1].sum()) * D.STEP
        for p in range(x.n_panels):
            k = np.arange(x.parts[p])
            assert np.array_equal(x.items[x.item0[p]:x.item0[p + 1], 3], x.desc[p, 0] + k * x.rows[p])
        assert np.all(x.src[x.pad] == 0)
        edges = np.bincount(x.items[:, 2], weights=x.item_edges, minlength=x.n_panels).astype(np.int64)
        assert np.array_equal(x.parts, np.maximum(1, (edges + D.ITEM_EDGES - 1) // D.ITEM_EDGES))
        assert np.array_equal(x.folded, x.parts > D.FOLD_MIN)
    for B in D.all_designs()[name].gs_blocks:
        assert all(j_lo % D.BLOCK_ROWS == 0 and j_lo <= j_hi for j_lo, j_hi, _, _ in side.blocks(B))


def dense_c(n, seed):
    """Dense contributions in (0, 1) on a grid of 2^-20: every row sum is exact in float64 whatever the order of its
    additions, so the models can be held to the plain gathers far below the rounding of a reordered sum."""
    return np.random.default_rng(seed).integers(1, 1 << 20, size=n) / float(1 << 20)


@pytest.mark.parametrize("name,layout", LAID)
def test_layout_models_equal_plain_gathers(pkg, monkeypatch, name, layout):
    """row_sums of the unmutated model = the CSR gather: bit for bit where one contribution is non-zero (every designed
    source), to 1e-15 relative on dense contributions; one block and every cut the design names."""
    d = D.all_designs()[name]
    host, L, side, x = D.laid(pkg, name, layout, monkeypatch)
    dst = np.repeat(np.arange(host.n), np.diff(host.in_rp.astype(np.int64)))
    src = np.asarray(host.in_ci[:host.m], dtype=np.int64)
    orig_rows = x.new2old[x.nz_rows]
    worst = 0.0
    for B in (d.gs_blocks if layout != "norelabel" else (1,)):
        blocks = side.blocks(B)
        model = D.MODEL_OF[layout](x, blocks)
        cases = [(s, None) for s in sorted(set(d.sources + d.one_level))] + [(None, 1), (None, 2)]
        for s, seed in cases[:6] + cases[-2:] if name == "panels" else cases:
            if s is not None:
                c = np.zeros(host.n)
                c[s] = 0.85 / 3.0
            else:
                c = dense_c(host.n, seed)
            want = np.bincount(dst, weights=c[src], minlength=host.n)[orig_rows]
            got = np.zeros(x.n_nz)
            for b in range(len(blocks)):
                part = D.row_sums(model, c[x.new2old], b)
                got[blocks[b][0]:blocks[b][1]] = part[blocks[b][0]:blocks[b][1]]
            if s is not None:
                assert np.array_equal(got, want), (name, layout, B, s)
            else:
                rel = float(np.max(np.abs(got - want) / want))
                worst = max(worst, rel)
                assert rel <= 1e-15, (name, layout, B, rel)
    print("layout model %s/%s against the CSR gather: largest relative difference %.3e" % (name, layout, worst))


# ------------------------------------------------------------------ 3. the numpy reference is the twin's
def queries(d):
    """(gs_blocks, source) of the full pushes the GPU tests run on a design."""
    return [(B, s) for B in d.gs_blocks for s in (d.sources if B == 1 else d.block_sources)]


@pytest.mark.parametrize("name", sorted(D.all_designs()))
def test_reference_equals_twin(pkg, orc, monkeypatch, name):
    d = D.all_designs()[name]
    host, _, side, _ = D.laid(pkg, name, d.layouts[0], monkeypatch)
    og = to_oracle(orc, host)
    rmax = D.fora_rmax(pkg, host)
    worst, deepest, dead = 0.0, 0, {}
    try:
        for B, s in queries(d):
            orc.set_sync_tuning(sweep_tuning(orc, B))
            p, r, levels, dead_pops = D.reference(pkg, name, s, B, side=side)
            po, ro, _, sto = og.forward_push(s, D.ALPHA, rmax, orc.SYNC)
            err = max(float(np.max(np.abs(p - po))), float(np.max(np.abs(r - ro))))
            worst, deepest = max(worst, err), max(deepest, levels)
            assert err <= TOL_PUSH, (name, B, s, err)
            assert levels == sto.levels == sto.dense_levels and dead_pops == sto.dead_end_pops, (name, B, s)
            dead[s] = dead_pops
        assert deepest >= 10
        # P8: a source without in-edges whose dead-end mass returns to it
        assert dead[d.names["pool"][0]] > 0 and dead[d.names["z"]] > 0
        print("reference against twin, %s: %d queries, largest difference %.3e" % (name, len(queries(d)), worst))
    finally:
        orc.set_sync_tuning(None)


@pytest.mark.parametrize("name", sorted(D.all_designs()))
def test_reference_equals_twin_at_alpha_one_half(pkg, orc, monkeypatch, name):
    d = D.all_designs()[name]
    host, _, side, _ = D.laid(pkg, name, d.layouts[0], monkeypatch)
    og = to_oracle(orc, host)
    rmax = D.fora_rmax(pkg, host, 0.5)
    try:
        orc.set_sync_tuning(sweep_tuning(orc, 1))
        for s in d.block_sources[:3]:
            p, r, levels, dead_pops = D.reference(pkg, name, s, 1, alpha=0.5, side=side)
            po, ro, _, sto = og.forward_push(s, 0.5, rmax, orc.SYNC)
            err = max(float(np.max(np.abs(p - po))), float(np.max(np.abs(r - ro))))
            assert err <= TOL_PUSH and levels == sto.levels and dead_pops == sto.dead_end_pops, (name, s, err)
    finally:
        orc.set_sync_tuning(None)


@pytest.mark.parametrize("name", sorted(D.all_designs()))
def test_power_iteration_equals_twin(pkg, orc, name):
    d = D.all_designs()[name]
    host = D.host_of(pkg, name)
    og = to_oracle(orc, host)
    for s in d.block_sources[:2]:
        for iters in (1, 2, 5):
            err = float(np.max(np.abs(D.power_iteration(host, s, D.ALPHA, iters) - og.power_method(s, D.ALPHA, iters))))
            assert err <= TOL_PUSH, (name, s, iters, err)


def test_topk_cases_have_no_ties(pkg, orc):
    """The twin's k + 1 largest values of every FORA top-k case of the GPU tests differ: the ids have one order."""
    t = sweep_tuning(orc, 1)
    for name, cases in D.TOPK_CASES.items():
        d = D.all_designs()[name]
        og = to_oracle(orc, D.host_of(pkg, name))
        for i, k in cases:
            try:
                orc.set_sync_tuning(t)
                ref, _ = og.fora_topk(d.sources[i], D.EPS, D.ALPHA, k, seed=4, schedule=orc.SYNC)
            finally:
                orc.set_sync_tuning(None)
            assert np.min(-np.diff(np.sort(ref)[::-1][:k + 1])) >= D.TOPK_GAP, (name, i, k)


@pytest.mark.parametrize("name", sorted(D.all_designs()))
def test_one_level_queries(pkg, name):
    """Every one-level source has a threshold under which it alone pushes; the reference then stops after one level
    with exactly the expected vectors (equal addends: no rounding to argue about)."""
    d = D.all_designs()[name]
    host = D.host_of(pkg, name)
    for s in d.one_level:
        rmax = D.one_level_rmax(host, s)
        assert rmax is not None, (name, s)
        p, r, levels, dead_pops = D.reference_push(host, s, D.ALPHA, rmax)
        pe, re_ = D.one_level_expected(host, s)
        assert levels == 1 and dead_pops == 0 and np.array_equal(p, pe) and np.array_equal(r, re_), (name, s)
    nm = d.names
    dout = np.diff(host.out_rp.astype(np.int64))
    if name == "sliced":   # parallel relationships: c + c + c on D
        c = (1.0 - D.ALPHA) / dout[nm["pool"][800]]
        assert D.one_level_expected(host, nm["pool"][800])[1][nm["D"]] == (c + c) + c
    if name == "panels":
        c = (1.0 - D.ALPHA) / dout[30]
        assert dout[30] == 8 and D.one_level_expected(host, 30)[1][nm["X1"]] == c + c


# ------------------------------------------------------------------ 4. every mutant is caught by the GPU tests' queries
def test_mutants_and_cases_are_the_same_set():
    assert set(D.MUTANT_CASES) == {m for ms in D.MUTANTS.values() for m in ms}
    kind = {"rowmajor": "hot", "sliced": "sliced", "panel": "panel"}
    for m, (name, layout, B, idx) in D.MUTANT_CASES.items():
        d = D.all_designs()[name]
        assert m in D.MUTANTS[kind[layout]] and layout in d.layouts and B in d.gs_blocks
        assert all((B, d.sources[i]) in queries(d) for i in idx), m


@pytest.mark.parametrize("kind", sorted(D.MUTANTS))
def test_every_mutant_is_caught(pkg, monkeypatch, kind):
    """Per mutant: the queries MUTANT_CASES names (they are among the GPU tests': a design's sources at the FORA
    threshold, alpha 0.15, the named gs_blocks); the largest difference of the mutant's reserve or residue from the
    reference's must be at least MARGIN.  A mutant that never comes to rest is stopped 20 levels behind the reference."""
    margins = {}
    for mutant in D.MUTANTS[kind]:
        name, layout, B, idx = D.MUTANT_CASES[mutant]
        d = D.all_designs()[name]
        host, _, side, x = D.laid(pkg, name, layout, monkeypatch)
        rmax = D.fora_rmax(pkg, host)
        best = 0.0
        for s in (d.sources[i] for i in idx):
            p, r, levels, _ = D.reference(pkg, name, s, B, side=side)
            wp, wr, _, _ = D.layout_push(host, layout, x, side, s, D.ALPHA, rmax, B=B, mutant=mutant,
                                         max_levels=levels + 20)
            best = max(best, float(np.max(np.abs(p - wp))), float(np.max(np.abs(r - wr))))
        margins[mutant] = best
        print("mutant %-28s on %-6s gs_blocks %d: off by %.3e, %.1e x TOL_PUSH" % (mutant, name, B, best, best / TOL_PUSH))
    for mutant, best in margins.items():
        assert best >= MARGIN, (mutant, best)


def test_unmutated_model_push_is_the_reference(pkg, monkeypatch):
    """The push through the unmutated model of each layout is the reference's, level for level."""
    for name, layout, B, i in (("hot", "rowmajor", 1, 3), ("sliced", "sliced", 2, 3), ("sliced", "sliced16", 3, 4),
                               ("panels", "panel", 3, 0)):
        d = D.all_designs()[name]
        host, _, side, x = D.laid(pkg, name, layout, monkeypatch)
        s = d.sources[i]
        p, r, levels, dead = D.reference(pkg, name, s, B, side=side)
        p2, r2, l2, d2 = D.layout_push(host, layout, x, side, s, D.ALPHA, D.fora_rmax(pkg, host), B=B)
        assert (l2, d2) == (levels, dead) and float(np.max(np.abs(p - p2))) <= 1e-15, (name, layout)
