"""The designs of tests/batch_sweep_designs.py held to their claims, without a device: every feature by name on the
inspector's output (both sides where claimed), the inspector against the lift's own arrays, the numpy pushes against the
oracle twin, and every mutant caught by the queries the GPU tests run (tests/test_gpu_batched_sweep.py)."""
import numpy as np
import pytest

import batch_sweep_designs as D
from conftest import to_oracle

TOL_PUSH = 1e-12  # tests/test_gpu_parity.py
TOL_MC = 1e-9
MARGIN = 1000 * TOL_MC  # the GPU tests hold a FORA vector to TOL_MC against the twin (and to TOL_PUSH, tighter,
#                         against the single-query entry point): a mutant has to miss the wider of the two by 1 000 x
GS_COUNTS = (2, 3, 6, 5)  # 5 and 6 leave a block empty

FWD_CLAIMS = {
    "edges": ["E1_group_of_128_single_edge_rows", "E1_group_with_short_rows_and_the_end_of_a_longer_one",
              "E2_row_into_next_group", "E2_row_through_two_startless_groups", "E3_row_starts_on_group_first_edge",
              "E3_row_ends_on_group_last_edge", "E4_row_ends_on_chunk_last_edge_then_row_on_chunk_first_edge",
              "E4_row_fills_one_chunk", "E5_row_crosses_one_chunk_boundary",
              "E5_long_row_over_a_chunk_without_row_start", "E6_m_not_multiple_of_chunk",
              "E7_row_gathers_ids_255_and_256", "A1_mixed_tile_is_filled_from_z_rows",
              "A1_tile_mixes_rows_with_and_without_edges_odd_tile_count", "A4_tile_with_cross_and_plain_rows"],
    "blocks": ["E6_m_multiple_of_chunk", "A2_rows_fill_their_tiles", "A4_tile_with_cross_and_plain_rows",
               "E5_row_crosses_one_chunk_boundary", "E4_row_ends_on_chunk_last_edge_then_row_on_chunk_first_edge"],
    "small": ["E7_fewer_nodes_than_table_lines", "A1_tile_mixes_rows_with_and_without_edges_odd_tile_count",
              "E6_m_not_multiple_of_chunk", "A4_tile_with_cross_and_plain_rows"],
}
# the backward side: (design, transposed) -> features
BWD_CLAIMS = {
    ("edges", False): ["E1_group_of_128_single_edge_rows", "E1_group_with_short_rows_and_the_end_of_a_longer_one",
                       "E2_row_into_next_group", "E3_row_starts_on_group_first_edge", "E3_row_ends_on_group_last_edge",
                       "E4_row_ends_on_chunk_last_edge_then_row_on_chunk_first_edge",
                       "E5_row_crosses_one_chunk_boundary", "E6_m_not_multiple_of_chunk",
                       "E7_row_gathers_ids_255_and_256", "A4_tile_with_cross_and_plain_rows"],
    ("edges", True): ["E1_group_with_short_rows_and_the_end_of_a_longer_one", "E2_row_into_next_group",
                      "E3_row_starts_on_group_first_edge", "E3_row_ends_on_group_last_edge",
                      "E5_row_crosses_one_chunk_boundary", "E6_m_not_multiple_of_chunk",
                      "A1_mixed_tile_is_filled_from_z_rows", "A4_tile_with_cross_and_plain_rows"],
    ("blocks", False): ["E5_long_row_over_a_chunk_without_row_start", "E7_row_gathers_ids_255_and_256",
                        "E5_row_crosses_one_chunk_boundary", "E6_m_multiple_of_chunk",
                        "A4_tile_with_cross_and_plain_rows"],
    ("blocks", True): ["E2_row_through_two_startless_groups", "E2_row_into_next_group",
                       "E5_row_crosses_one_chunk_boundary", "E6_m_multiple_of_chunk", "A2_rows_fill_their_tiles",
                       "A4_tile_with_cross_and_plain_rows"],
    ("small", False): ["E7_fewer_nodes_than_table_lines", "A1_tile_mixes_rows_with_and_without_edges_odd_tile_count"],
    ("small", True): ["E7_fewer_nodes_than_table_lines", "A1_tile_mixes_rows_with_and_without_edges_odd_tile_count"],
}
BLOCK_CLAIMS = {2: ["B2_boundary_on_a_chunk_boundary"],
                3: ["B1_boundary_inside_a_chunk", "B2_boundary_on_a_chunk_boundary",
                    "B3_chunk_crossing_row_last_of_block"],
                5: ["B4_empty_block", "B1_boundary_inside_a_chunk"],
                6: ["B1_boundary_inside_a_chunk", "B2_boundary_on_a_chunk_boundary",
                    "B3_chunk_crossing_row_last_of_block", "B3_chunk_crossing_row_first_of_block", "B4_empty_block"]}

_cache = {}


def laid(pkg, name, transposed=False):
    """(host, forward side, backward side) of a design or its transpose, lifted once."""
    key = (name, transposed)
    if key not in _cache:
        d = D.all_designs()[name]
        host = d.transposed(pkg) if transposed else d.host(pkg)
        lift = pkg.lift_host(host)
        _cache[key] = (host, D.inspect_forward(pkg, host, lift), D.inspect_backward(pkg, host, lift))
    return _cache[key]


def sweep_tuning(orc, B=1):
    t = orc.tuning_default()
    t.dense_frac, t.gs_frac, t.gs_blocks = 1e-9, 1e-9, B
    return t


# ------------------------------------------------------------------ 1. the designs carry their features
def test_design_sizes(pkg):
    for name in D.all_designs():
        host, fwd, _ = laid(pkg, name)
        assert host.n <= 4000 and host.m <= 30000, name
    assert laid(pkg, "blocks")[1].n_nz >= 1024
    assert laid(pkg, "small")[0].n < D.HOT_LINES


@pytest.mark.parametrize("name,feature", [(n, f) for n, fs in FWD_CLAIMS.items() for f in fs])
def test_forward_side_carries(pkg, name, feature):
    _, fwd, _ = laid(pkg, name)
    found = {**D.edge_features(fwd), **D.apply_features(fwd)}[feature]
    assert found, (name, feature)


@pytest.mark.parametrize("name,transposed,feature", [(n, t, f) for (n, t), fs in BWD_CLAIMS.items() for f in fs])
def test_backward_side_carries(pkg, name, transposed, feature):
    _, _, bwd = laid(pkg, name, transposed)
    found = {**D.edge_features(bwd), **D.apply_features(bwd)}[feature]
    assert found, (name, transposed, feature)


@pytest.mark.parametrize("B", sorted(BLOCK_CLAIMS))
def test_block_cuts_carry(pkg, B):
    _, fwd, _ = laid(pkg, "blocks")
    assert fwd.n_nz >= 1024
    found = D.block_features(fwd, B)
    for feature in BLOCK_CLAIMS[B]:
        assert found[feature], (B, feature, fwd.blocks(B))
    for j_lo, j_hi, e_lo, e_hi in fwd.blocks(B):
        assert j_lo % D.BLOCK_ROWS == 0 and j_lo <= j_hi and e_lo <= e_hi


def test_named_rows_lie_where_the_design_says(pkg):
    """The positions the docstrings of the designs state, and the pool node a query starts from on the edge it is
    meant to feed."""
    d = D.all_designs()["edges"]
    _, s, _ = laid(pkg, "edges")
    old2new = np.argsort(s.new2old)
    span = lambda v: (int(s.first[s.ordinal_of(old2new[v])]), int(s.last[s.ordinal_of(old2new[v])]) + 1)
    nm = d.names
    assert span(nm["hub"]) == (0, 100) and old2new[nm["hub"]] == 0
    assert span(nm["a"]) == (100, 128) and span(nm["b"]) == (256, 456) and span(nm["c"]) == (512, 1024)
    assert span(nm["d"]) == (1024, 1524) and span(nm["e"]) == (1524, 1554) and span(nm["f"]) == (1554, 2754)
    assert span(nm["last_row"])[1] == s.m and s.m % D.CHUNK == 192
    assert s.group_starts[4].sum() == 0  # the chunk inside f
    for row, i in (("b", 199), ("c", 511), ("e", 29), ("f", 700), ("f", 1199)):  # pool[i] on the row's i-th edge
        assert s.new2old[s.ci[span(nm[row])[0] + i]] == nm["pool"][i], (row, i)
    assert old2new[255] == 255 and old2new[256] == 256  # the two H rows at the table's edge, both gathered by R7
    r7 = s.ci[span(nm["R7"])[0]:span(nm["R7"])[1]]
    assert 255 in r7 and 256 in r7
    # the rows the apply kernel carries last: the forty extra nodes; a query starts from the very last
    assert s.new2old[s.z_rows[-1]] == nm["extra"][-1] and nm["extra"][-1] in d.sources
    db = D.all_designs()["blocks"]
    _, sb, _ = laid(pkg, "blocks")
    o2n = np.argsort(sb.new2old)
    for j, e in ((256, 3000), (512, 5120), (768, 7300), (1024, 9000)):
        assert sb.first[j] == e and o2n[j] == j
    assert (sb.first[255], sb.last[255]) == (2500, 2999) and (sb.first[768], sb.last[768]) == (7300, 7699)
    assert sb.new2old[sb.ci[2800]] == db.names["pool"][300] and sb.new2old[sb.ci[7600]] == db.names["pool"][300]
    assert sb.new2old[sb.ci[2950]] == db.names["pool"][450]
    ds = D.all_designs()["small"]
    _, ss, _ = laid(pkg, "small")
    nz_j, z_j = ss.tile_rows(ss.n_tiles - 1)
    assert nz_j.size == 22 and z_j.size == 30
    assert set(ss.new2old[ss.rows[nz_j]]) >= set(ds.names["dead"])  # the dead ends lie in the mixed tile
    assert set(ss.new2old[ss.z_rows[z_j]]) == set(ds.names["pool"])


# ------------------------------------------------------------------ 2. the inspector reads the layout as the lift wrote it
@pytest.mark.parametrize("name,transposed", sorted(BWD_CLAIMS))
def test_inspector_against_lift_arrays(pkg, name, transposed):
    host, fwd, bwd = laid(pkg, name, transposed)
    L = fwd.lift
    assert np.array_equal(fwd.cross, fwd.cross_given)  # the cross rule recomputed = the lift's bits
    flags = np.unpackbits(L["flags"], bitorder="little").astype(bool)
    want = np.zeros(flags.size, dtype=bool)
    want[fwd.first] = True
    assert np.array_equal(flags, want)
    starts = np.concatenate([[0], np.cumsum(fwd.group_starts.sum(axis=1))])
    assert np.array_equal(L["chunk_starts"][:starts.size], starts)
    assert not L["in_ci"][host.m:].any()  # the padding behind edge m gathers internal vertex 0
    # internal order: nodes with in-edges first, by out-degree descending, ties by id
    dout = np.diff(host.out_rp.astype(np.int64))
    din = np.diff(host.in_rp.astype(np.int64))
    order = sorted(range(host.n), key=lambda v: (din[v] == 0, -dout[v], v))
    assert np.array_equal(fwd.new2old, order)
    # backward side: rows with out-edges in internal order; behind them the rows without that somebody points to
    assert np.array_equal(bwd.rows, [i for i, v in enumerate(order) if dout[v] > 0])
    assert np.array_equal(bwd.z_rows, [i for i, v in enumerate(order) if dout[v] == 0 and din[v] > 0])
    assert np.array_equal(np.diff(L["out_rp"].astype(np.int64))[bwd.rows], bwd.length)


# ------------------------------------------------------------------ 3. the numpy pushes are the twin's
def test_forward_push_equals_twin(pkg, orc):
    try:
        for name, d in D.all_designs().items():
            host, fwd, _ = laid(pkg, name)
            og = to_oracle(orc, host)
            rmax = D.fora_rmax(pkg, host)
            worst, dead = 0.0, {}
            for B in (1,) + (GS_COUNTS if name == "blocks" else ()):
                orc.set_sync_tuning(sweep_tuning(orc, B))
                for s in d.sources:
                    p, r, levels, dead_pops = D.push_fwd(host, s, D.ALPHA, rmax, B=B, side=fwd if B > 1 else None)
                    po, ro, _, sto = og.forward_push(s, D.ALPHA, rmax, orc.SYNC)
                    err = max(float(np.max(np.abs(p - po))), float(np.max(np.abs(r - ro))))
                    worst = max(worst, err)
                    assert err <= TOL_PUSH, (name, B, s, err)
                    assert levels == sto.levels == sto.dense_levels and dead_pops == sto.dead_end_pops, (name, B, s)
                    dead[s] = dead_pops
                    if B == 1:  # the gathers through the inspected layout are the plain ones
                        p2, r2, l2, _ = D.push_fwd(host, s, D.ALPHA, rmax, side=fwd, mutant="none")
                        assert np.array_equal(p, p2) and np.array_equal(r, r2) and l2 == levels, (name, s)
            print("forward push, numpy against twin, %s: largest difference %.3e" % (name, worst))
            # A3: dead ends cross the threshold for a source with in-edges (the mass returns to its own row) and for
            # sources among the rows without in-edges
            if name == "edges":
                assert dead[d.names["hub"]] > 0 and dead[d.names["pool"][0]] > 0 and dead[d.names["extra"][-1]] > 0
            if name == "small":
                assert dead[d.names["hub"]] > 0 and dead[d.names["pool"][0]] > 0
    finally:
        orc.set_sync_tuning(None)


def test_backward_push_equals_twin(pkg, orc):
    for name, transposed, targets in D.backward_cases():
        host, _, _ = laid(pkg, name, transposed)
        og = to_oracle(orc, host)
        worst, deepest = 0.0, 0
        for t in targets:
            p, r, levels = D.push_bwd(host, t, D.ALPHA, D.BWD_RMAX)
            po, ro, sto = og.backward_push(t, D.ALPHA, D.BWD_RMAX, orc.SYNC)
            err = max(float(np.max(np.abs(p - po))), float(np.max(np.abs(r - ro))))
            worst, deepest = max(worst, err), max(deepest, levels)
            assert err <= TOL_PUSH and levels == sto.levels, (name, transposed, t, err, levels, sto.levels)
        assert deepest >= 3, (name, transposed)  # several consecutive sweeps
        print("backward push, numpy against twin, %s%s: largest difference %.3e" % (name, "^T" if transposed else "",
                                                                                     worst))


# ------------------------------------------------------------------ 4. every mutant is caught by the GPU tests' queries
def test_every_mutant_is_caught(pkg):
    """Per mutant: the queries the GPU tests run on its design (the design's sources at the FORA threshold, alpha 0.15;
    the block mutant at three blocks); the largest difference of the mutant's reserve from the true one over them must
    be at least MARGIN.  No mutant is left out."""
    assert set(D.MUTANT_CASES) == set(D.MUTANTS)
    margins = {}
    for mutant in D.MUTANTS:
        name, B = D.MUTANT_CASES[mutant]
        d = D.all_designs()[name]
        host, fwd, _ = laid(pkg, name)
        rmax = D.fora_rmax(pkg, host)
        best, where = 0.0, None
        for s in d.sources:
            true, _, _, _ = D.push_fwd(host, s, D.ALPHA, rmax, B=B, side=fwd)
            wrong, _, _, _ = D.push_fwd(host, s, D.ALPHA, rmax, B=B, side=fwd, mutant=mutant)
            diff = float(np.max(np.abs(true - wrong)))
            if diff > best:
                best, where = diff, s
        margins[mutant] = best
        print("mutant %-28s on %-6s gs_blocks %d: reserve off by %.3e (source %s), %.1e x TOL_MC"
              % (mutant, name, B, best, where, best / TOL_MC))
    print("smallest mutant margin: %.3e (%s), required %.1e" % (min(margins.values()), min(margins, key=margins.get),
                                                                 MARGIN))
    for mutant, best in margins.items():
        assert best >= MARGIN, (mutant, best)


def test_mutants_bite_where_they_are_aimed(pkg):
    """The mutant of a position is exposed by the query placed beside it (and not only by some other query)."""
    d = D.all_designs()["edges"]
    host, fwd, _ = laid(pkg, "edges")
    rmax = D.fora_rmax(pkg, host)
    pool = d.names["pool"]
    for mutant, s in (("later_group", pool[199]), ("later_chunk", pool[29]), ("startless_chunk", pool[700]),
                      ("pad_gathers", pool[29]), ("ids_below_256_zero", pool[0]), ("cross_rows_not_cleared", pool[29])):
        true = D.push_fwd(host, s, D.ALPHA, rmax, side=fwd)[0]
        wrong = D.push_fwd(host, s, D.ALPHA, rmax, side=fwd, mutant=mutant)[0]
        assert float(np.max(np.abs(true - wrong))) >= MARGIN, (mutant, s)
    # startless_chunk drops nothing but the middle of f: a query that feeds f's first chunk only does not see it
    true = D.push_fwd(host, pool[300], D.ALPHA, rmax, side=fwd)[0]
    wrong = D.push_fwd(host, pool[300], D.ALPHA, rmax, side=fwd, mutant="startless_chunk")[0]
    assert np.array_equal(true, wrong)
