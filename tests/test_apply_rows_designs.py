"""The designed graph of tests/apply_rows_designs.py carries the cases tests/test_gpu_batched_apply_rows.py runs on it:
asserted here on the inspected layout (pkg.lift_host, no device), so a design that loses one fails."""
import numpy as np

import apply_rows_designs as R
import batch_sweep_designs as D


def side_of(pkg):
    return D.inspect_forward(pkg, R.design().host(pkg))


def test_tile_classes(pkg):
    s = side_of(pkg)
    cls = R.tile_classes(s)
    assert s.n_nz == R.RING + R.DEAD and s.n_z == R.POOL
    assert s.n_tiles == 27 and s.n_tiles % 2 == 1  # the last pair is half empty
    # four ring tiles, a tile mixing ring rows and dead ends, four dead-end tiles, the boundary tile, seventeen
    # tiles without in-edges of which the last is not full
    assert list(cls) == [R.PLAIN] * 5 + [R.DEAD_END] * 4 + [R.PLAIN] + [R.NO_IN] * 17
    assert (cls == R.DEAD_END).sum() >= 3
    dout = np.diff(np.asarray(s.lift["out_rp"], dtype=np.int64))
    mixed = dout[s.rows[4 * R.TILE:5 * R.TILE]]
    assert (mixed == 0).any() and (mixed > 0).any()
    assert 0 < s.n_nz % R.TILE < R.TILE - 1 and (s.n_rows % R.TILE) != 0
    # with the relabeling a row's ordinal is its node, which is how the launcher finds a source's tile
    assert np.array_equal(s.rows, np.arange(s.n_nz)) and np.array_equal(s.z_rows, s.n_nz + np.arange(s.n_z))


def test_dead_end_rows_cross_chunks_and_blocks(pkg):
    s = side_of(pkg)
    dead_lo, dead_hi = R.RING, R.RING + R.DEAD
    cross_dead = [int(j) for j in np.flatnonzero(s.cross) if dead_lo <= j < dead_hi]
    assert len(cross_dead) >= 3
    cls = R.tile_classes(s)
    assert any(cls[j // R.TILE] == R.DEAD_END for j in cross_dead)  # cross rows inside a dead-end tile
    # two blocks cut inside the dead-end range, in front of a dead-end tile; five blocks with the same cut and empty ones
    assert [j for j, _, _, _ in s.blocks(2)] == [0, R.HEAVY_FROM]
    assert cls[R.HEAVY_FROM // R.TILE] == R.DEAD_END and dead_lo < R.HEAVY_FROM < dead_hi
    assert sorted(set(j for j, _, _, _ in s.blocks(5))) == [0, R.HEAVY_FROM]


def test_sources_lie_where_the_cases_say(pkg):
    s = side_of(pkg)
    cls = R.tile_classes(s)
    S = R.source_sets(s)
    z_tiles = [int(t) for t in np.flatnonzero(cls == R.NO_IN)]
    boundary = s.n_nz // R.TILE
    pos = [R.tile_of(s, x) for x in S["positions"]]
    assert pos[0] == boundary and cls[boundary] == R.PLAIN
    assert pos[1] == z_tiles[0] and pos[2] == z_tiles[-1] == s.n_tiles - 1
    assert pos[3] == pos[4] and cls[pos[3]] == R.NO_IN and S["positions"][3] != S["positions"][4]
    six = [R.tile_of(s, x) for x in S["sixteen"]]
    assert len(set(six)) == 16 and all(cls[t] == R.NO_IN for t in six)
    # columns change hands: 40 and more queries, sources without in-edges in many tiles, rows with in-edges and
    # queries that never push in between; neighbours in the list never share a source
    reuse = S["reuse"]
    tiles = [R.tile_of(s, x) for x in reuse]
    assert len(reuse) >= 40 and all(a != b for a, b in zip(reuse, reuse[1:]))
    assert len(set(t for t in tiles if cls[t] == R.NO_IN)) >= 8
    assert sum(1 for t in tiles if cls[t] == R.PLAIN) >= 12
    # the second call's sources are not the first's
    assert not set(S["second_call"]) & set(S["sixteen"])
    assert len(set(R.tile_of(s, x) for x in S["second_call"])) >= 8


def test_mass_returns_to_sources_without_in_edges(pkg):
    """A query from a row without in-edges sends mass to dead ends and takes it back over many consecutive levels."""
    host = R.design().host(pkg)
    s = D.inspect_forward(pkg, host)
    rmax = D.fora_rmax(pkg, host)
    S = R.source_sets(s)
    for src in (S["positions"][1], S["positions"][2], S["dead_ends"][1]):
        _, _, levels, dead_pops = D.push_fwd(host, src, D.ALPHA, rmax)
        assert levels >= 10 and dead_pops >= 100, (src, levels, dead_pops)
    dout = np.diff(host.out_rp.astype(np.int64))
    assert dout[S["dead_ends"][6]] == 0 and D.push_fwd(host, S["dead_ends"][6], D.ALPHA, rmax)[2] == 0
