"""A designed graph for the rows the batched apply kernel treats by class (csrc/kernels_dense_batch.hip:
k_build_apply_meta, k_dense_apply_batch, launch_dense_level_b8; engine.hpp: ApplyTileClass), beside the designs of
tests/batch_sweep_designs.py, whose inspector and reference it uses.

A 64-row tile whose rows all have in-edges and out-degree 0 is a dead-end tile: the kernel neither stages nor stores its
contribution lines and takes its residues for zero.  A tile whose rows all lie behind the rows with in-edges is only
visited when it holds the source of a column in the sweep, or did in one of the two sweeps before.  The internal order
(in-edges first, out-degree descending, ties by id) puts both kinds at the end of their ranges:

  rows    300 ring rows of out-degree 3 (j -> 3j + 1, 5j + 2 mod 300 and the dead end 300 + j), then 306 dead ends:
          n_nz = 606.  Tile 4 mixes 44 ring rows with 20 dead ends, tiles 5-8 are dead ends only, tile 9 holds the last
          30 dead ends and the first 34 rows without in-edges.  The dead ends from ordinal 512 on take 40 more in-edges
          each from the pool, so half of the edges lie behind ordinal 512: two blocks cut there, inside the dead-end
          range, and those rows cross chunk boundaries.  Behind them 1 098 pool nodes without in-edges (one edge into
          the ring each, the first 40 feed the heavy dead ends): sixteen full tiles 10-25 and 40 rows in tile 26, the
          27th: the last pair is half empty.  Two isolated nodes.

A query from a pool node sends a third of what the ring holds to dead ends at every level, and the dead ends return it
to the source, whose row has no in-edges: its tile is visited for as long as the query holds a column."""
import functools

import numpy as np

import batch_sweep_designs as D

TILE = D.TILE
PLAIN, DEAD_END, NO_IN = 0, 1, 2

RING, DEAD, POOL, HEAVY_FROM, HEAVY_FEED = 300, 306, 1098, 512, 40


def rows_design():
    ring = list(range(RING))
    dead = list(range(RING, RING + DEAD))
    pool = list(range(RING + DEAD, RING + DEAD + POOL))
    n = pool[-1] + 1 + 2
    edges = []
    for j in ring:
        edges += [(j, (3 * j + 1) % RING), (j, (5 * j + 2) % RING), (j, dead[j])]
    for i, p in enumerate(pool):
        edges.append((p, i % RING))
    for r in range(HEAVY_FROM, RING + DEAD):
        edges += [(pool[i], r) for i in range(HEAVY_FEED)]
    names = dict(ring=ring, dead=dead, pool=pool, isolated=n - 1)
    return D.Design("rows", n, edges, names, [])


@functools.lru_cache(maxsize=None)
def design():
    return rows_design()


def tile_classes(side):
    """The class of every apply tile by the kernel's rule, from the inspected forward side."""
    dout = np.diff(np.asarray(side.lift["out_rp"], dtype=np.int64))
    slots = side.n_tiles * TILE
    dead_row = np.zeros(slots, dtype=bool)
    dead_row[:side.n_nz] = dout[side.rows] == 0
    no_in = (np.arange(slots) >= side.n_nz).reshape(side.n_tiles, TILE).all(axis=1)
    dead = dead_row.reshape(side.n_tiles, TILE).all(axis=1)
    cls = np.full(side.n_tiles, PLAIN)
    cls[dead] = DEAD_END
    cls[no_in] = NO_IN
    return cls


def z_source(side, tile, k=0):
    """Original id of the k-th row of `tile` among the rows without in-edges."""
    lo = max(tile * TILE, side.n_nz) - side.n_nz
    return int(side.new2old[side.z_rows[lo + k]])


def tile_of(side, original):
    """Apply tile of a node's row (None: the sweep does not carry it)."""
    internal = int(np.flatnonzero(side.new2old == original)[0])
    j = side.ordinal_of(internal)
    if j is None:
        k = np.flatnonzero(side.z_rows == internal)
        if not k.size:
            return None
        j = side.n_nz + int(k[0])
    return j // TILE


def source_sets(side):
    """The source lists of the cases, by name (original ids), read off the inspected layout."""
    cls = tile_classes(side)
    z_tiles = [int(t) for t in np.flatnonzero(cls == NO_IN)]
    boundary = side.n_nz // TILE
    d = design().names
    first, last = z_tiles[0], z_tiles[-1]
    s = {}
    # the mixed boundary tile, the first and the last tile without in-edges, two sources in one tile, and ordinary rows
    s["positions"] = [z_source(side, boundary), z_source(side, first), z_source(side, last), z_source(side, first + 3, 5),
                      z_source(side, first + 3, 41), d["ring"][7], d["dead"][0], z_source(side, last, 39)]
    s["sixteen"] = [z_source(side, t, (7 * i) % TILE) for i, t in enumerate(z_tiles[:16])]
    # columns change hands: sources without in-edges from tile to tile, ring rows (long pushes), dead ends and an
    # isolated node (no push at all) in between
    reuse = []
    for i in range(48):
        kind = i % 4
        if kind in (0, 2):
            reuse.append(z_source(side, z_tiles[(5 * i) % len(z_tiles[:-1])], (11 * i) % TILE))
        elif kind == 1:
            reuse.append(d["ring"][(37 * i) % RING])
        else:
            reuse.append(d["dead"][(13 * i) % DEAD] if i % 8 == 3 else z_source(side, boundary, i % 30))
    s["reuse"] = reuse
    s["second_call"] = [z_source(side, z_tiles[(3 * i + 1) % 16], (5 * i + 2) % TILE) for i in range(12)] + [d["ring"][11]]
    s["dead_ends"] = [z_source(side, first, 1), d["pool"][0], d["pool"][39], d["ring"][0], d["ring"][299],
                      z_source(side, last, 3), d["dead"][250], d["pool"][500]]
    return s
