"""Designed graphs, a layout inspector and a numpy reference (with mutants) for the batched dense sweep
(csrc/kernels_dense_batch.hip: k_dense_edges_b, k_dense_apply_batch, launch_dense_level_b8).

The batched edge kernel sums a row of the sweep in five ways, by where the row lies in a 512-edge chunk and in the
chunk's four lane groups of 128 edges; around it sit the block tails, the zero padding behind edge m, the LDS table of
256 lines, the cross-bit clearing and the paired 64-row tiles of the apply kernel and the 256-row block cuts of the
Gauss-Seidel sweeps.  The internal order is fixed (lift.cpp: nodes with in-edges first, by out-degree descending, ties
by id; a row's in-edges keep their order), so a graph can put a row at every one of those positions on purpose:

  edges   E1-E5, E6 (m % 512 != 0), E7 (a row that gathers internal ids 255 and 256), A3, A4
  blocks  E6 (m % 512 == 0), A2 (n_nz % 64 == 0), B1-B4: 1 280 rows with in-edges, cuts at 256, 512, 768
  small   fewer than 256 nodes (the LDS table holds every vertex), A1 (one tile mixes rows with and without
          in-edges, an odd tile count), A3 (a source among zin_rows whose dead-end mass returns to it)

Rows are fed from a pool of nodes without in-edges (as tests/weighted_designs.dense_design does): row r of length L takes
its in-edges from pool[0 .. L), so pool[i] sits on the i-th edge of every row longer than i and a query from pool[i]
puts its one non-zero contribution exactly there.  edge_features, apply_features and block_features name every property; tests/test_batch_sweep_designs.py
asserts each on the inspector's output, so a design that loses one fails on the CPU.

The reference is push_fwd / push_bwd: frontier-synchronous pushes in numpy, float64 gathers in original ids, no layout
in them; every level a Jacobi pull (what dense_frac = 1e-9 and gs_blocks = 1 make the engine do) or, with B > 1, the
block sweeps of the oracle twin (entry, then in-place).  push_fwd(mutant=...) gathers through the inspected layout
with one wrong reading of it (MUTANTS); MUTANT_CASES names the design and the queries that expose each.

Not covered at these sizes: the grid-stride loops of both kernels, which need more than 4 096 chunks or about 260 000
rows to take a second trip; tests/test_gpu_scale.py runs graphs of that size."""
import functools

import numpy as np

from conftest import edges_to_host

CHUNK = 512      # in-edges a wave of the edge kernel owns
GROUP = 128      # edges of a lane group (16 lanes x 8 edges)
TILE = 64        # rows of an apply tile
BLOCK_ROWS = 256  # block cuts of the Gauss-Seidel sweeps are multiples of this many row ordinals
HOT_LINES = 256  # vertices in the edge kernel's LDS table (32 KB at 16 slots)

ALPHA = 0.15
EPS = 0.5


# ------------------------------------------------------------------ layout inspector
class Side:
    """One side of the sweep layout: rows (internal ids, in sweep order), the edge range of each, the vertex every edge
    gathers (internal id), the rows without edges the apply kernel carries behind them, cross bits."""

    def __init__(self, n, m, rows, z_rows, rp, ci, new2old, cross_given=None):
        self.n, self.m = int(n), int(m)
        self.rows = np.asarray(rows, dtype=np.int64)
        self.z_rows = np.asarray(z_rows, dtype=np.int64)
        self.n_nz, self.n_z = self.rows.size, self.z_rows.size
        rp = np.asarray(rp, dtype=np.int64)
        self.first = rp[self.rows]
        self.last = rp[self.rows + 1] - 1
        self.length = self.last - self.first + 1
        self.ci = np.asarray(ci[:self.m], dtype=np.int64)
        self.new2old = np.asarray(new2old, dtype=np.int64)
        self.n_chunks = (self.m + CHUNK - 1) // CHUNK
        self.pad = self.n_chunks * CHUNK - self.m
        # rows are contiguous and in order: the edge kernel finds a row by counting starts
        assert self.n_nz == 0 or (self.first[0] == 0 and self.last[-1] == self.m - 1)
        assert np.array_equal(self.first[1:], self.last[:-1] + 1)
        self.row_of_edge = np.repeat(np.arange(self.n_nz), self.length)
        self.first_chunk, self.last_chunk = self.first // CHUNK, self.last // CHUNK
        self.first_group, self.last_group = (self.first % CHUNK) // GROUP, (self.last % CHUNK) // GROUP
        # the rule of lift.cpp / graph.cpp: rows summed with atomics, cleared by the apply kernel
        self.cross = (self.first_chunk != self.last_chunk) | ((self.last + 1) % CHUNK == 0) | (self.last + 1 == self.m)
        self.cross_given = cross_given
        self.group_starts = np.zeros((self.n_chunks, CHUNK // GROUP), dtype=np.int64)  # row starts per chunk and group
        np.add.at(self.group_starts, (self.first_chunk, self.first_group), 1)
        self.n_rows = self.n_nz + self.n_z
        self.n_tiles = (self.n_rows + TILE - 1) // TILE

    def ordinal_of(self, internal):
        j = np.flatnonzero(self.rows == internal)
        return int(j[0]) if j.size else None

    def tile_rows(self, t):
        """(ordinals of rows with edges, indices into z_rows) of apply tile t."""
        lo, hi = t * TILE, min((t + 1) * TILE, self.n_rows)
        return np.arange(lo, min(hi, self.n_nz)), np.arange(max(lo, self.n_nz), hi) - self.n_nz

    def blocks(self, B):
        """gs_blocks_of's rule (levels.cpp): block b holds the ordinals [jb[b], jb[b + 1]), jb[b] = the first ordinal whose
        row start reaches b * m / B, rounded down to a multiple of 256.  Returns [(j_lo, j_hi, e_lo, e_hi)]."""
        jb = [0] * (B + 1)
        for b in range(1, B):
            target = b * self.m // B
            j = int(np.searchsorted(self.first, target, side="left")) & ~(BLOCK_ROWS - 1)
            jb[b] = max(jb[b - 1], j)
        jb[B] = self.n_nz
        edge = lambda j: int(self.first[j]) if j < self.n_nz else self.m
        return [(jb[b], jb[b + 1], edge(jb[b]), edge(jb[b + 1])) for b in range(B)]


def unpack_cross(words, count):
    bits = np.unpackbits(np.asarray(words, dtype="<u8").view(np.uint8), bitorder="little")
    return bits[:count].astype(bool)


def inspect_forward(pkg, host, lift=None):
    """The forward side: rows = nodes with in-edges over the lifted in-CSR, as pkg.lift_host gives them."""
    L = lift if lift is not None else pkg.lift_host(host)
    side = Side(host.n, host.m, L["nz_rows"], L["zin_rows"], L["in_rp"], L["in_ci"], L["new2old"],
                unpack_cross(L["cross"], L["nz_rows"].size))
    side.lift = L
    return side


def inspect_backward(pkg, host, lift=None):
    """The backward side as graph.cpp (ensure_bwd_layout) builds it: rows = nodes with out-edges, in internal order, over
    the lifted out-CSR; the rows behind them are the nodes without out-edges that somebody points to."""
    L = lift if lift is not None else pkg.lift_host(host)
    dout = np.diff(L["out_rp"].astype(np.int64))
    din = np.diff(L["in_rp"].astype(np.int64))
    side = Side(host.n, host.m, np.flatnonzero(dout > 0), np.flatnonzero((dout == 0) & (din > 0)), L["out_rp"],
                L["out_ci"], L["new2old"])
    side.lift = L
    return side


# ------------------------------------------------------------------ features, by name
def _rows(mask):
    return [int(j) for j in np.flatnonzero(mask)]


def edge_features(s):
    """E1-E7 on one side: name -> the row ordinals (or (chunk, group) pairs) that carry the feature; empty = absent."""
    f = {}
    same = s.first_chunk == s.last_chunk
    full = np.argwhere(s.group_starts == GROUP)
    f["E1_group_of_128_single_edge_rows"] = [tuple(int(x) for x in cg) for cg in full]
    carried = np.ones_like(s.group_starts, dtype=bool)  # the group's first edge is no row start: a row runs into it
    carried[s.first_chunk[s.first % GROUP == 0], s.first_group[s.first % GROUP == 0]] = False
    f["E1_group_with_short_rows_and_the_end_of_a_longer_one"] = [
        (int(c), int(g)) for c, g in np.argwhere((s.group_starts >= 3) & carried)
        if g > 0 and np.any((s.last // GROUP == c * 4 + g) & (s.first // GROUP < c * 4 + g) & (s.first_chunk == c))]
    f["E2_row_into_next_group"] = _rows(same & (s.last_group == s.first_group + 1))
    f["E2_row_through_two_startless_groups"] = _rows(same & (s.last_group == s.first_group + 3))
    f["E3_row_starts_on_group_first_edge"] = _rows((s.first % GROUP == 0) & (s.first % CHUNK != 0))
    f["E3_row_ends_on_group_last_edge"] = _rows((s.last % GROUP == GROUP - 1) & (s.last % CHUNK != CHUNK - 1))
    nxt = np.append(s.first[1:] % CHUNK == 0, False)
    f["E4_row_ends_on_chunk_last_edge_then_row_on_chunk_first_edge"] = _rows(same & (s.last % CHUNK == CHUNK - 1) &
                                                                              (s.length < CHUNK) & nxt)
    f["E4_row_fills_one_chunk"] = _rows((s.first % CHUNK == 0) & (s.length == CHUNK))
    f["E5_row_crosses_one_chunk_boundary"] = _rows((s.last_chunk == s.first_chunk + 1) & (s.first % CHUNK != 0))
    f["E5_long_row_over_a_chunk_without_row_start"] = _rows((s.length >= 1100) & (s.last_chunk >= s.first_chunk + 2) &
                                                            (s.first % CHUNK != 0))
    f["E6_m_not_multiple_of_chunk"] = [s.n_nz - 1] if s.m % CHUNK else []
    f["E6_m_multiple_of_chunk"] = [] if s.m % CHUNK else [s.n_nz - 1]
    both = []
    for j in range(s.n_nz):
        g = s.ci[s.first[j]:s.last[j] + 1]
        if np.any(g == HOT_LINES - 1) and np.any(g == HOT_LINES):
            both.append(j)
    f["E7_row_gathers_ids_255_and_256"] = both
    f["E7_fewer_nodes_than_table_lines"] = [0] if s.n < HOT_LINES else []
    return f


def apply_features(s):
    """A1, A2, A4 on one side (A3 is a property of the queries: see the tests)."""
    f = {}
    r = s.n_nz % TILE
    f["A1_tile_mixes_rows_with_and_without_edges_odd_tile_count"] = (
        [s.n_nz // TILE] if r not in (0, TILE - 1) and s.n_z >= 1 and s.n_tiles % 2 == 1 else [])
    f["A1_mixed_tile_is_filled_from_z_rows"] = [s.n_nz // TILE] if r and s.n_z >= TILE - r else []
    f["A2_rows_fill_their_tiles"] = [s.n_nz // TILE - 1] if r == 0 and s.n_nz else []
    mixed = []
    for t in range((s.n_nz + TILE - 1) // TILE):
        c = s.cross[t * TILE:min((t + 1) * TILE, s.n_nz)]
        if c.any() and not c.all():
            mixed.append(t)
    f["A4_tile_with_cross_and_plain_rows"] = mixed
    return f


def block_features(s, B):
    """B1-B4 for the cut into B blocks: name -> the block indices that carry the feature."""
    f = {"B1_boundary_inside_a_chunk": [], "B2_boundary_on_a_chunk_boundary": [],
         "B3_chunk_crossing_row_last_of_block": [], "B3_chunk_crossing_row_first_of_block": [],
         "B4_empty_block": []}
    crossing = s.first_chunk != s.last_chunk
    for b, (j_lo, j_hi, e_lo, e_hi) in enumerate(s.blocks(B)):
        if j_lo == j_hi:
            f["B4_empty_block"].append(b)
            continue
        if 0 < j_lo < s.n_nz:
            f["B1_boundary_inside_a_chunk" if e_lo % CHUNK else "B2_boundary_on_a_chunk_boundary"].append(b)
            if crossing[j_lo]:
                f["B3_chunk_crossing_row_first_of_block"].append(b)
        if j_hi < s.n_nz and crossing[j_hi - 1]:
            f["B3_chunk_crossing_row_last_of_block"].append(b)
    return f


# ------------------------------------------------------------------ designs
class Design:
    def __init__(self, name, n, edges, names, sources):
        self.name, self.n, self.edges, self.names, self.sources = name, n, edges, names, sources

    def host(self, pkg):
        return edges_to_host(pkg, self.n, self.edges)

    def transposed(self, pkg):
        return edges_to_host(pkg, self.n, [(v, u) for u, v in self.edges])


def _feed(edges, pool, row, count):
    edges += [(pool[i], row) for i in range(count)]


def edges_design():
    """Rows with in-edges, in internal order (= id order: the hub has out-degree 40, every H row 2, T1 rows 1, T0 0):
      hub     [0, 100)
      a       28 edges, [100, 128): ends on a group's last edge
      128 x 1 [128, 256): a lane group of single-edge rows, both mask words all ones; the first starts on a group's
              first edge
      b       200 edges, [256, 456): group 2 into group 3
      10, 10, 10, 26: group 3 holds the end of b and four short rows; the last ends on the chunk's last edge (511)
      c       512 edges, [512, 1024): starts on a chunk's first edge, fills the chunk, runs through two groups
              without a row start
      d       500 edges, [1024, 1524)
      e       30 edges, [1524, 1554): crosses one chunk boundary
      f       1 200 edges, [1554, 2754): chunk 4 = [2048, 2560) lies inside it and holds no row start
      130 x 3 filler; the H rows with ids 255 and 256 (internal ids 255 and 256) both point to R7
      T1      16 rows of out-degree 1 (R7 is the first), then T0: 24 dead ends; the last dead end's row ends at m,
              m % 512 = 192.
    Every H row points to two tail rows, the hub to all forty, T1 rows to dead ends.  Behind them the pool of 1 200
    nodes without in-edges, forty more with one out-edge each (1 549 rows for the apply kernel: tile 4 mixes the last
    53 rows with in-edges with pool rows, and 25 tiles leave the last pair half empty) and two isolated nodes."""
    lengths = [28] + [1] * 128 + [200, 10, 10, 10, 26, 512, 500, 30, 1200] + [3] * 130
    K = len(lengths)
    hub = 0
    H = list(range(1, 1 + K))
    T1 = list(range(1 + K, 1 + K + 16))
    T0 = list(range(T1[-1] + 1, T1[-1] + 1 + 24))
    pool = list(range(T0[-1] + 1, T0[-1] + 1 + 1200))
    extra = list(range(pool[-1] + 1, pool[-1] + 1 + 40))  # one out-edge each: the last rows the apply kernel carries
    n = extra[-1] + 1 + 2
    tails = T1 + T0
    edges = []
    _feed(edges, pool, hub, 100)
    for h, L in zip(H, lengths):
        _feed(edges, pool, h, L)
    R7 = T1[0]
    for j, h in enumerate(H):
        edges.append((h, R7 if h in (HOT_LINES - 1, HOT_LINES) else tails[(2 * j) % len(tails)]))
        edges.append((h, tails[(2 * j + 1) % len(tails)]))
    edges += [(hub, t) for t in tails]
    edges += [(t, T0[k % len(T0)]) for k, t in enumerate(T1)]
    edges += [(x, tails[k]) for k, x in enumerate(extra)]
    row = {nm: H[i] for nm, i in (("a", 0), ("b", 129), ("c", 134), ("d", 135), ("e", 136), ("f", 137))}
    names = dict(hub=hub, H=H, T1=T1, T0=T0, pool=pool, extra=extra, R7=R7, last_row=T0[-1], dead=T0[0], isolated=n - 1, **row)
    # beside the features: the pool node on b's last edge (group 3), on c's, on e's (behind the chunk boundary), in
    # the middle chunk of f and on f's last edge; pool[0] feeds every row (ids 255 and 256 among them); then the hub,
    # the last row without in-edges, rows with in-edges, a dead end, an isolated node
    sources = [pool[0], pool[29], pool[199], pool[511], pool[700], pool[1199], pool[2], extra[-1], hub, row["a"], R7,
               T1[5], T0[0], n - 1]
    return Design("edges", n, edges, names, sources)


def blocks_design():
    """1 279 ring rows of out-degree 3 (j -> 3j + 1, 5j + 2, 7j + 3 mod 1 279: three in-edges each) and a trap row (x -> x,
    fed by z) of out-degree 1: 1 280 rows with in-edges, in id order.  Row starts: ordinal 256 at edge 3 000 (inside
    chunk 5), 512 at 5 120 (a chunk boundary), 768 at 7 300, 1 024 at 9 000; m = 10 240 = 20 chunks.  Row 255 =
    [2 500, 3 000) crosses into chunk 5 and is the last row of block 0 at three blocks; row 768 = [7 300, 7 700) crosses
    into chunk 15 and is the first row of a block at six.  Four and six blocks leave block 0 empty."""
    R = 1279
    lengths = ([9] * 254 + [214, 500] + [8] * 255 + [80] + [8] * 255 + [140] + [400] + [5] * 254 + [30] +
               [4] * 254 + [222])
    assert len(lengths) == R
    x = R
    pool = list(range(R + 1, R + 1 + 497))
    z = pool[-1] + 1
    n = z + 1 + 2
    edges = []
    for j, L in enumerate(lengths):
        _feed(edges, pool, j, L - 3)
    for j in range(R):
        edges += [(j, (3 * j + 1) % R), (j, (5 * j + 2) % R), (j, (7 * j + 3) % R)]
    edges += [(z, x), (x, x)]
    names = dict(pool=pool, trap=x, z=z, row255=255, row256=256, row512=512, row768=768, isolated=n - 1)
    # pool[300] sits on row 255's edge 2 800 (the part of chunk 5 that block 1 shares) and row 768's 7 600; pool[450]
    # on 2 950 alone; pool[0] feeds every ring row (the shortest push); z feeds the trap (the longest)
    sources = [z, pool[300], pool[450], pool[0], pool[496], 255, 768, 0, x, n - 1]
    return Design("blocks", n, edges, names, sources)


def small_design():
    """182 nodes, fewer than the LDS table's 256 lines: 150 rows with in-edges (the hub with out-degree 20, 100 rows with 2,
    29 with 1, 20 dead ends), 30 pool nodes without in-edges and two isolated nodes.  180 rows make three apply tiles;
    the third holds the last 22 rows with in-edges (the dead ends) and the 30 pool rows."""
    nz, npool = 150, 30
    pool = list(range(nz, nz + npool))
    n = nz + npool + 2
    edges = []
    for i, p in enumerate(pool):
        edges += [(p, 5 * i + k) for k in range(5)]
        edges += [(p, (13 * i + 29 * k + 1) % nz) for k in range(1 + i % 4)]
    edges += [(0, d) for d in range(130, 150)]
    for j in range(1, 101):
        edges += [(j, (3 * j + 1) % nz), (j, (7 * j + 2) % nz)]
    for j in range(101, 130):
        edges.append((j, (11 * j) % nz))
    names = dict(hub=0, pool=pool, dead=list(range(130, 150)), isolated=n - 1)
    sources = [pool[0], pool[7], pool[29], 0, 1, 64, 129, 130, 149, n - 1]
    return Design("small", n, edges, names, sources)


@functools.lru_cache(maxsize=None)
def all_designs():
    return {d.name: d for d in (edges_design(), blocks_design(), small_design())}


BWD_RMAX = 1e-5  # threshold of the backward cases (un-normalised, strict)


def backward_cases():
    """(design, transposed, targets): the backward sweep runs over the out-CSR, so a design's transpose puts the
    designed rows (now out-rows, ordered by their length) on the backward side, and the design itself its pool rows;
    BWD_CLAIMS of the CPU tests names what each side carries.  Targets without in-edges (a one-entry answer) included."""
    e, b, s = (all_designs()[k].names for k in ("edges", "blocks", "small"))
    return [("edges", False, [e["dead"], e["last_row"], e["R7"], e["hub"], e["f"], e["pool"][0]]),
            ("edges", True, [e["pool"][0], e["pool"][199], e["pool"][700], e["hub"], e["R7"], e["dead"]]),
            ("blocks", False, [0, 255, 768, b["trap"]]),
            ("blocks", True, [b["pool"][0], b["pool"][300], b["z"], 255]),
            ("small", False, [s["hub"], s["dead"][0], 64]),
            ("small", True, [s["pool"][0], s["hub"], 1])]


def fora_rmax(pkg, host, alpha=ALPHA, eps=EPS):
    """The push threshold of a whole-graph FORA query with one round."""
    return pkg.fora_whole_params(pkg.conf_whole_graph(host.n, host.m, alpha), eps)[0]


# ------------------------------------------------------------------ numpy reference
MUTANTS = ("later_group", "later_chunk", "startless_chunk", "pad_gathers", "ids_from_256_zero", "ids_below_256_zero",
           "cross_rows_not_cleared", "shared_chunk_outside_block", "last_tile_skipped", "last_tile_z_rows_skipped")

# mutant -> (design, gs_blocks): the design built for it; the queries are the design's sources
MUTANT_CASES = {"later_group": ("edges", 1), "later_chunk": ("edges", 1), "startless_chunk": ("edges", 1),
                "pad_gathers": ("edges", 1), "ids_from_256_zero": ("edges", 1), "ids_below_256_zero": ("edges", 1),
                "cross_rows_not_cleared": ("edges", 1), "shared_chunk_outside_block": ("blocks", 3),
                "last_tile_skipped": ("small", 1), "last_tile_z_rows_skipped": ("small", 1)}


def _active(r, d, rmax):
    return np.where(d > 0, r / np.maximum(d, 1) >= rmax, r > 0.0)


class _Gather:
    """Row sums of one block pass.  Without a side: plain gathers over the host in-CSR.  With a side: through the
    inspected layout, where a mutant reads it wrongly."""

    def __init__(self, host, side, mutant, blocks):
        self.host, self.side, self.mutant, self.blocks = host, side, mutant, blocks
        self.dst = np.repeat(np.arange(host.n), np.diff(host.in_rp.astype(np.int64)))
        self.src = np.asarray(host.in_ci[:host.m], dtype=np.int64)
        if side is not None:
            s = side
            e = np.arange(s.m)
            self.keep = np.ones(s.m, dtype=bool)
            if mutant == "later_group":
                self.keep = e // GROUP == s.first[s.row_of_edge] // GROUP
            elif mutant == "later_chunk":
                self.keep = e // CHUNK == s.first_chunk[s.row_of_edge]
            elif mutant == "startless_chunk":
                self.keep = s.group_starts.sum(axis=1)[e // CHUNK] > 0
            elif mutant == "ids_from_256_zero":
                self.keep = s.ci < HOT_LINES
            elif mutant == "ids_below_256_zero":
                self.keep = s.ci >= HOT_LINES
            self.stale = np.zeros(s.n_nz)    # what rows summed with atomics still hold from the sweep before
            self.pending = np.zeros(s.n_nz)  # sums that a block's edge pass added to rows outside the block

    def sums(self, P, b):
        n = self.host.n
        if self.side is None:
            return np.bincount(self.dst, weights=P[self.src], minlength=n)
        s = self.side
        val = P[s.new2old][s.ci]
        acc = np.bincount(s.row_of_edge, weights=np.where(self.keep, val, 0.0), minlength=s.n_nz)
        if self.mutant == "pad_gathers":
            acc[-1] += s.pad * P[s.new2old[0]]
        j_lo, j_hi, e_lo, e_hi = self.blocks[b]
        if self.mutant == "cross_rows_not_cleared":
            acc[j_lo:j_hi] += np.where(s.cross[j_lo:j_hi], self.stale[j_lo:j_hi], 0.0)
            self.stale[j_lo:j_hi] = acc[j_lo:j_hi]
        if self.mutant == "shared_chunk_outside_block" and e_hi > e_lo:
            acc[j_lo:j_hi] += self.pending[j_lo:j_hi]
            self.pending[j_lo:j_hi] = 0.0
            c_lo, c_hi = e_lo // CHUNK * CHUNK, min((e_hi + CHUNK - 1) // CHUNK * CHUNK, s.m)
            out = np.r_[c_lo:e_lo, e_hi:c_hi]
            extra = np.bincount(s.row_of_edge[out], weights=val[out], minlength=s.n_nz)
            self.pending += np.where(s.cross, extra, 0.0)  # plain stores are overwritten, atomic sums stay
        full = np.zeros(n)
        full[s.new2old[s.rows]] = acc
        return full


def push_fwd(host, src, alpha, rmax, B=1, side=None, mutant=None, max_levels=400, gather=None):
    """Frontier-synchronous forward push from src where every level is a dense pull: Jacobi (B = 1), or the twin's
    block sweeps (B > 1: the first in the entry state, the others in place; needs the forward side for its blocks).
    A mutant may never come to rest (mass that is counted twice grows): the push stops after max_levels.
    gather: an object whose sums(P, b) gives the row sums of block pass b over original ids, in place of the plain
    gathers (tests/sweep1_designs.py: the layout models of the single-query sweep).
    Returns (reserve, residue, levels, dead-end pops)."""
    n = host.n
    dout = np.diff(host.out_rp.astype(np.int64))
    reserve, residue = np.zeros(n), np.zeros(n)
    if dout[src] == 0:
        reserve[src] = 1.0
        return reserve, residue, 0, 0
    if B > 1 or mutant is not None:
        assert side is not None
    blocks = side.blocks(B) if side is not None else [(0, 0, 0, 0)]
    if side is not None:
        orig = side.new2old[side.rows]
        members = [orig[j_lo:j_hi] for j_lo, j_hi, _, _ in blocks]
        rest = np.setdiff1d(np.arange(n), orig)  # rows without in-edges go with the last block
        if mutant in ("last_tile_skipped", "last_tile_z_rows_skipped"):
            nz_j, z_j = side.tile_rows(side.n_tiles - 1)
            skip = side.new2old[side.z_rows[z_j]]
            if mutant == "last_tile_skipped":
                skip = np.concatenate([skip, orig[nz_j]])
            members = [np.setdiff1d(mb, skip) for mb in members]
            rest = np.setdiff1d(rest, skip)
        members[-1] = np.concatenate([members[-1], rest])
    else:
        members = [np.arange(n)]
    if gather is None:
        gather = _Gather(host, side, mutant, blocks)
    reserve[src] = alpha
    P = np.zeros(n)
    P[src] = (1.0 - alpha) / dout[src]
    dead, nf, levels, dead_pops = 0.0, 1, 0, 0
    while nf and levels < max_levels:
        state = "J" if B == 1 else ("E" if levels == 0 else "G")
        Q = np.zeros(n)
        dead_next, nf = 0.0, 0
        for b, rows in enumerate(members):
            a = gather.sums(P, b)[rows]
            if dead > 0.0 and np.any(rows == src):
                a[rows == src] += dead
                dead = 0.0
            d, old = dout[rows], residue[rows]
            nw = old + a
            join = (a > 0.0) & ~_active(old, d, rmax) & _active(nw, d, rmax)
            residue[rows] = np.where(join, 0.0, nw)
            reserve[rows] += np.where(join, nw * alpha, 0.0)
            gone = join & (d == 0)
            dead_next += float(np.sum(nw[gone] * (1.0 - alpha)))
            dead_pops += int(gone.sum())
            cn = np.where(join & (d > 0), ((1.0 - alpha) * nw) / np.maximum(d, 1), 0.0)
            Q[rows] = cn
            if state == "E":
                P[rows] += cn
            elif state == "G":
                P[rows] = cn
            nf += int(join.sum())
        dead += dead_next
        P = Q
        levels += 1
    return reserve, residue, levels, dead_pops


def push_bwd(host, target, alpha, rmax):
    """Frontier-synchronous backward push from target (Backward_Search in pull form): every level each row sums
    (1 - alpha) * residue over its out-neighbours in the frontier and takes the sum divided by its out-degree; strict
    threshold.  Returns (reserve, residue, levels)."""
    n = host.n
    dout = np.diff(host.out_rp.astype(np.int64))
    din = np.diff(host.in_rp.astype(np.int64))
    reserve, residue = np.zeros(n), np.zeros(n)
    if din[target] == 0:
        reserve[target] = 1.0
        return reserve, residue, 0
    row = np.repeat(np.arange(n), dout)
    col = np.asarray(host.out_ci[:host.m], dtype=np.int64)
    residue[target] = 1.0
    front = np.array([target])
    levels = 0
    while front.size:
        c = np.zeros(n)
        c[front] = (1.0 - alpha) * residue[front]
        reserve[front] += residue[front] * alpha
        residue[front] = 0.0
        acc = np.bincount(row, weights=c[col], minlength=n)
        nw = residue + acc / np.maximum(dout, 1)
        front = np.flatnonzero((acc > 0.0) & ~(residue > rmax) & (nw > rmax))
        residue = nw
        levels += 1
    return reserve, residue, levels
