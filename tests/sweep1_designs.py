"""Designed graphs, layout inspectors, a numpy reference and layout models (with mutants) for the dense level of a
single query (csrc/kernels_dense.hip): k_dense_edges<HOT, SLICED> over the row-major and the sliced copy of the in-CSR,
k_dense_edges_panel + k_panel_fold + k_dense_apply<.., true> over the row-panel copy.

The internal order is fixed (lift.cpp: nodes with in-edges first, by out-degree descending, ties by id; a row's in-edges
keep their order), so a graph can put a row, a segment or a panel at every position these kernels treat differently:

  hot     16 600 rows with in-edges (n_hot = 16 384): one lane's eight gathers are the internal ids 16 380 .. 16 387,
          queries start at 16 383 and 16 384; the same graph under PPRHIP_RELABEL=0 runs the HOT = false kernels
  sliced  1 280 rows, six slices of 512 source ids (sixteen at the cap when 64 are asked for): S1-S11
  panels  57 544 rows in eight panels of 3, 33, 16, 5, 1, 4, 1 and 17 parts, the last of 200 rows: P1-P9

Rows are fed from a pool of nodes without in-edges (as tests/batch_sweep_designs.py does): a row with feed f takes
in-edges from pool[0 .. f), so a query from pool[i] puts its one non-zero contribution on a known edge of known rows.
Behind the feed a row takes the relationships of the ring (row j points to dout[j] rows picked by affine maps), so every
push runs for many levels.  hot_features, sliced_features, panel_features and the *_block_features name every property;
tests/test_sweep1_designs.py asserts each on the inspector's output.

The reference is batch_sweep_designs.push_fwd (frontier-synchronous, float64, original ids, no layout in it) with plain
CSR gathers (CsrGather), and power_iteration.  RowMajorModel, SlicedModel and PanelModel compute a block pass's row
sums from the inspected arrays the way the kernels read them - windows, flags, seg_row, items, parts, folds - and
MUTANTS change one reading each; MUTANT_CASES names the design, the gs_blocks and the queries that expose each.

Two of the panel mutants need a word.  Inside k_dense_edges_panel the bounds r_lo and r_hi only save work: a row's parts
are read by the block that owns the row, right behind that block's own edge pass, so parts written for rows of another
block are overwritten before anybody reads them.  What the bounds stand for is that a block runs the items of a panel it
owns only a piece of; r_lo_ignored / r_hi_ignored are therefore the launches that leave out the panel a block begins /
ends inside (the rows keep the parts of the sweep before).

Not covered at these sizes: the second trip of k_dense_edges' persistent loop (more chunks than 16 x the workgroups
of the launch) and the second deal of the panel kernel's item queue (more items than 2 x the CU count, about 16 M
edges); tests/test_gpu_scale.py serves both."""
import functools

import numpy as np

from batch_sweep_designs import fora_rmax, inspect_forward, push_fwd  # noqa: F401  (re-exported for the tests)

CHUNK = 512        # in-edges a wave of k_dense_edges owns
HOT = 16384        # contributions the LDS table of k_dense_edges<true, ..> holds
PANEL = 8192       # rows of a panel
STEP = 8192        # edges a workgroup of the panel kernel takes per turn
ITEM_EDGES = 32768  # a panel with more edges is cut into parts of about this many
FOLD_PARTS = 32
FOLD_MIN = 16
NO_FOLD = 0xffffffff
MAX_WINDOWS = 16
BLOCK_ROWS = 256

ALPHA = 0.15
EPS = 0.5

# the switches of each layout, set before the handle (or the host lift) is made
LAYOUT_ENV = {
    "rowmajor": {"PPRHIP_SLICED": "0"},
    "norelabel": {"PPRHIP_RELABEL": "0", "PPRHIP_SLICED": "0"},
    "sliced": {"PPRHIP_SLICE_IDS": "512"},
    "sliced16": {"PPRHIP_SLICE_IDS": "64"},
    "panel": {"PPRHIP_SWEEP1_PANELS": "1"},
}


def _ints(a):
    return [int(x) for x in a]


# ------------------------------------------------------------------ inspectors
def _start_bits(flags, m):
    return np.unpackbits(np.asarray(flags, dtype=np.uint8), bitorder="little")[:m].astype(bool)


class RowMajor:
    """The row-major copy as k_dense_edges<HOT, false> reads it: in_ci, a start flag per edge, the starts before every
    chunk; n_hot ids in the LDS table."""

    def __init__(self, L, n, m, relabeled=True):
        self.n, self.m = int(n), int(m)
        self.ci = np.asarray(L["in_ci"][:m], dtype=np.int64)
        self.start = _start_bits(L["flags"], m)
        self.chunk_starts = np.asarray(L["chunk_starts"], dtype=np.int64)
        self.row_of_edge = np.cumsum(self.start) - 1   # ordinal = (starts at or before the edge) - 1
        self.n_nz = int(L["nz_rows"].size)
        self.n_hot = min(self.n, HOT) if relabeled else 0
        self.new2old = np.asarray(L["new2old"], dtype=np.int64)
        self.nz_rows = np.asarray(L["nz_rows"], dtype=np.int64)


class Sliced:
    """The sliced copy: sl_ci / sl_flags / sl_chunk_starts, the row ordinal and first edge of every segment, the edge
    and segment base of every slice."""

    def __init__(self, L, n, m):
        self.n, self.m = int(n), int(m)
        self.S = int(L["edge_base"].size) - 1
        self.edge_base = np.asarray(L["edge_base"], dtype=np.int64)
        self.seg_base = np.asarray(L["seg_base"], dtype=np.int64)
        self.seg_row = np.asarray(L["seg_row"], dtype=np.int64)
        self.seg_off = np.asarray(L["seg_off"], dtype=np.int64)
        self.n_seg = self.seg_row.size
        self.ci = np.asarray(L["sl_ci"][:m], dtype=np.int64)
        self.start = _start_bits(L["sl_flags"], m)
        self.chunk_starts = np.asarray(L["sl_chunk_starts"], dtype=np.int64)
        self.n_chunks = (self.m + CHUNK - 1) // CHUNK
        self.seg_of_edge = np.cumsum(self.start) - 1
        self.seg_end = np.append(self.seg_off[1:], self.m)
        self.seg_slice = np.searchsorted(self.seg_base, np.arange(self.n_seg), side="right") - 1
        self.n_nz = int(L["nz_rows"].size)
        self.new2old = np.asarray(L["new2old"], dtype=np.int64)
        self.nz_rows = np.asarray(L["nz_rows"], dtype=np.int64)
        dout = np.diff(np.asarray(L["out_rp"], dtype=np.int64))
        self.n_src = int(np.flatnonzero(dout > 0).max()) + 1
        self.width = -(-self.n_src // self.S) if self.S else 0  # (the width at the cap; the asked one otherwise)

    def ranges(self, block, clamp=True):
        """Per slice, the edges of the block's rows in it: [(slice, e_lo, e_hi)], empty ones included
        (levels.cpp: sliced_windows_of before it joins)."""
        j_lo, j_hi = block[0], block[1]
        out = []
        for q in range(self.S):
            lo, hi = int(self.seg_base[q]), int(self.seg_base[q + 1])
            g_lo = lo + int(np.searchsorted(self.seg_row[lo:hi], j_lo, side="left"))
            g_hi = lo + int(np.searchsorted(self.seg_row[lo:hi], j_hi, side="left"))

            def edge(g):
                if g < hi:
                    return int(self.seg_off[g])
                if clamp:
                    return int(self.edge_base[q + 1])
                return int(self.seg_off[g]) if g < self.n_seg else 0  # (no clamp: the next slice's first segment)
            out.append((q, edge(g_lo), edge(g_hi)))
        return out

    def windows(self, block, mutant=None):
        """The block's windows [(e_lo, e_hi)], neighbouring ranges joined."""
        W = []
        for q, e_lo, e_hi in self.ranges(block, clamp=mutant != "last_slice_clamp_missing"):
            if e_hi <= e_lo:
                continue
            if W and W[-1][1] == e_lo:
                if mutant != "joined_window_gap":   # (the mutant joins and forgets to move the end)
                    W[-1][1] = e_hi
            else:
                W.append([e_lo, e_hi])
        return [tuple(w) for w in W]


class Panels:
    """The row-panel copy: items (edge0, steps, panel, part0), panels (base, parts, rows, fold), the item range of every
    panel, and per stored slot the source and the panel-local row (0xffff = padding)."""

    def __init__(self, L, n, m):
        self.n, self.m = int(n), int(m)
        self.n_panels, self.n_items, self.n_part, self.n_slots = (int(x) for x in L["panel_sizes"])
        self.items = np.asarray(L["panel_items"], dtype=np.int64).reshape(-1, 4)
        self.desc = np.asarray(L["panel_desc"], dtype=np.int64).reshape(-1, 4)
        self.item0 = np.asarray(L["panel_item0"], dtype=np.int64)
        self.src = np.asarray(L["panel_src"], dtype=np.int64)
        self.rloc = np.asarray(L["panel_row"], dtype=np.int64)
        self.n_nz = int(L["nz_rows"].size)
        self.new2old = np.asarray(L["new2old"], dtype=np.int64)
        self.nz_rows = np.asarray(L["nz_rows"], dtype=np.int64)
        self.parts, self.rows, self.fold = self.desc[:, 1], self.desc[:, 2], self.desc[:, 3]
        self.folded = self.fold != NO_FOLD
        steps = self.items[:, 1]
        self.slot_item = np.repeat(np.arange(self.n_items), steps * STEP)
        self.slot_turn = (np.arange(self.n_slots) - (self.items[:, 0] * STEP)[self.slot_item]) // STEP
        self.pad = self.rloc == 0xffff
        self.item_edges = np.bincount(self.slot_item, weights=~self.pad, minlength=self.n_items).astype(np.int64)
        self.slot_lo = self.items[:, 0] * STEP                     # first slot of every item
        self.panel_slot0 = np.append(self.slot_lo[self.item0[:-1]], self.n_slots)

    def cut(self, block):
        """(p_lo, p_hi) of the block's launch and, per panel of it, (r_lo, r_hi)."""
        j_lo, j_hi = block[0], block[1]
        p_lo, p_hi = j_lo // PANEL, min(self.n_panels, (j_hi + PANEL - 1) // PANEL)
        r = {}
        for p in range(p_lo, p_hi):
            row0 = p * PANEL
            r[p] = (max(j_lo - row0, 0), min(min(j_hi, self.n_nz) - row0, PANEL) if j_hi > row0 else 0)
        return p_lo, p_hi, r


def lift_of(pkg, host, layout, monkeypatch):
    """pkg.lift_host under the layout's switches."""
    for k, v in LAYOUT_ENV[layout].items():
        monkeypatch.setenv(k, v)
    try:
        return pkg.lift_host(host)
    finally:
        for k in LAYOUT_ENV[layout]:
            monkeypatch.delenv(k)


def inspect(L, host, layout):
    if layout in ("rowmajor", "norelabel"):
        return RowMajor(L, host.n, host.m, relabeled=layout == "rowmajor")
    if layout in ("sliced", "sliced16"):
        return Sliced(L, host.n, host.m)
    return Panels(L, host.n, host.m)


# ------------------------------------------------------------------ features, by name
def hot_features(rm, host):
    """H1, H2 on the row-major copy: name -> the rows (ordinals) / sources (original ids) that carry it."""
    f = {}
    h = rm.n_hot
    want = np.arange(h - 4, h + 4)
    e0 = np.arange(0, rm.m - 7, 8)
    win = rm.ci[e0[:, None] + np.arange(8)]
    ok = np.all(win == want, axis=1) & (rm.row_of_edge[e0] == rm.row_of_edge[e0 + 7])
    f["H1_one_lane_gathers_ids_16380_to_16387"] = _ints(rm.row_of_edge[e0[ok]])
    dout = np.diff(host.out_rp.astype(np.int64))
    for v in (h - 1, h):
        o = int(rm.new2old[v]) if v < rm.n else -1
        f["H2_source_with_internal_id_%d" % v] = [o] if o >= 0 and dout[o] > 0 else []
    gathered = np.zeros(rm.n, dtype=bool)
    gathered[rm.ci] = True
    f["H2_ids_16383_and_16384_are_gathered"] = [h - 1, h] if gathered[h - 1] and gathered[h] else []
    return f


def sliced_features(sl):
    """S1-S5, S10, S11 and the cap on the sliced copy: name -> rows (ordinals), segments or chunks."""
    f = {}
    per_row = np.zeros((sl.n_nz, sl.S), dtype=bool)
    per_row[sl.seg_row, sl.seg_slice] = True
    count = per_row.sum(axis=1)
    f["S1_row_with_a_segment_in_every_slice"] = _ints(np.flatnonzero(count == sl.S))
    f["S2_row_in_first_and_last_slice_only"] = _ints(np.flatnonzero((count == 2) & per_row[:, 0] & per_row[:, -1]))
    f["S3_segment_starts_on_lane_0_bit_0"] = _ints(np.flatnonzero(sl.seg_off % CHUNK == 0))
    f["S3_segment_starts_on_lane_0_bit_0_behind_chunk_0"] = _ints(
        np.flatnonzero((sl.seg_off % CHUNK == 0) & (sl.seg_off > 0)))
    whole = sl.seg_end // CHUNK - (sl.seg_off + CHUNK - 1) // CHUNK
    f["S4_segment_spans_two_whole_chunks"] = _ints(np.flatnonzero(whole >= 2))
    per_chunk = np.diff(sl.chunk_starts[:sl.n_chunks + 1])
    f["S4_chunk_without_start_flag"] = _ints(np.flatnonzero(per_chunk[:sl.m // CHUNK] == 0))
    f["S5_segment_ends_on_chunk_last_edge"] = _ints(np.flatnonzero((sl.seg_end % CHUNK == 0) & (sl.seg_end < sl.m)))
    f["S10_ids_above_the_last_source_are_never_gathered"] = [sl.n_src] if sl.n_src < sl.n else []
    f["S11_last_chunk_partly_filled"] = [sl.n_chunks - 1] if sl.m % CHUNK else []
    return f


def sliced_block_features(sl, blocks):
    """S6-S9 for one cut into blocks: name -> (block, slice) pairs or blocks."""
    f = {"S6_window_begins_and_ends_mid_chunk": [], "S7_two_windows_share_a_chunk": [],
         "S8_neighbouring_ranges_joined": [], "S9_slice_without_edge_of_the_block": []}
    for b, blk in enumerate(blocks):
        if blk[0] == blk[1]:
            continue
        ranges = sl.ranges(blk)
        W = sl.windows(blk)
        for q, e_lo, e_hi in ranges:
            if e_hi <= e_lo:
                f["S9_slice_without_edge_of_the_block"].append((b, q))
        for e_lo, e_hi in W:
            if e_lo % CHUNK and e_hi % CHUNK and e_hi < sl.m:
                f["S6_window_begins_and_ends_mid_chunk"].append((b, e_lo, e_hi))
        for (_, h0), (l1, _) in zip(W[:-1], W[1:]):
            if (h0 - 1) // CHUNK == l1 // CHUNK:
                f["S7_two_windows_share_a_chunk"].append((b, h0, l1))
        if len(W) < sum(1 for _, e_lo, e_hi in ranges if e_hi > e_lo):
            f["S8_neighbouring_ranges_joined"].append(b)
        assert len(W) <= MAX_WINDOWS
    return f


def panel_features(pn, L):
    """P1-P4, P7, P9 on the row-panel copy: name -> panels, items or rows (ordinals)."""
    f = {}
    for s in (1, 3, 4, 5, 16, 17, 32, 33):
        f["P1_panel_of_%d_parts" % s] = _ints(np.flatnonzero(pn.parts == s))
    last = pn.n_panels - 1
    f["P2_last_panel_short"] = [last] if pn.rows[last] < PANEL else []
    f["P2_last_panel_under_256_rows_and_folded"] = [last] if pn.rows[last] < 256 and pn.folded[last] else []
    f["P3_item_last_turn_is_padding"] = _ints(np.flatnonzero(pn.item_edges % STEP != 0))
    f["P3_item_edges_exact_multiple_of_8192"] = _ints(np.flatnonzero(pn.item_edges % STEP == 0))
    f["P4_item_of_1_turn"] = _ints(np.flatnonzero(pn.items[:, 1] == 1))
    f["P4_item_of_2_turns"] = _ints(np.flatnonzero(pn.items[:, 1] == 2))
    f["P4_item_of_3_or_more_turns"] = _ints(np.flatnonzero(pn.items[:, 1] >= 3))
    ok = ~pn.pad
    j = pn.items[:, 2][pn.slot_item[ok]] * PANEL + pn.rloc[ok]
    k = pn.slot_item[ok] - pn.item0[pn.items[:, 2][pn.slot_item[ok]]]
    pairs = np.unique(j * 64 + k)
    in_parts = np.bincount(pairs // 64, minlength=pn.n_nz)
    parts_of_row = pn.parts[np.arange(pn.n_nz) // PANEL]
    f["P7_row_with_in_edges_in_every_part"] = _ints(np.flatnonzero((in_parts == parts_of_row) & (parts_of_row >= 16)))
    f["P7_row_with_in_edges_in_one_part"] = _ints(np.flatnonzero((in_parts == 1) & (parts_of_row >= 16)))
    in_rp, in_ci = np.asarray(L["in_rp"], dtype=np.int64), np.asarray(L["in_ci"], dtype=np.int64)
    row = np.repeat(np.arange(pn.n), np.diff(in_rp))
    f["P9_self_loop_in_a_panel_row"] = _ints(np.unique(row[in_ci[:pn.m] == row]))
    key = np.sort(row * pn.n + in_ci[:pn.m])
    f["P9_parallel_relationships_in_a_panel_row"] = _ints(np.unique(key[1:][key[1:] == key[:-1]] // pn.n))
    return f


def panel_block_features(pn, blocks):
    """P5, P6 for one cut into blocks: name -> (block, panel) pairs or blocks."""
    f = {"P5_bound_cuts_a_folded_panel": [], "P5_bound_cuts_an_unfolded_panel": [],
         "P6_range_starts_unfolded_and_holds_a_folded_panel": []}
    for b, blk in enumerate(blocks):
        if blk[0] == blk[1]:
            continue
        p_lo, p_hi, r = pn.cut(blk)
        for p, (r_lo, r_hi) in r.items():
            if r_lo > 0 or r_hi < pn.rows[p]:
                f["P5_bound_cuts_a_folded_panel" if pn.folded[p] else "P5_bound_cuts_an_unfolded_panel"].append((b, p))
        if not pn.folded[p_lo] and pn.folded[p_lo + 1:p_hi].any():
            f["P6_range_starts_unfolded_and_holds_a_folded_panel"].append(b)
    return f


# ------------------------------------------------------------------ designs
class Design:
    def __init__(self, name, n, src, dst, names, sources, one_level, layouts, gs_blocks, block_sources=None):
        self.name, self.n, self.names = name, int(n), names
        self.block_sources = list(sources if block_sources is None else block_sources)  # the queries at gs_blocks > 1
        self.src, self.dst = np.asarray(src, dtype=np.int32), np.asarray(dst, dtype=np.int32)
        self.sources, self.one_level, self.layouts, self.gs_blocks = sources, one_level, layouts, gs_blocks

    def host(self, pkg):
        return pkg.HostCsr(self.n, self.src, self.dst)


_MULT = (3, 5, 7, 11, 13, 17, 19, 23)
_ADD = (1, 2, 3, 5, 7, 11, 13, 17)


def _ring(dout, targets):
    """The i-th ring relationship of every row with dout > i goes to targets[(mult_i * rank + add_i) % len(targets)],
    rank = the row's place among those rows.  Returns (src, dst)."""
    T = np.asarray(targets, dtype=np.int64)
    src, dst = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for i in range(int(dout.max())):
        rows = np.flatnonzero(dout > i)
        src.append(rows)
        dst.append(T[(_MULT[i] * np.arange(rows.size) + _ADD[i]) % T.size])
    return np.concatenate(src), np.concatenate(dst)


def _feeds(pool0, feed):
    """Row j takes in-edges from pool[0 .. feed[j]), rows in order."""
    feed = np.asarray(feed, dtype=np.int64)
    total = int(feed.sum())
    first = np.repeat(np.cumsum(feed) - feed, feed)
    return pool0 + np.arange(total) - first, np.repeat(np.arange(feed.size), feed)


def _assemble(R, dout, fixed, ring_targets, feed_of, ranges=()):
    """Edge list of a design: the fixed relationships first, then the feeds (pool = ids from R), then the ring, so a
    row's in-edges lie in that order.  dout[j] is the out-degree row j ends with (the fixed relationships count);
    feed_of(k) gives the feed of every row from its in-edges so far; ranges = extra (row, first pool index, count)."""
    fixed = np.asarray(fixed, dtype=np.int64).reshape(-1, 2)
    f_out = np.bincount(fixed[:, 0][fixed[:, 0] < R], minlength=R)
    assert np.all(dout - f_out >= 0)
    r_src, r_dst = _ring(dout - f_out, ring_targets)
    k = np.bincount(r_dst, minlength=R) + np.bincount(fixed[:, 1], minlength=R)[:R]
    feed = np.asarray(feed_of(k), dtype=np.int64)
    p_src, p_dst = _feeds(R, feed)
    x_src = [np.arange(R + a, R + a + c) for _, a, c in ranges]
    x_dst = [np.full(c, j) for j, _, c in ranges]
    src = np.concatenate([fixed[:, 0], p_src] + x_src + [r_src])
    dst = np.concatenate([fixed[:, 1], p_dst] + x_dst + [r_dst])
    return src, dst, feed, k


def hot_design():
    """16 600 rows with in-edges in id order: 16 380 of out-degree 2, then 212 of out-degree 1 - the first eight of
    them, the internal ids 16 380 .. 16 387, point to row X = 3 and nowhere else - then 8 dead ends.  Rows 0, 1, 2 take
    8 in-edges from the pool, so X starts at edge 24 and its first eight in-edges are lane 3's share of chunk 0; four
    pool edges follow.  Row 4 takes 600 pool edges (it crosses a chunk boundary), every other row one and its ring
    relationships.  Behind the rows: the pool of 600, a node z without in-edges that points to a dead end, an isolated
    node."""
    R, POOL, X = 16600, 600, 3
    h = HOT
    dout = np.full(R, 2, dtype=np.int64)
    dout[h - 4:R - 8] = 1
    dout[R - 8:] = 0
    dead = list(range(R - 8, R))
    fixed = [(h - 4 + i, X) for i in range(8)] + [(100 + i, d) for i, d in enumerate(dead)]
    z = R + POOL
    fixed.append((z, dead[0]))
    targets = np.arange(4, R - 8)

    def feed_of(k):
        f = np.ones(R, dtype=np.int64)
        f[:3] = 8
        f[X] = 4
        f[4] = 600
        f[R - 8:] = 0
        return f
    src, dst, feed, k = _assemble(R, dout, fixed, targets, feed_of)
    pool = list(range(R, R + POOL))
    n = z + 2
    names = dict(X=X, pool=pool, dead=dead, z=z, isolated=n - 1, lo=h - 1, hi=h)
    # pool[0] feeds every row; pool[3] X's tail behind the eight; pool[599] row 4 alone; the table's two sides; X
    sources = [pool[0], pool[3], pool[599], h - 1, h, h - 4, h + 3, X, 0, z, dead[0], n - 1]
    one_level = [pool[0], pool[3], pool[7], pool[599], h - 1, h, h - 4, h + 3, X]
    return Design("hot", n, src, dst, names, sources, one_level, ("rowmajor", "norelabel"), (1,))


def sliced_design():
    """1 280 rows with in-edges in id order (1 252 of out-degree 3, 20 of 1, 8 dead ends), a pool of 1 400, z, an
    isolated node; slices of 512 internal ids: rows [0, 512), rows [512, 1 024), rows from 1 024 with pool[0 .. 256),
    pool[256 .. 768), pool[768 .. 1 280), pool[1 280 .. 1 400) with z.
      A = 10    the whole pool and relationships from rows 5 and 600: a segment in every slice; its 120 edges of the last
                slice end on a chunk's last edge (F's feed is chosen for that), so the segment behind starts on lane 0
      L = 20    relationships from rows 7 and 9 and pool[1 290 .. 1 350): first and last slice only; L2 = 1 150 likewise
      D = 40    pool[0 .. 1 280) and pool[768 .. 1 280) twice more: parallel relationships, a segment of 1 536 edges
      T = 1 000 pool[0 .. 300): 44 edges in pool[256 .. 768) behind everything block 0 has there
      F = 50    the filler; rows 30 .. 33 keep the pool's out-degrees falling where D's and L's extra feeds begin
    The other rows take 8 (the first 256) or 12 pool edges and their ring relationships."""
    R, POOL = 1280, 1400
    A, Lr, L2, Dr, T, F = 10, 20, 1150, 40, 1000, 50
    dout = np.full(R, 3, dtype=np.int64)
    dout[R - 28:R - 8] = 1
    dout[R - 8:] = 0
    dead = list(range(R - 8, R))
    z = R + POOL
    fixed = [(5, A), (600, A), (7, Lr), (9, Lr), (8, L2), (11, L2)] + [(60 + i, d) for i, d in enumerate(dead)]
    fixed.append((z, dead[0]))
    targets = np.setdiff1d(np.arange(R - 8), [Lr, L2])
    ranges = [(Lr, 1290, 60), (L2, 1290, 60), (Dr, 768, 512), (Dr, 768, 512)]

    def feed_of(k, x=0):
        f = np.full(R, 12, dtype=np.int64)
        f[:256] = 8
        f[A] = POOL
        f[[Lr, L2]] = 0
        f[Dr] = 1280
        f[T] = 300
        f[[30, 31]] = 1290
        f[[32, 33]] = 768
        f[F] = 300 + x
        f[R - 8:] = 0
        return f
    src, dst, feed, k = _assemble(R, dout, fixed, targets, feed_of, ranges)
    # the last slice holds pool[1280 ..) and z: A's 120 edges come first; they must end on a chunk's last edge
    e5 = int(np.sum(src >= R + 1280))
    x = (-(src.size - e5 + 120)) % CHUNK
    src, dst, feed, k = _assemble(R, dout, fixed, targets, lambda kk: feed_of(kk, x), ranges)
    pool = list(range(R, R + POOL))
    n = z + 2
    names = dict(A=A, L=Lr, L2=L2, D=Dr, T=T, F=F, pool=pool, dead=dead, z=z, isolated=n - 1)
    sources = [pool[0], pool[10], pool[299], pool[800], pool[1285], pool[1399], 5, 600, z, dead[0], n - 1]
    one_level = [pool[0], pool[10], pool[299], pool[300], pool[800], pool[1285], pool[1300], pool[1399], 5, 600, 7]
    return Design("sliced", n, src, dst, names, sources, one_level, ("sliced", "sliced16", "rowmajor", "panel"),
                  (1, 2, 3))


PANEL_EDGES = (73000, 1048600, 524288, 140000, 8192, 100000, 12000, 524300)  # 3, 33, 16, 5, 1, 4, 1, 17 parts


def panels_design():
    """57 544 rows with in-edges in id order: seven panels of 8 192 rows with out-degrees 8, 7, 6, 5, 4, 3, 2 and a last
    panel of 200 rows (190 of out-degree 1, 10 dead ends).  The panels hold PANEL_EDGES in-edges, that is 3, 33, 16, 5,
    1, 4, 1 and 17 parts: the first panel is not folded and the second is; the 16 parts of the third are 32 768 edges
    each (four whole turns), the fifth has one in-edge per row (one whole turn), the seventh 12 000 (two turns, the
    second padded); the last panel is short and folded.  A panel's rows share its feed evenly, so pool[i] feeds whole
    panels and the last pool node of a panel's feed lies in its last part.  Row X1 (panel 1) takes the whole pool,
    relationships from rows 10, 20 000, 40 000 and 50 000 and two from row 30; row SL (panel 1) points to itself.
    Panels 4 and 6 are fed from the pool alone; the dead ends are reached from rows 40 .. 49.  m is about 2.43 M."""
    full = 7
    R = full * PANEL + 200
    POOL = 2800
    dout = np.repeat(np.array([8, 7, 6, 5, 4, 3, 2, 1]), PANEL)[:R].copy()
    dout[R - 10:] = 0
    dead = list(range(R - 10, R))
    X1, SL = PANEL + 100, PANEL + 200
    z = R + POOL
    fixed = [(10, X1), (20000, X1), (40000, X1), (50000, X1), (30, X1), (30, X1), (SL, SL)]
    fixed += [(40 + i, d) for i, d in enumerate(dead)] + [(z, dead[0])]
    panel_of = np.arange(R) // PANEL
    targets = np.flatnonzero(np.isin(panel_of, (0, 1, 2, 3, 5, 7)) & (np.arange(R) < R - 10))

    def feed_of(k):
        f = np.zeros(R, dtype=np.int64)
        for p, e in enumerate(PANEL_EDGES):
            rows = np.flatnonzero((panel_of == p) & (np.arange(R) < R - 10) & (np.arange(R) != X1))
            left = e - int(k[panel_of == p].sum()) - (POOL if p == 1 else 0)
            base, rem = divmod(left, rows.size)
            assert base >= 1 or (base == 0 and p == 0), (p, left)
            f[rows] = base
            f[rows[:rem]] += 1
        f[X1] = POOL
        return f
    src, dst, feed, k = _assemble(R, dout, fixed, targets, feed_of)
    assert feed.max() == POOL and np.sort(feed)[-2] < POOL - 20
    pool = list(range(R, R + POOL))
    n = z + 2
    last = [int(feed[(panel_of == p) & (np.arange(R) != X1)].max()) - 1 for p in range(len(PANEL_EDGES))]
    names = dict(X1=X1, SL=SL, pool=pool, dead=dead, z=z, isolated=n - 1, last_feed=last)
    # pool[0] feeds every row; the last pool node of the feeds of panels 2 (16 parts), 1 (33) and 7 (17): their last
    # parts; pool[-1] X1 alone; row 30 (parallel relationships); SL; z; a dead end; the isolated node
    sources = [pool[0], pool[last[2]], pool[last[1]], pool[last[7]], pool[POOL - 1], 30, SL, z, dead[0], n - 1]
    one_level = [pool[0], pool[1], pool[last[2]], pool[last[1]], pool[last[1] // 2], pool[last[7]], pool[last[7] // 2],
                 pool[POOL - 1], 30, SL, 20000]
    return Design("panels", n, src, dst, names, sources, one_level, ("panel",), (1, 2, 3, 6),
                  block_sources=[pool[0], pool[last[1]], z])


@functools.lru_cache(maxsize=None)
def all_designs():
    return {d.name: d for d in (hot_design(), sliced_design(), panels_design())}


# ------------------------------------------------------------------ numpy reference
class CsrGather:
    """Row sums of one block pass by plain gathers over the host in-CSR (original ids, no layout).  With blocks whose
    rows are runs of original ids (the designs': rows with in-edges are numbered in sweep order) a pass gathers the
    block's in-edges only; the sums are the same, the zeros are not computed."""

    def __init__(self, host, side=None, B=1):
        self.n = host.n
        self.rp = host.in_rp.astype(np.int64)
        self.dst = np.repeat(np.arange(host.n), np.diff(self.rp))
        self.src = np.asarray(host.in_ci[:host.m], dtype=np.int64)
        self.span = None
        if B > 1:
            orig = side.new2old[side.rows]
            self.span = []
            for j_lo, j_hi, _, _ in side.blocks(B):
                ids = orig[j_lo:j_hi]
                assert ids.size == 0 or np.array_equal(ids, np.arange(ids[0], ids[0] + ids.size))
                self.span.append((int(self.rp[ids[0]]), int(self.rp[ids[-1] + 1])) if ids.size else (0, 0))

    def sums(self, P, b):
        lo, hi = self.span[b] if self.span else (0, self.src.size)
        return np.bincount(self.dst[lo:hi], weights=P[self.src[lo:hi]], minlength=self.n)


def reference_push(host, s, alpha, rmax, B=1, side=None, max_levels=400):
    """(reserve, residue, levels, dead-end pops) of the frontier-synchronous push, every level a sweep of B blocks."""
    return push_fwd(host, s, alpha, rmax, B=B, side=side, gather=CsrGather(host, side, B), max_levels=max_levels)


def one_level_rmax(host, s, alpha=ALPHA):
    """A threshold under which the source pushes and nobody else does: halfway between the largest residue per
    out-degree the first level of the reference leaves and the source's own 1 / d.  None when there is no such value (a
    dead end receives mass, or a receiver outweighs the source)."""
    dout = np.diff(host.out_rp.astype(np.int64))
    if dout[s] == 0:
        return None
    top = 1.0 / dout[s]
    _, r, _, _ = reference_push(host, s, alpha, top, max_levels=1)
    if np.any((r > 0.0) & (dout == 0)):
        return None
    ratio = float(np.max(r / np.maximum(dout, 1)))
    return 0.5 * (ratio + top) if ratio < top else None


def one_level_expected(host, s, alpha=ALPHA):
    """(reserve, residue) after the source's push alone: the contribution c added once per relationship from the source
    (c, c + c, ...), alpha at the source; every sum has equal addends, so there is one float64 answer."""
    n = host.n
    lo, hi = int(host.out_rp[s]), int(host.out_rp[s + 1])
    c = ((1.0 - alpha) * 1.0) / float(hi - lo)
    mult = np.bincount(np.asarray(host.out_ci[lo:hi], dtype=np.int64), minlength=n)
    r = np.zeros(n)
    for t in range(int(mult.max())):
        r[mult > t] += c
    p = np.zeros(n)
    p[s] = 1.0 * alpha
    return p, r


def power_iteration(host, s, alpha, iters):
    """The power method (Power_Method.java) in numpy: iters Jacobi steps from residue 1 at s; dead-end mass returns to
    s."""
    n = host.n
    dout = np.diff(host.out_rp.astype(np.int64))
    dst = np.repeat(np.arange(n), np.diff(host.in_rp.astype(np.int64)))
    src = np.asarray(host.in_ci[:host.m], dtype=np.int64)
    cur, reserve = np.zeros(n), np.zeros(n)
    cur[s] = 1.0
    for _ in range(iters):
        reserve += cur * alpha
        remain = cur * (1.0 - alpha)
        nxt = np.bincount(dst, weights=(remain / np.maximum(dout, 1))[src], minlength=n)
        nxt[s] += float(remain[dout == 0].sum())
        cur = nxt
    return reserve


# ------------------------------------------------------------------ layout models and mutants
MUTANTS = {
    "hot": ("hot_bound_off_by_one_low", "hot_bound_off_by_one_high", "cold_reads_zero"),
    "sliced": ("seg_row_shifted", "lane0_start_dropped", "startless_chunk_dropped", "window_head_unmasked",
               "window_tail_unmasked", "shared_chunk_once", "joined_window_gap", "last_slice_clamp_missing"),
    "panel": ("pad_row_counted", "r_lo_ignored", "r_hi_ignored", "last_part_dropped", "fold_group_short",
              "fold_tail_zero_missing", "unfolded_tail_dropped", "rows_stride_full", "third_turn_stale"),
}


class RowMajorModel:
    """k_dense_edges<HOT, false>: a lane's gather comes from the table below n_hot and from memory from n_hot on; an
    edge adds to the row its start flags count to."""

    def __init__(self, rm, blocks, mutant=None):
        self.L, self.blocks, self.mutant = rm, blocks, mutant

    def block_sums(self, c, b):
        rm, h = self.L, self.L.n_hot
        v = c[rm.ci]
        if self.mutant == "hot_bound_off_by_one_low":     # the table is filled below n_hot - 1, read below n_hot
            v = np.where(rm.ci == h - 1, 0.0, v)
        elif self.mutant == "hot_bound_off_by_one_high":  # filled below n_hot, read up to n_hot
            v = np.where(rm.ci == h, 0.0, v)
        elif self.mutant == "cold_reads_zero":
            v = np.where(rm.ci >= h, 0.0, v)
        _, _, e_lo, e_hi = self.blocks[b]
        return np.bincount(rm.row_of_edge[e_lo:e_hi], weights=v[e_lo:e_hi], minlength=rm.n_nz)


class SlicedModel:
    """k_dense_edges<.., true>: per window of the block its chunks, the edges outside the window counted as zero, a
    segment's sum added to acc[seg_row[segment]]; the apply pass reads and clears the rows of the block."""

    def __init__(self, sl, blocks, mutant=None):
        self.L, self.blocks, self.mutant = sl, blocks, mutant
        self.acc = np.zeros(sl.n_nz)
        self.wins = [sl.windows(blk, mutant) for blk in blocks]
        seg = sl.seg_of_edge.copy()
        if mutant == "lane0_start_dropped":   # a segment that starts on a chunk's first edge runs on as the one before
            first = np.flatnonzero((sl.seg_off % CHUNK == 0) & (sl.seg_off > 0))
            drop = np.isin(seg, first)
            seg[drop] -= 1
        if mutant == "seg_row_shifted":
            seg = np.minimum(seg + 1, sl.n_seg - 1)
        self.row_of_edge = sl.seg_row[seg]
        per_chunk = np.diff(sl.chunk_starts[:sl.n_chunks + 1])
        self.chunk_live = per_chunk > 0 if mutant == "startless_chunk_dropped" else np.ones(sl.n_chunks, dtype=bool)

    def block_sums(self, c, b):
        sl, m = self.L, self.L.m
        seen = set()
        for e_lo, e_hi in self.wins[b]:
            lo, hi = e_lo // CHUNK * CHUNK, min((e_hi + CHUNK - 1) // CHUNK * CHUNK, m)
            e = np.arange(lo, hi)
            keep = self.chunk_live[e // CHUNK].copy()
            if self.mutant != "window_head_unmasked":
                keep &= e >= e_lo
            if self.mutant != "window_tail_unmasked":
                keep &= e < e_hi
            if self.mutant == "shared_chunk_once":   # a chunk two windows share is summed for the first only
                keep &= ~np.isin(e // CHUNK, list(seen))
                seen.update(range(lo // CHUNK, (hi + CHUNK - 1) // CHUNK))
            e = e[keep]
            self.acc += np.bincount(self.row_of_edge[e], weights=c[sl.ci[e]], minlength=sl.n_nz)
        j_lo, j_hi = self.blocks[b][0], self.blocks[b][1]
        out = np.zeros(sl.n_nz)
        out[j_lo:j_hi] = self.acc[j_lo:j_hi]
        self.acc[j_lo:j_hi] = 0.0
        return out


class PanelModel:
    """k_dense_edges_panel, k_panel_fold and the row sum of k_dense_apply<.., true> over a buffer of parts that lives
    as long as the model (stale parts stay): an item stores the sums of the block's rows at part0 + row, a folded panel's
    parts are added 32 at a time, a row adds its parts (or its fold sums) four at a time and then one by one."""

    def __init__(self, pn, blocks, mutant=None):
        self.L, self.blocks, self.mutant = pn, blocks, mutant
        self.part = np.zeros(pn.n_part + (FOLD_PARTS + 1) * PANEL)  # (room for the reads of the mutants)
        self.src, self.rloc, self.plans = pn.src, pn.rloc, {}
        if mutant == "third_turn_stale":   # from the third turn on a turn reads the indices of the turn before
            late = np.flatnonzero(pn.slot_turn >= 2)
            self.src, self.rloc = pn.src.copy(), pn.rloc.copy()
            self.src[late], self.rloc[late] = pn.src[late - STEP], pn.rloc[late - STEP]

    def _plan(self, b, p, bounds):
        """Of panel p in block pass b: the first part entry, the entries of all parts, and per kept slot (an edge of a
        row of the block) its entry relative to the first and its source.  Made once per model."""
        if (b, p) not in self.plans:
            pn = self.L
            r_lo, r_hi = bounds
            s0, s1 = int(pn.panel_slot0[p]), int(pn.panel_slot0[p + 1])
            item, r, u = pn.slot_item[s0:s1], self.rloc[s0:s1], self.src[s0:s1]
            if self.mutant == "pad_row_counted":   # the padding (source 0, row 0xffff) taken for the panel's last row
                r = np.where(r == 0xffff, pn.rows[p] - 1, r)
            keep = (r >= r_lo) & (r < r_hi)
            first = int(pn.desc[p, 0])
            idx = pn.items[:, 3][item[keep]] + r[keep] - first
            self.plans[(b, p)] = (first, int(pn.parts[p] * pn.rows[p]), idx, u[keep])
        return self.plans[(b, p)]

    def block_sums(self, c, b):
        pn, mt = self.L, self.mutant
        p_lo, p_hi, cut = pn.cut(self.blocks[b])
        j_lo, j_hi = self.blocks[b][0], min(self.blocks[b][1], pn.n_nz)
        run = list(range(p_lo, p_hi))
        if mt == "r_lo_ignored" and run and cut[p_lo][0] > 0:
            run = run[1:]
        if mt == "r_hi_ignored" and run and cut[run[-1]][1] < pn.rows[run[-1]] and j_hi < pn.n_nz:
            run = run[:-1]
        for p in run:
            first, size, idx, u = self._plan(b, p, cut[p])
            sums = np.bincount(idx, weights=c[u], minlength=size)
            r_lo, r_hi = cut[p]
            for k in range(int(pn.parts[p])):   # every item stores the block's rows, zeros included
                self.part[first + k * pn.rows[p] + r_lo:first + k * pn.rows[p] + r_hi] = \
                    sums[k * pn.rows[p] + r_lo:k * pn.rows[p] + r_hi]
        out = np.zeros(pn.n_nz)
        for p in range(p_lo, p_hi):
            r_lo, r_hi = cut[p]
            if r_hi <= r_lo:
                continue
            base, parts, rows, fold = (int(x) for x in pn.desc[p])
            stride = PANEL if mt == "rows_stride_full" else rows
            r = np.arange(r_lo, r_hi)
            n_parts = parts - 1 if mt == "last_part_dropped" and parts > 1 else parts
            if pn.folded[p]:
                groups = (parts + FOLD_PARTS - 1) // FOLD_PARTS
                for g in range(groups):
                    k0 = g * FOLD_PARTS
                    k1 = min(n_parts, k0 + FOLD_PARTS)
                    if k0 >= parts:
                        continue
                    v = np.zeros(r.size)
                    for k in range(k0, k0 + FOLD_PARTS if mt == "fold_tail_zero_missing" else k1):
                        v = v + self.part[base + k * stride + r]
                    self.part[fold + g * rows + r] = v
                first, cnt = fold, groups
                if mt == "fold_group_short":
                    cnt = max(1, parts // FOLD_PARTS)
            else:
                first, cnt = base, n_parts
                if mt == "unfolded_tail_dropped":
                    cnt = cnt // 4 * 4
            acc = np.zeros(r.size)
            for k in range(cnt):
                acc = acc + self.part[first + k * stride + r]
            out[p * PANEL + r] = acc
        return out


MODEL_OF = {"rowmajor": RowMajorModel, "norelabel": RowMajorModel, "sliced": SlicedModel, "sliced16": SlicedModel,
            "panel": PanelModel}


def row_sums(model, c, b=0):
    """The row sums (by row ordinal) block pass b of the layout model gives for the contributions c (internal ids)."""
    return model.block_sums(np.asarray(c, dtype=np.float64), b)


class LayoutGather:
    """push_fwd's gather through a layout model: contributions to internal ids, row sums back to original ids."""

    def __init__(self, model):
        self.model = model
        L = model.L
        self.new2old, self.orig_rows, self.n = L.new2old, L.new2old[L.nz_rows], L.n

    def sums(self, P, b):
        acc = self.model.block_sums(P[self.new2old], b)
        full = np.zeros(self.n)
        full[self.orig_rows] = acc
        return full


def layout_push(host, layout, insp, side, s, alpha, rmax, B=1, mutant=None, max_levels=400):
    """reference_push with the row sums of the layout's model (and one wrong reading of it)."""
    model = MODEL_OF[layout](insp, side.blocks(B), mutant)
    return push_fwd(host, s, alpha, rmax, B=B, side=side, gather=LayoutGather(model), max_levels=max_levels)


# mutant -> (design, layout, gs_blocks, indices into the design's sources: the queries that expose it); the GPU tests run
# every source of a design at every gs_blocks the design names, so each of these is one of their queries
MUTANT_CASES = {
    "hot_bound_off_by_one_low": ("hot", "rowmajor", 1, (3,)),    # the source with internal id 16 383
    "hot_bound_off_by_one_high": ("hot", "rowmajor", 1, (4,)),   # ... 16 384
    "cold_reads_zero": ("hot", "rowmajor", 1, (0,)),             # a pool node: every pool id is above the table
    "seg_row_shifted": ("sliced", "sliced", 1, (5,)),
    "lane0_start_dropped": ("sliced", "sliced", 1, (4,)),        # pool[1285]: the segments of the last slice
    "startless_chunk_dropped": ("sliced", "sliced", 1, (3,)),    # pool[800]: the middle of D's 1 536 edges
    "window_head_unmasked": ("sliced", "sliced", 2, (0,)),
    "window_tail_unmasked": ("sliced", "sliced", 3, (0,)),
    "shared_chunk_once": ("sliced", "sliced", 2, (3,)),
    "joined_window_gap": ("sliced", "sliced", 1, (5,)),
    "last_slice_clamp_missing": ("sliced", "sliced", 1, (4,)),
    "pad_row_counted": ("panels", "panel", 1, (0,)),
    "r_lo_ignored": ("panels", "panel", 3, (0,)),
    "r_hi_ignored": ("panels", "panel", 3, (0,)),
    "last_part_dropped": ("panels", "panel", 1, (2,)),           # the last pool node of panel 1's feed: part 32
    "fold_group_short": ("panels", "panel", 1, (2,)),
    "fold_tail_zero_missing": ("panels", "panel", 1, (0,)),
    "unfolded_tail_dropped": ("panels", "panel", 1, (0,)),
    "rows_stride_full": ("panels", "panel", 1, (2,)),
    "third_turn_stale": ("panels", "panel", 1, (0,)),
}

# FORA top-k: design -> (index into the design's sources, k).  The hot design's rows are so alike that most of its
# answers hold exact ties; these are cases whose k + 1 largest values differ by 1e-11 or more on the twin
# (tests/test_sweep1_designs.py checks it), so the order of the ids is decided
TOPK_CASES = {"hot": [(0, 10), (3, 2)], "sliced": [(0, 10), (1, 10)], "panels": [(0, 10), (1, 10)]}
TOPK_GAP = 1e-11


# ------------------------------------------------------------------ shared, computed once per session
_laid, _refs = {}, {}


def laid(pkg, name, layout, monkeypatch):
    """(host, lift arrays, forward side, inspected layout) of a design under a layout's switches."""
    key = (pkg.__name__, name, layout)
    if key not in _laid:
        host = host_of(pkg, name)
        L = lift_of(pkg, host, layout, monkeypatch)
        _laid[key] = (host, L, inspect_forward(pkg, host, L), inspect(L, host, layout))
    return _laid[key]


def host_of(pkg, name):
    key = (pkg.__name__, name)
    if key not in _laid:
        _laid[key] = all_designs()[name].host(pkg)
    return _laid[key]


def reference(pkg, name, s, B=1, alpha=ALPHA, side=None):
    """reference_push of a design's source at the design's FORA threshold, kept for the tests that share it (the
    arrays are not to be written to)."""
    key = (name, s, B, alpha)
    if key not in _refs:
        host = host_of(pkg, name)
        _refs[key] = reference_push(host, s, alpha, fora_rmax(pkg, host, alpha), B=B, side=side)
    return _refs[key]
