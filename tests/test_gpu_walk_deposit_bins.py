"""Walk deposits, the two binning passes (kernels_walk.hip: dep_move, k_dep_bin, k_dep_tile).

A record reaches its tile's run through the run of its coarse bin (PPRHIP_WALK_DEPOSIT_BIN consecutive tiles, hooks
library only): k_dep_bin sorts a workgroup's share of the records into the bins' runs, k_dep_tile sorts a unit (bin, slice
of the bin's run) into the bin's tile runs, and k_dep_sum reads those.  The tests use the designed sink graphs of
tests/test_gpu_walk_deposit.py (4 096 nodes, ids kept, tile 64: 64 tiles) and put the terminals where a bin begins,
ends, is empty, is short or takes everything.  Every case is compared with PPRHIP_WALK_DEPOSIT=atomic on the same
handle within TOL_MC, with np.add.at over the walks' terminals within walks * 2^-52 of the deposited mass, and by its
usage counters: records = walks (or the capacity), items = what the tile and slice rule gives."""
import numpy as np
import pytest

import test_gpu_walk_deposit as base
from test_gpu_walk_deposit import N, TILE, SinkGraph, build_graph, deposit_info, deposit_usage, designs_of
from walk_plans import TOL_MC

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]
SWITCHES = base.SWITCHES + ("PPRHIP_WALK_DEPOSIT_BIN",)
QUERIES = 40   # per call, as the issue of this file asks (the cache, and with it the records, engage from 32 on)
BIN_IDS = 4 * TILE   # ids of a bin of 4 tiles


@pytest.fixture
def switch(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_(mode=None, tile=None, slice_=None, cap=None, min_walks=None, bin_=None):
        for k, v in zip(SWITCHES, (mode, tile, slice_, cap, min_walks, bin_)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))

    return set_


class Case:
    """A sink graph with one carrier (and seed) per (sink, count) pair, and `n_sets` designs over it: design j sends the
    counts, rotated by j places, to the same sinks."""

    def __init__(self, orc, sinks, counts, n_sets=1):
        from conftest import load_hooks_pkg
        self.pkg = load_hooks_pkg()
        S = len(sinks)
        assert S == len(counts) and S % 2 == 0
        taken = set(int(s) for s in sinks)
        free = [v for v in range(70, N) if v not in taken and v % TILE not in (0, TILE - 1)]
        carriers = np.array(free[:n_sets * S])
        seeds = np.array(free[n_sets * S:2 * n_sets * S])
        all_sinks = np.concatenate([np.roll(np.asarray(sinks), j) for j in range(n_sets)])
        self.G = SinkGraph(self.pkg, carriers, all_sinks, seeds)
        self.g = build_graph(self.pkg, self.G.host)
        self.designs = designs_of(orc, self.G, counts, [carriers[j * S:(j + 1) * S] for j in range(n_sets)])
        self.sinks = [np.roll(np.asarray(sinks), j) for j in range(n_sets)]

    def close(self):
        self.g.close()

    def tile_counts(self, j=0, cap=None):
        """records per tile of one phase of design j: walk i of the plan is carrier order (ascending ids), and walks
        [0, cap) are recorded"""
        d = self.designs[j]
        term = np.repeat(self.sinks[j], d.counts)[:cap]
        return np.bincount(term // TILE, minlength=N // TILE)

    def run(self, switch, order, bin_, slice_=None, cap=None, what=""):
        """the call under PPRHIP_WALK_DEPOSIT=atomic, then binned; (binned vectors, usage of the binned call)"""
        pkg, g = self.pkg, self.g
        switch(mode="atomic")
        out_a, pq_a = base.run_designs(pkg, g, order)
        assert not deposit_info(pkg, g)["on"] and deposit_usage(pkg, g) == (0, 0, 0, 0)
        switch(tile=TILE, slice_=slice_, cap=cap, min_walks=0, bin_=bin_)
        out_b, pq_b = base.run_designs(pkg, g, order)
        info = deposit_info(pkg, g)
        usage = deposit_usage(pkg, g)
        print("%s: %s; items %d phases %d records %d beyond %d" % ((what, info) + usage))
        assert info["on"] and info["tile"] == TILE and info["n_tiles"] == N // TILE
        worst = 0.0
        for i in range(len(order)):
            assert pq_a[i].walks == pq_b[i].walks == order[i].plan.total, i
            err = float(np.max(np.abs(out_a[i] - out_b[i])))
            worst = max(worst, err)
            assert err <= TOL_MC, "%s query %d: binned and atomic vectors differ by %.3e" % (what, i, err)
        print("%s: max |binned - atomic| = %.3e" % (what, worst))
        base.check_designs(g, order, out_b, pq_b, what)
        return out_b, usage


def expect_usage(case, order_js, slice_, cap=None):
    """(items of the last phase, phases, records, walks beyond the capacity) of a call whose queries are designs order_js"""
    records = beyond = 0
    for j in order_js:
        total = case.designs[j].plan.total
        rec = total if cap is None else min(total, cap)
        records += rec
        beyond += total - rec
    cnt = case.tile_counts(order_js[-1], cap)
    items = int(np.sum(-(-cnt // slice_)))
    return items, len(order_js), records, beyond


# ------------------------------------------------------------------ 1. bin edges, 5. the degenerate ends, 7. a second call
EDGE_SINKS = sorted(set([0, N - 1] + [k * BIN_IDS - 1 for k in range(1, 16)] + [k * BIN_IDS for k in range(1, 16)]))
EDGE_COUNTS = [65, 1, 64, 2, 63, 129, 3, 300, 17, 16, 15, 1, 128, 33, 700, 2] * 2


@pytest.fixture(scope="module")
def edges(orc):
    assert len(EDGE_SINKS) == 32
    c = Case(orc, EDGE_SINKS, EDGE_COUNTS, n_sets=2)
    yield c
    c.close()


@pytest.mark.parametrize("bin_", [4, 1, 64])
def test_bin_edges(edges, switch, bin_):
    """terminals on the first and last id of every bin of 4 tiles: both sides of every bin boundary; the same records
    with a bin per tile and with one bin of all tiles"""
    a, b = edges.designs
    js = [0, 1] * (QUERIES // 2)
    out, usage = edges.run(switch, [edges.designs[j] for j in js], bin_, what="bin edges, bin %d" % bin_)
    assert usage == expect_usage(edges, js, base.deposit_info(edges.pkg, edges.g)["slice"])
    for s in EDGE_SINKS:
        assert out[0][s] > 0.0 and out[1][s] > 0.0


def test_second_call(edges, switch):
    """a second and a third call on the same handle, of other queries: cursors, counts and tables start afresh"""
    for n, js in enumerate(([0] * QUERIES, [1] * QUERIES, [1, 0] * (QUERIES // 2))):
        _, usage = edges.run(switch, [edges.designs[j] for j in js], 4, slice_=64, what="call %d" % n)
        assert usage == expect_usage(edges, js, 64)


# ------------------------------------------------------------------ 2. an empty bin between two, 4. a short last bin
@pytest.fixture(scope="module")
def gaps(orc):
    # bins of 4 tiles: records in bins 2 and 4, none in bin 3 or anywhere else; bins of 5: 12 whole bins and tiles 60-63
    sinks = [2 * BIN_IDS + 88, 3 * BIN_IDS - 1, 4 * BIN_IDS, 4 * BIN_IDS + 76, 60 * TILE - 1, 60 * TILE, N - 1, 0]
    c = Case(orc, sinks, [500, 3, 1, 700, 64, 65, 300, 2])
    yield c
    c.close()


def test_empty_bin(gaps, switch):
    """bins of 4 tiles: records in bins 2 and 4 (and 14, 15, 0), none in bins 1, 3 and 5"""
    js = [0] * QUERIES
    out, usage = gaps.run(switch, [gaps.designs[0]] * QUERIES, 4, what="empty bins")
    assert usage == expect_usage(gaps, js, 16384)
    cnt = gaps.tile_counts()
    per_bin = cnt.reshape(-1, 4).sum(axis=1)
    assert per_bin[2] > 0 and per_bin[3] == 0 and per_bin[4] > 0 and per_bin[1] == 0 and per_bin[5] == 0


def test_short_last_bin(gaps, switch):
    """64 tiles = 12 bins of 5 and one of 4: terminals on both sides of tile 60 and on the last id"""
    js = [0] * QUERIES
    out, usage = gaps.run(switch, [gaps.designs[0]] * QUERIES, 5, what="bin 5")
    assert usage == expect_usage(gaps, js, 16384)
    assert out[0][N - 1] > 0.0 and out[0][60 * TILE] > 0.0 and out[0][60 * TILE - 1] > 0.0


# ------------------------------------------------------------------ 3. one bin takes everything, 6. capacity
SLICE = 16
# bin 2 of 8 tiles (tiles 16-23): a hot tile of two sinks, runs of slice, slice + 1, slice - 1 and 1, 2 * slice + 1, 2
ONE_SINKS = [16 * TILE, 17 * TILE - 1, 17 * TILE + 5, 18 * TILE + 6, 19 * TILE + 7, 20 * TILE + 8, 21 * TILE, 24 * TILE - 1]
ONE_COUNTS = [600, 400, SLICE, SLICE + 1, SLICE - 1, 1, 2 * SLICE + 1, 2]


@pytest.fixture(scope="module")
def one_bin(orc):
    c = Case(orc, ONE_SINKS, ONE_COUNTS)
    yield c
    c.close()


def test_one_bin(one_bin, switch):
    """every record in one bin: 68 units of the second pass, 63 items on the hot tile"""
    js = [0] * QUERIES
    out, usage = one_bin.run(switch, [one_bin.designs[0]] * QUERIES, 8, slice_=SLICE, what="one bin")
    cnt = one_bin.tile_counts()
    assert [int(x) for x in cnt[16:24]] == [1000, SLICE, SLICE + 1, SLICE - 1, 1, 2 * SLICE + 1, 0, 2] and cnt.sum() == sum(ONE_COUNTS)
    assert usage == expect_usage(one_bin, js, SLICE) and usage[0] == 63 + 1 + 2 + 1 + 1 + 3 + 1


@pytest.mark.parametrize("cap", [1, 700, 1040])
def test_capacity_in_bin(one_bin, switch, cap):
    """the capacity cuts the records inside the bin (behind the first record, inside the hot tile, inside the run of
    slice - 1): walks [cap, total) of every phase add atomically"""
    js = [0] * QUERIES
    assert cap < sum(ONE_COUNTS)
    _, usage = one_bin.run(switch, [one_bin.designs[0]] * QUERIES, 8, slice_=SLICE, cap=cap, what="capacity %d" % cap)
    assert usage == expect_usage(one_bin, js, SLICE, cap)
    assert usage[2] == QUERIES * cap and usage[3] == QUERIES * (sum(ONE_COUNTS) - cap)
