"""The designs of tests/sweep_cut_designs.py on the CPU: the mirrored tile constant against the header, slot_layout
against brute force, and every claimed layout feature on the oracle twin's vector (the GPU test proves them again on the
device's vector).  Family A: the twin's push of the sinks runs no level and returns the normalized weights bit for bit,
and cut == vol.  Family B: the padded graph's vector is the unpadded graph's, bit for bit under one level schedule."""
import os
import re

import numpy as np
import pytest

import sweep_cut_designs as D
from conftest import HOOKS_LIB, PKG_NAME, ROOT

T = D.SWEEP_TILE


def test_tile_constant_mirrors_the_header():
    text = open(os.path.join(ROOT, PKG_NAME, "csrc", "engine.hpp")).read()
    m = re.search(r"constexpr\s+uint32_t\s+kSweepTile\s*=\s*(\d+)\s*;", text)
    assert m and int(m.group(1)) == D.SWEEP_TILE
    kern = open(os.path.join(ROOT, PKG_NAME, "csrc", "kernels_sweep.hip")).read()
    assert "kSweepPerThread = (int)(kSweepTile / 256u)" in kern and "__launch_bounds__(256) void k_sweep_edges" in kern
    assert D.SWEEP_THREADS == 256 and T % D.SWEEP_THREADS == 0


def test_grid_switches_exist_in_the_hooks_library_only():
    """The two switches are read through hook_env (nullptr in the product): their names are in libpprhip_hooks.so and
    not in libpprhip.so."""
    kern = open(os.path.join(ROOT, PKG_NAME, "csrc", "kernels_sweep.hip")).read()
    assert "hook_env(name)" in kern and "getenv" not in kern
    product = open(os.path.join(ROOT, PKG_NAME, "libpprhip.so"), "rb").read()
    hooks = open(HOOKS_LIB, "rb").read()
    for name in (b"PPRHIP_SWEEP_EDGE_GRID", b"PPRHIP_SWEEP_ITEM_GRID"):
        assert name in hooks and name not in product, name
        assert name.decode() in kern


# ------------------------------------------------------------------ slot_layout against brute force
def brute_layout(order, d_out, d_in, tile):
    """Slot by slot: who owns it, and whether it is the first slot of its node / of its node's in-row."""
    owner, first, split = [], [], []
    for p, v in enumerate(order):
        for k in range(int(d_out[v] + d_in[v])):
            owner.append(p)
            first.append(k == 0)
            split.append(k == d_out[v])
    out = []
    for t0 in range(0, len(owner), tile):
        own = owner[t0:t0 + tile]
        out.append(dict(first=own[0], count=own[-1] - own[0] + 1, first_crosses=not first[t0],
                        last_crosses=t0 + tile < len(owner) and owner[t0 + tile] == own[-1] and not first[t0 + tile],
                        starts={owner[s]: s - t0 for s in range(t0, t0 + len(own)) if first[s]},
                        splits={owner[s]: s - t0 for s in range(t0, t0 + len(own)) if split[s]}, slots=len(own)))
    return out


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 7, 8, 16])
def test_slot_layout_against_brute_force(tile):
    rng = np.random.default_rng(tile)
    for trial in range(60):
        n = int(rng.integers(1, 14))
        d_out = rng.integers(0, 2 * tile + 3, n)
        d_in = rng.integers(0, 4, n) * rng.integers(0, 2, n)
        ids = np.nonzero(d_out + d_in > 0)[0]
        if ids.size == 0:
            continue
        order = rng.permutation(ids)[:int(rng.integers(1, ids.size + 1))]
        got = D.slot_layout(order, d_out, d_in, tile)
        want = brute_layout(order, d_out, d_in, tile)
        assert len(got) == len(want)
        for L, W in zip(got, want):
            assert (L.first, L.count, L.first_crosses, L.last_crosses, L.slots) == \
                   (W["first"], W["count"], W["first_crosses"], W["last_crosses"], W["slots"]), (trial, L.t)
            assert L.starts.size == L.splits.size == L.count
            assert L.starts[0] <= 0                       # the kernel's s_start[0] is 0 whatever the first node's start
            for j in range(L.count):
                p = L.first + j
                v = order[p]
                assert (0 <= L.starts[j] < L.slots) == (p in W["starts"]) and W["starts"].get(p, L.starts[j]) == L.starts[j]
                if d_in[v] and 0 <= L.splits[j] < L.slots:
                    assert W["splits"][p] == L.splits[j]
                else:
                    assert p not in W["splits"]
                assert L.splits[j] - L.starts[j] == d_out[v]
        pos, inrow = D.slot_nodes(order, d_out, d_in)
        assert pos.size == sum(W["slots"] for W in want) and inrow.sum() == d_in[order].sum()


def test_slot_layout_on_a_written_sequence():
    """Design a_aligned's sequence at a tile of 8 (T -> 8: a hub of three tiles, a tile of single slots, nodes that start
    and end on, one before and one behind a boundary), every tile worked out by hand."""
    degs = [24] + [1] * 8 + [7, 1, 1, 9, 7] + [2] * 10 + [1]
    n = len(degs)
    tiles = D.slot_layout(np.arange(n), np.zeros(n, dtype=int), np.array(degs), 8)
    assert [(L.first, L.count, L.first_crosses, L.last_crosses) for L in tiles] == \
        [(0, 1, False, True), (0, 1, True, True), (0, 1, True, False), (1, 8, False, False), (9, 2, False, False),
         (11, 2, False, True), (12, 2, True, True), (13, 5, True, True), (17, 5, True, True), (21, 4, True, False)]
    assert list(tiles[5].starts) == [0, 1] and list(tiles[6].starts) == [-7, 2] and tiles[9].slots == 6


# ------------------------------------------------------------------ the designs on the twin's vector
@pytest.fixture(scope="module")
def views(orc):
    """(design name, normalize) -> View on the twin's vector, computed once."""
    cache = {}

    def get(d, normalize):
        key = (d.name, bool(normalize))
        if key not in cache:
            cache[key] = d.prove(D.twin_vector(orc, d, normalize), normalize)
        return cache[key]
    return get


@pytest.mark.parametrize("name", D.NAMES)
def test_claimed_features_on_the_twin(views, name):
    d = D.design(name)
    for normalize in d.normalizes:
        V = views(d, normalize)
        assert d.n % 256 != 0
        assert V.total <= 110000 and d.n <= 14000, (V.total, d.n)
        print("%s normalize %d: n %d, %d profiled, %d slots in %d tiles" % (d, normalize, d.n, V.order.size, V.total,
                                                                            len(V.tiles)))


def test_every_feature_is_claimed():
    ALL = D.all_designs()
    assert {f for d in ALL for f in d.claims} == set(D.FEATURES)
    for normalize in (True, False):   # families A and C claim theirs under both values, family B under each in some design
        assert {f for d in ALL if normalize in d.normalizes for f in d.claims} == set(D.FEATURES)
    assert {f[0] for f in D.FEATURES} == set("ABC")


@pytest.mark.parametrize("name", D.NAMES_A)
def test_sinks_keep_their_weights_and_cut_is_vol(orc, views, name):
    d = D.design(name)
    for normalize in (True, False):
        V = views(d, normalize)
        w = d.weights(normalize)
        p = np.zeros(d.n)
        p[d.seeds] = w / w.sum()
        assert np.array_equal(V.x, p), d                       # no level ran: the reserve is the normalized weights
        assert np.array_equal(V.ref["cut"], V.ref["vol"])      # every slot names an unranked source
        assert V.ref["support"] == d.seeds.size
        if d.name != "a_denormal":
            assert np.array_equal(V.order, d.seeds) and np.array_equal(V.deg, d.degs)   # the written permutation
            assert V.ref["best_size"] == 1                     # phi is 1 up to half the volume: the shortest prefix


@pytest.mark.parametrize("name", D.NAMES_B)
def test_feeders_change_no_push(orc, views, name):
    """Under one level schedule (every level sparse) the padded graph's vector is the unpadded graph's bit for bit.  The
    library's schedule turns a level into a sweep by the edge count, which the feeders raise: there the two pushes
    differ by their own error, each within rmax * sum of out-degrees of the exact vector."""
    d = D.design(name)
    V = views(d, d.normalizes[0])
    B = D.base()
    t = orc.tuning_default()
    t.dense_frac = 1e9
    orc.set_sync_tuning(t)
    try:
        plain = B.design("b_unpadded", np.zeros(B.n, dtype=np.int64), [], (True, False))
        assert np.array_equal(D.twin_vector(orc, d, True), D.twin_vector(orc, plain, True)), d
    finally:
        orc.set_sync_tuning(None)
    assert float(np.abs(V.x - D.base_vector()).max()) <= 2 * D.RMAX * d.m, d
    assert d.pad.sum() > 0 and V.x[list(B.feeders)].max() == 0.0 and np.all(d.d_in[list(B.feeders)] == 0)
    assert V.ref["support"] == B.n > 768 and len(V.tiles) >= 7
    # no dead ends among the ranked nodes; ranked-ranked relationships in and across tiles
    assert np.all(d.d_out[V.order] > 0)
    ra, rb = V.rank[d.src], V.rank[d.dst]
    both = (ra >= 0) & (rb >= 0) & (d.src != d.dst)
    ta, tb = V.volx[ra[both]] // T, V.volx[rb[both]] // T
    assert np.count_nonzero(ta == tb) > 100 and np.count_nonzero(ta != tb) > 100
    for kw in D.extra_sweeps(d, V):
        W = d.view(V.x, d.normalizes[0], **kw)
        assert 0 < W.ref["profiled"] <= V.ref["profiled"]
        if "max_size" in kw:   # a ranked neighbour beyond the cut is "none" in the profile
            out = (V.rank >= kw["max_size"])
            assert W.ref["profiled"] == kw["max_size"] and np.any(out[d.dst] & (W.rank[d.src] >= 0))
        else:
            assert W.ref["best_vol"] <= kw["max_vol"]
    bv = V.ref["best_vol"]
    assert d.view(V.x, d.normalizes[0], max_vol=bv).ref["best_size"] == V.ref["best_size"]
    assert d.view(V.x, d.normalizes[0], max_vol=bv - 1).ref["best_size"] != V.ref["best_size"]


def test_a_design_that_misses_fails():
    d = D.design("a_aligned")
    x = np.zeros(d.n)
    x[d.seeds] = 1.0           # a vector that orders the sinks by id: the written layout is gone
    with pytest.raises(AssertionError):
        d.prove(x, False)
