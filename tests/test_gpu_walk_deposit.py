"""Walk deposits by tile (engine.hpp: WalkDeposit; kernels_walk.hip "deposits by tile").

In a batched whole-graph FORA call that keeps the terminal cache, a walk phase of enough walks stores one record
(terminal, increment) per walk instead of adding at the terminal; the records are binned by tile of consecutive ids,
summed per tile in LDS and added to the vector in runs.  Terminals and increments are what they were; only the order of
the fp64 additions changes.  The tests run on libpprhip_hooks.so, where the switches exist:
PPRHIP_WALK_DEPOSIT=atomic (no records), PPRHIP_WALK_DEPOSIT_TILE / _SLICE / _CAP (a small tile, slice and capacity) and
PPRHIP_WALK_DEPOSIT_MIN (the walk count records start from; the product's is far above a test graph's phase).

The designed graphs are built with PPRHIP_RELABEL=0 (ids kept) and have 4 096 nodes, R-MAT 12's, so that a tile of 64
cuts them into 64 tiles: sinks (a self-loop each) where the terminals are wanted, carriers with one edge to a sink - every
walk of a carrier ends on its sink - and a seed node per carrier (tests/walk_plans.py: the one exact hop)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import walk_plans as wp
from walk_plans import ALPHA, TOL_MC, WALK_SEED

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]
EPS = 0.5
Q = 40       # queries per call: the cache, and with it the records, engage from 32 on
N = 4096
TILE = 64
SWITCHES = ("PPRHIP_WALK_DEPOSIT", "PPRHIP_WALK_DEPOSIT_TILE", "PPRHIP_WALK_DEPOSIT_SLICE", "PPRHIP_WALK_DEPOSIT_CAP",
            "PPRHIP_WALK_DEPOSIT_MIN")


# ------------------------------------------------------------------ hooks and switches
def hooks(pkg):
    L = pkg.lib()
    u64p, ip, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    L.pprhip_hook_walk_deposit_info.argtypes = [C.c_void_p, ip, ip, u64p, u32p, u32p, u32p, u64p]
    L.pprhip_hook_walk_deposit_usage.argtypes = [C.c_void_p, u64p, C.c_int]
    return L


def deposit_info(pkg, g):
    present, on, cap, nbytes = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64()
    tile, n_tiles, slc = C.c_uint32(), C.c_uint32(), C.c_uint32()
    pkg._check(hooks(pkg).pprhip_hook_walk_deposit_info(g.h, C.byref(present), C.byref(on), C.byref(cap), C.byref(tile),
                                                        C.byref(n_tiles), C.byref(slc), C.byref(nbytes)))
    return dict(present=bool(present.value), on=bool(on.value), cap=cap.value, tile=tile.value, n_tiles=n_tiles.value,
                slice=slc.value, bytes=nbytes.value)


def deposit_usage(pkg, g, reset=True):
    """(items of the last binned phase, binned phases, records, walks beyond the capacity) since the last reset"""
    u = (C.c_uint64 * 4)()
    pkg._check(hooks(pkg).pprhip_hook_walk_deposit_usage(g.h, u, int(reset)))
    return tuple(int(x) for x in u)


@pytest.fixture
def switch(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_(mode=None, tile=None, slice_=None, cap=None, min_walks=None):
        for k, v in zip(SWITCHES, (mode, tile, slice_, cap, min_walks)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))

    return set_


def build_graph(pkg, host):
    old = os.environ.get("PPRHIP_RELABEL")
    os.environ["PPRHIP_RELABEL"] = "0"
    try:
        return pkg.Graph(host)
    finally:
        if old is None:
            del os.environ["PPRHIP_RELABEL"]
        else:
            os.environ["PPRHIP_RELABEL"] = old


# ------------------------------------------------------------------ designed graphs
class SinkGraph:
    """N nodes: sink nodes with a self-loop, carrier i with its one edge to sinks[i], seed node i with its one edge to
    carrier i; everything else isolated.  What wp.Design reads of a plan graph."""

    def __init__(self, pkg, carriers, sinks, seeds):
        carriers, sinks, seeds = (np.asarray(x, dtype=np.int64) for x in (carriers, sinks, seeds))
        loops = np.unique(sinks)
        assert np.all(np.diff(carriers) > 0) and not set(carriers) & set(loops) and not set(seeds) & set(loops)
        assert not set(seeds) & set(carriers) and max(carriers.max(), seeds.max(), loops.max()) < N
        src = np.concatenate([loops, carriers, seeds]).astype(np.int32)
        dst = np.concatenate([loops, sinks, carriers]).astype(np.int32)
        self.n = N
        self.host = pkg.HostCsr(N, src, dst)
        self.deg = np.diff(self.host.out_rp.astype(np.int64))
        self.seed_of = np.full(N, -1, dtype=np.int64)
        self.seed_of[carriers] = seeds
        self.dead_seeds = np.zeros(0, dtype=np.int64)
        self.sink_of = dict(zip([int(c) for c in carriers], [int(s) for s in sinks]))


def expected_vector(g, D):
    """alpha * q_i on seed i, alpha * (1 - alpha) * q_i on carrier i, and np.add.at of every walk's increment at the
    terminal g.random_walks gives it; (vector, walks, deposited mass)."""
    starts = np.repeat(D.carriers, D.counts).astype(np.int32)
    idx = (np.arange(D.plan.total, dtype=np.int64) - np.repeat(D.woff, D.counts)).astype(np.uint64)
    term, _ = g.random_walks(starts, idx, ALPHA, seed=WALK_SEED, stream=0, no_zero_hop=True)
    assert np.array_equal(term, np.array([D.G.sink_of[int(s)] for s in starts]))   # the graph's design: carrier -> sink
    out = np.zeros(D.G.n)
    out[D.seed_nodes] += ALPHA * D.q
    out[D.carriers] += ALPHA * ((1.0 - ALPHA) * D.q)
    vals = np.repeat(D.inc, D.counts)
    np.add.at(out, term, vals)
    return out, D.plan.total, float(vals.sum())


def designs_of(orc, G, counts, carrier_sets):
    ds = [wp.Design(orc, G, wp.Plan("deposit-%d" % i, 12, counts, carriers=("ids", np.asarray(c))))
          for i, c in enumerate(carrier_sets)]
    lead = max(ds, key=lambda d: d.rmax0)
    for d in ds:
        if d is not lead:
            d.adopt(lead)
    return ds


def run_designs(pkg, g, order):
    a = order[0]
    g.set_tuning(pkg.tuning_batch())
    try:
        out, _, _, _, pq, _ = g.fora_batch_seeds([d.seeds for d in order], a.eps, ALPHA, seed=WALK_SEED,
                                                 weights=[d.weights for d in order], n_rounds=1,
                                                 conf=a.conf(pkg.ForaConf), fetch=True, per_query=True)
    finally:
        g.set_tuning(pkg.tuning_default())
    return out, pq


def check_designs(g, order, out, pq, what):
    """every vector within walks * 2^-52 of the deposited mass of np.add.at over its walks' terminals"""
    refs = {}
    worst = 0.0
    for i, d in enumerate(order):
        if id(d) not in refs:
            refs[id(d)] = expected_vector(g, d)
        ref, walks, mass = refs[id(d)]
        bound = walks * 2.0 ** -52 * mass
        err = float(np.max(np.abs(out[i] - ref)))
        worst = max(worst, err / bound)
        assert pq[i].walks == walks and pq[i].mc_sources == d.counts.size, (what, i)
        assert err <= bound, "%s query %d: max abs diff %.3e > walks * 2^-52 * mass = %.3e" % (what, i, err, bound)
        assert abs(float(out[i].sum()) - 1.0) <= TOL_MC
    print("%s: worst error %.3f of the bound" % (what, worst))


# ------------------------------------------------------------------ 1. binned against atomic
def live_sources(host, count, seed):
    live = np.nonzero(np.diff(host.out_rp) > 0)[0]
    rng = np.random.default_rng(seed)
    return [int(x) for x in live[rng.integers(0, live.size, count)]]


def batch(g, srcs, seed, k=8):
    return g.fora_batch_single_source(srcs, EPS, ALPHA, seed=seed, n_rounds=0, k=k, fetch=True, per_query=True)


@pytest.mark.parametrize("name,tile", [("got", None), ("rmat12", None), ("rmat12", TILE), ("rmat15", None)])
def test_binned_against_atomic(pkg, got, rmat12, rmat15, switch, name, tile):
    host = {"got": got, "rmat12": rmat12, "rmat15": rmat15}[name]
    srcs = live_sources(host, Q, seed=5)
    with pkg.Graph(host) as g:
        g.set_tuning(pkg.tuning_batch())
        switch(mode="atomic")
        out_a, ids_a, _, nsel_a, pq_a, _ = batch(g, srcs, seed=7)
        assert not deposit_info(pkg, g)["on"] and deposit_usage(pkg, g) == (0, 0, 0, 0)
        switch(tile=tile, min_walks=0)
        out_b, ids_b, _, nsel_b, pq_b, _ = batch(g, srcs, seed=7)
        info = deposit_info(pkg, g)
        items, phases, records, beyond = deposit_usage(pkg, g)
        walks = sum(int(x.walks) for x in pq_b)
        print("%s: %s; phases %d records %d beyond %d, %d walks" % (name, info, phases, records, beyond, walks))
        assert info["present"] and info["on"] and info["tile"] == (tile or 2048)
        assert info["n_tiles"] == -(-host.n // info["tile"])
        assert 0 < phases <= Q and records == walks and beyond == 0 and items > 0
        assert np.array_equal(nsel_a, nsel_b) and np.array_equal(ids_a, ids_b), "top-k id lists differ"
        worst = 0.0
        for i in range(Q):
            assert pq_a[i].walks == pq_b[i].walks and pq_a[i].walk_steps == pq_b[i].walk_steps, i
            assert pq_a[i].rounds == pq_b[i].rounds, i
            err = float(np.max(np.abs(out_a[i] - out_b[i])))
            worst = max(worst, err)
            assert err <= TOL_MC, "query %d: binned and atomic vectors differ by %.3e" % (i, err)
            assert abs(float(out_b[i].sum()) - 1.0) <= TOL_MC and abs(float(out_a[i].sum()) - 1.0) <= TOL_MC, i
        print("%s: max |binned - atomic| = %.3e" % (name, worst))


# ------------------------------------------------------------------ 2. tile edges
EDGE_SINKS = [TILE - 1, TILE, N - 1, 0, TILE - 1, TILE, 2047, 2048]
EDGE_COUNTS = [65, 64, 63, 129, 1, 2, 700, 300]


@pytest.fixture(scope="module")
def edge_graph(orc):
    from conftest import load_hooks_pkg
    pkg = load_hooks_pkg()
    S = len(EDGE_SINKS)
    # two carrier sets for one call: the second sends the same counts to the sinks in another order
    carriers = np.concatenate([128 + np.arange(S), 3000 + np.arange(S)])
    sinks = np.concatenate([EDGE_SINKS, EDGE_SINKS[3:] + EDGE_SINKS[:3]])
    G = SinkGraph(pkg, carriers, sinks, 1024 + np.arange(2 * S))
    g = build_graph(pkg, G.host)
    yield pkg, G, g, designs_of(orc, G, EDGE_COUNTS, [carriers[:S], carriers[S:]])
    g.close()


def test_tile_edges(edge_graph, switch):
    pkg, G, g, (a, b) = edge_graph
    order = [a, b] * 17                                  # 34 queries: the cache engages from 32 on
    switch(tile=TILE, min_walks=0)
    out, pq = run_designs(pkg, g, order)
    info = deposit_info(pkg, g)
    items, phases, records, beyond = deposit_usage(pkg, g)
    print("tile edges: %s; items %d phases %d records %d" % (info, items, phases, records))
    assert info["on"] and info["tile"] == TILE and info["n_tiles"] == N // TILE == 64
    assert phases == len(order) and records == len(order) * a.plan.total and beyond == 0
    assert items == len(set(s // TILE for s in EDGE_SINKS))          # tiles 0, 1, 31, 32, 63: one item each
    check_designs(g, order, out, pq, "tile edges")
    for s in EDGE_SINKS:
        assert out[0][s] > 0.0 and out[1][s] > 0.0


# ------------------------------------------------------------------ 3. hot tile, 4. capacity
HOT_COUNTS = [3000, 2000, 1, 64, 2500, 500, 129, 7]


@pytest.fixture(scope="module")
def hot_graph(orc):
    from conftest import load_hooks_pkg
    pkg = load_hooks_pkg()
    S = len(HOT_COUNTS)
    carriers = 256 + np.arange(S)
    sinks = [1000] * (S - 1) + [2600]                     # one node takes all but seven walks; tile 40 takes those
    G = SinkGraph(pkg, carriers, sinks, 3500 + np.arange(S))
    g = build_graph(pkg, G.host)
    yield pkg, G, g, designs_of(orc, G, HOT_COUNTS, [carriers])[0]
    g.close()


def test_hot_tile(hot_graph, switch):
    pkg, G, g, d = hot_graph
    order = [d] * 34
    slice_ = 256
    switch(tile=TILE, slice_=slice_, min_walks=0)
    out, pq = run_designs(pkg, g, order)
    info = deposit_info(pkg, g)
    items, phases, records, beyond = deposit_usage(pkg, g)
    hot = d.plan.total - HOT_COUNTS[-1]
    print("hot tile: %s; items %d phases %d records %d" % (info, items, phases, records))
    assert info["slice"] == slice_ and phases == 34 and records == 34 * d.plan.total and beyond == 0
    assert items == -(-hot // slice_) + 1 and items > 30      # the hot tile's slices and the one item of tile 40
    check_designs(g, order, out, pq, "hot tile")
    live = set(int(x) for x in np.nonzero(out[0])[0])
    assert live == set([1000, 2600]) | set(int(x) for x in d.carriers) | set(int(x) for x in d.seed_nodes)


@pytest.mark.parametrize("cap", [1, 4097, 8200])
def test_capacity(hot_graph, switch, cap):
    """walks [cap, total) of every phase add atomically beside the records of walks [0, cap)"""
    pkg, G, g, d = hot_graph
    assert cap < d.plan.total
    order = [d] * 34
    switch(tile=TILE, slice_=1024, cap=cap, min_walks=0)
    out, pq = run_designs(pkg, g, order)
    info = deposit_info(pkg, g)
    items, phases, records, beyond = deposit_usage(pkg, g)
    print("capacity %d: %s; items %d phases %d records %d beyond %d" % (cap, info, items, phases, records, beyond))
    assert info["cap"] == cap and phases == 34 and records == 34 * cap and beyond == 34 * (d.plan.total - cap)
    check_designs(g, order, out, pq, "capacity %d" % cap)


# ------------------------------------------------------------------ 5. walk counts
class OneEntry:
    """A seed set of one node: the seed's one hop leaves (1 - alpha) on its carrier, the plan's only entry, whose share of
    the budget is 1.0 exactly - so nrw = floor(omega * rsum) = c walks with omega * rsum = c + 0.5 (wp.Design's route to
    eps and conf, for one entry)."""

    def __init__(self, orc, pkg, G, carrier, c):
        a = ALPHA
        self.c, self.carrier, self.seed, self.n = c, int(carrier), int(G.seed_of[carrier]), G.n
        self.rsum = (1.0 - a) ** 2
        r_car = 1.0 - a
        omega = (c + 0.5) / self.rsum
        rmax = 2.0 * r_car
        self.pfail = 0.5
        L = math.log(2.0 / self.pfail)
        m = 1
        while 3.0 * m * omega * ((1.0 - a) * rmax) ** 2 - 2.0 < 1.0:
            m *= 2
        self.conf_m = m
        self.eps = 3.0 * m * omega * ((1.0 - a) * rmax) ** 2 - 2.0
        self.delta = (self.eps + 2.0) * L / self.eps / self.eps / omega
        self.rmax0, self.omega = orc.fora_whole_params(self.conf(orc.Conf), self.eps)
        assert abs(self.omega * self.rsum - (c + 0.5)) < 0.25 and self.rmax0 > 1.5 * r_car
        self.inc = self.rsum / c

    def conf(self, cls):
        cf = cls()
        cf.alpha, cf.delta, cf.pfail, cf.rsum, cf.min_delta, cf.k = ALPHA, self.delta, self.pfail, 1.0, 0.0, 0
        cf.n, cf.m = self.n, self.conf_m
        return cf


@pytest.mark.parametrize("c", [1, 63, 64, 65])
def test_walk_counts(edge_graph, orc, switch, c):
    pkg, G, g, _ = edge_graph
    carrier = 128                                       # its sink: id TILE - 1
    sink = G.sink_of[carrier]
    d = OneEntry(orc, pkg, G, carrier, c)
    ref = np.zeros(N)
    ref[d.seed] = ALPHA
    ref[carrier] = ALPHA * (1.0 - ALPHA)
    for _ in range(c):
        ref[sink] += d.inc
    g.set_tuning(pkg.tuning_batch())
    try:
        for min_walks, binned in ((c, True), (c + 1, False), (None, False)):
            switch(tile=TILE, min_walks=min_walks)
            out, _, _, _, pq, _ = g.fora_batch_seeds([[d.seed]] * 34, d.eps, ALPHA, seed=WALK_SEED, weights=[[1.0]] * 34,
                                                     n_rounds=1, conf=d.conf(pkg.ForaConf), fetch=True, per_query=True)
            info = deposit_info(pkg, g)
            items, phases, records, beyond = deposit_usage(pkg, g)
            print("%d walks, threshold %s: items %d phases %d records %d" % (c, min_walks, items, phases, records))
            assert info["on"]
            # below the threshold the walk kernel adds atomically and the four kernels behind it return at once
            assert (phases, records, beyond) == ((34, 34 * c, 0) if binned else (0, 0, 0))
            for i in range(34):
                assert pq[i].walks == c and pq[i].mc_sources == 1, i
                assert float(np.max(np.abs(out[i] - ref))) <= c * 2.0 ** -52 * d.rsum, (c, min_walks, i)
    finally:
        g.set_tuning(pkg.tuning_default())


def test_no_walks(edge_graph, switch):
    """a dead-end source: no walk phase; and a phase of 0 walks cannot exist beside it (every plan entry has a walk)"""
    pkg, G, g, _ = edge_graph
    dead = 4000
    assert G.deg[dead] == 0
    switch(tile=TILE, min_walks=0)
    g.set_tuning(pkg.tuning_batch())
    try:
        out, _, _, _, pq, _ = g.fora_batch_single_source([dead] * 34, EPS, ALPHA, seed=WALK_SEED, fetch=True, per_query=True)
    finally:
        g.set_tuning(pkg.tuning_default())
    assert deposit_usage(pkg, g) == (0, 0, 0, 0)
    for i in range(34):
        assert pq[i].walks == 0 and out[i][dead] == 1.0 and float(out[i].sum()) == 1.0
