"""k_mc_walk (plain, indexed, shared), k_index_serve and k_index_build on walk plans designed entry by entry
(tests/walk_plans.py; DESIGN.md 3 "Designed walk plans"): entry boundaries put on purpose at share and window
boundaries and one walk to either side, capacities of the walk index at c_i - 1, c_i and beyond, the terminal cache of a
batched call, and every terminal of an index.

Every vector is held against two references at TOL_MC = 1e-9 (walk sums in another order): the CPU twin, and a vector
rebuilt from the design and the oracle's single walker (Design.independent), with `walks`, `mc_sources`, `walk_steps`
and `rounds` equal.  min inc / TOL_MC >= 1000 is asserted per plan: one walk credited to another entry or terminal moves
two elements by >= 1000 tolerances.  That bound caps a plan at 0.7225 / 1e-6 = 722 500 walks where every entry has many (uniform blocks: 700 000), at
361 250 where one-walk entries stand beside larger ones (340 000), and at 722 500 entries where all have one walk
(600 000, on a built body graph: no R-MAT of test size has that many nodes with out-edges).  On 16 waves per CU of 256
that is a share of 192 walks (a window of 128 and one of 64) for the blocks and the 600 000 ones, 128 (one window) for
the giant entry and the mixed plan, 64 for everything smaller; shares of three to six windows come from the calls of
sixteen sets, whose walk phases run on a quarter of that grid.  Which plan meets a window of 128 entries (jl = 127) or
a serve chunk of 64 (jl = 63) with another behind it is counted on the CPU (test_walk_plans_design.py).
The graphs are built with PPRHIP_RELABEL=0, so plan entries are in carrier order as designed; the tests neither read
nor assume the CU count."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import walk_plans as wp
from walk_plans import ALPHA, TOL_MC, WALK_SEED

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]
TOL_SPEC = 1e-6


def assert_close(a, b, what):
    err = float(np.max(np.abs(a - b))) if a.size else 0.0
    print("%s: max abs diff %.3e" % (what, err))
    assert err <= TOL_MC, "%s: max abs diff %.3e > %.1e" % (what, err, TOL_MC)


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


@pytest.fixture(scope="module")
def ctx(orc):
    """Per scale: the plan graph on the device (hooks library, ids kept) and on the oracle; every test leaves the handle
    with the default tuning and without an index."""
    from conftest import load_hooks_pkg
    pkg = load_hooks_pkg()
    made = {}

    def get(scale):
        if scale not in made:
            G = wp.plan_graph(pkg, scale)
            made[scale] = (G, build_graph(pkg, G.host), wp.oracle_graph(orc, G))
        return made[scale]

    yield pkg, get
    for _, g, _ in made.values():
        g.close()


_plain = {}


def plain_query(pkg, orc, get, name):
    """The query of plan `name` on a handle without an index, checked against both references (once per plan)."""
    if name in _plain:
        return _plain[name]
    D = wp.design(orc, pkg, name)
    G, g, og = get(D.plan.scale)
    assert g.walk_index_info() is None
    est, st = g.fora_seeds(D.seeds, D.eps, ALPHA, seed=WALK_SEED, weights=D.weights, n_rounds=1, conf=D.conf(pkg.ForaConf))
    ref, sto = D.twin(orc, og)
    ind = D.independent(og)
    S = D.counts.size
    print("%s: S %d walks %d, share %d at a grid of %d (%d windows), min inc / TOL_MC %.0f" % (
        name, S, D.plan.total, D.share(), wp.GRID_REF, -(-D.share() // 128), D.sensitivity()))
    assert D.sensitivity() >= 1000.0
    assert st.walks == sto.walks == D.plan.total and st.mc_sources == sto.mc_sources == S
    assert st.walk_steps == sto.walk_steps and st.rounds == sto.rounds == 1 and st.levels == sto.levels == 1
    assert_close(est, ref, name + " plain vs twin")
    assert_close(est, ind, name + " plain vs independent")
    _plain[name] = (est, st)
    return _plain[name]


# ------------------------------------------------------------------ 1. plain
@pytest.mark.parametrize("name", list(wp.PLANS))
def test_plain(ctx, orc, name):
    pkg, get = ctx
    t0 = time.time()
    D = wp.design(orc, pkg, name)
    est, _ = plain_query(pkg, orc, get, name)
    if D.plan.n_dead:
        # dead-end seeds make no entry (mc_sources == S above) and hold the closed form alone: nothing walks into them
        assert np.all(np.abs(est[D.dead_nodes] - D.dead_reserve) <= 1e-15)
    print("%s: %.2f s" % (name, time.time() - t0))


# ------------------------------------------------------------------ 2. indexed
@pytest.mark.parametrize("name", list(wp.PLANS))
def test_indexed(ctx, orc, name):
    pkg, get = ctx
    t0 = time.time()
    D = wp.design(orc, pkg, name)
    G, g, og = get(D.plan.scale)
    est0, st0 = plain_query(pkg, orc, get, name)
    ind = D.independent(og)
    total = D.plan.total
    try:
        for label, rho in D.densities():
            g.build_walk_index(ALPHA, seed=WALK_SEED, density=rho)
            info = g.walk_index_info()
            assert info["terminals"] == int(np.ceil(G.deg * rho).sum())
            g.walk_index_usage(reset=True)
            est, st = g.fora_seeds(D.seeds, D.eps, ALPHA, seed=WALK_SEED, weights=D.weights, n_rounds=1,
                                   conf=D.conf(pkg.ForaConf))
            served, walked = g.walk_index_usage(reset=True)
            what = "%s %s (density %.6g, %d terminals)" % (name, label, rho, info["terminals"])
            print("%s: served %d walked %d live steps %d of %d" % (what, served, walked, st.walk_steps, st0.walk_steps))
            assert (served, walked) == D.usage(rho), what
            assert served + walked == st.walks == total and st.mc_sources == D.counts.size, what
            if label == "served":
                assert walked == 0
            if label.startswith(("one-over", "share-first-over")):
                assert walked == 1
            if label == "each-over-by-one":
                assert walked == D.counts.size
            if label == "all-over":
                assert served == D.counts.size
            assert st.walk_steps == D.overflow_steps(og, rho), what
            assert_close(est, est0, what + " vs plain")
            assert_close(est, ind, what + " vs independent")
            if D.plan.n_dead:
                assert g.walk_index_terminals(int(D.dead_nodes[0])).size == 0     # capacity 0 beside served entries
    finally:
        g.drop_walk_index()
    print("%s: %.2f s" % (name, time.time() - t0))


# ------------------------------------------------------------------ 3. batched calls: the narrow grid, the cache
BATCH_PLANS = wp.LARGE_PLANS + ["A-ones-130", "C-blocks-129-small", "D-mixed-small", "F-dead-dup-wide"]


@pytest.mark.parametrize("name", BATCH_PLANS)
def test_batched_call_of_sixteen(ctx, orc, name):
    """Sixteen copies of the set in one call, below the cache's threshold: k_mc_walk<plain>, then - with an index that
    holds every walk, and one that holds each entry's first walk only - k_index_serve and k_mc_walk<indexed>.  The walk
    phase of a batched call is launched with 4 waves per CU instead of 16 (fora.cpp: side_walk_waves), four times the
    share; nothing a caller can read shows a launch's grid, so the shares printed here and counted in
    test_walk_plans_design.py are inferred from the launchers, not observed."""
    pkg, get = ctx
    t0 = time.time()
    D = wp.design(orc, pkg, name)
    G, g, og = get(D.plan.scale)
    est0, st0 = plain_query(pkg, orc, get, name)
    ind = D.independent(og)
    full, chunks, windows = wp.replay(D.counts, wp.GRID_SIDE)
    print("%s: share %d on %d waves (%d windows; %d windows of 128 entries and %d chunks of 64 with a successor)" % (
        name, D.share(wp.GRID_SIDE), wp.GRID_SIDE, windows, full, chunks))
    dens = D.densities()
    g.set_tuning(pkg.tuning_batch())
    try:
        for label, rho in [(None, None), dens[0], dens[-1]]:
            if label:
                g.build_walk_index(ALPHA, seed=WALK_SEED, density=rho)
                g.walk_index_usage(reset=True)
            out, _, _, _, pq, _ = g.fora_batch_seeds([D.seeds] * 16, D.eps, ALPHA, seed=WALK_SEED,
                                                     weights=[D.weights] * 16, n_rounds=1, conf=D.conf(pkg.ForaConf),
                                                     fetch=True, per_query=True)
            steps = st0.walk_steps
            if label:
                served, walked = g.walk_index_usage(reset=True)
                assert (served, walked) == tuple(16 * x for x in D.usage(rho)), (name, label)
                steps = D.overflow_steps(og, rho)
            for i in range(16):
                assert pq[i].walks == st0.walks and pq[i].walk_steps == steps and pq[i].mc_sources == st0.mc_sources
                err = float(np.max(np.abs(out[i] - ind)))
                assert err <= TOL_MC and float(np.max(np.abs(out[i] - est0))) <= TOL_MC, (name, label, i, err)
    finally:
        g.set_tuning(pkg.tuning_default())
        g.drop_walk_index()
    print("%s: %.2f s" % (name, time.time() - t0))


def share_hooks(pkg):
    L = pkg.lib()
    u64p, ip = C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    L.pprhip_hook_walk_share_info.argtypes = [C.c_void_p, ip, ip, u64p, u64p, u64p]
    L.pprhip_hook_walk_share_usage.argtypes = [C.c_void_p, u64p, u64p, C.c_int]
    L.pprhip_hook_walk_share_fetch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, u64p]
    return L


def share_cells(pkg, g, node):
    cnt = C.c_uint64()
    L = share_hooks(pkg)
    pkg._check(L.pprhip_hook_walk_share_fetch(g.h, node, None, 0, C.byref(cnt)))
    out = np.empty(cnt.value, dtype=np.int32)
    if cnt.value:
        pkg._check(L.pprhip_hook_walk_share_fetch(g.h, node, out.ctypes.data_as(C.c_void_p), cnt.value, C.byref(cnt)))
    return out


def shared_designs(orc, pkg, scale, half):
    """Three sets of one W for one call: `a`; `b` on the same carriers with one walk more on its first half and one less
    on its second, so cells beyond a's walks stay empty until b draws them; `c` on other carriers."""
    G = wp.plan_graph(pkg, scale)
    top = G.top(4 * half)
    lo = [1, 2, 63, 64, 65, 127, 128, 129]
    hi = [2, 3, 66, 130, 300, 64, 129, 5]
    ca = np.array([lo[i % 8] for i in range(half)] + [hi[i % 8] for i in range(half)])
    cb = ca + np.concatenate([np.ones(half, dtype=np.int64), -np.ones(half, dtype=np.int64)])
    plans = [wp.Plan("shared-a", scale, ca, carriers=("ids", top[0::2])),
             wp.Plan("shared-b", scale, cb, carriers=("ids", top[0::2])),
             wp.Plan("shared-c", scale, ca, carriers=("ids", top[1::2]))]
    ds = [wp.Design(orc, G, p) for p in plans]
    lead = max(ds, key=lambda d: d.rmax0)
    for d in ds:
        if d is not lead:
            d.adopt(lead)
    return ds


@pytest.mark.parametrize("scale,half", [(12, 24), (15, 1200)])
def test_shared(ctx, orc, scale, half):
    pkg, get = ctx
    t0 = time.time()
    G, g, og = get(scale)
    ds = shared_designs(orc, pkg, scale, half)
    a, b, c = ds
    order = [a, a, b, c] * 8 + [b, a]                       # 34 queries: the cache engages from 32 on
    conf = a.conf(pkg.ForaConf)
    single = []
    for d in ds:
        ref, sto = d.twin(orc, og)
        assert sto.levels == 1 and sto.walks == d.plan.total and sto.mc_sources == d.counts.size   # the designer's check
        est, st = g.fora_seeds(d.seeds, d.eps, ALPHA, seed=WALK_SEED, weights=d.weights, n_rounds=1, conf=conf)
        assert st.walks == sto.walks and st.walk_steps == sto.walk_steps
        assert_close(est, ref, "%s single vs twin" % d.plan.name)
        assert_close(est, d.independent(og), "%s single vs independent" % d.plan.name)
        assert d.sensitivity() >= 1000.0
        single.append((est, st))
    by = {id(d): s for d, s in zip(ds, single)}
    # the cache's size, from the density the call starts at - a condition, checked before anything is launched
    density = (1.0 - ALPHA) * a.rmax0 * a.omega * (1.0 + 2.0 ** -20)
    cap = np.where(G.deg > 0, np.ceil(G.deg * density), 0).astype(np.int64)
    cells_total = int(cap.sum())
    print("scale %d: density %.6g, %d cells" % (scale, density, cells_total))
    assert cells_total < 64 << 20
    for d in ds:
        assert np.all(cap[d.carriers] >= d.counts)          # every walk of the call lies below its node's capacity
    L = share_hooks(pkg)
    g.set_tuning(pkg.tuning_batch())
    try:
        out, _, _, _, pq, _ = g.fora_batch_seeds([d.seeds for d in order], a.eps, ALPHA, seed=WALK_SEED,
                                                 weights=[d.weights for d in order], n_rounds=1, conf=conf, fetch=True,
                                                 per_query=True)
    finally:
        g.set_tuning(pkg.tuning_default())
    present, on, seed, cells, nbytes = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    pkg._check(L.pprhip_hook_walk_share_info(g.h, C.byref(present), C.byref(on), C.byref(seed), C.byref(cells),
                                             C.byref(nbytes)))
    assert present.value and seed.value == WALK_SEED and cells.value == cells_total
    served, stored = C.c_uint64(), C.c_uint64()
    pkg._check(L.pprhip_hook_walk_share_usage(g.h, C.byref(served), C.byref(stored), 1))
    for i, d in enumerate(order):
        est, st = by[id(d)]
        assert pq[i].walks == st.walks and pq[i].mc_sources == st.mc_sources, i
        err = float(np.max(np.abs(out[i] - est)))
        assert err <= TOL_MC, ("query %d (%s) vs its single query" % (i, d.plan.name), err)
        assert float(np.max(np.abs(out[i] - d.independent(og)))) <= TOL_MC, i
    # the cells: every walk index some query drew holds the oracle's terminal, everything beyond is empty
    drawn = np.zeros(G.n, dtype=np.int64)
    for d in ds:
        np.maximum.at(drawn, d.carriers, d.counts)
    nodes = np.nonzero(drawn)[0]
    starts = np.repeat(nodes, drawn[nodes]).astype(np.int32)
    idx = np.concatenate([np.arange(k) for k in drawn[nodes]]).astype(np.uint64)
    term, _ = og.random_walks(starts, idx, ALPHA, WALK_SEED, 0, True)
    want = dict(zip([int(v) for v in nodes], np.split(term, np.cumsum(drawn[nodes])[:-1])))
    check = range(G.n) if G.n < 10000 else [int(v) for v in nodes] + list(range(0, G.n, 37))
    for v in check:
        cellv = share_cells(pkg, g, v)
        assert cellv.size == cap[v], v
        k = int(drawn[v])
        if k:
            assert np.array_equal(cellv[:k], want[v]), "node %d: cached terminals differ from the oracle's walks" % v
        assert np.all(cellv[k:] == -1), "node %d: a cell beyond every query's walks is filled" % v
    # every walk below capacity (here: every walk) was either served or stored, none counted twice; each drawn cell was
    # stored at least once (two waves that probe an empty cell together both walk and both store)
    total = sum(d.plan.total for d in order)
    distinct = int(drawn.sum())
    print("scale %d: %d walks, served %d stored %d, %d distinct cells" % (scale, total, served.value, stored.value, distinct))
    assert served.value + stored.value == total == sum(x.walks for x in pq)
    assert stored.value >= distinct and served.value > 0
    print("shared scale %d: %.2f s" % (scale, time.time() - t0))


# ------------------------------------------------------------------ 4. k_index_build, every terminal
def index_graph(pkg, kind):
    """(host, hub, H): dead-end runs at the start, in the middle and at the end of the id order, live nodes of out-degree
    1..3 between them and one hub of H out-edges, whose capacity sets the index's total."""
    rng = np.random.default_rng(7)
    n, runs, n_small, hub, H = {"one": (30, [(0, 8), (14, 20), (25, 30)], 0, 12, 5000),
                                "few": (200, [(0, 20), (90, 110), (180, 200)], 29, 85, 400),
                                "many": (1500, [(0, 100), (700, 800), (1400, 1500)], 1000, 650, 16000)}[kind]
    dead = np.zeros(n, dtype=bool)
    for lo, hi in runs:
        dead[lo:hi] = True
    cand = np.nonzero(~dead)[0]
    cand = cand[cand != hub]
    small = rng.choice(cand, n_small, replace=False) if n_small else np.zeros(0, dtype=np.int64)
    src = [np.full(H, hub)]
    for v in small:
        src.append(np.full(int(rng.integers(1, 4)), v))
    src = np.concatenate(src).astype(np.int32)
    dst = rng.integers(0, n, src.size).astype(np.int32)
    return pkg.HostCsr(n, src, dst), hub, H


INDEX_CASES = [("one", t) for t in (1, 63, 64, 65, 4095, 4096, 4097)] + [("few", t) for t in (63, 64, 65)] + \
              [("many", t) for t in (4095, 4096, 4097)] + [("many", None)]


@pytest.mark.parametrize("kind,total", INDEX_CASES)
def test_index_build_every_terminal(ctx, orc, kind, total):
    pkg, _ = ctx
    host, hub, H = index_graph(pkg, kind)
    assert host.n <= 2000
    d = np.diff(host.out_rp.astype(np.int64))
    live = int((d > 0).sum())
    # a total: every live node but the hub has capacity 1 (the regime where most nodes hold one terminal), the hub the
    # rest; total None: the mixed case, capacities of 3 to 9 and the hub's 44 000
    rho = 2.75 if total is None else (total - (live - 1) - 0.5) / H
    cap = np.where(d > 0, np.ceil(d * rho), 0).astype(np.int64)
    if total is not None:
        assert int(cap.sum()) == total and np.all(cap[(d > 0) & (np.arange(host.n) != hub)] == 1)
    og = orc.OracleGraph(host.n, host.out_rp, host.out_ci, host.in_rp, host.in_ci)
    starts = np.repeat(np.arange(host.n), cap).astype(np.int32)
    idx = np.concatenate([np.arange(k) for k in cap]).astype(np.uint64)
    term, steps = og.random_walks(starts, idx, ALPHA, WALK_SEED, 0, True)
    want = np.split(term, np.cumsum(cap)[:-1])
    g = build_graph(pkg, host)
    try:
        st = g.build_walk_index(ALPHA, seed=WALK_SEED, density=rho)
        assert st.walks == int(cap.sum()) == g.walk_index_info()["terminals"]
        assert st.walk_steps == int(steps.astype(np.int64).sum())
        for v in range(host.n):
            got = g.walk_index_terminals(v)
            assert got.size == cap[v], "node %d: %d terminals, capacity %d" % (v, got.size, cap[v])
            assert np.array_equal(got, want[v]), "node %d: stored terminals differ from the oracle's walks" % v
    finally:
        g.close()
