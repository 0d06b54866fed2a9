"""The weighted walk index on the GPU (include/pprhip.h "weighted walk index"; DESIGN.md 2 "Weighted walk index").

An index built at (alpha, seed) holds, per node, the terminals of the very weighted walks the walk phase of
weighted_fora / weighted_fora_seeds draws from that node.  So its cells must be tests/weighted_ref.py's walks bit for
bit, and a served query must equal the host reference - and the same query without the index - up to the order of fp64
additions (TOL_MC, the bar tests/test_gpu_walk_index.py uses for walk increments summed in another order), with the same
walk and round counts and no live step.  Every test here runs the product library on small graphs."""
import numpy as np
import pytest

import weighted_query_ref as wqr
import weighted_ref as wr
from conftest import edges_to_host
from weighted_designs import sparse_design

pytestmark = pytest.mark.gpu
ALPHA = 0.15
EPS = 0.5
TOL_MC = 1e-9

# (graph, weight seed, source, walk seed) of tests/test_gpu_weighted.py: the last source of each graph is a dead end
FORA_CASES = [("got", 21, 63, 3), ("got", 21, 35, 3), ("got", 21, 71, 3),
              ("rmat12", 22, 1803, 4), ("rmat12", 22, 2025, 4), ("rmat12", 22, 3, 4)]
WSEED = {"got": 21, "rmat12": 22}
# (graph, seeds, their weights, walk seed): live seeds and a dead-end seed (got 71, R-MAT 12 node 3) in each set
SEED_SETS = [("got", [63, 35, 71], [2.0, 1.0, 1.0], 3), ("rmat12", [1803, 2025, 3, 7], [1.0, 3.0, 0.5, 2.0], 4)]


def _deg(host):
    return np.diff(host.out_rp.astype(np.int64))


def _rand_w(host, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, host.m)


def _walk_weights(host, by_deg):
    """Random weights; on the rows of degree 3, 65 and 1 500 one weight dominates so far that the small ones behind it
    vanish from the prefix (tests/test_gpu_weighted.py: _walk_weights)."""
    w = _rand_w(host, 43)
    rp = host.out_rp.astype(np.int64)
    for dgr, pos in ((3, 1), (65, 10), (1500, 700)):
        u = by_deg[dgr]
        w[rp[u]:rp[u + 1]] = 1e-3
        w[rp[u] + pos] = 1e16
    return w


def _rho0(pkg, host, alpha=ALPHA, eps=EPS):
    return pkg.walk_index_density(pkg.conf_whole_graph(host.n, host.m, alpha), eps)


def _cap(host, rho):
    """cap(v) = ceil(d(v) * density), none for a dead end (the fp64 product and ceil the library forms)."""
    return np.ceil(_deg(host).astype(np.float64) * np.float64(rho)).astype(np.int64)


def _ref_index(host, tab, cap, alpha, seed, nodes=None):
    """(terminals per node as a dict, steps summed): the reference's walks (seed, stream 0, v, 0 .. cap(v) - 1) with the
    forced first hop, for `nodes` (None: every node) in one call."""
    nodes = np.arange(host.n) if nodes is None else np.unique(np.asarray(nodes, dtype=np.int64))
    cnt = cap[nodes]
    starts = np.repeat(nodes, cnt)
    first = np.cumsum(cnt) - cnt
    j = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(first, cnt)
    term, steps = wr.walks(host, tab, starts, j.astype(np.uint64), alpha, seed, 0, True)
    return {int(v): term[int(a):int(a + c)] for v, a, c in zip(nodes, first, cnt)}, int(steps.sum())


def _check_nodes(g, host, ref, cap, nodes, alpha, seed, live=True):
    """The index's cells of `nodes` against the reference (a prefix of ref[v]: walk j does not depend on the density)
    and, with `live`, against weighted_random_walks of the same walks.  Returns the terminals compared."""
    compared = 0
    for v in nodes:
        v = int(v)
        term = g.weighted_walk_index_terminals(v)
        assert term.size == cap[v], "node %d: %d terminals, capacity %d" % (v, term.size, cap[v])
        if cap[v] == 0:
            assert _deg(host)[v] == 0, v
            continue
        assert np.array_equal(term, ref[v][:cap[v]]), "node %d: stored terminals differ from the reference's walks" % v
        if live:
            walked, _ = g.weighted_random_walks(np.full(cap[v], v, dtype=np.int32), np.arange(cap[v], dtype=np.uint64),
                                                alpha, seed, 0, True)
            assert np.array_equal(term, walked), "node %d: stored terminals differ from weighted_random_walks" % v
        compared += int(cap[v])
    return compared


def _close(a, b, what, worst):
    err = float(np.max(np.abs(a - b))) if a.size else 0.0
    worst[0] = max(worst[0], err)
    assert err <= TOL_MC, "%s: max abs diff %.3e > %.1e" % (what, err, TOL_MC)


@pytest.fixture(scope="module")
def graphs(pkg_product, got, rmat12):
    """One device graph per host graph with the weights of FORA_CASES on it; every test leaves them without an index."""
    made = {}

    def get(name):
        if name not in made:
            host = got if name == "got" else rmat12
            g = pkg_product.Graph(host, device=0)
            g.set_weights(_rand_w(host, WSEED[name]))
            made[name] = (g, host, _rand_w(host, WSEED[name]))
        return made[name]

    yield get
    for g, _, _ in made.values():
        g.close()


# ------------------------------------------------------------------ 1. the index is the walks
@pytest.fixture(scope="module")
def design(pkg_product):
    """sparse_design with the dominated rows' weights, and the reference's walks of every node at the largest density
    under test: computed once, the smaller densities read prefixes of them."""
    host, by_deg = sparse_design(pkg_product)
    w = _walk_weights(host, by_deg)
    tab = wr.table(host, w)
    ref, _ = _ref_index(host, tab, _cap(host, 2.5), ALPHA, 7)
    with pkg_product.Graph(host, device=0) as g:
        g.set_weights(w)
        yield g, host, by_deg, ref


@pytest.mark.parametrize("rho", [0.37, 1.0, 2.5])
def test_index_holds_the_walks_on_the_designed_rows(design, rho):
    """Rows of out-degree 1, 2, 3, 63, 64, 65, 1 500 and 2 500: capacities cross 64 and 128 inside a row, and at 2.5 the
    2 500-row (6 250 terminals) spans about a hundred waves' ranges of 64 positions."""
    g, host, by_deg, ref = design
    cap = _cap(host, rho)
    deg = _deg(host)
    st = g.build_weighted_walk_index(ALPHA, seed=7, density=rho)
    try:
        info = g.weighted_walk_index_info()
        assert info is not None and info["alpha"] == ALPHA and info["seed"] == 7 and info["density"] == rho
        assert info["terminals"] == int(cap[deg > 0].sum()) == st.walks and info["bytes"] >= 4 * info["terminals"]
        assert st.walk_steps >= st.walks > 0                      # forced first hop: every stored walk moved
        if rho == 2.5:
            assert cap[by_deg[2500]] == 6250 and -(-info["terminals"] // 64) >= 300
        rng = np.random.default_rng(17)
        dead = np.flatnonzero(deg == 0)
        nodes = list(by_deg.values()) + [int(x) for x in dead[:6]] + [0, host.n - 1]
        nodes += [int(x) for x in rng.integers(0, host.n, 200)]
        assert (cap[dead] == 0).all() and dead.size > 0
        compared = _check_nodes(g, host, ref, cap, nodes, ALPHA, 7)
        assert compared > sum(int(cap[u]) for u in by_deg.values()) > 0
    finally:
        g.drop_weighted_walk_index()
    assert g.weighted_walk_index_info() is None


def test_index_holds_the_walks_on_got_at_the_default_density(pkg_product, graphs):
    g, host, w = graphs("got")
    rho = _rho0(pkg_product, host)
    cap = _cap(host, rho)
    ref, ref_steps = _ref_index(host, wr.table(host, w), cap, ALPHA, 3)
    st = g.build_weighted_walk_index(ALPHA, seed=3)
    try:
        info = g.weighted_walk_index_info()
        assert info["alpha"] == ALPHA and info["seed"] == 3 and info["density"] == rho
        assert info["terminals"] == int(cap.sum()) == st.walks > 0
        assert st.walk_steps == ref_steps                         # the steps of the WHOLE index
        assert _check_nodes(g, host, ref, cap, range(host.n), ALPHA, 3) == info["terminals"]
    finally:
        g.drop_weighted_walk_index()


# ------------------------------------------------------------------ 2. wave-range edges of the build
def _tiny_few(pkg):
    """fewer than 64 terminals in all: one wave with a short range"""
    rng = np.random.default_rng(3)
    n = 12
    edges = [(u, int(v)) for u in range(n) for v in rng.integers(0, n, rng.integers(0, 4))]
    return edges_to_host(pkg, n, edges), 1.7


def _tiny_multiple(pkg):
    """128 relationships at density 1: the total is an exact multiple of 64, the last wave's range is full"""
    rng = np.random.default_rng(4)
    n = 40
    edges = [(int(u), int(v)) for u, v in zip(rng.integers(0, n, 128), rng.integers(0, n, 128))]
    return edges_to_host(pkg, n, edges), 1.0


def _tiny_dead_runs(pkg):
    """The internal order is: nodes with in-edges by out-degree descending, then the others likewise.  A (8 live nodes
    with in-edges, 64 relationships), D (3 dead ends with in-edges), B (8 live nodes nobody points to, 64 relationships),
    I (3 isolated nodes): at density 1 the second wave's range [64, 128) starts behind the run D of equal offsets 64
    and ends at the run I of offsets 128, which is the end of the table."""
    rng = np.random.default_rng(5)
    A, D, B = list(range(0, 8)), [8, 9, 10], list(range(11, 19))
    edges = []
    for i, d in zip(A, [12, 10, 9, 8, 8, 7, 6, 4]):
        fixed = [A[(i + 1) % 8], D[i % 3]]                        # every node of A and of D has an in-edge
        edges += [(i, v) for v in fixed] + [(i, int(v)) for v in rng.choice(A + D, d - 2)]
    for b, d in zip(B, [16, 12, 10, 8, 7, 5, 4, 2]):
        edges += [(b, int(v)) for v in rng.choice(A + D, d)]
    return edges_to_host(pkg, 22, edges), 1.0


@pytest.mark.parametrize("make", [_tiny_few, _tiny_multiple, _tiny_dead_runs])
def test_build_at_the_edges_of_a_waves_range(pkg_product, make):
    pkg = pkg_product
    host, rho = make(pkg)
    cap = _cap(host, rho)
    total = int(cap.sum())
    if make is _tiny_few:
        assert 0 < total < 64
    else:
        assert total == 128
    if make is _tiny_dead_runs:                                   # the runs sit where the docstring says
        new2old = pkg.lift_host(host)["new2old"]
        off = np.concatenate([[0], np.cumsum(cap[new2old])])
        assert np.flatnonzero(off == 64).size >= 4 and np.flatnonzero(off == 128).size >= 4 and off[-1] == 128
        assert (cap[new2old[-3:]] == 0).all()
    w = _rand_w(host, 44)
    ref, ref_steps = _ref_index(host, wr.table(host, w), cap, ALPHA, 11)
    with pkg.Graph(host, device=0) as g:
        g.set_weights(w)
        st = g.build_weighted_walk_index(ALPHA, seed=11, density=rho)
        assert st.walks == total == g.weighted_walk_index_info()["terminals"] and st.walk_steps == ref_steps
        assert _check_nodes(g, host, ref, cap, range(host.n), ALPHA, 11, live=False) == total


# ------------------------------------------------------------------ 3. served = the reference
def _served_equals(g, host, call, ref, ref_walks, ref_steps, seed, what, worst):
    """`call()` served from an index of (ALPHA, seed) against the reference and against itself without the index."""
    g.build_weighted_walk_index(ALPHA, seed=seed)
    try:
        g.weighted_walk_index_usage(reset=True)
        est, st = call()
        served, walked = g.weighted_walk_index_usage(reset=True)
    finally:
        g.drop_weighted_walk_index()
    est0, st0 = call()
    assert g.weighted_walk_index_usage() == (0, 0)
    print("%s: walks %d served %d walked %d live steps %d (reference %d)" % (what, st.walks, served, walked,
                                                                            st.walk_steps, ref_steps))
    _close(est, ref, "served vs reference " + what, worst)
    _close(est, est0, "served vs unindexed " + what, worst)
    assert st.walks == st0.walks == ref_walks and st.rounds == st0.rounds == 1, what
    assert st.mc_sources == st0.mc_sources, what
    assert served + walked == st.walks and walked == 0 and st.walk_steps == 0, what
    assert st0.walk_steps == ref_steps, what
    return est, st


@pytest.mark.parametrize("name,wseed,src,seed", FORA_CASES)
def test_served_fora_equals_the_reference(graphs, name, wseed, src, seed):
    g, host, w = graphs(name)
    assert wseed == WSEED[name]
    ref, ref_walks, ref_steps = wr.fora(host, w, src, EPS, ALPHA, seed)
    worst = [0.0]
    est, st = _served_equals(g, host, lambda: g.weighted_fora(src, EPS, ALPHA, seed), ref, ref_walks, ref_steps, seed,
                             "%s src %d" % (name, src), worst)
    print("worst max abs diff %.3e" % worst[0])
    if _deg(host)[src] == 0:                                      # the dead-end source: no walks, nothing to serve
        assert st.walks == 0 and est[src] == 1.0 and np.count_nonzero(est) == 1
    else:
        assert st.walks > 0


@pytest.mark.parametrize("name,seeds,sw,seed", SEED_SETS)
def test_served_fora_seeds_equals_the_reference(graphs, name, seeds, sw, seed):
    g, host, w = graphs(name)
    assert (_deg(host)[seeds] == 0).any() and (_deg(host)[seeds] > 0).any()
    ref, ref_walks, ref_steps = wqr.fora_seeds(host, w, seeds, sw, EPS, ALPHA, seed)
    worst = [0.0]
    _, st = _served_equals(g, host, lambda: g.weighted_fora_seeds(seeds, EPS, ALPHA, seed, weights=sw), ref, ref_walks,
                           ref_steps, seed, "%s seeds %s" % (name, seeds), worst)
    print("worst max abs diff %.3e" % worst[0])
    assert st.walks > 0


# ------------------------------------------------------------------ 4. overflow
def _plan(host, w, src, alpha, rmax):
    """weighted_ref.fora's walk plan at rmax: (start, index) of every walk, in plan order."""
    _, omega = wr.whole_params(host.n, host.m, alpha, EPS)
    _, residue, _, _ = wr.push_sync(host, w, src, alpha, rmax)
    rsum = float(residue.sum()) * (1 - alpha)
    nrw = int(omega * rsum)
    v = np.flatnonzero(residue > 0.0)
    omega_i = np.ceil(residue[v] * (1.0 - alpha) / rsum * float(nrw)).astype(np.int64)
    starts = np.repeat(v, omega_i)
    j = np.arange(int(omega_i.sum()), dtype=np.int64) - np.repeat(np.cumsum(omega_i) - omega_i, omega_i)
    return starts, j


@pytest.mark.parametrize("name,src,seed", [("got", 63, 3), ("rmat12", 1803, 4)])
@pytest.mark.parametrize("shrink", [64.0, 1.0])
def test_overflow_walks_are_walked_live(pkg_product, graphs, name, src, seed, shrink):
    """An index of density rho0 / 64, and one of rho0 = the density of rmax0, under a query at 4 rmax0: an entry's
    walks beyond its node's capacity are walked live with their own indices."""
    pkg = pkg_product
    g, host, w = graphs(name)
    rho = _rho0(pkg, host) / shrink
    rmax = 4.0 * wr.whole_params(host.n, host.m, ALPHA, EPS)[0]
    cap = _cap(host, rho)
    starts, j = _plan(host, w, src, ALPHA, rmax)
    over = j >= cap[starts]
    _, steps = wr.walks(host, wr.table(host, w), starts[over], j[over].astype(np.uint64), ALPHA, seed, 0, True)
    est0, st0 = g.weighted_fora(src, EPS, ALPHA, seed, rmax=rmax)
    g.build_weighted_walk_index(ALPHA, seed=seed, density=rho)
    try:
        g.weighted_walk_index_usage(reset=True)
        est, st = g.weighted_fora(src, EPS, ALPHA, seed, rmax=rmax)
        served, walked = g.weighted_walk_index_usage(reset=True)
    finally:
        g.drop_weighted_walk_index()
    what = "%s src %d density rho0 / %g" % (name, src, shrink)
    print("%s: walks %d served %d walked %d live steps %d of %d" % (what, st.walks, served, walked, st.walk_steps,
                                                                   st0.walk_steps))
    assert st.walks == st0.walks == starts.size and st.rounds == st0.rounds == 1, what
    assert served > 0 and walked > 0 and served + walked == st.walks, what
    assert walked == int(over.sum()) and st.walk_steps == int(steps.sum()) < st0.walk_steps, what
    worst = [0.0]
    _close(est, est0, "overflow vs unindexed " + what, worst)
    print("worst max abs diff %.3e" % worst[0])


# ------------------------------------------------------------------ 5. who reads it
def test_who_reads_the_weighted_index(pkg_product, graphs):
    g, host, w = graphs("rmat12")
    src, seed = 1803, 4
    alpha_next = float(np.nextafter(ALPHA, 1.0))                  # differs from ALPHA in the last bit
    ps, pt = [1803, 2025, 7], [5, 1803, 11]
    ws = np.array([1803, 2025, 7, 3] * 8, dtype=np.int32)
    wi = np.arange(ws.size, dtype=np.uint64)

    def others():
        out = {}
        out["seed"] = g.weighted_fora(src, EPS, ALPHA, seed + 1)
        out["alpha"] = g.weighted_fora(src, EPS, alpha_next, seed)
        nsel, ids, vals, est, st = g.weighted_fora_topk(src, EPS, ALPHA, 8, seed, cap=16, fetch=True)
        out["topk"] = (nsel, ids, est, st)
        out["pairs"] = g.weighted_ppr_pairs(ps, pt, EPS, ALPHA, seed)[0]
        out["walks"] = g.weighted_random_walks(ws, wi, ALPHA, seed, 0, True)
        return out

    worst = [0.0]
    plain = others()
    plain_fora, plain_st = g.weighted_fora(src, EPS, ALPHA, seed)
    plain_unw, plain_unw_st = g.fora_single_source(src, EPS, ALPHA, seed=seed, n_rounds=1)
    try:
        # only the weighted index
        g.build_weighted_walk_index(ALPHA, seed=seed)
        g.weighted_walk_index_usage(reset=True)
        est, st = g.weighted_fora(src, EPS, ALPHA, seed)            # a matching alpha and seed: served
        assert g.weighted_walk_index_usage(reset=True) == (st.walks, 0) and st.walks == plain_st.walks > 0
        _close(est, plain_fora, "served", worst)
        got_ = others()
        assert g.weighted_walk_index_usage() == (0, 0)            # none of them read it
        for key in ("seed", "alpha"):
            _close(got_[key][0], plain[key][0], "another " + key, worst)
            assert got_[key][1].walks == plain[key][1].walks and got_[key][1].walk_steps == plain[key][1].walk_steps > 0
        assert got_["topk"][0] == plain["topk"][0] and np.array_equal(got_["topk"][1], plain["topk"][1])
        _close(got_["topk"][2], plain["topk"][2], "weighted_fora_topk", worst)
        assert got_["topk"][3].walk_steps == plain["topk"][3].walk_steps > 0
        _close(got_["pairs"], plain["pairs"], "weighted_ppr_pairs", worst)
        assert np.array_equal(got_["walks"][0], plain["walks"][0]) and np.array_equal(got_["walks"][1], plain["walks"][1])
        unw, unw_st = g.fora_single_source(src, EPS, ALPHA, seed=seed, n_rounds=1)
        assert g.walk_index_usage() == (0, 0) and g.weighted_walk_index_usage() == (0, 0)
        assert unw_st.walks == plain_unw_st.walks and unw_st.walk_steps == plain_unw_st.walk_steps > 0
        _close(unw, plain_unw, "fora_single_source beside the weighted index", worst)
        # only the unweighted index
        g.drop_weighted_walk_index()
        g.build_walk_index(ALPHA, seed=seed)
        g.walk_index_usage(reset=True)
        est, st = g.weighted_fora(src, EPS, ALPHA, seed)
        assert g.walk_index_usage() == (0, 0) and g.weighted_walk_index_usage() == (0, 0)
        assert st.walks == plain_st.walks and st.walk_steps == plain_st.walk_steps > 0
        _close(est, plain_fora, "weighted_fora beside the unweighted index", worst)
        # both: each call reads its own
        g.build_weighted_walk_index(ALPHA, seed=seed)
        assert g.walk_index_info() is not None and g.weighted_walk_index_info() is not None
        unw, unw_st = g.fora_single_source(src, EPS, ALPHA, seed=seed, n_rounds=1)
        assert g.walk_index_usage(reset=True) == (unw_st.walks, 0) and g.weighted_walk_index_usage() == (0, 0)
        _close(unw, plain_unw, "fora_single_source with both", worst)
        est, st = g.weighted_fora(src, EPS, ALPHA, seed)
        assert g.weighted_walk_index_usage(reset=True) == (st.walks, 0) and g.walk_index_usage() == (0, 0)
        assert st.walk_steps == 0
        _close(est, plain_fora, "weighted_fora with both", worst)
        for v in (src, 2025):                                     # two tables of the same shape: the walks differ
            a, b = g.walk_index_terminals(v), g.weighted_walk_index_terminals(v)
            assert a.size == b.size >= 7 and not np.array_equal(a, b)
    finally:
        g.drop_walk_index()
        g.drop_weighted_walk_index()
    print("worst max abs diff %.3e" % worst[0])


# ------------------------------------------------------------------ 6. lifecycle
def test_lifecycle(pkg_product, rmat12):
    pkg = pkg_product
    host = rmat12
    w1, w2 = _rand_w(host, 51), _rand_w(host, 52)
    with pkg.Graph(host, device=0) as g:
        with pytest.raises(pkg.PprhipError, match="pprhip_weighted_walk_index_build: .*no relationship weights") as e:
            g.build_weighted_walk_index(ALPHA, seed=3)            # refused as every weighted_ call without weights
        assert e.value.code == pkg.ERR_STATE and g.weighted_walk_index_info() is None
        with pytest.raises(pkg.PprhipError, match="pprhip_weighted_walk_index_fetch") as e:
            g.weighted_walk_index_terminals(0)
        assert e.value.code == pkg.ERR_STATE
        g.drop_weighted_walk_index()                              # no-op without one
        g.set_weights(w1)
        g.build_weighted_walk_index(ALPHA, seed=3)
        first = g.weighted_walk_index_info()
        assert first is not None
        g.set_weights(w2)                                         # a second set of weights: the index went before them
        assert g.weighted_walk_index_info() is None
        g.build_weighted_walk_index(ALPHA, seed=3)
        assert g.weighted_walk_index_info() == first
        g.set_weights(None)
        assert g.weighted_walk_index_info() is None and g.weights_info() == (False, 0)
        g.set_weights(w1)
        g.build_weighted_walk_index(ALPHA, seed=3)
        g.release(pkg.Graph.RELEASE_WEIGHTS)
        assert g.weighted_walk_index_info() is None and g.weights_info() == (False, 0)
        g.set_weights(w1)
        g.build_weighted_walk_index(ALPHA, seed=3)
        cells = g.weighted_walk_index_terminals(1803)
        for bad in (np.nan, 0.0, -1.0):                           # a rejected set of weights changes nothing
            wb = w1.copy()
            wb[100] = bad
            with pytest.raises(pkg.PprhipError, match="edge 100"):
                g.set_weights(wb)
            assert g.weighted_walk_index_info() == first
        g.build_walk_index(ALPHA, seed=3)                         # the unweighted index comes and goes beside it
        g.drop_walk_index()
        assert g.weighted_walk_index_info() == first
        g.build_walk_index(ALPHA, seed=3)
        g.release(pkg.Graph.RELEASE_WALK_INDEX)
        assert g.walk_index_info() is None and g.weighted_walk_index_info() == first
        assert np.array_equal(g.weighted_walk_index_terminals(1803), cells)
        g.build_weighted_walk_index(0.3, seed=8, density=0.5)     # a rebuild replaces it
        info = g.weighted_walk_index_info()
        assert (info["alpha"], info["seed"], info["density"]) == (0.3, 8, 0.5)
        assert info["terminals"] == int(np.ceil(_deg(host) * 0.5).sum())
        with pytest.raises(pkg.PprhipError) as e:
            g.build_weighted_walk_index(ALPHA, seed=3, density=1e12)   # 2^36 terminals or more: the old one stays
        assert e.value.code == pkg.ERR_INVALID and g.weighted_walk_index_info() == info
        g.release(pkg.Graph.RELEASE_WEIGHTED_WALK_INDEX)
        assert g.weighted_walk_index_info() is None and g.weights_info()[0]
        g.drop_weighted_walk_index()


def test_drop_gives_the_bytes_back(pkg_product, rmat15, rmat12):
    """The method of tests/test_gpu_weighted.py::test_drop_and_release_give_the_bytes_back: free bytes of the device
    read through a small handle that stays.  Density 16 on R-MAT 15: 8.4 M terminals, 34 MB."""
    pkg = pkg_product
    w = _rand_w(rmat15, 61)
    with pkg.Graph(rmat12, device=0) as probe:
        with pkg.Graph(rmat15, device=0) as g:
            g.set_weights(w)
            g.build_weighted_walk_index(ALPHA, seed=3, density=16.0)   # first round: code objects, the allocator's pools
            g.drop_weighted_walk_index()
            free0, _ = probe.device_memory()
            g.build_weighted_walk_index(ALPHA, seed=3, density=16.0)
            nbytes = g.weighted_walk_index_info()["bytes"]
            free1, _ = probe.device_memory()
            g.build_weighted_walk_index(ALPHA, seed=4, density=16.0)   # a rebuild: no second table stays
            free1b, _ = probe.device_memory()
            g.drop_weighted_walk_index()
            free2, _ = probe.device_memory()
            g.build_weighted_walk_index(ALPHA, seed=3, density=16.0)
            g.set_weights(None)                                        # goes with the weights
            g.set_weights(w)
            free3, _ = probe.device_memory()
            g.build_weighted_walk_index(ALPHA, seed=3, density=16.0)   # the handle closes with an index on it
        free4, _ = probe.device_memory()
    slack = 8 << 20
    print("weighted walk index: %d bytes; device memory taken %d, after drop %+d, after the weights' change %+d" %
          (nbytes, free0 - free1, free0 - free2, free0 - free3))
    assert nbytes >= 4 * 16 * rmat15.m >= 3 * slack
    assert free0 - free1 >= nbytes - slack and abs(free1b - free1) <= slack
    assert abs(free0 - free2) <= slack and abs(free0 - free3) <= slack
    assert free4 >= free0
