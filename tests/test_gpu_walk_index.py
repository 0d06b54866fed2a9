"""The FORA+ walk index on the GPU (include/pprhip.h "walk index"; DESIGN.md 2 "Walk index").

An index built at (alpha, seed) holds, per node, the terminals of the very walks a whole-graph FORA walk phase draws
from that node, so a served query must equal the CPU twin - and the same query without the index - up to the order of
fp64 additions (TOL_MC, the bar tests/test_gpu_parity.py uses for sums of walk increments in another order), with the
same round and walk counts.  Every test here runs the product library."""
import numpy as np
import pytest

from conftest import to_oracle

pytestmark = pytest.mark.gpu
ALPHA = 0.15
EPS = 0.5
TOL_SPEC = 1e-6
TOL_MC = 1e-9


def assert_close(a, b, tol, what):
    err = float(np.max(np.abs(a - b))) if a.size else 0.0
    print("%s: max abs diff %.3e" % (what, err))
    assert err <= tol, "%s: max abs diff %.3e > %.1e" % (what, err, tol)
    assert err <= TOL_SPEC


def sources(host, count, seed=2):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(0, host.n, size=count)]


def live_sources(host, count, seed):
    live = np.nonzero(np.diff(host.out_rp) > 0)[0]
    rng = np.random.default_rng(seed)
    return [int(x) for x in live[rng.integers(0, live.size, count)]]


def to_orc_tuning(orc, t):
    o = orc.tuning_default()
    for f, _ in o._fields_:
        setattr(o, f, getattr(t, f))
    return o


def rho0(pkg, host, alpha=ALPHA, eps=EPS):
    return pkg.walk_index_density(pkg.conf_whole_graph(host.n, host.m, alpha), eps)


@pytest.fixture(scope="module")
def graphs(pkg_product, got, rmat12, rmat15):
    """One device graph per host graph for the whole module; every test leaves them without an index."""
    pkg = pkg_product
    made = {}

    def get(name):
        if name not in made:
            made[name] = pkg.Graph({"got": got, "rmat12": rmat12, "rmat15": rmat15}[name])
        return made[name]

    yield get
    for g in made.values():
        g.close()


# ------------------------------------------------------------------ 1. the index is the walks
@pytest.mark.parametrize("name", ["got", "rmat12"])
def test_index_holds_the_walks(pkg_product, orc, graphs, got, rmat12, name):
    pkg = pkg_product
    host = got if name == "got" else rmat12
    g = graphs(name)
    og = to_oracle(orc, host)
    rho = rho0(pkg, host)
    d = np.diff(host.out_rp).astype(np.float64)
    cap = np.ceil(d * rho).astype(np.int64)
    cap[d == 0] = 0
    try:
        st = g.build_walk_index(ALPHA, seed=3)
        info = g.walk_index_info()
        assert info is not None and info["alpha"] == ALPHA and info["seed"] == 3 and info["density"] == rho
        assert info["terminals"] == int(cap.sum()) == st.walks and info["bytes"] >= 4 * info["terminals"]
        assert st.walk_steps >= st.walks > 0 and st.mc_ms > 0     # forced first hop: every stored walk moved
        rng = np.random.default_rng(17)
        nodes = [int(v) for v in rng.integers(0, host.n, 200)]
        nodes += [int(np.argmax(d)), int(np.argmin(d))]
        compared = 0
        for v in nodes:
            term = g.walk_index_terminals(v)
            assert term.size == cap[v], "node %d: %d terminals, capacity %d" % (v, term.size, cap[v])
            if cap[v] == 0:
                assert d[v] == 0
                continue
            want = np.array([og.random_walk(v, ALPHA, 3, 0, j, True)[0] for j in range(int(cap[v]))], dtype=np.int32)
            assert np.array_equal(term, want), "node %d: stored terminals differ from the oracle's walks" % v
            live, _ = g.random_walks(np.full(cap[v], v, dtype=np.int32), np.arange(cap[v], dtype=np.uint64), ALPHA, seed=3,
                                     stream=0, no_zero_hop=True)
            assert np.array_equal(term, live), "node %d: stored terminals differ from random_walks" % v
            compared += int(cap[v])
        assert compared > 200
    finally:
        g.drop_walk_index()
    assert g.walk_index_info() is None


# ------------------------------------------------------------------ 2. served FORA = the twin
def _served_equals_twin(pkg, orc, host, g, srcs, seed, rounds):
    og = to_oracle(orc, host)
    for n_rounds in rounds:
        for s in srcs:
            g.build_walk_index(ALPHA, seed=seed)
            g.walk_index_usage(reset=True)
            est, st = g.fora_single_source(s, EPS, ALPHA, seed=seed, n_rounds=n_rounds)
            served, walked = g.walk_index_usage(reset=True)
            ref, sto = og.fora_whole(s, EPS, ALPHA, seed=seed, n_rounds=n_rounds, schedule=orc.SYNC)
            what = "src=%d rounds=%d" % (s, n_rounds)
            print("%s: walks %d served %d walked %d live steps %d (twin steps %d)" % (what, st.walks, served, walked,
                                                                                      st.walk_steps, sto.walk_steps))
            assert st.rounds == sto.rounds and st.walks == sto.walks, what
            assert_close(est, ref, TOL_MC, "served vs twin " + what)
            assert served + walked == st.walks, what
            if n_rounds >= 1:                      # the last round is never cut: the push converged at <= rmax0
                assert walked == 0 and st.walk_steps == 0, what
            else:
                assert st.walk_steps <= sto.walk_steps, what
            g.drop_walk_index()
            est0, st0 = g.fora_single_source(s, EPS, ALPHA, seed=seed, n_rounds=n_rounds)
            assert st0.walks == st.walks and st0.walk_steps == sto.walk_steps, what
            assert_close(est, est0, TOL_MC, "served vs unindexed " + what)
            assert g.walk_index_usage() == (0, 0)


@pytest.mark.parametrize("n_rounds", [1, 2, 4, 0])
def test_served_fora_equals_twin_got(pkg_product, orc, graphs, got, n_rounds):
    g = graphs("got")
    try:
        _served_equals_twin(pkg_product, orc, got, g, [0, 17, 42, 106] + sources(got, 4, seed=11), 3, [n_rounds])
    finally:
        g.drop_walk_index()


@pytest.mark.parametrize("n_rounds", [1, 2, 4, 0])
def test_served_fora_equals_twin_rmat12(pkg_product, orc, graphs, rmat12, n_rounds):
    g = graphs("rmat12")
    try:
        _served_equals_twin(pkg_product, orc, rmat12, g, sources(rmat12, 3, seed=5), 9, [n_rounds])
    finally:
        g.drop_walk_index()


# ------------------------------------------------------------------ 3. overflow path
@pytest.mark.parametrize("name", ["got", "rmat12"])
def test_overflow_walks_are_walked_live(pkg_product, orc, graphs, got, rmat12, name):
    pkg = pkg_product
    host = got if name == "got" else rmat12
    g = graphs(name)
    og = to_oracle(orc, host)
    steps = {}
    try:
        g.build_walk_index(ALPHA, seed=3, density=rho0(pkg, host) / 64.0)
        for s in live_sources(host, 3, seed=23):
            for n_rounds in (1, 0):
                g.walk_index_usage(reset=True)
                est, st = g.fora_single_source(s, EPS, ALPHA, seed=3, n_rounds=n_rounds)
                served, walked = g.walk_index_usage(reset=True)
                ref, sto = og.fora_whole(s, EPS, ALPHA, seed=3, n_rounds=n_rounds, schedule=orc.SYNC)
                what = "%s src=%d rounds=%d" % (name, s, n_rounds)
                print("%s: walks %d served %d walked %d live steps %d of %d" % (what, st.walks, served, walked,
                                                                               st.walk_steps, sto.walk_steps))
                assert st.rounds == sto.rounds and st.walks == sto.walks, what
                assert_close(est, ref, TOL_MC, "overflow vs twin " + what)
                assert served > 0 and walked > 0 and served + walked == st.walks, what
                steps[(s, n_rounds)] = (st.walks, st.walk_steps, est)
    finally:
        g.drop_walk_index()
    for (s, n_rounds), (walks, live_steps, est) in steps.items():   # the same calls without the index
        est0, st0 = g.fora_single_source(s, EPS, ALPHA, seed=3, n_rounds=n_rounds)
        assert st0.walks == walks and live_steps < st0.walk_steps, (name, s, n_rounds, live_steps, st0.walk_steps)
        assert_close(est, est0, TOL_MC, "overflow vs unindexed %s src=%d rounds=%d" % (name, s, n_rounds))


# ------------------------------------------------------------------ 4. a mismatch falls back
def test_other_seed_or_alpha_walks_as_before(pkg_product, orc, graphs, rmat12):
    g = graphs("rmat12")
    og = to_oracle(orc, rmat12)
    try:
        g.build_walk_index(ALPHA, seed=3)
        for s in live_sources(rmat12, 2, seed=29):
            for alpha, seed in ((ALPHA, 4), (0.3, 3)):
                g.walk_index_usage(reset=True)
                est, st = g.fora_single_source(s, EPS, alpha, seed=seed, n_rounds=2)
                assert g.walk_index_usage() == (0, 0)
                ref, sto = og.fora_whole(s, EPS, alpha, seed=seed, n_rounds=2, schedule=orc.SYNC)
                assert st.walks == sto.walks > 0 and st.walk_steps == sto.walk_steps
                assert_close(est, ref, TOL_MC, "fallback src=%d alpha=%g seed=%d" % (s, alpha, seed))
            est, st = g.fora_single_source(s, EPS, ALPHA, seed=3, n_rounds=2)     # and the index still serves its own
            assert g.walk_index_usage(reset=True) == (st.walks, 0)
    finally:
        g.drop_walk_index()


# ------------------------------------------------------------------ 5. every whole-graph path
def test_every_whole_graph_path_is_served(pkg_product, graphs, rmat15):
    pkg = pkg_product
    host = rmat15
    g = graphs("rmat15")
    srcs = np.array(live_sources(host, 35, seed=31), dtype=np.int32)
    sets = [live_sources(host, 1 + i % 4, seed=100 + i) for i in range(20)]
    seedset, weights = live_sources(host, 5, seed=41), [3.0, 1.0, 2.0, 0.5, 1.5]
    pair_s, pair_t = live_sources(host, 6, seed=43), live_sources(host, 6, seed=47)

    def whole_graph_paths(gr):
        out = {}
        out["fora_seeds"] = gr.fora_seeds(seedset, EPS, ALPHA, seed=3, weights=weights)[0]
        gr.set_tuning(pkg.tuning_batch())
        store = pkg.Results(gr, 40)
        try:
            _, ids, _, _, _, _ = gr.fora_batch_single_source(srcs, EPS, ALPHA, seed=3, k=8, keep=store)
            out["batch_single"] = np.stack([store.fetch(i) for i in range(srcs.size)])
            out["batch_single_ids"] = ids.copy()
            vec, ids, _, _, _, _ = gr.fora_batch_seeds(sets, EPS, ALPHA, seed=3, k=8, fetch=True)
            out["batch_seeds"] = vec
            out["batch_seeds_ids"] = ids.copy()
            with pkg.QueryStream(gr, EPS, ALPHA, k=8) as qs:
                t1 = qs.submit(srcs[:20], 3, keep=store)
                t2 = qs.submit(srcs[15:35], 3, keep=store, keep_first=20)
                ids1 = qs.wait(t1)[0].copy()
                ids2 = qs.wait(t2)[0].copy()
            out["stream"] = np.stack([store.fetch(i) for i in range(40)])
            out["stream_ids"] = np.concatenate([ids1, ids2])
        finally:
            store.close()
            gr.set_tuning(pkg.tuning_default())
        return out

    def other_paths(gr):
        out = {}
        nsel, ids, vals, est, _ = gr.fora_topk(int(srcs[0]), EPS, ALPHA, 8, seed=3, cap=16, fetch=True)
        out["topk"] = (nsel, ids, est)
        out["batch_topk"] = gr.fora_batch_topk(srcs[:20], 8, EPS, ALPHA, seed=3)[:2]
        out["mc"] = gr.monte_carlo(int(srcs[1]), EPS, ALPHA, seed=3)[0]
        out["pairs"] = gr.ppr_pairs(pair_s, pair_t, EPS, ALPHA, seed=3)[0]
        return out

    plain = whole_graph_paths(g)
    plain_other = other_paths(g)
    try:
        g.build_walk_index(ALPHA, seed=3)
        total = 0
        for name, call in (("fora_seeds", lambda: g.fora_seeds(seedset, EPS, ALPHA, seed=3, weights=weights)),):
            g.walk_index_usage(reset=True)
            est, st = call()
            served, walked = g.walk_index_usage(reset=True)
            assert served > 0 and served + walked == st.walks, name
            assert_close(est, plain["fora_seeds"], TOL_MC, name)
            total += served
        g.walk_index_usage(reset=True)
        idx = whole_graph_paths(g)
        served, walked = g.walk_index_usage(reset=True)
        print("batched paths: served %d walked %d" % (served, walked))
        assert served > 0
        for key in ("fora_seeds", "batch_single", "batch_seeds", "stream"):
            assert_close(idx[key], plain[key], TOL_MC, key)
        for key in ("batch_single_ids", "batch_seeds_ids", "stream_ids"):
            assert np.array_equal(idx[key], plain[key]), key
        # each batched path on its own: the counter moves
        g.set_tuning(pkg.tuning_batch())
        try:
            _, _, _, _, pq, stb = g.fora_batch_single_source(srcs, EPS, ALPHA, seed=3, k=8, per_query=True)
            s1, w1 = g.walk_index_usage(reset=True)
            assert s1 > 0 and s1 + w1 == stb.walks == sum(p.walks for p in pq)
            _, _, _, _, _, stb = g.fora_batch_seeds(sets, EPS, ALPHA, seed=3, k=8)
            s2, w2 = g.walk_index_usage(reset=True)
            assert s2 > 0 and s2 + w2 == stb.walks
            with pkg.QueryStream(g, EPS, ALPHA, k=8) as qs:
                t1 = qs.submit(srcs[:20], 3)
                t2 = qs.submit(srcs[15:35], 3)
                sw = qs.wait(t1)[3].walks + qs.wait(t2)[3].walks
            s3, w3 = g.walk_index_usage(reset=True)
            assert s3 > 0 and s3 + w3 == sw
        finally:
            g.set_tuning(pkg.tuning_default())
        # the paths that never read the index: counters untouched, results as on a handle without one
        g.walk_index_usage(reset=True)
        other = other_paths(g)
        assert g.walk_index_usage() == (0, 0)
        assert other["topk"][0] == plain_other["topk"][0] and np.array_equal(other["topk"][1], plain_other["topk"][1])
        assert_close(other["topk"][2], plain_other["topk"][2], TOL_MC, "fora_topk estimate")
        assert np.array_equal(other["batch_topk"][0], plain_other["batch_topk"][0])
        assert_close(other["batch_topk"][1], plain_other["batch_topk"][1], TOL_MC, "fora_batch_topk values")
        assert_close(other["mc"], plain_other["mc"], TOL_MC, "monte_carlo")
        assert_close(other["pairs"], plain_other["pairs"], TOL_MC, "ppr_pairs")
    finally:
        g.drop_walk_index()


def test_fora_batch_over_two_replicas(pkg_product, graphs, rmat15):
    """pprhip_fora_batch with two handles on the one GPU, each with an index of its own."""
    pkg = pkg_product
    srcs = np.array(live_sources(rmat15, 12, seed=53), dtype=np.int32)
    g1 = graphs("rmat15")
    with pkg.Graph(rmat15) as g2:
        ids0, vals0, nsel0, _ = pkg.fora_batch_multi([g1, g2], srcs, 8, EPS, ALPHA, seed=3)
        try:
            g1.build_walk_index(ALPHA, seed=3)
            g2.build_walk_index(ALPHA, seed=3)
            ids, vals, nsel, sts = pkg.fora_batch_multi([g1, g2], srcs, 8, EPS, ALPHA, seed=3)
            for g, st in ((g1, sts[0]), (g2, sts[1])):
                served, walked = g.walk_index_usage(reset=True)
                assert served > 0 and served + walked == st.walks
            assert np.array_equal(ids, ids0) and np.array_equal(nsel, nsel0)
            assert_close(vals, vals0, TOL_MC, "fora_batch over two replicas")
        finally:
            g1.drop_walk_index()


# ------------------------------------------------------------------ 6. indexed tuning
SERVED_WALK_NS = 0.136   # measured cost of a served walk (DESIGN.md 2 "Walk index"): what an indexed profile's c_walk_ns is


def _indexed_profiles(pkg):
    """The shipped profile, and the default profile with c_walk_ns at the measured cost of a served walk - the case an
    indexed profile exists for, whatever the shipped one is set to: a cheaper walk lets the push stop earlier."""
    low = pkg.tuning_default()
    low.c_walk_ns = SERVED_WALK_NS
    assert low.c_walk_ns < pkg.tuning_default().c_walk_ns
    return (("tuning_indexed", pkg.tuning_indexed()), ("c_walk_ns=%g" % SERVED_WALK_NS, low))


def test_indexed_tuning(pkg_product, orc, graphs, rmat12, rmat15):
    """Served queries under the shipped indexed profile and under a walk cost that is really lower.  Both must equal the
    twin under the same tuning (rounds, levels, walks, vector to 1e-9) and keep the (eps, delta) guarantee against the
    power method on R-MAT 15 at every node.  The level comparison with the default profile is asserted for
    tuning_indexed().  For the lowered cost it is printed, not asserted: the cost model compares modelled costs, not
    level counts, and a push that starts at a higher threshold can take more levels (measured: R-MAT 15 source 19182,
    32 + 14 dense levels at c_walk_ns = 0.136 against 30 + 11 at 0.35, the twin level for level the same; source 25778,
    15 + 9 against 21 + 12).  What the model does promise is asserted instead: the first round's threshold is rmax0
    halved while c_walk_ns * omega * (1 - alpha) * rmax * m >= the cost of prior_levels dense levels, a count that cannot
    grow when c_walk_ns falls - so where both runs take one round, the lowered cost ends at a threshold no lower, and
    the test requires that it is higher for at least one query (else the case it exists for did not occur)."""
    pkg = pkg_product
    higher = 0
    for name, host, count in (("rmat12", rmat12, 3), ("rmat15", rmat15, 3)):
        g = graphs(name)
        og = to_oracle(orc, host)
        delta = 1.0 / host.n
        try:
            g.build_walk_index(ALPHA, seed=3)
            for s in live_sources(host, count, seed=59):
                _, std = g.fora_single_source(s, EPS, ALPHA, seed=3, fetch=False)
                for tname, t in _indexed_profiles(pkg):
                    g.set_tuning(t)
                    g.walk_index_usage(reset=True)
                    est, st = g.fora_single_source(s, EPS, ALPHA, seed=3)
                    served, walked = g.walk_index_usage(reset=True)
                    g.set_tuning(pkg.tuning_default())
                    ref, sto = og.fora_whole(s, EPS, ALPHA, seed=3, n_rounds=0, schedule=orc.SYNC,
                                             tuning=to_orc_tuning(orc, t))
                    what = "%s src=%d %s" % (name, s, tname)
                    print("%s: rounds %d, rmax %.3g (default tuning %.3g), levels %d + %d dense (default %d + %d), walks %d "
                          "(default %d), served %d walked %d" % (what, st.rounds, st.rmax_final, std.rmax_final, st.levels,
                                                                 st.dense_levels, std.levels, std.dense_levels, st.walks,
                                                                 std.walks, served, walked))
                    assert st.rounds == sto.rounds and st.walks == sto.walks == served + walked, what
                    assert st.levels == sto.levels, what
                    assert_close(est, ref, TOL_MC, "indexed tuning vs twin " + what)
                    if tname == "tuning_indexed":
                        assert st.dense_levels + st.levels <= std.dense_levels + std.levels, what
                    if t.c_walk_ns < pkg.tuning_default().c_walk_ns and st.rounds == std.rounds == 1:
                        assert st.rmax_final >= std.rmax_final, what
                        higher += st.rmax_final > std.rmax_final
                    if name == "rmat15":
                        pi = og.power_method(s, ALPHA)
                        bound = EPS * np.maximum(pi, delta)
                        twin_out = int((np.abs(ref - pi) > bound).sum())
                        print("%s: nodes outside eps * max(pi, delta): twin %d, engine %d" % (
                            what, twin_out, int((np.abs(est - pi) > bound).sum())))
                        assert twin_out == 0, "the twin itself misses the (eps, delta) bound at %d nodes" % twin_out
                        assert np.all(np.abs(est - pi) <= bound), what
        finally:
            g.set_tuning(pkg.tuning_default())
            g.drop_walk_index()
    assert higher > 0, "a walk cost of %g ns never ended a push earlier: the case under test did not occur" % SERVED_WALK_NS


# ------------------------------------------------------------------ 7. lifecycle
def test_lifecycle(pkg_product, graphs, rmat12, rmat15):
    pkg = pkg_product
    g = graphs("rmat12")
    s = live_sources(rmat12, 1, seed=61)[0]
    try:
        g.build_walk_index(ALPHA, seed=3)
        first = g.walk_index_info()
        g.drop_walk_index()
        g.drop_walk_index()                                    # no-op without one
        assert g.walk_index_info() is None
        with pytest.raises(pkg.PprhipError) as e:
            g.walk_index_terminals(0)
        assert e.value.code == pkg.ERR_STATE
        g.build_walk_index(ALPHA, seed=3)
        assert g.walk_index_info() == first
        g.build_walk_index(0.3, seed=8, density=0.5)           # a second build replaces the first
        info = g.walk_index_info()
        assert (info["alpha"], info["seed"], info["density"]) == (0.3, 8, 0.5)
        d = np.diff(rmat12.out_rp)
        assert info["terminals"] == int(np.ceil(d * 0.5).sum())
        _, st = g.fora_single_source(s, EPS, 0.3, seed=8, n_rounds=1, fetch=False)
        served, walked = g.walk_index_usage(reset=True)
        assert served > 0 and served + walked == st.walks
        g.release(pkg.Graph.RELEASE_WALK_INDEX)                # PPRHIP_RELEASE_WALK_INDEX
        assert g.walk_index_info() is None
        with pytest.raises(pkg.PprhipError) as e:
            g.build_walk_index(ALPHA, seed=3, density=1e12)    # 2^36 terminals or more
        assert e.value.code == pkg.ERR_INVALID and g.walk_index_info() is None
        # a query stream owns the handle: a build is a call sequence error, and the index stays as it was
        g.build_walk_index(ALPHA, seed=3)
        with pkg.QueryStream(g, EPS, ALPHA, k=4) as qs:
            with pytest.raises(pkg.PprhipError) as e:
                g.build_walk_index(ALPHA, seed=4)
            assert e.value.code == pkg.ERR_STATE
            qs.wait(qs.submit([s], 3))
        assert g.walk_index_info() == first
    finally:
        g.drop_walk_index()
    # destroy with an index attached; device memory after twenty build / drop lives
    with pkg.Graph(rmat12) as probe:
        with pkg.Graph(rmat15) as g15:
            g15.build_walk_index(ALPHA, seed=3)                # (first life: code objects, allocator pools)
            g15.fora_single_source(s, EPS, ALPHA, seed=3, fetch=False)
        with pkg.Graph(rmat15) as g15:
            g15.build_walk_index(ALPHA, seed=3)
            g15.drop_walk_index()
            free0, _ = probe.device_memory()
            for i in range(20):
                g15.build_walk_index(ALPHA, seed=3 + i)
                if i % 2:
                    g15.drop_walk_index()
            g15.drop_walk_index()
            free1, _ = probe.device_memory()
            held = g15.build_walk_index(ALPHA, seed=3).walks * 4
        free2, _ = probe.device_memory()                       # the handle went with its index attached
    print("twenty build/drop lives: device %+.2f MB (one index: %.2f MB)" % ((free0 - free1) / 1e6, held / 1e6))
    assert free0 - free1 <= 64 << 20 and 20 * held > 64 << 20   # (a leak of one index per life would show)
    assert free2 >= free1


# ------------------------------------------------------------------ 8. full size
@pytest.mark.timeout(900)
def test_full_size_rmat22_walk_index(pkg_product):
    pkg = pkg_product
    host = pkg.HostCsr.rmat(22, 16, seed=1)
    conf = pkg.conf_whole_graph(host.n, host.m, ALPHA)
    rho = pkg.walk_index_density(conf, EPS)
    delta = 1.0 / host.n
    s = live_sources(host, 1, seed=62)[0]
    with pkg.Graph(host) as g:
        est0, st0 = g.fora_single_source(s, EPS, ALPHA, seed=5)
        stb = g.build_walk_index(ALPHA, seed=5)
        info = g.walk_index_info()
        print("R-MAT 22 walk index: density %.4f, %d terminals (bound %.0f), %.2f GB, built in %.1f ms (%d steps)" % (
            rho, info["terminals"], host.m * rho + host.n, info["bytes"] / 1e9, stb.mc_ms, stb.walk_steps))
        assert info["terminals"] <= host.m * rho + host.n
        est, st = g.fora_single_source(s, EPS, ALPHA, seed=5)
        served, walked = g.walk_index_usage()
        print("served query: walks %d served %d walked %d, mc_ms %.3f (unindexed %.3f)" % (st.walks, served, walked,
                                                                                         st.mc_ms, st0.mc_ms))
        assert st.walks == st0.walks == served + walked and served > 0 and st.rounds == st0.rounds
        assert_close(est, est0, TOL_MC, "served vs unindexed at R-MAT 22")
        pi, _ = g.power_method(s, ALPHA, 100)
        assert np.all(np.abs(est - pi) <= EPS * np.maximum(pi, delta))
