"""Seed sets, engine against twin (DESIGN §3 "engine ≡ twin"): pprhip_forward_push_seeds, pprhip_fora_seeds and
pprhip_fora_topk_seeds against orc_forward_push_seeds, orc_fora_whole_seeds and orc_fora_topk_seeds, level for level:
the same level counters and vectors to 1e-12 for the push, the check_fora rule for FORA, the same selection for top-k.
Every level shape (sparse only, dense only, mixed; Jacobi and 2-, 3- and 6-block Gauss-Seidel sweeps), the row-panel,
sliced and row-major copies of the in-CSR, the seed table's growth past 1 024 entries, and one handle running large
sets, small sets and single-source queries in turn."""
import numpy as np
import pytest

from conftest import to_oracle
from test_gpu_fuzz import check_fora, orc_tuning, random_graph
from test_seeds import exact_invariant_err, seed_p

pytestmark = pytest.mark.gpu

A = 0.15
EPS = 0.5
TOL_PUSH = 1e-12
TOL_MC = 1e-9
PUSH_COUNTERS = ("levels", "dense_levels", "pops", "dead_end_pops", "enqueues")
SHAPES = [(1e9, 1), (1e-9, 1), (1e-9, 2), (1e-9, 3), (1e-9, 6), (None, 2)]  # (dense_frac, gs_blocks); None: default


def kinds(host):
    dout = np.diff(np.asarray(host.out_rp, dtype=np.int64))
    din = np.diff(np.asarray(host.in_rp, dtype=np.int64))
    return np.nonzero(dout > 0)[0], np.nonzero(dout == 0)[0], np.nonzero((dout > 0) & (din == 0))[0]


def seed_sets(host, seed, sizes=(2, 3, 12, 60), half=True, every=True):
    """Named sets: the given sizes (a dead end, a node without in-edges, a duplicate and a zero weight among them),
    n/2, every node, one live seed among many dead ends (D -> 1), weights from 1e-12 to 1."""
    live, dead, zin = kinds(host)
    rng = np.random.default_rng(seed)
    out = {}
    for k in [k for k in sizes if k <= host.n] + ([host.n // 2] if half and host.n >= 4 else []):
        s = rng.choice(host.n, size=k, replace=False).astype(np.int32)
        if zin.size and k >= 3:
            s[0] = zin[0]
        if dead.size:
            s[-1] = dead[0]
        w = rng.uniform(0.1, 1.0, size=k)
        if k >= 3:
            s = np.concatenate([s, s[1:2], s[2:3]])
            w = np.concatenate([w, [0.25, 0.0]])
        out["k%d" % k] = (s, w)
    if every:
        out["all"] = (np.arange(host.n, dtype=np.int32), None)
    if live.size and dead.size >= 2:
        s = np.concatenate([live[:1], dead[:200]]).astype(np.int32)
        out["D~1"] = (s, np.concatenate([[1e-3], np.ones(s.size - 1)]))
    if live.size >= 3:
        s = rng.choice(live, size=min(8, live.size), replace=False).astype(np.int32)
        out["span"] = (s, 10.0 ** -rng.uniform(0, 12, size=s.size))
    return out


def set_shape(pkg, dev, dense_frac, blocks):
    t = pkg.tuning_default()
    if dense_frac is not None:
        t.dense_frac = dense_frac
    t.gs_blocks = blocks
    dev.set_tuning(t)  # (the conftest patch hands it to the twin's push and top-k as well)
    return t


def same_push(host, dev, og, s, w, rmax, what, exact=False):
    p, r, rsum, st = dev.forward_push_seeds(s, A, rmax, weights=w)
    po, ro, rso, sto = og.forward_push_seeds(s, A, rmax, weights=w)
    for f in PUSH_COUNTERS:
        assert getattr(st, f) == getattr(sto, f), (what, f, getattr(st, f), getattr(sto, f))
    assert np.max(np.abs(p - po), initial=0) <= TOL_PUSH, (what, "reserve", float(np.max(np.abs(p - po))))
    assert np.max(np.abs(r - ro), initial=0) <= TOL_PUSH, (what, "residue", float(np.max(np.abs(r - ro))))
    assert abs(rsum - rso) <= TOL_PUSH, what
    if exact:
        assert exact_invariant_err(host, seed_p(host.n, s, w), p, r, A) <= TOL_PUSH, what
    return st


def same_fora(dev, og, orc, t, s, w, n_rounds, what):
    est, st = dev.fora_seeds(s, EPS, A, seed=7, weights=w, n_rounds=n_rounds)
    ref, sto = og.fora_whole_seeds(s, EPS, A, seed=7, weights=w, n_rounds=n_rounds, tuning=orc_tuning(orc, t))
    check_fora(est, st, ref, sto, what)
    return st


def same_topk(host, dev, og, orc, s, w, k, what):
    """The twin's top-k: same rounds, estimates to TOL_MC, the same ids in the same order and the same n_sel.  Where the
    twin's estimate holds values within TOL_MC of each other (symmetric nodes of small graphs), the engine's order of
    them is accepted if it is the selection rule applied to its own estimate."""
    nsel, ids, vals, est, st = dev.fora_topk_seeds(s, EPS, A, k, seed=9, weights=w, cap=host.n, fetch=True)
    ref, sto = og.fora_topk_seeds(s, EPS, A, k, seed=9, weights=w)
    assert st.rounds == sto.rounds, what
    cnt_e, ids_e, vals_e = orc.topk(est, k, cap=host.n)
    assert nsel == cnt_e and list(ids) == list(ids_e) and np.array_equal(vals, vals_e), what
    if st.walks != sto.walks:  # a walk count on an integer boundary (check_fora's reason): the selection rule only
        assert abs(int(st.walks) - int(sto.walks)) <= 2, (what, st.walks, sto.walks)
        return st
    assert np.max(np.abs(est - ref), initial=0) <= TOL_MC, (what, float(np.max(np.abs(est - ref), initial=0)))
    cnt, oids, ovals = orc.topk(ref, k, cap=host.n)
    if nsel == cnt and list(ids) == list(oids):
        return st
    near = lambda x: np.sum(np.abs(ref - x) <= TOL_MC) > 1  # noqa: E731
    assert nsel == cnt or near(ovals[min(k, cnt) - 1]), (what, nsel, cnt)
    for i, (a, b) in enumerate(zip(ids, oids)):
        assert a == b or (abs(ref[a] - ref[b]) <= TOL_MC and near(ref[b])), (what, i, a, b)
    return st


def run_all(pkg, orc, host, dev, og, sets, shapes, rmaxes=(1e-3, 1e-6, 1e-9), rounds=(1, 2, 4, 0), ks=(1, 10, 50),
            fora_shapes=None, name=""):
    exact = host.n <= 4096
    seen = {"dense": 0, "sparse_only": 0}
    try:
        for frac, B in shapes:
            t = set_shape(pkg, dev, frac, B)
            full = fora_shapes is None or (frac, B) in fora_shapes
            for sname, (s, w) in sets.items():
                what = (name, frac, B, sname)
                for rmax in rmaxes:
                    st = same_push(host, dev, og, s, w, rmax, what + (rmax,), exact)
                    seen["dense"] += st.dense_levels
                    if frac == 1e9:
                        assert st.dense_levels == 0
                        seen["sparse_only"] += st.levels
                if full:
                    for n_rounds in rounds:
                        same_fora(dev, og, orc, t, s, w, n_rounds, what + ("fora", n_rounds))
                    for k in ks:
                        same_topk(host, dev, og, orc, s, w, k, what + ("topk", k))
    finally:
        dev.set_tuning(pkg.tuning_default())
    return seen


# ------------------------------------------------------------------ graphs x sets x level shapes
@pytest.mark.parametrize("graph", ["got", "toys", "rmat12", "rmat15"])
def test_seed_sets_against_twin(pkg, orc, got, toy_graphs, rmat12, rmat15, graph):
    if graph == "toys":
        hosts = sorted(toy_graphs.items())
    else:
        hosts = [(graph, {"got": got, "rmat12": rmat12, "rmat15": rmat15}[graph])]
    for name, host in hosts:
        og = to_oracle(orc, host)
        sets = seed_sets(host, 3)
        shapes, fora_shapes = SHAPES, None
        if graph == "rmat15":  # (the twin's levels cost CPU time here: FORA and top-k on three shapes)
            sets = {k: v for k, v in sets.items() if k in ("k3", "k60", "k16384", "all", "D~1", "span")}
            fora_shapes = [(1e9, 1), (1e-9, 3), (None, 2)]
        with pkg.Graph(host) as dev:
            seen = run_all(pkg, orc, host, dev, og, sets, shapes, fora_shapes=fora_shapes, name=name)
        if host.m:
            assert seen["dense"] > 0 and seen["sparse_only"] > 0, name


@pytest.mark.parametrize("seed", range(12))
def test_random_graph_seed_sets_against_twin(pkg, orc, seed):
    """The fuzz graphs of test_gpu_fuzz (the empty graph, self loops only, multi-edges, isolated nodes, dead ends)."""
    host = random_graph(pkg, seed)
    og = to_oracle(orc, host)
    sets = seed_sets(host, 100 + seed, sizes=(2, 3, 12))
    with pkg.Graph(host) as dev:
        run_all(pkg, orc, host, dev, og, sets, [(1e9, 1), (1e-9, 1), (1e-9, 2), (1e-9, 3), (0.05, 1)],
                rmaxes=(1e-2, 1e-6), rounds=(1, 0), ks=(1, 3), name="fuzz%d" % seed)


# ------------------------------------------------------------------ the copies of the in-CSR a sweep walks
@pytest.mark.parametrize("graph", ["got", "rmat12", "rmat15"])
def test_seed_sets_row_panel_copy(pkg, orc, got, rmat12, rmat15, graph, monkeypatch):
    """The row-panel copy (PPRHIP_SWEEP1_PANELS=1; by default from 2^26 edges on): live seeds land in k_dense_apply's
    panel form, seeds without in-edges as extra rows behind the last block; on a handle that ran queries before."""
    host = {"got": got, "rmat12": rmat12, "rmat15": rmat15}[graph]
    og = to_oracle(orc, host)
    monkeypatch.setenv("PPRHIP_SWEEP1_PANELS", "1")
    sets = seed_sets(host, 7, sizes=(3, 60), half=graph != "rmat15", every=graph == "got")
    if graph == "rmat15":
        sets["k2000"] = (np.random.default_rng(5).choice(host.n, size=2000, replace=False).astype(np.int32), None)
    with pkg.Graph(host) as dev:
        seen = run_all(pkg, orc, host, dev, og, sets, [(1e-9, 1), (1e-9, 2), (1e-9, 3), (1e-9, 6), (0.002, 2)],
                       rmaxes=(1e-6, 1e-9), rounds=(2, 0), ks=(10,), fora_shapes=[(1e-9, 3), (0.002, 2)], name=graph)
    assert seen["dense"] > 0


@pytest.mark.parametrize("layout", ["sliced", "row_major"])
def test_seed_sets_sliced_and_row_major_copies(pkg, orc, rmat15, layout, monkeypatch):
    """The sliced copy (PPRHIP_SLICE_IDS=1000: 33 slices of source ids) and the row-major one (PPRHIP_SLICED=0) at
    R-MAT 15, with a set of 2 000 distinct seeds that grows the seed table past its first 1 024 entries."""
    og = to_oracle(orc, rmat15)
    if layout == "sliced":
        monkeypatch.setenv("PPRHIP_SLICE_IDS", "1000")
    else:
        monkeypatch.setenv("PPRHIP_SLICED", "0")
    sets = seed_sets(rmat15, 8, sizes=(3, 60), half=False, every=False)
    sets["k2000"] = (np.random.default_rng(6).choice(rmat15.n, size=2000, replace=False).astype(np.int32),
                     np.random.default_rng(7).uniform(0.0, 1.0, size=2000))
    with pkg.Graph(rmat15) as dev:
        seen = run_all(pkg, orc, rmat15, dev, og, sets, [(1e-9, 1), (1e-9, 2), (1e-9, 3), (0.002, 2)],
                       rmaxes=(1e-6, 1e-9), rounds=(2, 0), ks=(10,), fora_shapes=[(1e-9, 3), (0.002, 2)],
                       name=layout)
    assert seen["dense"] > 0


# ------------------------------------------------------------------ one handle, one query after the other
@pytest.mark.parametrize("graph", ["rmat12", "rmat15"])
def test_seed_handle_history(pkg, orc, rmat12, rmat15, graph):
    """A large set, a small one, a large one again (past 1 024 seeds: the table grows), a single-source query, then a
    set again, on one handle: each against the twin, so stale landing weights, done counters, parked or armed flags
    from the query before would show."""
    host = {"rmat12": rmat12, "rmat15": rmat15}[graph]
    og = to_oracle(orc, host)
    rng = np.random.default_rng(12)
    live, dead, zin = kinds(host)
    big = rng.choice(host.n, size=host.n // 2, replace=False).astype(np.int32)
    small = np.array([zin[0], live[3], dead[0]], dtype=np.int32)
    big2 = rng.choice(host.n, size=1500, replace=False).astype(np.int32)
    src = int(live[5])
    with pkg.Graph(host) as dev:
        for frac, B in ((0.002, 3), (None, 2)):
            t = set_shape(pkg, dev, frac, B)
            for i, s in enumerate((big, small, big2, None, small, big)):
                what = (graph, frac, B, i)
                if s is None:
                    p, r, _, st = dev.forward_push(src, A, 1e-8)
                    po, ro, _, sto = og.forward_push(src, A, 1e-8, orc.SYNC)
                    assert st.levels == sto.levels and np.max(np.abs(p - po)) <= TOL_PUSH, what
                    est, st = dev.fora_single_source(src, EPS, A, seed=7, n_rounds=0)
                    ref, sto = og.fora_whole(src, EPS, A, seed=7, n_rounds=0, schedule=orc.SYNC,
                                             tuning=orc_tuning(orc, t))
                    check_fora(est, st, ref, sto, what)
                    n0, i0, _, e0, st0 = dev.fora_topk(src, EPS, A, 10, seed=9, cap=host.n, fetch=True)
                    reft, stot = og.fora_topk(src, EPS, A, 10, seed=9, schedule=orc.SYNC)
                    assert st0.rounds == stot.rounds, what
                    continue
                w = rng.uniform(0.1, 1.0, size=s.size)
                same_push(host, dev, og, s, w, 1e-8, what, exact=host.n <= 4096)
                same_fora(dev, og, orc, t, s, w, 0, what + ("fora",))
                same_topk(host, dev, og, orc, s, w, 10, what + ("topk",))
        dev.set_tuning(pkg.tuning_default())
