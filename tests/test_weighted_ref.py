"""The weighted calls' host references (tests/weighted_ref.py) pinned on the CPU, independently of the engine, and the
host half of the weights (pprhip_weight_table_host): integer weights against the multigraph, the exact push invariant,
powers of two against the oracle's unweighted twin, the walk against oracle.random_walk, the prefix rule bit for bit."""
import numpy as np
import pytest

import weighted_ref as wr
from conftest import edges_to_host, to_oracle
from targets_ref import ppr_exact as ppr_exact_unweighted

ALPHA = 0.15


def _edges(host):
    src = np.repeat(np.arange(host.n), np.diff(host.out_rp.astype(np.int64)))
    return src, host.out_ci[:host.m].astype(np.int64)


def _graphs(got, toy_graphs):
    g = dict(toy_graphs)
    g["got"] = got
    return g


def _restart_matrix(host, w, s, alpha):
    """M[v] = the PPR vector of the walk that starts at v, stops with probability alpha per step and jumps to s at a dead
    end: alpha (I - (1 - alpha) Q)^-1 with Q = P and the dead-end rows pointing at s.  Row s is pi_s; the other rows are
    what a residue r(v) of a push from s still owes."""
    Q = wr.transition(host, w)
    dead = np.diff(host.out_rp.astype(np.int64)) == 0
    Q[dead, s] = 1.0
    return alpha * np.linalg.inv(np.eye(host.n) - (1.0 - alpha) * Q)


def test_integer_weights_are_the_multigraph(pkg, got, toy_graphs):
    """ppr_exact with integer weights = the unweighted ppr_exact on the graph with each relationship repeated that many
    times."""
    rng = np.random.default_rng(11)
    for name, host in _graphs(got, toy_graphs).items():
        w = rng.integers(1, 5, host.m).astype(np.float64)
        src, dst = _edges(host)
        rep = w.astype(np.int64)
        multi = edges_to_host(pkg, host.n, list(zip(np.repeat(src, rep).tolist(), np.repeat(dst, rep).tolist())))
        a = wr.ppr_exact(host, w, ALPHA)
        b = ppr_exact_unweighted(multi, ALPHA)
        assert np.max(np.abs(a - b)) <= 1e-12, name


@pytest.mark.parametrize("rmax", [1e-2, 1e-5])
def test_push_invariant_and_threshold(got, toy_graphs, rmax):
    """pi_s = reserve + sum_v r(v) pi_v, exactly: pi_v is the walk from v that restarts at s (the dead-end mass of a push
    from s lands on s), and row s of that solve is ppr_exact's row s.  Every r / d < rmax at the end."""
    rng = np.random.default_rng(5)
    for name, host in _graphs(got, toy_graphs).items():
        w = rng.uniform(0.5, 1.5, host.m)
        pi = wr.ppr_exact(host, w, ALPHA)
        deg = np.diff(host.out_rp.astype(np.int64))
        srcs = range(host.n) if host.n <= 8 else [int(np.argmax(deg)), int(np.argmin(deg)), 17, 42]
        for s in srcs:
            M = _restart_matrix(host, w, s, ALPHA)
            assert np.max(np.abs(M[s] - pi[s])) <= 1e-12, (name, s)
            reserve, residue, levels, pops = wr.push_sync(host, w, s, ALPHA, rmax)
            assert np.max(np.abs(M[s] - (reserve + residue @ M))) <= 1e-12, (name, s)
            if deg[s] == 0:
                assert reserve[s] == 1.0 and levels == 0 and pops == 0
            else:
                assert not wr.active(residue, deg, rmax).any(), (name, s)
                assert abs(reserve.sum() + residue.sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("weight", [4.0, 0.25])
def test_power_of_two_weights_are_the_unweighted_push(orc, got, toy_graphs, rmat12, weight):
    """Every weight one power of two: every product of the weighted rule is exact, so push_sync is the oracle's
    frontier-synchronous forward push under plain Jacobi sweeps (gs_blocks = 1)."""
    t = orc.tuning_default()
    t.gs_blocks = 1
    orc.set_sync_tuning(t)
    try:
        graphs = _graphs(got, toy_graphs)
        graphs["rmat12"] = rmat12
        for name, host in graphs.items():
            og = to_oracle(orc, host)
            deg = np.diff(host.out_rp.astype(np.int64))
            w = np.full(host.m, weight)
            for s in sorted({0, host.n - 1, int(np.argmax(deg)), int(np.argmin(deg))}):
                for rmax in (1e-3, 1e-6):
                    p, r, _, st = og.forward_push(s, ALPHA, rmax)
                    reserve, residue, levels, pops = wr.push_sync(host, w, s, ALPHA, rmax)
                    assert levels == st.levels and pops == st.pops + st.dense_nodes, (name, s, rmax)
                    assert np.max(np.abs(reserve - p)) <= 1e-12 and np.max(np.abs(residue - r)) <= 1e-12, (name, s, rmax)
    finally:
        orc.set_sync_tuning(None)


def _pow2_graph(pkg):
    """96 nodes, out-degrees 0 (dead ends), 1, 2, 4, 8, 16 and 32, targets anywhere (dead ends included)."""
    rng = np.random.default_rng(7)
    n = 96
    degs = rng.choice([0, 1, 2, 4, 8, 16, 32], n)
    degs[:7] = [0, 1, 2, 4, 8, 16, 32]
    edges = [(u, int(v)) for u in range(n) for v in rng.integers(0, n, degs[u])]
    return edges_to_host(pkg, n, edges)


def test_numpy_philox_is_the_oracles(orc):
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 1 << 32, (64, 4), dtype=np.uint64)
    key = (0x9ABCDEF012345678 & 0xFFFFFFFF, 0x9ABCDEF012345678 >> 32)
    out = wr.philox_np(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[0], key[1])
    for i in range(64):
        ref = orc.philox(ctr[i].tolist(), list(key))
        assert [int(out[j][i]) for j in range(4)] == [int(x) for x in ref]


@pytest.mark.parametrize("no_zero_hop", [False, True])
def test_walk_is_the_oracles_walk_on_unit_weights(pkg, orc, no_zero_hop):
    """Out-degrees all powers of two and unit weights: word * d is exact, the prefix is 1 .. d, so the weighted pick is
    (word * d) >> 32 and walk() must be oracle.random_walk bit for bit - dead-end starts and dead-end restarts included."""
    host = _pow2_graph(pkg)
    og = to_oracle(orc, host)
    tab = wr.table(host, np.ones(host.m))
    seed = 0x1234567887654321
    starts = np.tile(np.arange(host.n, dtype=np.int32), 40)
    idx = (np.arange(starts.size, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 40)
    for stream in (0, 3):
        term_o, steps_o = og.random_walks(starts, idx, 0.2, seed, stream, no_zero_hop)
        term, steps = wr.walks(host, tab, starts, idx, 0.2, seed, stream, no_zero_hop)
        assert np.array_equal(term, term_o) and np.array_equal(steps, steps_o)
        for i in range(0, starts.size, 29):  # the scalar rule, on oracle.philox
            t, k = wr.walk(orc, host, tab, int(starts[i]), 0.2, seed, stream, int(idx[i]), no_zero_hop)
            assert (t, k) == (int(term_o[i]), int(steps_o[i]))
    assert steps_o.max() > 20 and (np.diff(host.out_rp)[term_o] == 0).any()  # long walks and dead ends were met


def test_vector_walks_are_the_scalar_walk_on_real_weights(pkg, orc, got):
    rng = np.random.default_rng(2)
    w = rng.uniform(0.5, 1.5, got.m)
    tab = wr.table(got, w)
    starts = rng.integers(0, got.n, 300).astype(np.int32)
    idx = rng.integers(0, 1 << 40, 300).astype(np.uint64)
    term, steps = wr.walks(got, tab, starts, idx, ALPHA, 77, 0, True)
    for i in range(300):
        assert wr.walk(orc, got, tab, int(starts[i]), ALPHA, 77, 0, int(idx[i]), True) == (int(term[i]), int(steps[i]))


def test_host_table_is_the_sequential_prefix(pkg):
    """pprhip_weight_table_host = per-row np.cumsum, bit for bit: rows of 0, 1, 2, 64, 65 and 5 000 entries, weights
    spanning 1e-300 .. 1e300 within one row."""
    rng = np.random.default_rng(3)
    lens = [1, 0, 2, 64, 65, 5000, 3]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    w = 10.0 ** rng.uniform(-300, 300, int(rp[-1]))
    cum, ws = pkg.weight_table_host(rp, w)
    for u, k in enumerate(lens):
        b, e = int(rp[u]), int(rp[u + 1])
        ref = np.cumsum(w[b:e])
        assert np.array_equal(cum[b:e], ref), u
        assert ws[u] == (ref[-1] if k else 0.0) and np.isfinite(ws[u])
    assert ws[5] > 1e299


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 0.0, -1.0])
def test_bad_weights_are_refused_with_the_edge_named(pkg, bad):
    rp = np.array([0, 3, 3, 7], dtype=np.uint32)
    w = np.ones(7)
    w[5] = bad
    with pytest.raises(pkg.PprhipError, match=r"edge 5 \(out of node 2\)") as ei:
        pkg.weight_table_host(rp, w)
    assert ei.value.code == pkg.ERR_INVALID


def test_overflowing_row_sum_is_refused_with_the_node_named(pkg):
    rp = np.array([0, 1, 4], dtype=np.uint32)
    w = np.array([1.0, 1e308, 1e308, 1e308])
    with pytest.raises(pkg.PprhipError, match="node 1") as ei:
        pkg.weight_table_host(rp, w)
    assert ei.value.code == pkg.ERR_INVALID


def test_designed_graphs_have_their_designed_layout(pkg):
    """tests/weighted_designs.py against the host lift: the dense design's in-rows sit at the chunk edges they are meant
    for, the sparse design's sources have the degrees they are named by."""
    from weighted_designs import CHUNK, dense_design, sparse_design
    host, d = dense_design(pkg)
    L = pkg.lift_host(host)
    o2n, irp = L["old2new"], L["in_rp"].astype(np.int64)
    assert [int(o2n[d[k]]) for k in "ABC"] == [0, 1, 2]
    assert irp[1] == CHUNK and irp[2] == 2 * CHUNK + 1 and irp[3] == irp[2] + 1100  # B starts on the boundary
    assert irp[2] // CHUNK == irp[1] // CHUNK + 1 and (irp[3] - 1) // CHUNK == irp[2] // CHUNK + 2
    assert host.m % CHUNK != 0 and host.m // CHUNK >= 4
    assert L["zin_rows"].size >= len(d["pool"]) and set(d["pool"]) <= set(L["new2old"][L["zin_rows"]].tolist()) and host.out_rp[d["dead"] + 1] == host.out_rp[d["dead"]]
    assert host.out_rp[d["isolated"] + 1] == host.out_rp[d["isolated"]] and host.in_rp[d["isolated"] + 1] == host.in_rp[d["isolated"]]
    hs, by_deg = sparse_design(pkg)
    deg = np.diff(hs.out_rp.astype(np.int64))
    assert all(deg[u] == k for k, u in by_deg.items()) and (deg[8:] == 0).any()
