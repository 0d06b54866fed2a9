"""The resumable top-k push (pprhip_fwdpush_topk_reset / _round) on the designed graphs of tests/topk_round_designs.py:
the parked set, the armed bits and the round-start rule at thread-group, armed-byte, armed-word, tile and scalar-tail
positions of k_seed_list_topk (kernels_frontier.hip), armed joins through take_armed in push_finish (kernels_push.hip:
the one-workgroup kernel, the two-launch level, the LDS-table path), in k_dense_apply<kFwdTopk> (kernels_dense.hip) and,
under fora_batch_topk, in take_armed_slot (kernels_dense_batch.hip).

Every design is exact (alpha = 0.5, dyadic values; tests/test_topk_round_designs.py proves it on the CPU), so after every
round both vectors are compared with the plain reference bit for bit, the residue sum and all seven counters for
equality:

  a  every design on a handle of its own (ids kept, the design's dense_frac, one Gauss-Seidel block), the whole sequence
     three times: as the library decides, with the LDS table on every level, with the table on none - the same bytes each
     time, so no armed bit or flag survives a reset
  b  every design against the oracle twin at the default tuning (two Gauss-Seidel blocks, which the plain reference does
     not model), on a relabelled handle, bit for bit
  c  every design without the one-workgroup kernel: PPRHIP_SPARSE_WG is read once per process, so one child process
     (tests/fixtures/topk_round_child.py) runs them all with PPRHIP_SPARSE_WG=0; without it designs this small only ever
     reach the one-workgroup kernel
  d  whole queries on the n = 2 * 2048 + 5 design: fora_topk, fora_batch_topk (every level dense) and the query stream
     against the twin at the matching seeds, with the plain reference showing that the rounds the calls ran armed nodes

Not covered, not reachable from the product: k_count_active<1> and k_seed_dense<1> (seed_scan returns before them for
seed kind 1), and k_seed_list<1>, which runs only under the measurement switch PPRHIP_TOPK_OLD_PASSES."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import topk_round_designs as T
from conftest import HOOKS_LIB, ROOT, to_oracle
from sparse_ref import same_bits
from test_gpu_sparse_level_designs import close_handle, open_handle

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]   # the table, relabel and one-workgroup switches are test hooks

ALL = list(T.all_designs().values())
A = T.ALPHA


def device_rounds(g, d):
    """[(reserve, residue, rsum, counters)] of the design's rounds, from a reset."""
    out = []
    g.topk_push_reset(d.start, A)
    for mn, rm in d.rounds:
        rsum, st = g.topk_push_round(mn, rm)
        out.append((g.reserve(), g.residue(), rsum, {k: int(getattr(st, k)) for k in T.COUNTERS}))
    return out


def check_against_reference(d, got, what):
    ref = T.run(d)
    assert len(got) == len(ref)
    for i, ((p, r, rsum, counters), R) in enumerate(zip(got, ref)):
        pe, re_ = R.vector("reserve", d.n), R.vector("residue", d.n)
        bad = np.flatnonzero(r.view(np.uint64) != re_.view(np.uint64))
        print("%s %s round %d: %s rsum %r, %d residues and %d reserves differ"
              % (d.name, what, i, counters, rsum, bad.size, int(np.sum(p.view(np.uint64) != pe.view(np.uint64)))))
        assert counters == R.totals(), (d, what, i, counters, R.totals())
        assert bad.size == 0, (d, what, i, bad[:8], r[bad[:8]], re_[bad[:8]])
        assert same_bits(r, re_) and same_bits(p, pe), (d, what, i)
        assert rsum == R.rsum, (d, what, i, rsum, R.rsum)


def same_bytes(a, b):
    return all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2:] == y[2:]
               for x, y in zip(a, b)) and len(a) == len(b)


# ------------------------------------------------------------------ a. every design, round by round, bit for bit
@pytest.mark.parametrize("d", ALL, ids=repr)
def test_rounds_equal_the_reference(pkg, monkeypatch, d):
    print(T.summary(d))
    g = open_handle(pkg, d)
    try:
        monkeypatch.delenv("PPRHIP_COMB_MIN_EDGES", raising=False)
        first = device_rounds(g, d)
        check_against_reference(d, first, "default")
        for what, value in (("table on", T.COMB_ON), ("table off", T.COMB_OFF)):
            monkeypatch.setenv("PPRHIP_COMB_MIN_EDGES", value)
            again = device_rounds(g, d)
            check_against_reference(d, again, what)
            assert same_bytes(again, first), (d, what)
    finally:
        close_handle(pkg, g)


# ------------------------------------------------------------------ b. the twin at the default tuning
@pytest.mark.parametrize("d", ALL, ids=repr)
def test_rounds_equal_the_twin_at_default_tuning(pkg, orc, d):
    g = pkg.Graph(d.host(pkg))
    try:
        t = pkg.tuning_default()
        assert t.gs_blocks == 2
        t.dense_frac = d.dense_frac
        g.set_tuning(t)                      # (the twin follows every set_tuning)
        tw = to_oracle(orc, d.host(pkg)).topk_push(d.start, A, orc.SYNC)
        g.topk_push_reset(d.start, A)
        for i, (mn, rm) in enumerate(d.rounds):
            rsum, st = g.topk_push_round(mn, rm)
            rsum_o, sto = tw.round(mn, rm)
            c, co = ({k: int(getattr(s, k)) for k in T.COUNTERS} for s in (st, sto))
            print("%s twin round %d: %s" % (d.name, i, c))
            assert c == co, (d, i, c, co)
            assert rsum == rsum_o, (d, i, rsum, rsum_o)
            assert same_bits(g.reserve(), tw.reserve) and same_bits(g.residue(), tw.residue), (d, i)
    finally:
        close_handle(pkg, g)


# ------------------------------------------------------------------ c. without the one-workgroup kernel
def child_main(pkg, out_path):
    """The child's half: every design's rounds on the library as it finds it."""
    out = {}
    for d in ALL:
        g = open_handle(pkg, d)
        for i, (p, r, rsum, counters) in enumerate(device_rounds(g, d)):
            key = "%s__%d" % (d.name, i)
            out[key + "__p"], out[key + "__r"] = p, r
            out[key + "__c"] = np.array([counters[k] for k in T.COUNTERS], dtype=np.int64)
            out[key + "__rsum"] = np.array([rsum])
        g.close()
    np.savez(out_path, **out)


def test_without_the_one_workgroup_kernel(pkg, tmp_path):
    out = str(tmp_path / "no_wg.npz")
    env = dict(os.environ, PPRHIP_SPARSE_WG="0", PPRHIP_LIB_PATH=HOOKS_LIB)
    env.pop("PPRHIP_COMB_MIN_EDGES", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fixtures", "topk_round_child.py"), out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-3000:])
    theirs = np.load(out)
    for d in ALL:
        got = []
        for i in range(len(d.rounds)):
            key = "%s__%d" % (d.name, i)
            got.append((theirs[key + "__p"], theirs[key + "__r"], float(theirs[key + "__rsum"][0]),
                        dict(zip(T.COUNTERS, (int(x) for x in theirs[key + "__c"])))))
        check_against_reference(d, got, "two launches")


# ------------------------------------------------------------------ d. whole queries
WQ = T.whole_query_design()
WQ_SOURCES = (3, 257, 2052, 4096)      # T nodes of the first, second and last tile of the round-start pass
WQ_K, WQ_EPS, WQ_SEED = 128, 0.5, 9


def armed_rounds(pkg, d, src, n_rounds):
    """The plain reference over the thresholds of the first n_rounds rounds of fora_topk(src): [(below, armed joins)]."""
    conf = pkg.conf_topk(d.n, d.m, WQ_K, A)
    th, delta = [], conf.delta
    for _ in range(n_rounds):
        mn, rm, _ = pkg.fora_topk_params(conf, WQ_EPS, delta)
        th.append((mn, rm))
        delta = max(conf.min_delta, delta / 4.0)
    d2 = copy.copy(d)
    d2.start = src
    rs = T.rounds(d2, th)
    print(T.summary(d2, rs))
    return [(R.below, R.armed_joins) for R in rs]


def twin_topk(pkg, orc, i, s):
    est, st = to_oracle(orc, WQ.host(pkg)).fora_topk(s, WQ_EPS, A, WQ_K, seed=WQ_SEED + i, schedule=orc.SYNC)
    return est, st


def test_fora_topk_equals_the_twin(pkg, orc):
    g = open_handle(pkg, WQ)
    try:
        t = pkg.tuning_default()
        t.gs_blocks = 1                      # (ids kept: the handle is not relabelled and sweeps are plain)
        g.set_tuning(t)
        for i, s in enumerate(WQ_SOURCES):
            nsel, ids, vals, est, st = g.fora_topk(s, WQ_EPS, A, WQ_K, seed=WQ_SEED + i, cap=WQ_K, fetch=True)
            ref, sto = twin_topk(pkg, orc, i, s)
            worst = float(np.max(np.abs(est - ref)))
            print("fora_topk src %d: rounds %d (twin %d), walks %d (twin %d), dense levels %d, largest difference %.3e"
                  % (s, st.rounds, sto.rounds, st.walks, sto.walks, st.dense_levels, worst))
            assert (st.rounds, st.walks) == (sto.rounds, sto.walks), s
            assert worst <= 1e-9, (s, worst)
            assert any(below and joins > 0 for below, joins in armed_rounds(pkg, WQ, s, st.rounds)), s
    finally:
        close_handle(pkg, g)


def test_fora_batch_topk_equals_the_twin(pkg, orc):
    g = open_handle(pkg, WQ)
    try:
        t = pkg.tuning_batch()
        t.gs_blocks, t.dense_frac = 1, 1e-9  # every level a sweep
        g.set_tuning(t)
        ids, vals, st = g.fora_batch_topk(np.array(WQ_SOURCES, dtype=np.int32), WQ_K, WQ_EPS, A, seed=WQ_SEED)
        assert st.dense_levels > 0, st.dense_levels
        rounds = walks = 0
        for i, s in enumerate(WQ_SOURCES):
            ref, sto = twin_topk(pkg, orc, i, s)
            m = int(np.sum(ids[i] >= 0))
            worst = float(np.max(np.abs(vals[i][:m] - ref[ids[i][:m]]), initial=0.0))
            print("fora_batch_topk src %d: %d entries, twin rounds %d walks %d, largest difference %.3e"
                  % (s, m, sto.rounds, sto.walks, worst))
            assert m == min(WQ_K, int(np.sum(ref > 0))), (s, m)
            assert worst <= 1e-9, (s, worst)
            assert any(below and joins > 0 for below, joins in armed_rounds(pkg, WQ, s, sto.rounds)), s
            rounds += sto.rounds
            walks += sto.walks
        print("fora_batch_topk: rounds %d (twin %d), walks %d (twin %d), dense levels %d"
              % (st.rounds, rounds, st.walks, walks, st.dense_levels))
        assert (st.rounds, st.walks) == (rounds, walks)
    finally:
        close_handle(pkg, g)


def test_query_stream_equals_the_twin(pkg, orc):
    """The stream runs its queries as fora_batch_single_source does - one whole-graph FORA push per query, no top-k
    rounds - so its reference is the twin's fora_whole at the same seed and tuning, not fora_topk."""
    g = open_handle(pkg, WQ)
    try:
        t = pkg.tuning_batch()
        t.gs_blocks = 1
        g.set_tuning(t)
        ot = orc.tuning_default()
        for f, _ in ot._fields_:
            setattr(ot, f, getattr(t, f))
        with pkg.QueryStream(g, WQ_EPS, A, k=WQ_K) as qs:
            ids, vals, nsel, st = qs.wait(qs.submit(np.array(WQ_SOURCES, dtype=np.int32), WQ_SEED))
        og = to_oracle(orc, WQ.host(pkg))
        rounds = walks = 0
        for i, s in enumerate(WQ_SOURCES):
            ref, sto = og.fora_whole(s, WQ_EPS, A, seed=WQ_SEED, n_rounds=0, schedule=orc.SYNC, tuning=ot)
            m = int(nsel[i])
            worst = float(np.max(np.abs(vals[i][:m] - ref[ids[i][:m]]), initial=0.0))
            print("stream src %d: %d entries, twin walks %d, largest difference %.3e" % (s, m, sto.walks, worst))
            assert m == min(WQ_K, int(np.sum(ref > 0))) and worst <= 1e-9, (s, m, worst)
            rounds += sto.rounds
            walks += sto.walks
        assert (st.rounds, st.walks) == (rounds, walks), (st.rounds, rounds, st.walks, walks)
    finally:
        close_handle(pkg, g)
