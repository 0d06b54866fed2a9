"""The sparse frontier level (csrc/kernels_push.hip: k_sparse_prepare, k_sparse_push, k_sparse_levels_wg; csrc/levels.cpp:
run_sparse_batch) on the designed graphs of tests/sparse_level_designs.py: tile, staging, crossing-list, LDS-table, batch,
one-workgroup-cap, grid-bound and level-shape edges, forward and, on the transposed designs, backward.

Every design is exact (alpha = 0.5, dyadic values; tests/test_sparse_level_designs.py proves it on the CPU), so every
vector is compared with the plain reference bit for bit and every counter for equality:

  a  the push of every design on a handle of its own, four times in a row: as the library decides, with the LDS table on
     every level (PPRHIP_COMB_MIN_EDGES=1), with the table on none, and once more - the same bytes and counters each time,
     so nothing is left behind in the level counters, the dead-end cell or the table
  b  the resumable top-k push over three rounds, thresholds falling by 4 and min_rmax the last one, on the B, W, T and N
     designs, against the oracle twin's topk_push, bit for bit.  Every round's rmax is >= min_rmax, so this covers
     parking and the round start from the parked set and arms no node; armed nodes, dropped nodes and rounds below
     min_rmax have designs and a plain reference of their own in tests/test_gpu_topk_round_designs.py
  c  the B, W and G designs without the one-workgroup kernel: PPRHIP_SPARSE_WG is read once per process, so one child
     process (tests/fixtures/sparse_level_child.py) runs them all with PPRHIP_SPARSE_WG=0 and its bytes equal this
     process's"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import sparse_level_designs as D
from conftest import HOOKS_LIB, ROOT, to_oracle
from sparse_ref import same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]   # the table, relabel and one-workgroup switches are test hooks

ALL = list(D.all_designs().values())
COUNTERS = ("levels", "dense_levels", "pops", "dense_nodes", "edge_pushes", "enqueues", "dead_end_pops")
NO_WG = D.designs("BWG")


def open_handle(pkg, d):
    """A handle of the design's own, under its level-shape threshold (one Gauss-Seidel block: a dense level is one plain
    sweep); a design whose claims name internal ids keeps the caller's."""
    if d.keep_ids:
        os.environ["PPRHIP_RELABEL"] = "0"
    try:
        g = pkg.Graph(d.host(pkg))
    finally:
        os.environ.pop("PPRHIP_RELABEL", None)
    t = pkg.tuning_default()
    t.dense_frac, t.gs_blocks = d.dense_frac, 1
    g.set_tuning(t)
    return g


def close_handle(pkg, g):
    g.set_tuning(pkg.tuning_default())   # (the twin follows every set_tuning: leave it at the defaults)
    g.close()


def device_push(g, d):
    """(reserve, residue, rsum or None, counters) of the design's push."""
    if d.fwd:
        p, r, rsum, st = g.forward_push(d.start, D.ALPHA, d.rmax)
    else:
        p, r, st = g.backward_push(d.start, D.ALPHA, d.rmax)
        rsum = None
    return p, r, rsum, {k: int(getattr(st, k)) for k in COUNTERS}


def check_against_reference(d, got, what):
    ref = D.run(d)
    p, r, rsum, counters = got
    pe, re_ = ref.vector("reserve", d.n), ref.vector("residue", d.n)
    bad = np.flatnonzero(r.view(np.uint64) != re_.view(np.uint64))
    print("%s %s: %s, %d residues and %d reserves differ" % (d.name, what, counters, bad.size,
                                                            int(np.sum(p.view(np.uint64) != pe.view(np.uint64)))))
    assert counters == ref.totals(), (d, what, counters, ref.totals())
    assert bad.size == 0, (d, what, bad[:8], r[bad[:8]], re_[bad[:8]])
    assert same_bits(r, re_) and same_bits(p, pe), (d, what)
    if d.fwd:
        assert rsum == math.fsum(ref.residue.values()), (d, what, rsum)   # (the exact sum: it is representable)


_own = {}   # design name -> what this process's library-default push returned (read by the child comparison)


def own_result(pkg, d):
    if d.name not in _own:
        g = open_handle(pkg, d)
        try:
            _own[d.name] = device_push(g, d)
        finally:
            close_handle(pkg, g)
    return _own[d.name]


# ------------------------------------------------------------------ a. every design, bit for bit
@pytest.mark.parametrize("d", ALL, ids=repr)
def test_push_equals_the_reference(pkg, monkeypatch, d):
    g = open_handle(pkg, d)
    try:
        monkeypatch.delenv("PPRHIP_COMB_MIN_EDGES", raising=False)
        first = device_push(g, d)
        check_against_reference(d, first, "default")
        _own.setdefault(d.name, first)
        for what, value in (("table on", D.COMB_ON), ("table off", D.COMB_OFF)):
            monkeypatch.setenv("PPRHIP_COMB_MIN_EDGES", value)
            check_against_reference(d, device_push(g, d), what)
        monkeypatch.delenv("PPRHIP_COMB_MIN_EDGES")
        again = device_push(g, d)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes(), d
        assert again[2:] == first[2:], d
    finally:
        close_handle(pkg, g)


# ------------------------------------------------------------------ b. the resumable top-k push against the twin
@pytest.mark.parametrize("d", D.designs("BWTN", "fwd"), ids=repr)
def test_topk_rounds_equal_the_twin(pkg, orc, d):
    g = open_handle(pkg, d)
    try:
        og = to_oracle(orc, d.host(pkg))
        g.topk_push_reset(d.start, D.ALPHA)
        tw = og.topk_push(d.start, D.ALPHA, orc.SYNC)
        levels = []
        for rnd in range(3):
            rm = d.rmax * 4.0 ** (2 - rnd)
            rs, st = g.topk_push_round(d.rmax, rm)
            rs_o, sto = tw.round(d.rmax, rm)
            levels.append(st.levels)
            assert (rs, st.levels, st.pops) == (rs_o, sto.levels, sto.pops), (d, rnd)
            assert same_bits(g.reserve(), tw.reserve) and same_bits(g.residue(), tw.residue), (d, rnd)
        print("%s top-k rounds: levels %s" % (d.name, levels))
        assert sum(levels) > 0, d
    finally:
        close_handle(pkg, g)


# ------------------------------------------------------------------ c. without the one-workgroup kernel
def child_main(pkg, out_path):
    """The child's half: every B, W and G design, forward and backward, on the library as it finds it."""
    out = {}
    for d in NO_WG:
        g = open_handle(pkg, d)
        p, r, rsum, counters = device_push(g, d)
        g.close()
        out[d.name + "__p"], out[d.name + "__r"] = p, r
        out[d.name + "__c"] = np.array([counters[k] for k in COUNTERS] + [0], dtype=np.int64)
        out[d.name + "__rsum"] = np.array([rsum if rsum is not None else 0.0])
    np.savez(out_path, **out)


def test_without_the_one_workgroup_kernel(pkg, tmp_path):
    out = str(tmp_path / "no_wg.npz")
    env = dict(os.environ, PPRHIP_SPARSE_WG="0", PPRHIP_LIB_PATH=HOOKS_LIB)
    env.pop("PPRHIP_COMB_MIN_EDGES", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fixtures", "sparse_level_child.py"), out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-3000:])
    theirs = np.load(out)
    assert len(NO_WG) >= 30 and {d.mode for d in NO_WG} == {"fwd", "bwd"}
    for d in NO_WG:
        p, r_, rsum, counters = own_result(pkg, d)
        assert theirs[d.name + "__p"].tobytes() == p.tobytes() and theirs[d.name + "__r"].tobytes() == r_.tobytes(), d
        assert list(theirs[d.name + "__c"][:-1]) == [counters[k] for k in COUNTERS], d
        assert theirs[d.name + "__rsum"][0] == (rsum if rsum is not None else 0.0), d
