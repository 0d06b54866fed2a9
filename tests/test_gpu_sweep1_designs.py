"""The dense level of a single query (csrc/kernels_dense.hip) on the designed graphs of tests/sweep1_designs.py, over the
row-major, the sliced and the row-panel copy of the in-CSR.  Every level of every push is a sweep (dense_frac = gs_frac
= 1e-9), so the rows, segments and panels placed at the hot table's bound, at chunk, window and slice edges, at part,
fold and block bounds are summed by the edge kernels and landed by the apply kernel in every level.

  a  one-level pushes: a threshold under which the source alone pushes; every residue is then the source's contribution
     added once per relationship, bit for bit (equal addends: no tolerance exists)
  b  full pushes against the numpy reference and the oracle twin (TOL_PUSH), at alpha 0.15 and 0.5, under 1, 2, 3 and 6
     Gauss-Seidel blocks where the design names them; a short run behind a long one on the same handle
  c  the three layouts of one graph against each other
  d  the power method, seed sets and FORA top-k over each layout

tests/test_sweep1_designs.py shows on the CPU that a wrong reading of any designed position moves a reserve or residue
of these very queries by 1e7 x TOL_PUSH or more.  Every case prints the largest difference it saw.

Not covered at these sizes: the second trip of k_dense_edges' persistent loop and the second deal of the panel kernel's
item queue (more items than 2 x the CU count, about 16 M edges); tests/test_gpu_scale.py serves both."""
import numpy as np
import pytest

import sweep1_designs as D
from conftest import shared_graph, to_oracle
from test_gpu_parity import TOL_MC, TOL_PUSH

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]  # the layout switches exist in the hooks library only

A = D.ALPHA
LAID = [(name, layout) for name, d in D.all_designs().items() for layout in d.layouts]
MAIN = [("hot", "rowmajor"), ("sliced", "sliced"), ("panels", "panel")]  # one design per layout


def dev_of(pkg, cache, name, layout, monkeypatch):
    """One handle per (design, layout), made under the layout's switches."""
    def make():
        for k, v in D.LAYOUT_ENV[layout].items():
            monkeypatch.setenv(k, v)
        try:
            return pkg.Graph(D.host_of(pkg, name))
        finally:
            for k in D.LAYOUT_ENV[layout]:
                monkeypatch.delenv(k)
    return shared_graph(cache, pkg, name + "/" + layout, make)


def sweep_tuning(pkg, B=1):
    t = pkg.tuning_batch()
    t.dense_frac, t.gs_frac, t.gs_blocks = 1e-9, 1e-9, B
    return t


def swept(st):
    assert st.dense_levels == st.levels and st.class_launches[1] > 0, (st.levels, st.dense_levels)


def diff(a, b):
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def blocks_of(name, layout):
    return (1,) if layout == "norelabel" else D.all_designs()[name].gs_blocks  # (blocks follow the internal order)


def side_of(pkg, name, layout, monkeypatch):
    return D.laid(pkg, name, "rowmajor" if layout == "norelabel" else layout, monkeypatch)[2]


# ------------------------------------------------------------------ a. one-level pushes, exact
@pytest.mark.parametrize("name,layout", LAID)
def test_one_level_pushes_are_exact(pkg, dev_cache, monkeypatch, name, layout):
    d = D.all_designs()[name]
    host, dev = D.host_of(pkg, name), dev_of(pkg, dev_cache, name, layout, monkeypatch)
    worst, count = 0.0, 0
    try:
        for B in blocks_of(name, layout):
            dev.set_tuning(sweep_tuning(pkg, B))
            for s in d.one_level:
                rmax = D.one_level_rmax(host, s)   # from the reference's first level
                p, r, rsum, st = dev.forward_push(s, A, rmax)
                pe, re_ = D.one_level_expected(host, s)
                worst = max(worst, diff(p, pe), diff(r, re_))
                assert st.levels == 1, (name, layout, B, s, st.levels)
                swept(st)
                bad = np.flatnonzero(r != re_)
                assert bad.size == 0, (name, layout, B, s, bad[:8], r[bad[:8]], re_[bad[:8]])
                assert np.array_equal(p, pe), (name, layout, B, s)
                count += 1
        print("one-level pushes %s/%s: %d queries, largest difference %.3e" % (name, layout, count, worst))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ b. full pushes
def push_cases():
    """(design, layout, gs_blocks, first source, count): a case's numpy references take a few seconds at the most."""
    out = []
    for name, layout in LAID:
        d = D.all_designs()[name]
        if name == "sliced" and layout in ("rowmajor", "panel"):
            continue   # (c) runs those
        for B in blocks_of(name, layout):
            srcs = d.sources if B == 1 else d.block_sources
            step = 2 if name == "panels" else len(srcs)
            out += [(name, layout, B, i, step) for i in range(0, len(srcs), step)]
    return out


def check_push(pkg, orc, og, dev, name, B, s, alpha, side):
    """One forward push at the FORA threshold against the reference and the twin; returns the largest difference."""
    host = D.host_of(pkg, name)
    rmax = D.fora_rmax(pkg, host, alpha)
    p, r, rsum, st = dev.forward_push(s, alpha, rmax)
    pr, rr, levels, dead_pops = D.reference(pkg, name, s, B, alpha=alpha, side=side)
    po, ro, _, sto = og.forward_push(s, alpha, rmax, orc.SYNC)
    worst = max(diff(p, pr), diff(r, rr), diff(p, po), diff(r, ro))
    what = (name, B, s, alpha)
    assert st.levels == levels == sto.levels, what + (st.levels, levels, sto.levels)
    assert st.pops + st.dense_nodes == sto.pops + sto.dense_nodes, what
    assert st.dead_end_pops == dead_pops == sto.dead_end_pops, what
    if st.levels:
        swept(st)
    assert worst <= TOL_PUSH, what + (worst,)
    assert abs(p.sum() + r.sum() - 1.0) < 1e-12, what
    return worst, st.levels


@pytest.mark.parametrize("name,layout,B,first,count", push_cases())
def test_full_pushes(pkg, orc, dev_cache, monkeypatch, name, layout, B, first, count):
    d = D.all_designs()[name]
    host, dev = D.host_of(pkg, name), dev_of(pkg, dev_cache, name, layout, monkeypatch)
    og = to_oracle(orc, host)
    side = side_of(pkg, name, layout, monkeypatch)
    srcs = (d.sources if B == 1 else d.block_sources)[first:first + count]
    try:
        dev.set_tuning(sweep_tuning(pkg, B))
        worst, deepest = 0.0, 0
        for s in srcs:
            w, levels = check_push(pkg, orc, og, dev, name, B, s, A, side)
            worst, deepest = max(worst, w), max(deepest, levels)
        if first == 0:
            assert deepest >= 10   # at least ten consecutive sweeps: stale parts, uncleared accumulators
        print("full pushes %s/%s gs_blocks %d sources %s: largest difference %.3e, up to %d sweeps"
              % (name, layout, B, srcs, worst, deepest))
    finally:
        dev.set_tuning(pkg.tuning_default())


@pytest.mark.parametrize("name,layout", MAIN)
def test_full_pushes_at_alpha_one_half(pkg, orc, dev_cache, monkeypatch, name, layout):
    d = D.all_designs()[name]
    host, dev = D.host_of(pkg, name), dev_of(pkg, dev_cache, name, layout, monkeypatch)
    og = to_oracle(orc, host)
    side = side_of(pkg, name, layout, monkeypatch)
    try:
        dev.set_tuning(sweep_tuning(pkg, 1))
        worst = max(check_push(pkg, orc, og, dev, name, 1, s, 0.5, side)[0] for s in d.block_sources[:3])
        print("full pushes %s/%s alpha 0.5: largest difference %.3e" % (name, layout, worst))
    finally:
        dev.set_tuning(pkg.tuning_default())


@pytest.mark.parametrize("name,layout", MAIN)
def test_short_run_behind_a_long_one(pkg, orc, dev_cache, monkeypatch, name, layout):
    """The longest push of the design (from z: its mass keeps coming back from a dead end), then on the same handle a
    push of one level - exact, whatever the parts and accumulators held - and the design's shortest full push."""
    d = D.all_designs()[name]
    host, dev = D.host_of(pkg, name), dev_of(pkg, dev_cache, name, layout, monkeypatch)
    og = to_oracle(orc, host)
    side = side_of(pkg, name, layout, monkeypatch)
    try:
        dev.set_tuning(sweep_tuning(pkg, 1))
        w_long, long_levels = check_push(pkg, orc, og, dev, name, 1, d.names["z"], A, side)
        s = d.one_level[2]
        p, r, _, st = dev.forward_push(s, A, D.one_level_rmax(host, s))
        pe, re_ = D.one_level_expected(host, s)
        assert st.levels == 1 and np.array_equal(p, pe) and np.array_equal(r, re_), (name, layout, s)
        runs = {x: D.reference(pkg, name, x, 1, side=side)[2] for x in d.block_sources if x != d.names["z"]}
        short = min((x for x in runs if runs[x] > 0), key=runs.get)
        w_short, short_levels = check_push(pkg, orc, og, dev, name, 1, short, A, side)
        assert 3 * short_levels <= 2 * long_levels, (short_levels, long_levels)
        print("short run behind a long one %s/%s: %d then 1 then %d sweeps, largest difference %.3e"
              % (name, layout, long_levels, short_levels, max(w_long, w_short)))
    finally:
        dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ c. layouts against each other
@pytest.mark.parametrize("B", [1, 2, 3])
def test_layouts_against_each_other(pkg, orc, dev_cache, monkeypatch, B):
    """The sliced design over the panel, the sliced and the row-major copy (PPRHIP_SLICED=0): levels for levels, vectors
    within TOL_PUSH, and all of them the twin's."""
    d = D.all_designs()["sliced"]
    host = D.host_of(pkg, "sliced")
    og = to_oracle(orc, host)
    devs = {layout: dev_of(pkg, dev_cache, "sliced", layout, monkeypatch) for layout in ("panel", "sliced", "rowmajor")}
    rmax = D.fora_rmax(pkg, host)
    try:
        for dev in devs.values():
            dev.set_tuning(sweep_tuning(pkg, B))
        worst = 0.0
        for s in d.sources:
            got = {k: dev.forward_push(s, A, rmax) for k, dev in devs.items()}
            po, ro, _, sto = og.forward_push(s, A, rmax, orc.SYNC)
            p0, r0, _, st0 = got["rowmajor"]
            for k, (p, r, _, st) in got.items():
                assert (st.levels, st.dense_levels) == (st0.levels, st0.dense_levels) == (sto.levels, sto.dense_levels), (B, s, k)
                w = max(diff(p, p0), diff(r, r0), diff(p, po), diff(r, ro))
                worst = max(worst, w)
                assert w <= TOL_PUSH, (B, s, k, w)
        print("layouts against each other, gs_blocks %d: largest difference %.3e" % (B, worst))
    finally:
        for dev in devs.values():
            dev.set_tuning(pkg.tuning_default())


# ------------------------------------------------------------------ d. the other modes of the apply kernel
@pytest.mark.parametrize("name,layout", LAID)
def test_power_method(pkg, dev_cache, monkeypatch, name, layout):
    d = D.all_designs()[name]
    host, dev = D.host_of(pkg, name), dev_of(pkg, dev_cache, name, layout, monkeypatch)
    worst = 0.0
    for s in d.block_sources[:2]:
        for iters in (1, 2, 5):
            pm, _ = dev.power_method(s, A, iters)
            w = diff(pm, D.power_iteration(host, s, A, iters))
            worst = max(worst, w)
            assert w <= 1e-12, (name, layout, s, iters, w)
    print("power method %s/%s: largest difference %.3e" % (name, layout, worst))


@pytest.mark.parametrize("name,layout", LAID)
def test_seed_sets(pkg, orc, dev_cache, monkeypatch, name, layout):
    """A seed set that holds a seed without in-edges (it takes an extra apply thread behind the last block) and a
    dead-end seed, against the twin."""
    d = D.all_designs()[name]
    nm = d.names
    host, dev = D.host_of(pkg, name), dev_of(pkg, dev_cache, name, layout, monkeypatch)
    og = to_oracle(orc, host)
    rmax = D.fora_rmax(pkg, host)
    sets = [([nm["pool"][5], nm["dead"][0], 7], [0.5, 0.25, 0.25]), ([nm["z"], nm["pool"][0], nm["dead"][1]], None)]
    try:
        worst = 0.0
        for B in blocks_of(name, layout)[:2]:
            dev.set_tuning(sweep_tuning(pkg, B))
            for seeds, w in sets:
                p, r, _, st = dev.forward_push_seeds(seeds, A, rmax, weights=w)
                po, ro, _, sto = og.forward_push_seeds(seeds, A, rmax, weights=w)
                assert st.levels == sto.levels and st.dead_end_pops == sto.dead_end_pops, (name, layout, B, seeds)
                swept(st)
                e = max(diff(p, po), diff(r, ro))
                worst = max(worst, e)
                assert e <= TOL_PUSH and abs(p.sum() + r.sum() - 1.0) < 1e-12, (name, layout, B, seeds, e)
        print("seed sets %s/%s: largest difference %.3e" % (name, layout, worst))
    finally:
        dev.set_tuning(pkg.tuning_default())


@pytest.mark.parametrize("name,layout", LAID)
def test_fora_topk(pkg, orc, dev_cache, monkeypatch, name, layout):
    d = D.all_designs()[name]
    host, dev = D.host_of(pkg, name), dev_of(pkg, dev_cache, name, layout, monkeypatch)
    og = to_oracle(orc, host)
    try:
        dev.set_tuning(sweep_tuning(pkg, 1))
        worst = 0.0
        for s, k in ((d.sources[i], k) for i, k in D.TOPK_CASES[name]):
            nsel, ids, vals, est, st = dev.fora_topk(s, D.EPS, A, k, seed=4, cap=host.n, fetch=True)
            ref, sto = og.fora_topk(s, D.EPS, A, k, seed=4, schedule=orc.SYNC)
            assert (st.levels, st.rounds, st.walks) == (sto.levels, sto.rounds, sto.walks), (name, layout, s)
            assert st.dense_levels == st.levels
            cnt, oids, ovals = orc.topk(ref, k)
            # (the order is decided: engine and twin differ by the order of fp64 additions only, far below this gap)
            assert np.min(-np.diff(np.sort(ref)[::-1][:k + 1])) >= D.TOPK_GAP, (name, s, k)
            assert nsel == cnt and list(ids) == list(oids), (name, layout, s)
            w = max(diff(est, ref), diff(vals, ovals))
            worst = max(worst, w)
            assert w <= TOL_MC, (name, layout, s, w)
        print("FORA top-k %s/%s: largest difference %.3e" % (name, layout, worst))
    finally:
        dev.set_tuning(pkg.tuning_default())
