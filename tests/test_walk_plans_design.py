"""The plan designer of tests/walk_plans.py against the CPU twin: every plan the GPU tests use (test_gpu_walk_plans.py)
must come out of `orc.fora_whole_seeds(..., n_rounds=1, conf=...)` exactly as designed.

What the twin must report: one push level - the level that pushes the live seeds, which runs at any threshold; a plan
cannot be had with none - that pops the live seeds and nothing else, `walks == sum c_i`, `mc_sources == S`, and
`rsum == (1 - alpha)^2 (1 - D) / (1 - (1 - alpha) D)` (D the weight of the dead-end seeds; (1 - alpha)^2 without them)
to the rounding of a sum of S terms.  The independent reference (Design.independent) is held against the twin here as
well, so a plan whose two references disagree never reaches the GPU."""
import numpy as np
import pytest

import walk_plans as wp


@pytest.fixture(scope="module")
def og_of(orc, pkg_product):
    return lambda name: wp.oracle_graph(orc, wp.plan_graph(pkg_product, wp.PLANS[name].scale))


@pytest.mark.parametrize("name", list(wp.PLANS))
def test_twin_reproduces_the_plan(orc, pkg_product, og_of, name):
    D = wp.design(orc, pkg_product, name)
    og = og_of(name)
    p = D.plan
    ref, st = D.twin(orc, og)
    S = p.counts.size
    print("%s: S %d walks %d, share %d (%d windows), eps %.4g conf.m %d rmax0 %.3g omega %.6g, min inc / TOL_MC %.0f" % (
        name, S, p.total, D.share(), -(-D.share() // 128), D.eps, D.conf_m, D.rmax0, D.omega, D.sensitivity()))
    assert st.levels == 1 and st.enqueues == 0
    if st.dense_levels:          # (the level of a large seed set runs as a sweep: the same single addition per carrier)
        assert st.dense_nodes == S and st.pops == 0
    else:
        assert st.pops == S and st.edge_pushes == S
    assert st.dead_end_pops == 0 and st.rounds == 1
    assert st.walks == p.total and st.mc_sources == S
    assert abs(st.rsum - D.rsum) <= (S + 4) * np.spacing(D.rsum)
    assert D.sensitivity() >= 1000.0
    # the plan itself, entry by entry: the residue the twin planned from is (1 - alpha) q_i on carrier i alone
    _, _, term, steps = D.walks(og)
    assert st.walk_steps == int(steps.astype(np.int64).sum())
    ind = D.independent(og)
    err = float(np.max(np.abs(ref - ind)))
    print("%s: twin vs independent reference %.3e" % (name, err))
    assert err <= wp.TOL_MC


def test_index_cases_exist_where_the_family_allows_them(orc, pkg_product):
    """Which capacity cases each plan is run at (Design.densities): a silent gap here would be a silent gap on the GPU."""
    want = {"A": {"served", "all-over"},                      # entries of one walk: cap >= 1 serves them at any density
            "B": {"served", "one-over", "all-over"},
            "C": {"served", "all-over"},                      # (small: equal degrees, every entry over by one; large: one)
            "D": {"served", "one-over", "all-over"},
            "G": {"served", "one-over", "all-over"},
            "F": {"served", "one-over", "all-over"}}
    first = each = 0
    for name in wp.PLANS:
        D = wp.design(orc, pkg_product, name)
        labels = [x[0] for x in D.densities()]
        kinds = {"one-over" if x.startswith(("one-over", "share-first")) else x for x in labels}
        kinds |= {"share-first" for x in labels if x.startswith("share-first")}
        print(name, labels)
        assert want.get(name[0], set()) <= kinds, (name, labels)
        for label, rho in D.densities():
            served, walked = D.usage(rho)
            assert served + walked == D.plan.total
            if label.startswith(("one-over", "share-first")):
                assert walked == 1
            if label == "all-over":
                assert served == D.counts.size
        first += "share-first" in kinds
        each += "each-over-by-one" in kinds
        if name.startswith("C-"):
            assert ("each-over-by-one" if name.endswith("small") else "one-over") in kinds, name
    assert first >= 3 and each >= 10


def test_windows_of_one_walk_entries_are_followed_by_a_window():
    """The regime the `e` advance exists for - a window of 128 entries (jl = 127), a serve chunk of 64 (jl = 63), and
    another behind it in the same wave - is met by design, on the single query's grid (16 waves per CU of 256) and on a
    batched call's (4 per CU; both grids are inferences from the launchers, see walk_plans.GRID_SIDE).  Counted from
    the share rule alone (walk_plans.replay)."""
    for name, grid, want_walk, want_serve in (("A-ones-%d" % wp.ONES_WIDE, wp.GRID_REF, 3000, 3000),
                                              ("A-ones-%d" % wp.ONES_WIDE, wp.GRID_SIDE, 3000, 3000),
                                              ("D-mixed-large", wp.GRID_SIDE, 4, 8)):
        full, chunks, windows = wp.replay(wp.PLANS[name].counts, grid)
        print("%s on %d waves: %d full windows and %d full chunks with a successor, up to %d windows per wave" % (
            name, grid, full, chunks, windows))
        assert full >= want_walk and chunks >= want_serve and windows >= 2, name
    for name in wp.PLANS:                                    # for the record: what every plan reaches on either grid
        r1, r2 = wp.replay(wp.PLANS[name].counts, wp.GRID_REF), wp.replay(wp.PLANS[name].counts, wp.GRID_SIDE)
        print("%-22s windows per wave %d / %d, full windows followed %d / %d, full chunks followed %d / %d" % (
            name, r1[2], r2[2], r1[0], r2[0], r1[1], r2[1]))
