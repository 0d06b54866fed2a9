"""pprhip_weighted_all_pair_backward on the GPU: the weighted instantiations of k_apbs_lds (both tables) and
k_apbs_dense, the weighted record build, and the driver around them.

Designed graphs (tests/weighted_apbs_designs.py: apbs_designed's designs with exact weights) under the modes `default`,
`tables`, `large`, `dense` and `whole`: offsets, targets and values equal index_of(search_w ...) bit for bit; where
apbs_designed.counters applies, (st.pops, st.edge_pushes, st.rounds) equal counters() on the WEIGHTED searches.  A
search that finds the record buffer full is run again and counted again, so a call whose entries outgrow the smallest
buffer is held to >= on pops and edge pushes (index and st.rounds exact all the same).  Only the crowds at
apbs_designed's own threshold are such calls; the crowds run a second time at 0.5 / (largest group's size), where the
same searches cross, the entries fit, and all three counters are held to == in every counter mode.  Every weighted call stands between two unweighted calls on the same handle, which
still equal apbs_designed's reference bit for bit.
Game of Thrones with random weights against tests/weighted_bwd_ref.py: bpush_sync(..., "push") per target: membership
exact for every target, values within TOL_PUSH, the k rule against index_from_entries on the reference's entries.
Then merged half ranges, and the life of the record array on the handle."""
import os

import numpy as np
import pytest

import apbs_designed as ad
import weighted_apbs_designs as wd
import weighted_bwd_ref as br
from weighted_apbs_designs import GOT_ALPHA, GOT_THRESHOLDS, GOT_W_SEED

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]
TOL_PUSH = 1e-12
KEEP_IDS = ("colliders", "hot")          # designs that need internal id == caller's id
WHOLE_CROWD = 64                         # targets of a crowd under "whole": every group at even and odd positions


class EnvSet:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def make_graph(pkg, name):
    D = ad.design(name)
    host = D.G.host(pkg)
    if name in KEEP_IDS:
        with EnvSet(PPRHIP_RELABEL="0"):
            lift = pkg.lift_host(host)
            g = pkg.Graph(host)
        ident = np.arange(D.G.n)
        assert np.array_equal(lift["old2new"], ident) and np.array_equal(lift["new2old"], ident)
    else:
        g = pkg.Graph(host)
    return D, g


@pytest.fixture(scope="module")
def ctx():
    """Per design: the graph on the device with the design's exact weights (hooks library; one handle per design)."""
    from conftest import load_hooks_pkg
    pkg = load_hooks_pkg()
    made = {}

    def get(name):
        if name not in made:
            D, g = make_graph(pkg, name)
            g.set_weights(wd.design_weights(name))
            made[name] = (D, g)
        return made[name]

    yield pkg, get
    for _, g in made.values():
        g.close()


_refs = {}


def references(name, lo, hi, rmax):
    """(weighted searches, their index, the unweighted index), made once per range and left unchanged."""
    key = (name, lo, hi, rmax)
    if key not in _refs:
        G = ad.design(name).G
        runs = wd.run_w(name, lo, hi, rmax)
        _refs[key] = (runs, ad.index_of(G, runs), ad.index_of(G, ad.run(G, lo, hi, rmax)))
    return _refs[key]


def same_index(ix, ref, what):
    off, tg, vl = [np.array(x) for x in ix.arrays()]
    ix.close()
    roff, rtg, rvl = ref
    assert np.array_equal(off, roff) and np.array_equal(tg, rtg), what
    assert np.array_equal(vl.view(np.uint64), rvl.view(np.uint64)), what


def query(name, g, lo, hi, rmax, env, mode, what=""):
    """One weighted All-Pair call under `env` between two unweighted ones; `mode`: the counters' mode or None."""
    D = ad.design(name)
    runs, ref_w, ref_u = references(name, lo, hi, rmax)
    env_u = {k: v for k, v in env.items() if not (k == "PPRHIP_APBS_TIER" and v == "3")}   # (tier 3: the batch slots)
    what = "%s %s [%d, %d) rmax %g %s" % (name, what, lo, hi, rmax, env)
    with EnvSet(**env_u):
        same_index(g.all_pair_backward(ad.ALPHA, rmax, -1, lo, hi)[0], ref_u, what + " (unweighted, before)")
    with EnvSet(**env):
        ix, st = g.weighted_all_pair_backward(ad.ALPHA, rmax, -1, lo, hi)
    same_index(ix, ref_w, what)
    with EnvSet(**env_u):
        same_index(g.all_pair_backward(ad.ALPHA, rmax, -1, lo, hi)[0], ref_u, what + " (unweighted, after)")
    print("%s: pops %d edge pushes %d rounds %d xl %d whole %d" % (what, st.pops, st.edge_pushes, st.rounds, st.xl_targets,
                                                                    st.dense_nodes))
    if mode in wd.COUNTER_MODES:
        pops, pushes, rounds = ad.counters(D.G, runs, mode)
        assert st.rounds == rounds, what
        if sum(len(S.entries) for S in runs) <= wd.RECORD_BUFFER_MIN:    # nothing waits for room and runs again
            assert (st.pops, st.edge_pushes) == (pops, pushes), what
        else:
            assert st.pops >= pops and st.edge_pushes >= pushes, what
        assert st.xl_targets == 0 and st.dense_nodes == 0, what
    if mode == "whole":
        assert (st.rounds, st.xl_targets, st.dense_nodes) == (0, 0, hi - lo), what
    return st


# ------------------------------------------------------------------ designed graphs, every mode
@pytest.mark.parametrize("mode", list(wd.MODES))
@pytest.mark.parametrize("name", ["fans", "levels", "routing", "colliders"])
def test_designs_every_mode(ctx, name, mode):
    """fans on the give-up loads 384 / 385 and 1536 / 1537, two levels on both tables' trips (4 * 64 and 4 * 256 edges,
    one below, on, above), routing by in-degree, probe chains that wrap."""
    _, get = ctx
    D, g = get(name)
    for label, lo, hi, rmax in wd.gpu_cases(name):
        query(name, g, lo, hi, rmax, wd.MODES[mode], mode, label)


@pytest.mark.parametrize("F,E", ad.TWO_LEVELS_DENSE)
def test_dense_chunks(ctx, F, E):
    """Dense tier with chunks of 16 edges: a level 2 of kDnShareMin - 1 chunks stays on its workgroup, one of kDnShareMin
    is posted and helper-shared, and one whose frontier is above kDnStage is posted whatever its chunk count."""
    _, get = ctx
    D, g = get("levels")
    t = D.targets["two%d_%d" % (F, E)]
    env = dict(wd.MODES["dense"], PPRHIP_APBS_CHUNK=str(ad.DN_CHUNK_TEST))
    g.release(g.RELEASE_ALL_PAIR)            # the workspace is built with the chunk size the first dense call finds
    try:
        for rmax in D.rmaxes:
            query("levels", g, t, t + 1, rmax, env, "dense", "chunks of 16")
    finally:
        g.release(g.RELEASE_ALL_PAIR)


@pytest.mark.parametrize("gadget,cap_f,xl", [("fanloop%d" % ad.CAPF_FRONT, ad.CAPF_FRONT, 0),
                                             ("fanloop%d" % ad.CAPF_FRONT, ad.CAPF_FRONT - 1, 1),
                                             ("fan%d" % (ad.CAPF_FRONT + 1), ad.CAPF_FRONT + 1, 0),
                                             ("fan%d" % (ad.CAPF_FRONT + 1), ad.CAPF_FRONT, 1)])
def test_cap_f(ctx, gadget, cap_f, xl):
    """PPRHIP_APBS_CAP_F at the designed frontier: a frontier of cap_f entries stays in the dense tier, one more gives the
    search up, and it runs as a whole-vector weighted push (st.xl_targets); the workspace is found clean afterwards."""
    _, get = ctx
    D, g = get("capf")
    t = D.targets[gadget]
    env = dict(wd.MODES["dense"], PPRHIP_APBS_CAP_F=str(cap_f))
    g.release(g.RELEASE_ALL_PAIR)
    try:
        for _ in range(2):
            st = query("capf", g, t, t + 1, ad.R_FAN, env, "dense" if xl == 0 else None, gadget)
            assert (st.rounds, st.xl_targets, st.dense_nodes) == (1, xl, 0)
            query("capf", g, 0, 2, ad.R_FAN, env, None, "both gadgets")
    finally:
        g.release(g.RELEASE_ALL_PAIR)


@pytest.mark.parametrize("hot", [str(ad.HOT_TEST), "0", None])
def test_hot_ids(ctx, hot):
    """PPRHIP_APBS_HOT=64, chunks of 16: ids 63 (hot) and 64 (not) take w / 128 in a level that stays on the workgroup and
    their row's share of 2^-4 in the next, which is posted (hot residues spilled before and filled after).  The weights
    change every source's reserve here."""
    _, get = ctx
    D, g = get("hot")
    env = dict(wd.MODES["dense"], PPRHIP_APBS_CHUNK=str(ad.DN_CHUNK_TEST))
    if hot is not None:
        env["PPRHIP_APBS_HOT"] = hot
    g.release(g.RELEASE_ALL_PAIR)
    try:
        for _ in range(2):
            for label, lo, hi, rmax in wd.gpu_cases("hot"):
                query("hot", g, lo, hi, rmax, env, "dense", "hot %s %s" % (hot, label))
    finally:
        g.release(g.RELEASE_ALL_PAIR)
    for mode in ("default", "whole"):
        query("hot", g, 0, 128, ad.R_HOT, wd.MODES[mode], mode, "hot range")


@pytest.mark.parametrize("mode", list(wd.MODES))
@pytest.mark.parametrize("name", ["crowd_small", "crowd_large"])
def test_crowd(ctx, name, mode):
    """More targets than a table kernel has workgroups, on shared sources whose rows carry both weights: a target at an
    even position of the largest group stops after level 1, one at an odd position pops every source.  At the first
    threshold the entries outgrow the record buffer, so searches wait for room and run again (>= on pops and edge pushes);
    at the second they fit and query() holds pops, edge pushes and rounds to counters() exactly.  "whole": the first 64
    targets, one whole-vector push each."""
    _, get = ctx
    D, g = get(name)
    hi = WHOLE_CROWD if mode == "whole" else D.T
    r_full, r_fit = wd.crowd_rmaxes(D)
    for rmax in (r_full, r_fit):
        entries = sum(len(S.entries) for S in references(name, 0, hi, rmax)[0])
        assert mode == "whole" or (entries <= wd.RECORD_BUFFER_MIN) == (rmax == r_fit)    # which branch query() takes
        st = query(name, g, 0, hi, rmax, wd.MODES[mode], mode, name)
        if mode in ("tables", "large"):
            big = sum(1 for t in range(D.T) if D.kinds[t][0] > 5)
            assert st.rounds == (big if name == "crowd_large" else 0)


# ------------------------------------------------------------------ Game of Thrones, random weights
@pytest.fixture(scope="module")
def got_ctx(got):
    from conftest import load_hooks_pkg
    pkg = load_hooks_pkg()
    w = np.random.default_rng(GOT_W_SEED).uniform(0.5, 1.5, got.m)
    g = pkg.Graph(got)
    g.set_weights(w)
    refs = {}

    def entries(thr):
        if thr not in refs:
            src, tgt, val = [], [], []
            for t in range(got.n):
                p = br.bpush_sync(got, w, [t], None, GOT_ALPHA, thr, "push")[0]
                u = np.flatnonzero((p > 0) & (p >= thr))
                src.append(u)
                tgt.append(np.full(u.size, t))
                val.append(p[u])
            refs[thr] = (np.concatenate(src).astype(np.int32), np.concatenate(tgt).astype(np.int32), np.concatenate(val))
        return refs[thr]

    yield pkg, g, entries
    g.close()


@pytest.mark.parametrize("mode", ["default", "dense", "whole"])
@pytest.mark.parametrize("k", [-1, 10])
@pytest.mark.parametrize("thr", GOT_THRESHOLDS)
def test_got_against_the_push_reference(got_ctx, got, thr, k, mode):
    """All 107 targets (test_weighted_apbs_designs.py pins that no compared value lies within 1e-6 of the threshold):
    every source's row holds exactly the reference's targets, values within TOL_PUSH; k = 10 against index_from_entries."""
    pkg, g, entries = got_ctx
    src, tgt, val = entries(thr)
    ref = pkg.index_from_entries(got.n, src, tgt, val, k)
    roff, rtg, rvl = [np.array(x) for x in ref.arrays()]
    ref.close()
    with EnvSet(**wd.MODES[mode]):
        ix, st = g.weighted_all_pair_backward(GOT_ALPHA, thr, k)
    off, tg, vl = [np.array(x) for x in ix.arrays()]
    ix.close()
    err = float(np.max(np.abs(vl - rvl), initial=0.0)) if vl.size == rvl.size else np.inf
    print("got thr %g k %d %s: %d entries, max |diff| %.3g" % (thr, k, mode, tg.size, err))
    assert np.array_equal(off, roff), (thr, k, mode)
    assert np.array_equal(tg, rtg), (thr, k, mode)          # membership, and the order the k rule gives a row
    assert err <= TOL_PUSH, (thr, k, mode, err)
    if k < 0:
        assert tg.size == src.size
    if mode == "whole":
        assert st.dense_nodes == got.n


# ------------------------------------------------------------------ ranges and merge
@pytest.mark.parametrize("name,cut", [("hot", 50), ("levels", 15)])
def test_half_ranges_merge_to_the_whole_range(ctx, name, cut):
    pkg, get = ctx
    D, g = get(name)
    rmax = D.rmaxes[0]
    hi = 128 if name == "hot" else len(D.gadgets)
    a, _ = g.weighted_all_pair_backward(ad.ALPHA, rmax, -1, 0, cut)
    b, _ = g.weighted_all_pair_backward(ad.ALPHA, rmax, -1, cut, hi)
    whole, _ = g.weighted_all_pair_backward(ad.ALPHA, rmax, -1, 0, hi)
    merged = pkg.merge_indexes([a, b], -1)
    ref = [np.array(x) for x in whole.arrays()]
    same_index(merged, ref, name)
    same_index(whole, references(name, 0, hi, rmax)[1], name)
    a.close()
    b.close()


# ------------------------------------------------------------------ the record array on the handle
def test_lifecycle(ctx):
    pkg, _ = ctx
    name = "hot"
    D, g = make_graph(pkg, name)
    m = D.G.m
    rmax = ad.R_HOT
    ref_w = references(name, 0, 128, rmax)[1]
    w1 = wd.design_weights(name)
    w2 = np.where(w1 == 0.5, 1.5, np.where(w1 == 1.5, 0.5, w1))      # the rows' weights swapped: W = d as before

    def refused():
        with pytest.raises(pkg.PprhipError) as e:
            g.weighted_all_pair_backward(ad.ALPHA, rmax, -1, 0, 128)
        msg = str(e.value)
        assert e.value.code == pkg.ERR_STATE and "no relationship weights" in msg, msg
        assert "pprhip_weighted_all_pair_backward: " in msg, msg

    try:
        refused()                                                     # no weights yet
        g.set_weights(w1)
        present, bytes0 = g.weights_info()
        assert present
        same_index(g.weighted_all_pair_backward(ad.ALPHA, rmax, -1, 0, 128)[0], ref_w, "first call")
        assert g.weights_info() == (True, bytes0 + 16 * m)            # the records, counted once they exist
        with pytest.raises(pkg.PprhipError) as e:                     # the unweighted call's range error
            g.weighted_all_pair_backward(ad.ALPHA, rmax, -1, 5, D.G.n + 1)
        assert e.value.code == pkg.ERR_INVALID and "bad target range" in str(e.value)
        g.release(g.RELEASE_ALL_PAIR)
        assert g.weights_info() == (True, bytes0)
        same_index(g.weighted_all_pair_backward(ad.ALPHA, rmax, -1, 0, 128)[0], ref_w, "after RELEASE_ALL_PAIR")
        assert g.weights_info() == (True, bytes0 + 16 * m)
        g.set_weights(w2)                                             # replaced: the records go with the old weights
        assert g.weights_info() == (True, bytes0)
        X = wd.Weighted(D.G, w2)
        ref2 = ad.index_of(D.G, [wd.search_w(D.G, X, t, rmax) for t in range(128)])
        assert not np.array_equal(ref2[2], ref_w[2])
        same_index(g.weighted_all_pair_backward(ad.ALPHA, rmax, -1, 0, 128)[0], ref2, "after set_weights(w2)")
        g.release(g.RELEASE_WEIGHTS)
        assert g.weights_info() == (False, 0)
        refused()
        g.set_weights(w1)
        same_index(g.weighted_all_pair_backward(ad.ALPHA, rmax, -1, 0, 128)[0], ref_w, "weights set again")
        g.set_weights(None)
        assert g.weights_info() == (False, 0)
        refused()
        same_index(g.all_pair_backward(ad.ALPHA, rmax, -1, 0, 128)[0], references(name, 0, 128, rmax)[2], "unweighted")
    finally:
        g.close()
