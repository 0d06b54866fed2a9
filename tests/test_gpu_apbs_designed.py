"""k_apbs_split, k_apbs_lds (both tables) and k_apbs_dense on the searches designed in tests/apbs_designed.py: sizes on
the tables' give-up loads, on FRONT and 4 * THREADS, on kDnStage, kDnShareMin, hot_n and cap_f, probe chains that wrap,
routing by in-degree, and more targets than a kernel has workgroups.

Every design is exact (alpha = 0.5, out-degrees powers of two), so offsets and targets equal the reference's and the
values equal it bit for bit; the twin is held to TOL_PUSH beside it.  The path a search takes is asserted through the
counters: st.rounds (targets that reached the dense tier), st.xl_targets (searches that outgrew the dense lists), and
st.pops / st.edge_pushes, which count a search again in every tier that ran it - a table that hands a search on has
counted the levels up to the one it overflowed in (apbs_designed.counters).  Whether a dense level was posted shows in
no counter; those cases are derived from the code (kDnStage, kDnShareMin) and checked by value only.
No test reads the CU count."""
import os

import numpy as np
import pytest

import apbs_designed as ad
from conftest import to_oracle

pytestmark = [pytest.mark.gpu, pytest.mark.hooks]
TOL_PUSH = 1e-12
MODES = {"default": {}, "tables": {"PPRHIP_APBS_DEG": "0,0"}, "large": {"PPRHIP_APBS_DEG": "1,0"},
         "dense": {"PPRHIP_APBS_TIER": "2"}}
KEEP_IDS = ("colliders", "hot")          # designs that need internal id == caller's id


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


@pytest.fixture(scope="module")
def ctx(orc):
    """Per design: the graph on the device (hooks library; one handle per design) and on the oracle."""
    from conftest import load_hooks_pkg
    pkg = load_hooks_pkg()
    made = {}

    def get(name):
        if name not in made:
            D = ad.design(name)
            host = D.G.host(pkg)
            if name in KEEP_IDS:
                with EnvSet(PPRHIP_RELABEL="0"):
                    lift = pkg.lift_host(host)
                    g = pkg.Graph(host)
                # the handle shows no id map; the lift it is built from (same library, same switch) does
                ident = np.arange(D.G.n)
                assert np.array_equal(lift["old2new"], ident) and np.array_equal(lift["new2old"], ident)
            else:
                g = pkg.Graph(host)
            made[name] = (D, g, to_oracle(orc, host))
        return made[name]

    yield pkg, get
    for _, g, _ in made.values():
        g.close()


_refs = {}


def references(orc, D, og, lo, hi, rmax):
    key = (D.name, lo, hi, rmax)
    if key not in _refs:
        runs = ad.run(D.G, lo, hi, rmax)
        _refs[key] = (runs, ad.index_of(D.G, runs), og.all_pair_backward(ad.ALPHA, rmax, -1, lo, hi, schedule=orc.SYNC))
    return _refs[key]


def query(orc, D, g, og, lo, hi, rmax, env, mode=None, what=""):
    """One All-Pair call under `env`: index == reference bit for bit, twin within TOL_PUSH; with `mode` the counters too."""
    runs, (roff, rtg, rvl), (ooff, otg, ovl) = references(orc, D, og, lo, hi, rmax)
    with EnvSet(**env):
        ix, st = g.all_pair_backward(ad.ALPHA, rmax, -1, lo, hi)
    off, tg, vl = [np.array(x) for x in ix.arrays()]
    ix.close()
    what = "%s %s [%d, %d) rmax %g %s" % (D, what, lo, hi, rmax, env)
    assert np.array_equal(off, roff) and np.array_equal(tg, rtg), what
    assert np.array_equal(vl.view(np.uint64), rvl.view(np.uint64)), what
    assert np.array_equal(off, ooff) and np.array_equal(tg, otg) and np.max(np.abs(vl - ovl), initial=0.0) <= TOL_PUSH, what
    if mode:
        pops, pushes, rounds = ad.counters(D.G, runs, mode)
        print("%s: pops %d edge pushes %d rounds %d xl %d" % (what, st.pops, st.edge_pushes, st.rounds, st.xl_targets))
        assert (st.pops, st.edge_pushes, st.rounds) == (pops, pushes, rounds), what
        assert st.xl_targets == 0 and st.dense_nodes == 0, what
    return st


# ------------------------------------------------------------------ fans: give-up loads, FRONT, kDnStage
@pytest.mark.parametrize("mode", ["default", "tables", "dense"])
@pytest.mark.parametrize("N", ad.FAN_SIZES)
def test_fan(ctx, orc, N, mode):
    """A fan of N nodes: exactly `limit` nodes stay in a table, limit + 1 are handed on (under "tables" a fan of 385 is
    counted 1 pop and 384 edges more than one of 384, one of 1537 reaches the dense tier: st.rounds); level 2 is a frontier
    of N - 1 entries without edges.  R_FAN: the sources' reserve equals rmax and is emitted; R_FAN_TIE: every add equals
    rmax and nothing joins the frontier."""
    _, get = ctx
    D, g, og = get("fans")
    t = D.targets["fan%d" % N]
    for rmax in D.rmaxes:
        query(orc, D, g, og, t, t + 1, rmax, MODES[mode], mode, "fan%d" % N)


# ------------------------------------------------------------------ two levels: 4 * THREADS, one cell hit by a run of adds
@pytest.mark.parametrize("mode", ["default", "tables", "dense"])
@pytest.mark.parametrize("F,E", ad.TWO_LEVELS)
def test_two_level(ctx, orc, F, E, mode):
    """Level 2: F frontier entries (some of in-degree 0), E edges one below, on and one above a trip of the edge loop;
    every source takes its whole run of equal adds in that level and must join the next frontier once (st.pops).
    F = 129 / 1025 is one entry more than a sub-batch of the small table / than kDnStage; under "tables" the searches of
    F >= 512 outgrow the small table in level 1 and are run by the large one."""
    _, get = ctx
    D, g, og = get("levels")
    t = D.targets["two%d_%d" % (F, E)]
    for rmax in D.rmaxes:
        query(orc, D, g, og, t, t + 1, rmax, MODES[mode], mode, "two_level %d %d" % (F, E))


@pytest.mark.parametrize("F,E", ad.TWO_LEVELS_DENSE)
def test_dense_chunks(ctx, orc, F, E):
    """Dense tier with chunks of 16 edges: a level 2 of kDnShareMin - 1 chunks stays on its workgroup, one of kDnShareMin
    is posted, and one of two chunks whose frontier is above kDnStage is posted whatever its chunk count."""
    _, get = ctx
    D, g, og = get("levels")
    t = D.targets["two%d_%d" % (F, E)]
    env = dict(MODES["dense"], PPRHIP_APBS_CHUNK=str(ad.DN_CHUNK_TEST))
    g.release(g.RELEASE_ALL_PAIR)            # the workspace is built with the chunk size the first dense call finds
    try:
        for rmax in D.rmaxes:
            query(orc, D, g, og, t, t + 1, rmax, env, "dense", "chunks of 16")
    finally:
        g.release(g.RELEASE_ALL_PAIR)


# ------------------------------------------------------------------ routing by in-degree
@pytest.mark.parametrize("mode", ["default", "tables", "dense"])
def test_routing(ctx, orc, mode):
    """300 targets of in-degree 0, 1, 3, 4, 11, 12 and 13 in one range, those without in-edges among the others in every
    wave of k_apbs_split.  Where a search starts shows in the counters of the four deep targets: the one of in-degree 3
    touches 404 nodes and is counted in the small and in the large table, the one of in-degree 4 in the large table only;
    in-degree 11 (1612 nodes) is counted in the large table and in the dense tier, in-degree 12 in the dense tier only.
    st.rounds: the targets of in-degree >= 12 and the one the large table handed on."""
    _, get = ctx
    D, g, og = get("routing")
    st = query(orc, D, g, og, 0, ad.ROUTING_TARGETS, ad.R_FAN, MODES[mode], mode, "routing")
    din = D.G.din[:ad.ROUTING_TARGETS]
    if mode == "default":
        assert st.rounds == int((din >= ad.DEG_DENSE).sum()) + 1
    if mode == "tables":
        assert st.rounds == 2
    if mode == "dense":
        assert st.rounds == ad.ROUTING_TARGETS


# ------------------------------------------------------------------ probe chains that wrap
@pytest.mark.parametrize("cap,mode", [(ad.SMALL_CAP, "tables"), (ad.LARGE_CAP, "large"), (ad.SMALL_CAP, "default"),
                                      (ad.LARGE_CAP, "dense")])
def test_colliders(ctx, orc, cap, mode):
    """Forty in-neighbours whose home slot is CAP - 2 or CAP - 1: the chain wraps through slot 0 (where target 0 of the
    large table's case sits itself).  "tables" keeps the search of 41 nodes in the small table, "large" (PPRHIP_APBS_DEG=1,0)
    starts it in the large one; pops, edge pushes and st.rounds == 0 say that neither table handed it on, which a probe
    that does not wrap would.  A probe sequence that wraps differently but still visits every slot it is asked for
    gives the same table contents and cannot be told apart by results."""
    _, get = ctx
    D, g, og = get("colliders")
    t = D.targets["collide%d" % cap]
    st = query(orc, D, g, og, t, t + 1, ad.R_FAN, MODES[mode], mode, "colliders %d" % cap)
    if mode in ("tables", "large"):
        assert st.rounds == 0 and st.pops == 1 + ad.COLLIDER_COUNT and st.edge_pushes == ad.COLLIDER_COUNT


# ------------------------------------------------------------------ hot ids of the dense tier
@pytest.mark.parametrize("hot", [str(ad.HOT_TEST), "0", None])
def test_hot_ids(ctx, orc, hot):
    """PPRHIP_APBS_HOT=64, chunks of 16: ids 63 (hot) and 64 (not) take residue in a level that stays on the workgroup
    (63: in LDS) and cross in the next, which is posted (hot residues spilled before and filled after), for a hot target
    (10) and a cold one (100).  The same with no hot ids and with the default (a quarter of the graph: 128)."""
    _, get = ctx
    D, g, og = get("hot")
    env = dict(MODES["dense"], PPRHIP_APBS_CHUNK=str(ad.DN_CHUNK_TEST))
    if hot is not None:
        env["PPRHIP_APBS_HOT"] = hot
    g.release(g.RELEASE_ALL_PAIR)
    try:
        for _ in range(2):
            for t in ad.HOT_TARGETS:
                query(orc, D, g, og, t, t + 1, ad.R_HOT, env, "dense", "hot %s" % hot)
        query(orc, D, g, og, 0, 128, ad.R_HOT, env, "dense", "hot %s, both targets among trivial ones" % hot)
    finally:
        g.release(g.RELEASE_ALL_PAIR)


# ------------------------------------------------------------------ cap_f
@pytest.mark.parametrize("gadget,cap_f,xl", [("fanloop%d" % ad.CAPF_FRONT, ad.CAPF_FRONT, 0),
                                             ("fanloop%d" % ad.CAPF_FRONT, ad.CAPF_FRONT - 1, 1),
                                             ("fan%d" % (ad.CAPF_FRONT + 1), ad.CAPF_FRONT + 1, 0),
                                             ("fan%d" % (ad.CAPF_FRONT + 1), ad.CAPF_FRONT, 1)])
def test_cap_f(ctx, orc, gadget, cap_f, xl):
    """The dense tier's lists of cap_f entries.  dn_edge_range appends to the next frontier while pos < cap_f: a frontier
    of exactly cap_f entries stays, one more gives the search up (fanloop40: frontier 40, 40 distinct pops).  The list of
    popped nodes has cap_f entries too (k_apbs_dense, pp < cap_f), and a plain fan pops its target before its frontier:
    fan41's frontier of 40 fits cap_f = 40 but its 41st pop does not, so there the give-up lies at cap_f = frontier and
    cap_f = frontier + 1 stays.  A search given up is run again on the handle's own vectors (st.xl_targets; at most 256
    of them), the workspace is cleared as a whole, and the next call and a single search find everything clean."""
    pkg, get = ctx
    D, g, og = get("capf")
    t = D.targets[gadget]
    env = dict(MODES["dense"], PPRHIP_APBS_CAP_F=str(cap_f))
    g.release(g.RELEASE_ALL_PAIR)
    try:
        for _ in range(2):
            st = query(orc, D, g, og, t, t + 1, ad.R_FAN, env, "dense" if xl == 0 else None, gadget)
            assert (st.rounds, st.xl_targets, st.dense_nodes) == (1, xl, 0)
            query(orc, D, g, og, 0, 2, ad.R_FAN, env, None, "both gadgets")
        single_search(g, D, t, ad.R_FAN)
    finally:
        g.release(g.RELEASE_ALL_PAIR)


def single_search(g, D, t, rmax):
    p, r, _ = g.backward_push(t, ad.ALPHA, rmax)
    S = ad.search(D.G, t, rmax, keep=True)
    rp, rr = np.zeros(D.G.n), np.zeros(D.G.n)
    for u, x in S.reserve.items():
        rp[u] = x
    for u, x in S.residue.items():
        rr[u] = x
    assert np.array_equal(p, rp) and np.array_equal(r, rr), "single search of target %d after All-Pair" % t


# ------------------------------------------------------------------ more targets than workgroups
@pytest.mark.parametrize("name,mode", [("crowd_small", "tables"), ("crowd_large", "large")])
def test_crowd(ctx, orc, name, mode):
    """More targets in a table kernel's list than its grid can hold on any part of at most 512 CUs (8 workgroups per CU
    for the small table: 4352 > 4096; 2 for the large one: 1152 > 1024), so some workgroup runs one search after another:
    fans that outgrow the table (it clears every slot) between fans of 5 (cleared by the used list), all on shared
    sources, so a slot left behind would be found again under the same key.  Twice on one handle, then a single search."""
    _, get = ctx
    D, g, og = get(name)
    rmax = D.rmaxes[0]
    for _ in range(2):
        st = query(orc, D, g, og, 0, D.T, rmax, MODES[mode], mode, name)
        big = sum(1 for t in range(D.T) if D.kinds[t][0] > 5)
        assert st.rounds == (big if name == "crowd_large" else 0)
    single_search(g, D, 0, rmax)
    single_search(g, D, 1, rmax)
