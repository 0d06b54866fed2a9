"""The designs of tests/sweep_cut_designs.py under the sweep cut by relationship weight (pprhip_weighted_sweep_cut,
pprhip_results_weighted_sweep_cut, pprhip_weighted_local_cluster_seeds).  A design places nodes in slot space, which
depends on the order and the count degrees only - k_wsweep_edges keeps the tiles of the count degree - so two routes
reuse every design unchanged:

  normalize = False.  The design's own unweighted push, relationship weights drawn with a fixed seed from {2^-10, 0.25,
  0.5, 1, 3, 7.5}.  The score is x(v): the weighted order is the unweighted one, Design.prove proves every claimed
  feature on the handle's vector as it does in test_gpu_sweep_cut_designs.py, and every word is compared with the
  weighted reference.
  normalize = True.  All weights 0.5: qdeg = q0 deg with q0 a power of two, so x / qdeg orders as x / deg does (but for
  a_denormal, whose scores underflow: left out).  The order is again the design's, the result is compared with the
  weighted reference, and it equals the unweighted Graph.sweep_cut of the same handle and vector times q0.

Each design runs on the product library, and on the hooks library under the grid caps of
test_gpu_sweep_cut_designs.py; results are byte-identical across the grids and across two sweeps of one handle.
DESIGN.md 3 lists the mutants of kernels_weighted_sweep.hip these tests catch."""
import numpy as np
import pytest

import sweep_cut_designs as D
from sweep_ref import edges_of
from test_gpu_weighted_sweep import bits, check, same, words
from weighted_sweep_ref import quanta, weighted_sweep_ref

pytestmark = pytest.mark.gpu

GRIDS = [(None, None), (1, None), (2, None), (3, None), (None, 1), (None, 3), (2, 3)]   # (edge grid, item grid)
NAMES = ("PPRHIP_SWEEP_EDGE_GRID", "PPRHIP_SWEEP_ITEM_GRID")
LEVELS = np.array([2.0 ** -10, 0.25, 0.5, 1.0, 3.0, 7.5])


def set_grids(monkeypatch, grid):
    for name, g in zip(NAMES, grid):
        if g is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(g))


def route_weights(m, normalize):
    """The relationship weights of a route, aligned with the host's out_ci."""
    if normalize:
        return np.full(m, 0.5)
    return LEVELS[np.random.default_rng(20).integers(0, LEVELS.size, m)]


def routes(d):
    return [nz for nz in (False, True) if nz in d.normalizes and not (nz and d.name == "a_denormal")]


def pushed(g, d, normalize):
    """The design's unweighted push for a sweep under `normalize`; its features proved on the handle's vector."""
    g.forward_push_seeds(d.seeds, D.ALPHA, D.RMAX, weights=d.weights(normalize), fetch=False)
    x = g.reserve()
    return x, d.prove(x, normalize)


def sweeps_of(d, V):
    kws = [dict(), dict(max_size=max(1, V.ref["support"] // 2))]
    if d.name in D.NAMES_B:
        kws += [kw for kw in D.extra_sweeps(d, V) if "max_size" in kw]
    return kws


def times_q0(unweighted, q0, got):
    """The weighted result is the unweighted one of the same handle and vector with vol and cut multiplied by q0."""
    order, vol, cut, info = got
    uo, uv, uc, ui = unweighted
    assert np.array_equal(order, uo) and np.array_equal(vol, uv * np.uint64(q0)) and np.array_equal(cut, uc * np.uint64(q0))
    assert (info.support, info.profiled, info.best_size, info.edge_slots) == (ui.support, ui.profiled, ui.best_size, ui.edge_slots)
    assert (info.best_cut_q, info.best_vol_q, info.total_vol_q) == (ui.best_cut * q0, ui.best_vol * q0, ui.total_vol * q0)
    assert bits(info.best_conductance) == bits(ui.best_conductance)


def run_on_one_grid(g, d, host, edges):
    """Both routes of the design against the reference; returns the results' bytes, in a fixed order."""
    out = []
    for normalize in routes(d):
        w = route_weights(host.m, normalize)
        g.set_weights(w)
        x, V = pushed(g, d, normalize)
        q0 = int(quanta(w)[0])
        for kw in sweeps_of(d, V):
            ref, got = check(g, edges, w, x=x, normalize=normalize, **kw)
            assert np.array_equal(ref["order"], V.ref["order"][:ref["profiled"]])        # the design's order
            assert words(g.weighted_sweep_cut(normalize=normalize, **kw)) == words(got), (d, kw)
            if normalize:
                times_q0(g.sweep_cut(normalize=True, **kw), q0, got)
            out.append(words(got))
        # bounds in weight units, from the reference's own profile: at the best prefix's volume and one quantum below
        bv = V.ref["best_vol"]
        if d.name in D.NAMES_B and bv > 1:
            full = weighted_sweep_ref(g.n, edges[0], edges[1], w, x, normalize=int(normalize))
            for vq in (full["best_vol_q"], full["best_vol_q"] - 1):
                _, got = check(g, edges, w, x=x, normalize=normalize, max_vol=float(np.ldexp(float(vq), -full["shift"])))
                out.append(words(got))
    return out


@pytest.mark.parametrize("name", D.NAMES)
def test_designs_on_the_product(pkg, name):
    d = D.design(name)
    host = d.host(pkg)
    with pkg.Graph(host, device=0) as g:
        assert run_on_one_grid(g, d, host, edges_of(host))


@pytest.mark.parametrize("name", D.NAMES)
def test_designs_under_capped_grids(pkg, monkeypatch, name):
    assert NAMES == ("PPRHIP_SWEEP_EDGE_GRID", "PPRHIP_SWEEP_ITEM_GRID")
    d = D.design(name)
    host = d.host(pkg)
    edges = edges_of(host)
    with pkg.Graph(host, device=0) as g:
        first = None
        for grid in GRIDS:
            set_grids(monkeypatch, grid)
            g.set_weights(None)            # qdeg and the shift are rebuilt under every grid
            got = run_on_one_grid(g, d, host, edges)
            first = got if first is None else first
            assert got == first, (d, grid)


def test_best_prefix_ties_go_to_the_shortest(pkg, monkeypatch):
    """c_ties: several hundred prefixes of conductance 0, the shortest wins under every item grid (PPRHIP_SWEEP_ITEM_GRID),
    and a max_vol between two tied prefixes admits the same one."""
    d = D.design("c_ties")
    host = d.host(pkg)
    edges = edges_of(host)
    with pkg.Graph(host, device=0) as g:
        for normalize in (True, False):
            w = route_weights(host.m, normalize)
            g.set_weights(w)
            x, V = pushed(g, d, normalize)
            full = weighted_sweep_ref(g.n, edges[0], edges[1], w, x, normalize=int(normalize))
            zero = np.nonzero(full["cut_q"] == 0)[0]
            assert np.array_equal(zero, np.nonzero(V.ref["cut"] == 0)[0]) and zero.size >= 300
            for item in (None, 1, 2, 3, 5):
                set_grids(monkeypatch, (None, item))
                _, _, _, info = g.weighted_sweep_cut(normalize=normalize, cap=0)
                assert (info.best_size, info.best_cut_q) == (int(zero[0]) + 1, 0) and bits(info.best_conductance) == bits(0.0)
                between = float(np.ldexp(float(full["vol_q"][zero[200]]), -full["shift"]))
                ref, _ = check(g, edges, w, x=x, normalize=normalize, max_vol=between)
                assert ref["best_size"] == int(zero[0]) + 1


@pytest.mark.parametrize("name", D.NAMES_B)
def test_local_cluster_and_result_store(pkg, monkeypatch, name):
    """Every family B design through the two other entry points (under PPRHIP_SWEEP_EDGE_GRID / PPRHIP_SWEEP_ITEM_GRID
    caps as well).  The one-call form pushes the design's seed set itself, over the weights: its vector is bit-equal to
    weighted_forward_push_seeds' and its members are the reference's.  A store is filled by
    weighted_fora_batch_seeds(keep=...) with the design's seed set and two others."""
    d = D.design(name)
    host = d.host(pkg)
    edges = edges_of(host)
    normalize = d.normalizes[0]
    w = route_weights(host.m, False)
    with pkg.Graph(host, device=0) as g:
        g.set_weights(w)
        g.weighted_forward_push_seeds(d.seeds, D.ALPHA, D.RMAX, weights=d.weights(normalize), fetch=False)
        x = g.reserve()
        full = weighted_sweep_ref(g.n, edges[0], edges[1], w, x, normalize=int(normalize))
        assert full["support"] > 768 and full["edge_slots"] >= 7 * D.SWEEP_TILE
        half = float(np.sum(w)) / 2
        for grid in ((None, None), (1, None), (3, 3)):
            set_grids(monkeypatch, grid)
            for kw in (dict(), dict(max_size=max(1, full["support"] // 2)), dict(max_size=d.cut_size or 100),
                       dict(max_vol=half / 4)):
                ref = weighted_sweep_ref(g.n, edges[0], edges[1], w, x, normalize=int(normalize), **kw)
                members, info, st = g.weighted_local_cluster(d.seeds, D.ALPHA, D.RMAX, weights=d.weights(normalize),
                                                             normalize=normalize, **kw)
                assert np.array_equal(g.reserve(), x) and st.levels > 0
                assert ref["best_size"] > 0 and np.array_equal(members, ref["order"][:ref["best_size"]])
                assert (info.support, info.profiled, info.best_size, info.best_cut_q, info.best_vol_q, info.edge_slots) == \
                    (ref["support"], ref["profiled"], ref["best_size"], ref["best_cut_q"], ref["best_vol_q"], ref["edge_slots"])
                assert bits(info.best_conductance) == bits(ref["best_conductance"])
                assert (info.shift, info.total_vol_q) == (ref["shift"], ref["total_vol_q"])
        few, info, _ = g.weighted_local_cluster(d.seeds, D.ALPHA, D.RMAX, weights=d.weights(normalize), normalize=normalize, cap=2)
        assert np.array_equal(few, full["order"][:2]) and info.best_size == full["best_size"]
        sets = [d.seeds, [int(d.hub)], [3, 700, 1200]]
        store = pkg.Results(g, len(sets))
        try:
            g.weighted_fora_batch_seeds(sets, 0.5, D.ALPHA, seed=5, weights=[d.weights(normalize), None, None], keep=store)
            for i in range(len(sets)):
                xs = store.fetch(i)
                first = None
                for grid in ((None, None), (2, None), (None, 1)):
                    set_grids(monkeypatch, grid)
                    for nz in (True, False):
                        ref = weighted_sweep_ref(g.n, edges[0], edges[1], w, xs, normalize=int(nz))
                        assert ref["support"] > 768
                        got = store.weighted_sweep_cut(i, normalize=nz)
                        same(got, ref)
                        assert words(store.weighted_sweep_cut(i, normalize=nz)) == words(got)
                    first = words(got) if first is None else first
                    assert words(got) == first
                assert np.array_equal(store.fetch(i), xs)
            with pytest.raises(pkg.PprhipError):
                store.weighted_sweep_cut(len(sets))
        finally:
            store.close()
            g.release(g.RELEASE_BATCH)
