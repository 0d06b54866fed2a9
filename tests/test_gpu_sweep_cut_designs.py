"""The designs of tests/sweep_cut_designs.py on the GPU (pprhip_sweep_cut, pprhip_results_sweep_cut,
pprhip_local_cluster_seeds): every design proves its layout features again on the vector the handle returns, and order,
vol, cut, the best prefix and the header words are compared exactly, the conductance bit for bit, with
tests/sweep_ref.py applied to that vector - no tolerance, as in test_gpu_sweep.py, whose `same` and `check` do the
comparing.

Each design runs on the product library, and on the hooks library with the grids capped: PPRHIP_SWEEP_EDGE_GRID 1, 2
and 3 (with seven tiles or more the workgroups of k_sweep_edges take unequal numbers of turns over the same two LDS
arrays) and PPRHIP_SWEEP_ITEM_GRID 1 and 3 (second and later rounds of the stride loops of k_sweep_support - whose
padded last round has idle lanes, n being no multiple of 256 - k_sweep_rank, k_sweep_tile_starts and k_sweep_best).
Results are byte-identical across the grids, and across two sweeps of one handle (the workspace is reused).

Nothing a caller can read tells how many workgroups a launch had, so no test here shows by itself that a cap took
effect (as with PPRHIP_APPLY_GRID): tests/test_sweep_cut_designs.py finds the switches' names in the hooks library and
not in the product, and DESIGN.md 3 lists two mutants of the kernels' later turns that fail these tests under the caps
and under nothing else."""
import numpy as np
import pytest

import sweep_cut_designs as D
from test_gpu_sweep import bits, check, same

pytestmark = pytest.mark.gpu

GRIDS = [(None, None), (1, None), (2, None), (3, None), (None, 1), (None, 3), (2, 3)]   # (edge grid, item grid)


def words(got):
    """A sweep's result as bytes and header words (the times left out)."""
    order, vol, cut, info = got
    return (order.tobytes(), vol.tobytes(), cut.tobytes(),
            tuple(sorted((k, bits(v) if isinstance(v, float) else v) for k, v in info.as_dict().items()
                         if not k.endswith("_ms"))))


def set_grids(monkeypatch, names, grid):
    for name, g in zip(names, grid):
        if g is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(g))


def pushed(g, d, normalize):
    """The design's push for a sweep under `normalize`; its features proved on the handle's vector."""
    g.forward_push_seeds(d.seeds, D.ALPHA, D.RMAX, weights=d.weights(normalize), fetch=False)
    x = g.reserve()
    return x, d.prove(x, normalize)


def sweeps_of(d, V):
    kws = [dict(), dict(max_size=max(1, V.ref["support"] // 2))]
    if d.name in D.NAMES_B:
        kws += D.extra_sweeps(d, V)
    return kws


def run_on_one_grid(g, d, edges):
    """Every sweep of the design against the reference; returns the results' bytes, in a fixed order."""
    out = []
    for normalize in (True, False):
        if normalize not in d.normalizes:
            continue
        x, V = pushed(g, d, normalize)
        for kw in sweeps_of(d, V):
            _, got = check(g, edges, x=x, normalize=normalize, **kw)
            again = g.sweep_cut(normalize=normalize, **kw)
            assert words(again) == words(got), (d, kw)
            out.append(words(got))
        _, got = check(g, edges, x=x, normalize=not normalize)    # the other order of the same vector
        out.append(words(got))
    return out


def edges_of_design(d):
    return d.src.astype(np.int64), d.dst.astype(np.int64)


@pytest.mark.parametrize("name", D.NAMES)
def test_designs_on_the_product(pkg, name):
    d = D.design(name)
    with pkg.Graph(d.host(pkg), device=0) as g:
        run_on_one_grid(g, d, edges_of_design(d))


@pytest.mark.parametrize("name", D.NAMES)
def test_designs_under_capped_grids(pkg, monkeypatch, name):
    d = D.design(name)
    names = ("PPRHIP_SWEEP_EDGE_GRID", "PPRHIP_SWEEP_ITEM_GRID")
    edges = edges_of_design(d)
    with pkg.Graph(d.host(pkg), device=0) as g:
        first = None
        for grid in GRIDS:
            set_grids(monkeypatch, names, grid)
            got = run_on_one_grid(g, d, edges)
            first = got if first is None else first
            assert got == first, (d, grid)


def test_best_prefix_ties_go_to_the_shortest(pkg, monkeypatch):
    """Several hundred prefixes of conductance 0 in different threads, waves and workgroups of k_sweep_best, none among
    the first 512 positions: the shortest wins whatever the grid (the partial count of k_sweep_best_final follows it)."""
    names = ("PPRHIP_SWEEP_EDGE_GRID", "PPRHIP_SWEEP_ITEM_GRID")
    d = D.design("c_ties")
    with pkg.Graph(d.host(pkg), device=0) as g:
        for normalize in (True, False):
            x, V = pushed(g, d, normalize)
            zero = np.nonzero(V.ref["cut"] == 0)[0]
            for item in (None, 1, 2, 3, 5):
                set_grids(monkeypatch, names, (None, item))
                _, _, _, info = g.sweep_cut(normalize=normalize, cap=0)
                assert (info.best_size, info.best_cut) == (int(zero[0]) + 1, 0) and bits(info.best_conductance) == bits(0.0)
                # max_vol between two tied prefixes: the shortest of the admitted ones is the same one
                check(g, edges_of_design(d), x=x, normalize=normalize, max_vol=int(V.ref["vol"][zero[200]]))


@pytest.mark.parametrize("name", D.NAMES_B)
def test_local_cluster_and_result_store(pkg, monkeypatch, name):
    """Every family B design through the two other entry points.  The one-call form pushes the design's seed set itself:
    the same vector, so the features hold, and it runs the design's bounded sweeps (the max_size cuts on kT - 1, kT and
    kT + 1 among them).  A store can only be filled by a batched call, so it keeps batched FORA vectors of the design's
    seed set and two others: the store path gets the design's graph (the padded rows, the self loops, the gadget) but
    not its designed order.  The designed features are evaluated on each stored vector all the same and the ones
    that hold are printed; what is asserted there is the exact comparison with the reference on what the store returns."""
    d = D.design(name)
    names = ("PPRHIP_SWEEP_EDGE_GRID", "PPRHIP_SWEEP_ITEM_GRID")
    edges = edges_of_design(d)
    normalize = d.normalizes[0]
    with pkg.Graph(d.host(pkg), device=0) as g:
        x, V = pushed(g, d, normalize)
        for grid in ((None, None), (1, None), (3, 3)):
            set_grids(monkeypatch, names, grid)
            for kw in sweeps_of(d, V):
                ref = d.view(x, normalize, **kw).ref
                members, info, st = g.local_cluster(d.seeds, D.ALPHA, D.RMAX, weights=d.weights(normalize),
                                                    normalize=normalize, **kw)
                assert np.array_equal(g.reserve(), x) and st.levels > 0
                assert ref["best_size"] > 0 and np.array_equal(members, ref["order"][:ref["best_size"]])
                assert (info.support, info.profiled, info.best_size, info.best_cut, info.best_vol, info.edge_slots) == \
                    (ref["support"], ref["profiled"], ref["best_size"], ref["best_cut"], ref["best_vol"], ref["edge_slots"])
                assert bits(info.best_conductance) == bits(ref["best_conductance"])
        sets = [d.seeds, [int(d.hub)], [3, 700, 1200]]
        store = pkg.Results(g, len(sets))
        try:
            g.fora_batch_seeds(sets, 0.5, D.ALPHA, seed=5, weights=[d.weights(normalize), None, None], keep=store)
            for i in range(len(sets)):
                xs = store.fetch(i)
                first = None
                for grid in ((None, None), (2, None), (None, 1)):
                    set_grids(monkeypatch, names, grid)
                    for nz in (True, False):
                        W = d.view(xs, nz)
                        assert W.ref["support"] > 768 and len(W.tiles) >= 7
                        if grid == (None, None):
                            print("%s, stored vector %d, normalize %d: of %s holds %s" % (
                                d, i, nz, d.claims, [f for f in d.claims if D.FEATURES[f](W)]))
                        got = store.sweep_cut(i, normalize=nz)
                        same(got, W.ref)
                        assert words(store.sweep_cut(i, normalize=nz)) == words(got)
                    first = words(got) if first is None else first
                    assert words(got) == first
                assert np.array_equal(store.fetch(i), xs)
        finally:
            store.close()
            g.release(g.RELEASE_BATCH)
