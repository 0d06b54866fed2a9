"""The walk index (include/pprhip.h "walk index") without a device: its density, the range checks of its entry points,
and the capacity rule cap(v) = ceil(d(v) * density) held against the CPU oracle's own walk counts.

The index serves a whole-graph FORA query only if it holds every walk the query starts: a residue node v starts
ceil(r(v) (1 - alpha) / rsum * floor(omega * rsum)) walks (Fora_Whole_Graph.java:112-131 as oracle/ppr_oracle.c restates
it), and a converged push at rmax leaves r(v) < d(v) * rmax.  The last test evaluates both sides on the oracle's push."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import to_oracle


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


@pytest.mark.parametrize("alpha", [0.15, 0.5])
@pytest.mark.parametrize("eps", [0.1, 0.5])
def test_density_is_the_documented_product(pkg_product, alpha, eps):
    pkg = pkg_product
    conf = pkg.conf_whole_graph(4096, 65536, alpha)
    rmax0, omega = pkg.fora_whole_params(conf, eps)
    for rmax in (0.0, rmax0 / 4):
        r = rmax0 if rmax == 0.0 else rmax
        want = np.float64(1.0 - alpha) * np.float64(r) * np.float64(omega) * (np.float64(1.0) + np.float64(2.0) ** -20)
        assert pkg.walk_index_density(conf, eps, rmax) == want


def test_density_refuses_values_out_of_range(pkg_product):
    pkg = pkg_product
    L = pkg.lib()
    out = C.c_double()

    def call(alpha=0.15, eps=0.5, rmax=0.0):
        c = pkg.conf_whole_graph(100, 1000, 0.15)
        c.alpha = alpha
        return L.pprhip_walk_index_density(C.byref(c), eps, rmax, C.byref(out))

    assert call() == pkg.OK
    for bad in (0.0, -0.1, 1.0, 1.5, math.nan, math.inf):
        assert call(alpha=bad) == pkg.ERR_INVALID
        assert "pprhip_walk_index_density" in _last(pkg) and "alpha = " in _last(pkg), _last(pkg)
    for bad in (0.0, -1.0, math.nan):
        assert call(eps=bad) == pkg.ERR_INVALID
        assert "pprhip_walk_index_density" in _last(pkg) and "eps = " in _last(pkg), _last(pkg)
    for bad in (-1e-6, math.inf, -math.inf, math.nan):
        assert call(rmax=bad) == pkg.ERR_INVALID
        assert "pprhip_walk_index_density" in _last(pkg) and "rmax = " in _last(pkg), _last(pkg)


@pytest.mark.parametrize("bad", [0.0, math.nan, math.inf, -1.0])
def test_build_checks_the_density_before_the_handle(pkg_product, bad):
    pkg = pkg_product
    rc = pkg.lib().pprhip_walk_index_build(None, 0.15, 1, bad, None)
    assert rc == pkg.ERR_INVALID
    assert "pprhip_walk_index_build" in _last(pkg) and "density = " in _last(pkg), _last(pkg)
    rc = pkg.lib().pprhip_walk_index_build(None, 0.15, 1, 0.25, None)       # in range: as far as the NULL handle
    assert rc == pkg.ERR_INVALID and "null graph handle" in _last(pkg)
    for bad_alpha in (0.0, 1.0, math.nan):
        rc = pkg.lib().pprhip_walk_index_build(None, bad_alpha, 1, 0.25, None)
        assert rc == pkg.ERR_INVALID and "alpha = " in _last(pkg)


def test_indexed_profiles_exist(pkg_product):
    pkg = pkg_product
    a, b = pkg.tuning_indexed(), pkg.tuning_indexed_batch()
    d, db = pkg.tuning_default(), pkg.tuning_batch()
    for f, _ in a._fields_:
        if f != "c_walk_ns":                                    # only the walk cost may differ from the profile it extends
            assert getattr(a, f) == getattr(d, f) and getattr(b, f) == getattr(db, f), f
    assert 0 < a.c_walk_ns <= d.c_walk_ns and 0 < b.c_walk_ns <= db.c_walk_ns
    assert pkg.Graph.RELEASE_WALK_INDEX == 4


@pytest.mark.parametrize("graph", ["got", "rmat12"])
def test_capacity_covers_the_oracles_walk_counts(pkg_product, orc, got, rmat12, graph):
    """For every node after OracleGraph.forward_push(s, alpha, rmax0):
    ceil(r(v)(1 - alpha) / rsum' * floor(omega * rsum')) <= ceil(d(v) * density), rsum' = (1 - alpha) * sum r."""
    pkg = pkg_product
    host = got if graph == "got" else rmat12
    alpha, eps = 0.15, 0.5
    og = to_oracle(orc, host)
    conf = pkg.conf_whole_graph(host.n, host.m, alpha)
    rmax0, omega = pkg.fora_whole_params(conf, eps)
    rho = pkg.walk_index_density(conf, eps)
    d = np.diff(host.out_rp).astype(np.float64)
    cap = np.ceil(d * rho)
    rng = np.random.default_rng(13)
    live = np.nonzero(d > 0)[0]
    srcs = [int(x) for x in live[rng.integers(0, live.size, 10)]]
    checked = 0
    for s in srcs:
        _, r, _, _ = og.forward_push(s, alpha, rmax0, orc.SYNC)
        rsum = r.sum() * (1.0 - alpha)
        nrw = float(int(omega * rsum))
        if not (rsum > 0.0 and nrw > 0.0):
            continue
        need = np.ceil(r * (1.0 - alpha) / rsum * nrw)
        worst = int(np.argmax(need - cap))
        assert np.all(need <= cap), "source %d node %d: %g walks, capacity %g (r = %g, d = %g)" % (
            s, worst, need[worst], cap[worst], r[worst], d[worst])
        checked += int((need > 0).sum())
    assert checked > 0
