"""Weighted local clustering (include/pprhip.h "weighted local clustering") without a device: the symbols, the Python
surface, and the checks of the entry points, which refuse a bad number or buffer before the handle is looked at and
name the entry point and the parameter."""
import ctypes as C
import math

import numpy as np
import pytest

SWEEP, STORE, CLUSTER = ("pprhip_weighted_sweep_cut", "pprhip_results_weighted_sweep_cut",
                         "pprhip_weighted_local_cluster_seeds")


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


class Calls:
    """The three entry points with one bad argument at a time and a NULL handle."""

    def __init__(self, pkg):
        self.pkg, self.L = pkg, pkg.lib()
        self.info = pkg.WeightedSweep()
        self.seeds = np.zeros(1, dtype=np.int32)

    def run(self, name, normalize=1, max_vol=0.0, bufs=(None, None, None), cap=0, info=True, alpha=0.15, rmax=1e-4):
        info = C.byref(self.info) if info else None
        if name == SWEEP:
            return self.L.pprhip_weighted_sweep_cut(None, normalize, 0, max_vol, *bufs, cap, info)
        if name == STORE:
            return self.L.pprhip_results_weighted_sweep_cut(None, 0, normalize, 0, max_vol, *bufs, cap, info)
        sp = self.seeds.ctypes.data_as(C.c_void_p)
        return self.L.pprhip_weighted_local_cluster_seeds(None, sp, None, 1, alpha, rmax, normalize, 0, max_vol, bufs[0], cap,
                                                          info, None)

    def refused(self, name, what, **kw):
        assert self.run(name, **kw) == self.pkg.ERR_INVALID, (name, kw)
        msg = _last(self.pkg)
        assert msg.startswith(name + ": ") and what in msg, msg


@pytest.fixture
def calls(pkg_product):
    return Calls(pkg_product)


def test_symbols_are_exported_and_bound(pkg_product):
    pkg = pkg_product
    L = pkg.lib()
    for s in (SWEEP, STORE, CLUSTER, "pprhip_weight_quantum"):
        assert s in pkg.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    assert C.sizeof(pkg.WeightedSweep) == 12 * 8
    fields = {"support", "profiled", "best_size", "best_cut_q", "best_vol_q", "best_conductance", "total_vol_q", "shift",
              "edge_slots", "sort_ms", "scan_ms", "total_ms"}
    assert set(pkg.WeightedSweep().as_dict()) == fields
    for method in ("weighted_sweep_cut", "weighted_local_cluster"):
        assert callable(getattr(pkg.Graph, method))
    assert callable(pkg.Results.weighted_sweep_cut) and callable(pkg.weight_quantum)


@pytest.mark.parametrize("name", [SWEEP, STORE, CLUSTER])
def test_numbers_and_buffers_are_refused_before_the_handle(calls, name):
    for bad in (2, -1):
        calls.refused(name, "normalize", normalize=bad)
        calls.refused(name, "normalize", normalize=bad, max_vol=-1.0, info=False)    # the first of several
    calls.refused(name, "null info", info=False)
    calls.refused(name, "null info", info=False, max_vol=math.nan)
    buf = np.zeros(4, dtype=np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    shapes = ((p, None, None),) if name == CLUSTER else ((p, None, None), (None, p, None), (None, None, p))
    for bufs in shapes:
        calls.refused(name, "cap = 0", bufs=bufs)
    for bad in (-1.0, -0.5, math.nan, math.inf, -math.inf):
        calls.refused(name, "max_vol", max_vol=bad)


def test_one_call_form_checks_alpha_and_rmax_before_the_handle(calls):
    for bad in (0.0, 1.0, 1.5, -0.1, math.nan):
        calls.refused(CLUSTER, "alpha", alpha=bad)
    for bad in (-1.0, math.nan, math.inf):
        calls.refused(CLUSTER, "rmax", rmax=bad)
    calls.refused(CLUSTER, "max_vol", max_vol=-1.0, alpha=2.0)      # the sweep's own parameters come first


def test_valid_values_reach_the_null_handle(calls):
    for max_vol in (0.0, 1e-300, 1.0, 1e300):
        for normalize in (0, 1):
            calls.refused(SWEEP, "null graph handle", normalize=normalize, max_vol=max_vol)
            calls.refused(CLUSTER, "null graph handle", normalize=normalize, max_vol=max_vol)
            calls.refused(STORE, "no result", normalize=normalize, max_vol=max_vol)
    buf = np.zeros(4, dtype=np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    calls.refused(SWEEP, "null graph handle", bufs=(p, p, p), cap=4)


def test_weight_quantum_refuses_bad_weights(pkg_product):
    pkg = pkg_product
    assert pkg.weight_quantum([1.0]) == 60 and pkg.weight_quantum([1.0, 1.0]) == 59 and pkg.weight_quantum([0.5] * 3) == 59
    assert pkg.weight_quantum([]) == 0
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(pkg.PprhipError) as e:
            pkg.weight_quantum([1.0, 2.0, bad, 1.0])
        assert e.value.code == pkg.ERR_INVALID and "pprhip_weight_quantum: edge 2" in str(e.value)
    s = C.c_int(7)
    assert pkg.lib().pprhip_weight_quantum(3, None, C.byref(s)) == pkg.ERR_INVALID and s.value == 7
    w = np.ones(3)
    assert pkg.lib().pprhip_weight_quantum(3, w.ctypes.data_as(C.c_void_p), None) == pkg.ERR_INVALID
