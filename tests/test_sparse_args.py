"""The sparse getters (include/pprhip.h "sparse results") without a device: every entry point checks threshold, order,
the count pointer and the cap / buffer pairing before it looks at its handle, and says which argument it refuses."""
import ctypes as C
import math

import numpy as np
import pytest


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


def _calls(pkg):
    """name -> call(threshold, order, ids, vals, cap, count, offsets) on a NULL handle"""
    L = pkg.lib()
    return {
        "pprhip_get_reserve_sparse": lambda t, o, i, v, k, c, offs: L.pprhip_get_reserve_sparse(None, t, o, i, v, k, c),
        "pprhip_get_residue_sparse": lambda t, o, i, v, k, c, offs: L.pprhip_get_residue_sparse(None, t, o, i, v, k, c),
        "pprhip_results_fetch_sparse": lambda t, o, i, v, k, c, offs: L.pprhip_results_fetch_sparse(None, 0, t, o, i, v, k, c),
        "pprhip_results_fetch_sparse_all": lambda t, o, i, v, k, c, offs: L.pprhip_results_fetch_sparse_all(
            None, t, o, offs, i, v, k, c),
    }


NAMES = ["pprhip_get_reserve_sparse", "pprhip_get_residue_sparse", "pprhip_results_fetch_sparse",
         "pprhip_results_fetch_sparse_all"]


@pytest.fixture
def bufs():
    ids = np.zeros(4, dtype=np.int32)
    vals = np.zeros(4)
    offs = np.zeros(2, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return ids, vals, offs, p(ids), p(vals), p(offs)


@pytest.mark.parametrize("name", NAMES)
def test_threshold_out_of_range(pkg_product, bufs, name):
    pkg, call = pkg_product, _calls(pkg_product)[name]
    _, _, _, pi, pv, po = bufs
    cnt = C.c_uint64(77)
    for bad in (-1e-300, math.nan, math.inf, -math.inf):
        assert call(bad, 0, pi, pv, 4, C.byref(cnt), po) == pkg.ERR_INVALID
        assert name + ":" in _last(pkg) and "threshold = " in _last(pkg), _last(pkg)
    assert cnt.value == 77


@pytest.mark.parametrize("name", NAMES)
def test_order_out_of_range(pkg_product, bufs, name):
    pkg, call = pkg_product, _calls(pkg_product)[name]
    _, _, _, pi, pv, po = bufs
    cnt = C.c_uint64()
    for bad in (-1, 2):
        assert call(0.0, bad, pi, pv, 4, C.byref(cnt), po) == pkg.ERR_INVALID
        assert name + ":" in _last(pkg) and "order = %d" % bad in _last(pkg), _last(pkg)


@pytest.mark.parametrize("name", NAMES)
def test_null_count_pointer(pkg_product, bufs, name):
    pkg, call = pkg_product, _calls(pkg_product)[name]
    _, _, _, pi, pv, po = bufs
    assert call(0.0, 0, pi, pv, 4, None, po) == pkg.ERR_INVALID
    assert name + ":" in _last(pkg) and "count" in _last(pkg), _last(pkg)


def test_all_refuses_null_offsets(pkg_product, bufs):
    pkg = pkg_product
    _, _, _, pi, pv, _ = bufs
    cnt = C.c_uint64()
    assert _calls(pkg)["pprhip_results_fetch_sparse_all"](0.0, 0, pi, pv, 4, C.byref(cnt), None) == pkg.ERR_INVALID
    assert "pprhip_results_fetch_sparse_all:" in _last(pkg) and "offsets_out" in _last(pkg), _last(pkg)


@pytest.mark.parametrize("name", NAMES)
def test_buffer_with_cap_zero(pkg_product, bufs, name):
    pkg, call = pkg_product, _calls(pkg_product)[name]
    _, _, _, pi, pv, po = bufs
    cnt = C.c_uint64()
    for i, v in ((pi, None), (None, pv), (pi, pv)):
        assert call(0.0, 1, i, v, 0, C.byref(cnt), po) == pkg.ERR_INVALID
        assert name + ":" in _last(pkg) and "cap = 0" in _last(pkg), _last(pkg)


@pytest.mark.parametrize("name", NAMES)
def test_in_range_arguments_reach_the_handle_check(pkg_product, bufs, name):
    pkg, call = pkg_product, _calls(pkg_product)[name]
    ids, vals, offs, pi, pv, po = bufs
    cnt = C.c_uint64(77)
    for t, o, i, v, k in ((0.0, 0, None, None, 0), (0.0, 1, pi, pv, 4), (1e-3, 0, pi, None, 2), (1.0, 1, None, pv, 1),
                          (5e-324, 0, None, None, 9)):
        assert call(t, o, i, v, k, C.byref(cnt), po) == pkg.ERR_INVALID
        msg = _last(pkg)
        assert name + ":" in msg and ("null graph handle" in msg or "no result" in msg or "null store" in msg), msg
    assert cnt.value == 77 and not ids.any() and not vals.any() and not offs.any()


def test_constants(pkg_product):
    pkg = pkg_product
    assert (pkg.SPARSE_BY_ID, pkg.SPARSE_BY_VALUE, pkg.RELEASE_SPARSE) == (0, 1, 16)
    assert pkg.Graph.RELEASE_SPARSE == 16
