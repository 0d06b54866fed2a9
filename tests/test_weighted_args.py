"""The weighted entry points at the C ABI without a device (include/pprhip.h "weighted relationships"): the symbols and
their binding, the numeric parameters refused before the handle is looked at ("Parameter ranges"), and the helper that
aligns an edge list's weights with HostCsr.out_ci."""
import ctypes as C
import math

import numpy as np
import pytest

WEIGHTED_SYMBOLS = ["pprhip_graph_set_weights", "pprhip_weights_info", "pprhip_weight_table_host",
                    "pprhip_weighted_power_method", "pprhip_weighted_forward_push", "pprhip_weighted_random_walk_batch",
                    "pprhip_weighted_fora"]
BAD_ALPHA = [0.0, -0.1, 1.0, 1.5, math.nan, math.inf]
BAD_EPS = [0.0, -1.0, math.nan, math.inf]
BAD_THRESHOLD = [-1e-6, math.nan, math.inf]
OK_ALPHA, OK_EPS, OK_RMAX = 0.15, 0.5, 1e-4


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


def _calls(pkg):
    """name -> call(alpha, eps, rmax, iters, conf edit) with a NULL handle."""
    L = pkg.lib()
    st = pkg.Stats()
    s2 = (C.c_int32 * 2)(0, 1)

    def conf(a, edit):
        c = pkg.conf_whole_graph(100, 1000, OK_ALPHA)
        c.alpha = a
        for k, v in (edit or {}).items():
            setattr(c, k, v)
        return C.byref(c)

    return {
        "pprhip_weighted_power_method": lambda a, e, r, it, ed: L.pprhip_weighted_power_method(None, 0, a, it, None,
                                                                                                C.byref(st)),
        "pprhip_weighted_forward_push": lambda a, e, r, it, ed: L.pprhip_weighted_forward_push(None, 0, a, r, None, None,
                                                                                                None, C.byref(st)),
        "pprhip_weighted_random_walk_batch": lambda a, e, r, it, ed: L.pprhip_weighted_random_walk_batch(
            None, s2, (C.c_uint64 * 2)(0, 1), 2, a, 1, 0, 0, (C.c_int32 * 2)(), None),
        "pprhip_weighted_fora": lambda a, e, r, it, ed: L.pprhip_weighted_fora(None, 0, e, conf(a, ed), 1, r, None,
                                                                                C.byref(st)),
    }


def _rejected(pkg, entry, name, rc):
    msg = _last(pkg)
    assert rc == pkg.ERR_INVALID, "%s accepted a bad %s (rc %d: %s)" % (entry, name, rc, msg)
    assert entry in msg and ("%s = " % name) in msg, "%s: the error does not name %s: %r" % (entry, name, msg)


def test_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for s in WEIGHTED_SYMBOLS:
        assert s in pkg.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    for name in ("set_weights", "weights_info", "weighted_power_method", "weighted_forward_push", "weighted_random_walks",
                 "weighted_fora"):
        assert callable(getattr(pkg.Graph, name, None)), name
    assert callable(pkg.weight_table_host) and callable(pkg.out_edge_order)
    assert pkg.Graph.RELEASE_WEIGHTS == 128 and pkg.RELEASE_WEIGHTS == 128


@pytest.mark.parametrize("entry", ["pprhip_weighted_power_method", "pprhip_weighted_forward_push",
                                   "pprhip_weighted_random_walk_batch", "pprhip_weighted_fora"])
def test_out_of_range_values_are_refused_before_the_handle(pkg, entry):
    call = _calls(pkg)[entry]
    alpha_name = "conf->alpha" if entry == "pprhip_weighted_fora" else "alpha"
    for bad in BAD_ALPHA:
        _rejected(pkg, entry, alpha_name, call(bad, OK_EPS, OK_RMAX, 10, None))
    if entry in ("pprhip_weighted_forward_push", "pprhip_weighted_fora"):
        for bad in BAD_THRESHOLD:
            _rejected(pkg, entry, "rmax", call(OK_ALPHA, OK_EPS, bad, 10, None))
    if entry == "pprhip_weighted_fora":
        for bad in BAD_EPS:
            _rejected(pkg, entry, "eps", call(OK_ALPHA, bad, OK_RMAX, 10, None))
        for field in ("delta", "pfail"):
            for bad in (0.0, -1.0, math.nan, math.inf):
                _rejected(pkg, entry, "conf->" + field, call(OK_ALPHA, OK_EPS, OK_RMAX, 10, {field: bad}))
    if entry == "pprhip_weighted_power_method":
        rc = call(OK_ALPHA, OK_EPS, OK_RMAX, -1, None)
        assert rc == pkg.ERR_INVALID and entry in _last(pkg) and "iters = -1" in _last(pkg)


@pytest.mark.parametrize("entry", ["pprhip_weighted_power_method", "pprhip_weighted_forward_push",
                                   "pprhip_weighted_random_walk_batch", "pprhip_weighted_fora"])
def test_valid_values_reach_the_null_handle(pkg, entry):
    """In range (rmax = 0 included: FORA's default, a legal push threshold), the call fails on the NULL handle."""
    for rmax in (OK_RMAX, 0.0):
        rc = _calls(pkg)[entry](OK_ALPHA, OK_EPS, rmax, 0, None)
        msg = _last(pkg)
        assert rc == pkg.ERR_INVALID and "null graph handle" in msg and entry in msg, (rc, msg)


def test_handle_calls_refuse_a_null_handle(pkg):
    L = pkg.lib()
    w = (C.c_double * 2)(1.0, 1.0)
    assert L.pprhip_graph_set_weights(None, w) == pkg.ERR_INVALID and "null graph handle" in _last(pkg)
    assert L.pprhip_weights_info(None, None, None) == pkg.ERR_INVALID and "null graph handle" in _last(pkg)
    rp = (C.c_uint32 * 2)(0, 2)
    assert L.pprhip_weight_table_host(0, 2, rp, w, None, None) == pkg.ERR_INVALID
    assert L.pprhip_weight_table_host(1, 2, None, w, None, None) == pkg.ERR_INVALID
    assert L.pprhip_weight_table_host(1, 2, rp, None, None, None) == pkg.ERR_INVALID
    assert L.pprhip_weight_table_host(1, 2, rp, w, None, None) == pkg.OK  # (validation alone: both outputs may be NULL)
    bad_rp = (C.c_uint32 * 3)(0, 3, 2)
    assert L.pprhip_weight_table_host(2, 2, bad_rp, w, None, None) == pkg.ERR_INVALID and "ascending" in _last(pkg)


@pytest.mark.parametrize("newest_first", [False, True])
def test_out_edge_order_aligns_an_edge_list_with_the_csr(pkg, newest_first):
    rng = np.random.default_rng(4)
    n, m = 50, 400
    src = rng.integers(0, n, m).astype(np.int32)
    dst = rng.integers(0, n, m).astype(np.int32)
    host = pkg.HostCsr(n, src, dst, newest_first)
    perm = pkg.out_edge_order(src, newest_first)
    assert sorted(perm.tolist()) == list(range(m))
    assert np.array_equal(host.out_ci, dst[perm])
    assert np.array_equal(np.repeat(np.arange(n), np.diff(host.out_rp.astype(np.int64))), src[perm])
