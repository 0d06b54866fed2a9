"""pprhip_weighted_all_pair_backward at the C ABI without a device (include/pprhip.h "weighted relationships", All-Pair
backward search): the symbol and its binding, and alpha and the threshold refused with the entry point and the parameter
named before the (NULL) handle is looked at ("Parameter ranges").  What needs a handle - PPRHIP_ERR_STATE without
weights, the target range, the index itself - is in tests/test_gpu_weighted_allpair.py."""
import ctypes as C
import math

ENTRY = "pprhip_weighted_all_pair_backward"
BAD_ALPHA = [0.0, -0.1, 1.0, 1.5, math.nan, math.inf]
BAD_THRESHOLD = [-1e-6, math.nan, math.inf]          # a threshold: finite and >= 0
OK_ALPHA, OK_THRESHOLD = 0.15, 1e-4


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


def _call(pkg, alpha, threshold):
    out, st = C.c_void_p(), pkg.Stats()
    return pkg.lib().pprhip_weighted_all_pair_backward(None, alpha, threshold, 8, 0, 1, C.byref(out), C.byref(st))


def test_symbol_is_exported_and_bound(pkg):
    L = pkg.lib()
    assert ENTRY in pkg.EXPORTS and hasattr(L, ENTRY) and getattr(L, ENTRY).argtypes
    assert callable(getattr(pkg.Graph, "weighted_all_pair_backward", None))
    # the weighted call takes what its unweighted counterpart takes
    assert L.pprhip_weighted_all_pair_backward.argtypes == L.pprhip_all_pair_backward.argtypes


def test_out_of_range_values_are_refused_before_the_handle(pkg):
    for name, values, call in (("alpha", BAD_ALPHA, lambda x: _call(pkg, x, OK_THRESHOLD)),
                               ("threshold", BAD_THRESHOLD, lambda x: _call(pkg, OK_ALPHA, x))):
        for bad in values:
            rc = call(bad)
            msg = _last(pkg)
            assert rc == pkg.ERR_INVALID, "%s accepted a bad %s (rc %d: %s)" % (ENTRY, name, rc, msg)
            assert ENTRY in msg and ("%s = " % name) in msg, "the error does not name %s: %r" % (name, msg)
    # alpha is looked at before the threshold
    assert _call(pkg, 0.0, math.nan) == pkg.ERR_INVALID and "alpha = " in _last(pkg)


def test_valid_values_reach_the_null_handle(pkg):
    for thr in (OK_THRESHOLD, 0.0):
        rc = _call(pkg, OK_ALPHA, thr)
        msg = _last(pkg)
        assert rc == pkg.ERR_INVALID and "null graph handle" in msg and ENTRY in msg, (rc, msg)
