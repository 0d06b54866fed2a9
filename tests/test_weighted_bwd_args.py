"""The weighted backward entry points at the C ABI without a device (include/pprhip.h "weighted relationships", the
backward direction): the symbols and their binding, and the numeric parameters refused with the entry point and the
parameter named before the (NULL) handle is looked at ("Parameter ranges").  What needs a handle - PPRHIP_ERR_STATE
without weights, ids, sets and offsets with the set named - is in tests/test_gpu_weighted_backward.py: the set checks
come after the handle, as in pprhip_ppr_targets."""
import ctypes as C
import math

import pytest

SYMBOLS = ["pprhip_weighted_backward_push", "pprhip_weighted_walk_survival", "pprhip_weighted_ppr_targets",
           "pprhip_weighted_ppr_pairs"]
METHODS = ["weighted_backward_push", "weighted_walk_survival", "weighted_ppr_targets", "weighted_ppr_target_sets",
           "weighted_ppr_pairs"]
BAD_ALPHA = [0.0, -0.1, 1.0, 1.5, math.nan, math.inf]
BAD_EPS = [0.0, -1.0, math.nan, math.inf]
OK_ALPHA, OK_EPS, OK_RMAX = 0.15, 0.5, 1e-4


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


def _calls(pkg):
    """name -> call(alpha, eps, rmax, conf edit) with a NULL handle."""
    L = pkg.lib()
    st = pkg.Stats()
    one = (C.c_int32 * 1)(0)
    val = (C.c_double * 1)()

    def conf(a, edit):
        c = pkg.conf_whole_graph(100, 1000, OK_ALPHA)
        c.alpha = a
        for k, v in (edit or {}).items():
            setattr(c, k, v)
        return C.byref(c)

    return {
        "pprhip_weighted_backward_push": lambda a, e, r, ed: L.pprhip_weighted_backward_push(None, 0, a, r, None, None,
                                                                                              C.byref(st)),
        "pprhip_weighted_walk_survival": lambda a, e, r, ed: L.pprhip_weighted_walk_survival(None, a, None),
        "pprhip_weighted_ppr_targets": lambda a, e, r, ed: L.pprhip_weighted_ppr_targets(
            None, one, None, None, 1, a, r, None, None, 0, None, None, None, None, C.byref(st)),
        "pprhip_weighted_ppr_pairs": lambda a, e, r, ed: L.pprhip_weighted_ppr_pairs(None, one, one, 1, e, conf(a, ed), r, 1,
                                                                                      val, C.byref(st)),
    }


def _rejected(pkg, entry, name, rc):
    msg = _last(pkg)
    assert rc == pkg.ERR_INVALID, "%s accepted a bad %s (rc %d: %s)" % (entry, name, rc, msg)
    assert entry in msg and ("%s = " % name) in msg, "%s: the error does not name %s: %r" % (entry, name, msg)


def test_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    for name in METHODS:
        assert callable(getattr(pkg.Graph, name, None)), name
    # the weighted calls take what their unweighted counterparts take
    for a, b in (("pprhip_weighted_backward_push", "pprhip_backward_push"),
                 ("pprhip_weighted_walk_survival", "pprhip_walk_survival"),
                 ("pprhip_weighted_ppr_targets", "pprhip_ppr_targets"), ("pprhip_weighted_ppr_pairs", "pprhip_ppr_pairs")):
        assert getattr(L, a).argtypes == getattr(L, b).argtypes, a


@pytest.mark.parametrize("entry", SYMBOLS)
def test_out_of_range_values_are_refused_before_the_handle(pkg, entry):
    call = _calls(pkg)[entry]
    alpha_name = "conf->alpha" if entry == "pprhip_weighted_ppr_pairs" else "alpha"
    for bad in BAD_ALPHA:
        _rejected(pkg, entry, alpha_name, call(bad, OK_EPS, OK_RMAX, None))
    bad_rmax = {"pprhip_weighted_backward_push": [-1e-6, math.nan, math.inf],       # a threshold: finite and >= 0
                "pprhip_weighted_ppr_targets": [0.0, -1e-3, 1.5, math.nan, math.inf],  # 0 < rmax <= 1
                "pprhip_weighted_ppr_pairs": [-1e-3, 1.5, math.nan, math.inf],         # 0 (the default) or 0 < rmax <= 1
                "pprhip_weighted_walk_survival": []}[entry]
    for bad in bad_rmax:
        _rejected(pkg, entry, "rmax", call(OK_ALPHA, OK_EPS, bad, None))
    if entry == "pprhip_weighted_ppr_pairs":
        for bad in BAD_EPS:
            _rejected(pkg, entry, "eps", call(OK_ALPHA, bad, OK_RMAX, None))
        for field in ("delta", "pfail"):
            for bad in (0.0, -1.0, math.nan, math.inf):
                _rejected(pkg, entry, "conf->" + field, call(OK_ALPHA, OK_EPS, OK_RMAX, {field: bad}))
        st = pkg.Stats()
        rc = pkg.lib().pprhip_weighted_ppr_pairs(None, None, None, 0, OK_EPS, None, OK_RMAX, 1, None, C.byref(st))
        assert rc == pkg.ERR_INVALID and entry in _last(pkg) and "null conf" in _last(pkg)


@pytest.mark.parametrize("entry", SYMBOLS)
def test_valid_values_reach_the_null_handle(pkg, entry):
    rc = _calls(pkg)[entry](OK_ALPHA, OK_EPS, OK_RMAX, None)
    msg = _last(pkg)
    assert rc == pkg.ERR_INVALID and "null graph handle" in msg and entry in msg, (rc, msg)
