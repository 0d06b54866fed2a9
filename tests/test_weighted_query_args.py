"""The weighted seed-set and top-k entry points at the C ABI without a device (include/pprhip.h "weighted seed sets and
top-k"): the symbols and their binding, the numeric parameters refused before the handle is looked at ("Parameter
ranges"), and valid values reaching the NULL handle."""
import ctypes as C
import math

import pytest

SYMBOLS = ["pprhip_weighted_forward_push_seeds", "pprhip_weighted_fora_seeds", "pprhip_weighted_fora_topk",
           "pprhip_weighted_fora_topk_seeds"]
METHODS = ["weighted_forward_push_seeds", "weighted_fora_seeds", "weighted_fora_topk", "weighted_fora_topk_seeds"]
TOPK = ("pprhip_weighted_fora_topk", "pprhip_weighted_fora_topk_seeds")
BAD_ALPHA = [0.0, -0.1, 1.0, 1.5, math.nan, math.inf]
BAD_POSITIVE = [0.0, -1.0, math.nan, math.inf]
BAD_THRESHOLD = [-1e-6, math.nan, math.inf]
OK_ALPHA, OK_EPS, OK_RMAX = 0.15, 0.5, 1e-4


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


def _calls(pkg):
    """name -> call(alpha, eps, rmax, conf edit) with a NULL handle."""
    L = pkg.lib()
    st = pkg.Stats()
    s2 = (C.c_int32 * 2)(0, 1)
    ids, vals, nsel = (C.c_int32 * 4)(), (C.c_double * 4)(), C.c_int(0)

    def conf(a, edit, topk):
        c = pkg.conf_topk(100, 1000, 4, OK_ALPHA) if topk else pkg.conf_whole_graph(100, 1000, OK_ALPHA)
        c.alpha = a
        for k, v in (edit or {}).items():
            setattr(c, k, v)
        return C.byref(c)

    return {
        SYMBOLS[0]: lambda a, e, r, ed: L.pprhip_weighted_forward_push_seeds(None, s2, None, 2, a, r, None, None, None,
                                                                             C.byref(st)),
        SYMBOLS[1]: lambda a, e, r, ed: L.pprhip_weighted_fora_seeds(None, s2, None, 2, e, conf(a, ed, False), 1, r,
                                                                     None, C.byref(st)),
        SYMBOLS[2]: lambda a, e, r, ed: L.pprhip_weighted_fora_topk(None, 0, e, conf(a, ed, True), 1, ids, vals, 4,
                                                                    C.byref(nsel), None, C.byref(st)),
        SYMBOLS[3]: lambda a, e, r, ed: L.pprhip_weighted_fora_topk_seeds(None, s2, None, 2, e, conf(a, ed, True), 1,
                                                                          ids, vals, 4, C.byref(nsel), None,
                                                                          C.byref(st)),
    }


def _rejected(pkg, entry, name, rc):
    msg = _last(pkg)
    assert rc == pkg.ERR_INVALID, "%s accepted a bad %s (rc %d: %s)" % (entry, name, rc, msg)
    assert entry + ":" in msg and ("%s = " % name) in msg, "%s: the error does not name %s: %r" % (entry, name, msg)


def test_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for s in SYMBOLS:
        assert s in pkg.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    for name in METHODS:
        assert callable(getattr(pkg.Graph, name, None)), name
    assert L.pprhip_version() == 100
    # argument for argument the namesakes' signatures (pprhip_weighted_fora_seeds: rmax in place of n_rounds)
    assert L.pprhip_weighted_forward_push_seeds.argtypes == L.pprhip_forward_push_seeds.argtypes
    assert L.pprhip_weighted_fora_topk.argtypes == L.pprhip_fora_topk.argtypes
    assert L.pprhip_weighted_fora_topk_seeds.argtypes == L.pprhip_fora_topk_seeds.argtypes
    a, b = L.pprhip_weighted_fora_seeds.argtypes, L.pprhip_fora_seeds.argtypes
    assert len(a) == len(b) and a[:7] == b[:7] and a[7] is C.c_double and a[8:] == b[8:]


@pytest.mark.parametrize("entry", SYMBOLS)
def test_out_of_range_values_are_refused_before_the_handle(pkg, entry):
    call = _calls(pkg)[entry]
    alpha_name = "alpha" if entry == SYMBOLS[0] else "conf->alpha"
    for bad in BAD_ALPHA:
        _rejected(pkg, entry, alpha_name, call(bad, OK_EPS, OK_RMAX, None))
    if entry in SYMBOLS[:2]:
        for bad in BAD_THRESHOLD:
            _rejected(pkg, entry, "rmax", call(OK_ALPHA, OK_EPS, bad, None))
    if entry != SYMBOLS[0]:
        for bad in BAD_POSITIVE:
            _rejected(pkg, entry, "eps", call(OK_ALPHA, bad, OK_RMAX, None))
            _rejected(pkg, entry, "conf->delta", call(OK_ALPHA, OK_EPS, OK_RMAX, {"delta": bad}))
    if entry == SYMBOLS[1]:
        for bad in BAD_POSITIVE:
            _rejected(pkg, entry, "conf->pfail", call(OK_ALPHA, OK_EPS, OK_RMAX, {"pfail": bad}))
    if entry in TOPK:  # a top-k conf: pfail may be +inf (n div k = 1), never negative or NaN; min_delta > 0
        for bad in (-1.0, math.nan):
            _rejected(pkg, entry, "conf->pfail", call(OK_ALPHA, OK_EPS, OK_RMAX, {"pfail": bad}))
        for bad in BAD_POSITIVE:
            _rejected(pkg, entry, "conf->min_delta", call(OK_ALPHA, OK_EPS, OK_RMAX, {"min_delta": bad}))


@pytest.mark.parametrize("entry", SYMBOLS)
def test_valid_values_reach_the_null_handle(pkg, entry):
    """In range (rmax = 0 included: FORA's default, a legal push threshold), the call fails on the NULL handle."""
    for rmax in (OK_RMAX, 0.0):
        rc = _calls(pkg)[entry](OK_ALPHA, OK_EPS, rmax, None)
        msg = _last(pkg)
        assert rc == pkg.ERR_INVALID and "null graph handle" in msg and entry + ":" in msg, (rc, msg)
