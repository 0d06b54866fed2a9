"""The batched weighted top-k entry points at the C ABI without a device (include/pprhip.h "batched weighted top-k"):
the symbols and their binding, and the parameter and conf checks that are refused before the handle is looked at - a
conf that is no top-k conf, eps <= 0, q < 0, NULL rows with q > 0 - and valid values reaching the NULL handle."""
import ctypes as C
import math

import pytest

SYMBOLS = ["pprhip_weighted_fora_batch_topk", "pprhip_weighted_fora_batch_topk_seeds"]
METHODS = ["weighted_fora_batch_topk", "weighted_fora_batch_topk_seeds"]
BAD_POSITIVE = [0.0, -1.0, math.nan, math.inf]
OK_ALPHA, OK_EPS, K = 0.15, 0.5, 4


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


def _calls(pkg):
    """name -> call(eps, conf, q, rows) with a NULL handle; rows False: NULL ids_out / vals_out."""
    L = pkg.lib()
    st = pkg.Stats()
    srcs = (C.c_int32 * 2)(0, 1)
    offsets = (C.c_uint64 * 3)(0, 1, 2)
    ids, vals, nsel = (C.c_int32 * (2 * K))(), (C.c_double * (2 * K))(), (C.c_int * 2)()

    def rows(on):
        return (ids, vals) if on else (None, None)

    return {
        SYMBOLS[0]: lambda e, c, q, on: L.pprhip_weighted_fora_batch_topk(None, srcs, q, e, C.byref(c), 1, None, *rows(on),
                                                                          nsel, None, C.byref(st)),
        SYMBOLS[1]: lambda e, c, q, on: L.pprhip_weighted_fora_batch_topk_seeds(None, srcs, None, offsets, q, e,
                                                                                C.byref(c), 1, None, *rows(on), nsel,
                                                                                None, C.byref(st)),
    }


def _topk_conf(pkg, **edit):
    c = pkg.conf_topk(100, 1000, K, OK_ALPHA)
    for k, v in edit.items():
        setattr(c, k, v)
    return c


def _refused(pkg, entry, rc, what):
    msg = _last(pkg)
    assert rc == pkg.ERR_INVALID, "%s accepted %s (rc %d: %s)" % (entry, what, rc, msg)
    assert entry + ":" in msg and "null graph handle" not in msg, "%s: %s reached the handle: %r" % (entry, what, msg)
    return msg


def test_symbols_are_exported_and_bound(pkg):
    L = pkg.lib()
    for s in SYMBOLS + ["pprhip_walk_multi_shares"]:
        assert s in pkg.EXPORTS and hasattr(L, s) and getattr(L, s).argtypes, s
    for name in METHODS:
        assert callable(getattr(pkg.Graph, name, None)), name
    assert callable(pkg.walk_multi_shares)
    # the seed-set form: the sources replaced by seeds / weights / offsets, everything else argument for argument
    a, b = L.pprhip_weighted_fora_batch_topk.argtypes, L.pprhip_weighted_fora_batch_topk_seeds.argtypes
    assert len(a) == 12 and len(b) == 14 and a[0] == b[0] and a[2:] == b[4:]


@pytest.mark.parametrize("entry", SYMBOLS)
def test_bad_parameters_are_refused_before_the_handle(pkg, entry):
    call = _calls(pkg)[entry]
    for bad in BAD_POSITIVE:
        assert "eps = " in _refused(pkg, entry, call(bad, _topk_conf(pkg), 2, True), "eps %r" % bad)
    # a conf that is no top-k conf: the whole-graph conf (k = 0, no delta schedule), and top-k confs with a broken field
    _refused(pkg, entry, call(OK_EPS, pkg.conf_whole_graph(100, 1000, OK_ALPHA), 2, True), "a whole-graph conf")
    for bad in BAD_POSITIVE:
        assert "conf->delta" in _refused(pkg, entry, call(OK_EPS, _topk_conf(pkg, delta=bad), 2, True), "delta")
        assert "conf->min_delta" in _refused(pkg, entry, call(OK_EPS, _topk_conf(pkg, min_delta=bad), 2, True), "min_delta")
    for bad in (0.0, 1.0, math.nan):
        assert "conf->alpha" in _refused(pkg, entry, call(OK_EPS, _topk_conf(pkg, alpha=bad), 2, True), "alpha")
    _refused(pkg, entry, call(OK_EPS, _topk_conf(pkg, k=0), 2, True), "k = 0")
    _refused(pkg, entry, call(OK_EPS, _topk_conf(pkg), -1, True), "q < 0")
    _refused(pkg, entry, call(OK_EPS, _topk_conf(pkg), 2, False), "NULL rows with q > 0")


@pytest.mark.parametrize("entry", SYMBOLS)
def test_valid_values_reach_the_null_handle(pkg, entry):
    for q, on in ((2, True), (1, True), (0, True), (0, False)):  # (NULL rows are fine for a call of no query)
        rc = _calls(pkg)[entry](OK_EPS, _topk_conf(pkg), q, on)
        msg = _last(pkg)
        assert rc == pkg.ERR_INVALID and "null graph handle" in msg and entry + ":" in msg, (q, on, rc, msg)
