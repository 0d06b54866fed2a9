"""The twelve forward single-query entry points at the C ABI without a device: the four forward push calls, the two
weighted whole-graph FORA calls, the two walk-batch calls and the four FORA top-k calls.  They share their bodies
(csrc/forward_calls.cpp, the top-k check sequence of csrc/weighted_query.cpp, topk_args_ok), so every refusal has to
name the entry point that was called and no sibling of it: a shared body that hard-codes one caller's name fails here.
Numeric parameters are refused before the handle is looked at (include/pprhip.h "Parameter ranges"): the message
names the parameter, not the NULL handle.  The output row of a top-k call (k, cap, ids / vals) is checked behind the
handle in all four calls, so with a NULL handle that refusal is the handle's - PPRHIP_ERR_INVALID under the caller's
name either way; the row check itself (topk_args_ok) and where it stands among the refusals is held on a live handle
by tests/test_gpu_forward_front.py::test_a_bad_topk_row_on_a_live_handle."""
import ctypes as C
import math
import re

import pytest

BAD_ALPHA = [0.0, -0.1, 1.0, 1.5, math.nan, math.inf]
BAD_EPS = [0.0, -1.0, math.nan, math.inf]
BAD_THRESHOLD = [-1e-6, math.nan, math.inf]
OK_ALPHA, OK_EPS, OK_RMAX = 0.15, 0.5, 1e-4

PUSH = ["pprhip_forward_push", "pprhip_forward_push_seeds", "pprhip_weighted_forward_push",
        "pprhip_weighted_forward_push_seeds"]
FORA = ["pprhip_weighted_fora", "pprhip_weighted_fora_seeds"]
WALK = ["pprhip_random_walk_batch", "pprhip_weighted_random_walk_batch"]
TOPK = ["pprhip_fora_topk", "pprhip_fora_topk_seeds", "pprhip_weighted_fora_topk", "pprhip_weighted_fora_topk_seeds"]
ENTRIES = PUSH + FORA + WALK + TOPK


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


def _call(pkg, entry, alpha=OK_ALPHA, eps=OK_EPS, rmax=OK_RMAX, k=4, cap=4, row=True):
    """entry with a NULL handle; row False: no ids / vals arrays for the top-k row."""
    f = getattr(pkg.lib(), entry)
    st = pkg.Stats()
    seeds = (C.c_int32 * 2)(0, 1)
    start = (seeds, None, 2) if entry.endswith("_seeds") else (0,)
    if entry in PUSH:
        return f(None, *start, alpha, rmax, None, None, None, C.byref(st))
    if entry in WALK:
        return f(None, seeds, (C.c_uint64 * 2)(0, 1), 2, alpha, 1, 0, 0, (C.c_int32 * 2)(), None)
    if entry in FORA:
        conf = pkg.conf_whole_graph(100, 1000, OK_ALPHA)
        conf.alpha = alpha
        return f(None, *start, eps, C.byref(conf), 1, rmax, None, C.byref(st))
    conf = pkg.conf_topk(100, 1000, 4, OK_ALPHA)
    conf.alpha = alpha
    conf.k = k
    ids, vals, n_out = (C.c_int32 * 8)(), (C.c_double * 8)(), C.c_int(0)
    return f(None, *start, eps, C.byref(conf), 1, ids if row else None, vals if row else None, cap, C.byref(n_out), None,
             C.byref(st))


def _names_only(entry, msg):
    """every pprhip_* name in the message is the entry point's own"""
    names = set(re.findall(r"pprhip_[a-z0-9_]+", msg))
    assert names == {entry}, "%s: the message names %s: %r" % (entry, sorted(names), msg)


def _refused(pkg, entry, param, rc):
    msg = _last(pkg)
    assert rc == pkg.ERR_INVALID, "%s accepted a bad %s (rc %d: %s)" % (entry, param, rc, msg)
    _names_only(entry, msg)
    assert ("%s = " % param) in msg and "null graph handle" not in msg, "%s: %r does not name %s" % (entry, msg, param)


def test_the_entry_points_are_exported_and_bound(pkg):
    for e in ENTRIES:
        assert e in pkg.EXPORTS and getattr(pkg.lib(), e).argtypes, e


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_bad_alpha_is_refused_before_the_handle(pkg, entry):
    name = "alpha" if entry in PUSH + WALK else "conf->alpha"
    for bad in BAD_ALPHA:
        _refused(pkg, entry, name, _call(pkg, entry, alpha=bad))


@pytest.mark.parametrize("entry", FORA + TOPK)
def test_a_bad_eps_is_refused_before_the_handle(pkg, entry):
    for bad in BAD_EPS:
        _refused(pkg, entry, "eps", _call(pkg, entry, eps=bad))


@pytest.mark.parametrize("entry", PUSH + FORA)
def test_a_bad_rmax_is_refused_before_the_handle(pkg, entry):
    for bad in BAD_THRESHOLD:
        _refused(pkg, entry, "rmax", _call(pkg, entry, rmax=bad))


@pytest.mark.parametrize("entry", TOPK)
def test_a_bad_topk_row_is_refused_under_the_callers_name(pkg, entry):
    for kw in (dict(cap=-1), dict(k=0), dict(k=-3), dict(row=False)):
        rc = _call(pkg, entry, **kw)
        msg = _last(pkg)
        assert rc == pkg.ERR_INVALID, (entry, kw, rc, msg)
        _names_only(entry, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_valid_values_reach_the_null_handle(pkg, entry):
    """In range (rmax = 0 included: the weighted FORA's default, a legal push threshold) the call fails on the handle."""
    for rmax in (OK_RMAX, 0.0):
        rc = _call(pkg, entry, rmax=rmax)
        msg = _last(pkg)
        assert rc == pkg.ERR_INVALID and "null graph handle" in msg, (entry, rc, msg)
        _names_only(entry, msg)
