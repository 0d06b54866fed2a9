"""Range checks of alpha, eps and the thresholds at the C ABI, without a device (include/pprhip.h, "Parameter ranges").

An out-of-range value must never reach a kernel: at alpha <= 0 or NaN no walk stops, at alpha = 0 a push on a cycle
keeps its mass for ever, at alpha = 1 rmax0 divides by zero, at eps <= 0 the walk count is infinite.  Every entry point
checks these values before it looks at its handle, so each call below passes a NULL handle (NULL per-GPU array, NULL
communicator) with one bad value: the library must answer PPRHIP_ERR_INVALID and name the parameter.  Without the check
the call would fail on the NULL handle instead, with a message that names no parameter - so these tests fail on a
library without the checks, on the CPU, instead of hanging a GPU."""
import ctypes as C
import math

import pytest

BAD_ALPHA = [0.0, -0.1, 1.0, 1.5, math.nan, math.inf]
BAD_EPS = [0.0, -1.0, math.nan]
BAD_THRESHOLD = [-1e-6, math.nan]
OK_ALPHA, OK_EPS, OK_RMAX = 0.15, 0.5, 1e-4


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


def _conf(pkg, alpha=OK_ALPHA, topk=False):
    """A valid conf (n = 100, m = 1000) with conf.alpha overwritten afterwards: the conf is caller-owned and editable."""
    c = pkg.conf_topk(100, 1000, 10, OK_ALPHA) if topk else pkg.conf_whole_graph(100, 1000, OK_ALPHA)
    c.alpha = alpha
    return c


def _entry_points(pkg):
    """name -> (parameters it takes, call(alpha, eps, rmax) with a NULL handle).  "alpha" of a FORA entry point is the
    conf's; rmax stands for every threshold (rmax, min_rmax, the All-Pair threshold)."""
    L = pkg.lib()
    st = pkg.Stats()
    s2 = (C.c_int32 * 2)(0, 1)
    ids, vals, cnt = (C.c_int32 * 16)(), (C.c_double * 16)(), C.c_int(0)
    out_ptr = C.c_void_p()
    cuts = (C.c_uint32 * 3)()
    d1, d2, d3 = C.c_double(), C.c_double(), C.c_double()
    null_gpus = C.cast(None, C.POINTER(C.c_void_p))

    def whole(a):
        return C.byref(_conf(pkg, a))

    def topk(a):
        return C.byref(_conf(pkg, a, topk=True))

    return {
        "pprhip_forward_push": (("alpha", "rmax"), lambda a, e, r: L.pprhip_forward_push(None, 0, a, r, None, None, None,
                                                                                           C.byref(st))),
        "pprhip_fwdpush_topk_reset": (("alpha",), lambda a, e, r: L.pprhip_fwdpush_topk_reset(None, 0, a)),
        "pprhip_fwdpush_topk_round": (("min_rmax", "rmax"), None),  # (called apart: two thresholds)
        "pprhip_random_walk_batch": (("alpha",), lambda a, e, r: L.pprhip_random_walk_batch(
            None, s2, (C.c_uint64 * 2)(0, 1), 2, a, 1, 0, 0, (C.c_int32 * 2)(), None)),
        "pprhip_fora_single_source": (("alpha", "eps"), lambda a, e, r: L.pprhip_fora_single_source(
            None, 0, e, whole(a), 1, 0, None, C.byref(st))),
        "pprhip_fora_topk": (("alpha", "eps"), lambda a, e, r: L.pprhip_fora_topk(
            None, 0, e, topk(a), 1, ids, vals, 16, C.byref(cnt), None, C.byref(st))),
        "pprhip_monte_carlo": (("alpha", "eps"), lambda a, e, r: L.pprhip_monte_carlo(None, 0, e, whole(a), 1, None,
                                                                                        C.byref(st))),
        "pprhip_fora_batch_single_source": (("alpha", "eps"), lambda a, e, r: L.pprhip_fora_batch_single_source(
            None, s2, 2, e, whole(a), 1, 0, None, 0, None, None, None, None, C.byref(st))),
        "pprhip_fora_batch_single_source_resident": (("alpha", "eps"), lambda a, e, r:
            L.pprhip_fora_batch_single_source_resident(None, s2, 2, e, whole(a), 1, 0, None, None, 0, None, None, None,
                                                       None, C.byref(st))),
        "pprhip_fora_stream_open": (("alpha", "eps"), lambda a, e, r: L.pprhip_fora_stream_open(
            None, e, whole(a), 0, C.byref(out_ptr))),
        "pprhip_fora_batch_topk": (("alpha", "eps"), lambda a, e, r: L.pprhip_fora_batch_topk(
            None, s2, 2, 4, e, a, 1, ids, vals, C.byref(st))),
        "pprhip_forward_push_seeds": (("alpha", "rmax"), lambda a, e, r: L.pprhip_forward_push_seeds(
            None, s2, None, 2, a, r, None, None, None, C.byref(st))),
        "pprhip_fora_seeds": (("alpha", "eps"), lambda a, e, r: L.pprhip_fora_seeds(
            None, s2, None, 2, e, whole(a), 1, 0, None, C.byref(st))),
        "pprhip_fora_topk_seeds": (("alpha", "eps"), lambda a, e, r: L.pprhip_fora_topk_seeds(
            None, s2, None, 2, e, topk(a), 1, ids, vals, 16, C.byref(cnt), None, C.byref(st))),
        "pprhip_backward_push": (("alpha", "rmax"), lambda a, e, r: L.pprhip_backward_push(None, 0, a, r, None, None,
                                                                                             C.byref(st))),
        "pprhip_all_pair_backward": (("alpha", "threshold"), lambda a, e, r: L.pprhip_all_pair_backward(
            None, a, r, 8, 0, 1, C.byref(out_ptr), C.byref(st))),
        "pprhip_all_pair_backward_multi": (("alpha", "threshold"), lambda a, e, r: L.pprhip_all_pair_backward_multi(
            null_gpus, 1, a, r, 8, C.byref(out_ptr), None)),
        "pprhip_all_pair_backward_sharded": (("alpha", "threshold"), lambda a, e, r:
            L.pprhip_all_pair_backward_sharded(None, a, r, 8, C.byref(out_ptr), C.byref(st))),
        "pprhip_shard_target_cuts": (("alpha", "threshold"), lambda a, e, r: L.pprhip_shard_target_cuts(
            None, 2, a, r if r != OK_RMAX else 1e-3, 2, cuts, None)),
        "pprhip_fora_batch": (("alpha", "eps"), lambda a, e, r: L.pprhip_fora_batch(
            null_gpus, 1, s2, 2, 4, e, whole(a), 1, 0, ids, vals, None, None)),
        "pprhip_power_method": (("alpha",), lambda a, e, r: L.pprhip_power_method(None, 0, a, 10, None, C.byref(st))),
        "pprhip_conf_fora_whole_graph": (("alpha",), lambda a, e, r: L.pprhip_conf_fora_whole_graph(
            100, 1000, a, C.byref(pkg.ForaConf()))),
        "pprhip_conf_fora_topk": (("alpha",), lambda a, e, r: L.pprhip_conf_fora_topk(
            100, 1000, 10, a, C.byref(pkg.ForaConf()))),
        "pprhip_fora_whole_params": (("alpha", "eps"), lambda a, e, r: L.pprhip_fora_whole_params(
            whole(a), e, C.byref(d1), C.byref(d2))),
        "pprhip_fora_topk_params": (("alpha", "eps"), lambda a, e, r: L.pprhip_fora_topk_params(
            topk(a), e, 0.1, C.byref(d1), C.byref(d2), C.byref(d3))),
    }


def _param_name(entry, p):
    if p == "alpha" and ("fora" in entry or "monte_carlo" in entry) and not entry.startswith(
            ("pprhip_conf_", "pprhip_fora_batch_topk")):
        return "conf->alpha"
    return p


def _expect_rejected(pkg, entry, name, rc):
    msg = _last(pkg)
    assert rc == pkg.ERR_INVALID, "%s accepted a bad %s (rc %d: %s)" % (entry, name, rc, msg)
    fn = entry.replace("_resident", "")  # (the resident call reports under the name of the call it extends)
    assert fn in msg and ("%s = " % name) in msg, "%s: the error does not name %s: %r" % (entry, name, msg)


ENTRY_NAMES = sorted(["pprhip_forward_push", "pprhip_fwdpush_topk_reset", "pprhip_fwdpush_topk_round",
                      "pprhip_random_walk_batch", "pprhip_fora_single_source", "pprhip_fora_topk", "pprhip_monte_carlo",
                      "pprhip_fora_batch_single_source", "pprhip_fora_batch_single_source_resident",
                      "pprhip_fora_stream_open", "pprhip_fora_batch_topk", "pprhip_forward_push_seeds",
                      "pprhip_fora_seeds", "pprhip_fora_topk_seeds", "pprhip_backward_push", "pprhip_all_pair_backward",
                      "pprhip_all_pair_backward_multi", "pprhip_all_pair_backward_sharded", "pprhip_shard_target_cuts",
                      "pprhip_fora_batch", "pprhip_power_method", "pprhip_conf_fora_whole_graph",
                      "pprhip_conf_fora_topk", "pprhip_fora_whole_params", "pprhip_fora_topk_params"])


def test_every_entry_point_is_covered(pkg_product):
    assert sorted(_entry_points(pkg_product)) == ENTRY_NAMES


@pytest.mark.parametrize("entry", ENTRY_NAMES)
def test_out_of_range_values_are_refused_before_the_handle(pkg_product, entry):
    pkg = pkg_product
    L = pkg.lib()
    params, call = _entry_points(pkg)[entry]
    checked = 0
    if entry == "pprhip_fwdpush_topk_round":
        for bad in BAD_THRESHOLD:
            _expect_rejected(pkg, entry, "min_rmax", L.pprhip_fwdpush_topk_round(None, bad, OK_RMAX, None, None))
            _expect_rejected(pkg, entry, "rmax", L.pprhip_fwdpush_topk_round(None, 1e-5, bad, None, None))
            checked += 2
    else:
        for p in params:
            bads = {"alpha": BAD_ALPHA, "eps": BAD_EPS}.get(p, BAD_THRESHOLD)
            for bad in bads:
                a, e, r = (bad if p == "alpha" else OK_ALPHA, bad if p == "eps" else OK_EPS,
                           bad if p in ("rmax", "threshold") else OK_RMAX)
                _expect_rejected(pkg, entry, _param_name(entry, p), call(a, e, r))
                checked += 1
    assert checked >= 2


@pytest.mark.parametrize("entry", [e for e in ENTRY_NAMES if not e.startswith(("pprhip_conf_", "pprhip_fora_whole_params",
                                                                                "pprhip_fora_topk_params"))])
def test_valid_values_still_fail_on_the_null_handle(pkg_product, entry):
    """In range, the call gets as far as it did before the checks: the NULL handle (per-GPU array, communicator)."""
    pkg = pkg_product
    L = pkg.lib()
    if entry == "pprhip_fwdpush_topk_round":
        rc = L.pprhip_fwdpush_topk_round(None, 1e-5, OK_RMAX, None, None)
    else:
        rc = _entry_points(pkg)[entry][1](OK_ALPHA, OK_EPS, OK_RMAX)
    msg = _last(pkg)
    assert rc in (pkg.ERR_INVALID, pkg.ERR_NO_DEVICE), (rc, msg)
    assert "outside (0, 1)" not in msg and "must be" not in msg and ("null" in msg or "handle" in msg), msg


@pytest.mark.parametrize("zero", ["rmax", "threshold", "min_rmax"])
def test_zero_thresholds_pass_the_check(pkg_product, zero):
    """0 is a legitimate threshold (the degenerate top-k configurations run at 0 and end by underflow)."""
    pkg = pkg_product
    L = pkg.lib()
    st = pkg.Stats()
    if zero == "rmax":
        rc = L.pprhip_forward_push(None, 0, OK_ALPHA, 0.0, None, None, None, C.byref(st))
    elif zero == "threshold":
        rc = L.pprhip_all_pair_backward(None, OK_ALPHA, 0.0, 8, 0, 1, C.byref(C.c_void_p()), C.byref(st))
    else:
        rc = L.pprhip_fwdpush_topk_round(None, 0.0, 0.0, None, None)
    assert rc == pkg.ERR_INVALID and "null graph handle" in _last(pkg)


@pytest.mark.parametrize("field,bad", [("delta", 0.0), ("delta", -1.0), ("delta", math.nan), ("delta", math.inf),
                                       ("pfail", 0.0), ("pfail", -0.5), ("pfail", math.nan), ("pfail", math.inf)])
def test_whole_graph_conf_fields(pkg_product, field, bad):
    pkg = pkg_product
    L = pkg.lib()
    st = pkg.Stats()
    c = _conf(pkg)
    setattr(c, field, bad)
    rc = L.pprhip_fora_single_source(None, 0, OK_EPS, C.byref(c), 1, 0, None, C.byref(st))
    _expect_rejected(pkg, "pprhip_fora_single_source", "conf->" + field, rc)
    rc = L.pprhip_fora_whole_params(C.byref(c), OK_EPS, C.byref(C.c_double()), C.byref(C.c_double()))
    _expect_rejected(pkg, "pprhip_fora_whole_params", "conf->" + field, rc)


def test_topk_conf_fields(pkg_product):
    """A top-k conf must have delta and min_delta finite and > 0 and pfail > 0; the values pprhip_conf_fora_topk derives
    for the degenerate configurations (pfail = inf at n div k = 1, -0 at k > n) still pass."""
    pkg = pkg_product
    L = pkg.lib()
    st = pkg.Stats()
    ids, vals, cnt = (C.c_int32 * 4)(), (C.c_double * 4)(), C.c_int(0)

    def call(c):
        return L.pprhip_fora_topk(None, 0, OK_EPS, C.byref(c), 1, ids, vals, 4, C.byref(cnt), None, C.byref(st))

    for field, bad in [("delta", 0.0), ("delta", math.nan), ("min_delta", 0.0), ("min_delta", -1.0),
                       ("min_delta", math.inf), ("pfail", -0.5), ("pfail", math.nan)]:
        c = _conf(pkg, topk=True)
        setattr(c, field, bad)
        _expect_rejected(pkg, "pprhip_fora_topk", "conf->" + field, call(c))
    for n, k in ((15, 10), (5, 10)):
        c = pkg.conf_topk(n, 40, k, OK_ALPHA)
        assert math.isinf(c.pfail) if n // k == 1 else c.pfail == 0.0
        assert call(c) == pkg.ERR_INVALID and "null graph handle" in _last(pkg)


def test_power_method_iters(pkg_product):
    pkg = pkg_product
    rc = pkg.lib().pprhip_power_method(None, 0, OK_ALPHA, -1, None, None)
    _expect_rejected(pkg, "pprhip_power_method", "iters", rc)
