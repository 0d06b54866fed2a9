"""Single pairs without a device: pprhip_pair_params against its closed forms (include/pprhip.h "single pairs",
DESIGN.md §2 "Single pairs"), and the range checks of the three pair entry points with a NULL handle - a bad alpha,
eps or rmax must be refused with PPRHIP_ERR_INVALID and a message that names the parameter, before the handle is
looked at (a NULL handle would otherwise be the error)."""
import ctypes as C
import math

import pytest

BAD_ALPHA = [0.0, -0.1, 1.0, 1.5, math.nan, math.inf]
BAD_EPS = [0.0, -1.0, math.nan, math.inf]
BAD_RMAX = [-1e-6, 1.0000001, 2.0, math.nan, math.inf]


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


def _closed_form(n, m, eps, delta, pfail, rmax_in=0.0):
    lg = math.log(2.0 / pfail)
    omega = 3.0 * lg / (eps * eps) / delta
    rmax = rmax_in
    if rmax == 0.0:
        rmax = min(1.0, eps * math.sqrt((m / n) * delta / (3.0 * lg)))
    return rmax, math.ceil(omega * rmax)


@pytest.mark.parametrize("n,m,alpha,eps", [(1 << 22, 16 << 22, 0.15, 0.5), (107, 352, 0.15, 0.2),
                                           (4096, 65536, 0.05, 0.3), (1000, 5000, 0.5, 0.1), (50, 49, 0.2, 1.0)])
def test_pair_params_closed_form_whole_graph_conf(pkg, n, m, alpha, eps):
    conf = pkg.conf_whole_graph(n, m, alpha)
    rmax, walks = pkg.pair_params(conf, eps)
    er, ew = _closed_form(n, m, eps, 1.0 / n, 1.0 / n)
    assert rmax == pytest.approx(er, rel=1e-14) and 0.0 < rmax <= 1.0
    assert walks == ew


@pytest.mark.parametrize("delta,pfail", [(1e-3, 1e-4), (0.01, 0.5), (1e-6, 1e-9)])
def test_pair_params_closed_form_own_delta_pfail(pkg, delta, pfail):
    conf = pkg.conf_whole_graph(10000, 200000, 0.15)
    conf.delta, conf.pfail = delta, pfail
    rmax, walks = pkg.pair_params(conf, 0.4)
    er, ew = _closed_form(10000, 200000, 0.4, delta, pfail)
    assert rmax == pytest.approx(er, rel=1e-14)
    assert walks == ew


def test_pair_params_arithmetic_of_the_issue_at_rmat22(pkg):
    rmax, walks = pkg.pair_params(pkg.conf_whole_graph(1 << 22, 16 << 22, 0.15), 0.5)
    assert 1.3e-4 < rmax < 1.5e-4 and 1.0e5 < walks < 1.2e5


def test_pair_params_explicit_rmax_passes_through(pkg):
    conf = pkg.conf_whole_graph(4096, 65536, 0.15)
    for r in (1e-6, 3e-3, 0.5, 1.0):
        rmax, walks = pkg.pair_params(conf, 0.5, r)
        assert rmax == r
        assert walks == _closed_form(4096, 65536, 0.5, 1.0 / 4096, 1.0 / 4096, r)[1]


def test_pair_params_default_clamped_to_one(pkg):
    # a dense graph with a large eps: the balanced threshold would exceed 1
    conf = pkg.conf_whole_graph(4, 4000, 0.15)
    lg = math.log(8.0)
    assert 5.0 * math.sqrt(1000.0 * 0.25 / (3.0 * lg)) > 1.0
    rmax, walks = pkg.pair_params(conf, 5.0)
    assert rmax == 1.0
    assert walks == math.ceil(3.0 * math.log(8.0) / 25.0 / 0.25)


def _pair_calls(pkg):
    """name -> call(conf, eps, rmax) with a NULL handle (pprhip_walk_survival takes alpha = conf.alpha)."""
    L = pkg.lib()
    r, w = C.c_double(), C.c_uint64()
    s1 = (C.c_int32 * 1)(0)
    out = (C.c_double * 1)()
    st = pkg.Stats()
    return {
        "pprhip_pair_params": (("alpha", "eps", "rmax"),
                               lambda c, e, x: L.pprhip_pair_params(C.byref(c), e, x, C.byref(r), C.byref(w))),
        "pprhip_walk_survival": (("alpha",), lambda c, e, x: L.pprhip_walk_survival(None, c.alpha, None)),
        "pprhip_ppr_pairs": (("alpha", "eps", "rmax"),
                             lambda c, e, x: L.pprhip_ppr_pairs(None, s1, s1, 1, e, C.byref(c), x, 1, out,
                                                                C.byref(st))),
    }


@pytest.mark.parametrize("name", ["pprhip_pair_params", "pprhip_walk_survival", "pprhip_ppr_pairs"])
def test_pair_entry_points_reject_bad_alpha(pkg, name):
    takes, call = _pair_calls(pkg)[name]
    for a in BAD_ALPHA:
        c = pkg.conf_whole_graph(100, 1000, 0.15)
        c.alpha = a
        assert call(c, 0.5, 0.0) == pkg.ERR_INVALID, (name, a)
        msg = _last(pkg)
        assert name in msg and "alpha" in msg, (name, a, msg)


@pytest.mark.parametrize("name", ["pprhip_pair_params", "pprhip_ppr_pairs"])
def test_pair_entry_points_reject_bad_eps_and_rmax(pkg, name):
    _, call = _pair_calls(pkg)[name]
    c = pkg.conf_whole_graph(100, 1000, 0.15)
    for e in BAD_EPS:
        assert call(c, e, 0.0) == pkg.ERR_INVALID, (name, e)
        msg = _last(pkg)
        assert name in msg and "eps" in msg, (name, e, msg)
    for x in BAD_RMAX:
        assert call(c, 0.5, x) == pkg.ERR_INVALID, (name, x)
        msg = _last(pkg)
        assert name in msg and "rmax" in msg, (name, x, msg)


def test_ppr_pairs_good_parameters_reach_the_handle_check(pkg):
    """With every parameter in range the NULL handle is what fails (the checks above are about the parameters)."""
    _, call = _pair_calls(pkg)["pprhip_ppr_pairs"]
    assert call(pkg.conf_whole_graph(100, 1000, 0.15), 0.5, 1e-3) == pkg.ERR_INVALID
    assert "null graph handle" in _last(pkg)


def test_pair_walk_stream_constant(pkg):
    import os
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pprhip.h")
    assert "#define PPRHIP_PAIR_WALK_STREAM 0xFFFFu" in open(hdr).read()
    assert pkg.PAIR_WALK_STREAM == 0xFFFF
