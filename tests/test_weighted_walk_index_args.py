"""The weighted walk index (include/pprhip.h "weighted walk index") without a device: the checks of its five entry
points run in the order of the unweighted ones - alpha, then the density, then the handle - and every message carries
the name of the weighted call, never its unweighted namesake's."""
import ctypes as C
import math

import pytest

NAMES = ["build", "drop", "info", "fetch", "usage"]


def _last(pkg):
    return (pkg.lib().pprhip_last_error() or b"").decode()


def _named(pkg, call):
    """The last message names pprhip_weighted_walk_index_<call> (so it cannot be pprhip_walk_index_<call>'s)."""
    msg = _last(pkg)
    assert msg.startswith("pprhip_weighted_walk_index_%s: " % call), msg
    return msg


def test_the_package_declares_the_five_calls_and_the_release_bit(pkg_product):
    pkg = pkg_product
    for call in NAMES:
        name = "pprhip_weighted_walk_index_" + call
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name), name
    assert pkg.Graph.RELEASE_WEIGHTED_WALK_INDEX == pkg.RELEASE_WEIGHTED_WALK_INDEX == 256   # the next free bit
    bits = [pkg.Graph.RELEASE_ALL_PAIR, pkg.Graph.RELEASE_BATCH, pkg.Graph.RELEASE_WALK_INDEX, pkg.Graph.RELEASE_SWEEP,
            pkg.Graph.RELEASE_SPARSE, pkg.Graph.RELEASE_WEIGHTS, pkg.Graph.RELEASE_WEIGHTED_WALK_INDEX]
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 for b in bits)
    assert not {32, 64} & set(bits)            # the two flags the release tests use as the ones nobody knows
    for method in ("build_weighted_walk_index", "drop_weighted_walk_index", "weighted_walk_index_info",
                   "weighted_walk_index_terminals", "weighted_walk_index_usage"):
        assert callable(getattr(pkg.Graph, method))


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, math.nan, math.inf])
def test_build_checks_alpha_first(pkg_product, bad):
    pkg = pkg_product
    rc = pkg.lib().pprhip_weighted_walk_index_build(None, bad, 1, math.nan, None)     # (a bad density behind it)
    assert rc == pkg.ERR_INVALID
    assert "alpha = " in _named(pkg, "build")


@pytest.mark.parametrize("bad", [0.0, math.nan, math.inf, -1.0])
def test_build_checks_the_density_before_the_handle(pkg_product, bad):
    pkg = pkg_product
    rc = pkg.lib().pprhip_weighted_walk_index_build(None, 0.15, 1, bad, None)
    assert rc == pkg.ERR_INVALID
    assert "density = " in _named(pkg, "build")
    rc = pkg.lib().pprhip_weighted_walk_index_build(None, 0.15, 1, 0.25, None)        # in range: as far as the NULL handle
    assert rc == pkg.ERR_INVALID and "null graph handle" in _named(pkg, "build")


def test_null_handles(pkg_product):
    pkg = pkg_product
    L = pkg.lib()
    cnt, a, b = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.pprhip_weighted_walk_index_drop(None) == pkg.ERR_INVALID
    assert "null graph handle" in _named(pkg, "drop")
    assert L.pprhip_weighted_walk_index_fetch(None, 0, None, 0, C.byref(cnt)) == pkg.ERR_INVALID
    assert "null graph handle" in _named(pkg, "fetch")
    assert L.pprhip_weighted_walk_index_usage(None, C.byref(a), C.byref(b), 0) == pkg.ERR_INVALID
    assert "null graph handle" in _named(pkg, "usage")


def test_info_on_a_null_handle(pkg_product):
    pkg = pkg_product
    present, alpha, seed, density = C.c_int(7), C.c_double(7.0), C.c_uint64(7), C.c_double(7.0)
    terminals, nbytes = C.c_uint64(7), C.c_uint64(7)
    rc = pkg.lib().pprhip_weighted_walk_index_info(None, C.byref(present), C.byref(alpha), C.byref(seed), C.byref(density),
                                                  C.byref(terminals), C.byref(nbytes))
    assert rc == pkg.ERR_INVALID and "null graph handle" in _named(pkg, "info")
    assert (present.value, seed.value, terminals.value, nbytes.value) == (7, 7, 7, 7)   # nothing was written
    assert pkg.lib().pprhip_weighted_walk_index_info(None, None, None, None, None, None, None) == pkg.ERR_INVALID


def test_the_density_has_no_twin(pkg_product):
    """pprhip_walk_index_density serves both indexes: the weighted push test keeps the relationship count."""
    pkg = pkg_product
    assert "pprhip_weighted_walk_index_density" not in pkg.EXPORTS
    assert not hasattr(pkg.lib(), "pprhip_weighted_walk_index_density")
