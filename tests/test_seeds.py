"""Seed sets (PPR personalized to a weighted node set) without a device: the C ABI symbols, the Python wrappers, the
argument rules, and the numpy statement of the target (rule B: dead-end mass jumps to p) checked on closed forms.
The GPU half is tests/test_gpu_seeds.py, which uses `rule_b` below as its oracle."""
import ctypes as C

import numpy as np
import pytest

from conftest import edges_to_host, load_hooks_pkg

SEED_SYMBOLS = ["pprhip_forward_push_seeds", "pprhip_fora_seeds", "pprhip_fora_topk_seeds"]
ALPHA = 0.15


def rule_b(host, seeds, weights, alpha, tol=1e-14):
    """pi_p of the walk that starts at a node drawn from p, stops with probability alpha per step and jumps to a node
    drawn from p at a dead end: sum_t alpha (1 - alpha)^t x_t, x_0 = p, x_{t+1} = x_t M (M: a uniform out-edge, or p at
    a dead end).  Stops when the mass not yet summed, (1 - alpha)^t, is below tol."""
    n = host.n
    seeds = np.atleast_1d(np.asarray(seeds, dtype=np.int64))
    w = np.ones(seeds.size) if weights is None else np.atleast_1d(np.asarray(weights, dtype=np.float64))
    p = np.bincount(seeds, weights=w, minlength=n).astype(np.float64)
    p /= p.sum()
    out_rp = np.asarray(host.out_rp, dtype=np.int64)
    deg = np.diff(out_rp)
    src = np.repeat(np.arange(n), deg)
    dst = np.asarray(host.out_ci, dtype=np.int64)
    dead = deg == 0
    inv = np.where(dead, 0.0, 1.0 / np.maximum(deg, 1))
    x = p.copy()
    pi = np.zeros(n)
    left = 1.0
    while left > tol:
        pi += alpha * left * x
        nx = np.bincount(dst, weights=(x * inv)[src], minlength=n) + x[dead].sum() * p
        x = nx
        left *= 1.0 - alpha
    return pi


def seed_p(n, seeds, weights):
    """p: the weights normalized by their sum, duplicates summed (the dense vector of DESIGN §2 "Seed sets")."""
    seeds = np.atleast_1d(np.asarray(seeds, dtype=np.int64))
    w = np.ones(seeds.size) if weights is None else np.atleast_1d(np.asarray(weights, dtype=np.float64))
    p = np.bincount(seeds, weights=w, minlength=n).astype(np.float64)
    return p / p.sum()


def pi_p_left(host, p, x, alpha, tol=1e-18):
    """x^T Pi_p with Pi_p = alpha (I - (1 - alpha) P_p)^-1, P_p the random-walk matrix whose dead-end rows are p (row v of
    Pi_p: the walk from v that stops with probability alpha per step and restarts at p at a dead end).  Summed as the
    Neumann series alpha sum_t (1 - alpha)^t x^T P_p^t until the part not yet summed, (1 - alpha)^t |x|_1, is below tol:
    the same matrix as a dense solve (tests/test_oracle_seeds.py checks both agree), at the cost of sparse products."""
    n = host.n
    out_rp = np.asarray(host.out_rp, dtype=np.int64)
    deg = np.diff(out_rp)
    src = np.repeat(np.arange(n), deg)
    dst = np.asarray(host.out_ci, dtype=np.int64)
    dead = deg == 0
    inv = np.where(dead, 0.0, 1.0 / np.maximum(deg, 1))
    x = np.asarray(x, dtype=np.float64).copy()
    pi = np.zeros(n)
    left = float(np.abs(x).sum())
    while left > tol:
        pi += alpha * x
        x = (1.0 - alpha) * (np.bincount(dst, weights=(x * inv)[src], minlength=n) + x[dead].sum() * p)
        left *= 1.0 - alpha
    return pi


def exact_invariant_err(host, p, reserve, residue, alpha):
    """max |p^T Pi_p - (reserve + r^T Pi_p)|: the push invariant of a seed-set push, which holds at every rmax (the dead-end
    seeds' closed form keeps it exact); a landing error of any size shows here, not only one larger than rsum."""
    return float(np.max(np.abs(pi_p_left(host, p, p, alpha) - (reserve + pi_p_left(host, p, residue, alpha))),
                        initial=0.0))


def test_libraries_export_the_seed_entry_points(pkg_product):
    lib = pkg_product.lib()
    hooks = load_hooks_pkg().lib()
    for s in SEED_SYMBOLS:
        assert hasattr(lib, s), s
        assert hasattr(hooks, s), s
        assert s in pkg_product.EXPORTS


def test_python_wrappers_exist(pkg_product):
    for name in ("forward_push_seeds", "fora_seeds", "fora_topk_seeds"):
        assert callable(getattr(pkg_product.Graph, name, None)), name


def test_entry_points_without_a_device_fail_cleanly(pkg_product):
    lib = pkg_product.lib()
    s = (C.c_int32 * 2)(0, 1)
    conf = pkg_product.ForaConf()
    st = pkg_product.Stats()
    ok = (pkg_product.ERR_NO_DEVICE, pkg_product.ERR_INVALID)
    assert lib.pprhip_forward_push_seeds(None, s, None, 2, ALPHA, 1e-4, None, None, None, C.byref(st)) in ok
    assert lib.pprhip_fora_seeds(None, s, None, 2, 0.5, C.byref(conf), 1, 0, None, C.byref(st)) in ok
    ids, vals, nsel = (C.c_int32 * 4)(), (C.c_double * 4)(), C.c_int(0)
    conf.k = 4
    assert lib.pprhip_fora_topk_seeds(None, s, None, 2, 0.5, C.byref(conf), 1, ids, vals, 4, C.byref(nsel), None,
                                      C.byref(st)) in ok


def _normalize(pkg, n, seeds, weights):
    L = pkg.lib()
    L.pprhip_hook_seed_normalize.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.POINTER(C.c_int)]
    s = np.ascontiguousarray(seeds, dtype=np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    ids = np.zeros(max(s.size, 1), dtype=np.int32)
    p = np.zeros(max(s.size, 1))
    cnt = C.c_int(-1)
    rc = L.pprhip_hook_seed_normalize(n, s.ctypes.data if s.size else None, None if w is None else w.ctypes.data,
                                      s.size, ids.ctypes.data, p.ctypes.data, C.byref(cnt))
    return rc, ids[:max(cnt.value, 0)], p[:max(cnt.value, 0)]


@pytest.mark.hooks
def test_normalization_rules(pkg):
    rc, ids, p = _normalize(pkg, 10, [3, 1, 3, 7], None)
    assert rc == 0 and ids.tolist() == [1, 3, 7] and np.allclose(p, [0.25, 0.5, 0.25], rtol=0, atol=1e-16)
    rc, ids, p = _normalize(pkg, 10, [4, 2, 4, 9], [1.0, 0.0, 3.0, 4.0])  # duplicates summed, zero weight dropped
    assert rc == 0 and ids.tolist() == [4, 9] and np.allclose(p, [0.5, 0.5], rtol=0, atol=1e-16)
    assert abs(p.sum() - 1.0) <= 1e-15
    invalid = [([], None), ([10], None), ([-1], None), ([1, 2], [1.0, -0.5]), ([1], [float("nan")]),
               ([1], [float("inf")]), ([1, 2], [0.0, 0.0]), ([1, 2], [1e308, 1e308])]
    for seeds, w in invalid:
        rc, _, _ = _normalize(pkg, 10, seeds, w)
        assert rc == -1, (seeds, w)


def _parse_set(pkg, n, ids_in, weights, normalize, noun):
    """The parser the seed sets and the target sets share, through its hook: (rc, ids, weights, message)."""
    L = pkg.lib()
    L.pprhip_hook_parse_weighted_set.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_char_p,
                                                  C.c_char_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    s = np.ascontiguousarray(ids_in, dtype=np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    ids = np.zeros(max(s.size, 1), dtype=np.int32)
    out = np.zeros(max(s.size, 1))
    cnt = C.c_int(-1)
    rc = L.pprhip_hook_parse_weighted_set(n, s.ctypes.data if s.size else None, None if w is None else w.ctypes.data,
                                          s.size, int(normalize), noun.encode(), b"caller", ids.ctypes.data,
                                          out.ctypes.data, C.byref(cnt))
    msg = L.pprhip_last_error().decode("utf-8", "replace") if rc != 0 else ""
    return rc, ids[:max(cnt.value, 0)], out[:max(cnt.value, 0)], msg


# sets of at most 12 entries; the weights of a repeated id are dyadic, so their sum is exact in any order
PARSED_SETS = [
    ([3, 1, 3, 7], None),                                                       # duplicates, uniform weights
    ([4, 2, 4, 9], [1.0, 0.0, 3.0, 4.0]),                                       # ... and a zero weight
    ([5], [0.3]),                                                               # a lone member, weight not 1
    ([5], None),
    ([11, 0, 6, 0, 2, 11, 8, 0, 6, 3, 9, 1],
     [0.5, 0.25, 0.1, 0.125, 0.7, 1.5, 0.0, 2.0, 0.3, 1e-9, 3.3, 0.0]),         # 12 entries, 0 three times, 6 and 11 twice
]


@pytest.mark.hooks
@pytest.mark.parametrize("noun", ["seed", "target"])
def test_shared_set_parser_against_numpy_and_the_seed_hook(pkg, noun):
    n = 12
    for ids_in, w in PARSED_SETS:
        wv = np.ones(len(ids_in)) if w is None else np.asarray(w, dtype=np.float64)
        dense = np.bincount(np.asarray(ids_in), weights=wv, minlength=n)  # (per id: one weight, a + b, or dyadic sums)
        want_ids = np.flatnonzero(dense > 0)
        rc, ids, got, _ = _parse_set(pkg, n, ids_in, w, False, noun)
        assert rc == 0 and ids.tolist() == want_ids.tolist(), (ids_in, w)
        assert got.tolist() == dense[want_ids].tolist(), (ids_in, w)  # unchanged, duplicates as their sum: exactly
        rc, ids, got, _ = _parse_set(pkg, n, ids_in, w, True, noun)
        rc0, ids0, p0 = _normalize(pkg, n, ids_in, w)
        assert rc == 0 and rc0 == 0 and ids.tolist() == ids0.tolist()
        assert got.tobytes() == p0.tobytes(), (ids_in, w)  # bit for bit what the seed-set entry points get
        # against numpy: two sums of k <= 12 non-negative terms differ by at most 2 (k - 1) u, each division adds u
        assert np.allclose(got, dense[want_ids] / wv.sum(), rtol=24 * 2.0 ** -53, atol=0)


@pytest.mark.hooks
@pytest.mark.parametrize("noun", ["seed", "target"])
@pytest.mark.parametrize("normalize", [False, True])
def test_shared_set_parser_refusals_name_the_noun(pkg, noun, normalize):
    n = 12
    refused = [([], None),                                  # the empty set
               ([n], None), ([1, n, 2], [1.0, 1.0, 1.0]),   # an id of n
               ([1, 2], [1.0, -0.5]),                       # a negative weight
               ([1], [float("nan")]),                       # a NaN weight
               ([1, 2, 2], [0.0, 0.0, 0.0])]                # all-zero weights
    for ids_in, w in refused:
        rc, ids, got, msg = _parse_set(pkg, n, ids_in, w, normalize, noun)
        assert rc == pkg.ERR_INVALID and ids.size == 0 and got.size == 0, (ids_in, w)
        assert msg.startswith("caller: ") and noun in msg, msg  # (the calling function's name, then the noun)


# ------------------------------------------------------------------ the rule-B oracle on closed forms
def test_rule_b_cycle_two_seeds_is_linear(pkg_product):
    n = 5
    host = edges_to_host(pkg_product, n, [(i, (i + 1) % n) for i in range(n)])
    a = ALPHA

    def single(s):
        v = np.zeros(n)
        for k in range(n):
            v[(s + k) % n] = a * (1 - a) ** k / (1 - (1 - a) ** n)
        return v

    got = rule_b(host, [1, 3], [0.3, 0.7], a)
    assert np.max(np.abs(got - (0.3 * single(1) + 0.7 * single(3)))) <= 1e-13


def test_rule_b_star_with_dead_end_leaves(pkg_product):
    host = edges_to_host(pkg_product, 6, [(0, i) for i in range(1, 6)])
    a = ALPHA
    # from the centre: stop, or a leaf; at a leaf stop, or back to p = {0}
    c = a / (1 - (1 - a) ** 2)
    want = np.array([c] + [c * (1 - a) / 5] * 5)
    assert np.max(np.abs(rule_b(host, [0], None, a) - want)) <= 1e-13
    # p = {centre: 1/2, leaf 1: 1/2}: pi = a p (I - (1 - a) M)^-1, every leaf's row of M being p
    p = np.array([0.5, 0.5, 0, 0, 0, 0])
    M = np.zeros((6, 6))
    M[0, 1:] = 0.2
    for leaf in range(1, 6):
        M[leaf] = p
    want = a * p @ np.linalg.inv(np.eye(6) - (1 - a) * M)
    assert np.max(np.abs(rule_b(host, [0, 1], None, a) - want)) <= 1e-13


def test_rule_b_every_seed_a_dead_end_is_p(pkg_product):
    host = edges_to_host(pkg_product, 6, [(0, i) for i in range(1, 6)])
    got = rule_b(host, [2, 4, 5, 4], None, ALPHA)
    assert np.max(np.abs(got - np.array([0, 0, 0.25, 0, 0.5, 0.25]))) <= 1e-13
