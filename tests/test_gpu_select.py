"""The top-k radix select (kernels_select.hip, driven by select_finish / select_topk_passes in select.cpp) past its
first pass and past its candidate buffer, and the same overflow in the backward search (finish_search in bwd_runs.cpp).

A seed set whose seeds are all dead ends leaves reserve = w / sum(w) and runs no level (seeds.cpp: seed_plan), so on an
out-star the seed weights load any vector into the reserve, up to one common correctly rounded division;
pprhip_topk_select then selects over exactly that vector.  Every expectation is computed from the vector the call
returned, by the oracle's qsort (orc.topk, orc.kth_largest) checked once per vector against np.lexsort; the select only
moves values, so ids, order, values, n_sel and kth are compared exactly.  `select_path` below is a numpy model of the two
drivers: every case asserts Stats.select_passes against it, so a case that took another path than it names fails.

Paths by (family, k), from `select_path` over w / cumsum(w)[-1] (the vector the seed load leaves; each case asserts
its own path against the fetched vector at run time).  fast / fast2: one pass, candidates in the read-back prefix / by a
second copy; pNN: the multi-pass form stopped at pbits = NN; whole: all six histograms, gather overflow, whole-vector
finish (7 passes counted); all-whole: no k-th, one histogram, whole-vector finish (2 passes counted).

    k                  s4      s16     s28     s40     uniform  equal
    1, 100             fast    fast    fast    fast    fast2    fast
    101, 5000          p60     p48     p36     p24     fast2    whole
    200000             p60     p60     p36     p36     p24      whole
    2^18 - 100         whole   p60     p48     p36     p24      whole
    2^18               whole   whole   p60     p48     p36      whole
    2^18 + 1, + 101    whole   whole   whole   whole   whole    whole
    entries (271436)   whole   whole   whole   whole   whole    whole
    entries + 1        all-whole in every family

The other cases: candidate-count edge 2047 / 2048 (fast) and 2049 (fast2); wide range, small-after-large, isolated
seeds, tiny-after-whole: fast, and "all" for k > entries; fora_topk_seeds s16 k = 101: p48; fora_batch_topk_seeds
k = 128: p48, whole, all; all_pair_backward from tier 3: the finish_search overflow.
Wall time of this file on an MI355X: 6.5 s for its 25 cases (pytest's total); the slowest, a family of 11 selects with
the oracle's sorts, takes 0.9 s.
"""
import numpy as np
import pytest

from conftest import shared_graph, to_oracle

pytestmark = pytest.mark.gpu

A = 0.15
EPS = 0.5
TOL_PUSH = 1e-12  # as tests/test_gpu_parity.py: the engine and the twin differ in fp64 addition order only

SEL_CAP = 1 << 18  # graph.cpp: alloc_workspace, G->sel_cap (records the candidate buffer holds)
SEL_PRE = 2048     # select.cpp: kSelPre (records the fast path's one read-back brings along)

N_CLUSTER = (1 << 18) + 8192
N_HEAD, N_TAIL = 100, 1000
N_LEAVES = N_CLUSTER + N_HEAD + N_TAIL
N_STAR = 1 + N_LEAVES
ONE_BITS = 0x3FF0000000000000  # the bit pattern of 1.0

FAMILIES = ("s4", "s16", "s28", "s40", "uniform", "equal")
# the paths each family is there for (the table in the module docstring); each test asserts that its cases reached them
FAMILY_PATHS = {
    "s4": {"fast", "passes60", "whole"},
    "s16": {"fast", "passes48", "passes60", "whole"},
    "s28": {"fast", "passes36", "passes48", "passes60", "whole"},
    "s40": {"fast", "passes24", "passes36", "passes48", "whole"},
    "uniform": {"fast2", "passes24", "passes36", "whole"},
    "equal": {"fast", "whole"},
}


# ------------------------------------------------------------------ the path model
def select_path(p, k):
    """What select_finish and select_topk_passes (select.cpp) do with the vector p and k, from their histograms alone:
    (path, select_passes, candidates).  path: "empty" (no entry > 0), "fast" / "fast2" (one pass; fast2: more than
    SEL_PRE candidates, fetched by a second copy), "passesNN" (the multi-pass form stopped at pbits = NN with at most
    SEL_CAP candidates), "whole" (it ran to pbits = 64, the gather overflowed and the host finished on the whole
    vector), and for k > entries "all" (fast path) / "all-whole" (one histogram, then the whole vector).  select_passes:
    1 for the fast path, 1 + the histograms of the multi-pass form otherwise."""
    bits = np.ascontiguousarray(p, dtype=np.float64).view(np.uint64)
    bits = bits[p > 0.0]
    total = int(bits.size)
    if total == 0:
        return "empty", 1, 0
    # k_select_hist<true> over the 12 leading bits + k_select_choose
    if k > total:
        expected = total
    else:
        hist = np.bincount((bits >> np.uint64(52)).astype(np.int64), minlength=4096)
        above = 0
        for b in range(4095, -1, -1):
            if above < k <= above + hist[b]:
                break
            above += int(hist[b])
        expected = above + int(hist[b])
    if expected <= SEL_CAP:  # select_finish: cnt <= kPre, or the second copy
        name = "all" if k > total else "fast"
        return (name + "2" if expected > SEL_PRE and name == "fast" else name), 1, expected
    # select_topk_passes
    if k > total:
        return "all-whole", 2, total
    prefix, pbits, k_rem, above, hists = 0, 0, k, 0, 0
    while pbits < 64:
        dbits = min(12, 64 - pbits)
        shift = np.uint64(64 - pbits - dbits)
        cand = bits if pbits == 0 else bits[(bits >> np.uint64(64 - pbits)) == np.uint64(prefix)]
        hist = np.bincount(((cand >> shift) & np.uint64((1 << dbits) - 1)).astype(np.int64), minlength=1 << dbits)
        hists += 1
        cum = 0
        for b in range((1 << dbits) - 1, -1, -1):
            if cum + hist[b] >= k_rem:
                break
            cum += int(hist[b])
        above += cum
        k_rem -= cum
        prefix = (prefix << dbits) | b
        pbits += dbits
        expected = above + int(hist[b])
        if expected <= SEL_CAP:
            return "passes%d" % pbits, 1 + hists, expected
    return "whole", 1 + hists, expected


# ------------------------------------------------------------------ vectors and graphs
def family_weights(name, seed=1):
    """The N_LEAVES weights of a family, by leaf (leaf i is node i + 1): the cluster, 100 head entries in [2, 3) and
    1000 tail entries in [2^-10, 2^-9), shuffled."""
    rng = np.random.default_rng(seed)
    if name == "uniform":
        cluster = rng.uniform(1.0, 2.0, size=N_CLUSTER)
    elif name == "equal":
        cluster = np.ones(N_CLUSTER)
    else:
        s = int(name[1:])
        j = rng.integers(0, 1 << s, size=N_CLUSTER, dtype=np.uint64)
        cluster = (np.uint64(ONE_BITS) + j).view(np.float64)
    head = rng.uniform(2.0, 3.0, size=N_HEAD)
    tail = rng.uniform(2.0 ** -10, 2.0 ** -9, size=N_TAIL)
    w = np.concatenate([cluster, head, tail])
    rng.shuffle(w)
    return w


def family_ks(npos):
    return [1, 100, 101, 5000, 200000, SEL_CAP - 100, SEL_CAP, SEL_CAP + 1, SEL_CAP + 101, npos, npos + 1]


def shuffled_seeds(ids, w, seed=7):
    """the set in a shuffled order (parse_weighted_set sorts it by id again)"""
    perm = np.random.default_rng(seed).permutation(len(ids))
    return np.asarray(ids, dtype=np.int32)[perm], np.asarray(w, dtype=np.float64)[perm]


def out_star(pkg, n, n_isolated=0):
    """node 0 -> every node in [1, n - n_isolated): those are dead ends with one in-edge; the rest has no edge"""
    dst = np.arange(1, n - n_isolated, dtype=np.int32)
    return pkg.HostCsr(n, np.zeros(dst.size, dtype=np.int32), dst)


def in_star(pkg, n):
    """every leaf -> the hub, node 0"""
    src = np.arange(1, n, dtype=np.int32)
    return pkg.HostCsr(n, src, np.zeros(src.size, dtype=np.int32))


@pytest.fixture
def dev_star(pkg, dev_cache):
    return shared_graph(dev_cache, pkg, "dev_star", lambda: pkg.Graph(out_star(pkg, N_STAR)))


N_ISO_GRAPH, N_ISO = 3000, 2000  # the second graph: a hub, 999 leaves and 2000 isolated nodes


@pytest.fixture
def dev_iso(pkg, dev_cache):
    return shared_graph(dev_cache, pkg, "dev_iso", lambda: pkg.Graph(out_star(pkg, N_ISO_GRAPH, N_ISO)))


def load(dev, ids, w):
    """the weights w on the dead ends ids as the reserve vector; returns the vector the call leaves"""
    s, ws = shuffled_seeds(ids, w)
    p, r, rsum, st = dev.forward_push_seeds(s, A, 1e-6, weights=ws)
    assert rsum == 0.0 and not r.any() and st.levels == 0
    return p


def load_family(dev, name):
    return load(dev, np.arange(1, N_STAR), family_weights(name))


class Expect:
    """The expected answers over one fetched vector.  The lists are the oracle's; one np.lexsort per vector checks
    them (every list is a prefix of that order)."""

    def __init__(self, orc, p):
        self.orc, self.p = orc, p
        self.npos = int((p > 0.0).sum())
        self.order = np.lexsort((np.arange(p.size), -p))[:self.npos].astype(np.int32)

    def topk(self, k):
        cnt, oids, ovals = self.orc.topk(self.p, k)
        okth = self.orc.kth_largest(self.p, k)
        assert np.array_equal(oids, self.order[:cnt]) and np.array_equal(ovals, self.p[self.order[:cnt]])
        if k <= self.npos:
            assert okth == self.p[self.order[k - 1]] and cnt == int((self.p >= okth).sum())
        else:
            assert okth is None and cnt == self.npos
        return cnt, oids, ovals, okth


def check_select(dev, ex, k, what):
    """one pprhip_topk_select over the vector of ex: the path the model names (by select_passes) and the exact answer"""
    path, passes, _ = select_path(ex.p, k)
    n_sel, ids, vals, kth, st = dev.topk_select(k, cap=ex.p.size)
    print("%s k=%d: %s, select_passes %d (model %d), n_sel %d" % (what, k, path, st.select_passes, passes, n_sel))
    assert st.select_passes == passes, (what, k, path, st.select_passes, passes)
    cnt, oids, ovals, okth = ex.topk(k)
    assert n_sel == cnt, (what, k, path)
    assert np.array_equal(ids, oids), (what, k, path)
    assert np.array_equal(vals, ovals), (what, k, path)
    assert (okth is None and kth == 0.0) or okth == kth, (what, k, path)
    return path


# ------------------------------------------------------------------ 1. the model and the builders, without a device
def test_model_and_builders():
    """(plain numpy: this part also runs where the file is tried without a device)"""
    assert select_path(np.zeros(5), 3) == ("empty", 1, 0)
    v = np.array([0.0, 3.0, 1.5, 1.25, 0.0, 2.0 ** -1074])
    assert select_path(v, 1) == ("fast", 1, 1)
    assert select_path(v, 3) == ("fast", 1, 3)      # 1.5 and 1.25 share the leading 12 bits
    assert select_path(v, 4) == ("fast", 1, 4)      # a denormal is an entry
    assert select_path(v, 5) == ("all", 1, 4)
    ties = np.full(SEL_CAP + 1, 0.5)
    assert select_path(ties, 1) == ("whole", 7, SEL_CAP + 1)
    assert select_path(ties, SEL_CAP + 2) == ("all-whole", 2, SEL_CAP + 1)
    assert select_path(ties[:SEL_CAP], SEL_CAP) == ("fast2", 1, SEL_CAP)
    assert select_path(ties[:SEL_PRE], 1) == ("fast", 1, SEL_PRE)
    # more than SEL_CAP entries of one binade, 4096 values that differ in the next 12 bits: one more digit separates them
    x = (np.uint64(ONE_BITS) + ((np.arange(SEL_CAP + 4096, dtype=np.uint64) % np.uint64(4096)) << np.uint64(40))).view(np.float64)
    assert select_path(x, 1) == ("passes24", 3, 65) and select_path(x, 66) == ("passes24", 3, 130)
    # ... and in the last four bits only: all six histograms
    y = (np.uint64(ONE_BITS) + (np.arange(SEL_CAP + 16, dtype=np.uint64) & np.uint64(15))).view(np.float64)
    assert select_path(y, 1) == ("passes64", 7, (SEL_CAP + 16) // 16)
    for name in FAMILIES:
        w = family_weights(name)
        assert w.size == N_LEAVES and np.all(w > 0.0) and np.array_equal(w, family_weights(name))
        assert int(((w >= 1.0) & (w < 2.0)).sum()) == N_CLUSTER and int((w >= 2.0).sum()) == N_HEAD
        p = w / np.cumsum(w)[-1]  # what parse_weighted_set makes of it (sum in id order, one division per entry)
        got = {select_path(p, k)[0] for k in family_ks(N_LEAVES)}
        assert FAMILY_PATHS[name] | {"all-whole"} <= got, (name, got)


# ------------------------------------------------------------------ 2. the vector families
@pytest.mark.parametrize("family", FAMILIES)
def test_select_families(orc, dev_star, family):
    """2^18 + 8192 entries in one binade (16 adjacent values; 2^16, 2^28, 2^40 values next to 1.0; distinct mantissas;
    all equal) under 100 larger and over 1000 smaller ones, for k on both sides of every limit of the two drivers."""
    p = load_family(dev_star, family)
    ex = Expect(orc, p)
    assert ex.npos == N_LEAVES and p[0] == 0.0
    seen = {check_select(dev_star, ex, k, family) for k in family_ks(ex.npos)}
    assert FAMILY_PATHS[family] | {"all-whole"} <= seen, (family, seen)


# ------------------------------------------------------------------ 3. edges of the fast path
@pytest.mark.parametrize("count", [SEL_PRE - 1, SEL_PRE, SEL_PRE + 1])
def test_candidate_count_edge(orc, dev_star, count):
    """Exactly count candidates at or above the chosen bin's lower edge - the prefix of the one read-back holds them
    (cnt <= kPre) or a second copy fetches them - over 40 entries of lower binades that no candidate list may hold;
    and k = the entries, one more, and 1 (k_select_choose: the lowest bin, no bin, the highest)."""
    rng = np.random.default_rng(count)
    ids = rng.choice(np.arange(1, N_STAR), size=count + 40, replace=False)
    w = np.concatenate([rng.uniform(1.0, 2.0, size=count), rng.uniform(2.0 ** -20, 2.0 ** -19, size=40)])
    p = load(dev_star, ids, w)
    ex = Expect(orc, p)
    assert ex.npos == count + 40
    path, _, cand = select_path(p, count)  # the bin of the count-th largest is the lowest that a larger entry is in
    assert cand == count and path == ("fast2" if count > SEL_PRE else "fast")
    assert check_select(dev_star, ex, count, "edge %d" % count) == path
    assert check_select(dev_star, ex, ex.npos, "edge %d" % count) == ("fast2" if ex.npos > SEL_PRE else "fast")
    assert check_select(dev_star, ex, ex.npos + 1, "edge %d" % count) == "all"
    assert check_select(dev_star, ex, 1, "edge %d" % count) == "fast"


def test_wide_range_and_denormals(orc, dev_star):
    """Weights over 60 binades, some so small that w / sum is denormal or underflows to 0.  The entries of the fetched
    vector that are > 0.0 are the expectation: a denormal counts as an entry (the lowest bin of the first histogram, whose
    lower edge is the pattern 0), an underflowed one is no entry."""
    rng = np.random.default_rng(5)
    ids = rng.choice(np.arange(1, N_STAR), size=600 + 8, replace=False)
    w = np.concatenate([rng.uniform(1.0, 2.0, size=600) * 2.0 ** rng.integers(-50, 11, size=600),
                        2.0 ** np.array([-1030.0, -1040.0, -1045.0, -1050.0, -1073.0, -1074.0, -1074.0, -1074.0])])
    p = load(dev_star, ids, w)
    ex = Expect(orc, p)
    tiny = p[ids[600:]]
    assert w.sum() > 1024.0 and int((tiny == 0.0).sum()) == 4       # w / sum underflowed ...
    assert int(((tiny > 0.0) & (tiny < 2.0 ** -1022)).sum()) == 4   # ... or is denormal
    assert ex.npos == 600 + int((tiny > 0.0).sum())
    for k in (1, 7, 600, 601, ex.npos - 1, ex.npos, ex.npos + 1):
        assert check_select(dev_star, ex, k, "wide") in ("fast", "all")


def test_small_set_after_large(orc, dev_star):
    """A set of 9 seeds straight after one of every leaf: what the larger set left is gone from the reserve, and the
    select sees the 9 entries only."""
    big = load_family(dev_star, "uniform")
    assert int((big > 0.0).sum()) == N_LEAVES
    ids = np.array([5, 77, 4096, 4097, 100000, SEL_CAP, SEL_CAP + 1, N_STAR - 2, N_STAR - 1])
    p = load(dev_star, ids, np.array([3.0, 1.0, 1.0, 2.0, 0.5, 1.0, 7.0, 0.25, 1.0]))
    assert np.array_equal(dev_star.reserve(), p)
    want = np.zeros(N_STAR)
    want[ids] = np.array([3.0, 1.0, 1.0, 2.0, 0.5, 1.0, 7.0, 0.25, 1.0]) / 16.75
    assert np.array_equal(p, want)
    ex = Expect(orc, p)
    for k in (1, 3, 4, 9, 10):
        assert check_select(dev_star, ex, k, "small after large") in ("fast", "all")


def test_isolated_seeds(orc, dev_iso):
    """Isolated nodes as seeds: their internal ids lie past the nodes with edges, so the passes of the query cover all
    n entries (reset_query_state), and a set of leaves only afterwards covers the nodes with edges and finds the rest
    cleared."""
    rng = np.random.default_rng(9)
    leaves = rng.choice(np.arange(1, N_ISO_GRAPH - N_ISO), size=300, replace=False)
    iso = rng.choice(np.arange(N_ISO_GRAPH - N_ISO, N_ISO_GRAPH), size=700, replace=False)
    for ids in (np.concatenate([leaves, iso]), iso, leaves[:50], np.concatenate([iso[:3], [N_ISO_GRAPH - 1]])):
        w = rng.uniform(0.5, 4.0, size=ids.size)
        w[::7] = 1.0  # ties
        p = load(dev_iso, ids, w)
        assert np.array_equal(dev_iso.reserve(), p)
        ex = Expect(orc, p)
        assert ex.npos == ids.size and not p[np.setdiff1d(np.arange(N_ISO_GRAPH), ids)].any()
        for k in (1, 10, ids.size // 2, ids.size, ids.size + 1):
            check_select(dev_iso, ex, k, "isolated %d" % ids.size)


# ------------------------------------------------------------------ 4. the other entry points
def test_fora_topk_seeds_through_passes(pkg, orc, dev_star):
    """pprhip_fora_topk_seeds over the s = 16 family at k = 101.  Every seed is a dead end: no round and no walk runs,
    the estimate is p (topk_step: kTopkRoundStart -> kTopkFinal) and the query's one selection - over the estimate
    vector - falls into the multi-pass form."""
    p = load_family(dev_star, "s16")
    ex = Expect(orc, p)
    path, passes, _ = select_path(p, 101)
    assert path.startswith("passes")
    want = dev_star.topk_select(101, cap=N_STAR)
    s, ws = shuffled_seeds(np.arange(1, N_STAR), family_weights("s16"))
    n_sel, ids, vals, est, st = dev_star.fora_topk_seeds(s, EPS, A, 101, seed=3, weights=ws, cap=N_STAR, fetch=True)
    assert st.walks == 0 and st.select_passes == passes
    assert np.array_equal(est, p) and np.array_equal(dev_star.reserve(), p)
    assert n_sel == want[0] and np.array_equal(ids, want[1]) and np.array_equal(vals, want[2])
    cnt, oids, ovals, okth = ex.topk(101)
    assert n_sel == cnt and np.array_equal(ids, oids) and np.array_equal(vals, ovals)
    assert check_select(dev_star, ex, 101, "after fora_topk_seeds") == path  # (now over the estimate vector)


def test_fora_batch_topk_seeds_through_passes(pkg, orc, dev_star):
    """Three sets in one pprhip_fora_batch_topk_seeds call at k = 128: the s = 16 family (multi-pass form), the all-equal
    family (whole-vector finish) and a small set (fast path), each on a batch workspace.  Row i is the single-set call
    cut to k columns and padded with -1 / 0.0, as test_fora_batch_topk asserts - and the oracle's list over p."""
    k = 128
    all_ids = np.arange(1, N_STAR)
    small_ids = np.array([9, 10, 11, 70000, N_STAR - 1])
    sets = [shuffled_seeds(all_ids, family_weights("s16")), shuffled_seeds(all_ids, family_weights("equal")),
            shuffled_seeds(small_ids, np.array([1.0, 2.0, 2.0, 5.0, 0.5]))]
    ids, vals, st = dev_star.fora_batch_topk_seeds([s for s, _ in sets], k, EPS, A, seed=11, weights=[w for _, w in sets])
    assert ids.shape == (3, k) and st.walks == 0
    paths, passes = [], 0
    for i, (s, w) in enumerate(sets):
        nsel, sids, svals, est, sst = dev_star.fora_topk_seeds(s, EPS, A, k, seed=11 + i, weights=w, cap=k, fetch=True)
        path, n_pass, _ = select_path(est, k)
        assert sst.select_passes == n_pass and sst.walks == 0
        paths.append(path)
        passes += n_pass
        m = min(nsel, k)
        assert np.array_equal(ids[i][:m], sids[:m]) and np.array_equal(vals[i][:m], svals[:m])
        assert np.all(ids[i][m:] == -1) and np.all(vals[i][m:] == 0.0)
        cnt, oids, ovals, _ = Expect(orc, est).topk(k)
        assert nsel == cnt and np.array_equal(ids[i][:m], oids[:m]) and np.array_equal(vals[i][:m], ovals[:m])
    assert paths[0].startswith("passes") and paths[1:] == ["whole", "all"], paths
    assert st.select_passes == passes


def test_fast_path_after_whole_vector_finish(orc, dev_star):
    """A fast-path select over a tiny set straight after a select that ended on the whole vector, and after one that
    found no k-th: every exit leaves the histogram all-zero and the candidate counter ready for the next select."""
    tiny_ids, tiny_w = np.array([3, 4, 5, 6, N_STAR - 1]), np.array([1.0, 1.0, 2.0, 0.5, 1.0])
    for k_big in (SEL_CAP - 100, N_LEAVES + 1):
        big = Expect(orc, load_family(dev_star, "equal"))
        assert check_select(dev_star, big, k_big, "equal") in ("whole", "all-whole")
        ex = Expect(orc, load(dev_star, tiny_ids, tiny_w))
        for k in (2, 1, 5, 6):
            assert check_select(dev_star, ex, k, "tiny after whole") in ("fast", "all")


# ------------------------------------------------------------------ 5. the backward-search overflow
@pytest.fixture(scope="module")
def in_star_ref(orc, pkg_product):
    """the in-star, its twin, and the twin's answers (computed once)"""
    host = in_star(pkg_product, N_STAR)
    og = to_oracle(orc, host)
    thr = 1e-3  # below alpha (1 - alpha) = 0.1275, the entry of every leaf
    ref = {"push": og.backward_push(0, A, thr, orc.SYNC)}
    for k in (-1, 10):
        ref[k] = og.all_pair_backward(A, thr, k, 0, 1, schedule=orc.SYNC)
    return host, thr, ref


@pytest.fixture
def dev_in_star(pkg, in_star_ref, dev_cache):
    return shared_graph(dev_cache, pkg, "dev_in_star", lambda: pkg.Graph(in_star_ref[0]))


def test_backward_push_in_star(pkg, dev_in_star, in_star_ref):
    """pprhip_backward_push from the hub of an in-star of 2^18 + 9292 leaves against the twin, compared as
    test_backward_push_got compares."""
    _, thr, ref = in_star_ref
    p, r, st = dev_in_star.backward_push(0, A, thr)
    po, ro, sto = ref["push"]
    assert np.max(np.abs(p - po)) <= TOL_PUSH and np.max(np.abs(r - ro)) <= TOL_PUSH
    assert st.levels == sto.levels and st.pops + st.dense_nodes == sto.pops
    assert st.dense_levels > 0 or st.edge_pushes == sto.edge_pushes
    assert abs(p[0] - A) <= TOL_PUSH and np.all(np.abs(p[1:] - A * (1 - A)) <= TOL_PUSH) and not r.any()


@pytest.mark.parametrize("tier", [None, "1", "2", "3"])
@pytest.mark.parametrize("k", [-1, 10])
def test_all_pair_backward_overflow(pkg, dev_in_star, in_star_ref, k, tier, monkeypatch):
    """One target, the hub, whose search finds every node: 2^18 + 9293 sources, more than the candidate buffer holds.
    By the default routing and from each tier PPRHIP_APBS_TIER can start at; every tier takes a search of this size
    and returns rows (none answers with an error code).  Started at tier 3 the search runs on a batch workspace and
    ends in finish_search (bwd_runs.cpp), whose gather overflows (cnt > sel_cap) and whose entries then come from the whole vector."""
    if tier is not None:
        monkeypatch.setenv("PPRHIP_APBS_TIER", tier)
    _, thr, ref = in_star_ref
    ix, st = dev_in_star.all_pair_backward(A, thr, k, t_begin=0, t_end=1)
    off, tg, vl = ix.arrays()
    ix.close()
    ooff, otg, ovl = ref[k]
    assert np.array_equal(off, ooff) and np.array_equal(tg, otg)
    assert np.max(np.abs(vl - ovl)) <= TOL_PUSH
    assert off[-1] == N_STAR > SEL_CAP and np.all(np.diff(off) == 1) and not tg.any()  # one entry per row: the hub's
    assert abs(vl[0] - A) <= TOL_PUSH and np.all(np.abs(vl[1:] - A * (1 - A)) <= TOL_PUSH)
    if tier == "3":  # the whole-vector search on a batch workspace (the only path of this call that counts levels
        assert st.levels > 0 and st.xl_targets == 0  # without a dense-tier pass before it)
