"""Developer benchmark: single-pair PPR (pprhip_ppr_pairs) on R-MAT 22, alpha 0.15, eps 0.5 - pairs per second and the
push / walk milliseconds of (a) 256 random pairs with distinct targets, in one call and one pair per call, (b) one
target with 4 096 sources, (c) one source with 256 targets; the one-off survival solve; and beside them the FORA
single-source time per query a pair costs without this path.
Usage: python tools/bench_pairs.py [scale]"""
import importlib
import os
import sys
import time

import numpy as np
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py runs
import torch  # noqa: F401  (loads the HIP runtime first)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("personalized-pagerank-algorithms-on-neo4j_amd")

scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
EPS, ALPHA = 0.5, 0.15
host = pkg.HostCsr.rmat(scale, 16, seed=1)
rng = np.random.default_rng(4)
n = host.n


def case(label, g, sources, targets, calls=1, reps=3):
    """reps timed runs (after one warm-up) of the pairs split into `calls` equal calls; the best run is reported"""
    s_parts, t_parts = np.array_split(sources, calls), np.array_split(targets, calls)
    g.ppr_pairs(s_parts[0], t_parts[0], EPS, ALPHA, 1)
    best = None
    for r in range(reps):
        push = mc = walks = 0.0
        t0 = time.perf_counter()
        for sp, tp in zip(s_parts, t_parts):
            _, st = g.ppr_pairs(sp, tp, EPS, ALPHA, 2 + r)
            push += st.push_ms
            mc += st.mc_ms
            walks += st.walks
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, push, mc, walks)
    dt, push, mc, walks = best
    print("%-44s pairs %5d  calls %4d  %9.1f pairs/s  %8.2f ms  push %8.2f ms  walks %8.2f ms (summed over targets)"
          "  %.3g walks" % (label, sources.size, calls, sources.size / dt, dt * 1e3, push, mc, walks), flush=True)


with pkg.Graph(host) as g:
    conf = pkg.conf_whole_graph(n, host.m, ALPHA)
    rmax, w = pkg.pair_params(conf, EPS)
    print("R-MAT %d: n = %d, m = %d, alpha %.2f, eps %.2f: r_max %.3g, %d walks per pair" % (scale, n, host.m, ALPHA, EPS,
                                                                                           rmax, w), flush=True)
    t0 = time.perf_counter()
    g.walk_survival(ALPHA)
    print("survival solve (once per handle and alpha): %.1f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)
    t0 = time.perf_counter()
    g.walk_survival(ALPHA)
    print("survival, kept (a second call: fetch only): %.1f ms" % ((time.perf_counter() - t0) * 1e3), flush=True)

    live = np.flatnonzero(np.diff(host.out_rp) > 0)
    g.fora_single_source(int(live[0]), EPS, ALPHA, seed=1, fetch=False)
    tf = []
    for s in rng.choice(live, 8, replace=False):
        t0 = time.perf_counter()
        g.fora_single_source(int(s), EPS, ALPHA, seed=1, fetch=False)
        tf.append(time.perf_counter() - t0)
    print("FORA single-source per query (the cost of one pair without this path): %.2f ms (median of 8)"
          % (np.median(tf) * 1e3), flush=True)

    tg = rng.choice(n, 256, replace=False)
    sg = rng.integers(0, n, 256)
    case("(a) 256 random pairs, distinct targets", g, sg, tg)
    case("(a) 256 random pairs, one pair per call", g, sg, tg, calls=256, reps=1)
    t_hub = int(np.argmax(np.diff(host.in_rp.astype(np.int64))))
    t_rand = int(rng.integers(0, n))
    case("(b) one target (largest in-degree), 4096 src", g, rng.integers(0, n, 4096), np.full(4096, t_hub))
    case("(b) one random target, 4096 sources", g, rng.integers(0, n, 4096), np.full(4096, t_rand))
    s0 = int(rng.choice(live))
    case("(c) one source, 256 random targets", g, np.full(256, s0), rng.choice(n, 256, replace=False))
