"""Developer benchmark: FORA from a seed set (pprhip_fora_seeds), one query at a time, against single-source FORA
(pprhip_fora_single_source) on the same graph and box.  R-MAT 22 by default; K seeds drawn uniformly, uniform weights.
Usage: python tools/bench_seeds.py [scale] [queries per K]"""
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
q = int(sys.argv[2]) if len(sys.argv) > 2 else 8
EPS, ALPHA = 0.5, 0.15
host = pkg.HostCsr.rmat(scale, 16, seed=1)
rng = np.random.default_rng(2)
live = np.nonzero(np.diff(host.out_rp) > 0)[0]


def run(label, call):
    call(0)  # warm-up
    agg = {"rounds": 0, "levels": 0, "dense_levels": 0, "walks": 0}
    t0 = time.perf_counter()
    for i in range(q):
        _, st = call(i + 1)
        for k in agg:
            agg[k] += getattr(st, k)
    ms = 1e3 * (time.perf_counter() - t0) / q
    print("%-28s %8.2f ms/query  rounds %.1f  levels %.1f  dense levels %.1f  walks %.0f"
          % (label, ms, agg["rounds"] / q, agg["levels"] / q, agg["dense_levels"] / q, agg["walks"] / q), flush=True)


with pkg.Graph(host) as g:
    srcs = rng.choice(live, size=q + 1).astype(np.int32)
    run("single source", lambda i: g.fora_single_source(int(srcs[i]), EPS, ALPHA, seed=3, fetch=False))
    run("seed set K = 1", lambda i: g.fora_seeds([int(srcs[i])], EPS, ALPHA, seed=3, fetch=False))
    for k in (32, 1024, 65536):
        sets = [rng.choice(host.n, size=k, replace=False).astype(np.int32) for _ in range(q + 1)]
        run("seed set K = %d" % k, lambda i, sets=sets: g.fora_seeds(sets[i], EPS, ALPHA, seed=3, fetch=False))
