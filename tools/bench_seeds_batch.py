"""Developer benchmark: batched seed sets (pprhip_fora_batch_seeds, pprhip_fora_batch_topk_seeds) against seed sets one
at a time (pprhip_fora_seeds) and against batched single-source FORA (pprhip_fora_batch_single_source) on the same graph
and box.  R-MAT 22 by default, eps = 0.5, K seeds drawn uniformly, uniform weights, the batch tuning for the batched
calls (as bench.py runs them).  Prints queries/s per row.
Usage: python tools/bench_seeds_batch.py [scale] [queries per row]"""
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
q = int(sys.argv[2]) if len(sys.argv) > 2 else 64
EPS, ALPHA = 0.5, 0.15
host = pkg.HostCsr.rmat(scale, 16, seed=1)
rng = np.random.default_rng(2)
live = np.nonzero(np.diff(host.out_rp) > 0)[0]


def row(label, call, per_call):
    """call() runs per_call queries; one warm-up call, then calls until q queries have run"""
    call()
    calls = max(1, q // per_call)
    agg = {"dense_levels": 0, "sweeps": 0}
    t0 = time.perf_counter()
    for _ in range(calls):
        st = call()
        if st is not None:
            agg["dense_levels"] += st.dense_levels
            agg["sweeps"] += st.class_launches[5]
    dt = time.perf_counter() - t0
    extra = ""
    if agg["sweeps"]:
        extra = "  dense levels per sweep %.1f" % (agg["dense_levels"] / agg["sweeps"])
    print("%-36s %8.1f queries/s  (%d queries, %.1f ms/query)%s"
          % (label, calls * per_call / dt, calls * per_call, 1e3 * dt / (calls * per_call), extra), flush=True)


with pkg.Graph(host) as g:
    srcs = rng.choice(live, size=q).astype(np.int32)
    g.set_tuning(pkg.tuning_batch())
    row("batched single source", lambda: g.fora_batch_single_source(srcs, EPS, ALPHA, seed=3)[5], q)
    for k in (1, 32, 1024):
        # (K = 1: the batched single-source row's sources, as tools/bench_seeds.py takes them - a node drawn from all
        # n is often a dead end or isolated, a query without levels)
        sets = [srcs[i:i + 1] for i in range(q)] if k == 1 else \
            [rng.choice(host.n, size=k, replace=False).astype(np.int32) for _ in range(q)]
        g.set_tuning(pkg.tuning_default())

        def one_at_a_time(sets=sets):
            for s in sets:
                g.fora_seeds(s, EPS, ALPHA, seed=3, fetch=False)

        row("seed sets K = %d, one at a time" % k, one_at_a_time, q)
        g.set_tuning(pkg.tuning_batch())
        row("seed sets K = %d, batched" % k, lambda sets=sets: g.fora_batch_seeds(sets, EPS, ALPHA, seed=3)[5], q)
        if k == 32:
            row("seed sets K = 32, batched top-32",
                lambda sets=sets: g.fora_batch_topk_seeds(sets, 32, EPS, ALPHA, seed=3)[2], q)
