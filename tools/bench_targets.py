"""Developer benchmark: single-target PPR (pprhip_ppr_targets) on R-MAT 22, alpha 0.15 - targets per second with the
push milliseconds and, from one more run with kernel timing on, the time of the short kernels around the push (the start,
the division by S, the selection, the copies into the store), for (a) 256 random targets in one call, (b) the same 256
targets one per call, (c) the largest in-degree target, (d) one 1 024-member set; each with top-k 32 and with the vectors
kept in a result store.  The one-off survival solve is timed beside them.  Writes the figures as JSON.
Usage: python tools/bench_targets.py [scale] [rmax] [out.json]"""
import importlib
import json
import os
import sys
import time

import numpy as np
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py runs
import torch  # noqa: F401  (loads the HIP runtime first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("personalized-pagerank-algorithms-on-neo4j_amd")

scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
RMAX = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-4
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "targets_rmat%d.json" % scale)
ALPHA, K = 0.15, 32
SETUP = 6  # PPRHIP_KERNEL_QUERY_SETUP
host = pkg.HostCsr.rmat(scale, 16, seed=1)
rng = np.random.default_rng(4)
n = host.n
results = {"graph": "R-MAT %d" % scale, "n": int(n), "m": int(host.m), "alpha": ALPHA, "rmax": RMAX, "k": K, "cases": []}


def case(label, g, run, queries, calls, reps=25):
    """reps timed runs (after one warm-up) of `calls` calls that answer `queries` queries: the best run is reported, and
    the median of the runs beside it (a run takes milliseconds, so one run alone says little).  run(i, mode) makes call
    i and returns its summed Stats; mode: "topk" (k = 32, no vectors) or "keep" (result store)."""
    for mode in ("topk", "keep"):
        run(0, mode)
        best, times = None, []
        for _ in range(reps):
            acc = dict(push_ms=0.0, pops=0, edge_pushes=0, levels=0, dense_levels=0)
            t0 = time.perf_counter()
            for i in range(calls):
                st = run(i, mode)
                acc["push_ms"] += st.push_ms
                for f in ("pops", "edge_pushes", "levels", "dense_levels"):
                    acc[f] += int(getattr(st, f))
            dt = time.perf_counter() - t0
            times.append(dt)
            if best is None or dt < best[0]:
                best = (dt, acc)
        dt, acc = best
        # the kernels around the push (start, finish, selection, store): one more run with kernel timing on
        pkg.lib().pprhip_set_kernel_timing(1)
        acc["finish_select_ms"] = sum(run(i, mode).class_ms[SETUP] for i in range(calls))
        pkg.lib().pprhip_set_kernel_timing(0)
        rec = dict(case=label, mode=mode, queries=int(queries), calls=int(calls), runs=reps, ms=dt * 1e3,
                   median_ms=float(np.median(times)) * 1e3, queries_per_s=queries / dt, **acc)
        results["cases"].append(rec)
        print("%-40s %-4s queries %4d calls %4d  %9.1f /s  %9.2f ms (median of %d: %9.2f)  push %9.2f ms (summed over "
              "queries)  start+finish+select+store kernels %7.2f ms  levels %d (%d dense)"
              % (label, mode, queries, calls, rec["queries_per_s"], rec["ms"], reps, rec["median_ms"], acc["push_ms"],
                 acc["finish_select_ms"], acc["levels"], acc["dense_levels"]), flush=True)


with pkg.Graph(host) as g:
    print("R-MAT %d: n = %d, m = %d, alpha %.2f, rmax %.3g" % (scale, n, host.m, ALPHA, RMAX), flush=True)
    t0 = time.perf_counter()
    g.walk_survival(ALPHA)
    results["survival_solve_ms"] = (time.perf_counter() - t0) * 1e3
    print("survival solve (once per handle and alpha): %.1f ms" % results["survival_solve_ms"], flush=True)

    tg = rng.choice(n, 256, replace=False).astype(np.int32)
    hub = int(np.argmax(np.diff(host.in_rp.astype(np.int64))))
    members = rng.choice(n, 1024, replace=False).astype(np.int32)
    store = pkg.Results(g, 256)
    try:
        def many(i, mode):
            return g.ppr_targets(tg, ALPHA, RMAX, k=K if mode == "topk" else 0, keep=store if mode == "keep" else None,
                                 fetch=False)[2]

        def one_by_one(i, mode):
            return g.ppr_targets(tg[i:i + 1], ALPHA, RMAX, k=K if mode == "topk" else 0,
                                 keep=store if mode == "keep" else None, fetch=False)[2]

        def the_hub(i, mode):
            return g.ppr_targets([hub], ALPHA, RMAX, k=K if mode == "topk" else 0, keep=store if mode == "keep" else None,
                                 fetch=False)[2]

        def the_set(i, mode):
            return g.ppr_target_sets([members], ALPHA, RMAX, k=K if mode == "topk" else 0,
                                     keep=store if mode == "keep" else None, fetch=False)[2]

        case("(a) 256 random targets, one call", g, many, 256, 1)
        case("(b) 256 random targets, one per call", g, one_by_one, 256, 256, reps=5)
        case("(c) largest in-degree target", g, the_hub, 1, 1)
        case("(d) one set of 1024 members", g, the_set, 1, 1)
    finally:
        store.close()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(results, f, indent=1)
    f.write("\n")
print("written: %s" % out_path)
