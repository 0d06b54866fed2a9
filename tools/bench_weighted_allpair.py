"""Developer benchmark: pprhip_weighted_all_pair_backward beside pprhip_all_pair_backward on one handle, and beside what
a user had before it - a loop of weighted_backward_push over the targets with the entries filtered on the host.
R-MAT 22, alpha 0.15, threshold 1e-3 (tools/bench_allpair.py's), k = 32, the first 2^18 targets and all targets, the two
weight sets of tools/bench_weighted.py (uniform in (0.5, 1.5); Pareto, shape 1.5).  Per set and range: the weighted call
as min / median / max of `REPS` runs after a warm-up (host clock around the call, index finalisation included), the
unweighted call likewise in the same run, the build of the weighted record array (ONE sample per weight set: the first
call over [0, 1) on fresh weights - allocation and build included - minus the same call again; bytes from weights_info), and the loop over LOOP_TARGETS targets sampled from the range, scaled to
the range.  No figure is asserted; the first CHECK_TARGETS sampled targets of every loop are compared, entry for entry,
with the call over [t, t + 1).
Usage: python tools/bench_weighted_allpair.py [scale] [out.json]"""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "weighted_allpair_rmat%d.json" % scale)
ALPHA, THRESHOLD, K, REPS, LOOP_TARGETS, WALKS, CHECK_TARGETS = 0.15, 1e-3, 32, 5, 256, 1 << 22, 16


def stat(values):
    v = [float(x) for x in values]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), runs=len(v))


def fmt(s):
    return "%.1f (%.1f - %.1f)" % (s["median"], s["min"], s["max"])


def timed_call(call, lo, hi, reps=REPS):
    """call(lo, hi) -> (Index, Stats): once to warm up, then reps times on the host clock (ms); the last run's figures"""
    ix, _ = call(lo, hi)
    ix.close()
    ms, info = [], {}
    for _ in range(reps):
        t0 = time.perf_counter()
        ix, st = call(lo, hi)
        ms.append((time.perf_counter() - t0) * 1e3)
        info = dict(entries=int(ix.arrays()[1].size), dense_tier_targets=int(st.rounds), xl_targets=int(st.xl_targets),
                    whole_vector_targets=int(st.dense_nodes), pops=int(st.pops), edge_pushes=int(st.edge_pushes),
                    push_ms=float(st.push_ms))
        ix.close()
    return dict(ms=stat(ms), **info)


host = pkg.HostCsr.rmat(scale, 16, seed=1)
n, m = host.n, host.m
# tools/bench_weighted.py's weight sets: the same generator and the same draws before them
rng = np.random.default_rng(4)
live = np.flatnonzero(np.diff(host.out_rp.astype(np.int64)) > 0)
rng.integers(0, live.size)
rng.integers(0, live.size, WALKS)
rng.integers(0, 1 << 40, WALKS)
weight_sets = [("uniform (0.5, 1.5)", rng.uniform(0.5, 1.5, m)), ("Pareto shape 1.5 + 0.01", rng.pareto(1.5, m) + 0.01)]
ranges = [("first 2^18 targets", 0, min(n, 1 << 18)), ("all targets", 0, n)]
res = {"graph": "R-MAT %d" % scale, "n": int(n), "m": int(m), "alpha": ALPHA, "threshold": THRESHOLD, "k": K, "reps": REPS,
       "loop_targets": LOOP_TARGETS, "unweighted": {}, "sets": []}

with pkg.Graph(host) as g:
    print("R-MAT %d: n = %d, m = %d, alpha %.2f, threshold %g, k %d; ms as median (min - max) of %d runs" %
          (scale, n, m, ALPHA, THRESHOLD, K, REPS), flush=True)
    unweighted = lambda lo, hi: g.all_pair_backward(ALPHA, THRESHOLD, K, lo, hi)  # noqa: E731
    weighted = lambda lo, hi: g.weighted_all_pair_backward(ALPHA, THRESHOLD, K, lo, hi)  # noqa: E731
    for label, lo, hi in ranges:
        res["unweighted"][label] = timed_call(unweighted, lo, hi)
        print("unweighted, %-20s %s ms" % (label, fmt(res["unweighted"][label]["ms"])), flush=True)
    for name, w in weight_sets:
        rec = {"weights": name, "ranges": {}}
        g.set_weights(w)
        bytes0 = g.weights_info()[1]
        tiny = []
        for _ in range(2):  # the first call builds the records; the workspaces are there already
            t0 = time.perf_counter()
            ix, _ = weighted(0, 1)
            tiny.append((time.perf_counter() - t0) * 1e3)
            ix.close()
        rec["record_build_ms"] = tiny[0] - tiny[1]
        rec["record_bytes"] = int(g.weights_info()[1] - bytes0)
        print("---- weights: %s; record array %.2f GB, built in %.1f ms" % (name, rec["record_bytes"] / 1e9,
                                                                             rec["record_build_ms"]), flush=True)
        for label, lo, hi in ranges:
            r = {"weighted": timed_call(weighted, lo, hi), "unweighted_same_run": timed_call(unweighted, lo, hi)}
            # what a user had before: one weighted_backward_push per target, n doubles back, filtered on the host
            pick = np.sort(np.random.default_rng(7).choice(np.arange(lo, hi), LOOP_TARGETS, replace=False))
            g.weighted_backward_push(int(pick[0]), ALPHA, THRESHOLD)
            t0 = time.perf_counter()
            kept = 0
            for t in pick:
                p, _, _ = g.weighted_backward_push(int(t), ALPHA, THRESHOLD)
                kept += int(np.flatnonzero((p > 0) & (p >= THRESHOLD)).size)
            loop_ms = (time.perf_counter() - t0) * 1e3
            # self-check at this scale: the call over [t, t + 1) holds the entries the push keeps (any mismatch raises)
            for t in pick[:CHECK_TARGETS]:
                p, _, _ = g.weighted_backward_push(int(t), ALPHA, THRESHOLD)
                ix, _ = g.weighted_all_pair_backward(ALPHA, THRESHOLD, -1, int(t), int(t) + 1)
                off, tg, vl = ix.arrays()
                ix.close()
                want = np.flatnonzero((p > 0) & (p >= THRESHOLD))
                got_src = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
                if not (np.array_equal(got_src, want) and np.all(tg == t) and np.max(np.abs(vl - p[want]), initial=0.0) <= 1e-12):
                    raise RuntimeError("weighted All-Pair disagrees with weighted_backward_push at target %d" % t)
            r["self_check_targets"] = CHECK_TARGETS
            r["push_loop"] = dict(sampled_targets=LOOP_TARGETS, sampled_ms=loop_ms, entries_kept=kept,
                                  scaled_to_range_ms=loop_ms * (hi - lo) / LOOP_TARGETS)
            r["weighted_over_unweighted"] = r["weighted"]["ms"]["median"] / r["unweighted_same_run"]["ms"]["median"]
            r["loop_over_weighted"] = r["push_loop"]["scaled_to_range_ms"] / r["weighted"]["ms"]["median"]
            rec["ranges"][label] = r
            print("%-20s weighted %s ms, unweighted %s ms (x %.2f); push loop %.0f ms for %d targets = %.0f ms scaled "
                  "(x %.0f)" % (label, fmt(r["weighted"]["ms"]), fmt(r["unweighted_same_run"]["ms"]),
                                r["weighted_over_unweighted"], loop_ms, LOOP_TARGETS, r["push_loop"]["scaled_to_range_ms"],
                                r["loop_over_weighted"]), flush=True)
        res["sets"].append(rec)
    g.set_weights(None)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("written: %s" % out_path)
