"""Developer benchmark: the weighted top-k calls (include/pprhip.h "weighted seed sets and top-k") beside the routes a
caller had before them, on one handle, R-MAT 22, alpha 0.15, eps 0.5, k = 32.  Two weight sets: uniform in (0.5, 1.5)
and a heavy-tailed one (Pareto, shape 1.5).  Per set, in the same run: weighted_fora_topk from the largest-out-degree
source and from a random source, weighted_fora_topk_seeds from a 16-seed set, and weighted_fora + topk_select from the
same two sources; unweighted fora_topk from the same sources and set once, before the weights arrive.  Recorded per
query: the host clock around the call, the device-event total and its push / walk / select split, rounds, levels,
walks and walk steps.  Every time: the median of `reps` runs after a warm-up, with min and max.  Nothing is asserted.
Usage: python tools/bench_weighted_topk.py [scale] [out.json]"""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "weighted_topk_rmat%d.json" % scale)
ALPHA, EPS, K, REPS, SEED = 0.15, 0.5, 32, 5, 3


def stat(values):
    v = [float(x) for x in values]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), runs=len(v))


def fmt(s):
    return "%.3f (%.3f - %.3f)" % (s["median"], s["min"], s["max"])


def measure(run, stats_of, extra=None):
    """run() once to warm up, then REPS times: host clock, device total and the phase split; counters of the last run.
    extra: a second call that belongs to the query (the selection behind a whole-graph FORA), inside the host clock."""
    def both():
        r = run()
        return r, (extra() if extra else None)
    both()
    host_ms, tot, push, mc, sel = [], [], [], [], []
    st = None
    for _ in range(REPS):
        t0 = time.perf_counter()
        r, e = both()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        st = stats_of(r)
        est = e[4] if e else None  # topk_select's Stats
        tot.append(st.total_ms + (est.total_ms if est else 0.0))
        push.append(st.push_ms)
        mc.append(st.mc_ms)
        sel.append(st.select_ms + (est.total_ms if est else 0.0))
    return dict(host_ms=stat(host_ms), total_ms=stat(tot), push_ms=stat(push), mc_ms=stat(mc), select_ms=stat(sel),
                rounds=int(st.rounds), levels=int(st.levels), dense_levels=int(st.dense_levels), walks=int(st.walks),
                walk_steps=int(st.walk_steps), mc_sources=int(st.mc_sources))


def line(tag, r):
    print("%-44s host %s ms; device %s = push %.3f + walks %.3f + select %.3f; rounds %d, levels %d, walks %d" %
          (tag, fmt(r["host_ms"]), fmt(r["total_ms"]), r["push_ms"]["median"], r["mc_ms"]["median"],
           r["select_ms"]["median"], r["rounds"], r["levels"], r["walks"]), flush=True)


host = pkg.HostCsr.rmat(scale, 16, seed=1)
n, m = host.n, host.m
rng = np.random.default_rng(4)
od = np.diff(host.out_rp.astype(np.int64))
live = np.flatnonzero(od > 0)
src_random = int(live[rng.integers(0, live.size)])
src_hub = int(np.argmax(od))
seed_set = live[rng.choice(live.size, 16, replace=False)].astype(np.int32)
sources = (("largest_out_degree", src_hub), ("random", src_random))
weight_sets = [("uniform (0.5, 1.5)", rng.uniform(0.5, 1.5, m)), ("Pareto shape 1.5 + 0.01", rng.pareto(1.5, m) + 0.01)]
res = {"graph": "R-MAT %d" % scale, "n": int(n), "m": int(m), "alpha": ALPHA, "eps": EPS, "k": K, "reps": REPS,
       "sources": {"random": src_random, "largest_out_degree": src_hub, "seed_set": [int(x) for x in seed_set]},
       "sets": []}

with pkg.Graph(host) as g:
    print("R-MAT %d: n = %d, m = %d, alpha %.2f, eps %.1f, top-%d; medians of %d runs (min - max)" %
          (scale, n, m, ALPHA, EPS, K, REPS), flush=True)
    un = {}
    for key, s in sources:
        un[key] = measure(lambda s=s: g.fora_topk(s, EPS, ALPHA, K, SEED), lambda r: r[4])
        line("unweighted fora_topk, %s" % key, un[key])
    un["seed_set"] = measure(lambda: g.fora_topk_seeds(seed_set, EPS, ALPHA, K, SEED), lambda r: r[4])
    line("unweighted fora_topk_seeds, 16 seeds", un["seed_set"])
    un["note"] = ("fora_topk runs its next push beside the walks and reports the phases by kernel-class times, which "
                  "are zero without kernel timing: only host_ms and total_ms are meaningful here")
    res["unweighted"] = un
    for name, w in weight_sets:
        g.set_weights(w)
        rec = {"weights": name, "topk": {}, "fora_select": {}}
        print("---- weights: %s" % name, flush=True)
        for key, s in sources:
            rec["topk"][key] = measure(lambda s=s: g.weighted_fora_topk(s, EPS, ALPHA, K, SEED), lambda r: r[4])
            line("weighted_fora_topk, %s" % key, rec["topk"][key])
        rec["topk"]["seed_set"] = measure(lambda: g.weighted_fora_topk_seeds(seed_set, EPS, ALPHA, K, SEED), lambda r: r[4])
        line("weighted_fora_topk_seeds, 16 seeds", rec["topk"]["seed_set"])
        for key, s in sources:
            rec["fora_select"][key] = measure(lambda s=s: g.weighted_fora(s, EPS, ALPHA, SEED, fetch=False), lambda r: r[1],
                                              extra=lambda: g.topk_select(K))
            line("weighted_fora + topk_select, %s" % key, rec["fora_select"][key])
            a, b = rec["topk"][key], rec["fora_select"][key]
            rec.setdefault("topk_over_fora_select", {})[key] = dict(
                host=a["host_ms"]["median"] / b["host_ms"]["median"], walks=a["walks"] / max(b["walks"], 1))
        res["sets"].append(rec)
    g.set_weights(None)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("written: %s" % out_path)
