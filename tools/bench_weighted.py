"""Developer benchmark: the weighted calls (include/pprhip.h "weighted relationships") beside their unweighted
counterparts on one handle, R-MAT 22, alpha 0.15.  Two weight sets: uniform in (0.5, 1.5) and a heavy-tailed one
(Pareto, shape 1.5).  Per set: pprhip_graph_set_weights (host clock, bytes in HBM); the weighted dense level from
weighted_power_method (device-event time of the call / its levels) beside the unweighted power_method level, with the
level's streamed bytes; a push at rmax 1e-4 from a random and from the largest-out-degree source; the walk rate of
weighted_random_walks against random_walks on the same starts (host clock around the calls, transfers included, and the
device-event walk phase of the FORA calls); weighted_fora at eps 0.5 against fora_single_source(n_rounds = 1).
Every figure: the median of `reps` runs after a warm-up, with min and max.  Nothing is asserted.
Usage: python tools/bench_weighted.py [scale] [out.json] [parent.json]
parent.json (optional): {"power_level_ms": {...}} measured with the same loop on the parent commit's library; copied
into the record beside this commit's unweighted level."""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "weighted_rmat%d.json" % scale)
parent_path = sys.argv[3] if len(sys.argv) > 3 else ""
ALPHA, RMAX, EPS, REPS, ITERS, WALKS = 0.15, 1e-4, 0.5, 5, 21, 1 << 22


def stat(values):
    v = [float(x) for x in values]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), runs=len(v))


def timed(run, field=None, reps=REPS):
    """run() once to warm up, then reps times: the host clock in ms around it, or Stats.<field> of what it returns"""
    run()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = run()
        out.append(field(r) if field else (time.perf_counter() - t0) * 1e3)
    return stat(out)


def fmt(s):
    return "%.3f (%.3f - %.3f)" % (s["median"], s["min"], s["max"])


host = pkg.HostCsr.rmat(scale, 16, seed=1)
n, m = host.n, host.m
rng = np.random.default_rng(4)
od = np.diff(host.out_rp.astype(np.int64))
live = np.flatnonzero(od > 0)
src_random = int(live[rng.integers(0, live.size)])
src_hub = int(np.argmax(od))
starts = live[rng.integers(0, live.size, WALKS)].astype(np.int32)
widx = rng.integers(0, 1 << 40, WALKS).astype(np.uint64)
weight_sets = [("uniform (0.5, 1.5)", rng.uniform(0.5, 1.5, m)), ("Pareto shape 1.5 + 0.01", rng.pareto(1.5, m) + 0.01)]
res = {"graph": "R-MAT %d" % scale, "n": int(n), "m": int(m), "alpha": ALPHA, "rmax": RMAX, "eps": EPS, "reps": REPS,
       "sources": {"random": src_random, "largest_out_degree": src_hub}, "sets": []}
rows = []

with pkg.Graph(host) as g:
    print("R-MAT %d: n = %d, m = %d, alpha %.2f; medians of %d runs (min - max)" % (scale, n, m, ALPHA, REPS), flush=True)
    levels = ITERS - 1
    un_level = timed(lambda: g.power_method(src_hub, ALPHA, ITERS), lambda r: r[1].total_ms / levels)
    res["unweighted"] = {"power_level_ms": un_level}
    if parent_path and os.path.exists(parent_path):
        res["unweighted"]["parent_commit"] = json.load(open(parent_path))
    un_push = {k: timed(lambda s=s: g.forward_push(s, ALPHA, RMAX, fetch=False), lambda r: r[3].total_ms)
               for k, s in (("random", src_random), ("largest_out_degree", src_hub))}
    un_walk = timed(lambda: g.random_walks(starts, widx, ALPHA, 9, 0, True))
    un_steps = int(g.random_walks(starts, widx, ALPHA, 9, 0, True)[1].sum())
    un_fora = {}
    for k, s in (("random", src_random), ("largest_out_degree", src_hub)):
        st = g.fora_single_source(s, EPS, ALPHA, seed=3, n_rounds=1, fetch=False)[1]
        un_fora[k] = dict(total_ms=timed(lambda s=s: g.fora_single_source(s, EPS, ALPHA, seed=3, n_rounds=1, fetch=False),
                                         lambda r: r[1].total_ms),
                          mc_ms=timed(lambda s=s: g.fora_single_source(s, EPS, ALPHA, seed=3, n_rounds=1, fetch=False),
                                      lambda r: r[1].mc_ms),
                          walks=int(st.walks), walk_steps=int(st.walk_steps), levels=int(st.levels))
    res["unweighted"].update(push_ms=un_push, walk_call_ms=un_walk, walk_call_steps=un_steps, fora=un_fora)
    print("unweighted power_method level  %s ms" % fmt(un_level), flush=True)
    for name, w in weight_sets:
        rec = {"weights": name}
        rec["set_weights_ms"] = timed(lambda: g.set_weights(w), reps=3)
        rec["bytes"] = int(g.weights_info()[1])
        rec["power_level_ms"] = timed(lambda: g.weighted_power_method(src_hub, ALPHA, ITERS),
                                      lambda r: r[1].total_ms / levels)
        rec["level_streamed_bytes"] = 12 * m  # 4-byte source + 8-byte weight per in-edge; the gathers come on top
        rec["level_stream_GB_per_s"] = 12 * m / (rec["power_level_ms"]["median"] * 1e-3) / 1e9
        rec["push_ms"], rec["push_levels"] = {}, {}
        for k, s in (("random", src_random), ("largest_out_degree", src_hub)):
            rec["push_ms"][k] = timed(lambda s=s: g.weighted_forward_push(s, ALPHA, RMAX, fetch=False),
                                      lambda r: r[3].total_ms)
            st = g.weighted_forward_push(s, ALPHA, RMAX, fetch=False)[3]
            rec["push_levels"][k] = dict(levels=int(st.levels), dense_levels=int(st.dense_levels), pops=int(st.pops),
                                         dense_nodes=int(st.dense_nodes), edge_pushes=int(st.edge_pushes))
        rec["walk_call_ms"] = timed(lambda: g.weighted_random_walks(starts, widx, ALPHA, 9, 0, True))
        rec["walk_call_steps"] = int(g.weighted_random_walks(starts, widx, ALPHA, 9, 0, True)[1].sum())
        rec["walk_call_steps_per_s"] = rec["walk_call_steps"] / (rec["walk_call_ms"]["median"] * 1e-3)
        rec["fora"] = {}
        for k, s in (("random", src_random), ("largest_out_degree", src_hub)):
            st = g.weighted_fora(s, EPS, ALPHA, seed=3, fetch=False)[1]
            f = dict(total_ms=timed(lambda s=s: g.weighted_fora(s, EPS, ALPHA, seed=3, fetch=False), lambda r: r[1].total_ms),
                     push_ms=timed(lambda s=s: g.weighted_fora(s, EPS, ALPHA, seed=3, fetch=False), lambda r: r[1].push_ms),
                     mc_ms=timed(lambda s=s: g.weighted_fora(s, EPS, ALPHA, seed=3, fetch=False), lambda r: r[1].mc_ms),
                     walks=int(st.walks), walk_steps=int(st.walk_steps), levels=int(st.levels),
                     dense_levels=int(st.dense_levels))
            f["walk_phase_steps_per_s"] = f["walk_steps"] / (f["mc_ms"]["median"] * 1e-3) if f["mc_ms"]["median"] else 0.0
            rec["fora"][k] = f
        res["sets"].append(rec)
        print("---- weights: %s" % name)
        print("set_weights                    %s ms, %.2f GB in HBM" % (fmt(rec["set_weights_ms"]), rec["bytes"] / 1e9))
        print("weighted dense level           %s ms  (%d B streamed: %.0f GB/s of index + weight stream)" %
              (fmt(rec["power_level_ms"]), rec["level_streamed_bytes"], rec["level_stream_GB_per_s"]))
        for k in ("random", "largest_out_degree"):
            print("push 1e-4, %-19s %s ms  (unweighted %s); %s" % (k, fmt(rec["push_ms"][k]), fmt(un_push[k]),
                                                                  rec["push_levels"][k]))
        print("walk call, %d walks       %s ms, %.2f G steps/s  (unweighted %s ms, %.2f G steps/s)" %
              (WALKS, fmt(rec["walk_call_ms"]), rec["walk_call_steps_per_s"] / 1e9, fmt(un_walk),
               un_steps / (un_walk["median"] * 1e-3) / 1e9))
        for k in ("random", "largest_out_degree"):
            f, u = rec["fora"][k], un_fora[k]
            print("FORA eps 0.5, %-16s %s ms, walks %s ms (%d walks, %.2f G steps/s)  (unweighted, 1 round: %s ms, walks "
                  "%s ms, %d walks)" % (k, fmt(f["total_ms"]), fmt(f["mc_ms"]), f["walks"], f["walk_phase_steps_per_s"] / 1e9,
                                         fmt(u["total_ms"]), fmt(u["mc_ms"]), u["walks"]))
        sys.stdout.flush()
    g.set_weights(None)
    # the unweighted level again behind everything else: what the handle gives after the weights have come and gone
    res["unweighted"]["power_level_ms_after"] = timed(lambda: g.power_method(src_hub, ALPHA, ITERS),
                                                      lambda r: r[1].total_ms / levels)
    print("unweighted power_method level after the drop  %s ms" % fmt(res["unweighted"]["power_level_ms_after"]))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("written: %s" % out_path)
