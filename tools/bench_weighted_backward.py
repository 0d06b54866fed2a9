"""Developer benchmark: the weighted backward calls (include/pprhip.h "weighted relationships", the backward direction)
beside their unweighted counterparts, measured in the same run on the same handle; R-MAT 22, alpha 0.15.  Two weight
sets: uniform in (0.5, 1.5) and a heavy-tailed one (Pareto, shape 1.5).  Per set: the backward push at rmax 1e-4 from a
random target and from the largest-in-degree target; the time per dense backward level (an all-dense push from the hub:
device-event time of the call / its levels) beside the weighted forward dense level and the unweighted ones; the
survival solve (host clock; every run at a fresh alpha, so that it iterates); weighted_ppr_targets on 256 random
targets, top-32 and kept, beside ppr_targets with one target per call; weighted_ppr_pairs on 256 random pairs at eps
0.5 beside ppr_pairs with one pair per call, with the push and walk shares.
Every figure: the median of `reps` runs after a warm-up, with min and max.  Nothing is asserted.
Usage: python tools/bench_weighted_backward.py [scale] [out.json]"""
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
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "weighted_backward_rmat%d.json" % scale)
ALPHA, RMAX, RMAX_DENSE, EPS, REPS, ITERS, Q, K = 0.15, 1e-4, 1e-6, 0.5, 5, 21, 256, 32
ALL_DENSE = 1e-12


def stat(values):
    v = [float(x) for x in values]
    return dict(median=float(np.median(v)), min=min(v), max=max(v), runs=len(v))


def timed(run, field=None, reps=REPS):
    """run() once to warm up, then reps times: the host clock in ms around it, or field(what it returns)"""
    run()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = run()
        out.append(field(r) if field else (time.perf_counter() - t0) * 1e3)
    return stat(out)


def timed3(run, reps=REPS):
    """run() returns (push_ms, walk_ms); one warm-up, then reps runs: stats of the host clock, the push and the walks"""
    run()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        p, w = run()
        out.append(((time.perf_counter() - t0) * 1e3, p, w))
    return [stat([o[i] for o in out]) for i in range(3)]


def fmt(s):
    return "%.3f (%.3f - %.3f)" % (s["median"], s["min"], s["max"])


_alpha_tick = [0]


def fresh_alpha():
    """alpha 0.15 up to 1e-9: the survival vectors are kept per alpha, a fresh one makes the solve run"""
    _alpha_tick[0] += 1
    return ALPHA + 1e-11 * _alpha_tick[0]


def tuned(g, dense_frac=None):
    t = pkg.tuning_default()
    if dense_frac is not None:
        t.dense_frac = dense_frac
    g.set_tuning(t)


def dense_level(run):
    """ms per level of an all-dense push: (total_ms / levels, levels)"""
    st = run()
    return timed(run, lambda r: r.total_ms / max(r.levels, 1)), int(st.levels), int(st.dense_levels)


host = pkg.HostCsr.rmat(scale, 16, seed=1)
n, m = host.n, host.m
rng = np.random.default_rng(4)
ind = np.diff(host.in_rp.astype(np.int64))
od = np.diff(host.out_rp.astype(np.int64))
with_in = np.flatnonzero(ind > 0)
t_random = int(with_in[rng.integers(0, with_in.size)])
t_hub = int(np.argmax(ind))
s_hub = int(np.argmax(od))
targets = with_in[rng.integers(0, with_in.size, Q)].astype(np.int32)
live = np.flatnonzero(od > 0)
sources = live[rng.integers(0, live.size, Q)].astype(np.int32)
weight_sets = [("uniform (0.5, 1.5)", rng.uniform(0.5, 1.5, m)), ("Pareto shape 1.5 + 0.01", rng.pareto(1.5, m) + 0.01)]
res = {"graph": "R-MAT %d" % scale, "n": int(n), "m": int(m), "alpha": ALPHA, "rmax": RMAX, "rmax_dense_level": RMAX_DENSE,
       "eps": EPS, "reps": REPS, "queries": Q, "k": K,
       "targets": {"random": t_random, "largest_in_degree": t_hub}, "sets": []}
named = (("random", t_random), ("largest_in_degree", t_hub))

with pkg.Graph(host) as g:
    print("R-MAT %d: n = %d, m = %d, alpha %.2f; medians of %d runs (min - max)" % (scale, n, m, ALPHA, REPS), flush=True)
    un = {}
    tuned(g)
    un["push_ms"] = {k: timed(lambda t=t: g.backward_push(t, ALPHA, RMAX), lambda r: r[2].total_ms) for k, t in named}
    tuned(g, ALL_DENSE)
    lv, levels, dl = dense_level(lambda: g.backward_push(t_hub, ALPHA, RMAX_DENSE)[2])
    un["backward_dense_level_ms"], un["backward_dense_levels"] = lv, [levels, dl]
    tuned(g)
    un["forward_dense_level_ms"] = timed(lambda: g.power_method(s_hub, ALPHA, ITERS), lambda r: r[1].total_ms / (ITERS - 1))
    un["survival_ms"] = timed(lambda: g.walk_survival(fresh_alpha()), reps=3)
    un["targets_one_per_call_ms"] = timed(lambda: [g.ppr_targets([int(t)], ALPHA, RMAX, k=K, fetch=False) for t in targets])
    conf = pkg.conf_whole_graph(n, m, ALPHA)

    def un_pairs():
        push = walk = 0.0
        for s, t in zip(sources, targets):
            st = g.ppr_pairs([int(s)], [int(t)], EPS, ALPHA, 9, conf=conf)[1]
            push += st.push_ms
            walk += st.mc_ms
        return push, walk

    un["pairs_one_per_call_ms"], un["pairs_push_ms"], un["pairs_walk_ms"] = timed3(un_pairs)
    res["unweighted"] = un
    print("unweighted: push %s / %s ms; dense level backward %s ms, forward %s ms; survival %s ms; %d targets one per call "
          "%s ms; %d pairs one per call %s ms (push %s, walks %s)" %
          (fmt(un["push_ms"]["random"]), fmt(un["push_ms"]["largest_in_degree"]), fmt(un["backward_dense_level_ms"]),
           fmt(un["forward_dense_level_ms"]), fmt(un["survival_ms"]), Q, fmt(un["targets_one_per_call_ms"]), Q,
           fmt(un["pairs_one_per_call_ms"]), fmt(un["pairs_push_ms"]), fmt(un["pairs_walk_ms"])), flush=True)
    keep = pkg.Results(g, Q)
    try:
        for name, w in weight_sets:
            rec = {"weights": name}
            g.set_weights(w)
            tuned(g)
            rec["push_ms"], rec["push_levels"] = {}, {}
            for k, t in named:
                rec["push_ms"][k] = timed(lambda t=t: g.weighted_backward_push(t, ALPHA, RMAX), lambda r: r[2].total_ms)
                st = g.weighted_backward_push(t, ALPHA, RMAX)[2]
                rec["push_levels"][k] = dict(levels=int(st.levels), dense_levels=int(st.dense_levels), pops=int(st.pops),
                                             dense_nodes=int(st.dense_nodes), edge_pushes=int(st.edge_pushes))
            tuned(g, ALL_DENSE)
            lv, levels, dl = dense_level(lambda: g.weighted_backward_push(t_hub, ALPHA, RMAX_DENSE)[2])
            rec["backward_dense_level_ms"], rec["backward_dense_levels"] = lv, [levels, dl]
            tuned(g)
            rec["forward_dense_level_ms"] = timed(lambda: g.weighted_power_method(s_hub, ALPHA, ITERS),
                                                  lambda r: r[1].total_ms / (ITERS - 1))
            rec["level_streamed_bytes"] = 12 * m  # 4-byte index + 8-byte weight per edge; the gathers come on top
            rec["survival_ms"] = timed(lambda: g.weighted_walk_survival(fresh_alpha()), reps=3)
            g.weighted_walk_survival(ALPHA)  # kept for what follows: the calls below do not solve again
            rec["targets_topk_ms"] = timed(lambda: g.weighted_ppr_targets(targets, ALPHA, RMAX, k=K, fetch=False))
            rec["targets_kept_ms"] = timed(lambda: g.weighted_ppr_targets(targets, ALPHA, RMAX, keep=keep, fetch=False))

            def w_pairs():
                st = g.weighted_ppr_pairs(sources, targets, EPS, ALPHA, 9, conf=conf)[1]
                return st.push_ms, st.mc_ms

            rec["pairs_ms"], rec["pairs_push_ms"], rec["pairs_walk_ms"] = timed3(w_pairs)
            st = g.weighted_ppr_pairs(sources, targets, EPS, ALPHA, 9, conf=conf)[1]
            rec["pairs_walks"], rec["pairs_walk_steps"], rec["pairs_rmax"] = int(st.walks), int(st.walk_steps), st.rmax_final
            res["sets"].append(rec)
            print("---- weights: %s" % name)
            for k, _ in named:
                print("backward push 1e-4, %-18s %s ms  (unweighted %s); %s" %
                      (k, fmt(rec["push_ms"][k]), fmt(un["push_ms"][k]), rec["push_levels"][k]))
            print("dense level: backward %s ms, forward %s ms  (unweighted backward %s, forward %s)" %
                  (fmt(rec["backward_dense_level_ms"]), fmt(rec["forward_dense_level_ms"]),
                   fmt(un["backward_dense_level_ms"]), fmt(un["forward_dense_level_ms"])))
            print("survival solve %s ms  (unweighted %s)" % (fmt(rec["survival_ms"]), fmt(un["survival_ms"])))
            print("%d targets: top-%d %s ms, kept %s ms  (unweighted, one target per call, top-%d: %s)" %
                  (Q, K, fmt(rec["targets_topk_ms"]), fmt(rec["targets_kept_ms"]), K, fmt(un["targets_one_per_call_ms"])))
            print("%d pairs eps %.1f: %s ms, push %s, walks %s, %d walks  (unweighted, one pair per call: %s, push %s, "
                  "walks %s)" % (Q, EPS, fmt(rec["pairs_ms"]), fmt(rec["pairs_push_ms"]), fmt(rec["pairs_walk_ms"]),
                                 rec["pairs_walks"], fmt(un["pairs_one_per_call_ms"]), fmt(un["pairs_push_ms"]),
                                 fmt(un["pairs_walk_ms"])))
            sys.stdout.flush()
    finally:
        keep.close()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("written: %s" % out_path)
