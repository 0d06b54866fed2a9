"""Developer benchmark: batched weighted FORA top-k (pprhip_weighted_fora_batch_topk) on R-MAT <scale>, alpha 0.15,
eps 0.5, k = 32; two weight sets - uniform in (0.5, 1.5) and Pareto (shape 1.5) + 0.01; 64 random sources with
out-edges; three repetitions after one warm-up, the host's clock around whole calls, min / median / max.  One process,
one handle.  Rows per weight set:
  a. weighted_fora_batch_topk of the 64, one call;
  b. the same 64 as a loop of weighted_fora_topk with seed + i (the comparison: the same build, since the commit before
     has no batched call);
  c. the unweighted fora_batch_topk of the same sources, for scale;
  d. 16 queries - the largest-out-degree source and 15 random ones - batched and as the loop;
  e. of call a: sweeps and busy columns per sweep, merged walk launches and columns per launch, and - from one more
     call and one more loop with every kernel class timed - the merged launches' time beside the sum of the same
     phases' single launches.
The ids of row a are compared with row b's, position by position, wherever row b's neighbouring values are more than
1e-9 (relative) apart.  The project's rule for a claim: a gain is claimed only from five times the larger spread
(max - min of the two rows compared); "slower" is recorded wherever the batched median is above the loop's.

Usage: python tools/bench_weighted_topk_batch.py --scale 22 [--out profiles/weighted_topk_batch_rmat22.json]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, ALPHA, SEED, REPS, Q, K = 0.5, 0.15, 3, 3, 64, 32


def stats3(xs):
    xs = sorted(float(x) for x in xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1]}


def timed(fn):
    """REPS repetitions after one warm-up: ({min, median, max} ms, the last repetition's result)."""
    fn()
    ms, out = [], None
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats3(ms), out


def compare(a, b):
    """the project's rule on two rows of wall times (a: batched, b: loop)"""
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    gain = b["median"] - a["median"]
    return {"loop_over_batch_of_medians": b["median"] / a["median"], "gain_ms": gain, "larger_spread_ms": spread,
            "gain_claimed": bool(gain >= 5.0 * spread), "batch_slower": bool(a["median"] > b["median"])}


def ids_agree(np, ids, vals_loop, ids_loop, est_rest):
    """rows of a against rows of b under the near-tie rule; returns (positions compared, positions that differ)"""
    compared = differ = 0
    for i in range(ids.shape[0]):
        v = vals_loop[i]
        cnt = int(np.count_nonzero(ids_loop[i] >= 0))
        near = np.zeros(cnt, dtype=bool)
        if cnt > 1:
            gap = np.abs(np.diff(v[:cnt])) <= 1e-9 * v[:cnt - 1]
            near[:-1] |= gap
            near[1:] |= gap
        if cnt == K and est_rest[i] is not None:
            near[-1] |= abs(v[cnt - 1] - est_rest[i]) <= 1e-9 * v[cnt - 1]
        compared += int((~near).sum())
        differ += int(np.count_nonzero(ids[i][:cnt][~near] != ids_loop[i][:cnt][~near]))
    return compared, differ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py runs
    import torch  # noqa: F401  (loads the HIP runtime first)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module("personalized-pagerank-algorithms-on-neo4j_amd")
    host = pkg.HostCsr.rmat(args.scale, 16, seed=1)
    od = np.diff(host.out_rp.astype(np.int64))
    live = np.flatnonzero(od > 0)
    rng = np.random.default_rng(4)
    srcs = live[rng.choice(live.size, Q, replace=False)].astype(np.int32)
    hub16 = np.concatenate(([int(np.argmax(od))], srcs[:15])).astype(np.int32)
    weight_sets = [("uniform (0.5, 1.5)", rng.uniform(0.5, 1.5, host.m)),
                   ("Pareto shape 1.5 + 0.01", rng.pareto(1.5, host.m) + 0.01)]
    record = {"scale": args.scale, "n": int(host.n), "m": int(host.m), "alpha": ALPHA, "eps": EPS, "k": K, "seed": SEED,
              "repetitions": REPS, "queries": Q, "sets": []}
    with pkg.Graph(host) as g:
        for wname, w in weight_sets:
            g.set_weights(w)

            def batch(s):
                return g.weighted_fora_batch_topk(s, K, EPS, ALPHA, SEED, per_query=True)

            def loop(s, fetch=False):
                return [g.weighted_fora_topk(int(x), EPS, ALPHA, K, SEED + i, fetch=fetch) for i, x in enumerate(s)]

            a_ms, (ids, vals, n_out, st, pq) = timed(lambda: batch(srcs))
            b_ms, singles = timed(lambda: loop(srcs))
            c_ms, _ = timed(lambda: g.fora_batch_topk(srcs, K, EPS, ALPHA, SEED))
            d_ms, (_, _, _, dst, dpq) = timed(lambda: batch(hub16))
            dl_ms, _ = timed(lambda: loop(hub16))
            # the ids of a against b (one more loop that fetches the estimates, for the value just below the row)
            full = loop(srcs, fetch=True)
            rest = []
            for r in full:
                e = np.sort(r[3])[::-1]
                rest.append(float(e[K]) if e.size > K else None)
            ids_b = np.full((Q, K), -1, dtype=np.int32)
            vals_b = np.zeros((Q, K))
            for i, r in enumerate(full):
                c = min(int(r[0]), K)
                ids_b[i, :c], vals_b[i, :c] = r[1][:c], r[2][:c]
            compared, differ = ids_agree(np, ids, vals_b, ids_b, rest)
            worst_val = float(np.max(np.abs(vals - vals_b)))
            decisions_equal = all((p.rounds, p.levels, p.walks, p.walk_steps) == (r[4].rounds, r[4].levels, r[4].walks, r[4].walk_steps)
                                  for p, r in zip(pq, full))
            # e: the kernel classes timed, batched and in the loop
            was = pkg.set_kernel_timing(1)
            _, _, _, tst, _ = batch(srcs)
            tl = loop(srcs)
            pkg.set_kernel_timing(was)
            sweeps, launches = int(st.class_launches[5]), int(st.class_launches[3])
            rounds = sum(int(p.rounds) for p in pq)
            dense = sum(int(p.dense_levels) for p in pq)
            rec = {"weights": wname,
                   "a_batch_64_ms": a_ms, "b_loop_64_ms": b_ms, "c_unweighted_batch_topk_64_ms": c_ms,
                   "d_batch_hub_and_15_ms": d_ms, "d_loop_hub_and_15_ms": dl_ms,
                   "a_queries_per_s": 1e3 * Q / a_ms["median"], "b_queries_per_s": 1e3 * Q / b_ms["median"],
                   "c_queries_per_s": 1e3 * Q / c_ms["median"],
                   "a_against_b": compare(a_ms, b_ms), "d_against_its_loop": compare(d_ms, dl_ms),
                   "e": {"sweeps_per_call": sweeps, "busy_columns_per_sweep": dense / sweeps if sweeps else None,
                         "merged_walk_launches": launches, "columns_per_walk_launch": rounds / launches if launches else None,
                         "rounds_per_query": rounds / Q, "walks_per_query": sum(int(p.walks) for p in pq) / Q,
                         "d_sweeps": int(dst.class_launches[5]),
                         "d_busy_columns_per_sweep": (sum(int(p.dense_levels) for p in dpq) / int(dst.class_launches[5])
                                                      if dst.class_launches[5] else None),
                         "d_merged_walk_launches": int(dst.class_launches[3]),
                         "merged_walk_ms_per_call": float(tst.class_ms[3]),
                         "single_walk_ms_sum_of_the_loop": float(sum(r[4].class_ms[3] for r in tl)),
                         "sweeps_ms_per_call": float(tst.class_ms[5]),
                         "single_dense_levels_ms_sum_of_the_loop": float(sum(r[4].class_ms[1] for r in tl)),
                         "loop_mc_ms_sum": float(sum(r[4].mc_ms for r in singles)),
                         "loop_push_ms_sum": float(sum(r[4].push_ms for r in singles))},
                   "ids_a_against_b": {"positions_compared": compared, "positions_that_differ": differ,
                                       "worst_value_difference": worst_val, "decisions_equal": bool(decisions_equal)}}
            record["sets"].append(rec)
            print("[%s] a %.1f ms  b %.1f ms  c %.1f ms  d %.1f / loop %.1f ms (medians); ids differ at %d of %d" % (
                wname, a_ms["median"], b_ms["median"], c_ms["median"], d_ms["median"], dl_ms["median"], differ, compared),
                flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    print("RESULT " + json.dumps(record), flush=True)
    return 0 if all(s["ids_a_against_b"]["positions_that_differ"] == 0 for s in record["sets"]) else 1


if __name__ == "__main__":
    sys.exit(main())
