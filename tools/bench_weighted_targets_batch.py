"""Developer benchmark: weighted single targets (pprhip_weighted_ppr_targets) on R-MAT <scale>, alpha 0.15, rmax 1e-4,
this tree against a build of the parent commit (--baseline DIR: the package directory of a built checkout of it).

Both builds are loaded into one process, side by side, on one graph and the same inputs, and measured alternating:
repetition by repetition first the baseline, then this tree; one warm-up, then three repetitions, the host clock around
whole calls as min / median / max.  Two weight sets - uniform in (0.5, 1.5) and Pareto (shape 1.5) + 0.01 - and rows
  a  256 random targets in one call, top-32 and the vectors kept in a result store,
  b  the 64 targets of largest in-degree in one call,
  c  16 sets of 1 024 members in one call,
  d  the largest in-degree target together with 15 random ones in one call,
  e  the 256 targets one per call (the serial path on either build).
For this tree's batched calls it also records the sweeps per call and the busy columns per sweep (dense levels of all
queries / sweeps), and - from one more call of row b with the sweeps' kernel classes timed - the time of one batched
backward sweep beside one single-query dense backward level's.  (The driver's rounds are in no statistics field; the
host model tests/weighted_bwd_batch_ref.py counts them on small graphs.)
The outputs of the two builds must agree within 1e-12 (top-32 values of every query, the whole vectors of the first and
last query of a row); a row's gain is claimed only where the medians differ by at least five times the larger spread.

Usage: python tools/bench_weighted_targets_batch.py --scale 22 --baseline DIR [--baseline-rev REV] [--rev REV]
       [--out FILE.json]"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN_PKG = os.path.join(ROOT, "personalized-pagerank-algorithms-on-neo4j_amd")
ALPHA, RMAX, REPS, K = 0.15, 1e-4, 3, 32
TOL = 1e-12


def load_package(pkg_dir, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def stats3(xs):
    xs = sorted(float(x) for x in xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1]}


def run_row(np, pkg, g, row, keep):
    """One repetition of a row on one build: (ms, top-k values, the first and last vector, summed stats, per-query)."""
    kind, arg = row["kind"], row["arg"]
    t0 = time.perf_counter()
    if kind == "targets":
        _, sel, st, pq = g.weighted_ppr_targets(arg, ALPHA, RMAX, k=K, keep=keep, fetch=False)
        vals = sel[1]
    elif kind == "sets":
        _, sel, st, pq = g.weighted_ppr_target_sets(arg, ALPHA, RMAX, k=K, keep=keep, fetch=False)
        vals = sel[1]
    else:  # one call per target
        rows, st, pq = [], None, []
        for t in arg:
            _, sel, st, one = g.weighted_ppr_targets([int(t)], ALPHA, RMAX, k=K, keep=keep, fetch=False)
            rows.append(sel[1][0].copy())
            pq += one
        vals = np.array(rows)
    ms = (time.perf_counter() - t0) * 1e3
    q = 1 if kind == "single" else len(arg)
    ends = [keep.fetch(0), keep.fetch(q - 1)]
    return ms, vals, ends, st, pq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--baseline", required=True, help="package directory of a built checkout of the parent commit")
    ap.add_argument("--baseline-rev", default="unknown", help="commit of the baseline build, for the record")
    ap.add_argument("--rev", default="", help="what this tree is, for the record (default: git's HEAD)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py runs
    import torch  # noqa: F401  (loads the HIP runtime first)
    p = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE,
                       stderr=subprocess.DEVNULL, text=True)
    own_rev = args.rev or (p.stdout.strip() if p.returncode == 0 and p.stdout.strip() else "unknown")
    builds = [("baseline", args.baseline_rev, load_package(args.baseline, "pprhip_bench_base")),
              ("this tree", own_rev, load_package(OWN_PKG, "pprhip_bench_own"))]
    host = builds[1][2].HostCsr.rmat(args.scale, 16, seed=1)
    ind = np.diff(host.in_rp.astype(np.int64))
    rng = np.random.default_rng(4)
    rand256 = rng.choice(host.n, 256, replace=False).astype(np.int32)
    hubs = np.argsort(-ind)[:64].astype(np.int32)
    sets = [rng.choice(host.n, 1024, replace=False).astype(np.int32) for _ in range(16)]
    rows = [{"row": "a", "what": "256 random targets, one call", "kind": "targets", "arg": rand256},
            {"row": "b", "what": "the 64 targets of largest in-degree, one call", "kind": "targets", "arg": hubs},
            {"row": "c", "what": "16 sets of 1 024 members, one call", "kind": "sets", "arg": sets},
            {"row": "d", "what": "the largest in-degree target and 15 random ones, one call", "kind": "targets",
             "arg": np.concatenate([hubs[:1], rand256[:15]]).astype(np.int32)},
            {"row": "e", "what": "the 256 targets, one per call", "kind": "single", "arg": rand256}]
    weight_sets = [("uniform (0.5, 1.5)", rng.uniform(0.5, 1.5, host.m)),
                   ("Pareto shape 1.5 + 0.01", rng.pareto(1.5, host.m) + 0.01)]
    record = {"alpha": ALPHA, "rmax": RMAX, "top_k": K, "repetitions": REPS, "scale": args.scale, "n": int(host.n),
              "m": int(host.m), "builds": [{"build": b[0], "rev": b[1]} for b in builds], "weights": []}
    graphs = [b[2].Graph(host) for b in builds]
    keeps = [b[2].Results(g, 256) for b, g in zip(builds, graphs)]
    try:
        for wname, w in weight_sets:
            for g in graphs:
                g.set_weights(w)
                g.weighted_walk_survival(ALPHA)
            wrec = {"weights": wname, "rows": []}
            for row in rows:
                ms = [[], []]
                last = [None, None]
                for rep in range(REPS + 1):  # (the first one warms up)
                    for b in (0, 1):  # alternating: the baseline, then this tree
                        out = run_row(np, builds[b][2], graphs[b], row, keeps[b])
                        if rep:
                            ms[b].append(out[0])
                        last[b] = out
                diff = max(float(np.max(np.abs(last[0][1] - last[1][1]))),
                           max(float(np.max(np.abs(x - y))) for x, y in zip(last[0][2], last[1][2])))
                base, own = stats3(ms[0]), stats3(ms[1])
                spread = max(base["max"] - base["min"], own["max"] - own["min"])
                gap = base["median"] - own["median"]
                st, pq = last[1][3], last[1][4]
                dense = sum(int(s.dense_levels) for s in pq)
                sweeps = int(st.class_launches[5]) if row["kind"] != "single" else 0
                rec = {"row": row["row"], "what": row["what"], "baseline_ms": base, "this_tree_ms": own,
                       "baseline_over_this_tree_of_medians": base["median"] / own["median"],
                       "medians_differ_by_5_spreads": abs(gap) >= 5.0 * spread,
                       "ranges_meet": own["min"] <= base["max"] and base["min"] <= own["max"],
                       "max_abs_diff_of_outputs": diff, "outputs_agree": diff <= TOL,
                       "levels": sum(int(s.levels) for s in pq), "dense_levels": dense, "sweeps_per_call": sweeps,
                       "busy_columns_per_sweep": dense / sweeps if sweeps else None}
                wrec["rows"].append(rec)
                print("[%s] row %s: baseline %.2f / %.2f / %.2f ms, this tree %.2f / %.2f / %.2f ms, %d sweeps for %d dense "
                      "levels, max |diff| %.2e" % (wname, row["row"], base["min"], base["median"], base["max"], own["min"],
                                                   own["median"], own["max"], sweeps, dense, diff), flush=True)
            # one sweep beside one single-query dense level: row b once more with the sweeps' classes timed
            was = [b[2].set_kernel_timing(2) for b in builds]
            st_b = run_row(np, builds[1][2], graphs[1], rows[1], keeps[1])[3]
            one = run_row(np, builds[1][2], graphs[1], {"kind": "single", "arg": hubs[:4]}, keeps[1])[4]
            for b, x in zip(builds, was):
                b[2].set_kernel_timing(x)
            lv = sum(int(s.class_launches[1]) for s in one)
            wrec["batched_sweep_ms"] = st_b.class_ms[5] / st_b.class_launches[5] if st_b.class_launches[5] else None
            wrec["single_dense_level_ms"] = sum(s.class_ms[1] for s in one) / lv if lv else None
            print("[%s] one batched backward sweep %s ms, one single-query dense backward level %s ms" % (
                wname, wrec["batched_sweep_ms"], wrec["single_dense_level_ms"]), flush=True)
            record["weights"].append(wrec)
    finally:
        for k in keeps:
            k.close()
        for g in graphs:
            g.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    bad = [(w["weights"], r["row"]) for w in record["weights"] for r in w["rows"] if not r["outputs_agree"]]
    if bad:
        sys.exit("the two builds' outputs differ by more than 1e-12 in %s" % bad)


if __name__ == "__main__":
    main()
