"""Developer benchmark: the weighted walk index (pprhip_weighted_walk_index_build) on R-MAT <scale>, alpha 0.15, eps 0.5.

Measures pprhip_weighted_fora under two weight sets - uniform in (0.5, 1.5) and Pareto (shape 1.5) + 0.01 - from the
largest-out-degree source and from a random live source, three repetitions each after one warm-up (min / median / max):
the walk phase (mc_ms, device events) and the whole call (total_ms), in three settings:
  1. on the parent commit's build (--baseline DIR: the package directory of a built checkout of the parent commit),
  2. on this tree without an index,
  3. on this tree served from the index.
For the index it records the build (kernel and wall time, three builds), its terminals and bytes, and for the served
runs the walks served / walked live and the walk phase's nanoseconds per walk.

Every build is measured by the same script in the same visit, each in a child process under its own time limit; a
child that fails or times out ends the run.  The record names the builds "baseline" and "this tree" with their commits
(--baseline-rev; this tree's from git when it can be asked).  Two statements are evaluated and recorded, not asserted:
the served walk phase is shorter than the baseline's in every repetition (its maximum below the baseline's minimum), and
the unindexed walk phase of this tree lies within the baseline's spread (their [min, max] ranges meet).

Usage: python tools/bench_weighted_walk_index.py --scale 22 [--baseline DIR --baseline-rev REV] [--out FILE.json]
       [--limit SECONDS]"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN_PKG = os.path.join(ROOT, "personalized-pagerank-algorithms-on-neo4j_amd")
EPS, ALPHA, SEED, REPS = 0.5, 0.15, 3, 3


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


def measure(g, src):
    """REPS repetitions (after one warm-up) of weighted_fora from src on the handle as it stands."""
    g.weighted_fora(src, EPS, ALPHA, seed=SEED, fetch=False)
    sts = [g.weighted_fora(src, EPS, ALPHA, seed=SEED, fetch=False)[1] for _ in range(REPS)]
    walks = int(sts[0].walks)
    return {"mc_ms": stats3([st.mc_ms for st in sts]), "total_ms": stats3([st.total_ms for st in sts]),
            "push_ms": stats3([st.push_ms for st in sts]), "walks": walks, "live_steps": int(sts[0].walk_steps),
            "ns_per_walk": stats3([1e6 * st.mc_ms / walks for st in sts]) if walks else None}


def child(args):
    import numpy as np
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py runs
    import torch  # noqa: F401  (loads the HIP runtime first)
    pkg = load_package(args.package_dir, "pprhip_bench_pkg")
    host = pkg.HostCsr.rmat(args.scale, 16, seed=1)
    od = np.diff(host.out_rp.astype(np.int64))
    live = np.flatnonzero(od > 0)
    rng = np.random.default_rng(4)
    sources = [("largest_out_degree", int(np.argmax(od))), ("random", int(live[rng.integers(0, live.size)]))]
    weight_sets = [("uniform (0.5, 1.5)", rng.uniform(0.5, 1.5, host.m)),
                   ("Pareto shape 1.5 + 0.01", rng.pareto(1.5, host.m) + 0.01)]
    indexed = hasattr(pkg.Graph, "build_weighted_walk_index")
    res = {"build": args.label, "rev": args.rev, "scale": args.scale, "n": int(host.n), "m": int(host.m),
           "sources": dict(sources), "sets": []}
    with pkg.Graph(host) as g:
        for wname, w in weight_sets:
            g.set_weights(w)
            rec = {"weights": wname, "unindexed": {k: measure(g, s) for k, s in sources}}
            if indexed:
                builds = []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    st = g.build_weighted_walk_index(ALPHA, SEED)
                    builds.append({"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": st.mc_ms,
                                   "steps": int(st.walk_steps)})
                info = g.weighted_walk_index_info()
                rec["index"] = {"density": info["density"], "terminals": info["terminals"], "bytes": info["bytes"],
                                "build_kernel_ms": stats3([b["kernel_ms"] for b in builds]),
                                "build_wall_ms": stats3([b["wall_ms"] for b in builds]), "build_steps": builds[0]["steps"]}
                rec["served"] = {}
                for k, s in sources:
                    g.weighted_walk_index_usage(reset=True)
                    run = measure(g, s)
                    served, walked = g.weighted_walk_index_usage(reset=True)
                    run["served"], run["walked"] = served // (REPS + 1), walked // (REPS + 1)  # per call
                    rec["served"][k] = run
                g.drop_weighted_walk_index()
            res["sets"].append(rec)
    print("RESULT " + json.dumps(res), flush=True)


def verdict(base, own):
    """The two statements of the module docstring, per weight set and source."""
    out = []
    for sb, so in zip(base["sets"], own["sets"]):
        for k in so["unindexed"]:
            b, u, s = sb["unindexed"][k]["mc_ms"], so["unindexed"][k]["mc_ms"], so["served"][k]["mc_ms"]
            out.append({"weights": so["weights"], "source": k,
                        "served_shorter_in_every_repetition": s["max"] < b["min"],
                        "unindexed_within_baseline_spread": u["min"] <= b["max"] and b["min"] <= u["max"],
                        "baseline_mc_ms": b, "unindexed_mc_ms": u, "served_mc_ms": s,
                        "served_speedup_of_medians": b["median"] / s["median"] if s["median"] > 0 else None})
    return out


def fmt(s):
    return "%8.3f / %8.3f / %8.3f" % (s["min"], s["median"], s["max"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--baseline", default=None, help="package directory of a built checkout of the parent commit")
    ap.add_argument("--baseline-rev", default="", help="commit of the baseline build, for the record")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=420, help="time limit of one child, seconds")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--rev", default="")
    ap.add_argument("--package-dir", default=OWN_PKG)
    args = ap.parse_args()
    if args.child:
        return child(args)
    own_rev = args.rev
    if not own_rev:  # (the record names builds by label and commit, never by where they lay)
        p = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE,
                           stderr=subprocess.DEVNULL, text=True)
        own_rev = p.stdout.strip() if p.returncode == 0 and p.stdout.strip() else "unknown"
    builds = ([(args.baseline, "baseline", args.baseline_rev or "unknown")] if args.baseline else []) + \
             [(OWN_PKG, "this tree", own_rev)]
    results = []
    for pkg_dir, label, rev in builds:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--scale", str(args.scale), "--package-dir", pkg_dir,
               "--label", label, "--rev", rev]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)  # (a time-out raises: the run ends)
        if p.returncode != 0:
            sys.exit("child for the build '%s' ended with status %d: nothing more is started" % (label, p.returncode))
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
        results.append(json.loads(line[7:]))
    record = {"alpha": ALPHA, "eps": EPS, "seed": SEED, "repetitions": REPS, "builds": results}
    if len(results) == 2:
        record["statements"] = verdict(results[0], results[1])
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    for r in results:
        print("== %s (%s)  (R-MAT %d, n = %d, m = %d); ms as min / median / max of %d" % (
            r["build"], r["rev"], r["scale"], r["n"], r["m"], REPS))
        for rec in r["sets"]:
            print("-- weights: %s" % rec["weights"])
            if "index" in rec:
                ix = rec["index"]
                print("   index: density %.4f, %d terminals, %.3f GB, build kernel %s ms, wall %s ms, %d steps" % (
                    ix["density"], ix["terminals"], ix["bytes"] / 1e9, fmt(ix["build_kernel_ms"]), fmt(ix["build_wall_ms"]),
                    ix["build_steps"]))
            for setting in ("unindexed", "served"):
                for k, m in rec.get(setting, {}).items():
                    print("   %-9s %-18s walks %s ms   call %s ms   %.4g walks, %.3f ns per walk (median)%s" % (
                        setting, k, fmt(m["mc_ms"]), fmt(m["total_ms"]), m["walks"],
                        m["ns_per_walk"]["median"] if m["ns_per_walk"] else 0.0,
                        "   served %d, walked %d" % (m["served"], m["walked"]) if "served" in m else ""))
    for v in record.get("statements", []):
        print("%s, %s: served shorter than the baseline in every repetition: %s (x%.2f of medians); unindexed within the "
              "baseline's spread: %s" % (v["weights"], v["source"], v["served_shorter_in_every_repetition"],
                                         v["served_speedup_of_medians"] or 0.0, v["unindexed_within_baseline_spread"]))


if __name__ == "__main__":
    main()
