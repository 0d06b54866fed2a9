"""Developer benchmark: the FORA+ walk index (pprhip_walk_index_build) on R-MAT <scale>, alpha 0.15, eps 0.5.

Measures whole-graph FORA one query at a time (pprhip_fora_single_source) and 16 in flight (the batched call under the
batch profile), without an index and served from one, three repetitions each (min / median / max): queries per second,
the walk phase per query (mc_ms; batched: the walk class time of the call / q), dense levels per query, and for a served
run the nanoseconds per served walk.  The index's build time, terminals and bytes are reported beside the derived bound
m * density + n.

The unindexed baseline is another BUILD, not this build's own fallback path: --baseline DIR names the package directory
of a checkout of the parent commit (built there with make); it is measured by the same script in the same visit, and
its index part is skipped because it has no such entry points.  Every measurement runs in a child process under its own
time limit; a child that fails or times out ends the run.

--c-walk-single X --c-walk-batch Y add a served run under the two profiles with c_walk_ns set to X / Y: the indexed
tuning, c_walk_ns = the measured nanoseconds per served walk of an earlier run.  The record names the two builds
"baseline" and "this tree" with their commits (--baseline-rev; this tree's from git when it can be asked).

Usage: python tools/bench_walk_index.py --scale 22 [--baseline DIR --baseline-rev REV] [--c-walk-single X --c-walk-batch Y]
       [--out FILE.json] [--limit SECONDS]"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN_PKG = os.path.join(ROOT, "personalized-pagerank-algorithms-on-neo4j_amd")
EPS, ALPHA, SEED, REPS = 0.5, 0.15, 5, 3
N_SINGLE, N_BATCH = 16, 64


def load_package(pkg_dir, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def stats3(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1]}


def measure(pkg, g, srcs_single, srcs_batch, label, c_walk_single=0.0, c_walk_batch=0.0):
    """REPS repetitions (after one warm-up) of the two workloads on the handle as it stands, under the default and the
    batch profile; c_walk_* > 0 replaces that profile's c_walk_ns."""
    import numpy as np
    t_single, t_batch = pkg.tuning_default(), pkg.tuning_batch()
    if c_walk_single > 0:
        t_single.c_walk_ns = c_walk_single
    if c_walk_batch > 0:
        t_batch.c_walk_ns = c_walk_batch
    out = {"label": label, "c_walk_ns": [t_single.c_walk_ns, t_batch.c_walk_ns]}
    g.set_tuning(t_single)
    g.fora_single_source(int(srcs_single[0]), EPS, ALPHA, seed=SEED, fetch=False)
    qps, mc, dense, walks, steps = [], [], [], [], []
    for _ in range(REPS):
        sts = []
        t0 = time.perf_counter()
        for s in srcs_single:
            sts.append(g.fora_single_source(int(s), EPS, ALPHA, seed=SEED, fetch=False)[1])
        dt = time.perf_counter() - t0
        qps.append(len(srcs_single) / dt)
        mc.append(float(np.median([st.mc_ms for st in sts])))
        dense.append(float(np.mean([st.dense_levels for st in sts])))
        walks.append(float(np.mean([st.walks for st in sts])))
        steps.append(float(np.mean([st.walk_steps for st in sts])))
    out["single"] = {"queries_per_s": stats3(qps), "mc_ms_per_query": stats3(mc), "dense_levels_per_query": dense[0],
                     "walks_per_query": walks[0], "live_steps_per_query": steps[0],
                     "ns_per_walk": stats3([1e6 * m / walks[0] for m in mc])}
    g.set_tuning(t_batch)
    g.fora_batch_single_source(srcs_batch[:16], EPS, ALPHA, seed=SEED, k=8)
    qps, mc, dense, walks = [], [], [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        st = g.fora_batch_single_source(srcs_batch, EPS, ALPHA, seed=SEED, k=8)[5]
        dt = time.perf_counter() - t0
        q = len(srcs_batch)
        qps.append(q / dt)
        mc.append(st.class_ms[3] / q)
        dense.append(st.dense_levels / q)
        walks.append(st.walks / q)
    out["batch16"] = {"queries_per_s": stats3(qps), "mc_ms_per_query": stats3(mc), "dense_levels_per_query": dense[0],
                      "walks_per_query": walks[0], "ns_per_walk": stats3([1e6 * m / walks[0] for m in mc])}
    g.set_tuning(pkg.tuning_default())
    return out


def child(args):
    import numpy as np
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py runs
    import torch  # noqa: F401  (loads the HIP runtime first)
    pkg = load_package(args.package_dir, "pprhip_bench_pkg")
    host = pkg.HostCsr.rmat(args.scale, 16, seed=1)
    live = np.flatnonzero(np.diff(host.out_rp) > 0)
    rng = np.random.default_rng(4)
    srcs_single = rng.choice(live, N_SINGLE, replace=False).astype(np.int32)
    srcs_batch = rng.choice(live, N_BATCH, replace=False).astype(np.int32)
    res = {"build": args.label, "rev": args.rev, "scale": args.scale, "n": int(host.n), "m": int(host.m), "runs": []}
    with pkg.Graph(host) as g:
        res["runs"].append(measure(pkg, g, srcs_single, srcs_batch, "unindexed"))
        if hasattr(pkg.Graph, "build_walk_index"):
            conf = pkg.conf_whole_graph(host.n, host.m, ALPHA)
            rho = pkg.walk_index_density(conf, EPS)
            builds = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                st = g.build_walk_index(ALPHA, SEED)
                builds.append({"wall_ms": (time.perf_counter() - t0) * 1e3, "kernel_ms": st.mc_ms, "steps": int(st.walk_steps)})
            info = g.walk_index_info()
            res["index"] = {"density": rho, "terminals": info["terminals"], "bytes": info["bytes"],
                            "bound_terminals": host.m * rho + host.n, "within_bound": info["terminals"] <= host.m * rho + host.n,
                            "build_kernel_ms": stats3([b["kernel_ms"] for b in builds]),
                            "build_wall_ms": stats3([b["wall_ms"] for b in builds]), "build_steps": builds[0]["steps"]}
            g.walk_index_usage(reset=True)
            run = measure(pkg, g, srcs_single, srcs_batch, "served")
            run["served"], run["walked"] = g.walk_index_usage(reset=True)
            res["runs"].append(run)
            if args.c_walk_single > 0 or args.c_walk_batch > 0:  # the indexed tuning: c_walk_ns = cost of a served walk
                run = measure(pkg, g, srcs_single, srcs_batch, "served, c_walk", args.c_walk_single, args.c_walk_batch)
                run["served"], run["walked"] = g.walk_index_usage(reset=True)
                res["runs"].append(run)
        else:
            res["index"] = None  # a build without the walk index: the baseline
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--baseline", default=None, help="package directory of a built checkout of the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=420, help="time limit of one child, seconds")
    ap.add_argument("--c-walk-single", type=float, default=0.0,
                    help="a further served run with c_walk_ns of the default profile set to this (the cost of a served walk)")
    ap.add_argument("--c-walk-batch", type=float, default=0.0, help="... and of the batch profile to this")
    ap.add_argument("--baseline-rev", default="", help="commit of the baseline build, for the record")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--rev", default="")
    ap.add_argument("--package-dir", default=OWN_PKG)
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = []
    own_rev = args.rev
    if not own_rev:  # (the record names builds by label and commit, never by where they lay)
        p = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                           text=True)
        own_rev = p.stdout.strip() if p.returncode == 0 else "unknown"
    builds = ([(args.baseline, "baseline", args.baseline_rev or "unknown")] if args.baseline else []) + [(OWN_PKG, "this tree", own_rev)]
    for pkg_dir, label, rev in builds:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--scale", str(args.scale), "--package-dir", pkg_dir,
               "--label", label, "--rev", rev, "--c-walk-single", str(args.c_walk_single), "--c-walk-batch",
               str(args.c_walk_batch)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)  # (a time-out raises: the run ends)
        if p.returncode != 0:
            sys.exit("child for the build '%s' ended with status %d: nothing more is started" % (label, p.returncode))
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
        results.append(json.loads(line[7:]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    for r in results:
        print("== %s (%s)  (R-MAT %d, n = %d, m = %d)" % (r["build"], r["rev"], r["scale"], r["n"], r["m"]))
        if r["index"]:
            ix = r["index"]
            print("   index: density %.4f, %d terminals (bound %.0f), %.3f GB, build kernel %.1f ms (median), %d steps" % (
                ix["density"], ix["terminals"], ix["bound_terminals"], ix["bytes"] / 1e9, ix["build_kernel_ms"]["median"],
                ix["build_steps"]))
        for run in r["runs"]:
            for mode in ("single", "batch16"):
                m = run[mode]
                print("   %-14s %-8s %8.1f / %8.1f / %8.1f queries/s   mc %7.3f / %7.3f / %7.3f ms per query   "
                      "%5.2f dense levels   %.3g walks   %6.3f ns per walk (median)" % (
                          run["label"], mode, m["queries_per_s"]["min"], m["queries_per_s"]["median"], m["queries_per_s"]["max"],
                          m["mc_ms_per_query"]["min"], m["mc_ms_per_query"]["median"], m["mc_ms_per_query"]["max"],
                          m["dense_levels_per_query"], m["walks_per_query"], m["ns_per_walk"]["median"]))
            if "served" in run:
                print("   %-14s walks served %d, walked live %d (c_walk_ns %g / %g)" % (
                    run["label"], run["served"], run["walked"], run["c_walk_ns"][0], run["c_walk_ns"][1]))


if __name__ == "__main__":
    main()
