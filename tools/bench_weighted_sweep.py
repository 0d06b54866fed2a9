"""Developer benchmark: the sweep cut by relationship weight (pprhip_weighted_sweep_cut) on R-MAT <scale>, alpha 0.15.

Two weight sets, uniform (0.5, 1.5) and Pareto(1.5) + 0.01, drawn with a fixed seed.  For each: the vectors of a weighted
push from one live source (the node of largest out-degree) at rmax 1e-4 and 1e-7 and of weighted_fora at eps = 0.5.  Each
vector is swept REPS times after a warm-up, the weighted and the unweighted sweep of the same vector alternating on the
same handle in the same run (median, min - max): support, edge slots, the sort, scan and total times of both sweeps (HIP
events), and the ratio of the two scan kernels' medians.  The weighted scan streams 12 bytes per slot (a 4-byte column
index and an 8-byte weight) where the unweighted one streams 4, both with the same random 4-byte gather of the rank.
Once per weight set: the one-off build of qdeg (the host's clock around the first weighted sweep after set_weights, which
ends in a device synchronise, less the same clock around the sweep repeated).  For comparison: the host doing the same
by itself - fetching the vector and running tests/weighted_sweep_ref.py's numpy sweep on this box's CPU, once per vector -
with its result checked against the device's.

Usage: python tools/bench_weighted_sweep.py [--scale 22] [--out FILE.json] [--no-host]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ALPHA, EPS, REPS = 0.15, 0.5, 5
W_SLOT_BYTES, U_SLOT_BYTES = 16, 8   # streamed + gathered bytes per slot: 4 + 8 + 4 weighted, 4 + 4 unweighted


def stats(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1]}


def times(infos):
    return {k: stats([getattr(i, k) for i in infos]) for k in ("sort_ms", "scan_ms", "total_ms")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy sweep on the CPU")
    args = ap.parse_args()
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py runs
    import importlib

    import numpy as np
    pkg = importlib.import_module("personalized-pagerank-algorithms-on-neo4j_amd")
    from sweep_ref import edges_of
    from weighted_sweep_ref import weighted_sweep_ref
    host = pkg.HostCsr.rmat(args.scale, 16, seed=1)
    src = int(np.argmax(np.diff(host.out_rp.astype(np.int64))))
    edges = None if args.no_host else edges_of(host)
    rng = np.random.default_rng(7)
    sets = [("uniform(0.5, 1.5)", rng.uniform(0.5, 1.5, host.m)), ("pareto(1.5) + 0.01", rng.pareto(1.5, host.m) + 0.01)]
    res = {"scale": args.scale, "n": int(host.n), "m": int(host.m), "alpha": ALPHA, "source": src, "reps": REPS,
           "weighted_slot_bytes": W_SLOT_BYTES, "unweighted_slot_bytes": U_SLOT_BYTES, "weight_sets": []}
    with pkg.Graph(host) as g:
        g.forward_push(src, ALPHA, 1e-3, fetch=False)
        g.sweep_cut(cap=0)  # warm-up: the workspace, the library sorts' first launch
        for wname, w in sets:
            g.set_weights(w)
            g.weighted_forward_push(src, ALPHA, 1e-3, fetch=False)
            t0 = time.perf_counter()
            first = g.weighted_sweep_cut(cap=0)[3]
            t1 = time.perf_counter()
            g.weighted_sweep_cut(cap=0)
            t2 = time.perf_counter()
            out = {"weights": wname, "shift": int(first.shift), "total_vol_q": int(first.total_vol_q),
                   "first_sweep_wall_ms": (t1 - t0) * 1e3, "second_sweep_wall_ms": (t2 - t1) * 1e3,
                   "qdeg_build_ms": (t1 - t0) * 1e3 - (t2 - t1) * 1e3, "rows": []}
            runs = [("push rmax 1e-4", lambda: g.weighted_forward_push(src, ALPHA, 1e-4, fetch=False)[3]),
                    ("push rmax 1e-7", lambda: g.weighted_forward_push(src, ALPHA, 1e-7, fetch=False)[3]),
                    ("fora eps 0.5", lambda: g.weighted_fora(src, EPS, ALPHA, seed=3, fetch=False)[1])]
            for label, run in runs:
                st = run()
                g.weighted_sweep_cut(cap=0)  # warm-up at this vector's shapes, both sweeps
                g.sweep_cut(cap=0)
                wi, ui = [], []
                for _ in range(REPS):        # alternating
                    wi.append(g.weighted_sweep_cut(cap=0)[3])
                    ui.append(g.sweep_cut(cap=0)[3])
                i0 = wi[0]
                row = {"vector": label, "query_ms": st.total_ms, "support": int(i0.support), "edge_slots": int(i0.edge_slots),
                       "best_size": int(i0.best_size), "best_conductance": i0.best_conductance,
                       "unweighted_best_size": int(ui[0].best_size), "weighted": times(wi), "unweighted": times(ui)}
                row["scan_ratio"] = row["weighted"]["scan_ms"]["median"] / row["unweighted"]["scan_ms"]["median"]
                row["total_ratio"] = row["weighted"]["total_ms"]["median"] / row["unweighted"]["total_ms"]["median"]
                row["weighted_scan_GB_per_s"] = W_SLOT_BYTES * i0.edge_slots / (row["weighted"]["scan_ms"]["median"] * 1e-3) / 1e9
                row["unweighted_scan_GB_per_s"] = U_SLOT_BYTES * i0.edge_slots / (row["unweighted"]["scan_ms"]["median"] * 1e-3) / 1e9
                if edges is not None:
                    t0 = time.perf_counter()
                    x = g.reserve()
                    t1 = time.perf_counter()
                    ref = weighted_sweep_ref(host.n, edges[0], edges[1], w, x)
                    t2 = time.perf_counter()
                    row["host_fetch_ms"] = (t1 - t0) * 1e3
                    row["host_sweep_ms"] = (t2 - t1) * 1e3
                    row["host_agrees"] = bool(
                        ref["best_size"] == i0.best_size and ref["best_cut_q"] == i0.best_cut_q and
                        ref["best_vol_q"] == i0.best_vol_q and ref["support"] == i0.support and
                        ref["best_conductance"] == i0.best_conductance and ref["total_vol_q"] == i0.total_vol_q and
                        ref["shift"] == i0.shift)
                out["rows"].append(row)
            res["weight_sets"].append(out)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print("R-MAT %d, n = %d, m = %d, source %d, alpha %.2f; medians of %d (min - max)" % (
        args.scale, host.n, host.m, src, ALPHA, REPS))
    for s in res["weight_sets"]:
        print(" weights %s: shift %d, qdeg build %.3f ms (first sweep %.3f ms, repeated %.3f ms on the host's clock)" % (
            s["weights"], s["shift"], s["qdeg_build_ms"], s["first_sweep_wall_ms"], s["second_sweep_wall_ms"]))
        for r in s["rows"]:
            wt, ut = r["weighted"], r["unweighted"]
            print("  %-15s support %9d  slots %10d | weighted %7.3f ms (%.3f - %.3f) = sort %6.3f + scan %6.3f (%.3f - %.3f)"
                  " + rest | unweighted %7.3f ms (%.3f - %.3f), scan %6.3f (%.3f - %.3f) | scan ratio %.2f%s" % (
                      r["vector"], r["support"], r["edge_slots"], wt["total_ms"]["median"], wt["total_ms"]["min"],
                      wt["total_ms"]["max"], wt["sort_ms"]["median"], wt["scan_ms"]["median"], wt["scan_ms"]["min"],
                      wt["scan_ms"]["max"], ut["total_ms"]["median"], ut["total_ms"]["min"], ut["total_ms"]["max"],
                      ut["scan_ms"]["median"], ut["scan_ms"]["min"], ut["scan_ms"]["max"], r["scan_ratio"],
                      "" if "host_sweep_ms" not in r else " | host: fetch %.1f + numpy sweep %.0f ms, agrees: %s" % (
                          r["host_fetch_ms"], r["host_sweep_ms"], r["host_agrees"])))
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
