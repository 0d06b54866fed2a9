"""Developer benchmark: the sweep cut (pprhip_sweep_cut) on R-MAT <scale>, alpha 0.15.

forward_push from one live source (the node of largest out-degree) at rmax in {1e-5, 1e-7, rmax0 of eps = 0.5}, then the
sweep over the vector left in HBM, three repetitions each (min / median / max): support, edge slots, the sort, scan and
total times of the sweep (HIP events), the edge slots per second of the scan kernel and its algorithmic bytes per second
at 8 bytes per slot (one streamed 4-byte column index, one gathered 4-byte rank), beside push_ms of the call that made the
vector.  For comparison: the host doing the same by itself - fetching the vector and running tests/sweep_ref.py's numpy
sweep on this box's CPU, once per rmax - with its result checked against the device's.

Usage: python tools/bench_sweep.py [--scale 22] [--out FILE.json] [--no-host]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ALPHA, EPS, REPS = 0.15, 0.5, 3
SLOT_BYTES = 8


def stats3(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1]}


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
    from sweep_ref import edges_of, sweep_ref
    host = pkg.HostCsr.rmat(args.scale, 16, seed=1)
    src = int(np.argmax(np.diff(host.out_rp.astype(np.int64))))
    conf = pkg.conf_whole_graph(host.n, host.m, ALPHA)
    rmax0 = pkg.fora_whole_params(conf, EPS)[0]
    edges = None if args.no_host else edges_of(host)
    res = {"scale": args.scale, "n": int(host.n), "m": int(host.m), "alpha": ALPHA, "source": src, "slot_bytes": SLOT_BYTES,
           "rows": []}
    with pkg.Graph(host) as g:
        g.forward_push(src, ALPHA, 1e-3, fetch=False)
        g.sweep_cut(cap=0)  # warm-up: the workspace, the library sorts' first launch
        for label, rmax in (("1e-5", 1e-5), ("1e-7", 1e-7), ("rmax0(eps=0.5)", rmax0)):
            push, infos = [], []
            for _ in range(REPS):
                st = g.forward_push(src, ALPHA, rmax, fetch=False)[3]
                push.append(st.push_ms)
                infos.append(g.sweep_cut(cap=0)[3])
            i0 = infos[0]
            row = {"rmax": label, "rmax_value": rmax, "support": int(i0.support), "edge_slots": int(i0.edge_slots),
                   "best_size": int(i0.best_size), "best_conductance": i0.best_conductance,
                   "push_ms": stats3(push), "sort_ms": stats3([i.sort_ms for i in infos]),
                   "scan_ms": stats3([i.scan_ms for i in infos]), "total_ms": stats3([i.total_ms for i in infos])}
            row["scan_slots_per_s"] = stats3([i.edge_slots / (i.scan_ms * 1e-3) for i in infos])
            row["scan_GB_per_s"] = stats3([SLOT_BYTES * i.edge_slots / (i.scan_ms * 1e-3) / 1e9 for i in infos])
            if edges is not None:
                t0 = time.perf_counter()
                x = g.reserve()
                t1 = time.perf_counter()
                ref = sweep_ref(host.n, edges[0], edges[1], x)
                t2 = time.perf_counter()
                row["host_fetch_ms"] = (t1 - t0) * 1e3
                row["host_sweep_ms"] = (t2 - t1) * 1e3
                row["host_agrees"] = bool(ref["best_size"] == i0.best_size and ref["best_cut"] == i0.best_cut and
                                          ref["best_vol"] == i0.best_vol and ref["support"] == i0.support and
                                          ref["best_conductance"] == i0.best_conductance)
            res["rows"].append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print("R-MAT %d, n = %d, m = %d, source %d, alpha %.2f; medians of %d" % (args.scale, host.n, host.m, src, ALPHA, REPS))
    for r in res["rows"]:
        print("  rmax %-15s support %9d  slots %10d  push %8.3f ms | sweep %7.3f ms = sort %6.3f + scan %6.3f + rest; "
              "scan %6.2f G slots/s (%6.1f GB/s)%s" % (
                  r["rmax"], r["support"], r["edge_slots"], r["push_ms"]["median"], r["total_ms"]["median"],
                  r["sort_ms"]["median"], r["scan_ms"]["median"], r["scan_slots_per_s"]["median"] / 1e9,
                  r["scan_GB_per_s"]["median"],
                  "" if "host_sweep_ms" not in r else " | host: fetch %.1f + numpy sweep %.0f ms, agrees: %s" % (
                      r["host_fetch_ms"], r["host_sweep_ms"], r["host_agrees"])))
    print("RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
