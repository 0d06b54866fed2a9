"""Child process of tests/test_gpu_topk_round_designs.py::test_without_the_one_workgroup_kernel.

levels.cpp reads PPRHIP_SPARSE_WG once per process, so the parent starts this process with PPRHIP_SPARSE_WG=0: every
sparse level of every top-k round then runs as its two launches (k_sparse_prepare, k_sparse_push), where the armed bits
are taken by many workgroups at once.  Runs every design of tests/topk_round_designs.py round by round, writes vectors,
residue sums and counters to the file named on the command line and prints "ok"."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
# (PPRHIP_SPARSE_WG is a test switch, compiled into libpprhip_hooks.so only)
os.environ.setdefault("PPRHIP_LIB_PATH", os.path.join(ROOT, "personalized-pagerank-algorithms-on-neo4j_amd", "libpprhip_hooks.so"))
assert os.environ.get("PPRHIP_SPARSE_WG") == "0", "the parent sets the switch"
pkg = importlib.import_module("personalized-pagerank-algorithms-on-neo4j_amd")

import test_gpu_topk_round_designs as G  # noqa: E402

G.child_main(pkg, sys.argv[1])
print("ok")
