"""bench.py on the GPU: a plain run measures the headline only, --full adds what takes runs of its own."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("kernel_ms_per_query", "kernel_class_time", "cpu_baseline", "one_query_at_a_time", "topk_sample",
             "all_pair_sample", "all_pair_rmat24", "all_pair_scaling", "value_q50", "compute_stream_idle_frac")


def _bench_line(args, tmpdir):
    os.makedirs(tmpdir, exist_ok=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, TMPDIR=tmpdir))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_full_adds_the_rest(tmp_path):
    base = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--scale", "16", "--queries-per-step", "16"]
    plain = _bench_line(base + ["--dump-outputs", str(tmp_path / "dump")], str(tmp_path / "t_plain"))
    assert all(k in plain for k in HEADLINE) and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["self_check"]["status"] == "ok" and plain["dumped_outputs"]["step"] == 2
    assert not [k for k in FULL_ONLY if k in plain] and "other_kernels" not in plain["roofline"]
    # --full without the samples, counter passes and CPU baselines: the step with every kernel class timed
    full = _bench_line(base + ["--full", "--no-extras", "--no-pmc", "--no-cpu-baseline"], str(tmp_path / "t_full"))
    assert all(k in full for k in HEADLINE) and full["kernel_ms_per_query"] and "other_kernels" in full["roofline"]
    assert full["self_check"]["status"] == "ok"
    assert not [x for x in os.listdir(tmp_path / "t_full") if x.startswith("pprhip_bench_graphs_")]  # (gone with the run)
