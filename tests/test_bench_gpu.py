"""bench.py's plain run on the device: one JSON line whose steps and ms_per_step are the timed K1 steps, and --dump-outputs writes what the
last step computed -- checked against the CPU oracle on the same synthetic boards (bit-exact; the float64 files hold the int32 values)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_plain_run_dumps_the_last_steps_outputs(tmp_path, oracle):
    import bench
    from gomokuai_amd import lib as G
    n = 4 * bench.DUMP_BOARDS_CELLS                         # more boards than the per-cell cap: scores / density come from the seeded sample
    out_dir = str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "7", "--warmup", "2", "--boards", str(n), "--dump-outputs", out_dir],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["metric"] == "board-evals/s"
    for leg in ("secondary", "selfplay_pipeline", "incremental", "supervisor", "poolrave", "network_guided", "cpu_baseline"):
        assert leg not in line, "a plain run measures the headline only (%s is --full's)" % leg
    assert line["roofline"]["without_settling"] is None
    moves, lens, _ = G.synth_boards(n, 0, first_board=0)
    ref = dict(zip(("scores", "density", "totals", "status"), oracle.replay_batch(moves, lens)))
    sample = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, size=bench.DUMP_BOARDS_CELLS, replace=False))
    for name, rows in (("scores", sample), ("density", sample), ("totals", slice(None)), ("status", slice(None))):
        got = np.load(os.path.join(out_dir, name + ".npy"))
        assert got.dtype == np.float64
        assert np.array_equal(got, ref[name][rows].astype(np.float64)), "%s differs from the oracle" % name
