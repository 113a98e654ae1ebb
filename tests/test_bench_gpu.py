"""A plain `bench.py` run on the GPU: one timed region of exactly K steps, none of the --full legs in its line, and --dump-outputs
writing the fused rows of the last timed step -- the same rows on a second run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _plain(out_dir):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.lstrip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "fused_av_embedding.npy"))


def test_plain_bench_times_k_steps_and_dumps_the_last_one(tmp_path):
    res, rows = _plain(tmp_path / "a")
    assert res["steps"] == 3 and res["warmup"] == 1 and res["dtype"] == "f16x3" and res["higher_is_better"] is True
    assert res["value_regions"] == [res["value"]]                                   # one timed region
    assert abs(res["value"] * res["ms_per_step"] / 1e3 - 64) < 0.05 * 64           # ms_per_step is one step of 64 pairs
    for leg in ("alt_mode", "configs", "cpu_baseline", "parity", "h2d_inclusive", "ranks"):
        assert leg not in res, leg
    assert rows.dtype == np.float32 and rows.shape == (64, 1024) and np.isfinite(rows).all()
    _, again = _plain(tmp_path / "b")
    assert np.array_equal(rows, again)
