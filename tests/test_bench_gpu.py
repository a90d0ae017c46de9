"""GPU: `bench.py --gpus 1 --steps K --warmup W` as it is run for every change -- one JSON line with the headline fields and
none of what --full adds -- and --dump-outputs: what the last timed step returned, from the same inputs and with the same
kernels in every run with the same arguments, so that two runs agree bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch-per-gpu", "2"] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_outputs(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "a"))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["config"]["batch_per_gpu"] == 2
    assert d["unit"] == "clips/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - 2) < 0.01      # clips per second over the same timed steps
    assert not {"roofline", "box", "cpu_baseline"} & set(d), sorted(d)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["buffers.npy", "grads.npy", "loss.npy", "out_noun.npy", "out_verb.npy", "params.npy"], files
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert a["out_verb"].shape == (2, 125) and a["out_noun"].shape == (2, 352)
    assert all(x.dtype == np.float32 and np.isfinite(x).all() for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    # a second process with the same arguments: same inputs and initial weights and, from bench_plans.json, the same
    # kernels (bench.pin_plans) -- so the same bits; each process tuning its own plan would differ beyond rounding
    assert d["config"]["launch_plans"] == "committed (bench_plans.json)", d["config"]["launch_plans"]
    _bench("--dump-outputs", str(tmp_path / "b"))
    for k, x in a.items():
        assert np.array_equal(x, np.load(tmp_path / "b" / (k + ".npy"))), k
