"""bench.py's contract: --steps K times exactly K steps, the line carries ms_per_step, and --dump-outputs writes what the
last timed step computed -- the same arrays, bit for bit, from two runs with the same arguments (seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


FULL_ONLY = ("roofline", "distinct_batches", "epoch_loop", "dropin_loop", "neuralnet_train", "inference_loop", "other_nets",
             "cpu_baseline")


def _line(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args)
    run = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    line = [ln for ln in run.stdout.decode().splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def _bench(out_dir, steps, warmup):
    return _line("--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", out_dir, "--no-cpu-baseline",
                 "--epoch-graphs", "0", "--no-other-nets")


def test_plain_run_reports_the_timed_steps_alone_and_full_adds_the_secondary_figures():
    plain = _line("--steps", "3", "--warmup", "1")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain, key
    assert plain["value"] > 0 and plain["unit"] == "graphs/s" and plain["higher_is_better"] is True
    assert not [k for k in FULL_ONLY if k in plain]
    # --full, with the long legs dropped again by their own options: the roofline and the CPU oracle come back
    full = _line("--steps", "3", "--warmup", "1", "--full", "--epoch-graphs", "0", "--no-other-nets", "--cpu-seconds", "1")
    assert full["roofline"]["kernel_us"] > 0 and full["roofline"]["kernel"] in full["roofline"]["kernels"]
    assert full["cpu_baseline"]["value"] > 0
    assert not [k for k in FULL_ONLY if k in full and k not in ("roofline", "cpu_baseline")]


def test_steps_are_the_timed_steps_and_dumped_outputs_repeat(tmp_path):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    res = [_bench(d, 7, 3) for d in dirs]
    for r in res:
        assert r["steps"] == 7 and r["timed_steps"] == 7 and r["repeats"] == 1
        assert r["ms_per_step"] > 0 and abs(r["ms_per_step"] - r["timed_seconds"] * 1e3 / 7) < 1e-9
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {"pred.npy", "loss.npy"} <= set(names)
    assert any(n.startswith("grad.") for n in names) and any(n.startswith("param.") for n in names)
    total = 0
    for n in names:
        a, b = np.load(os.path.join(dirs[0], n)), np.load(os.path.join(dirs[1], n))
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        np.testing.assert_array_equal(a, b, err_msg=n)
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(os.path.join(dirs[0], "pred.npy")).size == 64
    loss = np.load(os.path.join(dirs[0], "loss.npy")).reshape(-1)
    assert loss.size == 1
    np.testing.assert_allclose(float(loss[0]), res[0]["config"]["final_loss"], rtol=1e-6)
