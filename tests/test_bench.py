"""bench.py's plain run and --dump-outputs.

* CPU: the dump helper keeps the float dtypes, stays within its 64 MB and samples the same positions on every run;
* GPU: a plain run times exactly --steps steps in one window, prints the headline keys without the --full ones, and writes what
  the timed ResNet step computed in its last step.
"""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_dtypes_limit_and_repeatable_sample(tmp_path):
    rng = np.random.default_rng(3)
    arrays = [("loss", np.array([2.5], np.float32)), ("index", np.arange(10, dtype=np.int64)),
              ("wide", rng.random((4096, 4096)).astype(np.float32)), ("wide64", rng.random((2048, 4096))),
              ("half", rng.random((4096, 2048)).astype(np.float16))]
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    files = sorted(glob.glob(str(tmp_path / "a" / "*.npy")))
    assert [os.path.basename(f) for f in files] == ["half.npy", "index.npy", "loss.npy", "wide.npy", "wide64.npy"]
    assert sum(os.path.getsize(f) for f in files) <= bench.DUMP_LIMIT_BYTES
    got = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    assert got["loss"].dtype == np.float32 and got["loss"].tolist() == [2.5]
    assert got["index"].dtype == np.float64 and got["index"].tolist() == list(range(10))
    assert got["wide64"].dtype == np.float64 and got["wide"].dtype == np.float32 and got["half"].dtype == np.float32
    assert got["wide"].size < 4096 * 4096 and np.isin(got["wide"], arrays[2][1]).all()
    for name, arr in got.items():
        assert np.array_equal(arr, np.load(str(tmp_path / "b" / f"{name}.npy"))), name


@pytest.mark.gpu
def test_plain_run_times_exactly_the_steps_and_dumps_the_last_step(gpu, tmp_path):
    out_dir = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "64",
                          "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["metric"] == "training-step samples/sec" and line["unit"] == "samples/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["steps"] == 3 and line["full"] is False
    assert line["timed_windows"]["count"] == 1
    assert line["ms_per_step"] > 0 and abs(line["value"] - 64 / (line["ms_per_step"] / 1e3)) <= 1e-6 * line["value"]
    assert not {"roofline", "cpu_baseline", "also", "kernel_classes", "step_roofline"} & set(line)
    files = sorted(glob.glob(str(out_dir / "*.npy")))
    names = [os.path.basename(f)[:-4] for f in files]
    assert "loss_sum" in names
    assert sum(n.startswith("grad_") for n in names) == 37 and sum(n.startswith("state_") for n in names) == 74
    assert sum(os.path.getsize(f) for f in files) <= bench.DUMP_LIMIT_BYTES
    for f in files:
        arr = np.load(f)
        assert arr.dtype in (np.float32, np.float64) and np.isfinite(arr).all(), f
