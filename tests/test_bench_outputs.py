"""bench.py's plain run and `--dump-outputs`: exactly `--steps` timed steps, none of the
`--full` legs, and the last step's rows and waterfall image written as float32 arrays that a
second computation on the same seeded inputs reproduces bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bounded_sample_is_fixed_and_within_budget():
    small = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert bench.bounded_sample(small, 1) is small
    w = 8192
    n = bench.DUMP_MAX_BYTES // (4 * w)
    big = np.broadcast_to(np.arange(n + 100, dtype=np.float32)[:, None], (n + 100, w))
    a, b = bench.bounded_sample(big, 1), bench.bounded_sample(big, 1)
    assert a.shape == (n, w) and a.nbytes <= bench.DUMP_MAX_BYTES
    np.testing.assert_array_equal(a, b)
    assert (np.diff(a[:, 0]) > 0).all()  # rows keep their order, none twice
    assert 2 * bench.DUMP_MAX_BYTES <= 64_000_000  # rows + waterfall together


@pytest.mark.gpu
def test_plain_run_times_the_steps_asked_and_dumps_its_outputs(tmp_path):
    import torch
    from pypanadapter_amd import ZoomFFT
    F, steps = 128, 3
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                          str(steps), "--warmup", "1", "--frames", str(F), "--dump-outputs",
                          str(tmp_path)], capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    res = json.loads(lines[0])
    assert res["steps"] == steps and res["full"] is False
    # both figures are rounded to 4 decimals: 5e-5 s on timed_seconds, 5e-8 s per step
    assert res["ms_per_step"] > 0
    assert abs(res["ms_per_step"] * steps / 1e3 - res["timed_seconds"]) <= 1e-4
    assert res["unit"] == "MS/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["metric"] == bench.METRIC
    # the legs behind --full did not run
    assert res["cpu_baseline"] is None and res["end_to_end"] is None
    assert res["parity_checked_frames"] is None and not res["kernels"]
    assert sorted(os.listdir(tmp_path)) == ["rows.npy", "waterfall.npy"]
    rows = np.load(tmp_path / "rows.npy")
    img = np.load(tmp_path / "waterfall.npy")

    cfg = bench.CONFIGS["cfg2"]
    N, z, fs = cfg["n_fft"], cfg["zoom"], cfg["fs"]
    L, W = N * cfg["n_avg"], N // z
    assert rows.dtype == np.float32 and rows.shape == (F, W) and np.isfinite(rows).all()
    assert img.dtype == np.float32 and img.shape == (W // 4, W)
    # the same seeded frames through a plan of our own: identical inputs, identical arrays
    dev = torch.device("cuda", 0)
    x = bench.make_frames(torch, F, L, cfg, dev, 1234)
    d_rows = torch.empty((F, W), dtype=torch.float32, device=dev)
    with ZoomFFT(N, z, fs, n_win=W) as plan:
        st = torch.cuda.current_stream().cuda_stream
        plan.process_device(x.data_ptr(), L, F, d_rows.data_ptr(), st)
        plan.waterfall_push_device(d_rows.data_ptr(), F, st)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(plan.waterfall_image(), img)  # F = H: one push fills it
    np.testing.assert_array_equal(d_rows.cpu().numpy(), rows)
