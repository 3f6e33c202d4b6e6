#!/usr/bin/env python3
"""Same-box times of the Welch detectors (zfft_plan_average): per-launch device time (the plan's
HIP-event timings, median of 5 calls after 2 warm ones) of the Welch stage in mean, median and
max mode on the benchmark batches -- mean's "welch_rows" / "welch4" next to the detectors'
"welch_segs" / "welch4_segs" + "welch_select" (summed over the chunks) -- and of the segment
scratch cap (the default, 1 GiB: one launch set for these batches, against smaller caps).  Every (batch, mode,
cap) runs in a child process of its own under a time limit; the first failure ends the run.
Stamped with the kernel-source hash.  usage: python tools/welch_average_times.py OUT.json"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = {  # name: (n_fft, zoom, n_win, L, frames)
    "cfg2": (4096, 8, 512, 299008, 4096),
    "cfg1": (1024, 4, 256, 262144, 4096),
    "cfg5": (65536, 8, 8192, 1048576, 2048),
    "cfg2_one_frame": (4096, 8, 512, 299008, 1),
}
CAPS_MB = {"cfg2": (0, 64), "cfg1": (0, 64, 128, 256), "cfg5": (0, 64), "cfg2_one_frame": (0,)}
STEP_LIMIT_S = 120


def one(name, mode, cap_mb):
    import ctypes
    import statistics

    import torch
    from pypanadapter_amd import ZoomFFT
    N, z, W, L, F = BATCHES[name]
    dev = torch.device("cuda", 0)
    x = torch.randn((F, L, 2), device=dev, dtype=torch.float32)
    rows = torch.empty((F, W), device=dev, dtype=torch.float32)
    with ZoomFFT(N, z, 2.4e6, n_win=W, average=mode) as plan:
        hook = plan.lib.zfft__plan_average_cap
        hook.argtypes, hook.restype = [ctypes.c_void_p, ctypes.c_int64], ctypes.c_int
        assert hook(plan._plan, cap_mb << 20) == 0
        plan.set_timing(True)
        st = torch.cuda.current_stream()
        runs = []
        for r in range(7):
            plan.process_device(x.data_ptr(), L, F, rows.data_ptr(), st.cuda_stream)
            torch.cuda.synchronize()
            t = {}
            for nm, ms in zip(plan.launch_names(), plan.timings()):
                t[nm] = t.get(nm, 0.0) + ms
            t["chunks"] = plan.launch_names().count("welch_select")
            if r >= 2:
                runs.append(t)
    out = {k: round(statistics.median(r[k] for r in runs), 4) for k in runs[0]}
    out["welch_total"] = round(statistics.median(sum(v for k, v in r.items() if k.startswith("welch")) for r in runs), 4)
    print("RESULT " + json.dumps(out), flush=True)


def main(out):
    from pypanadapter_amd import build
    res = {"source_hash": build.source_hash(), "what": "ms per launch name (summed over chunks), median of 5 "
           "process_device calls after 2 warm ones; cap_mb 0 = the default (1024: one launch set here)",
           "times": {}}
    for name in BATCHES:
        for mode in ("mean", "median", "max"):
            for cap in (CAPS_MB[name] if mode == "median" else (0,)):  # the cap sweep in median mode
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, mode, str(cap)],
                                   capture_output=True, text=True, timeout=STEP_LIMIT_S)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    print(r.stdout + r.stderr)
                    json.dump(res, open(out, "w"), indent=1)
                    sys.exit(f"{name} {mode} cap {cap}: failed (exit {r.returncode}); stopping")
                res["times"][f"{name}/{mode}/cap{cap}"] = json.loads(line[0][7:])
                print(name, mode, cap, line[0][7:], flush=True)
                json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    elif len(sys.argv) == 2:
        main(sys.argv[1])
    else:
        sys.exit(__doc__)
