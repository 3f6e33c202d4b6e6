#!/usr/bin/env python3
"""Same-box times of the time-resolved waterfall (zfft_plan_segments_per_line): per-launch
device time (the plan's HIP-event timings, median of 5 calls after 2 warm ones) of the Welch
stage at g = 1, 2, 4 segments per line and g = 0 (one row per frame) in mean, median and max
mode, on the benchmark batches and one cfg2 frame.  At g >= 1 every detector runs the segment
pass ("welch_segs" / "welch4_segs") and a per-line reduction ("welch_lines" for mean,
"welch_select" for median and max); mean lines of the one-workgroup kernels are fused
("welch_lines" alone) and "mean_scratch" times them on the scratch route for comparison; g = 0
mean is "welch_rows" / "welch4", the comparison point.  Every (batch, mode) runs in a child process of its own under a time limit; the first
failure ends the run.  Stamped with the kernel-source hash.
usage: python tools/welch_lines_times.py [OUT.json]   (default profiles/wlines/welch_lines_times.json)"""
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
    "n512": (512, 1, 512, 8704, 16384),  # the Stockham kernel (N < 1024), 33 segments
}
GS = (1, 2, 4, 0)
STEP_LIMIT_S = 180


def one(name, mode):
    import ctypes
    import statistics

    import torch
    from pypanadapter_amd import ZoomFFT
    N, z, W, L, F = BATCHES[name]
    dev = torch.device("cuda", 0)
    x = torch.randn((F, L, 2), device=dev, dtype=torch.float32)
    with ZoomFFT(N, z, 2.4e6, n_win=W, average=mode.split("_")[0]) as plan:
        hook = plan.lib.zfft__plan_lines_route
        hook.argtypes, hook.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
        assert hook(plan._plan, 1 if mode == "mean_scratch" else 0) == 0
        plan.set_timing(True)
        st = torch.cuda.current_stream()
        for g in GS:
            plan.set_segments_per_line(g)
            R = plan.lines(L)
            rows = torch.empty((F * R, W), device=dev, dtype=torch.float32)
            runs = []
            for r in range(7):
                plan.process_device(x.data_ptr(), L, F, rows.data_ptr(), st.cuda_stream)
                torch.cuda.synchronize()
                t = {}
                for nm, ms in zip(plan.launch_names(), plan.timings()):
                    t[nm] = t.get(nm, 0.0) + ms
                if r >= 2:
                    runs.append(t)
            out = {k: round(statistics.median(r[k] for r in runs), 4) for k in runs[0]}
            tot = [sum(v for k, v in r.items() if k.startswith("welch")) for r in runs]
            out["welch_total"] = round(statistics.median(tot), 4)
            out["welch_total_min_max"] = [round(min(tot), 4), round(max(tot), 4)]
            out["lines"] = R
            print(f"RESULT {g} " + json.dumps(out), flush=True)
            del rows


def main(out):
    from pypanadapter_amd import build
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"source_hash": build.source_hash(), "what": "ms per launch name, median of 5 process_device calls "
           "after 2 warm ones; welch_total = the names starting with welch, with its smallest and largest "
           "of the five; key batch/mode/g (g = segments per line, 0 = one row per frame)", "times": {}}
    for name in BATCHES:
        for mode in ("mean", "mean_scratch", "median", "max"):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, mode],
                                   capture_output=True, text=True, timeout=STEP_LIMIT_S)
            except subprocess.TimeoutExpired as e:
                print((e.stdout or b"").decode(errors="replace") + (e.stderr or b"").decode(errors="replace"))
                json.dump(res, open(out, "w"), indent=1)
                sys.exit(f"{name} {mode}: no result within {STEP_LIMIT_S} s; stopping")
            lines = [ln.split(" ", 2) for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            for _, g, js in lines:
                res["times"][f"{name}/{mode}/g{g}"] = json.loads(js)
                print(name, mode, g, js, flush=True)
            json.dump(res, open(out, "w"), indent=1)
            if r.returncode != 0 or len(lines) != len(GS):
                print(r.stdout + r.stderr)
                sys.exit(f"{name} {mode}: failed (exit {r.returncode}); stopping")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3])
    elif len(sys.argv) <= 2:
        main(sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "wlines", "welch_lines_times.json"))
    else:
        sys.exit(__doc__)
