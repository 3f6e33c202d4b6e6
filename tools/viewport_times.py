#!/usr/bin/env python3
"""Same-box times of the display viewport (zfft_viewport_push_device, timing names "view_lines" and
"view_finish"; zfft_viewport_push_render), into profiles/viewport/viewport_times.json:
  streaming   69,632 rows of 512 per push into 256 pixels, per detector, at rows_per_line 64 and 1,
              and 65,536 rows as one group (the split form): the plan's HIP-event timing, median of
              5 pushes after 2 warm ones, from three buffers in turn (428 MB: each push reads from
              HBM), with the bytes read and their share of the streaming rate (6.3 TB/s, MI355X);
              "persist_hist" on the same rows in the same process is the yardstick;
  display     one host row of 8192 columns through viewport_push_render into a page-locked
              1080 x 1920 image, wall clock per call, median of 30 after 5; beside it
              waterfall_push_emit (zfft_waterfall_push_render) of the same row into the ring's
              2048 x 8192 image, the per-line display there was before;
  accuracy    the worst MEAN figures against the float64 rule on 4096 x 512 rows.
The measurements run in a child process under a time limit; a failure ends the run.
usage: python tools/viewport_times.py [OUT.json]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM_GBS = 6300.0
W, WIDTH = 512, 256
STREAMING = {"m64": (69632, 64), "m1": (69632, 1), "one_group_65536": (65536, 65536)}
STEP_LIMIT_S = 300


def result(key, out):
    print(f"RESULT {key} " + json.dumps(out), flush=True)


def one():
    import statistics
    import time

    import numpy as np
    import torch
    from pypanadapter_amd import ZoomFFT, pinned_empty
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    bufs = [-160.0 + 120.0 * torch.rand((69632, W), device=dev, generator=g) for _ in range(3)]

    def timed(plan, push, count, names):
        ms = []
        for r in range(7):
            push(bufs[r % 3].data_ptr(), count, st)
            torch.cuda.synchronize()
            assert plan.launch_names() == names, plan.launch_names()
            ms.append(plan.timings())
        tot = [sum(t) for t in ms[2:]]
        med = statistics.median(tot)
        nbytes = count * W * 4
        return {"ms": round(med, 5), "min_max": [round(min(tot), 5), round(max(tot), 5)],
                "launch_ms": {n: round(statistics.median(t[i] for t in ms[2:]), 5) for i, n in enumerate(names)},
                "bytes": nbytes, "GBps": round(nbytes / med / 1e6, 1),
                "share_of_streaming_rate": round(nbytes / med / 1e6 / STREAM_GBS, 4)}

    with ZoomFFT(4096, 8, 2.4e6, n_win=W) as plan:
        plan.set_timing(True)
        plan.set_persistence(256, -130.0, -2.0)
        for case, (count, m) in STREAMING.items():
            result(f"streaming/{case}/persist_hist", timed(plan, plan.persistence_push_device, count, ["persist_hist"]))
            for det in ("max", "min", "mean"):
                plan.set_viewport(1080, WIDTH, 0, W, det, m)
                out = timed(plan, plan.viewport_push_device, count, ["view_lines", "view_finish"])
                assert plan.viewport_state()[0] == 7 * count
                result(f"streaming/{case}/{det}", out)
        # accuracy of MEAN on many rows, against the float64 rule
        import viewport_ref as vr
        from conftest import row_errors
        host = bufs[0][:4096].cpu().numpy()
        worst = [0.0, 0.0]
        for m, width in ((64, 256), (4096, 64)):
            plan.set_viewport(64, width, 0, W, "mean", m)
            plan.viewport_push(host)
            img = plan.viewport_image()[64 - 4096 // m:]
            ref, _ = vr.ref_lines(host, W, (0, W, width), "mean", m)
            for a, b in zip(img, ref):
                ddb, damp = row_errors(a, b)
                worst = [max(worst[0], ddb), max(worst[1], damp)]
        result("accuracy/mean_4096x512", {"max_abs_ddB": worst[0], "max_damp_over_peak": worst[1]})
        plan.set_viewport(0, 0)

    row = (-160.0 + 120.0 * np.random.default_rng(5).random(8192)).astype(np.float32)

    def wall(call, n=35, warm=5):
        t = []
        for _ in range(n):
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e3)
        t = t[warm:]
        return {"ms": round(statistics.median(t), 4), "min_max": [round(min(t), 4), round(max(t), 4)]}

    with ZoomFFT(8192, 1, 2.4e6, n_win=8192) as plan:
        plan.set_viewport(1080, 1920, 0, 8192, "max", 1)
        out = pinned_empty((1080, 1920, 4), np.uint8)
        res = wall(lambda: plan.viewport_push_render(row, out))
        res["image_bytes"] = out.nbytes
        result("display/viewport_push_render_1080x1920", res)
        small = pinned_empty((270, 480, 4), np.uint8)
        plan.set_viewport(270, 480, 0, 8192, "max", 1)
        res = wall(lambda: plan.viewport_push_render(row, small))
        res["image_bytes"] = small.nbytes
        result("display/viewport_push_render_270x480_zero_copy", res)
        plan.set_viewport(0, 0)
        big = pinned_empty((2048, 8192, 4), np.uint8)
        res = wall(lambda: plan.waterfall_push_emit(row.reshape(1, -1), False, big), n=15, warm=3)
        res["image_bytes"] = big.nbytes
        result("display/waterfall_push_render_2048x8192", res)


def main(out):
    from pypanadapter_amd import build
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"source_hash": build.source_hash(),
           "what": "streaming: view_lines + view_finish ms by the plan's timings, median of 5 pushes after 2 warm "
                   "ones, three buffers in turn, bytes = count x 512 x 4 read; display: wall clock ms per call",
           "times": {}}
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"], capture_output=True, text=True,
                           timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        print((e.stdout or b"").decode(errors="replace") + (e.stderr or b"").decode(errors="replace"))
        sys.exit(f"no result within {STEP_LIMIT_S} s; stopping")
    lines = [ln.split(" ", 2) for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    for _, key, js in lines:
        res["times"][key] = json.loads(js)
        print(key, js, flush=True)
    json.dump(res, open(out, "w"), indent=1)
    if r.returncode != 0 or len(lines) != 16:
        print(r.stdout + r.stderr)
        sys.exit(f"failed (exit {r.returncode}, {len(lines)} results); stopping")


if __name__ == "__main__":
    if sys.argv[1:] == ["--one"]:
        one()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "viewport", "viewport_times.json"))
