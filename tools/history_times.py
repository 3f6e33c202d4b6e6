#!/usr/bin/env python3
"""Same-box times of the row history (zfft_plan_history; timing names "history_pack",
"history_unpack", "history_view", "history_finish"), into profiles/history/history_times.json:
  pack      69,632 rows of 512 per push, and one row of 8192, per format: the plan's HIP-event
            timing, median of 5 pushes after 2 warm ones, from three buffers in turn (428 MB: each
            push reads from HBM), with the bytes moved (floats read + codes written) and their share
            of the streaming rate (6.3 TB/s, MI355X);
  view      a store of 130,680 rows of 8192 columns (1.07 GB as U8: larger than the 256 MiB
            Infinity Cache) reduced to 1080 x 1920 at rows_per_line 121, MAX and MEAN, per format,
            with the stored bytes read and their share of the streaming rate;
  baseline  the same rows as float32 (4.28 GB) through zfft_viewport_push_device into a 1080 x 1920
            viewport with the same rows_per_line, in the same process: the code there was before.
            ratio = baseline ms / U8 MAX view ms; the view reads a quarter of the bytes;
  unpack    history_unpack of the whole U8 store into float rows.
Each step runs in a child process under its own time limit; a failure ends the run.
usage: python tools/history_times.py [OUT.json]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_GBS = 6300.0
LO, HI = -150.0, -50.0
FORMATS = {"f32": 4, "u16": 2, "u8": 1}
STEPS = {"pack": 7, "view": 8}  # step: results expected
STEP_LIMIT_S = 240


def result(key, out):
    print(f"RESULT {key} " + json.dumps(out), flush=True)


def timed(plan, call, names, nbytes):
    """Median of 5 calls after 2 warm ones of the plan's own timings, summed over the launches;
    call(r) is the r-th."""
    import statistics

    import torch
    ms = []
    for r in range(7):
        call(r)
        torch.cuda.synchronize()
        assert plan.launch_names() == names, plan.launch_names()
        ms.append(plan.timings())
    tot = [sum(t) for t in ms[2:]]
    med = statistics.median(tot)
    return {"ms": round(med, 5), "min_max": [round(min(tot), 5), round(max(tot), 5)],
            "launch_ms": {n: round(statistics.median(t[i] for t in ms[2:]), 5) for i, n in enumerate(names)},
            "bytes": nbytes, "GBps": round(nbytes / med / 1e6, 1),
            "share_of_streaming_rate": round(nbytes / med / 1e6 / STREAM_GBS, 4)}


def step_pack():
    import torch
    from pypanadapter_amd import ZoomFFT
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    for key, n_fft, zoom, W, count in (("69632x512", 4096, 8, 512, 69632), ("1x8192", 8192, 1, 8192, 1)):
        # three buffers in turn (428 MB for the streaming case): each push reads from HBM
        bufs = [-160.0 + 120.0 * torch.rand((count, W), device=dev, generator=g) for _ in range(3)]
        rows = bufs[0]
        with ZoomFFT(n_fft, zoom, 2.4e6, n_win=W) as plan:
            plan.set_timing(True)
            for fmt, eb in FORMATS.items():
                plan.set_history(count, fmt, LO, HI)
                out = timed(plan, lambda r: plan.history_push_device(bufs[r % 3].data_ptr(), count, st), ["history_pack"],
                            count * W * (4 + eb))
                assert plan.history_state() == (7 * count, 6 * count)
                result(f"pack/{key}/{fmt}", out)
    # the store really holds what was pushed
    with ZoomFFT(4096, 8, 2.4e6, n_win=512) as plan:
        plan.set_history(4, "u8", LO, HI)
        plan.history_push_device(rows.data_ptr(), 1, st)  # (a row of 8192 floats holds 16 rows of 512)
        back = torch.empty((1, 512), device=dev)
        plan.history_read_device(0, 1, back.data_ptr(), st)
        torch.cuda.synchronize()
        err = float((back - rows.reshape(-1)[:512].clamp(LO, HI)).abs().max())
        result("pack/round_trip_max_abs_error_u8", {"dB": err, "half_step": 0.5 * (HI - LO) / 254})
        assert err <= 0.513 * (HI - LO) / 254


def step_view():
    import torch
    from pypanadapter_amd import ZoomFFT
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(12)
    W, H, PX, M = 8192, 1080, 1920, 121
    count = H * M  # 130,680 rows
    rows = torch.empty((count, W), device=dev)
    for a in range(0, count, 8192):
        rows[a:a + 8192] = -160.0 + 120.0 * torch.rand((min(8192, count - a), W), device=dev, generator=g)
    img = torch.empty((H, PX), device=dev)
    with ZoomFFT(8192, 1, 2.4e6, n_win=W) as plan:
        plan.set_timing(True)
        plan.set_viewport(H, PX, 0, W, "max", M)
        base = timed(plan, lambda r: plan.viewport_push_device(rows.data_ptr(), count, st), ["view_lines", "view_finish"],
                     count * W * 4)
        want = torch.from_numpy(plan.viewport_image()).to(dev)
        plan.set_viewport(0, 0)
        result("view/baseline_viewport_push_f32_max", base)
        for fmt, eb in FORMATS.items():
            plan.set_history(count, fmt, LO, HI)
            plan.history_push_device(rows.data_ptr(), count, st)
            for det in ("max", "mean"):
                out = timed(plan, lambda r: plan.history_view_device(img.data_ptr(), 0, H, PX, M, det, stream=st),
                            ["history_view"], count * W * eb)
                if det == "max":
                    out["baseline_ms_over_this_ms"] = round(base["ms"] / out["ms"], 3)
                    if fmt == "f32":  # the same rows, unquantised: the live viewport's image
                        assert torch.equal(img, want)
                result(f"view/{fmt}/{det}", out)
        # the whole U8 store back into float rows (the last use of `rows`)
        out = timed(plan, lambda r: plan.history_read_device(0, count, rows.data_ptr(), st), ["history_unpack"],
                    count * W * (1 + 4))
        result("view/unpack_u8", out)


def main(out):
    from pypanadapter_amd import build
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"source_hash": build.source_hash(),
           "what": "ms by the plan's HIP-event timings, median of 5 calls after 2 warm ones; bytes = floats read + "
                   "codes written (pack), stored bytes read (view), codes read + floats written (unpack)",
           "times": {}}
    for step, expected in STEPS.items():
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True,
                               text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired as e:
            print((e.stdout or b"").decode(errors="replace") + (e.stderr or b"").decode(errors="replace"))
            sys.exit(f"{step}: no result within {STEP_LIMIT_S} s; stopping")
        lines = [ln.split(" ", 2) for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        for _, key, js in lines:
            res["times"][key] = json.loads(js)
            print(key, js, flush=True)
        json.dump(res, open(out, "w"), indent=1)
        if r.returncode != 0 or len(lines) != expected:
            print(r.stdout + r.stderr)
            sys.exit(f"{step} failed (exit {r.returncode}, {len(lines)} results); stopping")
    u8 = res["times"]["view/u8/max"]
    print(f"U8 MAX view {u8['ms']} ms, baseline {res['times']['view/baseline_viewport_push_f32_max']['ms']} ms: "
          f"ratio {u8['baseline_ms_over_this_ms']}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        {"pack": step_pack, "view": step_view}[sys.argv[2]]()
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "history", "history_times.json"))
