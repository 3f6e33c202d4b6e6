#!/usr/bin/env python3
"""Same-box times of the channel taps' kernel (zfft_tap_push_device, timing name "tap_push"): the
plan's HIP-event timing, median of 5 calls after 2 warm ones, of one push of cfg2's buffer --
4096 x 299,008 complex64 as one stream of 1,224,736,768 samples (9.8 GB) -- through
  1, 4 and 16 taps at (decim, n_taps) = (64, 513), and 1 tap at (8, 65),
the taps at different frequencies, default designs.  Each time comes with two yardsticks measured
in the same run: "fc_decim" at zoom 8 on the same buffer (zfft_process_device on a cfg2 plan: the
nearest existing kernel by work), and the bytes the push moves (the input once, the outputs once)
at the 6.29 TB/s streaming rate of an MI355X; and with the complex multiply-adds per second.
The (64, 513) cases run a second time on the plain LDS array instead of the staging layout the
chooser picked (hook zfft__plan_tap_layout; "<case>/plain", "pad_shift" names the layout of each):
the measurement behind the layout chooser of DESIGN 3.3.9.
usage: python tools/tap_times.py [OUT.json]   (default profiles/tap/tap_times.json)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_GBS = 6290.0
FRAMES, L, FS = 4096, 299008, 2.4e6
CASES = {"1x(64,513)": (1, 64, 513), "4x(64,513)": (4, 64, 513), "16x(64,513)": (16, 64, 513), "1x(8,65)": (1, 8, 65)}


def med(ms):
    return {"ms": round(statistics.median(ms[2:]), 4), "min_max": [round(min(ms[2:]), 4), round(max(ms[2:]), 4)]}


def form_shift(plan, n, taps):
    """pad_shift of the chooser for a push of n samples through taps = [(fw, D, T, n_open)] (hook zfft__tap_form)."""
    import ctypes

    import numpy as np
    hook, P = plan.lib.zfft__tap_form, ctypes.c_void_p
    hook.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, P, P, P, P, P, P]
    hook.restype = ctypes.c_int
    cols = [np.array([t[i] for t in taps], dtype=dt) for i, dt in enumerate((np.int64, np.int32, np.int32, np.uint64))]
    form, items = np.zeros(8, np.int64), np.zeros((len(taps), 6), np.int64)
    assert hook(0, n, plan.tap_shape()[1], len(taps), *[c.ctypes.data_as(P) for c in cols], form.ctypes.data_as(P),
                items.ctypes.data_as(P)) == 0
    return int(form[7])


def main(out):
    import ctypes

    import torch
    from pypanadapter_amd import ZoomFFT, build, _lib
    layout = _lib.load().zfft__plan_tap_layout
    layout.argtypes, layout.restype = [ctypes.c_void_p, ctypes.c_int32], ctypes.c_int
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    n = FRAMES * L
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    x = torch.empty((FRAMES, L, 2), device=dev, dtype=torch.float32)
    for f in range(0, FRAMES, 256):  # (in pieces: the generator's scratch stays small)
        x[f:f + 256].normal_(0.0, 0.5, generator=g)
    res = {"source_hash": build.source_hash(), "samples": n, "what": "ms by the plan's timings, median of 5 calls after 2 "
           "warm ones, with the smallest and largest of the five; bytes = input once + outputs once; "
           "ms_at_streaming_rate = bytes at 6.29 TB/s; vs_fc_decim = ms / the fc_decim ms of this run", "times": {}}
    with ZoomFFT(4096, 8, FS) as plan:
        plan.set_timing(True)
        rows = torch.empty((FRAMES, plan.n_win), device=dev, dtype=torch.float32)
        ms = []
        for _ in range(7):
            plan.process_device(x.data_ptr(), L, FRAMES, rows.data_ptr(), st)
            torch.cuda.synchronize()
            names, t = plan.launch_names(), plan.timings()
            assert "fc_decim" in names, names
            ms.append(sum(v for k, v in zip(names, t) if k == "fc_decim"))
        fc = med(ms)
        fc["bytes"] = n * 8 + n // 8 * 8
        fc["ms_at_streaming_rate"] = round(fc["bytes"] / STREAM_GBS / 1e6, 4)
        res["times"]["fc_decim_zoom8"] = fc
        print("fc_decim_zoom8", json.dumps(fc), flush=True)
        del rows
    for case, (k, D, T) in CASES.items():
        with ZoomFFT(32, 1, FS) as plan:
            plan.set_timing(True)
            plan.set_taps(k, T)
            for s in range(k):
                plan.tap_open(s, (s - k / 2 + 0.37) * FS / (k + 1), D)
            total = int(plan.tap_counts(n).sum())
            y = torch.empty((total, 2), device=dev, dtype=torch.float32)
            chosen = form_shift(plan, n, [(plan.tap_info(s)["freq_word"], D, T, 0) for s in range(k)])

            def timed(shift):
                assert layout(plan._plan, shift) == 0
                ms = []
                for _ in range(7):
                    plan.tap_reset(0)
                    plan.tap_push_device(x.data_ptr(), n, y.data_ptr(), st)
                    torch.cuda.synchronize()
                    assert plan.launch_names() == ["tap_push"]
                    ms.append(plan.timings()[0])
                return med(ms)

            r = timed(0)
            if D == 64:  # the same push on the plain array (the outputs are the same: the layout is the staging's alone)
                ref = y[:200000].clone()
                p = timed(31)
                assert torch.equal(y[:200000], ref)
                p["pad_shift"], p["chosen_ms_over_this_ms"] = 31, round(r["ms"] / p["ms"], 4)
                res["times"][case + "/plain"] = p
                print(case + "/plain", json.dumps(p), flush=True)
            r["pad_shift"] = chosen
            r["bytes"] = n * 8 + total * 8
            r["ms_at_streaming_rate"] = round(r["bytes"] / STREAM_GBS / 1e6, 4)
            r["share_of_streaming_rate"] = round(r["ms_at_streaming_rate"] / r["ms"], 4)
            r["vs_fc_decim"] = round(r["ms"] / fc["ms"], 3)
            r["complex_mac_per_s"] = round(total * T / r["ms"] * 1e3, -9)
            r["rms_out"] = round(float(y[:100000].pow(2).sum(dim=1).mean().sqrt()), 6)
            res["times"][case] = r
            print(case, json.dumps(r), flush=True)
            del y
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tap", "tap_times.json"))
