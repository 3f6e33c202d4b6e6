#!/usr/bin/env python3
"""Same-box times of the level bank's kernels (zfft_level_push_device, timing names "level_peaks",
"level_gains", "level_apply"): the plan's HIP-event timing, median of 5 calls after 2 warm ones, of
one push of
  - the (64, 8, 32) bank's AM audio at Da = 4 for cfg2's buffer (4096 x 299,008 complex64 as one
    stream): 9.57 M steps x 64 lanes at B = 64, H = 73 (the streams form, a wave a tile);
  - the (1024, 2, 512) bank's AM audio at Da = 4, 598 k steps x 1024 lanes, B = 64, H = 73;
  - one lane pair of the (64, 8, 32) bank's audio read in place at the array's stride of 64 (the
    time form);
each straight out of the device buffer the demodulator wrote, beside "fc_decim" at zoom 8
(zfft_process_device on a cfg2 plan) measured in the same run, whose bytes over its time are the
streaming rate this job measured.  Each time comes with the bytes the push moves (x read twice,
once for the peaks and once for the product, and written once) and the time those bytes need at
fc_decim's rate of this run and at 6.29 TB/s.  The first failure ends the run.
usage: python tools/level_times.py [OUT.json]   (default profiles/level/level_times.json)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM_GBS = 6290.0
FRAMES, L, FS = 4096, 299008, 2.4e6
DA, B, H = 4, 64, 73
NAMES = ["level_peaks", "level_gains", "level_apply"]


def med(ms):
    return {"ms": round(statistics.median(ms[2:]), 4), "min_max": [round(min(ms[2:]), 4), round(max(ms[2:]), 4)]}


def main(out):
    import torch
    from pypanadapter_amd import ZoomFFT, build
    from test_level_host import level_form
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    n = FRAMES * L
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    x = torch.empty((FRAMES, L, 2), device=dev, dtype=torch.float32)
    for f in range(0, FRAMES, 256):  # (in pieces: the generator's scratch stays small)
        x[f:f + 256].normal_(0.0, 0.5, generator=gen)
    res = {"source_hash": build.source_hash(), "samples": n, "what": "ms by the plan's timings, median of 5 calls after 2 "
           "warm ones, with the smallest and largest of the five, per launch and summed; bytes = x read twice + "
           "outputs once; ms_at_fc_decim_rate = bytes at the rate fc_decim moved its own bytes in this run; "
           "ms_at_streaming_rate = bytes at 6.29 TB/s", "times": {}}
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
        fc["gb_per_s"] = round(fc["bytes"] / fc["ms"] / 1e6, 1)
        fc["ms_at_streaming_rate"] = round(fc["bytes"] / STREAM_GBS / 1e6, 4)
        res["times"]["fc_decim_zoom8"] = fc
        print("fc_decim_zoom8", json.dumps(fc), flush=True)
        del rows

    def run(plan, case, ptr, steps, K, stride):
        """K lanes at ptr, rows `stride` floats apart, through the bank at (B, H), the key the samples."""
        plan.set_level(K, B, H, target=0.5, gmax=1e4, floor=1e-6, squelch=1e-3)
        outs = plan.level_steps(steps)
        r_out = torch.empty((outs * K,), device=dev, dtype=torch.float32)
        per = {k: [] for k in NAMES}
        total = []
        for _ in range(7):
            plan.level_reset(0)
            plan.level_push_device(ptr, steps, stride, r_out.data_ptr(), stream=st)
            torch.cuda.synchronize()
            assert plan.launch_names() == NAMES, plan.launch_names()
            t = plan.timings()
            for k, v in zip(NAMES, t):
                per[k].append(v)
            total.append(sum(t))
        r = med(total)
        r["launches"] = {k: med(v) for k, v in per.items()}
        f = level_form(plan.lib, K, B, H, 0, 0, steps)
        r.update({"form": "streams" if f["kind"] else "time", "launch_count": 3, "steps": steps, "lanes_in": K, "stride": stride,
                  "block": B, "hold": H, "outputs": outs,
                  "tiles": {k: f[k] for k in ("lanes", "rows", "chunk", "piece", "lds_bytes", "g_lanes", "g_blocks", "g_lds_bytes",
                                              "p_tiles", "g_tiles", "a_tiles", "p_grid", "g_grid", "a_grid")}})
        r["bytes"] = 2 * steps * K * 4 + outs * K * 4
        r["ms_at_fc_decim_rate"] = round(r["bytes"] / fc["gb_per_s"] / 1e6, 4)
        r["ms_at_streaming_rate"] = round(r["bytes"] / STREAM_GBS / 1e6, 4)
        r["times_its_bytes_at_fc_decim_rate"] = round(r["ms"] / r["ms_at_fc_decim_rate"], 3)
        r["steps_lanes_per_s"] = round(outs * K / r["ms"] * 1e3, -9)
        r["peak_out"] = round(float(r_out[:1000000].abs().max()), 6)
        env, gain = plan.level_meter()
        r["open_lanes"] = int((gain > 0).sum())
        res["times"][case] = r
        print(case, json.dumps(r), flush=True)
        plan.set_level(0)
        del r_out

    for name, (M, P, D) in (("bank(64,8,32)", (64, 8, 32)), ("bank(1024,2,512)", (1024, 2, 512))):
        with ZoomFFT(32, 1, FS) as plan:
            plan.set_timing(True)
            plan.set_channels(M, P, M // D)
            steps = plan.chan_steps(n)
            y = torch.empty((steps * M, 2), device=dev, dtype=torch.float32)
            plan.chan_push_device(x.data_ptr(), n, y.data_ptr(), st)
            plan.set_demod(M, decim=DA)
            plan.demod_mode("am")
            asteps = plan.demod_steps(steps)
            a = torch.empty((asteps * M,), device=dev, dtype=torch.float32)
            plan.demod_push_device(y.data_ptr(), steps, M, 1, a.data_ptr(), st)
            torch.cuda.synchronize()
            plan.set_demod(0)
            del y
            run(plan, f"{name}/am-audio/B{B}-H{H}", a.data_ptr(), asteps, M, M)
            if M == 64:
                # lanes 5 and 6 of the audio, read in place
                run(plan, f"{name}/lane-pair/B{B}-H{H}", a.data_ptr() + 4 * 5, asteps, 2, M)
            del a
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "level", "level_times.json"))
