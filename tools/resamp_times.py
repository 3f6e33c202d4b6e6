#!/usr/bin/env python3
"""Same-box times of the resampler bank's kernel (zfft_resamp_push_device, timing name
"resamp_push"): the plan's HIP-event timing, median of 5 calls after 2 warm ones, of one push of
  - the (64, 8, 32) bank's FM audio at Da = 4 for cfg2's buffer (4096 x 299,008 complex64 as one
    stream): 9.57 M steps x 64 lanes, resampled 64 / 25 (18.75 kHz to 48 kHz) to float32 and to
    int16 (the streams form, a wave a tile);
  - the (1024, 2, 512) bank's FM audio at Da = 4, 598 k steps x 1024 lanes, 64 / 25 to float32;
  - one channel of the (64, 8, 32) bank as a complex stream, 38.3 M steps x 2 lanes read in place out
    of the bank's output, 16 / 25 (75 kHz to 48 kHz IQ; the time form);
each straight out of the device buffer the producer wrote, beside "fc_decim" at zoom 8
(zfft_process_device on a cfg2 plan) measured in the same run on the same buffer, whose bytes over
its time are the streaming rate this job measured.  Each time comes with the bytes the push moves
(the input once, the outputs once) and the time those bytes need at fc_decim's rate of this run
and at 6.29 TB/s.  The first failure ends the run.
usage: python tools/resamp_times.py [OUT.json]   (default profiles/resamp/resamp_times.json)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_GBS = 6290.0
FRAMES, L, FS = 4096, 299008, 2.4e6
DA = 4


def med(ms):
    return {"ms": round(statistics.median(ms[2:]), 4), "min_max": [round(min(ms[2:]), 4), round(max(ms[2:]), 4)]}


def main(out):
    import ctypes

    import numpy as np
    import torch
    from pypanadapter_amd import ZoomFFT, build
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    n = FRAMES * L
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    x = torch.empty((FRAMES, L, 2), device=dev, dtype=torch.float32)
    for f in range(0, FRAMES, 256):  # (in pieces: the generator's scratch stays small)
        x[f:f + 256].normal_(0.0, 0.5, generator=gen)
    res = {"source_hash": build.source_hash(), "samples": n, "what": "ms by the plan's timings, median of 5 calls after 2 "
           "warm ones, with the smallest and largest of the five; bytes = input once + outputs once; "
           "ms_at_fc_decim_rate = bytes at the rate fc_decim moved its own bytes in this run; "
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

    def form_of(plan, steps, stride):
        K, Lr, Mr, T, fmt = plan.resamp_shape()
        hook = plan.lib.zfft__resamp_form
        hook.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p]
        hook.restype = ctypes.c_int
        form = np.zeros(13, np.int64)
        assert hook(K, Lr, Mr, T, stride, fmt, 0, steps, form.ctypes.data_as(ctypes.c_void_p)) == 0
        return {"form": "streams" if form[0] else "time", "lanes": int(form[1]), "span": int(form[2]),
                "lds_bytes": int(form[6]), "grid": int(form[12]), "taps_per_phase": T}

    def run(plan, case, ptr, steps, K, stride, Lr, Mr, fmt):
        """K lanes at ptr, rows `stride` floats apart, through the bank at Lr / Mr, the default design."""
        plan.set_resamp(K, Lr, Mr, format=fmt)
        outs = plan.resamp_steps(steps)
        size = 2 if fmt == "s16" else 4
        r_out = torch.empty((outs * K,), device=dev, dtype=torch.int16 if fmt == "s16" else torch.float32)
        ms = []
        for _ in range(7):
            plan.resamp_reset(0)
            plan.resamp_push_device(ptr, steps, stride, r_out.data_ptr(), st)
            torch.cuda.synchronize()
            assert plan.launch_names() == ["resamp_push"]
            ms.append(plan.timings()[0])
        r = med(ms)
        r.update(form_of(plan, steps, stride))
        r["steps"], r["lanes_in"], r["L"], r["M"], r["format"], r["outputs"] = steps, K, Lr, Mr, fmt, outs
        r["bytes"] = steps * K * 4 + outs * K * size
        r["ms_at_fc_decim_rate"] = round(r["bytes"] / fc["gb_per_s"] / 1e6, 4)
        r["ms_at_streaming_rate"] = round(r["bytes"] / STREAM_GBS / 1e6, 4)
        r["times_its_bytes_at_fc_decim_rate"] = round(r["ms"] / r["ms_at_fc_decim_rate"], 3)
        r["outputs_per_s"] = round(outs * K / r["ms"] * 1e3, -9)
        r["rms_out"] = round(float(r_out[:100000].float().pow(2).mean().sqrt()), 6)
        res["times"][case] = r
        print(case, json.dumps(r), flush=True)
        plan.set_resamp(0)
        del r_out

    for name, (M, P, D) in (("bank(64,8,32)", (64, 8, 32)), ("bank(1024,2,512)", (1024, 2, 512))):
        with ZoomFFT(32, 1, FS) as plan:
            plan.set_timing(True)
            plan.set_channels(M, P, M // D)
            steps = plan.chan_steps(n)
            y = torch.empty((steps * M, 2), device=dev, dtype=torch.float32)
            plan.chan_push_device(x.data_ptr(), n, y.data_ptr(), st)
            plan.set_demod(M, decim=DA)
            plan.demod_mode("fm")
            asteps = plan.demod_steps(steps)
            a = torch.empty((asteps * M,), device=dev, dtype=torch.float32)
            plan.demod_push_device(y.data_ptr(), steps, M, 1, a.data_ptr(), st)
            torch.cuda.synchronize()
            plan.set_demod(0)
            run(plan, f"{name}/fm-audio/64:25/f32", a.data_ptr(), asteps, M, M, 64, 25, "f32")
            if M == 64:
                run(plan, f"{name}/fm-audio/64:25/s16", a.data_ptr(), asteps, M, M, 64, 25, "s16")
                # channel 5 as a complex stream: two lanes of the bank's rows, read in place
                run(plan, f"{name}/channel-iq/16:25/f32", y.data_ptr() + 8 * 5, steps, 2, 2 * M, 16, 25, "f32")
            del y, a
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resamp", "resamp_times.json"))
