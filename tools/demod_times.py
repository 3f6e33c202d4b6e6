#!/usr/bin/env python3
"""Same-box times of the demodulator bank's kernel (zfft_demod_push_device, timing name
"demod_push"): the plan's HIP-event timing, median of 5 calls after 2 warm ones, of one push of
  - the (64, 8, 32) bank's output for cfg2's buffer (4096 x 299,008 complex64 as one stream of
    1,224,736,768 samples): 38.3 M steps x 64 streams, 19.6 GB in, through the bank at Da = 4,
    Ta = 33 (the default design) in each of the four modes (the streams form);
  - the (1024, 2, 512) bank's output for the same buffer, 2.39 M steps x 1024 streams, in FM;
  - one (8, 65) tap's stream of the same buffer, 153 M steps, in FM (the time form);
each straight out of the device buffer the producer wrote, beside "fc_decim" at zoom 8
(zfft_process_device on a cfg2 plan) measured in the same run on the same buffer, whose bytes over
its time are the streaming rate this job measured.  Each time comes with the bytes the push moves
(the input once, the outputs once) and the time those bytes need at fc_decim's rate of this run
and at 6.29 TB/s.

With --ab PARENT_TREE: the off-cost A/B instead -- a built checkout of the parent commit at
PARENT_TREE and this tree alternating in one job, five pairs, parent first, each bench.py --gpus 1
--steps 100 --warmup 5 --no-cpu (cfg2) in a child process under a time limit; ms/step, written to
profiles/demod/bench_ab.json.  The first failure ends the run.
usage: python tools/demod_times.py [OUT.json]   (default profiles/demod/demod_times.json)
       python tools/demod_times.py --ab PARENT_TREE [OUT.json]"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_GBS = 6290.0
FRAMES, L, FS = 4096, 299008, 2.4e6
DA = 4
STEP_LIMIT_S = 240


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

    def form_of(plan, K, Ta, ss, ts, steps):
        hook = plan.lib.zfft__demod_form
        hook.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_int64] * 2 + [ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p]
        hook.restype = ctypes.c_int
        form = np.zeros(12, np.int64)
        assert hook(K, Ta, DA, ss, ts, 0, steps, form.ctypes.data_as(ctypes.c_void_p)) == 0
        return {"form": "streams" if form[0] else "time", "lanes": int(form[1]), "span": int(form[3]),
                "lds_bytes": int(form[5]), "grid": int(form[11])}

    def run(plan, case, y, steps, K, ss, ts, modes):
        """The bank at Da = 4 on the K streams at y, once per mode."""
        plan.set_demod(K, decim=DA)
        Ta = plan.demod_shape()[1]
        outs = plan.demod_steps(steps)
        a = torch.empty((outs * K,), device=dev, dtype=torch.float32)
        for mode in modes:
            plan.demod_mode(mode, bfo_hz=1500.0, rate=FS / 32)
            ms = []
            for _ in range(7):
                plan.demod_reset(0)
                plan.demod_push_device(y.data_ptr(), steps, ss, ts, a.data_ptr(), st)
                torch.cuda.synchronize()
                assert plan.launch_names() == ["demod_push"]
                ms.append(plan.timings()[0])
            r = med(ms)
            r.update(form_of(plan, K, Ta, ss, ts, steps))
            r["steps"], r["streams"], r["n_taps"], r["decim"] = steps, K, Ta, DA
            r["bytes"] = steps * K * 8 + outs * K * 4
            r["ms_at_fc_decim_rate"] = round(r["bytes"] / fc["gb_per_s"] / 1e6, 4)
            r["ms_at_streaming_rate"] = round(r["bytes"] / STREAM_GBS / 1e6, 4)
            r["times_its_bytes_at_fc_decim_rate"] = round(r["ms"] / r["ms_at_fc_decim_rate"], 3)
            r["detected_per_s"] = round(steps * K / r["ms"] * 1e3, -9)
            r["rms_out"] = round(float(a[:100000].pow(2).mean().sqrt()), 6)
            res["times"][f"{case}/{mode}"] = r
            print(f"{case}/{mode}", json.dumps(r), flush=True)
        plan.set_demod(0)
        del a

    for case, (M, P, D), modes in (("bank(64,8,32)", (64, 8, 32), ("am", "fm", "ssb", "power")),
                                   ("bank(1024,2,512)", (1024, 2, 512), ("fm",))):
        with ZoomFFT(32, 1, FS) as plan:
            plan.set_timing(True)
            plan.set_channels(M, P, M // D)
            steps = plan.chan_steps(n)
            y = torch.empty((steps * M, 2), device=dev, dtype=torch.float32)
            plan.chan_push_device(x.data_ptr(), n, y.data_ptr(), st)
            torch.cuda.synchronize()
            run(plan, case, y, steps, M, M, 1, modes)
            del y
    with ZoomFFT(32, 1, FS) as plan:
        plan.set_timing(True)
        plan.set_taps(1, 65)
        plan.tap_open(0, 100e3, 8)
        steps = int(plan.tap_counts(n)[0])
        y = torch.empty((steps, 2), device=dev, dtype=torch.float32)
        plan.tap_push_device(x.data_ptr(), n, y.data_ptr(), st)
        torch.cuda.synchronize()
        run(plan, "tap(8,65)", y, steps, 1, 1, 0, ("fm",))
        del y
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


def ab(parent_tree, out):
    parent_tree = os.path.abspath(parent_tree)
    assert os.path.exists(os.path.join(parent_tree, "pypanadapter_amd", "lib", "libzfft.so")), parent_tree
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"what": "bench.py --gpus 1 --steps 100 --warmup 5 --no-cpu at cfg2 with the demodulator off (bench.py never "
           "enables it), ms/step, the parent's tree and this tree alternating in one job on one MI355X, parent first "
           "in each of the five pairs", "bench_ms_per_step": {"parent": [], "this": []}}
    for pair in range(5):
        for name in ("parent", "this"):
            tree = parent_tree if name == "parent" else ROOT
            env = dict(os.environ)
            env.pop("ZFFT_LIB_PATH", None)
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "100", "--warmup", "5", "--no-cpu"]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S, env=env, cwd=tree)
            except subprocess.TimeoutExpired:
                sys.exit(f"bench {name} {pair}: no result within {STEP_LIMIT_S} s; stopping")
            if r.returncode != 0:
                print(r.stdout + r.stderr)
                sys.exit(f"bench {name} {pair}: failed (exit {r.returncode}); stopping")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            res["bench_ms_per_step"][name].append(json.loads(line)["ms_per_step"])
            print(pair, name, res["bench_ms_per_step"][name][-1], flush=True)
            json.dump(res, open(out, "w"), indent=1)
    p, t = res["bench_ms_per_step"]["parent"], res["bench_ms_per_step"]["this"]
    res["median"] = {"parent": statistics.median(p), "this": statistics.median(t)}
    res["this_minus_parent_per_pair"] = [round(b - a, 4) for a, b in zip(p, t)]
    res["signs"] = {"this_slower": sum(b > a for a, b in zip(p, t)), "this_faster": sum(b < a for a, b in zip(p, t))}
    res["parent_min_max"] = [min(p), max(p)]
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["median"]))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--ab":
        ab(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "demod", "bench_ab.json"))
        sys.exit(0)
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "demod", "demod_times.json"))
