#!/usr/bin/env python3
"""Same-box times of the channeliser's kernel (zfft_chan_push_device, timing name "chan_push"): the
plan's HIP-event timing, median of 5 calls after 2 warm ones, of one push of cfg2's buffer --
4096 x 299,008 complex64 as one stream of 1,224,736,768 samples (9.8 GB) -- through the bank at
  (M, P, D) = (64, 8, 32), (1024, 2, 512) and (8, 8, 4), all channels kept, default prototypes,
beside two yardsticks measured in the same run on the same buffer: "fc_decim" at zoom 8
(zfft_process_device on a cfg2 plan), whose bytes over its time are the streaming rate this job
measured, and sixteen channel taps at (decim, n_taps) = (32, 512) on channel centres of the
64-channel bank -- what a user had before the bank.  Each bank time comes with the bytes the push
moves (the input once, the outputs once), the time those bytes need at fc_decim's rate of this
run and at 6.29 TB/s, and the real-by-complex multiply-adds per second of its FIR.  The (64, 8, 32)
bank runs once more keeping one channel of the 64 ("<case>/1_channel_kept"): the same staging, FIR
and transform with 1/64 of the stores.

With --ab PARENT_TREE: the off-cost A/B instead -- a built checkout of the parent commit at
PARENT_TREE and this tree alternating in one job, five pairs, parent first, each bench.py --gpus 1
--steps 100 --warmup 5 --no-cpu (cfg2) in a child process under a time limit; ms/step, written to
profiles/chan/bench_ab.json.  The first failure ends the run.
usage: python tools/chan_times.py [OUT.json]   (default profiles/chan/chan_times.json)
       python tools/chan_times.py --ab PARENT_TREE [OUT.json]"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_GBS = 6290.0
FRAMES, L, FS = 4096, 299008, 2.4e6
BANKS = {"bank(64,8,32)": (64, 8, 32), "bank(1024,2,512)": (1024, 2, 512), "bank(8,8,4)": (8, 8, 4)}
TAPS = (16, 32, 512)
STEP_LIMIT_S = 240


def med(ms):
    return {"ms": round(statistics.median(ms[2:]), 4), "min_max": [round(min(ms[2:]), 4), round(max(ms[2:]), 4)]}


def main(out):
    import ctypes

    import numpy as np
    import torch
    from pypanadapter_amd import ZoomFFT, build, chan_design
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
           "ms_at_fc_decim_rate = bytes at the rate fc_decim moved its own bytes in this run; "
           "ms_at_streaming_rate = bytes at 6.29 TB/s; vs_16_taps = ms / the sixteen taps' ms of this run", "times": {}}
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
    k, D, T = TAPS
    with ZoomFFT(32, 1, FS) as plan:
        plan.set_timing(True)
        plan.set_taps(k, T)
        h = chan_design(64, 8).astype(np.float32)
        for s in range(k):
            plan.tap_open(s, (s - k // 2) * FS / 64, D, taps=h)  # sixteen neighbouring channels of the 64-channel bank
        total = int(plan.tap_counts(n).sum())
        y = torch.empty((total, 2), device=dev, dtype=torch.float32)
        ms = []
        for _ in range(7):
            plan.tap_reset(0)
            plan.tap_push_device(x.data_ptr(), n, y.data_ptr(), st)
            torch.cuda.synchronize()
            assert plan.launch_names() == ["tap_push"]
            ms.append(plan.timings()[0])
        taps = med(ms)
        taps["bytes"] = n * 8 + total * 8
        taps["complex_mac_per_s"] = round(total * T / taps["ms"] * 1e3, -9)
        res["times"]["16x(32,512)_taps"] = taps
        print("16x(32,512)_taps", json.dumps(taps), flush=True)
        tap_head = y.reshape(k, -1, 2)[:, :64].clone()  # (the taps' outputs lie back to back in slot order)
        del y
    for case, (M, P, D) in BANKS.items():
        with ZoomFFT(32, 1, FS) as plan:
            plan.set_timing(True)
            plan.set_channels(M, P, M // D)
            steps = plan.chan_steps(n)
            y = torch.empty((steps * M, 2), device=dev, dtype=torch.float32)
            hook = plan.lib.zfft__chan_form
            hook.argtypes = [ctypes.c_uint64, ctypes.c_int64] + [ctypes.c_int32] * 4 + [ctypes.c_void_p]
            hook.restype = ctypes.c_int
            form = np.zeros(13, np.int64)
            assert hook(0, n, M, P, D, M, form.ctypes.data_as(ctypes.c_void_p)) == 0
            ms = []
            for _ in range(7):
                plan.chan_reset(0)
                plan.chan_push_device(x.data_ptr(), n, y.data_ptr(), st)
                torch.cuda.synchronize()
                assert plan.launch_names() == ["chan_push"]
                ms.append(plan.timings()[0])
            r = med(ms)
            r["span"], r["points"], r["lds_bytes"], r["grid"] = int(form[0]), int(form[2]), int(form[7]), int(form[8])
            r["bytes"] = n * 8 + steps * M * 8
            r["ms_at_fc_decim_rate"] = round(r["bytes"] / fc["gb_per_s"] / 1e6, 4)
            r["ms_at_streaming_rate"] = round(r["bytes"] / STREAM_GBS / 1e6, 4)
            r["share_of_fc_decim_rate"] = round(r["ms_at_fc_decim_rate"] / r["ms"], 4)
            r["share_of_streaming_rate"] = round(r["ms_at_streaming_rate"] / r["ms"], 4)
            r["vs_16_taps"] = round(r["ms"] / taps["ms"], 4)
            r["real_complex_mac_per_s"] = round(steps * M * P / r["ms"] * 1e3, -9)
            r["rms_out"] = round(float(y[:100000].pow(2).sum(dim=1).mean().sqrt()), 6)
            if M == 64:  # the same numbers as the taps gave, channel by channel: tap s is channel s - 8 mod 64
                got = y[:64 * M].reshape(64, M, 2)
                worst = max(float((got[:, (s - k // 2) % M] - tap_head[s]).abs().max()) for s in range(k))
                r["max_abs_difference_from_the_taps"] = worst
                assert worst < 1e-3, worst  # (outputs of about 0.1: a wrong channel would differ by that)
            res["times"][case] = r
            print(case, json.dumps(r), flush=True)
            if M == 64:  # the same push keeping one channel: everything but the stores (what bounds the bank)
                plan.chan_select(0, 1)
                ms = []
                for _ in range(7):
                    plan.chan_reset(0)
                    plan.chan_push_device(x.data_ptr(), n, y.data_ptr(), st)
                    torch.cuda.synchronize()
                    ms.append(plan.timings()[0])
                one = med(ms)
                one["bytes"] = n * 8 + steps * 8
                one["ms_at_fc_decim_rate"] = round(one["bytes"] / fc["gb_per_s"] / 1e6, 4)
                res["times"][case + "/1_channel_kept"] = one
                print(case + "/1_channel_kept", json.dumps(one), flush=True)
            del y
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


def ab(parent_tree, out):
    parent_tree = os.path.abspath(parent_tree)
    assert os.path.exists(os.path.join(parent_tree, "pypanadapter_amd", "lib", "libzfft.so")), parent_tree
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"what": "bench.py --gpus 1 --steps 100 --warmup 5 --no-cpu at cfg2 with the channeliser off (bench.py never "
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
    res["parent_min_max"] = [min(p), max(p)]
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res["median"]))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--ab":
        ab(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "chan", "bench_ab.json"))
        sys.exit(0)
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chan", "chan_times.json"))
