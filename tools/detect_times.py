#!/usr/bin/env python3
"""Same-box times of the row detector's kernel (zfft_detect_device, timing name "detect_rows"):
the plan's HIP-event timing, median of 5 calls after 2 warm ones, of
  cfg2_g1     69,632 rows of 512 (the lines of one cfg2 call at g = 1, 142.6 MB),
  one_row     one 512-wide row (the UI's use),
  wide        2,048 rows of 65,536 columns (536.9 MB),
with rows "uniform" (over [-135, -3]), "floor" (90 % of each row within 3 units of its floor,
the rest anywhere: the quiet band, where most of a row shares sign, exponent and top mantissa
bits), "quant" (the floor rows rounded to 0.5 units: hundreds of ties) and "all_on" (every column
on, threshold -1000: one run of 512 columns per row, the worst case of the run and occupancy
code); one_row and wide take the floor rows only.  Each from one buffer given again and again
("resident") and from three buffers in turn ("streamed").  Each time comes with the bytes the
call reads, their time at the streaming rate (6.3 TB/s, MI355X), and for cfg2_g1 "persist_hist"
(256 levels) on the same rows in the same run.  Library variants (name=path of a libzfft.so built
with another ZFFT_DETECT_SELECT) run after the shipped one, each in a child process of its own
under a time limit; the first failure ends the run.
usage: python tools/detect_times.py [OUT.json] [name=libpath ...]
       (default profiles/detect/detect_times.json)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_GBS = 6300.0
K = 8
# case: (n_fft, n_win, rows, kinds)
CASES = {"cfg2_g1": (512, 512, 69632, ("uniform", "floor", "quant", "all_on")),
         "one_row": (512, 512, 1, ("floor",)),
         "wide": (65536, 65536, 2048, ("floor",))}
N_RESULTS = 2 * sum(len(c[3]) for c in CASES.values())
STEP_LIMIT_S = 300


def make_rows(torch, dev, count, W, kind, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    wide = -135.0 + 132.0 * torch.rand((count, W), device=dev, generator=g)
    if kind == "uniform":
        return wide
    near = -121.5 + 3.0 * torch.rand((count, W), device=dev, generator=g)
    rows = torch.where(torch.rand((count, W), device=dev, generator=g) < 0.9, near, wide)
    if kind == "quant":
        rows = torch.round(rows * 2.0) / 2.0
    return rows.contiguous()


def one():
    import statistics

    import torch
    from pypanadapter_amd import ZoomFFT
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    for case, (N, W, count, kinds) in CASES.items():
        with ZoomFFT(N, 1, 2.4e6, n_win=W) as plan:
            plan.set_timing(True)
            floor = torch.empty(count, device=dev, dtype=torch.float32)
            found = torch.empty(count, device=dev, dtype=torch.int32)
            events = torch.empty((count, K, 4), device=dev, dtype=torch.int32)
            for kind in kinds:
                plan.set_detect(0.5, -1000.0 if kind == "all_on" else 12.0, 1, K)
                if case == "cfg2_g1":
                    plan.set_persistence(256, -130.0, -2.0)
                bufs = [make_rows(torch, dev, count, W, "floor" if kind == "all_on" else kind, 11 + k)
                        for k in range(3)]
                for mode, nbuf in (("resident", 1), ("streamed", 3)):
                    ms, ps = [], []
                    for r in range(7):
                        plan.detect_device(bufs[r % nbuf].data_ptr(), count, floor.data_ptr(), found.data_ptr(),
                                           events.data_ptr(), st)
                        torch.cuda.synchronize()
                        assert plan.launch_names() == ["detect_rows"]
                        ms.append(plan.timings()[0])
                        if case == "cfg2_g1":
                            plan.persistence_push_device(bufs[r % nbuf].data_ptr(), count, st)
                            torch.cuda.synchronize()
                            assert plan.launch_names() == ["persist_hist"]
                            ps.append(plan.timings()[0])
                    med = statistics.median(ms[2:])
                    nbytes = count * W * 4
                    out = {"ms": round(med, 5), "min_max": [round(min(ms[2:]), 5), round(max(ms[2:]), 5)],
                           "bytes": nbytes, "ms_at_streaming_rate": round(nbytes / STREAM_GBS / 1e6, 5),
                           "GBps": round(nbytes / med / 1e6, 1), "mean_found": round(float(found.float().mean()), 3)}
                    if ps:
                        out["persist_hist_ms"] = round(statistics.median(ps[2:]), 5)
                    print(f"RESULT {case}/{kind}/{mode} " + json.dumps(out), flush=True)
                occ, seen = plan.detect_occupancy()
                assert seen == 14 * count and (int(occ.sum()) > 0 or kind == "uniform")
                del bufs


def main(out, variants):
    from pypanadapter_amd import build
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"source_hash": build.source_hash(), "what": "detect_rows ms by the plan's timings, median of 5 calls after "
           "2 warm ones, with the smallest and largest of the five; bytes = rows x columns x 4 read, "
           "ms_at_streaming_rate = bytes at 6.3 TB/s; persist_hist_ms = the persistence push (256 levels) of the "
           "same rows in the same run; key library/case/rows/resident or streamed", "times": {}}
    for name, lib in [("shipped", "")] + variants:
        env = dict(os.environ)
        if lib:
            env["ZFFT_LIB_PATH"] = os.path.abspath(lib)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"], capture_output=True,
                               text=True, timeout=STEP_LIMIT_S, env=env)
        except subprocess.TimeoutExpired as e:
            print((e.stdout or b"").decode(errors="replace") + (e.stderr or b"").decode(errors="replace"))
            sys.exit(f"{name}: no result within {STEP_LIMIT_S} s; stopping")
        lines = [ln.split(" ", 2) for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        for _, key, js in lines:
            res["times"][f"{name}/{key}"] = json.loads(js)
            print(name, key, js, flush=True)
        json.dump(res, open(out, "w"), indent=1)
        if r.returncode != 0 or len(lines) != N_RESULTS:
            print(r.stdout + r.stderr)
            sys.exit(f"{name}: failed (exit {r.returncode}); stopping")


if __name__ == "__main__":
    if sys.argv[1:] == ["--one"]:
        one()
    else:
        args = sys.argv[1:]
        out = args.pop(0) if args and "=" not in args[0] else os.path.join(ROOT, "profiles", "detect", "detect_times.json")
        main(out, [tuple(a.split("=", 1)) for a in args])
