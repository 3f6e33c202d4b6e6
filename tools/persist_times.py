#!/usr/bin/env python3
"""Same-box times of the persistence spectrum's kernel (zfft_persistence_push_device, timing name
"persist_hist"): the plan's HIP-event timing, median of 5 pushes after 2 warm ones, of
  cfg2_g1     69,632 rows of 512 (the lines of one cfg2 call at g = 1) at 256 levels,
  one_row     one 512-wide row (the UI's use),
each with rows uniform over the range and with "floor" rows (90 % of a column's values in three
adjacent levels, the noise-floor case), from one buffer pushed again and again ("resident": its
143 MB stay in the Infinity Cache, as rows a Welch kernel has just written may) and from three
buffers in turn ("streamed": 428 MB, each push reads from HBM).  Each time comes with the bytes
the push reads and their share of the streaming rate (6.3 TB/s, MI355X).  Library variants
(name=path of a libzfft.so built with another ZFFT_PERSIST_WAVES) run after the shipped one, each
in a child process of its own under a time limit; the first failure ends the run.
usage: python tools/persist_times.py [OUT.json] [name=libpath ...]
       (default profiles/persist/persist_times.json)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_GBS = 6300.0
LEVELS, LO, HI, W = 256, -130.0, -2.0, 512
CASES = {"cfg2_g1": 69632, "one_row": 1}
STEP_LIMIT_S = 120


def make_rows(torch, dev, count, kind, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    wide = LO - 5.0 + (HI - LO + 10.0) * torch.rand((count, W), device=dev, generator=g)
    if kind == "uniform":
        return wide
    centre = torch.randint(1, LEVELS - 1, (W,), device=dev, generator=g).float()
    step = (HI - LO) / LEVELS
    near = LO + (centre[None, :] - 1.0 + 3.0 * torch.rand((count, W), device=dev, generator=g)) * step
    return torch.where(torch.rand((count, W), device=dev, generator=g) < 0.9, near, wide)


def one():
    import statistics

    import torch
    from pypanadapter_amd import ZoomFFT
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    with ZoomFFT(4096, 8, 2.4e6, n_win=W) as plan:
        plan.set_timing(True)
        plan.set_persistence(LEVELS, LO, HI)
        for case, count in CASES.items():
            for kind in ("uniform", "floor"):
                bufs = [make_rows(torch, dev, count, kind, 11 + k) for k in range(3)]
                for mode, nbuf in (("resident", 1), ("streamed", 3)):
                    ms = []
                    for r in range(7):
                        plan.persistence_push_device(bufs[r % nbuf].data_ptr(), count, st)
                        torch.cuda.synchronize()
                        assert plan.launch_names() == ["persist_hist"]
                        ms.append(plan.timings()[0])
                    med = statistics.median(ms[2:])
                    nbytes = count * W * 4
                    out = {"ms": round(med, 5), "min_max": [round(min(ms[2:]), 5), round(max(ms[2:]), 5)],
                           "bytes": nbytes, "GBps": round(nbytes / med / 1e6, 1),
                           "share_of_streaming_rate": round(nbytes / med / 1e6 / STREAM_GBS, 4)}
                    print(f"RESULT {case}/{kind}/{mode} " + json.dumps(out), flush=True)
                hist, seen = plan.persistence()
                assert seen == 14 * count and int(hist.sum()) > 0
                plan.persistence_reset()
                del bufs


def main(out, variants):
    from pypanadapter_amd import build
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"source_hash": build.source_hash(), "what": "persist_hist ms by the plan's timings, median of 5 pushes "
           "after 2 warm ones, with the smallest and largest of the five; bytes = count x 512 x 4 read; key "
           "library/case/rows/resident or streamed", "times": {}}
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
        if r.returncode != 0 or len(lines) != 8:
            print(r.stdout + r.stderr)
            sys.exit(f"{name}: failed (exit {r.returncode}); stopping")


if __name__ == "__main__":
    if sys.argv[1:] == ["--one"]:
        one()
    else:
        args = sys.argv[1:]
        out = args.pop(0) if args and "=" not in args[0] else os.path.join(ROOT, "profiles", "persist", "persist_times.json")
        main(out, [tuple(a.split("=", 1)) for a in args])
