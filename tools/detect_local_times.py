#!/usr/bin/env python3
"""Same-box times of the row detector's local floor (zfft_plan_detect_local; timing names
"detect_floor" and "detect_rows"): the plan's HIP-event timings, median of 5 calls after 2 warm
ones, of
  cfg2_g1     69,632 rows of 512 (the lines of one cfg2 call at g = 1, 142.6 MB), rows "floor"
              (90 % of each row within 3 units of its floor: the quiet band) and "uniform",
  one_row     one 512-wide row (the UI's use),
  one_wide    one 8,192-wide row,
  wide        2,048 rows of 65,536 columns (536.9 MB, two passes through the 256 MiB scratch),
each at (half_window, guard) = (16, 2), (64, 4), (128, 8), from three buffers in turn.  Beside
each: the row-global detector ("global_detect_rows_ms") on the same rows in the same run, the
floor kernel alone through zfft_detect_floors_device ("floors_only_ms"), the bytes a call moves
(rows read once by each kernel, floors written and read once), their time at the streaming rate
(6.3 TB/s, MI355X), the rule's arithmetic as a key sweep would do it ("compares_per_column": 34
sweeps of 2 half_window cells) and what the bit-sliced kernel does instead
("mask_words_per_column": 33 steps of 2 x 1, 2 or 4 mask words).

With --ab PARENT_TREE: the off-cost A/B instead -- a built checkout of the parent commit at
PARENT_TREE and this tree alternating in one job, five pairs, each in a child process under a
time limit: bench.py at cfg2 (ms/step) and detect_rows in global mode on the 69,632 x 512 floor
rows (ms); written to profiles/detect_local/bench_ab.json.  (Whole trees, not ZFFT_LIB_PATH: this
tree's binding asks the library for the new exports, which the parent's does not have.)  The
first failure ends the run.
usage: python tools/detect_local_times.py [OUT.json]
       python tools/detect_local_times.py --ab PARENT_TREE [OUT.json]"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("ZFFT_AB_TREE") or HERE  # (--global-rows under --ab: the tree whose package runs)
sys.path.insert(0, ROOT)
from tools.detect_times import make_rows  # noqa: E402  (the same rows as profiles/detect)

STREAM_GBS = 6300.0
K = 8
SHAPES = ((16, 2), (64, 4), (128, 8))
# case: (n_fft, n_win, rows, kinds)
CASES = {"cfg2_g1": (512, 512, 69632, ("floor", "uniform")),
         "one_row": (512, 512, 1, ("floor",)),
         "one_wide": (8192, 8192, 1, ("floor",)),
         "wide": (65536, 65536, 2048, ("floor",))}
N_RESULTS = len(SHAPES) * sum(len(c[3]) for c in CASES.values())
STEP_LIMIT_S = 400
OUT_DIR = os.path.join(HERE, "profiles", "detect_local")


def _median(xs):
    return round(statistics.median(xs[2:]), 5)


def one():
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
            floors = torch.empty((count, W), device=dev, dtype=torch.float32)
            for kind in kinds:
                bufs = [make_rows(torch, dev, count, W, kind, 11 + k) for k in range(3)]

                def detect(r):
                    plan.detect_device(bufs[r % 3].data_ptr(), count, floor.data_ptr(), found.data_ptr(),
                                       events.data_ptr(), st)
                    torch.cuda.synchronize()
                    return plan.launch_names(), plan.timings()

                def floors_only(r):
                    plan.detect_floors_device(bufs[r % 3].data_ptr(), count, floors.data_ptr(), st)
                    torch.cuda.synchronize()
                    assert plan.launch_names() == ["detect_floor"]
                    return plan.timings()[0]

                plan.set_detect(0.5, 12.0, 1, K)
                gl = []
                for r in range(7):
                    names, ms = detect(r)
                    assert names == ["detect_rows"]
                    gl.append(ms[0])
                gfound = float(found.float().mean())
                for h, gd in SHAPES:
                    plan.set_detect_local(h, gd)
                    fl, rw = [], []
                    for r in range(7):
                        names, ms = detect(r)
                        assert names[:2] == ["detect_floor", "detect_rows"] and len(names) % 2 == 0
                        fl.append(sum(ms[0::2]))
                        rw.append(sum(ms[1::2]))
                    lfound = float(found.float().mean())
                    only = [floors_only(r) for r in range(7)]
                    cells = count * W
                    nbytes = cells * 4 * 4  # rows read by both kernels, floors written and read
                    out = {"detect_floor_ms": _median(fl), "detect_rows_ms": _median(rw),
                           "passes": len(names) // 2, "floors_only_ms": _median(only),
                           "global_detect_rows_ms": _median(gl),
                           "bytes": nbytes, "ms_at_streaming_rate": round(nbytes / STREAM_GBS / 1e6, 5),
                           "compares_per_column": 34 * 2 * h,
                           "mask_words_per_column": 33 * 2 * (1 if h <= 32 else 2 if h <= 64 else 4),
                           "G_columns_per_s_floor_kernel": round(cells / _median(only) / 1e6, 2),
                           "mean_found": round(lfound, 3), "global_mean_found": round(gfound, 3)}
                    print(f"RESULT {case}/{kind}/h{h}g{gd} " + json.dumps(out), flush=True)
                plan.set_detect_local(0)
                del bufs


def global_rows_ms():
    """detect_rows in global mode on the 69,632 x 512 floor rows: one RESULT line."""
    import torch
    from pypanadapter_amd import ZoomFFT
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    N, W, count, _ = CASES["cfg2_g1"]
    with ZoomFFT(N, 1, 2.4e6, n_win=W) as plan:
        plan.set_timing(True)
        plan.set_detect(0.5, 12.0, 1, K)
        floor = torch.empty(count, device=dev, dtype=torch.float32)
        found = torch.empty(count, device=dev, dtype=torch.int32)
        events = torch.empty((count, K, 4), device=dev, dtype=torch.int32)
        bufs = [make_rows(torch, dev, count, W, "floor", 11 + k) for k in range(3)]
        ms = []
        for r in range(7):
            plan.detect_device(bufs[r % 3].data_ptr(), count, floor.data_ptr(), found.data_ptr(), events.data_ptr(), st)
            torch.cuda.synchronize()
            assert plan.launch_names() == ["detect_rows"]
            ms.append(plan.timings()[0])
        print("RESULT " + json.dumps({"ms": _median(ms)}), flush=True)


def _child(cmd, env, what, cwd=HERE):
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S, env=env, cwd=cwd)
    except subprocess.TimeoutExpired as e:
        print((e.stdout or b"").decode(errors="replace") + (e.stderr or b"").decode(errors="replace"))
        sys.exit(f"{what}: no result within {STEP_LIMIT_S} s; stopping")
    if r.returncode != 0:
        print(r.stdout + r.stderr)
        sys.exit(f"{what}: failed (exit {r.returncode}); stopping")
    return r.stdout


def ab(parent_tree, out):
    parent_tree = os.path.abspath(parent_tree)
    assert os.path.exists(os.path.join(parent_tree, "pypanadapter_amd", "lib", "libzfft.so")), parent_tree
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"what": "the local floor off: the parent's tree and this tree alternating in one job on one MI355X, "
           "parent first in each of five pairs; bench = bench.py --gpus 1 --steps 100 --warmup 5 "
           "--no-cpu at cfg2, ms/step; detect_rows = the row-global detector's kernel on 69,632 x 512 floor rows, "
           "ms by the plan's timings, median of 5 calls after 2 warm ones",
           "bench_ms_per_step": {"parent": [], "this": []}, "detect_rows_ms": {"parent": [], "this": []}}
    for pair in range(5):
        for name in ("parent", "this"):
            tree = parent_tree if name == "parent" else HERE
            env = dict(os.environ)
            env.pop("ZFFT_LIB_PATH", None)
            env["ZFFT_AB_TREE"] = tree
            text = _child([sys.executable, "bench.py", "--gpus", "1", "--steps", "100", "--warmup", "5", "--no-cpu"],
                          env, f"bench {name} {pair}", cwd=tree)
            line = [ln for ln in text.splitlines() if ln.startswith("{")][-1]
            res["bench_ms_per_step"][name].append(json.loads(line)["ms_per_step"])
            text = _child([sys.executable, os.path.abspath(__file__), "--global-rows"], env, f"detect_rows {name} {pair}",
                          cwd=tree)
            line = [ln for ln in text.splitlines() if ln.startswith("RESULT ")][-1]
            res["detect_rows_ms"][name].append(json.loads(line.split(" ", 1)[1])["ms"])
            print(pair, name, res["bench_ms_per_step"][name][-1], res["detect_rows_ms"][name][-1], flush=True)
            json.dump(res, open(out, "w"), indent=1)
    for key in ("bench_ms_per_step", "detect_rows_ms"):
        p, t = res[key]["parent"], res[key]["this"]
        res[key]["median"] = {"parent": statistics.median(p), "this": statistics.median(t)}
        res[key]["parent_min_max"] = [min(p), max(p)]
        res[key]["this_within_parent_spread"] = bool(min(p) <= statistics.median(t) <= max(p))
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: res[k]["median"] for k in ("bench_ms_per_step", "detect_rows_ms")}))


def main(out):
    from pypanadapter_amd import build
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = {"source_hash": build.source_hash(), "what": __doc__.split("\n\nWith --ab")[0], "times": {}}
    text = _child([sys.executable, os.path.abspath(__file__), "--one"], dict(os.environ), "times")
    for ln in text.splitlines():
        if ln.startswith("RESULT "):
            _, key, js = ln.split(" ", 2)
            res["times"][key] = json.loads(js)
            print(key, js, flush=True)
    json.dump(res, open(out, "w"), indent=1)
    if len(res["times"]) != N_RESULTS:
        sys.exit(f"{len(res['times'])} of {N_RESULTS} results; stopping")


if __name__ == "__main__":
    args = sys.argv[1:]
    if args == ["--one"]:
        one()
    elif args == ["--global-rows"]:
        global_rows_ms()
    elif args and args[0] == "--ab":
        ab(args[1], args[2] if len(args) > 2 else os.path.join(OUT_DIR, "bench_ab.json"))
    else:
        main(args[0] if args else os.path.join(OUT_DIR, "detect_local_times.json"))
