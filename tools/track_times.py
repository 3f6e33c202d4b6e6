#!/usr/bin/env python3
"""Same-box times of the emission tracker (zfft_plan_track; timing names "track_*"): the plan's
HIP-event timings per launch, median of 5 pushes after 2 warm ones, from three record buffers in
turn (each what zfft_detect_device wrote for its own rows; the tracks of a push are read before
the next, untimed), of
  cfg2_g1     69,632 rows of 512 columns at K = 8 (the lines of one cfg2 call at g = 1), gap 0,
              with the record sets "sparse" (noise and a three-column run in 3 % of the rows),
              "carriers" (8 long-lived carriers in every row: nothing closes) and "blips" (8 fresh
              one-row runs in every row: every run opens and closes a track, 557,056 a push),
  wide        2,048 rows of 65,536 columns at K = 32, 32 carriers, gap 0,
  one_row     one 512-wide row per call at K = 8 and gap 7, 8 carriers (200 calls; also the host
              time per call, enqueue to completion).
Beside each, in the same run: "detect_rows_ms", the detector's kernel on the rows that produced
the records, and "copy_ms", the call's found and events copied to page-locked host memory -- the
least any host-side tracker pays before it links anything.

With --ab PARENT_TREE: the off-cost A/B instead -- a built checkout of the parent commit at
PARENT_TREE and this tree alternating in one job, five pairs, each in a child process under a
time limit: bench.py at cfg2 (ms/step) and detect_rows in global mode on the 69,632 x 512 floor
rows (ms); written to profiles/track/bench_ab.json.  The first failure ends the run.
usage: python tools/track_times.py [OUT.json]
       python tools/track_times.py --ab PARENT_TREE [OUT.json]"""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("ZFFT_AB_TREE") or HERE  # (--global-rows under --ab: the tree whose package runs)
sys.path.insert(0, ROOT)

STEP_LIMIT_S = 400
OUT_DIR = os.path.join(HERE, "profiles", "track")
N_RESULTS = 5


def _median(xs):
    return round(statistics.median(xs[2:]), 5)


def scene_rows(torch, dev, count, W, kind, seed, n_car=8):
    """Noise around -120 (sigma 1.5: floor + 12 stands 8 sigma out) with the scene planted at -80."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rows = -120.0 + 1.5 * torch.randn((count, W), device=dev, generator=g)
    r = torch.arange(count, device=dev)
    if kind == "sparse":
        hit = torch.rand(count, device=dev, generator=g) < 0.03
        col = torch.randint(4, W - 8, (count,), device=dev, generator=g)
        for d in range(3):
            rows[r[hit], col[hit] + d] = -80.0
    elif kind == "carriers":
        step = W // n_car
        for k in range(n_car):
            rows[:, step * k + step // 2:step * k + step // 2 + 3] = -80.0 - k
    elif kind == "blips":
        step = W // 8
        for k in range(8):  # the place moves by 4 columns a row and comes back after 8 rows
            for d in range(2):
                rows[r, step * k + 8 + 4 * (r % 8) + d] = -80.0 - k
    return rows.contiguous()


def _copy_ms(torch, found, events, pin_f, pin_e):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(7):
        torch.cuda.synchronize()
        a.record()
        pin_f.copy_(found, non_blocking=True)
        pin_e.copy_(events, non_blocking=True)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return _median(ms)


def _case(torch, plan, dev, st, count, W, K, kinds, track, n_car=8):
    floor = torch.empty(count, device=dev, dtype=torch.float32)
    pin_f = torch.empty(count, dtype=torch.int32).pin_memory()
    pin_e = torch.empty((count, K, 4), dtype=torch.int32).pin_memory()
    for kind in kinds:
        plan.set_detect(0.5, 12.0, 1, K)
        plan.set_track(*track, max_tracks=1 << 22)
        recs, det = [], []
        for k in range(3):
            rows = scene_rows(torch, dev, count, W, kind, 11 + k, n_car)
            found = torch.empty(count, device=dev, dtype=torch.int32)
            events = torch.empty((count, K, 4), device=dev, dtype=torch.int32)
            for _ in range(3):
                plan.detect_device(rows.data_ptr(), count, floor.data_ptr(), found.data_ptr(), events.data_ptr(), st)
                torch.cuda.synchronize()
                assert plan.launch_names() == ["detect_rows"]
                det.append(plan.timings()[0])
            recs.append((found, events))
            del rows
        per, names = {}, None
        reported = 0
        for r in range(7):
            f, e = recs[r % 3]
            plan.track_push_device(f.data_ptr(), e.data_ptr(), count, st)
            torch.cuda.synchronize()
            names = plan.launch_names()
            for n, ms in zip(names, plan.timings()):
                per.setdefault(n, [0.0] * 7)[r] += ms
            reported = len(plan.tracks())
        state = plan.track_state()
        assert state["dropped"] == 0 and state["truncated_rows"] == 0, state
        launches = {n: _median(v) for n, v in per.items()}
        total = round(sum(launches.values()), 5)
        copy = _copy_ms(torch, recs[0][0], recs[0][1], pin_f, pin_e)
        detect = round(statistics.median(det), 5)
        out = {"track_ms": total, "launches_ms": launches, "launch_count": len(names), "detect_rows_ms": detect,
               "copy_ms": copy, "copy_bytes": count * (4 + 16 * K),
               "mean_found": round(float(recs[0][0].float().mean()), 3), "reported_per_push": reported,
               "open": state["open"], "tracker_below_copy": bool(total < copy),
               "tracker_below_detect": bool(total < detect)}
        yield kind, out


def one():
    import torch
    from pypanadapter_amd import ZoomFFT
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    with ZoomFFT(512, 1, 2.4e6, n_win=512) as plan:
        plan.set_timing(True)
        for kind, out in _case(torch, plan, dev, st, 69632, 512, 8, ("sparse", "carriers", "blips"), (0, 0, 1)):
            print(f"RESULT cfg2_g1/{kind} " + json.dumps(out), flush=True)
    with ZoomFFT(65536, 1, 2.4e6, n_win=65536) as plan:
        plan.set_timing(True)
        for kind, out in _case(torch, plan, dev, st, 2048, 65536, 32, ("carriers",), (0, 0, 1), n_car=32):
            print(f"RESULT wide/{kind} " + json.dumps(out), flush=True)
    with ZoomFFT(512, 1, 2.4e6, n_win=512) as plan:  # one row per call, gap 7
        plan.set_timing(True)
        plan.set_detect(0.5, 12.0, 1, 8)
        plan.set_track(7, 0, 1, max_tracks=1 << 16)
        calls = 200
        rows = scene_rows(torch, dev, calls, 512, "carriers", 5)
        floor = torch.empty(calls, device=dev, dtype=torch.float32)
        found = torch.empty(calls, device=dev, dtype=torch.int32)
        events = torch.empty((calls, 8, 4), device=dev, dtype=torch.int32)
        plan.detect_device(rows.data_ptr(), calls, floor.data_ptr(), found.data_ptr(), events.data_ptr(), st)
        torch.cuda.synchronize()
        det = []
        for r in range(7):
            plan.detect_device(rows.data_ptr(), 1, floor.data_ptr(), found.data_ptr(), events.data_ptr(), st)
            torch.cuda.synchronize()
            det.append(plan.timings()[0])
        plan.detect_device(rows.data_ptr(), calls, floor.data_ptr(), found.data_ptr(), events.data_ptr(), st)
        torch.cuda.synchronize()
        dev_ms, host_ms, per = [], [], {}
        for r in range(calls):
            t0 = time.perf_counter()
            plan.track_push_device(found.data_ptr() + 4 * r, events.data_ptr() + 16 * 8 * r, 1, st)
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            ms = plan.timings()
            dev_ms.append(sum(ms))
            for n, v in zip(plan.launch_names(), ms):
                per.setdefault(n, []).append(v)
        pin_f = torch.empty(1, dtype=torch.int32).pin_memory()
        pin_e = torch.empty((1, 8, 4), dtype=torch.int32).pin_memory()
        copy = _copy_ms(torch, found[:1], events[:1], pin_f, pin_e)
        state = plan.track_state()
        assert state["open"] == 8 and state["dropped"] == 0, state
        total = round(statistics.median(dev_ms[20:]), 5)
        out = {"track_ms": total, "launches_ms": {n: round(statistics.median(v[20:]), 5) for n, v in per.items()},
               "launch_count": len(per), "host_ms_per_call": round(statistics.median(host_ms[20:]), 5),
               "detect_rows_ms": _median(det), "copy_ms": copy, "copy_bytes": 4 + 16 * 8, "open": state["open"],
               "tracker_below_copy": bool(total < copy), "tracker_below_detect": bool(total < _median(det))}
        print("RESULT one_row/carriers " + json.dumps(out), flush=True)


def global_rows_ms():
    """detect_rows in global mode on the 69,632 x 512 floor rows: one RESULT line."""
    import torch
    from pypanadapter_amd import ZoomFFT
    from tools.detect_times import make_rows
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    W, count, K = 512, 69632, 8
    with ZoomFFT(512, 1, 2.4e6, n_win=W) as plan:
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
    res = {"what": "tracking off: the parent's tree and this tree alternating in one job on one MI355X, "
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
        main(args[0] if args else os.path.join(OUT_DIR, "track_times.json"))
