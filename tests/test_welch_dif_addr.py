"""CPU check of the DIF Welch kernel's LDS address rule and window-hold table (zfft_dif_addr.h,
DESIGN §3.3), through a small host program compiled from the header the kernel is compiled from
(tests/host/dif_addr_check.cpp).  The kernel stores stage 1 at slot(t) plus a constant per value
and reads and writes the middle stages at slot(base) plus a constant:

  slot(T k + t)   == slot(t)    + (T + T/16) k      0 <= t < T = N/16, 0 <= k < 16
  slot(base + S m) == slot(base) + slot(S m)         base = (t / S) 16 S + t mod S, S = N / 16^stage

for every N in 1024 .. 16384, every thread and every value; the constants must fit the LDS
instructions' 16-bit byte offset (8-byte slots), past which stage 1 of N = 16384 takes a second
base.  The program checks each identity exhaustively and exits 1 at the first mismatch."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pypanadapter_amd", "csrc")
SIZES = (1024, 2048, 4096, 8192, 16384)


def _run(tmp_path, defines=()):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/dif_addr_check.cpp"
    exe = str(tmp_path / ("dif_addr_check" + "_".join(defines).replace("=", "")))
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, *[f"-D{d}" for d in defines],
                    os.path.join(ROOT, "tests", "host", "dif_addr_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def test_address_identity_for_every_size_thread_and_value(tmp_path):
    lines = _run(tmp_path)
    stage1 = {}
    for l in lines:
        if " stage=1 " in l:
            f = dict(kv.split("=") for kv in l.split())
            stage1[int(f["N"])] = f
    assert sorted(stage1) == list(SIZES)
    for N in SIZES:
        f = stage1[N]
        assert int(f["checked"]) == N and int(f["stride"]) == N // 16       # every t, every k
        assert int(f["max_slot"]) == N - 1 + (N - 1) // 16                  # the image's last slot
        # 2176 bytes per value at N = 4096; only N = 16384 outgrows the offset field, from k = 8
        assert int(f["second_base_from"]) == (8 if N == 16384 else 16)
    mids = [l for l in lines if " stage=" in l and " stage=1 " not in l]
    # radix-16 stages before the last: 2 at N = 1024 .. 4096 (stage 2), 3 at 8192 and 16384
    assert sorted((int(l.split()[0][2:]), int(l.split()[1][6:])) for l in mids) == \
        [(1024, 2), (2048, 2), (4096, 2), (8192, 2), (8192, 3), (16384, 2), (16384, 3)]
    for l in mids:
        f = dict(kv.split("=") for kv in l.split())
        assert int(f["checked"]) == int(f["N"])
    assert [l for l in lines if " last " in l] == [f"N={N} last slots={N + N // 16 - 1}" for N in SIZES]


def _holds(lines):
    out = {}
    for l in lines:
        if l.startswith("hold "):
            N, p, h, s, ln, n = (int(v) for v in l.split()[1:])
            out[(N, bool(p), bool(h), bool(s), bool(ln))] = n
    return out


def test_window_hold_table(tmp_path):
    """All 16 values for the batch headline's instantiation, none where the register bound is
    128 (tests/test_welch_build.py checks the bounds themselves); ZFFT_DIF_WHOLD=0 holds none."""
    holds = _holds(_run(tmp_path))
    assert len(holds) == 60 and all(0 <= n <= 16 for n in holds.values())
    for lines_form in ((False, False), (True, False), (False, True)):
        assert holds[(4096, True, True, *lines_form)] == 16
    for key, n in holds.items():
        N, prune = key[0], key[1]
        if N == 16384 or (N <= 2048 and prune):
            assert n == 0, key
    off = _holds(_run(tmp_path, ("ZFFT_DIF_WHOLD=0",)))
    assert len(off) == 60 and not any(off.values())
