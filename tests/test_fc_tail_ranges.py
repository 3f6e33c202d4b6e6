"""CPU check of the FC decimator's range-checked window requests (fc_prefetch_plan.h, FC_TAIL_CARRY;
DESIGN §3.9).  Request j of a window is 512 samples, a pair per lane, read through a buffer
resource of its own: the base is the request's first byte, the size the frame's bytes left from
there (at most the request's), the lane's offset the only address.  A small host program
(tests/host/fc_tail_ranges_dump.cpp) prints base and size from the constexpr functions the kernel
is compiled from; here a raw buffer load is modelled on them -- dword by dword, a dword at or past
the resource's size reads 0 -- and compared with the definition the kernel's per-sample loads
follow: sample n of the frame for 0 <= n < L, 0 outside.  Every block after a frame's first,
every request, every lane, zoom 8 and 4, complex64 / complex32 / real f32; frame lengths around
every position of the frame's end against the window grid."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pypanadapter_amd", "csrc")
STEP = {8: 13, 4: 14}                   # 512-sample requests a block advances (kFcStep, kFc4Step)
EB = {0: 8, 1: 4, 3: 4}                 # bytes per sample: complex64, complex32, real f32
N = 8192


def lengths(Z):
    hop = 512 * STEP[Z]
    Ls = set(range(N, N + 32))
    for k in (1, 2):
        Ls |= set(range(N + hop * k - 17, N + hop * k + 18))
    if Z == 8:
        Ls.add(13313)                   # nb = 3: the last window's requests j >= 2 lie past the frame
    return sorted(Ls)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/fc_tail_ranges_dump.cpp"
    exe = str(tmp_path_factory.mktemp("fc_tail") / "fc_tail_ranges_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "fc_tail_ranges_dump.cpp"), "-o", exe], check=True)

    def run(Z):
        r = subprocess.run([exe, str(Z), *map(str, lengths(Z))], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr
        lane, reqs = {}, []
        for line in r.stdout.splitlines():
            w = line.split()
            if w[0] == "lane":
                lane.setdefault(int(w[1]), []).append(int(w[3]))
            else:
                reqs.append(tuple(int(v) for v in w[1:]))
        return {eb: np.array(v, dtype=np.int64) for eb, v in lane.items()}, reqs
    return run


def test_lengths_are_the_documented_set():
    assert len(lengths(8)) == 32 + 2 * 35 + 1 and len(lengths(4)) == 32 + 2 * 35
    assert 8192 + 6656 - 17 in lengths(8) and 8192 + 2 * 7168 + 17 in lengths(4)


@pytest.mark.parametrize("Z", [8, 4])
def test_requests_return_the_frames_samples_and_zero_past_its_end(dump, Z):
    lane, reqs = dump(Z)
    S, keep = STEP[Z], 16 - STEP[Z]
    K, P = (N - 512 * S) // 2, 512 * S // Z
    for eb in (4, 8):
        assert lane[eb].shape == (256,)
    seen = set()
    t = np.arange(256, dtype=np.int64)
    for z, DT, L, b, more, j, base, size in reqs:
        assert z == Z and keep <= j < 16
        eb = EB[DT]
        nb = -(-(-(-L // Z)) // P)
        assert 1 <= b <= nb and more == (b < nb)
        seen.add((DT, L, b, j))
        s = 512 * S * b - K
        assert s >= 0                                   # the window starts inside the frame
        assert base == (s + 512 * j) * eb and 0 <= size <= 512 * eb and size % eb == 0
        # the resource lies inside the frame: nothing in range is outside the caller's buffer
        assert size == 0 or (base >= 0 and base + size <= L * eb)
        # the load: 2 eb bytes per lane at the lane's offset, range-checked per dword
        off = lane[eb]
        dw = off[:, None] + 4 * np.arange(2 * eb // 4)[None, :]       # byte offset of each dword
        inr = dw < size
        # the frame as dwords: dword d holds 1 + d (never 0), so a returned value names its address
        got = np.where(inr, 1 + (base + dw) // 4, 0)
        # the definition: samples n, n + 1 with n = s + 512 j + 2 t; 0 outside the frame, and
        # nothing at all when no block follows (the kernel asks for nothing then)
        n = (s + 512 * j + 2 * t)[:, None] + (np.arange(2 * eb // 4)[None, :] * 4) // eb
        want = np.where((n >= 0) & (n < L) & bool(more), 1 + (n * eb) // 4 + (np.arange(2 * eb // 4)[None, :] % (eb // 4)), 0)
        assert np.array_equal(got, want), (Z, DT, L, b, j)
    # every block after the first (and the window past the last), every request, every format
    for L in lengths(Z):
        nb = -(-(-(-L // Z)) // P)
        for DT in EB:
            for b in range(1, nb + 1):
                for j in range(keep, 16):
                    assert (DT, L, b, j) in seen, (DT, L, b, j)


def test_a_pair_across_an_odd_frames_end_is_one_sample_and_one_zero(dump):
    """L odd: the lane whose pair is (L - 1, L) gets the sample and a 0, in every format."""
    lane, reqs = dump(8)
    hit = 0
    for z, DT, L, b, more, j, base, size in reqs:
        if not (L % 2 and more):
            continue
        eb = EB[DT]
        s = 512 * 13 * b - 768
        k = L - 1 - (s + 512 * j)
        if 0 <= k < 512 and k % 2 == 0:                  # sample L - 1 is the first of lane k / 2's pair
            off = int(lane[eb][k // 2])
            assert off < size <= off + eb, (DT, L, b, j, off, size)
            hit += 1
    assert hit >= 3 * 30


def test_last_window_of_13313_requests_only_its_first_two(dump):
    """Zoom 8, L = 13,313: nb = 3, the last window starts at 12,544 with 769 samples of the frame
    left, so request 3 (the first new one, j = KEEP) and everything after it is wholly past."""
    _, reqs = dump(8)
    mine = [r for r in reqs if r[2] == 13313 and r[1] == 0]
    assert {r[3] for r in mine} == {1, 2, 3}
    last = [r for r in mine if r[3] == 2]
    assert len(last) == 13 and all(r[7] == 0 for r in last)
    first = {r[5]: r[7] for r in mine if r[3] == 1}      # window 1 starts at 5,888: 7,425 left
    assert first[13] == 4096 and first[14] == (7425 - 14 * 512) * 8 and first[15] == 0
