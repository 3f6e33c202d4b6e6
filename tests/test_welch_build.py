"""CPU check of the in-place DIF Welch kernel's register budget (zfft_kernels.hip):
every welch_dif_kernel<N, PRUNE, HALF, SEG, LINES> instantiation compiles for gfx950 without VGPR
or SGPR spills and without scratch, within the VGPR bound of the waves per SIMD its
__launch_bounds__ ask for (512 VGPRs per SIMD lane: 128 at 4 waves, 168 at 3, 256 at 2; a
1024-thread workgroup is 4 waves per SIMD whatever the second argument says), and at no lower
occupancy than before the window was held in registers (zfft_dif_addr.h: win_hold).  A change that
makes one spill or drop a wave (a larger hold, a longer prefetch) fails here before it reaches a
GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pypanadapter_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
VGPR_BOUND = {4: 128, 3: 168, 2: 256}
SIZES = (1024, 2048, 4096, 8192, 16384)


def declared_waves(N, prune):
    """The second __launch_bounds__ argument (Dif<N>::WAVES_PRUNE / WAVES_FULL), raised to what
    the workgroup size itself takes."""
    declared = (4 if prune else 3) if N <= 2048 else (3 if prune else 2) if N == 4096 else 2
    threads = max(256, N // 16)
    return max(declared, threads // 64 // 4)


def occupancy_before(N, prune, half, seg, lines):
    """Waves per SIMD of the instantiation before this header existed: the register count of the
    N = 4096 full forms and of three N = 8192 forms was within 168 although they declare 2."""
    if N == 4096:
        return 3
    if N == 8192:
        return 3 if half and not lines else 2
    return declared_waves(N, prune)


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    obj = tmp_path_factory.mktemp("welch_build") / "zfft.o"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC,
                          "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
                          os.path.join(CSRC, "zfft_kernels.hip"), "-o", str(obj),
                          "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    found, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            found[name] = {}
            continue
        m = re.search(r"(VGPRs Spill|SGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            found[name][m.group(1)] = int(m.group(2))
    by_args = {}
    for name, u in found.items():
        # _ZN4zfft16welch_dif_kernelILi4096ELb1ELb1ELb0ELb0EEEv...: N, PRUNE, HALF, SEG, LINES
        m = re.match(r"_ZN4zfft16welch_dif_kernelILi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])EEEv", name)
        if m:
            N, *flags = (int(g) for g in m.groups())
            by_args[(N, *(bool(f) for f in flags))] = u
    return by_args


def test_the_instantiations_are_those_the_launcher_names(usage):
    """Five sizes x PRUNE x HALF x (sum, SEG, LINES)."""
    want = {(N, p, h, s, l) for N in SIZES for p in (False, True) for h in (False, True)
            for s, l in ((False, False), (True, False), (False, True))}
    assert set(usage) == want, sorted(set(usage) ^ want)
    assert len(usage) == 60


def test_no_spills_and_within_the_launch_bound(usage):
    for key, u in sorted(usage.items()):
        N, prune = key[0], key[1]
        assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, (key, u)
        assert u.get("ScratchSize [bytes/lane]") == 0, (key, u)
        assert 0 < u.get("VGPRs", 0) <= VGPR_BOUND[declared_waves(N, prune)], (key, u)


def test_occupancy_did_not_drop(usage):
    for key, u in sorted(usage.items()):
        assert u.get("Occupancy [waves/SIMD]", 0) >= occupancy_before(*key), (key, u)
