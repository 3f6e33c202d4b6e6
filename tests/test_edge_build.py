"""CPU check of the batched frame-end kernel's register budget (pc_edge_batch_kernel,
pc_kernels.hip): every <DT, FLIP> instantiation compiles for gfx950 without scratch
and within 64 VGPRs, so eight of its waves fit a SIMD's 512 registers, and the kernels it
replaced (the side stream's V^T x and the U v behind the join) are gone from the code object."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pypanadapter_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    obj = tmp_path_factory.mktemp("edge_build") / "pc.o"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC,
                          "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
                          os.path.join(CSRC, "pc_kernels.hip"), "-o", str(obj),
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
    return found


def _batch(usage):
    by_args = {}
    for name, u in usage.items():
        # _ZN4zfft2pc20pc_edge_batch_kernelILi0ELi1EEEv...: DT, FLIP
        m = re.match(r"_ZN4zfft2pc20pc_edge_batch_kernelILi(\d)ELi([01])EEEv", name)
        if m:
            by_args[(int(m.group(1)), int(m.group(2)))] = u
    return by_args


def test_the_instantiations_are_those_the_launcher_names(usage):
    """Four input formats x np.flip."""
    assert set(_batch(usage)) == {(dt, fl) for dt in range(4) for fl in (0, 1)}


def test_no_scratch_and_eight_waves_fit(usage):
    for key, u in sorted(_batch(usage).items()):
        assert u.get("ScratchSize [bytes/lane]") == 0, (key, u)
        assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, (key, u)
        assert 0 < u.get("VGPRs", 0) <= 64, (key, u)


def test_the_split_kernels_are_gone(usage):
    assert usage, "no kernel found in the compiler's remarks"
    left = [n for n in usage if "pc_edge_v_kernel" in n or "pc_edge_u_kernel" in n]
    assert not left, left
