"""CPU check of the zoom-2 FC kernel's register budget (fc2_kernels.hip: fc_kernels.hip's template
at Z = 2): each of the eight fc_decim_kernel<2, dtype, flip> instantiations compiles
for gfx950 without VGPR spills or scratch at its launch bound (256 threads, two workgroups per CU:
at most 256 VGPRs and half a CU's 160 KiB of LDS)."""
import os
import re
import shutil
import subprocess

import pytest

from test_fc_build import CSRC, HIPCC, ROOT


def test_fc2_decim_instantiations_do_not_spill(tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC,
                          "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-c",
                          os.path.join(CSRC, "fc2_kernels.hip"), "-o", str(tmp_path / "fc2.o"),
                          "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"(VGPRs Spill|SGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    usage = {k: v for k, v in usage.items() if "fc_decim_kernel" in k}
    assert len(usage) == 8 and all("fc_decim_kernelILi2E" in k for k in usage), sorted(usage)
    for name, u in usage.items():
        assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, (name, u)
        assert u.get("ScratchSize [bytes/lane]") == 0, (name, u)
        assert 0 < u.get("VGPRs", 0) <= 256, (name, u)
        assert 0 < u.get("LDS Size [bytes/block]", 0) <= 80 * 1024, (name, u)
