"""The register check of tests/test_fc_build_parent.py for the knob of the range-checked window
requests (FC_TAIL_CARRY, fc_prefetch_plan.h): with the shipped value 1 and with 0,
which gives the code of before for every instantiation, all 16 fc_decim_kernel instantiations of
zoom 8 and 4 compile for gfx950 without spills or scratch at their launch bound, so both sides of
an A/B (and of tests/test_gpu_fc_tail.py) build from one checkout."""
import pytest

from test_fc_build_parent import _resource_usage


@pytest.mark.parametrize("knob", [1, 0])
def test_fc_decim_tail_carry_knob_does_not_spill(tmp_path, knob):
    usage = _resource_usage(tmp_path, (f"FC_TAIL_CARRY={knob}",))
    assert len(usage) == 16, sorted(usage)     # zoom {8, 4} x 4 input formats x 2 flips
    for name, u in usage.items():
        assert u.get("VGPRs Spill") == 0 and u.get("SGPRs Spill") == 0, (name, u)
        assert u.get("ScratchSize [bytes/lane]") == 0, (name, u)
        assert 0 < u.get("VGPRs", 0) <= 256, (name, u)
