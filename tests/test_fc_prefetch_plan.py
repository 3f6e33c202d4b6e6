"""CPU check of the FC decimator's prefetch group plans (fc_prefetch_plan.h): the
constexpr tables the kernel is compiled from, printed by a small host program
(tests/host/fc_prefetch_plan_dump.cpp).  A window is 16 pairs per thread; the last KEEP = 16 - S
are carried in registers into the next window, the S others are requested in groups at up to five
points of the block.  For every instantiation (zoom x input format x flip) the groups together
request each of the S new pairs exactly once and none of the carried ones, with the shipped
knobs and with the one that restores the request schedule of before the spread (FC_PARENT)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pypanadapter_amd", "csrc")
STEPS = {8: 13, 4: 14, 2: 15}      # S per zoom (zfft_internal.h: kFcStep, kFc4Step, kFc2Step)
POINTS = 5


def _plans(tmp_path, defines=()):
    """{(Z, DT, FLIP): [pairs of group 0, ..., pairs of group 4]}"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/host/fc_prefetch_plan_dump.cpp"
    exe = str(tmp_path / ("fc_prefetch_plan_dump" + "_".join(defines).replace("=", "")))
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, *[f"-D{d}" for d in defines],
                    os.path.join(ROOT, "tests", "host", "fc_prefetch_plan_dump.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    plans = {}
    for line in r.stdout.splitlines():
        head, _, pairs = line.partition("  ")
        Z, DT, FLIP, S, KEEP, g = (int(v) for v in head.split())
        assert S == STEPS[Z] and KEEP == 16 - S, line
        groups = plans.setdefault((Z, DT, FLIP), [])
        assert g == len(groups), line
        groups.append([int(v) for v in pairs.split()])
    return plans


def _check(plans):
    assert sorted(plans) == [(Z, DT, FLIP) for Z in (2, 4, 8) for DT in range(4) for FLIP in (0, 1)]
    for (Z, DT, FLIP), groups in plans.items():
        S = STEPS[Z]
        keep = 16 - S
        assert len(groups) == POINTS, (Z, DT, FLIP, groups)
        asked = [p for g in groups for p in g]
        assert sorted(asked) == list(range(keep, 16)), (Z, DT, FLIP, groups)   # each new pair once
        assert not set(asked) & set(range(keep)), (Z, DT, FLIP, groups)        # no carried pair
        assert len(asked) == S


@pytest.mark.parametrize("defines", [(), ("FC_PARENT=1",), ("FC_PF_SPREAD=0",)],
                         ids=["shipped", "parent", "burst"])
def test_every_plan_requests_each_new_pair_once(tmp_path, defines):
    _check(_plans(tmp_path, defines))


def test_steps_covered(tmp_path):
    """S = 13 (zoom 8), 14 (zoom 4) and 15 (zoom 2) are all there."""
    plans = _plans(tmp_path)
    assert {len([p for g in gs for p in g]) for gs in plans.values()} == {13, 14, 15}


def test_parent_knob_requests_at_the_head(tmp_path):
    """FC_PARENT=1: zoom 8 and 4 request the whole window at the block head; zoom 2 keeps its
    split (complex64: 10 at the head, 5 after pass C) with and without the knob."""
    parent, shipped = _plans(tmp_path, ("FC_PARENT=1",)), _plans(tmp_path)
    for (Z, DT, FLIP), groups in parent.items():
        if Z != 2:
            assert [len(g) for g in groups] == [STEPS[Z], 0, 0, 0, 0], (Z, DT, FLIP, groups)
        else:
            assert groups == shipped[(Z, DT, FLIP)]
    assert [len(g) for g in shipped[(2, 0, 0)]] == [10, 0, 0, 0, 5]
    # the flagship's instantiation does spread
    assert sum(1 for g in shipped[(8, 0, 0)] if g) >= 3, shipped[(8, 0, 0)]
