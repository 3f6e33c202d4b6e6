"""Ties the device-free hook zfft__welch_plan (pinned by test_welch_plan.py) to what a plan
ran: after a timed ZoomFFT.rows(...) the hook's description for that call must name the Welch
launches at the end of launch_names() -- one launch set per chunk of the segment scratch -- and
the split that zfft__plan_welch_split reports."""
import ctypes
import re

from test_welch_plan import welch_plan

_DESC = re.compile(r"(\w+) (\w+) split=(\d+) last_split=(\d+) lines=(\d+) chunk=(\d+) select=(\w+)$")
WELCH_NAMES = {"welch_rows", "welch4", "welch_lines", "welch_segs", "welch4_segs", "welch_select"}


def assert_plan_ran(plan, L, frames, welch=0, lines_route=0, cap_bytes=0):
    """plan: a ZoomFFT with set_timing(True) whose last call processed `frames` frames of L
    samples (a batched host call: the frames of its last batch); welch, lines_route, cap_bytes:
    what the test set through set_welch and the hooks.  Returns the description."""
    from pypanadapter_amd import _lib, engine
    rc, desc = welch_plan(plan.n_fft, plan.n_win, plan.zoom, engine.IN_DTYPES[plan.in_dtype][0], welch,
                          _lib.AVERAGES[plan.average], plan.segments_per_line, lines_route, cap_bytes, L, frames)
    assert rc == 0, (rc, desc)
    m = _DESC.match(desc)
    assert m, desc
    fft, out, select = m.group(1), m.group(2), m.group(7)
    split, last_split, lines, chunk = (int(m.group(i)) for i in (3, 4, 5, 6))
    if out == "segs":
        sets = -(-frames // chunk)
        want = ["welch4_segs" if fft == "four" else "welch_segs",
                "welch_lines" if select == "mean_lines" else "welch_select"] * sets
    else:
        assert chunk == frames and select == "none", desc
        want = ["welch_lines" if out == "lines" else "welch4" if fft == "four" else "welch_rows"]
    names = plan.launch_names()
    assert names[-len(want):] == want, (desc, names)
    assert not WELCH_NAMES & set(names[:-len(want)][-1:]), (desc, names)  # and not one launch set more
    assert lines == plan.lines(L), (desc, plan.lines(L))
    if fft != "four":  # (the four-step form has no split and leaves the hook's value alone)
        hook = plan.lib.zfft__plan_welch_split
        hook.argtypes, hook.restype = [ctypes.c_void_p], ctypes.c_int
        assert hook(plan._plan) == last_split, (desc, hook(plan._plan))
        assert (split > 1) == (out == "parts") or out in ("segs", "lines"), desc
    return desc
