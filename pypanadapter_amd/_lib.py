"""ctypes binding of libzfft.so (include/zfft.h).

ctypes releases the GIL for the duration of each call, so a QThreadPool worker
(pypanadapter_thread.py:1485-1549) can run the engine while the GUI thread paints.
There is no CPU fallback: if the library is missing the import of the engine fails.
"""
from __future__ import annotations

import ctypes
import importlib.util
import os

from .build import LIB_PATH

ZFFT_OK = 0
ZFFT_EINVAL = -1
ZFFT_ESHORT = -2
ZFFT_EHIP = -3
ZFFT_ENOMEM = -4
ZFFT_ENODEV = -5
ZFFT_EUNSUPPORTED = -6
ZFFT_EINTERNAL = -7

WINDOW_KINDS = {
    "hamming": 0, "hann": 1, "blackman": 2, "blackmanharris": 3, "nuttall": 4, "flattop": 5,
    "barthann": 6, "bartlett": 7, "triang": 8, "bohman": 9, "parzen": 10, "boxcar": 11,
    "kaiser": 12, "gaussian": 13, "general_gaussian": 14, "tukey": 15, "exponential": 16,
    "chebwin": 17, "dpss": 18,
}
# scipy.signal.get_window aliases (scipy/signal/windows/_windows.py `_win_equiv`)
WINDOW_ALIASES = {
    "hamm": "hamming", "ham": "hamming", "han": "hann", "black": "blackman",
    "blk": "blackman", "blackharr": "blackmanharris", "bkh": "blackmanharris", "nutl": "nuttall",
    "nut": "nuttall", "flat": "flattop", "flt": "flattop", "brthan": "barthann", "bth": "barthann",
    "bman": "bohman", "bmn": "bohman",
    "bart": "bartlett", "brt": "bartlett", "triangle": "triang", "tri": "triang", "parz": "parzen",
    "par": "parzen", "box": "boxcar", "ones": "boxcar", "rect": "boxcar", "rectangular": "boxcar",
    "ksr": "kaiser", "gauss": "gaussian", "gss": "gaussian", "general gaussian": "general_gaussian",
    "general gauss": "general_gaussian", "general_gauss": "general_gaussian", "ggs": "general_gaussian",
    "tuk": "tukey", "poisson": "exponential", "cheb": "chebwin",
}
WIN_ARRAY = 100
# enum zfft_average: how a frame's Welch segments combine (zfft_plan_average)
AVERAGES = {"mean": 0, "median": 1, "max": 2}
# enum zfft_view_detector: what a viewport pixel shows of its bucket (zfft_plan_viewport)
VIEW_DETECTORS = {"max": 0, "min": 1, "mean": 2}
# enum zfft_history_format: how the row history stores a value (zfft_plan_history)
HISTORY_FORMATS = {"f32": 0, "u16": 1, "u8": 2}


class zfft_config(ctypes.Structure):
    _fields_ = [
        ("n_fft", ctypes.c_int32), ("zoom", ctypes.c_int32), ("n_win", ctypes.c_int32),
        ("window_kind", ctypes.c_int32), ("fs", ctypes.c_double), ("f_lo", ctypes.c_double),
        ("window_param", ctypes.c_double * 2), ("scroll", ctypes.c_int32),
        ("in_dtype", ctypes.c_int32), ("device", ctypes.c_int32), ("flip_input", ctypes.c_int32),
    ]


class zfft_history_window(ctypes.Structure):
    _fields_ = [
        ("first", ctypes.c_int64), ("rows_per_line", ctypes.c_int32), ("lines", ctypes.c_int32),
        ("col0", ctypes.c_int32), ("col1", ctypes.c_int32), ("width", ctypes.c_int32),
        ("detector", ctypes.c_int32),
    ]


EXPORTS = [
    "zfft_plan_create", "zfft_plan_destroy", "zfft_process", "zfft_process_device",
    "zfft_decimate", "zfft_decimate_frames", "zfft_decimated_length", "zfft_waterfall_push", "zfft_waterfall_push_device",
    "zfft_waterfall_read", "zfft_waterfall_reset", "zfft_waterfall_shape", "zfft_window_values",
    "zfft_plan_tune", "zfft_plan_timing", "zfft_plan_timings", "zfft_plan_timing_names",
    "zfft_plan_path", "zfft_plan_welch", "zfft_plan_average", "zfft_plan_set_lo_frames", "zfft_last_error",
    "zfft_plan_config", "zfft_plan_row_length", "zfft_ring_create", "zfft_ring_destroy", "zfft_ring_add",
    "zfft_ring_state", "zfft_ring_take", "zfft_ring_process",
    "zfft_colormap_lut", "zfft_waterfall_colormap", "zfft_waterfall_levels",
    "zfft_waterfall_get_levels", "zfft_waterfall_autolevel", "zfft_waterfall_render",
    "zfft_waterfall_render_device", "zfft_waterfall_push_render", "zfft_waterfall_push_read64",
    "zfft_host_alloc", "zfft_host_free",
    "zfft_device_count", "zfft_version",
    "zfft_plan_segments_per_line", "zfft_line_count", "zfft_line_times", "zfft_ring_process_lines",
    "zfft_plan_persistence", "zfft_persistence_shape", "zfft_persistence_push_device",
    "zfft_persistence_push", "zfft_persistence_decay", "zfft_persistence_reset", "zfft_persistence_read",
    "zfft_plan_detect", "zfft_detect_shape", "zfft_detect_device", "zfft_detect", "zfft_detect_occupancy",
    "zfft_detect_reset",
    "zfft_plan_detect_local", "zfft_detect_local_shape", "zfft_detect_floors_device", "zfft_detect_floors",
    "zfft_plan_track", "zfft_track_shape", "zfft_track_push_device", "zfft_track_push", "zfft_track_read",
    "zfft_track_open", "zfft_track_flush", "zfft_track_state", "zfft_track_reset",
    "zfft_plan_viewport", "zfft_viewport_edge", "zfft_viewport_shape", "zfft_viewport_push_device",
    "zfft_viewport_push", "zfft_viewport_state", "zfft_viewport_read", "zfft_viewport_traces",
    "zfft_viewport_hold_reset", "zfft_viewport_reset", "zfft_viewport_render_device", "zfft_viewport_render",
    "zfft_viewport_push_render",
    "zfft_plan_history", "zfft_history_shape", "zfft_history_push_device", "zfft_history_push",
    "zfft_history_state", "zfft_history_read_device", "zfft_history_read", "zfft_history_view_device",
    "zfft_history_view", "zfft_history_render", "zfft_history_replay_viewport", "zfft_history_reset",
    "zfft_history_codes", "zfft_history_values",
    "zfft_plan_taps", "zfft_tap_shape", "zfft_tap_open", "zfft_tap_close", "zfft_tap_info", "zfft_tap_counts",
    "zfft_tap_push_device", "zfft_tap_push", "zfft_tap_state", "zfft_tap_reset", "zfft_tap_design",
    "zfft_tap_table",
    "zfft_plan_chan", "zfft_chan_shape", "zfft_chan_select", "zfft_chan_steps", "zfft_chan_push_device",
    "zfft_chan_push", "zfft_chan_state", "zfft_chan_reset", "zfft_chan_info", "zfft_chan_design",
    "zfft_plan_demod", "zfft_demod_shape", "zfft_demod_mode", "zfft_demod_steps", "zfft_demod_push_device",
    "zfft_demod_push", "zfft_demod_state", "zfft_demod_reset", "zfft_demod_info", "zfft_demod_design",
    "zfft_plan_resamp", "zfft_resamp_shape", "zfft_resamp_steps", "zfft_resamp_push_device", "zfft_resamp_push",
    "zfft_resamp_state", "zfft_resamp_reset", "zfft_resamp_info", "zfft_resamp_design",
    "zfft_plan_level", "zfft_level_shape", "zfft_level_steps", "zfft_level_push_device", "zfft_level_push",
    "zfft_level_state", "zfft_level_reset", "zfft_level_info", "zfft_level_meter",
]

_lib = None


class ZfftError(RuntimeError):
    pass


def _share_hip_runtime_with_torch() -> None:
    """PyTorch-ROCm ships its own libamdhip64.so (file name without the .7 suffix but the
    same SONAME, libamdhip64.so.7).  If libzfft.so loads first, the dynamic linker maps
    /opt/rocm's runtime under that SONAME and torch later maps its own file too: two HIP
    runtimes in one process, and torch then reports "No HIP GPUs are available".  When
    torch is installed, pre-load its runtime globally so libzfft.so binds to that one."""
    if os.environ.get("ZFFT_HIP_RUNTIME", "") == "system":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if not spec or not spec.submodule_search_locations:
        return
    hip = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(hip):
        ctypes.CDLL(hip, mode=ctypes.RTLD_GLOBAL)


def load(path: str = ""):
    """Load libzfft.so; raises OSError (loudly) when it has not been built.  ZFFT_LIB_PATH
    selects another in-tree build of the same library (A/B of build variants)."""
    global _lib
    path = path or os.environ.get("ZFFT_LIB_PATH") or LIB_PATH
    if _lib is not None:
        return _lib
    _share_hip_runtime_with_torch()
    if not os.path.exists(path):
        raise OSError(f"libzfft.so not built at {path}: run `python -m pypanadapter_amd.build` "
                      "(there is no CPU fallback)")
    lib = ctypes.CDLL(path)
    P, I32, I64, D = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    cfgp = ctypes.POINTER(zfft_config)
    winp = ctypes.POINTER(zfft_history_window)
    sig = {
        "zfft_plan_create": (ctypes.c_int, [cfgp, P, ctypes.POINTER(P)]),
        "zfft_plan_destroy": (ctypes.c_int, [P]),
        "zfft_process": (ctypes.c_int, [P, P, I64, I32, P]),
        "zfft_process_device": (ctypes.c_int, [P, P, I64, I32, P, P]),
        "zfft_decimate": (ctypes.c_int, [P, P, I64, P, ctypes.POINTER(I64)]),
        "zfft_decimate_frames": (ctypes.c_int, [P, P, I64, I32, P, ctypes.POINTER(I64)]),
        "zfft_decimated_length": (I64, [I64, I32]),
        "zfft_waterfall_push": (ctypes.c_int, [P, P]),
        "zfft_waterfall_push_device": (ctypes.c_int, [P, P, I32, P]),
        "zfft_waterfall_read": (ctypes.c_int, [P, P]),
        "zfft_waterfall_reset": (ctypes.c_int, [P, I32]),
        "zfft_waterfall_shape": (ctypes.c_int, [P, ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "zfft_window_values": (ctypes.c_int, [I32, P, I32, P]),
        "zfft_plan_tune": (ctypes.c_int, [P, I32, I32]),
        "zfft_plan_timing": (ctypes.c_int, [P, I32]),
        "zfft_plan_timings": (ctypes.c_int, [P, P, I32, ctypes.POINTER(I32)]),
        "zfft_plan_timing_names": (ctypes.c_char_p, [P]),
        "zfft_plan_path": (ctypes.c_int, [P, I32]),
        "zfft_plan_welch": (ctypes.c_int, [P, I32]),
        "zfft_plan_average": (ctypes.c_int, [P, I32]),
        "zfft_plan_set_lo_frames": (ctypes.c_int, [P, P, I32, I32]),
        "zfft_last_error": (ctypes.c_char_p, []),
        "zfft_plan_config": (ctypes.c_int, [P, cfgp]),
        "zfft_plan_row_length": (ctypes.c_int, [P]),
        "zfft_ring_create": (ctypes.c_int, [I64, I32, ctypes.POINTER(P)]),
        "zfft_ring_destroy": (ctypes.c_int, [P]),
        "zfft_ring_add": (ctypes.c_int, [P, P, I64]),
        "zfft_ring_state": (ctypes.c_int, [P, ctypes.POINTER(I64), ctypes.POINTER(I64),
                                            ctypes.POINTER(I64)]),
        "zfft_ring_take": (ctypes.c_int, [P, ctypes.POINTER(P), ctypes.POINTER(I64),
                                           ctypes.POINTER(I64)]),
        "zfft_ring_process": (ctypes.c_int, [P, P, P, ctypes.POINTER(I32)]),
        "zfft_plan_segments_per_line": (ctypes.c_int, [P, I32]),
        "zfft_line_count": (I64, [I64, I32, I32, I32]),
        "zfft_line_times": (ctypes.c_int, [I64, I32, I32, D, I32, P, I32, ctypes.POINTER(I32)]),
        "zfft_ring_process_lines": (ctypes.c_int, [P, P, P, I32, ctypes.POINTER(I32)]),
        "zfft_plan_persistence": (ctypes.c_int, [P, I32, D, D]),
        "zfft_persistence_shape": (ctypes.c_int, [P, ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "zfft_persistence_push_device": (ctypes.c_int, [P, P, I32, P]),
        "zfft_persistence_push": (ctypes.c_int, [P, P, I32]),
        "zfft_persistence_decay": (ctypes.c_int, [P, D]),
        "zfft_persistence_reset": (ctypes.c_int, [P]),
        "zfft_persistence_read": (ctypes.c_int, [P, P, ctypes.POINTER(ctypes.c_uint64)]),
        "zfft_plan_detect": (ctypes.c_int, [P, D, D, I32, I32]),
        "zfft_detect_shape": (ctypes.c_int, [P, ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "zfft_detect_device": (ctypes.c_int, [P, P, I32, P, P, P, P]),
        "zfft_detect": (ctypes.c_int, [P, P, I32, P, P, P]),
        "zfft_detect_occupancy": (ctypes.c_int, [P, P, ctypes.POINTER(ctypes.c_uint64)]),
        "zfft_detect_reset": (ctypes.c_int, [P]),
        "zfft_plan_detect_local": (ctypes.c_int, [P, I32, I32]),
        "zfft_detect_local_shape": (ctypes.c_int, [P, ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "zfft_detect_floors_device": (ctypes.c_int, [P, P, I32, P, P]),
        "zfft_detect_floors": (ctypes.c_int, [P, P, I32, P]),
        "zfft_plan_track": (ctypes.c_int, [P, I32, I32, I32, I32]),
        "zfft_track_shape": (ctypes.c_int, [P] + [ctypes.POINTER(I32)] * 4),
        "zfft_track_push_device": (ctypes.c_int, [P, P, P, I32, P]),
        "zfft_track_push": (ctypes.c_int, [P, P, P, I32]),
        "zfft_track_read": (ctypes.c_int, [P, P, I32, ctypes.POINTER(I32)]),
        "zfft_track_open": (ctypes.c_int, [P, P, I32, ctypes.POINTER(I32)]),
        "zfft_track_flush": (ctypes.c_int, [P]),
        "zfft_track_state": (ctypes.c_int, [P, P]),
        "zfft_track_reset": (ctypes.c_int, [P]),
        "zfft_plan_viewport": (ctypes.c_int, [P, I32, I32, I32, I32, I32, I32]),
        "zfft_viewport_edge": (I64, [I32, I32, I32, I32]),
        "zfft_viewport_shape": (ctypes.c_int, [P, ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "zfft_viewport_push_device": (ctypes.c_int, [P, P, I32, P]),
        "zfft_viewport_push": (ctypes.c_int, [P, P, I32]),
        "zfft_viewport_state": (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                                ctypes.POINTER(I32)]),
        "zfft_viewport_read": (ctypes.c_int, [P, P]),
        "zfft_viewport_traces": (ctypes.c_int, [P, P, P, P]),
        "zfft_viewport_hold_reset": (ctypes.c_int, [P]),
        "zfft_viewport_reset": (ctypes.c_int, [P]),
        "zfft_viewport_render_device": (ctypes.c_int, [P, P, P]),
        "zfft_viewport_render": (ctypes.c_int, [P, P]),
        "zfft_viewport_push_render": (ctypes.c_int, [P, P, I32, P]),
        "zfft_plan_history": (ctypes.c_int, [P, I64, I32, D, D]),
        "zfft_history_shape": (ctypes.c_int, [P, ctypes.POINTER(I64), ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "zfft_history_push_device": (ctypes.c_int, [P, P, I32, P]),
        "zfft_history_push": (ctypes.c_int, [P, P, I32]),
        "zfft_history_state": (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
        "zfft_history_read_device": (ctypes.c_int, [P, I64, I32, P, P]),
        "zfft_history_read": (ctypes.c_int, [P, I64, I32, P]),
        "zfft_history_view_device": (ctypes.c_int, [P, winp, P, P]),
        "zfft_history_view": (ctypes.c_int, [P, winp, P]),
        "zfft_history_render": (ctypes.c_int, [P, winp, P]),
        "zfft_history_replay_viewport": (ctypes.c_int, [P, I64]),
        "zfft_history_reset": (ctypes.c_int, [P]),
        "zfft_history_codes": (ctypes.c_int, [I32, D, D, P, I64, P]),
        "zfft_history_values": (ctypes.c_int, [I32, D, D, P, I64, P]),
        "zfft_plan_taps": (ctypes.c_int, [P, I32, I32]),
        "zfft_tap_shape": (ctypes.c_int, [P, ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "zfft_tap_open": (ctypes.c_int, [P, I32, I64, I32, I32, P]),
        "zfft_tap_close": (ctypes.c_int, [P, I32]),
        "zfft_tap_info": (ctypes.c_int, [P, I32, ctypes.POINTER(I32), ctypes.POINTER(I64), ctypes.POINTER(I32),
                                          ctypes.POINTER(I32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(D)]),
        "zfft_tap_counts": (ctypes.c_int, [P, I64, P]),
        "zfft_tap_push_device": (ctypes.c_int, [P, P, I64, P, P]),
        "zfft_tap_push": (ctypes.c_int, [P, P, I64, P, P]),
        "zfft_tap_state": (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_uint64)]),
        "zfft_tap_reset": (ctypes.c_int, [P, I64]),
        "zfft_tap_design": (ctypes.c_int, [I32, D, D, P]),
        "zfft_tap_table": (ctypes.c_int, [I64, I32, P, P]),
        "zfft_plan_chan": (ctypes.c_int, [P, I32, I32, I32, P]),
        "zfft_chan_shape": (ctypes.c_int, [P] + [ctypes.POINTER(I32)] * 5),
        "zfft_chan_select": (ctypes.c_int, [P, I32, I32]),
        "zfft_chan_steps": (ctypes.c_int, [P, I64, ctypes.POINTER(I64)]),
        "zfft_chan_push_device": (ctypes.c_int, [P, P, I64, P, P]),
        "zfft_chan_push": (ctypes.c_int, [P, P, I64, P, P]),
        "zfft_chan_state": (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_uint64)]),
        "zfft_chan_reset": (ctypes.c_int, [P, I64]),
        "zfft_chan_info": (ctypes.c_int, [P, ctypes.POINTER(D), ctypes.POINTER(D)]),
        "zfft_chan_design": (ctypes.c_int, [I32, I32, D, P]),
        "zfft_plan_demod": (ctypes.c_int, [P, I32, I32, I32, P]),
        "zfft_demod_shape": (ctypes.c_int, [P] + [ctypes.POINTER(I32)] * 3),
        "zfft_demod_mode": (ctypes.c_int, [P, I32, I32, I32, I64]),
        "zfft_demod_steps": (ctypes.c_int, [P, I64, ctypes.POINTER(I64)]),
        "zfft_demod_push_device": (ctypes.c_int, [P, P, I64, I64, I64, P, P]),
        "zfft_demod_push": (ctypes.c_int, [P, P, I64, I64, I64, P, P]),
        "zfft_demod_state": (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_uint64)]),
        "zfft_demod_reset": (ctypes.c_int, [P, I64]),
        "zfft_demod_info": (ctypes.c_int, [P, ctypes.POINTER(D), ctypes.POINTER(D)]),
        "zfft_demod_design": (ctypes.c_int, [I32, D, D, P]),
        "zfft_plan_resamp": (ctypes.c_int, [P, I32, I32, I32, I32, P, I32, ctypes.c_float]),
        "zfft_resamp_shape": (ctypes.c_int, [P] + [ctypes.POINTER(I32)] * 5),
        "zfft_resamp_steps": (ctypes.c_int, [P, I64, ctypes.POINTER(I64)]),
        "zfft_resamp_push_device": (ctypes.c_int, [P, P, I64, I64, P, P]),
        "zfft_resamp_push": (ctypes.c_int, [P, P, I64, I64, P, P]),
        "zfft_resamp_state": (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_uint64)]),
        "zfft_resamp_reset": (ctypes.c_int, [P, I64]),
        "zfft_resamp_info": (ctypes.c_int, [P, ctypes.POINTER(D), ctypes.POINTER(D)]),
        "zfft_resamp_design": (ctypes.c_int, [I32, I32, I32, D, P]),
        "zfft_plan_level": (ctypes.c_int, [P, I32, I32, I32] + [ctypes.c_float] * 4),
        "zfft_level_shape": (ctypes.c_int, [P] + [ctypes.POINTER(I32)] * 3 + [ctypes.POINTER(ctypes.c_float)] * 4),
        "zfft_level_steps": (ctypes.c_int, [P, I64, ctypes.POINTER(I64)]),
        "zfft_level_push_device": (ctypes.c_int, [P, P, I64, I64, P, I64, P, P]),
        "zfft_level_push": (ctypes.c_int, [P, P, P, I64, I64, P, P]),
        "zfft_level_state": (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_uint64)]),
        "zfft_level_reset": (ctypes.c_int, [P, I64]),
        "zfft_level_info": (ctypes.c_int, [P, ctypes.POINTER(D), ctypes.POINTER(D), ctypes.POINTER(D)]),
        "zfft_level_meter": (ctypes.c_int, [P, P, P]),
        "zfft_colormap_lut": (ctypes.c_int, [ctypes.c_char_p, P]),
        "zfft_waterfall_colormap": (ctypes.c_int, [P, ctypes.c_char_p]),
        "zfft_waterfall_levels": (ctypes.c_int, [P, D, D]),
        "zfft_waterfall_get_levels": (ctypes.c_int, [P, ctypes.POINTER(D), ctypes.POINTER(D)]),
        "zfft_waterfall_autolevel": (ctypes.c_int, [P, ctypes.POINTER(D), ctypes.POINTER(D)]),
        "zfft_waterfall_render": (ctypes.c_int, [P, P]),
        "zfft_waterfall_render_device": (ctypes.c_int, [P, P, P]),
        "zfft_waterfall_push_render": (ctypes.c_int, [P, P, I32, P]),
        "zfft_waterfall_push_read64": (ctypes.c_int, [P, P, I32, P]),
        "zfft_host_alloc": (ctypes.c_int, [ctypes.c_size_t, ctypes.POINTER(P)]),
        "zfft_host_free": (ctypes.c_int, [P]),
        "zfft_device_count": (ctypes.c_int, []),
        "zfft_version": (ctypes.c_int, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    """Map a negative ZFFT_E* code to the exception the reference path would raise."""
    if rc == ZFFT_OK:
        return
    msg = (_lib.zfft_last_error() or b"").decode(errors="replace") if _lib else ""
    text = f"{what}: {msg} (code {rc})"
    if rc in (ZFFT_EINVAL, ZFFT_ESHORT):
        raise ValueError(text)  # scipy raises ValueError for these (e.g. padlen)
    if rc == ZFFT_EUNSUPPORTED:
        raise NotImplementedError(text)
    raise ZfftError(text)
