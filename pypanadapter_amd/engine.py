"""Host-side engine: one `ZoomFFT` plan per (N, zoom, W, window, fs, f_lo, scroll).

Mirrors the reference's per-frame DSP (pypanadapter_spectrum.py:2088-2119) and its
waterfall model (S:1625-1664) behind libzfft.so.  Host numpy buffers go through the
synchronous C-ABI calls; device tensors (torch, on the plan's device) go through
`process_device`, which enqueues on a caller-supplied HIP stream and does not sync.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from ._lib import check, zfft_config


def _window_spec(window):
    """AppState.fft_tapering value -> (kind, params, array_or_None).

    Accepts what the reference stores (S:1358-1363): a scipy window name, a
    (name, p0[, p1]) tuple, or an explicit array (any other scipy window).  Absent
    parameters are NaN: the native generator applies scipy's default or refuses the window
    as get_window does.
    """
    if isinstance(window, np.ndarray) or (isinstance(window, (list,)) and window and
                                          not isinstance(window[0], str)):
        return _lib.WIN_ARRAY, (0.0, 0.0), np.ascontiguousarray(window, dtype=np.float32)
    name, params = (window, ()) if isinstance(window, str) else (window[0], tuple(window[1:]))
    name = _lib.WINDOW_ALIASES.get(name.lower(), name.lower())
    if name not in _lib.WINDOW_KINDS:
        raise ValueError(f"window {window!r} has no native generator; pass it as an array "
                         "(e.g. scipy.signal.get_window(window, n_fft))")
    if len(params) > 2:
        raise ValueError(f"window {window!r}: at most two parameters")
    p = [float(v) for v in params] + [float("nan")] * 2
    return _lib.WINDOW_KINDS[name], (p[0], p[1]), None


def full_rows(rows, n_win: int, row_length: int) -> np.ndarray:
    """Host rows, (count, n_win) or (count, row_length) as `rows()` crops them (or one row), as
    C-contiguous float32 of n_win columns."""
    r = np.asarray(rows, dtype=np.float32)
    r = r.reshape(-1, r.shape[-1])
    if r.shape[1] != n_win:
        if r.shape[1] != row_length:
            raise ValueError("rows must be n_win or row_length wide")
        full = np.full((r.shape[0], n_win), np.nan, dtype=np.float32)  # the tail is never read
        full[:, :r.shape[1]] = r
        r = full
    return np.ascontiguousarray(r)


# in_dtype name -> (zfft_config.in_dtype, numpy element type of the host array)
IN_DTYPES = {"complex64": (0, np.complex64), "complex32": (1, np.float16), "cu8": (2, np.uint8),
             "f32": (3, np.float32)}


class ZoomFFT:
    """A plan: IQ frames -> dB rows (+ the on-device waterfall ring)."""

    def __init__(self, n_fft: int, zoom: int, fs: float, n_win: int | None = None,
                 window="hamming", f_lo: float = 1.0, scroll: int = 1, device: int = 0,
                 in_dtype: str = "complex64", flip: bool = False, average: str = "mean",
                 segments_per_line: int = 0):
        """in_dtype: "complex64" (complex ndarray), "complex32" (float16 interleaved I,Q,
        shape (..., 2L)), "cu8" (RTL-SDR uint8 interleaved I,Q, value b/127.5 - 1) or "f32"
        (real samples, AudioPan; at zoom 1 the rows are one-sided and `row_length` long).
        flip: reverse every frame on load (the sources' np.flip, S:541-543).
        average: the Welch detector over a frame's segments, see `set_average`.
        segments_per_line: Welch segments per waterfall line, see `set_segments_per_line`."""
        self.lib = _lib.load()
        if average not in _lib.AVERAGES:
            raise ValueError(f"average must be one of {sorted(_lib.AVERAGES)}")
        if in_dtype not in IN_DTYPES:
            raise ValueError(f"in_dtype must be one of {sorted(IN_DTYPES)}")
        self.in_dtype, self.flip = in_dtype, bool(flip)
        self.n_fft, self.zoom, self.fs, self.f_lo = int(n_fft), int(zoom), float(fs), float(f_lo)
        self.n_win = int(n_win) if n_win is not None else self.n_fft // self.zoom
        kind, params, arr = _window_spec(window)
        cfg = zfft_config()
        cfg.n_fft, cfg.zoom, cfg.n_win, cfg.window_kind = self.n_fft, self.zoom, self.n_win, kind
        cfg.fs, cfg.f_lo = self.fs, self.f_lo
        cfg.window_param[0], cfg.window_param[1] = params
        cfg.scroll, cfg.device = int(scroll), int(device)
        cfg.in_dtype, cfg.flip_input = IN_DTYPES[in_dtype][0], int(self.flip)
        if arr is not None and arr.size != self.n_fft:
            raise ValueError("array window must have length n_fft (welch nperseg)")
        self._window_array = arr  # kept alive for the call
        self._plan = ctypes.c_void_p()
        check(self.lib.zfft_plan_create(ctypes.byref(cfg),
                                        arr.ctypes.data_as(ctypes.c_void_p) if arr is not None else None,
                                        ctypes.byref(self._plan)), "zfft_plan_create")
        self.scroll = int(scroll)
        self.device = int(device)
        self.average = "mean"
        if average != "mean":
            self.set_average(average)
        self.segments_per_line = 0
        if segments_per_line:
            self.set_segments_per_line(segments_per_line)

    # ---------------------------------------------------------------- lifetime
    def close(self):
        if getattr(self, "_plan", None) and self._plan.value:
            self.lib.zfft_plan_destroy(self._plan)
            self._plan = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def tune(self, block: int = 0, warmup: int = 0):
        check(self.lib.zfft_plan_tune(self._plan, int(block), int(warmup)), "zfft_plan_tune")

    def set_timing(self, enable: bool) -> None:
        check(self.lib.zfft_plan_timing(self._plan, int(bool(enable))), "zfft_plan_timing")

    def timings(self) -> list:
        """Per-launch ms of the last process call (needs set_timing(True)), in launch order,
        one per name of `launch_names()`: XA schedule [xa_stage_mix, xa_stage, ..., welch_rows
        | welch4 (median / max: welch_segs | welch4_segs, then welch_select; with segments_per_line whatever the plan ran for the lines)]; blocked schedules a forward and a backward pass per stage; a batched host
        call repeats the sequence per batch after a "batch_wait" interval."""
        buf = (ctypes.c_float * 1024)()
        n = ctypes.c_int32()
        check(self.lib.zfft_plan_timings(self._plan, buf, 1024, ctypes.byref(n)), "zfft_plan_timings")
        return [float(buf[i]) for i in range(n.value)]

    def launch_names(self) -> list:
        """Names of the intervals `timings()` returns (from the last timed call)."""
        raw = self.lib.zfft_plan_timing_names(self._plan) or b""
        return [n for n in raw.decode().split(",") if n]

    def set_path(self, path: int) -> None:
        """0 auto, 1 exact reference pass order (blocked; the auto choice for small batches,
        e.g. one frame per call), 2 fused interior + exact edges (blocked; auto from 2^27
        samples per call), 3 XA tiles (all-pole + FIR + half-rate all-pole, one wave per
        frame; auto for >= 768 frames, or >= 384 frames of <= 2^19 samples), 4 PC polyphase
        cascade tiles (zoom 8, frames >= 16384 samples; the auto choice there below 4096
        frames per call), 5 the PC walk (one workgroup per frame; zoom 8: auto from 4096
        frames; zoom 4: the two-stage walk, on request only -- XA is faster there; path 4 at
        zoom 4 is its tiles, automatic below 1024 frames per call; at zoom 2, 4 and 5 are
        one-stage tiles in XA's factorisation, automatic below 512).  At zoom
        >= 16, 4 / 5 run PC for the first three stages and XA for the rest; automatic wherever
        XA would take the batch.  6 FC, fast convolution in 8192-sample windows (zoom 8, zoom 4
        and the head of zoom >= 16; automatic from 16 / 32 frames per call; elsewhere as 5).
        7 FC wherever a form exists, on request only: as 6, plus zoom 2 (the one-stage model
        truncated at |k| <= 256, within 5.4e-7 of the float64 reference's decimated IQ) and, at
        zoom >= 16, FC launches for the stages after the head too while their input has
        >= 16384 samples (zoom 16 / 64 within 6.9e-7 / 7.6e-7 against 4e-6 with the other
        tails); frames of >= 16384 samples below 2^31 bytes, outside that as 6.  Times:
        DESIGN §3.9.1, profiles/r08fc2."""
        check(self.lib.zfft_plan_path(self._plan, int(path)), "zfft_plan_path")

    def set_welch(self, mode: int) -> None:
        """0 auto, 1 one workgroup per frame (n_fft <= 16384), 2 four-step (n_fft >= 4096)."""
        check(self.lib.zfft_plan_welch(self._plan, int(mode)), "zfft_plan_welch")

    def set_average(self, average: str) -> None:
        """How a frame's Welch segments combine into its row (zfft_plan_average): "mean"
        (scipy.signal.welch's default, the reference's call), "median"
        (scipy.signal.welch(average='median'): the bias-corrected median, which an impulse in a
        few segments does not lift) or "max" (peak hold over the frame's segments, for
        transmissions shorter than a frame).  Holds for every later call, `IQRing.process`
        included, until changed."""
        if average not in _lib.AVERAGES:
            raise ValueError(f"average must be one of {sorted(_lib.AVERAGES)}")
        check(self.lib.zfft_plan_average(self._plan, _lib.AVERAGES[average]), "zfft_plan_average")
        self.average = average

    def set_segments_per_line(self, g: int) -> None:
        """Time-resolved waterfall (zfft_plan_segments_per_line): 0, the default, gives one row
        per frame; g >= 1 gives `lines(n_samples)` = ceil(nseg / g) rows per frame in time order,
        each the plan's detector over g consecutive Welch segments (the last over the rest).
        g = 1 is scipy.signal.spectrogram's columns through the reference's crop and dB;
        g >= nseg is the one row of g = 0.  Holds for every later call until changed."""
        check(self.lib.zfft_plan_segments_per_line(self._plan, int(g)), "zfft_plan_segments_per_line")
        self.segments_per_line = int(g)

    def lines(self, n_samples: int) -> int:
        """Rows per frame of n_samples input samples (zfft_line_count); 1 at g = 0."""
        n = self.lib.zfft_line_count(int(n_samples), self.zoom, self.n_fft, self.segments_per_line)
        if n < 1:
            raise ValueError(f"zfft_line_count: bad arguments (n_samples {n_samples})")
        return int(n)

    def line_times(self, n_samples: int) -> np.ndarray:
        """Centre time of each of the frame's lines, seconds from its first sample
        (zfft_line_times: scipy.signal.spectrogram's t at the input rate, averaged per line)."""
        n = self.lines(n_samples)
        t = np.empty(n, dtype=np.float64)
        got = ctypes.c_int32()
        check(self.lib.zfft_line_times(int(n_samples), self.zoom, self.n_fft, self.fs,
                                       self.segments_per_line, t.ctypes.data_as(ctypes.c_void_p), n,
                                       ctypes.byref(got)), "zfft_line_times")
        return t[:got.value]

    def set_lo_frames(self, f_lo, frames_per_lo: int = 1) -> None:
        """Batched multi-IF (config 4): frame f of each call is mixed with
        f_lo[(f // frames_per_lo) % len(f_lo)] (the reference's f_demod per IF, S:2090);
        an empty list restores the plan's f_lo.  Zoom 1 never mixes (S:2108): several
        rows raise ValueError there."""
        arr = np.ascontiguousarray(f_lo, dtype=np.float64).ravel()
        check(self.lib.zfft_plan_set_lo_frames(self._plan, arr.ctypes.data_as(ctypes.c_void_p) if arr.size else None,
                                               int(arr.size), int(frames_per_lo)), "zfft_plan_set_lo_frames")
        if arr.size == 1:
            self.f_lo = float(arr[0])

    # ---------------------------------------------------------------- DSP
    def _as_iq(self, x) -> np.ndarray:
        """The caller's frames in the plan's input format, C-contiguous; the last axis holds
        L complex samples (complex64) or 2L interleaved I,Q values (complex32, cu8)."""
        x = np.asarray(x)
        dt = IN_DTYPES[self.in_dtype][1]
        if self.in_dtype == "complex64":
            if x.dtype != dt:
                x = x.astype(dt)
        elif self.in_dtype == "f32":
            if np.iscomplexobj(x):
                raise ValueError("f32 input must be real")
            x = x.astype(dt, copy=False)
        elif x.dtype != dt or x.shape[-1] % 2:
            raise ValueError(f"{self.in_dtype} input must be {np.dtype(dt).name} with "
                             "interleaved I,Q on the last axis")
        return np.ascontiguousarray(x)

    def _samples(self, x) -> int:
        return x.shape[-1] if self.in_dtype in ("complex64", "f32") else x.shape[-1] // 2

    @property
    def row_length(self) -> int:
        """Valid floats per row: n_win, or the one-sided slice for real input at zoom 1."""
        n = self.lib.zfft_plan_row_length(self._plan)
        if n < 0:
            check(n, "zfft_plan_row_length")
        return n

    def rows(self, frames) -> np.ndarray:
        """(F, L) or (L,) complex IQ -> (F, W) or (W,) float32 dB rows; with
        segments_per_line >= 1, (F, R, W) or (R, W): the R = lines(L) lines of each frame."""
        x = self._as_iq(frames)
        single = x.ndim == 1
        x2 = x.reshape(1, -1) if single else x
        F, L = x2.shape[0], self._samples(x2)
        by_line = self.segments_per_line >= 1
        R = self.lines(L) if by_line else 1
        out = np.empty((F * R, self.n_win), dtype=np.float32)
        check(self.lib.zfft_process(self._plan, x2.ctypes.data_as(ctypes.c_void_p), L, F,
                                    out.ctypes.data_as(ctypes.c_void_p)), "zfft_process")
        n = self.row_length
        if n != self.n_win:  # one-sided rows (real input at zoom 1)
            out = np.ascontiguousarray(out[:, :n])
        if by_line:
            out = out.reshape(F, R, -1)
        return out[0] if single else out

    def process_host(self, iq_ptr: int, n_samples: int, n_frames: int, rows_ptr: int) -> None:
        """zfft_process on raw host pointers (e.g. a pinned torch tensor's data_ptr()): frames in
        the plan's input format, rows n_frames * R * n_win floats (R = lines(n_samples); 1 without
        segments_per_line).  Synchronous; large inputs go in
        batches whose H2D copy overlaps the previous batch's compute."""
        check(self.lib.zfft_process(self._plan, ctypes.c_void_p(iq_ptr), int(n_samples),
                                    int(n_frames), ctypes.c_void_p(rows_ptr)), "zfft_process")

    def process_device(self, d_iq_ptr: int, n_samples: int, n_frames: int, d_rows_ptr: int,
                       stream: int = 0) -> None:
        """Device pointers (e.g. torch .data_ptr()); enqueued on `stream`, no sync.  The row
        buffer holds n_frames * R * n_win floats (R = lines(n_samples); 1 without
        segments_per_line) and is taken on trust."""
        check(self.lib.zfft_process_device(self._plan, ctypes.c_void_p(d_iq_ptr), int(n_samples),
                                           int(n_frames), ctypes.c_void_p(d_rows_ptr),
                                           ctypes.c_void_p(stream or None)), "zfft_process_device")

    def decimate(self, x) -> np.ndarray:
        """zoomfft(x, zoom) of the reference (S:2088-2100) -> complex64."""
        x = self._as_iq(x).ravel()
        L = self._samples(x)
        m = self.lib.zfft_decimated_length(L, self.zoom)
        out = np.empty(max(m, 1), dtype=np.complex64)
        n_out = ctypes.c_int64()
        check(self.lib.zfft_decimate(self._plan, x.ctypes.data_as(ctypes.c_void_p), L,
                                     out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_out)),
              "zfft_decimate")
        return out[:n_out.value]

    def decimate_frames(self, frames) -> np.ndarray:
        """`decimate` of every frame of an (F, L) batch in one call -> (F, m) complex64, on the
        schedule F frames per call earn (one workgroup per frame from 1024 frames: `set_path`)."""
        x = self._as_iq(frames)
        if x.ndim != 2:
            raise ValueError("frames must be (F, L)")
        F, L = x.shape[0], self._samples(x)
        m = self.lib.zfft_decimated_length(L, self.zoom)
        out = np.empty((F, max(m, 1)), dtype=np.complex64)
        n_out = ctypes.c_int64()
        check(self.lib.zfft_decimate_frames(self._plan, x.ctypes.data_as(ctypes.c_void_p), L, F,
                                            out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_out)),
              "zfft_decimate_frames")
        return out[:, :n_out.value]

    # ---------------------------------------------------------------- waterfall
    def waterfall_push(self, row=None) -> None:
        if row is None:
            check(self.lib.zfft_waterfall_push(self._plan, None), "zfft_waterfall_push")
            return
        r = np.ascontiguousarray(row, dtype=np.float32)
        if r.size != self.n_win:
            raise ValueError("row length must equal n_win")
        check(self.lib.zfft_waterfall_push(self._plan, r.ctypes.data_as(ctypes.c_void_p)),
              "zfft_waterfall_push")

    def waterfall_push_device(self, d_rows_ptr: int, count: int, stream: int = 0) -> None:
        check(self.lib.zfft_waterfall_push_device(self._plan, ctypes.c_void_p(d_rows_ptr),
                                                  int(count), ctypes.c_void_p(stream or None)),
              "zfft_waterfall_push_device")

    def waterfall_shape(self):
        h, w = ctypes.c_int32(), ctypes.c_int32()
        check(self.lib.zfft_waterfall_shape(self._plan, ctypes.byref(h), ctypes.byref(w)),
              "zfft_waterfall_shape")
        return h.value, w.value

    def waterfall_image(self) -> np.ndarray:
        h, w = self.waterfall_shape()
        img = np.empty((h, w), dtype=np.float32)
        check(self.lib.zfft_waterfall_read(self._plan, img.ctypes.data_as(ctypes.c_void_p)),
              "zfft_waterfall_read")
        return img

    def waterfall_reset(self, scroll: int) -> None:
        """Waterfall.init_image with a (possibly new) scroll direction (S:1625-1636, 2074-2077)."""
        check(self.lib.zfft_waterfall_reset(self._plan, int(scroll)), "zfft_waterfall_reset")
        self.scroll = int(scroll)

    # ---------------------------------------------------------------- rendering (§8f-2)
    def waterfall_colormap(self, name: str) -> None:
        """Waterfall.lookuptable (S:1611-1623): unknown names fall back to 'Default'."""
        check(self.lib.zfft_waterfall_colormap(self._plan, str(name).encode()), "zfft_waterfall_colormap")

    def waterfall_levels(self, low: float | None = None, high: float | None = None):
        """Waterfall.newlevel (S:1680-1684) when given; returns the current (low, high)."""
        if low is not None:
            check(self.lib.zfft_waterfall_levels(self._plan, float(low), float(high)),
                  "zfft_waterfall_levels")
        lo, hi = ctypes.c_double(), ctypes.c_double()
        check(self.lib.zfft_waterfall_get_levels(self._plan, ctypes.byref(lo), ctypes.byref(hi)),
              "zfft_waterfall_get_levels")
        return lo.value, hi.value

    def waterfall_autolevel(self):
        """Waterfall.autolevel (S:1667-1678) as intended: levels = percentiles 2, 98 of the
        pixels below 0, computed on the device; returns (low, high)."""
        lo, hi = ctypes.c_double(), ctypes.c_double()
        check(self.lib.zfft_waterfall_autolevel(self._plan, ctypes.byref(lo), ctypes.byref(hi)),
              "zfft_waterfall_autolevel")
        return lo.value, hi.value

    def waterfall_render(self, out: np.ndarray | None = None) -> np.ndarray:
        """RGBA uint8 (H, W, 4): the pixels pyqtgraph's ImageItem draws for the ring image.

        Without `out` the image lands in one of two page-locked buffers the engine owns and
        uses in turn (the D2H copy then runs at PCIe DMA rate; a pageable array is staged
        through the runtime's bounce buffer at a fraction of it): the returned array stays
        valid until the render after next -- what `setImage` each line needs.  Pass `out`
        (any C-contiguous (H, W, 4) uint8 array; page-locked from `pinned_empty` for speed)
        to keep an image longer."""
        h, w = self.waterfall_shape()
        if out is None:
            slots = getattr(self, "_render_slots", None)
            if not slots or slots[0].shape != (h, w, 4):
                slots = self._render_slots = [pinned_empty((h, w, 4), np.uint8) for _ in range(2)]
                self._render_k = 0
            out = slots[self._render_k % 2]
            self._render_k += 1
        elif out.shape != (h, w, 4) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous uint8 array of shape {(h, w, 4)}")
        check(self.lib.zfft_waterfall_render(self._plan, out.ctypes.data_as(ctypes.c_void_p)),
              "zfft_waterfall_render")
        return out

    def waterfall_push_emit(self, rows, f64: bool, out: np.ndarray | None = None) -> np.ndarray:
        """`rows` ((count, n_win) float32 host rows, or None) pushed, then the image in one
        round trip (zfft_waterfall_push_render / _push_read64): RGBA uint8 (H, W, 4), or the
        float64 (H, W) image when `f64`.  Without `out` the image lands in one of two
        page-locked buffers the engine owns and uses in turn, valid until the call after next
        (as waterfall_render); pass `out` to keep one.  (The per-line display path: kept to a
        few attribute reads and two integer pointers on the Python side.)"""
        st = self.__dict__.get("_emit_state")
        if st is None:
            h, w = self.waterfall_shape()  # fixed per plan (n_win / 4 x n_win)
            st = self._emit_state = {
                True: [[pinned_empty((h, w), np.float64) for _ in range(2)], 0, (h, w), np.float64,
                       self.lib.zfft_waterfall_push_read64, "zfft_waterfall_push_read64"],
                False: [[pinned_empty((h, w, 4), np.uint8) for _ in range(2)], 0, (h, w, 4), np.uint8,
                        self.lib.zfft_waterfall_push_render, "zfft_waterfall_push_render"],
                "w": w}
        slot = st[bool(f64)]
        if out is None:
            out = slot[0][slot[1] & 1]
            slot[1] += 1
        elif out.shape != slot[2] or out.dtype != slot[3] or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous {np.dtype(slot[3]).name} array of shape {slot[2]}")
        if rows is None:
            count, ptr = 0, None
        else:
            r = rows if (rows.dtype == np.float32 and rows.flags.c_contiguous) else \
                np.ascontiguousarray(rows, dtype=np.float32)
            count, ptr = r.size // st["w"], r.ctypes.data
        check(slot[4](self._plan, ptr, count, out.ctypes.data), slot[5])
        return out

    def waterfall_render_device(self, d_rgba_ptr: int, stream: int = 0) -> None:
        """RGBA8 pixels of the ring into device memory (H*W*4 bytes), enqueued on `stream`."""
        check(self.lib.zfft_waterfall_render_device(self._plan, ctypes.c_void_p(d_rgba_ptr),
                                                    ctypes.c_void_p(stream or None)),
              "zfft_waterfall_render_device")

    # ---------------------------------------------------------------- persistence spectrum
    def set_persistence(self, levels: int, db_min: float = 0.0, db_max: float = 0.0) -> None:
        """The persistence (digital-phosphor) table (zfft_plan_persistence): per column a
        histogram of the pushed rows' levels, `levels` (2..256) equal steps from db_min (level 0)
        up to, not including, db_max; values outside, NaN and infinities are counted nowhere.
        Zeroes the table; levels = 0 turns it off and frees it.  The binning rule is in
        include/zfft.h, bit for bit reproducible in numpy float32."""
        check(self.lib.zfft_plan_persistence(self._plan, int(levels), float(db_min), float(db_max)),
              "zfft_plan_persistence")

    def persistence_shape(self):
        lv, w = ctypes.c_int32(), ctypes.c_int32()
        check(self.lib.zfft_persistence_shape(self._plan, ctypes.byref(lv), ctypes.byref(w)),
              "zfft_persistence_shape")
        return lv.value, w.value

    def persistence_push(self, rows) -> None:
        """Host rows, (count, n_win) or (count, row_length) as `rows()` crops them (or one row),
        binned into the table; synchronous."""
        r = full_rows(rows, self.n_win, self.row_length)
        check(self.lib.zfft_persistence_push(self._plan, r.ctypes.data_as(ctypes.c_void_p), r.shape[0]),
              "zfft_persistence_push")

    def persistence_push_device(self, d_rows_ptr: int, count: int, stream: int = 0) -> None:
        """`count` device rows of n_win floats (e.g. what process_device wrote), enqueued on
        `stream`, no sync."""
        check(self.lib.zfft_persistence_push_device(self._plan, ctypes.c_void_p(d_rows_ptr), int(count),
                                                    ctypes.c_void_p(stream or None)),
              "zfft_persistence_push_device")

    def persistence_decay(self, keep: float) -> None:
        """Every count c becomes floor(c * keep), rows_seen likewise; 0 <= keep <= 1."""
        check(self.lib.zfft_persistence_decay(self._plan, float(keep)), "zfft_persistence_decay")

    def persistence_reset(self) -> None:
        check(self.lib.zfft_persistence_reset(self._plan), "zfft_persistence_reset")

    def persistence(self):
        """(hist, rows_seen): uint32 counts of shape (levels, n_win), level 0 the lowest, and the
        number of rows pushed since the last reset (scaled by the decays)."""
        hist = np.empty(self.persistence_shape(), dtype=np.uint32)
        seen = ctypes.c_uint64()
        check(self.lib.zfft_persistence_read(self._plan, hist.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.byref(seen)), "zfft_persistence_read")
        return hist, int(seen.value)

    def persistence_density(self) -> np.ndarray:
        """float64 hist / max(rows_seen, 1): the share of the rows a column spent in each level."""
        hist, seen = self.persistence()
        return hist / float(max(seen, 1))

    # ---------------------------------------------------------------- signal detection on rows
    def set_detect(self, quantile: float = 0.5, threshold_db: float = 12.0, min_width: int = 1,
                   max_per_row: int = 8) -> None:
        """The row detector (zfft_plan_detect): per row the noise floor (the value of rank
        floor(quantile (m - 1)) among its m finite values), the emissions (runs of at least
        `min_width` columns at or above floor + threshold_db, at most `max_per_row` (1..32)
        recorded per row) and a per-column occupancy count.  threshold_db is in row units,
        20 log10(PSD): a power ratio of 4 is 12.04.  Zeroes the occupancy; max_per_row = 0
        turns detection off.  The rule is in include/zfft.h, bit for bit reproducible in numpy."""
        check(self.lib.zfft_plan_detect(self._plan, float(quantile), float(threshold_db), int(min_width),
                                        int(max_per_row)), "zfft_plan_detect")

    def set_detect_local(self, half_window: int, guard: int = 0) -> None:
        """A local noise floor per column (zfft_plan_detect_local; order-statistic CFAR): column j
        is judged against the rank-floor(quantile (m - 1)) value of the finite rows' values in the
        `half_window` (1..128) columns beyond `guard` (0..128) columns on either side of it, cut
        at the row's ends, instead of the row's one floor.  half_window = 0 is the row-global
        floor again.  Detection must be on; zeroes the occupancy.  `detect` and `detect_device`
        follow the mode; the per-row `floor` they return stays the row-global one."""
        check(self.lib.zfft_plan_detect_local(self._plan, int(half_window), int(guard)), "zfft_plan_detect_local")

    def detect_local_shape(self):
        """(half_window, guard); (0, 0) with the row-global floor."""
        h, g = ctypes.c_int32(), ctypes.c_int32()
        check(self.lib.zfft_detect_local_shape(self._plan, ctypes.byref(h), ctypes.byref(g)),
              "zfft_detect_local_shape")
        return h.value, g.value

    def detect_floors(self, rows) -> np.ndarray:
        """float32 (count, n_win): the local floor of every column of host rows (as `detect`
        takes them), NaN where a column has no finite reference cell and at or beyond
        row_length; local mode only; synchronous.  No occupancy, no rows_seen."""
        r = full_rows(rows, self.n_win, self.row_length)
        out = np.empty_like(r)
        check(self.lib.zfft_detect_floors(self._plan, r.ctypes.data_as(ctypes.c_void_p), r.shape[0],
                                          out.ctypes.data_as(ctypes.c_void_p)), "zfft_detect_floors")
        return out

    def detect_floors_device(self, d_rows_ptr: int, count: int, d_floors_ptr: int, stream: int = 0) -> None:
        """`count` device rows of n_win floats into device floors of the same shape (columns at
        or beyond row_length are left untouched); enqueued on `stream`, no sync."""
        check(self.lib.zfft_detect_floors_device(self._plan, ctypes.c_void_p(d_rows_ptr), int(count),
                                                 ctypes.c_void_p(d_floors_ptr), ctypes.c_void_p(stream or None)),
              "zfft_detect_floors_device")

    def detect_shape(self):
        """(max_per_row, n_win)."""
        k, w = ctypes.c_int32(), ctypes.c_int32()
        check(self.lib.zfft_detect_shape(self._plan, ctypes.byref(k), ctypes.byref(w)), "zfft_detect_shape")
        return k.value, w.value

    def detect(self, rows):
        """Host rows, (count, n_win) or (count, row_length) as `rows()` crops them (or one row):
        (floor float32[count], found int32[count], events), events a structured array of shape
        (count, max_per_row) with fields first, last, peak, peak_db; synchronous."""
        K = self.detect_shape()[0]
        r = full_rows(rows, self.n_win, self.row_length)
        count = r.shape[0]
        floor = np.empty(count, dtype=np.float32)
        found = np.empty(count, dtype=np.int32)
        events = np.empty((count, K), dtype=EMISSION_DTYPE)
        check(self.lib.zfft_detect(self._plan, r.ctypes.data_as(ctypes.c_void_p), count,
                                   floor.ctypes.data_as(ctypes.c_void_p), found.ctypes.data_as(ctypes.c_void_p),
                                   events.ctypes.data_as(ctypes.c_void_p)), "zfft_detect")
        return floor, found, events

    def detect_device(self, d_rows_ptr: int, count: int, d_floor_ptr: int, d_found_ptr: int,
                      d_events_ptr: int, stream: int = 0) -> None:
        """`count` device rows of n_win floats (e.g. what process_device wrote) into device outputs:
        count floats, count int32 and count * max_per_row 16-byte records (16-byte aligned);
        enqueued on `stream`, no sync."""
        check(self.lib.zfft_detect_device(self._plan, ctypes.c_void_p(d_rows_ptr), int(count),
                                          ctypes.c_void_p(d_floor_ptr), ctypes.c_void_p(d_found_ptr),
                                          ctypes.c_void_p(d_events_ptr), ctypes.c_void_p(stream or None)),
              "zfft_detect_device")

    def detect_occupancy(self):
        """(occ, rows_seen): uint32 counts per column (n_win), how often each was part of an
        emission, and the rows given since the last reset."""
        occ = np.empty(self.n_win, dtype=np.uint32)
        seen = ctypes.c_uint64()
        check(self.lib.zfft_detect_occupancy(self._plan, occ.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.byref(seen)), "zfft_detect_occupancy")
        return occ, int(seen.value)

    def detect_reset(self) -> None:
        check(self.lib.zfft_detect_reset(self._plan), "zfft_detect_reset")

    # ---------------------------------------------------------------- emission tracks
    def set_track(self, gap: int = 0, slack: int = 0, min_rows: int = 1, max_tracks: int = 65536) -> None:
        """The emission tracker (zfft_plan_track): the detector's runs linked across rows on the
        device.  Runs at most `gap` + 1 rows apart (gap in [0, 7]) whose column ranges come
        within `slack` of each other (0: they share a column; at most 64) belong to one track; a
        track that no later row can reach is closed, reported when it spans at least `min_rows`
        rows and counted in `short_tracks` otherwise; at most `max_tracks` reported tracks wait
        for `tracks()`.  Detection must be on; max_tracks = 0 turns tracking off.  Resets the
        tracker.  The rule is in include/zfft.h, bit for bit reproducible in numpy."""
        check(self.lib.zfft_plan_track(self._plan, int(gap), int(slack), int(min_rows), int(max_tracks)),
              "zfft_plan_track")

    def track_shape(self):
        """(gap, slack, min_rows, max_tracks)."""
        v = [ctypes.c_int32() for _ in range(4)]
        check(self.lib.zfft_track_shape(self._plan, *[ctypes.byref(x) for x in v]), "zfft_track_shape")
        return tuple(x.value for x in v)

    def track_push(self, found, events) -> None:
        """The next rows' `found` (count int32) and `events` (count, max_per_row) as `detect`
        returned them, from the host; the records are checked against the detector's contract.
        Synchronous."""
        K = self.detect_shape()[0]
        f = np.ascontiguousarray(np.atleast_1d(found), dtype=np.int32)
        e = np.ascontiguousarray(events, dtype=EMISSION_DTYPE).reshape(-1, K)
        if f.ndim != 1 or e.shape[0] != f.shape[0]:
            raise ValueError(f"found must be (count,) and events (count, {K})")
        check(self.lib.zfft_track_push(self._plan, f.ctypes.data_as(ctypes.c_void_p),
                                       e.ctypes.data_as(ctypes.c_void_p), f.shape[0]), "zfft_track_push")

    def track_push_device(self, d_found_ptr: int, d_events_ptr: int, count: int, stream: int = 0) -> None:
        """The buffers `detect_device` wrote for `count` rows; enqueued on `stream`, no sync."""
        check(self.lib.zfft_track_push_device(self._plan, ctypes.c_void_p(d_found_ptr), ctypes.c_void_p(d_events_ptr),
                                              int(count), ctypes.c_void_p(stream or None)), "zfft_track_push_device")

    def _track_records(self, fn, name, max):
        out = np.empty(max, dtype=TRACK_DTYPE)
        n = ctypes.c_int32()
        check(fn(self._plan, out.ctypes.data_as(ctypes.c_void_p), int(max), ctypes.byref(n)), name)
        return out[:n.value].copy()

    def tracks(self, max: int | None = None) -> np.ndarray:
        """The reported tracks not yet read (at most `max`), in ascending (row_last, row_first,
        slot_first), as a TRACK_DTYPE array; they leave the store.  Waits for enqueued pushes."""
        if max is None:
            max = self.track_state()["unread"]
        return self._track_records(self.lib.zfft_track_read, "zfft_track_read", max)

    def open_tracks(self) -> np.ndarray:
        """The tracks still open, as they stand now, in ascending (row_first, slot_first)."""
        return self._track_records(self.lib.zfft_track_open, "zfft_track_open", 256)

    def track_flush(self) -> None:
        """Close every open track as it stands; later rows link to nothing earlier."""
        check(self.lib.zfft_track_flush(self._plan), "zfft_track_flush")

    def track_state(self) -> dict:
        """rows_seen, open, unread, dropped, short_tracks, truncated_rows."""
        v = (ctypes.c_uint64 * 6)()
        check(self.lib.zfft_track_state(self._plan, ctypes.cast(v, ctypes.c_void_p)), "zfft_track_state")
        return dict(zip(("rows_seen", "open", "unread", "dropped", "short_tracks", "truncated_rows"), map(int, v)))

    def track_reset(self) -> None:
        check(self.lib.zfft_track_reset(self._plan), "zfft_track_reset")

    # ---------------------------------------------------------------- channel taps
    def set_taps(self, max_taps: int, max_len: int = 2048) -> None:
        """Channel taps (zfft_plan_taps): up to `max_taps` (at most 64) digital down-converters on
        the plan's input samples, each an oscillator, a real FIR of at most `max_len` (at most
        2048) taps and an integer decimation, with their state on the device from push to push.
        The outputs do not depend on how the stream is cut into pushes, bit for bit.
        set_taps(0, 0) turns them off and frees them.  A call closes every tap and restarts the
        sample count.  The rule is in include/zfft.h, reproducible in numpy (tests/tap_ref.py)."""
        check(self.lib.zfft_plan_taps(self._plan, int(max_taps), int(max_len)), "zfft_plan_taps")
        self._tap_open = set()  # the open slots, mirrored here: a push asks the library once, not per slot

    def tap_shape(self):
        """(max_taps, max_len)."""
        m, n = ctypes.c_int32(), ctypes.c_int32()
        check(self.lib.zfft_tap_shape(self._plan, ctypes.byref(m), ctypes.byref(n)), "zfft_tap_shape")
        return m.value, n.value

    @staticmethod
    def _phase_word(f_hz: float, rate: float) -> int:
        """round(f_hz / rate * 2^32), wrapped into [-2^31, 2^31): the taps' and the bank's frequency words."""
        return (int(round(float(f_hz) / rate * 2.0 ** 32)) + 2 ** 31) % 2 ** 32 - 2 ** 31

    def _stretch(self, x, who: str):
        """A host push's 1-D stretch of samples in the plan's input format, and its sample count."""
        x = self._as_iq(x)
        if x.ndim != 1:
            raise ValueError(f"{who} takes a 1-D stretch of samples")
        return x, self._samples(x)

    def tap_freq_word(self, f_hz: float) -> int:
        """The freq_word nearest f_hz: round(f_hz / fs * 2^32), wrapped into [-2^31, 2^31)."""
        return self._phase_word(f_hz, self.fs)

    def tap_open(self, slot: int, f_hz: float, decim: int, taps=None, cutoff: float | None = None,
                 beta: float = 8.0) -> float:
        """Open (or replace) the tap in `slot` at centre frequency f_hz, decimating by `decim`
        (1 .. 512); returns the frequency actually used (a multiple of fs / 2^32).  taps: real
        FIR taps at the input rate; None designs a Kaiser-windowed sinc (`tap_design`) of
        min(8 decim + 1, max_len) taps, `cutoff` cycles per input sample (default 0.4 / decim)
        and `beta`.  The tap's first output is the first multiple of decim at or after the
        samples pushed so far, and it sees the input before that."""
        decim = int(decim)
        if taps is None:
            taps = tap_design(min(8 * decim + 1, self.tap_shape()[1]), 0.4 / decim if cutoff is None else cutoff, beta)
        h = np.ascontiguousarray(taps, dtype=np.float32).ravel()
        fw = self.tap_freq_word(f_hz)
        check(self.lib.zfft_tap_open(self._plan, int(slot), fw, decim, h.size, h.ctypes.data_as(ctypes.c_void_p)),
              "zfft_tap_open")
        self._tap_open.add(int(slot))
        return fw * self.fs / 2.0 ** 32

    def tap_close(self, slot: int) -> None:
        check(self.lib.zfft_tap_close(self._plan, int(slot)), "zfft_tap_close")
        self._tap_open.discard(int(slot))

    def tap_open_slots(self) -> list:
        """The open slots in ascending order: the order of `tap_push`'s arrays."""
        self.tap_shape()  # (ValueError while the taps are off)
        return sorted(self._tap_open)

    def tap_info(self, slot: int) -> dict:
        """open, freq_word, f_hz, decim, n_taps, n_open (the sample count at which it was opened)
        and group_delay ((n_taps - 1) / 2 input samples: reported, not compensated)."""
        o, d, t = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        fw, n0, gd = ctypes.c_int64(), ctypes.c_uint64(), ctypes.c_double()
        check(self.lib.zfft_tap_info(self._plan, int(slot), ctypes.byref(o), ctypes.byref(fw), ctypes.byref(d),
                                     ctypes.byref(t), ctypes.byref(n0), ctypes.byref(gd)), "zfft_tap_info")
        return {"open": bool(o.value), "freq_word": fw.value, "f_hz": fw.value * self.fs / 2.0 ** 32,
                "decim": d.value, "n_taps": t.value, "n_open": n0.value, "group_delay": gd.value}

    def tap_counts(self, n: int) -> np.ndarray:
        """Output samples per slot (closed: 0) of a push of n samples now; int64, max_taps long."""
        out = np.zeros(self.tap_shape()[0], dtype=np.int64)
        check(self.lib.zfft_tap_counts(self._plan, int(n), out.ctypes.data_as(ctypes.c_void_p)), "zfft_tap_counts")
        return out

    def tap_push(self, x) -> list:
        """The next samples of the stream (1-D, the plan's input format) from the host; returns
        one complex64 array per open slot, in slot order.  Synchronous."""
        x, n = self._stretch(x, "tap_push")
        counts = self.tap_counts(n)
        out = np.empty(int(counts.sum()), dtype=np.complex64)
        check(self.lib.zfft_tap_push(self._plan, x.ctypes.data_as(ctypes.c_void_p), n,
                                     out.ctypes.data_as(ctypes.c_void_p), None), "zfft_tap_push")
        ends = np.cumsum(counts)
        return [out[ends[s] - counts[s]:ends[s]] for s in sorted(self._tap_open)]

    def tap_push_device(self, d_iq_ptr: int, n: int, d_out_ptr: int, stream: int = 0) -> None:
        """n samples on the device; the outputs (sum of tap_counts(n) complex64, the open taps in
        slot order back to back) into d_out_ptr; enqueued on `stream`, no sync."""
        check(self.lib.zfft_tap_push_device(self._plan, ctypes.c_void_p(d_iq_ptr), int(n), ctypes.c_void_p(d_out_ptr),
                                            ctypes.c_void_p(stream or None)), "zfft_tap_push_device")

    def tap_state(self) -> int:
        """The input samples counted so far."""
        v = ctypes.c_uint64()
        check(self.lib.zfft_tap_state(self._plan, ctypes.byref(v)), "zfft_tap_state")
        return v.value

    def tap_reset(self, n0: int = 0) -> None:
        """Restart the sample count at n0 with an all-zero past; open taps stay open."""
        check(self.lib.zfft_tap_reset(self._plan, int(n0)), "zfft_tap_reset")

    # ---------------------------------------------------------------- channeliser
    def set_channels(self, n_chan: int, taps_per_channel: int = 8, oversample: int = 2, taps=None,
                     beta: float = 8.0) -> None:
        """Channeliser (zfft_plan_chan): a polyphase-FFT bank of `n_chan` uniform channels (a power
        of two in [8, 1024]) on the input samples, every channel fs / n_chan wide between its -6 dB
        edges and emitted at fs / decim, decim = n_chan / oversample (oversample 1 or 2).  taps:
        n_chan * taps_per_channel real prototype taps at the input rate; None designs
        `chan_design(n_chan, taps_per_channel, beta)`.  set_channels(0) turns it off and frees it.
        A call restarts the sample count with all channels selected.  The rule is in
        include/zfft.h, reproducible in numpy (tests/chan_ref.py)."""
        if int(n_chan) == 0:
            check(self.lib.zfft_plan_chan(self._plan, 0, 0, 0, None), "zfft_plan_chan")
            return
        if oversample not in (1, 2):
            raise ValueError("oversample is 1 (critically sampled) or 2")
        if taps is None:
            taps = chan_design(n_chan, taps_per_channel, beta)
        h = np.ascontiguousarray(taps, dtype=np.float32).ravel()
        if h.size != int(n_chan) * int(taps_per_channel):
            raise ValueError("taps: n_chan * taps_per_channel values")
        check(self.lib.zfft_plan_chan(self._plan, int(n_chan), int(taps_per_channel), int(n_chan) // oversample,
                                      h.ctypes.data_as(ctypes.c_void_p)), "zfft_plan_chan")

    def chan_shape(self):
        """(n_chan, taps_per_channel, decim, c_first, c_count)."""
        v = [ctypes.c_int32() for _ in range(5)]
        check(self.lib.zfft_chan_shape(self._plan, *[ctypes.byref(x) for x in v]), "zfft_chan_shape")
        return tuple(x.value for x in v)

    def chan_select(self, c_first: int, c_count: int) -> None:
        """Keep the channels (c_first + i) mod n_chan, i < c_count: (0, n_chan) is all of them in
        transform order, (n_chan / 2, n_chan) ascending frequency."""
        check(self.lib.zfft_chan_select(self._plan, int(c_first), int(c_count)), "zfft_chan_select")

    def chan_steps(self, n: int) -> int:
        """Output steps of a push of n samples now."""
        v = ctypes.c_int64()
        check(self.lib.zfft_chan_steps(self._plan, int(n), ctypes.byref(v)), "zfft_chan_steps")
        return v.value

    def chan_push(self, x) -> np.ndarray:
        """The next samples of the stream (1-D, the plan's input format) from the host; returns a
        (steps, c_count) complex64 array, one row per output step.  Synchronous."""
        x, n = self._stretch(x, "chan_push")
        out = np.empty((self.chan_steps(n), self.chan_shape()[4]), dtype=np.complex64)
        check(self.lib.zfft_chan_push(self._plan, x.ctypes.data_as(ctypes.c_void_p), n,
                                      out.ctypes.data_as(ctypes.c_void_p), None), "zfft_chan_push")
        return out

    def chan_push_device(self, d_iq_ptr: int, n: int, d_out_ptr: int, stream: int = 0) -> None:
        """n samples on the device; chan_steps(n) x c_count complex64 into d_out_ptr; enqueued on
        `stream`, no sync."""
        check(self.lib.zfft_chan_push_device(self._plan, ctypes.c_void_p(d_iq_ptr), int(n),
                                             ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(stream or None)),
              "zfft_chan_push_device")

    def chan_state(self) -> int:
        """The input samples counted so far."""
        v = ctypes.c_uint64()
        check(self.lib.zfft_chan_state(self._plan, ctypes.byref(v)), "zfft_chan_state")
        return v.value

    def chan_reset(self, n0: int = 0) -> None:
        """Restart the sample count at n0 with an all-zero past; the shape and selection stay."""
        check(self.lib.zfft_chan_reset(self._plan, int(n0)), "zfft_chan_reset")

    def chan_info(self) -> dict:
        """group_delay ((n_chan * taps_per_channel - 1) / 2 input samples: reported, not
        compensated) and rate_ratio (output samples per input sample, 1 / decim)."""
        gd, rr = ctypes.c_double(), ctypes.c_double()
        check(self.lib.zfft_chan_info(self._plan, ctypes.byref(gd), ctypes.byref(rr)), "zfft_chan_info")
        return {"group_delay": gd.value, "rate_ratio": rr.value}

    def chan_freqs(self) -> np.ndarray:
        """The centre of every kept channel in Hz in the samples' baseband (negative for the
        channels from n_chan / 2 on), in the order of chan_push's columns."""
        m, _, _, c0, k = self.chan_shape()
        c = (c0 + np.arange(k)) % m
        return np.where(c >= m // 2, c - m, c) * (self.fs / m)

    # ---------------------------------------------------------------- demodulator bank
    DEMOD_MODES = {"am": 0, "fm": 1, "ssb": 2, "power": 3}

    def set_demod(self, streams: int, taps=None, decim: int = 1) -> None:
        """Demodulator bank (zfft_plan_demod): AM, FM, SSB or power audio out of `streams` (at
        most 1024) complex baseband streams on the device -- what `chan_push_device` and
        `tap_push_device` write -- through one shared real audio FIR `taps` (at most 1024 taps;
        None designs `demod_design(8 * decim + 1, 0.4 / decim)`) decimating by `decim` (1 .. 64).
        set_demod(0) turns it off and frees it.  A call restarts the step count with every stream
        at AM.  The rule is in include/zfft.h, reproducible in numpy (tests/demod_ref.py)."""
        if int(streams) == 0:
            check(self.lib.zfft_plan_demod(self._plan, 0, 0, 0, None), "zfft_plan_demod")
            return
        if taps is None:
            check(self.lib.zfft_plan_demod(self._plan, int(streams), 0, int(decim), None), "zfft_plan_demod")
            return
        g = np.ascontiguousarray(taps, dtype=np.float32).ravel()
        check(self.lib.zfft_plan_demod(self._plan, int(streams), g.size, int(decim), g.ctypes.data_as(ctypes.c_void_p)),
              "zfft_plan_demod")

    def demod_shape(self):
        """(streams, n_taps, decim)."""
        v = [ctypes.c_int32() for _ in range(3)]
        check(self.lib.zfft_demod_shape(self._plan, *[ctypes.byref(x) for x in v]), "zfft_demod_shape")
        return tuple(x.value for x in v)

    def demod_mode(self, mode, bfo_hz: float = 0.0, rate: float | None = None, first: int = 0,
                   count: int | None = None) -> float:
        """Streams [first, first + count) (default: all from `first`) to `mode` ("am", "fm", "ssb",
        "power" or a ZFFT_DEMOD_* value); bfo_hz is SSB's beat frequency at the streams' sample
        rate `rate` (default: the plan's fs), positive for USB and negative for LSB.  Returns the
        frequency actually used, a multiple of rate / 2^32.  Applies to the next push, carried
        window included."""
        m = self.DEMOD_MODES[mode.lower()] if isinstance(mode, str) else int(mode)
        rate = self.fs if rate is None else float(rate)
        word = self._phase_word(bfo_hz, rate)
        if count is None:
            count = self.demod_shape()[0] - int(first)
        check(self.lib.zfft_demod_mode(self._plan, int(first), int(count), m, word), "zfft_demod_mode")
        return word * rate / 2.0 ** 32

    def demod_steps(self, steps: int) -> int:
        """Outputs of a push of `steps` steps now."""
        v = ctypes.c_int64()
        check(self.lib.zfft_demod_steps(self._plan, int(steps), ctypes.byref(v)), "zfft_demod_steps")
        return v.value

    def demod_push(self, x) -> np.ndarray:
        """The next steps of the streams from the host: complex64, (steps, streams) or, for one
        stream, 1-D; returns (outputs, streams) float32.  Synchronous."""
        k = self.demod_shape()[0]
        x = np.ascontiguousarray(x, dtype=np.complex64)
        if x.ndim == 1 and k == 1:
            x = x.reshape(-1, 1)
        if x.ndim != 2 or x.shape[1] != k:
            raise ValueError("demod_push takes (steps, streams) complex64, or 1-D for one stream")
        out = np.empty((self.demod_steps(x.shape[0]), k), dtype=np.float32)
        check(self.lib.zfft_demod_push(self._plan, x.ctypes.data_as(ctypes.c_void_p), x.shape[0], k, 1,
                                       out.ctypes.data_as(ctypes.c_void_p), None), "zfft_demod_push")
        return out

    def demod_push_device(self, d_x_ptr: int, steps: int, step_stride: int, stream_stride: int, d_out_ptr: int,
                          stream: int = 0) -> None:
        """`steps` steps on the device, stream s at step n at complex64 index n * step_stride +
        s * stream_stride ((streams, 1) for chan_push_device's output, (1, count) for taps written
        back to back); demod_steps(steps) x streams float32 into d_out_ptr; enqueued on `stream`,
        no sync."""
        check(self.lib.zfft_demod_push_device(self._plan, ctypes.c_void_p(d_x_ptr), int(steps), int(step_stride),
                                              int(stream_stride), ctypes.c_void_p(d_out_ptr),
                                              ctypes.c_void_p(stream or None)), "zfft_demod_push_device")

    def demod_state(self) -> int:
        """The steps counted so far."""
        v = ctypes.c_uint64()
        check(self.lib.zfft_demod_state(self._plan, ctypes.byref(v)), "zfft_demod_state")
        return v.value

    def demod_reset(self, n0: int = 0) -> None:
        """Restart the step count at n0 with an all-zero past; the shape and the modes stay."""
        check(self.lib.zfft_demod_reset(self._plan, int(n0)), "zfft_demod_reset")

    def demod_info(self) -> dict:
        """group_delay ((n_taps - 1) / 2 steps: reported, not compensated) and rate_ratio (outputs
        per step, 1 / decim)."""
        gd, rr = ctypes.c_double(), ctypes.c_double()
        check(self.lib.zfft_demod_info(self._plan, ctypes.byref(gd), ctypes.byref(rr)), "zfft_demod_info")
        return {"group_delay": gd.value, "rate_ratio": rr.value}

    # ---------------------------------------------------------------- resampler bank
    RESAMP_FORMATS = {"f32": 0, "s16": 1}

    def set_resamp(self, lanes: int, L: int = 1, M: int = 1, taps=None, taps_per_phase: int | None = None,
                   format="f32", scale: float = 32767.0) -> None:
        """Resampler bank (zfft_plan_resamp): `lanes` (at most 2048) real float32 lanes on the
        device -- what `demod_push_device` writes, or a complex stream as two lanes -- at L / M
        times their rate (the fraction is reduced; then L <= 512, M <= 4096), through one shared
        real prototype `taps` of L * taps_per_phase values at the upsampled rate (None designs
        `resamp_design(L, M, 16 * ceil(max(L, M) / L))`), as "f32" or as "s16": int16
        clamp(rint(y * scale)).  set_resamp(0) turns it off and frees it.  A call restarts the step
        count.  The rule is in include/zfft.h, reproducible in numpy (tests/resamp_ref.py)."""
        if int(lanes) == 0:
            check(self.lib.zfft_plan_resamp(self._plan, 0, 0, 0, 0, None, 0, 0.0), "zfft_plan_resamp")
            return
        fmt = self.RESAMP_FORMATS[format.lower()] if isinstance(format, str) else int(format)
        g = math.gcd(int(L), int(M))
        L, M = (int(L) // g, int(M) // g) if g else (int(L), int(M))
        if taps is None:
            check(self.lib.zfft_plan_resamp(self._plan, int(lanes), L, M, int(taps_per_phase or 0), None, fmt, float(scale)),
                  "zfft_plan_resamp")
            return
        h = np.ascontiguousarray(taps, dtype=np.float32).ravel()
        if taps_per_phase is None:
            taps_per_phase = h.size // max(L, 1)
        if h.size != L * int(taps_per_phase):
            raise ValueError("taps: L * taps_per_phase values (L of the reduced fraction)")
        check(self.lib.zfft_plan_resamp(self._plan, int(lanes), L, M, int(taps_per_phase), h.ctypes.data_as(ctypes.c_void_p),
                                        fmt, float(scale)), "zfft_plan_resamp")

    def resamp_shape(self):
        """(lanes, L, M, taps_per_phase, format)."""
        v = [ctypes.c_int32() for _ in range(5)]
        check(self.lib.zfft_resamp_shape(self._plan, *[ctypes.byref(x) for x in v]), "zfft_resamp_shape")
        return tuple(x.value for x in v)

    def resamp_steps(self, steps: int) -> int:
        """Outputs of a push of `steps` steps now."""
        v = ctypes.c_int64()
        check(self.lib.zfft_resamp_steps(self._plan, int(steps), ctypes.byref(v)), "zfft_resamp_steps")
        return v.value

    def resamp_push(self, x) -> np.ndarray:
        """The next steps of the lanes from the host: (steps, lanes) float32 (1-D for one lane), or
        (steps, lanes / 2) complex64 (1-D for two lanes); returns (outputs, lanes) float32 or int16,
        or (outputs, lanes / 2) complex64 for complex input of a float32 bank.  Synchronous."""
        k, _, _, _, fmt = self.resamp_shape()
        x = np.asarray(x)
        cplx = np.iscomplexobj(x)
        x = np.ascontiguousarray(x, dtype=np.complex64 if cplx else np.float32)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        if x.ndim != 2 or x.shape[1] * (2 if cplx else 1) != k:
            raise ValueError("resamp_push takes (steps, lanes) float32 or (steps, lanes / 2) complex64")
        out = np.empty((self.resamp_steps(x.shape[0]), k), dtype=np.int16 if fmt == 1 else np.float32)
        check(self.lib.zfft_resamp_push(self._plan, x.ctypes.data_as(ctypes.c_void_p), x.shape[0], k,
                                        out.ctypes.data_as(ctypes.c_void_p), None), "zfft_resamp_push")
        return out.view(np.complex64) if cplx and fmt == 0 else out

    def resamp_push_device(self, d_x_ptr: int, steps: int, step_stride: int, d_out_ptr: int, stream: int = 0) -> None:
        """`steps` steps on the device, lane s at step n at float32 index n * step_stride + s
        ((streams, streams) for demod_push_device's output); resamp_steps(steps) x lanes float32 or
        int16 into d_out_ptr; enqueued on `stream`, no sync."""
        check(self.lib.zfft_resamp_push_device(self._plan, ctypes.c_void_p(d_x_ptr), int(steps), int(step_stride),
                                               ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(stream or None)),
              "zfft_resamp_push_device")

    def resamp_state(self) -> int:
        """The steps counted so far."""
        v = ctypes.c_uint64()
        check(self.lib.zfft_resamp_state(self._plan, ctypes.byref(v)), "zfft_resamp_state")
        return v.value

    def resamp_reset(self, n0: int = 0) -> None:
        """Restart the step count at n0 with an all-zero past; the shape and the taps stay."""
        check(self.lib.zfft_resamp_reset(self._plan, int(n0)), "zfft_resamp_reset")

    def resamp_info(self) -> dict:
        """group_delay ((taps_per_phase * L - 1) / (2 L) input steps: reported, not compensated)
        and rate_ratio (outputs per step, L / M)."""
        gd, rr = ctypes.c_double(), ctypes.c_double()
        check(self.lib.zfft_resamp_info(self._plan, ctypes.byref(gd), ctypes.byref(rr)), "zfft_resamp_info")
        return {"group_delay": gd.value, "rate_ratio": rr.value}

    # ---------------------------------------------------------------- level bank
    def set_level(self, lanes: int, block: int = 64, hold: int = 0, target: float = 0.5, gmax: float = 1e4,
                  floor: float = 1e-6, squelch: float = 0.0) -> None:
        """Level bank (zfft_plan_level): look-ahead gain control and squelch on `lanes` (at most
        2048) real float32 lanes on the device -- what `demod_push_device` writes -- between the
        demodulator and the resampler.  Per block of `block` steps (a power of two, 8 .. 1024) and
        lane, the gain is min(gmax, target / max(E, floor)), E the key's peak over the block and the
        `hold` (0 .. 4096) before it, 0 where E < squelch (squelch = 0: no squelch); it ramps over
        the block before a louder one, so the output stays within target, B to 2 B - 1 steps late.
        set_level(0) turns it off and frees it.  A call restarts the step count.  The rule is in
        include/zfft.h, reproducible in numpy (tests/level_ref.py)."""
        if int(lanes) == 0:
            check(self.lib.zfft_plan_level(self._plan, 0, 0, 0, 0.0, 0.0, 0.0, 0.0), "zfft_plan_level")
            return
        check(self.lib.zfft_plan_level(self._plan, int(lanes), int(block), int(hold), float(target), float(gmax),
                                       float(floor), float(squelch)), "zfft_plan_level")

    def level_shape(self):
        """(lanes, block, hold, target, gmax, floor, squelch), the four levels as float32 took them."""
        v = [ctypes.c_int32() for _ in range(3)] + [ctypes.c_float() for _ in range(4)]
        check(self.lib.zfft_level_shape(self._plan, *[ctypes.byref(x) for x in v]), "zfft_level_shape")
        return tuple(x.value for x in v)

    def level_steps(self, steps: int) -> int:
        """Steps a push of `steps` steps now would emit."""
        v = ctypes.c_int64()
        check(self.lib.zfft_level_steps(self._plan, int(steps), ctypes.byref(v)), "zfft_level_steps")
        return v.value

    def level_push(self, x, key=None) -> np.ndarray:
        """The next steps of the lanes from the host: (steps, lanes) float32 (1-D for one lane), and
        optionally a key of the same shape the gains are taken from; returns (emitted, lanes)
        float32.  Synchronous."""
        k = self.level_shape()[0]
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        if x.ndim != 2 or x.shape[1] != k:
            raise ValueError("level_push takes (steps, lanes) float32")
        kp = None
        if key is not None:
            key = np.ascontiguousarray(key, dtype=np.float32)
            if key.reshape(-1, 1).shape == x.shape:
                key = key.reshape(-1, 1)
            if key.shape != x.shape:
                raise ValueError("level_push: the key has the samples' shape")
            kp = key.ctypes.data_as(ctypes.c_void_p)
        out = np.empty((self.level_steps(x.shape[0]), k), dtype=np.float32)
        check(self.lib.zfft_level_push(self._plan, x.ctypes.data_as(ctypes.c_void_p), kp, x.shape[0], k,
                                       out.ctypes.data_as(ctypes.c_void_p), None), "zfft_level_push")
        return out

    def level_push_device(self, d_x_ptr: int, steps: int, step_stride: int, d_out_ptr: int, d_key_ptr: int = 0,
                          key_stride: int = 0, stream: int = 0) -> None:
        """`steps` steps on the device, lane s at step n at float32 index n * step_stride + s
        ((streams, streams) for demod_push_device's output), the key (0: the samples themselves)
        at n * key_stride + s; level_steps(steps) x lanes float32 into d_out_ptr; enqueued on
        `stream`, no sync."""
        check(self.lib.zfft_level_push_device(self._plan, ctypes.c_void_p(d_x_ptr), int(steps), int(step_stride),
                                              ctypes.c_void_p(d_key_ptr or None), int(key_stride),
                                              ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(stream or None)),
              "zfft_level_push_device")

    def level_state(self) -> int:
        """The steps counted so far."""
        v = ctypes.c_uint64()
        check(self.lib.zfft_level_state(self._plan, ctypes.byref(v)), "zfft_level_state")
        return v.value

    def level_reset(self, n0: int = 0) -> None:
        """Restart the step count at n0 with an all-zero past; the shape and the levels stay."""
        check(self.lib.zfft_level_reset(self._plan, int(n0)), "zfft_level_reset")

    def level_info(self) -> dict:
        """latency_min and latency_max (block and 2 block - 1 steps: reported, not compensated) and
        rate_ratio (1)."""
        a, b, rr = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(self.lib.zfft_level_info(self._plan, ctypes.byref(a), ctypes.byref(b), ctypes.byref(rr)), "zfft_level_info")
        return {"latency_min": a.value, "latency_max": b.value, "rate_ratio": rr.value}

    def level_meter(self):
        """(envelope, gain): float32 arrays of one value a lane, of the newest complete block.
        Synchronous."""
        k = self.level_shape()[0]
        env, gain = np.empty(k, np.float32), np.empty(k, np.float32)
        check(self.lib.zfft_level_meter(self._plan, env.ctypes.data_as(ctypes.c_void_p), gain.ctypes.data_as(ctypes.c_void_p)),
              "zfft_level_meter")
        return env, gain

    # ---------------------------------------------------------------- display viewport
    def set_viewport(self, height: int, width: int, col0: int = 0, col1: int | None = None,
                     detector: str = "max", rows_per_line: int = 1) -> None:
        """The display viewport (zfft_plan_viewport): a (height, width) image on the device, fed by
        `viewport_push*`.  Pixel x shows the `detector` ("max", "min" or "mean", the mean PSD) of
        the columns [e(x), e(x+1)) of [col0, col1) (col1 None: row_length) over `rows_per_line`
        consecutive rows; width <= col1 - col0.  Rendered through the plan's colormap and levels;
        also keeps the traces last / max hold / min hold at that width.  Resets the viewport;
        height = 0 turns it off and frees it.  The rule is in include/zfft.h."""
        if detector not in _lib.VIEW_DETECTORS:
            raise ValueError(f"detector must be one of {sorted(_lib.VIEW_DETECTORS)}")
        c1 = self.row_length if col1 is None else int(col1)
        check(self.lib.zfft_plan_viewport(self._plan, int(height), int(width), int(col0), c1,
                                          _lib.VIEW_DETECTORS[detector], int(rows_per_line)), "zfft_plan_viewport")
        self.__dict__.pop("_view_slots", None)

    def viewport_shape(self):
        h, w = ctypes.c_int32(), ctypes.c_int32()
        check(self.lib.zfft_viewport_shape(self._plan, ctypes.byref(h), ctypes.byref(w)), "zfft_viewport_shape")
        return h.value, w.value

    def viewport_push(self, rows) -> None:
        """Host rows, (count, n_win) or (count, row_length) as `rows()` crops them (or one row),
        reduced into the viewport; synchronous."""
        r = full_rows(rows, self.n_win, self.row_length)
        check(self.lib.zfft_viewport_push(self._plan, r.ctypes.data_as(ctypes.c_void_p), r.shape[0]),
              "zfft_viewport_push")

    def viewport_push_device(self, d_rows_ptr: int, count: int, stream: int = 0) -> None:
        """`count` device rows of n_win floats (e.g. what process_device wrote), enqueued on
        `stream`, no sync."""
        check(self.lib.zfft_viewport_push_device(self._plan, ctypes.c_void_p(d_rows_ptr), int(count),
                                                 ctypes.c_void_p(stream or None)), "zfft_viewport_push_device")

    def viewport_state(self):
        """(rows_seen, lines, pending): rows pushed, lines completed and the rows of the pending
        group since the enable or the last reset."""
        seen, lines, pend = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int32()
        check(self.lib.zfft_viewport_state(self._plan, ctypes.byref(seen), ctypes.byref(lines),
                                           ctypes.byref(pend)), "zfft_viewport_state")
        return int(seen.value), int(lines.value), int(pend.value)

    def viewport_image(self) -> np.ndarray:
        """float32 (height, width) in image order; lines not yet written are NaN."""
        img = np.empty(self.viewport_shape(), dtype=np.float32)
        check(self.lib.zfft_viewport_read(self._plan, img.ctypes.data_as(ctypes.c_void_p)), "zfft_viewport_read")
        return img

    def viewport_traces(self):
        """(last, max_hold, min_hold), float32 (width,) each; NaN before the first line."""
        w = self.viewport_shape()[1]
        t = np.empty((3, w), dtype=np.float32)
        check(self.lib.zfft_viewport_traces(self._plan, *(t[k].ctypes.data_as(ctypes.c_void_p) for k in range(3))),
              "zfft_viewport_traces")
        return t[0], t[1], t[2]

    def viewport_hold_reset(self) -> None:
        check(self.lib.zfft_viewport_hold_reset(self._plan), "zfft_viewport_hold_reset")

    def viewport_reset(self) -> None:
        """Image, traces, pending group and counters as after `set_viewport`; the scroll direction
        is read again (`waterfall_reset` changes it)."""
        check(self.lib.zfft_viewport_reset(self._plan), "zfft_viewport_reset")

    def _viewport_out(self, out):
        h, w = self.viewport_shape()
        if out is None:
            slots = self.__dict__.get("_view_slots")
            if not slots or slots[0][0].shape != (h, w, 4):
                slots = self._view_slots = [[pinned_empty((h, w, 4), np.uint8) for _ in range(2)], 0]
            out = slots[0][slots[1] & 1]
            slots[1] += 1
        elif out.shape != (h, w, 4) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous uint8 array of shape {(h, w, 4)}")
        return out

    def viewport_render(self, out: np.ndarray | None = None) -> np.ndarray:
        """RGBA uint8 (height, width, 4) of the viewport through the plan's colormap and levels;
        NaN (lines not yet written) has alpha 0.  `out` as in `waterfall_render`."""
        out = self._viewport_out(out)
        check(self.lib.zfft_viewport_render(self._plan, out.ctypes.data_as(ctypes.c_void_p)), "zfft_viewport_render")
        return out

    def viewport_render_device(self, d_rgba_ptr: int, stream: int = 0) -> None:
        """RGBA8 pixels of the viewport into device memory (height*width*4 bytes), enqueued on `stream`."""
        check(self.lib.zfft_viewport_render_device(self._plan, ctypes.c_void_p(d_rgba_ptr),
                                                   ctypes.c_void_p(stream or None)), "zfft_viewport_render_device")

    def viewport_push_render(self, rows, out: np.ndarray | None = None) -> np.ndarray:
        """`rows` (host rows as in `viewport_push`, or None) pushed, then the RGBA image, in one
        round trip (zfft_viewport_push_render): the per-line display call."""
        out = self._viewport_out(out)
        if rows is None:
            count, ptr = 0, None
        else:
            r = full_rows(rows, self.n_win, self.row_length)
            count, ptr = r.shape[0], r.ctypes.data
        check(self.lib.zfft_viewport_push_render(self._plan, ptr, count, out.ctypes.data), "zfft_viewport_push_render")
        return out

    # ---------------------------------------------------------------- row history
    def set_history(self, capacity: int, format: str = "u8", db_min: float = -220.0, db_max: float = -120.0) -> None:
        """The row history (zfft_plan_history): a ring on the device of the last `capacity` rows
        given to `history_push*`, stored as float32 ("f32") or as 16- / 8-bit codes ("u16",
        "u8") on 65534 / 254 equal steps from db_min to db_max (levels outside clamp; NaN keeps a
        code of its own), so that what has scrolled past can be viewed again with any window, time
        scale and detector.  Resets the store; capacity = 0 turns it off and frees it.  The rule,
        the quantiser included, is in include/zfft.h."""
        if format not in _lib.HISTORY_FORMATS:
            raise ValueError(f"format must be one of {sorted(_lib.HISTORY_FORMATS)}")
        check(self.lib.zfft_plan_history(self._plan, int(capacity), _lib.HISTORY_FORMATS[format], float(db_min),
                                         float(db_max)), "zfft_plan_history")

    def history_shape(self):
        """(capacity, columns, format)."""
        cap, cols, fmt = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        check(self.lib.zfft_history_shape(self._plan, ctypes.byref(cap), ctypes.byref(cols), ctypes.byref(fmt)),
              "zfft_history_shape")
        return int(cap.value), cols.value, {v: k for k, v in _lib.HISTORY_FORMATS.items()}[fmt.value]

    def history_push(self, rows) -> None:
        """Host rows, (count, n_win) or (count, row_length) as `rows()` crops them (or one row),
        appended to the store; synchronous."""
        r = full_rows(rows, self.n_win, self.row_length)
        check(self.lib.zfft_history_push(self._plan, r.ctypes.data_as(ctypes.c_void_p), r.shape[0]),
              "zfft_history_push")

    def history_push_device(self, d_rows_ptr: int, count: int, stream: int = 0) -> None:
        """`count` device rows of n_win floats (e.g. what process_device wrote), enqueued on
        `stream`, no sync."""
        check(self.lib.zfft_history_push_device(self._plan, ctypes.c_void_p(d_rows_ptr), int(count),
                                                ctypes.c_void_p(stream or None)), "zfft_history_push_device")

    def history_state(self):
        """(rows_seen, oldest): rows pushed since the enable or the last reset, and the number of
        the oldest row still stored; rows [oldest, rows_seen) can be read and viewed."""
        seen, oldest = ctypes.c_uint64(), ctypes.c_uint64()
        check(self.lib.zfft_history_state(self._plan, ctypes.byref(seen), ctypes.byref(oldest)), "zfft_history_state")
        return int(seen.value), int(oldest.value)

    def history_rows(self, first: int, count: int) -> np.ndarray:
        """The stored rows [first, first + count) as the store returns them, float32 (count,
        n_win); columns at or beyond row_length are NaN."""
        if int(count) < 1:
            raise ValueError("count must be at least 1")
        out = np.empty((int(count), self.n_win), dtype=np.float32)
        check(self.lib.zfft_history_read(self._plan, int(first), int(count), out.ctypes.data_as(ctypes.c_void_p)),
              "zfft_history_read")
        return out

    def history_read_device(self, first: int, count: int, d_rows_ptr: int, stream: int = 0) -> None:
        """The stored rows [first, first + count) into device rows of n_win floats (valid input to
        `viewport_push_device`, `persistence_push_device`, `detect_device` on the same stream);
        enqueued on `stream`, no sync."""
        check(self.lib.zfft_history_read_device(self._plan, int(first), int(count), ctypes.c_void_p(d_rows_ptr),
                                                ctypes.c_void_p(stream or None)), "zfft_history_read_device")

    def _history_window(self, first, lines, width, rows_per_line, detector, col0, col1):
        if detector not in _lib.VIEW_DETECTORS:
            raise ValueError(f"detector must be one of {sorted(_lib.VIEW_DETECTORS)}")
        c1 = self.row_length if col1 is None else int(col1)
        return _lib.zfft_history_window(int(first), int(rows_per_line), int(lines), int(col0), c1, int(width),
                                        _lib.VIEW_DETECTORS[detector])

    def history_view(self, first: int, lines: int, width: int, rows_per_line: int = 1, detector: str = "max",
                     col0: int = 0, col1: int | None = None) -> np.ndarray:
        """float32 (lines, width): line L, in time order, the `detector` of the stored rows
        [first + L m, first + (L + 1) m), m = rows_per_line, and of the columns [e(x), e(x+1)) of
        [col0, col1) per pixel, by the viewport's rule.  `first` may be negative or run past
        rows_seen: a line with a row that is not in the store is NaN."""
        w = self._history_window(first, lines, width, rows_per_line, detector, col0, col1)
        img = np.empty((max(int(lines), 0), max(int(width), 0)), dtype=np.float32)
        check(self.lib.zfft_history_view(self._plan, ctypes.byref(w), img.ctypes.data_as(ctypes.c_void_p)),
              "zfft_history_view")
        return img

    def history_view_device(self, d_img_ptr: int, first: int, lines: int, width: int, rows_per_line: int = 1,
                            detector: str = "max", col0: int = 0, col1: int | None = None, stream: int = 0) -> None:
        """`history_view` into device memory (lines * width floats), enqueued on `stream`, no sync."""
        w = self._history_window(first, lines, width, rows_per_line, detector, col0, col1)
        check(self.lib.zfft_history_view_device(self._plan, ctypes.byref(w), ctypes.c_void_p(d_img_ptr),
                                                ctypes.c_void_p(stream or None)), "zfft_history_view_device")

    def history_render(self, first: int, lines: int, width: int, rows_per_line: int = 1, detector: str = "max",
                       col0: int = 0, col1: int | None = None, out: np.ndarray | None = None) -> np.ndarray:
        """RGBA uint8 (lines, width, 4) of `history_view` through the plan's colormap and levels;
        NaN has alpha 0."""
        w = self._history_window(first, lines, width, rows_per_line, detector, col0, col1)
        shape = (max(int(lines), 0), max(int(width), 0), 4)
        if out is None:
            out = np.empty(shape, dtype=np.uint8)
        elif out.shape != shape or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous uint8 array of shape {shape}")
        check(self.lib.zfft_history_render(self._plan, ctypes.byref(w), out.ctypes.data_as(ctypes.c_void_p)),
              "zfft_history_render")
        return out

    def history_replay_viewport(self, first: int = 0) -> None:
        """`viewport_reset`, then the stored rows from max(first, oldest) on pushed into the
        viewport in order: after `set_viewport` with a new geometry (a zoom, a pan, another
        detector or time scale) the display is rebuilt from the history and live pushes carry on."""
        check(self.lib.zfft_history_replay_viewport(self._plan, int(first)), "zfft_history_replay_viewport")

    def history_reset(self) -> None:
        check(self.lib.zfft_history_reset(self._plan), "zfft_history_reset")


# zfft_emission (include/zfft.h): one record of ZoomFFT.detect
EMISSION_DTYPE = np.dtype([("first", np.int32), ("last", np.int32), ("peak", np.int32), ("peak_db", np.float32)])
# zfft_track (include/zfft.h): one record of ZoomFFT.tracks / open_tracks
TRACK_DTYPE = np.dtype([("row_first", np.int64), ("row_last", np.int64), ("peak_row", np.int64),
                        ("cells", np.uint64), ("runs", np.uint64), ("col_first", np.int32),
                        ("col_last", np.int32), ("peak_col", np.int32), ("slot_first", np.int32),
                        ("peak_db", np.float32), ("reserved", np.int32)])


_IN_DTYPES = {"complex64": (0, np.complex64, 1), "complex32": (1, np.float16, 2),
              "cu8": (2, np.uint8, 2), "f32": (3, np.float32, 1)}


class IQRing:
    """Host IQ accumulation ring: pypanadapter_thread.py's `Data`
    (T:1400-1483) in pinned host memory, between the reader thread (`add`) and the PSD
    worker (`take` / `process`).  See include/zfft.h zfft_ring_* for the semantics."""

    def __init__(self, chunk_size: int = 8196 * 2, in_dtype: str = "complex64"):
        self.lib = _lib.load()
        if in_dtype not in _IN_DTYPES:
            raise ValueError(f"in_dtype must be one of {sorted(_IN_DTYPES)}")
        self.in_dtype = in_dtype
        code, self._np, self._per = _IN_DTYPES[in_dtype]
        self._ring = ctypes.c_void_p()
        check(self.lib.zfft_ring_create(int(chunk_size), code, ctypes.byref(self._ring)),
              "zfft_ring_create")
        self.chunk_size = int(chunk_size)
        self.max_size = 16 * self.chunk_size

    def close(self):
        if self._ring:
            self.lib.zfft_ring_destroy(self._ring)
            self._ring = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raw(self, chunk) -> tuple:
        a = np.ascontiguousarray(chunk)
        if self.in_dtype in ("complex64", "f32"):
            a = np.ascontiguousarray(a, dtype=self._np).reshape(-1)
            return a, a.shape[0]
        a = np.ascontiguousarray(a, dtype=self._np).reshape(-1)
        if a.size % 2:
            raise ValueError("interleaved I,Q input needs an even number of values")
        return a, a.size // 2

    def add(self, chunk) -> None:
        """Data.add (T:1433-1457) without the pacing sleep."""
        a, n = self._raw(chunk)
        check(self.lib.zfft_ring_add(self._ring, a.ctypes.data_as(ctypes.c_void_p), n),
              "zfft_ring_add")

    def state(self):
        """(size, real_size, total_size) as Data holds them."""
        v = [ctypes.c_int64() for _ in range(3)]
        check(self.lib.zfft_ring_state(self._ring, *(ctypes.byref(x) for x in v)), "zfft_ring_state")
        return tuple(x.value for x in v)

    def take(self):
        """get_data_start / data[:real_size] / get_data_end (T:1516-1520): the frame (a view
        of the drained buffer, valid until the next take) and total_size."""
        p, n, tot = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        check(self.lib.zfft_ring_take(self._ring, ctypes.byref(p), ctypes.byref(n),
                                      ctypes.byref(tot)), "zfft_ring_take")
        count = n.value * self._per
        if count == 0:
            return np.empty(0, dtype=self._np), tot.value
        buf = (ctypes.c_char * (count * np.dtype(self._np).itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=self._np, count=count), tot.value

    def process(self, plan: "ZoomFFT"):
        """PSD.update (T:1513-1548): the next row from the drained frame, or None when the
        frame is shorter than fft_size (T:1522-1523).  A plan with segments_per_line >= 1 gives
        the drained frame's (R, W) lines instead (zfft_ring_process_lines)."""
        if plan.segments_per_line >= 1:
            cap = plan.lines(self.max_size)
            rows = np.empty((cap, plan.n_win), dtype=np.float32)
            produced = ctypes.c_int32()
            check(self.lib.zfft_ring_process_lines(self._ring, plan._plan, rows.ctypes.data_as(ctypes.c_void_p),
                                                   cap, ctypes.byref(produced)), "zfft_ring_process_lines")
            return np.ascontiguousarray(rows[:produced.value, :plan.row_length]) if produced.value else None
        row = np.empty(plan.n_win, dtype=np.float32)
        produced = ctypes.c_int32()
        check(self.lib.zfft_ring_process(self._ring, plan._plan, row.ctypes.data_as(ctypes.c_void_p),
                                         ctypes.byref(produced)), "zfft_ring_process")
        return row[:plan.row_length] if produced.value else None


class _PinnedBlock:
    """One zfft_host_alloc block; arrays made by `pinned_empty` hold a reference to it."""

    def __init__(self, nbytes: int):
        self._lib = _lib.load()
        p = ctypes.c_void_p()
        check(self._lib.zfft_host_alloc(max(1, int(nbytes)), ctypes.byref(p)), "zfft_host_alloc")
        self.ptr = p.value

    def __del__(self):
        if getattr(self, "ptr", None):
            self._lib.zfft_host_free(ctypes.c_void_p(self.ptr))
            self.ptr = None


def pinned_empty(shape, dtype) -> np.ndarray:
    """An uninitialised numpy array in page-locked host memory (zfft_host_alloc), freed when
    the last array viewing it is collected: the fast destination for D2H copies (renders,
    rows) and source for H2D."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    blk = _PinnedBlock(n)
    raw = (ctypes.c_char * max(1, n)).from_address(blk.ptr)
    raw._zfft_owner = blk  # the ctypes array keeps the block alive; the ndarray keeps it
    return np.frombuffer(raw, dtype=dt, count=int(np.prod(shape))).reshape(shape)


def colormap_lut(name: str) -> np.ndarray:
    """The 256 x 4 RGBA lookup table of a Waterfall colormap (host-side, no GPU needed)."""
    lib = _lib.load()
    out = np.empty((256, 4), dtype=np.uint8)
    check(lib.zfft_colormap_lut(str(name).encode(), out.ctypes.data_as(ctypes.c_void_p)),
          "zfft_colormap_lut")
    return out


def native_window(window, length: int) -> np.ndarray:
    """fp64 window from the library's native generator (no scipy needed)."""
    lib = _lib.load()
    kind, params, arr = _window_spec(window)
    if arr is not None:
        raise ValueError("array windows are not generated")
    out = np.empty(length, dtype=np.float64)
    p = (ctypes.c_double * 2)(*params)
    check(lib.zfft_window_values(kind, p, int(length), out.ctypes.data_as(ctypes.c_void_p)),
          "zfft_window_values")
    return out


def tap_design(n_taps: int, cutoff: float, beta: float = 8.0) -> np.ndarray:
    """A tap's default low-pass (zfft_tap_design; no GPU needed): a Kaiser-windowed sinc in
    float64 with unit gain at DC, `cutoff` in cycles per input sample --
    scipy.signal.firwin(n_taps, 2 * cutoff, window=("kaiser", beta))."""
    out = np.empty(int(n_taps), dtype=np.float64)
    check(_lib.load().zfft_tap_design(int(n_taps), float(cutoff), float(beta), out.ctypes.data_as(ctypes.c_void_p)),
          "zfft_tap_design")
    return out


def chan_design(n_chan: int, taps_per_channel: int = 8, beta: float = 8.0) -> np.ndarray:
    """The channeliser's default prototype (zfft_chan_design; no GPU needed):
    tap_design(n_chan * taps_per_channel, 0.5 / n_chan, beta) -- -6 dB at the channel edge, unit
    gain at DC."""
    out = np.empty(int(n_chan) * int(taps_per_channel), dtype=np.float64)
    check(_lib.load().zfft_chan_design(int(n_chan), int(taps_per_channel), float(beta),
                                       out.ctypes.data_as(ctypes.c_void_p)), "zfft_chan_design")
    return out


def demod_design(n_taps: int, cutoff: float, beta: float = 8.0) -> np.ndarray:
    """The demodulator bank's audio design (zfft_demod_design; no GPU needed): tap_design for at
    most 1024 taps; the bank's default is demod_design(8 * decim + 1, 0.4 / decim)."""
    out = np.empty(max(int(n_taps), 0), dtype=np.float64)
    check(_lib.load().zfft_demod_design(int(n_taps), float(cutoff), float(beta),
                                        out.ctypes.data_as(ctypes.c_void_p)), "zfft_demod_design")
    return out


def resamp_design(L: int, M: int, taps_per_phase: int | None = None, beta: float = 8.0) -> np.ndarray:
    """The resampler bank's design (zfft_resamp_design; no GPU needed): tap_design's formula at
    length L * taps_per_phase and cutoff 0.4 / max(L, M) cycles per upsampled sample, times L; L / M
    a reduced fraction.  taps_per_phase None is the bank's default, 16 * ceil(max(L, M) / L)."""
    if taps_per_phase is None:
        taps_per_phase = 16 * (-(-max(int(L), int(M)) // max(int(L), 1)))
    out = np.empty(max(int(L) * int(taps_per_phase), 0), dtype=np.float64)
    check(_lib.load().zfft_resamp_design(int(L), int(M), int(taps_per_phase), float(beta),
                                         out.ctypes.data_as(ctypes.c_void_p)), "zfft_resamp_design")
    return out


def tap_table(freq_word: int, taps) -> np.ndarray:
    """The modulated table c[k] a tap runs with (zfft_tap_table; no GPU needed), complex64."""
    h = np.ascontiguousarray(taps, dtype=np.float32).ravel()
    out = np.empty(h.size, dtype=np.complex64)
    check(_lib.load().zfft_tap_table(int(freq_word), h.size, h.ctypes.data_as(ctypes.c_void_p),
                                     out.ctypes.data_as(ctypes.c_void_p)), "zfft_tap_table")
    return out


def device_count() -> int:
    return int(_lib.load().zfft_device_count())
