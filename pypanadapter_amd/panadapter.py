"""Drop-in facade for the reference's DSP call sites.

The reference computes each waterfall line inline (pypanadapter_spectrum.py:2102-2119):

    if AppState.fft_ratio > 1:
        chunk = self.zoomfft(chunk, AppState.fft_ratio)
    sample_freq, spec = scipy.signal.welch(chunk, fs, window=AppState.fft_tapering,
                                           nperseg=AppState.fft_size, nfft=AppState.fft_size)
    spec = np.fft.fftshift(spec)[N//2 - self.N_WIN//2 : N//2 + self.N_WIN//2]
    psd = 20 * np.log10(abs(spec))
    self.waterfall.image_update(psd)

With this module those lines become `psd = psd_row(chunk, ...)` and `Waterfall` keeps its
`image_update(psd)` / `img_array` surface, backed by the device ring.  Like the
reference, `AppState` fields may change between frames: `PlanCache` re-creates the plan
whenever (N, zoom, W, window, fs, f_lo) change (S:1753-1757, 2079-2086, 1358-1363).
"""
from __future__ import annotations

import threading
from fractions import Fraction

import numpy as np

from .engine import ZoomFFT

_tls = threading.local()  # a plan is not re-entrant: one cache per calling thread


def _key(window):
    if isinstance(window, np.ndarray):
        return ("array", window.tobytes())
    return window if isinstance(window, str) else tuple(window)


class PlanCache:
    """Plan keyed on the AppState fields the reference re-reads every frame."""

    def __init__(self, device: int = 0):
        self.device = device
        self._key = None
        self.plan: ZoomFFT | None = None

    def get(self, fs, n_fft, zoom, n_win, window="hamming", f_lo=1.0,
            in_dtype="complex64", average="mean", segments_per_line=0) -> ZoomFFT:
        key = (float(fs), int(n_fft), int(zoom), int(n_win), _key(window), float(f_lo), in_dtype,
               average, int(segments_per_line))
        if key != self._key:
            if self.plan is not None:
                self.plan.close()
            self.plan = ZoomFFT(n_fft, zoom, fs, n_win=n_win, window=window, f_lo=f_lo,
                                device=self.device, in_dtype=in_dtype, average=average,
                                segments_per_line=int(segments_per_line))
            self._key = key
        return self.plan


def _cache(device: int, purpose: str = "rows") -> PlanCache:
    """Per thread, device and purpose: zoomfft and psd_row (each detector of it) keep separate
    plans, so code alternating them does not rebuild a plan on every call."""
    caches = getattr(_tls, "caches", None)
    if caches is None:
        caches = _tls.caches = {}
    key = (device, purpose)
    if key not in caches:
        caches[key] = PlanCache(device)
    return caches[key]


def zoomfft(x, ratio: int, fs: float, f_lo: float = 1.0, device: int = 0) -> np.ndarray:
    """ApplicationDisplay.zoomfft (S:2088-2100): LO mix + log2(ratio) x decimate(x, 2)."""
    plan = _cache(device, "zoomfft").get(fs, 32, int(ratio), 2, "hamming", f_lo)
    return plan.decimate(x)


def psd_row(chunk, fs: float, fft_size: int, fft_ratio: int, n_win: int | None = None,
            window="hamming", f_lo: float = 1.0, device: int = 0,
            average: str = "mean") -> np.ndarray:
    """The row ApplicationDisplay.update hands to waterfall.image_update (S:2102-2119).

    Returns a fresh, writable float64 array (the reference's dtype), length n_win
    (default N / zoom, i.e. N_WIN after fft_change, S:1757).  A real chunk (AudioPan,
    S:712-713) runs as real input: mixed to complex by the LO when zooming, and through
    welch's one-sided branch at zoom 1, whose row is the reference's shorter slice.
    average: "mean" (the reference's welch call), "median" (welch(average='median'): impulsive
    interference in a few segments does not lift the row) or "max" (peak hold over the chunk's
    segments); see ZoomFFT.set_average.
    """
    n_win = int(fft_size) // int(fft_ratio) if n_win is None else int(n_win)
    real = not np.iscomplexobj(chunk)
    purpose = "rows" if average == "mean" else "rows/" + str(average)
    plan = _cache(device, purpose).get(fs, fft_size, fft_ratio, n_win, window, f_lo,
                                       "f32" if real else "complex64", average)
    return plan.rows(chunk).astype(np.float64)


def psd_lines(chunk, fs: float, fft_size: int, fft_ratio: int, segments_per_line: int,
              n_win: int | None = None, window="hamming", f_lo: float = 1.0, device: int = 0,
              average: str = "mean") -> np.ndarray:
    """The time-resolved form of `psd_row`: (R, n_win) float64, the chunk's lines in time order,
    each the detector over `segments_per_line` consecutive Welch segments (1: the columns of
    scipy.signal.spectrogram through the reference's crop and dB) -- what a caller feeds to
    `Waterfall.image_update` one by one.  R = ceil(nseg / segments_per_line); 0, or a value of
    at least nseg, gives the one row of `psd_row` as (1, n_win).  Its plan (one per detector,
    rebuilt when `segments_per_line` or another field changes) is cached apart from `psd_row`'s."""
    n_win = int(fft_size) // int(fft_ratio) if n_win is None else int(n_win)
    g = int(segments_per_line)
    real = not np.iscomplexobj(chunk)
    plan = _cache(device, f"lines/{average}").get(fs, fft_size, fft_ratio, n_win, window, f_lo,
                                                       "f32" if real else "complex64", average, g)
    rows = plan.rows(chunk).astype(np.float64)
    return rows.reshape(-1, rows.shape[-1])


def thread_psd_row(chunk, fs: float, fft_size: int, fft_ratio: int, window="hamming",
                   f_lo: float = 1.0, device: int = 0, average: str = "mean"):
    """PSD.update of the threaded variant (pypanadapter_thread.py:1513-1548): skips chunks
    shorter than fft_size (T:1522-1523) and crops W = 2*int(0.5*N/zoom) (T:1542)."""
    if len(chunk) < fft_size:
        return None
    n_win = 2 * int(0.5 * fft_size / fft_ratio)
    return psd_row(chunk, fs, fft_size, fft_ratio, n_win, window, f_lo, device, average)


class Waterfall:
    """Waterfall.init_image / image_update / img_array (S:1625-1664) on the device ring.

    `image_update(psd)` stamps the grid into the caller's row in place (as S:1646-1648
    does; the reference then plots that same stamped row, S:2130), writes it as the new
    line, rolls by `scroll` and stamps the tick marks.  `img_array` materialises the
    image in the reference's row order (float64, like the reference's array).

    The device ring holds float32 (half the HBM and PCIe of float64 per line; the GPU
    rows are float32 anyway).  A float64 row from the reference's own pipeline (its psd is
    float64, S:2106) is stored as its float32 rounding, so `img_array` equals the
    reference's image exactly for float32-representable rows and within half a float32 ulp
    (<= 7.6e-6 dB for |dB| < 256) otherwise; the grid stamps (0) and the -500 fill are exact.
    Pinned by tests/test_gpu_parity.py::test_waterfall_float64_rows_are_held_as_float32.

    `image_update` stages the row on the host; the device push happens with the next read of
    the image (`img_array`, `render`, `autolevel`), together with that read in one round trip
    (zfft_waterfall_push_read64 / _push_render: one kernel, one copy, one wait per line), or
    when H rows are pending.  The image returned is the same as with a push per call.

    Buffer reuse: `img_array` and `render()` return one of two page-locked arrays this
    Waterfall owns and uses in turn, so an array stays valid until the read after next (what
    pyqtgraph's setImage per line needs: it copies or draws at once).  A caller that keeps
    images (recording, diffing, handing them to another thread) copies them, or passes its
    own array as `out=` to `render` / `image(out=...)`.  Like the reference's class, one
    Waterfall is for one thread.
    """

    def __init__(self, scroll: int = 1, device: int = 0, fs: float = 2.4e6):
        self.scroll = int(scroll)
        self.device = device
        self.fs = fs
        self.fftwidth = 0
        self._plan: ZoomFFT | None = None
        self._cmap = "Default"
        self._levels = (-220.0, -120.0)  # Waterfall.__init__ (S:1593-1598)
        self._pending: list[np.ndarray] = []  # rows image_update staged for the next read

    def _ensure(self, width: int):
        if width != self.fftwidth or self._plan is None:
            self._pending = []  # a new width re-inits the image (S:1632-1636)
            if self._plan is not None:
                self._plan.close()
            n_fft = 1 << max(5, (width - 1).bit_length())
            self._plan = ZoomFFT(n_fft, 1, self.fs, n_win=width, scroll=self.scroll,
                                 device=self.device)
            self._plan.waterfall_colormap(self._cmap)
            self._plan.waterfall_levels(*self._levels)
            self.fftwidth = width

    def init_image(self):
        self._pending = []
        if self._plan is not None:
            self._plan.waterfall_reset(self.scroll)

    def _take_pending(self):
        n = len(self._pending)
        rows = None if n == 0 else self._pending[0] if n == 1 else np.stack(self._pending)
        self._pending = []
        return rows

    def flush(self) -> None:
        """Push the staged rows to the device ring now (no image read)."""
        if self._plan is not None and self._pending:
            for r in np.atleast_2d(self._take_pending()):
                self._plan.waterfall_push(r)

    def close(self):
        """Release the device ring (the reference's image is garbage-collected)."""
        self._pending = []
        if self._plan is not None:
            self._plan.close()
            self._plan = None
            self.fftwidth = 0

    def set_scroll(self, scroll: int):
        """ApplicationDisplay.on_invertscroll_clicked (S:2074-2077): new direction + init."""
        self.scroll = int(scroll)
        self.init_image()

    def image_update(self, psd: np.ndarray) -> None:
        width = int(np.size(psd))
        self._ensure(width)
        for x in (0, width // 2, width - 1):
            psd[x] = 0
        self._pending.append(np.array(psd, dtype=np.float32).reshape(width))
        if len(self._pending) >= max(1, width // 4):  # H rows: the oldest would scroll out
            self.flush()

    def image(self, out: np.ndarray | None = None) -> np.ndarray:
        """The float64 (H, W) image in the reference's row order, staged rows pushed first."""
        if self._plan is None:
            raise AttributeError("img_array is created by the first image_update")
        return self._plan.waterfall_push_emit(self._take_pending(), True, out)

    @property
    def img_array(self) -> np.ndarray:
        return self.image()

    # ---- rendering: Waterfall.lookuptable / newlevel / autolevel, and the
    #      RGBA image pyqtgraph's ImageItem draws from img_array (S:1579-1623, 1667-1685)
    Colors = ("Default", "Matrix", "Red Green", "Tropical")

    def _need_plan(self):
        if self._plan is None:
            raise AttributeError("the waterfall image is created by the first image_update")
        return self._plan

    def lookuptable(self, choice: str) -> None:
        self._cmap = choice if choice in self.Colors else "Default"  # S:1613-1614
        if self._plan is not None:
            self._plan.waterfall_colormap(self._cmap)

    def newlevel(self, low: float, high: float):
        self._levels = (float(low), float(high))
        if self._plan is not None:
            self._plan.waterfall_levels(low, high)
        return low, high

    def autolevel(self):
        """Levels from the 2nd / 98th percentiles of the pixels below 0 (what S:1676
        computes; the reference stores them in unused attributes, so its button is a no-op)."""
        plan = self._need_plan()
        self.flush()
        self._levels = plan.waterfall_autolevel()
        return self._levels

    @property
    def levels(self):
        return self._plan.waterfall_levels() if self._plan is not None else self._levels

    def render(self, out: np.ndarray | None = None) -> np.ndarray:
        """RGBA uint8 (H, W, 4) in img_array's row order, staged rows pushed first (one
        round trip); see the class docstring for the reuse of the returned array."""
        return self._need_plan().waterfall_push_emit(self._take_pending(), False, out)


class Persistence:
    """The persistence (digital-phosphor) view of a stream of rows: per column a histogram of the
    levels seen, on the device (ZoomFFT.set_persistence; binning rule in include/zfft.h).

        view = Persistence(levels=200, db_min=-220.0, db_max=-20.0)
        view.update(psd_lines(chunk, fs, N, zoom, 1))
        img = view.image()          # uint32 (levels, W), level 0 = db_min, for an ImageItem

    `update` takes one row or (R, W) rows and lazily builds a plan for their width, like
    `Waterfall`; a new width rebuilds it and starts from zeros.  `decay(keep)` fades the counts
    (c -> floor(c keep)), `reset()` clears them, `density()` is image / rows seen."""

    def __init__(self, levels: int = 200, db_min: float = -220.0, db_max: float = -20.0,
                 device: int = 0, fs: float = 2.4e6):
        self.levels, self.db_min, self.db_max = int(levels), float(db_min), float(db_max)
        self.device = device
        self.fs = fs
        self.width = 0
        self._plan: ZoomFFT | None = None

    def _ensure(self, width: int):
        if width != self.width or self._plan is None:
            self.close()
            n_win = width + (width & 1)  # a plan's rows are even: an odd width gets a NaN column
            n_fft = 1 << max(5, (n_win - 1).bit_length())
            self._plan = ZoomFFT(n_fft, 1, self.fs, n_win=n_win, device=self.device)
            self._plan.set_persistence(self.levels, self.db_min, self.db_max)
            self.width = width

    def _need_plan(self):
        if self._plan is None:
            raise AttributeError("the persistence image is created by the first update")
        return self._plan

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None
            self.width = 0

    def update(self, psd_rows) -> None:
        rows = np.asarray(psd_rows, dtype=np.float32)
        rows = rows.reshape(-1, rows.shape[-1])
        width = rows.shape[1]
        self._ensure(width)
        if self._plan.n_win != width:
            rows = np.concatenate([rows, np.full((len(rows), 1), np.nan, np.float32)], axis=1)
        self._plan.persistence_push(rows)

    def image(self) -> np.ndarray:
        return self._need_plan().persistence()[0][:, :self.width]

    @property
    def rows_seen(self) -> int:
        return self._need_plan().persistence()[1]

    def density(self) -> np.ndarray:
        return self._need_plan().persistence_density()[:, :self.width]

    def decay(self, keep: float) -> None:
        self._need_plan().persistence_decay(keep)

    def reset(self) -> None:
        self._need_plan().persistence_reset()


class Detector:
    """Signal detection on a stream of rows, on the device (ZoomFFT.set_detect; the rule is in
    include/zfft.h): per row the noise floor, the emissions above floor + threshold_db, and per
    column how often it was part of one.

        det = Detector(threshold_db=12.0)        # row units, 20 log10: 12.04 is 4x in power
        floor, found, events = det.update(psd_lines(chunk, fs, N, zoom, 1))
        busy = det.occupancy()                   # float64 (W,), share of the rows seen

    `update` takes one row or (R, W) rows and lazily builds a plan for their width, like
    `Persistence`; a new width rebuilds it and starts from zeros.  `events` is (R, max_per_row)
    with fields first, last, peak, peak_db; `frequencies` maps its columns to Hz.

    `local=(half_window, guard)` judges every column against a floor of its own, the `quantile`
    of the half_window columns beyond `guard` columns on either side (order-statistic CFAR,
    ZoomFFT.set_detect_local): for rows whose floor is not flat.  `floors` gives those floors.

    `track=(gap, slack, min_rows)` links what `update` detects across rows on the device
    (ZoomFFT.set_track): `tracks()` returns the emissions that have ended since the last call --
    first and last row, the band, the peak -- and `open_tracks()` those still on the air;
    `track_extent` maps them to seconds and Hz."""

    def __init__(self, quantile: float = 0.5, threshold_db: float = 12.0, min_width: int = 1,
                 max_per_row: int = 8, device: int = 0, fs: float = 2.4e6, local=None, track=None,
                 max_tracks: int = 65536):
        self.track = None if track is None else tuple(int(v) for v in track)
        self.max_tracks = int(max_tracks)
        self.quantile, self.threshold_db = float(quantile), float(threshold_db)
        self.min_width, self.max_per_row = int(min_width), int(max_per_row)
        self.local = None if local is None else (int(local[0]), int(local[1]))
        self.device = device
        self.fs = fs
        self.width = 0
        self._plan: ZoomFFT | None = None

    def _ensure(self, width: int):
        if width != self.width or self._plan is None:
            self.close()
            n_win = width + (width & 1)  # a plan's rows are even: an odd width gets a NaN column
            n_fft = 1 << max(5, (n_win - 1).bit_length())
            self._plan = ZoomFFT(n_fft, 1, self.fs, n_win=n_win, device=self.device)
            self._plan.set_detect(self.quantile, self.threshold_db, self.min_width, self.max_per_row)
            if self.local is not None:
                self._plan.set_detect_local(*self.local)
            if self.track is not None:
                self._plan.set_track(*self.track, max_tracks=self.max_tracks)
            self.width = width

    def _need_plan(self):
        if self._plan is None:
            raise AttributeError("the detector's plan is created by the first update")
        return self._plan

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None
            self.width = 0

    def _rows(self, psd_rows):
        rows = np.asarray(psd_rows, dtype=np.float32)
        rows = rows.reshape(-1, rows.shape[-1])
        width = rows.shape[1]
        self._ensure(width)
        if self._plan.n_win != width:
            rows = np.concatenate([rows, np.full((len(rows), 1), np.nan, np.float32)], axis=1)
        return rows

    def update(self, psd_rows):
        """(floor float32[R], found int32[R], events[R, max_per_row]) of the rows."""
        rows = self._rows(psd_rows)  # (builds the plan)
        out = self._plan.detect(rows)
        if self.track is not None:
            self._plan.track_push(out[1], out[2])
        return out

    def tracks(self, max: int | None = None) -> np.ndarray:
        """The emissions that ended since the last call (ZoomFFT.tracks; `track=` detectors only)."""
        return self._need_plan().tracks(max)

    def open_tracks(self) -> np.ndarray:
        """The emissions still open: a carrier that never ends is only ever seen here."""
        return self._need_plan().open_tracks()

    def track_extent(self, tracks, fs: float, n_fft: int, zoom: int, line_period: float) -> dict:
        """Where the tracks lie in time and frequency: t_start, t_end (seconds; a row lasts
        `line_period` and row r covers [r, r + 1) periods), f_lo, f_hi and f_peak (Hz from the
        centre, the column centres as `frequencies` gives them), t_peak, peak_db."""
        f = self.frequencies(fs, n_fft, zoom)
        t = np.asarray(tracks)
        ok = lambda c: np.clip(c, 0, self.width - 1)  # (the NaN column of an odd width is never on)
        return dict(t_start=t["row_first"] * float(line_period), t_end=(t["row_last"] + 1) * float(line_period),
                    f_lo=f[ok(t["col_first"])], f_hi=f[ok(t["col_last"])], f_peak=f[ok(t["peak_col"])],
                    t_peak=t["peak_row"] * float(line_period), peak_db=t["peak_db"].copy())

    def floors(self, psd_rows) -> np.ndarray:
        """float32 (R, W): the local floor of every column of the rows (`local` detectors only);
        counts nothing."""
        rows = self._rows(psd_rows)
        return self._plan.detect_floors(rows)[:, :self.width]

    @property
    def rows_seen(self) -> int:
        return self._need_plan().detect_occupancy()[1]

    def occupancy(self) -> np.ndarray:
        """float64 occ / max(rows_seen, 1) per column: the share of the rows in which the column
        was part of an emission."""
        occ, seen = self._need_plan().detect_occupancy()
        return occ[:self.width] / float(max(seen, 1))

    def reset(self) -> None:
        self._need_plan().detect_reset()

    def frequencies(self, fs: float, n_fft: int, zoom: int) -> np.ndarray:
        """Offset in Hz from the centre (the LO) of every column of a two-sided row of this
        width: the row is fftshift(P)[N/2 - W/2 : N/2 + W/2] (zfft_plan_row_length), so column j
        is bin j - W/2 of bins fs / (zoom n_fft) wide."""
        if not self.width:
            raise AttributeError("the detector's width is set by the first update")
        return (np.arange(self.width) - self.width // 2) * (float(fs) / (int(zoom) * int(n_fft)))


class Viewport:
    """A display-sized view of a stream of rows, reduced on the device (ZoomFFT.set_viewport; the
    rule is in include/zfft.h): every pixel the max, min or mean PSD of the bucket of columns and
    the `rows_per_line` rows that fall into it, so a 1920 x 1080 widget shows every narrow or
    short emission of rows far wider and faster than the screen.

        view = Viewport(1080, 1920, detector="max", rows_per_line=16)
        view.levels(-220.0, -120.0)
        view.update(psd_lines(chunk, fs, N, zoom, 1))
        rgba = view.render()                    # uint8 (1080, 1920, 4) for an ImageItem
        last, max_hold, min_hold = view.traces()

    `update` takes one row or (R, W) rows and lazily builds a plan for their width, like
    `Persistence`; a new width rebuilds it and starts empty.  The view's `width` may not exceed
    the columns it covers ([col0, col1), default the whole row)."""

    def __init__(self, height: int, width: int, detector: str = "max", rows_per_line: int = 1,
                 col0: int = 0, col1: int | None = None, scroll: int = 1, colormap: str = "Default",
                 device: int = 0, fs: float = 2.4e6):
        self.height, self.width = int(height), int(width)
        self.detector, self.rows_per_line = detector, int(rows_per_line)
        self.col0, self.col1 = int(col0), col1
        self.scroll, self.colormap = int(scroll), colormap
        self.device = device
        self.fs = fs
        self.cols = 0
        self._levels = None
        self._plan: ZoomFFT | None = None

    def _ensure(self, cols: int):
        if cols != self.cols or self._plan is None:
            self.close()
            n_win = cols + (cols & 1)  # a plan's rows are even: an odd width gets a NaN column
            n_fft = 1 << max(5, (n_win - 1).bit_length())
            plan = ZoomFFT(n_fft, 1, self.fs, n_win=n_win, scroll=self.scroll, device=self.device)
            try:
                plan.set_viewport(self.height, self.width, self.col0, cols if self.col1 is None else self.col1,
                                  self.detector, self.rows_per_line)
                plan.waterfall_colormap(self.colormap)
                if self._levels is not None:
                    plan.waterfall_levels(*self._levels)
            except Exception:
                plan.close()
                raise
            self._plan = plan
            self.cols = cols

    def _need_plan(self):
        if self._plan is None:
            raise AttributeError("the viewport's image is created by the first update")
        return self._plan

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None
            self.cols = 0

    def levels(self, low: float | None = None, high: float | None = None):
        """Set (when given) and return the render levels (low, high)."""
        if low is not None:
            self._levels = (float(low), float(high))
            if self._plan is not None:
                self._plan.waterfall_levels(*self._levels)
        if self._plan is not None:
            return self._plan.waterfall_levels()
        return self._levels if self._levels is not None else (-220.0, -120.0)

    def update(self, psd_rows) -> None:
        rows = np.asarray(psd_rows, dtype=np.float32)
        rows = rows.reshape(-1, rows.shape[-1])
        cols = rows.shape[1]
        self._ensure(cols)
        if self._plan.n_win != cols:
            rows = np.concatenate([rows, np.full((len(rows), 1), np.nan, np.float32)], axis=1)
        self._plan.viewport_push(rows)

    def image(self) -> np.ndarray:
        """float32 (height, width); lines not yet written are NaN."""
        return self._need_plan().viewport_image()

    def render(self, out: np.ndarray | None = None) -> np.ndarray:
        """RGBA uint8 (height, width, 4); see ZoomFFT.waterfall_render for the reuse of the
        returned array."""
        return self._need_plan().viewport_render(out)

    def traces(self):
        """(last, max_hold, min_hold), float32 (width,) each."""
        return self._need_plan().viewport_traces()

    @property
    def state(self):
        """(rows_seen, lines, pending)."""
        return self._need_plan().viewport_state()

    def hold_reset(self) -> None:
        self._need_plan().viewport_hold_reset()

    def reset(self) -> None:
        self._need_plan().viewport_reset()

    def frequencies(self, fs: float, n_fft: int, zoom: int) -> np.ndarray:
        """Offset in Hz from the centre (the LO) of every pixel: the mean of its bucket's columns
        under `Detector.frequencies`' mapping of a two-sided row of this width (column j is bin
        j - W/2 of bins fs / (zoom n_fft) wide)."""
        if not self.cols:
            raise AttributeError("the viewport's columns are set by the first update")
        c1 = self.cols if self.col1 is None else int(self.col1)
        e = self.col0 + np.arange(self.width + 1, dtype=np.int64) * (c1 - self.col0) // self.width
        centre = (e[:-1] + e[1:] - 1) / 2.0
        return (centre - self.cols // 2) * (float(fs) / (int(zoom) * int(n_fft)))


class History:
    """The last `capacity` rows of a stream kept on the device (ZoomFFT.set_history; the rule is
    in include/zfft.h) as 8- or 16-bit codes on the level scale db_min .. db_max (or as float32),
    so that a display can zoom, pan, change its time scale or detector and scroll back over what
    has already passed: `view` reduces any stretch of the stored rows to any pixel grid.

        hist = History(1 << 20, "u8", -160.0, -40.0)
        hist.update(psd_lines(chunk, fs, N, zoom, 1))
        first = hist.latest(1080, 16)           # the newest 1080 lines of 16 rows
        rgba = hist.render(first, 1080, 1920, rows_per_line=16, col0=2000, col1=6000)

    `update` takes one row or (R, W) rows and lazily builds a plan for their width, like
    `Persistence` and `Viewport`; a new width rebuilds it and starts empty."""

    def __init__(self, capacity: int, format: str = "u8", db_min: float = -220.0, db_max: float = -120.0,
                 colormap: str = "Default", device: int = 0, fs: float = 2.4e6):
        self.capacity, self.format = int(capacity), format
        self.db_min, self.db_max = float(db_min), float(db_max)
        self.colormap = colormap
        self.device = device
        self.fs = fs
        self.cols = 0
        self._levels = None
        self._plan: ZoomFFT | None = None

    def _ensure(self, cols: int):
        if cols != self.cols or self._plan is None:
            self.close()
            n_win = cols + (cols & 1)  # a plan's rows are even: an odd width gets a NaN column
            n_fft = 1 << max(5, (n_win - 1).bit_length())
            plan = ZoomFFT(n_fft, 1, self.fs, n_win=n_win, device=self.device)
            try:
                plan.set_history(self.capacity, self.format, self.db_min, self.db_max)
                plan.waterfall_colormap(self.colormap)
                if self._levels is not None:
                    plan.waterfall_levels(*self._levels)
            except Exception:
                plan.close()
                raise
            self._plan = plan
            self.cols = cols

    def _need_plan(self):
        if self._plan is None:
            raise AttributeError("the history's store is created by the first update")
        return self._plan

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None
            self.cols = 0

    def levels(self, low: float | None = None, high: float | None = None):
        """Set (when given) and return the render levels (low, high)."""
        if low is not None:
            self._levels = (float(low), float(high))
            if self._plan is not None:
                self._plan.waterfall_levels(*self._levels)
        if self._plan is not None:
            return self._plan.waterfall_levels()
        return self._levels if self._levels is not None else (-220.0, -120.0)

    def update(self, psd_rows) -> None:
        rows = np.asarray(psd_rows, dtype=np.float32)
        rows = rows.reshape(-1, rows.shape[-1])
        cols = rows.shape[1]
        self._ensure(cols)
        if self._plan.n_win != cols:
            rows = np.concatenate([rows, np.full((len(rows), 1), np.nan, np.float32)], axis=1)
        self._plan.history_push(rows)

    def _c1(self, col1):
        return self.cols if col1 is None else int(col1)

    def view(self, first: int, lines: int, width: int, rows_per_line: int = 1, detector: str = "max",
             col0: int = 0, col1: int | None = None) -> np.ndarray:
        """float32 (lines, width), oldest line first; see ZoomFFT.history_view."""
        plan = self._need_plan()
        return plan.history_view(first, lines, width, rows_per_line, detector, col0, self._c1(col1))

    def render(self, first: int, lines: int, width: int, rows_per_line: int = 1, detector: str = "max",
               col0: int = 0, col1: int | None = None, out: np.ndarray | None = None) -> np.ndarray:
        """RGBA uint8 (lines, width, 4) of `view` through the colormap and levels."""
        plan = self._need_plan()
        return plan.history_render(first, lines, width, rows_per_line, detector, col0, self._c1(col1), out)

    def rows(self, first: int, count: int) -> np.ndarray:
        """The stored rows [first, first + count) as the store returns them, (count, cols)."""
        return self._need_plan().history_rows(first, count)[:, :self.cols]

    @property
    def state(self):
        """(rows_seen, oldest)."""
        return self._need_plan().history_state()

    def latest(self, lines: int, rows_per_line: int = 1) -> int:
        """The `first` whose window of `lines` lines of `rows_per_line` rows ends at rows_seen (it
        may be negative or lie before `oldest`: those lines are NaN)."""
        return self.state[0] - int(lines) * int(rows_per_line)

    def reset(self) -> None:
        self._need_plan().history_reset()

    def frequencies(self, width: int, fs: float, n_fft: int, zoom: int, col0: int = 0,
                    col1: int | None = None) -> np.ndarray:
        """Offset in Hz from the centre (the LO) of every pixel of a view of `width` pixels over
        [col0, col1), as `Viewport.frequencies`."""
        if not self.cols:
            raise AttributeError("the history's columns are set by the first update")
        c1 = self._c1(col1)
        e = int(col0) + np.arange(int(width) + 1, dtype=np.int64) * (c1 - int(col0)) // int(width)
        centre = (e[:-1] + e[1:] - 1) / 2.0
        return (centre - self.cols // 2) * (float(fs) / (int(zoom) * int(n_fft)))


class Tap:
    """Narrowband complex streams out of the wideband input, on the device (ZoomFFT.set_taps; the
    rule is in include/zfft.h): every tap is an oscillator, a low-pass and an integer decimation
    with its state kept from push to push, so the outputs are one continuous stream however the
    input arrives.

        taps = Tap(fs)                                   # for a caller of read_samples()
        taps.open(0, 7.074e6 - f_centre, decim=128)      # a click on a carrier
        ext = det.track_extent(det.open_tracks(), fs, N, zoom, line_period)
        slot = taps.open_for(ext, 0)                     # ... or a track handed over
        iq = taps.push(chunk)[slot]                      # complex64 at taps.rate(slot)

    `push` takes the next stretch of samples (any length) and returns {slot: complex64 outputs}.
    Frequencies are Hz in the samples' own baseband; the group delay (n_taps - 1) / 2 input
    samples is reported by `info`, not compensated."""

    def __init__(self, fs: float, max_taps: int = 8, max_len: int = 2048, in_dtype: str = "complex64",
                 device: int = 0):
        self.fs = float(fs)
        self._plan = ZoomFFT(32, 1, self.fs, device=device, in_dtype=in_dtype)  # (the taps read samples, not rows)
        self._plan.set_taps(max_taps, max_len)
        self.max_taps, self.max_len = int(max_taps), int(max_len)

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None

    def open(self, slot: int, f_hz: float, decim: int, taps=None, cutoff: float | None = None,
             beta: float = 8.0) -> float:
        """ZoomFFT.tap_open: returns the centre frequency actually used."""
        return self._plan.tap_open(slot, f_hz, decim, taps=taps, cutoff=cutoff, beta=beta)

    def open_for(self, extent: dict, index: int = 0, margin: float = 1.25, slot: int | None = None,
                 centre: float = 0.0) -> int:
        """Open a tap on entry `index` of `Detector.track_extent`: at the middle of the track's band
        [f_lo, f_hi] (Hz from the rows' centre, which is `centre` Hz in the samples' baseband: 0 at
        zoom 1, the plan's f_lo otherwise), with the largest decimation whose output rate
        fs / decim is still at least `margin` times the band's width, and the default design.
        Takes the first free slot unless `slot` is given; returns the slot."""
        f_lo = float(np.atleast_1d(extent["f_lo"])[index])
        f_hi = float(np.atleast_1d(extent["f_hi"])[index])
        need = float(margin) * abs(f_hi - f_lo)
        decim = 512 if need <= 0 else int(min(512, max(1, np.floor(self.fs / need))))
        if slot is None:
            free = sorted(set(range(self.max_taps)) - set(self._plan.tap_open_slots()))
            if not free:
                raise ValueError("every tap slot is open")
            slot = free[0]
        self.open(slot, centre + 0.5 * (f_lo + f_hi), decim)
        return int(slot)

    def close_tap(self, slot: int) -> None:
        self._plan.tap_close(slot)

    def info(self, slot: int) -> dict:
        return self._plan.tap_info(slot)

    def rate(self, slot: int) -> float:
        """The tap's output rate fs / decim in Hz."""
        return self.fs / self._plan.tap_info(slot)["decim"]

    def counts(self, n: int) -> np.ndarray:
        return self._plan.tap_counts(n)

    def push(self, chunk) -> dict:
        """{slot: complex64 outputs} of the open taps for the next samples of the stream."""
        return dict(zip(self._plan.tap_open_slots(), self._plan.tap_push(chunk)))

    @property
    def samples_seen(self) -> int:
        return self._plan.tap_state()

    def reset(self, n0: int = 0) -> None:
        self._plan.tap_reset(n0)


class Channelizer:
    """Every channel of the band at once, on the device (ZoomFFT.set_channels; the rule is in
    include/zfft.h): a polyphase-FFT bank of `n_chan` uniform channels with its state kept from
    push to push, so each column is one continuous narrowband stream however the input arrives.

        bank = Channelizer(fs, 64)                       # for a caller of read_samples()
        y = bank.push(chunk)                             # (steps, 64) complex64 at bank.rate
        ext = det.track_extent(det.open_tracks(), fs, N, zoom, line_period)
        iq = y[:, bank.channel_for(ext, 0)]              # the channel a track lies in

    Columns are in ascending frequency (`freqs`, Hz in the samples' own baseband) unless
    `ascending=False` keeps the transform's order.  The group delay is reported, not compensated."""

    def __init__(self, fs: float, n_chan: int, taps_per_channel: int = 8, oversample: int = 2, taps=None,
                 beta: float = 8.0, in_dtype: str = "complex64", ascending: bool = True, device: int = 0):
        self.fs = float(fs)
        self._plan = ZoomFFT(32, 1, self.fs, device=device, in_dtype=in_dtype)  # (the bank reads samples, not rows)
        self._plan.set_channels(n_chan, taps_per_channel, oversample, taps=taps, beta=beta)
        self.n_chan = int(n_chan)
        if ascending:
            self._plan.chan_select(self.n_chan // 2, self.n_chan)

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None

    def select(self, c_first: int, c_count: int) -> None:
        self._plan.chan_select(c_first, c_count)

    @property
    def freqs(self) -> np.ndarray:
        """The centre of every kept channel in Hz, in the order of `push`'s columns."""
        return self._plan.chan_freqs()

    @property
    def rate(self) -> float:
        """The channels' output rate fs / decim in Hz."""
        return self.fs * self._plan.chan_info()["rate_ratio"]

    @property
    def group_delay(self) -> float:
        """(n_chan * taps_per_channel - 1) / 2 input samples."""
        return self._plan.chan_info()["group_delay"]

    def steps(self, n: int) -> int:
        return self._plan.chan_steps(n)

    def push(self, chunk) -> np.ndarray:
        """(steps, kept channels) complex64 for the next samples of the stream."""
        return self._plan.chan_push(chunk)

    def channel_of(self, f_hz: float) -> int:
        """The column of `push` whose channel covers f_hz (Hz in the samples' baseband, taken
        modulo fs); ValueError when that channel is not kept."""
        _, _, _, c0, k = self._plan.chan_shape()
        c = int(np.floor(float(f_hz) / self.fs * self.n_chan + 0.5)) % self.n_chan
        i = (c - c0) % self.n_chan
        if i >= k:
            raise ValueError(f"channel {c} is not among the kept channels")
        return i

    def channel_for(self, extent: dict, index: int = 0, centre: float = 0.0) -> int:
        """The column covering the middle of entry `index` of `Detector.track_extent` (its band
        [f_lo, f_hi] in Hz from the rows' centre, which is `centre` Hz in the samples' baseband)."""
        f_lo = float(np.atleast_1d(extent["f_lo"])[index])
        f_hi = float(np.atleast_1d(extent["f_hi"])[index])
        return self.channel_of(centre + 0.5 * (f_lo + f_hi))

    @property
    def samples_seen(self) -> int:
        return self._plan.chan_state()

    def reset(self, n0: int = 0) -> None:
        self._plan.chan_reset(n0)


class Demodulator:
    """Audio out of what a `Channelizer` or a `Tap` pushes, on the device (ZoomFFT.set_demod; the
    rule is in include/zfft.h): every stream is detected ("am", "fm", "ssb" or "power") and runs
    through one shared audio low-pass decimating by `audio_decim`, with its state kept from push
    to push.

        bank = Channelizer(fs, 64)
        audio = Demodulator.for_channelizer(bank, "fm", audio_decim=4)
        a = audio.push(bank.push(chunk))                 # (steps, 64) float32 at audio.rate
        audio.mode("ssb", bfo_hz=1500.0, first=col, count=1)   # one channel to USB

    The bank lives on its source's plan (one demodulator per source), so a caller who keeps the
    source's output on the device (`chan_push_device`, `tap_push_device`) can hand it to
    `plan.demod_push_device` with no copy.  "power" is the zero-span trace: power against time on
    one frequency, the audio filter acting as video filter.  FM's +-1 is +-rate_in / 2.  The group
    delay is reported, not compensated."""

    def __init__(self, plan, streams: int, rate_in: float, mode="am", audio_decim: int = 1, taps=None,
                 bfo_hz: float = 0.0):
        self._plan, self.streams, self.rate_in = plan, int(streams), float(rate_in)
        plan.set_demod(self.streams, taps=taps, decim=audio_decim)
        self.mode(mode, bfo_hz)

    @classmethod
    def for_channelizer(cls, chan: "Channelizer", mode="am", audio_decim: int = 1, taps=None, bfo_hz: float = 0.0):
        """One stream per kept channel of `chan`, in the order of its columns; `push` takes what
        `chan.push` returns.  (A later `chan.select` of another count needs a new Demodulator.)"""
        return cls(chan._plan, chan._plan.chan_shape()[4], chan.rate, mode, audio_decim, taps, bfo_hz)

    @classmethod
    def for_tap(cls, tap: "Tap", mode="am", audio_decim: int = 1, slot: int | None = None, taps=None,
                bfo_hz: float = 0.0):
        """One stream: the open tap in `slot` (default: the only open one); `push` takes that
        slot's array of `tap.push`."""
        if slot is None:
            (slot,) = tap._plan.tap_open_slots()
        return cls(tap._plan, 1, tap.rate(slot), mode, audio_decim, taps, bfo_hz)

    def close(self):
        """Turns the bank off on the source's plan, which stays the source's."""
        if self._plan is not None:
            if self._plan._plan.value:  # (the source may have closed its plan already)
                self._plan.set_demod(0)
            self._plan = None

    def mode(self, mode, bfo_hz: float = 0.0, first: int = 0, count: int | None = None) -> float:
        """ZoomFFT.demod_mode at the streams' rate: returns the BFO frequency actually used."""
        return self._plan.demod_mode(mode, bfo_hz, rate=self.rate_in, first=first, count=count)

    @property
    def rate(self) -> float:
        """The audio's rate in Hz: the streams' rate / audio_decim."""
        return self.rate_in * self._plan.demod_info()["rate_ratio"]

    @property
    def group_delay(self) -> float:
        """(n_taps - 1) / 2 steps of the streams."""
        return self._plan.demod_info()["group_delay"]

    def steps(self, n: int) -> int:
        return self._plan.demod_steps(n)

    def push(self, y) -> np.ndarray:
        """(outputs, streams) float32 for the next (steps, streams) complex64 of the source."""
        return self._plan.demod_push(y)

    @property
    def steps_seen(self) -> int:
        return self._plan.demod_state()

    def reset(self, n0: int = 0) -> None:
        self._plan.demod_reset(n0)


class Resampler:
    """What a `Demodulator`, a `Tap` or a `Channelizer` pushes at a rate a device takes, on the
    device (ZoomFFT.set_resamp; the rule is in include/zfft.h): `lanes` real lanes -- a complex
    stream is two -- at rate_out / rate_in = L / M times their rate through one polyphase filter,
    with its state kept from push to push, as float32 or as int16 PCM.

        audio = Demodulator.for_channelizer(bank, "fm", audio_decim=4)      # 18.75 kHz
        pcm = Resampler.for_demodulator(audio, 48e3, format="s16")          # 64 / 25
        s = pcm.push(audio.push(bank.push(chunk)))                           # (outputs, 64) int16 at pcm.rate

    The ratio is reduced to lowest terms and must then have L <= 512 and M <= 4096 (a ValueError
    names it otherwise).  The bank lives on its source's plan, so a caller who keeps the source's
    output on the device can hand it to `plan.resamp_push_device` with no copy.  The group delay is
    reported, not compensated."""

    def __init__(self, plan, lanes: int, rate_in: float, rate_out: float, taps=None, taps_per_phase: int | None = None,
                 format: str = "f32", scale: float = 32767.0):
        self._plan, self.lanes, self.rate_in = plan, int(lanes), Fraction(rate_in)
        ratio = Fraction(rate_out) / self.rate_in
        self.L, self.M = ratio.numerator, ratio.denominator
        if not (1 <= self.L <= 512 and 1 <= self.M <= 4096):
            raise ValueError(f"rate_out / rate_in reduces to L / M = {self.L} / {self.M}: outside L <= 512, M <= 4096")
        plan.set_resamp(self.lanes, self.L, self.M, taps=taps, taps_per_phase=taps_per_phase, format=format, scale=scale)

    @classmethod
    def for_demodulator(cls, demod: "Demodulator", rate_out: float, format: str = "f32", **kw):
        """One lane per stream of `demod`; `push` takes what `demod.push` returns."""
        info = demod._plan.demod_shape()
        return cls(demod._plan, info[0], Fraction(demod.rate_in) / info[2], rate_out, format=format, **kw)

    @classmethod
    def for_level(cls, level: "LevelControl", rate_out: float, format: str = "f32", **kw):
        """One lane per lane of `level`, at its rate; `push` takes what `level.push` returns."""
        return cls(level._plan, level.lanes, Fraction(level.rate), rate_out, format=format, **kw)

    @classmethod
    def for_tap(cls, tap: "Tap", rate_out: float, slot: int | None = None, **kw):
        """Complex in, complex out: the open tap in `slot` (default: the only open one) as two
        lanes; `push` takes that slot's array of `tap.push` and returns complex64."""
        if slot is None:
            (slot,) = tap._plan.tap_open_slots()
        return cls(tap._plan, 2, Fraction(tap.fs) / tap._plan.tap_info(slot)["decim"], rate_out, **kw)

    def close(self):
        """Turns the bank off on the source's plan, which stays the source's."""
        if self._plan is not None:
            if self._plan._plan.value:  # (the source may have closed its plan already)
                self._plan.set_resamp(0)
            self._plan = None

    @property
    def rate(self) -> float:
        """The output rate in Hz, exactly rate_in * L / M."""
        return float(self.rate_in * self.L / self.M)

    @property
    def group_delay(self) -> float:
        """(taps_per_phase * L - 1) / (2 L) input steps."""
        return self._plan.resamp_info()["group_delay"]

    def steps(self, n: int) -> int:
        return self._plan.resamp_steps(n)

    def push(self, y) -> np.ndarray:
        """(outputs, lanes) float32 or int16 for the next (steps, lanes) float32 of the source;
        complex64 in gives complex64 out (float32 format)."""
        return self._plan.resamp_push(y)

    @property
    def steps_seen(self) -> int:
        return self._plan.resamp_state()

    def reset(self, n0: int = 0) -> None:
        self._plan.resamp_reset(n0)


class LevelControl:
    """Look-ahead gain control, squelch and a level meter on what a `Demodulator` pushes, on the
    device (ZoomFFT.set_level; the rule is in include/zfft.h): per block of `block` steps and lane,
    the gain that brings the envelope -- the peak over the block and `hold` blocks before it -- to
    `target`, at most `gmax`, 0 below `squelch`; it ramps over the block before a louder one, so
    the output stays within target, and comes `block` to 2 block - 1 steps late.

        audio = Demodulator.for_channelizer(bank, "am", audio_decim=4)      # 18.75 kHz
        agc = LevelControl.for_demodulator(audio, target=0.5, attack_s=3e-3, hold_s=0.25, squelch=1e-4)
        pcm = Resampler.for_level(agc, 48e3, format="s16")
        s = pcm.push(agc.push(audio.push(bank.push(chunk))))                 # (outputs, 64) int16
        open_now = agc.meter()["open"]                                        # which channels carry something

    The bank lives on its source's plan, so a caller who keeps the audio on the device can hand it
    to `plan.level_push_device` with no copy.  `push(y, key=...)` takes the gains from `key` (the
    side chain: FM audio gated by a power trace).  The latency is reported, not compensated."""

    MIN_BLOCK, MAX_BLOCK, MAX_HOLD = 8, 1024, 4096

    def __init__(self, plan, lanes: int, rate: float, block: int = 64, hold: int = 0, target: float = 0.5,
                 gmax: float = 1e4, floor: float = 1e-6, squelch: float | None = None):
        self._plan, self.lanes, self.rate = plan, int(lanes), float(rate)
        self.block, self.hold = int(block), int(hold)
        if self.block < self.MIN_BLOCK or self.block > self.MAX_BLOCK or self.block & (self.block - 1):
            raise ValueError(f"block = {self.block}: not a power of two in [{self.MIN_BLOCK}, {self.MAX_BLOCK}]")
        if not 0 <= self.hold <= self.MAX_HOLD:
            raise ValueError(f"hold = {self.hold} blocks: outside [0, {self.MAX_HOLD}]")
        plan.set_level(self.lanes, self.block, self.hold, target, gmax, floor, 0.0 if squelch is None else squelch)

    @classmethod
    def for_demodulator(cls, demod: "Demodulator", target: float = 0.5, attack_s: float = 3e-3, hold_s: float = 0.25,
                        squelch: float | None = None, **kw):
        """One lane per stream of `demod`; `push` takes what `demod.push` returns.  The block is
        the power of two nearest attack_s x the audio rate (in the ratio's sense), clipped to
        [8, 1024]; the hold ceil(hold_s x rate / block) blocks (a ValueError names it past 4096)."""
        rate = demod.rate
        want = max(float(attack_s) * rate, 1.0)
        block = int(min(max(2 ** int(np.floor(np.log2(want) + 0.5)), cls.MIN_BLOCK), cls.MAX_BLOCK))
        hold = int(np.ceil(float(hold_s) * rate / block))
        if hold_s < 0 or hold > cls.MAX_HOLD:
            raise ValueError(f"hold_s = {hold_s} s is {hold} blocks of {block} steps at {rate} Hz: outside [0, {cls.MAX_HOLD}]")
        return cls(demod._plan, demod.streams, rate, block, hold, target, squelch=squelch, **kw)

    def close(self):
        """Turns the bank off on the source's plan, which stays the source's."""
        if self._plan is not None:
            if self._plan._plan.value:  # (the source may have closed its plan already)
                self._plan.set_level(0)
            self._plan = None

    @property
    def latency(self):
        """(least, most) steps an output comes after its input: (block, 2 block - 1)."""
        info = self._plan.level_info()
        return info["latency_min"], info["latency_max"]

    def steps(self, n: int) -> int:
        return self._plan.level_steps(n)

    def push(self, y, key=None) -> np.ndarray:
        """(emitted, lanes) float32 for the next (steps, lanes) float32 of the source."""
        return self._plan.level_push(y, key)

    def meter(self) -> dict:
        """envelope and gain of the newest complete block of every lane, and open = gain > 0."""
        env, gain = self._plan.level_meter()
        return {"envelope": env, "gain": gain, "open": gain > 0}

    @property
    def steps_seen(self) -> int:
        return self._plan.level_state()

    def reset(self, n0: int = 0) -> None:
        self._plan.level_reset(n0)


class Data:
    """pypanadapter_thread.py's `Data` (T:1400-1483) on the pinned double-buffered IQRing
    (SURVEY §8f-1), same calls: the reader thread's `add(chunk)` (T:2191) and the PSD
    worker's `get_data_start(); size = real_size; chunk = data[:size]; get_data_end()`
    (T:1516-1520).  `get_data_start` drains the ring, so `data[:real_size]` stays intact
    while the reader keeps adding (the reference hands out a view it keeps overwriting).
    `new_complex` takes complex64 (or, with `in_dtype="cu8"`, the RTL-SDR's raw interleaved
    uint8 I,Q bytes), `new_real` real float32 samples (AudioPan).  `fft_size` stands for
    AppState.fft_size, the target setter's lower bound (T:1477).  The NewtRap pacing
    (`delay_time`, the sleep in add) is out of scope; `target` keeps the reference's rules.
    Pinned by tests/golden/ring.npz, sequences of the reference's own class."""

    def __init__(self, chunk_size: int = 8196 * 2, in_dtype: str = "complex64",
                 fft_size: int = 2048):
        self.chunk_size = int(chunk_size)
        self.max_size = self.chunk_size * 16          # T:1406
        self.target_size = self.max_size * .9         # T:1407
        self.in_dtype = in_dtype
        self.fft_size = int(fft_size)
        self._ring = None
        self.data = None
        self.real = False
        self.real_size = 0
        self.total_size = 0

    def _new(self, in_dtype: str, real: bool):
        from .engine import IQRing
        if self._ring is not None:
            self._ring.close()
        self._ring = IQRing(self.chunk_size, in_dtype)
        self.real = real
        self.data, self.real_size, self.total_size = None, 0, 0
        return self

    def new_complex(self):
        """T:1419-1423 (new_common: empty buffer, counts 0)."""
        return self._new("complex64" if self.in_dtype == "f32" else self.in_dtype, False)

    def new_real(self):
        """T:1413-1417: real samples (AudioPan's float32 stream)."""
        return self._new("f32", True)

    def add(self, chunk):
        """T:1433-1457 without the pacing sleep: fold back at max_size, then the target clip
        np.clip(target_size, 8192, max_size) (T:1445) before the write."""
        self.target_size = np.clip(self.target_size, 8192, self.max_size)
        self._ring.add(chunk)

    def get_data_start(self):
        frame, total = self._ring.take()
        self.data = frame
        self.real_size = len(frame) if self._ring.in_dtype in ("complex64", "f32") else len(frame) // 2
        self.total_size = total

    def get_data_end(self):
        pass  # the counts were reset by the drain in get_data_start

    def process(self, plan):
        """get_data_start + PSD.update's DSP in one call (zfft_ring_process)."""
        return self._ring.process(plan)

    @property
    def size(self):
        """Data.size: where the next chunk goes (T:1426, 1449)."""
        return self._ring.state()[0]

    @property
    def target(self):
        return self.target_size

    @target.setter
    def target(self, t):
        if t >= self.fft_size and t <= self.max_size:  # T:1474-1479
            self.target_size = t

    @property
    def maxsize(self):
        return self.max_size
