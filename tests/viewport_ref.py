"""The display viewport's rule (include/zfft.h, zfft_plan_viewport) in numpy: plain reductions,
MAX and MIN in float32 (np.fmax / np.fmin, bit for bit what the device must give), MEAN in
float64.  Pinned on hand-made values by test_viewport_host.py, used by test_gpu_viewport.py."""
import numpy as np

DETECTORS = ("max", "min", "mean")


def edges(col0, col1, width):
    """e(x) = col0 + floor(x * span / width), x = 0 .. width, in int64."""
    x = np.arange(width + 1, dtype=np.int64)
    return col0 + x * (col1 - col0) // width


def _row_buckets(rows, geometry, detector):
    """Every row reduced over its buckets: (count, width), float32 values (max / min) or float64
    linear sums (mean)."""
    col0, col1, width = geometry
    e = edges(col0, col1, width)
    at = (e[:-1] - col0).astype(np.intp)
    v = np.asarray(rows, dtype=np.float32)[:, col0:col1]
    if detector == "mean":
        with np.errstate(over="ignore"):
            return np.add.reduceat(10.0 ** (v.astype(np.float64) / 20.0), at, axis=1)
    return (np.fmax if detector == "max" else np.fmin).reduceat(v, at, axis=1)


def empty_pending(geometry, detector):
    width = geometry[2]
    if detector == "mean":
        return 0, np.zeros(width, np.float64)
    return 0, np.full(width, np.nan, np.float32)


def ref_lines(rows, n, geometry, detector, m, pending_state=None):
    """(lines, pending_state) of `rows` pushed after `pending_state` = (rows so far, accumulator)
    (None: an empty group).  Only columns [col0, col1) <= n of a row are read.  lines is
    (L, width): float32 for max / min, float64 for mean."""
    col0, col1, width = geometry
    assert 0 <= col0 < col1 <= n and 1 <= width <= col1 - col0 and m >= 1
    have, acc = empty_pending(geometry, detector) if pending_state is None else pending_state
    acc = acc.copy()
    per_row = _row_buckets(rows, geometry, detector)
    bucket = np.diff(edges(col0, col1, width)).astype(np.float64)
    comb = {"max": np.fmax, "min": np.fmin, "mean": np.add}[detector]
    lines = []
    for r in per_row:
        acc = comb(acc, r)
        have += 1
        if have == m:
            if detector == "mean":
                with np.errstate(divide="ignore", invalid="ignore"):
                    lines.append(20.0 * np.log10(acc / (m * bucket)))
            else:
                lines.append(acc)
            have, acc = empty_pending(geometry, detector)
    dt = np.float64 if detector == "mean" else np.float32
    out = np.array(lines, dtype=dt).reshape(len(lines), width)
    return out, (have, acc)


def ref_image(lines, height, scroll):
    """The image after `lines` (oldest first) went into an all-NaN ring of `height` lines: scroll
    +1 puts the newest at row height - 1 and older ones above it, -1 the newest at row 0."""
    lines = np.asarray(lines)
    img = np.full((height, lines.shape[1]), np.nan, lines.dtype)
    k = min(height, len(lines))
    if k:
        if scroll > 0:
            img[height - k:] = lines[-k:]
        else:
            img[:k] = lines[-k:][::-1]
    return img


def ref_holds(lines, start=None):
    """(last, max_hold, min_hold) after `lines`, from `start` = (max_hold, min_hold) or NaN."""
    lines = np.asarray(lines)
    w = lines.shape[1]
    nan = np.full(w, np.nan, lines.dtype)
    mx, mn = (nan, nan) if start is None else start
    if len(lines) == 0:
        return nan, mx, mn
    return lines[-1], np.fmax(mx, np.fmax.reduce(lines, axis=0)), np.fmin(mn, np.fmin.reduce(lines, axis=0))


def plant_specials(rows, geometry, m, inf=True):
    """Plants into rows (in place) inside [col0, col1): a NaN, -0.0 and 0.0, an all-NaN cell (every
    row of the first group, pixel 1's bucket) and, with `inf`, +inf, -inf and a cell of -inf only
    (the first group, the last pixel's bucket).  Returns the number of planted values."""
    col0, col1, width = geometry
    e = edges(col0, col1, width)
    g = min(m, len(rows))
    n = 0
    px = min(1, width - 1)
    rows[:g, e[px]:e[px + 1]] = np.nan
    n += g * int(e[px + 1] - e[px])
    if inf and width >= 3:
        rows[:g, e[width - 1]:e[width]] = -np.inf
        n += g * int(e[width] - e[width - 1])
    mid = int(e[width // 2]) if width >= 4 else None
    if mid is not None:
        r = len(rows) - 1
        rows[r, mid] = np.nan
        rows[0, mid] = -0.0
        if mid + 1 < col1:
            rows[0, mid + 1] = 0.0
        n += 3
        if inf:
            rows[r, int(e[width // 2 + 1])] = np.inf
            rows[0, int(e[width // 2 - 1])] = -np.inf
            n += 2
    return n


def poison_outside(rows, n, geometry):
    """+inf, NaN and 1e30 in turn in every column outside [col0, col1) (the columns at or beyond
    the row length n included): none of them may reach a result."""
    col0, col1, _ = geometry
    bad = np.array([np.inf, np.nan, 1e30], np.float32)
    for lo, hi in ((0, col0), (col1, rows.shape[1])):
        if hi > lo:
            rows[:, lo:hi] = bad[(np.arange(lo, hi)[None, :] + np.arange(len(rows))[:, None]) % 3]
    return rows
