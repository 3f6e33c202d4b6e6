"""The row history's rule (include/zfft.h, zfft_plan_history) in numpy: the quantiser in float32,
bit for bit what the library must give, and a view as viewport_ref.ref_lines over the unpacked
rows, with NaN lines where a row is not in the store.  Used by test_history_host.py (against the
host quantiser) and test_gpu_history.py (against the device)."""
import numpy as np

import viewport_ref as vr

FORMATS = {"f32": 0, "u16": 1, "u8": 2}
KMAX = {"u8": 254, "u16": 65534}
# the level ranges the rule's three properties were checked on
RANGES = ((-220.0, -20.0), (-160.0, -40.0), (-250.5, -99.25), (0.0, 100.0), (-1e-3, 1e-3), (-300.0, 300.0))


def constants(fmt, db_min, db_max):
    """(K, lo, inv, step): float32 constants, the divisions in double and rounded once."""
    K = KMAX[fmt]
    rng = np.float64(db_max) - np.float64(db_min)
    return K, np.float32(db_min), np.float32(np.float64(K) / rng), np.float32(rng / np.float64(K))


def pack(v, fmt, db_min, db_max):
    """uint16 codes of float32 values: NaN -> 0, else 1 + rint(clip((v - lo) * inv, 0, K))."""
    K, lo, inv, _ = constants(fmt, db_min, db_max)
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v - lo).astype(np.float32) * inv  # a float32 difference, then a float32 product
        t = np.fmin(np.fmax(t.astype(np.float32), np.float32(0)), np.float32(K))
        code = 1 + np.rint(t).astype(np.int64)  # round half to even
    code[np.isnan(v)] = 0
    return code.astype(np.uint16)


def unpack(codes, fmt, db_min, db_max):
    """float32 values of codes: 0 -> NaN, else lo + float32(code - 1) * step, two roundings."""
    _, lo, _, step = constants(fmt, db_min, db_max)
    c = np.asarray(codes).astype(np.int64)
    prod = ((c - 1).astype(np.float32) * step).astype(np.float32)
    out = (lo + prod).astype(np.float32)
    out[c == 0] = np.nan
    return out


def stored(rows, fmt, db_min, db_max):
    """What the store returns for float32 rows: unpack(pack(v)), or v itself for f32."""
    rows = np.asarray(rows, dtype=np.float32)
    if fmt == "f32":
        return rows.copy()
    return unpack(pack(rows, fmt, db_min, db_max), fmt, db_min, db_max).reshape(rows.shape)


def ref_view(kept, oldest, n, first, lines, geometry, detector, m):
    """(lines, width) of the window over `kept`, the unpacked rows [oldest, oldest + len(kept)):
    line L covers rows [first + L m, first + (L + 1) m) and is all NaN unless they are all kept.
    float32 for max / min, float64 for mean."""
    width = geometry[2]
    out = np.full((lines, width), np.nan, np.float64 if detector == "mean" else np.float32)
    seen = oldest + len(kept)
    for L in range(lines):
        a = first + L * m
        if a >= oldest and a + m <= seen:
            got, pend = vr.ref_lines(kept[a - oldest:a - oldest + m], n, geometry, detector, m)
            assert len(got) == 1 and pend[0] == 0
            out[L] = got[0]
    return out
