"""CPU checks of the persistence spectrum: the binning rule of include/zfft.h as
persistence_ref.ref_hist states it, pinned on hand-made values, and the C-ABI's new names."""
import numpy as np

import persistence_ref as pr
from test_host import header_functions

NAMES = ["zfft_plan_persistence", "zfft_persistence_shape", "zfft_persistence_push_device",
         "zfft_persistence_push", "zfft_persistence_decay", "zfft_persistence_reset",
         "zfft_persistence_read"]


def test_rule_on_hand_made_values():
    """lo = -100, 8 levels of 5 dB: db_min and every interior edge open their level, db_max and
    everything above, below, NaN and the infinities count nowhere, the largest float below db_max
    is in the top level."""
    vals = np.array([[v for v, _ in pr.EDGE_VALUES]], dtype=np.float32)
    hist = pr.ref_hist(vals, pr.EDGE_LEVELS, pr.EDGE_MIN, pr.EDGE_MAX, vals.shape[1])
    assert hist.shape == (8, vals.shape[1]) and hist.dtype == np.uint32
    for j, (v, level) in enumerate(pr.EDGE_VALUES):
        want = np.zeros(8, dtype=np.uint32)
        if level is not None:
            want[level] = 1
        np.testing.assert_array_equal(hist[:, j], want, err_msg=f"value {v!r}")
    assert vals[0, 9] < np.float32(-60.0) and vals[0, 9] > np.float32(-60.001)


def test_rule_counts_rows_and_leaves_the_tail_columns():
    rows = np.array([[-99.0, -61.0, -72.5, -72.5], [-99.0, -200.0, -72.5, -72.5],
                     [-97.5, np.nan, -77.4, -72.5]], dtype=np.float32)
    hist = pr.ref_hist(rows, 8, -100.0, -60.0, 3)
    assert hist.sum() == 7 and not hist[:, 3].any()  # column 3 is beyond row_length
    assert hist[0, 0] == 3 and hist[7, 1] == 1 and hist[5, 2] == 2 and hist[4, 2] == 1
    # -0.0 is a level like any other when the range holds it
    z = pr.ref_hist(np.array([[-0.0, 0.0]], dtype=np.float32), 2, 0.0, 1.0, 2)
    np.testing.assert_array_equal(z, [[1, 1], [0, 0]])


def test_plant_edges_covers_every_edge():
    rows = np.full((37, 50), -80.0, dtype=np.float32)
    n = pr.plant_edges(rows, 5, -100.0, -60.0, 48)
    assert n == 12 and not np.any(rows[:, 48:] != -80.0)
    hist = pr.ref_hist(rows, 5, -100.0, -60.0, 48)
    # 6 edges (db_max uncounted) + the float below db_max; the six other plants count nowhere
    assert hist.sum() == 37 * 48 - 12 + 6


def test_new_names_are_declared_and_exported(zfft_lib):
    from pypanadapter_amd import _lib
    declared = header_functions()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert getattr(zfft_lib, name).argtypes is not None, name
