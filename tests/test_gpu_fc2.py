"""GPU parity of decimator path 7, "FC wherever a form exists" (fc_kernels.hip):

* zoom 2 -- the reference's default fft_ratio (pypanadapter_spectrum.py:1497), one
  decimate(x, 2) (S:2096-2098) -- as fc_decim_kernel<2, ...>: two residues of a 4096-point DFT
  per 8192-sample window, the one-stage model truncated at |k| <= 256 (tail 1.4e-8 of sum |g|),
  3840 outputs per window, the frame ends by zoom 2's maps;
* zoom >= 16: after the three-stage FC head the remaining stages as FC launches on the head's
  complex64 output ("fc_tail": three stages at a time, then two or one; unit LO table, their
  own zoom's maps), while a launch's input has >= 16384 samples.

Against the float64 oracle of the reference's cascade, its rows and the golden rows recorded
from the reference.  The decimated-IQ gates are the measured worst of this file + ~7 % (FC sums
in a fixed order, so the worst repeats; ledger profiles/r08fc2/ledger_fc2.json)."""
import numpy as np
import pytest

from conftest import assert_row_close, case_input, check_rel, golden_cases, golden_rows, window_of
from test_gpu_pc import PC_TOL, _encode, _frames

pytestmark = pytest.mark.gpu
# measured worst per key (profiles/r08fc2/ledger_fc2.json) + ~7 %: 4.906e-7, 4.390e-7, 5.029e-7 /
# 4.096e-7 / 3.924e-7; chains 6.435e-7 (16), 3.449e-7 (32), 7.062e-7 (64), 3.256e-7 (512).  All
# inside their caps: 6.5e-7 at zoom 2 (the bound include/zfft.h documents for FC), 7.5e-6 for the
# chains (what the present tails are held to, and what the fallback cases here keep).
FC2_TOL = {"fc2/decimate": 5.25e-7, "fc2/decimate_lo": 4.70e-7, "fc2/format/complex32": 5.38e-7,
           "fc2/format/cu8": 4.38e-7, "fc2/format/f32": 4.20e-7}
CHAIN_TOL = {16: 6.89e-7, 32: 3.69e-7, 64: 7.56e-7, 512: 3.48e-7}
assert max(FC2_TOL.values()) <= 6.5e-7 and max(CHAIN_TOL.values()) <= 7.5e-6
# both L mod 2 at the shortest frame, a window ending exactly at the frame end (window b starts at
# 7680 b - 256) and one sample past it, a short last block, a cfg2-sized frame
FC2_LENGTHS = [16384, 16385, 7680 * 2 + 8192 - 256, 7680 * 2 + 8192 - 256 + 1, 7680 * 3 + 5, 299008 + 3]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zfft_lib):
    from pypanadapter_amd import device_count
    assert device_count() >= 1, "GPU tests need a HIP device"


def _decimate_named(plan, x):
    plan.set_timing(True)
    d = plan.decimate(x)
    return d, plan.launch_names()


def _noise(rng, L, f):
    x = (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(np.complex64)
    return x + np.exp(2j * np.pi * f * np.arange(L)).astype(np.complex64)


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
def test_fc2_decimate_vs_oracle(oracle_lib, flip):
    """One frame per call (the frame split into runs of blocks over many workgroups)."""
    from pypanadapter_amd import ZoomFFT
    rng = np.random.default_rng(5400 + flip)
    for L in FC2_LENGTHS:
        x = _noise(rng, L, 0.031)
        with ZoomFFT(2048, 2, 2.4e6, flip=flip) as plan:
            plan.set_path(7)
            d, names = _decimate_named(plan, x)
        assert "fc_decim" in names, names
        ref = oracle_lib.zoomfft(x[::-1].copy() if flip else x, 2, 2.4e6)
        assert d.shape == ref.shape, (L, d.shape, ref.shape)
        e = check_rel(d, ref, FC2_TOL["fc2/decimate"], "fc2/decimate", (L, flip))
        print(f"fc2/decimate L={L} flip={flip}: {e:.3e}")


def test_fc2_lo_offsets_vs_oracle(oracle_lib):
    """The LO moved into the filter: f_lo across the band (and past it)."""
    from pypanadapter_amd import ZoomFFT
    rng = np.random.default_rng(5470)
    L = 299008 + 5
    x = (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(np.complex64)
    for f_lo in (1.0, 150e3 + 1.0, -300e3 + 1.0, 1.1e6, 0.0):
        with ZoomFFT(2048, 2, 2.4e6, f_lo=f_lo) as plan:
            plan.set_path(7)
            d = plan.decimate(x)
        ref = oracle_lib.zoomfft(x, 2, 2.4e6, f_lo=f_lo)
        e = check_rel(d, ref, FC2_TOL["fc2/decimate_lo"], "fc2/decimate_lo", f_lo)
        print(f"fc2/decimate_lo f_lo={f_lo}: {e:.3e}")


@pytest.mark.parametrize("fmt", ["complex32", "cu8", "f32"])
def test_fc2_input_formats_and_lo(oracle_lib, fmt):
    """The raw formats with np.flip, and per-frame LO rows (one zoom-2 filter table each); the
    -300 kHz row is the band-edge case that rejected an earlier zoom-2 form."""
    from pypanadapter_amd import ZoomFFT
    F, L, N = 3, 65536 + 1, 1024
    x = _frames(F, L, N, 2, 512, seed0=6700)
    arr, vals = _encode(x, fmt)
    with ZoomFFT(N, 2, 2.4e6, n_win=512, in_dtype=fmt, flip=True) as plan:
        plan.set_path(7)
        d, names = _decimate_named(plan, arr[1])
        f_lo = [1.0, 150e3 + 1.0, -300e3 + 1.0]
        plan.set_lo_frames(f_lo, 1)
        rows = plan.rows(arr)
    assert "fc_decim" in names, names
    key = f"fc2/format/{fmt}"
    e = check_rel(d, oracle_lib.zoomfft(vals[1, ::-1].copy(), 2, 2.4e6), FC2_TOL[key], key)
    print(f"fc2/format/{fmt}: {e:.3e}")
    for f in range(F):
        assert_row_close(rows[f], oracle_lib.psd_row(vals[f, ::-1].copy(), 2.4e6, N, 2, 512, f_lo=f_lo[f % 3]),
                         f"{fmt} frame {f}")


@pytest.mark.parametrize("N,L,F", [(4096, 299008, 4), (1024, 65536, 4), (2048, 131072 + 3, 3)])
def test_fc2_rows_vs_oracle(oracle_lib, N, L, F):
    from pypanadapter_amd import ZoomFFT
    W = N // 2
    x = _frames(F, L, N, 2, W, seed0=5500 + N // 1024)
    with ZoomFFT(N, 2, 2.4e6, n_win=W) as plan:
        plan.set_path(7)
        rows = plan.rows(x)
    for f in range(F):
        assert_row_close(rows[f], oracle_lib.psd_row(x[f], 2.4e6, N, 2, W), f"N={N} L={L} frame {f}")


def test_fc2_golden_rows():
    """Every zoom-2 golden row the reference recorded whose frame FC takes (>= 16384 samples)."""
    from pypanadapter_amd import ZoomFFT
    ran = []
    for c in golden_cases()["cases"]:
        if c["zoom"] != 2 or c["n_samples"] < 16384:
            continue
        x = case_input(c)
        with ZoomFFT(c["n_fft"], 2, c["fs"], n_win=c["n_win"], window=window_of(c["window"]),
                     f_lo=c["f_lo"]) as plan:
            plan.set_path(7)
            plan.set_timing(True)
            row = plan.rows(x)
            assert "fc_decim" in plan.launch_names()
        assert_row_close(row, golden_rows()[c["name"]], c["name"])
        ran.append(c["name"])
    assert {"z2_default_ui", "fs_2p56M"} <= set(ran), ran


def test_fc2_batch_rows_vs_oracle(oracle_lib):
    """A 1024-frame batch: one workgroup walks each frame, every window after the first taking
    the previous window's last 512 samples from registers and the rest from the prefetch (the
    few-frame calls above split frames into one-block runs and never carry).  Picked frames
    against the oracle, the others zero."""
    import torch
    from pypanadapter_amd import ZoomFFT
    F, L, N, W = 1024, 32768 + 1, 1024, 512
    picks = (0, 511, F - 1)
    dev = torch.device("cuda:0")
    x = torch.zeros((F, L, 2), device=dev, dtype=torch.float32)
    xs = {f: _frames(1, L, N, 2, W, seed0=8500 + f)[0] for f in picks}
    for f, v in xs.items():
        x[f] = torch.from_numpy(np.ascontiguousarray(v).view(np.float32).reshape(L, 2)).to(dev)
    rows = torch.empty((F, W), device=dev, dtype=torch.float32)
    with ZoomFFT(N, 2, 2.4e6, n_win=W) as plan:
        plan.set_path(7)
        plan.set_timing(True)
        st = torch.cuda.current_stream()
        plan.process_device(x.data_ptr(), L, F, rows.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        names = plan.launch_names()
    assert names[0] == "fc_decim", names
    got = rows.cpu().numpy()
    for f in picks:
        assert_row_close(got[f], oracle_lib.psd_row(xs[f], 2.4e6, N, 2, W), f"frame {f}")


def test_fc2_close_to_tiles():
    """FC and zoom 2's tiles (path 4) on the same frames: two fp32 forms of one stage, within
    the tiles' documented tolerance."""
    from pypanadapter_amd import ZoomFFT
    x = _frames(4, 131072 + 1, 2048, 2, 1024, seed0=6960)
    out = {}
    for path in (4, 7):
        with ZoomFFT(2048, 2, 2.4e6) as plan:
            plan.set_path(path)
            out[path] = np.stack([plan.decimate(x[f]) for f in (0, 3)])
    check_rel(out[7], out[4], PC_TOL, "fc2/vs_tiles")


def test_fc2_size_independent_properties():
    """Determinism, frame-order equivariance and exact x2 scaling (+12.04 dB) at a batch."""
    from pypanadapter_amd import ZoomFFT
    x = _frames(12, 65536 + 1, 1024, 2, 512, seed0=7500)
    with ZoomFFT(1024, 2, 2.4e6) as plan:
        plan.set_path(7)
        a = plan.rows(x)
        b = plan.rows(x)
        perm = np.random.default_rng(1).permutation(12)
        c = plan.rows(x[perm])
        d = plan.rows(2 * x)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(c, a[perm])
    np.testing.assert_allclose(d - a, 20 * np.log10(4.0), atol=2e-4)


# ---- zoom >= 16: the FC head, then FC tails ----

@pytest.mark.parametrize("zoom,lengths", [(16, [131072 + 5, 262144, 299008]), (64, [(1 << 20) + 3]),
                                          (32, [262144 + 3]), (512, [(1 << 20) + 3])],
                         ids=["zoom16", "zoom64", "zoom32", "zoom512"])
def test_fc_chain_decimate_vs_oracle(oracle_lib, zoom, lengths):
    """Zoom 16: one fc_decim_kernel<2> tail; 32: one <4>; 64: one <8>; 512 on 2^20 + 3 samples:
    two <8> tails (131073 and 16385 samples in).  No XA stage, no tiles."""
    from pypanadapter_amd import ZoomFFT
    rng = np.random.default_rng(4750 + zoom)
    for L in lengths:
        x = _noise(rng, L, 0.0023)
        with ZoomFFT(4096, zoom, 2.4e6) as plan:
            plan.set_path(7)
            d, names = _decimate_named(plan, x)
        assert names[0] == "fc_decim" and "fc_tail" in names, names
        assert not {"xa_stage", "pc_tail", "exact_forward"} & set(names), names
        assert names.count("fc_tail") == (2 if zoom == 512 else 1), names
        ref = oracle_lib.zoomfft(x, zoom, 2.4e6)
        assert d.shape == ref.shape, (L, d.shape, ref.shape)
        e = check_rel(d, ref, CHAIN_TOL[zoom], f"fc_chain/zoom{zoom}", L)
        print(f"fc_chain/zoom{zoom} L={L}: {e:.3e}")


def test_fc_chain_falls_back_below_16384(oracle_lib):
    """Zoom 16 on 16390 samples: the head's output (2049 samples) is too short for an FC launch,
    the blocked passes take the last stage; zoom 128 on 299008: one <8> tail, then the blocked
    passes on its 4672-sample output."""
    from pypanadapter_amd import ZoomFFT
    rng = np.random.default_rng(4790)
    for zoom, L, ntail in ((16, 16390, 0), (128, 299008, 1)):
        x = _noise(rng, L, 0.0023)
        with ZoomFFT(4096, zoom, 2.4e6) as plan:
            plan.set_path(7)
            d, names = _decimate_named(plan, x)
        assert names[0] == "fc_decim" and names.count("fc_tail") == ntail, names
        assert "exact_backward" in names and "xa_stage" not in names, names
        check_rel(d, oracle_lib.zoomfft(x, zoom, 2.4e6), 7.5e-6, f"fc_chain/fallback_zoom{zoom}", L)


@pytest.mark.parametrize("zoom,N,W,L,F", [(16, 4096, 256, 299008, 3), (64, 16384, 256, (1 << 20) + 3, 2)])
def test_fc_chain_rows_vs_oracle(oracle_lib, zoom, N, W, L, F):
    from pypanadapter_amd import ZoomFFT
    x = _frames(F, L, N, zoom, W, seed0=5700 + zoom)
    with ZoomFFT(N, zoom, 2.4e6, n_win=W) as plan:
        plan.set_path(7)
        plan.set_timing(True)
        rows = plan.rows(x)
        names = plan.launch_names()
    assert names[0] == "fc_decim" and "fc_tail" in names and "xa_stage" not in names, names
    for f in range(F):
        assert_row_close(rows[f], oracle_lib.psd_row(x[f], 2.4e6, N, zoom, W), f"zoom {zoom} frame {f}")


def test_fc_chain_golden_rows():
    """The golden rows z16_n4096 and z64_n16384_short: FC tails where the head's output has
    >= 16384 samples, else the fallback's launches."""
    from pypanadapter_amd import ZoomFFT
    ran = 0
    for c in golden_cases()["cases"]:
        if c["name"] not in ("z16_n4096", "z64_n16384_short"):
            continue
        x = case_input(c)
        with ZoomFFT(c["n_fft"], c["zoom"], c["fs"], n_win=c["n_win"], window=window_of(c["window"]),
                     f_lo=c["f_lo"]) as plan:
            plan.set_path(7)
            plan.set_timing(True)
            row = plan.rows(x)
            names = plan.launch_names()
        assert names[0] == "fc_decim", names
        if (c["n_samples"] + 7) // 8 >= 16384:
            assert "fc_tail" in names and "xa_stage" not in names, names
        else:
            assert "fc_tail" not in names and "exact_backward" in names, names
        assert_row_close(row, golden_rows()[c["name"]], c["name"])
        ran += 1
    assert ran == 2
