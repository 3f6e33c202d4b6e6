"""CPU checks of the zoom-2 FC decimator's host tables and index maps (pc_tables.cpp fc_build_row /
fc_build_twiddles at zoom 2; kernel fc_decim_kernel<2, ...> in fc_kernels.hip), no
GPU needed:

* the one-stage model's input-rate response g = |H|^2 (rebuilt here from scipy's cheby1
  sections) leaves < 2e-8 of sum |g| beyond |k| = 256 (kFc2K);
* the response the library's own zoom-2 row holds (the row un-folded: G[k], G[k + 4096] from
  C[k][0], C[k][1], then the inverse DFT), together with the shipped zoom-2 frame-end maps,
  reproduces scipy.signal.decimate(x, 2) of the mixed input (pypanadapter_spectrum.py:2088-2098)
  to 2e-7 of its peak -- the bound test_pc_tables.py / test_fc_tables.py use for the
  1.4e-8-tail truncations;
* one window computed in numpy with the kernel's own thread maps and LDS addresses (passes A, B,
  C with the library's row in the kernel's pair order, the inverse stages 1..5 at their ps()
  addresses inside the window's array) equals ifft(fft(w) fft(g'))[::2] to fp64 rounding of the
  fp32 row;
* inverse stages 2..4 touch only their wave's slots at NB = 4."""
import numpy as np
import pytest
import scipy.signal as ss

from test_pc_tables import _call, _edge2

SOS = ss.cheby1(8, 0.05, 0.4, output="sos")
N, Z = 8192, 2
M, R1, NB = N // Z, N // Z // 256, N // Z // 1024      # 4096, 16, 4
K, P, J0 = 256, 3840, 128                              # kFc2K, kFc2P, K / Z
TW, ROW = 22, 23                                       # zfft__pc_tables: zoom-2 twiddles, row
BIG = N + 2 * (N // 32)                                # kBigSlots


def _g_full():
    imp = np.zeros(6000)
    imp[0] = 1
    h = ss.sosfilt(SOS, imp)
    return np.convolve(h, h[::-1])


def _lib_row(arg):
    """C[k][r], k < 4096, from the kernel's order: float2 index ((k3 256 + t) 2 + r."""
    v = _call(ROW, arg)
    assert v.size == 2 * N
    z = v[0::2] + 1j * v[1::2]
    C = np.zeros((M, Z), complex)
    for t in range(256):
        kp = (t >> 4) + 16 * (t & 15)
        for k3 in range(R1):
            for r in range(Z):
                C[kp + 256 * k3, r] = z[(k3 * 256 + t) * 2 + r]
    return C


def _lib_response(arg):
    """g'[k], |k| <= K, as the library's row holds it (and what it holds outside, for the check
    that the row is the truncated response): C[k][0] = (G[k] + G[k + M]) / (N sqrt 2),
    C[k][1] = W_N^k (G[k] - G[k + M]) / (N sqrt 2)."""
    C = _lib_row(arg)
    k = np.arange(M)
    c1 = C[:, 1] * np.exp(2j * np.pi * k / N)
    G = np.concatenate([C[:, 0] + c1, C[:, 0] - c1]) * (N * np.sqrt(2) / 2)
    g = np.fft.ifft(G)
    kk = np.arange(-K, K + 1)
    rest = np.delete(g, kk % N)
    return g[kk % N], np.abs(rest).sum()


def _lo(L, ratio):
    return np.sqrt(2) * np.exp(-2j * np.pi * np.mod(np.arange(L) * ratio, 1.0))


def test_fc2_truncation_tail():
    g = _g_full()
    c = len(g) // 2
    tail = np.abs(g[:c - K]).sum() + np.abs(g[c + K + 1:]).sum()
    assert tail < 2e-8 * np.abs(g).sum(), tail / np.abs(g).sum()


def test_fc2_twiddles():
    v = _call(TW)
    w = v[0::2] + 1j * v[1::2]
    assert w.size == M
    np.testing.assert_allclose(w, np.exp(-2j * np.pi * np.arange(M) / M), rtol=0, atol=1e-7)


@pytest.mark.parametrize("arg", [0, 437, 65536 + 437, 1048576 - 131072])
def test_fc2_row_is_the_truncated_modulated_response(arg):
    """arg / 2^20 = f_lo / fs.  The row un-folded is g e^(2 pi i ratio k) on |k| <= 256 and
    nothing elsewhere (to the row's fp32 rounding)."""
    got, rest = _lib_response(arg)
    g = _g_full()
    c = len(g) // 2
    kk = np.arange(-K, K + 1)
    want = g[c - K:c + K + 1] * np.exp(2j * np.pi * np.mod(arg / 2 ** 20 * kk, 1.0))
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-7 * np.abs(want).max())
    assert rest < 2e-6 * np.abs(want).sum(), rest


@pytest.mark.parametrize("L", [16384, 16385, 20006, 7680 * 3 + 5])
@pytest.mark.parametrize("arg", [0, 65536 + 437])
def test_fc2_model_plus_edge_maps_is_reference_decimate(L, arg):
    """The library's truncated zoom-2 response (the LO as its modulation, lo[2 m] on the
    outputs) plus the shipped maps on the mixed input = decimate(x lo, 2): both L mod 2, with
    and without an LO offset."""
    ratio = arg / 2 ** 20
    rng = np.random.default_rng(L)
    x = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    x += 3 * np.exp(2j * np.pi * 0.041 * np.arange(L))
    lo = _lo(L, ratio)
    ref = ss.decimate(x * lo, 2)
    g, _ = _lib_response(arg)
    nd = len(ref)
    out = np.convolve(x, g)[K:K + L][::Z][:nd] * lo[::Z][:nd]
    (UL, VL), (UR, VR) = _edge2(0, 0, shipped=True), _edge2(1, L % 2, shipped=True)
    CL, CR = UL @ VL.T, UR @ VR.T
    xm = x * lo
    out[:CL.shape[0]] += CL @ xm[:CL.shape[1]]
    out[nd - CR.shape[0]:] += (CR @ xm[::-1][:CR.shape[1]])[::-1]
    err = np.abs(out - ref).max() / np.abs(ref).max()
    print(f"fc2 model L={L} arg={arg}: {err:.3e}")
    assert err < 2e-7, err


def _ps(i):
    """ps<2>: one pad slot per 16 and one more per 256 (stage 5's lanes read 256 b0 apart)."""
    return i + (i >> 4) + (i >> 8)


def test_fc2_block_in_the_kernels_index_maps():
    """One window through the kernel's thread maps and LDS addresses with the library's row: y[j]
    for j in [128, 128 + 3840) equals the window's circular convolution with g', decimated by 2
    (the kernel multiplies by lo[2 m] afterwards; the row carries 1 / sqrt 2 for that)."""
    rng = np.random.default_rng(5)
    w = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    arg = 65536 + 437
    C = _lib_row(arg)
    z = _call(ROW, arg)
    zrow = z[0::2] + 1j * z[1::2]
    WM = lambda e: np.exp(-2j * np.pi * np.asarray(e) / M)
    dft = lambda R: np.exp(-2j * np.pi * np.outer(np.arange(R), np.arange(R)) / R)
    d16, d4 = dft(16), dft(4)
    big = np.full(BIG, np.nan, complex)              # the window's array, v2f slots
    for t in range(256):                              # pass A: pair n = 2t + 512 i, residues 0, 1
        j0 = t // (Z // 2)
        aA = 2 * t + 2 * (t >> 4)
        for r in range(2):
            v = np.array([w[2 * t + r + 512 * i] for i in range(16)])
            o = (d16 @ v) * WM(j0 * np.arange(16))
            for k1 in range(16):
                big[aA + 544 * k1 + r] = o[k1]
    assert not np.isnan(big[[2 * i + 2 * (i // 16) + r for i in range(N // 2) for r in (0, 1)]]).any()
    nxt = big.copy()
    for t in range(256):                              # pass B: k1 = t >> 4, j1 = t & 15, in place
        j1 = (t & 15) // (Z // 2)
        aB = 2 * (t & 15) + 544 * (t >> 4)
        for r in range(2):
            v = np.array([big[aB + 34 * i + r] for i in range(16)])
            o = (d16 @ v) * WM(16 * j1 * np.arange(16))
            for k2 in range(16):
                nxt[aB + 34 * k2 + r] = o[k2]
    big = nxt
    small = np.full(BIG, np.nan, complex)             # the inverse array: the same LDS, ps() slots
    for t in range(256):                              # pass C + MAC + inverse stage 1
        kp = (t >> 4) + 16 * (t & 15)
        aC = 544 * (t >> 4) + 34 * (t & 15)
        ea = d16 @ np.array([big[aC + 2 * j] for j in range(R1)])
        eb = d16 @ np.array([big[aC + 2 * j + 1] for j in range(R1)])
        # the thread's 16 table pairs: byte offset 16 t + 4096 j -> float2 (256 j + t) 2 + r
        c0 = np.array([zrow[(256 * j + t) * 2] for j in range(R1)])
        c1 = np.array([zrow[(256 * j + t) * 2 + 1] for j in range(R1)])
        np.testing.assert_array_equal(c0, C[kp + 256 * np.arange(R1), 0])
        yf = ea * c0 + eb * c1
        o = np.conj(d16) @ yf * np.conj(WM(kp * np.arange(R1)))
        for q in range(R1):
            small[_ps(kp) + 273 * q] = o[q]
            assert _ps(kp) + 273 * q == _ps(kp + 256 * q) < BIG
    used = {_ps(i) for i in range(M)}
    assert len(used) == M and not np.isnan(small[sorted(used)]).any()
    # stages 2..4: butterfly t + 256 h at + 1092 h (the lane exchanges between them as index maps)
    for S, lowf, basef in ((64, lambda u: u & 63, lambda t: (t & 63) + 256 * (t >> 6)),
                           (16, lambda u: u & 15, lambda t: (t & 15) + 64 * ((t >> 4) & 3) + 256 * (t >> 6)),
                           (4, lambda u: u & 3,
                            lambda t: (t & 3) + 16 * ((t >> 2) & 3) + 64 * ((t >> 4) & 3) + 256 * (t >> 6))):
        new = small.copy()
        for t in range(256):
            for h in range(NB):
                a0 = _ps(basef(t)) + 1092 * h
                st = S + (S >> 4)                   # 68, 17, 4: the pads folded into the strides
                idx = a0 + st * np.arange(4)
                assert list(idx) == [_ps(basef(t) + 1024 * h + S * a) for a in range(4)]
                new[idx] = np.conj(d4) @ small[idx] * np.conj(WM((M // (4 * S)) * lowf(t) * np.arange(4)))
        small = new
    y = np.zeros(M, complex)
    seen = set()
    for t in range(256):                              # stage 5: u = b0 + 16 (b1 + 4 b2 + 16 b3)
        for h in range(NB):
            u = t + 256 * h
            r = u // R1
            i5 = _ps(4 * ((r >> 4) & 3) + 16 * ((r >> 2) & 3) + 64 * (r & 3) + 256 * (u % R1))
            seen.update(range(i5, i5 + 4))
            y[u + (M // 4) * np.arange(4)] = np.conj(d4) @ small[i5 + np.arange(4)]
    assert seen == used
    # the row un-folded, all 8192 entries of its spectrum (its fp32 rounding included)
    c1 = C[:, 1] * np.exp(2j * np.pi * np.arange(M) / N)
    G = np.concatenate([C[:, 0] + c1, C[:, 0] - c1]) * (N / 2)
    direct = np.fft.ifft(np.fft.fft(w) * G)[::Z]
    err = np.abs(y - direct).max() / np.abs(direct).max()
    assert err < 1e-12, err
    # and on the block's outputs that is the linear convolution with the truncated response
    g, _ = _lib_response(arg)
    jv = np.arange(J0, J0 + P)
    lin = np.convolve(w, g)[K:K + N][::Z] / np.sqrt(2)
    err = np.abs(y[jv] - lin[jv]).max() / np.abs(lin[jv]).max()
    assert err < 1e-6, err               # the row's fp32 rounding outside |k| <= 256


def test_fc2_inverse_stages_2_to_4_are_wave_local():
    """Every slot a wave's butterflies read or write in stages 2..4 has b0 = i >> 8 equal to
    (t >> 6) + 4 h, and each stage's slots of one wave are the same set: the exchanges between
    them stay in the wave's registers (xchg_54, xchg_32) at NB = 4 too."""
    bases = ((lambda u: (u & 63) + 256 * (u >> 6), 64),
             (lambda u: (u & 15) + 64 * ((u >> 4) & 3) + 256 * (u >> 6), 16),
             (lambda u: (u & 3) + 16 * ((u >> 2) & 3) + 64 * ((u >> 4) & 3) + 256 * (u >> 6), 4))
    allslots = set()
    for wv in range(4):
        sets = []
        for base, S in bases:
            slots = set()
            for t in range(64 * wv, 64 * wv + 64):
                for h in range(NB):
                    for a in range(4):
                        i = base(t) + 1024 * h + S * a
                        assert i >> 8 == (t >> 6) + 4 * h
                        slots.add(i)
            sets.append(slots)
        assert sets[0] == sets[1] == sets[2]
        assert len(sets[0]) == 256 * NB
        allslots |= sets[0]
    assert allslots == set(range(M))


def test_fc2_lane_exchange_maps_match_the_stage_bases():
    """xchg_54: lane l, register a holds element l + 64 a and ends with (l & 15) + 16 a + 64 (l >> 4);
    xchg_32 then gives (l & 3) + 4 a + 16 ((l >> 2) & 3) + 64 (l >> 4).  With the wave's offset
    256 (t >> 6) + 1024 h these are stage 3's and stage 4's butterfly inputs (their bases + 16 a,
    + 4 a), so the same exchanges serve the 4096-point inverse."""
    for l in range(64):
        for a in range(4):
            assert (l & 15) + 16 * a + 64 * (l >> 4) == ((l & 15) + 64 * ((l >> 4) & 3)) + 16 * a
            assert (l & 3) + 4 * a + 16 * ((l >> 2) & 3) + 64 * (l >> 4) == \
                ((l & 3) + 16 * ((l >> 2) & 3) + 64 * ((l >> 4) & 3)) + 4 * a
