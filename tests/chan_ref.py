"""Reference of the channeliser: the rule of include/zfft.h (zfft_plan_chan) in numpy float64,
written straight from the formula -- never a call into the library.

    y[m, c] = sum_{k<T} h[k] x[m D - k] exp(-2 pi i c (m D - k) / M),   m D >= the start

as a window sum into w[n mod M] (n = m D - k the absolute sample index, a Python int) and
np.fft.fft.  x is whatever the plan's in_dtype loader makes of the caller's samples in float32
(tap_ref.loader), 0 before the start of the count.  The error gate is derived, not measured
(`gate`): P rounded multiply-adds per branch, and per radix-2-equivalent level of the transform a
complex multiply (sqrt 5 u), a twiddle rounded once from float64 (u) and an add (u), 4.24 u <= 5 u
of the l1 norm; + 2 for second order."""
import numpy as np

# (M, P, D): both decimations, P = 1, the T = 2048 halo, the largest M; and, for the form
# boundary of the kernel (P <= 8: coefficients in registers, longer branches: in LDS), P = 9 and
# P = 12 beside the P = 8 cases, on both first radices (log2 M even and odd) and both D
CASES = [(8, 1, 8), (8, 3, 4), (16, 4, 16), (64, 8, 32), (128, 4, 64), (256, 8, 128), (1024, 2, 512),
         (16, 9, 8), (32, 12, 32)]


def ceil_div(a, d):
    return -(-int(a) // int(d))


def steps(n0, n, D):
    """Steps of a push of n samples at count n0 (n0 at or after the start)."""
    return max(0, ceil_div(n0 + n, D) - ceil_div(n0, D))


def step_indices(n0, n, D):
    """The m of those steps, Python ints."""
    return list(range(ceil_div(n0, D), max(ceil_div(n0 + n, D), ceil_div(n0, D))))


def ref_chan(x, n_first, M, D, h, ms):
    """y[m, c], m in ms (Python ints), c < M, for the stream whose sample n_first + i is x[i] and
    every other sample 0; complex128, (len(ms), M)."""
    x = np.asarray(x, dtype=np.complex128)
    h = np.asarray(h, dtype=np.float64)
    T = h.size
    k = np.arange(T, dtype=np.int64)
    out = np.zeros((len(ms), M), dtype=np.complex128)
    for j, m in enumerate(ms):
        top = int(m) * int(D)                 # the absolute index of x[m D]
        rel = (top - int(n_first)) - k        # where x[m D - k] lies in x
        ok = (rel >= 0) & (rel < x.size)
        xv = np.where(ok, x[np.clip(rel, 0, max(x.size - 1, 0))], 0.0)
        s = (top % M - k) % M                 # (m D - k) mod M
        w = np.zeros(M, dtype=np.complex128)
        np.add.at(w, s, h * xv)
        out[j] = np.fft.fft(w)
    return out


def ref_push(x, n0, M, D, h):
    """All steps of one push of x at count n0 (the past all zero)."""
    return ref_chan(x, n0, M, D, h, step_indices(n0, len(x), D))


def gate(h, M, P, xmax):
    h = np.asarray(h, dtype=np.float64)
    return (P + 5 * int(np.log2(M)) + 2) * 2.0 ** -24 * np.abs(h).sum() * float(xmax)


def impulse_gate(h, M, P, amp):
    """`gate` for an input with a single non-zero sample: sum|h| max|x| is max|h| amp."""
    h = np.asarray(h, dtype=np.float64)
    return (P + 5 * int(np.log2(M)) + 2) * 2.0 ** -24 * np.abs(h).max() * float(amp)
