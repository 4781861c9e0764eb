"""float64 statements of the Ddc's definition (include/gr4pm_hip.h), for the tests.

K channels, decimation D, real prototype h[0 .. L-1], x[i] = 0 before the first sample, whose absolute index is start:
    w_k = llrint(f_k 2^32) mod 2^32,   phi_k(i) = (w_k i) mod 2^32   (integers)
    y_k[n] = sum_t h[t] x[i - t] exp(-2 pi j phi_k(i - t) / 2^32),   i = start + n D + D - 1
ddc64() computes exactly these lines (mix, np.convolve, keep every D-th sample from D - 1 on); ddc64_rotated() is the
form the kernel implements (rotated taps g_k[t] = h[t] exp(+2 pi j phi_k(t) / 2^32), one rotator per output item) and is
pinned to the former by tests/test_ddc_ref.py; ddc64_direct() evaluates single items with Python integers for the
phases.  All phases are integers modulo 2^32 before they become an angle: nothing here loses precision at a large
stream position."""
import math

import numpy as np

EPS32 = 2.0 ** -24
TWO32 = 1 << 32


def frequency_word(f):
    """llrint(f 2^32) mod 2^32 (ties to even, as llrint in the default rounding mode); fmod is exact"""
    return round(math.fmod(float(f), 1.0) * 4294967296.0) % TWO32


def quantised(f):
    """w / 2^32 folded to [-0.5, 0.5)"""
    w = frequency_word(f)
    return (w - TWO32 if w >= TWO32 // 2 else w) / 4294967296.0


def phases(w, first, n):
    """phi(i) = (w i) mod 2^32 for i = first .. first + n - 1, as uint64 (w and i mod 2^32 are below 2^32: no overflow)"""
    i = (np.arange(n, dtype=np.uint64) + np.uint64(first % TWO32)) & np.uint64(TWO32 - 1)
    return (np.uint64(w) * i) & np.uint64(TWO32 - 1)


def unit(phi, sign):
    """exp(sign 2 pi j phi / 2^32)"""
    return np.exp(sign * 2j * np.pi * (phi.astype(np.float64) / 4294967296.0))


def ddc64(x, h, D, freqs, start=0):
    """the definition, literally, in complex128.  [K, len(x) // D]"""
    x = np.asarray(x, dtype=np.complex128)
    h = np.asarray(h, dtype=np.float64)
    F = x.size // D
    y = np.zeros((len(freqs), F), dtype=np.complex128)
    for k, f in enumerate(freqs):
        z = x * unit(phases(frequency_word(f), start, x.size), -1.0)
        y[k] = np.convolve(h, z)[D - 1::D][:F]
    return y


def rotated_taps(h, freqs):
    """[K, L]: g_k[t] = h[t] exp(+2 pi j phi_k(t) / 2^32)"""
    h = np.asarray(h, dtype=np.float64)
    return np.stack([h * unit(phases(frequency_word(f), 0, h.size), 1.0) for f in freqs])


def ddc64_rotated(x, h, D, freqs, start=0, frames_per_block=1024):
    """y_k[n] = r_k[n] sum_t g_k[t] x[i - t],  r_k[n] = exp(-2 pi j phi_k(i) / 2^32): windows of the stream times the
    tap table, block by block of frames"""
    x = np.asarray(x, dtype=np.complex128)
    g = rotated_taps(h, freqs)
    K, L = g.shape
    F = x.size // D
    xp = np.concatenate([np.zeros(L - 1, np.complex128), x[:F * D]])
    # window n: xp[n D + D - 1 .. n D + D - 1 + L - 1] = x[i - L + 1 .. i]; tap t takes its item L - 1 - t
    win = np.lib.stride_tricks.sliding_window_view(xp, L)[D - 1::D][:F]
    gt = np.ascontiguousarray(g[:, ::-1].T)
    y = np.zeros((K, F), dtype=np.complex128)
    for lo in range(0, F, frames_per_block):
        y[:, lo:lo + frames_per_block] = (win[lo:lo + frames_per_block] @ gt).T
    for k, f in enumerate(freqs):
        w = frequency_word(f)
        i = (np.arange(F, dtype=np.uint64) * np.uint64(D) + np.uint64((start + D - 1) % TWO32)) & np.uint64(TWO32 - 1)
        y[k] *= unit((np.uint64(w) * i) & np.uint64(TWO32 - 1), -1.0)
    return y


def ddc64_direct(x, h, D, freqs, start, items):
    """the definition for the output items `items`, one sum each, the phases with Python integers.  [K, len(items)]"""
    x = np.asarray(x, dtype=np.complex128)
    h = np.asarray(h, dtype=np.float64)
    y = np.zeros((len(freqs), len(items)), dtype=np.complex128)
    for k, f in enumerate(freqs):
        w = frequency_word(f)
        for c, n in enumerate(items):
            j = n * D + D - 1  # index into x; the absolute index is start + j
            acc = 0.0 + 0.0j
            for t in range(min(h.size, j + 1)):
                phi = (w * (start + j - t)) % TWO32
                acc += h[t] * x[j - t] * complex(math.cos(2.0 * math.pi * phi / 4294967296.0),
                                                 -math.sin(2.0 * math.pi * phi / 4294967296.0))
            y[k, c] = acc
    return y


def kaiser_taps64(D, L, passband=0.25, stopband=0.75):
    """the design gr4pm_ddc_taps states, in numpy, in double (not rounded to float), for any length L"""
    dw = 2.0 * np.pi * (stopband - passband) / D
    A = 2.285 * dw * (L - 1) + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50 else (0.5842 * (A - 21.0) ** 0.4 + 0.07886 * (A - 21.0) if A >= 21 else 0.0)
    fc = 0.5 * (passband + stopband) / D
    t = np.arange(L) - 0.5 * (L - 1)
    h = 2.0 * fc * np.sinc(2.0 * fc * t) * np.kaiser(L, beta)
    return h / np.sum(h)


def window_max(x, D, L):
    """per output item n: max |x| over the L samples it is made of (x[i - L + 1 .. i], i = n D + D - 1)"""
    F = len(x) // D
    a = np.concatenate([np.zeros(L - 1), np.abs(np.asarray(x)[:F * D].astype(np.complex128))])
    c = np.maximum.accumulate  # running maxima over blocks of L: max over any window of L in two lookups
    pad = (-a.size) % L
    b = np.concatenate([a, np.zeros(pad)]).reshape(-1, L)
    fwd = c(b, axis=1).reshape(-1)          # max of the block's items up to here
    bwd = c(b[:, ::-1], axis=1)[:, ::-1].reshape(-1)  # max of the block's items from here on
    lo = np.arange(F) * D + D - 1           # window n: a[lo .. lo + L - 1]
    return np.maximum(bwd[lo], fwd[lo + L - 1])
