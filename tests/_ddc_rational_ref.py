"""float64 statements of the rational Ddc's definition (include/gr4pm_hip.h), for the tests.

K channels, resampling by I / D, real prototype h[0 .. L-1] at the rate I fs (P = ceil(L / I), h[t] = 0 for t >= L),
x[i] = 0 before the first sample, whose absolute index is start.  Output item n, counted from the handle's start:
    m_n = n D + D - 1,   j_n = m_n div I  (the input index is start + j_n),   p_n = m_n mod I
    y_k[n] = sum_s h[p_n + s I] x[j_n - s] exp(-2 pi j phi_k(start + j_n - s) / 2^32)
N samples make floor(N I / D) items.  rddc64() computes these lines literally (mix, zero-stuff by I, np.convolve with
h, keep m = n D + D - 1); rddc64_rotated() is the form the kernel implements (rotated taps g_k[p][s] = h[p + s I]
exp(+2 pi j phi_k(s) / 2^32), one rotator per item) and is pinned to the former by tests/test_ddc_rational_ref.py;
rddc64_direct() evaluates single items with Python integers for the phases.  Frequency words and phases are
_ddc_ref's: integers modulo 2^32 before they become an angle."""
import math

import numpy as np

import _ddc_ref as dref
from _ddc_ref import EPS32, TWO32, frequency_word, phases, unit  # noqa: F401  (what the tests take from here)


def item_count(N, I, D):
    return N * I // D


def items(N, I, D):
    """(j, p) of the floor(N I / D) items N samples make: the input index counted from the start, and the branch"""
    m = np.arange(item_count(N, I, D), dtype=np.int64) * D + (D - 1)
    return m // I, m % I


def rddc64(x, h, I, D, freqs, start=0):
    """the definition, literally, in complex128.  [K, len(x) I // D]"""
    x = np.asarray(x, dtype=np.complex128)
    h = np.asarray(h, dtype=np.float64)
    F = item_count(x.size, I, D)
    y = np.zeros((len(freqs), F), dtype=np.complex128)
    for k, f in enumerate(freqs if F else []):
        u = np.zeros(x.size * I, dtype=np.complex128)
        u[::I] = x * unit(phases(frequency_word(f), start, x.size), -1.0)
        y[k] = np.convolve(h, u)[D - 1::D][:F]
    return y


def branch_taps(h, I):
    """[I, P]: row p is h[p::I], zeros after its end"""
    h = np.asarray(h, dtype=np.float64)
    P = -(-h.size // I)
    return np.concatenate([h, np.zeros(P * I - h.size)]).reshape(P, I).T.copy()


def rddc64_rotated(x, h, I, D, freqs, start=0, items_per_block=1024):
    """y_k[n] = r_k[n] sum_s g_k[p_n][s] x[j_n - s],  r_k[n] = exp(-2 pi j phi_k(start + j_n) / 2^32): branch by branch,
    windows of the stream times the branch's tap table"""
    x = np.asarray(x, dtype=np.complex128)
    hb = branch_taps(h, I)
    P = hb.shape[1]
    j, p = items(x.size, I, D)
    xp = np.concatenate([np.zeros(P - 1, np.complex128), x])
    win = np.lib.stride_tricks.sliding_window_view(xp, P)  # win[j] = x[j - P + 1 .. j]; tap s takes its item P - 1 - s
    K = len(freqs)
    rot = np.stack([unit(phases(frequency_word(f), 0, P), 1.0) for f in freqs])  # [K, P]: exp(+2 pi j phi_k(s) / 2^32)
    y = np.zeros((K, j.size), dtype=np.complex128)
    for b in range(I):
        idx = np.nonzero(p == b)[0]
        gt = np.ascontiguousarray((hb[b][None, :] * rot)[:, ::-1].T)  # [P, K]
        for lo in range(0, idx.size, items_per_block):
            sel = idx[lo:lo + items_per_block]
            y[:, sel] = (win[j[sel]] @ gt).T
    for k, f in enumerate(freqs):
        i = (j.astype(np.uint64) + np.uint64(start % TWO32)) & np.uint64(TWO32 - 1)
        y[k] *= unit((np.uint64(frequency_word(f)) * i) & np.uint64(TWO32 - 1), -1.0)
    return y


def rddc64_direct(x, h, I, D, freqs, start, which):
    """the definition for the output items `which`, one sum each, the phases with Python integers.  [K, len(which)]"""
    x = np.asarray(x, dtype=np.complex128)
    h = np.asarray(h, dtype=np.float64)
    y = np.zeros((len(freqs), len(which)), dtype=np.complex128)
    for k, f in enumerate(freqs):
        w = frequency_word(f)
        for c, n in enumerate(which):
            m = int(n) * D + D - 1
            j, p = divmod(m, I)
            acc, s = 0.0 + 0.0j, 0
            while p + s * I < h.size and s <= j:
                phi = (w * (start + j - s)) % TWO32
                acc += h[p + s * I] * x[j - s] * complex(math.cos(2.0 * math.pi * phi / 4294967296.0),
                                                         -math.sin(2.0 * math.pi * phi / 4294967296.0))
                s += 1
            y[k, c] = acc
    return y


def branch_abs_sum(h, I):
    """[I]: sum_s |h[p + s I]|"""
    return np.sum(np.abs(branch_taps(h, I)), axis=1)


def window_max(x, ends, P):
    """max |x| over x[e - P + 1 .. e] for every e of `ends` (x = 0 before the start): running maxima over blocks of P,
    so any window of P is two lookups"""
    ends = np.asarray(ends, dtype=np.int64)
    a = np.concatenate([np.zeros(P - 1), np.abs(np.asarray(x).astype(np.complex128))])
    pad = (-a.size) % P
    b = np.concatenate([a, np.zeros(pad)]).reshape(-1, P)
    fwd = np.maximum.accumulate(b, axis=1).reshape(-1)
    bwd = np.maximum.accumulate(b[:, ::-1], axis=1)[:, ::-1].reshape(-1)
    return np.maximum(bwd[ends], fwd[ends + P - 1])  # the window is a[e .. e + P - 1]


def rational_taps64(I, D, L, passband=0.25, stopband=0.75):
    """the design gr4pm_ddc_rational_taps states, in numpy, in double (not rounded to float), for any length L: the
    Kaiser design of gr4pm_ddc_taps for a decimation by D, DC gain I"""
    return dref.kaiser_taps64(D, L, passband, stopband) * I
