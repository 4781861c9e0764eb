"""float64 statements of the Duc's definition (include/gr4pm_hip.h), for the tests.

K rows v_k[m] at fs / I (zero before the first item), interpolation I, real prototype h[0 .. L-1], real gains a_k; output
sample j = m I + r (0 <= r < I) has the absolute index i = start + j:
    w_k = llrint(f_k 2^32) mod 2^32,   phi_k(i) = (w_k i) mod 2^32   (integers, as in tests/_ddc_ref.py)
    x[i] = sum_k a_k exp(+2 pi j phi_k(i) / 2^32) sum_{p : p I + r < L} h[p I + r] v_k[m - p]
duc64() computes exactly these lines (zero-stuff, np.convolve, mix, sum); duc64_rotated() is the form the kernel
implements (rotated taps g_k[t] = a_k h[t] exp(+2 pi j phi_k(t) / 2^32), one rotator per input item) and is pinned to
the former by tests/test_duc_ref.py; duc64_direct() evaluates single samples with Python integers for the phases.
window_scale() is the magnitude the GPU tests measure errors against."""
import math

import numpy as np

from _ddc_ref import EPS32, TWO32, frequency_word, kaiser_taps64, phases, unit  # noqa: F401


def _rows(v):
    v = np.asarray(v, dtype=np.complex128)
    return v[None, :] if v.ndim == 1 else v


def _gains(gains, K):
    return np.ones(K) if gains is None else np.asarray(gains, dtype=np.float64)


def duc64(v, h, I, freqs, gains=None, start=0):
    """the definition, literally, in complex128.  [n I]"""
    v = _rows(v)
    h = np.asarray(h, dtype=np.float64)
    K, n = v.shape
    a = _gains(gains, K)
    x = np.zeros(n * I, dtype=np.complex128)
    for k, f in enumerate(freqs):
        up = np.zeros(n * I, dtype=np.complex128)
        up[::I] = v[k]
        x += a[k] * np.convolve(h, up)[:n * I] * unit(phases(frequency_word(f), start, n * I), 1.0)
    return x


def rotated_taps(h, I, freqs, gains=None):
    """[K, P, I]: g_k[p I + r] = a_k h[p I + r] exp(+2 pi j phi_k(p I + r) / 2^32), zero from L on"""
    h = np.asarray(h, dtype=np.float64)
    P = -(-h.size // I)
    a = _gains(gains, len(freqs))
    g = np.zeros((len(freqs), P * I), dtype=np.complex128)
    for k, f in enumerate(freqs):
        g[k, :h.size] = a[k] * h * unit(phases(frequency_word(f), 0, h.size), 1.0)
    return g.reshape(len(freqs), P, I)


def duc64_rotated(v, h, I, freqs, gains=None, start=0, frames_per_block=4096):
    """x[m I + r] = sum_k sum_p g_k[p I + r] z_k[m - p],  z_k[m'] = v_k[m'] exp(+2 pi j phi_k(start + m' I) / 2^32):
    windows of the rotated rows times the tap table, block by block of frames.  [n I]"""
    v = _rows(v)
    K, n = v.shape
    g = rotated_taps(h, I, freqs, gains)
    P = g.shape[1]
    x = np.zeros((n, I), dtype=np.complex128)
    for k, f in enumerate(freqs):
        w = frequency_word(f)
        i = (np.arange(n, dtype=np.uint64) * np.uint64(I) + np.uint64(start % TWO32)) & np.uint64(TWO32 - 1)
        z = v[k] * unit((np.uint64(w) * i) & np.uint64(TWO32 - 1), 1.0)
        zp = np.concatenate([np.zeros(P - 1, np.complex128), z])
        # window m: zp[m .. m + P - 1] = z[m - P + 1 .. m]; phase p takes its item P - 1 - p
        win = np.lib.stride_tricks.sliding_window_view(zp, P)
        gm = np.ascontiguousarray(g[k, ::-1, :])
        for lo in range(0, n, frames_per_block):
            x[lo:lo + frames_per_block] += win[lo:lo + frames_per_block] @ gm
    return x.reshape(-1)


def duc64_direct(v, h, I, freqs, gains, start, samples):
    """the definition for the output samples `samples` (indices j into the call's output), one sum each, the phases
    with Python integers.  [len(samples)]"""
    v = _rows(v)
    h = np.asarray(h, dtype=np.float64)
    a = _gains(gains, v.shape[0])
    out = np.zeros(len(samples), dtype=np.complex128)
    for c, j in enumerate(samples):
        m, r = divmod(int(j), I)
        acc = 0.0 + 0.0j
        for k, f in enumerate(freqs):
            phi = (frequency_word(f) * (start + int(j))) % TWO32
            s = 0.0 + 0.0j
            for p in range(m + 1):
                if p * I + r >= h.size:
                    break
                s += h[p * I + r] * v[k, m - p]
            ang = 2.0 * math.pi * phi / 4294967296.0
            acc += a[k] * complex(math.cos(ang), math.sin(ang)) * s
        out[c] = acc
    return out


def window_scale(v, h, I, gains=None):
    """S[j] = sum_k |a_k| (sum_{p : p I + r < L} |h[p I + r]|) max_{those p} |v_k[m - p]|,  j = m I + r.  [n I]"""
    v = _rows(v)
    h = np.abs(np.asarray(h, dtype=np.float64))
    K, n = v.shape
    a = np.abs(_gains(gains, K))
    P = -(-h.size // I)
    hs = np.concatenate([h, np.zeros(P * I - h.size)]).reshape(P, I).sum(axis=0)  # per phase r
    full = np.arange(I) + (P - 1) * I < h.size                                     # phases with P taps, else P - 1
    S = np.zeros((n, I))
    for k in range(K):
        av = np.concatenate([np.zeros(P - 1), np.abs(v[k])])
        wP = np.lib.stride_tricks.sliding_window_view(av, P).max(axis=1)            # max |v[m - P + 1 .. m]|
        wQ = np.lib.stride_tricks.sliding_window_view(av[1:], P - 1).max(axis=1) if P > 1 else np.zeros(n)
        S += a[k] * hs[None, :] * np.where(full[None, :], wP[:, None], wQ[:, None])
    return S.reshape(-1)
