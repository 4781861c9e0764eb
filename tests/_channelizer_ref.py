"""float64 statements of the Channelizer's definition (include/gr4pm_hip.h), for the tests.

M channels, real prototype h[0 .. L-1], L = P M, x[i] = 0 for i < 0:
    z_k[i] = x[i] exp(-2 pi j k i / M),   w_k = h * z_k,   y_k[n] = w_k[n M + M - 1]
analysis64() computes exactly these lines; analysis64_polyphase() is the form the kernel implements (branch sums, one
forward M-point DFT per frame) and is pinned to the former by tests/test_channelizer_ref.py."""
import numpy as np

import _ddc_ref

EPS32 = 2.0 ** -24


def analysis64(x, h, M):
    """the definition, literally, in complex128: mix, np.convolve, keep every M-th sample from M - 1 on.  [M, len(x) // M]"""
    x = np.asarray(x, dtype=np.complex128)
    h = np.asarray(h, dtype=np.float64)
    F = x.size // M
    i = np.arange(x.size)
    y = np.zeros((M, F), dtype=np.complex128)
    for k in range(M):
        z = x * np.exp(-2j * np.pi * ((k * i) % M) / M)
        w = np.convolve(h, z)
        y[k] = w[M - 1::M][:F]
    return y


def analysis64_polyphase(x, h, M):
    """u_n[m] = sum_p h[p M + M - 1 - m] x[(n - p) M + m];  y_k[n] = sum_m u_n[m] exp(-2 pi j k m / M)"""
    x = np.asarray(x, dtype=np.complex128)
    h = np.asarray(h, dtype=np.float64)
    P = h.size // M
    assert P * M == h.size
    F = x.size // M
    xp = np.concatenate([np.zeros((P - 1) * M, np.complex128), x[:F * M]]).reshape(F + P - 1, M)
    hr = h.reshape(P, M)[:, ::-1]
    u = np.zeros((F, M), dtype=np.complex128)
    for p in range(P):
        u += hr[p][None, :] * xp[P - 1 - p:P - 1 - p + F]
    return np.ascontiguousarray(np.fft.fft(u, axis=1).T)


def kaiser_taps64(M, P=12, passband=0.25, stopband=0.75):
    """the design gr4pm_channelizer_taps states, in numpy, in double (not rounded to float)"""
    return _ddc_ref.kaiser_taps64(M, P * M, passband, stopband)


def response_db(h, M, oversample=64):
    """(f in units of the channel spacing, 20 log10 |H(f)|) on an oversample * L point grid, 0 <= f <= M / 2"""
    n = oversample * len(h)
    H = np.fft.fft(np.asarray(h, dtype=np.float64), n)[: n // 2 + 1]
    f = np.arange(n // 2 + 1) * (M / n)
    return f, 20.0 * np.log10(np.maximum(np.abs(H), 1e-300))


def window_max(x, M, P):
    """per output item n: max |x| over the L = P M samples it is made of (frames n - P + 1 .. n)"""
    F = len(x) // M
    fm = np.abs(np.asarray(x)[:F * M].astype(np.complex128)).reshape(F, M).max(axis=1)
    fm = np.concatenate([np.zeros(P - 1), fm])
    out = np.zeros(F)
    for p in range(P):
        out = np.maximum(out, fm[p:p + F])
    return out


def synthesis64(rows, h, M, n_items):
    """the matching synthesis bank in complex128: every channel's baseband items zero-stuffed by M, filtered with M h,
    mixed to +k fs / M, summed.  rows: {k: items}; returns n_items * M wideband samples.  Through analysis64 with the
    same h, channel k's item j comes out as item j + P - 1 of row k."""
    h = np.asarray(h, dtype=np.float64)
    N = n_items * M
    i = np.arange(N)
    x = np.zeros(N, dtype=np.complex128)
    for k, items in rows.items():
        up = np.zeros(N, dtype=np.complex128)
        v = np.asarray(items, dtype=np.complex128)[:n_items]
        up[:v.size * M:M] = v
        x += np.convolve(up, M * h)[:N] * np.exp(2j * np.pi * ((k * i) % M) / M)
    return x
