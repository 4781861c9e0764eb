"""The FftFilter block's definition in complex128 (include/gr4pm_hip.h), its restatement in float32
and the bound between them.  NumPy only.

N = 2048, complex taps h[0 .. L - 1], an overlap V with L - 1 <= V <= N - 64, hop = N - V, x[i] = 0 for i < 0.  Segment s is
the N items from s hop - V; X_s = FFT_N(x_s); G[k] = (1 / N) sum_t h[t] exp(-2 pi j k t / N); y_s = N IFFT_N(X_s G);
out[s hop + p - V] = y_s[p] for p = V .. N - 1.  So out[n] = sum_t h[t] x[n - t]."""
import numpy as np

from _fft_ddc_ref import fft32

N = 2048
EPS32 = 2.0 ** -24

# the device cases (L, V) of tests/test_fft_filter.py
CASES = [(1, 0), (2, 1), (64, 63), (200, 256), (1025, 1024), (1985, 1984)]


def default_overlap(L):
    return min(-(-(L - 1) // 256) * 256, N - 64)


def segments(n, V):
    return n // (N - V)


def segment_matrix(x, V):
    """[S, N] complex128: the complete segments of the stream x"""
    x = np.asarray(x, dtype=np.complex128)
    S, hop = segments(x.size, V), N - V
    if S == 0:
        return np.zeros((0, N), np.complex128)
    xp = np.concatenate([np.zeros(V, np.complex128), x])
    return np.lib.stride_tricks.sliding_window_view(xp, N)[::hop][:S]


def response(h):
    """G[0 .. N) in complex128"""
    h = np.asarray(h, dtype=np.complex128)
    return np.fft.fft(h, N) / N


def round32(z):
    return np.asarray(z).astype(np.complex64).astype(np.complex128)


def fft_filter64(x, h, V=None, round_table=False):
    """the definition in complex128: the samples of the complete segments, [segments hop]"""
    V = default_overlap(len(h)) if V is None else V
    G = response(h)
    if round_table:
        G = round32(G)
    X = np.fft.fft(segment_matrix(x, V), axis=1)
    y = np.fft.ifft(X * G[None, :], axis=1) * N
    return y[:, V:].reshape(-1)


def flushed(x, V):
    """x with the zeros that complete its last segment"""
    hop = N - V
    return np.concatenate([np.asarray(x), np.zeros(-len(x) % hop, dtype=np.asarray(x).dtype)])


def fft_filter32(x, h, V):
    """the definition's steps in float32: fft32 forward, the rounded table, one product, fft32 inverse"""
    seg = segment_matrix(x, V).astype(np.complex64)
    G = response(h).astype(np.complex64)
    Z = (fft32(seg, -1.0) * G[None, :]).astype(np.complex64)
    return fft32(Z, +1.0)[:, V:].reshape(-1)


def device_bound(x, h, V):
    """[segments hop]: the first-order bound on |float32 result - fft_filter64|, u = 2^-24: DESIGN.md section 25's derivation
    with R = 1, B = N and no rotator.  delta_s = 8 u ||X_s||_2 per forward bin; Z = X G: eY[k] = delta_s |G[k]| + 4 u |Z[k]|
    (the table's rounding and the product's four); the second transform carries eY to every output with unit weights,
    sqrt(N) ||eY||_2, and adds its own 8 u sqrt(N) ||Z||_2."""
    hop = N - V
    G = response(h)
    X = np.fft.fft(segment_matrix(x, V), axis=1)
    Z = X * G[None, :]
    delta = 8.0 * EPS32 * np.sqrt((np.abs(X) ** 2).sum(axis=1))
    eY = delta[:, None] * np.abs(G)[None, :] + 4.0 * EPS32 * np.abs(Z)
    b = np.sqrt(N) * np.sqrt((eY ** 2).sum(axis=1)) + 8.0 * EPS32 * np.sqrt(N) * np.sqrt((np.abs(Z) ** 2).sum(axis=1))
    return np.repeat(b, hop)


def stimulus(n, seed):
    """seeded complex normal samples with a stretch of 300 samples 30 times larger"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
    lo = n // 3
    x[lo:lo + 300] *= 30.0
    return x.astype(np.complex64)


def random_taps(L, seed):
    """random complex taps of unit energy"""
    rng = np.random.default_rng(seed)
    h = rng.standard_normal(L) + 1j * rng.standard_normal(L)
    return (h / np.sqrt((np.abs(h) ** 2).sum())).astype(np.complex64)


def segment_rms(e, hop):
    """[segments]: the RMS of e over each segment's hop samples"""
    return np.sqrt((np.abs(e.reshape(-1, hop)) ** 2).mean(axis=1))
