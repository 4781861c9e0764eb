"""float64 statement of the MixedFftDdc's definition (csrc/hostlogic/fft_ddc_mixed_plan.hpp holds its integer side), for the
tests: tests/_fft_ddc_ref.py's with a decimation per channel.

N = 2048, K channels; channel k has f_k, D_k (a power of two in 4 .. 64), B_k = N / D_k, a real prototype h_k[0 .. L_k-1]
and R_k images.  Dmax = max D_k; one overlap V (Dmax | V, V <= N - 64, V - (Dmax - D_k) >= L_k - 1 for every k),
hop = N - V.  One segment grid for all channels, anchored on Dmax:
    segment s: the N items from a_s = s hop - V + Dmax - 1 on,   X_s = FFT_N(x_s)
    w_k, c_k, G_k[u], Z[u], Y[v], y'[n']: _fft_ddc_ref's with h_k, B_k, R_k
    first_k = (V - Dmax) / D_k + 1,   n' = first_k .. first_k + hop / D_k - 1,   p = n' D_k,   i = start + a_s + p
    out_k[s hop / D_k + n' - first_k] = exp(-2 pi j phi / 2^32) y'[n'],   phi = (w_k i - c_k 2^21 p) mod 2^32
Frame n of row k has i = start + n D_k + D_k - 1: row k is the Ddc's at D_k (tests/_ddc_ref.py) when R_k = D_k.  The two
bounds are _fft_ddc_ref's derivations with these segments, each channel's own h_k, B_k, R_k and the kept range from
first_k; no constant is refitted."""
import numpy as np

from _ddc_ref import EPS32, TWO32, frequency_word
from _fft_ddc_ref import M32, N, fft32, nearest_bin, response, round32, segment_matrix, slice_index


def default_overlap(Ds, Ls):
    """the smallest multiple of 256 that is >= max_k (Dmax - D_k + L_k - 1)"""
    return (max(max(Ds) - D + L - 1 for D, L in zip(Ds, Ls)) + 255) // 256 * 256


def first_kept(D, Dmax, V):
    return (V - Dmax) // D + 1


def segments(n, Ds, V):
    """complete segments after n samples: s >= 0 with a_s + N <= n"""
    room = n - N + V - max(Ds) + 1
    return 0 if room < 0 else room // (N - V) + 1


def rotators(w, c, D, Dmax, V, S, start):
    """[S, hop / D]: exp(-2 pi j phi / 2^32) of the frames of a channel at D that are kept"""
    hop = N - V
    first = first_kept(D, Dmax, V)
    p = np.arange(first, first + hop // D, dtype=np.uint64) * np.uint64(D)
    a = np.array([(start + s * hop - V + Dmax - 1) % TWO32 for s in range(S)], dtype=np.uint64)
    i = (a[:, None] + p[None, :]) & M32
    ph = (((np.uint64(w) * i) & M32) + (np.uint64(TWO32) - ((np.uint64((c << 21) % TWO32) * p) & M32))[None, :]) & M32
    return np.exp(-2j * np.pi * (ph.astype(np.float64) / 4294967296.0))


def _settings(hs, Ds, Rs, V):
    K = len(Ds)
    Rs = [Rs] * K if np.ndim(Rs) == 0 else list(Rs)
    hs = [np.asarray(h) for h in hs]
    V = default_overlap(Ds, [h.size for h in hs]) if V is None else V
    assert len(hs) == K and len(Rs) == K and V % max(Ds) == 0
    assert all(V - (max(Ds) - D) >= h.size - 1 for D, h in zip(Ds, hs))
    return hs, Rs, V


def _fold(Z, u, R, B):
    """Y[v] = sum of Z[u], u = v mod B, in ascending u"""
    Y = np.zeros((Z.shape[0], B), dtype=Z.dtype)
    for r in range(R):  # image r holds u = -R B / 2 + r B .. + B - 1
        Y[:, u[r * B:(r + 1) * B] % B] += Z[:, r * B:(r + 1) * B]
    return Y


def mixed64(x, hs, Ds, freqs, V=None, Rs=2, start=0, round_table=False):
    """the definition in complex128: a list of K rows, row k with segments hop / D_k frames"""
    hs, Rs, V = _settings(hs, Ds, Rs, V)
    Dmax, hop = max(Ds), N - V
    seg = segment_matrix(x, Dmax, V)
    S = seg.shape[0]
    X = np.fft.fft(seg, axis=1)
    out = []
    for h, D, R, f in zip(hs, Ds, Rs, freqs):
        B, first = N // D, first_kept(D, Dmax, V)
        w = frequency_word(f)
        c = nearest_bin(w)
        u = slice_index(R, B)
        G = response(np.asarray(h, dtype=np.float64), w, u)
        if round_table:
            G = round32(G)
        Y = _fold(X[:, (c + u) % N] * G[None, :], u, R, B)
        y = np.fft.ifft(Y, axis=1)[:, first:first + hop // D] * B
        out.append((y * rotators(w, c, D, Dmax, V, S, start)).reshape(-1))
    return out


def truncation_bound(x, hs, Ds, freqs, V, Rs):
    """a list of K arrays [S]: ||x_s||_2 ||H_k outside the slice||_2 / sqrt(N) per segment: Cauchy-Schwarz on the bins the
    slice of channel k drops (H_k: the unscaled response at all N bins, N G_k)"""
    hs, Rs, V = _settings(hs, Ds, Rs, V)
    seg = segment_matrix(x, max(Ds), V)
    xn = np.sqrt((np.abs(seg) ** 2).sum(axis=1))
    out = []
    for h, D, R, f in zip(hs, Ds, Rs, freqs):
        B = N // D
        outside = np.arange(R * B // 2, N - R * B // 2, dtype=np.int64)  # u mod N of the bins that are not in the slice
        H = N * response(np.asarray(h, dtype=np.float64), frequency_word(f), outside) if outside.size else np.zeros(0)
        out.append(xn * np.sqrt((np.abs(H) ** 2).sum()) / np.sqrt(N))
    return out


def mixed32(x, hs, Ds, freqs, V, Rs, start=0):
    """the definition's steps in its order in float32 (_fft_ddc_ref.fft_ddc32 per channel): a float32 transform, the
    rounded table, one product, the fold in ascending u, a float32 inverse transform, the rotator rounded to float32"""
    hs, Rs, V = _settings(hs, Ds, Rs, V)
    Dmax, hop = max(Ds), N - V
    seg = segment_matrix(x, Dmax, V).astype(np.complex64)
    S = seg.shape[0]
    X = fft32(seg, -1.0)
    out = []
    for h, D, R, f in zip(hs, Ds, Rs, freqs):
        B, first = N // D, first_kept(D, Dmax, V)
        w = frequency_word(f)
        c = nearest_bin(w)
        u = slice_index(R, B)
        G = response(np.asarray(h, dtype=np.float64), w, u).astype(np.complex64)
        Y = _fold((X[:, (c + u) % N] * G[None, :]).astype(np.complex64), u, R, B)
        y = fft32(Y, +1.0)[:, first:first + hop // D]
        out.append((y * rotators(w, c, D, Dmax, V, S, start).astype(np.complex64)).astype(np.complex64).reshape(-1))
    return out


def device_bound(x, hs, Ds, freqs, V, Rs):
    """a list of K arrays [frames_k]: the first-order bound on |float32 result - mixed64(round_table=False)|, u = 2^-24:
    _fft_ddc_ref.device_bound's derivation per channel, sqrt(B_k) ||eY||_2 + 8 u sqrt(B_k) ||Y||_2 +
    6 u |y'[n']| with eY[v] = delta sum |G_k[u]| + (R_k + 3) u sum |Z[u]| over u = v mod B_k and delta = 8 u ||X64_s||_2"""
    hs, Rs, V = _settings(hs, Ds, Rs, V)
    Dmax, hop = max(Ds), N - V
    seg = segment_matrix(x, Dmax, V)
    X = np.fft.fft(seg, axis=1)
    delta = 8.0 * EPS32 * np.sqrt((np.abs(X) ** 2).sum(axis=1))
    out = []
    for h, D, R, f in zip(hs, Ds, Rs, freqs):
        B, first = N // D, first_kept(D, Dmax, V)
        w = frequency_word(f)
        c = nearest_bin(w)
        u = slice_index(R, B)
        G = response(np.asarray(h, dtype=np.float64), w, u)
        Z = X[:, (c + u) % N] * G[None, :]
        Y = _fold(Z, u, R, B)
        sG = _fold(np.abs(G)[None, :], u, R, B)[0]
        sZ = _fold(np.abs(Z), u, R, B)
        eY = delta[:, None] * sG[None, :] + (R + 3) * EPS32 * sZ
        y = np.fft.ifft(Y, axis=1)[:, first:first + hop // D] * B
        per_segment = np.sqrt(B) * np.sqrt((eY ** 2).sum(axis=1)) + 8.0 * EPS32 * np.sqrt(B) * np.sqrt((np.abs(Y) ** 2).sum(axis=1))
        out.append((per_segment[:, None] + 6.0 * EPS32 * np.abs(y)).reshape(-1))
    return out
