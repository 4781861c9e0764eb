"""float64 statement of the FftDdc's definition (csrc/hostlogic/fft_ddc_plan.hpp holds its integer side), for the tests.

N = 2048, K channels, D a power of two in 4 .. 64, B = N / D, a real prototype h[0 .. L-1], an overlap V (D | V,
L - 1 <= V <= N - 64), hop = N - V, R images (a power of two, 1 <= R <= D), x[i] = 0 before the first sample, whose
absolute index is start:
    w_k = llrint(f_k 2^32) mod 2^32,   c_k = floor(w_k N / 2^32 + 1/2) mod N
    segment s: the N items from a_s = s hop - V + D - 1 on,   X_s = FFT_N(x_s)
    G_k[u] = (1 / N) sum_t h[t] exp(-2 pi j ((c_k + u) / N - w_k / 2^32) t),   u in [-R B / 2, R B / 2)
    Z[u] = X_s[(c_k + u) mod N] G_k[u],   Y[v] = sum_{u = v mod B} Z[u]  (ascending u),   y'[n'] = sum_v Y[v] exp(+2 pi j v n' / B)
    n' = V / D .. B - 1,   p = n' D,   i = start + a_s + p,   phi = (w_k i - c_k 2^21 p) mod 2^32
    out_k[s hop / D + n' - V / D] = exp(-2 pi j phi / 2^32) y'[n']
which is the Ddc's y_k[n] (tests/_ddc_ref.py) when R = D, and differs from it by the prototype's response outside the
slice otherwise.  All phases are integers modulo 2^32 before they become an angle."""
import numpy as np

from _ddc_ref import EPS32, TWO32, frequency_word

N = 2048
M32 = np.uint64(TWO32 - 1)


def nearest_bin(w):
    return ((w + (1 << 20)) >> 21) % N


def phi(w, c, i, p):
    """(w i - c 2^21 p) mod 2^32 in wrapping 32-bit arithmetic, as k_fft_ddc_channel forms it (fft_ddc_phi)"""
    return ((w * (i % TWO32)) % TWO32 - ((c << 21) % TWO32) * p) % TWO32


def default_overlap(L):
    return (L - 1 + 255) // 256 * 256


def segments(n, D, V):
    """complete segments after n samples: s >= 0 with a_s + N <= n"""
    room = n - N + V - D + 1
    return 0 if room < 0 else room // (N - V) + 1


def slice_index(R, B):
    """u for the table's items 0 .. R B - 1"""
    return np.arange(R * B, dtype=np.int64) - R * B // 2


def response(h, w, u):
    """G[u] in complex128 for the offsets u from the nearest bin, the phase of every term an exact integer"""
    h = np.asarray(h, dtype=np.float64)
    c = nearest_bin(w)
    psi = ((((c + np.asarray(u, dtype=np.int64)) % N).astype(np.uint64) << np.uint64(21)) + np.uint64(TWO32 - w)) & M32
    t = np.arange(h.size, dtype=np.uint64)
    ph = (psi[:, None] * t[None, :]) & M32  # psi < 2^32 and t < 2^11: no overflow
    return (h[None, :] * np.exp(-2j * np.pi * (ph.astype(np.float64) / 4294967296.0))).sum(axis=1) / N


def round32(z):
    """each component to float32 once, back in complex128"""
    return np.asarray(z).astype(np.complex64).astype(np.complex128)


def segment_matrix(x, D, V):
    """[S, N] complex128: the complete segments of the stream x"""
    x = np.asarray(x, dtype=np.complex128)
    S, hop = segments(x.size, D, V), N - V
    lead = V - D + 1
    xp = np.concatenate([np.zeros(lead, np.complex128), x]) if lead > 0 else x[-lead:]
    if S == 0:
        return np.zeros((0, N), np.complex128)
    return np.lib.stride_tricks.sliding_window_view(xp, N)[::hop][:S]


def rotators(w, c, D, V, S, start):
    """[S, hop / D]: exp(-2 pi j phi / 2^32) of the frames that are kept"""
    hop = N - V
    p = np.arange(V // D, N // D, dtype=np.uint64) * np.uint64(D)
    a = np.array([(start + s * hop - V + D - 1) % TWO32 for s in range(S)], dtype=np.uint64)
    i = (a[:, None] + p[None, :]) & M32
    ph = (((np.uint64(w) * i) & M32) + (np.uint64(TWO32) - ((np.uint64((c << 21) % TWO32) * p) & M32))[None, :]) & M32
    return np.exp(-2j * np.pi * (ph.astype(np.float64) / 4294967296.0))


def fft_ddc64(x, h, D, freqs, V=None, R=2, start=0, round_table=False):
    """the definition in complex128.  [K, segments hop / D].  round_table: G rounded to float32 as the device holds it"""
    h = np.asarray(h, dtype=np.float64)
    V = default_overlap(h.size) if V is None else V
    B, hop = N // D, N - V
    seg = segment_matrix(x, D, V)
    S = seg.shape[0]
    X = np.fft.fft(seg, axis=1)
    u = slice_index(R, B)
    out = np.zeros((len(freqs), S * (hop // D)), dtype=np.complex128)
    for k, f in enumerate(freqs):
        w = frequency_word(f)
        c = nearest_bin(w)
        G = response(h, w, u)
        if round_table:
            G = round32(G)
        Z = X[:, (c + u) % N] * G[None, :]
        Y = np.zeros((S, B), dtype=np.complex128)
        for r in range(R):  # ascending u: image r holds u = -R B / 2 + r B .. + B - 1
            Y[:, u[r * B:(r + 1) * B] % B] += Z[:, r * B:(r + 1) * B]
        y = np.fft.ifft(Y, axis=1)[:, V // D:] * B
        out[k] = (y * rotators(w, c, D, V, S, start)).reshape(-1)
    return out


def truncation_bound(x, h, D, freqs, V, R):
    """[K, S]: ||x_s||_2 ||H_k outside the slice||_2 / sqrt(N) per channel and segment: Cauchy-Schwarz on the bins the slice
    drops (H_k: the unscaled response at all N bins, N G_k)"""
    B = N // D
    seg = segment_matrix(x, D, V)
    xn = np.sqrt((np.abs(seg) ** 2).sum(axis=1))
    outside = np.arange(R * B // 2, N - R * B // 2, dtype=np.int64)  # u mod N of the bins that are not in the slice
    b = np.zeros((len(freqs), seg.shape[0]))
    for k, f in enumerate(freqs):
        H = N * response(h, frequency_word(f), outside) if outside.size else np.zeros(0)
        b[k] = xn * np.sqrt((np.abs(H) ** 2).sum()) / np.sqrt(N)
    return b


# ---- float32 --------------------------------------------------------------------------------------------------------

def fft32(a, sign):
    """radix-2 decimation in time over the last axis in complex64 arithmetic, the twiddles rounded to float32 once;
    sign -1: forward, +1: inverse, unnormalised"""
    a = np.asarray(a, dtype=np.complex64)
    n = a.shape[-1]
    bits = n.bit_length() - 1
    rev = np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)]) if bits else np.zeros(1, dtype=np.int64)
    a = a[..., rev].copy()
    half = 1
    while half < n:
        tw = np.exp(sign * 2j * np.pi * np.arange(half) / (2 * half)).astype(np.complex64)
        a = a.reshape(a.shape[:-1] + (n // (2 * half), 2, half))
        lo, hi = a[..., 0, :], (a[..., 1, :] * tw).astype(np.complex64)
        a = np.stack([lo + hi, lo - hi], axis=-2).astype(np.complex64).reshape(a.shape[:-3] + (n,))
        half *= 2
    return a


def fft_ddc32(x, h, D, freqs, V, R, start=0):
    """the definition's steps in its order in float32: a float32 transform, the rounded table, one product, the fold in
    ascending u, a float32 inverse transform, the rotator rounded to float32"""
    B, hop = N // D, N - V
    seg = segment_matrix(x, D, V).astype(np.complex64)
    S = seg.shape[0]
    X = fft32(seg, -1.0)
    u = slice_index(R, B)
    out = np.zeros((len(freqs), S * (hop // D)), dtype=np.complex64)
    for k, f in enumerate(freqs):
        w = frequency_word(f)
        c = nearest_bin(w)
        G = response(h, w, u).astype(np.complex64)
        Z = (X[:, (c + u) % N] * G[None, :]).astype(np.complex64)
        Y = np.zeros((S, B), dtype=np.complex64)
        for r in range(R):
            Y[:, u[r * B:(r + 1) * B] % B] += Z[:, r * B:(r + 1) * B]
        y = fft32(Y, +1.0)[:, V // D:]
        out[k] = (y * rotators(w, c, D, V, S, start).astype(np.complex64)).astype(np.complex64).reshape(-1)
    return out


def device_bound(x, h, D, freqs, V, R):
    """[K, frames]: the first-order bound on |float32 result - fft_ddc64(round_table=False)|, u = 2^-24.
    delta = 8 u ||X64_s||_2 per forward bin (section 20).  Z = X G: |dZ| <= |G| delta + 4 u |Z| (the table's rounding u |G|,
    the product's four roundings 3 u |X| |G|).  The fold's R - 1 additions: (R - 1) u sum |Z|.  So per folded bin
    eY[v] = delta sum_{u = v} |G[u]| + (R + 3) u sum_{u = v} |Z[u]|.  The inverse transform carries eY to every output
    with unit weights, sqrt(B) ||eY||_2 by Cauchy-Schwarz, and adds its own 8 u ||y'||_2 = 8 u sqrt(B) ||Y||_2 (the forward
    transform's constant).  The rotator: two roundings of the phasor and four of the product, 6 u |y'[n']|."""
    B, hop = N // D, N - V
    seg = segment_matrix(x, D, V)
    S = seg.shape[0]
    X = np.fft.fft(seg, axis=1)
    delta = 8.0 * EPS32 * np.sqrt((np.abs(X) ** 2).sum(axis=1))
    u = slice_index(R, B)
    out = np.zeros((len(freqs), S * (hop // D)))
    for k, f in enumerate(freqs):
        w = frequency_word(f)
        c = nearest_bin(w)
        G = response(h, w, u)
        Z = X[:, (c + u) % N] * G[None, :]
        Y = np.zeros((S, B), dtype=np.complex128)
        sG, sZ = np.zeros(B), np.zeros((S, B))
        for r in range(R):
            v = u[r * B:(r + 1) * B] % B
            Y[:, v] += Z[:, r * B:(r + 1) * B]
            sG[v] += np.abs(G[r * B:(r + 1) * B])
            sZ[:, v] += np.abs(Z[:, r * B:(r + 1) * B])
        eY = delta[:, None] * sG[None, :] + (R + 3) * EPS32 * sZ
        y = np.fft.ifft(Y, axis=1)[:, V // D:] * B
        per_segment = np.sqrt(B) * np.sqrt((eY ** 2).sum(axis=1)) + 8.0 * EPS32 * np.sqrt(B) * np.sqrt((np.abs(Y) ** 2).sum(axis=1))
        out[k] = (per_segment[:, None] + 6.0 * EPS32 * np.abs(y)).reshape(-1)
    return out
