"""float64 statement of the FftDuc's definition (csrc/hostlogic/fft_duc_plan.hpp holds its integer side), for the tests.

N = 2048, K rows v_k[m] (zero for m < 0), I a power of two in 4 .. 64, B = N / I, a real prototype h[0 .. L-1], real gains
a_k, an overlap V (I | V, L - 1 <= V <= N - 64), hop = N - V, hopI = hop / I, R images (a power of two, 1 <= R <= I);
the first output sample has the absolute index start:
    w_k = llrint(f_k 2^32) mod 2^32,   c_k = floor(w_k N / 2^32 + 1/2) mod N
    z_k[m] = v_k[m] exp(+2 pi j ((w_k (start + m I)) mod 2^32) / 2^32)
    segment s: the output samples a_s .. a_s + N - 1, a_s = s hop - V; the items m = a_s / I + n', n' = 0 .. B - 1
    Z_k[v] = sum_n' z_k[a_s / I + n'] exp(-2 pi j v n' / B)
    G_k[u] = (a_k / N) sum_t h[t] exp(-2 pi j ((c_k + u) / N - w_k / 2^32) t),   u in [-R B / 2, R B / 2)
    S_s[b] = sum_k G_k[u] Z_k[b mod B],  b = (c_k + u) mod N   (from zero, k ascending)
    x_s[p] = sum_b S_s[b] exp(+2 pi j b p / N),   out[s hop + p - V] = x_s[p] for p = V .. N - 1
which is the Duc's x[start + j] (tests/_duc_ref.py) when R = I, and differs from it by the prototype's response outside
the slices otherwise.  All phases are integers modulo 2^32 before they become an angle."""
import numpy as np

from _ddc_ref import EPS32, TWO32, frequency_word, unit
from _fft_ddc_ref import N, default_overlap, fft32, nearest_bin, response, round32, slice_index  # noqa: F401

M32 = np.uint64(TWO32 - 1)


def _rows(v):
    v = np.asarray(v)
    return v[None, :] if v.ndim == 1 else v


def _gains(gains, K):
    return np.ones(K) if gains is None else np.asarray(gains, dtype=np.float64)


def segments(n, I, V):
    """complete segments after n items per row"""
    return n // ((N - V) // I)


def rotator(w, I, start, m0, n):
    """exp(+2 pi j ((w (start + m I)) mod 2^32) / 2^32) for the items m = m0 .. m0 + n - 1 (m0 may be negative)"""
    i = np.array([(start + (m0 + j) * I) % TWO32 for j in range(n)], dtype=np.uint64)
    return unit((np.uint64(w) * i) & M32, 1.0)


def table(h, I, R, f, gain):
    """G_k[u] in complex128 for the table's items 0 .. R B - 1, and their bins (c_k + u) mod N"""
    w = frequency_word(f)
    u = slice_index(R, N // I)
    return gain * response(h, w, u), (nearest_bin(w) + u) % N


def _windows(virtual, I, V, S):
    """[K, S, B]: segment i of the virtual rows (V / I items in front of the new ones) is the items [i hopI, i hopI + B)"""
    B, hop_items = N // I, (N - V) // I
    K = virtual.shape[0]
    if S == 0:
        return np.zeros((K, 0, B), dtype=virtual.dtype)
    return np.lib.stride_tricks.sliding_window_view(virtual, B, axis=1)[:, ::hop_items][:, :S]


def _synthesise(virtual, m0, h, I, freqs, gains, V, R, start, round_table):
    """the definition on rows whose item 0 has the index m0 = a / I for the first segment's a.  [S hop]"""
    K = virtual.shape[0]
    B, hop = N // I, N - V
    S = (virtual.shape[1] - V // I) // (hop // I)
    a = _gains(gains, K)
    z = np.stack([virtual[k] * rotator(frequency_word(f), I, start, m0, virtual.shape[1]) for k, f in enumerate(freqs)])
    Z = np.fft.fft(_windows(z, I, V, S), axis=2)
    spec = np.zeros((S, N), dtype=np.complex128)
    for k, f in enumerate(freqs):
        G, b = table(h, I, R, f, a[k])
        if round_table:
            G = round32(G)
        spec[:, b] += G[None, :] * Z[k][:, b % B]  # a channel's bins are all different
    return (np.fft.ifft(spec, axis=1)[:, V:] * N).reshape(-1)


def fft_duc64(v, h, I, freqs, gains=None, V=None, R=2, start=0, round_table=False):
    """the definition in complex128: all complete segments of the rows v[K, n].  [segments hop].  round_table: G rounded to
    float32 as the device holds it"""
    v = _rows(np.asarray(v, dtype=np.complex128))
    h = np.asarray(h, dtype=np.float64)
    V = default_overlap(h.size) if V is None else V
    virtual = np.concatenate([np.zeros((v.shape[0], V // I), np.complex128), v], axis=1)
    return _synthesise(virtual, -(V // I), h, I, freqs, gains, V, R, start, round_table)


class FftDuc64:
    """the same as a stream: process() takes any number of items per row and returns the whole segments they complete"""

    def __init__(self, h, I, freqs, gains=None, V=None, R=2, start=0):
        self.h = np.asarray(h, dtype=np.float64)
        self.I, self.freqs, self.gains, self.R, self.start = I, list(freqs), gains, R, start
        self.V = default_overlap(self.h.size) if V is None else V
        self.hop_items = (N - self.V) // I
        self.reset()

    def reset(self):
        self.carried = np.zeros((len(self.freqs), self.V // self.I), np.complex128)
        self.done = 0  # segments delivered

    @property
    def pending(self):
        return self.carried.shape[1] - self.V // self.I

    def process(self, v):
        virtual = np.concatenate([self.carried, _rows(np.asarray(v, dtype=np.complex128))], axis=1)
        S = (virtual.shape[1] - self.V // self.I) // self.hop_items
        out = _synthesise(virtual, self.done * self.hop_items - self.V // self.I, self.h, self.I, self.freqs, self.gains,
                          self.V, self.R, self.start, False)
        self.carried = virtual[:, S * self.hop_items:]
        self.done += S
        return out


def segment_norms(v, I, V):
    """[K, S]: ||v_k over segment s||_2"""
    v = _rows(np.asarray(v, dtype=np.complex128))
    virtual = np.concatenate([np.zeros((v.shape[0], V // I), np.complex128), v], axis=1)
    return np.sqrt((np.abs(_windows(virtual, I, V, segments(v.shape[1], I, V))) ** 2).sum(axis=2))


def truncation_bound(v, h, I, freqs, gains, V, R):
    """[S]: the bound on |fft_duc64(R) - fft_duc64(I)| for every sample of a segment.  The dropped terms of sample p are
    sum_k sum_{b outside slice k} G_k[b - c_k] Z_k[b mod B] e^{2 pi j b p / N}; by Cauchy-Schwarz per channel at most
    ||G_k outside||_2 (sum_{b outside} |Z_k[b mod B]|^2)^(1/2).  The N - R B bins outside are consecutive, so they hold
    every residue modulo B exactly I - R times: the second factor is ((I - R) ||Z_k||^2)^(1/2) = ((I - R) B)^(1/2) ||z_k||_2
    (Parseval at B points), and |z| = |v|.  With H_k = N G_k:
        sum_k ||v_k over the segment||_2 ||H_k outside the slice||_2 (1 - R / I)^(1/2) / sqrt(N)"""
    B = N // I
    K = len(freqs)
    a = _gains(gains, K)
    vn = segment_norms(v, I, V)
    outside = np.arange(R * B // 2, N - R * B // 2, dtype=np.int64)  # u mod N of the bins that are not in the slice
    b = np.zeros(vn.shape[1])
    for k, f in enumerate(freqs):
        H = N * a[k] * response(h, frequency_word(f), outside) if outside.size else np.zeros(0)
        b += vn[k] * np.sqrt((np.abs(H) ** 2).sum()) * np.sqrt(1.0 - R / I) / np.sqrt(N)
    return b


# ---- float32 --------------------------------------------------------------------------------------------------------

def fft_duc32(v, h, I, freqs, gains, V, R, start=0):
    """the definition's steps in its order in float32: the rotator rounded to float32 and its product, a float32 transform of
    B points, the rounded table, one product, the sum in ascending k from zero, a float32 transform of N points"""
    v = _rows(np.asarray(v, dtype=np.complex64))
    K = v.shape[0]
    B = N // I
    S = segments(v.shape[1], I, V)
    a = _gains(gains, K)
    virtual = np.concatenate([np.zeros((K, V // I), np.complex64), v], axis=1)
    z = np.stack([(virtual[k] * rotator(frequency_word(f), I, start, -(V // I), virtual.shape[1]).astype(np.complex64))
                  .astype(np.complex64) for k, f in enumerate(freqs)])
    Z = fft32(_windows(z, I, V, S), -1.0)
    spec = np.zeros((S, N), dtype=np.complex64)
    for k, f in enumerate(freqs):
        G, b = table(h, I, R, f, a[k])
        spec[:, b] += (G.astype(np.complex64)[None, :] * Z[k][:, b % B]).astype(np.complex64)
    return fft32(spec, +1.0)[:, V:].reshape(-1)


def device_bound(v, h, I, freqs, gains, V, R, start=0):
    """[S hop]: the first-order bound on |float32 result - fft_duc64(round_table=False)|, u = 2^-24.
    The rotator: two roundings of the phasor and four of the product, |dz[m]| <= 6 u |v[m]|.  The B-point transform
    carries them to every bin with unit weights, sqrt(B) ||dz||_2 by Cauchy-Schwarz, and adds its own 8 u ||Z_k||_2 (section
    20's constant, as section 25 uses it at B points): dZ_k per bin.  The product G Z: |G| dZ_k + 4 u |G| |Z| (the table's
    rounding u |G|, the product's four roundings 3 u |G| |Z|).  A bin that n_b channels reach takes n_b - 1 additions
    behind the first term, (n_b - 1) u sum |G Z|.  So per bin eS[b] = sum_k |G_k| dZ_k + (n_b + 3) u sum_k |G_k Z_k|.
    The N-point transform carries eS to every sample with unit weights, sum_b eS[b], and adds its own
    8 u ||x_s||_2 = 8 u sqrt(N) ||S_s||_2."""
    v = _rows(np.asarray(v, dtype=np.complex128))
    K = v.shape[0]
    B, hop = N // I, N - V
    S = segments(v.shape[1], I, V)
    a = _gains(gains, K)
    virtual = np.concatenate([np.zeros((K, V // I), np.complex128), v], axis=1)
    z = np.stack([virtual[k] * rotator(frequency_word(f), I, start, -(V // I), virtual.shape[1]) for k, f in enumerate(freqs)])
    zw = _windows(z, I, V, S)
    Z = np.fft.fft(zw, axis=2)
    vn = np.sqrt((np.abs(zw) ** 2).sum(axis=2))  # [K, S]
    dZ = np.sqrt(B) * 6.0 * EPS32 * vn + 8.0 * EPS32 * np.sqrt(B) * vn
    spec = np.zeros((S, N), dtype=np.complex128)
    carried, products, reach = np.zeros((S, N)), np.zeros((S, N)), np.zeros(N)
    for k, f in enumerate(freqs):
        G, b = table(h, I, R, f, a[k])
        spec[:, b] += G[None, :] * Z[k][:, b % B]
        carried[:, b] += np.abs(G)[None, :] * dZ[k][:, None]
        products[:, b] += np.abs(G)[None, :] * np.abs(Z[k][:, b % B])
        reach[b] += 1
    eS = carried + (reach[None, :] + 3.0) * EPS32 * products
    per_segment = eS.sum(axis=1) + 8.0 * EPS32 * np.sqrt(N) * np.sqrt((np.abs(spec) ** 2).sum(axis=1))
    return np.repeat(per_segment, hop)
