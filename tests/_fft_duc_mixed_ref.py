"""float64 statement of the MixedFftDuc's definition (csrc/hostlogic/fft_duc_mixed_plan.hpp holds its integer side), for the
tests: tests/_fft_duc_ref.py's with an interpolation, a prototype and an image count per row.

N = 2048, K rows; row k has f_k, I_k (a power of two in 4 .. 64), B_k = N / I_k, a real gain a_k, a real prototype h_k and R_k
images; Imax = max I_k; one overlap V (Imax | V, L_k - 1 <= V <= N - 64), hop = N - V.  Row k's item m sits at output sample
m I_k, all rows start at output sample 0 with zeros before it, and the first output sample has the absolute index start:
    z_k[m] = v_k[m] exp(+2 pi j ((w_k (start + m I_k)) mod 2^32) / 2^32)
    segment s: the output samples a_s .. a_s + N - 1, a_s = s hop - V; row k's items m = a_s / I_k + n', n' = 0 .. B_k - 1
    Z_k[v] = sum_n' z_k[a_s / I_k + n'] exp(-2 pi j v n' / B_k)
    S_s[b] = sum_k G_k[u] Z_k[b mod B_k],  b = (c_k + u) mod N,  u in [-R_k B_k / 2, R_k B_k / 2)   (from zero, k ascending)
    x_s[p] = sum_b S_s[b] exp(+2 pi j b p / N),   out[s hop + p - V] = x_s[p] for p = V .. N - 1
with w_k, c_k and G_k as in tests/_fft_duc_ref.py from h_k, a_k, B_k, R_k.  The rows come as a list of K arrays, row k with
slots Imax / I_k items for a whole number of slots (a slot is Imax output samples).  The two bounds are that file's
derivations per row with h_k, B_k, R_k, I_k; nothing is refitted, and n_b counts the rows that reach bin b."""
import numpy as np

from _ddc_ref import EPS32, frequency_word
from _fft_duc_ref import N, _gains, _windows, default_overlap, fft32, response, rotator, round32, table  # noqa: F401
import _fft_duc_ref as fref


def _per_row(x, K):
    return [x] * K if np.ndim(x) == 0 else list(x)


def slots_of(rows, Is):
    """the slots the rows hold: row k has slots Imax / I_k items"""
    Imax = max(Is)
    s = {len(v) * I // Imax for v, I in zip(rows, Is)}
    assert len(s) == 1 and all(len(v) * I % Imax == 0 for v, I in zip(rows, Is)), "the rows do not cover the same whole slots"
    return s.pop()


def items_for(Is, slots):
    Imax = max(Is)
    return [slots * Imax // I for I in Is]


def default_overlap_mixed(hs):
    return max(default_overlap(len(h)) for h in hs)


def _row_windows(virtual, m0, I, V, S, w, start, dtype=np.complex128):
    """[S, B_k]: the rotated items of the segments of one row whose virtual item 0 has the index m0"""
    z = (virtual * rotator(w, I, start, m0, virtual.size).astype(dtype)).astype(dtype)
    return _windows(z[None, :], I, V, S)[0]


def _synthesise(virtuals, m0s, hs, Is, freqs, gains, V, Rs, start, round_table, S):
    """the definition on rows whose item 0 has the index m0s[k] = a / I_k for the first segment's a.  [S hop]"""
    K = len(virtuals)
    a = _gains(gains, K)
    spec = np.zeros((S, N), dtype=np.complex128)
    for k, f in enumerate(freqs):
        Z = np.fft.fft(_row_windows(virtuals[k], m0s[k], Is[k], V, S, frequency_word(f), start)[None], axis=2)[0]
        G, b = table(hs[k], Is[k], Rs[k], f, a[k])
        if round_table:
            G = round32(G)
        spec[:, b] += G[None, :] * Z[:, b % (N // Is[k])]  # a row's bins are all different
    return (np.fft.ifft(spec, axis=1)[:, V:] * N).reshape(-1)


def mixed_fft_duc64(rows, hs, Is, freqs, gains=None, V=None, Rs=2, start=0, round_table=False):
    """the definition in complex128: all complete segments of the rows.  [segments hop]"""
    K = len(rows)
    hs = [np.asarray(h, dtype=np.float64) for h in hs]
    Rs = _per_row(Rs, K)
    V = default_overlap_mixed(hs) if V is None else V
    Imax = max(Is)
    S = slots_of(rows, Is) // ((N - V) // Imax)
    virtuals = [np.concatenate([np.zeros(V // I, np.complex128), np.asarray(v, dtype=np.complex128)]) for v, I in zip(rows, Is)]
    return _synthesise(virtuals, [-(V // I) for I in Is], hs, Is, freqs, gains, V, Rs, start, round_table, S)


class MixedFftDuc64:
    """the same as a stream: process() takes the rows of any whole number of slots and returns the segments they complete"""

    def __init__(self, hs, Is, freqs, gains=None, V=None, Rs=2, start=0):
        self.hs = [np.asarray(h, dtype=np.float64) for h in hs]
        self.Is, self.freqs, self.gains, self.start = list(Is), list(freqs), gains, start
        self.Rs = _per_row(Rs, len(self.Is))
        self.V = default_overlap_mixed(self.hs) if V is None else V
        self.Imax = max(self.Is)
        self.hop_slots = (N - self.V) // self.Imax
        self.reset()

    def reset(self):
        self.carried = [np.zeros(self.V // I, np.complex128) for I in self.Is]
        self.done = 0  # segments delivered
        self.pending = 0  # slots

    def process(self, rows):
        slots = slots_of(rows, self.Is)
        virtuals = [np.concatenate([c, np.asarray(v, dtype=np.complex128)]) for c, v in zip(self.carried, rows)]
        S = (self.pending + slots) // self.hop_slots
        hop = N - self.V
        m0s = [(self.done * hop - self.V) // I for I in self.Is]
        out = _synthesise(virtuals, m0s, self.hs, self.Is, self.freqs, self.gains, self.V, self.Rs, self.start, False, S)
        self.carried = [v[S * (hop // I):] for v, I in zip(virtuals, self.Is)]
        self.done += S
        self.pending = (self.pending + slots) % self.hop_slots
        return out


def truncation_bound(rows, hs, Is, freqs, gains, V, Rs):
    """[S]: the bound on |mixed_fft_duc64(Rs) - mixed_fft_duc64(Is)| for every sample of a segment: the sum over the rows of
    tests/_fft_duc_ref.py's bound of the row alone, with h_k, B_k, R_k, I_k (the dropped terms add up over the rows)"""
    K = len(rows)
    a, Rs = _gains(gains, K), _per_row(Rs, K)
    return sum(fref.truncation_bound(rows[k], hs[k], Is[k], [freqs[k]], [a[k]], V, Rs[k]) for k in range(K))


# ---- float32 --------------------------------------------------------------------------------------------------------

def mixed_fft_duc32(rows, hs, Is, freqs, gains, V, Rs, start=0):
    """the definition's steps in its order in float32, as tests/_fft_duc_ref.py's fft_duc32 has them, per row at B_k points"""
    K = len(rows)
    a, Rs = _gains(gains, K), _per_row(Rs, K)
    S = slots_of(rows, Is) // ((N - V) // max(Is))
    spec = np.zeros((S, N), dtype=np.complex64)
    for k, f in enumerate(freqs):
        I = Is[k]
        virtual = np.concatenate([np.zeros(V // I, np.complex64), np.asarray(rows[k], dtype=np.complex64)])
        Z = fft32(_row_windows(virtual, -(V // I), I, V, S, frequency_word(f), start, np.complex64), -1.0)
        G, b = table(hs[k], I, Rs[k], f, a[k])
        spec[:, b] += (G.astype(np.complex64)[None, :] * Z[:, b % (N // I)]).astype(np.complex64)
    return fft32(spec, +1.0)[:, V:].reshape(-1)


def device_bound(rows, hs, Is, freqs, gains, V, Rs, start=0):
    """[S hop]: the first-order bound on |float32 result - mixed_fft_duc64(round_table=False)|, u = 2^-24: tests/_fft_duc_ref.py's
    device_bound term for term with B_k in the place of B.  The rotator: |dz[m]| <= 6 u |v[m]|; the B_k-point transform carries
    it to every bin, sqrt(B_k) ||dz||_2, and adds 8 u ||Z_k||_2 = 8 u sqrt(B_k) ||z_k||_2; the product adds 4 u |G| |Z|; a bin
    that n_b rows reach, whatever their B_k, takes n_b - 1 additions behind the first term.  Per bin
    eS[b] = sum_k |G_k| dZ_k + (n_b + 3) u sum_k |G_k Z_k|; the N-point transform carries eS to every sample, sum_b eS[b], and
    adds 8 u sqrt(N) ||S_s||_2."""
    K = len(rows)
    a, Rs = _gains(gains, K), _per_row(Rs, K)
    hop = N - V
    S = slots_of(rows, Is) // (hop // max(Is))
    spec = np.zeros((S, N), dtype=np.complex128)
    carried, products, reach = np.zeros((S, N)), np.zeros((S, N)), np.zeros(N)
    for k, f in enumerate(freqs):
        I, B = Is[k], N // Is[k]
        virtual = np.concatenate([np.zeros(V // I, np.complex128), np.asarray(rows[k], dtype=np.complex128)])
        zw = _row_windows(virtual, -(V // I), I, V, S, frequency_word(f), start)
        Z = np.fft.fft(zw, axis=1)
        vn = np.sqrt((np.abs(zw) ** 2).sum(axis=1))  # [S]
        dZ = np.sqrt(B) * 6.0 * EPS32 * vn + 8.0 * EPS32 * np.sqrt(B) * vn
        G, b = table(hs[k], I, Rs[k], f, a[k])
        spec[:, b] += G[None, :] * Z[:, b % B]
        carried[:, b] += np.abs(G)[None, :] * dZ[:, None]
        products[:, b] += np.abs(G)[None, :] * np.abs(Z[:, b % B])
        reach[b] += 1
    eS = carried + (reach[None, :] + 3.0) * EPS32 * products
    per_segment = eS.sum(axis=1) + 8.0 * EPS32 * np.sqrt(N) * np.sqrt((np.abs(spec) ** 2).sum(axis=1))
    return np.repeat(per_segment, hop)
