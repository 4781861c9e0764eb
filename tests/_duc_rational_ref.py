"""float64 statements of the rational Duc's definition (include/gr4pm_hip.h), for the tests.

K rows v_k[m] (zero before the first item), resampling by I / D, real prototype h[0 .. L-1] at I times the rows' rate
(P = ceil(L / I), h[t] = 0 for t >= L), real gains a_k.  Output sample j, counted from the handle's start:
    i = start + j,   u_j = j D,   m_j = u_j div I,   r_j = u_j mod I
    x[i] = sum_k a_k exp(+2 pi j phi_k(i) / 2^32) sum_{p : p I + r_j < L} h[p I + r_j] v_k[m_j - p]
N items per row make ceil(N I / D) samples.  rduc64() computes these lines literally (zero-stuff by I, np.convolve with
h, keep every D-th, mix, sum); rduc64_form() is the form the kernel implements (filter with the real taps a_k h branch
by branch, then the rotator q_k(i) = A_k[i div B] T_k[i mod B] aligned to the absolute index, B = 1024) and is pinned
to the former by tests/test_duc_rational_ref.py; rduc64_direct() evaluates single samples with Python integers for the
phases.  Frequency words and phases are _ddc_ref's: integers modulo 2^32 before they become an angle.  window_scale()
is the magnitude the GPU tests measure errors against."""
import math

import numpy as np

from _ddc_ref import EPS32, TWO32, frequency_word, kaiser_taps64, phases, unit  # noqa: F401  (what the tests take from here)

B = 1024  # the rotator's aligned block: one constant here and in csrc/duc.hip (kRotBlock)


def _rows(v):
    v = np.asarray(v, dtype=np.complex128)
    return v[None, :] if v.ndim == 1 else v


def _gains(gains, K):
    return np.ones(K) if gains is None else np.asarray(gains, dtype=np.float64)


def sample_count(N, I, D):
    return -(-N * I // D)


def samples(N, I, D):
    """(m, r) of the ceil(N I / D) samples N items make: the newest item counted from the start, and the branch"""
    u = np.arange(sample_count(N, I, D), dtype=np.int64) * D
    return u // I, u % I


def rduc64(v, h, I, D, freqs, gains=None, start=0):
    """the definition, literally, in complex128.  [ceil(n I / D)]"""
    v = _rows(v)
    h = np.asarray(h, dtype=np.float64)
    K, n = v.shape
    a = _gains(gains, K)
    F = sample_count(n, I, D)
    x = np.zeros(F, dtype=np.complex128)
    for k, f in enumerate(freqs if F else []):
        up = np.zeros(n * I, dtype=np.complex128)
        up[::I] = v[k]
        x += a[k] * np.convolve(h, up)[:n * I][::D] * unit(phases(frequency_word(f), start, F), 1.0)
    return x


def branch_taps(h, I):
    """[I, P]: row r is h[r::I], zeros after its end"""
    h = np.asarray(h, dtype=np.float64)
    P = -(-h.size // I)
    return np.concatenate([h, np.zeros(P * I - h.size)]).reshape(P, I).T.copy()


def filtered(v, h, I, D, samples_per_block=4096):
    """b[j] = sum_p h[p I + r_j] v[m_j - p] for one row: branch by branch, windows of the row times the branch's taps"""
    v = np.asarray(v, dtype=np.complex128)
    hb = branch_taps(h, I)
    P = hb.shape[1]
    m, r = samples(v.size, I, D)
    vp = np.concatenate([np.zeros(P - 1, np.complex128), v])
    win = np.lib.stride_tricks.sliding_window_view(vp, P)  # win[m] = v[m - P + 1 .. m]; tap p takes its item P - 1 - p
    b = np.zeros(m.size, dtype=np.complex128)
    for br in range(I):
        idx = np.nonzero(r == br)[0]
        g = np.ascontiguousarray(hb[br][::-1])
        for lo in range(0, idx.size, samples_per_block):
            sel = idx[lo:lo + samples_per_block]
            b[sel] = win[m[sel]] @ g
    return b


def rotator(w, start, F):
    """q(i) = A[i div B] T[i mod B] for i = start .. start + F - 1: A from the exact integer phase of the aligned
    block's first sample, T[t] = exp(+2 pi j phi(t) / 2^32)"""
    i = np.arange(F, dtype=np.uint64) + np.uint64(start % TWO32)  # below 2^33: the low 32 bits are all the phase needs
    base = (i & np.uint64(TWO32 - 1)) & ~np.uint64(B - 1)
    A = unit((np.uint64(w) * base) & np.uint64(TWO32 - 1), 1.0)
    T = unit(phases(w, 0, B), 1.0)
    return A * T[(i & np.uint64(B - 1)).astype(np.int64)]


def rduc64_form(v, h, I, D, freqs, gains=None, start=0, samples_per_block=4096):
    """x[i] = sum_k q_k(i) b_k[j] with b_k made from the real taps a_k h: the evaluation's form.  [ceil(n I / D)]"""
    v = _rows(v)
    h = np.asarray(h, dtype=np.float64)
    K, n = v.shape
    a = _gains(gains, K)
    F = sample_count(n, I, D)
    x = np.zeros(F, dtype=np.complex128)
    for k, f in enumerate(freqs if F else []):
        x += rotator(frequency_word(f), start, F) * filtered(v[k], a[k] * h, I, D, samples_per_block)
    return x


def rduc64_direct(v, h, I, D, freqs, gains, start, which):
    """the definition for the output samples `which` (indices j counted from the start), one sum each, the phases with
    Python integers.  [len(which)]"""
    v = _rows(v)
    h = np.asarray(h, dtype=np.float64)
    a = _gains(gains, v.shape[0])
    out = np.zeros(len(which), dtype=np.complex128)
    for c, j in enumerate(which):
        m, r = divmod(int(j) * D, I)
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


def window_max(v, ends, P):
    """max |v| over v[e - P + 1 .. e] for every e of `ends` (v = 0 before the start): running maxima over blocks of P,
    so any window of P is two lookups"""
    ends = np.asarray(ends, dtype=np.int64)
    a = np.concatenate([np.zeros(P - 1), np.abs(np.asarray(v).astype(np.complex128))])
    pad = (-a.size) % P
    b = np.concatenate([a, np.zeros(pad)]).reshape(-1, P)
    fwd = np.maximum.accumulate(b, axis=1).reshape(-1)
    bwd = np.maximum.accumulate(b[:, ::-1], axis=1)[:, ::-1].reshape(-1)
    return np.maximum(bwd[ends], fwd[ends + P - 1])  # the window is a[e .. e + P - 1]


def window_scale(v, h, I, D, gains=None):
    """S[j] = sum_k |a_k| (sum_{p : p I + r_j < L} |h[p I + r_j]|) max_{those p} |v_k[m_j - p]|.  [ceil(n I / D)]"""
    v = _rows(v)
    ha = np.abs(np.asarray(h, dtype=np.float64))
    K, n = v.shape
    a = np.abs(_gains(gains, K))
    P = -(-ha.size // I)
    m, r = samples(n, I, D)
    hs = branch_taps(ha, I).sum(axis=1)                      # per branch
    full = np.arange(I) + (P - 1) * I < ha.size              # branches with P taps, else P - 1
    S = np.zeros(m.size)
    for k in range(K):
        wP = window_max(v[k], m, P)
        wQ = window_max(v[k], m, P - 1) if P > 1 else np.zeros(m.size)
        S += a[k] * hs[r] * np.where(full[r], wP, wQ)
    return S


def rational_taps64(I, D, L, passband=0.25, stopband=0.75):
    """the design gr4pm_duc_rational_taps states, in numpy, in double (not rounded to float), for any length L: the
    Kaiser design of gr4pm_duc_taps for an interpolation by I, DC gain I (D enters through the refusal only)"""
    return kaiser_taps64(I, L, passband, stopband) * I
