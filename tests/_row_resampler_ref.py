"""Statements of the RowResampler's definition (include/gr4pm_hip.h), for the tests.

A handle has Q phases (a power of two), P taps per phase and the float32 prototype h[0 .. Q P - 1] at the virtual rate Q
per input item, h[Q P] = 0; its tables are H[q][s] = h[s Q + q] and Dh[q][s] = fl32(h[s Q + q + 1] - h[s Q + q]).  Output
item m of a row of n items x[0 .. n) with the record (step, phase0, freq), positions in Q32.32 Python integers:
    pos = phase0 + m step,  i = pos >> 32,  mu = pos & 0xffffffff,  b = 32 - log2 Q,  q = mu >> b,  alpha = (mu & (2^b - 1)) 2^-b
    c_s = H[q][s] + alpha Dh[q][s],   acc = sum_s c_s x[i - s]   (x = 0 outside [0, n))
    theta = floor(freq pos / 2^32) mod 2^32,   y[m] = exp(-2 pi j theta / 2^32) acc
and the row has the items m with i <= n + P - 2.
resample64() states this in float64 with the exact alpha; resample32() in float32 in the definition's operation order
(alpha rounded to float32, every fmaf one rounding, the rotator from double sincospi rounded to float32, four fmaf from
zero); literal() evaluates y(pos) = sum_i x[i] Ht(pos - i) with the piecewise-linear kernel Ht through h in
fractions.Fraction; error_bound() is the first-order bound of the float32 evaluation that section 24 derives."""
import math
from fractions import Fraction

import numpy as np

EPS32 = 2.0 ** -24
TWO32 = 1 << 32


def tables(h, Q):
    """(H, Dh) as float32 [Q, P]"""
    h = np.asarray(h, dtype=np.float32).reshape(-1)
    assert h.size % Q == 0
    P = h.size // Q
    ext = np.concatenate([h.astype(np.float64), [0.0]])
    H = h.reshape(P, Q).T.copy()
    Dh = (ext[1:] - ext[:-1]).astype(np.float32).reshape(P, Q).T.copy()
    return H, Dh


def output_items(n, P, step, phase0, n_cols=None):
    """M: the m >= 0 with (phase0 + m step) >> 32 <= n + P - 2; 0 for an empty row; cut at n_cols"""
    n, P, step, phase0 = int(n), int(P), int(step), int(phase0)
    end = (n + P - 1) << 32
    M = 0 if n == 0 or phase0 >= end else (end - 1 - phase0) // step + 1
    return M if n_cols is None else min(M, int(n_cols))


def theta(freq, pos):
    """floor(freq pos / 2^32) mod 2^32 for the signed word freq"""
    return ((int(freq) * int(pos)) >> 32) % TWO32  # Python's >> floors


def theta_as_defined(freq, pos):
    """(freq (pos >> 32) + ((freq mu) >> 32)) mod 2^32, the header's expression, with wrapping 32-bit pieces"""
    freq, pos = int(freq), int(pos)
    hi = ((freq % TWO32) * ((pos >> 32) % TWO32)) % TWO32
    lo = ((freq * (pos & (TWO32 - 1))) >> 32) % TWO32
    return (hi + lo) % TWO32


def _items(M, step, phase0, Q):
    pos = [int(phase0) + m * int(step) for m in range(M)]
    b = 32 - (Q.bit_length() - 1)
    i = np.array([p >> 32 for p in pos], dtype=np.int64)
    mu = np.array([p & (TWO32 - 1) for p in pos], dtype=np.int64)
    return pos, i, mu >> b, mu & ((1 << b) - 1), b


def _windows(x, n, P, i, dtype):
    """W[m, s] = x[i[m] - s], zero outside [0, n)"""
    xp = np.concatenate([np.zeros(P - 1, dtype), np.asarray(x[:n]).astype(dtype), np.zeros(P, dtype)])
    return xp[(i[:, None] + (P - 1)) - np.arange(P)[None, :]]


def resample64(x, n, h, Q, step, phase0=0, freq=0, n_cols=None):
    """the row's M items in complex128"""
    H, Dh = tables(h, Q)
    P = H.shape[1]
    M = output_items(n, P, step, phase0, n_cols)
    if M == 0:
        return np.zeros(0, np.complex128)
    pos, i, q, frac, b = _items(M, step, phase0, Q)
    alpha = frac.astype(np.float64) / float(1 << b)
    c = H[q].astype(np.float64) + alpha[:, None] * Dh[q].astype(np.float64)
    acc = np.sum(c * _windows(x, n, P, i, np.complex128), axis=1)
    th = np.array([theta(freq, p) for p in pos], dtype=np.float64)
    return acc * np.exp(-2j * np.pi * (th / 4294967296.0))


def _fma32(a, b, c):
    """fl32(a b + c): the product of two float32 is exact in float64; the sum rounds to float64 and then to float32, which
    differs from one rounding only at a double-rounding tie"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def resample32(x, n, h, Q, step, phase0=0, freq=0, n_cols=None):
    """the row's M items in complex64, in the definition's operation order"""
    H, Dh = tables(h, Q)
    P = H.shape[1]
    M = output_items(n, P, step, phase0, n_cols)
    if M == 0:
        return np.zeros(0, np.complex64)
    pos, i, q, frac, b = _items(M, step, phase0, Q)
    alpha = frac.astype(np.float32) * np.float32(2.0 ** -b)  # int -> float32 rounds to nearest
    W = _windows(np.asarray(x).astype(np.complex64), n, P, i, np.complex64)
    re, im = np.zeros(M, np.float32), np.zeros(M, np.float32)
    for s in range(P):
        c = _fma32(alpha, Dh[q, s], H[q, s])
        re = _fma32(c, W[:, s].real.copy(), re)
        im = _fma32(c, W[:, s].imag.copy(), im)
    th = np.array([theta(freq, p) for p in pos], dtype=np.float64)
    ang = -th / 2147483648.0  # the argument of sincospi, exact
    cs, sn = np.cos(np.pi * ang).astype(np.float32), np.sin(np.pi * ang).astype(np.float32)
    zero = np.zeros(M, np.float32)
    yr = _fma32(-sn, im, _fma32(cs, re, zero))
    yi = _fma32(sn, re, _fma32(cs, im, zero))
    return (yr.astype(np.float64) + 1j * yi.astype(np.float64)).astype(np.complex64)


def literal(x, n, h, Q, pos):
    """y(pos) = sum_i x[i] Ht(pos - i), pos a Fraction in input items, Ht(t) the piecewise-linear function through
    Ht(k / Q) = h[k] (zero for t < 0 and from Q P / Q on), before the rotator; complex, from Fractions"""
    h = [Fraction(float(v)) for v in np.asarray(h, dtype=np.float32)] + [Fraction(0)]
    L = len(h) - 1
    re = im = Fraction(0)
    for i in range(int(n)):
        u = (Fraction(pos) - i) * Q
        if u < 0 or u >= L:
            continue
        k = math.floor(u)
        w = h[k] + (u - k) * (h[k + 1] - h[k])
        re += w * Fraction(float(np.real(x[i])))
        im += w * Fraction(float(np.imag(x[i])))
    return complex(float(re), float(im))


def error_bound(x, n, h, Q, step, phase0=0, n_cols=None):
    """per item, first order in u = 2^-24: with A = sum_s |c_s| and B = sum_s |alpha Dh[q][s]|,
        |y32 - y| <= u max|x| ((P + 1 + 5) A + B)
    P for the accumulation's fmaf, 1 for the fmaf of c_s, B for alpha's rounding, 5 for the rotator (its two rounded
    components and the two roundings of each output component); max|x| over the item's window"""
    H, Dh = tables(h, Q)
    P = H.shape[1]
    M = output_items(n, P, step, phase0, n_cols)
    if M == 0:
        return np.zeros(0)
    _, i, q, frac, b = _items(M, step, phase0, Q)
    alpha = frac.astype(np.float64) / float(1 << b)
    c = H[q].astype(np.float64) + alpha[:, None] * Dh[q].astype(np.float64)
    A = np.sum(np.abs(c), axis=1)
    B = np.sum(np.abs(alpha[:, None] * Dh[q].astype(np.float64)), axis=1)
    xmax = np.max(np.abs(_windows(x, n, P, i, np.complex128)), axis=1)
    return EPS32 * xmax * ((P + 6) * A + B)


def kaiser_taps64(Q, P, max_step=1.0, passband=0.25, stopband=0.75):
    """the design gr4pm_row_resampler_taps states, in double: P' = ceil(P max(1, max_step)) taps per phase, the edges
    divided by max(1, max_step), DC gain Q"""
    import _ddc_ref as dref
    widen = max(1.0, float(max_step))
    span = int(math.ceil(P * widen))
    return dref.kaiser_taps64(Q, Q * span, passband / widen, stopband / widen) * Q
