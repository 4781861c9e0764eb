"""Float64 numpy restatement of the LineSpectrum block's definition, of the line finder and of the simplest ratio, written
from their specification (include/gr4pm_hip.h), not from the library.

    row of n_r items, u = gain x (gain and x are float32 values, the product is exact in float64)
    y[i] = |u|^2 (envelope), u^2 (square), (u^2)^2 (fourth) for i < n_r, 0 beyond; items at or beyond n_r are not looked at
    S = 0 if n_r = 0 else 1 + ceil(max(n_r - N, 0) / hop); segment s = y[s hop .. s hop + N), zero-filled
    square, fourth: acc[k] = sum_s |FFT(w y_s)[k]|^2
    envelope: Z_p = FFT(w (y_2p + i y_2p+1)), acc[k] = sum_p (|Z_p[k]|^2 + |Z_p[(N - k) mod N]|^2) / 2
    out = acc / (S sum w^2), zeros when S = 0

The error bound.  eps = 2^-24.  The transform's input y32 differs from y64 by at most c eps |y|
per item, first order, from the operation count (every float32 operation: relative error eps; FMA contraction only removes
roundings):
    u = g x: eps per component, so |du| <= eps |u|
    envelope  |u|^2 from u: 2 eps |u|^2; its own two products and one sum: eps ux^2 + eps uy^2 + eps y <= 2 eps y;
              the window product: eps.  c = 5
    square    u^2 from u: 2 |u| |du| = 2 eps |u|^2; its own: re = ux^2 - uy^2: eps ux^2 + eps uy^2 + eps |re| <= 2 eps |v|,
              im = 2 ux uy: eps |v|, together sqrt(5) eps |v| <= 3 eps |v|; the window product: eps.  c = 6
    fourth    v = u^2 carries 5 eps |v| from the line above; v^2 from v: 2 |v| |dv| = 10 eps |v|^2; its own: 3 eps; the
              window product: eps.  c = 14
An input error e_i moves a bin by at most sum_i w_i |e_i|, so with T the float64 transform (Y_s, or Z_p of a pair, where
|e_i| <= c eps (|y_a| + |y_b|))
    delta = 8 eps ||T||_2 + c eps sum_i w_i |y_i|
    |acc32 - acc64| <= sum (2 |T[k]| delta + delta^2) + 64 eps acc64[k]
and for the envelope the same per pair, folded as acc is: (b[k] + b[(N - k) mod N]) / 2.
"""
import math

import numpy as np

N = 2048
RUN = 64
STATISTICS = ("envelope", "square", "fourth")
C_INPUT = {"envelope": 5.0, "square": 6.0, "fourth": 14.0}
EPS = 2.0 ** -24


def hann(n=N):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)).astype(np.float32)


def segments(n, hop):
    return 0 if n == 0 else 1 + (-(-(n - N) // hop) if n > N else 0)


def nonlinearity(x, statistic, gain=1.0):
    u = np.asarray(x).astype(np.complex128) * float(np.float32(gain))
    if statistic == "envelope":
        return u.real ** 2 + u.imag ** 2
    if statistic == "square":
        return u * u
    if statistic == "fourth":
        return (u * u) * (u * u)
    raise ValueError(statistic)


def segment_matrix(row, n_r, hop, statistic, gain=1.0):
    """y_s for every segment, [S, N], zero-filled; only row[:n_r] is looked at"""
    y = nonlinearity(np.asarray(row)[:n_r], statistic, gain)
    S = segments(n_r, hop)
    out = np.zeros((S, N), dtype=y.dtype)
    for s in range(S):
        part = y[s * hop: s * hop + N]
        out[s, :part.size] = part
    return out


def transforms(row, n_r, hop, window, statistic, gain=1.0):
    """(T[t, k], L1[t]): the float64 transforms the definition sums (Y_s, or Z_p of the envelope's pairs) and
    sum_i w_i |y_i| of each one's input (for a pair: of both segments)"""
    w = np.asarray(window, dtype=np.float32).astype(np.float64)
    ys = segment_matrix(row, n_r, hop, statistic, gain)
    if statistic == "envelope":
        if ys.shape[0] % 2:
            ys = np.concatenate([ys, np.zeros((1, N))])
        l1 = (w * (np.abs(ys[0::2]) + np.abs(ys[1::2]))).sum(axis=1)
        ys = ys[0::2] + 1j * ys[1::2]
    else:
        l1 = (w * np.abs(ys)).sum(axis=1)
    T = np.fft.fft(w * ys, axis=1) if ys.shape[0] else np.zeros((0, N), dtype=np.complex128)
    return T, l1


def fold(a):
    """(a[k] + a[(N - k) mod N]) / 2"""
    return 0.5 * (a + a[(N - np.arange(N)) % N])


def row_spectrum(row, n_r, hop, window, statistic, gain=1.0):
    """dict(out, acc, bound, segments): the definition in float64, and the float32 bound of acc"""
    S = segments(n_r, hop)
    wp = float(np.sum(np.asarray(window, dtype=np.float32).astype(np.float64) ** 2))
    if S == 0:
        return dict(out=np.zeros(N), acc=np.zeros(N), bound=np.zeros(N), segments=0, window_power=wp)
    T, l1 = transforms(row, n_r, hop, window, statistic, gain)
    P = T.real ** 2 + T.imag ** 2
    delta = (8.0 * EPS * np.sqrt(P.sum(axis=1)) + C_INPUT[statistic] * EPS * l1)[:, None]
    acc = P.sum(axis=0)
    bound = (2.0 * np.abs(T) * delta + delta ** 2).sum(axis=0) + RUN * EPS * acc
    if statistic == "envelope":
        acc, bound = fold(acc), fold(bound)
    return dict(out=acc / (S * wp), acc=acc, bound=bound, segments=S, window_power=wp)


def worst_ratio(err, bound):
    """max err / bound over the bins with a bound above 0 (0 when there is none: err must be 0 there anyway)"""
    live = bound > 0
    return float(np.max(err[live] / bound[live])) if live.any() else 0.0


def envelope_direct(row, n_r, hop, window, gain=1.0):
    """sum_s |Y_s[k]|^2 by one real transform per segment: what the pairs must equal"""
    w = np.asarray(window, dtype=np.float32).astype(np.float64)
    ys = segment_matrix(row, n_r, hop, "envelope", gain)
    Y = np.fft.fft(w * ys, axis=1)
    return (Y.real ** 2 + Y.imag ** 2).sum(axis=0)


def find_line(sp, first_bin=0, n_bins=None, guard_bins=2):
    sp = np.asarray(sp, dtype=np.float64)
    n = sp.size
    n_bins = n if n_bins is None else n_bins
    assert 0 <= first_bin < n and 2 * guard_bins + 3 <= n_bins <= n
    idx = [(first_bin + i) % n for i in range(n_bins)]
    win = sp[idx]
    ip = 0
    for i in range(n_bins):
        if win[i] > win[ip]:
            ip = i
    b, peak = idx[ip], float(win[ip])
    floor = float(np.sort(win)[(n_bins - 1) // 2])
    far = [float(sp[k]) for k in idx if min(abs(k - b), n - abs(k - b)) > guard_bins]
    other = max(far)
    found = peak > 0.0
    d = snr = margin = 0.0
    if found:
        with np.errstate(divide="ignore"):
            snr = 10.0 * np.log10(np.float64(peak) / floor)
            margin = 10.0 * np.log10(np.float64(peak) / other)
        a, c = float(sp[(b - 1) % n]), float(sp[(b + 1) % n])
        if a > 0.0 and c > 0.0:
            la, lb, lc = math.log(a), math.log(peak), math.log(c)
            curv = la - 2.0 * lb + lc
            if curv < 0.0:
                d = min(0.5, max(-0.5, 0.5 * (la - lc) / curv))
    f = (b + d) / n
    f -= math.floor(f + 0.5)
    return dict(frequency=f, snr_db=float(snr), margin_db=float(margin), peak=peak, floor=floor, bin=b, found=int(found))


def simplest_ratio(value, rel_tol, max_num, max_den):
    """(num, den) or None: by trying every denominator in ascending order, its smallest admissible numerator first"""
    lo, hi = value * (1.0 - rel_tol), value * (1.0 + rel_tol)
    for den in range(1, max_den + 1):
        num = max(1, math.ceil(lo * float(den)))
        while float(num) < lo * float(den):
            num += 1
        while num > 1 and float(num - 1) >= lo * float(den):
            num -= 1
        if float(num) <= hi * float(den) and num <= max_num:
            return num, den
        if num > max_num:
            return None  # a larger denominator needs a larger numerator still
    return None
