"""Float64 numpy restatement of the Spectrum block's definition and of the carrier finder, written from their
specification (include/gr4pm_hip.h), not from the library.

    segment s = x[s hop .. s hop + N), N = 2048; no zero prehistory: T < N ? 0 : (T - N) / hop + 1 segments after T samples
    X_s = FFT_N(w x_s) (forward, unnormalised), acc[k] = sum_s |X_s[k]|^2, max[k] = max_s |X_s[k]|^2
    mean = acc / (segments sum w^2), max_hold = max / sum w^2
"""
import numpy as np

N = 2048


def segments(T, hop, n=N):
    return 0 if T < n else (T - n) // hop + 1


def hann(n=N):
    """periodic Hann in float64, rounded to float32 once"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)).astype(np.float32)


def spectra(x, hop, window):
    """X64[s, k]: the float64 transforms of every segment of x (complex, any float type) under the float32 window"""
    x = np.asarray(x).astype(np.complex128)
    w = np.asarray(window, dtype=np.float32).astype(np.float64)
    S = segments(x.size, hop)
    X = np.empty((S, N), dtype=np.complex128)
    for s in range(S):
        X[s] = np.fft.fft(w * x[s * hop: s * hop + N])
    return X


def welch(x, hop, window):
    """dict(acc, max, mean, max_hold, segments, X) in float64"""
    X = spectra(x, hop, window)
    P = X.real ** 2 + X.imag ** 2
    wp = float(np.sum(np.asarray(window, dtype=np.float32).astype(np.float64) ** 2))
    S = X.shape[0]
    acc = P.sum(axis=0) if S else np.zeros(N)
    mx = P.max(axis=0) if S else np.zeros(N)
    return dict(acc=acc, max=mx, mean=acc / (S * wp) if S else np.zeros(N), max_hold=mx / wp, segments=S, X=X, window_power=wp)


def bounds(X, float_run, C=8.0):
    """the float32 error bounds of acc and max against float64: with delta_s = C 2^-24 ||X_s||_2,
    |acc32 - acc64| <= sum_s (2 |X_s[k]| delta_s + delta_s^2) + float_run 2^-24 acc64[k] and
    |max32 - max64| <= max_s (2 |X_s[k]| delta_s + delta_s^2)"""
    eps = 2.0 ** -24
    if not X.shape[0]:
        return np.zeros(N), np.zeros(N)
    delta = C * eps * np.sqrt((X.real ** 2 + X.imag ** 2).sum(axis=1))[:, None]
    per = 2.0 * np.abs(X) * delta + delta ** 2
    acc = (X.real ** 2 + X.imag ** 2).sum(axis=0)
    return per.sum(axis=0) + float_run * eps * acc, per.max(axis=0)


CARRIER_FIELDS = ("frequency", "bandwidth", "power", "snr_db", "first_bin", "n_bins")


def find_carriers(psd, threshold_db=6.0, max_gap_bins=2, min_width_bins=4):
    """list of dicts in ascending frequency"""
    psd = np.asarray(psd, dtype=np.float64)
    n = psd.size
    floor = np.sort(psd)[(n - 1) // 2]
    occ = psd > floor * 10.0 ** (threshold_db / 10.0)
    if not occ.any() or occ.all():
        return []
    # walk the circle from behind the longest stretch of free bins (the first of equals by its first bin)
    best_start, best_len = 0, 0
    for k in range(n):
        if occ[k] or not occ[k - 1]:
            continue
        ln = 0
        while not occ[(k + ln) % n]:
            ln += 1
        if ln > best_len:
            best_start, best_len = k, ln
    p0 = (best_start + best_len) % n
    order = [(p0 + i) % n for i in range(n - best_len)]
    runs = []  # [first index into order, last index]
    for i, k in enumerate(order):
        if not occ[k]:
            continue
        if runs and i - runs[-1][1] - 1 <= max_gap_bins:
            runs[-1][1] = i
        else:
            runs.append([i, i])
    out = []
    for i0, i1 in runs:
        ln = i1 - i0 + 1
        if ln < min_width_bins:
            continue
        a = order[i0]
        num = den = 0.0
        peak = -np.inf
        for t in range(ln):
            v = float(psd[(a + t) % n])
            num += t * (v - floor)
            den += v - floor
            peak = max(peak, v)
        f = (a + num / den) / n
        f -= np.floor(f + 0.5)
        with np.errstate(divide="ignore"):
            snr = 10.0 * np.log10(peak / floor)
        out.append(dict(frequency=f, bandwidth=ln / n, power=den, snr_db=snr, first_bin=a, n_bins=ln))
    out.sort(key=lambda c: c["frequency"])
    return out
