"""Float64 numpy restatement of the Spectrogram block's definition, of the band power and of the burst finder, written
from their specification (include/gr4pm_hip.h) on top of _spectrum_ref.spectra, not from the
library.

    the segments and X_s are the Spectrum's; R = average
    row t = the segments t R .. t R + R - 1, S // R rows after S segments
    mean: row[t][k] = sum_s |X_s[k]|^2 / (R sum w^2)        max: row[t][k] = max_s |X_s[k]|^2 / sum w^2
    row t covers the samples [t R hop, t R hop + (R - 1) hop + N)
"""
import numpy as np

import _spectrum_ref as sref

N = sref.N
EPS = 2.0 ** -24


def n_rows(T, hop, R):
    return sref.segments(T, hop) // R


def window_power(window):
    return float(np.sum(np.asarray(window, dtype=np.float32).astype(np.float64) ** 2))


def normaliser(window, R, detector):
    """what a row's sum (or maximum) is divided by"""
    return (R if detector == "mean" else 1) * window_power(window)


def rows_from_spectra(X, R, detector, window):
    """float64 rows [S // R, N] from the float64 transforms X[S, N]"""
    T = X.shape[0] // R
    P = (X.real ** 2 + X.imag ** 2)[: T * R].reshape(T, R, N)
    red = P.sum(axis=1) if detector == "mean" else P.max(axis=1)
    return red / normaliser(window, R, detector)


def rows(x, hop, R, detector, window):
    return rows_from_spectra(sref.spectra(x, hop, window), R, detector, window)


def bound(X, R, detector, window, C=8.0):
    """the float32 error bound of every row value against float64, [S // R, N]: with delta_s = C 2^-24 ||X_s||_2 and
    e_s[k] = 2 |X_s[k]| delta_s + delta_s^2, divided by the row's normaliser,
        mean: sum_s e_s[k] + R 2^-24 sum_s |X_s[k]|^2        max: max_s e_s[k]
    plus 3 * 2^-24 * row64 for the rounding of inv and of the one product at the store"""
    T = X.shape[0] // R
    P = X.real ** 2 + X.imag ** 2
    delta = C * EPS * np.sqrt(P.sum(axis=1))[:, None]
    e = (2.0 * np.abs(X) * delta + delta ** 2)[: T * R].reshape(T, R, N)
    P = P[: T * R].reshape(T, R, N)
    if detector == "mean":
        b, red = e.sum(axis=1) + R * EPS * P.sum(axis=1), P.sum(axis=1)
    else:
        b, red = e.max(axis=1), P.max(axis=1)
    norm = normaliser(window, R, detector)
    return b / norm + 3.0 * EPS * red / norm


def band_power(rows_, bands):
    """[K, T] float64: the sum of the bins first_bin .. first_bin + n_bins - 1 mod N of each row, in double"""
    r = np.asarray(rows_).astype(np.float64)
    return np.stack([r[:, (a + np.arange(n)) % N].sum(axis=1) for a, n in bands]) if len(bands) else np.zeros((0, r.shape[0]))


def find_bursts(p, threshold_db=6.0, max_gap_rows=1, min_rows=2, floor=None):
    """list of dicts in ascending time"""
    p = np.asarray(p, dtype=np.float64)
    T = p.size
    if floor is None or not floor > 0:
        floor = float(np.sort(p)[(T - 1) // 2])
    active = p > floor * 10.0 ** (threshold_db / 10.0)
    runs = []  # [first, last], both active
    for t in np.flatnonzero(active):
        if runs and t - runs[-1][1] - 1 <= max_gap_rows:
            runs[-1][1] = int(t)
        else:
            runs.append([int(t), int(t)])
    out = []
    for a, b in runs:
        ln = b - a + 1
        if ln < min_rows:
            continue
        total, peak, peak_row = 0.0, -np.inf, a
        for t in range(a, b + 1):
            total += float(p[t]) - floor
            if p[t] > peak:
                peak, peak_row = float(p[t]), t
        with np.errstate(divide="ignore"):
            snr = 10.0 * np.log10(peak / floor)
        out.append(dict(first_row=a, n_rows=ln, peak_row=peak_row, power=total / ln, snr_db=snr))
    return out


def spans(found, row_advance, row_span, first_row=0):
    """[(start_sample, end_sample)] of find_bursts' result"""
    return [((first_row + b["first_row"]) * row_advance, (first_row + b["first_row"] + b["n_rows"] - 1) * row_advance + row_span)
            for b in found]


# ---- what tests/test_spectrogram_ref.py (CPU) and tests/test_spectrogram.py (GPU) share ----

# (hop, samples, R): every hop class of the Spectrum's tests; at hop 1 a stream of 301 segments (4 rows of 64 and a
# remainder) and one of 8192, whose 8192 and 2730 rows make waves walk runs of several rows
SHAPES = [(2048, 40000, 1), (2048, 40000, 3), (1024, 40000, 1), (1024, 40000, 3), (1000, 40000, 1), (1000, 40000, 3),
          (1, 2348, 1), (1, 2348, 3), (1, 2348, 64), (1, 10239, 1), (1, 10239, 3)]
DETECTORS = ("mean", "max")
KINDS = ("hann", "rect")

_cache = {}


def stimulus(n, seed=5):
    """tests/test_spectrum.py's: seeded Gaussian noise plus two tones, one of them off the bin grid"""
    if (n, seed) not in _cache:
        rng = np.random.default_rng(seed)
        t = np.arange(n, dtype=np.float64)
        x = 0.5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        x += 0.8 * np.exp(2j * np.pi * 0.12345 * t) + 0.3 * np.exp(2j * np.pi * (-777.0 / 2048) * t)
        x = x.astype(np.complex64)
        x.setflags(write=False)
        _cache[(n, seed)] = x
    return _cache[(n, seed)]


def window_of(kind):
    return sref.hann() if kind == "hann" else np.ones(N, dtype=np.float32)


def reference(n, hop, kind):
    """the float64 transforms of stimulus(n), computed once for the cases of one (stream, hop, window), which run back to
    back, and left unchanged; only the latest is kept (8192 segments are 256 MiB)"""
    key = ("X", n, hop, kind)
    if key not in _cache:
        for other in [k for k in _cache if k[0] == "X"]:
            del _cache[other]
        X = sref.spectra(stimulus(n), hop, window_of(kind))
        X.setflags(write=False)
        _cache[key] = X
    return _cache[key]


def worst_over_bound(got, n, hop, R, detector, kind):
    """max over rows and bins of |got - row64| / bound, for rows `got` of stimulus(n)"""
    X, w = reference(n, hop, kind), window_of(kind)
    want = rows_from_spectra(X, R, detector, w)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not want.size:
        return 0.0
    return float(np.max(np.abs(np.asarray(got).astype(np.float64) - want) / bound(X, R, detector, w)))
