"""float64 statement of Ddc.extract (include/gr4pm_hip.h), for the tests: spans of the Ddc's output
from the zero-extended stream, built from _ddc_ref.ddc64_rotated.

The stream of a call is x inside [x_index, x_index + len(x)) and zero everywhere else, including everything before the
handle's start; frame n of channel k is _ddc_ref's y_k[n] with i = start + n D + D - 1.  tests/test_ddc_extract_ref.py
pins single items to _ddc_ref.ddc64_direct."""
import numpy as np

import _ddc_ref as dref


def zero_extended(x, start, x_index, first_sample, n_samples):
    """the call's stream at the absolute indices first_sample .. first_sample + n_samples - 1 (first_sample >= start), in
    the dtype of x"""
    x = np.asarray(x)
    assert first_sample >= start
    z = np.zeros(n_samples, dtype=x.dtype)
    lo = max(first_sample, x_index, start)
    hi = min(first_sample + n_samples, x_index + x.size)
    if hi > lo:
        z[lo - first_sample:hi - first_sample] = x[lo - x_index:hi - x_index]
    return z


def extract64(x, h, D, freqs, start, x_index, spans, n_cols):
    """[len(spans), n_cols] complex128: row b holds the frames first_frame .. first_frame + n_frames - 1 of channel
    spans[b][0], zeros behind them.  spans: (channel, first_frame, n_frames)."""
    h = np.asarray(h, dtype=np.float64)
    L = h.size
    out = np.zeros((len(spans), n_cols), dtype=np.complex128)
    lead = -(-(L - 1) // D)  # frames whose window reaches before the first sample handed to ddc64_rotated
    for b, (k, first, n) in enumerate(spans):
        if n == 0:
            continue
        assert n <= n_cols
        f_lo = max(0, first - lead)  # f_lo = 0: the zeros ddc64_rotated puts in front are the stream's own
        s0 = start + f_lo * D
        z = zero_extended(np.asarray(x).astype(np.complex128), start, x_index, s0, (first + n - f_lo) * D)
        y = dref.ddc64_rotated(z, h, D, [freqs[k]], s0)
        out[b, :n] = y[0, first - f_lo:first - f_lo + n]
    return out


def window_max(x, D, L, start, x_index, spans, n_cols):
    """per item of extract64's result: max |x| over the L samples of the zero-extended stream it is made of (0 behind a span)"""
    out = np.zeros((len(spans), n_cols))
    lead = -(-(L - 1) // D)
    for b, (_, first, n) in enumerate(spans):
        if n == 0:
            continue
        f_lo = max(0, first - lead)
        z = zero_extended(x, start, x_index, start + f_lo * D, (first + n - f_lo) * D)
        out[b, :n] = dref.window_max(z, D, L)[first - f_lo:first - f_lo + n]
    return out
