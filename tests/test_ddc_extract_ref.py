"""The float64 reference of Ddc.extract (tests/_ddc_extract_ref.py) against a direct evaluation of single items with
Python integers (_ddc_ref.ddc64_direct on the zero-extended stream), on the CPU: items whose samples lie before the
handle's start, a buffer that begins before the start (those samples count as zero), a buffer that begins late, spans
across the buffer's end and behind it, and a start beyond 2^32."""
import numpy as np
import pytest

import _ddc_extract_ref as xref
import _ddc_ref as dref

FREQS = [-0.3137, 3.0 * 2.0 ** -32, 0.123456789]
D, L = 5, 60


def stream(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


# (start, x_index - start): the buffer at the start, 37 samples before it, 143 samples after it
@pytest.mark.parametrize("start,offset", [(0, 0), (12345, 0), (12345, -37), (12345, 143), ((1 << 32) - 100, 0), ((1 << 40) + 3, 143),
                                          ((1 << 40) + 3, -37)])
def test_single_items_against_python_integers(start, offset):
    x = stream(70 * D + 2, 7)
    h = np.random.default_rng(8).standard_normal(L)
    x_index = start + offset
    n_stream = x.size + offset  # the buffer's end, counted from the start
    last = n_stream // D - 1    # the last frame whose samples all lie inside or before the buffer
    spans = [(0, 0, 13),               # frame 0 .. 11: samples before the start
             (1, 20, 1),
             (2, last - 4, 5),         # ends at the buffer's last frame
             (0, last - 2, 9),         # across the buffer's end
             (1, last + 20, 3),        # behind it: zeros
             (2, 7, 0),
             (1, 28, 6), (2, 30, 6)]   # overlapping, two channels (with offset 143: across the buffer's first sample)
    n_cols = 13 + 7
    got = xref.extract64(x, h, D, FREQS, start, x_index, spans, n_cols)
    assert got.shape == (len(spans), n_cols)
    # the zero-extended stream from the start on, long enough for every span, and the items one by one
    n_frames = max(f + n for _, f, n in spans)
    z = xref.zero_extended(x, start, x_index, start, n_frames * D)
    if offset < 0:
        assert np.array_equal(z[:10], x[-offset:-offset + 10])  # what lies before the start is dropped, not shifted
    if offset > 0:
        assert not z[:offset].any() and z[offset] == x[0]
    sc = np.sum(np.abs(h)) * np.max(np.abs(x))
    for b, (k, first, n) in enumerate(spans):
        want = dref.ddc64_direct(z, h, D, [FREQS[k]], start, list(range(first, first + n)))[0] if n else np.zeros(0)
        assert np.max(np.abs(got[b, :n] - want), initial=0.0) <= 1e-12 * sc, (b, k, first, n)
        assert not got[b, n:].any()
    assert not got[4].any()                      # behind the buffer by more than the filter's length
    assert np.all(got[3, :9] != 0)               # the filter's length behind the buffer's end still sees it
    # the start matters: the same buffer at another start gives other values
    other = xref.extract64(x, h, D, FREQS, start + 1, x_index + 1, spans, n_cols)
    assert np.abs(other[2, 0] - got[2, 0]) > 1e-3 * np.abs(got[2, 0])


def test_window_max_of_a_span():
    x = stream(300, 3) * (np.random.default_rng(4).random(300) < 0.2)
    start, x_index = 1000, 1040
    spans = [(0, 0, 9), (1, 50, 12), (0, 3, 0)]
    got = xref.window_max(x, D, L, start, x_index, spans, 14)
    z = np.abs(xref.zero_extended(x, start, x_index, start, 62 * D))
    for b, (_, first, n) in enumerate(spans):
        for c in range(n):
            i = (first + c) * D + D - 1
            assert got[b, c] == np.max(z[max(0, i - L + 1):i + 1])
        assert not got[b, n:].any()
