"""Ddc.extract on the GPU (gr4pm_ddc_extract): spans of a recording, computed on their own, have the
bits of the streaming output's slices -- at every tile boundary, with chunked taps, from integer IQ, from a start beyond
2^32, from a window of the recording and past its end; they stay within test_ddc.py's bound of the float64 reference;
the call leaves the handle's stream alone; more than 64 spans go through; and every refusal returns its status.

Input is seeded random complex64, 40 000 samples."""
import ctypes as C
import functools

import numpy as np
import pytest

import _ddc_extract_ref as xref
import _ddc_ref as dref
from _frontend import FREQ_POOL, bits, dev, exact_iq_forms, host, load_package, random_taps

pytestmark = pytest.mark.gpu

N = 40000
# (16, 8192, 9): chunked taps, T = 255, channel 8 alone in the second group; (1000, 2000, 2): tiles of 3 frames, 40 frames
SHAPES = [(5, 60, 3), (1, 1, 1), (3, 96, 2), (20, 161, 16), (16, 8192, 9), (1000, 2000, 2)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def tile_frames(D, L):
    """T of hostlogic/xlate_geometry.hpp's ddc_geometry(D, L)"""
    cols = 8192 // D
    cols -= cols % 2 == 0
    T = 256
    if T + (L - 1) // D > cols:
        T = min(cols // 2, 256)
    return T


def freqs_of(D, L, K):
    o = SHAPES.index((D, L, K)) if (D, L, K) in SHAPES else 0
    return [FREQ_POOL[(o + k) % len(FREQ_POOL)] for k in range(K)]


@functools.lru_cache(maxsize=None)
def stream(n=N, seed=11):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    return x


def make(pkg, D, L, K, start=0, n=N):
    return pkg.Ddc(freqs_of(D, L, K), D, taps=random_taps(D, L, 3), start_index=start, max_frames=n // D + 1)


def the_spans(D, L, K, F):
    """(channel, first_frame, n_frames) for a stream of F frames: frame 0, where the window lies before the start; 1,
    T - 1, T, T + 1 and 2 T + 3 frames; a span that ends at the last frame; two overlapping spans of different channels;
    one span twice; an empty one; every channel"""
    T = tile_frames(D, L)
    spans = [(0, 0, min((L - 1) // D + 2, F))]
    for i, n in enumerate(n for n in (1, T - 1, T, T + 1, 2 * T + 3) if 0 < n <= F):
        spans.append((i % K, min(7 + 13 * i, F - n), n))
    n = min(T + 1, F)
    spans.append((K - 1, F - n, n))
    a = min(F // 3, F - n - n // 2)
    spans += [(0, a, n), (K - 1, a + n // 2, n)]
    spans += [(K // 2, F // 2, min(5, F - F // 2))] * 2
    spans.append((0, 5, 0))
    spans += [(k, (3 * k) % (F - 1), 2) for k in range(K)]
    return spans


def assert_rows_are_slices(rows, lengths, spans, full, what=""):
    rows = host(rows)
    assert rows.shape[0] == len(spans) and list(lengths) == [n for _, _, n in spans]
    for b, (k, a, n) in enumerate(spans):
        assert np.array_equal(bits(rows[b, :n]), bits(full[k, a:a + n])), f"{what} span {b} = {(k, a, n)}"
        assert not bits(rows[b, n:]).any(), f"{what} span {b} = {(k, a, n)}: the rest of the row is not +0"


# ---- (a) bit for bit against the stream ----

@pytest.mark.parametrize("D,L,K", SHAPES)
def test_spans_are_slices_of_the_stream(pkg, D, L, K):
    x = stream()
    d = make(pkg, D, L, K)
    full = host(d.process_bulk(dev(x)))
    F = N // D
    assert full.shape == (K, F)
    spans = the_spans(D, L, K, F)
    assert {k for k, _, _ in spans} == set(range(K))
    n_cols = max(n for _, _, n in spans) + 7
    rows, lengths = make(pkg, D, L, K).extract(dev(x), spans, n_cols=n_cols)
    assert tuple(rows.shape) == (len(spans), n_cols)
    assert_rows_are_slices(rows, lengths, spans, full)
    # into a tensor of the caller's, full of something else, with a wider row stride
    import torch
    out = torch.full((len(spans), n_cols + 9), complex("nan"), dtype=torch.complex64, device="cuda")
    rows2, _ = d.extract(dev(x), spans, n_cols=n_cols, out=out)
    assert rows2.data_ptr() == out.data_ptr()
    assert_rows_are_slices(rows2, lengths, spans, full, "out=")
    assert np.all(np.isnan(host(out)[:, n_cols:]))  # nothing behind n_cols is written
    # a structured array, and n_cols by default the longest span
    rec = np.array([(k, n, a) for k, a, n in spans], dtype=pkg.Ddc.SPAN_DTYPE)
    rows3, _ = d.extract(dev(x), rec)
    assert rows3.shape[1] == n_cols - 7
    assert np.array_equal(bits(host(rows3)), bits(host(rows)[:, :n_cols - 7]))


def test_integer_input(pkg):
    D, L, K = 5, 60, 3
    x, forms = exact_iq_forms(N, 5)
    spans = the_spans(D, L, K, N // D)
    n_cols = max(n for _, _, n in spans) + 7
    first = None
    for v, scale in forms:
        d = make(pkg, D, L, K)
        full = host(d.process_bulk(dev(v), scale=scale))
        rows, lengths = d.extract(dev(v), spans, n_cols=n_cols, scale=scale)
        assert_rows_are_slices(rows, lengths, spans, full, str(v.dtype))
        first = full if first is None else first
        assert np.array_equal(bits(full), bits(first))  # the forms hold the same samples


def test_start_beyond_2_32(pkg):
    D, L, K = 5, 60, 3
    start = (1 << 40) + 3
    x = stream()
    d = make(pkg, D, L, K, start=start)
    full = host(d.process_bulk(dev(x)))
    assert not np.array_equal(bits(full), bits(host(make(pkg, D, L, K).process_bulk(dev(x)))))  # the start matters
    spans = the_spans(D, L, K, N // D)
    rows, lengths = d.extract(dev(x), spans, n_cols=max(n for _, _, n in spans) + 7)
    assert_rows_are_slices(rows, lengths, spans, full)


# ---- (b) a window of the stream, (c) zero extension ----

@pytest.mark.parametrize("start", [0, (1 << 40) + 3])
def test_a_window_of_the_stream(pkg, start):
    D, L, K = 5, 60, 3
    x = stream()
    d = make(pkg, D, L, K, start=start)
    full = host(d.process_bulk(dev(x)))
    cut = 20000
    f_min = -(-(cut + L - D) // D)  # the first frame whose oldest sample, f D + D - 1 - (L - 1), is at or after the cut
    assert f_min * D + D - L >= cut > (f_min - 1) * D + D - L
    spans = [(0, f_min, 300), (1, f_min + 1, 257), (2, N // D - 40, 40), (1, f_min + 700, 1)]
    rows, lengths = d.extract(dev(x[cut:]), spans, n_cols=307, x_index=start + cut)
    assert_rows_are_slices(rows, lengths, spans, full)
    # one frame earlier the window's oldest sample is missing: that item differs, the rest of the row does not
    rows, _ = d.extract(dev(x[cut:]), [(0, f_min - 1, 5)], x_index=start + cut)
    got = host(rows)[0]
    assert got[0] != full[0, f_min - 1] and np.array_equal(bits(got[1:]), bits(full[0, f_min:f_min + 4]))


def test_zero_extension(pkg):
    D, L, K = 5, 60, 3
    x = stream()
    pad = 400 * D
    d = make(pkg, D, L, K, n=N + pad)
    full = host(d.process_bulk(dev(np.concatenate([x, np.zeros(pad, np.complex64)]))))
    F = N // D
    spans = [(0, F - 10, 300), (2, F - 1, 2), (1, F + 10, 3), (1, F + 200, 50)]
    rows, lengths = d.extract(dev(x), spans, n_cols=307)
    assert_rows_are_slices(rows, lengths, spans, full)
    assert not bits(host(rows)[3]).any() and host(rows)[2].any()  # L - 1 samples behind the end still see the buffer
    # a buffer that begins before the handle's start: what lies before the start counts as zero
    d5 = make(pkg, D, L, K, start=1000)
    full5 = host(d5.process_bulk(dev(x[37:])))
    spans = [(0, 0, 30), (2, 3, 258)]
    rows, lengths = d5.extract(dev(x), spans, n_cols=265, x_index=1000 - 37)
    assert_rows_are_slices(rows, lengths, spans, full5)


# ---- (d) against float64 ----

@pytest.mark.parametrize("D,L,K", [(5, 60, 3), (64, 768, 8)])
def test_against_float64(pkg, D, L, K):
    """test_ddc.py's bound, |y - y64| <= C 2^-24 sum|h| max|x| with C = L + 8, against extract64; the maximum is taken
    over the L samples of the zero-extended stream an item is made of, and an item made of zeros alone is exactly zero"""
    x = stream()
    h = random_taps(D, L, 3)
    f = freqs_of(D, L, K)
    start, cut = 12345, 3000
    T = tile_frames(D, L)
    spans = [(0, 0, T + 1), (K - 1, cut // D - 3, 2 * T + 3), (K // 2, N // D - 20, 60), (1, N // D + 100, 4)]
    n_cols = 2 * T + 10
    d = pkg.Ddc(f, D, taps=h, start_index=start)
    rows, _ = d.extract(dev(x[cut:]), spans, n_cols=n_cols, x_index=start + cut)
    y = host(rows).astype(np.complex128)
    y64 = xref.extract64(x[cut:], h, D, f, start, start + cut, spans, n_cols)
    scale = dref.EPS32 * np.sum(np.abs(h.astype(np.float64))) * xref.window_max(x[cut:], D, L, start, start + cut, spans, n_cols)
    err = np.abs(y - y64)
    assert np.all(err[scale == 0] == 0) and np.any(scale == 0)
    r = err[scale > 0] / scale[scale > 0]
    print(f"\n[ddc extract float64] D = {D}, L = {L}, K = {K}: max ratio {r.max():.3f}, rms {np.sqrt(np.mean(r ** 2)):.4f} (C = {L + 8})")
    assert r.max() <= L + 8
    assert np.max(np.abs(y64)) > 0.1  # the stimulus reaches the output


# ---- (e) the handle is untouched, (f) more than 64 spans ----

def test_the_handle_is_untouched(pkg):
    D, L, K = 5, 60, 3
    x = stream()
    full = host(make(pkg, D, L, K).process_bulk(dev(x)))
    d = make(pkg, D, L, K)
    a = 17003  # not a multiple of D: the handle carries an incomplete frame across the extract
    first = host(d.process_bulk(dev(x[:a])))
    rows, lengths = d.extract(dev(x), [(1, 100, 300), (0, 0, 7)], x_index=0)
    assert_rows_are_slices(rows, lengths, [(1, 100, 300), (0, 0, 7)], full)
    second = host(d.process_bulk(dev(x[a:])))
    assert np.array_equal(bits(np.concatenate([first, second], axis=1)), bits(full))


def test_more_than_64_spans(pkg):
    D, L, K = 5, 60, 3
    x = stream()
    d = make(pkg, D, L, K)
    full = host(d.process_bulk(dev(x)))
    rng = np.random.default_rng(9)
    spans = [(int(rng.integers(0, K)), int(rng.integers(0, N // D - 300)), int(rng.integers(0, 300))) for _ in range(130)]
    rows, lengths = d.extract(dev(x), spans, n_cols=300)
    assert_rows_are_slices(rows, lengths, spans, full)


# ---- (g) the refusals ----

def test_every_refusal_returns_its_status(pkg):
    import torch
    lib = pkg.lib()
    D, L, K = 5, 60, 3
    x = dev(stream())
    d = make(pkg, D, L, K)
    full = host(d.process_bulk(x))
    d.reset()
    Span = pkg.Ddc.SPAN_DTYPE
    n_cols, stride = 16, 24
    out = torch.full((65, stride), complex("nan"), dtype=torch.complex64, device="cuda")

    def call(h=d, inp=x.data_ptr(), n_in=N, in_index=0, spans=((0, 0, 4), (2, 7, 5)), n_spans=None, outp=out.data_ptr(),
             out_stride=stride, cols=n_cols, fmt=None):
        rec = np.array([(k, n, a) for k, a, n in spans], dtype=Span) if spans is not None else None
        ptr = rec.ctypes.data_as(C.c_void_p) if rec is not None else None
        count = len(spans) if n_spans is None else n_spans
        if fmt is None:
            return lib.gr4pm_ddc_extract(h._h if h else None, inp, n_in, in_index, ptr, count, outp, out_stride, cols)
        return lib.gr4pm_ddc_extract_iq(h._h if h else None, inp, fmt, 0.0, n_in, in_index, ptr, count, outp, out_stride, cols)

    rational = pkg.Ddc([0.1, 0.2, 0.3], 5, interpolation=2)
    top = ((1 << 64) - 1) // D
    refused = [
        (dict(h=rational), -1, b"interpolation"),
        (dict(h=rational, n_spans=0), -1, b"interpolation"),
        (dict(spans=((0, 0, 1),) * 65), -1, b"spans"),
        (dict(spans=None, n_spans=2), -1, b"spans"),
        (dict(spans=((0, 0, 4), (3, 7, 5))), -1, b"channel"),
        (dict(spans=((0, 0, 4), (2, 7, 17))), -5, b"columns"),
        (dict(out_stride=15), -1, b"stride"),
        (dict(spans=((0, 0, 4), (2, top - 1, 5))), -5, b"64 bits"),
        (dict(spans=((0, 0, 4), (2, (1 << 64) - 3, 5))), -5, b"64 bits"),
        (dict(in_index=(1 << 64) - 100), -5, b"index"),
        (dict(inp=None), -1, b"input"),
        (dict(outp=None), -1, b"output"),
        (dict(fmt=9), -1, b"format"),
        (dict(h=None), -1, None),
    ]
    for kw, status, text in refused:
        assert call(**kw) == status, kw
        assert text is None or text in lib.gr4pm_last_error(), (kw, lib.gr4pm_last_error())
    # what is no refusal: nothing to do, one span with any stride, no input for no samples
    assert call(n_spans=0) == 0 and call(cols=0) == 0 and call(spans=(), outp=None) == 0
    torch.cuda.synchronize()
    assert np.all(np.isnan(host(out)))  # nothing was enqueued: the output is unwritten
    with pytest.raises(pkg.Gr4pmError):
        rational.extract(x, [(0, 0, 4)])
    with pytest.raises(pkg.Gr4pmError):
        d.extract(x, [(3, 0, 4)])
    with pytest.raises(pkg.Gr4pmError):
        d.extract(x, [(0, 0, 4)], n_cols=3)
    with pytest.raises(pkg.Gr4pmError):
        d.extract(x, [(0, -1, 4)])
    assert call(spans=((1, 3, 9),), out_stride=0) == 0
    assert np.array_equal(bits(host(out)[0, :9]), bits(full[1, 3:12])) and not bits(host(out)[0, 9:n_cols]).any()
    assert call(inp=None, n_in=0) == 0
    assert not bits(host(out)[:2, :n_cols]).any() and np.all(np.isnan(host(out)[:2, n_cols:]))
    # 64 spans are admitted; the handle still works, and still stands at its start
    spans = tuple((b % K, 11 * b, 1 + b % 16) for b in range(64))
    assert call(spans=spans) == 0
    got = host(out)
    for b, (k, a, n) in enumerate(spans):
        assert np.array_equal(bits(got[b, :n]), bits(full[k, a:a + n])) and not bits(got[b, n:n_cols]).any()
    assert np.all(np.isnan(got[64])) and np.all(np.isnan(got[:, n_cols:]))
    assert np.array_equal(bits(host(d.process_bulk(x))), bits(full))
