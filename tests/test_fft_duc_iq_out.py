"""The FftDuc and the MixedFftDuc writing sc16 / sc8 / cu8 from the inverse kernel (gr4pm_fft_duc_process_iq,
gr4pm_fft_duc_mixed_process_iq) against today's two-call form on a second handle with the same
settings: pkg.iq_pack of the twin's band, byte for byte and count for count (tests/_iq_out.py).

Shapes: FftDuc(K = 3, I = 16) (hop 1792 samples = 112 items) in calls of 50, 0, 400, 1 and 137 items;
MixedFftDuc([-0.31, 0.05, 0.17], [4, 16, 64]) (hop 1280 samples = 20 slots) in calls of 7, 0, 70, 1 and 30 slots; and the
FftDuc at the smallest hop its constructor takes, overlap 1984 and hop 64 (the hop is 2048 minus a multiple of the
interpolation, so never odd), in calls of 3, 0, 30, 1 and 14 items.  In each the first call delivers no whole segment,
the third at least three -- segment 0 with its skipped lanes, and a wave's run of more than one segment -- and
flush(format=...) closes the stream.

The kernel's unit is built with -ffp-contract=fast, under which cu8's x * gain + 127.5 fuses unless pack_component keeps the
product from the sum (iq_format.hpp: kContracting).  The gains above are powers of two, where the product is exact and fused and unfused agree in every bit, so
those cases cannot see a lost guard.  test_cu8_at_a_gain_that_is_no_power_of_two can: 2^23 samples of both banks at gain
200, where the fused form gives another byte in about two components per million, and the test first counts on the host
how many of its own components a fused pack would change."""
import ctypes as C

import numpy as np
import pytest

import _iq_out as io
import _iq_ref
from _frontend import host, load_package

pytestmark = pytest.mark.gpu

FREQS = [-0.31, 0.05, 0.17]


def _uniform(name, cuts, seed, **kw):
    return io.Shape(name, lambda pkg: pkg.FftDuc(FREQS, 16, **kw), [1, 1, 1], sum(cuts), cuts, True, seed)


def _mixed(name, cuts, seed):
    Is = [4, 16, 64]
    return io.Shape(name, lambda pkg: pkg.MixedFftDuc(FREQS, Is), [max(Is) // i for i in Is], sum(cuts), cuts, True, seed)


UNIFORM = _uniform("FftDuc_K3_I16", (50, 0, 400, 1, 137), 21)
MIXED = _mixed("Mixed_4_16_64", (7, 0, 70, 1, 30), 22)
SHORT_HOP = _uniform("FftDuc_hop64", (3, 0, 30, 1, 14), 23, overlap=1984)
SHAPES = [UNIFORM, MIXED, SHORT_HOP]
CASES = [(s, f, g) for s in SHAPES for f in io.FORMATS for g in io.gains(f)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_the_shapes_are_what_the_cuts_were_chosen_for(pkg):
    u, m, s = (x.make(pkg) for x in SHAPES)
    assert (u.hop, m.hop, s.hop) == (1792, 1280, 64)
    for shape in SHAPES:
        b, lengths = shape.make(pkg), []
        for lo, hi in shape.spans():
            lengths.append(shape.call(b, lo, hi).shape[0])
        assert lengths[0] == 0 and lengths[2] >= 3 * b.hop and b.flush().shape[0] > 0


@pytest.mark.parametrize("fmt", io.FORMATS)
def test_the_yardstick_is_the_numpy_statement(pkg, fmt):
    for shape in (UNIFORM, MIXED):
        for gain in io.gains(fmt):
            io.check_against_numpy(pkg, shape, fmt, gain)


@pytest.mark.parametrize("shape,fmt,gain", CASES, ids=lambda v: str(v))
def test_call_by_call_equals_the_twin_packed(pkg, shape, fmt, gain):
    import torch
    want, count = io.packed(pkg, shape, fmt, gain)
    if gain is not None:  # a case where nothing or everything clamps shows nothing
        assert 0 < count < want.numel() // 2, (count, want.numel())
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    parts = io.fused(pkg, shape, fmt, gain, clipped=c)
    assert parts[0].shape[0] == 0 and parts[0].dtype == io.dtype_of(fmt)
    io.assert_calls_equal(parts, want)
    assert int(c.item()) == count


LONG = [_uniform("FftDuc_K3_I16_long", (1 << 19,), 24), _mixed("Mixed_4_16_64_long", (1 << 17,), 25)]


@pytest.mark.parametrize("shape", LONG, ids=str)
def test_cu8_at_a_gain_that_is_no_power_of_two(pkg, shape):
    """the one case that fails if pack_component's product and sum fuse in the inverse kernel's unit (seen to fail with a
    library whose pack had no guard against it)"""
    import torch
    gain = 200.0
    band = host(io.twin(pkg, shape))
    assert band.size >= 1 << 23
    x = band.view(np.float32).astype(np.float64)  # float32 x float32 is exact in float64, and so is adding 127.5 to it here
    fused = np.rint((x * gain + 127.5).astype(np.float32))
    apart = np.rint((x * gain).astype(np.float32) + np.float32(127.5))
    assert np.count_nonzero(fused != apart) >= 8  # else the case shows nothing
    want, count = io.packed(pkg, shape, "cu8", gain)
    assert np.array_equal(host(want).reshape(-1), np.clip(apart, 0, 255).astype(np.uint8))
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    parts = io.fused(pkg, shape, "cu8", gain, clipped=c)
    io.assert_calls_equal(parts, want)
    assert int(c.item()) == count


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("fmt", io.FORMATS)
def test_nan_items_pack_to_the_formats_nan_value(pkg, shape, fmt):
    import torch
    band = host(io.twin(pkg, shape, nan=True))
    hit = np.isnan(band.real) | np.isnan(band.imag)  # the whole segments the item is in
    assert 0 < hit.sum() < band.size
    want, count = io.packed(pkg, shape, fmt, None, nan=True)
    rows = [r.copy() for r in shape.rows]
    rows[0][io.nan_item(shape)] = np.nan
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    parts = io.fused(pkg, shape, fmt, None, rows=rows, clipped=c)
    io.assert_calls_equal(parts, want)
    got = host(torch.cat(parts))
    assert np.all(got[hit] == _iq_ref.FORMATS[fmt][6])
    assert int(c.item()) == count >= 2 * hit.sum()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("fmt", io.FORMATS)
def test_out_aligned_and_one_item_off(pkg, shape, fmt):
    import torch
    want, count = io.packed(pkg, shape, fmt, io.gains(fmt)[1])
    for off in (0, 1):
        bufs = []

        def outs(n):
            buf = torch.full((n + 9, 2), 77, dtype=io.dtype_of(fmt), device="cuda")
            assert buf.data_ptr() % 16 == 0
            bufs.append((buf, n))
            return buf[off:off + n]

        c = torch.zeros(1, dtype=torch.int64, device="cuda")
        parts = io.fused(pkg, shape, fmt, io.gains(fmt)[1], clipped=c, outs=outs)
        io.assert_calls_equal(parts, want)
        assert int(c.item()) == count
        for (buf, n), p in zip(bufs, parts):  # written where it was told to, and nowhere else (flush() makes its own)
            assert bool((buf[:off] == 77).all()) and bool((buf[off + n:] == 77).all())


@pytest.mark.parametrize("shape", [UNIFORM, MIXED], ids=str)
def test_formats_mix_on_one_handle(pkg, shape):
    import torch
    band = io.twin(pkg, shape)
    b = shape.make(pkg)
    at, u = 0, shape.units
    spans = [(0, u // 4), (u // 4, u // 2), (u // 2, u // 2 + 1), (u // 2 + 1, u - 3), (u - 3, u)]
    for (lo, hi), fmt in list(zip(spans, [None, "sc16", "cu8", "sc8", None])) + [((None, None), "cu8")]:
        if lo is None:
            x = b.flush(format=fmt)
        else:
            x = shape.call(b, lo, hi) if fmt is None else shape.call(b, lo, hi, format=fmt)
        n = x.shape[0]
        want = band[at:at + n] if fmt is None else pkg.iq_pack(band[at:at + n], fmt)
        assert torch.equal(x, want), (fmt, lo, hi)
        at += n
    assert at == band.numel()


@pytest.mark.parametrize("shape", [UNIFORM, MIXED], ids=str)
def test_refusals_leave_the_stream_where_it_was(pkg, shape):
    import torch
    want, _ = io.packed(pkg, shape, "cu8", None)
    b = shape.make(pkg)
    lo, hi = shape.cuts[0], shape.cuts[0] + shape.cuts[2]
    first = shape.call(b, 0, lo, format="cu8")
    n_next = shape.samples(b, lo, hi)
    assert n_next > 0
    with pytest.raises(pkg.Gr4pmError):
        shape.call(b, lo, hi, format="sc12")
    with pytest.raises(pkg.Gr4pmError):
        shape.call(b, lo, hi, format="cu8", out=torch.empty((n_next - 1, 2), dtype=torch.uint8, device="cuda"))
    with pytest.raises(pkg.Gr4pmError):
        shape.call(b, lo, hi, format="cu8", out=torch.empty((n_next, 2), dtype=torch.int8, device="cuda"))
    # the entries themselves: an unknown format and too little room, refused with *n_out = 0 before anything is enqueued
    L, v = pkg.lib(), shape.window(lo, hi)
    entry = L.gr4pm_fft_duc_mixed_process_iq if shape is MIXED else L.gr4pm_fft_duc_process_iq
    out = torch.full((n_next, 2), 77, dtype=torch.uint8, device="cuda")
    n = C.c_size_t(5)
    assert entry(b._h, v.data_ptr(), v.stride(0), hi - lo, out.data_ptr(), 9, 0.0, n_next, C.byref(n), None) == -1
    assert n.value == 0 and b"format" in L.gr4pm_last_error()
    n = C.c_size_t(5)
    assert entry(b._h, v.data_ptr(), v.stride(0), hi - lo, out.data_ptr(), 3, 0.0, n_next - 1, C.byref(n), None) != 0
    assert n.value == 0 and bool((out == 77).all())
    rest = [shape.call(b, lo, hi, format="cu8"), shape.call(b, hi, shape.units, format="cu8"), b.flush(format="cu8")]
    io.assert_calls_equal([first] + rest, want)


@pytest.mark.parametrize("fmt", io.FORMATS)
def test_the_counter_is_added_to_and_may_be_absent(pkg, fmt):
    import torch
    for shape in (UNIFORM, MIXED):
        gain = io.gains(fmt)[1]
        want, count = io.packed(pkg, shape, fmt, gain)
        io.assert_calls_equal(io.fused(pkg, shape, fmt, gain, clipped=None), want)
        c = torch.full((1,), 7, dtype=torch.int64, device="cuda")
        io.fused(pkg, shape, fmt, gain, clipped=c)
        assert int(c.item()) == 7 + count
