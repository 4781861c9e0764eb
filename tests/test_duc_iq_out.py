"""The Duc writing sc16 / sc8 / cu8 from its kernel (gr4pm_duc_process_iq) against today's two-call
form on a second handle with the same settings: pkg.iq_pack(twin.process_bulk(v), fmt, gain, clipped=c2), byte for byte
and count for count (tests/_iq_out.py; that yardstick is itself checked against tests/_iq_ref.pack once per format).

Shapes: K = 3 at I = 5; K = 1 at I = 1 (the store's I == 1 branch); K = 2 at I = 64; the rational 25/4 and 16/3 with
K = 2; default prototypes.  Each handle is fed in calls of 1, 37, 0, 300 (16/3: 500) and 162 items.  The largest call
must span more than one of the kernel's tiles and end inside one: test_the_largest_call_crosses_a_tile_and_ends_inside_one
asks every handle for its tile (Duc.tile_items) and checks that.  A call's default `out` is 16-byte aligned; the alignment
test also writes to a view one item behind such a boundary."""
import ctypes as C

import numpy as np
import pytest

import _iq_out as io
import _iq_ref
from _frontend import host, load_package

pytestmark = pytest.mark.gpu


def _shape(name, K, I, D, seed, big=300):
    freqs = [-0.31, 0.05, 0.17][:K]
    cuts = (1, 37, 0, big, 162)
    return io.Shape(name, lambda pkg: pkg.Duc(freqs, I, decimation=D, max_items=1024), [1] * K, sum(cuts), cuts, False, seed)


SHAPES = [_shape("K3_I5", 3, 5, 1, 11), _shape("K1_I1", 1, 1, 1, 12), _shape("K2_I64", 2, 64, 1, 13),
          _shape("K2_25over4", 2, 25, 4, 14), _shape("K2_16over3", 2, 16, 3, 15, big=500)]
CASES = [(s, f, g) for s in SHAPES for f in io.FORMATS for g in io.gains(f)]


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_largest_call_crosses_a_tile_and_ends_inside_one(pkg, shape):
    b = shape.make(pkg)
    tile, spans = b.tile_items, list(shape.spans())
    assert tile >= 1
    made = [shape.call(b, lo, hi, format="sc16").shape[0] for lo, hi in spans]
    assert max(made) > tile and max(made) % tile != 0, (tile, made)


@pytest.mark.parametrize("fmt", io.FORMATS)
def test_the_yardstick_is_the_numpy_statement(pkg, fmt):
    for gain in io.gains(fmt):
        io.check_against_numpy(pkg, SHAPES[0], fmt, gain)


@pytest.mark.parametrize("shape,fmt,gain", CASES, ids=lambda v: str(v))
def test_call_by_call_equals_the_twin_packed(pkg, shape, fmt, gain):
    import torch
    want, count = io.packed(pkg, shape, fmt, gain)
    if gain is not None:  # a case where nothing or everything clamps shows nothing
        assert 0 < count < want.numel() // 2, (count, want.numel())
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    parts = io.fused(pkg, shape, fmt, gain, clipped=c)
    assert [p.shape[0] for p in parts][2] == 0 and parts[0].dtype == io.dtype_of(fmt)
    io.assert_calls_equal(parts, want)
    assert int(c.item()) == count


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("fmt", io.FORMATS)
def test_nan_items_pack_to_the_formats_nan_value(pkg, shape, fmt):
    import torch
    band = host(io.twin(pkg, shape, nan=True))
    hit = np.isnan(band.real) | np.isnan(band.imag)
    assert 0 < hit.sum() < band.size // 2
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
        for (buf, n), p in zip(bufs, parts):  # written where it was told to, and nowhere else
            assert n == 0 or p.data_ptr() == buf.data_ptr() + off * buf.element_size() * 2
            assert bool((buf[:off] == 77).all()) and bool((buf[off + n:] == 77).all())


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=str)
def test_formats_mix_on_one_handle(pkg, shape):
    import torch
    band = io.twin(pkg, shape)
    b = shape.make(pkg)
    at = 0
    for (lo, hi), fmt in zip([(0, 100), (100, 230), (230, 231), (231, 400), (400, shape.units)], [None, "sc16", "cu8", "sc8", None]):
        x = shape.call(b, lo, hi) if fmt is None else shape.call(b, lo, hi, format=fmt)
        n = x.shape[0]
        want = band[at:at + n] if fmt is None else pkg.iq_pack(band[at:at + n], fmt)
        assert torch.equal(x, want), (fmt, lo, hi)
        at += n
    assert at == band.numel()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]], ids=str)
def test_refusals_leave_the_stream_where_it_was(pkg, shape):
    import torch
    want, _ = io.packed(pkg, shape, "sc16", None)
    b = shape.make(pkg)
    first = shape.call(b, 0, 40, format="sc16")
    n_next = shape.samples(b, 40, 200)
    with pytest.raises(pkg.Gr4pmError):
        shape.call(b, 40, 200, format="sc12")
    with pytest.raises(pkg.Gr4pmError):
        shape.call(b, 40, 200, format="sc16", out=torch.empty((n_next - 1, 2), dtype=torch.int16, device="cuda"))
    with pytest.raises(pkg.Gr4pmError):
        shape.call(b, 40, 200, format="sc16", out=torch.empty((n_next, 2), dtype=torch.int8, device="cuda"))
    with pytest.raises(pkg.Gr4pmError):
        shape.call(b, 40, 200, format="sc16", out=torch.empty(n_next, dtype=torch.complex64, device="cuda"))
    # the entry itself: an unknown format and too little room, refused with *n_out = 0 before anything is enqueued
    L, v = pkg.lib(), shape.window(40, 200)
    out = torch.full((n_next, 2), 77, dtype=torch.int16, device="cuda")
    n = C.c_size_t(5)
    assert L.gr4pm_duc_process_iq(b._h, v.data_ptr(), v.stride(0), 160, out.data_ptr(), 9, 0.0, n_next, C.byref(n), None) == -1
    assert n.value == 0 and b"format" in L.gr4pm_last_error()
    n = C.c_size_t(5)
    assert L.gr4pm_duc_process_iq(b._h, v.data_ptr(), v.stride(0), 160, out.data_ptr(), 1, 0.0, n_next - 1, C.byref(n), None) != 0
    assert n.value == 0 and bool((out == 77).all())
    rest = [shape.call(b, 40, 200, format="sc16"), shape.call(b, 200, shape.units, format="sc16")]
    io.assert_calls_equal([first] + rest, want)


@pytest.mark.parametrize("fmt", io.FORMATS)
def test_the_counter_is_added_to_and_may_be_absent(pkg, fmt):
    import torch
    shape, gain = SHAPES[0], io.gains(fmt)[1]
    want, count = io.packed(pkg, shape, fmt, gain)
    io.assert_calls_equal(io.fused(pkg, shape, fmt, gain, clipped=None), want)
    c = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    io.fused(pkg, shape, fmt, gain, clipped=c)
    assert int(c.item()) == 7 + count
