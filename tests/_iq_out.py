"""What the GPU tests of the transmit banks' integer output share (test_duc_iq_out.py, test_fft_duc_iq_out.py; DESIGN.md
section 31): a bank of either kind fed in calls, and the yardstick, which is the code that exists without the feature:
a second handle with the same settings (the twin) run in one shot, its complex64 band packed by pkg.iq_pack().  Every
comparison is torch.equal on integer tensors and == on counters.

A Shape feeds `units` (items per row; slots for the MixedFftDuc) lo .. hi of its seeded rows to a handle and closes the
stream with flush() where the bank has one.  The twin's band and its packed forms are computed once per shape and left
unchanged."""
import functools

import numpy as np

import _iq_ref
from _frontend import dev, host

FORMATS = ("sc16", "sc8", "cu8")
AMPLITUDE = 0.3  # of the rows' complex normal items: at four times the default gain some components clip, fewer than half


def gains(fmt):
    """the default gain, and four times it: the second must clip"""
    return (None, 4.0 * _iq_ref.FORMATS[fmt][2])


def dtype_of(fmt):
    import torch
    return {"sc16": torch.int16, "sc8": torch.int8, "cu8": torch.uint8}[fmt]


class Shape:
    """name: the test id.  make(pkg): a new handle.  per_unit[k]: items of row k in one unit.  units: all of them.
    cuts: the calls, in units.  flush: the bank has flush()"""

    def __init__(self, name, make, per_unit, units, cuts, flush, seed):
        self.name, self.make, self.per_unit, self.units, self.cuts, self.flush = name, make, list(per_unit), units, tuple(cuts), flush
        assert sum(cuts) == units
        rng = np.random.default_rng(seed)
        self.rows = [(AMPLITUDE * np.sqrt(0.5) * (rng.standard_normal(units * p) + 1j * rng.standard_normal(units * p))).astype(np.complex64)
                     for p in self.per_unit]

    def __repr__(self):
        return self.name

    def window(self, lo, hi, rows=None):
        """[K, n_cols] complex64 on the device: row k's items of the units lo .. hi at its front, NaN behind them (must
        not be read)"""
        rows = self.rows if rows is None else rows
        n = [(hi - lo) * p for p in self.per_unit]
        a = np.full((len(rows), max(n)), np.nan + 1j * np.nan, dtype=np.complex64)
        for k, p in enumerate(self.per_unit):
            a[k, :n[k]] = rows[k][lo * p:hi * p]
        return dev(a)

    def call(self, block, lo, hi, rows=None, **kw):
        v = self.window(lo, hi, rows)
        if len(set(self.per_unit)) > 1:
            return block.process_bulk(v, slots=hi - lo, **kw)
        return block.process_bulk(v, **kw)

    def samples(self, block, lo, hi):
        return block.output_items(hi - lo)

    def spans(self):
        at = 0
        for c in self.cuts:
            yield at, at + c
            at += c


@functools.lru_cache(maxsize=None)
def _twin(pkg, shape, nan):
    """the twin's whole band, complex64 on the device: one call and the flush.  nan: one item of row 0 is NaN"""
    import torch
    rows = shape.rows
    if nan:
        rows = [r.copy() for r in rows]
        rows[0][nan_item(shape)] = np.nan
    t = shape.make(pkg)
    parts = [shape.call(t, 0, shape.units, rows)]
    if shape.flush:
        parts.append(t.flush())
    return torch.cat(parts)


def nan_item(shape):
    return (shape.units * shape.per_unit[0]) // 3


def twin(pkg, shape, nan=False):
    return _twin(pkg, shape, nan)


@functools.lru_cache(maxsize=None)
def packed(pkg, shape, fmt, gain, nan=False):
    """(the twin's band packed by pkg.iq_pack, its clipped count): today's two-call form"""
    import torch
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    x = pkg.iq_pack(twin(pkg, shape, nan), fmt, gain, clipped=c)
    return x, int(c.item())


def fused(pkg, shape, fmt, gain, rows=None, clipped=None, outs=None):
    """a new handle fed in the shape's calls with format=fmt, then flushed: the list of the calls' tensors.  outs(n): the
    `out` of a call that makes n items, or None"""
    b = shape.make(pkg)
    parts = []
    for lo, hi in shape.spans():
        kw = dict(format=fmt, gain=gain, clipped=clipped)
        if outs is not None:
            kw["out"] = outs(shape.samples(b, lo, hi))
        parts.append(shape.call(b, lo, hi, rows, **kw))
    if shape.flush:
        parts.append(b.flush(format=fmt, gain=gain, clipped=clipped))
    return parts


def assert_calls_equal(parts, want):
    """the calls' tensors against the consecutive slices of `want`, each of them and the total length"""
    import torch
    at = 0
    for i, p in enumerate(parts):
        n = p.shape[0]
        assert p.dtype == want.dtype and tuple(p.shape[1:]) == tuple(want.shape[1:]), (i, p.dtype, tuple(p.shape))
        assert torch.equal(p, want[at:at + n]), f"call {i}: items {at} .. {at + n} differ"
        at += n
    assert at == want.shape[0], (at, want.shape[0])


def check_against_numpy(pkg, shape, fmt, gain):
    """the yardstick itself, once per format: pkg.iq_pack of the twin's band against tests/_iq_ref.pack on the host"""
    x, count = packed(pkg, shape, fmt, gain)
    want, want_count = _iq_ref.pack(host(twin(pkg, shape)), fmt, gain)
    assert np.array_equal(host(x), want) and count == want_count
