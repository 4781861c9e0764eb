"""The integer IQ formats of include/gr4pm_hip.h (gr4pm_iq_format) stated in numpy, float32 operation by float32
operation: what gr4pm_iq_unpack / gr4pm_iq_pack and the channelizer's integer ingest must give byte for byte.

An item is (I, Q); integer arrays carry a last dimension of 2, complex arrays are complex64."""
import numpy as np

# name: (dtype, default scale, default gain, lowest, highest, offset, what NaN packs to)
FORMATS = {
    "sc16": (np.int16, 2.0 ** -15, 2.0 ** 15, -32768, 32767, 0.0, 0),
    "sc8": (np.int8, 2.0 ** -7, 2.0 ** 7, -128, 127, 0.0, 0),
    "cu8": (np.uint8, 2.0 ** -7, 2.0 ** 7, 0, 255, 127.5, 128),
}


def unpack(v, fmt, scale=None):
    """[..., 2] integers -> [...] complex64: float(v) * scale, cu8: (float(v) - 127.5) * scale"""
    dtype, dscale, _, _, _, bias, _ = FORMATS[fmt]
    v = np.ascontiguousarray(v)
    assert v.dtype == dtype and v.shape[-1] == 2
    f = v.astype(np.float32)
    if bias:
        f = f - np.float32(bias)
    f = f * np.float32(dscale if scale is None else scale)
    assert f.dtype == np.float32
    return np.ascontiguousarray(f).view(np.complex64)[..., 0]


def pack(x, fmt, gain=None):
    """[...] complex64 -> ([..., 2] integers, clipped components): t = x * gain (cu8: t = t + 127.5), rint (ties to
    even), clamp; NaN: 0 (cu8: 128); clamped and NaN components count as clipped"""
    dtype, _, dgain, lo, hi, bias, nan_value = FORMATS[fmt]
    x = np.ascontiguousarray(x, dtype=np.complex64)
    c = x.view(np.float32).reshape(x.shape + (2,))
    with np.errstate(all="ignore"):
        t = c * np.float32(dgain if gain is None else gain)
        if bias:
            t = t + np.float32(bias)
        assert t.dtype == np.float32
        r = np.rint(t)
        nan = np.isnan(t)
        clipped = nan | (r < lo) | (r > hi)
        r = np.clip(r, lo, hi)
        r[nan] = nan_value
    return r.astype(dtype), int(np.count_nonzero(clipped))
