"""The integer IQ formats without a GPU: tests/_iq_ref.py (the numpy statement of include/gr4pm_hip.h's definition)
against the properties the definition promises, the three entry points in the header, the library and the package, and
every argument error of gr4pm_iq_unpack / gr4pm_iq_pack / gr4pm_channelizer_process_iq, which are refused before any
HIP call and so return their status on a machine without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import _iq_ref as iqr

ROOT = ge.ROOT
NEW = ["gr4pm_iq_unpack", "gr4pm_iq_pack", "gr4pm_channelizer_process_iq"]


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgr4pm_hip.so")):
        ge.build()
    return ge.load_package()


def every_value(fmt):
    """[K, 2] integers in which every value of the type occurs as I and as Q"""
    dtype, _, _, lo, hi, _, _ = iqr.FORMATS[fmt]
    v = np.arange(lo, hi + 1, dtype=np.int64)
    return np.stack([v, v[::-1]], axis=1).astype(dtype)


@pytest.mark.parametrize("fmt", list(iqr.FORMATS))
def test_pack_of_unpack_is_the_identity(fmt):
    v = every_value(fmt)
    assert v.shape[0] == (65536 if fmt == "sc16" else 256)
    x = iqr.unpack(v, fmt)
    assert x.dtype == np.complex64 and x.shape == (v.shape[0],)
    back, clipped = iqr.pack(x, fmt)
    assert back.dtype == v.dtype and np.array_equal(back, v) and clipped == 0
    # the default scale is a power of two: unpack is exact
    bias = iqr.FORMATS[fmt][5]
    assert np.array_equal(x.real.astype(np.float64), (v[:, 0].astype(np.float64) - bias) * iqr.FORMATS[fmt][1])


def c64(re, im=0.0):
    re = np.asarray(re, dtype=np.float32)
    x = np.zeros(re.shape, dtype=np.complex64)
    x.real, x.imag = re, np.asarray(im, dtype=np.float32)  # (not re + 1j im: 0 * inf would put NaN into the other part)
    return x


def test_ties_go_to_even():
    k = np.arange(-6, 6)
    for fmt, gain in (("sc16", 2.0 ** 15), ("sc8", 2.0 ** 7)):
        got, clipped = iqr.pack(c64((k + 0.5) / gain), fmt)     # exact in float32: the product is k + 0.5
        assert np.array_equal(got[:, 0], np.where(k % 2 == 0, k, k + 1)) and clipped == 0
        assert np.all(got[:, 1] == 0)
    # cu8: t = x gain + 127.5, so x = k / 128 lands on k + 127.5
    got, clipped = iqr.pack(c64(k / 128.0), "cu8")
    t = k + 127.5
    assert np.array_equal(got[:, 0], np.where(np.floor(t) % 2 == 0, np.floor(t), np.ceil(t))) and clipped == 0
    assert np.all(got[:, 1] == 128)                              # 127.5 itself: the even neighbour


def test_saturation_infinities_nan_and_negative_zero():
    inf, nan = np.inf, np.nan
    # sc16, gain 2^15: 32767.5 is a tie that rounds to 32768 and clips, 32767.49 does not; -32768.5 ties to -32768: no clip
    x = c64([32767.0 / 32768, 32767.5 / 32768, 1.0, -1.0, -32768.5 / 32768, -32769.0 / 32768, inf, -inf, nan, -0.0, 1e-40],
            [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, nan, inf, 0.0, -1e-40])
    got, clipped = iqr.pack(x, "sc16")
    assert got[:, 0].tolist() == [32767, 32767, 32767, -32768, -32768, -32768, 32767, -32768, 0, 0, 0]
    assert got[:, 1].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 32767, 0, 0]
    assert clipped == 2 + 1 + 2 + 2 + 1
    got, clipped = iqr.pack(c64([1.0, 127.4 / 128, -1.0, -128.6 / 128, nan, -0.0, inf]), "sc8")
    assert got[:, 0].tolist() == [127, 127, -128, -128, 0, 0, 127] and clipped == 4
    got, clipped = iqr.pack(c64([127.5 / 128, 127.4 / 128, 1.0, -127.5 / 128, -128.1 / 128, nan, -0.0, -inf]), "cu8")
    assert got[:, 0].tolist() == [255, 255, 255, 0, 0, 128, 128, 0] and clipped == 1 + 1 + 1 + 1
    assert np.all(got[:, 1] == 128)
    # a gain that overflows float32: infinity, clamped and counted
    got, clipped = iqr.pack(c64([3e38, -3e38]), "sc16", gain=1e3)
    assert got[:, 0].tolist() == [32767, -32768] and clipped == 2


def test_symbols_are_declared_exported_and_listed(pkg):
    header = open(os.path.join(ROOT, "include", "gr4pm_hip.h")).read()
    declared = set(re.findall(r"\b(gr4pm_[a-z0-9_]+)\s*\(", header))
    r = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {l.split()[-1] for l in r.stdout.splitlines() if l.strip()}
    for s in NEW:
        assert s in declared and s in exported and s in pkg.EXPORTS and hasattr(pkg.lib(), s), s
    for name, value in (("GR4PM_IQ_SC16", 1), ("GR4PM_IQ_SC8", 2), ("GR4PM_IQ_CU8", 3)):
        assert re.search(rf"\b{name} = {value}\b", header), name
    assert pkg.IQ_FORMATS == {"sc16": 1, "sc8": 2, "cu8": 3}


def test_argument_errors_return_invalid_without_a_device(pkg):
    L = pkg.lib()
    a, b = C.c_void_p(0x1000), C.c_void_p(0x2000)  # never dereferenced: every call below is refused before any HIP call
    INVALID = -1
    for fmt in (1, 2, 3):
        # a null pointer with n > 0
        assert L.gr4pm_iq_unpack(None, 8, fmt, 0.0, 1, 8, b, 8, None) == INVALID
        assert L.gr4pm_iq_unpack(a, 8, fmt, 0.0, 1, 8, None, 8, None) == INVALID
        assert L.gr4pm_iq_pack(None, 8, 1, 8, fmt, 0.0, b, 8, None, None) == INVALID
        assert L.gr4pm_iq_pack(a, 8, 1, 8, fmt, 0.0, None, 8, None, None) == INVALID
        assert b"null" in L.gr4pm_last_error()
        # a stride below n, on either side
        assert L.gr4pm_iq_unpack(a, 7, fmt, 0.0, 3, 8, b, 8, None) == INVALID
        assert L.gr4pm_iq_unpack(a, 8, fmt, 0.0, 3, 8, b, 7, None) == INVALID
        assert L.gr4pm_iq_pack(a, 7, 3, 8, fmt, 0.0, b, 8, None, None) == INVALID
        assert L.gr4pm_iq_pack(a, 8, 3, 8, fmt, 0.0, b, 7, None, None) == INVALID
        assert b"stride" in L.gr4pm_last_error()
        # nothing to do is not an error: no pointer is needed, no device either
        assert L.gr4pm_iq_unpack(None, 0, fmt, 0.0, 1, 0, None, 0, None) == 0
        assert L.gr4pm_iq_pack(None, 0, 0, 8, fmt, 0.0, None, 0, None, None) == 0
    for fmt in (0, 4, -1, 1 << 20):
        assert L.gr4pm_iq_unpack(a, 8, fmt, 0.0, 1, 8, b, 8, None) == INVALID
        assert L.gr4pm_iq_pack(a, 8, 1, 8, fmt, 0.0, b, 8, None, None) == INVALID
        assert L.gr4pm_iq_unpack(None, 0, fmt, 0.0, 1, 0, None, 0, None) == INVALID  # also with nothing to do
        assert b"format" in L.gr4pm_last_error()
        n = C.c_size_t(7)
        assert L.gr4pm_channelizer_process_iq(None, a, fmt, 0.0, 8, b, 8, 8, C.byref(n)) == INVALID
    n = C.c_size_t(7)
    assert L.gr4pm_channelizer_process_iq(None, a, 1, 0.0, 8, b, 8, 8, C.byref(n)) == INVALID  # no handle
