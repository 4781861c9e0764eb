"""The Channelizer without a GPU: its float64 definition and polyphase form agree; the tap design (host-only entry point)
against numpy; tones land in the right row with the right sense of rotation; the stimulus of the GPU end-to-end test is
one the oracle's detector decodes; the ABI's error paths."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import _channelizer_ref as cref
import _oracle as orc
import _signals as sig


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgr4pm_hip.so")):
        ge.build()
    return ge.load_package()


@pytest.mark.parametrize("M", [2, 8, 64])
@pytest.mark.parametrize("P", [1, 3, 12])
def test_polyphase_form_equals_the_definition(M, P):
    """mix / convolve / decimate == branch sums + forward FFT to 1e-12 of sum|h| max|x|, lengths not multiples of M:
    pins the DFT's sign, the branch order and the M - 1 offset"""
    rng = np.random.default_rng(100 * M + P)
    h = rng.standard_normal(P * M)
    for n in (5 * M + 1, 17 * M + M - 1, 40 * M + M // 2):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        a, b = cref.analysis64(x, h, M), cref.analysis64_polyphase(x, h, M)
        assert a.shape == b.shape == (M, n // M)
        assert np.max(np.abs(a - b)) <= 1e-12 * np.sum(np.abs(h)) * np.max(np.abs(x))
    # not vacuous: the reversed branch order or the other sign is wrong by order 1
    if M > 2:
        for wrong in (cref.analysis64_polyphase(x, h[::-1], M), np.conj(cref.analysis64_polyphase(np.conj(x), h, M))):
            assert np.max(np.abs(a - wrong)) > 1e-3 * np.sum(np.abs(h))


@pytest.mark.parametrize("M,P", [(2, 1), (8, 32), (16, 12), (64, 12), (256, 8), (1024, 3), (64, 5)])
def test_taps_match_the_numpy_design(pkg, M, P):
    """every tap within one float32 ulp of the largest tap of the same formula in numpy (np.kaiser, np.sinc) in double;
    DC gain 1 within 2^-22"""
    h = pkg.channelizer_taps(M, P)
    ref = cref.kaiser_taps64(M, P)
    assert h.dtype == np.float32 and h.size == P * M
    ulp = np.spacing(np.float32(np.max(np.abs(ref))))
    assert np.max(np.abs(h.astype(np.float64) - ref)) <= ulp
    assert abs(np.sum(h.astype(np.float64)) - 1.0) <= 2.0 ** -22
    assert np.array_equal(h, h[::-1]) or np.max(np.abs(h - h[::-1])) <= ulp  # linear phase


@pytest.mark.parametrize("M", [16, 64, 256])
def test_default_design_meets_its_stopband(pkg, M):
    """the default P = 12 design, from the float32 taps by a 64 L point float64 FFT: passband ripple and stopband
    attenuation recorded; the stopband held to the 80 dB Kaiser's length rule was entered with, less 3 dB for the rule
    being approximate"""
    h = pkg.channelizer_taps(M)
    f, db = cref.response_db(h, M)
    ripple = np.max(np.abs(db[f <= 0.25]))
    stop = np.max(db[f >= 0.75])
    print(f"\n[channelizer taps] M = {M}, P = 12: passband ripple {ripple:.2e} dB, stopband {stop:.1f} dB")
    assert stop <= -(80.0 - 3.0)
    assert ripple < 0.01  # the passband of a 90 dB Kaiser design is flat to its stopband's level


def test_tones_land_in_their_row_and_rotate_the_right_way(pkg):
    """a tone at channel k's centre: row k at amplitude 1, every other row >= 77 dB down once the filter has filled;
    a tone 0.1 spacings above the centre rotates by +0.1 cycles per output item"""
    M, P = 16, 12
    h = pkg.channelizer_taps(M, P)
    i = np.arange(60 * M)
    for k in (0, 1, 5, 8, 15):
        y = cref.analysis64(np.exp(2j * np.pi * k * i / M), h, M)[:, P:]
        assert np.max(np.abs(np.abs(y[k]) - 1.0)) < 1e-6
        others = np.delete(np.abs(y), k, axis=0)
        assert 20 * np.log10(np.max(others)) <= -77.0, k
        y = cref.analysis64(np.exp(2j * np.pi * (k + 0.1) * i / M), h, M)[k, P:]
        step = np.angle(y[1:] * np.conj(y[:-1])) / (2 * np.pi)
        assert np.max(np.abs(step - 0.1)) < 1e-6, k
        assert abs(np.mean(np.abs(y)) - 1.0) < 1e-3  # 0.1 of the spacing is inside the passband


def wideband_stimulus(M, occupied, n_symbols, locations, sigma=0.05, seed=7):
    """a qa syncword stream (its own small frequency error) in each occupied channel, synthesised to one wideband
    float64 stream, plus noise of `sigma` on the wideband stream.  Returns (x, per-channel locations)."""
    rows = {}
    for j, k in enumerate(occupied):
        locs = [loc + 37 * j for loc in locations]
        rows[k], _ = sig.qa_syncword_stream(n_symbols, locs, 0.004 * (j - len(occupied) // 2), seed=seed + j)
    n_items = min(v.size for v in rows.values())
    h = cref.kaiser_taps64(M)
    x = cref.synthesis64(rows, h, M, n_items)
    return x + sig.awgn(x.size, sigma, seed + 100).astype(np.complex128), len(locations)


def test_end_to_end_stimulus_is_one_the_oracle_decodes(pkg):
    """the stimulus of the GPU end-to-end test at small size: 5 of 16 channels occupied, neighbours (0, 1, 15 and 7, 8)
    included, noise at sigma 0.05 on the wideband stream; through analysis64 with the default taps, rounded to
    complex64, each row through the oracle's SyncwordDetection: as many tags as syncwords in every occupied channel,
    none in an empty one.  power_threshold is the 20.0 tests/test_syncword_float64.py runs this noise level with: the
    median test is scale-invariant, so on a row of noise alone the receiver's default of 9.5 fires about once in 10^5
    items whatever the level (row 4 of this stimulus, item 1559) -- a property of the detector, not of the bank"""
    M = 16
    occupied = [0, 1, 15, 7, 8]
    x, n_sync = wideband_stimulus(M, occupied, 6000, [300, 1500, 2600, 4100, 4900])
    h = pkg.channelizer_taps(M)
    y = cref.analysis64(x, h, M).astype(np.complex64)
    rrc, _ = orc.unit_norm_rrc(4)
    for k in range(M):
        det = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0)
        _, _, tags = det.process(y[k])
        assert tags.size == (n_sync if k in occupied else 0), (k, tags["index"])


def test_abi_error_paths_without_a_device(pkg):
    """gr4pm_channelizer_taps refuses M not a power of two, P out of range, passband >= stopband; create refuses a
    duplicate or out-of-range select and, with valid settings, returns GR4PM_ERR_NO_DEVICE where there is no GPU"""
    L = pkg.lib()
    out = np.zeros(1024 * 32, np.float32)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert L.gr4pm_channelizer_taps(64, 12, 0.25, 0.75, ptr) == 0
    for M, P, pb, sb in [(48, 12, 0.25, 0.75), (1, 12, 0.25, 0.75), (2048, 12, 0.25, 0.75), (0, 12, 0.25, 0.75),
                         (64, 0, 0.25, 0.75), (64, 33, 0.25, 0.75), (64, 12, 0.75, 0.75), (64, 12, 0.8, 0.3),
                         (64, 12, float("nan"), 0.75), (64, 12, -0.1, 0.75)]:
        assert L.gr4pm_channelizer_taps(M, P, pb, sb, ptr) == -1, (M, P, pb, sb)
        assert b"channelizer" in L.gr4pm_last_error()
    assert L.gr4pm_channelizer_taps(64, 12, 0.25, 0.75, None) == -1
    with pytest.raises(pkg.Gr4pmError):
        pkg.channelizer_taps(48)

    from gr4_packet_modem_amd import _abi
    h = C.c_void_p()

    def create(M, P, select=(), max_frames=1 << 20):
        sel = np.asarray(select, dtype=np.uint32)
        p = _abi.ChannelizerParams(M, P, None, sel.size, sel.ctypes.data_as(C.c_void_p) if sel.size else None,
                                   max_frames, None)
        return L.gr4pm_channelizer_create(C.byref(p), C.byref(h))

    assert create(48, 12) == -1 and create(64, 0) == -1 and create(64, 33) == -1 and create(64, 12, max_frames=0) == -1
    assert create(64, 12, [1, 2, 1]) == -1 and b"duplicate" in L.gr4pm_last_error()
    assert create(64, 12, [1, 64]) == -1 and b"not a channel" in L.gr4pm_last_error()
    assert L.gr4pm_channelizer_create(None, C.byref(h)) == -1
    st = create(64, 12, [3, 1])
    if L.gr4pm_device_count() <= 0:
        assert st == -6 and not h.value  # GR4PM_ERR_NO_DEVICE
    else:
        assert st == 0 and h.value
        L.gr4pm_channelizer_destroy(h)
    n = C.c_size_t(0)
    assert L.gr4pm_channelizer_output_items(None, 5, C.byref(n)) == -1
    assert L.gr4pm_channelizer_process(None, None, 0, None, 0, 0, C.byref(n)) == -1
    assert L.gr4pm_channelizer_reset(None) == -1
    L.gr4pm_channelizer_destroy(None)
