"""A CW interferer inside the channel, removed by an FftFilter in front of the receiver: six bursts of
the PacketTransmitter (64 seeded bytes each, gaps of 4000, 4 samples per symbol), noise of sigma 0.05 and
a exp(2 pi j 0.05 n); notch_taps of one band (0.05, width 0.012), 1025 taps, 60 dB; the stream through the filter in calls
of 4097 samples, then into NativePacketReceiver(decode_headers=True, packets_only=True) with a zero tail."""
import numpy as np
import pytest

import _notch_scene as ns
from _frontend import dev, load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def test_notch_restores_the_packets(pkg):
    """a = _notch_scene.CW_AMPLITUDE, the smallest of 2, 5, 10, 30 at which the receiver without the filter delivers fewer
    than six packets on the MI355X: a = 2 (0 of 6 without the filter at 2, 5, 10 and 30 alike; 6 of 6 with it; the notch
    band's power 64.5 dB down at each).  With
    the filter all six payloads come back byte for byte, without it fewer than six, and the filtered stream's power in the
    notch band lies at least 50 dB below the unfiltered stream's."""
    sent, x = ns.scene(pkg)
    taps = ns.notch(pkg)
    assert taps.size == ns.NOTCH_TAPS
    y = ns.filtered(pkg, x, taps)
    assert y.numel() == x.size
    assert ns.receive(pkg, y) == sent
    plain = ns.receive(pkg, dev(x))
    print(f"a = {ns.CW_AMPLITUDE}: {len(plain)} packets without the filter")
    assert len(plain) < 6
    before, after = ns.notch_band_power(pkg, dev(x)), ns.notch_band_power(pkg, y)
    print(f"notch band power: {10 * np.log10(after / before):.1f} dB")
    assert after <= before * 10.0 ** (-50.0 / 10.0)
