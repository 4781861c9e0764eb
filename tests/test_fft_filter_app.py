"""apps/packet_receiver_file.py --notch 0.05:0.012 (its function and its command line, in process) on the scene of
tests/test_fft_filter_notch.py as a cu8 and as a cf32 file, in one chunk and in chunks of 65 536: every packet is
delivered, the same packets both ways."""
import importlib.util
import os

import numpy as np
import pytest

import _notch_scene as ns
from _frontend import dev, load_package

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def load_app(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "apps", name + ".py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    return app


@pytest.fixture(scope="module")
def files(pkg, tmp_path_factory):
    """the scene with the receiver's block of silence behind it, as cf32 and as cu8 at nine tenths of full scale"""
    sent, x = ns.scene(pkg)
    x = np.concatenate([x, np.zeros(ns.ZERO_TAIL, np.complex64)])
    d = tmp_path_factory.mktemp("notch")
    paths = {"cf32": str(d / "scene.cf32"), "cu8": str(d / "scene.cu8")}
    x.tofile(paths["cf32"])
    gain = 0.9 * 128.0 / float(np.abs(x.view(np.float32)).max())
    pkg.iq_pack(dev(x), "cu8", gain).cpu().numpy().tofile(paths["cu8"])
    return sent, paths, 1.0 / gain


@pytest.mark.parametrize("fmt", ["cf32", "cu8"])
def test_notch_in_front_of_the_file_receiver(pkg, files, fmt):
    rxa = load_app("packet_receiver_file")
    sent, paths, scale = files
    kw = dict(pkg=pkg, fmt=fmt, scale=None if fmt == "cf32" else scale)
    notch = pkg.band_filter_taps([(ns.CW_FREQUENCY, ns.NOTCH_WIDTH)], "stop", ns.NOTCH_TAPS)
    whole = rxa.receive_file(paths[fmt], chunk_items=1 << 20, notch=notch, **kw)
    assert whole["packets"] == sent
    chunked = rxa.receive_file(paths[fmt], chunk_items=65536, notch=notch, **kw)
    assert chunked["packets"] == sent == whole["packets"]


def test_notch_on_the_command_line(pkg, files, tmp_path, capsys):
    rxa = load_app("packet_receiver_file")
    sent, paths, scale = files
    out = str(tmp_path / "packets.bin")
    rxa.main([paths["cu8"], "--format", "cu8", "--scale", repr(scale), "--notch", f"{ns.CW_FREQUENCY}:{ns.NOTCH_WIDTH}",
              "--chunk-items", "65536", "--out", out])
    assert f"packets {len(sent)} (0 CRC failures)" in capsys.readouterr().out
    data, got, pos = open(out, "rb").read(), [], 0
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 2], "big")
        got.append(data[pos + 2:pos + 2 + n])
        pos += 2 + n
    assert got == sent
    for bad in (["--notch", "0.05"], ["--notch", "0.05:0.012", "--scan"], ["--notch", "0.05:0.012", "--notch-taps", "1024"]):
        with pytest.raises((SystemExit, pkg.Gr4pmError)):
            rxa.main([paths["cu8"], "--format", "cu8", *bad])
