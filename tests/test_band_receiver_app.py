"""apps/band_receiver_file.py on the GPU: the scene of tests/test_row_stream_carriers.py (two carriers of 20 and 25 wideband
samples per symbol) as an sc16 file.  With the carriers typed, chunks of 65 536 items deliver the packets one chunk
delivers, and both are what was sent; --scan finds both carriers, measures their offsets and rates (printed, asserted only
through the packets) and delivers every packet."""
import os
import re
import subprocess
import sys

import pytest

import test_row_stream_carriers as band
from _frontend import load_package

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "apps", "band_receiver_file.py")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def recording(pkg, tmp_path_factory):
    x, sent = band.build_scene(pkg)
    path = str(tmp_path_factory.mktemp("band") / "wide.sc16")
    pkg.iq_pack(x, "sc16", gain=8192.0).cpu().numpy().tofile(path)
    assert os.path.getsize(path) == 4 * band.WIDE
    return path, sent


def records(path):
    """the packets of a file of uint16 big-endian length + bytes records"""
    data, out, pos = open(path, "rb").read(), [], 0
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 2], "big")
        out.append(data[pos + 2:pos + 2 + n])
        pos += 2 + n
    assert pos == len(data)
    return out


def run_app(path, prefix, *args):
    r = subprocess.run([sys.executable, APP, path, "4", "20.0", "--format", "sc16", "--out-prefix", prefix, *args],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    return r.stdout


def test_typed_carriers_in_chunks_and_in_one(pkg, recording, tmp_path):
    path, sent = recording
    typed = []
    for f, s in zip(band.CARRIERS, band.PER_SYMBOL):
        typed += [f"--carrier={f}:{pkg.fft_ddc_decimation(1.35 / s)}:{1.0 / s!r}"]  # (= for a frequency below zero)
    for name, chunk in (("chunks", 65536), ("one", 1 << 22)):
        out = run_app(path, str(tmp_path / name), "--chunk-items", str(chunk), *typed)
        assert len(re.findall(r"^carrier \d frequency ", out, flags=re.M)) == 2
        for k in range(2):
            assert records(str(tmp_path / f"{name}.{k}.bin")) == sent[k], (name, k)


def test_scan_finds_both_carriers_and_delivers_every_packet(pkg, recording, tmp_path):
    path, sent = recording
    out = run_app(path, str(tmp_path / "scan"), "--scan")
    lines = re.findall(r"^carrier (\d) frequency (\S+) decimation (\d+) symbols_per_sample (\S+):", out, flags=re.M)
    assert len(lines) == 2, out
    for k, f, d, rate in lines:  # find_carriers orders by frequency, as CARRIERS is
        assert records(str(tmp_path / f"scan.{k}.bin")) == sent[int(k)], (k, f, d, rate)
