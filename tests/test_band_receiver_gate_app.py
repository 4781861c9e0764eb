"""apps/band_receiver_file.py --gate on the GPU: the scene of tests/test_row_stream_carriers.py as an sc16 file.  With the
carriers typed WITHOUT their symbol rates, chunks of 65 536 items and one chunk deliver every packet that was sent; --scan
--gate finds both carriers and delivers every packet too.  The floors are measured by the app over its first chunk.  (The
run without --gate is tests/test_band_receiver_app.py's, unchanged.)"""
import re

import pytest

import test_band_receiver_app as app
import test_row_stream_carriers as band
from _frontend import load_package

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def recording(pkg, tmp_path_factory):
    x, sent = band.build_scene(pkg)
    path = str(tmp_path_factory.mktemp("gate") / "wide.sc16")
    pkg.iq_pack(x, "sc16", gain=8192.0).cpu().numpy().tofile(path)
    return path, sent


def gate_lines(out):
    return re.findall(r"^carrier (\d) frequency \S+ decimation \d+ bursts (\d+) \((\d+) dropped, (\d+) truncated\)", out, flags=re.M)


def test_typed_carriers_without_rates_in_chunks_and_in_one(pkg, recording, tmp_path):
    path, sent = recording
    typed = [f"--carrier={f}:{pkg.fft_ddc_decimation(1.35 / s)}" for f, s in zip(band.CARRIERS, band.PER_SYMBOL)]
    for name, chunk in (("chunks", 65536), ("one", 1 << 22)):
        out = app.run_app(path, str(tmp_path / name), "--gate", "--chunk-items", str(chunk), *typed)
        assert "floors measured over the first chunk" in out
        assert gate_lines(out) == [(str(k), str(band.BURSTS[k]), "0", "0") for k in range(2)], out
        for k in range(2):
            assert app.records(str(tmp_path / f"{name}.{k}.bin")) == sent[k], (name, k)


def test_scan_with_gate_delivers_every_packet(pkg, recording, tmp_path):
    path, sent = recording
    out = app.run_app(path, str(tmp_path / "scan"), "--gate", "--scan")
    assert [k for k, _, _, _ in gate_lines(out)] == ["0", "1"], out
    for k in range(2):
        assert app.records(str(tmp_path / f"scan.{k}.bin")) == sent[k], k


def test_a_carrier_without_its_rate_needs_the_gate(recording, tmp_path):
    import subprocess
    import sys
    path, _ = recording
    r = subprocess.run([sys.executable, app.APP, path, "--format", "sc16", "--carrier=0.17:8"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--gate" in r.stderr
