"""The GR4 drop-in of NoiseSource (hip::NoiseSource<T> in gr4-packet-modem_amd/host/gr4pm_gr4_blocks.hpp, reached through
host/gnuradio-4.0/packet-modem/noise_source.hpp): it compiles with g++ 11 and ROCm clang, its settings never touch the
device, the reference's transceiver app instantiates it instead of the reference's CPU block, and on the GPU its
processBulk() in ragged chunks yields the stream of blocks.py's NoiseSource."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

DRIVER_SRC = os.path.join(ROOT, "tests", "gr4_noise_driver.cpp")
DRIVER = os.path.join(ROOT, "tests", "gr4_noise_driver.bin")
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"


def build_driver():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgr4pm_hip.so")):
        ge.build()
    subprocess.check_call(ge.gr4_compile_command(DRIVER_SRC, DRIVER))
    return DRIVER


@pytest.mark.parametrize("cxx", ["g++", CLANGXX])
def test_drop_in_header_compiles_with_gxx_11_and_rocm_clang(cxx):
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-D__HIP_PLATFORM_AMD__", "-fsyntax-only", "-x", "c++",
                           "-I", os.path.join(ROOT, "tests", "gr4_stub"), "-I", os.path.join(ge.PKG_DIR, "host"),
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", DRIVER_SRC])


def test_settings_never_touch_the_device():
    """emplaceBlock() with the reference's property maps and a later settingsChanged() run on a machine without a GPU:
    the handle is made in start() / the first processBulk() only"""
    r = subprocess.run([build_driver(), "settings-only"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "settings ok gaussian 0.1 Laplacian 7" in r.stdout


@pytest.mark.parametrize("source", ["apps/packet_transceiver.cpp", "benchmarks/benchmark_packet_transceiver.cpp"])
def test_reference_transceiver_uses_the_drop_in(source):
    """apps/packet_transceiver.cpp:75-76 emplaces NoiseSource<c64>: compiled against the drop-ins (the recipe of
    test_gr4_blocks.py), the binary holds hip::NoiseSource and calls the C ABI, and the reference's per-sample CPU loop
    is not in it.  benchmarks/benchmark_packet_transceiver.cpp has no noise source; its binary must not gain the
    reference's either."""
    import test_gr4_blocks as tgb
    if not os.path.exists(os.path.join(tgb.REFERENCE_ROOT, source)):
        pytest.skip("the reference tree is not on this machine")
    exe = tgb._flowgraph_binary(source, tgb.CLANGXX)
    syms = subprocess.run(["nm", "-C", exe], capture_output=True, text=True, check=True).stdout
    assert "gr::packet_modem::NoiseSource<" not in syms
    assert "gr::packet_modem::random::" not in syms
    if source.startswith("apps/"):
        assert "gr::packet_modem::hip::NoiseSource<std::complex<float> >" in syms
        assert " U gr4pm_noise_source_create" in syms  # start(); the stand-in runs no processBulk(), so only that is linked


# ---------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def pkg():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return ge.load_package()


@pytest.mark.gpu
@pytest.mark.parametrize("item,typ,seed,amp", [("c64", "gaussian", 0, 0.05), ("c64", "uniform", 1, 1.0),
                                               ("float", "gaussian", 42, 1.0), ("float", "impulse", 5, 0.5),
                                               ("float", "laplacian", 2**64 - 1, 1.0)])
def test_process_bulk_in_ragged_chunks_equals_the_python_block(pkg, tmp_path, item, typ, seed, amp):
    n = 1_500_001
    out = tmp_path / "noise.bin"
    r = subprocess.run([build_driver(), item, typ, str(seed), str(amp), str(n), str(out)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = pkg.NoiseSource(typ, amp, seed, item, max_items=n).process_bulk(n).cpu().numpy()
    assert out.read_bytes() == want.tobytes()


@pytest.mark.gpu
def test_amplitude_setting_mid_stream_keeps_the_position(pkg, tmp_path):
    n, at = 1_500_000, 1_100_000  # past the driver's fixed chunks (they end at 1 052 678): ragged ones around the switch
    out = tmp_path / "noise.bin"
    r = subprocess.run([build_driver(), "c64", "gaussian", "3", "1.0", str(n), str(out), "0.25", str(at)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.frombuffer(out.read_bytes(), dtype=np.complex64)
    a = pkg.NoiseSource("gaussian", 1.0, 3, "c64", max_items=n).process_bulk(n).cpu().numpy()
    b = pkg.NoiseSource("gaussian", 0.25, 3, "c64", max_items=n).process_bulk(n).cpu().numpy()
    # the switch lands on the first chunk boundary at or after `at`: the stream is a's up to there and b's after
    assert (got != a).any()
    k = int(np.argmax(got != a))
    assert at <= k < n and got[:k].tobytes() == a[:k].tobytes() and got[k:].tobytes() == b[k:].tobytes()
