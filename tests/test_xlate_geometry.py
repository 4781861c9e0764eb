"""The tiles of k_ddc, k_ddc_rational, k_duc and k_duc_rational (csrc/hostlogic/xlate_geometry.hpp, the arithmetic the
creates of csrc/ddc.hip and csrc/duc.hip run on the host) as a stand-alone program under UndefinedBehaviorSanitizer and
AddressSanitizer: tests/hostlogic/xlate_geometry_check.cpp sweeps every shape the creates admit and asserts what the
kernels rest on.  No GPU, no HIP."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_geometry_sweep_under_sanitizers(tmp_path):
    """every D in 1 .. 1024 for k_ddc, every I in 1 .. 1024 for k_duc, every coprime pair of the rational kernels (I up
    to 64 with D up to 1024 for the Ddc, I up to 1024 with D up to 64 for the Duc), K in 1 .. 8 and 64, L at 1, I - 1,
    I, I + 1, D, D + 1, 12 max(I, D) and 8192: the LDS of every tile within what its create asks for, the ranges and
    parities of its sizes, and umulhi(j, rcp) == j div n up to the largest index each kernel divides"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "needs a host C++ compiler"
    exe = str(tmp_path / "xlate_geometry_check.bin")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "gr4-packet-modem_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "hostlogic", "xlate_geometry_check.cpp")], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    m = re.fullmatch(r"xlate_geometry_check: (\d+) shapes, (\d+) refused, 0 failures\n", run.stdout)
    assert m, run.stdout[-2000:]
    # 1024 D and 1024 I at up to 8 lengths (9 K for the Duc), and 2 x 9 K x up to 8 lengths for every coprime pair
    assert int(m.group(1)) > 5_000_000
    assert int(m.group(2)) == 0  # no admitted shape of the sweep is refused for want of a tile
