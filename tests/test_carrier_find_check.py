"""The host logic of the Spectrum block as stand-alone programs under UndefinedBehaviorSanitizer and AddressSanitizer:
tests/hostlogic/spectrum_plan_check.cpp sweeps csrc/hostlogic/spectrum_plan.hpp (segments and tail of every call) over
every hop, tests/hostlogic/carrier_find_check.cpp runs csrc/hostlogic/carrier_find.hpp on synthetic spectra with room for
all carriers, for one and for none.  No GPU, no HIP, nothing loaded into python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_check(tmp_path, name):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "needs a host C++ compiler"
    exe = str(tmp_path / (name + ".bin"))
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "gr4-packet-modem_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "hostlogic", name + ".cpp")], check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    return run.stdout


def test_spectrum_plan_sweep_under_sanitizers(tmp_path):
    """every hop in 1 .. 2048, calls of 0, 1, hop - 1, hop, N - 1, N, N + 1 and 3 N + 7 samples in four orders: the
    segments of the calls sum to the closed form, and no segment reads outside the tail plus the input"""
    out = run_check(tmp_path, "spectrum_plan_check")
    m = re.fullmatch(r"spectrum_plan_check: (\d+) calls, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) == 2048 * 4 * 16


def test_carrier_find_under_sanitizers(tmp_path):
    out = run_check(tmp_path, "carrier_find_check")
    m = re.fullmatch(r"carrier_find_check: (\d+) cases, 0 failures\n", out)
    assert m, out[-2000:]
    assert int(m.group(1)) >= 14
