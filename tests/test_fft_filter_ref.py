"""The FftFilter's references against each other, without a GPU: the complex128 definition (tests/_fft_filter_ref.py) is the
causal convolution, and its float32 restatement stays inside the bound the device is held to."""
import os
import re
import subprocess

import numpy as np
import pytest

import _fft_filter_ref as ref

N = ref.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_signal(L, V):
    hop = N - V
    return ref.stimulus(5 * hop + 77, 100 + L), ref.random_taps(L, 200 + L)


@pytest.mark.parametrize("L,V", ref.CASES)
def test_definition_is_the_causal_convolution(L, V):
    """fft_filter64 equals np.convolve to 1e-12 relative, at every device case"""
    x, h = case_signal(L, V)
    want = np.convolve(x.astype(np.complex128), h.astype(np.complex128))
    got = ref.fft_filter64(x, h, V)
    assert got.size == (x.size // (N - V)) * (N - V)
    assert np.abs(got - want[:got.size]).max() <= 1e-12 * np.abs(want).max()
    # with the zeros that complete the last segment: every sample of the stream
    full = ref.fft_filter64(ref.flushed(x, V), h, V)[:x.size]
    assert np.abs(full - want[:x.size]).max() <= 1e-12 * np.abs(want).max()


def test_default_overlap():
    assert [ref.default_overlap(L) for L in (1, 2, 257, 258, 1025, 1793, 1794, 1985)] == [0, 256, 256, 512, 1024, 1792, 1984, 1984]


@pytest.mark.parametrize("L,V", ref.CASES)
def test_float32_restatement_is_inside_the_bound(L, V):
    """fft_filter32 (radix-2 in complex64, the rounded table) against fft_filter64: inside device_bound everywhere.  Worst
    error / bound per case: (1, 0) 0.0010, (2, 1) 0.0008, (64, 63) 0.0009, (200, 256) 0.0007, (1025, 1024) 0.0007,
    (1985, 1984) 0.0005."""
    x, h = case_signal(L, V)
    want = ref.fft_filter64(x, h, V)
    got = ref.fft_filter32(x, h, V)
    bound = ref.device_bound(x, h, V)
    ratio = (np.abs(got - want) / bound).max()
    print(f"fft_filter32 ({L}, {V}): worst error / bound {ratio:.4f}")
    assert np.isfinite(got).all()
    assert ratio <= 1.0
    assert ratio > 1e-5  # the bound is of the error's kind, not vacuous


def test_kernel_segment_host_emulation(tmp_path):
    """tests/fft_filter_emu.cpp: one segment of k_fft_filter with the 64 lanes run phase by phase on the CPU (the forward
    transform, conj(X) W with the table in the kernel's layout, the transform again, the swap back) against the direct
    convolution in double at the kept samples: float32 rounding, a few 1e-7 of the largest output"""
    exe = tmp_path / "fft_filter_emu"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "gr4-packet-modem_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "fft_filter_emu.cpp")])
    out = subprocess.check_output([str(exe)]).decode()
    errs = [float(e) for e in re.findall(r"max_rel_err ([0-9.e+-]+)", out)]
    assert len(errs) == 1 and errs[0] < 1e-6, out
