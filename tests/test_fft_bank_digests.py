"""The raw output bytes of the four FFT bank blocks (FftDdc, MixedFftDdc, FftDuc, MixedFftDuc) against recorded SHA-256
digests (tests/golden/fft_bank_digests.json, written by tests/golden/make_fft_bank_digests.py on an MI355X from the
commit before the uniform handles became fronts of the mixed ones).

The tests that compare a mixed handle at equal rates with the uniform block compare two fronts of one implementation;
the float64 bounds of test_fft_ddc.py and test_fft_duc.py hold the values, and these digests hold the bits.

Inputs: the one_call() of test_fft_ddc.py and test_fft_duc.py at every DEVICE_CASES shape (five hops and a remainder:
B = 512 and B = 32, K = 1 and K = 64, R = 1 and R = rate), the one_call() of test_fft_ddc_mixed.py and
test_fft_duc_mixed.py at theirs, and one FftDdc shape once more fed as sc16 (the same stream, rounded to 2^-13)."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import test_fft_ddc as ddc
import test_fft_ddc_mixed as ddc_mixed
import test_fft_duc as duc
import test_fft_duc_mixed as duc_mixed
from _frontend import load_package

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fft_bank_digests.json")
SC16_CASE = ddc.CASES[1]
SC16_SCALE = 2.0 ** -13


def sc16_stream(D, V, R, K):
    """test_fft_ddc.py's stream of the case as [n, 2] int16 at SC16_SCALE (|components| stay below 4)"""
    x = ddc.setting(D, V, R, K)[0]
    q = np.rint(np.ascontiguousarray(x).view(np.float32).reshape(-1, 2).astype(np.float64) / SC16_SCALE)
    assert np.max(np.abs(q)) < 32768
    return q.astype(np.int16)


def fft_ddc_sc16():
    return ddc.run(ddc.make(load_package(), *SC16_CASE), sc16_stream(*SC16_CASE), scale=SC16_SCALE)


def name(prefix, *parts):
    return prefix + "_" + "_".join("-".join(str(v) for v in p) if isinstance(p, tuple) else str(p) for p in parts)


# key -> a function that returns the block's output: an array, or a list of rows whose bytes follow one another
OUTPUTS = {}
for c in ddc.CASES:
    OUTPUTS[name("fft_ddc", *c)] = functools.partial(ddc.one_call, *c)
OUTPUTS[name("fft_ddc_sc16", *SC16_CASE)] = fft_ddc_sc16
for c in duc.CASES:
    OUTPUTS[name("fft_duc", *c)] = functools.partial(duc.one_call, *c)
for i, case_id in zip(ddc_mixed.CASES, ddc_mixed.cpu.CASE_IDS):
    OUTPUTS["fft_ddc_mixed_" + case_id] = functools.partial(ddc_mixed.one_call, i)
for c, case_id in zip(duc_mixed.CASES, ddc_mixed.cpu.CASE_IDS):
    OUTPUTS["fft_duc_mixed_" + case_id.replace("D", "I")] = functools.partial(duc_mixed.one_call, *c)


def digest(key):
    out = OUTPUTS[key]()
    h = hashlib.sha256()
    for a in out if isinstance(out, list) else [out]:
        assert a.dtype == np.complex64
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(OUTPUTS))
def test_output_bytes_have_the_recorded_digest(key):
    with open(GOLDEN) as f:
        recorded = json.load(f)["digests"]
    assert sorted(recorded) == sorted(OUTPUTS)
    assert digest(key) == recorded[key]
