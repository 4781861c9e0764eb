"""The raw output bytes of the RowResampler and the StreamRowResampler against recorded SHA-256 digests
(tests/golden/row_resampler_digests.json, written by tests/golden/make_row_resampler_digests.py on an MI355X from the
commit the file names: the last one at which k_row_resample and k_row_stream were two kernels written out twice).

The tests that compare the stream block with the one-shot block compare two fronts of one kernel body; the float64
bound of test_row_resampler.py holds the values, and these digests hold the bits.

Inputs are the existing tests' own.  One-shot: for every (Q, P) of test_row_resampler.SIZES and every step of its STEPS
the whole [21, 6144] array of the float64 comparison's call (lengths 0, 1, P - 1, P, 255, 257, 5000 at three phase0, the
four frequency words, the +0 padding), and the 70-row call (64 + 6) at (32, 12).  Stream: for every (Q, P) of
test_row_stream.SIZES and each of phases_of(P) the per-row concatenation of feed() (six rows, 47 ragged calls and the
flush), the case that starts beyond 2^33, and the three calls around a set_row."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import test_row_resampler as one_shot
import test_row_stream as stream

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_resampler_digests.json")

# key -> a function that returns the block's output: an array, or a list of rows whose bytes follow one another
OUTPUTS = {}
for Q, P in one_shot.SIZES:
    for k, step in enumerate(one_shot.STEPS):
        OUTPUTS[f"one_shot_{Q}-{P}_step{step}"] = functools.partial(one_shot.bound_output, Q, P, k)
OUTPUTS["one_shot_70_rows"] = one_shot.seventy_rows_output
for Q, P in stream.SIZES:
    for k, phase in enumerate(stream.phases_of(P)):
        OUTPUTS[f"stream_{Q}-{P}_phase{phase}"] = functools.partial(stream.cutting_output, Q, P, k)
OUTPUTS["stream_start_index"] = stream.far_output
OUTPUTS["stream_set_row"] = stream.set_row_output


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
