"""Seeded stimulus generators shared by the oracle tests and the GPU parity tests.

They rebuild, with numpy RNG seeds, the stimuli of the reference's own tests
(test/qa_*.cpp) -- the reference seeds from std::random_device, so the *procedure* is
reproduced, not the bits."""
import numpy as np

import _oracle as orc

# CCSDS 64-bit syncword, packet_receiver.hpp:45-59 / qa_syncword_detection.cpp:35-49
SYNCWORD = np.array(
    [0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1, 1,
     0, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 0],
    dtype=np.uint8,
)
BPSK = np.array([1.0 + 0j, -1.0 + 0j], dtype=np.complex64)
QA_SYNCWORD_LOCATIONS = [100, 1000, 1250, 10000, 13721, 43124, 58000, 127018, 525178, 893251]


def qa_syncword_stream(num_symbols, locations, freq_error, seed=1234, sps=4):
    """qa_syncword_detection.cpp:21-90: random BPSK symbols with the syncword inserted at
    `locations`, unit-norm 45-tap RRC interpolation by sps, rotator at freq_error."""
    rng = np.random.default_rng(seed)
    symbols = rng.integers(0, 2, size=num_symbols, dtype=np.uint8)
    for loc in locations:
        symbols[loc:loc + SYNCWORD.size] = SYNCWORD
    rrc, _ = orc.unit_norm_rrc(sps)
    x = orc.interpolating_fir(BPSK[symbols], sps, rrc)
    x = orc.rotator(x, np.float32(freq_error))
    return x, rrc


def awgn(n, sigma, seed):
    rng = np.random.default_rng(seed)
    return (sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)).astype(np.complex64)


def packet_segments(segments, sps=4, rrc=None, seed=0):
    """QA segments one after the other, each with a packet of its own.  A segment is a dict: n_sym (random BPSK symbols
    through the RRC interpolator, filter state zero at its start), loc (symbol index of the syncword, None: no packet),
    cfo (radians per sample), phase (carrier phase AT the packet's first sample), amp, sigma (AWGN per complex sample,
    added after the scaling), lead (noise-only samples in front), tone = (amplitude, radians per sample) added over the
    whole segment.  Everything after the float32 interpolator is computed in double and rounded once.
    Returns (x complex64, [stream position of each packet's first template sample, None without packet])."""
    if rrc is None:
        rrc, _ = orc.unit_norm_rrc(sps)
    rng = np.random.default_rng(seed)
    parts, positions, at = [], [], 0
    for i, s in enumerate(segments):
        symbols = rng.integers(0, 2, size=s["n_sym"], dtype=np.uint8)
        loc = s.get("loc")
        if loc is not None:
            symbols[loc:loc + SYNCWORD.size] = SYNCWORD
        y = orc.interpolating_fir(BPSK[symbols], sps, rrc).astype(np.complex128)
        n = np.arange(y.size, dtype=np.float64) - (loc * sps if loc is not None else 0)
        y = y * (s.get("amp", 1.0) * np.exp(1j * (s.get("phase", 0.0) + s.get("cfo", 0.0) * n)))
        if "tone" in s:
            y = y + s["tone"][0] * np.exp(1j * s["tone"][1] * n)
        lead = int(s.get("lead", 0))
        y = np.concatenate([np.zeros(lead, np.complex128), y])
        sigma = s.get("sigma", 0.0)
        if sigma:
            y = y + awgn(y.size, sigma, seed * 1000 + 17 + i).astype(np.complex128)
        positions.append(at + lead + loc * sps if loc is not None else None)
        parts.append(y)
        at += y.size
    return np.concatenate(parts).astype(np.complex64), positions
