#!/usr/bin/env python3
"""Regenerates tests/golden/noise_source_ref.npz and noise_source_ref_digests.json: the reference NoiseSource's output.

Needs the reference checkout ($REF) and ROCm clang++ ($REFCXX); the defaults are oracle/Makefile's.
make_noise_golden.cpp is compiled with that clang++, -std=c++23, against libstdc++ -- the toolchain oracle/Makefile
compiles the reference with -- and includes the reference's random.hpp from the checkout.  Only data is written: the
first 2048 items of every (item, type, seed, amplitude) case the reference accepts, and the SHA-256 of the first 2^24
items of each as raw little-endian bytes.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# the reference checkout and the compiler of the toolchain convention: the defaults of
# oracle/Makefile's REF and REFCXX, overridable the same way
REF = os.environ.get("REF", "/root/reference")
CXX = os.environ.get("REFCXX", "/opt/rocm/lib/llvm/bin/clang++")

SEEDS = [0, 1, 42, 2**63 + 5, 2**64 - 1]
AMPLITUDES = ["1", "0.05"]
CASES = [("c64", "uniform"), ("c64", "gaussian"), ("float", "uniform"), ("float", "gaussian"),
         ("float", "laplacian"), ("float", "impulse")]
N_ARRAY = 2048
N_DIGEST = 1 << 24


def case_key(item, typ, seed, amp):
    return f"{item}_{typ}_{seed}_{amp}"


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "make_noise_golden")
        subprocess.check_call([CXX, "-O2", "-std=c++23", "-I", os.path.join(REF, "blocks", "include"), "-o", exe,
                               os.path.join(HERE, "make_noise_golden.cpp")])
        arrays, digests = {}, {}
        for item, typ in CASES:
            dt = np.complex64 if item == "c64" else np.float32
            for seed in SEEDS:
                for amp in AMPLITUDES:
                    raw = subprocess.check_output([exe, item, typ, str(seed), amp, str(N_DIGEST)])
                    assert len(raw) == N_DIGEST * np.dtype(dt).itemsize
                    key = case_key(item, typ, seed, amp)
                    digests[key] = hashlib.sha256(raw).hexdigest()
                    arrays[key] = np.frombuffer(raw[: N_ARRAY * np.dtype(dt).itemsize], dtype=dt).copy()
                    print(key, digests[key], flush=True)
    np.savez_compressed(os.path.join(HERE, "noise_source_ref.npz"), **arrays)
    with open(os.path.join(HERE, "noise_source_ref_digests.json"), "w") as f:
        json.dump({"n_items": N_DIGEST, "digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
