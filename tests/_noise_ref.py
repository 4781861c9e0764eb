"""The reference NoiseSource's stream restated in numpy (short streams): xoroshiro128+ in Python integers,
generate_canonical<float, 24> with an exact integer round-to-nearest of the 64-bit draw, glibc's logf in double
(the table and polynomial of csrc/noise_source.hip), and float32 arithmetic one rounding per operation."""
import os
import subprocess

import numpy as np

M64 = (1 << 64) - 1
_INVC = [float.fromhex(h) for h in (
    "0x1.661ec79f8f3bep+0", "0x1.571ed4aaf883dp+0", "0x1.49539f0f010bp+0", "0x1.3c995b0b80385p+0",
    "0x1.30d190c8864a5p+0", "0x1.25e227b0b8eap+0", "0x1.1bb4a4a1a343fp+0", "0x1.12358f08ae5bap+0",
    "0x1.0953f419900a7p+0", "0x1p+0", "0x1.e608cfd9a47acp-1", "0x1.ca4b31f026aap-1",
    "0x1.b2036576afce6p-1", "0x1.9c2d163a1aa2dp-1", "0x1.886e6037841edp-1", "0x1.767dcf5534862p-1")]
_LOGC = [float.fromhex(h) for h in (
    "-0x1.57bf7808caadep-2", "-0x1.2bef0a7c06ddbp-2", "-0x1.01eae7f513a67p-2", "-0x1.b31d8a68224e9p-3",
    "-0x1.6574f0ac07758p-3", "-0x1.1aa2bc79c81p-3", "-0x1.a4e76ce8c0e5ep-4", "-0x1.1973c5a611cccp-4",
    "-0x1.252f438e10c1ep-5", "0x0p+0", "0x1.aa5aa5df25984p-5", "0x1.c5e53aa362eb4p-4",
    "0x1.526e57720db08p-3", "0x1.bc2860d22477p-3", "0x1.1058bc8a07ee1p-2", "0x1.4043057b6ee09p-2")]
_LN2 = float.fromhex("0x1.62e42fefa39efp-1")
_A = [float.fromhex(h) for h in ("-0x1.00ea348b88334p-2", "0x1.5575b0be00b6ap-2", "-0x1.ffffef20a4123p-2")]
SQRT2_F = np.float32(1.41421356237309504880)


def _fma(a, b, c):
    """a * b + c with one rounding (exact rationals, then to double)"""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def logf(x):
    """glibc logf of one float32 (normal, positive, zero: what the noise types produce)"""
    x = np.float32(x)
    ix = int(x.view(np.uint32))
    if ix == 0x3F800000:
        return np.float32(0.0)
    if ix == 0:
        return np.float32(-np.inf)
    if ix < 0x00800000:
        ix = int((x * np.float32(2.0 ** 23)).view(np.uint32)) - (23 << 23)
    tmp = (ix - 0x3F330000) & 0xFFFFFFFF
    i = (tmp >> 19) & 15
    k = (tmp - (1 << 32) if tmp & 0x80000000 else tmp) >> 23
    iz = (ix - (tmp & 0xFF800000)) & 0xFFFFFFFF
    z = float(np.uint32(iz).view(np.float32))
    r = _fma(z, _INVC[i], -1.0)
    y0 = _LOGC[i] + float(k) * _LN2
    r2 = r * r
    y = _fma(_A[1], r, _A[2])
    y = _fma(_A[0], r2, y)
    y = _fma(y, r2, y0 + r)
    return np.float32(y)


def u64_to_float(u):
    """float(u) rounded to nearest even, as an exact float32"""
    if u == 0:
        return np.float32(0.0)
    sh = u.bit_length() - 24
    if sh > 0:
        q, rem, half = u >> sh, u & ((1 << sh) - 1), 1 << (sh - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
        u = q << sh
    return np.float32(u)


class Rng:
    """random(seed) of random.hpp over xoroshiro128p.h"""

    def __init__(self, seed):
        s0 = (seed + 0x9E3779B97F4A7C15) & M64
        z = s0
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        self.s = [s0, z ^ (z >> 31)]
        a = [0, 0]
        for word in (0xBEAC0467EBA5FACB, 0xD86B048B86AA9922):
            for b in range(64):
                if word >> b & 1:
                    a[0] ^= self.s[0]
                    a[1] ^= self.s[1]
                self.next()
        self.s = a
        self.stored, self.stored_val = False, np.float32(0)

    def next(self):
        s0, s1 = self.s
        r = (s0 + s1) & M64
        s1 ^= s0
        self.s = [(((s0 << 55) | (s0 >> 9)) & M64) ^ s1 ^ ((s1 << 14) & M64), ((s1 << 36) | (s1 >> 28)) & M64]
        return r

    def ran1(self):
        r = u64_to_float(self.next()) * np.float32(2.0 ** -64)
        return np.float32(np.nextafter(np.float32(1), np.float32(0))) if r >= 1 else r

    def gasdev(self):
        if self.stored:
            self.stored = False
            return self.stored_val
        two, one = np.float32(2), np.float32(1)
        while True:
            x = two * self.ran1() - one
            y = two * self.ran1() - one
            s = x * x + y * y
            if not (s >= one or s == 0):
                break
        f = np.sqrt(np.float32(-2) * logf(s) / s, dtype=np.float32)
        self.stored, self.stored_val = True, x * f
        return y * f


def stream(item, typ, seed, amplitude, n):
    """the first n items of NoiseSource<item>(typ, amplitude, seed) after start()"""
    rng = Rng(seed)
    amp = np.float32(amplitude)
    amp_c = amp / SQRT2_F
    two, one, half = np.float32(2), np.float32(1), np.float32(0.5)
    with np.errstate(all="ignore"):
        if item == "c64":
            out = np.empty(n, np.complex64)
            for i in range(n):
                if typ == "uniform":
                    re = amp_c * ((rng.ran1() * two) - one)
                    im = amp_c * ((rng.ran1() * two) - one)
                else:
                    re = amp_c * rng.gasdev()
                    im = amp_c * rng.gasdev()
                out[i] = np.complex64(complex(re, im))
            return out
        out = np.empty(n, np.float32)
        for i in range(n):
            if typ == "uniform":
                v = (rng.ran1() * two) - one
            elif typ == "gaussian":
                v = rng.gasdev()
            elif typ == "laplacian":
                z = rng.ran1()
                v = -logf(two * (one - z)) if z > half else logf(two * z)
            else:
                z = -SQRT2_F * logf(rng.ran1())
                v = np.float32(0) if abs(z) <= np.float32(9) else z
            out[i] = amp * v
        return out


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_stream_tool(out_dir):
    """tests/noise_ref_stream.c: the same restatement in C, for long streams"""
    exe = os.path.join(out_dir, "noise_ref_stream")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", exe,
                           os.path.join(ROOT, "tests", "noise_ref_stream.c"), "-lm"])
    return exe


def long_stream(exe, item, typ, seed, amplitude, n):
    raw = subprocess.check_output([exe, item, typ, str(seed), str(amplitude), str(n)])
    return np.frombuffer(raw, dtype=np.complex64 if item == "c64" else np.float32)
