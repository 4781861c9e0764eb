"""A statement of the StreamRowResampler's definition (include/gr4pm_hip.h), for the tests.

A row is an unbounded sequence x[a], +0 in front of `start`; output item m sits at pos_m = phase0 + m step, a Python integer
with 32 fractional bits that is never reduced.  Its value is the RowResampler's (tests/_row_resampler_ref.py) with
    theta(pos) = Phi + floor(freq (pos - ref) / 2^32) mod 2^32,   Phi = 0 and ref = 0 at create
and set_row(step, freq) at the next item m*, position p*: pos_m = p* + (m - m*) step, Phi <- theta_old(p*), ref <- p*.
Row keeps the state the definition names -- A, the next item and its position, Phi, ref, the last P - 1 items -- and makes
the items of a call from the history and the new items.  The filter is _row_resampler_ref's resample32 / resample64 on
that stretch (freq = 0: its rotator is then the identity, which changes no value), so the tables, the branch, alpha, the
windows and the operation order are that file's code; the rotator is applied here with that file's _fma32 in its order."""
import numpy as np

import _row_resampler_ref as ref

TWO32 = ref.TWO32


def rotate32(acc, th):
    """exp(-2 pi j th / 2^32) acc in float32: double sincospi of -th / 2^31 rounded to float32, four fmaf from zero"""
    th = np.asarray(th, dtype=np.float64)
    ang = -th / 2147483648.0
    cs, sn = np.cos(np.pi * ang).astype(np.float32), np.sin(np.pi * ang).astype(np.float32)
    re, im = acc.real.astype(np.float32), acc.imag.astype(np.float32)
    zero = np.zeros(re.size, np.float32)
    yr = ref._fma32(-sn, im, ref._fma32(cs, re, zero))
    yi = ref._fma32(sn, re, ref._fma32(cs, im, zero))
    return (yr.astype(np.float64) + 1j * yi.astype(np.float64)).astype(np.complex64)


def rotate64(acc, th):
    return acc * np.exp(-2j * np.pi * (np.asarray(th, dtype=np.float64) / 4294967296.0))


class Row:
    """one row of a handle; bits=32: complex64 in the definition's operation order, bits=64: complex128"""

    def __init__(self, h, Q, step, phase0=0, freq=0, start=0, bits=32):
        self.h, self.Q = np.asarray(h, dtype=np.float32).reshape(-1), int(Q)
        self.P = self.h.size // self.Q
        self.step, self.phase0, self.freq, self.start, self.bits = int(step), int(phase0), int(freq), int(start), bits
        self.dtype = np.complex64 if bits == 32 else np.complex128
        self.create()

    def create(self):
        """the created state, with the current step and freq"""
        self.A, self.phi, self.ref = self.start, 0, 0
        self.hist = np.zeros(self.P - 1, self.dtype)
        edge = self.start << 32
        self.next_m = 0 if self.phase0 >= edge else -((self.phase0 - edge) // self.step)  # ceil((edge - phase0) / step)
        self.next_pos = self.phase0 + self.next_m * self.step
        self.positions, self.thetas = [], []  # of every item made since create

    def theta(self, pos):
        return (self.phi + ((self.freq * (int(pos) - self.ref)) >> 32)) % TWO32

    def count(self, span):
        """the items not yet made with floor(pos) <= A + span - 1"""
        end = (self.A + int(span)) << 32
        return 0 if self.next_pos >= end else (end - 1 - self.next_pos) // self.step + 1

    def _make(self, new, span):
        P = self.P
        new = np.asarray(new).astype(self.dtype)
        M = self.count(span)
        stretch = np.concatenate([self.hist, new, np.zeros(span - new.size, self.dtype)])  # items A - (P - 1) ..
        local = self.next_pos - ((self.A - (P - 1)) << 32)
        one_shot = ref.resample32 if self.bits == 32 else ref.resample64
        acc = one_shot(stretch, stretch.size, self.h, self.Q, self.step, local, 0, n_cols=M)
        assert acc.size == M
        pos = [self.next_pos + k * self.step for k in range(M)]
        th = [self.theta(p) for p in pos]
        self.positions += pos
        self.thetas += th
        self.next_m += M
        self.next_pos += M * self.step
        if M == 0:
            return np.zeros(0, self.dtype)
        return rotate32(acc, th) if self.bits == 32 else rotate64(acc, th)

    def process(self, new):
        """the next len(new) items of the row"""
        new = np.asarray(new)
        y = self._make(new, new.size)
        self.hist = np.concatenate([self.hist, new.astype(self.dtype)])[new.size:]
        self.A += new.size
        return y

    def flush(self):
        y = self._make(np.zeros(0, self.dtype), self.P - 1)
        self.create()
        return y

    def set_row(self, step, freq):
        self.phi, self.ref = self.theta(self.next_pos), self.next_pos
        self.step, self.freq = int(step), int(freq)


def cutting(P, n, shift=0):
    """the cutting of the tests: forty calls of 1 item, then P - 2, P - 1, P, 0, 255, 257, then the rest; rotated by
    `shift` calls so that the rows of one handle are cut differently"""
    cut = [1] * 40 + [max(P - 2, 0), P - 1, P, 0, 255, 257]
    assert sum(cut) <= n
    cut.append(n - sum(cut))
    shift %= len(cut)
    return cut[shift:] + cut[:shift]
