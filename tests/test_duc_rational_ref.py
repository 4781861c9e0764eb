"""The rational Duc's float64 references (tests/_duc_rational_ref.py) against each other, on the CPU: the definition
(zero-stuff, filter, keep every D-th, mix, sum), the form the kernel implements and plain zero-stuff / np.convolve /
[::D], large start indices against a direct evaluation with Python integers, D = 1 against the integer Duc's
reference, the sample count under random call cuts, the float64 loopback through the rational Ddc's reference, the
host-only tap design, and the HIP-free position arithmetic (csrc/hostlogic/resample_position.hpp) as a stand-alone program
under UndefinedBehaviorSanitizer and AddressSanitizer against Python integers."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import _ddc_rational_ref as dref_r
import _ddc_ref as dref
import _duc_rational_ref as rref
import _duc_ref as uref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREQS = [0.0, 0.5, -0.3137, 3.0 * 2.0 ** -32, 0.123456789, -0.05, 0.41, 1.0 / 3.0]
GAINS = [1.0, -0.5, 2.0, 0.75, 1.25, -1.0, 3.0, 0.125]
SHAPES = [(25, 4, 300, 3), (12, 5, 61, 2), (3, 2, 24, 1), (1, 7, 30, 1), (5, 3, 3, 2), (64, 63, 768, 2)]


def rows(K, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))


def taps(L, seed):
    return np.random.default_rng(seed).standard_normal(L)


@pytest.mark.parametrize("I,D,L,K", SHAPES)
@pytest.mark.parametrize("start", [0, 12345, (1 << 32) - 1000, (1 << 40) + 3])
def test_form_equals_the_definition_and_the_direct_sums(I, D, L, K, start):
    P = -(-L // I)
    n = max(6 * P + 40, -(-1300 * D // I))  # the first large start crosses 2^32 after 1000 samples, and a block of B
    v = rows(K, n, I + D + L)
    h = taps(L, K)
    for gains in (None, GAINS[:K]):
        a = rref.rduc64(v, h, I, D, FREQS[:K], gains, start)
        b = rref.rduc64_form(v, h, I, D, FREQS[:K], gains, start, samples_per_block=7)
        F = -(-n * I // D)
        assert a.shape == b.shape == (F,) and F > 1200
        S = rref.window_scale(v, h, I, D, gains)
        assert np.all(np.abs(a - b) <= 1e-12 * S)
        assert np.max(np.abs(a)) > 0.1 * np.max(S)
        which = sorted({0, 1, I - 1, I, 999, 1000, 1001, 1023, 1024, F // 2, F - 2, F - 1} & set(range(F)))
        c = rref.rduc64_direct(v, h, I, D, FREQS[:K], gains, start, which)
        assert np.all(np.abs(b[which] - c) <= 1e-12 * np.maximum(S[which], 1e-300))
    if start and K >= 3:  # the start matters (to a row whose frequency is neither 0 nor 0.5)
        assert np.max(np.abs(rref.rduc64(v, h, I, D, FREQS[:K], GAINS[:K], 0) - a)) > 1e-3 * np.max(S)


@pytest.mark.parametrize("I,D,L", [(25, 4, 300), (12, 5, 61), (3, 2, 24), (1, 7, 30), (5, 3, 3), (64, 63, 768)])
def test_zero_stuff_convolve_and_pick(I, D, L):
    """one row at f = 0 with gain 1: x[j] = (zero-stuffed v * h)[j D], and N items make ceil(N I / D) samples"""
    N = 5 * -(-L // I) + 23
    v = rows(1, N, L)[0]
    h = taps(L, I)
    up = np.zeros(N * I, dtype=np.complex128)
    up[::I] = v
    want = np.convolve(h, up)[:N * I][::D]
    assert want.size == -(-N * I // D)
    for fn in (rref.rduc64, rref.rduc64_form):
        got = fn(v, h, I, D, [0.0])
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 1e-12 * np.sum(np.abs(h)) * np.max(np.abs(v))
    m, r = rref.samples(N, I, D)
    assert np.all(m * I + r == np.arange(want.size) * D) and np.all(r < I) and m[-1] < N
    assert (want.size * D) // I >= N  # the next sample waits for an item that has not arrived
    if L < I:
        assert np.all(want[r >= L] == 0) and np.any(r >= L)


@pytest.mark.parametrize("I,L,K", [(5, 60, 3), (1, 1, 1), (3, 7, 2)])
def test_decimation_one_is_the_integer_duc(I, L, K):
    v = rows(K, 300, I + L)
    h = taps(L, K)
    want = uref.duc64(v, h, I, FREQS[:K], GAINS[:K], 777)
    for fn in (rref.rduc64, rref.rduc64_form):
        got = fn(v, h, I, 1, FREQS[:K], GAINS[:K], 777)
        assert got.shape == want.shape
        assert np.all(np.abs(got - want) <= 1e-12 * uref.window_scale(v, h, I, GAINS[:K]))
    assert np.allclose(rref.window_scale(v, h, I, 1, GAINS[:K]), uref.window_scale(v, h, I, GAINS[:K]), rtol=1e-12, atol=0)


@pytest.mark.parametrize("I,D", [(25, 4), (3, 2), (12, 5), (1, 7), (64, 63), (63, 64), (1023, 64), (2, 3), (5, 1)])
def test_sample_count_under_random_call_cuts(I, D):
    """a call writes the difference of ceil(N I / D) across the call; sample j exists exactly when item (j D) div I has
    arrived"""
    rng = np.random.default_rng(I * 100 + D)
    N = 0
    for n in [0, 1, 1, 1, 0, 2, D, D + 1, I, 1] + [int(t) for t in rng.integers(0, 3 * D + 2, 200)]:
        before, after = rref.sample_count(N, I, D), rref.sample_count(N + n, I, D)
        made = [j for j in range(before, after + 2) if N <= (j * D) // I < N + n]
        assert made == list(range(before, after))
        N += n
        m, r = rref.samples(N, I, D)
        assert m.size == after and (after == 0 or m[-1] < N) and (after * D) // I >= N
    if I < D:
        assert rref.sample_count(1, I, D) == 1 and rref.sample_count(2, I, D) - rref.sample_count(1, I, D) in (0, 1)


def test_window_scale():
    rng = np.random.default_rng(3)
    for I, D, L, K in [(25, 4, 300, 2), (3, 2, 7, 2), (1, 7, 30, 1), (5, 3, 3, 2), (4, 3, 2, 1)]:
        n = 9 * D + 5
        v = rng.standard_normal((K, n)) * (rng.random((K, n)) < 0.2)
        h = rng.standard_normal(L)
        a = GAINS[:K]
        got = rref.window_scale(v, h, I, D, a)
        assert got.size == -(-n * I // D)
        for j in range(got.size):
            m, r = divmod(j * D, I)
            ps = [p for p in range(-(-L // I)) if p * I + r < L]
            want = sum(abs(a[k]) * sum(abs(h[p * I + r]) for p in ps) *
                       max([abs(v[k, m - p]) for p in ps if m - p >= 0], default=0.0) for k in range(K))
            assert abs(got[j] - want) <= 1e-12 * max(want, 1e-300)


@pytest.mark.parametrize("I,D,P,f", [(25, 4, 12, 0.13), (3, 2, 12, -0.37)])
def test_float64_loopback(I, D, P, f):
    """rddc64(rduc64(v)) at one carrier, the default designs on both sides at P taps per phase: the Duc's prototype
    (DC gain I) and the Ddc's (interpolation D, decimation I: DC gain D) are the same Kaiser design of L = P I taps at I
    times the row's rate.  A row band-limited to the design's passband (|f| <= 0.25 of its rate) comes back delayed by
    the two filters' L - 1 samples at that rate less the Ddc's I - 1, that is by P - 1 items.  The level, by the integer
    Duc's argument (tests/test_duc_ref.py::test_float64_loopback): the passband passes both filters, (1 +- delta)^2,
    every image or alias is attenuated twice, so the RMS error is within 2 delta + O(delta^2) of the row's RMS: asserted
    at 3 delta, delta = 10^(-A / 20) the ripple of Kaiser's length rule."""
    L, n = I * P, 4096
    A = 2.285 * (2.0 * np.pi * 0.5 / I) * (L - 1) + 7.95
    delta = 10.0 ** (-A / 20.0)
    rng = np.random.default_rng(I)
    spec = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    spec[np.abs(np.fft.fftfreq(n)) > 0.25] = 0
    v = np.fft.ifft(spec)
    v /= np.sqrt(np.mean(np.abs(v) ** 2))
    hu = rref.rational_taps64(I, D, L)
    hd = dref_r.rational_taps64(D, I, L)
    assert np.allclose(hu * D, hd * I, rtol=1e-13, atol=0)
    start = (1 << 32) - 777
    x = rref.rduc64(v, hu, I, D, [f], None, start)
    y = dref_r.rddc64(x, hd, D, I, [f], start)[0]
    assert y.size == x.size * D // I and abs(y.size - n) <= 1
    lags = np.arange(0, 3 * P)
    mid = slice(4 * P, n - 4 * P)
    corr = [abs(np.vdot(v[mid], y[mid.start + lag:mid.stop + lag])) for lag in lags]
    lag = int(lags[int(np.argmax(corr))])
    assert lag == P - 1
    err = y[mid.start + lag:mid.stop + lag] - v[mid]
    rms = np.sqrt(np.mean(np.abs(err) ** 2))
    print(f"\n[rational duc loopback] {I} / {D}, P = {P}: A = {A:.1f} dB, delta = {delta:.3e}, rms error {rms:.3e} = "
          f"{rms / delta:.3f} delta")
    assert rms <= 3.0 * delta
    assert rms > 1e-3 * delta  # the comparison is not vacuous: the ripple is there


def test_tap_design():
    """gr4pm_duc_rational_taps (host only): the stated Kaiser design with DC gain I, the floats of gr4pm_duc_taps at
    D = 1, and the refusals, the cutoff's among them"""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    for I, D, P in [(25, 4, 12), (12, 5, 12), (3, 2, 8), (1000, 63, 2), (64, 63, 12), (5, 3, 1)]:
        h = pkg.duc_rational_taps(I, D, P)
        assert h.dtype == np.float32 and h.size == I * P
        h64 = rref.rational_taps64(I, D, I * P)
        assert np.all(np.abs(h - h64) <= dref.EPS32 * np.abs(h64) + 1e-12 * I)  # one rounding to float32, after the gain
        assert abs(float(np.sum(h.astype(np.float64))) - I) < 1e-5 * I
        if P >= 8:  # every branch has gain about 1
            assert np.all(np.abs(rref.branch_taps(h, I).sum(axis=1) - 1.0) < 1e-3)
    # band edges in units of the input rate, I < D: the cutoff up to half of the OUTPUT rate, I / D of the input's
    h = pkg.duc_rational_taps(2, 3, 12, 0.25 * 2 / 3, 0.75 * 2 / 3)
    h64 = rref.rational_taps64(2, 3, 24, 0.25 * 2 / 3, 0.75 * 2 / 3)
    assert np.all(np.abs(h - h64) <= dref.EPS32 * np.abs(h64) + 1e-12)
    for I, P in [(5, 12), (20, 8), (1000, 2), (1, 12), (16, 12)]:
        assert np.array_equal(pkg.duc_rational_taps(I, 1, P).view(np.uint32), pkg.duc_taps(I, P).view(np.uint32))
    assert np.array_equal(pkg.duc_rational_taps(16, 1, 12, 0.2, 0.6).view(np.uint32), pkg.duc_taps(16, 12, 0.2, 0.6).view(np.uint32))
    for bad in [(0, 4, 12), (1025, 4, 1), (25, 0, 12), (25, 65, 12), (25, 4, 0), (1023, 4, 9)]:
        with pytest.raises(pkg.Gr4pmError):
            pkg.duc_rational_taps(*bad)
    with pytest.raises(pkg.Gr4pmError):
        pkg.duc_rational_taps(25, 4, 12, 0.75, 0.25)
    # the cutoff: at most half of the input rate (I >= D) ...
    assert pkg.duc_rational_taps(25, 4, 12, 0.25, 0.75).size == 300
    with pytest.raises(pkg.Gr4pmError, match="cutoff"):
        pkg.duc_rational_taps(25, 4, 12, 0.25, 0.76)
    # ... and at most half of the output rate (I < D): the defaults are beyond it
    with pytest.raises(pkg.Gr4pmError, match="cutoff"):
        pkg.duc_rational_taps(2, 3, 12)
    with pytest.raises(pkg.Gr4pmError, match="cutoff"):
        pkg.duc_rational_taps(2, 3, 12, 0.2, 0.47)
    assert pkg.duc_rational_taps(2, 3, 12, 0.2, 0.46).size == 24


def test_position_header_under_sanitizers(tmp_path):
    """csrc/hostlogic/resample_position.hpp, the arithmetic gr4pm_duc_process and gr4pm_ddc_process run on the host, as
    a stand-alone program built with -fsanitize=undefined,address: the outputs of every call, first() and the state
    behind it against Python integers, for random (I, D) and call lengths, from positions near 2^63 and across the wrap
    of the 64-bit counters.  Every case runs as a Duc's (lead = 0: N items have made ceil(N I / D) samples) and, with the
    pair swapped so that I <= 64 and D <= 1024, as a Ddc's (lead = D - 1: floor(N I / D) items, and the calls of any cut
    of N samples sum to _ddc_rational_ref.item_count)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "needs a host C++ compiler"
    exe = str(tmp_path / "resample_position_check.bin")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "gr4-packet-modem_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "hostlogic", "resample_position_check.cpp")], check=True, capture_output=True, text=True)
    rng = np.random.default_rng(19)
    M = 1 << 64
    lines, want, cuts = [], [], []  # cuts: (first line of `want`, calls, I, D, N before, N after) of every Ddc case
    pairs = [(25, 4), (3, 2), (12, 5), (1, 7), (5, 3), (1000, 63), (63, 64), (1023, 64), (2, 3), (1024, 63), (1, 64)]
    while len(pairs) < 60:
        i, d = int(rng.integers(1, 1025)), int(rng.integers(2, 65))
        if math.gcd(i, d) == 1:
            pairs.append((i, d))
    bases = [0, 1, (1 << 31) + 5, (1 << 63) - 1000, (1 << 63) + 3, M - 50, (M - 3 * 1024) // 1024]

    def case(I, D, lead, N, lens):
        made = lambda n: max(0, -(-(n * I - lead) // D))  # outputs whose newest item (lead + j D) div I is below n
        J = made(N)
        m, r = divmod(lead + J * D, I)
        lines.append(" ".join(str(t) for t in [I, D, lead, N % M, m % M, r, len(lens)] + lens))
        for n in lens:
            first = lead + J * D - N * I
            assert 0 <= first < I + D
            N += n
            Jn = made(N)
            m, r = divmod(lead + Jn * D, I)
            want.append(f"{Jn - J} {first} {N % M} {m % M} {r}")
            J = Jn
        want.append(f"reset 0 {lead // I} {lead % I}")
        return N

    for c, (I, D) in enumerate(pairs):
        N = bases[c % len(bases)] + int(rng.integers(0, 100))  # items taken so far: a Python integer, never reduced
        lens = [0, 1, 1, 0, 1, D, I] + [int(t) for t in rng.integers(0, 4 * D + 3, 30)] + [1 << 31, int(rng.integers(1, 1 << 31))]
        case(I, D, 0, N, lens)
    assert all(w == "reset 0 0 0" for w in want if w.startswith("reset"))
    for c, (D, I) in enumerate(pairs):  # the same pairs, bases and kinds of cut as a Ddc's: I <= 64, D <= 1024
        assert I <= 64 and D <= 1024
        for N in (bases[c % len(bases)] + int(rng.integers(0, 100)), 0):
            lens = [0, 1, 1, 0, 1, D, I] + [int(t) for t in rng.integers(0, 4 * D + 3, 30)] + [1 << 31, int(rng.integers(1, 1 << 31))]
            at = len(want)
            cuts.append((at, len(lens), I, D, N, case(I, D, D - 1, N, lens)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    got = run.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, bad[:5]
    for at, calls, I, D, N0, N1 in cuts:  # what the program printed, summed over the cut
        total = sum(int(g.split()[0]) for g in got[at:at + calls])
        assert total == dref_r.item_count(N1, I, D) - dref_r.item_count(N0, I, D)
        assert N0 or total == N1 * I // D
