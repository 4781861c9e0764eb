"""SyncwordDetection against float64: the correlator's powers within an energy-relative bound of the exact overlap-save
powers, exact power-of-two scaling, and the detector's decisions exact on the GPU's own powers.

The float32 correlator's error is relative to the block's energy, not to each output (a lag 40 dB under the stream's
peak is still counted by the median test), so every lag is held to
    | sqrt(zpow) - sqrt(zpow64) | <= C * 2^-24 * E_j,   E_j = ||FFT64(x[j:j+N])|| * max_b ||T_b||
with C = 2 for the CPU oracle and C = 8 for every GPU form.  The decisions (best lag, ties, the median test's '<')
are held exactly to tests/_float64_ref.detect() run on the powers the GPU itself reports."""
import numpy as np
import pytest

import _float64_ref as f64
import _oracle as orc
import _signals as sig

EPS = f64.EPS32
SCALES = (-24, -7, 5, 24)
N_SYM = 50000


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.complex64 else a.view(np.uint32)


def short_rrc(sps, ntaps):
    rrc = orc.rrc_taps(1.0, float(sps), 1.0, 0.35, ntaps)
    return (rrc / np.sqrt(np.sum(rrc.astype(np.float64) ** 2))).astype(np.float32)


def template_length(rrc, sps):
    return 63 * sps + rrc.size


# ------------------------------------------------------------------------------------------------------- stimuli
def impulse_stretch(S, N, L, amp=1.0):
    """zeros with one impulse per third block at block offsets 0, 1, S-1, S, N-L, N-1, 1792, 1793 (the lag mapping and
    the correlator's pruned lags >= 1793)"""
    offs = [0, 1, S - 1, S, N - L, N - 1, 1792, 1793]
    x = np.zeros((3 * len(offs) + 2) * S + N + max(offs), dtype=np.complex64)
    for i, o in enumerate(offs):
        x[(3 * i + 1) * S + o] = amp
    return x


def dynamic_range_stream(sps=4, rrc=None, S=1752, N=2048, seed=5, quiet=True):
    """a qa stream cut into segments scaled 2^-20, 1, 2^10, 2^-10, 2^3, 2^-16 and (quiet) 2^-64 (powers down to ~1e-31,
    still normal), each with noise 26 dB under it; then (quiet) noise alone, exact zeros, and unit impulses at chosen
    block offsets"""
    scales = [-20, 0, 10, -10, 3, -16] + ([-64] if quiet else [])
    seg_sym = N_SYM // len(scales)
    locs = [s * seg_sym + o for s in range(len(scales)) for o in (300, 4000)]
    x, qa_rrc = sig.qa_syncword_stream(N_SYM, locs, 0.005, seed=seed, sps=sps)
    x = x.astype(np.complex128)
    seg = x.size // len(scales)
    noise = sig.awgn(x.size, 0.05, seed + 1).astype(np.complex128)
    for i, k in enumerate(scales):
        sl = slice(i * seg, x.size if i == len(scales) - 1 else (i + 1) * seg)
        x[sl] = (x[sl] + noise[sl]) * 2.0 ** k
    L = template_length(qa_rrc if rrc is None else rrc, sps)
    if not quiet:
        return x.astype(np.complex64)
    parts = [x.astype(np.complex64), sig.awgn(3 * N, 0.3, seed + 2), np.zeros(3 * N, np.complex64),
             impulse_stretch(S, N, L)]
    return np.concatenate(parts).astype(np.complex64)


def scaling_stream(sps=4, seed=11):
    """segments at 2^-4 .. 2^4 with components on a grid of 2^-24: every x * 2^k of SCALES stays far from the float range's
    ends (checked by the tests)"""
    x, _ = sig.qa_syncword_stream(30000, [300, 7000, 21000], 0.003, seed=seed, sps=sps)
    x = (x + sig.awgn(x.size, 0.1, seed + 1)).astype(np.complex128)
    seg = x.size // 3
    for i, k in enumerate((-4, 0, 4)):
        x[i * seg:(i + 1) * seg] *= 2.0 ** k
    x = np.round(x * 2.0 ** 24) / 2.0 ** 24
    return np.concatenate([x.astype(np.complex64), np.zeros(5000, np.complex64)])


# ------------------------------------------------------------------------------------------------------- CPU: refs
ORACLE_CONFIGS = {
    "sps4_9bins": dict(sps=4, rrc=None, lo=-4, hi=4, N=2048),
    "sps2_short": dict(sps=2, rrc=("short", 2, 22), lo=-4, hi=4, N=2048),
    "n4096_1025taps": dict(sps=4, rrc=("short", 4, 1024), lo=-2, hi=2, N=4096),
    "n512": dict(sps=4, rrc=None, lo=-1, hi=1, N=512),
}


def config_rrc(cfg):
    if cfg["rrc"] is None:
        return orc.unit_norm_rrc(cfg["sps"])[0]
    _, sps, ntaps = cfg["rrc"]
    return short_rrc(sps, ntaps)


@pytest.mark.parametrize("name", sorted(ORACLE_CONFIGS))
def test_templates64_match_the_oracle_templates(name):
    """the float64 template spectra agree with the oracle's (a float32 FFT of float32 products) to fp32 rounding of the
    spectrum's norm"""
    cfg = ORACLE_CONFIGS[name]
    rrc = config_rrc(cfg)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, cfg["lo"], cfg["hi"], fft_size=cfg["N"],
                                samples_per_symbol=cfg["sps"])
    t64 = f64.templates64(rrc, cfg["sps"], cfg["lo"], cfg["hi"], cfg["N"])
    assert t64.shape == (cfg["hi"] - cfg["lo"] + 1, cfg["N"])
    for b in range(t64.shape[0]):
        t = ref.template(b)
        assert np.max(np.abs(t - t64[b])) <= 1.0 * EPS * np.linalg.norm(t64[b]), b
        # not vacuous: the spectra differ from bin to bin far beyond that
        if b:
            assert np.max(np.abs(t64[b] - t64[b - 1])) > 1e3 * EPS * np.linalg.norm(t64[b])


def oracle_run(x, cfg, chunks=None, T=768, pt=20.0):
    """the oracle's debug powers / bins / tags, in one call or the given ragged calls (consumed items carried)"""
    rrc = config_rrc(cfg)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, cfg["lo"], cfg["hi"], fft_size=cfg["N"],
                                samples_per_symbol=cfg["sps"], time_threshold=T, power_threshold=pt)
    if chunks is None:
        _, _, tags, zp, bn = ref.process(x, debug=True, tags_cap=1 << 16)
        return zp, bn, tags["index"].astype(np.uint64)
    pos, zs, bs, ts = 0, [], [], []
    for m in chunks:
        if pos + cfg["N"] > x.size:
            break
        _, o, t, zp, bn = ref.process(x[pos:pos + m], debug=True, tags_cap=1 << 16)
        zs.append(zp)
        bs.append(bn)
        ts.append(t["index"].astype(np.uint64))  # the oracle counts indices from the stream's start
        pos += o.size
    return np.concatenate(zs), np.concatenate(bs), np.concatenate(ts)


def ragged(n, seed, N=2048):
    """call lengths in [N, 40000)"""
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.integers(N, 40000, size=n // N + 2)]


@pytest.mark.parametrize("name", sorted(ORACLE_CONFIGS))
@pytest.mark.parametrize("calls", ["one", "ragged"])
def test_oracle_powers_within_the_float64_bound(name, calls):
    """CPU oracle: |sqrt(zpow) - sqrt(zpow64)| <= 2 * 2^-24 * E_j at every lag; exactly 0 where a block is all zeros;
    the per-lag best bin equals float64's wherever the best two bins are further apart than twice the bound"""
    cfg = ORACLE_CONFIGS[name]
    rrc = config_rrc(cfg)
    L = template_length(rrc, cfg["sps"])
    S = cfg["N"] - L + 1
    x = dynamic_range_stream(cfg["sps"], rrc, S, cfg["N"])
    zp, bn, _ = oracle_run(x, cfg, None if calls == "one" else ragged(x.size, 7, cfg["N"]))
    r = f64.zpow64(x, f64.templates64(rrc, cfg["sps"], cfg["lo"], cfg["hi"], cfg["N"]), cfg["N"], L)
    assert zp.size == r.zpow.size or (calls == "ragged" and zp.size < r.zpow.size)
    n = zp.size
    E = r.E_per_lag()[:n]
    assert np.min(r.zpow[:n][r.zpow[:n] > 0]) > 2.0 ** -120  # the stimulus keeps every power normal
    if cfg["N"] == 2048:
        assert np.min(r.zpow[:n][r.zpow[:n] > 0]) < 1e-30    # ... and reaches far below 1e-30
    err = np.abs(np.sqrt(zp.astype(np.float64)) - np.sqrt(r.zpow[:n]))
    assert np.all(err <= 2 * EPS * E), np.max(err / (EPS * E))
    assert np.all(zp[E == 0] == 0) and np.count_nonzero(E == 0) > 4 * S
    sep = r.gap[:n] > 2 * (2 * EPS * E)
    assert np.count_nonzero(sep) > n // 2
    assert np.array_equal(bn[sep] - cfg["lo"], r.bins[:n][sep])


def periodic_stream(S, sps=4, periods=60, seed=3, amp=1.0):
    """period exactly S (consecutive overlap-save blocks see identical samples: identical powers, exact ties), one
    syncword per period"""
    rng = np.random.default_rng(seed)
    rrc, _ = orc.unit_norm_rrc(sps)
    sym = rng.integers(0, 2, size=(S * 4) // sps + 200).astype(np.uint8)
    sym[100:164] = sig.SYNCWORD
    y = orc.interpolating_fir(sig.BPSK[sym], sps, rrc)
    one = y[S:2 * S]  # inside the filtered stream: one syncword in every period
    return (np.tile(one, periods) * np.float32(amp)).astype(np.complex64), rrc


def dc_burst_stream(sps=4, seed=9):
    """a constant stretch (every item a candidate: more than kTestsPerBlock in each block) with bursts inside it"""
    x, rrc = sig.qa_syncword_stream(40000, [500, 9000, 20000, 31000], 0.0, seed=seed, sps=sps)
    x = (0.5 * x).astype(np.complex64)
    dc = np.full(x.size, 0.25 + 0.0j, dtype=np.complex64)
    dc[30000:50000] += x[30000:50000]
    dc[90000:96000] += 4 * x[90000:96000]
    return dc, rrc


def edge_threshold(best, h):
    """a float32 power_threshold with f32(best) / pt == h exactly (searched over a few ulps around best / h), or None"""
    best, h = np.float32(best), np.float32(h)
    p0 = np.float32(best / h)
    for d in range(-8, 9):
        pt = (p0.view(np.int32) + np.int32(d)).view(np.float32)
        if np.float32(best / pt) == h:
            return pt
    return None


def threshold_edges(z, T, n_points=3):
    """resets of z whose (T+1)-th smallest history value h* gives an edge threshold in [1.5, 1e6]: (pt*, pt below,
    pt above) for the strongest ones.  At pt* the test counts exactly T powers '<' h* (fail); one ulp lower it passes."""
    out = []
    for b, c in f64.resets(z, T):
        hv = np.sort(f64.history_values(z, c, T))
        h = hv[T]
        if h <= 0 or hv[T - 1] == h or z[b] <= 0:  # exactly T powers below h*
            continue
        pt = edge_threshold(z[b], h)
        if pt is None or not 1.5 <= pt <= 1e6:
            continue
        out.append((float(z[b]), pt))
    out.sort(reverse=True)
    res = []
    for _, pt in out[:n_points]:
        res += [pt, np.nextafter(pt, np.float32(0)), np.nextafter(pt, np.float32(np.inf))]
    return res


def detector_cases():
    """(name, x, rrc, sps, lo, hi, T, pt) for the CPU and the GPU decision tests"""
    cases = []
    rng = np.random.default_rng(2024)
    for case in range(12):  # the ranges of tools/fuzz_detector.py
        sps = int(rng.choice([2, 4]))
        rrc = short_rrc(sps, int(rng.choice([10, 22, 44])) * (sps // 2))
        T = int(rng.integers(64, 1100))
        lo = int(rng.integers(-6, 3))
        hi = int(rng.integers(lo, min(lo + 9, 7)))
        pt = float(rng.uniform(6.0, 14.0))
        L = template_length(rrc, sps)
        nsym = int(rng.integers(20000, 40000))
        symbols = rng.integers(0, 2, nsym).astype(np.uint8)
        for loc in np.sort(rng.choice(np.arange(100, nsym - 200), int(rng.integers(3, 12)), replace=False)):
            symbols[loc:loc + 64] = sig.SYNCWORD
        f = float(rng.uniform(lo - 0.4, hi + 0.4)) * np.pi / L
        x = orc.rotator(orc.interpolating_fir(sig.BPSK[symbols], sps, rrc), np.float32(f))
        x = (x + sig.awgn(x.size, float(rng.uniform(0.02, 0.4)), 1000 + case)).astype(np.complex64)
        cases.append((f"random{case}", x, rrc, sps, lo, hi, T, pt))
    for T in (1751, 1752, 1753, 3504):  # S - 1, S, S + 1, 2S at sps 4, 45 taps
        x, rrc = periodic_stream(1752)
        cases.append((f"ties_T{T}", x, rrc, 4, -1, 1, T, 6.0))
    x, rrc = dc_burst_stream()
    for T in (768, 200):
        cases.append((f"dc_T{T}", x, rrc, 4, -4, 4, T, 9.5))
    return cases


_CASES = None


def cases_by_name():
    global _CASES
    if _CASES is None:
        _CASES = {c[0]: c for c in detector_cases()}
    return _CASES


CASE_NAMES = [f"random{i}" for i in range(12)] + [f"ties_T{T}" for T in (1751, 1752, 1753, 3504)] + \
    ["dc_T768", "dc_T200"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_detect_reproduces_the_oracle_tags(name):
    """detect() on the oracle's own debug powers == the oracle's tag indices, including exact ties (periodic input) and
    thresholds at the edge of the median test, in one call and in ragged calls"""
    _, x, rrc, sps, lo, hi, T, pt = cases_by_name()[name]
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, lo, hi, samples_per_symbol=sps, time_threshold=T,
                                power_threshold=pt)
    _, _, tags, zp, _ = ref.process(x, debug=True, tags_cap=1 << 16)
    assert np.array_equal(f64.detect(zp, T, pt), tags["index"])
    if name.startswith("ties"):
        S = 2048 - template_length(rrc, sps) + 1
        assert np.array_equal(zp[S:2 * S], zp[2 * S:3 * S])          # the ties are exact
        assert np.max(zp[S:2 * S]) == np.max(zp[:4 * S]) and tags.size > 5
    pts = threshold_edges(zp, T, 2)
    assert len(pts) >= 3
    for p in pts:
        ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, lo, hi, samples_per_symbol=sps, time_threshold=T,
                                    power_threshold=float(p))
        _, _, t, zp2, _ = ref.process(x, debug=True, tags_cap=1 << 16)
        assert np.array_equal(bits(zp2), bits(zp))
        assert np.array_equal(f64.detect(zp, T, p), t["index"]), p
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, lo, hi, samples_per_symbol=sps, time_threshold=T,
                                power_threshold=pt)
    pos, zs, ts = 0, [], []
    for m in ragged(x.size, 5):
        if pos + 2048 > x.size:
            break
        _, o, t, z, _ = ref.process(x[pos:pos + m], debug=True, tags_cap=1 << 16)
        zs.append(z)
        ts.append(t["index"].astype(np.uint64))
        pos += o.size
    assert np.array_equal(f64.detect(zs, T, pt), np.concatenate(ts))


def test_threshold_edge_flips_exactly_one_decision():
    """detect()'s '<': at pt* (f32(best) / pt* == h*, the (T+1)-th smallest history value) that reset fails, one ulp
    lower it passes"""
    _, x, rrc, sps, lo, hi, T, pt = cases_by_name()["random0"]
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, lo, hi, samples_per_symbol=sps, time_threshold=T,
                                power_threshold=pt)
    _, _, _, zp, _ = ref.process(x, debug=True, tags_cap=1 << 16)
    pts = threshold_edges(zp, T, 1)
    a, lower = set(f64.detect(zp, T, pts[0]).tolist()), set(f64.detect(zp, T, pts[1]).tolist())
    assert a < lower and len(lower - a) >= 1


def test_detect_fast_path_equals_the_loop():
    """the reset-to-reset jumps == the sample-by-sample loop, on powers full of ties and zero stretches"""
    rng = np.random.default_rng(0)
    for T in (1, 3, 32, 40, 100, 257):
        for q in (3, 1000):
            z = rng.integers(0, q, 30000).astype(np.float32)
            z[5000:6000] = 0
            z[9000:9400] = 7
            assert f64.resets(z, T, loop=True) == f64.resets(z, T, loop=False)
            assert np.array_equal(f64.detect(z, T, 1.5, loop=True), f64.detect(z, T, 1.5, loop=False))


@pytest.mark.timeout(120)
def test_detect_handles_2_22_samples_in_seconds():
    import time
    z = np.random.default_rng(1).random(1 << 22).astype(np.float32)
    t0 = time.perf_counter()
    d = f64.detect(z, 768, 1.05)
    assert time.perf_counter() - t0 < 5.0 and d.size > 1000


def test_oracle_is_exactly_scale_invariant():
    """x -> 2^k x, k in {-24, -7, 5, 24}, on the dynamic-range stream: zpow bit-for-bit 2^2k times, identical bins,
    tag indices, phase / freq / time_est / freq_bin bits, amplitude bit-for-bit 2^k times"""
    x = dynamic_range_stream(quiet=False)  # without the 2^-64 segment: every scaled power stays normal
    cfg = ORACLE_CONFIGS["sps4_9bins"]
    z0, b0, _ = oracle_run(x, cfg)
    rrc = config_rrc(cfg)
    base = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0)
    _, o0, t0, _, _ = base.process(x, debug=True)
    assert t0.size >= 8
    for k in SCALES:
        xs = (x * np.float32(2.0 ** k)).astype(np.complex64)
        assert np.array_equal(xs / np.float32(2.0 ** k), x)
        ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0)
        _, o, t, z, b = ref.process(xs, debug=True)
        assert np.array_equal(bits(z), bits((z0 * np.float32(2.0 ** (2 * k))).astype(np.float32))), k
        assert np.array_equal(b, b0)
        assert np.array_equal(bits(o), bits((o0 * np.float32(2.0 ** k)).astype(np.complex64)))
        for f in ("index", "phase", "freq", "time_est", "freq_bin"):
            assert np.array_equal(t[f], t0[f]), (k, f)
        assert np.array_equal(bits(t["amplitude"]), bits((t0["amplitude"] * np.float32(2.0 ** k)).astype(np.float32)))


# ------------------------------------------------------------------------------------------------------- GPU
SWITCHES = ("GR4PM_CORRELATOR", "GR4PM_W64_ONE", "GR4PM_SD_SEPARATE_MEDIAN", "GR4PM_CANDIDATES_LDS", "GR4PM_SD_NO_SUPER")

# form -> (environment at creation, sps, rrc (None: the 45-tap unit-norm one, or (sps, taps)), lo, hi, fft_size)
FORMS = {
    "w64_9bins": ({}, 4, None, -4, 4, 2048),
    "w64_3bins": ({}, 4, None, -1, 1, 2048),
    "w64_one": ({}, 4, None, 0, 0, 2048),                                   # k_correlate_w64_one
    "w64_one_off": ({"GR4PM_W64_ONE": "0"}, 4, None, 0, 0, 2048),          # the general kernel, one bin
    "wave": ({"GR4PM_CORRELATOR": "wave"}, 4, None, -4, 4, 2048),
    "pair": ({"GR4PM_CORRELATOR": "pair"}, 4, None, -4, 4, 2048),
    "long_stride": ({}, 2, (2, 22), -4, 4, 2048),                           # S = 1900 > 1793: no pruned lags
    "c4096": ({}, 4, (4, 1024), -2, 2, 4096),                               # k_correlate_4096
    "c4096_radix2": ({"GR4PM_CORRELATOR": "radix2"}, 4, (4, 1024), -2, 2, 4096),
    "generic1024": ({}, 4, None, -2, 2, 1024),
    "generic512": ({}, 4, None, -1, 1, 512),
}


@pytest.fixture(scope="module")
def pkg():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__ as ge
    return ge.load_package()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def set_switches(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def form_setup(form):
    env, sps, rr, lo, hi, N = FORMS[form]
    rrc = orc.unit_norm_rrc(sps)[0] if rr is None else short_rrc(*rr)
    L = template_length(rrc, sps)
    return env, sps, rrc, lo, hi, N, L, N - L + 1


def gpu_calls(sd, x, chunks=None, rows=1, tags_cap=8192):
    """run x ([n] or [rows, n]) in one call or in ragged calls; per row: concatenated powers and tags (index made
    absolute), plus the items consumed"""
    x2 = x.reshape(rows, -1)
    N = sd.fft_size
    pos, zs, ts = 0, [[] for _ in range(rows)], [[] for _ in range(rows)]
    for m in (chunks if chunks is not None else [x2.shape[1]]):
        if pos + N > x2.shape[1]:
            break
        xin = dev(x2[:, pos:pos + m]) if rows > 1 else dev(x2[0, pos:pos + m])
        st, _, tags, n = sd.process_bulk(xin, want_output=False, tags_cap=tags_cap)
        assert st == 0 and n > 0
        z = sd.last_zpow(n).cpu().numpy()
        tl = tags if rows > 1 else [tags]
        for r in range(rows):
            zs[r].append(z[r])
            t = tl[r].copy()
            t["index"] += pos
            ts[r].append(t)
        pos += n
    return [np.concatenate(z) for z in zs], [np.concatenate(t) for t in ts], pos


def check_bound(zg, r, tags, lo, T, bar=8.0):
    n = zg.size
    E = r.E_per_lag()[:n]
    err = np.abs(np.sqrt(zg.astype(np.float64)) - np.sqrt(r.zpow[:n]))
    C = float(np.max(err[E > 0] / (EPS * E[E > 0])))
    assert np.all(err <= bar * EPS * E), ("C", C, int(np.argmax(err / np.maximum(E, 1e-300))))
    assert np.all(zg[E == 0] == 0)
    lag = tags["index"].astype(np.int64) - (2 * T + 1)
    sep = r.gap[lag] > 2 * bar * EPS * E[lag]
    assert np.array_equal(tags["freq_bin"][sep], lo + r.bins[lag][sep])
    return C, int(np.count_nonzero(sep))


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_gpu_powers_within_the_float64_bound(pkg, monkeypatch, form):
    """every correlator form: |sqrt(zpow) - sqrt(zpow64)| <= 8 * 2^-24 * E_j at every lag of every block, in one call
    and in ragged calls; exactly 0 where a block is all zeros; a tag's freq_bin equals float64's best bin wherever that
    leads the second by more than twice the bound.  Measured C (one call, MI355X): w64_9bins 1.22, w64_3bins 1.22,
    w64_one 1.22, w64_one_off 1.22, wave 0.97, pair 0.97, long_stride 0.65, c4096 0.69, c4096_radix2 0.68,
    generic1024 1.54, generic512 1.59; four channels 0.85 / 1.14 / 0.81 / 1.14 (the oracle: 1.08)"""
    env, sps, rrc, lo, hi, N, L, S = form_setup(form)
    set_switches(monkeypatch, env)
    x = dynamic_range_stream(sps, rrc, S, N)
    r = f64.zpow64(x, f64.templates64(rrc, sps, lo, hi, N), N, L)
    T = 768
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, lo, hi, fft_size=N, samples_per_symbol=sps,
                               time_threshold=T, power_threshold=20.0, max_items=x.size)
    (zg,), (tags,), n = gpu_calls(sd, x)
    assert n == r.zpow.size and tags.size >= 6
    C, n_sep = check_bound(zg, r, tags, lo, T)
    print(f"\n[float64 bound] {form}: C = {C:.3f}, {tags.size} tags ({n_sep} with a separated bin)")
    sd2 = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, lo, hi, fft_size=N, samples_per_symbol=sps,
                                time_threshold=T, power_threshold=20.0, max_items=x.size)
    (zr,), (tr,), _ = gpu_calls(sd2, x, ragged(x.size, 17, N))
    check_bound(zr, r, tr, lo, T)
    assert np.array_equal(tr["index"], tags["index"][:tr.size])


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_gpu_four_channels_at_four_scales_within_the_float64_bound(pkg, monkeypatch):
    """n_channels = 4 in one launch, channel c at 2^-20, 1, 2^10, 2^-8 with its own content: a channel-stride or a
    shared-scale fault cannot hide"""
    set_switches(monkeypatch, {})
    rrc = orc.unit_norm_rrc(4)[0]
    rows = []
    for c, k in enumerate((-20, 0, 10, -8)):
        x, _ = sig.qa_syncword_stream(30000, [500 + 700 * c, 9000, 21000 - 300 * c], 0.004 * (c - 1), seed=40 + c)
        x = (x + sig.awgn(x.size, 0.05, 50 + c)) * np.float32(2.0 ** k)
        x[40000 + 3000 * c:52000 + 3000 * c] = 0
        rows.append(x.astype(np.complex64))
    X = np.stack(rows)
    T = 768
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0, n_channels=4,
                               max_items=X.shape[1])
    zs, ts, n = gpu_calls(sd, X, rows=4)
    t64 = f64.templates64(rrc, 4, -4, 4, 2048)
    for c in range(4):
        r = f64.zpow64(X[c], t64, 2048, 297)
        assert zs[c].size == r.zpow.size and ts[c].size >= 3
        C, _ = check_bound(zs[c], r, ts[c], -4, T)
        print(f"\n[float64 bound] channel {c}: C = {C:.3f}")
        assert np.array_equal(ts[c]["index"], f64.detect(zs[c], T, 20.0))


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_gpu_power_of_two_scaling_is_exact(pkg, monkeypatch, form):
    """x -> 2^k x, k in {-24, -7, 5, 24}: zpow bit-for-bit 2^2k times, output items 2^k times, tag index / freq_bin /
    phase / freq / time_est / esn0_db identical, amplitude 2^k and noise_power 2^2k times.  Every step of the
    correlator is linear: a difference can only come from an absolute constant, a flush to zero or a reciprocal in place
    of a division"""
    env, sps, rrc, lo, hi, N, L, S = form_setup(form)
    set_switches(monkeypatch, env)
    x = scaling_stream(sps)

    def run(xs):
        sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, lo, hi, fft_size=N, samples_per_symbol=sps,
                                   power_threshold=20.0, max_items=xs.size)
        st, out, tags, n = sd.process_bulk(dev(xs))
        assert st == 0
        return out.cpu().numpy(), tags, sd.last_zpow(n).cpu().numpy()[0]

    o0, t0, z0 = run(x)
    assert t0.size >= 3
    nz = np.concatenate([np.abs(x.real), np.abs(x.imag)])
    nz = nz[nz > 0]
    for k in SCALES:
        f = np.float32(2.0 ** k)
        assert np.max(z0) * 2.0 ** (2 * k) < 2.0 ** 120 and np.min(nz) * 2.0 ** k > 2.0 ** -60
        o, t, z = run((x * f).astype(np.complex64))
        assert np.array_equal(bits(z), bits((z0 * np.float32(2.0 ** (2 * k))).astype(np.float32))), k
        assert np.array_equal(bits(o), bits((o0 * f).astype(np.complex64))), k
        for fld in ("index", "freq_bin", "phase", "freq", "time_est", "esn0_db"):
            assert np.array_equal(t[fld], t0[fld]), (k, fld)
        assert np.array_equal(bits(t["amplitude"]), bits((t0["amplitude"] * f).astype(np.float32))), k
        assert np.array_equal(bits(t["noise_power"]), bits((t0["noise_power"] * np.float32(2.0 ** (2 * k))).astype(np.float32))), k


DETECTOR_SWITCHES = {"default": {}, "separate_median": {"GR4PM_SD_SEPARATE_MEDIAN": "1"},
                     "candidates_lds": {"GR4PM_CANDIDATES_LDS": "1"}, "no_super": {"GR4PM_SD_NO_SUPER": "1"}}


def gpu_detector(pkg, x, rrc, sps, lo, hi, T, pt, chunks=None, rows=1):
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, lo, hi, samples_per_symbol=sps, time_threshold=T,
                               power_threshold=float(pt), n_channels=rows, max_items=x.shape[-1])
    zs, ts, n = gpu_calls(sd, x, chunks, rows=rows, tags_cap=1 << 15)
    return sd, zs, ts, n


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("switch", sorted(DETECTOR_SWITCHES))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_detector_decisions_exact(pkg, monkeypatch, name, switch):
    """GPU tag indices == detect() on the GPU's own powers, exactly: random settings, exact ties (input periodic in S),
    a constant stretch (more than 8 candidates a block: the deferred k_median_tests path), and power_threshold at the
    edge of the median test (f32(best) / pt == h*, the (T+1)-th smallest history value) and one ulp either side; in one
    call and in ragged calls.  The powers do not depend on the two thresholds: bit-identical across such runs"""
    set_switches(monkeypatch, DETECTOR_SWITCHES[switch])
    _, x, rrc, sps, lo, hi, T, pt = cases_by_name()[name]
    sd, (z,), (tags,), n = gpu_detector(pkg, x, rrc, sps, lo, hi, T, pt)
    assert np.array_equal(tags["index"], f64.detect(z, T, pt))
    if name.startswith("dc") and switch == "default":
        visited, deferred = sd.scan_counts()
        assert deferred > 0, (visited, deferred)  # the deferred path decided some of them
    if name.startswith("ties"):
        S = 2048 - template_length(rrc, sps) + 1
        assert np.array_equal(bits(z[S:2 * S]), bits(z[2 * S:3 * S])) and tags.size > 5
    _, (zr,), (tr,), _ = gpu_detector(pkg, x, rrc, sps, lo, hi, T, pt, ragged(x.size, 23))
    assert np.array_equal(tr["index"], f64.detect(zr, T, pt))
    T2, pt2 = (T + 37, pt * 1.7)
    _, (z2,), _, n2 = gpu_detector(pkg, x, rrc, sps, lo, hi, T2, pt2)
    assert n2 == n and np.array_equal(bits(z2), bits(z))
    pts = threshold_edges(z, T, 2)
    assert len(pts) >= 3
    for p in pts:
        _, (ze,), (te,), _ = gpu_detector(pkg, x, rrc, sps, lo, hi, T, p)
        assert np.array_equal(bits(ze), bits(z))
        assert np.array_equal(te["index"], f64.detect(z, T, p)), p


WINDOW_T = (1, 64, 767, 768, 769, 1751, 1752, 1753, 3000, 8192)


@pytest.fixture(scope="module")
def window_stream():
    locs = [300, 2000, 2100, 9000, 15000, 22222, 30000]
    x, rrc = sig.qa_syncword_stream(36000, locs, 0.006, seed=77)
    return (0.7 * x + sig.awgn(x.size, 0.3, 78)).astype(np.complex64), rrc


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("switch", sorted(DETECTOR_SWITCHES))
@pytest.mark.parametrize("T", WINDOW_T)
def test_gpu_detector_window_sizes(pkg, monkeypatch, window_stream, T, switch):
    """T across the built range (1 .. 8192) and around its internal sizes (768 = 12 x 64, S - 1 .. S + 1): tags ==
    detect() on the GPU's powers, in one call and in ragged calls"""
    set_switches(monkeypatch, DETECTOR_SWITCHES[switch])
    x, rrc = window_stream
    _, (z,), (tags,), _ = gpu_detector(pkg, x, rrc, 4, -4, 4, T, 9.5)
    assert np.array_equal(tags["index"], f64.detect(z, T, 9.5))
    _, (zr,), (tr,), _ = gpu_detector(pkg, x, rrc, 4, -4, 4, T, 9.5, ragged(x.size, T))
    assert np.array_equal(tr["index"], f64.detect(zr, T, 9.5))


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("switch", sorted(DETECTOR_SWITCHES))
def test_gpu_detector_three_channels(pkg, monkeypatch, switch):
    """n_channels = 3, each with its own content: per row, tags == detect() on that row's powers, one call and ragged"""
    set_switches(monkeypatch, DETECTOR_SWITCHES[switch])
    rows = []
    for c in range(3):
        x, rrc = sig.qa_syncword_stream(30000, [400 + 900 * c, 8000, 17000 + 100 * c, 26000], 0.003 * c, seed=60 + c)
        rows.append((0.5 * x + sig.awgn(x.size, 0.2 + 0.1 * c, 70 + c)).astype(np.complex64))
    X = np.stack(rows)
    for chunks in (None, ragged(X.shape[1], 31)):
        _, zs, ts, _ = gpu_detector(pkg, X, rrc, 4, -4, 4, 768, 9.5, chunks, rows=3)
        for c in range(3):
            assert ts[c].size >= 3 and np.array_equal(ts[c]["index"], f64.detect(zs[c], 768, 9.5)), c


@pytest.mark.gpu
@pytest.mark.timeout(60)
def test_gpu_time_threshold_outside_1_to_8192_is_refused(pkg):
    rrc = orc.unit_norm_rrc(4)[0]
    for T in (0, 8193):
        with pytest.raises(pkg.Gr4pmError, match="not built"):
            pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, time_threshold=T)
    for T in (1, 8192):
        pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, time_threshold=T, max_items=1 << 16)
