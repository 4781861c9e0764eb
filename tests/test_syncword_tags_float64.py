"""SyncwordDetection's tag VALUES against float64: amplitude, phase, freq, noise_power, esn0_db and time_est of every
tag within the bound that the raw values' own bounds allow (tests/_float64_ref.tag_tolerance), on every correlator form,
in one call and in ragged calls, where the record's pieces come from different places (call boundaries at the
detection, histories of many calls, several channels) and at 2 to 64 frequency bins.

Raw bars (derived in _float64_ref.gpu_raw_err): 6 * 2^-24 * A_b on the direct sum (z, left, right), 8 * 2^-24 * E_j on
the float-FFT powers (prev, next; and z, left, right behind k_tags_generic, which takes them from a float FFT of the
block), 8 + 16 on the noise power.  self_corr (hpp:161-164, a float sum at creation) is an input of output_tag(): the
tags are evaluated with the detector's own value, and that value is held to the float64 sum on its own."""
import numpy as np
import pytest

import _float64_ref as f64
import _oracle as orc
import _signals as sig
import test_syncword_float64 as base

EPS = f64.EPS32
PI_F = float(np.float32(np.pi))
T_DEFAULT, PT = 768, 12.0
SKIP_CAP = 0.10
pkg = base.pkg  # the module's GPU fixture


# ------------------------------------------------------------------------------------------------------- stimuli
def packet_plan(lo, hi):
    """the packets of one stream: interior bins at frac 0 / +0.3 / -0.3, carrier phases next to +-pi with frac of either
    sign (arg z and the corrected phase cross +-pi in both directions), a half-bin offset, each edge bin, one beyond the
    range, amplitudes 2^-10 .. 2^5, SNRs 30 .. 2 dB, and one under a stopband tone"""
    interior = list(range(lo + 1, hi))

    def pick(i):
        return interior[i % len(interior)] if interior else lo

    mid = pick(len(interior) // 2)
    P = [dict(bin=mid, frac=0.0, phase=0.7, a=0, snr=30.0),                      # starts at sample 0
         dict(bin=pick(0), frac=0.3, phase=np.pi - 0.01, a=5, snr=30.0),
         dict(bin=pick(1), frac=-0.3, phase=-np.pi + 0.01, a=-10, snr=25.0),
         dict(bin=pick(2), frac=-0.3, phase=np.pi - 0.01, a=-4, snr=20.0),
         dict(bin=pick(3), frac=0.3, phase=-np.pi + 0.01, a=2, snr=20.0),
         # (the parabola reads frac = 0.3 as 0.25: with these two the corrected phase leaves [-pi, pi) and the explicit
         # wrap of hpp:88-92 runs, once in each direction)
         dict(bin=pick(1), frac=0.3, phase=np.pi - 0.2, a=-1, snr=30.0),
         dict(bin=pick(2), frac=-0.3, phase=-np.pi + 0.2, a=1, snr=25.0),
         dict(bin=pick(0), frac=0.5, phase=1.9, a=0, snr=30.0),
         dict(bin=lo, frac=0.0, phase=-2.2, a=-2, snr=20.0)]
    if hi > lo:
        P += [dict(bin=hi, frac=0.0, phase=2.9, a=3, snr=15.0),
              dict(bin=hi, frac=0.7, phase=-0.4, a=0, snr=25.0)]                 # beyond the range
    P += [dict(bin=mid, frac=0.2, phase=0.3, a=-7, snr=10.0),
          dict(bin=pick(1), frac=-0.1, phase=-1.1, a=1, snr=2.0),               # esn0_db near 0
          dict(bin=mid, frac=0.1, phase=1.0, a=0, snr=25.0, tone=True)]
    for p in P:
        p["clean"] = bool(p["snr"] >= 20.0 and lo < p["bin"] < hi and abs(p["frac"]) <= 0.3 and not p.get("tone"))
    return P


def build_stream(plan, sps, rrc, L, seg_samples=6800, seed=1, tone_log2=None, first_at=0, count=None):
    segs = []
    for i, p in enumerate(plan[:count]):
        n_sym = seg_samples // sps
        amp = 2.0 ** p["a"]
        s = dict(n_sym=n_sym, loc=0 if i == 0 else n_sym // 2, cfo=(p["bin"] + p["frac"]) * np.pi / L,
                 phase=p["phase"], amp=amp, sigma=amp * 10.0 ** (-p["snr"] / 20.0), lead=first_at if i == 0 else 0)
        if p.get("tone") and tone_log2 is not None:
            s["tone"] = (amp * 2.0 ** tone_log2, (0.8 if sps >= 4 else 0.9) * np.pi)
        segs.append(s)
    segs.append(dict(n_sym=6000 // sps, loc=None, sigma=0.01))  # (the last packet's tag leaves with a later block)
    x, pos = sig.packet_segments(segs, sps, rrc, seed)
    return x, pos[:-1]


def oracle_tags(x, rrc, sps, lo, hi, N, T, pt, out=False):
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, lo, hi, fft_size=N, samples_per_symbol=sps,
                                time_threshold=T, power_threshold=pt)
    _, o, tags, zp, _ = ref.process(x, debug=True, tags_cap=1 << 14)
    return (tags, zp, o, ref._syncword_self_corr) if out else (tags, ref._syncword_self_corr)


def found(tags, positions, T):
    lag = set((tags["index"].astype(np.int64) - (2 * T + 1)).tolist())
    return [p is None or any(p + d in lag for d in (-1, 0, 1)) for p in positions]


class Stimulus:
    def __init__(self, x, positions, plan, settings, T=T_DEFAULT, pt=PT):
        self.x, self.positions, self.plan, self.T, self.pt = x, positions, plan, T, pt
        self.rrc, self.sps, self.lo, self.hi, self.N = settings
        self.s64 = f64.Stream64(x, *settings)
        self.oracle = None

    def clean_positions(self):
        return [p for p, q in zip(self.positions, self.plan) if q["clean"]]


_STIMULI = {}


def form_stimuli(form):
    """(main stream, the stream whose first packet starts at sample 1) of a form.  The tone's amplitude: the largest
    power of two (times the packet's) at which the CPU oracle still tags every packet"""
    if form not in _STIMULI:
        _, sps, rrc, lo, hi, N, L, _ = base.form_setup(form)
        plan = packet_plan(lo, hi)
        settings = (rrc, sps, lo, hi, N)
        tone = None
        for k in range(-6, 15):
            x, pos = build_stream(plan, sps, rrc, L, tone_log2=k)
            tags, _ = oracle_tags(x, rrc, sps, lo, hi, N, T_DEFAULT, PT)
            if not all(found(tags, pos, T_DEFAULT)):
                break
            tone = k
        assert tone is not None, "the oracle misses a packet without any tone"
        x, pos = build_stream(plan, sps, rrc, L, tone_log2=tone)
        main = Stimulus(x, pos, plan, settings)
        main.tone_log2 = tone
        x1, pos1 = build_stream(plan, sps, rrc, L, first_at=1, count=3)
        _STIMULI[form] = (main, Stimulus(x1, pos1, plan[:3], settings))
    return _STIMULI[form]


# ------------------------------------------------------------------------------------------------------- the check
class Stats:
    def __init__(self):
        self.ratio = {f: 0.0 for f in f64.FIELDS}
        self.pairs = self.skipped = self.tags = 0
        self.Cz = 0.0
        self.fail = []

    def line(self):
        r = ", ".join(f"{f} {v:.3f}" for f, v in self.ratio.items())
        return f"{self.tags} tags, {self.skipped}/{self.pairs} pairs skipped, C_z = {self.Cz:.2f}; max err / tol: {r}"


def check_tags(tags, st, raw_err, self_corr, label, floor=None, stats=None, cap=SKIP_CAP):
    """every tag of `tags` against float64 on the stimulus `st`; raw_err(raw) -> the raw bounds of the side under test.
    All failures of a run are reported together."""
    s = stats or Stats()
    lo, hi, H = st.lo, st.hi, 2 * st.T + 1
    nb = hi - lo + 1
    clean = set(st.clean_positions())
    seen_clean = set()
    for t in tags:
        pos = int(t["index"]) - H
        raw = f64.raw64(st.s64, pos)
        err = raw_err(raw)
        ez = np.broadcast_to(np.asarray(err["z"], dtype=np.float64), (nb,))
        b = int(t["freq_bin"]) - lo
        amps = np.abs(raw.z)
        order = np.argsort(-amps, kind="stable")
        best = int(order[0])
        if nb > 1:
            second = int(order[1])
            if amps[best] - amps[second] > 2.0 * max(ez[best], ez[second]):
                if b != best:
                    s.fail.append((label, pos, "freq_bin", b + lo, best + lo))
                    continue
            elif b not in (best, second):
                s.fail.append((label, pos, "freq_bin (near tie)", b + lo, (best + lo, second + lo)))
                continue
        elif b != 0:
            s.fail.append((label, pos, "freq_bin", b + lo, lo))
            continue
        ref = f64.tag64(raw, b, self_corr)
        tol, ill = f64.tag_tolerance(raw, b, err, self_corr)
        errs = f64.field_errors(t, ref)
        s.tags += 1
        is_clean = any(pos + d in clean for d in (-1, 0, 1))
        if is_clean:
            seen_clean.add(min(clean, key=lambda p: abs(p - pos)))
        for f in f64.FIELDS:
            s.pairs += 1
            if ill[f]:
                s.skipped += 1
                if is_clean:
                    s.fail.append((label, pos, f, "ill-conditioned on a clean packet"))
                continue
            if not errs[f] <= tol[f]:
                s.fail.append((label, pos, f, float(t[f]), ref[f], errs[f], tol[f]))
            elif tol[f] > 0:
                s.ratio[f] = max(s.ratio[f], errs[f] / tol[f])
        if not -PI_F <= float(t["phase"]) <= PI_F:
            s.fail.append((label, pos, "phase outside [-pi_f, pi_f]", float(t["phase"])))
        if not lo < lo + b < hi:
            if float(t["freq"]) != float(lo + b) * (np.pi / float(raw.L)):
                s.fail.append((label, pos, "freq of an edge bin", float(t["freq"])))
            # no interpolation: the tag holds z itself (behind finish_tag's sqrt and division)
            zt = float(t["amplitude"]) * raw.N * float(self_corr) * np.exp(1j * float(t["phase"]))
            s.Cz = max(s.Cz, abs(zt - raw.z[b]) / (EPS * raw.A[b]))
    if floor is not None and len(tags) < floor:
        s.fail.append((label, "tag count", len(tags), floor))
    if floor is not None and seen_clean != clean:
        s.fail.append((label, "clean packets without a tag", sorted(clean - seen_clean)))
    if s.pairs and s.skipped > cap * s.pairs:
        s.fail.append((label, "skip cap", s.skipped, s.pairs))
    return s


def oracle_check(st, label, floor=None):
    tags, sc = oracle_tags(st.x, st.rrc, st.sps, st.lo, st.hi, st.N, st.T, st.pt)
    s = check_tags(tags, st, f64.oracle_raw_err, sc, label, floor=len(st.positions) if floor is None else floor)
    print(f"\n[tags float64] oracle {label}: {s.line()}")
    assert not s.fail, s.fail
    return tags


def self_corr_bound(st, sc):
    """the float self-correlation (hpp:155-164: float sums of <= ceil(taps / sps) products per sample, then of L
    squares one after the other) against the float64 sum: (L + 4 ceil(taps / sps)) 2^-24 relative"""
    m = -(-st.rrc.size // st.sps)
    ref = st.s64.self_corr
    assert abs(float(sc) - ref) <= (st.s64.L + 4 * m) * EPS * ref, (sc, ref)


# ------------------------------------------------------------------------------------------------------- CPU
def test_direct_sum_equals_the_fft_form():
    """raw64's |z_b|^2 (time-domain sum) == the overlap-save power of that bin at that lag (zpow64's form) to 1e-12
    relative, at lags 0, 1, S - 1 and inside, for 2048 and 4096"""
    for form in ("w64_9bins", "c4096", "generic512"):
        main, _ = form_stimuli(form)
        S = main.s64.S
        for pos in (0, 1, S - 1, S, 3 * S + 77, main.positions[3], main.positions[3] + 1):
            raw = f64.raw64(main.s64, pos)
            scale = np.max(raw.p_bins)
            assert np.max(np.abs(np.abs(raw.z) ** 2 - raw.p_bins)) <= 1e-12 * scale, (form, pos)
        r = f64.zpow64(main.x[:6 * S + main.N], main.s64.tmpl, main.N, main.s64.L)
        for pos in (0, 5, S + 1, 4 * S - 1):
            raw = f64.raw64(main.s64, pos)
            assert abs(np.max(np.abs(raw.z) ** 2) - r.zpow[pos]) <= 1e-12 * r.zpow[pos]
            assert abs(raw.next - r.zpow[pos + 1]) <= 1e-12 * r.zpow[pos + 1]
            assert raw.prev == (0.0 if pos == 0 else f64.raw64(main.s64, pos - 1).p_bins.max())
        # and the function form on the plain stream
        a = f64.raw64(main.x, main.positions[2], main.rrc, main.sps, main.lo, main.hi, main.N)
        b = f64.raw64(main.s64, main.positions[2])
        assert np.array_equal(a.z, b.z) and a.noise == b.noise and a.prev == b.prev


def test_library_template_recipe_meets_the_three_roundings():
    """the library's time-domain templates restated in float32 (a float-accumulated syncword times a float phasor) and
    summed in double: |z - z64| <= 3 * 2^-24 * A_b, the template term of the local bound"""
    main, _ = form_stimuli("w64_9bins")
    rrc, sps, L = main.rrc, main.sps, main.s64.L
    sw = np.zeros(L, dtype=np.complex64)
    for j, sym in enumerate(sig.SYNCWORD):
        for k in range(rrc.size):
            sw[j * sps + k] = np.complex64(sw[j * sps + k] + np.complex64(sig.BPSK[sym] * rrc[k]))
    worst = 0.0
    for b in range(main.hi - main.lo + 1):
        incr = float(main.lo + b) * np.pi / float(L)
        phase, c, s = 0.0, np.empty(L, np.float32), np.empty(L, np.float32)
        for i in range(L):
            c[i], s[i] = np.float32(np.cos(phase)), np.float32(np.sin(phase))
            phase += incr
            phase += -2.0 * np.pi if phase >= np.pi else 2.0 * np.pi
        tr = (sw.real * c - sw.imag * s).astype(np.float32)
        ti = (sw.real * s + sw.imag * c).astype(np.float32)
        td = tr.astype(np.float64) + 1j * ti.astype(np.float64)
        for pos in main.positions[:6]:
            raw = f64.raw64(main.s64, pos)
            z = main.N * np.sum(main.s64.x[pos:pos + L] * np.conj(td))
            worst = max(worst, abs(z - raw.z[b]) / (EPS * raw.A[b]))
    print(f"\n[tags float64] float32 templates, double sum: C = {worst:.3f}")
    assert worst <= 3.0


def test_tag64_branches():
    """an edge bin: freq == bin * (pi / L) exactly, no interpolation; b == c: quad and time_est +0.5; a == b: -0.5; the
    corrected phase wraps into [-pi, pi)"""
    main, _ = form_stimuli("w64_9bins")
    raw = f64.raw64(main.s64, main.positions[1])
    L = raw.L
    for b, fb in ((0, main.lo), (raw.z.size - 1, main.hi)):
        t = f64.tag64(raw, b)
        assert t["freq"] == float(fb) * (np.pi / float(L))
        assert t["phase"] == float(np.angle(raw.z[b]))
        assert t["amplitude"] == float(np.sqrt(abs(raw.z[b]) ** 2) / (raw.N * raw.self_corr))
    fake = f64.Raw64(**raw.__dict__)
    fake.z = raw.z.copy()
    fake.z[5] = fake.z[4] * np.exp(0.3j)           # right == best
    fake.z[3] = 0.1 * fake.z[4]
    fake.prev, fake.next = 0.0, abs(fake.z[4]) ** 2  # a = 0, c == b
    t = f64.tag64(fake, 4)
    assert t["time_est"] == 0.5
    assert t["freq"] == float(main.lo + 4) * (np.pi / L) + 0.5 * (np.pi / L)
    fake.z[3], fake.z[5] = fake.z[4], 0.1 * fake.z[4]
    fake.prev, fake.next = fake.next, 0.0
    t = f64.tag64(fake, 4)
    assert t["time_est"] == -0.5 and t["freq"] == float(main.lo + 4) * (np.pi / L) - 0.5 * (np.pi / L)
    # wraps: arg z = pi - 0.01 with quad = -0.5 -> pi - 0.01 + pi/4 -> minus 2 pi; and the other way
    for arg, (l, r), want in ((np.pi - 0.01, (1.0, 0.1), np.pi - 0.01 + np.pi / 4 - 2 * np.pi),
                              (-np.pi + 0.01, (0.1, 1.0), -np.pi + 0.01 - np.pi / 4 + 2 * np.pi)):
        fake.z[4] = abs(raw.z[4]) * np.exp(1j * arg)
        fake.z[3], fake.z[5] = l * fake.z[4], r * fake.z[4]
        t = f64.tag64(fake, 4)
        assert abs(t["phase"] - want) < 1e-12 and -np.pi <= t["phase"] < np.pi
    # the stimulus crosses +-pi in both directions (arg z on the other side of the cut than the tag's phase)
    crossings = set()
    for pos, p in zip(main.positions, main.plan):
        raw = f64.raw64(main.s64, pos)
        b = int(np.argmax(np.abs(raw.z)))
        a0, a1 = float(np.angle(raw.z[b])), f64.tag64(raw, b)["phase"]
        if abs(a0 - a1) > np.pi:
            crossings.add(np.sign(a0))
    assert crossings == {-1.0, 1.0}


@pytest.mark.parametrize("form", sorted(base.FORMS))
def test_oracle_tags_within_the_float64_bound(form):
    """the CPU oracle on every form's stimulus: all packets tagged, every field within tag_tolerance of tag64 under the
    oracle's raw bounds, at most 10 % of the (tag, field) pairs ill-conditioned and none on the clean packets"""
    main, shifted = form_stimuli(form)
    assert main.x.size <= 102000 and main.positions[0] == 0 and shifted.positions[0] == 1
    tags = oracle_check(main, f"{form} (tone 2^{main.tone_log2})")
    assert all(found(tags, main.positions, main.T))
    oracle_check(shifted, f"{form} shifted")


# ------------------------------------------------------------------------------------------------------- GPU
def make_sd(pkg, st, rows=1, max_items=None):
    return pkg.SyncwordDetection(st.rrc, sig.SYNCWORD, sig.BPSK, st.lo, st.hi, fft_size=st.N,
                                 samples_per_symbol=st.sps, time_threshold=st.T, power_threshold=st.pt,
                                 n_channels=rows, max_items=max_items or st.x.shape[-1])


def gpu_check(pkg, st, label, local, chunks_list, floor=None, zpow_ref=None):
    """the stimulus in one call (None) and in each call pattern: the bounds on every tag of every run, the same tags
    (index, freq_bin) in every run for the items it consumed"""
    floor = len(st.positions) - 1 if floor is None else floor
    first = None
    for chunks in chunks_list:
        sd = make_sd(pkg, st)
        self_corr_bound(st, sd._syncword_self_corr)
        (zg,), (tags,), n = base.gpu_calls(sd, st.x, chunks)
        lab = f"{label} {'one call' if chunks is None else f'{len(chunks)} calls'}"
        s = check_tags(tags, st, lambda raw: f64.gpu_raw_err(raw, local), sd._syncword_self_corr, lab,
                       floor=floor if chunks is None else None)
        print(f"\n[tags float64] {lab}: {s.line()}")
        assert not s.fail, s.fail
        if zpow_ref is not None:
            base.check_bound(zg, zpow_ref, tags, st.lo, st.T)
        if first is None:
            first = tags
        else:
            assert tags.size >= min(floor, first.size) - 1
            assert np.array_equal(tags["index"], first["index"][:tags.size]), lab
            assert np.array_equal(tags["freq_bin"], first["freq_bin"][:tags.size]), lab
    return first


def is_local(form):
    """k_tags sums the detection's lag directly; k_tags_generic (fft_size != 2048, but for k_correlate_4096) does not"""
    env, _, _, _, _, N, _, _ = base.form_setup(form)
    return N == 2048 or (N == 4096 and env.get("GR4PM_CORRELATOR") != "radix2")


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("form", sorted(base.FORMS))
def test_gpu_tag_values_within_the_float64_bound(pkg, monkeypatch, form):
    """every correlator form, one call and ragged calls, the main stream and the one whose first packet starts at
    sample 1: every float field of every tag within tag_tolerance of tag64 at the bin the GPU chose; freq_bin float64's
    wherever that leads by more than twice the bound, else one of the best two; -pi_f <= phase <= pi_f; the packet
    under the stopband tone (2^10 .. 2^14 times the packet) meets the LOCAL bound on amplitude and phase.  Measured on MI355X, the
    largest error / tolerance of any field: 0.11 (amplitude, w64_3bins); phase <= 0.09, freq <= 0.06, noise_power <= 0.04,
    esn0_db <= 0.05, time_est <= 0.04.  C_z = |z - z64| / (2^-24 A_b), read back from the edge-bin tags (so behind
    finish_tag's sqrt and division): w64_9bins / wave / pair 0.70, w64_3bins 1.99, w64_one / w64_one_off 1.63,
    long_stride 1.75, c4096 0.53; behind the float FFT of k_tags_generic: c4096_radix2 0.56, generic1024 1.83,
    generic512 2.15.  Ill-conditioned pairs: c4096 20 / 342, c4096_radix2 24 / 342 (tags on plain data under the
    1025-tap template), none elsewhere"""
    env = base.form_setup(form)[0]
    base.set_switches(monkeypatch, env)
    main, shifted = form_stimuli(form)
    local = is_local(form)
    gpu_check(pkg, main, form, local, [None, base.ragged(main.x.size, 17, main.N)])
    gpu_check(pkg, shifted, form + " shifted", local, [None, [main.N + 3 * main.s64.S, 1 << 20]])


# --------------------------------------------------------------------- where the record's pieces come from
def boundary_stream(seed=5):
    """default form; packets whose detection lag is 0, 1, S - 2, S - 1 of blocks 4, 9, 14, 19 (by construction)"""
    _, sps, rrc, lo, hi, N, L, S = base.form_setup("w64_9bins")
    blocks, lags = (4, 9, 14, 19), (0, 1, S - 2, S - 1)
    segs, at = [], 0
    for i, (j, k) in enumerate(zip(blocks, lags)):
        target = j * S + k
        n_sym = 1900
        loc = 900
        lead = target - at - loc * sps
        assert lead >= 0
        segs.append(dict(n_sym=n_sym, loc=loc, lead=lead, cfo=(i - 1.7) * np.pi / L, phase=0.5 + i, amp=2.0 ** (2 - 2 * i),
                         sigma=2.0 ** (2 - 2 * i) * (0.03 + 0.04 * i)))
        at += lead + n_sym * sps
    x, pos = sig.packet_segments(segs, sps, rrc, seed)
    assert pos == [j * S + k for j, k in zip(blocks, lags)]
    plan = [dict(clean=True)] * 4
    return Stimulus(x, pos, plan, (rrc, sps, lo, hi, N)), blocks


def calls_with_boundaries(boundaries, N, S):
    """call sizes N + k S whose consumed items end at the given block indices; a last call takes the rest"""
    sizes, at = [], 0
    for b in sorted(set(boundaries)):
        sizes.append(N + (b - at - 1) * S)
        at = b
    return sizes + [1 << 20]


def boundary_patterns(blocks, N, S):
    at_pos = calls_with_boundaries([b for j in blocks for b in (j, j + 1)], N, S)   # at pos (lag 0), pos + 1 (S - 1)
    later = calls_with_boundaries([j + 2 for j in blocks], N, S)                    # one block later
    return [None, at_pos, later]


def test_oracle_on_the_boundary_stream():
    st, _ = boundary_stream()
    tags = oracle_check(st, "boundary stream")
    assert all(found(tags, st.positions, st.T))
    assert sorted(p % st.s64.S for p in st.positions) == [0, 1, st.s64.S - 2, st.s64.S - 1]


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_gpu_tags_at_call_boundaries(pkg, monkeypatch):
    """detections at lag 0, 1, S - 2, S - 1 of a block, calls of N + k S items so that a call ends exactly at pos (prev
    from the z carry), at pos + 1 (z from carried samples, noise from the carried slot) and one block later: every
    field within the float64 bound in every pattern.  Measured on MI355X: error / tolerance <= 0.07 (amplitude)"""
    base.set_switches(monkeypatch, {})
    st, blocks = boundary_stream()
    gpu_check(pkg, st, "boundaries", True, boundary_patterns(blocks, st.N, st.s64.S), floor=4)


def long_history_stream(T, seed=8):
    """packets 18 000 samples apart, the noise level changing every 1500 samples (a neighbouring block's noise power is
    visibly wrong)"""
    _, sps, rrc, lo, hi, N, L, S = base.form_setup("w64_9bins")
    segs = [dict(n_sym=4500, loc=2250, cfo=(0.3 * i - 0.8) * np.pi / L, phase=1.0 - i, amp=1.0) for i in range(5)]
    x, pos = sig.packet_segments(segs, sps, rrc, seed)
    x = np.concatenate([x, np.zeros(9000, np.complex64)])
    rng = np.random.default_rng(seed)
    sigma = np.repeat(rng.uniform(0.02, 0.3, x.size // 1500 + 1), 1500)[:x.size].astype(np.float32)
    x = (x + sigma * sig.awgn(x.size, 1.0, seed + 1)).astype(np.complex64)
    plan = [dict(clean=True)] * 5
    return Stimulus(x, pos, plan, (rrc, sps, -2, 2, N), T=T, pt=9.5)


@pytest.mark.parametrize("T", [1000, 8192])
def test_oracle_on_the_long_history_stream(T):
    st = long_history_stream(T)
    assert st.x.size <= 100000
    oracle_check(st, f"long history T = {T}", floor=4)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("T", [1000, 8192])
def test_gpu_tags_with_a_history_of_many_calls(pkg, monkeypatch, T):
    """hist = 2T + 1 = 16385 (9.4 S) and 2001, the stream in 2048-item calls (one block each): the detection lies many
    calls back, its samples come from the sample carry and its block's noise power was never left behind.  Measured on
    MI355X: error / tolerance <= 0.06 (amplitude), noise_power 0.012 / 0.008"""
    base.set_switches(monkeypatch, {})
    st = long_history_stream(T)
    sd = make_sd(pkg, st, max_items=1 << 14)
    (_,), (tags,), _ = base.gpu_calls(sd, st.x, [2048] * (st.x.size // st.s64.S + 2))
    s = check_tags(tags, st, f64.gpu_raw_err, sd._syncword_self_corr, f"T = {T}", floor=4)
    print(f"\n[tags float64] long history T = {T}: {s.line()}")
    assert not s.fail, s.fail


def channel_streams():
    _, sps, rrc, lo, hi, N, L, _ = base.form_setup("w64_9bins")
    out = []
    for c, k in enumerate((-12, 0, 8)):
        plan = packet_plan(lo, hi)[1 + c:6 + c]
        segs = [dict(n_sym=2000, loc=700 + 150 * c + 40 * i, cfo=(p["bin"] + p["frac"]) * np.pi / L, phase=p["phase"],
                     amp=2.0 ** k, sigma=2.0 ** k * 10.0 ** (-p["snr"] / 20.0)) for i, p in enumerate(plan)]
        x, pos = sig.packet_segments(segs, sps, rrc, 30 + c)
        out.append(Stimulus(x, pos, plan, (rrc, sps, lo, hi, N)))
    return out


def test_oracle_on_the_channel_streams():
    for c, st in enumerate(channel_streams()):
        oracle_check(st, f"channel {c}")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_gpu_tags_of_three_channels(pkg, monkeypatch):
    """n_channels = 3 at 2^-12, 1, 2^8, each row with its own packets: the same bounds per row, one call and ragged.
    Measured on MI355X: error / tolerance <= 0.10 (phase, channel 1)"""
    base.set_switches(monkeypatch, {})
    sts = channel_streams()
    X = np.stack([st.x for st in sts])
    for chunks in (None, base.ragged(X.shape[1], 41)):
        sd = make_sd(pkg, sts[0], rows=3, max_items=X.shape[1])
        _, ts, _ = base.gpu_calls(sd, X, chunks, rows=3)
        for c, st in enumerate(sts):
            s = check_tags(ts[c], st, f64.gpu_raw_err, sd._syncword_self_corr, f"channel {c}",
                           floor=len(st.positions) - 1 if chunks is None else None)
            print(f"\n[tags float64] channel {c} {'one call' if chunks is None else 'ragged'}: {s.line()}")
            assert not s.fail, s.fail


# --------------------------------------------------------------------- 2 to 64 frequency bins
BIN_RANGES = {2: (0, 1), 4: (-1, 2), 5: (-3, 1), 9: (-2, 6), 10: (-3, 6), 18: (-5, 12), 19: (-12, 6), 28: (-9, 18),
              64: (-40, 23)}
# (environment, fft_size, rrc) of the forms run at 10 and 19 bins
BIN_FORMS = {"wave": ({"GR4PM_CORRELATOR": "wave"}, 2048, None), "pair": ({"GR4PM_CORRELATOR": "pair"}, 2048, None),
             "c4096": ({}, 4096, (4, 1024)), "generic1024": ({}, 1024, None),
             "variant0": ({"GR4PM_W64_VARIANT": "0"}, 2048, None),
             "variant65536": ({"GR4PM_W64_VARIANT": "65536"}, 2048, None)}
_BIN_STIMULI = {}


def bins_stimulus(n_bins, N=2048, rr=None):
    """one packet in bin index 0, n_bins - 1, 8, 9, 10, 17, 18 and the middle (those that exist), 25 dB"""
    key = (n_bins, N, rr)
    if key not in _BIN_STIMULI:
        lo, hi = BIN_RANGES[n_bins]
        assert hi - lo + 1 == n_bins
        rrc = orc.unit_norm_rrc(4)[0] if rr is None else base.short_rrc(*rr)
        L = base.template_length(rrc, 4)
        idx = sorted({i for i in (0, n_bins - 1, 8, 9, 10, 17, 18, n_bins // 2) if i < n_bins})
        plan = []
        for m, i in enumerate(idx):
            edge = i in (0, n_bins - 1)
            plan.append(dict(bin=lo + i, frac=0.0 if edge else (0.2, -0.25, 0.1)[m % 3], phase=0.9 * m - 2.5,
                             a=(0, -3, 4)[m % 3], snr=25.0, clean=not edge))
        seg = 8000 if N <= 2048 else 11000
        segs = [dict(n_sym=seg // 4, loc=seg // 8, cfo=(p["bin"] + p["frac"]) * np.pi / L, phase=p["phase"],
                     amp=2.0 ** p["a"], sigma=2.0 ** p["a"] * 10.0 ** (-p["snr"] / 20.0)) for p in plan]
        x, pos = sig.packet_segments(segs, 4, rrc, 100 + n_bins)
        _BIN_STIMULI[key] = Stimulus(x, pos, plan, (rrc, 4, lo, hi, N), pt=9.5)
    return _BIN_STIMULI[key]


@pytest.mark.parametrize("n_bins", sorted(BIN_RANGES))
def test_oracle_at_every_bin_count(n_bins):
    st = bins_stimulus(n_bins)
    tags = oracle_check(st, f"{n_bins} bins")
    assert all(found(tags, st.positions, st.T))
    by_pos = {int(t["index"]) - (2 * st.T + 1): int(t["freq_bin"]) for t in tags}
    assert [by_pos[p] for p in st.positions] == [q["bin"] for q in st.plan]


def run_bins(pkg, st, label, local):
    """against the oracle: pass-through bit for bit, index and freq_bin exact, assert_tags_match, the powers as the
    settings matrix holds them; against float64: the powers' bound and the tags' bounds, one call and ragged"""
    from test_gpu_parity import assert_tags_match
    ref_tags, ref_zpow, ref_out, _ = oracle_tags(st.x, st.rrc, st.sps, st.lo, st.hi, st.N, st.T, st.pt, out=True)
    sd = make_sd(pkg, st)
    status, out, tags, n = sd.process_bulk(base.dev(st.x), tags_cap=8192)
    assert status == 0 and n == ref_out.size
    assert np.array_equal(base.bits(out.cpu().numpy()), base.bits(ref_out))
    assert tags.size >= len(st.positions)
    assert_tags_match(tags, ref_tags)
    zg = sd.last_zpow(n).cpu().numpy()[0]
    assert np.max(np.abs(zg - ref_zpow)) / np.max(ref_zpow) < 5e-6
    r = f64.zpow64(st.x, st.s64.tmpl, st.N, st.s64.L, chunk_blocks=4)
    first = gpu_check(pkg, st, label, local, [None, base.ragged(st.x.size, 29, st.N)], floor=len(st.positions),
                      zpow_ref=r)
    assert np.array_equal(first["index"], ref_tags["index"]) and np.array_equal(first["freq_bin"], ref_tags["freq_bin"])


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_bins", sorted(BIN_RANGES))
def test_gpu_bin_counts(pkg, monkeypatch, n_bins):
    """2 .. 64 bins on asymmetric ranges, the default form: k_tags' second and later bin groups (bin0 = 9, 18, ...), the
    padding of a partial last group, ten and more templates in the correlator, and two edge bins without an interior
    one.  Measured on MI355X: every count runs; error / tolerance <= 0.15 (amplitude, 2 bins), C_z 0.51 .. 2.86"""
    base.set_switches(monkeypatch, {})
    monkeypatch.delenv("GR4PM_W64_VARIANT", raising=False)
    run_bins(pkg, bins_stimulus(n_bins), f"{n_bins} bins", True)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_bins", [10, 19])
@pytest.mark.parametrize("form", sorted(BIN_FORMS))
def test_gpu_bin_counts_on_the_other_forms(pkg, monkeypatch, form, n_bins):
    """10 and 19 templates on the wave, pair, 4096, generic and the two bit-identical w64 variants: a form that cannot
    hold that many refuses at create with a Gr4pmError that names the limit (recorded in the output); one that runs
    meets every bound.  On MI355X no form refuses: all twelve run and meet the bounds (error / tolerance <= 0.12)"""
    env, N, rr = BIN_FORMS[form]
    base.set_switches(monkeypatch, {})
    monkeypatch.delenv("GR4PM_W64_VARIANT", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st = bins_stimulus(n_bins, N, rr)
    try:
        make_sd(pkg, st)
    except pkg.Gr4pmError as e:
        assert "max" in str(e) and "bins" in str(e), str(e)
        print(f"\n[tags float64] {form} refuses {n_bins} bins: {e}")
        return
    run_bins(pkg, st, f"{form} {n_bins} bins", N != 1024)
