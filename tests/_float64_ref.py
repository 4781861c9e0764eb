"""Float64 restatement of SyncwordDetection's correlator and the exact decision loop on a given power sequence.

Test infrastructure only (tests/test_syncword_float64.py).  The correlator part answers "how close is a float32
correlator to the exact overlap-save powers": its error is bounded by the block's energy, not by each output, so
zpow64() returns the per-block scale E_j = ||FFT64(x[j:j+N])|| * max_b ||T_b|| next to the powers.  detect() restates
the decision loop (syncword_detection.hpp:267-343, orc_sd_process) on powers it is given, so that the detector's
decisions can be held exactly to the reference without FFT rounding in the way."""
import numpy as np

import _signals as sig

EPS32 = 2.0 ** -24


def syncword_samples64(rrc, sps, syncword=sig.SYNCWORD, constellation=sig.BPSK):
    """hpp:155-160: the syncword's symbols through the RRC interpolator, in float64"""
    rrc = np.asarray(rrc, dtype=np.float32).astype(np.float64)
    sym = np.asarray(constellation, dtype=np.complex64).astype(np.complex128)[np.asarray(syncword)]
    up = np.zeros((sym.size - 1) * sps + 1, dtype=np.complex128)
    up[::sps] = sym
    return np.convolve(up, rrc)


def shifted64(rrc, sps, lo, hi, syncword=sig.SYNCWORD, constellation=sig.BPSK):
    """hpp:166-182: per frequency bin b in [lo, hi] the frequency-shifted syncword s_b[n], n < L, in float64.
    The phase walks in double with the reference's wrap quirk (`else if (phase < kPi)`: every step wraps by 2 pi),
    which moves the rounding of cos / sin, not their value."""
    sw = syncword_samples64(rrc, sps, syncword, constellation)
    L = sw.size
    out = np.empty((hi - lo + 1, L), dtype=np.complex128)
    for b, freq_bin in enumerate(range(lo, hi + 1)):
        incr = float(freq_bin) * np.pi / float(L)
        phases = np.empty(L)
        phase = 0.0
        for i in range(L):
            phases[i] = phase
            phase += incr
            if phase >= np.pi:
                phase -= 2.0 * np.pi
            elif phase < np.pi:  # sic, hpp:179
                phase += 2.0 * np.pi
        out[b] = sw * (np.cos(phases) + 1j * np.sin(phases))
    return out


def templates64(rrc, sps, lo, hi, N, syncword=sig.SYNCWORD, constellation=sig.BPSK):
    """hpp:166-189: per frequency bin b in [lo, hi] the conjugated spectrum of the shifted syncword, in float64"""
    td = shifted64(rrc, sps, lo, hi, syncword, constellation)
    L = td.shape[1]
    if L > N:
        raise ValueError("template longer than fft_size")
    shifted = np.zeros((td.shape[0], N), dtype=np.complex128)
    shifted[:, :L] = td
    return np.conj(np.fft.fft(shifted, axis=1))


def lag_index(N, S):
    """hpp:296: lag k of a block reads the correlation at 0 for k = 0 and at N - k otherwise"""
    k = np.arange(S)
    return np.where(k == 0, 0, N - k)


class Zpow64:
    """float64 overlap-save powers of a stream: zpow (max over bins), bin (first best bin), gap (amplitude of the best
    bin minus that of the second, inf with one bin), E (per block), all per lag except E"""

    def __init__(self, zpow, bins, gap, E, S):
        self.zpow, self.bins, self.gap, self.E, self.S = zpow, bins, gap, E, S

    def E_per_lag(self):
        return np.repeat(self.E, self.S)


def zpow64(x, tmpl, N, L, chunk_blocks=64):
    """the correlator in float64 on x (complex64, taken exactly): blocks j * S, S = N - L + 1, while j * S + N <= x.size
    (hpp:238), bins as templates64() returns them"""
    x = np.asarray(x, dtype=np.complex64).astype(np.complex128)
    S = N - L + 1
    n_blocks = (x.size - N) // S + 1 if x.size >= N else 0
    zi = lag_index(N, S)
    tnorm = float(np.max(np.linalg.norm(tmpl, axis=1)))
    nb = tmpl.shape[0]
    zpow = np.empty(n_blocks * S)
    bins = np.empty(n_blocks * S, dtype=np.int32)
    gap = np.full(n_blocks * S, np.inf)
    E = np.empty(n_blocks)
    for c0 in range(0, n_blocks, chunk_blocks):
        c1 = min(c0 + chunk_blocks, n_blocks)
        idx = (np.arange(c0, c1) * S)[:, None] + np.arange(N)[None, :]
        X = np.fft.fft(x[idx], axis=1)                                   # [blocks, N]
        E[c0:c1] = np.linalg.norm(X, axis=1) * tnorm
        corr = np.fft.fft(X[:, None, :] * tmpl[None, :, :], axis=2)       # [blocks, bins, N] (forward, hpp:250)
        p = np.abs(corr[:, :, zi]) ** 2                                  # [blocks, bins, S]
        best = np.argmax(p, axis=1)                                      # first of equal maxima (hpp:300 '>')
        sl = slice(c0 * S, c1 * S)
        zpow[sl] = np.take_along_axis(p, best[:, None, :], axis=1)[:, 0, :].ravel()
        bins[sl] = best.ravel()
        if nb > 1:
            amp = np.sqrt(np.sort(p, axis=1))
            gap[sl] = (amp[:, -1, :] - amp[:, -2, :]).ravel()
    return Zpow64(zpow, bins, gap, E, S)


def _as_stream(zpow):
    if isinstance(zpow, (list, tuple)):
        return np.concatenate([np.asarray(z, dtype=np.float32) for z in zpow]) if len(zpow) else np.zeros(0, np.float32)
    return np.asarray(zpow, dtype=np.float32)


def resets(zpow, T, loop=None):
    """hpp:269-282, 292-295: the (best_idx, curr_idx) pairs at which the loop runs its median test, curr_idx < len.
    Where they fall depends on the powers and T only, never on power_threshold.  best / best_idx follow the strict '>'
    (the first of equal maxima) and restart at every reset (best = 0, best_idx = curr_idx)."""
    z = _as_stream(zpow)
    n, T = z.size, int(T)
    out = []
    if loop if loop is not None else T < 32:  # the loop itself, sample by sample
        best, b = 0.0, 0
        zl = z.tolist()
        for c in range(n):
            if c - b > T:
                out.append((b, c))
                best, b = 0.0, c
            if zl[c] > best:
                best, b = zl[c], c
        return out
    # From best_idx b the running maximum ends, inside (b, b + T], at the window's first maximum if that exceeds z[b]
    # (each step of the way stays within T of the one before, so no reset falls between); otherwise the reset falls at
    # b + T + 1, where b starts again.  Two jumps cover at least T + 1 items.
    b = 0
    while True:
        w = z[b + 1:b + T + 1]
        if w.size == 0:
            break
        m = int(np.argmax(w))
        if w[m] > z[b]:
            b = b + 1 + m
            continue
        c = b + T + 1
        if c >= n:
            break
        out.append((b, c))
        b = c
    return out


def history_below(zpow, c, T, thr):
    """hpp:273-278: how many of the 2T + 1 powers before curr_idx c lie below thr (zeros before the stream: the
    history starts as default items)"""
    z = _as_stream(zpow)
    H = 2 * int(T) + 1
    h = z[max(c - H, 0):c]
    return int(np.count_nonzero(h < thr)) + (H - h.size if np.float32(0) < thr else 0)


def history_values(zpow, c, T):
    z = _as_stream(zpow)
    H = 2 * int(T) + 1
    h = z[max(c - H, 0):c]
    return np.concatenate([np.zeros(H - h.size, np.float32), h])


def detect(zpow, T, power_threshold, loop=None):
    """hpp:267-343 on the power sequence `zpow` (float32; a list of arrays = consecutive calls): the tag indices as the
    ABI reports them, best_idx + 2T + 1 (hpp:283, the output delay), for the items consumed.  At each reset
    thr = best / power_threshold in float32, below counts '<', and the test passes when 2 * below >= 2T + 1."""
    z = _as_stream(zpow)
    H = 2 * int(T) + 1
    pt = np.float32(power_threshold)
    tags = []
    for b, c in resets(z, T, loop):
        thr = np.float32(z[b] / pt)
        if 2 * history_below(z, c, T, thr) >= H and b + H < z.size:
            tags.append(b + H)
    return np.array(tags, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ the tag's values
FIELDS = ("amplitude", "phase", "freq", "noise_power", "esn0_db", "time_est")


class Stream64:
    """a stream and one detector setting in float64: the time-domain templates s_b, their spectra, and the overlap-save
    blocks' powers on demand (one block is a few transforms; they are kept)"""

    def __init__(self, x, rrc, sps, lo, hi, N):
        self.x = np.asarray(x, dtype=np.complex64).astype(np.complex128)
        self.rrc, self.sps, self.lo, self.hi, self.N = np.asarray(rrc, dtype=np.float32), int(sps), int(lo), int(hi), int(N)
        self.td = shifted64(self.rrc, sps, lo, hi)
        self.L = self.td.shape[1]
        self.S = self.N - self.L + 1
        self.tmpl = templates64(self.rrc, sps, lo, hi, N)
        self.tnorm = float(np.max(np.linalg.norm(self.tmpl, axis=1)))
        self.snorm = np.linalg.norm(self.td, axis=1)
        self.self_corr = float(np.sum(np.abs(syncword_samples64(self.rrc, sps)) ** 2))  # hpp:161-164
        self._zi = lag_index(self.N, self.S)
        self._blocks = {}

    def block(self, j):
        """(powers [bins, S], ||FFT64(block)||, unnormalised noise sum S64) of block j (it must lie inside the stream)"""
        if j not in self._blocks:
            seg = self.x[j * self.S:j * self.S + self.N]
            if seg.size < self.N:
                raise IndexError("block past the end of the stream")
            X = np.fft.fft(seg)
            corr = np.fft.fft(X[None, :] * self.tmpl, axis=1)
            p = np.abs(corr[:, self._zi]) ** 2
            S64 = float(np.sum(np.abs(X[self.N // 4:3 * self.N // 4]) ** 2))
            self._blocks[j] = (p, float(np.linalg.norm(X)), S64)
        return self._blocks[j]

    def power(self, pos):
        """(zpow64, E_j) of the item at stream position pos; (0, 0) before the stream (hpp: default history items)"""
        if pos < 0:
            return 0.0, 0.0
        j = pos // self.S
        p, xn, _ = self.block(j)
        return float(np.max(p[:, pos - j * self.S])), xn * self.tnorm


class Raw64:
    """what output_tag() reads for the detection at `pos`, exactly: z [bins] (complex), A [bins] (each bin's local
    scale), p_bins [bins] (|z|^2 by the FFT form, for cross-checks), prev / next (powers at pos -+ 1) with E_prev /
    E_next, E (the block's), noise (hpp:257-265), X_norm = ||FFT64(block)||, S64 (the unnormalised noise sum)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def raw64(x, pos, rrc=None, sps=None, lo=None, hi=None, N=None):
    """For a detection at stream position pos (tag index - (2T + 1)):
      z_b = N * sum_n x[pos + n] conj(s_b[n]) for every bin, from the float64 time-domain templates (no FFT);
      A_b = N * ||x[pos:pos+L]||_2 * ||s_b||_2;
      the powers at pos - 1 and pos + 1 (0 before the stream) from the FFT form, with E_j of the block each lies in;
      the noise power of the block containing pos, sum_{k=N/4}^{3N/4-1} |FFT64(block)_k|^2 / ((N/2) N).
    x may be a Stream64 (then the settings are its own)."""
    s = x if isinstance(x, Stream64) else Stream64(x, rrc, sps, lo, hi, N)
    pos = int(pos)
    seg = s.x[pos:pos + s.L]
    if seg.size < s.L:
        raise IndexError("detection past the end of the stream")
    z = s.N * (np.conj(s.td) @ seg)
    A = s.N * float(np.linalg.norm(seg)) * s.snorm
    j = pos // s.S
    p, xn, S64 = s.block(j)
    prev, E_prev = s.power(pos - 1)
    nxt, E_next = s.power(pos + 1)
    return Raw64(pos=pos, z=z, A=A, p_bins=p[:, pos - j * s.S].copy(), prev=prev, next=nxt, E_prev=E_prev,
                 E_next=E_next, E=xn * s.tnorm, noise=S64 / (float(s.N // 2) * float(s.N)), X_norm=xn, S64=S64,
                 N=s.N, L=s.L, sps=s.sps, lo=s.lo, hi=s.hi, self_corr=s.self_corr)


def _clamp(v, lo, hi):
    """std::clamp: a NaN passes through"""
    return lo if v < lo else hi if hi < v else v


def _tag_core(q, meta, exact=True):
    """output_tag() (hpp:56-115) on amplitudes q = (|z|, arg z, sqrt left, sqrt right, sqrt prev, sqrt next,
    sqrt noise).  exact = False leaves out the two clamps and the phase wrap (for the sensitivities: a clamp only ever
    shrinks a difference, and phases are compared modulo 2 pi)."""
    zmag, zarg, l, r, pv, nx, n = (np.float64(v) for v in q)
    bin_, lo, hi, L, N, sps, self_corr = meta
    fb = lo + bin_
    spacing = np.pi / float(L)
    freq = float(fb) * spacing
    phase = zarg
    b = zmag * zmag
    with np.errstate(all="ignore"):
        if lo < fb < hi:
            a, c = l * l, r * r
            quad = (c - a) / (2.0 * (2.0 * b - (a + c)))
            if exact:
                quad = _clamp(quad, -0.5, 0.5)
            dfreq = quad * spacing
            freq = freq + dfreq
            phase = phase - dfreq * 0.5 * float(L)
            if exact:
                if phase >= np.pi:
                    phase -= 2.0 * np.pi
                elif phase < -np.pi:
                    phase += 2.0 * np.pi
            power = b + (c - a) * (c - a) / (16.0 * (b - 0.5 * (a + c)))
        else:
            power = b
        amp = np.sqrt(power) / (float(N) * self_corr)
        spow = amp * amp * self_corr
        esn0 = 10.0 * np.log10((spow * float(sps)) / (n * n * float(L)))
        a, c = pv * pv, nx * nx
        t = (c - a) / (2.0 * (2.0 * b - (a + c)))
        if exact:
            t = _clamp(t, -0.5, 0.5)
    return dict(amplitude=float(amp), phase=float(phase), freq=float(freq), noise_power=float(n * n),
                esn0_db=float(esn0), time_est=float(t))


def _q_meta(raw, bin_, self_corr):
    nb = raw.z.size
    z = raw.z[bin_]
    l = abs(raw.z[bin_ - 1]) if bin_ > 0 else 0.0        # hpp:329-333
    r = abs(raw.z[bin_ + 1]) if bin_ < nb - 1 else 0.0   # hpp:334-338
    q = [abs(z), float(np.angle(z)), l, r, np.sqrt(raw.prev), np.sqrt(raw.next), np.sqrt(raw.noise)]
    meta = (int(bin_), raw.lo, raw.hi, raw.L, raw.N, raw.sps, raw.self_corr if self_corr is None else float(self_corr))
    return q, meta


def tag64(raw, bin_, self_corr=None):
    """output_tag() (hpp:56-115) in float64 for the GIVEN bin index (0-based): the edge-bin branch, both clamps, the
    phase correction and its wrap into [-pi, pi).  self_corr: the detector's own constant (hpp:161-164 defines it as a
    float sum; it is an input of output_tag(), held on its own by the tests), default the float64 sum."""
    q, meta = _q_meta(raw, bin_, self_corr)
    return _tag_core(q, meta)


def ulp32(v):
    return float(np.spacing(np.float32(abs(v)))) if np.isfinite(v) else 0.0


def gpu_raw_err(raw, local=True):
    """Bounds on what the library's tag kernels hand to finish_tag(), each in amplitude (sqrt) form.
    z, left, right -- k_tags' direct sum in double (local = True): 6 * 2^-24 * A_b.  The library's time-domain
      templates are float32: a float32 syncword times a float32 phasor, up to three roundings of 2^-24 relative per
      template sample, so the sum is off by at most 3 * 2^-24 * N sum |x||s| <= 3 * 2^-24 * A_b (Cauchy-Schwarz); the
      cast of the two components to float adds sqrt(2) * 2^-24 |z| <= sqrt(2) * 2^-24 * A_b; the double accumulation
      is negligible; 3 + sqrt(2) rounds up to 6.  k_tags_generic takes z, left and right from a float FFT of the block
      (local = False): the transform bound 8 * 2^-24 * E_j that the powers test holds.
    prev, next -- the float-FFT power row: 8 * 2^-24 * E_j of the block each lies in.
    noise -- (8 * 2^-24 * ||FFT64(block)|| + 16 * 2^-24 * sqrt(S64)) / sqrt((N/2) N): the transform bound on the
      half-spectrum vector (triangle inequality), and a float sum of N/2 non-negative terms in a tree of depth <= 12."""
    ez = 6.0 * EPS32 * raw.A if local else np.full(raw.z.size, 8.0 * EPS32 * raw.E)
    return dict(z=ez, prev=8.0 * EPS32 * raw.E_prev, next=8.0 * EPS32 * raw.E_next,
                noise=(8.0 * EPS32 * raw.X_norm + 16.0 * EPS32 * np.sqrt(raw.S64)) / np.sqrt((raw.N // 2) * float(raw.N)))


def oracle_raw_err(raw):
    """The CPU oracle takes every value from its float FFT: 2 * 2^-24 * E_j (the bar its powers are held to) for z,
    left, right, prev, next.  Its noise power is a float sum of N/2 non-negative terms ONE AFTER THE OTHER: relative
    error at most (N/2) 2^-24 of the sum, (N/4) 2^-24 sqrt(S64) in sqrt form, behind the transform's 2 * 2^-24 ||X||."""
    return dict(z=np.full(raw.z.size, 2.0 * EPS32 * raw.E), prev=2.0 * EPS32 * raw.E_prev, next=2.0 * EPS32 * raw.E_next,
                noise=(2.0 * EPS32 * raw.X_norm + (raw.N // 4) * EPS32 * np.sqrt(raw.S64)) / np.sqrt((raw.N // 2) * float(raw.N)))


def tag_tolerance(raw, bin_, raw_err, self_corr=None):
    """(tol, ill): per field the bound on |field - tag64's| that the raw bounds allow, and whether the field is
    ill-conditioned at this tag.  tol = 2 * sum_q |d field / d q| * err_q (first-order sensitivities by central
    differences of output_tag() without clamps and wrap, doubled for the higher orders: a denominator moves by less than
    a quarter of itself, 1 / (1 - 1/4) < 2) + two float32 ulps of the field (finish_tag's own float evaluation).
    Ill-conditioned: a raw bound, taken to powers (2 v e + e^2), reaches a quarter of the denominator it enters --
    2b - (a + c) over the bins (amplitude, phase, freq, esn0_db of an interior bin) or over time (time_est) -- or of
    |z| (phase).  noise_power never is."""
    q, meta = _q_meta(raw, bin_, self_corr)
    nb = raw.z.size
    ez = np.broadcast_to(np.asarray(raw_err["z"], dtype=np.float64), (nb,))
    e = [ez[bin_], ez[bin_] / q[0] if q[0] > 0 else np.inf, ez[bin_ - 1] if bin_ > 0 else 0.0,
         ez[bin_ + 1] if bin_ < nb - 1 else 0.0, raw_err["prev"], raw_err["next"], raw_err["noise"]]
    base = _tag_core(q, meta)
    tol = {f: 2.0 * ulp32(base[f]) for f in FIELDS}
    for i in range(len(q)):
        if e[i] == 0.0:
            continue
        h = 1e-6 if i == 1 else max(abs(q[i]), 1e-300) * 1e-6
        qp, qm = list(q), list(q)
        qp[i] += h
        qm[i] -= h
        fp, fm = _tag_core(qp, meta, exact=False), _tag_core(qm, meta, exact=False)
        for f in FIELDS:
            d = abs(fp[f] - fm[f]) / (2.0 * h)
            tol[f] += 2.0 * (d * e[i] if np.isfinite(e[i]) and np.isfinite(d) else np.inf) if d != 0.0 else 0.0

    def dpow(v, err):
        return 2.0 * v * err + err * err

    interior = raw.lo < raw.lo + bin_ < raw.hi
    b = q[0] * q[0]
    ill_z = not e[0] < q[0] / 4.0
    ill_bins = interior and not (2.0 * dpow(q[0], e[0]) + dpow(q[2], e[2]) + dpow(q[3], e[3])
                                 < (2.0 * b - (q[2] ** 2 + q[3] ** 2)) / 4.0)
    ill_time = not (2.0 * dpow(q[0], e[0]) + dpow(q[4], e[4]) + dpow(q[5], e[5])
                    < (2.0 * b - (q[4] ** 2 + q[5] ** 2)) / 4.0)
    ill = dict(amplitude=ill_bins, phase=ill_z or ill_bins, freq=ill_bins, noise_power=False, esn0_db=ill_bins,
               time_est=ill_time)
    return tol, ill


def field_errors(tag, ref):
    """|tag's field - ref's| per field; phases modulo 2 pi"""
    out = {}
    for f in FIELDS:
        d = float(tag[f]) - ref[f]
        if f == "phase":
            d = float(np.angle(np.exp(1j * d)))
        out[f] = abs(d) if np.isfinite(d) or not (np.isinf(float(tag[f])) and float(tag[f]) == ref[f]) else 0.0
    return out
