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


def templates64(rrc, sps, lo, hi, N, syncword=sig.SYNCWORD, constellation=sig.BPSK):
    """hpp:166-189: per frequency bin b in [lo, hi] the conjugated spectrum of the shifted syncword, in float64.
    The phase walks in double with the reference's wrap quirk (`else if (phase < kPi)`: every step wraps by 2 pi),
    which moves the rounding of cos / sin, not their value."""
    sw = syncword_samples64(rrc, sps, syncword, constellation)
    L = sw.size
    if L > N:
        raise ValueError("template longer than fft_size")
    out = np.empty((hi - lo + 1, N), dtype=np.complex128)
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
        shifted = np.zeros(N, dtype=np.complex128)
        shifted[:L] = sw * (np.cos(phases) + 1j * np.sin(phases))
        out[b] = np.conj(np.fft.fft(shifted))
    return out


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
