"""The receive side at samples per symbol other than 4: the generic symbol-filter kernel (k_symbol_filter<T, 2>, <T, 8>
and the run-time form, plain and with the fused CoarseFrequencyCorrection, single- and multi-channel launch), the
receivers' wiring at those rates (arm of 11 sps taps, detector stride 2048 - (63 sps + n_rrc) + 1, CFC delay
(n_rrc - 1) / 2 + sps) and the decode_headers receiver's first-pass window, which is 228 symbols and not 912 items.

Every comparison is bit for bit against the CPU oracle (tests/_oracle.py), or between two forms of the library that must
agree bit for bit; the one exception, the detector's float tag fields against the oracle detector, is named where it is
made.  Every stimulus that a receiver has to find is checked here on the oracle detector first: a stimulus that the
reference itself would not detect where the test expects it fails the test, it does not thin it out."""
import functools

import numpy as np
import pytest

import __graft_entry__ as ge
import _oracle as orc
import _signals as sig
from test_gpu_parity import _tx_packets, assert_tags_match, bits, host, same_ptags, same_tags
from test_packet_transmitter import RefTx, rand_payloads

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TAG_FIELDS = ("index", "amplitude", "phase", "freq", "time_est", "flags")
DETECTOR_DELAY = 2 * 768 + 1   # syncword_detection.hpp:318-319: out[i] = in[i - (2 time_threshold + 1)]


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ge.load_package()


def dev(a):
    """a device copy (of a copy: the shared stimuli are read-only arrays, which torch does not wrap)"""
    return torch.from_numpy(np.array(a)).cuda()


def receiver_design(sps):
    """packet_receiver.hpp:60-74,94-115 at `sps` samples per symbol: (rrc, pfb, symbol filter delay, CFC delay)"""
    rrc, norm = orc.unit_norm_rrc(sps)
    pfb = orc.rrc_taps(32.0 / float(norm), 32.0 * sps, 1.0, 0.35, 32 * sps * 11)[:-1]
    return rrc, pfb, rrc.size - 1, (rrc.size - 1) // 2 + sps


def detector_stride(sps):
    """items SyncwordDetection consumes per transform: fft_size - (63 sps + n_rrc) + 1 (1752 at 4 samples per symbol)"""
    return 2048 - (63 * sps + orc.unit_norm_rrc(sps)[0].size) + 1


def run_in_calls(call, x, tags, cuts):
    """feeds x[cuts[k]:cuts[k + 1]] call by call as a scheduler would (what a call does not consume is offered again);
    returns (symbols, tags with stream indices, items consumed in all)"""
    ys, ts, pos, produced = [], [], 0, 0
    for end in cuts[1:]:
        if end <= pos:
            continue
        t = tags[(tags["index"] >= pos) & (tags["index"] < end)].copy()
        t["index"] -= pos
        y, to, c = call(dev(x[pos:end]), t)
        to = to.copy()
        to["index"] += produced
        produced += y.numel()
        ys.append(host(y))
        ts.append(to)
        pos += c
    return np.concatenate(ys), np.concatenate(ts), pos


# ------------------------------------------------------------------ 1. SymbolFilter, generic kernel
N_SYMBOLS = 2 * 256 + 37   # two full workgroups of 256 symbols and one partly filled

# (samples per symbol, arms, taps, delay, items).  n_taps is never a multiple of num_arms: arms of two lengths in one
# filter.  delay is never a multiple of sps (but at 1): reset_clock_phase != 0.  Instances of k_symbol_filter: sps 2 and 8
# are compiled in, 1, 3 and 5 take the run-time form; 4 with float items and 8 with complex items keep the generic kernel
# with arms of 71 taps (k_symbol_filter_long takes complex items at 4 samples per symbol only).
SYMF_CASES = {}
for _sps in (1, 2, 3, 5, 8):
    for _items in ("complex64", "float32"):
        SYMF_CASES[f"sps{_sps}-{_items}"] = (_sps, 32, 32 * 11 * _sps - 13, 11 * _sps + 1, _items)
SYMF_CASES["sps3-complex64-3arms"] = (3, 3, 3 * 17 + 1, 10, "complex64")
SYMF_CASES["sps4-float32-arm71"] = (4, 32, 32 * 70 + 5, 43, "float32")
SYMF_CASES["sps8-complex64-arm71"] = (8, 32, 32 * 70 + 5, 8 * 9 + 3, "complex64")


def symf_tag_indices(sps):
    """the eleven tags of test_symbol_filter_with_tags_all_clock_phase_cases laid over this stream: their indices (at 4
    samples per symbol, among them two tags three items and two tags one item apart) scaled by sps / 4, then moved off
    the multiples of sps (where there is room: not at 1) -- all but the first, which stays on item 0"""
    out = [0]
    for i4 in (183, 366, 457, 549, 552, 813, 1017, 1281, 1282, 2080):
        i = i4 * sps // 4
        while i <= out[-1] or (sps > 1 and i % sps == 0):
            i += 1
        out.append(i)
    return out


@functools.lru_cache(maxsize=None)
def symf_case(name):
    """input, tags and the oracle's answer of one case: computed once, shared by the call patterns, never written to"""
    sps, num_arms, n_taps, delay, items = SYMF_CASES[name]
    rng = np.random.default_rng(1000 * sps + n_taps)
    taps = rng.standard_normal(n_taps).astype(np.float32)
    n = sps * N_SYMBOLS + (sps - 1)   # ... and a remainder shorter than a symbol
    tags = np.zeros(0, dtype=orc.TAG_DTYPE)
    if items == "complex64":
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
        idx = symf_tag_indices(sps)
        assert idx[-1] < n and (sps == 1 or all(i % sps for i in idx[1:]))
        tags = np.zeros(len(idx), dtype=orc.TAG_DTYPE)
        tags["index"] = idx
        tags["amplitude"] = rng.uniform(0.5, 2.0, len(idx))
        tags["time_est"] = [0.1, -0.2, 0.49, -0.5, 0.0, -0.01, 0.3, -0.3, 0.5, 0.2, -0.45]
        tags["phase"] = rng.uniform(-3, 3, len(idx))
        tags["freq"] = rng.uniform(-0.03, 0.03, len(idx))
        tags["flags"] = 1     # TAG_SYNCWORD (asserted against the package in the test)
        tags["flags"][4] = 2  # TAG_OTHER: a non-syncword tag is only re-timed
        want, want_tags, want_cons = orc.symbol_filter(x, taps, num_arms, sps, delay, tags=tags)
    else:
        x = rng.standard_normal(n).astype(np.float32)
        want, want_tags, want_cons = orc.symbol_filter(x, taps, num_arms, sps, delay)
    for a in (x, taps, tags, want, want_tags):
        a.setflags(write=False)
    return x, taps, tags, want, want_tags, want_cons


@pytest.mark.parametrize("calls", ["one", "split"])
@pytest.mark.parametrize("name", list(SYMF_CASES))
def test_symbol_filter_generic_kernel_vs_oracle(pkg, name, calls):
    """plain SymbolFilter on the generic kernel against the oracle: symbols, items consumed and (complex items; the
    oracle's float path takes no tags) all six re-timed tag fields, in one call and in calls cut so that one piece is
    shorter than a symbol, one is shorter than the arm (its tile comes from the carried history) and one cut falls one
    item behind a tag"""
    sps, num_arms, n_taps, delay, items = SYMF_CASES[name]
    assert (pkg.TAG_SYNCWORD, pkg.TAG_OTHER) == (1, 2)
    x, taps, tags, want, want_tags, want_cons = symf_case(name)
    n, arm = x.size, -(-n_taps // num_arms)
    assert n_taps % num_arms and (sps == 1 or delay % sps)
    cuts = [0, n]
    if calls == "split":
        behind_tag = int(symf_tag_indices(sps)[8]) + 1
        cuts = [0, 257 * sps + 1, 257 * sps + 1 + max(sps - 1, 1), behind_tag, behind_tag + arm - 2, n]
        assert cuts == sorted(set(cuts)) and cuts[2] - cuts[1] < max(sps, 2) and cuts[4] - cuts[3] < arm
    f = pkg.SymbolFilter(taps, num_arms, sps, delay, items)
    gtags = tags.astype(pkg.TAG_DTYPE)
    if items == "complex64":
        y, t, cons = run_in_calls(lambda xd, tt: f.process_bulk(xd, tt), x, gtags, cuts)
    else:
        y, t, cons = run_in_calls(lambda xd, tt: f.process_bulk(xd), x, gtags, cuts)
    differing = int(np.count_nonzero(bits(y[: want.size]) != bits(want[: y.size])))
    print(f"{name} {calls}: {y.size} symbols, {differing} differ; consumed {cons} of {n}; {t.size} tags")
    assert y.size == want.size and differing == 0
    assert cons == want_cons
    assert t.size == want_tags.size
    for k in TAG_FIELDS:
        assert np.array_equal(t[k], want_tags[k]), k


# ------------------------------------------------------------------ 2. fused CFC + SymbolFilter, the receivers' design
@pytest.mark.parametrize("sps", [2, 3, 8])
def test_fused_cfc_symbol_filter_at_the_receivers_design(pkg, sps):
    """cfc_symbol_filter at the receivers' design for `sps` (arm 11 sps, filter delay n_rrc - 1, CFC delay
    (n_rrc - 1) / 2 + sps; never k_symbol_filter_fast) against (a) CoarseFrequencyCorrection then SymbolFilter run
    separately, (b) the oracle's two blocks, (c) cfc_symbol_filter_plan + _run with the next plan made before the current
    run.  Tags at ragged distances: one before the first output, two inside one phasor checkpoint chunk (fewer than 8
    items apart), the last item and one of the last sps - 1 items of a call, frequencies +0 and -0; five calls, one of
    them shorter than a checkpoint chunk."""
    rrc, pfb, symf_delay, cfc_delay = receiver_design(sps)
    assert pfb.size == 32 * 11 * sps
    rng = np.random.default_rng(7700 + sps)
    n = 3000 * sps + (sps - 1)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    A, B = 1000 * sps + 1, 2000 * sps + (sps - 1)
    cuts = [0, A, B, B + 5, 2500 * sps, n]
    idx = np.array([1, 211 * sps + 3, 211 * sps + 8, 700 * sps + 1, A - 1, A + 5 * sps + 2, 1800 * sps + (sps - 1),
                    B - (sps - 1), B + 2, 2600 * sps + 3, n - 2 * sps - 1], dtype=np.uint64)
    assert np.all(np.diff(idx.astype(np.int64)) > 0) and idx[2] - idx[1] < 8 and B - idx[7] <= sps - 1
    tags = np.zeros(idx.size, dtype=pkg.TAG_DTYPE)
    tags["index"] = idx
    tags["amplitude"] = rng.uniform(0.5, 2.0, idx.size)
    tags["time_est"] = rng.uniform(-0.5, 0.5, idx.size)
    tags["phase"] = rng.uniform(-3, 3, idx.size)
    tags["freq"] = rng.uniform(-0.03, 0.03, idx.size)
    tags["freq"][3], tags["freq"][6] = 0.0, -0.0
    tags["flags"] = pkg.TAG_SYNCWORD
    # (b) the oracle
    z = orc.coarse_frequency_correction(x, tags["index"], tags["freq"], delay=cfc_delay)
    want, want_tags, want_cons = orc.symbol_filter(z, pfb, 32, sps, symf_delay, tags=tags.astype(orc.TAG_DTYPE))
    # (a) separate blocks and the fused call, piece by piece
    a_cfc, a_sf = pkg.CoarseFrequencyCorrection(cfc_delay), pkg.SymbolFilter(pfb, 32, sps, symf_delay)
    b_cfc, b_sf = pkg.CoarseFrequencyCorrection(cfc_delay), pkg.SymbolFilter(pfb, 32, sps, symf_delay)
    c_cfc, c_sf = pkg.CoarseFrequencyCorrection(cfc_delay), pkg.SymbolFilter(pfb, 32, sps, symf_delay)
    ya, ta, ca = run_in_calls(lambda xd, t: a_sf.process_bulk(a_cfc.process_bulk(xd, t), t), x, tags, cuts)
    yb, tb, cb = run_in_calls(lambda xd, t: pkg.cfc_symbol_filter(b_cfc, b_sf, xd, t), x, tags, cuts)
    d_sep = int(np.count_nonzero(bits(ya[: yb.size]) != bits(yb[: ya.size])))
    d_orc = int(np.count_nonzero(bits(yb[: want.size]) != bits(want[: yb.size])))
    print(f"sps {sps}: {yb.size} symbols; fused vs separate {d_sep} differ, fused vs oracle {d_orc} differ")
    assert ya.size == yb.size and d_sep == 0 and ca == cb
    assert np.array_equal(ta, tb)
    assert yb.size == want.size and d_orc == 0 and cb == want_cons == n
    assert tb.size == want_tags.size
    for k in TAG_FIELDS:
        assert np.array_equal(tb[k], want_tags[k]), k
    # (c) plan then run, software-pipelined: plan(k + 1) is issued before run(k); every call takes its whole piece
    pieces = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        t = tags[(tags["index"] >= lo) & (tags["index"] < hi)].copy()
        t["index"] -= lo
        pieces.append((dev(x[lo:hi]), t))
    got = []
    plan = pkg.cfc_symbol_filter_plan(c_cfc, pieces[0][0].numel(), pieces[0][1])
    for k, (xd, t) in enumerate(pieces):
        nxt = None
        if k + 1 < len(pieces):
            nxt = pkg.cfc_symbol_filter_plan(c_cfc, pieces[k + 1][0].numel(), pieces[k + 1][1])
        got.append(pkg.cfc_symbol_filter_run(c_cfc, plan, c_sf, xd, t))
        plan = nxt
    assert [c for _, _, c in got] == [xd.numel() for xd, _ in pieces]
    yc = np.concatenate([host(y) for y, _, _ in got])
    off, tc = 0, []
    for y, t, _ in got:
        t = t.copy()
        t["index"] += off
        off += y.numel()
        tc.append(t)
    d_plan = int(np.count_nonzero(bits(yc[: yb.size]) != bits(yb[: yc.size])))
    print(f"sps {sps}: plan + run vs fused {d_plan} differ")
    assert yc.size == yb.size and d_plan == 0 and np.array_equal(np.concatenate(tc), tb)


# ------------------------------------------------------------------ 3. the Python-composed PacketReceiver, stage by stage
@functools.lru_cache(maxsize=None)
def front_end_stimulus(sps):
    """the bursts of test_packet_receiver_front_end_chain at `sps` samples per symbol: syncword + random QPSK body behind
    gaps of 300 .. 900 symbols, a carrier offset of 0.011 * 4 / sps radians per item (the same per symbol), AWGN 0.05"""
    rng = np.random.default_rng(91)
    n_pkt = 5
    rrc, _ = orc.unit_norm_rrc(sps)
    a = np.float32(np.sqrt(0.5))
    syms, starts = [], []
    for k in range(n_pkt):
        gap = np.zeros(int(rng.integers(300, 900)), dtype=np.complex64)
        payload_len = int(rng.integers(10, 200))
        nb = 128 + (payload_len + 4) * 4
        body = (np.where(rng.integers(0, 2, nb) == 0, a, -a) + 1j * np.where(rng.integers(0, 2, nb) == 0, a, -a)).astype(np.complex64)
        syms += [gap, sig.BPSK[sig.SYNCWORD], body]
        starts.append((sum(len(s) for s in syms[:-2]), payload_len))
    syms.append(np.zeros(1500, dtype=np.complex64))
    x = orc.interpolating_fir(np.concatenate(syms), sps, rrc)
    x = (orc.rotator(x, np.float32(0.011 * 4 / sps)) + sig.awgn(x.size, 0.05, 92)).astype(np.complex64)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, samples_per_symbol=sps, power_threshold=9.5)
    _, ref_out, ref_tags = ref.process(x)
    for arr in (x, ref_out, ref_tags):
        arr.setflags(write=False)
    return x, tuple(starts), ref_out, ref_tags


@pytest.mark.parametrize("sps", [2, 3, 8])
def test_packet_receiver_front_end_chain_at_other_rates(pkg, sps):
    """PacketReceiver(samples_per_symbol=sps) wiring (packet_receiver.hpp:34-127): the detector finds every burst at
    1537 + sps * start (so does the oracle detector, asserted first) with tag values within the bound of
    test_packet_receiver_front_end_chain (rtol 2e-4 against the oracle detector, whose FFT bits are not pinned); behind
    it every stage is bit-exact against the oracle stage fed with the GPU's detector tags -- CFC at delay
    (n_rrc - 1) / 2 + sps, the symbol filter of packet_receiver.hpp:100-110 at this rate, wipe-off, Costas loop."""
    x, starts, ref_out, ref_tags = front_end_stimulus(sps)
    rrc, pfb, symf_delay, cfc_delay = receiver_design(sps)
    expect = [DETECTOR_DELAY + sps * s for s, _ in starts]
    assert ref_tags["index"].tolist() == expect, "the reference itself does not detect this stimulus where expected"
    rx = pkg.PacketReceiver(samples_per_symbol=sps, max_items=x.size)

    def header_fn(tag):
        sym_idx = (int(tag["index"]) - DETECTOR_DELAY) / sps
        k = int(np.argmin([abs(s - sym_idx) for s, _ in starts]))
        return starts[k][1]

    res = rx.process_bulk(dev(x), header_fn)
    det = res["detector_tags"]
    assert det["index"].tolist() == expect and np.all(res["accepted"])
    for key in ("amplitude", "noise_power"):
        print(f"sps {sps}: detector {key} max relative deviation from the oracle "
              f"{np.max(np.abs(det[key] / ref_tags[key] - 1.0)):.3g}")
    assert_tags_match(det, ref_tags, rtol=2e-4)
    otags = det.astype(orc.TAG_DTYPE)
    z = orc.coarse_frequency_correction(ref_out, det["index"], det["freq"], delay=cfc_delay)
    sym, sym_tags, _ = orc.symbol_filter(z, pfb, 32, sps, symf_delay, tags=otags)
    bipolar = np.where(sig.SYNCWORD == 1, -1.0, 1.0).astype(np.float32)
    w = orc.syncword_wipeoff(sym, bipolar, sym_tags["index"])
    c = orc.costas_loop(w, "QPSK", 0.01, sym_tags["index"], sym_tags["phase"])
    got = host(res["symbols"])
    differing = int(np.count_nonzero(bits(got[: c.size]) != bits(c[: got.size])))
    print(f"sps {sps}: {got.size} Costas output symbols, {differing} differ from the oracle stages")
    assert got.size == c.size
    assert np.array_equal(res["tags"]["index"], sym_tags["index"])
    assert differing == 0


# ------------------------------------------------------------------ 4. the native receivers
@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("soft_bits", [False, True])
@pytest.mark.parametrize("sps", [2, 8])
def test_native_packet_receiver_equals_python_composition_at_other_rates(pkg, sps, pipelined, soft_bits):
    """test_native_packet_receiver_equals_python_composition at 2 and 8 samples per symbol: three batches of a device
    ring with look-ahead, three packets in each; symbols, LLRs and every tag bit for bit"""
    H, n = DETECTOR_DELAY, 4200 * sps
    rrc = orc.unit_norm_rrc(sps)[0]
    wins, expect = [], []
    for seed in (1, 2, 3):
        x, starts, _ = _tx_packets(np.random.default_rng(seed), [60, 60, 60], [300, 500, 420], sps=sps)
        x = np.concatenate([x, np.zeros(n, np.complex64)])[:n]
        wins.append((x + sig.awgn(n, 0.05, 710 + seed)).astype(np.complex64))
        expect += [len(expect) // 3 * n + H + sps * s for s in starts]
    stream = np.concatenate(wins)
    _, _, ref_tags = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, samples_per_symbol=sps,
                                           power_threshold=9.5).process(stream)
    assert ref_tags["index"].tolist() == expect, "the reference itself does not detect this stimulus where expected"
    ring = torch.zeros(2 + H + 3 * n, dtype=torch.complex64, device="cuda")
    ring[2 + H:] = dev(stream)
    ref = pkg.PacketReceiver(samples_per_symbol=sps, max_items=n, pipelined=False, soft_bits=soft_bits)
    nat = pkg.NativePacketReceiver(samples_per_symbol=sps, max_items=n, pipelined=pipelined, soft_bits=soft_bits)
    want, got = [], []
    for k in range(3):
        lo = 2 + H + k * n
        w, hist = ring[lo:lo + n], ring[lo - H:lo]
        nxt = ring[lo + n:lo + 2 * n] if k < 2 else None
        want.append(ref.process_bulk(w, 60, history=hist, next_x=nxt))
        r = nat.process_bulk(w, 60, history=hist, next_x=nxt)
        if r is not None:
            got.append(r)
    got += nat.flush()
    assert len(got) == 3
    for a, b in zip(want, got):
        assert a["consumed"] == b["consumed"] and same_tags(a["detector_tags"], b["detector_tags"])
        assert np.array_equal(a["accepted"], b["accepted"]) and same_tags(a["tags"], b["tags"])
        assert np.array_equal(bits(host(a["symbols"])), bits(host(b["symbols"])))
        if soft_bits:
            assert a["llr"].cpu().numpy().tobytes() == b["llr"].cpu().numpy().tobytes()
            assert same_ptags(a["llr_tags"], b["llr_tags"]) and same_ptags(a["packet_tags"], b["packet_tags"])
    # (a window is longer than what the detector consumes of it, so the receivers see the stream with short stretches of
    # the silence behind each window's packets left out: the nine bursts stay whole)
    assert sum(r["detector_tags"].size for r in got) == 9 and sum(r["tags"].size for r in got) >= 8


@pytest.mark.parametrize("sps", [2, 8])
def test_native_multichannel_receiver_equals_single_channel_receivers_at_other_rates(pkg, sps):
    """NativeMultiChannelReceiver(2, samples_per_symbol=sps) -- one launch of the generic fused kernel over both
    channels (the `chans` table) -- == one PacketReceiver per channel, bit for bit, over two calls; channels with
    different carrier offsets and burst positions.  (The seeds of the random symbols between the syncwords are ones at
    which the oracle detector raises no false alarm in them; at 9.5 it does at some.)"""
    C, n_sym = 2, 4096
    n = n_sym * sps
    rrc = orc.unit_norm_rrc(sps)[0]
    xs = np.zeros((C, 2 * n), dtype=np.complex64)
    for c in range(C):
        locs = [700 + 300 * c + 1300 * k for k in range(5)]
        stream, _ = sig.qa_syncword_stream(2 * n_sym, locs, (-0.02 + 0.04 * c) * 4 / sps, seed=60 + c, sps=sps)
        xs[c] = (0.7 * stream[: 2 * n] + sig.awgn(2 * n, 0.05, 90 + c)).astype(np.complex64)
        _, _, ref_tags = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, samples_per_symbol=sps,
                                               power_threshold=9.5).process(xs[c])
        assert ref_tags["index"].tolist() == [DETECTOR_DELAY + sps * s for s in locs], \
            "the reference itself does not detect this stimulus where expected"
    native = pkg.NativeMultiChannelReceiver(C, samples_per_symbol=sps, max_items=n, tags_cap=256, workers=2)
    singles = [pkg.PacketReceiver(samples_per_symbol=sps, max_items=n) for _ in range(C)]
    xd = dev(xs)
    parts = [xd[:, part * n:(part + 1) * n].contiguous() for part in range(2)]
    native.announce(parts[1])
    total_tags = 0
    for part in range(2):
        got = native.process_bulk(parts[part], 100)
        for c in range(C):
            want = singles[c].process_bulk(parts[part][c], 100, tags_cap=256)
            assert got[c]["consumed"] == want["consumed"] > 0
            assert same_tags(got[c]["detector_tags"], want["detector_tags"])
            assert same_tags(got[c]["tags"], want["tags"])
            assert np.array_equal(bits(host(got[c]["symbols"])), bits(host(want["symbols"])))
            total_tags += got[c]["tags"].size
    assert total_tags >= 3 * C


def e2e_layout(sps, seed):
    """a dozen random payloads of 1 .. 200 bytes with random packet types behind gaps of 1200 .. 4000 items.  Two gaps
    are then moved, inside that range, by less than a detector stride, so that the ends of the first two of three calls
    -- multiples of the stride -- fall (1) 100 symbols behind the detection of packet 4, whose 228-symbol header window
    therefore continues in the next batch, and (2) in the middle of the payload of packet 8."""
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in rng.integers(1, 201, 12)]
    lengths[8] = 200
    payloads = rand_payloads(rng, lengths)
    types = [int(v) for v in rng.integers(0, 2, 12)]
    gaps = [int(v) for v in rng.integers(1200, 4001, 12)]
    stride = detector_stride(sps)
    blen = [sps * (4 * n + 228) for n in lengths]

    def detection(k):  # index of packet k's detection in the detector's output stream
        return DETECTOR_DELAY + sum(gaps[: k + 1]) + sum(blen[:k])

    ends = []
    for k, behind in ((4, 100 * sps), (8, (192 + 2 * lengths[8]) * sps)):
        shift = -(detection(k) + behind) % stride
        gaps[k] += shift if gaps[k] + shift <= 4000 else shift - stride
        assert 1200 <= gaps[k] <= 4000 and (detection(k) + behind) % stride == 0
        ends.append(detection(k) + behind)
    # a call of q * stride + (2048 - stride) items lets the detector consume q * stride of them
    cuts = [ends[0] + 2048 - stride, ends[1] - ends[0] + 2048 - stride]
    return payloads, types, gaps, [detection(k) for k in range(12)], ends, cuts


def channel(pkg, x, sps, seed):
    """Rotator at 0.01 * 4 / sps, then AWGN at Es/N0 = 20 dB for the transmitter's power of 0.32 (n0 = 0.32 sps 10^-2,
    as Channel does); the noise is drawn on the host from a fixed seed"""
    x = pkg.Rotator(np.float32(0.01 * 4 / sps)).process_bulk(x)
    n0 = 0.32 * sps * 10.0 ** (-0.1 * 20.0)
    return (x + dev(sig.awgn(x.numel(), np.sqrt(n0), seed))).to(torch.complex64)


def oracle_detections(x, sps):
    rrc = orc.unit_norm_rrc(sps)[0]
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, samples_per_symbol=sps, power_threshold=9.5)
    return ref.process(host(x), tags_cap=8192)[2]["index"].tolist()


def delivered(results):
    data = np.concatenate([host(r["packets"]) for r in results])
    lens = np.concatenate([r["packet_lengths"] for r in results])
    out, pos = [], 0
    for n in lens[lens > 0]:
        out.append(data[pos:pos + int(n)].tobytes())
        pos += int(n)
    return out, lens


@pytest.mark.parametrize("mode", ["one_call", "three_calls"])
@pytest.mark.parametrize("packets_only", [False, True])
@pytest.mark.parametrize("sps", [5, 8])
def test_native_packet_receiver_decodes_packets_at_other_rates(pkg, sps, packets_only, mode):
    """PacketTransmitter(sps) -> Rotator -> AWGN 20 dB -> NativePacketReceiver(sps, decode_headers=True): every payload
    and packet type comes back and the chain's own header decode agrees with the first pass (header_mismatches == 0),
    in one call and in three calls whose cuts leave one detection waiting for the next batch and split one payload.
    (The seeds are ones at which the oracle detector finds the twelve bursts and raises no false alarm inside a payload.)
    5 and 8 only: at 2 and 3 the mode is refused, see test_decode_headers_is_refused_below_four_samples_per_symbol."""
    payloads, types, gaps, detections, ends, cuts = e2e_layout(sps, 4010 + sps)
    tx = pkg.PacketTransmitter(samples_per_symbol=sps)
    x, offs, _ = tx.process_bulk(payloads, packet_types=types, gaps=gaps)
    # (the transmitter at this rate is the reference's, bit for bit: what the stimulus was checked with off the GPU)
    assert np.array_equal(bits(host(x)), bits(RefTx(pkg, sps).process(payloads, types, gaps)[0]))
    x = torch.cat([x, torch.zeros(1000 * sps + 4096, dtype=torch.complex64, device=x.device)])
    x = channel(pkg, x, sps, 4110 + sps)
    assert [DETECTOR_DELAY + int(o) for o in offs] == detections
    assert oracle_detections(x, sps) == detections, "the reference itself does not detect this stimulus where expected"
    rx = pkg.NativePacketReceiver(samples_per_symbol=sps, max_items=x.numel(), decode_headers=True,
                                  packets_only=packets_only)
    got, pos = [], 0
    for c in ([x.numel()] if mode == "one_call" else cuts + [x.numel()]):
        got.append(rx.process_bulk(x[pos:min(pos + c, x.numel())]))
        assert got[-1]["status"] == 0
        pos += got[-1]["consumed"]
    if mode == "three_calls":
        # the cuts are where e2e_layout put them: behind a detection by less than the window that follows it (228 - 16
        # symbols), and inside packet 8's payload
        assert [got[0]["consumed"], got[0]["consumed"] + got[1]["consumed"]] == ends
        assert 0 < ends[0] - detections[4] < (228 - 16) * sps
        assert (192 + 20) * sps < ends[1] - detections[8] < (192 + 4 * len(payloads[8]) - 20) * sps
    assert sum(int(r["header_mismatches"]) for r in got) == 0
    msgs = np.concatenate([r["header_messages"] for r in got])
    valid = msgs["invalid_header"] == 0
    assert [int(v) for v in msgs["packet_length"][valid]] == [len(p) for p in payloads]
    assert [int(v) for v in np.concatenate([r["packet_type"] for r in got])[valid]] == types
    out, lens = delivered(got)
    print(f"sps {sps} packets_only {packets_only} {mode}: {len(out)} of {len(payloads)} packets, "
          f"{sum(a != b for a, b in zip(out, payloads))} differ")
    assert out == payloads


@pytest.mark.parametrize("sps", [1, 2, 3])
def test_decode_headers_is_refused_below_four_samples_per_symbol(pkg, sps):
    """In place of the end-to-end run at 2 and 3 samples per symbol, and of 120 packets of 1500 bytes 64 items apart at 2:
    the receivers refuse decode_headers there, natively with GR4PM_ERR_INVALID.  The reference's SymbolFilter moves its
    clock phase at a detection through two special cases written for 4 samples per symbol (symbol_filter.hpp:158-195);
    at 2 the first of them leaves the clock half a symbol off for the packet.  The library's blocks are the reference's
    bit for bit at these rates too (the tests above), so the front end runs and its symbols do not decode.  Measured
    on the CPU oracle's blocks alone -- detector, CFC, symbol filter, wipe-off, PayloadMetadataInsert, tag-driven
    Costas loop, SyncwordRemove, hard decisions against the transmitted symbols -- on the stimulus of
    test_native_packet_receiver_decodes_packets_at_other_rates, twelve packets at Es/N0 = 20 dB, three seeds per rate:
    packets whose header has symbol errors 12 / 12 / 12 at 1, 10 / 7 / 8 at 2, 4 / 1 / 5 at 3, and 0 / 0 / 0 at each of
    4, 5, 6, 7 and 8.  On the GPU, before the refusal existed, the run at 2 gave 5 header mismatches, the run at 3
    nine headers of twelve, one of them with a wrong length, and the dense stream at 2 a header mismatch.  The front end and the soft_bits mode exist at every rate."""
    for packets_only in (False, True):
        with pytest.raises(pkg.Gr4pmError, match="4 samples per symbol"):
            pkg.NativePacketReceiver(samples_per_symbol=sps, max_items=1 << 16, decode_headers=True, packets_only=packets_only)
    with pytest.raises(pkg.Gr4pmError, match="4 samples per symbol"):
        pkg.PacketReceiver(samples_per_symbol=sps, max_items=1 << 16, decode_headers=True)
    assert pkg.NativePacketReceiver(samples_per_symbol=sps, max_items=1 << 16, soft_bits=True) is not None
