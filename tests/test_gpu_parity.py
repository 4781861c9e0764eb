"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle on the same
seeded inputs, plus the reference's own qa_*.cpp expectations re-run on the GPU output.

Bars: indices / freq_bin / pass-through / FIR outputs bit-exact; FFT-derived float tag
values within 1e-4 relative (FFTW's own bits are unpinned, see oracle/gr4pm_oracle.h);
recurrences (rotator, CFC) bit-exact; Costas bit-exact too (the device restates glibc's sinf / cosf)."""
import os
import time

import numpy as np
import pytest

import __graft_entry__ as ge
import _oracle as orc
import _signals as sig

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _same_records(a, b):
    """field by field: the padding bytes of an aligned record are not part of the ABI (and are not initialised)"""
    return a.dtype == b.dtype and a.shape == b.shape and all(np.array_equal(a[n], b[n]) for n in a.dtype.names)


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ge.load_package()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.complex64 else a.view(np.uint32)


def assert_tags_match(tags, ref, rtol=1e-4):
    assert np.array_equal(tags["index"], ref["index"]), (tags["index"], ref["index"])
    assert np.array_equal(tags["freq_bin"], ref["freq_bin"])
    for key in ("amplitude", "noise_power"):
        assert np.allclose(tags[key], ref[key], rtol=rtol, atol=0), key
    assert np.allclose(tags["freq"], ref["freq"], rtol=0, atol=2e-6)
    dphi = np.angle(np.exp(1j * (tags["phase"].astype(np.float64) - ref["phase"].astype(np.float64))))
    assert np.max(np.abs(dphi), initial=0) < 2e-4
    assert np.allclose(tags["esn0_db"], ref["esn0_db"], rtol=0, atol=2e-3)
    assert np.allclose(tags["time_est"], ref["time_est"], rtol=0, atol=2e-4)


# ------------------------------------------------------------------ SyncwordDetection
@pytest.mark.parametrize("freq_error", [0.0, 0.005, 0.015, -0.005, -0.015])
def test_syncword_detection_vs_oracle_and_reference_qa(pkg, freq_error):
    """test/qa_syncword_detection.cpp:21-151 at 200k symbols + oracle comparison"""
    locations = [100, 1000, 1250, 10000, 13721, 43124, 58000, 127018, 180000 - 64]
    x, rrc = sig.qa_syncword_stream(200000, locations, freq_error, seed=21)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0)
    st0, ref_out, ref_tags, ref_zpow, _ = ref.process(x, debug=True)
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0, max_items=x.size)
    st, out, tags, n = sd.process_bulk(dev(x))
    assert st == st0 == 0 and n == ref_out.size
    assert sd._syncword_samples_size == 297 and abs(sd._syncword_self_corr - ref._syncword_self_corr) < 1e-5
    out = host(out)
    delay = 2 * sd.time_threshold + 1
    assert np.all(out[:delay] == 0)                                        # qa :108-110
    assert np.array_equal(bits(out[delay:]), bits(x[: n - delay]))         # qa :111-113
    assert np.array_equal(bits(out), bits(ref_out))
    assert tags.size == len(locations)
    for tag, loc in zip(tags, locations):
        assert tag["index"] == delay + 4 * loc                             # qa :117-120
        assert 0.95 < tag["amplitude"] < 1.01 and tag["esn0_db"] >= 30.0
        assert abs(np.float32(tag["freq"]) - np.float32(freq_error)) < 5e-4
        assert tag["noise_power"] < 5e-4 and abs(tag["time_est"]) < 0.05
        if freq_error == 0.0:
            assert abs(tag["phase"]) < 1e-6
    assert_tags_match(tags, ref_tags)
    zpow = host(sd.last_zpow(n))[0]
    scale = np.max(ref_zpow)
    assert np.max(np.abs(zpow - ref_zpow)) / scale < 2e-6


def test_syncword_detection_streaming_chunks_match_single_call(pkg):
    """state carried across calls (hpp:191-199,349): arbitrary chunking == one call == oracle"""
    locations = [100, 1000, 1250, 10000, 13721, 43124, 58000 - 64]
    x, rrc = sig.qa_syncword_stream(60000, locations, 0.005, seed=5)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0)
    _, ref_out, ref_tags = ref.process(x)
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0, max_items=1 << 16)
    xd = dev(x)
    rng = np.random.default_rng(3)
    pos, outs, all_tags = 0, [], []
    while pos + 2048 <= x.size:
        n_req = int(rng.integers(2048, 30000))
        st, o, t, n = sd.process_bulk(xd[pos:pos + n_req].contiguous())
        assert st == 0 and n > 0
        t = t.copy()
        t["index"] += pos
        outs.append(host(o))
        all_tags.append(t)
        pos += n
    out = np.concatenate(outs)
    tags = np.concatenate(all_tags)
    assert np.array_equal(bits(out), bits(ref_out[: out.size]))
    k = tags.size
    assert k >= 6
    assert_tags_match(tags, ref_tags[:k])


def same_tags(a, b):
    """field-wise bit equality (the records carry padding bytes)"""
    return a.size == b.size and all(a[f].tobytes() == b[f].tobytes() for f in a.dtype.names)


def test_scan_with_supergroup_tables_equals_the_two_level_scan(pkg, monkeypatch):
    """round 6: calls of more than 16 groups of 32 tiles (2^24 items) resolve the greedy scan over THREE levels of jump
    tables (k_super_tables, k_scan_entries); GR4PM_SD_NO_SUPER=1 at creation keeps the two-level walk of rounds 1 - 5.
    Identical tags on 2^25 samples -- bursts in noise, a constant stretch (every item a candidate: the tables' dense path),
    silence -- in one call and in two ragged ones (the second call's scan enters at the position the first one left)"""
    base, rrc = sig.qa_syncword_stream(75000, [700, 9000, 31000, 52000, 70001], 0.01, seed=21)
    reps = (1 << 25) // base.size + 1
    n = 1 << 25
    x = np.tile(0.6 * base, reps)[:n].astype(np.complex64)
    x += sig.awgn(n, 0.2, 22)
    x[5_000_000:5_040_000] = 0.25
    x[20_000_000:20_300_000] = 0
    res = {}
    for kind in ("three", "two"):
        monkeypatch.delenv("GR4PM_SD_NO_SUPER", raising=False)
        if kind == "two":
            monkeypatch.setenv("GR4PM_SD_NO_SUPER", "1")
        sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5, max_items=n)
        one = sd.process_bulk(dev(x), want_output=False, tags_cap=8192)
        sd2 = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5, max_items=n)
        cut = 17_000_123
        parts = [sd2.process_bulk(dev(x[:cut]), want_output=False, tags_cap=8192),
                 sd2.process_bulk(dev(x[cut:]), want_output=False, tags_cap=8192)]
        res[kind] = (one, parts, sd.scan_counts())
    monkeypatch.delenv("GR4PM_SD_NO_SUPER", raising=False)
    (one3, parts3, counts3), (one2, parts2, counts2) = res["three"], res["two"]
    assert one3[2].size >= 500 and counts3 == counts2 and counts3[0] >= n // 2000
    assert same_tags(one3[2], one2[2])
    for a, b in zip(parts3, parts2):
        assert same_tags(a[2], b[2])
    assert parts3[0][2].size + parts3[1][2].size == one3[2].size  # (the two calls find what the one call finds)


def test_syncword_detection_lookahead_matches_plain_calls(pkg):
    """gr4pm_syncword_detection_hint_next: announcing the next input (right, wrong, or with a
    different length) never changes out/tags; compared chunk by chunk with a plain handle and
    with the oracle"""
    locations = [100, 1000, 1250, 10000, 13721, 43124, 58000 - 64]
    x, rrc = sig.qa_syncword_stream(60000, locations, 0.005, seed=5)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0)
    _, ref_out, ref_tags = ref.process(x)
    plain = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0, max_items=1 << 16)
    ahead = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0, max_items=1 << 16)
    xd = dev(x)
    S = 2048 - 297 + 1
    rng = np.random.default_rng(11)
    # chunk boundaries are known up front (consumed = whole strides, hpp:238)
    chunks, pos = [], 0
    while pos + 2048 <= x.size:
        n_req = min(int(rng.integers(2048, 20000)), x.size - pos)
        chunks.append((pos, n_req))
        pos += ((n_req - 2048) // S + 1) * S
    outs, all_tags = [], []
    for i, (pos, n_req) in enumerate(chunks):
        nxt = None
        if i + 1 < len(chunks):
            p2, n2 = chunks[i + 1]
            kind = i % 4
            if kind == 0 or kind == 1:
                nxt = xd[p2:p2 + n2]                 # the right announcement
            elif kind == 2:
                nxt = xd[p2 + 8:p2 + 8 + n2 - 8]     # a wrong one: dropped, recomputed
            # kind 3: none
        st, o, t, n = ahead.process_bulk(xd[pos:pos + n_req], next_x=nxt)
        st2, o2, t2, n2_ = plain.process_bulk(xd[pos:pos + n_req])
        assert st == 0 and n == n2_ and n > 0
        assert np.array_equal(bits(host(o)), bits(host(o2)))
        assert same_tags(t, t2)
        t = t.copy()
        t["index"] += pos
        outs.append(host(o))
        all_tags.append(t)
    out = np.concatenate(outs)
    tags = np.concatenate(all_tags)
    assert np.array_equal(bits(out), bits(ref_out[: out.size]))
    assert tags.size >= 6
    assert_tags_match(tags, ref_tags[: tags.size])
    # reset() forgets a pending look-ahead
    ahead.process_bulk(xd[:8192], next_x=xd[7008:20000])
    ahead.reset() if hasattr(ahead, "reset") else ahead.start()
    plain.start()
    st, o, t, n = ahead.process_bulk(xd[7008:20000])
    st2, o2, t2, n2_ = plain.process_bulk(xd[7008:20000])
    assert n == n2_ and np.array_equal(bits(host(o)), bits(host(o2))) and same_tags(t, t2)


def test_syncword_detection_announced_two_calls_ahead(pkg):
    """gr4pm_syncword_detection_announce: fronts of up to two future calls in flight (right ones,
    a wrong one in the middle, more announcements than are kept) never change out/tags"""
    locations = [100, 1000, 1250, 10000, 13721, 43124, 58000 - 64, 70000, 90500, 118000]
    x, rrc = sig.qa_syncword_stream(125000, locations, -0.004, seed=6)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0)
    _, ref_out, ref_tags = ref.process(x)
    plain = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0, max_items=1 << 16)
    ahead = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0, max_items=1 << 16)
    xd = dev(x)
    S = 2048 - 297 + 1
    rng = np.random.default_rng(12)
    chunks, pos = [], 0
    while pos + 2048 <= x.size:
        n_req = min(int(rng.integers(2048, 12000)), x.size - pos)
        chunks.append((pos, n_req))
        pos += ((n_req - 2048) // S + 1) * S
    assert len(chunks) > 16
    outs, all_tags = [], []
    announced = 0    # chunks up to this index have been announced
    quiet_until = 0  # no announcements before this call
    for i, (pos, n_req) in enumerate(chunks):
        if i == 9:
            # a wrong announcement: launched as the front of call 11, dropped there
            ahead.announce(xd[chunks[11][0] + 16:chunks[11][0] + 16 + 4096])
            quiet_until = 12
        elif i == 15:
            # more announcements than are kept: only the first one fits, the others are ignored
            for k in range(announced + 1, min(announced + 5, len(chunks))):
                ahead.announce(xd[chunks[k][0]:chunks[k][0] + chunks[k][1]])
            quiet_until = 20
        elif i >= quiet_until:
            announced = max(announced, i)
            while announced < min(i + 2, len(chunks) - 1):
                announced += 1
                p2, n2 = chunks[announced]
                ahead.announce(xd[p2:p2 + n2])
        st, o, t, n = ahead.process_bulk(xd[pos:pos + n_req])
        st2, o2, t2, n2_ = plain.process_bulk(xd[pos:pos + n_req])
        assert st == 0 and n == n2_ and n > 0
        assert np.array_equal(bits(host(o)), bits(host(o2))), i
        assert same_tags(t, t2), i
        t = t.copy()
        t["index"] += pos
        outs.append(host(o))
        all_tags.append(t)
    out = np.concatenate(outs)
    tags = np.concatenate(all_tags)
    assert np.array_equal(bits(out), bits(ref_out[: out.size]))
    assert tags.size >= 9
    assert_tags_match(tags, ref_tags[: tags.size])


def test_two_waves_per_block_correlator_is_bit_identical(pkg, monkeypatch):
    """k_correlate_pair (fft2048_pair.hpp: two waves per overlap-save block, 16 points per lane;
    selected with GR4PM_CORRELATOR=pair when the handle is created) does the same arithmetic in
    another distribution: identical correlation powers, identical output and tags"""
    locations = [100, 1000, 1250, 10000, 13721, 43124, 58000 - 64]
    x, rrc = sig.qa_syncword_stream(60000, locations, 0.007, seed=15)
    x = (x + sig.awgn(x.size, 0.2, 16)).astype(np.complex64)
    xd = dev(x)
    res = {}
    for kind in ("wave", "pair"):
        monkeypatch.setenv("GR4PM_CORRELATOR", kind)
        sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5, max_items=1 << 18)
        outs, tags, z = [], [], []
        for lo, hi in ((0, 100000), (100000 - 1600, x.size)):  # two calls (odd block counts, idle pair at the end)
            st, o, t, n = sd.process_bulk(xd[lo:hi])
            assert st == 0 and n > 0
            outs.append(host(o)); tags.append(t); z.append(host(sd.last_zpow(n)))
        res[kind] = (outs, tags, z)
    for a, b in zip(res["wave"][2], res["pair"][2]):
        assert a.size > 50000 and np.array_equal(bits(a), bits(b))
    for a, b in zip(res["wave"][0], res["pair"][0]):
        assert np.array_equal(bits(a), bits(b))
    for a, b in zip(res["wave"][1], res["pair"][1]):
        assert a.size >= 2 and same_tags(a, b)


def test_one_bin_correlator_three_waves_per_simd_is_bit_identical(pkg, monkeypatch):
    """correlate_w64_one.hpp (GR4PM_W64_ONE=1 when the handle is created: one frequency bin, twelve waves per CU, the
    exchange through a half-size buffer in two passes) against the general kernel: the same powers bit for bit, the
    same output and tags, over two calls with odd block counts and over two channels"""
    locations = [100, 1000, 1250, 10000, 13721, 43124, 58000 - 64]
    x, rrc = sig.qa_syncword_stream(60000, locations, 0.0, seed=21)
    x = (x + sig.awgn(x.size, 0.2, 22)).astype(np.complex64)
    xd = dev(x)
    res = {}
    for one in ("0", "1"):
        monkeypatch.setenv("GR4PM_W64_ONE", one)
        sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, 0, 0, power_threshold=9.5, max_items=1 << 18)
        outs, tags, z = [], [], []
        for lo, hi in ((0, 100000), (100000 - 1600, x.size)):
            st, o, t, n = sd.process_bulk(xd[lo:hi])
            assert st == 0 and n > 0
            outs.append(host(o)); tags.append(t); z.append(host(sd.last_zpow(n)))
        res[one] = (outs, tags, z)
    for a, b in zip(res["0"][2], res["1"][2]):
        assert a.size > 50000 and np.array_equal(bits(a), bits(b))
    for a, b in zip(res["0"][0], res["1"][0]):
        assert np.array_equal(bits(a), bits(b))
    for a, b in zip(res["0"][1], res["1"][1]):
        assert a.size >= 2 and same_tags(a, b)


def test_correlator_block_hand_out_does_not_change_a_bit(pkg, monkeypatch):
    """k_correlate_w64 hands the blocks of a workgroup out through a counter in LDS (which wave computes which block
    depends on timing): the powers are those of the fixed shares of rounds 1 - 3 (GR4PM_W64_VARIANT=131072), for 1, 3, 6
    and 16 blocks per wave and workgroup and for persistent waves, nine bins and one, one channel and three, over two
    calls with odd block counts -- bit for bit, tags included"""
    locations = [100, 1000, 1250, 10000, 13721, 43124, 58000 - 64, 90011]
    x, rrc = sig.qa_syncword_stream(100000, locations, 0.0, seed=31)
    x = (x + sig.awgn(x.size, 0.2, 32)).astype(np.complex64)
    for n_channels, bins in ((1, 4), (1, 0), (3, 4)):
        xd = dev(np.stack([np.roll(x, 1000 * c) for c in range(n_channels)])) if n_channels > 1 else dev(x)
        res = {}
        for name, env in (("fixed", {"GR4PM_W64_VARIANT": "131072"}), ("1", {"GR4PM_W64_BLOCKS_PER_WAVE": "1"}),
                          ("3", {"GR4PM_W64_BLOCKS_PER_WAVE": "3"}), ("default", {}),
                          ("16", {"GR4PM_W64_BLOCKS_PER_WAVE": "16"}), ("persistent", {"GR4PM_W64_BLOCKS_PER_WAVE": "0"})):
            for k in ("GR4PM_W64_VARIANT", "GR4PM_W64_BLOCKS_PER_WAVE"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -bins, bins, power_threshold=9.5, max_items=1 << 18,
                                       n_channels=n_channels)
            z, tags = [], []
            for lo, hi in ((0, 160000), (160000 - 1600, 4 * 100000 - 3)):
                piece = xd[..., lo:hi].contiguous()
                st, o, t, n = sd.process_bulk(piece)
                assert st == 0 and n > 0
                z.append(host(sd.last_zpow(n)))
                tags.append(t)
            res[name] = (z, tags)
        for name, (z, tags) in res.items():
            for a, b in zip(res["fixed"][0], z):
                assert a.size > 100000 and np.array_equal(bits(a), bits(b)), (n_channels, bins, name)
            for a, b in zip(res["fixed"][1], tags):
                if n_channels == 1:
                    assert a.size >= 2 and same_tags(a, b), (bins, name)
                else:
                    assert all(same_tags(p, q) for p, q in zip(a, b)), (bins, name)


@pytest.mark.parametrize("kind", ["wave", "pair"])
def test_correlator_spin_timeout_is_reported(pkg, monkeypatch, kind):
    """the round-1 correlator kernels hand templates over through bounded spins: a spin that runs out raises the
    handle's fault word and process() fails with GR4PM_ERR_HIP instead of returning powers computed from a
    stale template (GR4PM_TEST_SPIN_LIMIT=0 forces every wait to time out); the default kernel has no spins"""
    x, rrc = sig.qa_syncword_stream(20000, [100, 1000, 5000], 0.0, seed=3)
    monkeypatch.setenv("GR4PM_CORRELATOR", kind)
    monkeypatch.setenv("GR4PM_TEST_SPIN_LIMIT", "0")
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0, max_items=x.size)
    with pytest.raises(pkg.Gr4pmError, match="hand-off timed out"):
        sd.process_bulk(dev(x))
    monkeypatch.delenv("GR4PM_TEST_SPIN_LIMIT")
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0, max_items=x.size)
    st, out, tags, n = sd.process_bulk(dev(x))
    assert st == 0 and tags.size == 3


def test_candidate_kernels_agree(pkg, monkeypatch):
    """the LDS-free candidate kernel (one wave walks T-item blocks in registers; default at T = 768) and the LDS one
    (GR4PM_CANDIDATES_LDS) flag the same items: identical tags on bursts + noise + a constant stretch (ties), in one
    call and in ragged chunks, two channels"""
    rng = np.random.default_rng(5)
    n = 300000
    x, rrc = sig.qa_syncword_stream(n // 4, [700, 9000, 31000, 52000, 70001], 0.01, seed=12)
    x = (0.6 * x[:n] + sig.awgn(n, 0.2, 13)).astype(np.complex64)
    x[120000:150000] = 0.25  # constant input: equal powers, every tie counts
    x[200000:200700] = 0
    xs = np.stack([x, np.roll(x, 12345)]).astype(np.complex64)
    res = {}
    # "wave": round 5's default, k_candidates_wave<12, true> -- the median test of every candidate done on the registers
    # that hold its history, k_tile_visit looks the visited ones up; "split": round 4's two passes over the powers
    # (k_candidates_wave<12, false> + k_median_tests, GR4PM_SD_SEPARATE_MEDIAN); "lds": the LDS kernel + k_median_tests
    for kind in ("wave", "split", "lds"):
        monkeypatch.delenv("GR4PM_SD_SEPARATE_MEDIAN", raising=False)
        if kind == "lds":
            monkeypatch.setenv("GR4PM_CANDIDATES_LDS", "1")
        if kind == "split":
            monkeypatch.setenv("GR4PM_SD_SEPARATE_MEDIAN", "1")
        sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5, max_items=n, n_channels=2)
        one = sd.process_bulk(dev(xs))
        sd2 = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5, max_items=n, n_channels=2)
        chunks, pos = [], 0
        for m in (70000, 4096, 100001, 125903):
            chunks.append(sd2.process_bulk(dev(np.ascontiguousarray(xs[:, pos:pos + m]))))
            pos += m
        res[kind] = (one, chunks)
    monkeypatch.delenv("GR4PM_CANDIDATES_LDS")
    (one_w, ch_w), (one_l, ch_l), (one_s, ch_s) = res["wave"], res["lds"], res["split"]
    # where the tests ran (gr4pm_syncword_detection_scan_counts): "split" tests every visited candidate from memory; the
    # fused kernel leaves that to the candidates it deferred -- here the ties of the constant stretches (every item a
    # candidate, eight tested per block) and little else: a candidate it rules out as unvisitable is never visited
    counts = {}
    for kind in ("wave", "split"):
        monkeypatch.delenv("GR4PM_SD_SEPARATE_MEDIAN", raising=False)
        if kind == "split":
            monkeypatch.setenv("GR4PM_SD_SEPARATE_MEDIAN", "1")
        for name, sig_x in (("stream", x), ("noise", sig.awgn(n, 0.2, 99)), ("zeros", np.zeros(n, np.complex64))):
            sd1 = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5, max_items=n)
            sd1.process_bulk(dev(sig_x.astype(np.complex64)), want_output=False, tags_cap=4096)
            counts[kind, name] = sd1.scan_counts()
    monkeypatch.delenv("GR4PM_SD_SEPARATE_MEDIAN", raising=False)
    for name in ("stream", "noise", "zeros"):
        visited, from_memory = counts["split", name]
        assert visited == from_memory >= n // 2000 and counts["wave", name][0] == visited, (name, counts)
    assert counts["wave", "noise"][1] <= counts["wave", "noise"][0] // 20, counts      # noise: (nearly) everything in registers
    assert counts["wave", "zeros"][1] >= counts["wave", "zeros"][0] * 9 // 10, counts  # constant input: deferred, tested from memory
    assert 0 < counts["wave", "stream"][1] < counts["wave", "stream"][0] // 3, counts
    assert sum(t.size for t in one_w[2]) >= 8
    for c in range(2):
        assert same_tags(one_w[2][c], one_l[2][c]) and same_tags(one_w[2][c], one_s[2][c])
        for a, b, d in zip(ch_w, ch_l, ch_s):
            assert same_tags(a[2][c], b[2][c]) and same_tags(a[2][c], d[2][c])
    # thresholds at which the median test REJECTS visited candidates (9.5 lets nearly every local maximum of this stream
    # through, so a wrong count would go unnoticed): the three forms agree there too, and against the oracle
    for thr in (1.5, 3.0, 60.0):
        got = {}
        for kind in ("wave", "split"):
            monkeypatch.delenv("GR4PM_SD_SEPARATE_MEDIAN", raising=False)
            if kind == "split":
                monkeypatch.setenv("GR4PM_SD_SEPARATE_MEDIAN", "1")
            sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=thr, max_items=n)
            pos, tags = 0, []
            for m in (70000, 4096, 100001, 125903):
                _, _, t, nd = sd.process_bulk(dev(np.ascontiguousarray(x[pos:pos + m])), want_output=False, tags_cap=4096)
                t = t.copy()
                t["index"] += pos
                tags.append(t)
                pos += nd
            got[kind] = np.concatenate(tags)
        monkeypatch.delenv("GR4PM_SD_SEPARATE_MEDIAN", raising=False)
        assert same_tags(got["wave"], got["split"]), thr
        ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=thr)
        _, ref_out, ref_tags = ref.process(x, tags_cap=4096)
        lim = min(pos, ref_out.size) - 2 * 768 - 1
        assert np.array_equal(got["wave"]["index"][got["wave"]["index"] < lim], ref_tags["index"][ref_tags["index"] < lim]), thr


def test_syncword_detection_awgn_threshold_and_noise_only(pkg):
    """default threshold 9.5, bursts in AWGN: same detections (incl. none on noise) as the oracle"""
    rng = np.random.default_rng(77)
    locations = [500, 9000, 20000, 33000]
    x, rrc = sig.qa_syncword_stream(40000, locations, -0.012, seed=8)
    x = (0.5 * x + sig.awgn(x.size, 0.3, 9)).astype(np.complex64)
    x[70000:110000] = sig.awgn(40000, 0.3, 10)  # noise-only stretch
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5)
    _, ref_out, ref_tags, ref_zpow, _ = ref.process(x, debug=True)
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5, max_items=x.size)
    st, out, tags, n = sd.process_bulk(dev(x))
    assert n == ref_out.size and np.array_equal(bits(host(out)), bits(ref_out))
    assert_tags_match(tags, ref_tags, rtol=2e-4)
    assert tags.size >= 3


def test_syncword_detection_two_samples_per_symbol_long_stride(pkg):
    """samples_per_symbol = 2: the template is 63 * 2 + 23 = 149 samples, the overlap-save stride 2048 - 149 + 1 = 1900.
    Above a stride of 1793 the lags held by output registers 1 .. 3 of the correlator are stored, i.e. the kernel
    variant that computes all 32 registers runs (the default stride, 1752, takes the one that leaves them out):
    powers, pass-through samples and tags against the oracle, in one call and in chunks"""
    locations = [300, 4100, 9000, 15000, 22222]
    x, rrc = sig.qa_syncword_stream(30000, locations, 0.01, seed=21, sps=2)
    x = (0.6 * x + sig.awgn(x.size, 0.15, 22)).astype(np.complex64)
    kw = dict(samples_per_symbol=2, power_threshold=9.5)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, **kw)
    _, ref_out, ref_tags, ref_zpow, _ = ref.process(x, debug=True)
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, max_items=x.size, **kw)
    st, out, tags, n = sd.process_bulk(dev(x))
    assert n == ref_out.size and n % 1900 == 0 and np.array_equal(bits(host(out)), bits(ref_out))
    assert_tags_match(tags, ref_tags, rtol=2e-4)
    assert tags.size >= 4
    zpow = host(sd.last_zpow(n))[0]
    assert np.max(np.abs(zpow - ref_zpow)) / np.max(ref_zpow) < 2e-6  # every lag of every block, incl. 1793 .. 1899
    sd2 = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, max_items=x.size, **kw)
    pos, all_tags = 0, []
    for m in (20000, 7000, x.size):
        st, out2, t2, n2 = sd2.process_bulk(dev(x[pos:min(pos + m, x.size)]))
        t2 = t2.copy()
        t2["index"] += pos
        all_tags.append(t2)
        pos += n2
        if pos + 2048 > x.size:
            break
    got = np.concatenate(all_tags)
    assert same_tags(got[: tags.size], tags[: got.size])


def test_syncword_detection_zero_input_and_short_input(pkg):
    """benchmark_syncword_detection.cpp feeds zeros: no tags, zeros out; < fft_size -> INSUFFICIENT"""
    rrc, _ = orc.unit_norm_rrc(4)
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, max_items=1 << 17)
    st, out, tags, n = sd.process_bulk(torch.zeros(2047, dtype=torch.complex64, device="cuda"))
    assert st == 1 and n == 0                                              # hpp:215-227
    z = torch.zeros(100000, dtype=torch.complex64, device="cuda")
    st, out, tags, n = sd.process_bulk(z)
    assert st == 0 and n == ((100000 - 2048) // 1752 + 1) * 1752 and tags.size == 0
    assert torch.count_nonzero(out).item() == 0


def test_syncword_detection_invalid_settings_raise(pkg):
    rrc, _ = orc.unit_norm_rrc(4)
    with pytest.raises(pkg.Gr4pmError, match="min_freq_bin"):             # hpp:145-147
        pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, 2, 1)
    with pytest.raises(pkg.Gr4pmError, match="fft_size too small"):       # hpp:150-152
        pkg.SyncwordDetection(rrc, np.tile(sig.SYNCWORD, 9), sig.BPSK, 0, 0)


def test_syncword_detection_multichannel_batch(pkg):
    """independent channels in one launch == each channel alone"""
    chans, refs = [], []
    rrc, _ = orc.unit_norm_rrc(4)
    for c in range(3):
        x, _ = sig.qa_syncword_stream(30000, [200 + 700 * c, 9000 + 13 * c, 20000], 0.004 * (c - 1), seed=40 + c)
        chans.append(x)
        ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0)
        refs.append(ref.process(x))
    X = np.stack(chans)
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=20.0, n_channels=3,
                               max_items=X.shape[1])
    st, out, tags, n = sd.process_bulk(dev(X))
    out = host(out)
    for c in range(3):
        _, ref_out, ref_tags = refs[c]
        assert n == ref_out.size and np.array_equal(bits(out[c]), bits(ref_out))
        assert_tags_match(tags[c], ref_tags)


# ------------------------------------------------------------------ rotators
def test_rotator_bit_exact_and_reference_qa(pkg):
    """test/qa_rotator.cpp:16-45 + bit-exact vs the oracle's serial recurrence"""
    n = 100000
    x = np.ones(n, dtype=np.complex64)
    y = host(pkg.Rotator(0.1).process_bulk(dev(x)))
    assert np.max(np.abs(y - np.exp(1j * np.float64(np.float32(0.1)) * np.arange(n)))) < 5e-4
    assert np.array_equal(bits(y), bits(orc.rotator(x, np.float32(0.1))))
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(5000) + 1j * rng.standard_normal(5000)).astype(np.complex64)
    r = pkg.Rotator(-0.3217)
    y1 = host(r.process_bulk(dev(x[:1237])))
    y2 = host(r.process_bulk(dev(x[1237:])))                               # state carried across calls
    assert np.array_equal(bits(np.concatenate([y1, y2])), bits(orc.rotator(x, np.float32(-0.3217))))


@pytest.mark.parametrize("delay", [0, 26])
def test_coarse_frequency_correction(pkg, delay):
    """test/qa_coarse_frequency_correction.cpp:15-92 (delay 0) and the receiver's delay 26"""
    n = 10000
    x = np.ones(n, dtype=np.complex64)
    tags = np.zeros(5, dtype=pkg.TAG_DTYPE)
    tags["index"] = [100, 1000, 1500, 5000, 6500]
    tags["freq"] = [0.1, 0.1, 0.1, 0.0, 0.2]
    tags["flags"] = pkg.TAG_SYNCWORD
    y = host(pkg.CoarseFrequencyCorrection(delay).process_bulk(dev(x), tags))
    want = orc.coarse_frequency_correction(x, tags["index"], tags["freq"], delay=delay)
    assert np.array_equal(bits(y), bits(want))
    if delay == 0:
        assert np.all(y[:100] == 1.0) and np.all(y[5000:6500] == 1.0)
        for start, end, fr in [(100, 1000, 0.1), (1000, 1500, 0.1), (1500, 5000, 0.1), (6500, n, 0.2)]:
            k = np.arange(end - start)
            assert np.max(np.abs(y[start:end] - np.exp(-1j * np.float64(np.float32(fr)) * k))) < 1e-3


def test_coarse_frequency_correction_pending_delay_across_calls(pkg):
    rng = np.random.default_rng(2)
    x = (rng.standard_normal(4000) + 1j * rng.standard_normal(4000)).astype(np.complex64)
    idx, fr = np.array([990, 2000, 2010], dtype=np.uint64), np.array([0.05, -0.02, 0.07])
    want = orc.coarse_frequency_correction(x, idx, fr, delay=26)
    cfc = pkg.CoarseFrequencyCorrection(26)
    outs = []
    for a, b in [(0, 1000), (1000, 2005), (2005, 4000)]:
        t = np.zeros(0, dtype=pkg.TAG_DTYPE)
        sel = (idx >= a) & (idx < b)
        t = np.zeros(sel.sum(), dtype=pkg.TAG_DTYPE)
        t["index"], t["freq"], t["flags"] = idx[sel] - a, fr[sel], pkg.TAG_SYNCWORD
        outs.append(host(cfc.process_bulk(dev(x[a:b]), t)))
    assert np.array_equal(bits(np.concatenate(outs)), bits(want))


@pytest.mark.parametrize("delay", [0, 26])
def test_coarse_frequency_correction_many_ragged_segments(pkg, delay):
    """hundreds of set_freq tags at ragged distances (shorter than a checkpoint chunk, longer than the 512-sample
    renormalisation period, one carried over a call boundary): the checkpoint kernel and the parallel apply
    against the oracle bit for bit, in one call and split in three"""
    rng = np.random.default_rng(400 + delay)
    n = 400000
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    gaps = np.concatenate([rng.integers(1, 40, 150), rng.integers(40, 3000, 350), rng.integers(400, 700, 100)])
    rng.shuffle(gaps)
    idx = np.cumsum(gaps)
    idx = idx[idx < n - 10].astype(np.uint64)
    fr = rng.uniform(-0.04, 0.04, idx.size)
    want = orc.coarse_frequency_correction(x, idx, fr, delay=delay)
    tags = np.zeros(idx.size, dtype=pkg.TAG_DTYPE)
    tags["index"], tags["freq"], tags["flags"] = idx, fr, pkg.TAG_SYNCWORD
    y = host(pkg.CoarseFrequencyCorrection(delay).process_bulk(dev(x), tags))
    assert np.array_equal(bits(y), bits(want))
    cfc = pkg.CoarseFrequencyCorrection(delay)
    outs = []
    for a, b in [(0, 100003), (100003, 250000), (250000, n)]:
        t = tags[(tags["index"] >= a) & (tags["index"] < b)].copy()
        t["index"] -= a
        outs.append(host(cfc.process_bulk(dev(x[a:b]), t)))
    assert np.array_equal(bits(np.concatenate(outs)), bits(want))


@pytest.mark.gpu
def test_device_sincosf_is_glibc_bit_exact(pkg):
    """the Costas loop's local oscillator: sinf / cosf on the device against the host libm the reference calls
    (costas_loop.hpp:113-115), bit for bit -- dense around the quadrant boundaries, the tiny-argument cut,
    and 2^24 random phases of the loop's range"""
    rng = np.random.default_rng(1)
    parts = [rng.uniform(-3.2, 3.2, 1 << 24).astype(np.float32), np.float32([0.0, -0.0, np.pi, -np.pi, 3.2, -3.2, 1e-30, 2.0 ** -12])]
    for c in (np.pi / 4, np.pi / 2, 3 * np.pi / 4, np.pi, 2.0 ** -12, 2.0 ** -126):
        base = np.float32(c)
        near = base.view(np.uint32) + np.arange(-4096, 4096, dtype=np.int64)
        parts += [near.astype(np.uint32).view(np.float32), -near.astype(np.uint32).view(np.float32)]
    x = np.concatenate(parts).astype(np.float32)
    s, c = pkg.sincosf(x)
    rs, rc = orc.sincosf(x)
    ds, dc = int(np.sum(s.view(np.uint32) != rs.view(np.uint32))), int(np.sum(c.view(np.uint32) != rc.view(np.uint32)))
    print("sincosf: differing sin", ds, "cos", dc, "of", x.size)
    assert ds == 0 and dc == 0


def test_device_costas_phase_wrap_is_exact(pkg):
    """costas_loop.hpp:141-145 (phase >= pi: - 2 pi, phase < -pi: + 2 pi, in float) as the kernels evaluate it -- two
    fused multiply-adds with the clamp modifier instead of compares -- on every float within 4096 ulps of +-pi, of
    +-2 pi and of +-3 pi, the signed zeros, tiny values and 2^22 random phases"""
    pi = np.float32(3.14159265358979323846)
    two_pi = np.float32(2.0) * pi
    rng = np.random.default_rng(2)
    parts = [rng.uniform(-10.0, 10.0, 1 << 22).astype(np.float32),
             np.float32([0.0, -0.0, 1e-30, -1e-30, pi, -pi, two_pi, -two_pi, 3.0, -3.0, 9.5, -9.5])]
    for c in (pi, two_pi, np.float32(3.0) * pi):
        near = np.float32(c).view(np.uint32) + np.arange(-4096, 4097, dtype=np.int64)
        parts += [near.astype(np.uint32).view(np.float32), -near.astype(np.uint32).view(np.float32)]
    x = np.concatenate(parts).astype(np.float32)
    want = np.where(x >= pi, x - two_pi, np.where(x < -pi, x + two_pi, x)).astype(np.float32)
    got = pkg.costas_phase_wrap(x)
    bad = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
    print("phase wrap: differing", bad, "of", x.size)
    assert bad == 0


# ------------------------------------------------------------------ Costas
@pytest.mark.parametrize("constellation", ["PILOT", "BPSK", "QPSK"])
def test_costas_loop(pkg, constellation):
    """test/qa_costas_loop.cpp:17-65 + oracle comparison"""
    rng = np.random.default_rng(13)
    n = 100000
    if constellation == "PILOT":
        x = np.ones(n, dtype=np.complex64)
    elif constellation == "BPSK":
        x = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0).astype(np.complex64)
    else:
        a = np.float32(np.sqrt(0.5))
        x = (np.where(rng.integers(0, 2, n) == 0, a, -a) + 1j * np.where(rng.integers(0, 2, n) == 0, a, -a)).astype(np.complex64)
    rot = orc.rotator(x, np.float32(0.01))
    cl = pkg.CostasLoop(0.01, constellation)
    assert cl.coeffs == orc.costas_coeffs(0.01, constellation)
    y = host(cl.process_bulk(dev(rot)))
    assert np.all(np.abs(y[1000:] * np.conj(x[1000:]) - 1.0) < 1e-2)       # qa :56-62
    want = orc.costas_loop(rot, constellation)
    print("costas max |gpu - oracle| =", np.max(np.abs(y - want)), "differing items:", int(np.sum(bits(y) != bits(want))))
    assert np.array_equal(bits(y), bits(want))  # north_star: <= 1 ULP; measured: 0 ULP (glibc sinf / cosf restated in double)


def test_costas_loop_phase_tags_and_carry(pkg):
    rng = np.random.default_rng(14)
    n = 20000
    x = np.where(rng.integers(0, 2, n) == 0, 1.0, -1.0).astype(np.complex64)
    x = (x * np.exp(1j * 0.7) + sig.awgn(n, 0.1, 15)).astype(np.complex64)
    idx = np.array([0, 5000, 5001, 12000], dtype=np.uint64)
    ph = np.array([0.7, 0.6, 0.8, -2.4], dtype=np.float32)
    want = orc.costas_loop(x, "BPSK", 0.01, idx, ph)
    cl = pkg.CostasLoop(0.01, "BPSK")
    outs = []
    for a, b in [(0, 7000), (7000, n)]:
        sel = (idx >= a) & (idx < b)
        t = np.zeros(sel.sum(), dtype=pkg.TAG_DTYPE)
        t["index"], t["phase"], t["flags"] = idx[sel] - a, ph[sel], pkg.TAG_SYNCWORD
        outs.append(host(cl.process_bulk(dev(x[a:b]), t)))
    assert np.array_equal(bits(np.concatenate(outs)), bits(want))


# ------------------------------------------------------------------ wipe-off / SDF
def test_syncword_wipeoff(pkg):
    """test/qa_syncword_wipeoff.cpp:13-48 (c64 items)"""
    n = 1000
    ramp = np.arange(n).astype(np.complex64)
    bipolar = np.where(sig.SYNCWORD == 1, -1.0, 1.0).astype(np.float32)
    v = ramp.copy()
    idx = [10, 100, 250]
    for i in idx:
        v[i:i + 64] *= bipolar
    tags = np.zeros(4, dtype=pkg.TAG_DTYPE)
    tags["index"], tags["flags"] = idx + [260], pkg.TAG_SYNCWORD           # 260: inside a syncword -> ignored
    w = pkg.SyncwordWipeoff(bipolar)
    y = np.concatenate([host(w.process_bulk(dev(v[:270]), tags)),          # call boundary inside the 3rd syncword
                        host(w.process_bulk(dev(v[270:]), None))])
    assert np.array_equal(y, ramp)
    assert np.array_equal(bits(y), bits(orc.syncword_wipeoff(v, bipolar, idx + [260])))


def test_syncword_detection_filter(pkg):
    """test/qa_syncword_detection_filter.cpp:14-61"""
    num_items = 100000
    v = np.arange(num_items).astype(np.complex64)
    vd = dev(v)
    tag_idx = [12345, 14345]
    f = pkg.SyncwordDetectionFilter()
    out = torch.zeros(num_items, dtype=torch.complex64, device="cuda")
    out_tags, pos = [], 0
    bounds = sorted(set([0] + tag_idx + [num_items]))
    while pos < num_items:
        nxt = min(b for b in bounds if b > pos)
        flags = pkg.TAG_SYNCWORD if pos in tag_idx else 0
        c, hc, ic, tf = f.process_bulk(vd[pos:nxt], out[pos:nxt], flags, headers=[1500])
        if tf:
            out_tags.append((pos, tf))
        assert c > 0
        pos += c
    assert np.array_equal(host(out), v)
    assert out_tags == [(12345, pkg.TAG_SYNCWORD)]


# ------------------------------------------------------------------ FIR family
def test_interpolating_fir_filter(pkg):
    """test/qa_interpolating_fir_filter.cpp:16-55 (exact vs zero-stuffed convolution, integer-valued
    floats) + bit-exact vs the oracle on c64 with the RRC taps, state carried across calls"""
    rng = np.random.default_rng(12)
    n, interp = 100000, 5
    v = rng.integers(-8, 9, n).astype(np.float32)
    taps = np.arange(1, 24, dtype=np.float32)
    got = host(pkg.InterpolatingFirFilter(interp, taps, "float32").process_bulk(dev(v)))
    stuffed = np.zeros(n * interp)
    stuffed[::interp] = v
    assert np.array_equal(got.astype(np.float64), np.convolve(stuffed, taps.astype(np.float64))[: n * interp])
    rrc, _ = orc.unit_norm_rrc(4)
    x = (rng.standard_normal(30000) + 1j * rng.standard_normal(30000)).astype(np.complex64)
    f = pkg.InterpolatingFirFilter(4, rrc)
    y = np.concatenate([host(f.process_bulk(dev(x[:7]))), host(f.process_bulk(dev(x[7:11111]))),
                        host(f.process_bulk(dev(x[11111:])))])
    assert np.array_equal(bits(y), bits(orc.interpolating_fir(x, 4, rrc)))


@pytest.mark.parametrize("interp,ntaps,dtype", [
    (4, 1025, "complex64"),   # configs[4]'s shaping filter: arms of 257 / 256 taps, longer than one 256-item tile's reach
    (4, 2049, "complex64"),   # arms of 513 taps: two tiles of history
    (5, 23, "complex64"),     # L * arm_stride = 25: odd, the item tile must still be 8-byte aligned in LDS
    (3, 9, "complex64"),      # L * arm_stride = 9
    (7, 100, "float32"),      # ragged arms (15, 15, 14, ...), not the L == 4 path
    (4, 1025, "float32"),
])
def test_interpolating_fir_filter_long_arms_and_odd_layouts(pkg, interp, ntaps, dtype):
    """interpolating_fir_filter.hpp:76-102 at the sizes k_interp_fir was rewritten for: every output against the
    oracle bit for bit, history carried over calls of 1 .. several thousand items (shorter than an arm, shorter than
    a tile, several tiles)"""
    rng = np.random.default_rng(ntaps * 10 + interp)
    taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    n = 9000
    if dtype == "complex64":
        x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    else:
        x = rng.standard_normal(n).astype(np.float32)
    want = orc.interpolating_fir(x, interp, taps)
    f = pkg.InterpolatingFirFilter(interp, taps, dtype)
    cuts = [0, 1, 3, 200, 255, 256, 257, 700, 2500, 2501, 6000, n]
    got = np.concatenate([host(f.process_bulk(dev(x[a:b]))) for a, b in zip(cuts[:-1], cuts[1:])])
    assert got.size == want.size
    if dtype == "complex64":
        assert np.array_equal(bits(got), bits(want))
    else:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the same through the oracle call by call (its history is carried the same way)
    o = orc.InterpolatingFir(interp, taps)
    assert np.array_equal(np.concatenate([o.process(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]), want)


def test_interpolating_fir_filter_lds_limit_is_reported(pkg):
    """the tile + taps of one workgroup must fit the CU's LDS: a filter that cannot is refused, not mis-launched"""
    taps = np.ones(64 * 1024, dtype=np.float32)
    f = pkg.InterpolatingFirFilter(4, taps)
    with pytest.raises(pkg.Gr4pmError, match="LDS"):
        f.process_bulk(dev(np.ones(1000, dtype=np.complex64)))


def test_symbol_filter_32x1025_taps_with_tags(pkg):
    """configs[4]'s receiving filter (bench.py --config 5): SymbolFilter with 32 arms x 1025 taps, delay 1025,
    c64 items, tag-driven clock phase (symbol_filter.hpp:112-252) -- the generic kernel (k_symbol_filter), not the
    receiver's 44-tap fast path but, since round 4, k_symbol_filter_long; outputs and re-timed tags bit for bit against
    the oracle, one call and split calls"""
    pfb = orc.rrc_taps(32.0, 128.0, 1.0, 0.35, 32 * 1024)   # 32769 taps: arms of 1025 (arm 0) and 1024 taps
    assert pfb.size == 32 * 1024 + 1
    rng = np.random.default_rng(1025)
    n = 40000
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    idx = [0, 3001, 6002, 6500, 12000, 12003, 20444, 25557, 31000, 31001, 39998]
    tags = np.zeros(len(idx), dtype=pkg.TAG_DTYPE)
    tags["index"] = idx
    tags["amplitude"] = rng.uniform(0.5, 2.0, len(idx))
    tags["time_est"] = [0.1, -0.2, 0.49, -0.5, 0.0, -0.01, 0.3, -0.3, 0.5, 0.2, -0.45]
    tags["phase"] = rng.uniform(-3, 3, len(idx))
    tags["freq"] = rng.uniform(-0.03, 0.03, len(idx))
    tags["flags"] = pkg.TAG_SYNCWORD
    tags["flags"][4] = pkg.TAG_OTHER
    want, want_tags, want_cons = orc.symbol_filter(x, pfb, 32, 4, 1025, tags=tags.astype(orc.TAG_DTYPE))
    for cuts in ([0, n], [0, 2500, 2501, 13000, 31001, n]):
        f = pkg.SymbolFilter(pfb, 32, 4, 1025)
        ys, ts, cons, produced = [], [], 0, 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            t = tags[(tags["index"] >= a) & (tags["index"] < b)].copy()
            t["index"] -= a
            y, to, c = f.process_bulk(dev(x[a:b]), t)
            assert c == b - a
            to = to.copy()
            to["index"] += produced
            produced += y.numel()
            ys.append(host(y))
            ts.append(to)
            cons += c
        y, t = np.concatenate(ys), np.concatenate(ts)
        assert cons == want_cons == n and y.size == want.size
        assert np.array_equal(bits(y), bits(want))
        assert t.size == want_tags.size
        for k in ("index", "amplitude", "phase", "freq", "time_est", "flags"):
            assert np.array_equal(t[k], want_tags[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("n_taps,num_arms", [(64 * 8, 8), (64 * 8 + 1, 8), (64 * 8 + 2, 8), (64 * 8 + 3, 8), (65 * 8 + 5, 8), (129 * 4, 4),
                                             (257 * 3 + 1, 3), (2049, 1)])
def test_symbol_filter_long_arms_all_layouts(pkg, n_taps, num_arms):
    """k_symbol_filter_long (plain SymbolFilter, complex items, 4 samples per symbol, arms of 64 taps and more): every
    layout of its tap walk -- 1 .. 4 head taps on the top tap position ((arm_size - 1) % 4), an even and an odd number
    of whole tap positions behind them, arms of different lengths inside one filter (n_taps not a multiple of
    num_arms), one and two passes left over after the two-pass loop -- with tags that change arm, scale and clock
    phase and a symbol count that leaves the last workgroup and the last lane half empty: bit for bit the oracle's"""
    rng = np.random.default_rng(n_taps)
    taps = rng.standard_normal(n_taps).astype(np.float32)
    n = 4 * 1501 + 3
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    idx = [0, 777, 2500, 4001, 5998]
    tags = np.zeros(len(idx), dtype=pkg.TAG_DTYPE)
    tags["index"] = idx
    tags["amplitude"] = rng.uniform(0.5, 2.0, len(idx))
    tags["time_est"] = [0.3, -0.2, 0.49, -0.45, 0.05]
    tags["flags"] = pkg.TAG_SYNCWORD
    delay = 37
    want, want_tags, want_cons = orc.symbol_filter(x, taps, num_arms, 4, delay, tags=tags.astype(orc.TAG_DTYPE))
    f = pkg.SymbolFilter(taps, num_arms, 4, delay)
    y, t, cons = f.process_bulk(dev(x), tags)
    assert cons == want_cons and y.numel() == want.size
    assert np.array_equal(bits(host(y)), bits(want))
    assert np.array_equal(t["index"], want_tags["index"])


def test_symbol_filter_free_running_reference_qa(pkg):
    """test/qa_symbol_filter.cpp:17-63 (float items, no tags) + bit-exact vs oracle"""
    num_symbols = 200000
    rng = np.random.default_rng(11)
    sym = np.where(rng.integers(0, 2, num_symbols) == 0, 1.0, -1.0).astype(np.float32)
    x = orc.interpolating_fir(sym, 4, orc.rrc_taps(1.0, 4.0, 1.0, 0.35, 44))
    pfb = orc.rrc_taps(32.0, 128.0, 1.0, 0.35, 32 * 4 * 11)
    y, _, consumed = pkg.SymbolFilter(pfb, 32, 4, 0, "float32").process_bulk(dev(x))
    y = host(y)
    assert y.size == num_symbols and consumed == x.size
    assert np.all(np.abs(np.abs(y[11:]) - 0.24819523) < 5e-3)
    want, _, _ = orc.symbol_filter(x, pfb, 32, 4, 0)
    assert np.array_equal(bits(y), bits(want))


def _receiver_pfb():
    rrc, norm = orc.unit_norm_rrc(4)
    pfb = orc.rrc_taps(32.0 / float(norm), 128.0, 1.0, 0.35, 32 * 4 * 11)[:-1]  # packet_receiver.hpp:100-110
    return rrc, pfb


@pytest.mark.parametrize("split", [None, 2501])
def test_symbol_filter_with_tags_all_clock_phase_cases(pkg, split):
    """tag-driven path (symbol_filter.hpp:130-206), untested upstream: all special cases of the
    clock phase, negative time_est, tag re-timing; c64 items as in the receiver"""
    rrc, pfb = _receiver_pfb()
    rng = np.random.default_rng(31)
    n = 12000
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    idx = [0, 1001, 2002, 2500, 3000, 3003, 4444, 5557, 7000, 7001, 9998]
    tags = np.zeros(len(idx), dtype=pkg.TAG_DTYPE)
    tags["index"] = idx
    tags["amplitude"] = rng.uniform(0.5, 2.0, len(idx))
    tags["time_est"] = [0.1, -0.2, 0.49, -0.5, 0.0, -0.01, 0.3, -0.3, 0.5, 0.2, -0.45]
    tags["phase"] = rng.uniform(-3, 3, len(idx))
    tags["freq"] = rng.uniform(-0.03, 0.03, len(idx))
    tags["flags"] = pkg.TAG_SYNCWORD
    tags["flags"][4] = pkg.TAG_OTHER                                       # a non-syncword tag is only re-timed
    otags = tags.astype(orc.TAG_DTYPE)
    want, want_tags, want_cons = orc.symbol_filter(x, pfb, 32, 4, 44, tags=otags)
    f = pkg.SymbolFilter(pfb, 32, 4, 44)
    if split is None:
        y, t, cons = f.process_bulk(dev(x), tags)
        y = host(y)
    else:
        ta = tags[tags["index"] < split]
        tb = tags[tags["index"] >= split].copy()
        tb["index"] -= split
        y1, t1, c1 = f.process_bulk(dev(x[:split]), ta)
        y2, t2, c2 = f.process_bulk(dev(x[split:]), tb)
        assert c1 == split
        t2 = t2.copy()
        t2["index"] += y1.numel()
        y, t, cons = np.concatenate([host(y1), host(y2)]), np.concatenate([t1, t2]), c1 + c2
    assert cons == want_cons == n and y.size == want.size
    assert np.array_equal(bits(y), bits(want))
    assert t.size == want_tags.size
    for k in ("index", "amplitude", "phase", "freq", "time_est", "flags"):
        assert np.array_equal(t[k], want_tags[k]), k


def test_pfb_arb_resampler(pkg):
    """test/qa_pfb_arb_resampler.cpp:16-70 (TRate = double) + bit-exact vs oracle, both TRate"""
    n, rate, f = 100000, 1.1234, 0.01
    taps = pkg.default_pfb_arb_taps()
    x = np.exp(1j * f * np.arange(n)).astype(np.complex64)
    y, cons = pkg.PfbArbResampler(rate, None, 32, "float64").process_bulk(dev(x))
    y = host(y)
    assert abs(y.size - n * rate) <= 5                                      # qa :45-49
    k = np.arange(1000, y.size)
    phase0 = np.angle(y[1000])
    assert np.max(np.abs(y[1000:] - np.exp(1j * (phase0 + (f / rate) * (k - 1000))))) < 3e-3   # qa :50-69
    want, wcons = orc.pfb_arb_resampler(x, rate, taps, 32, rate_is_double=True)
    assert cons == wcons and np.array_equal(bits(y), bits(want))
    r = pkg.PfbArbResampler(1.0 + 1.2e-6, taps, 32, "float32")
    y1, c1 = r.process_bulk(dev(x[:40001]))
    y2, c2 = r.process_bulk(dev(x[c1:]))
    want, _ = orc.pfb_arb_resampler(x, 1.0 + 1.2e-6, taps, 32, rate_is_double=False)
    got = np.concatenate([host(y1), host(y2)])
    assert np.array_equal(bits(got), bits(want[: got.size])) and abs(got.size - want.size) <= 1


@pytest.mark.parametrize("rate_dtype", ["float64", "float32"])
@pytest.mark.parametrize("rate", [0.37, 0.7, 1.0 - 50e-6, 1.0 + 50e-6, 1.1234, 3.3, 40.5, 0.011])
def test_pfb_arb_resampler_random_calls(pkg, rate, rate_dtype):
    """pfb_arb_resampler.hpp:122-182 call by call against the oracle with ITS state carried the same way: random
    input span sizes (1 item .. thousands), random output span sizes (full, cut inside a 64-output chunk of the
    device plan, one item), rates below and above 1 (decim_rate from 0 to 2900 = 90 filter_size): consumed, produced
    and every output bit for bit in every call.  The serial plan lane takes q0 or q0 + 1 items per output and one
    division per 64 outputs (k_arb_plan); its first pass and the passes near either span's end run the loop as
    written -- all of them are crossed here."""
    taps = pkg.default_pfb_arb_taps()
    is_double = rate_dtype == "float64"
    rng = np.random.default_rng(int(rate * 1000) + (7 if is_double else 0))
    n = 60000 if rate < 5 else 8000
    f = 0.02
    x = (np.exp(1j * f * np.arange(n)) + 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    r = pkg.PfbArbResampler(rate, taps, 32, rate_dtype)
    o = orc.PfbArbResampler(rate, taps, 32, rate_is_double=is_double)
    pos, calls, produced = 0, 0, 0
    while pos < n and calls < 60:
        kind = calls % 6
        n_in = int(rng.integers(1, 6)) if kind == 5 else int(rng.integers(1, 4000 if rate < 5 else 300))
        n_in = min(n_in, n - pos)
        full = int(n_in * rate) + 64
        if kind == 0:
            out_cap = full
        elif kind == 1:
            out_cap = max(1, int(full * rng.uniform(0.2, 0.9)))        # the output span runs out first
        elif kind == 2:
            out_cap = 64 * int(rng.integers(1, 8)) + int(rng.integers(1, 63))  # ends inside a 64-output chunk
        elif kind == 3:
            out_cap = 1
        else:
            out_cap = full
        want, wcons = o.process(x[pos:pos + n_in], out_cap)
        y, cons = r.process_bulk(dev(x[pos:pos + n_in]), out_cap=out_cap)
        y = host(y)
        assert cons == wcons and y.size == want.size, (calls, kind, n_in, out_cap, cons, wcons, y.size, want.size)
        assert np.array_equal(bits(y), bits(want)), (calls, kind, n_in, out_cap)
        pos += cons
        produced += y.size
        calls += 1
        if cons == 0 and y.size == 0:
            break
    assert calls >= 20 and produced > 500


def test_pfb_arb_resampler_tiny_rate_is_refused(pkg):
    """decim_rate / filter_size >= 2^30 would wrap the plan's 32-bit item counts: reported, not mis-computed"""
    r = pkg.PfbArbResampler(1e-10, None, 32, "float64")
    with pytest.raises(pkg.Gr4pmError, match="rate too small"):
        r.process_bulk(dev(np.ones(100, dtype=np.complex64)), out_cap=8)


# ------------------------------------------------------------------ SDF gate + receiver chain
def test_syncword_detection_filter_gate_matches_process(pkg):
    """the copy-free tag gate == the per-chunk state machine (syncword_detection_filter.hpp:75-185)
    driven chunk by chunk with the header message of the open packet pending"""
    rng = np.random.default_rng(5)
    total = 400000
    idx = np.sort(rng.choice(total - 10, 60, replace=False) + 1).astype(np.uint64)
    lens = [int(rng.integers(1, 3000)) if rng.random() > 0.2 else None for _ in idx]
    acc, _ = pkg.SyncwordDetectionFilter().gate(idx, lens, per_tag=True)
    f = orc.SyncwordDetectionFilter()
    want, pending = [], []
    bounds = [0] + [int(i) for i in idx] + [total]
    for k in range(len(bounds) - 1):
        a, b = bounds[k], bounds[k + 1]
        first = True
        while a < b:
            flags = 1 if (k > 0 and first) else 0
            st, o, c, hc, ic, tf = f.process(np.zeros(b - a, np.complex64), b - a, flags, headers=pending, n_ignored=0)
            if flags:
                want.append(bool(tf & 1))
                if tf & 1:  # accepted: from now on the decoder's answer for THIS packet is pending
                    pending = [lens[k - 1]]
                    hc = 0
            if hc:
                pending = []
            first = False
            a += c
            if c == 0:  # stalled waiting for the header of the packet just accepted
                assert pending
    assert acc.tolist() == want


def test_packet_receiver_front_end_chain(pkg):
    """PacketReceiver wiring (packet_receiver.hpp:34-127): every stage bit-exact against the oracle
    stage fed with the same tags; detector tags against the oracle detector within tolerance"""
    rng = np.random.default_rng(91)
    sps, n_pkt = 4, 6
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
    x = (orc.rotator(x, np.float32(0.011)) + sig.awgn(x.size, 0.05, 92)).astype(np.complex64)
    rx = pkg.PacketReceiver(max_items=x.size)

    def header_fn(tag):
        # the header decode is outside the hot path: look the length up from the known layout
        sym_idx = (int(tag["index"]) - 1537) / sps
        k = int(np.argmin([abs(s - sym_idx) for s, _ in starts]))
        return starts[k][1]

    res = rx.process_bulk(dev(x), header_fn)
    det = res["detector_tags"]
    assert det.size == n_pkt and np.all(res["accepted"])
    assert np.array_equal(det["index"], [1537 + sps * s for s, _ in starts])
    # detector vs oracle detector
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5)
    _, ref_out, ref_tags = ref.process(x)
    assert_tags_match(det, ref_tags, rtol=2e-4)
    # downstream stages: oracle fed with the GPU's own tags must agree (Costas: device sincos)
    otags = det.astype(orc.TAG_DTYPE)
    z = orc.coarse_frequency_correction(ref_out, det["index"], det["freq"], delay=26)
    pfb = orc.rrc_taps(32.0 / float(orc.unit_norm_rrc(sps)[1]), 128.0, 1.0, 0.35, 32 * sps * 11)[:-1]
    sym, sym_tags, _ = orc.symbol_filter(z, pfb, 32, sps, 44, tags=otags)
    bipolar = np.where(sig.SYNCWORD == 1, -1.0, 1.0).astype(np.float32)
    w = orc.syncword_wipeoff(sym, bipolar, sym_tags["index"])
    c = orc.costas_loop(w, "QPSK", 0.01, sym_tags["index"], sym_tags["phase"])
    got = host(res["symbols"])
    assert got.size == c.size
    assert np.array_equal(res["tags"]["index"], sym_tags["index"])
    assert np.array_equal(bits(got), bits(c))
    # and the chain does its job: once the loop has locked, payload symbols sit on the QPSK points
    for t in sym_tags:
        s0 = int(t["index"]) + 64 + 40
        pts = got[s0:s0 + 60]
        assert np.max(np.abs(np.abs(pts.real) - a)) < 0.3 and np.max(np.abs(np.abs(pts.imag) - a)) < 0.3


@pytest.mark.parametrize("pipelined", [False, True])
def test_packet_receiver_soft_bits(pkg, pipelined):
    """PacketReceiver(soft_bits=True): IQ samples in, LLRs of header + payload out
    (packet_receiver.hpp:34-131,191-247).  The transmitted bits come back, and the symbol-rate
    tail agrees with the oracle tail fed with the same symbol-rate tags."""
    rng = np.random.default_rng(191)
    sps, n_pkt = 4, 5
    rrc, _ = orc.unit_norm_rrc(sps)
    a = np.float32(np.sqrt(0.5))
    syms, starts, tx_bits = [], [], []
    for k in range(n_pkt):
        gap = np.zeros(int(rng.integers(300, 900)), dtype=np.complex64)
        payload_len = int(rng.integers(10, 200))
        nb = 128 + (payload_len + 4) * 4
        b = rng.integers(0, 2, (nb, 2))
        body = ((1 - 2 * b[:, 0]) * a + 1j * (1 - 2 * b[:, 1]) * a).astype(np.complex64)
        syms += [gap, sig.BPSK[sig.SYNCWORD], body]
        starts.append((sum(len(s) for s in syms[:-2]), payload_len))
        tx_bits.append(b)
    syms.append(np.zeros(1500, dtype=np.complex64))
    x = orc.interpolating_fir(np.concatenate(syms), sps, rrc)
    x = (orc.rotator(x, np.float32(0.009)) * np.exp(1j * 0.8) + sig.awgn(x.size, 0.05, 192)).astype(np.complex64)
    rx = pkg.PacketReceiver(max_items=x.size, pipelined=pipelined, soft_bits=True)

    def header_fn(tag):
        # a detection that is not on a transmitted syncword (the noise-only lead-in can produce
        # one) decodes to an invalid header, like the reference's header_parser would report
        sym_idx = (int(tag["index"]) - 1537) / sps
        k = int(np.argmin([abs(s - sym_idx) for s, _ in starts]))
        return starts[k][1] if abs(starts[k][0] - sym_idx) < 2 else None

    res = rx.process_bulk(dev(x), header_fn)
    if pipelined:
        assert res is None
        (res,) = rx.flush()
    hdrs = [header_fn(t) for t in res["detector_tags"][res["accepted"]]]
    assert sum(h is not None for h in hdrs) == n_pkt and res["ignored_syncwords"] == 0
    llr = res["llr"].cpu().numpy()
    n_false = sum(h is None for h in hdrs)   # their 128 "header" symbols pass before the verdict
    assert llr.size == 2 * (sum(128 + (p + 4) * 4 for _, p in starts) + 128 * n_false)
    lt = res["llr_tags"]
    assert int(np.sum(lt["kind"] == pkg.PKT_PAYLOAD)) == n_pkt
    assert int(np.sum(lt["kind"] == pkg.PKT_HEADER_START)) == len(hdrs)
    for b, (_, plen), ptag in zip(tx_bits, starts, lt[lt["kind"] == pkg.PKT_PAYLOAD]):
        assert ptag["packet_length"] == plen and ptag["payload_bits"] == 8 * (plen + 4)
        pos = int(ptag["index"]) - 256          # the packet's header LLRs start 128 symbols earlier
        hard = (llr[pos:pos + 2 * b.shape[0]] < 0).astype(int).reshape(-1, 2)
        assert np.array_equal(hard, b)          # header and payload bits, every one of them
    # oracle tail on the receiver's own wiped-off symbols and tags
    pt = res["packet_tags"]
    sw_tags = pt[pt["kind"] == pkg.PKT_SYNCWORD]["syncword"].astype(orc.TAG_DTYPE)
    sym_tags = res["tags"].astype(orc.TAG_DTYPE)
    assert np.array_equal(sw_tags["phase"], sym_tags["phase"])
    # rebuild the wipe-off output the tail consumed: the receiver keeps the Costas output, so run the
    # oracle tail from the oracle front end driven by the GPU's detector tags
    det = res["detector_tags"]
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5)
    _, ref_out, _ = ref.process(x)
    z = orc.coarse_frequency_correction(ref_out, det["index"], det["freq"], delay=26)
    pfb = orc.rrc_taps(32.0 / float(orc.unit_norm_rrc(sps)[1]), 128.0, 1.0, 0.35, 32 * sps * 11)[:-1]
    sym, stags, _ = orc.symbol_filter(z, pfb, 32, sps, 44, tags=det.astype(orc.TAG_DTYPE))
    w = orc.syncword_wipeoff(sym, np.where(sig.SYNCWORD == 1, -1.0, 1.0).astype(np.float32), stags["index"])
    o1 = orc.PayloadMetadataInsert(64, 128).process(w, stags, headers=hdrs)
    o2 = orc.CostasLoop(0.01, "BPSK").process(o1["out"], o1["tags"])
    o3, o3t = orc.SyncwordRemove(64).process(o2, o1["tags"])
    o4, o4t = orc.ConstellationLLRDecoder(0.7, "QPSK").process(o3, o3t)
    assert same_ptags(res["llr_tags"], o4t)
    assert np.max(np.abs(llr - o4)) < 1e-4


# ------------------------------------------------------------------ full-size properties
def test_syncword_detection_full_size_properties(pkg):
    """BASELINE size (2^28 samples, one call): properties that need no oracle --
    every inserted syncword is found at exactly delay + 4*loc with the right freq_bin, nothing
    else is found, the pass-through is the input delayed by 2T+1 (checksum of checksums), and
    processing the same stream in two calls gives the same tags (state carry at scale)."""
    n = 1 << 28
    sps, L = 4, 297
    rrc, _ = orc.unit_norm_rrc(sps)
    g = torch.Generator(device="cuda")
    g.manual_seed(123)
    # AWGN floor well below the threshold + one clean shaped syncword every ~1e6 samples
    x = torch.complex(torch.randn(n, generator=g, device="cuda"), torch.randn(n, generator=g, device="cuda")) * 0.05
    sw = orc.interpolating_fir(np.concatenate([sig.BPSK[sig.SYNCWORD], np.zeros(11, np.complex64)]), sps, rrc)[:L]
    rng = np.random.default_rng(9)
    locs = np.sort(rng.choice(np.arange(5000, n - 5000, 999_983), 200, replace=False)) // 4 * 4
    freqs = rng.uniform(-0.03, 0.03, locs.size)  # inside bins -3..3: edge bins are not interpolated (hpp:65)
    swd = dev(sw)
    k = torch.arange(L, device="cuda")
    for loc, f in zip(locs, freqs):
        x[loc:loc + L] += swd * torch.polar(torch.ones(L, device="cuda"), f * k)
    x = x.contiguous()
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5, max_items=n)
    st, out, tags, done = sd.process_bulk(x, tags_cap=4096)
    delay = 2 * sd.time_threshold + 1
    found = locs[locs + delay < done]
    assert tags.size == found.size
    assert np.array_equal(tags["index"], found + delay)
    assert np.array_equal(tags["freq_bin"], np.round(freqs[: found.size] / (np.pi / L)).astype(np.int32))
    assert np.all(np.abs(tags["freq"] - freqs[: found.size]) < 1e-3) and np.all(np.abs(tags["amplitude"] - 1.0) < 0.05)
    # pass-through: out == input delayed, compared through 64-bit checksums of 2^20-sample blocks
    xi = x.view(torch.float32).view(torch.int64)[: done - delay]
    oi = out.view(torch.float32).view(torch.int64)[delay:done]
    blk = 1 << 20
    m = (xi.numel() // blk) * blk
    assert torch.equal(xi[:m].view(-1, blk).sum(1), oi[:m].view(-1, blk).sum(1))
    assert torch.equal(xi[m:], oi[m:]) and torch.count_nonzero(out[:delay]).item() == 0
    del out
    # the same stream in two calls
    sd2 = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5, max_items=n)
    cut = (n // 3) // 1752 * 1752 + 2048
    st, _, t1, d1 = sd2.process_bulk(x[:cut].contiguous(), want_output=False, tags_cap=4096)
    st, _, t2, d2 = sd2.process_bulk(x[d1:].contiguous(), want_output=False, tags_cap=4096)
    t2 = t2.copy()
    t2["index"] += d1
    both = np.concatenate([t1, t2])
    assert d1 + d2 == done and np.array_equal(both["index"], tags["index"])
    assert np.array_equal(both["amplitude"], tags["amplitude"]) and np.array_equal(both["phase"], tags["phase"])


def test_packet_receiver_full_size_round_trip(pkg):
    """BASELINE size (2^26 samples through the complete receiver): packets made by BurstGenerator
    (1500 random bytes + CRC-32 each, carrier offset, Es/N0 = 20 dB) go through the native pipelined
    receiver in eight batches, announced two ahead (cuts land anywhere inside packets); every packet
    that lies completely inside the stream comes back byte for byte, in order, nothing else does,
    and the headers pass A predicted are the ones the chain decodes (0 mismatches)"""
    import bench
    n = 1 << 26
    x, n_pkt = bench.packet_stream(pkg, n, seed=77, device=torch.device("cuda"))
    rng = np.random.default_rng(77)  # packet_stream draws its payloads from this generator, in this order
    payloads = [rng.integers(0, 256, 1500, dtype=np.uint8).tobytes() for _ in range(n_pkt)]
    batch = n // 8
    rx = pkg.NativePacketReceiver(max_items=batch, tags_cap=2048, decode_headers=True, pipelined=True)
    # a streaming caller presents the unconsumed tail again: whole strides are consumed (hpp:238)
    chunks, pos = [], 0
    while pos + 2048 <= n and len(chunks) < 8:
        take = min(batch, n - pos)
        chunks.append(x[pos:pos + take])
        pos += ((take - 2048) // 1752 + 1) * 1752
    results, announced = [], 0
    for k, c in enumerate(chunks):
        while announced < min(k + 2, len(chunks) - 1):
            announced += 1
            rx.announce(chunks[announced])
        r = rx.process_bulk(c)
        if r is not None:
            results.append(r)
    results += rx.flush()
    assert len(results) == 8 and sum(r["consumed"] for r in results) == pos > n - batch // 64
    assert sum(r["header_mismatches"] for r in results) == 0
    got = []
    for r in results:
        data, pos = r["packets"].cpu().numpy(), 0
        for ln in r["packet_lengths"]:
            if ln > 0:
                got.append(data[pos:pos + int(ln)].tobytes())
                pos += int(ln)
    per_packet = (64 + 128 + 1504 * 4 + 9 + 11 + 500) * 4
    complete = pos // per_packet - 1  # packets that certainly end inside the consumed samples
    assert len(got) >= complete and got == payloads[: len(got)]


def _same_tag_records(a, b):
    return a.size == b.size and all(np.array_equal(a[k], b[k]) for k in a.dtype.names)


@pytest.mark.timeout(900)
def test_headline_configuration_at_its_size_pipelined_equals_sequential_and_oracle_prefix(pkg):
    """The configuration BENCH's `value` is measured on, as a whole and at its size (bench.py main(): configs[1] at
    SURVEY 8(d) config 2's size): three 2^28-sample calls of NativePacketReceiver(pipelined, output_ring) on the bench's
    own burst ring (headline_ring: two windows presented alternately, each with its history in front), announced two
    calls ahead.  That is the path with the dynamic block hand-out beside the 32-VGPR PLL (k_costas_cap: calls of
    >= 2^25 symbols while a later batch is in flight, costas_loop.hip) and the switch to the fast PLL form on the
    last batch.  Checked against
      (1) the one-stream sequential receiver (pipelined = False: no look-ahead, every stage in the caller's thread, the
          112-VGPR PLL throughout): consumed, detector tags, gate decisions, re-timed tags and all 3 x 2^26 symbols bit
          for bit (syncword_detection.hpp:204-356, costas_loop.hpp:92-148 at the size the number is quoted on);
      (2) the CPU oracle on the first 2^22 samples: detector tags (indices exact, floats in bands) and, fed with the
          GPU's accepted tags, CFC -> SymbolFilter -> wipe-off -> Costas bit for bit;
      (3) the generator: one accepted tag per packet period."""
    import bench
    n, device = 1 << 28, torch.device("cuda")
    rrc = bench.unit_norm_rrc(pkg)
    x, n_pkt = bench.burst_stream(pkg, n, rrc, seed=1, device=device)
    xb, n_pkt_b = bench.burst_stream(pkg, n, rrc, seed=1001, device=device)
    ring, windows = bench.headline_ring(x, xb)
    del x, xb
    cap = max(64, 2 * max(n_pkt, n_pkt_b) + 64)
    calls = 3

    def run(pipelined):
        rx = pkg.NativePacketReceiver(bench.SPS, bench.BINS, 9.5, "QPSK", max_items=n, tags_cap=cap, pipelined=pipelined,
                                      output_ring=True)
        results, announced = [], 0
        for k in range(calls):
            w, history = windows[k % 2]
            if pipelined:  # bench.py's step(): the inputs of the next calls announced, at most two ahead
                while announced < min(k + 2, calls - 1):
                    announced += 1
                    rx.announce(windows[announced % 2][0])
            r = rx.process_bulk(w, 1500, tags_cap=cap, history=history)
            if r is not None:
                results.append(r)
        results += rx.flush()
        return results

    piped = run(True)
    assert len(piped) == calls
    kept = [dict(r, symbols=r["symbols"].clone()) for r in piped]  # (the output ring is reused by the next receiver's)
    del piped
    torch.cuda.synchronize()
    seq = run(False)
    stride_items = ((n - 2048) // 1752 + 1) * 1752
    for k, (a, b) in enumerate(zip(kept, seq)):
        assert a["consumed"] == b["consumed"] == stride_items
        assert _same_tag_records(a["detector_tags"], b["detector_tags"]), k
        assert np.array_equal(a["accepted"], b["accepted"])
        assert _same_tag_records(a["tags"], b["tags"]), k
        assert a["symbols"].numel() == b["symbols"].numel() > (n // 4) - 2048
        assert torch.equal(a["symbols"].view(torch.float32).view(torch.int64), b["symbols"].view(torch.float32).view(torch.int64)), k
        # (3) the generator's packets: one accepted tag per period, at the period's spacing
        bench.check_tag_count(f"call {k}", int(a["tags"].size), 1, n)
        det = a["detector_tags"][a["accepted"]]["index"].astype(np.int64)
        assert np.all(np.abs(np.diff(det) - bench.BURST_PERIOD) <= 2)
    # calls 0 and 2 present the same window: identical detections apart from the state carried in from the call before
    assert abs(int(kept[0]["tags"].size) - int(kept[2]["tags"].size)) <= 1
    # (2) the oracle on the first 2^22 samples of call 0
    m = (1 << 22) + 2048
    first = kept[0]
    xh = host(windows[0][0][:m])
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5)
    _, ref_out, ref_tags = ref.process(xh, tags_cap=1 << 12)
    done = ref_out.size
    det = first["detector_tags"]
    inside = det["index"] < done - 2 * 768 - 1  # (the scan decides a detection up to time_threshold items later)
    ref_inside = ref_tags["index"] < done - 2 * 768 - 1
    assert_tags_match(det[inside], ref_tags[ref_inside], rtol=2e-4)
    # the delayed stream the chain reads in place: the ring's history, then the window (the detector's own pass-through
    # starts with 2T+1 zeros, syncword_detection.hpp:318-319; a streaming caller's ring holds the items before instead)
    delayed = np.concatenate([host(windows[0][1]), xh])[:done]
    acc = det[inside & first["accepted"]]
    z = orc.coarse_frequency_correction(delayed, acc["index"], acc["freq"], delay=26)
    pfb = orc.rrc_taps(32.0 / float(orc.unit_norm_rrc(4)[1]), 128.0, 1.0, 0.35, 32 * 4 * 11)[:-1]
    sym, sym_tags, _ = orc.symbol_filter(z, pfb, 32, 4, 44, tags=acc.astype(orc.TAG_DTYPE))
    w = orc.syncword_wipeoff(sym, np.where(sig.SYNCWORD == 1, -1.0, 1.0).astype(np.float32), sym_tags["index"])
    c = orc.costas_loop(w, "QPSK", 0.01, sym_tags["index"], sym_tags["phase"])
    k_sym = c.size - 1024  # (symbols behind the last tag the oracle saw may belong to a detection it has not made yet)
    got = host(first["symbols"][:k_sym])
    gt = first["tags"][first["tags"]["index"] < k_sym]
    st = sym_tags[sym_tags["index"] < k_sym]
    assert np.array_equal(gt["index"], st["index"]) and gt.size >= 150
    assert np.array_equal(bits(got), bits(c[:k_sym]))


@pytest.mark.timeout(900)
def test_config5_streamed_ring_at_its_size(pkg):
    """BENCH's `config5` sub-record at its size (BASELINE configs[4] as SURVEY 8(d) config 5 defines it): 2^30 samples
    of the bench's configs[4] stream (fft_size 4096, 1025-tap RRC: syncword 1277 samples, stride 2820) through a device
    ring in windows of 2^28 offered items with the look-ahead (next_x: k_correlate_4096 of the next window behind the
    current call's scan), B = 1 and B = 9 with the bench's thresholds.  The streamed calls give the tags of plain,
    non-announced calls record for record; every burst the generator placed is found; and the first window's first
    2^21 samples agree with the CPU oracle at fft_size 4096 (indices, freq_bin exact; floats in bands)."""
    import bench
    device = torch.device("cuda")
    total, window, nfft = 1 << 30, 1 << 28, 4096
    x, rrc, fir = bench.config5_stream(pkg, total, device)
    del fir
    L = 63 * 4 + rrc.size
    S = nfft - L + 1
    assert (L, S) == (1277, 2820)
    wins = bench.config5_windows(total, window, nfft, S)
    assert len(wins) == 5
    bursts = 1537 + 4 * np.arange(2000, total // 4 - 64, 16384)  # config5_stream: a syncword every 16384 symbols
    for b, thr in ((0, 60.0), (4, 30.0)):
        def run(lookahead):
            sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -b, b, fft_size=nfft, power_threshold=thr, max_items=window)
            out, done = [], 0
            for k, (pos, take) in enumerate(wins):
                nxt = x[wins[k + 1][0]:wins[k + 1][0] + wins[k + 1][1]] if (lookahead and k + 1 < len(wins)) else None
                _, _, t, nd = sd.process_bulk(x[pos:pos + take], want_output=False, tags_cap=1 << 17, next_x=nxt)
                assert nd == ((take - nfft) // S + 1) * S and pos == done
                t = t.copy()
                t["index"] += pos
                out.append(t)
                done += nd
            return np.concatenate(out), done
        streamed, done = run(True)
        plain, done2 = run(False)
        assert done == done2 > total - window // 64
        assert _same_tag_records(streamed, plain), (b, streamed.size, plain.size)
        found = np.isin(bursts[bursts < done - 1537], streamed["index"])
        assert found.all(), (b, int((~found).sum()))
        extra = streamed.size - int(found.sum())
        assert extra <= 0.02 * found.sum(), (b, extra)  # (detections on plain data: a 1025-tap template, see bench.py)
        # the oracle on the first 2^21 samples
        m = (1 << 21) + nfft
        ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -b, b, fft_size=nfft, power_threshold=thr)
        _, ref_out, ref_tags = ref.process(host(x[:m]), tags_cap=1 << 12)
        lim = ref_out.size - 2 * 768 - 1
        assert_tags_match(streamed[streamed["index"] < lim], ref_tags[ref_tags["index"] < lim], rtol=3e-4)
        assert int((ref_tags["index"] < lim).sum()) >= 30


def test_config3_channel_bank_every_packet_is_found(pkg):
    """the channels bench.py builds for configs[2] / [3] (channel c = its own burst stream, seed
    c, carrier offset -0.04 + 0.08 c / (C - 1) rad/sample) lie inside the +-4-bin search range: the detector finds every
    packet of every channel, so no serial segment of the chain is longer than one packet period"""
    import bench
    C, n = 8, 1 << 20
    device = torch.device("cuda")
    rrc = bench.unit_norm_rrc(pkg)
    xs = bench.channel_bank_config3(pkg, n, rrc, C, device, seed0=3)
    period = (64 + 128 + 1504 * 4 + 500) * 4
    sd = pkg.SyncwordDetection(rrc, bench.SYNCWORD, np.array([1, -1], dtype=np.complex64), -4, 4, power_threshold=9.5,
                               n_channels=C, max_items=n)
    st, out, tags, nd = sd.process_bulk(xs, want_output=False, tags_cap=256)
    assert st == 0
    expected = (nd - 1537 - 300) // period  # whole packets inside the produced range
    for c in range(C):
        idx = np.sort(tags[c]["index"].astype(np.int64))
        assert idx.size >= expected, (c, idx.size, expected)
        assert np.all(np.diff(idx) < 1.5 * period), c   # no gap of two packets between detections


def test_multichannel_receiver_full_size_config2(pkg):
    """BASELINE configs[2] at its full size: 64 channels x 2^22 samples per batch (the bench's burst stream with the
    per-channel CFO sweep), three batches in flight with the streaming stride.  Size-independent properties: the
    pipelined receiver (one launch for all channels, input read in place) returns, bit for bit, what a second
    receiver returns that processes batch by batch with a delayed copy; channels 0, 21, 42 and 63 equal one
    single-channel PacketReceiver each; the centre channels find (almost) every packet"""
    import bench
    C, n = 64, 1 << 22
    device = torch.device("cuda")
    rrc = bench.unit_norm_rrc(pkg)
    x, n_pkt = bench.burst_stream(pkg, 3 * n, rrc, seed=5, device=device)
    xs = bench.channel_bank(x, C)
    stride = ((n - 2048) // 1752 + 1) * 1752  # a streaming caller presents the unconsumed tail again (hpp:238)
    parts = [xs[:, b * stride:b * stride + n] for b in range(3) if b * stride + n <= xs.shape[1]]
    assert len(parts) == 3
    cap = 2 * (n_pkt // 3) + 64
    pipe = pkg.NativeMultiChannelReceiver(C, max_items=n, tags_cap=cap, workers=8)
    pipe.set_input_in_place(True)
    sync = pkg.NativeMultiChannelReceiver(C, max_items=n, tags_cap=cap, workers=8)
    for w in parts:
        assert pipe.submit(w, 1500) == stride
    got = [pipe.collect() for _ in parts]
    want = [sync.process_bulk(w, 1500) for w in parts]
    singles = {c: pkg.PacketReceiver(max_items=n) for c in (0, 21, 42, 63)}
    found = np.zeros(C, dtype=np.int64)
    for b in range(3):
        for c in range(C):
            g, w_ = got[b][c], want[b][c]
            assert g["consumed"] == w_["consumed"] == stride
            assert torch.equal(g["symbols"].view(torch.int64), w_["symbols"].view(torch.int64)), (b, c)
            assert same_tags(g["tags"], w_["tags"]) and same_tags(g["detector_tags"], w_["detector_tags"])
            found[c] += g["detector_tags"].size
        for c, rx in singles.items():
            ref = rx.process_bulk(parts[b][c], 1500, tags_cap=cap)
            assert torch.equal(got[b][c]["symbols"].view(torch.int64), ref["symbols"].view(torch.int64)), (b, c)
            assert same_tags(got[b][c]["tags"], ref["tags"])
    expect = 3 * stride // ((64 + 128 + 1504 * 4 + 500) * 4)
    assert found[24:40].min() >= expect - 2 and found.max() <= expect + 4  # the edge channels miss up to a fifth


def test_c_abi_from_cpp(pkg, tmp_path):
    """the boundary is usable from plain C++ (what a gr::Block wrapper does): build
    tests/cabi_smoke.cpp against include/gr4pm_hip.h + libgr4pm_hip.so and run it"""
    import os
    import subprocess
    exe = tmp_path / "cabi_smoke"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wno-unused-result",
                           "-I", os.path.join(ge.ROOT, "include"), "-o", str(exe),
                           os.path.join(ge.ROOT, "tests", "cabi_smoke.cpp"),
                           "-L" + os.path.dirname(pkg.LIB_PATH), "-lgr4pm_hip",
                           "-Wl,-rpath," + os.path.dirname(pkg.LIB_PATH)])
    out = subprocess.check_output([str(exe)]).decode()
    assert out.startswith("OK"), out


@pytest.mark.parametrize("fft_size,ntaps_req", [(4096, 1024), (1024, 44), (512, 44)])
def test_syncword_detection_other_fft_sizes(pkg, fft_size, ntaps_req):
    """fft_size is a free setting in the reference (hpp:133); BASELINE config 5 shape: N = 4096 with
    a 1024-tap RRC (1025 taps -> L = 63*4 + 1025 = 1277, stride 2820).  Generic-size kernels."""
    sps = 4
    rrc = orc.rrc_taps(1.0, float(sps), 1.0, 0.35, ntaps_req)
    rrc = (rrc / np.sqrt(np.sum(rrc.astype(np.float64) ** 2))).astype(np.float32)
    rng = np.random.default_rng(fft_size)
    nsym = 40000
    symbols = rng.integers(0, 2, nsym).astype(np.uint8)
    locs = [300, 5000, 12000, 25000, 33000]
    for loc in locs:
        symbols[loc:loc + 64] = sig.SYNCWORD
    x = orc.interpolating_fir(sig.BPSK[symbols], sps, rrc)
    x = (orc.rotator(x, np.float32(0.004)) + sig.awgn(x.size, 0.05, 7)).astype(np.complex64)
    L = 63 * sps + rrc.size
    if L > fft_size:
        pytest.skip("syncword longer than the block")
    kw = dict(fft_size=fft_size, power_threshold=15.0)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -2, 2, **kw)
    st0, ref_out, ref_tags, ref_zpow, _ = ref.process(x, debug=True)
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -2, 2, max_items=x.size, **kw)
    assert sd._syncword_samples_size == L
    st, out, tags, n = sd.process_bulk(dev(x))
    assert st == st0 == 0 and n == ref_out.size
    assert np.array_equal(bits(host(out)), bits(ref_out))
    assert ref_tags.size >= 4
    assert_tags_match(tags, ref_tags, rtol=3e-4)
    zpow = host(sd.last_zpow(n))[0]
    assert np.max(np.abs(zpow - ref_zpow)) / np.max(ref_zpow) < 5e-6
    # streaming in two calls gives the same tags
    sd2 = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -2, 2, max_items=x.size, **kw)
    cut = x.size // 2
    _, _, t1, d1 = sd2.process_bulk(dev(x[:cut]), want_output=False)
    _, _, t2, d2 = sd2.process_bulk(dev(x[d1:]), want_output=False)
    t2 = t2.copy()
    t2["index"] += d1
    assert d1 + d2 == n and np.array_equal(np.concatenate([t1, t2])["index"], tags["index"])


@pytest.mark.parametrize("bins,offsets", [(4, (-3.6, -1.2, 0.3, 2.1, 3.9)), (0, (-0.3, -0.1, 0.0, 0.2, 0.3))])
def test_syncword_detection_config4_nine_bins_vs_oracle(pkg, bins, offsets):
    """BASELINE configs[4] as bench.py runs it (`config5` sub-record: SURVEY.md 8(d) config 5, B in {1, 9}): fft_size
    4096, 1025-tap RRC (L = 1277, stride 2820), NINE frequency bins and ONE, power_threshold 30 -- k_correlate_4096 and
    the detector against the oracle: correlation powers within 5e-6 of full scale, tag indices and freq_bin exact, tag
    floats within tolerance; one call and two"""
    sps = 4
    rrc = orc.rrc_taps(1.0, float(sps), 1.0, 0.35, 1024)
    rrc = (rrc / np.sqrt(np.sum(rrc.astype(np.float64) ** 2))).astype(np.float32)
    assert rrc.size == 1025
    rng = np.random.default_rng(4096)
    nsym = 60000
    symbols = rng.integers(0, 2, nsym).astype(np.uint8)
    locs = [700, 9000, 21000, 40000, 52000]
    for loc in locs:
        symbols[loc:loc + 64] = sig.SYNCWORD
    x = orc.interpolating_fir(sig.BPSK[symbols], sps, rrc)
    # carrier offsets that put detections in different bins (bin spacing pi / L rad/sample, hpp:166-182)
    L = 63 * sps + rrc.size
    seg = x.size // 5
    for k, b in enumerate(offsets):
        x[k * seg:(k + 1) * seg] = orc.rotator(x[k * seg:(k + 1) * seg], np.float32(b * np.pi / L))
    x = (x + sig.awgn(x.size, 0.05, 9)).astype(np.complex64)
    kw = dict(fft_size=4096, power_threshold=30.0)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -bins, bins, **kw)
    st0, ref_out, ref_tags, ref_zpow, _ = ref.process(x, debug=True)
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -bins, bins, max_items=x.size, **kw)
    st, out, tags, n = sd.process_bulk(dev(x))
    assert st == st0 == 0 and n == ref_out.size
    assert np.array_equal(bits(host(out)), bits(ref_out))
    assert set(1537 + 4 * np.array(locs)) <= set(ref_tags["index"].tolist())
    assert len(set(ref_tags["freq_bin"].tolist())) >= (4 if bins else 1)
    assert_tags_match(tags, ref_tags, rtol=3e-4)
    zpow = host(sd.last_zpow(n))[0]
    assert np.max(np.abs(zpow - ref_zpow)) / np.max(ref_zpow) < 5e-6
    sd2 = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -bins, bins, max_items=x.size, **kw)
    cut = 4096 + 17 * 2820
    _, _, t1, d1 = sd2.process_bulk(dev(x[:cut]), want_output=False)
    _, _, t2, d2 = sd2.process_bulk(dev(x[d1:]), want_output=False)
    t2 = t2.copy()
    t2["index"] += d1
    assert d1 + d2 == n
    assert_tags_match(np.concatenate([t1, t2]), ref_tags, rtol=3e-4)


def test_fft4096_workgroup_correlator_against_the_radix2_kernel(pkg, monkeypatch):
    """fft_size 4096 runs k_correlate_4096 (16 x 16 x 16, three in-register passes); GR4PM_CORRELATOR=radix2 keeps
    the generic radix-2 kernel for it: same powers within float rounding, identical tags"""
    sps = 4
    rrc = orc.rrc_taps(1.0, float(sps), 1.0, 0.35, 1024)
    rrc = (rrc / np.sqrt(np.sum(rrc.astype(np.float64) ** 2))).astype(np.float32)
    rng = np.random.default_rng(4)
    symbols = rng.integers(0, 2, 60000).astype(np.uint8)
    for loc in (700, 9000, 21000, 40000, 52000):
        symbols[loc:loc + 64] = sig.SYNCWORD
    x = orc.interpolating_fir(sig.BPSK[symbols], sps, rrc)
    x = (orc.rotator(x, np.float32(-0.003)) + sig.awgn(x.size, 0.05, 8)).astype(np.complex64)
    res = {}
    for kind in ("w64", "radix2"):
        monkeypatch.setenv("GR4PM_CORRELATOR", kind)
        sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, fft_size=4096, power_threshold=30.0, max_items=x.size)
        st, out, tags, n = sd.process_bulk(dev(x))
        res[kind] = (tags, host(sd.last_zpow(n))[0])
    (ta, za), (tb, zb) = res["w64"], res["radix2"]
    assert np.array_equal(ta["index"], tb["index"]) and np.array_equal(ta["freq_bin"], tb["freq_bin"])
    assert set(1537 + 4 * np.array([700, 9000, 21000, 40000, 52000])) <= set(ta["index"].tolist())  # (+ a start-up transient)
    assert np.max(np.abs(za - zb)) / np.max(zb) < 2e-6


def test_syncword_detection_unsupported_fft_size_is_reported(pkg):
    rrc, _ = orc.unit_norm_rrc(4)
    with pytest.raises(pkg.Gr4pmError, match="not built"):
        pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, 0, 0, fft_size=3000)


def test_syncword_detection_64_channels_cfo_sweep(pkg):
    """BASELINE config 3 shape at test size: 64 channels in one handle, per-channel CFO sweep
    -0.04 .. +0.04 rad/sample; every channel must equal the oracle run on that channel alone"""
    C, nsym, sps = 64, 6000, 4
    rrc, _ = orc.unit_norm_rrc(sps)
    rng = np.random.default_rng(64)
    X, refs = [], []
    for c in range(C):
        symbols = rng.integers(0, 2, nsym).astype(np.uint8)
        locs = [200 + 13 * c, 2500 + 7 * c, 4800]
        for loc in locs:
            symbols[loc:loc + 64] = sig.SYNCWORD
        f = -0.04 + 0.08 * c / (C - 1)
        x = orc.rotator(orc.interpolating_fir(sig.BPSK[symbols], sps, rrc), np.float32(f))
        x = (x + sig.awgn(x.size, 0.05, 1000 + c)).astype(np.complex64)
        X.append(x)
        ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5)
        refs.append(ref.process(x))
    X = np.stack(X)
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -4, 4, power_threshold=9.5, n_channels=C,
                               max_items=X.shape[1])
    st, out, tags, n = sd.process_bulk(dev(X))
    out = host(out)
    for c in range(C):
        _, ref_out, ref_tags = refs[c]
        assert n == ref_out.size and np.array_equal(bits(out[c]), bits(ref_out)), c
        assert ref_tags.size >= 3  # the three inserted syncwords (+ whatever the oracle also finds)
        assert_tags_match(tags[c], ref_tags, rtol=3e-4)


# ------------------------------------------------------------------ settings matrix
@pytest.mark.parametrize("sps,ntaps_req,tthr,bins,thr", [
    (4, 44, 100, (-2, 5), 12.0),     # short window (T not a multiple of 64), asymmetric bins
    (4, 44, 1000, (0, 0), 9.5),      # one bin, long window with a partial last block
    (3, 33, 768, (-4, 4), 15.0),     # L = 63*3+33 = 222 -> stride 1827 (odd): 8-byte-aligned loads path
    (2, 22, 500, (-1, 1), 15.0),     # sps 2, L = 149
    (8, 88, 768, (-3, 3), 15.0),     # sps 8, L = 593
])
def test_syncword_detection_settings_matrix(pkg, sps, ntaps_req, tthr, bins, thr):
    rrc = orc.rrc_taps(1.0, float(sps), 1.0, 0.35, ntaps_req)
    rrc = (rrc / np.sqrt(np.sum(rrc.astype(np.float64) ** 2))).astype(np.float32)
    rng = np.random.default_rng(sps * 1000 + tthr)
    nsym = 120000 // sps
    symbols = rng.integers(0, 2, nsym).astype(np.uint8)
    locs = [nsym // 10, nsym // 3, nsym // 2 + 17, (4 * nsym) // 5]
    for loc in locs:
        symbols[loc:loc + 64] = sig.SYNCWORD
    L = 63 * sps + rrc.size
    f = 0.5 * (bins[0] + bins[1]) * np.pi / L + 0.002
    x = orc.rotator(orc.interpolating_fir(sig.BPSK[symbols], sps, rrc), np.float32(f))
    x = (x + sig.awgn(x.size, 0.1, tthr)).astype(np.complex64)
    kw = dict(samples_per_symbol=sps, time_threshold=tthr, power_threshold=thr)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, bins[0], bins[1], **kw)
    _, ref_out, ref_tags, ref_zpow, _ = ref.process(x, debug=True)
    sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, bins[0], bins[1], max_items=x.size, **kw)
    st, out, tags, n = sd.process_bulk(dev(x))
    assert n == ref_out.size and np.array_equal(bits(host(out)), bits(ref_out))
    assert ref_tags.size >= 3
    assert_tags_match(tags, ref_tags, rtol=3e-4)
    assert np.max(np.abs(host(sd.last_zpow(n))[0] - ref_zpow)) / np.max(ref_zpow) < 5e-6
    # chunked
    sd2 = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, bins[0], bins[1], max_items=x.size, **kw)
    pos, got = 0, []
    for size in (2048, 5000, 2048 + 3 * (2048 - L + 1), 40000, x.size):
        if pos + 2048 > x.size:
            break
        _, _, t, d = sd2.process_bulk(dev(x[pos:pos + size]), want_output=False)
        t = t.copy()
        t["index"] += pos
        got.append(t)
        pos += d
    got = np.concatenate(got)
    assert np.array_equal(got["index"], tags["index"][: got.size]) and got.size >= tags.size - 1


def test_syncword_detection_history_longer_than_stride_small_calls(pkg):
    """hist = 2T + 1 = 2001 > S = 1752 (T = 1000): a detection that leaves in a call can lie two or more blocks
    before the call's first item, and with 2048-item calls (one block each) more than one CALL back -- its block's
    noise power is then not among the values k_correlate_w64 left behind.  Every float of every tag against the
    oracle (syncword_detection.hpp:56-115,257-265), not only the indices."""
    rrc = orc.rrc_taps(1.0, 4.0, 1.0, 0.35, 44)
    rrc = (rrc / np.sqrt(np.sum(rrc.astype(np.float64) ** 2))).astype(np.float32)
    rng = np.random.default_rng(1000)
    nsym = 30000
    symbols = rng.integers(0, 2, nsym).astype(np.uint8)
    locs = [1200, 4050, 9031, 15002, 20990, 26011]
    for loc in locs:
        symbols[loc:loc + 64] = sig.SYNCWORD
    x = orc.rotator(orc.interpolating_fir(sig.BPSK[symbols], 4, rrc), np.float32(0.003))
    # noise level that changes from packet to packet: a neighbouring block's noise power is visibly wrong
    sigma = np.repeat(rng.uniform(0.02, 0.3, x.size // 5000 + 1), 5000)[: x.size].astype(np.float32)
    x = (x + sigma * sig.awgn(x.size, 1.0, 7)).astype(np.complex64)
    kw = dict(time_threshold=1000, power_threshold=9.5)
    ref = orc.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -2, 2, **kw)
    _, _, ref_tags = ref.process(x)
    assert ref_tags.size >= 5
    for sizes in ([2048], [2048, 2048 + 1752, 2048, 2048 + 2 * 1752, 6000]):
        sd = pkg.SyncwordDetection(rrc, sig.SYNCWORD, sig.BPSK, -2, 2, max_items=1 << 14, **kw)
        xd = dev(x)
        pos, got, i = 0, [], 0
        while pos + 2048 <= x.size:
            size = sizes[i % len(sizes)]
            i += 1
            st, _, t, d = sd.process_bulk(xd[pos:pos + size].contiguous(), want_output=False)
            assert st == 0 and d > 0
            t = t.copy()
            t["index"] += pos
            got.append(t)
            pos += d
        got = np.concatenate(got)
        assert got.size >= ref_tags.size - 1
        assert_tags_match(got, ref_tags[: got.size], rtol=3e-4)


def test_rotator_and_costas_multichannel(pkg):
    """batched handles: independent state per channel (== each channel alone)"""
    rng = np.random.default_rng(3)
    C, n = 5, 30000
    x = (rng.standard_normal((C, n)) + 1j * rng.standard_normal((C, n))).astype(np.complex64)
    cfc = pkg.CoarseFrequencyCorrection(26, n_channels=C)
    tags = np.zeros(7, dtype=pkg.TAG_DTYPE)
    tags["index"] = [10, 5000, 100, 9000, 20000, 0, 29990]
    tags["freq"] = [0.01, -0.02, 0.03, 0.0, 0.015, -0.007, 0.02]
    tags["phase"] = [0.1, -0.2, 0.3, 1.0, -1.5, 2.0, -3.0]
    tags["flags"] = pkg.TAG_SYNCWORD
    chan = np.array([0, 0, 1, 2, 2, 4, 4], dtype=np.uint32)
    order = np.lexsort((tags["index"], chan))
    y = host(cfc.process_bulk(dev(x), tags[order], chan[order]))
    cl = pkg.CostasLoop(0.01, "QPSK", n_channels=C)
    z = host(cl.process_bulk(dev(x), tags[order], chan[order]))
    for c in range(C):
        sel = chan == c
        idx = np.sort(tags["index"][sel])
        o = np.argsort(tags["index"][sel])
        want = orc.coarse_frequency_correction(x[c], idx, tags["freq"][sel][o], delay=26)
        assert np.array_equal(bits(y[c]), bits(want)), c
        wantz = orc.costas_loop(x[c], "QPSK", 0.01, idx, tags["phase"][sel][o])
        assert np.array_equal(bits(z[c]), bits(wantz)), c


def test_stream_blocks_empty_and_tiny_inputs(pkg):
    """empty / one-item calls and calls without tags are legal and keep the state"""
    e = torch.zeros(0, dtype=torch.complex64, device="cuda")
    one = dev(np.array([1 + 2j], dtype=np.complex64))
    r = pkg.Rotator(0.5)
    assert r.process_bulk(e).numel() == 0
    a = host(r.process_bulk(one))
    b = host(r.process_bulk(one))
    want = orc.rotator(np.array([1 + 2j, 1 + 2j], np.complex64), np.float32(0.5))
    assert np.array_equal(bits(np.concatenate([a, b])), bits(want))
    assert pkg.CostasLoop().process_bulk(e).numel() == 0
    assert pkg.SyncwordWipeoff(np.ones(4, np.float32)).process_bulk(e).numel() == 0
    assert pkg.InterpolatingFirFilter(4, np.ones(5, np.float32)).process_bulk(e).numel() == 0
    rrc, pfb = _receiver_pfb()
    y, t, c = pkg.SymbolFilter(pfb, 32, 4, 44).process_bulk(e)
    assert y.numel() == 0 and c == 0
    y, c = pkg.PfbArbResampler(1.1).process_bulk(e)
    assert y.numel() == 0 and c == 0


def test_fused_cfc_symbol_filter_equals_separate_blocks(pkg):
    """gr4pm_cfc_symbol_filter_process == CoarseFrequencyCorrection then SymbolFilter, bit for bit,
    including the carried state over several calls (tags near call boundaries, pending delays)"""
    rrc, pfb = _receiver_pfb()
    rng = np.random.default_rng(77)
    n = 40000
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    idx = np.array([3, 5000, 9990, 10010, 17000, 17003, 25000, 39990], dtype=np.uint64)
    tags = np.zeros(idx.size, dtype=pkg.TAG_DTYPE)
    tags["index"] = idx
    tags["amplitude"] = rng.uniform(0.5, 2.0, idx.size)
    tags["time_est"] = rng.uniform(-0.5, 0.5, idx.size)
    tags["phase"] = rng.uniform(-3, 3, idx.size)
    tags["freq"] = rng.uniform(-0.03, 0.03, idx.size)
    tags["flags"] = pkg.TAG_SYNCWORD
    cuts = [0, 10000, 10001, 26000, n]
    a_cfc, a_sf = pkg.CoarseFrequencyCorrection(26), pkg.SymbolFilter(pfb, 32, 4, 44)
    b_cfc, b_sf = pkg.CoarseFrequencyCorrection(26), pkg.SymbolFilter(pfb, 32, 4, 44)
    ya, ta, yb, tb = [], [], [], []
    oa = ob = 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        t = tags[(tags["index"] >= lo) & (tags["index"] < hi)].copy()
        t["index"] -= lo
        xd = dev(x[lo:hi])
        y, tt, c = a_sf.process_bulk(a_cfc.process_bulk(xd, t), t)
        assert c == hi - lo
        tt = tt.copy(); tt["index"] += oa; oa += y.numel()
        ya.append(host(y)); ta.append(tt)
        y, tt, c = pkg.cfc_symbol_filter(b_cfc, b_sf, xd, t)
        assert c == hi - lo
        tt = tt.copy(); tt["index"] += ob; ob += y.numel()
        yb.append(host(y)); tb.append(tt)
    ya, yb, ta, tb = np.concatenate(ya), np.concatenate(yb), np.concatenate(ta), np.concatenate(tb)
    assert np.array_equal(bits(ya), bits(yb))
    assert np.array_equal(ta, tb)
    # and against the oracle
    z = orc.coarse_frequency_correction(x, tags["index"], tags["freq"], delay=26)
    want, want_tags, _ = orc.symbol_filter(z, pfb, 32, 4, 44, tags=tags.astype(orc.TAG_DTYPE))
    assert np.array_equal(bits(yb), bits(want)) and np.array_equal(tb["index"], want_tags["index"])


def test_cfc_fixed_point_before_the_first_tag_and_at_zero_frequency(pkg):
    """coarse_frequency_correction.hpp:44-45,50-59,84-86: from start() to the first syncword_freq tag -- and after every
    tag whose frequency is exactly 0 -- the phasor is (1, -+0) with increment (1, -+0): a fixed point of the recurrence.
    Those segments get no serial chain (RotSeg mode 2: constant checkpoints by a parallel fill; on the stream the
    reference publishes its receiver benchmark on, zeros without a tag, that is everything), and the consumers still
    MULTIPLY by the constant, so the bits are the reference's: x * (1, -0) turns -0 into +0 in places and the test
    stream is full of signed zeros.  Against the oracle: a stream whose first tag comes after 2^24 samples, then tags
    with frequencies != 0, == +0 and == -0 at ragged distances, in one call and in calls cut inside fixed and chained
    stretches; CoarseFrequencyCorrection alone (delay 0 and 26), the fused CFC + SymbolFilter call of the receiver,
    and Rotator(0)."""
    rrc, pfb = _receiver_pfb()
    rng = np.random.default_rng(2024)
    n = (1 << 24) + (1 << 18)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    z = rng.integers(0, 16, n)
    x.real[z == 0] = 0.0
    x.real[z == 1] = -0.0
    x.imag[z == 2] = 0.0
    x.imag[z == 3] = -0.0
    x[z == 4] = np.complex64(complex(-0.0, -0.0))
    first = (1 << 24) + 777
    idx = np.array([first, first + 9000, first + 9030, first + 40000, first + 90000, first + 90003, first + 150000,
                    first + 200000], dtype=np.uint64)
    fr = np.array([0.011, 0.0, -0.02, -0.0, 0.0, 0.03, 0.0, -0.0])
    tags = np.zeros(idx.size, dtype=pkg.TAG_DTYPE)
    tags["index"], tags["freq"], tags["flags"] = idx, fr, pkg.TAG_SYNCWORD
    tags["amplitude"], tags["time_est"] = 1.0, rng.uniform(-0.5, 0.5, idx.size)
    xd = dev(x)
    cuts = [0, 1 << 23, first - 5, first + 9010, first + 100000, n]
    for delay in (0, 26):
        want = orc.coarse_frequency_correction(x, idx, fr, delay=delay)
        assert not np.array_equal(bits(want[: 1 << 20]), bits(x[: 1 << 20]))  # (not a copy: the signed zeros)
        assert np.array_equal(want[: 1 << 20], x[: 1 << 20])                  # (... but the same values)
        y = host(pkg.CoarseFrequencyCorrection(delay).process_bulk(xd, tags))
        assert np.array_equal(bits(y), bits(want)), delay
        cfc, outs = pkg.CoarseFrequencyCorrection(delay), []
        for a, b in zip(cuts[:-1], cuts[1:]):
            t = tags[(tags["index"] >= a) & (tags["index"] < b)].copy()
            t["index"] -= a
            outs.append(host(cfc.process_bulk(xd[a:b], t)))
        assert np.array_equal(bits(np.concatenate(outs)), bits(want)), delay
    # the receiver's fused call (CFC delay 26 -> 32-arm SymbolFilter)
    want, want_tags, _ = orc.symbol_filter(orc.coarse_frequency_correction(x, idx, fr, delay=26), pfb, 32, 4, 44,
                                           tags=tags.astype(orc.TAG_DTYPE))
    cfc, sf, ys, ts, off = pkg.CoarseFrequencyCorrection(26), pkg.SymbolFilter(pfb, 32, 4, 44), [], [], 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        t = tags[(tags["index"] >= a) & (tags["index"] < b)].copy()
        t["index"] -= a
        y, tt, c = pkg.cfc_symbol_filter(cfc, sf, xd[a:b], t)
        assert c == b - a
        tt = tt.copy()
        tt["index"] += off
        off += y.numel()
        ys.append(host(y))
        ts.append(tt)
    assert np.array_equal(bits(np.concatenate(ys)), bits(want))
    assert np.array_equal(np.concatenate(ts)["index"], want_tags["index"])
    # Rotator with phase_incr 0 (rotator.hpp:44-65): exp stays (1, +0)
    m = 1 << 20
    r = pkg.Rotator(0.0)
    got = np.concatenate([host(r.process_bulk(xd[:m // 3])), host(r.process_bulk(xd[m // 3:m]))])
    assert np.array_equal(bits(got), bits(orc.rotator(x[:m], np.float32(0.0))))


def test_cfc_symbol_filter_plan_then_run_equals_fused_call(pkg):
    """gr4pm_cfc_symbol_filter_plan + _run (the two pipeline stages of the native receiver) ==
    gr4pm_cfc_symbol_filter_process, bit for bit, also when the plan of the next call is made
    before the run of the current one (two plans exist)"""
    rrc, pfb = _receiver_pfb()
    rng = np.random.default_rng(78)
    n = 48000
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    idx = np.array([3, 5000, 9990, 10010, 17000, 17003, 25000, 39990, 47990], dtype=np.uint64)
    tags = np.zeros(idx.size, dtype=pkg.TAG_DTYPE)
    tags["index"] = idx
    tags["amplitude"] = rng.uniform(0.5, 2.0, idx.size)
    tags["time_est"] = rng.uniform(-0.5, 0.5, idx.size)
    tags["phase"] = rng.uniform(-3, 3, idx.size)
    tags["freq"] = rng.uniform(-0.03, 0.03, idx.size)
    tags["flags"] = pkg.TAG_SYNCWORD
    cuts = [0, 10000, 10001, 26000, 40000, n]
    a_cfc, a_sf = pkg.CoarseFrequencyCorrection(26), pkg.SymbolFilter(pfb, 32, 4, 44)
    b_cfc, b_sf = pkg.CoarseFrequencyCorrection(26), pkg.SymbolFilter(pfb, 32, 4, 44)
    pieces = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        t = tags[(tags["index"] >= lo) & (tags["index"] < hi)].copy()
        t["index"] -= lo
        pieces.append((dev(x[lo:hi]), t))
    want = [pkg.cfc_symbol_filter(a_cfc, a_sf, xd, t) for xd, t in pieces]
    # software pipeline: plan(k + 1) is issued before run(k)
    got = []
    plan = pkg.cfc_symbol_filter_plan(b_cfc, pieces[0][0].numel(), pieces[0][1])
    for k, (xd, t) in enumerate(pieces):
        nxt = None
        if k + 1 < len(pieces):
            nxt = pkg.cfc_symbol_filter_plan(b_cfc, pieces[k + 1][0].numel(), pieces[k + 1][1])
        got.append(pkg.cfc_symbol_filter_run(b_cfc, plan, b_sf, xd, t))
        plan = nxt
    for (ya, ta, ca), (yb, tb, cb) in zip(want, got):
        assert ca == cb and np.array_equal(bits(host(ya)), bits(host(yb))) and np.array_equal(ta, tb)
    # a run without its plan is refused
    with pytest.raises(pkg.Gr4pmError):
        pkg.cfc_symbol_filter_run(b_cfc, 0, b_sf, dev(x[:1234]), None)


def test_syncword_wipeoff_in_place(pkg):
    """out == in: only the syncword items are touched, same result as the copying call"""
    rng = np.random.default_rng(5)
    n = 5000
    v = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    bipolar = np.where(sig.SYNCWORD == 1, -1.0, 1.0).astype(np.float32)
    tags = np.zeros(4, dtype=pkg.TAG_DTYPE)
    tags["index"], tags["flags"] = [10, 100, 2250, 4980], pkg.TAG_SYNCWORD  # the last one continues in the next call
    a, b = pkg.SyncwordWipeoff(bipolar), pkg.SyncwordWipeoff(bipolar)
    for piece, t in ((v[:n], tags), (v[:300], None)):
        ya = host(a.process_bulk(dev(piece), t))
        xb = dev(piece).clone()
        yb = b.process_bulk(xb, t, in_place=True)
        assert yb.data_ptr() == xb.data_ptr()
        assert np.array_equal(bits(ya), bits(host(yb)))


def test_multichannel_receiver_64_channels_pipelined_equals_synchronous(pkg, monkeypatch):
    """BASELINE configs[2] at its channel count: 64 channels with the per-channel CFO sweep of SURVEY 8(d) config 3
    (-0.04 .. +0.04 rad/sample), six batches.  submit() / collect() with up to four batches in flight (stages in
    their own threads, the symbol filters and wipe-offs of all channels in ONE launch each, the detector's delayed
    stream read in place) == process() batch by
    batch with one launch per channel (GR4PM_MC_PER_CHANNEL=1), bit for bit: symbols, re-timed tags, detector tags;
    and channel 0 / 31 / 63 against one single-channel PacketReceiver each"""
    C, n, n_batches = 64, 1 << 15, 6
    rng = np.random.default_rng(77)
    total = n * n_batches
    base, _ = sig.qa_syncword_stream(total // 4, sorted(rng.choice(np.arange(500, total // 4 - 2500, 1700), size=24, replace=False).tolist()), 0.0, seed=5)
    base = (0.7 * base[:total] + sig.awgn(total, 0.05, 6)).astype(np.complex64)
    k = np.arange(total, dtype=np.float64)
    xs = np.stack([np.roll(base, 997 * c) * np.exp(1j * ((-0.04 + 0.08 * c / (C - 1)) * k)) for c in range(C)]).astype(np.complex64)
    xd = dev(xs)
    parts = [xd[:, b * n:(b + 1) * n].contiguous() for b in range(n_batches)]
    monkeypatch.setenv("GR4PM_MC_PER_CHANNEL", "1")
    sync = pkg.NativeMultiChannelReceiver(C, max_items=n, tags_cap=128, workers=8)
    monkeypatch.delenv("GR4PM_MC_PER_CHANNEL")
    pipe = pkg.NativeMultiChannelReceiver(C, max_items=n, tags_cap=128, workers=8)
    pipe.set_input_in_place(True)  # `parts` stay alive: the delayed stream is read in place, no copy per batch
    want = [sync.process_bulk(w, 200) for w in parts]
    got = []
    for b, w in enumerate(parts):
        if pipe.in_flight() == 4:
            got.append(pipe.collect())
        pipe.submit(w, 200)
    while pipe.in_flight():
        got.append(pipe.collect())
    assert len(got) == n_batches
    n_tags = 0
    for b in range(n_batches):
        for c in range(C):
            g, w_ = got[b][c], want[b][c]
            assert g["consumed"] == w_["consumed"]
            assert np.array_equal(bits(host(g["symbols"])), bits(host(w_["symbols"]))), (b, c)
            assert same_tags(g["tags"], w_["tags"]) and same_tags(g["detector_tags"], w_["detector_tags"])
            n_tags += g["tags"].size
    assert n_tags > 15 * C  # most packets are found on most channels (the edge channels miss some)
    for c in (0, 31, 63):
        single = pkg.PacketReceiver(max_items=n)
        for b in range(n_batches):
            ref = single.process_bulk(parts[b][c], 200, tags_cap=128)
            assert np.array_equal(bits(host(got[b][c]["symbols"])), bits(host(ref["symbols"]))), (b, c)
            assert same_tags(got[b][c]["tags"], ref["tags"])


def test_multichannel_packet_receiver_equals_single_channel_receivers(pkg):
    """BASELINE config 3 (full chain): MultiChannelPacketReceiver (one batched detector, per-channel
    chains on worker threads) == one PacketReceiver per channel, bit for bit, over two calls
    (carried state of every block), channels with different CFO and burst positions"""
    C, n = 5, 1 << 17
    rng = np.random.default_rng(2024)
    xs = np.zeros((C, 2 * n), dtype=np.complex64)
    for c in range(C):
        locs = sorted(rng.choice(np.arange(2000, 2 * n // 4 - 2500, 2500), size=9, replace=False).tolist())
        stream, _ = sig.qa_syncword_stream(2 * n // 4, locs, -0.02 + 0.04 * c / (C - 1), seed=40 + c)
        xs[c] = (0.7 * stream[: 2 * n] + sig.awgn(2 * n, 0.05, 90 + c)).astype(np.complex64)
    multi = pkg.MultiChannelPacketReceiver(C, max_items=n, workers=3)
    native = pkg.NativeMultiChannelReceiver(C, max_items=n, tags_cap=256, workers=3)  # the same inside the library
    singles = [pkg.PacketReceiver(max_items=n) for _ in range(C)]
    xd = dev(xs)
    total_tags = 0
    parts = [xd[:, part * n:(part + 1) * n].contiguous() for part in range(2)]
    native.announce(parts[1])  # the detector's look-ahead: the second call's front runs behind the first call
    for part in range(2):
        w = parts[part]
        got = multi.process_bulk(w, 300, tags_cap=256)
        got_native = native.process_bulk(w, 300)
        for c in range(C):
            want = singles[c].process_bulk(w[c], 300, tags_cap=256)
            for g in (got[c], got_native[c]):
                assert g["consumed"] == want["consumed"] > 0
                assert same_tags(g["detector_tags"], want["detector_tags"])
                assert same_tags(g["tags"], want["tags"])
                assert np.array_equal(bits(host(g["symbols"])), bits(host(want["symbols"])))
            total_tags += got[c]["tags"].size
    assert total_tags >= 4 * C


# ------------------------------------------------------------------ SURVEY 8(f) rank 1:
# PayloadMetadataInsert, CostasLoop with control tags, SyncwordRemove, ConstellationLLRDecoder
def _sync_tags(pkg, index, amplitude=0.1, phase=0.0):
    t = np.zeros(len(index), dtype=pkg.TAG_DTYPE)
    t["index"], t["amplitude"], t["phase"], t["flags"] = index, amplitude, phase, pkg.TAG_SYNCWORD
    return t


def same_ptags(a, b):
    """field-wise equality of control tags (records carry padding bytes)"""
    if a.size != b.size:
        return False
    for f in a.dtype.names:
        if f == "syncword":
            if not all(a[f][g].tobytes() == b[f][g].tobytes() for g in a[f].dtype.names):
                return False
        elif a[f].tobytes() != b[f].tobytes():
            return False
    return True


def test_payload_metadata_insert_reference_qa(pkg):
    """test/qa_payload_metadata_insert.cpp:15-157 through the C-ABI, item for item with the oracle"""
    v = np.arange(100000).astype(np.complex64)
    tags = _sync_tags(pkg, [12345])
    r = pkg.PayloadMetadataInsert(64, 128).process_bulk(dev(v), tags)                 # header never arrives
    assert r["out"].numel() == 192 and np.array_equal(host(r["out"]), v[12345:12345 + 192])
    assert r["consumed"] == 12345 + 192 and [int(k) for k in r["tags"]["kind"]] == [1, 2]
    r = pkg.PayloadMetadataInsert(64, 128).process_bulk(dev(v), tags, headers=[100])   # packet_length 100
    want = orc.PayloadMetadataInsert(64, 128).process(v, tags, headers=[100])
    assert r["out"].numel() == 192 + 416 and np.array_equal(bits(host(r["out"])), bits(want["out"]))
    assert same_ptags(r["tags"], want["tags"]) and r["consumed"] == want["consumed"] == v.size
    pt = r["tags"][2]
    assert pt["index"] == 192 and pt["payload_bits"] == 832 and pt["payload_symbols"] == 416 and pt["constellation"] < 0


def test_payload_metadata_insert_chunks_late_and_invalid_headers(pkg):
    """random chunking, headers delivered only when the block stalls for them (:243-247), an invalid
    header (:212-221), a syncword inside a packet (:126-147): GPU == oracle call by call"""
    rng = np.random.default_rng(21)
    n = 200000
    v = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    idx = [1000, 1100, 9000, 20000, 60000, 61000, 150000]
    tags = _sync_tags(pkg, idx, amplitude=np.linspace(0.1, 0.7, len(idx)), phase=np.linspace(-1, 1, len(idx)))
    pending = [300, None, 50, 1500, 1]
    gpu, ref = pkg.PayloadMetadataInsert(64, 128), orc.PayloadMetadataInsert(64, 128)
    pos, headers, out_g, tags_g, ignored = 0, [], [], [], 0
    xd = dev(v)
    while pos < n:
        m = min(int(rng.integers(1, 30000)), n - pos)
        tt = tags[(tags["index"] >= pos) & (tags["index"] < pos + m)].copy()
        tt["index"] -= pos
        g = gpu.process_bulk(xd[pos:pos + m], tt, headers=headers)
        w = ref.process(v[pos:pos + m], tt, headers=headers)
        assert g["consumed"] == w["consumed"] and g["headers_used"] == w["headers_used"] and g["ignored"] == w["ignored"]
        assert np.array_equal(bits(host(g["out"])), bits(w["out"])) and same_ptags(g["tags"], w["tags"])
        out_g.append(host(g["out"]))
        ignored += g["ignored"]
        headers = headers[g["headers_used"]:]
        if g["consumed"] == 0 and pending:
            headers.append(pending.pop(0))
        elif g["consumed"] == 0:
            break
        pos += g["consumed"]
    assert not pending and ignored >= 1
    total = np.concatenate(out_g)
    assert total.size == 192 + 1216 + 192 + 192 + 216 + 192 + 6016 + 192 + 20


def test_syncword_remove(pkg):
    """test/qa_syncword_remove.cpp:13-45 on c64 items + tag handling (syncword_remove.hpp:51-64)"""
    v = np.arange(1000).astype(np.complex64)
    tags = np.zeros(3, dtype=pkg.PACKET_TAG_DTYPE)
    tags["index"], tags["kind"] = [10, 100, 250], pkg.PKT_SYNCWORD
    out, tout = pkg.SyncwordRemove(64).process_bulk(dev(v), tags)
    expected = np.delete(v, np.concatenate([np.arange(i, i + 64) for i in [10, 100, 250]]))
    assert np.array_equal(host(out), expected) and tout.size == 0
    # with header/payload tags, chunked with carried state, against the oracle
    rng = np.random.default_rng(4)
    n = 50000
    v = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    tags = np.zeros(9, dtype=pkg.PACKET_TAG_DTYPE)
    tags["index"] = [100, 164, 292, 3000, 3020, 3064, 3192, 40000, 40064]
    tags["kind"] = [1, 2, 3, 1, 1, 2, 3, 1, 2]
    tags["payload_symbols"] = np.arange(9)
    gpu, ref = pkg.SyncwordRemove(64), orc.SyncwordRemove(64)
    pos = 0
    for m in [120, 30, 2900, 5, 37000, 9945]:
        tt = tags[(tags["index"] >= pos) & (tags["index"] < pos + m)].copy()
        tt["index"] -= pos
        o, t = gpu.process_bulk(dev(v[pos:pos + m]), tt)
        wo, wt = ref.process(v[pos:pos + m], tt)
        assert np.array_equal(bits(host(o)), bits(wo)) and same_ptags(t, wt)
        pos += m
    assert pos == n


@pytest.mark.parametrize("constellation", ["BPSK", "QPSK"])
def test_constellation_llr_decoder(pkg, constellation):
    """test/qa_constellation_llr_decoder.cpp:15-62 (noise_sigma 1 -> scale 2), bit-exact"""
    rng = np.random.default_rng(3)
    n = 100000
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    y, tags = pkg.ConstellationLLRDecoder(1.0, constellation).process_bulk(dev(x))
    y = y.cpu().numpy()
    if constellation == "BPSK":
        assert y.size == n and np.array_equal(y, np.float32(2.0) * x.real)
    else:
        assert y.size == 2 * n and np.array_equal(y[0::2], np.float32(2) * x.real) and np.array_equal(y[1::2], np.float32(2) * x.imag)
    assert tags.size == 0
    want, _ = orc.ConstellationLLRDecoder(1.0, constellation).process(x)
    assert y.tobytes() == want.tobytes()


def test_constellation_llr_decoder_tags_and_pilot(pkg):
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(5000) + 1j * rng.standard_normal(5000)).astype(np.complex64)
    tags = np.zeros(4, dtype=pkg.PACKET_TAG_DTYPE)
    tags["index"], tags["kind"] = [0, 128, 1000, 1128], [2, 3, 2, 3]
    tags["constellation"], tags["loop_bandwidth"] = [2, -1, 1, 2], -1.0
    y, tout = pkg.ConstellationLLRDecoder(0.7, "BPSK").process_bulk(dev(x), tags)
    wy, wt = orc.ConstellationLLRDecoder(0.7, "BPSK").process(x, tags)
    assert y.cpu().numpy().tobytes() == wy.tobytes() and same_ptags(tout, wt)
    assert [int(i) for i in tout["index"]] == [0, 256, 2000, 2128]
    with pytest.raises(pkg.Gr4pmError):
        pkg.ConstellationLLRDecoder(1.0, "PILOT")


def test_symbol_rate_chain_to_llrs(pkg):
    """wiped-off symbols -> PayloadMetadataInsert -> CostasLoop (tag-driven PILOT/QPSK and loop
    bandwidths) -> SyncwordRemove -> ConstellationLLRDecoder, GPU against the oracle chain; the
    hard decisions of the payload LLRs recover the transmitted bits"""
    rng = np.random.default_rng(31)
    lengths = [100, 20, 1500, 7, 400]
    gap = 300
    a = np.float32(np.sqrt(0.5))
    sym, idx, bits_tx, pos = [], [], [], 50
    stream = [np.zeros(50, np.complex64)]
    for k, plen in enumerate(lengths):
        n_sym = 128 + (plen + 4) * 4
        b = rng.integers(0, 2, (n_sym, 2))
        q = ((1 - 2 * b[:, 0]) * a + 1j * (1 - 2 * b[:, 1]) * a).astype(np.complex64)
        pkt = np.concatenate([np.ones(64, np.complex64), q])   # syncword already wiped off: pure pilot
        ph = rng.uniform(-3, 3)
        pkt = pkt * np.exp(1j * (ph + 0.003 * (k - 2) * np.arange(pkt.size)))
        idx.append(pos)
        bits_tx.append(b)
        stream.append(pkt.astype(np.complex64))
        stream.append(np.zeros(gap, np.complex64))
        pos += pkt.size + gap
        sym.append(ph)
    x = np.concatenate(stream)
    x = (x + sig.awgn(x.size, 0.05, 77)).astype(np.complex64)
    tags = _sync_tags(pkg, idx, amplitude=1.0, phase=np.array(sym, dtype=np.float32))
    # oracle chain
    o1 = orc.PayloadMetadataInsert(64, 128).process(x, tags, headers=lengths)
    o2 = orc.CostasLoop(0.01, "BPSK").process(o1["out"], o1["tags"])
    o3, o3t = orc.SyncwordRemove(64).process(o2, o1["tags"])
    o4, o4t = orc.ConstellationLLRDecoder(0.7, "QPSK").process(o3, o3t)
    # GPU chain, input in two pieces
    pmi, cl, sr, dec = (pkg.PayloadMetadataInsert(64, 128), pkg.CostasLoop(0.01, "BPSK"), pkg.SyncwordRemove(64),
                        pkg.ConstellationLLRDecoder(0.7, "QPSK"))
    llr, ltags, cut, headers, base = [], [], 5000, list(lengths), 0
    for lo, hi in [(0, cut), (cut, x.size)]:
        tt = tags[(tags["index"] >= lo) & (tags["index"] < hi)].copy()
        tt["index"] -= lo
        g1 = pmi.process_bulk(dev(x[lo:hi]), tt, headers=headers)
        assert g1["consumed"] == hi - lo
        headers = headers[g1["headers_used"]:]
        g2 = cl.process_packets(g1["out"], g1["tags"])
        g3, g3t = sr.process_bulk(g2, g1["tags"])
        g4, g4t = dec.process_bulk(g3, g3t)
        g4t["index"] += base
        base += g4.numel()
        llr.append(g4.cpu().numpy())
        ltags.append(g4t)
    llr, ltags = np.concatenate(llr), np.concatenate(ltags)
    assert llr.size == o4.size == 2 * sum(128 + (p + 4) * 4 for p in lengths)
    err = np.max(np.abs(llr - o4))
    print("chain to LLRs: max |gpu - oracle| =", err, "of scale", np.max(np.abs(o4)))
    assert err == 0.0                       # every stage of the chain is bit-exact, the Costas loop included
    assert same_ptags(ltags, o4t)
    # payload bits (LLR > 0 <-> bit 0, constellation_llr_decoder.hpp:24-26)
    p = 0
    for b in bits_tx:
        hard = (llr[p:p + 2 * b.shape[0]] < 0).astype(int).reshape(-1, 2)
        assert np.array_equal(hard[64:], b[64:])   # the loop has settled after the first symbols
        p += 2 * b.shape[0]


# ------------------------------------------------------------------ header decode loop
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_additive_scrambler(pkg):
    """test/qa_additive_scrambler.cpp:26-112 through the C-ABI (hard and soft symbols), resets by tag
    and by count, state carried across calls; bit-exact against the oracle"""
    ccsds = np.load(os.path.join(GOLDEN, "qa_ccsds_scrambling_sequence.npy"))
    rng = np.random.default_rng(1)
    x = rng.integers(0, 2, 100000).astype(np.uint8)
    y = pkg.AdditiveScrambler(0xA9, 0xFF, 7, dtype="uint8").process_bulk(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.array_equal(y, x ^ ccsds[np.arange(x.size) % 255])
    first40 = np.load(os.path.join(GOLDEN, "qa_ccsds_2023_first40.npy"))
    z = pkg.AdditiveScrambler(0x4001, 0x18E38, 16, dtype="uint8").process_bulk(torch.zeros(40, dtype=torch.uint8).cuda())
    assert np.array_equal(z.cpu().numpy(), first40)
    z = pkg.AdditiveScrambler(0xA9, 0xFF, 7, dtype="uint8").process_bulk(torch.zeros(100000, dtype=torch.uint8).cuda(),
                                                                          np.arange(0, 100000, 100))
    assert np.array_equal(z.cpu().numpy(), ccsds[np.arange(100000) % 100])
    # the receiver's descrambler (packet_receiver.hpp:131-135) on soft symbols, in pieces, vs the oracle
    llr = rng.standard_normal(300000).astype(np.float32)
    resets = np.sort(rng.choice(300000, 40, replace=False))
    want = orc.AdditiveScrambler(0x4001, 0x18E38, 16).process(llr, resets)
    gpu = pkg.AdditiveScrambler(0x4001, 0x18E38, 16)
    got, pos = [], 0
    for m in [1, 70000, 131071, 98928]:
        r = resets[(resets >= pos) & (resets < pos + m)] - pos
        got.append(gpu.process_bulk(torch.from_numpy(llr[pos:pos + m]).cuda(), r).cpu().numpy())
        pos += m
    assert pos == llr.size and np.concatenate(got).tobytes() == want.tobytes()
    c = pkg.AdditiveScrambler(0xA9, 0xFF, 7, count=100).process_bulk(torch.ones(1000).cuda()).cpu().numpy()
    assert np.array_equal(c, 1.0 - 2.0 * ccsds[np.arange(1000) % 100])


@pytest.mark.parametrize("header_size,payload_bits", [(256, 1500), (128, 1500), (256, 1), (64, 17321)])
def test_header_payload_split(pkg, header_size, payload_bits):
    """test/qa_header_payload_split.cpp:14-57"""
    v = np.arange(header_size + payload_bits).astype(np.float32)
    tags = np.zeros(1, dtype=pkg.PACKET_TAG_DTYPE)
    tags["index"], tags["kind"], tags["payload_bits"] = header_size, pkg.PKT_PAYLOAD, payload_bits
    h, p, ht, pt = pkg.HeaderPayloadSplit(header_size).process_bulk(torch.from_numpy(v).cuda(), tags)
    assert np.array_equal(h.cpu().numpy(), v[:header_size]) and np.array_equal(p.cpu().numpy(), v[header_size:])
    assert ht.size == 0 and pt.size == 1 and pt[0]["index"] == 0


def test_header_payload_split_stream_vs_oracle(pkg):
    """packets back to back, failed headers (no payload tag), chunked calls with carried state"""
    rng = np.random.default_rng(6)
    items, tags, pos = [], [], 0
    for k in range(60):
        items.append(rng.standard_normal(256).astype(np.float32))
        pos += 256
        t = np.zeros(1, dtype=pkg.PACKET_TAG_DTYPE)
        t["index"], t["kind"] = pos - 256, pkg.PKT_HEADER_START
        tags.append(t)
        if k % 5 != 3:   # header decoded: a payload follows
            n = int(rng.integers(1, 3000))
            t = np.zeros(1, dtype=pkg.PACKET_TAG_DTYPE)
            t["index"], t["kind"], t["payload_bits"] = pos, pkg.PKT_PAYLOAD, n
            tags.append(t)
            items.append(rng.standard_normal(n).astype(np.float32))
            pos += n
    x, tags = np.concatenate(items), np.concatenate(tags)
    gpu, ref = pkg.HeaderPayloadSplit(256), orc.HeaderPayloadSplit(256)
    p0 = 0
    while p0 < x.size:
        m = min(int(rng.integers(1, 20000)), x.size - p0)
        tt = tags[(tags["index"] >= p0) & (tags["index"] < p0 + m)].copy()
        tt["index"] -= p0
        h, p, ht, pt = gpu.process_bulk(torch.from_numpy(x[p0:p0 + m]).cuda(), tt)
        wh, wp, wht, wpt = ref.process(x[p0:p0 + m], tt)
        assert h.cpu().numpy().tobytes() == wh.tobytes() and p.cpu().numpy().tobytes() == wp.tobytes()
        assert same_ptags(ht, wht) and same_ptags(pt, wpt)
        p0 += m
    bad = np.zeros(1, dtype=pkg.PACKET_TAG_DTYPE)
    bad["index"], bad["kind"], bad["payload_bits"] = 10, pkg.PKT_PAYLOAD, 5
    with pytest.raises(pkg.Gr4pmError):
        pkg.HeaderPayloadSplit(256).process_bulk(torch.zeros(100).cuda(), bad)
    # HeaderPayloadSplit<std::complex<float>> (packet_receiver.hpp:159-162, the symbol tap: gr4pm_header_payload_split_
    # process_c64, the instantiation the reference's packet_receiver.hpp needs from the drop-in header): the same state
    # machine over complex items -- real and imaginary parts are each what the oracle's float block gives
    xc = (x + 1j * rng.standard_normal(x.size)).astype(np.complex64)
    gpu, ref_re, ref_im = pkg.HeaderPayloadSplit(256), orc.HeaderPayloadSplit(256), orc.HeaderPayloadSplit(256)
    p0 = 0
    while p0 < xc.size:
        m = min(int(rng.integers(1, 20000)), xc.size - p0)
        tt = tags[(tags["index"] >= p0) & (tags["index"] < p0 + m)].copy()
        tt["index"] -= p0
        h, p, ht, pt = gpu.process_bulk(torch.from_numpy(xc[p0:p0 + m]).cuda(), tt)
        wh, wp, wht, wpt = ref_re.process(np.ascontiguousarray(xc[p0:p0 + m].real), tt)
        ih, ip, _, _ = ref_im.process(np.ascontiguousarray(xc[p0:p0 + m].imag), tt)
        h, p = h.cpu().numpy(), p.cpu().numpy()
        assert h.dtype == np.complex64 and h.real.tobytes() == wh.tobytes() and h.imag.tobytes() == ih.tobytes()
        assert p.real.tobytes() == wp.tobytes() and p.imag.tobytes() == ip.tobytes()
        assert same_ptags(ht, wht) and same_ptags(pt, wpt)
        p0 += m


def test_header_fec_decoder_reference_qa(pkg):
    """test/qa_header_fec_decoder.cpp:16-101 through the C-ABI"""
    gen = np.load(os.path.join(GOLDEN, "header_ldpc_generator.npy"))
    v = np.load(os.path.join(GOLDEN, "qa_header_fec_valid_bytes.npy"))
    llr = 1.0 - 2.0 * np.unpackbits(orc.header_fec_encode(v, gen).ravel()).astype(np.float32)
    dec = pkg.HeaderFecDecoder()
    out, invalid = dec.process_bulk(torch.from_numpy(llr).cuda())
    assert np.array_equal(out.ravel(), v) and not invalid.any()
    r = np.load(os.path.join(GOLDEN, "qa_header_fec_random_bytes.npy"))
    out, invalid = dec.process_bulk(torch.from_numpy(1.0 - 2.0 * np.unpackbits(r).astype(np.float32)).cuda())
    assert out.shape == (8, 4) and invalid.all()
    msgs, ptype = pkg.header_parse(out, invalid)
    assert msgs["invalid_header"].all() and (ptype == -1).all()


def test_header_fec_decoder_noisy_vs_oracle(pkg):
    """4000 headers at Es/N0 = 0 dB and -3 dB: decoded bytes and verdicts identical to the oracle's
    (same schedule, same arithmetic), parser agrees with header_parser.hpp:56-85"""
    gen = np.load(os.path.join(GOLDEN, "header_ldpc_generator.npy"))
    rng = np.random.default_rng(12)
    n = 4000
    lengths = rng.integers(0, 65536, n)
    types = rng.integers(0, 3, n)
    hdr = np.stack([orc.header_format(int(a), int(t)) for a, t in zip(lengths, types)])
    bits = np.unpackbits(orc.header_fec_encode(hdr, gen).ravel()).astype(np.float32).reshape(n, 256)
    sigma = np.where(np.arange(n) % 2 == 0, np.sqrt(0.5), 1.0)[:, None]
    y = (1.0 - 2.0 * bits) * np.sqrt(0.5) + sigma * rng.standard_normal(bits.shape)
    llr = (2.0 / 0.7**2 * y).astype(np.float32).ravel()    # the receiver's fixed noise_sigma, packet_receiver.hpp:129
    want, want_inv = orc.HeaderFecDecoder(pkg.header_ldpc_alist()).process(llr)
    got, got_inv = pkg.HeaderFecDecoder().process_bulk(torch.from_numpy(llr).cuda())
    assert np.array_equal(got_inv, want_inv) and np.array_equal(got, want)
    ok = ~got_inv
    assert ok[0::2].mean() > 0.95 and np.array_equal(got[ok], hdr[ok])
    msgs, ptype = pkg.header_parse(got, got_inv)
    for m, pt, h, bad in zip(msgs, ptype, got, got_inv):
        want_len = orc.header_parse(h, bad)
        assert (m["invalid_header"] == 1) == (want_len is None)
        if want_len is not None:
            assert m["packet_length"] == want_len and pt == h[2]


def test_header_fec_decoder_8bit_messages_vs_oracle(pkg):
    """the decoder's second message arithmetic (gr4pm_header_fec_decoder_params::arithmetic = 1: 8-bit messages, what the
    reference's decoder name "HLAminstari8" says it runs, header_fec_decoder.hpp:276) against the oracle's restatement of
    the same form: bytes and verdicts identical; the reference's own byte vectors decode in this form too"""
    gen = np.load(os.path.join(GOLDEN, "header_ldpc_generator.npy"))
    rng = np.random.default_rng(13)
    n = 4000
    hdr = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    bits = np.unpackbits(orc.header_fec_encode(hdr, gen).ravel()).astype(np.float32).reshape(n, 256)
    sigma = np.where(np.arange(n) % 2 == 0, np.sqrt(0.5), 1.0)[:, None]
    y = (1.0 - 2.0 * bits) * np.sqrt(0.5) + sigma * rng.standard_normal(bits.shape)
    llr = (2.0 / 0.7**2 * y).astype(np.float32).ravel()
    llr[: 256 * 50] *= 40.0  # some codewords far into the saturation of channel LLRs and messages
    want, want_inv = orc.HeaderFecDecoder(pkg.header_ldpc_alist()).process(llr, arithmetic=1)
    dec = pkg.HeaderFecDecoder(arithmetic=1)
    got, got_inv = dec.process_bulk(torch.from_numpy(llr).cuda())
    assert np.array_equal(got_inv, want_inv) and np.array_equal(got, want)
    assert (~got_inv)[0::2].mean() > 0.95
    v = np.load(os.path.join(GOLDEN, "qa_header_fec_valid_bytes.npy"))   # test/qa_header_fec_decoder.cpp:16-101
    out, invalid = dec.process_bulk(torch.from_numpy(1.0 - 2.0 * np.unpackbits(orc.header_fec_encode(v, gen).ravel()).astype(np.float32)).cuda())
    assert np.array_equal(out.ravel(), v) and not invalid.any()
    r = np.load(os.path.join(GOLDEN, "qa_header_fec_random_bytes.npy"))
    out, invalid = dec.process_bulk(torch.from_numpy(1.0 - 2.0 * np.unpackbits(r).astype(np.float32)).cuda())
    assert invalid.all()
    with pytest.raises(pkg.Gr4pmError, match="arithmetic"):
        pkg.HeaderFecDecoder(arithmetic=2)


def test_header_fec_decoder_decisions_do_not_hang_on_the_message_width(pkg):
    """SURVEY 8(f) rank 2 stays "parity unpinned": the reference decodes its headers in the Rust crate ldpc-toolbox
    ("HLAminstari8": horizontal-layered schedule, A-Min* check rule, 8-bit messages), which is not part of the reference
    tree.  The product runs that schedule and that rule with float32 messages; the ONE known difference is the message
    width.  100 000 noisy headers per Es/N0 point through both forms of the product's decoder (float32 / 8-bit messages,
    LLRs scaled as the receiver scales them, packet_receiver.hpp:129: 2 / 0.7^2):
      * where the reference is run and tested (test/qa_loopback.cpp:24-140: AWGN of amplitude 0.05 on unit-energy
        symbols = Es/N0 23 dB) and down to 2 dB: not one frame error, not one differing decision in either form;
      * across the waterfall (0 ... -4 dB): frame-error rates within 0.02 of each other and within 15 % relative where
        the rate is above 1 %, decisions differing on under a tenth of the frames;
      * neither form ever delivers a wrong header as valid beyond 1 in 10 000 (the 4-byte header has no CRC: what the
        decoder accepts is a codeword)."""
    gen = np.load(os.path.join(GOLDEN, "header_ldpc_generator.npy"))
    rng = np.random.default_rng(14)
    n = 100000
    hdr = rng.integers(0, 256, (n, 4)).astype(np.uint8)
    tx = torch.from_numpy((1.0 - 2.0 * np.unpackbits(orc.header_fec_encode(hdr, gen).ravel()).astype(np.float32)) * np.float32(np.sqrt(0.5))).cuda()
    dec = [pkg.HeaderFecDecoder(arithmetic=0), pkg.HeaderFecDecoder(arithmetic=1)]
    g = torch.Generator(device="cuda")
    g.manual_seed(15)
    table = []
    for esn0_db in (23.0, 10.0, 5.0, 2.0, 0.0, -1.0, -2.0, -3.0, -4.0):
        sigma = float(np.sqrt(0.5 / 10 ** (esn0_db / 10)))
        llr = (tx + sigma * torch.randn(tx.numel(), generator=g, device="cuda")) * (2.0 / 0.7**2)
        res = [d.process_bulk(llr) for d in dec]
        err = [inv | np.any(out != hdr, axis=1) for out, inv in res]
        undetected = [float(np.mean(~inv & np.any(out != hdr, axis=1))) for out, inv in res]
        fer = [float(e.mean()) for e in err]
        differ = float(np.mean(err[0] != err[1]))
        table.append((esn0_db, fer[0], fer[1], differ, undetected[0], undetected[1]))
        if esn0_db >= 2.0:
            assert fer == [0.0, 0.0] and differ == 0.0, table[-1]
        else:
            assert abs(fer[0] - fer[1]) <= 0.02, table[-1]
            if min(fer) > 0.01:
                assert abs(fer[0] - fer[1]) <= 0.15 * max(fer), table[-1]
            assert differ < 0.1, table[-1]
        assert max(undetected) <= 1e-4, table[-1]
    assert table[-1][1] > 0.2 and table[4][1] < 1e-3, table  # the sweep did cross the waterfall
    print("Es/N0 dB, FER float32, FER 8-bit, frames with differing verdicts, undetected float32, undetected 8-bit")
    for row in table:
        print("%6.1f  %.5f  %.5f  %.5f  %.6f  %.6f" % row)


def _tx_packets(rng, lengths, gaps, sps=4, types=None):
    """transmit side of the header loop for the tests (numpy + oracle helpers): syncword, header
    (header_formatter.hpp:104-107 -> header_fec_encoder.hpp -> CCSDS 131.0-B-5 scrambler restarted at
    the header), payload bits under the same running scrambler, QPSK, RRC at 4 samples/symbol"""
    gen = np.load(os.path.join(GOLDEN, "header_ldpc_generator.npy"))
    a = np.float32(np.sqrt(0.5))
    rrc, _ = orc.unit_norm_rrc(sps)
    syms, starts, payloads = [], [], []
    for k, (plen, gap) in enumerate(zip(lengths, gaps)):
        hdr = orc.header_format(plen, 0 if types is None else types[k])
        coded = np.unpackbits(orc.header_fec_encode(hdr, gen).ravel())
        payload = rng.integers(0, 2, 8 * (plen + 4)).astype(np.uint8)
        bits = orc.AdditiveScrambler(0x4001, 0x18E38, 16).process(np.concatenate([coded, payload]))
        q = ((1 - 2.0 * bits[0::2]) * a + 1j * (1 - 2.0 * bits[1::2]) * a).astype(np.complex64)
        syms += [np.zeros(gap, np.complex64), sig.BPSK[sig.SYNCWORD], q]
        starts.append(sum(len(s) for s in syms[:-2]))
        payloads.append(payload)
    syms.append(np.zeros(1500, np.complex64))
    return orc.interpolating_fir(np.concatenate(syms), sps, rrc), starts, payloads


def test_packet_receiver_device_ring_equals_copy(pkg):
    """history= (the chain reads SyncwordDetection's delayed stream in place from the caller's ring,
    syncword_detection.hpp:318-319) gives exactly the symbols of the copying path, for windows at
    different offsets of one ring"""
    rng = np.random.default_rng(77)
    xs = []
    for seed in (1, 2):
        x, _, _ = _tx_packets(np.random.default_rng(seed), [50, 200, 9], [400, 700, 350])
        x = np.concatenate([x, np.zeros(30000, np.complex64)])[:30000]
        xs.append((x + sig.awgn(30000, 0.05, 80 + seed)).astype(np.complex64))
    H = 1537
    ring = torch.zeros(3 + H + 2 * 30000, dtype=torch.complex64, device="cuda")
    a0, b0 = 3 + H, 3 + H + 30000
    ring[a0:a0 + 30000] = dev(xs[0])
    ring[b0:b0 + 30000] = dev(xs[1])
    ring[a0 - H:a0] = 0          # the stream starts with window A: zeros before it (empty history)
    plain = pkg.PacketReceiver(max_items=30000)
    inring = pkg.PacketReceiver(max_items=30000)
    for lo in (a0, b0):
        w = ring[lo:lo + 30000]
        want = plain.process_bulk(w, 100)
        got = inring.process_bulk(w, 100, history=ring[lo - H:lo])
        assert got["consumed"] == want["consumed"] and got["tags"].size == want["tags"].size > 0
        assert np.array_equal(bits(host(got["symbols"])), bits(host(want["symbols"])))
        # the next window continues the stream: its history is the tail of this one, which is what
        # the ring holds in front of window B only for the samples the detector consumed
        if lo == a0:
            c = want["consumed"]
            ring[b0:b0 + 30000 - c] = ring[a0 + c:a0 + 30000].clone()   # unconsumed tail of A comes first
            ring[b0 + 30000 - c:b0 + 30000] = dev(xs[1])[:c]
            ring[b0 - H:b0] = ring[a0 + c - H:a0 + c].clone()


@pytest.mark.parametrize("mode", ["one_call", "three_calls", "pipelined"])
def test_packet_receiver_decodes_its_own_headers(pkg, mode):
    """PacketReceiver(decode_headers=True): nothing but IQ samples goes in.  Every transmitted header
    is decoded (length, type), every payload bit comes back from the descrambled payload LLRs, the
    headers the exact chain decodes agree with the ones it was given, and cutting the stream in
    the middle of a header (pending message) changes nothing."""
    rng = np.random.default_rng(401)
    lengths = [100, 17, 1500, 1, 333, 64, 900]
    gaps = [int(g) for g in rng.integers(250, 900, len(lengths))]
    types = [0, 1, 0, 0, 1, 0, 0]
    x, starts, payloads = _tx_packets(rng, lengths, gaps, types=types)
    x = (orc.rotator(x, np.float32(-0.013)) * np.exp(1j * 2.1) + sig.awgn(x.size, 0.05, 402)).astype(np.complex64)
    if mode == "three_calls":
        # the detector consumes whole strides of 1752 samples and delays by 1537: pad the front so
        # that a stride boundary falls on symbol 110 of packet 2 (46 symbols into its header)
        S = 1752
        target = 4 * (starts[2] + 110) + 1537
        k1 = target // S + 1
        pad = k1 * S - target
        x = np.concatenate([sig.awgn(pad, 0.05, 403).astype(np.complex64), x])
        c1 = k1 * S + 2048 - S
        c2 = (k1 + 9) * S + 2048 - S
    rx = pkg.PacketReceiver(max_items=x.size, pipelined=(mode == "pipelined"), decode_headers=True)
    results = []
    xd = dev(x)
    if mode == "three_calls":
        pos = 0
        for want in [c1, c2 - k1 * S, x.size]:
            r = rx.process_bulk(xd[pos:min(pos + want, x.size)])
            if not results:  # the first cut is inside packet 2's header: its message is still pending
                assert rx._pending_real is not None and r["headers"]["invalid_header"][-1] == 2
            results.append(r)
            pos += r["consumed"]
            if pos + 2048 > x.size:
                break
    else:
        r = rx.process_bulk(xd)
        results = rx.flush() if mode == "pipelined" else [r]
    msgs = np.concatenate([r["header_messages"] for r in results])
    ptype = np.concatenate([r["packet_type"] for r in results])
    assert sum(r["header_mismatches"] for r in results) == 0
    good = msgs[msgs["invalid_header"] == 0]
    assert [int(v) for v in good["packet_length"]] == lengths
    assert [int(t) for t in ptype[msgs["invalid_header"] == 0]] == types
    pay = np.concatenate([r["payload_llr"].cpu().numpy() for r in results])
    want_bits = np.concatenate(payloads)
    assert pay.size == want_bits.size
    assert np.array_equal((pay < 0).astype(np.uint8), want_bits)
    if mode == "three_calls":
        assert len(results) == 3


# ------------------------------------------------------------------ payload tail (packet_receiver.hpp:140-147)
def test_binary_slicer_pack_bits_crc(pkg):
    """test/qa_binary_slicer.cpp (both polarities), pack_bits.hpp (MSB / LSB), test/qa_crc.cpp:17-21 and the
    CRC-32 / CRC-16 / CRC-8 check values through the C-ABI; CrcCheck against the oracle"""
    import zlib
    rng = np.random.default_rng(5)
    x = rng.standard_normal(100000).astype(np.float32)
    x[:3] = [0.0, -0.0, 1e-30]
    xd = torch.from_numpy(x).cuda()
    assert np.array_equal(pkg.binary_slicer(xd).cpu().numpy(), (x > 0).astype(np.uint8))
    assert np.array_equal(pkg.binary_slicer(xd, invert=True).cpu().numpy(), (x < 0).astype(np.uint8))
    bits = rng.integers(0, 2, 80000).astype(np.uint8)
    bd = torch.from_numpy(bits).cuda()
    assert np.array_equal(pkg.pack_bits(bd).cpu().numpy(), np.packbits(bits))
    assert np.array_equal(pkg.pack_bits(bd, msb_first=False).cpu().numpy(), np.packbits(bits, bitorder="little"))
    two = rng.integers(0, 4, 40000).astype(np.uint8)
    want = (two[0::4] << 6) | (two[1::4] << 4) | (two[2::4] << 2) | two[3::4]
    assert np.array_equal(pkg.pack_bits(torch.from_numpy(two).cuda(), 4, 2).cpu().numpy(), want)
    assert np.array_equal(pkg.slice_pack(xd[:80000]).cpu().numpy(), np.packbits((x[:80000] < 0).astype(np.uint8)))
    crc16 = pkg.CrcCheck(16, 0x1021, 0xFFFF, 0xFFFF, True, True)
    assert crc16.compute(np.zeros(10, np.uint8)) == 0x6378
    msg = np.frombuffer(b"123456789", dtype=np.uint8)
    assert pkg.CrcCheck().compute(msg) == 0xCBF43926
    assert pkg.CrcCheck(16, 0x1021, 0xFFFF, 0, False, False).compute(msg) == 0x29B1
    # packets: good, corrupted, too short; CRC-32 big-endian at the end (crc_check.hpp:167-178)
    pk, lens = [], []
    for k, n in enumerate([100, 1, 1500, 3, 64, 65535, 4, 2, 777]):
        body = rng.integers(0, 256, n).astype(np.uint8)
        if n <= 4 and k >= 6:
            pk.append(body)
            lens.append(n)
            continue
        crc = zlib.crc32(body.tobytes())
        tail = np.array([(crc >> s) & 0xFF for s in (24, 16, 8, 0)], dtype=np.uint8)
        if k in (2, 8):
            body = body.copy()
            body[n // 2] ^= 0x40
        pk.append(np.concatenate([body, tail]))
        lens.append(n + 4)
    stream = np.concatenate(pk)
    for discard in (False, True):
        want, want_len = orc.crc_check(stream, lens, discard_crc=discard, **orc.CRC32)
        got, got_len = pkg.CrcCheck(discard_crc=discard).process_bulk(torch.from_numpy(stream).cuda(), lens)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_len, want_len)
    assert [int(v > 0) for v in want_len] == [1, 1, 0, 1, 1, 1, 0, 0, 0]


@pytest.mark.gpu
def test_crc_check_thousands_of_packets_leave_back_to_back(pkg):
    """crc_check.hpp:180-202 with more packets than one pass of the device-side span builder handles (k_crc_spans: 1024 a
    time with a running carry): random lengths, one packet in five corrupted, a few too short to hold a CRC -- the passing
    ones back to back, their lengths, both discard_crc settings, against the oracle"""
    import zlib
    rng = np.random.default_rng(77)
    n_pk = 3 * 1024 + 77
    pk, lens = [], []
    for k in range(n_pk):
        n = int(rng.integers(1, 300)) if k % 97 else 1500
        if k % 211 == 5:  # too short for a CRC-32
            pk.append(rng.integers(0, 256, 3).astype(np.uint8))
            lens.append(3)
            continue
        body = rng.integers(0, 256, n).astype(np.uint8)
        crc = zlib.crc32(body.tobytes())
        tail = np.array([(crc >> sh) & 0xFF for sh in (24, 16, 8, 0)], dtype=np.uint8)
        if rng.random() < 0.2:
            body = body.copy()
            body[int(rng.integers(0, n))] ^= 1 << int(rng.integers(0, 8))
        pk.append(np.concatenate([body, tail]))
        lens.append(n + 4)
    stream = np.concatenate(pk)
    sd = torch.from_numpy(stream).cuda()
    for discard in (False, True):
        want, want_len = orc.crc_check(stream, lens, discard_crc=discard, **orc.CRC32)
        got, got_len = pkg.CrcCheck(discard_crc=discard).process_bulk(sd, lens)
        assert np.array_equal(got_len, want_len)
        assert np.array_equal(got.cpu().numpy(), want)
    passed = int(np.count_nonzero(np.asarray(want_len)))
    assert 0.7 * n_pk < passed < 0.9 * n_pk  # (the mix the test is about)


@pytest.mark.parametrize("name,params", [
    ("CRC-32 (the receiver's)", dict(num_bits=32, poly=0x4C11DB7, initial_value=0xFFFFFFFF, final_xor=0xFFFFFFFF,
                                     input_reflected=True, result_reflected=True)),
    ("CRC-32/MPEG-2: plain input, 32 bits", dict(num_bits=32, poly=0x4C11DB7, initial_value=0xFFFFFFFF, final_xor=0,
                                                  input_reflected=False, result_reflected=False)),
    ("CRC-32, reflected in, plain out", dict(num_bits=32, poly=0x4C11DB7, initial_value=0x12345678, final_xor=0xA5A5A5A5,
                                              input_reflected=True, result_reflected=False)),
    ("CRC-16/ARC: reflected, 16 bits", dict(num_bits=16, poly=0x8005, initial_value=0, final_xor=0,
                                             input_reflected=True, result_reflected=True)),
    ("CRC-8/ROHC: reflected, 8 bits", dict(num_bits=8, poly=0x07, initial_value=0xFF, final_xor=0,
                                            input_reflected=True, result_reflected=True)),
    ("CRC-16/CCITT-FALSE: plain input, 16 bits (byte-wise kernel)", dict(num_bits=16, poly=0x1021, initial_value=0xFFFF,
                                                                        final_xor=0, input_reflected=False,
                                                                        result_reflected=False)),
    ("CRC-64/XZ (byte-wise kernel)", dict(num_bits=64, poly=0x42F0E1EBA9EA3693, initial_value=0xFFFFFFFFFFFFFFFF,
                                           final_xor=0xFFFFFFFFFFFFFFFF, input_reflected=True, result_reflected=True)),
])
def test_crc_check_eight_bytes_a_step_equals_the_byte_loop(pkg, monkeypatch, name, params):
    """round 6: k_crc_check_sliced (registers of <= 32 bits; reflected input, or plain input at 32 bits) against the oracle's
    byte loop (crc.hpp:119-156, crc_check.hpp:152-208) and against the library's own byte-wise kernel
    (GR4PM_CRC_BYTEWISE): packets of 1 .. 700 bytes back to back -- every alignment of a packet's first byte, every
    length of head and tail around the 8-byte words --, one in four damaged, some too short; skip_header_bytes and both
    byte orders of the CRC in the packet"""
    rng = np.random.default_rng(len(name))
    nb = params["num_bits"] // 8
    for skip, swap in ((0, False), (3, False), (0, True), (11, True)):
        pk, lens = [], []
        for k in range(400):
            n = int(rng.integers(1, 700))
            body = rng.integers(0, 256, n).astype(np.uint8)
            if k % 37 == 0:  # too short to hold a CRC
                pk.append(body[:nb])
                lens.append(min(n, nb))
                continue
            crc = orc.crc_compute(body[min(skip, n):], **params)
            tail = np.array([(crc >> (8 * i)) & 0xFF for i in range(nb)], dtype=np.uint8)
            if not swap:
                tail = tail[::-1]
            if rng.random() < 0.25:
                body = body.copy()
                body[int(rng.integers(0, n))] ^= 1 << int(rng.integers(0, 8))
            pk.append(np.concatenate([body, tail]))
            lens.append(n + nb)
        stream = np.concatenate(pk)
        sd = torch.from_numpy(stream).cuda()
        want, want_len = orc.crc_check(stream, lens, swap_endianness=swap, skip_header_bytes=skip, **params)
        got, got_len = pkg.CrcCheck(swap_endianness=swap, skip_header_bytes=skip, **params).process_bulk(sd, lens)
        assert np.array_equal(got_len, want_len), (name, skip, swap)
        assert np.array_equal(got.cpu().numpy(), want)
        monkeypatch.setenv("GR4PM_CRC_BYTEWISE", "1")
        got_b, got_len_b = pkg.CrcCheck(swap_endianness=swap, skip_header_bytes=skip, **params).process_bulk(sd, lens)
        monkeypatch.delenv("GR4PM_CRC_BYTEWISE")
        assert np.array_equal(got_len_b, want_len) and np.array_equal(got_b.cpu().numpy(), want)
        passed = int(np.count_nonzero(np.asarray(want_len)))
        # (a damaged byte in front of skip_header_bytes is not covered by the CRC; an 8-bit CRC misses one error in 256)
        assert 0.6 * len(lens) < passed < 0.9 * len(lens), (name, passed)


@pytest.mark.parametrize("mode", ["one_call", "three_calls"])
def test_packet_receiver_iq_to_packets(pkg, mode):
    """the whole receive chain of packet_receiver.hpp on the device: IQ samples in, the bytes of every
    packet whose CRC-32 matches out (payload = user bytes + CRC-32, crc_append on the transmit side)"""
    import zlib
    rng = np.random.default_rng(501)
    lengths = [100, 17, 1500, 1, 333, 64, 900]
    gaps = [int(g) for g in rng.integers(250, 900, len(lengths))]
    gen = np.load(os.path.join(GOLDEN, "header_ldpc_generator.npy"))
    a = np.float32(np.sqrt(0.5))
    rrc, _ = orc.unit_norm_rrc(4)
    syms, user = [], []
    for k, (plen, gap) in enumerate(zip(lengths, gaps)):
        data = rng.integers(0, 256, plen).astype(np.uint8)
        crc = zlib.crc32(data.tobytes())
        if k == 4:
            crc ^= 0x00010000                                     # this one arrives damaged
        body = np.concatenate([data, np.array([(crc >> s) & 0xFF for s in (24, 16, 8, 0)], dtype=np.uint8)])
        coded = np.unpackbits(orc.header_fec_encode(orc.header_format(plen), gen).ravel())
        bits = orc.AdditiveScrambler(0x4001, 0x18E38, 16).process(np.concatenate([coded, np.unpackbits(body)]))
        q = ((1 - 2.0 * bits[0::2]) * a + 1j * (1 - 2.0 * bits[1::2]) * a).astype(np.complex64)
        syms += [np.zeros(gap, np.complex64), sig.BPSK[sig.SYNCWORD], q]
        user.append(data)
    syms.append(np.zeros(1500, np.complex64))
    x = orc.interpolating_fir(np.concatenate(syms), 4, rrc)
    x = (orc.rotator(x, np.float32(0.007)) * np.exp(-1j * 0.9) + sig.awgn(x.size, 0.05, 502)).astype(np.complex64)
    rx = pkg.PacketReceiver(max_items=x.size, decode_headers=True)
    xd = dev(x)
    results = []
    if mode == "one_call":
        results.append(rx.process_bulk(xd))
    else:
        pos = 0
        for want in [7 * 1752 + 296, 30 * 1752 + 296, x.size]:   # cuts land inside payloads
            r = rx.process_bulk(xd[pos:min(pos + want, x.size)])
            results.append(r)
            pos += r["consumed"]
    out = np.concatenate([r["packets"].cpu().numpy() for r in results])
    out_len = np.concatenate([r["packet_lengths"] for r in results])
    assert [int(v) for v in out_len] == [0 if k == 4 else n for k, n in enumerate(lengths)]
    assert np.array_equal(out, np.concatenate([u for k, u in enumerate(user) if k != 4]))


def test_packet_receiver_file_app(pkg, tmp_path):
    """apps/packet_receiver_file.py (the reference's apps/packet_receiver_file.cpp): a raw complex64 IQ
    file in, the transmitted packets out, streamed in chunks that cut packets anywhere"""
    import importlib.util
    import zlib
    spec = importlib.util.spec_from_file_location("packet_receiver_file",
                                                  os.path.join(os.path.dirname(GOLDEN), "..", "apps", "packet_receiver_file.py"))
    app = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(app)
    rng = np.random.default_rng(601)
    lengths = [int(v) for v in rng.integers(1, 600, 40)]
    gaps = [int(g) for g in rng.integers(250, 700, len(lengths))]
    gen = np.load(os.path.join(GOLDEN, "header_ldpc_generator.npy"))
    a = np.float32(np.sqrt(0.5))
    rrc, _ = orc.unit_norm_rrc(4)
    syms, user = [], []
    for plen, gap in zip(lengths, gaps):
        data = rng.integers(0, 256, plen).astype(np.uint8)
        crc = zlib.crc32(data.tobytes())
        body = np.concatenate([data, np.array([(crc >> s) & 0xFF for s in (24, 16, 8, 0)], dtype=np.uint8)])
        coded = np.unpackbits(orc.header_fec_encode(orc.header_format(plen), gen).ravel())
        bits = orc.AdditiveScrambler(0x4001, 0x18E38, 16).process(np.concatenate([coded, np.unpackbits(body)]))
        q = ((1 - 2.0 * bits[0::2]) * a + 1j * (1 - 2.0 * bits[1::2]) * a).astype(np.complex64)
        syms += [np.zeros(gap, np.complex64), sig.BPSK[sig.SYNCWORD], q]
        user.append(data.tobytes())
    syms.append(np.zeros(2500, np.complex64))
    x = orc.interpolating_fir(np.concatenate(syms), 4, rrc)
    x = (orc.rotator(x, np.float32(-0.004)) + sig.awgn(x.size, 0.05, 602)).astype(np.complex64)
    path = tmp_path / "iq.c64"
    x.astype("<c8").tofile(path)                      # raw interleaved float32 I/Q, file_source.hpp:53
    out = tmp_path / "packets.bin"
    r = app.receive_file(str(path), chunk_items=50000, out=str(out), pkg=pkg)
    assert r["packets"] == user and r["crc_failures"] == 0 and r["invalid_headers"] == 0
    assert r["items"] > x.size - 4096
    blob = out.read_bytes()
    pos, got = 0, []
    while pos < len(blob):
        n = int.from_bytes(blob[pos:pos + 2], "big")
        got.append(blob[pos + 2:pos + 2 + n])
        pos += 2 + n
    assert got == user


@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("soft_bits", [False, True])
def test_native_packet_receiver_equals_python_composition(pkg, pipelined, soft_bits):
    """gr4pm_packet_receiver (the chain composed and pipelined inside the C++ library) gives exactly what
    the block-by-block composition in blocks.py gives: symbols, LLRs and every tag, over several batches
    of a device ring with look-ahead"""
    rng = np.random.default_rng(700)
    H, n = 1537, 60000
    wins = []
    for seed in (1, 2, 3):
        x, _, _ = _tx_packets(np.random.default_rng(seed), [120, 120, 120, 120], [300, 500, 420, 610])
        x = np.concatenate([x, np.zeros(n, np.complex64)])[:n]
        wins.append((x + sig.awgn(n, 0.05, 710 + seed)).astype(np.complex64))
    ring = torch.zeros(2 + H + 3 * n, dtype=torch.complex64, device="cuda")
    for k, w in enumerate(wins):
        ring[2 + H + k * n:2 + H + (k + 1) * n] = dev(w)
    ref = pkg.PacketReceiver(max_items=n, pipelined=False, soft_bits=soft_bits)
    nat = pkg.NativePacketReceiver(max_items=n, pipelined=pipelined, soft_bits=soft_bits)
    want, got = [], []
    for k in range(3):
        lo = 2 + H + k * n
        w, hist = ring[lo:lo + n], ring[lo - H:lo]
        nxt = ring[lo + n:lo + 2 * n] if k < 2 else None
        want.append(ref.process_bulk(w, 120, history=hist, next_x=nxt))
        r = nat.process_bulk(w, 120, history=hist, next_x=nxt)
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
    assert sum(r["tags"].size for r in got) >= 8
    assert np.array_equal(pkg.SYNCWORD, np.unpackbits(np.frombuffer(bytes.fromhex("034776C7272895B0"), dtype=np.uint8)))


def test_native_packet_receiver_symbol_pdu_tap(pkg):
    """packet_receiver.hpp:159-189 (zmq_output): SyncwordRemove's symbols -> HeaderPayloadSplit<c64>{128,
    "payload_symbols"} -> TaggedStreamToPdu -> PUB sinks.  The receiver lists the PDUs of every batch and, with a
    callback, delivers each complete one on the host.  Checked three ways: (1) against header_payload_split.hpp:46-135
    restated here over the packet tags (state carried across batches), (2) against the LLRs of the same symbols
    (constellation_llr_decoder.hpp: QPSK LLR pair = scale * (re, im)), (3) callback deliveries = the listed PDUs,
    PDUs that cross a batch boundary included."""
    H, n = 1537, 40000
    payload_len = 120
    x, _, _ = _tx_packets(np.random.default_rng(5), [payload_len] * 9, [300, 500, 420, 610, 350, 800, 333, 450, 700])
    x = np.concatenate([x, np.zeros(3 * n, np.complex64)])[: 3 * n]
    x = (x + sig.awgn(x.size, 0.05, 9)).astype(np.complex64)
    ring = torch.zeros(2 + H + 3 * n, dtype=torch.complex64, device="cuda")
    ring[2 + H:] = dev(x)
    nat = pkg.NativePacketReceiver(max_items=n, pipelined=True, soft_bits=True)
    delivered = []
    nat.set_symbol_pdu_callback(lambda kind, sym: delivered.append((kind, sym)))
    got = []
    for k in range(3):
        lo = 2 + H + k * n
        r = nat.process_bulk(ring[lo:lo + n], payload_len, history=ring[lo - H:lo])
        if r is not None:
            got.append(r)
    got += nat.flush()
    assert len(got) == 3
    # (1) the split restated: position counting, payload tag exactly at the end of a header
    in_payload, position, payload_items = False, 0, 0
    listed = []  # (kind, symbols) of complete PDUs, assembled from the per-batch pieces
    acc = {0: [], 1: []}
    n_hdr = n_pay = 0
    for r in got:
        sym = host(r["pdu_symbols"])
        llr = r["llr"].cpu().numpy()
        assert llr.size == 2 * sym.size
        scale = llr[0] / sym[0].real if sym.size else 1.0
        assert np.allclose(llr[0::2], scale * sym.real, rtol=1e-6) and np.allclose(llr[1::2], scale * sym.imag, rtol=1e-6)  # (2)
        tags = r["llr_tags"]  # same tags, at 2 LLRs per symbol
        pay_at = {int(t["index"]) // 2: int(t["payload_symbols"]) for t in tags if t["kind"] == 3}
        pieces, pos = [], 0
        while pos < sym.size:
            if pos in pay_at:
                assert not in_payload and position == 128
                in_payload, position, payload_items = True, 0, pay_at[pos]
            nxt = min([q for q in pay_at if q > pos] + [sym.size])
            if not in_payload and position == 128:
                position = 0
            want = (payload_items if in_payload else 128) - position
            m = min(nxt - pos, want)
            first = position == 0
            position += m
            last = position >= (payload_items if in_payload else 128)
            pieces.append((pos, m, 1 if in_payload else 0, first, last))
            pos += m
            if in_payload and position >= payload_items:
                in_payload, position = False, 0
        merged = []
        for pc in pieces:  # pieces of one PDU separated only by a tag
            if merged and merged[-1][2] == pc[2] and not merged[-1][4] and not pc[3] and merged[-1][0] + merged[-1][1] == pc[0]:
                merged[-1] = (merged[-1][0], merged[-1][1] + pc[1], pc[2], merged[-1][3], pc[4])
            else:
                merged.append(pc)
        pd = r["symbol_pdus"]
        assert [(int(p["offset"]), int(p["length"]), int(p["kind"]), bool(p["first"]), bool(p["last"])) for p in pd] == \
            [(a, b, c, bool(d), bool(e)) for a, b, c, d, e in merged]
        for p in pd:
            k = int(p["kind"])
            if p["first"]:
                acc[k] = []
            acc[k].append(sym[int(p["offset"]):int(p["offset"] + p["length"])])
            if p["last"]:
                listed.append((k, np.concatenate(acc[k])))
                n_hdr += k == 0
                n_pay += k == 1
    assert n_hdr >= 8 and n_pay >= 8
    assert all(s.size == 128 for k, s in listed if k == 0)
    assert all(s.size == (payload_len + 4) * 4 for k, s in listed if k == 1)   # payload + CRC-32, QPSK: 4 symbols per byte
    # (3) the callback saw exactly the complete PDUs, in order
    assert len(delivered) == len(listed)
    for (k1, s1), (k2, s2) in zip(delivered, listed):
        assert k1 == k2 and np.array_equal(bits(s1), bits(s2))
    nat.set_symbol_pdu_callback(None)
    with pytest.raises(pkg.Gr4pmError, match="soft_bits"):
        pkg.NativePacketReceiver(max_items=n).set_symbol_pdu_callback(lambda k, s: None)


def test_native_packet_receiver_publishes_symbol_pdus_on_zmq_pub_sockets(pkg):
    """SURVEY 8(f) rank 4, the wire format of the symbol tap: packet_receiver.hpp:163-168 binds two ZmqPduPubSink<c64>
    (tcp port 5000: header PDUs, 5001: payload PDUs), scripts/plot_symbols.py:10-17 subscribes and reads every message
    as complex64.  gr4pm_packet_receiver_publish_symbol_pdus does that on the library's own ZMTP 3.0 endpoints
    (ephemeral ports here): two SUB peers written on plain sockets (tests/test_zmq_pub.py) receive header PDUs of 128
    symbols and payload PDUs of `payload_symbols` symbols, bit for bit the PDUs the receiver lists in its result spans,
    PDUs that cross a batch boundary included."""
    from test_zmq_pub import RawSub, wait_for
    H, n = 1537, 40000
    payload_len = 120
    x, _, _ = _tx_packets(np.random.default_rng(5), [payload_len] * 9, [300, 500, 420, 610, 350, 800, 333, 450, 700])
    x = np.concatenate([x, np.zeros(3 * n, np.complex64)])[: 3 * n]
    x = (x + sig.awgn(x.size, 0.05, 9)).astype(np.complex64)
    ring = torch.zeros(2 + H + 3 * n, dtype=torch.complex64, device="cuda")
    ring[2 + H:] = dev(x)
    nat = pkg.NativePacketReceiver(max_items=n, pipelined=True, soft_bits=True)
    hdr_port, pay_port = nat.publish_symbol_pdus("tcp://127.0.0.1:*", "tcp://127.0.0.1:*")
    assert hdr_port > 0 and pay_port > 0 and hdr_port != pay_port
    subs = [RawSub(hdr_port), RawSub(pay_port)]
    time.sleep(0.2)  # (subscriptions are in before the first PDU: a PUB socket does not keep messages for late joiners)
    got = []
    for k in range(3):
        lo = 2 + H + k * n
        r = nat.process_bulk(ring[lo:lo + n], payload_len, history=ring[lo - H:lo])
        if r is not None:
            got.append(r)
    got += nat.flush()
    listed, acc = {0: [], 1: []}, {0: [], 1: []}
    for r in got:
        sym = host(r["pdu_symbols"])
        for p in r["symbol_pdus"]:
            k = int(p["kind"])
            if p["first"]:
                acc[k] = []
            acc[k].append(sym[int(p["offset"]):int(p["offset"] + p["length"])])
            if p["last"]:
                listed[k].append(np.concatenate(acc[k]))
    assert len(listed[0]) >= 8 and len(listed[1]) >= 8
    for kind in (0, 1):
        for want in listed[kind]:
            z = np.frombuffer(subs[kind].message(), "complex64")  # plot_symbols.py:17
            assert z.size == (128 if kind == 0 else (payload_len + 4) * 4)
            assert np.array_equal(bits(z), bits(want))
    nat.publish_symbol_pdus(None, None)  # the endpoints close: the peers see the end of their streams
    for s in subs:
        with pytest.raises((EOFError, ConnectionError)):
            s.message()
        s.close()
    with pytest.raises(pkg.Gr4pmError, match="soft_bits"):
        pkg.NativePacketReceiver(max_items=n).publish_symbol_pdus("tcp://127.0.0.1:*", "tcp://127.0.0.1:*")


@pytest.mark.parametrize("soft_bits", [False, True])
def test_native_packet_receiver_many_batches_pipelined_equals_sequential(pkg, soft_bits):
    """every stage of the pipelined receiver works on another batch at any moment (up to six in
    flight): twenty-four batches of different sizes, announced two ahead, give bit for bit what the same
    receiver gives batch by batch without the pipeline -- repeated, so that a buffer that two
    stages share by mistake shows up"""
    n_total = 24 * 70000
    x, _, _ = _tx_packets(np.random.default_rng(31), [200] * 130, list(np.random.default_rng(32).integers(300, 2500, 130)))
    x = np.concatenate([x, np.zeros(n_total, np.complex64)])[:n_total]
    xd = dev((x + sig.awgn(n_total, 0.05, 33)).astype(np.complex64))
    rng = np.random.default_rng(34)
    chunks, pos = [], 0
    while pos + 40000 <= n_total:
        take = int(rng.integers(20000, 70000))
        take = min(take, n_total - pos)
        chunks.append(xd[pos:pos + take])
        pos += ((take - 2048) // 1752 + 1) * 1752
    assert len(chunks) >= 24

    def run(pipelined):
        rx = pkg.NativePacketReceiver(max_items=70000, pipelined=pipelined, soft_bits=soft_bits)
        out, announced = [], 0
        for k, c in enumerate(chunks):
            while pipelined and announced < min(k + 2, len(chunks) - 1):
                announced += 1
                rx.announce(chunks[announced])
            r = rx.process_bulk(c, 200)
            if r is not None:
                out.append(r)
        return out + rx.flush()

    want = run(False)
    assert sum(r["tags"].size for r in want) >= 100
    for _ in range(3):
        got = run(True)
        assert len(got) == len(want)
        for a, b in zip(want, got):
            assert a["consumed"] == b["consumed"] and same_tags(a["tags"], b["tags"])
            assert np.array_equal(bits(host(a["symbols"])), bits(host(b["symbols"])))
            if soft_bits:
                assert a["llr"].cpu().numpy().tobytes() == b["llr"].cpu().numpy().tobytes()


def test_native_packet_receiver_decode_many_batches_pipelined_equals_sequential(pkg):
    """the same for the complete receiver (decode_headers: pass A, gate, symbol filter, control
    blocks, header loop and payload tail are six stages on six threads): forty batches whose cuts
    land inside headers and payloads; header messages, packet bytes and CRC verdicts are those of
    the batch-by-batch run, and every transmitted packet comes back"""
    rng = np.random.default_rng(41)
    payloads = [rng.integers(0, 256, int(n)).astype(np.uint8).tobytes() for n in rng.integers(20, 600, 260)]
    gaps = rng.integers(800, 3000, len(payloads))
    x = pkg.BurstGenerator().stream(payloads, gaps, freq_error=-0.008, esn0_db=20.0, seed=42)
    n_total = x.numel()
    chunks, pos = [], 0
    while pos + 40000 <= n_total:
        take = min(int(rng.integers(30000, 90000)), n_total - pos)
        chunks.append(x[pos:pos + take])
        pos += ((take - 2048) // 1752 + 1) * 1752
    assert len(chunks) >= 30

    def run(pipelined):
        rx = pkg.NativePacketReceiver(max_items=90000, tags_cap=1024, pipelined=pipelined, decode_headers=True)
        out, announced = [], 0
        for k, c in enumerate(chunks):
            while pipelined and announced < min(k + 2, len(chunks) - 1):
                announced += 1
                rx.announce(chunks[announced])
            r = rx.process_bulk(c)
            if r is not None:
                out.append(r)
        return out + rx.flush()

    def packets(results):
        got = []
        for r in results:
            data, p = r["packets"].cpu().numpy(), 0
            for ln in r["packet_lengths"]:
                if ln > 0:
                    got.append(data[p:p + int(ln)].tobytes())
                    p += int(ln)
        return got

    want = run(False)
    assert sum(r["header_mismatches"] for r in want) == 0
    sent = [p for p in payloads][: len(packets(want))]
    assert len(sent) >= len(payloads) - 3 and packets(want) == sent
    for _ in range(3):
        got = run(True)
        assert len(got) == len(want)
        for a, b in zip(want, got):
            assert a["consumed"] == b["consumed"] and b["header_mismatches"] == 0
            assert np.array_equal(a["header_messages"], b["header_messages"])
            assert np.array_equal(a["packet_lengths"], b["packet_lengths"])
            assert np.array_equal(a["packets"].cpu().numpy(), b["packets"].cpu().numpy())


@pytest.mark.parametrize("decode", [False, True])
def test_phasor_chains_of_consecutive_batches_side_by_side(pkg, monkeypatch, decode):
    """round 6: the CoarseFrequencyCorrection chains of consecutive batches on the rotator's own streams (independent
    segments | the channels' last segments | the continuations of the carried phasor, a ring of state rows, three events a
    plan that the fused symbol filter waits for on ITS stream) against one chain kernel per batch on the stage's stream.
    GR4PM_ROT_ASYNC=1 forces the form the library otherwise chooses for chains of >= 2^17 items in a process with >= 8
    hardware queues; GR4PM_TEST_ROT_DELAY_US starts every chain kernel 2.5 ms late (its three kernels by different amounts),
    so that a consumer that does not wait, or a continuation that reads the state before the batch in front wrote it,
    gives different bits.  Thirty batches with cuts inside packets and gaps, batches without any packet in between
    (continuations that are their channel's last segment), pipelined and batch by batch, two receivers each"""
    rng = np.random.default_rng(61)
    payloads = [rng.integers(0, 256, int(n)).astype(np.uint8).tobytes() for n in rng.integers(20, 400, 220)]
    gaps = rng.integers(800, 3000, len(payloads))
    gaps[40] = 200000  # three batches in a row without a tag
    gaps[41] = 1
    x = pkg.BurstGenerator().stream(payloads, gaps, freq_error=0.011, esn0_db=20.0, seed=62)
    n_total = x.numel()
    chunks, pos = [], 0
    while pos + 40000 <= n_total:
        take = min(int(rng.integers(30000, 70000)), n_total - pos)
        chunks.append(x[pos:pos + take])
        pos += ((take - 2048) // 1752 + 1) * 1752
    assert len(chunks) >= 25

    def run(pipelined, side_by_side):
        monkeypatch.delenv("GR4PM_ROT_ASYNC", raising=False)
        monkeypatch.delenv("GR4PM_TEST_ROT_DELAY_US", raising=False)
        monkeypatch.setenv("GR4PM_ROT_SERIAL", "1")
        if side_by_side:
            monkeypatch.delenv("GR4PM_ROT_SERIAL")
            monkeypatch.setenv("GR4PM_ROT_ASYNC", "1")
            monkeypatch.setenv("GR4PM_TEST_ROT_DELAY_US", "2500")
        res = []
        for rep in range(2):
            rx = pkg.NativePacketReceiver(max_items=70000, tags_cap=1024, pipelined=pipelined, decode_headers=decode)
            out, announced = [], 0
            for k, c in enumerate(chunks):
                while pipelined and announced < min(k + 2, len(chunks) - 1):
                    announced += 1
                    rx.announce(chunks[announced])
                r = rx.process_bulk(c) if decode else rx.process_bulk(c, 100)
                if r is not None:
                    out.append(r)
            res.append(out + rx.flush())
            del rx
        return res

    want = run(False, False)
    assert sum(r["tags"].size for r in want[0]) >= 100
    for pipelined in (False, True):
        got = run(pipelined, True)
        for w_rep, g_rep in zip(want, got):
            assert len(w_rep) == len(g_rep)
            for a, b in zip(w_rep, g_rep):
                assert a["consumed"] == b["consumed"] and same_tags(a["tags"], b["tags"])
                if decode:
                    assert np.array_equal(a["packet_lengths"], b["packet_lengths"])
                    assert np.array_equal(a["packets"].cpu().numpy(), b["packets"].cpu().numpy())
                else:
                    assert np.array_equal(bits(host(a["symbols"])), bits(host(b["symbols"])))
    monkeypatch.delenv("GR4PM_ROT_ASYNC", raising=False)
    monkeypatch.delenv("GR4PM_TEST_ROT_DELAY_US", raising=False)


@pytest.mark.parametrize("pipelined", [False, True])
def test_native_packet_receiver_packets_only_equals_the_full_form(pkg, pipelined):
    """round 6: gr4pm_packet_receiver_params::packets_only -- SyncwordRemove, the LLR decoder, the descrambler,
    HeaderPayloadSplit, the slicer and the packer as host state machines + ONE kernel over the Costas loop's output
    (hostlogic/tail_plan.hpp, k_tail_fused) -- against the full form, which runs the blocks one by one and materialises
    every stream between them: 300 packets of 1 .. 1500 bytes (their payloads end at every phase of the packer's bytes
    and of the four-symbol groups), damaged headers and damaged CRCs among them, cut into batches of ragged sizes so that
    headers and payloads cross batch boundaries at every symbol phase.  Batch by batch: consumed items, every tag list,
    header messages, packet types, the counts of the streams that are no longer written, packet lengths and packet bytes
    are identical; every undamaged packet comes back."""
    rng = np.random.default_rng(61)
    lengths = [int(v) for v in rng.integers(1, 700, 290)] + [1500, 1499, 1, 2, 3, 4, 5, 6, 7, 8]
    payloads = [rng.integers(0, 256, n).astype(np.uint8).tobytes() for n in lengths]
    gaps = rng.integers(300, 2500, len(payloads))
    x = pkg.BurstGenerator().stream(payloads, gaps, freq_error=0.006, esn0_db=18.0, seed=62)
    # damage: a burst of strong noise over some headers (invalid_header) and inside some payloads (CRC failure)
    n_total = x.numel()
    hit = torch.zeros(n_total, dtype=torch.complex64, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(63)
    for _ in range(25):
        at = int(rng.integers(0, n_total - 400))
        hit[at:at + 300] = torch.complex(torch.randn(300, generator=g, device="cuda"), torch.randn(300, generator=g, device="cuda")) * 2.0
    x = (x + hit).contiguous()
    chunks, pos = [], 0
    while pos + 12000 <= n_total:
        take = min(int(rng.integers(9000, 70000)), n_total - pos)
        chunks.append(x[pos:pos + take])
        pos += ((take - 2048) // 1752 + 1) * 1752
    assert len(chunks) >= 40

    def run(packets_only):
        rx = pkg.NativePacketReceiver(max_items=70000, tags_cap=1024, pipelined=pipelined, decode_headers=True,
                                      packets_only=packets_only)
        out, announced = [], 0
        for k, c in enumerate(chunks):
            while pipelined and announced < min(k + 2, len(chunks) - 1):
                announced += 1
                rx.announce(chunks[announced])
            r = rx.process_bulk(c)
            if r is not None:
                out.append(r)
        return out + rx.flush()

    full, lean = run(False), run(True)
    assert len(full) == len(lean) == len(chunks)
    n_ok = n_bad_hdr = n_bad_crc = 0
    for a, b in zip(full, lean):
        assert a["consumed"] == b["consumed"] and a["header_mismatches"] == b["header_mismatches"]
        assert np.array_equal(bits(host(a["symbols"])), bits(host(b["symbols"])))
        for key in ("tags", "detector_tags", "packet_tags", "llr_tags", "payload_tags"):
            assert _same_records(a[key], b[key]), key
        assert _same_records(a["header_messages"], b["header_messages"]) and np.array_equal(a["packet_type"], b["packet_type"])
        assert a["llr"].numel() == b["n_llr"] and a["payload_llr"].numel() == b["n_payload_llr"]
        assert b["llr"] is None and b["payload_llr"] is None and b["pdu_symbols"] is None and b["symbol_pdus"].size == 0
        assert np.array_equal(a["packet_lengths"], b["packet_lengths"])
        assert np.array_equal(a["packets"].cpu().numpy(), b["packets"].cpu().numpy())
        n_ok += int(np.sum(b["packet_lengths"] > 0))
        n_bad_crc += int(np.sum(b["packet_lengths"] == 0))
        n_bad_hdr += int(np.sum(b["header_messages"]["invalid_header"] != 0))
    assert n_ok >= len(payloads) - 40 and n_bad_crc >= 3 and n_bad_hdr >= 1, (n_ok, n_bad_crc, n_bad_hdr)
    got = b"".join(r["packets"].cpu().numpy().tobytes() for r in lean)
    sent_ok = [p for p in payloads if p in got]
    assert len(sent_ok) >= n_ok - 5  # (one-byte payloads can also match by accident; the bit-for-bit check is above)
    with pytest.raises(pkg.Gr4pmError, match="packets_only"):
        pkg.NativePacketReceiver(max_items=70000, soft_bits=True, packets_only=True)
    with pytest.raises(pkg.Gr4pmError, match="packets_only"):
        pkg.NativePacketReceiver(max_items=70000, decode_headers=True, packets_only=True).set_symbol_pdu_callback(lambda k, s: None)


@pytest.mark.parametrize("packets_only", [False, True])
def test_native_packet_receiver_goes_on_after_a_batch_whose_packets_did_not_fit(pkg, packets_only):
    """a batch that fails in the payload tail (here: the caller's packet buffer is too small for the
    batch's packets: GR4PM_INSUFFICIENT_OUTPUT_ITEMS) has popped packet lengths without consuming their bits; the stage
    lives on, and the next batch used to index the payload stream below zero (a wild device read).  Now the carried state
    starts empty again: the failed batch and the packet cut by its end are lost, every later batch delivers its packets,
    bit for bit those of a receiver that started behind the failed batch would deliver... here: every packet that lies
    wholly inside a later batch comes back, in both forms of the receiver."""
    rng = np.random.default_rng(71)
    payloads = [rng.integers(0, 256, 200).astype(np.uint8).tobytes() for _ in range(100)]
    # sparse | dense | sparse: two packets per batch, then eleven (2 244 bytes), then two again
    gaps = np.concatenate([np.full(20, 6000), np.full(40, 300), np.full(40, 6000)])
    x = pkg.BurstGenerator().stream(payloads, gaps, freq_error=0.004, esn0_db=20.0, seed=72)
    n = 60000
    chunks, pos = [], 0
    while pos + n <= x.numel():
        chunks.append(x[pos:pos + n])
        pos += ((n - 2048) // 1752 + 1) * 1752
    assert len(chunks) >= 8
    # a 1500-byte buffer holds a sparse batch's packets, not a dense one's
    rx = pkg.NativePacketReceiver(max_items=n, tags_cap=256, pipelined=True, decode_headers=True, packets_only=packets_only,
                                  packets_cap=1500)
    ok = pkg.NativePacketReceiver(max_items=n, tags_cap=256, pipelined=True, decode_headers=True, packets_only=packets_only)
    out, ref = [], []
    for c in chunks:
        for rcv, dst in ((rx, out), (ok, ref)):
            r = rcv.process_bulk(c)
            if r is not None:
                dst.append(r)
    out += rx.flush()
    ref += ok.flush()
    assert len(out) == len(ref) == len(chunks)
    failed = [i for i, r in enumerate(out) if r["status"] != 0]
    assert failed and failed[0] > 0 and failed[-1] < len(out) - 5 and all("packets_cap" in out[i]["error"] for i in failed), \
        [r["status"] for r in out]
    # every packet of `ok`: its start in the payload LLR stream (counted from the first batch) and its end
    starts, ends, pay_end = [], [], []
    for b in ref:
        P = pay_end[-1] if pay_end else 0
        starts += [P + int(t["index"]) for t in b["payload_tags"]]
        ends += [P + int(t["index"]) + int(t["payload_bits"]) for t in b["payload_tags"]]
        pay_end.append(P + b["n_payload_llr"])
    good_after = 0
    for i, (a, b) in enumerate(zip(out, ref)):
        if a["status"] != 0:
            continue
        assert a["consumed"] == b["consumed"]
        if i and out[i - 1]["status"] != 0:
            # the first batch behind a failed one: `ok`'s packets, less the one the end of the failed batch cut (which
            # started before that end and ends in this batch); all the others intact
            lost = sum(1 for s, e in zip(starts, ends) if s < pay_end[i - 1] < e <= pay_end[i])
            want_len = [int(v) for v in b["packet_lengths"]][lost:]
            assert [int(v) for v in a["packet_lengths"]] == want_len, (i, lost)
            skip = int(np.sum(b["packet_lengths"][:lost]))
            assert np.array_equal(a["packets"].cpu().numpy(), b["packets"].cpu().numpy()[skip:]), i
            assert a["packet_lengths"].size or not want_len
            continue
        assert np.array_equal(a["packet_lengths"], b["packet_lengths"])
        assert np.array_equal(a["packets"].cpu().numpy(), b["packets"].cpu().numpy())
        good_after += int(np.sum(a["packet_lengths"] > 0)) if i > failed[0] else 0
    assert good_after >= 10  # the receiver did go on delivering


@pytest.mark.parametrize("mode", ["one_call", "three_calls", "pipelined"])
def test_native_packet_receiver_decodes_headers_and_packets(pkg, mode):
    """gr4pm_packet_receiver with decode_headers: the whole receiver inside the C++ library, IQ samples
    in, CRC-checked packets out; same results as the host-layer composition"""
    import zlib
    rng = np.random.default_rng(801)
    lengths = [100, 17, 1500, 1, 333, 64, 900, 250, 40]
    gaps = [int(g) for g in rng.integers(250, 900, len(lengths))]
    gen = np.load(os.path.join(GOLDEN, "header_ldpc_generator.npy"))
    a = np.float32(np.sqrt(0.5))
    rrc, _ = orc.unit_norm_rrc(4)
    syms, user = [], []
    for k, (plen, gap) in enumerate(zip(lengths, gaps)):
        data = rng.integers(0, 256, plen).astype(np.uint8)
        crc = zlib.crc32(data.tobytes()) ^ (0x100 if k == 6 else 0)     # packet 6 arrives damaged
        body = np.concatenate([data, np.array([(crc >> s) & 0xFF for s in (24, 16, 8, 0)], dtype=np.uint8)])
        coded = np.unpackbits(orc.header_fec_encode(orc.header_format(plen, k % 2), gen).ravel())
        bits_ = orc.AdditiveScrambler(0x4001, 0x18E38, 16).process(np.concatenate([coded, np.unpackbits(body)]))
        q = ((1 - 2.0 * bits_[0::2]) * a + 1j * (1 - 2.0 * bits_[1::2]) * a).astype(np.complex64)
        syms += [np.zeros(gap, np.complex64), sig.BPSK[sig.SYNCWORD], q]
        user.append(data)
    syms.append(np.zeros(2000, np.complex64))
    x = orc.interpolating_fir(np.concatenate(syms), 4, rrc)
    x = (orc.rotator(x, np.float32(0.011)) * np.exp(1j * 0.4) + sig.awgn(x.size, 0.05, 802)).astype(np.complex64)
    xd = dev(x)
    ref = pkg.PacketReceiver(max_items=x.size, decode_headers=True)
    nat = pkg.NativePacketReceiver(max_items=x.size, pipelined=(mode == "pipelined"), decode_headers=True)
    cuts = [x.size] if mode != "three_calls" else [9 * 1752 + 296, 25 * 1752 + 296, x.size]
    want, got, pos = [], [], 0
    for c in cuts:
        piece = xd[pos:min(pos + c, x.size)]
        w = ref.process_bulk(piece)
        want.append(w)
        r = nat.process_bulk(piece)
        if r is not None:
            got.append(r)
        pos += w["consumed"]
        if pos + 4096 > x.size:
            break
    got += nat.flush()
    assert len(got) == len(want)
    for w, g in zip(want, got):
        assert w["consumed"] == g["consumed"] and g["header_mismatches"] == 0
        assert np.array_equal(bits(host(w["symbols"])), bits(host(g["symbols"])))
        assert w["llr"].cpu().numpy().tobytes() == g["llr"].cpu().numpy().tobytes()
        assert _same_records(w["header_messages"], g["header_messages"])
        assert np.array_equal(w["packet_type"], g["packet_type"])
        assert w["payload_llr"].cpu().numpy().tobytes() == g["payload_llr"].cpu().numpy().tobytes()
        assert np.array_equal(w["packet_lengths"], g["packet_lengths"])
        assert np.array_equal(w["packets"].cpu().numpy(), g["packets"].cpu().numpy())
    out = np.concatenate([g["packets"].cpu().numpy() for g in got])
    lens = np.concatenate([g["packet_lengths"] for g in got])
    assert [int(v) for v in lens] == [0 if k == 6 else n for k, n in enumerate(lengths)]
    assert np.array_equal(out, np.concatenate([u for k, u in enumerate(user) if k != 6]))
    msgs = np.concatenate([g["header_messages"] for g in got])
    assert [int(v) for v in msgs["packet_length"][msgs["invalid_header"] == 0]] == lengths


# ------------------------------------------------------------------ burst generator pieces
def test_mapper_and_burst_shaper_reference_qa(pkg):
    """test/qa_mapper.cpp:14-31 and test/qa_burst_shaper.cpp:15-90 through the C-ABI; the shaper also on
    complex items against a numpy restatement of burst_shaper.hpp:98-124"""
    mp = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8], dtype=np.float32)
    v = torch.arange(16, dtype=torch.uint8).cuda()
    assert np.array_equal(pkg.mapper(v, mp).cpu().numpy(), np.concatenate([mp, mp]))
    with pytest.raises(pkg.Gr4pmError):
        pkg.mapper(v, mp[:6])                                   # not a power of two, mapper.hpp:37-41
    lengths = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 100, 250, 1000, 10000, 100000, 7, 3, 25, 14, 28, 178]
    leading = np.array([0.1, 0.5, 0.9], dtype=np.float32)
    trailing = np.array([0.8, 0.2], dtype=np.float32)

    def shaped(x, n_lead, n_trail, lead, trail):
        y = x.copy()
        k = min(x.size, n_lead)
        y[:k] = x[:k] * lead[:k]
        rest = x.size - k
        t = min(rest, n_trail)
        if t:
            y[x.size - t:] = x[x.size - t:] * trail[n_trail - t:]
        return y

    ones = torch.ones(sum(lengths)).cuda()
    got = pkg.burst_shaper(ones, leading, trailing, lengths).cpu().numpy()
    pos = 0
    for n in lengths:
        pdu = got[pos:pos + n]
        assert np.array_equal(pdu[:3], leading[:n][:3])
        if n > 5:
            assert np.all(pdu[3:-2] == 1.0)
        if n > 3:
            t = min(n - 3, 2)
            assert np.array_equal(pdu[-t:], trailing[-t:])
        pos += n
    rng = np.random.default_rng(2)
    x = (rng.standard_normal(sum(lengths)) + 1j * rng.standard_normal(sum(lengths))).astype(np.complex64)
    lead = rng.random(32).astype(np.float32)
    trail = rng.random(44).astype(np.float32)
    got = pkg.burst_shaper(dev(x), lead, trail, lengths).cpu().numpy()
    want, pos = [], 0
    for n in lengths:
        want.append(shaped(x[pos:pos + n], 32, 44, lead, trail))
        pos += n
    assert np.array_equal(bits(got), bits(np.concatenate(want)))


def test_burst_generator_sfo_and_closed_form_carrier(pkg):
    """the channel model's remaining leg (apps/packet_transceiver.cpp:69-73): PfbArbResampler at 1 + 20 ppm in
    front of the carrier offset; and the generator-only closed-form carrier.  All packets come back through the
    native receiver, CRC-checked, either way."""
    rng = np.random.default_rng(31)
    gen = pkg.BurstGenerator()
    payloads = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(40, 300, 12)]
    gaps = rng.integers(3000, 6000, len(payloads))
    for kw in (dict(sfo_ppm=20.0), dict(carrier="closed_form"), dict(sfo_ppm=-15.0, carrier="closed_form")):
        x = gen.stream(payloads, gaps, freq_error=0.008, esn0_db=22.0, seed=7, **kw)
        rx = pkg.NativePacketReceiver(max_items=x.numel(), tags_cap=256, decode_headers=True)
        res = rx.process_bulk(x)
        lens, data = res["packet_lengths"], res["packets"].cpu().numpy()
        got, pos = [], 0
        for n in lens[lens > 0]:
            got.append(data[pos:pos + int(n)].tobytes())
            pos += int(n)
        assert got == payloads, kw
    # the closed-form carrier is the reference Rotator's signal up to rounding
    y = gen.stream(payloads[:2], gaps[:2], freq_error=0.008, seed=7)
    z = gen.stream(payloads[:2], gaps[:2], freq_error=0.008, seed=7, carrier="closed_form")
    assert float((y - z).abs().max()) < 2e-4


def test_burst_generator_loopback(pkg):
    """packet_transmitter_pdu.hpp's burst path and packet_transceiver.cpp's channel on the device, received
    by the native receiver: every packet comes back byte for byte at Es/N0 = 20 dB with carrier offset"""
    rng = np.random.default_rng(900)
    payloads = [rng.integers(0, 256, int(n)).astype(np.uint8).tobytes() for n in rng.integers(1, 1400, 30)]
    gaps = rng.integers(1200, 4000, len(payloads))
    gen = pkg.BurstGenerator()
    x = gen.stream(payloads, gaps, freq_error=0.012, esn0_db=20.0, seed=3)  # the payload is uncoded
    power = float(torch.mean(torch.abs(gen.bursts(payloads[:4])[0][200:-200]) ** 2))
    assert 0.25 < power < 0.40                                  # "tx_power = 0.32", packet_transceiver.cpp:48
    rx = pkg.NativePacketReceiver(max_items=x.numel(), tags_cap=1024, decode_headers=True)
    r = rx.process_bulk(x)
    lens = r["packet_lengths"]
    assert r["header_mismatches"] == 0 and int(np.sum(r["header_messages"]["invalid_header"] == 0)) >= len(payloads)
    data = r["packets"].cpu().numpy()
    got, pos = [], 0
    for n in lens[lens > 0]:
        got.append(data[pos:pos + int(n)].tobytes())
        pos += int(n)
    assert got == payloads


def test_tag_driven_costas_chains_in_the_32_register_form():
    """round 6: k_costas_chains_cap -- the PLL of the soft_bits / decode_headers receivers (tag-driven constellation and
    loop bandwidth, costas_loop.hpp:52-106) held to 32 VGPRs so that it starts beside a correlator workgroup -- gives the
    bits of the 121-register form: the chain test against the ORACLE (test_symbol_rate_chain_to_llrs: max |gpu - oracle|
    = 0) and the receivers' own comparisons, re-run in a process where every CostasLoop takes that form at every size
    (GR4PM_COSTAS_FORM=2, GR4PM_COSTAS_CAP_MIN_LOG2=0), then once more in the 71-register form"""
    import subprocess
    import sys
    for form in ("2", "1"):
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                            "test_symbol_rate_chain_to_llrs or test_packet_receiver_iq_to_packets or "
                            "test_native_packet_receiver_packets_only or test_native_packet_receiver_decodes_headers_and_packets"],
                           capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, GR4PM_COSTAS_FORM=form, GR4PM_COSTAS_CAP_MIN_LOG2="0"))
        assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("tool,cases,env", [("fuzz_detector.py", 8, {}), ("fuzz_cfc_symf.py", 6, {}), ("fuzz_costas.py", 9, {}),
                                            ("fuzz_costas.py", 9, {"GR4PM_COSTAS_FORM": "1"}),
                                            ("fuzz_costas.py", 12, {"GR4PM_COSTAS_FORM": "2", "GR4PM_COSTAS_CAP_MIN_LOG2": "0"}),
                                            ("fuzz_cfc_symf.py --sps 2", 6, {}), ("fuzz_cfc_symf.py --sps 3", 6, {}),
                                            ("fuzz_cfc_symf.py --sps 8", 6, {})])
def test_randomised_differential_tools(tool, cases, env):
    """a few cases of every randomised differential test under tools/ (random settings, tags, chunkings against the
    oracle; the long runs are quoted in HISTORY.md section 2).  GR4PM_COSTAS_FORM: the PLL kernel's 62-VGPR form and the
    32-VGPR form the pipelined receivers run -- the same bits.  --sps: the fused CFC + SymbolFilter at the receivers'
    design for 2, 3 and 8 samples per symbol (the generic kernel; the row without it runs k_symbol_filter_fast)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool, *options = tool.split()
    r = subprocess.run([sys.executable, os.path.join(root, "tools", tool), str(cases), "12345", *options], capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"{cases} of {cases} cases agree" in r.stdout



@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode", ["front_end", "decode_headers", "multichannel"])
def test_receivers_survive_allocation_failures(pkg, mode):
    """include/gr4pm_hip.h: "No exceptions cross the ABI".  The library's test-only allocator hook
    (gr4pm_test_fail_allocations) makes the k-th allocation of a whole receiver life -- create, a few pipelined
    batches, collect, destroy -- throw std::bad_alloc, for k swept over that life.  Whichever thread it strikes (the
    caller inside an entry point, or one of the receiver's stage threads): no exception, no std::terminate, no hang --
    the failure is an error status of the call or of the batch (Gr4pmError here), every batch in flight is still
    collected, and a receiver created afterwards gives the undisturbed result bit for bit.
    Runs on the TEST build of the library (libgr4pm_hip_test.so = the same objects + the hook)."""
    pkg = ge.load_test_build()
    L = pkg.lib()
    n = 60000
    x, _, _ = _tx_packets(np.random.default_rng(5), [200] * 12, list(np.random.default_rng(6).integers(300, 2000, 12)))
    x = np.concatenate([x, np.zeros(4 * n, np.complex64)])[:4 * n]
    x = (x + sig.awgn(x.size, 0.05, 7)).astype(np.complex64)
    if mode == "multichannel":
        xd = dev(np.stack([x, np.roll(x, 777)]))
        chunks = [xd[:, k * 58000:k * 58000 + n].contiguous() for k in range(3)]
    else:
        xd = dev(x)
        chunks = [xd[k * 58000:k * 58000 + n] for k in range(3)]

    def life(fail_after):
        errors, out = [], []
        if fail_after is not None:
            L.gr4pm_test_fail_allocations(fail_after, 1)
        try:
            if mode == "multichannel":
                rx = pkg.NativeMultiChannelReceiver(2, max_items=n, tags_cap=256)
            else:
                rx = pkg.NativePacketReceiver(max_items=n, tags_cap=256, pipelined=True,
                                              decode_headers=(mode == "decode_headers"))
        except pkg.Gr4pmError as e:
            L.gr4pm_test_fail_allocations(-1, 0)
            return [str(e)], []
        for c in chunks:
            try:
                if mode == "multichannel":
                    rx.submit(c, 200)
                else:
                    r = rx.process_bulk(c, None if mode == "decode_headers" else 200)
                    if r is not None:
                        out.append(r)
            except pkg.Gr4pmError as e:
                errors.append(str(e))
        while (rx.in_flight() if mode == "multichannel" else L.gr4pm_packet_receiver_inflight(rx._h)):
            try:
                out.append(rx.collect())
            except pkg.Gr4pmError as e:
                errors.append(str(e))
        del rx
        L.gr4pm_test_fail_allocations(-1, 0)
        return errors, out

    def key(results):
        if mode == "multichannel":
            return [tuple(host(d["symbols"]).tobytes() for d in r) for r in results]
        return [(r["consumed"], host(r["symbols"]).tobytes()) for r in results]

    c0 = L.gr4pm_test_allocation_count()
    errors, want = life(None)
    total = L.gr4pm_test_allocation_count() - c0
    assert not errors and total > 50, (errors, total)
    struck = 0
    for k in sorted(set(np.linspace(0, total - 1, 48).astype(int).tolist())):
        errors, _ = life(k)
        if errors:
            struck += 1
            assert any(("memory" in e) or ("bad_alloc" in e) or ("NOMEM" in e) or ("-4" in e) for e in errors), errors
    assert struck >= 24, struck  # most injected failures hit an allocation that matters and were reported

    # ... and EVERY allocation of the create call in turn (it designs filters through the library's own firdes entry
    # point, whose "0 taps" report of a failed allocation has to become GR4PM_ERR_NOMEM, not a bad filter length)
    def create():
        if mode == "multichannel":
            return pkg.NativeMultiChannelReceiver(2, max_items=n, tags_cap=256)
        return pkg.NativePacketReceiver(max_items=n, tags_cap=256, pipelined=True, decode_headers=(mode == "decode_headers"))

    c0 = L.gr4pm_test_allocation_count()
    rx = create()
    in_create = L.gr4pm_test_allocation_count() - c0
    del rx
    assert in_create > 20, in_create
    refused = 0
    for k in range(in_create):
        L.gr4pm_test_fail_allocations(k, 1)
        try:
            rx = create()
            del rx
        except pkg.Gr4pmError as e:
            refused += 1
            assert ("memory" in str(e)) or ("bad_alloc" in str(e)) or ("NOMEM" in str(e)) or ("-4" in str(e)), (k, str(e))
        finally:
            L.gr4pm_test_fail_allocations(-1, 0)
    assert refused >= in_create // 2, (refused, in_create)
    errors, again = life(None)
    assert not errors and key(again) == key(want)


def _alloc_case(pkg, name):
    """(create, run) of one block for test_block_creates_survive_allocation_failures: run(handle) = the bytes of one
    process_bulk on 1,024 items (the transmitter, whose input is packets: four of 64 bytes, its max_payload_bytes)"""
    rng = np.random.default_rng(11)
    x = dev((rng.standard_normal(1024) + 1j * rng.standard_normal(1024)).astype(np.complex64))
    if name == "InterpolatingFirFilter":
        taps = rng.standard_normal(33).astype(np.float32)
        return (lambda: pkg.InterpolatingFirFilter(4, taps)), (lambda h: host(h.process_bulk(x)).tobytes())
    if name == "PfbArbResampler":
        def run(h):
            y, consumed = h.process_bulk(x)
            return consumed, host(y).tobytes()
        return (lambda: pkg.PfbArbResampler(rate=1.25, filter_size=32)), run
    if name == "SyncwordWipeoff":
        bipolar = np.where(sig.SYNCWORD == 1, -1.0, 1.0).astype(np.float32)
        tags = np.zeros(3, dtype=pkg.TAG_DTYPE)
        tags["index"], tags["flags"] = [10, 500, 1000], pkg.TAG_SYNCWORD  # the last one runs past the call's end
        return (lambda: pkg.SyncwordWipeoff(bipolar)), (lambda h: host(h.process_bulk(x, tags)).tobytes())
    if name == "SyncwordDetectionFilter":
        def run(h):
            out = torch.zeros(1024, dtype=torch.complex64, device="cuda")
            r = h.process_bulk(x, out, pkg.TAG_SYNCWORD, headers=[100])
            return r, host(out).tobytes()
        return (lambda: pkg.SyncwordDetectionFilter()), run
    if name == "CrcCheck":
        def run(h):
            data = np.random.default_rng(12).integers(0, 256, 1024).astype(np.uint8)
            for k in (0, 2):  # two of the four packets carry their CRC-32, the others fail the check
                crc = h.compute(data[256 * k:256 * k + 252])
                data[256 * k + 252:256 * (k + 1)] = np.frombuffer(crc.to_bytes(4, "big"), np.uint8)
            out, out_len = h.process_bulk(dev(data), [256] * 4)
            return host(out).tobytes(), out_len.tobytes()
        return (lambda: pkg.CrcCheck()), run
    if name == "NoiseSource":
        return (lambda: pkg.NoiseSource(max_items=1 << 12)), (lambda h: host(h.process_bulk(1024)).tobytes())
    assert name == "PacketTransmitter"
    payloads = [rng.integers(0, 256, 64).astype(np.uint8).tobytes() for _ in range(4)]

    def run(h):
        y, offsets, lengths = h.process_bulk(payloads)
        return host(y).tobytes(), offsets.tobytes(), lengths.tobytes()
    return (lambda: pkg.PacketTransmitter(max_packets=8, max_payload_bytes=256)), run


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["InterpolatingFirFilter", "PfbArbResampler", "SyncwordWipeoff", "SyncwordDetectionFilter",
                                  "CrcCheck", "NoiseSource", "PacketTransmitter"])
def test_block_creates_survive_allocation_failures(pkg, name):
    """The create functions of the blocks that no receiver instantiates (test_receivers_survive_allocation_failures
    covers the others): every host allocation of one create call fails in turn (gr4pm_test_fail_allocations, TEST build
    of the library: its own operator new only, nothing happens on the device).  A create that fails raises Gr4pmError
    with the out-of-memory wording and hands no handle out; afterwards a handle created normally gives, on 1,024 items,
    the bytes of a handle created before."""
    pkg = ge.load_test_build()
    L = pkg.lib()
    create, run = _alloc_case(pkg, name)
    c0 = L.gr4pm_test_allocation_count()
    h = create()
    in_create = L.gr4pm_test_allocation_count() - c0
    want = run(h)
    del h
    assert in_create >= 1, in_create  # (the handle itself)
    refused = 0
    for k in range(in_create):
        L.gr4pm_test_fail_allocations(k, 1)
        try:
            h = create()
            del h
        except pkg.Gr4pmError as e:
            refused += 1
            assert ("memory" in str(e)) or ("bad_alloc" in str(e)) or ("NOMEM" in str(e)) or ("-4" in str(e)), (k, str(e))
        finally:
            L.gr4pm_test_fail_allocations(-1, 0)
    print(f"{name}: {in_create} allocations in create, {refused} refused")
    assert refused == in_create, (refused, in_create)  # (these creates have no allocation they can do without)
    assert run(create()) == want


@pytest.mark.gpu
def test_symbol_filter_output_span_runs_out(pkg):
    """symbol_filter.hpp:208: the loop stops as soon as the output span is full.  Found by the CPU sanitizer /
    differential build (tests/hostlogic): when the outputs of a call fitted the span EXACTLY the replay went on to
    consume the items behind the last output, and with a full span it still handled the tag of the next chunk (whose
    special cases :160-195 consume an item).  Symbols, re-timed tags and `consumed` against the oracle for every
    capacity around the exact fit, with a tag right behind the last output's item."""
    rrc, pfb = _receiver_pfb()
    rng = np.random.default_rng(77)
    n = 2003
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    for tag_at, te in [(None, 0.0), (1999, -0.3), (2000, 0.2), (2001, -0.4), (1997, 0.45)]:
        tags = np.zeros(0 if tag_at is None else 2, dtype=pkg.TAG_DTYPE)
        if tag_at is not None:
            tags["index"] = [500, tag_at]
            tags["amplitude"] = [1.5, 0.7]
            tags["time_est"] = [0.2, te]
            tags["flags"] = pkg.TAG_SYNCWORD
        otags = tags.astype(orc.TAG_DTYPE)
        full = orc.symbol_filter(x, pfb, 32, 4, 44, tags=otags)[0].size
        for cap in (full - 2, full - 1, full, full + 1):
            want, want_tags, want_cons = orc.symbol_filter(x, pfb, 32, 4, 44, tags=otags, out_cap=cap)
            f = pkg.SymbolFilter(pfb, 32, 4, 44)
            y, t, cons = f.process_bulk(dev(x), tags, out_cap=cap)
            assert cons == want_cons and y.numel() == want.size, (tag_at, cap, cons, want_cons)
            assert np.array_equal(bits(host(y)), bits(want))
            assert np.array_equal(t["index"], want_tags["index"])
            # the rest of the stream in a second call ends where one unlimited call ends
            if cons < n:
                rest = tags[tags["index"] >= cons].copy()
                rest["index"] -= cons
                y2, _, c2 = f.process_bulk(dev(x[cons:]), rest)
                whole = orc.symbol_filter(x, pfb, 32, 4, 44, tags=otags)[0]
                assert c2 == n - cons
                assert np.array_equal(bits(np.concatenate([host(y), host(y2)])), bits(whole))


@pytest.mark.gpu
def test_native_packet_receiver_decode_cut_just_behind_a_header(pkg):
    """decode_headers: a batch that ends 816 .. 848 items behind a syncword.  The real chain has then produced the
    packet's 192 syncword + header symbols, while pass A -- whose window needs 848 items behind the tag -- delivers the
    header message only with the next batch: PayloadMetadataInsert waits at the payload's first symbol
    (payload_metadata_insert.hpp:243-247) and the stage carries the symbols it could not take to the front of the next
    batch.  Round 3 failed such a batch ("PayloadMetadataInsert stalled ...": about one random cut in 200; found by
    tools/stress_receiver.py in round 4).  Every cut over a range that covers the band: the packets of the two-batch run
    are those of one call."""
    rng = np.random.default_rng(77)
    payloads = [rng.integers(0, 256, int(n)).astype(np.uint8).tobytes() for n in (300, 257, 411, 120)]
    x = pkg.BurstGenerator().stream(payloads, [3000, 2500, 2000, 2200], freq_error=0.006, esn0_db=20.0, seed=78)
    x = torch.cat([x, torch.zeros(8000, dtype=x.dtype, device=x.device)])

    def packets(results):
        got = []
        for r in results:
            data, p = r["packets"].cpu().numpy(), 0
            for ln in r["packet_lengths"]:
                if ln > 0:
                    got.append(data[p:p + int(ln)].tobytes())
                    p += int(ln)
        return got

    one = pkg.NativePacketReceiver(max_items=x.numel(), tags_cap=256, decode_headers=True)
    whole = one.process_bulk(x)
    assert packets([whole]) == payloads
    tag = int(whole["detector_tags"]["index"][1]) - 1537  # sample index of the second packet's syncword in the stream
    # The detector consumes whole strides of 1752 items, so the place where the first batch ends relative to the tag is
    # moved by shifting the STREAM: `behind` = items of the delayed stream (what the chain behind the detector sees)
    # that the first batch holds past the tag; the shifts cover 700 .. 700 + 1752, the band 816 .. 848 included.
    seen = []
    for shift in range(0, 1752, 8):
        xs = torch.cat([torch.zeros(shift, dtype=x.dtype, device=x.device), x])
        n_strides = (tag + shift + 1537 + 700 + 1751) // 1752
        first = 2048 + (n_strides - 1) * 1752
        rx = pkg.NativePacketReceiver(max_items=xs.numel(), tags_cap=256, decode_headers=True)
        a = rx.process_bulk(xs[:first])
        assert a["consumed"] == n_strides * 1752
        seen.append(a["consumed"] - (tag + shift + 1537))
        b = rx.process_bulk(xs[a["consumed"]:])
        assert packets([a, b]) == payloads, (shift, seen[-1])
        assert a["header_mismatches"] == 0 and b["header_mismatches"] == 0
    assert min(seen) <= 716 and max(seen) >= 2400 and any(816 <= v < 848 for v in seen)
    # the host-layer composition (blocks.py PacketReceiver) takes the same way through the band: bit for bit the native one
    for shift in [sh for sh, v in zip(range(0, 1752, 8), seen) if 812 <= v < 852]:
        xs = torch.cat([torch.zeros(shift, dtype=x.dtype, device=x.device), x])
        first = 2048 + ((tag + shift + 1537 + 700 + 1751) // 1752 - 1) * 1752
        nat = pkg.NativePacketReceiver(max_items=xs.numel(), tags_cap=256, decode_headers=True)
        ref = pkg.PacketReceiver(max_items=xs.numel(), decode_headers=True)
        pos = 0
        for piece_end in (first, xs.numel()):
            g = nat.process_bulk(xs[pos:piece_end])
            w = ref.process_bulk(xs[pos:piece_end])
            assert w["consumed"] == g["consumed"] and g["header_mismatches"] == 0 and w["header_mismatches"] == 0
            assert np.array_equal(bits(host(w["symbols"])), bits(host(g["symbols"])))
            assert w["llr"].cpu().numpy().tobytes() == g["llr"].cpu().numpy().tobytes()
            assert _same_records(w["header_messages"], g["header_messages"])
            assert np.array_equal(w["packet_lengths"], g["packet_lengths"])
            assert np.array_equal(w["packets"].cpu().numpy(), g["packets"].cpu().numpy())
            pos += g["consumed"]


_DESTROY_IN_FLIGHT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as ge
pkg = ge.load_package()
rng = np.random.default_rng(77)
payloads = [rng.integers(0, 256, int(n)).astype(np.uint8).tobytes() for n in (300, 257, 411, 120)]
x = pkg.BurstGenerator().stream(payloads, [3000, 2500, 2000, 2200], freq_error=0.006, esn0_db=20.0, seed=78)
x = torch.cat([x, torch.zeros(8000, dtype=x.dtype, device=x.device)])
one = pkg.NativePacketReceiver(max_items=x.numel(), tags_cap=256, decode_headers=True)
tag = int(one.process_bulk(x)["detector_tags"]["index"][1]) - 1537
del one
n = 0
for pipelined in (True, False):
    for shift in range(0, 1752, 24):
        xs = torch.cat([torch.zeros(shift, dtype=x.dtype, device=x.device), x])
        first = 2048 + ((tag + shift + 1537 + 700 + 1751) // 1752 - 1) * 1752
        rx = pkg.NativePacketReceiver(max_items=xs.numel(), tags_cap=256, decode_headers=True, pipelined=pipelined)
        rx.submit(xs[:first])
        rx.submit(xs[first - 296:])       # (whole strides of the first call: 2048 + k 1752 -> consumed (k + 1) 1752)
        if pipelined and shift % 48 == 0:
            rx.submit(xs[first - 296:])   # a third batch queued behind them
        del rx                             # destroy with everything in flight, nothing collected
        n += 1
print("destroyed", n)
"""


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_native_packet_receiver_destroy_with_batches_in_flight():
    """gr4pm_packet_receiver_destroy with batches queued between the stage threads, decode_headers, and a pending header
    (a detection in the last ~850 items of the first batch: stage 1 of the second batch waits for stage 1b to be done
    with the first).  Round 4's destroy() stopped every stage queue at once: an idle stage 1b left, stage 1 waited for
    it for ever and join() never returned.  Now only the head of the chain is stopped and the end travels behind the
    queued batches.  Every cut over a detector stride, pipelined and not, in a child process (a hang is a timeout)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _DESTROY_IN_FLIGHT, root], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0 and "destroyed 146" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_bench_selfcheck_runs_on_one_gpu():
    """`bench.py --selfcheck` (what the N-rank launcher runs first, and what every rank of a torch.distributed.run job
    goes through before the timed regions): identities, the scatter shape, two batches through the native receiver,
    detections counted -- on one GPU here, so that the code every multi-GPU job starts with has run on hardware."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--selfcheck"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["selfcheck"] == "ok" and rec["ranks"] == 1 and rec["tags"] > 0 and len(rec["job"]["ranks"]) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("launcher", ["torch.distributed.run", "bench.py --gpus 2"])
def test_bench_two_ranks_share_the_gpu_through_the_whole_n_gt_1_path(launcher):
    """The N > 1 code of bench.py on hardware, as far as a one-GPU box allows: two ranks (started the way the driver
    starts them, and by bench.py's own launcher) that both take cuda:0 and talk over gloo
    (GR4PM_BENCH_SHARED_DEVICE_TEST=1) go through the self-check, the channel scatter, the barrier-bracketed timed
    regions with MAX / SUM aggregation and the configs[3] leg (64 channels per rank from rank 0's host ring), and
    rank 0 prints ONE line for two ranks.  RCCL itself is the one thing this cannot reach; the rates mean nothing
    (two processes share a GPU) and the line says so."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = ["--gpus", "2", "--steps", "3", "--warmup", "2", "--repeats", "2", "--items", str(1 << 24), "--no-cpu-baseline",
            "--full"]
    env = dict(os.environ, GR4PM_BENCH_SHARED_DEVICE_TEST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    if launcher == "torch.distributed.run":
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py")] + args
    else:
        cmd = [sys.executable, os.path.join(root, "bench.py")] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "weak" and "shared_device_test" in rec
    assert rec["job"]["world"] == 2 and [x["rank"] for x in rec["job"]["ranks"]] == [0, 1] and rec["job"]["backend"] == "gloo"
    # both ranks' samples are in the sum: 3 steps x 2 ranks x (whole strides of 2^24 items)
    per_step = ((1 << 24) - 2048) // 1752 * 1752 + 1752
    assert abs(rec["value"] * 1e6 * rec["ms_per_step"] * 1e-3 * 3 / (3 * 2 * per_step) - 1.0) < 0.01
    # round 5: every rank generates its own headline channel (seeded by the rank), the line carries every rank's own time
    assert "generated on each GPU" in rec["config"]["input"]
    assert len(rec["ms_per_step_per_rank"]) == 2 and max(rec["ms_per_step_per_rank"]) == pytest.approx(rec["ms_per_step"], rel=1e-3)
    c3 = rec["config3"]
    assert c3["value"] > 0 and "128 channels in all" in c3["workload"] and "per_gpu" in c3
    # ... and the host sample ring's scatter (the workload's one collective) its own time and rate
    assert c3["scatter"]["bytes_from_rank0"] == 8 * 64 * (1 << 22) and c3["scatter"]["gbs"] > 0 and len(c3["ms_per_step_per_rank"]) == 2


@pytest.mark.gpu
@pytest.mark.timeout(1500)
def test_bench_eight_ranks_share_the_gpu_with_the_config3_ring_shape():
    """the N = 8 job of BASELINE configs[3] as far as ONE GPU allows -- eight ranks started by
    torch.distributed.run, all on cuda:0, gloo instead of RCCL (GR4PM_BENCH_SHARED_DEVICE_TEST=1): rendezvous, eight
    identities, the self-check, the headline regions with MAX / SUM aggregation over eight ranks, then the configs[3] leg
    with the ring in its real SHAPE -- rank 0's host sample ring [8, 64, n] scattered as eight [64, n] slabs, 512 channels
    in all -- cut down in items only (n = 2^16 per channel instead of 2^22).  One line for eight ranks.  Then the same job
    where rank 0 is told it has too little host memory for the ring: every rank leaves with the budget's message and the
    launcher reports it, nobody hangs in the scatter."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n3 = 1 << 16
    args = ["--gpus", "8", "--steps", "2", "--warmup", "1", "--repeats", "1", "--items", str(1 << 22), "--no-cpu-baseline",
            "--config3-items", str(n3), "--full"]
    env = dict(os.environ, GR4PM_BENCH_SHARED_DEVICE_TEST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)

    def run(extra_env):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr",
               "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py")] + args
        return subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=dict(env, **extra_env), cwd=root)

    r = run({})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 8 and rec["scaling"] == "weak" and "shared_device_test" in rec
    assert rec["job"]["world"] == 8 and [x["rank"] for x in rec["job"]["ranks"]] == list(range(8))
    assert len(rec["ms_per_step_per_rank"]) == 8
    c3 = rec["config3"]
    assert "512 channels in all" in c3["workload"] and c3["value"] > 0 and len(c3["ms_per_step_per_rank"]) == 8
    assert c3["scatter"]["bytes_from_rank0"] == 7 * 8 * 64 * n3  # seven slabs leave rank 0
    # the ring at its real size would be 8 x 64 x 2^22 x 8 B = 17.2 GB of pinned host memory: refused, by every rank, when
    # rank 0 does not have it (here: told so)
    r = run({"GR4PM_BENCH_TEST_HOST_AVAILABLE": str(1 << 20)})
    assert r.returncode != 0 and "cannot hold the sample ring of 8 ranks" in r.stderr, r.stderr[-3000:]
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_bench_collectives_over_rccl_with_one_rank():
    """RCCL itself, as far as one GPU reaches: a one-rank "nccl" group (init_process_group with device_id and the
    bounded timeout, as bench.init_ranks makes it) carries every collective bench.py uses -- all_gather_object for the
    identities, broadcast_object_list for the scatter budget, scatter of float views of complex slabs [C, n],
    all_reduce MAX / SUM / MIN, barrier -- with bench.py's own helpers."""
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    code = """
import sys, torch
sys.path.insert(0, %r)
import bench
device = torch.device("cuda", 0)
torch.cuda.set_device(0)
dist = bench.init_ranks("nccl", 0)
assert dist.get_backend() == "nccl"
job = bench.rank_identities(dist, device, 1)
bench.check_distinct_devices(job, 1)
bench.scatter_budget(dist, 0, 1, 8 << 20, device, host_ring=True)
g = torch.Generator(device=device); g.manual_seed(3)
src = torch.view_as_complex(torch.randn((1, 4, 1 << 16, 2), device=device, generator=g))
x = bench.scatter_channels(dist, lambda: src, (4, 1 << 16), device, 0, 1)
assert torch.equal(torch.view_as_real(x), torch.view_as_real(src[0]))
dt, total = bench.aggregate(dist, 1.5, 7.0, device)
assert (dt, total) == (1.5, 7.0)
t = torch.tensor([3.0], dtype=torch.float64, device=device)
dist.all_reduce(t, op=dist.ReduceOp.MIN)
dist.barrier()
torch.cuda.synchronize()
dist.destroy_process_group()
print("rccl one-rank ok", job["backend"], job["ranks"][0]["name"])
""" % root
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0 and "rccl one-rank ok nccl" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
