"""NativePacketReceiver after a batch that failed in its payload tail (GR4PM_INSUFFICIENT_OUTPUT_ITEMS: the caller's packet
buffer, packets_cap, is too small for the batch's packets).  The header loop has already run over the whole failed batch,
so where that batch ends decides what the next one starts with: between two packets, inside a header, or inside a payload
with R of its LLRs still to come.  A sweep moves the end of the failed batch over a whole burst period and checks every
batch behind it against a receiver that never failed, and against the transmitter's own payloads.  Also: the output ring
covers every batch the library keeps in flight."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pytestmark = pytest.mark.gpu

N = 60000                                   # items per batch
STEP = ((N - 2048) // 1752 + 1) * 1752      # what the receiver consumes of each (the chunks overlap by N - STEP)
CAP = 1500                                  # packets_cap of the receiver that fails
HEADER_LLRS = 256                           # HeaderPayloadSplit's header_size
PKT_HEADER_START = 2                        # GR4PM_PKT_HEADER_START


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return ge.load_package()


def burst_len(n_bytes):
    return 4 * (4 * n_bytes + 228)          # PacketTransmitter, burst mode, sps 4


def layout(seed, long_last):
    """sparse lead-in (at most two short packets a batch) | a dense cluster (gaps of 300 samples, 100 .. 400 bytes; with
    long_last the cluster ends with a 9000-byte packet, longer than a batch) starting early in batch 3 | a sparse tail of
    more than six batches.  Every length is random, so that a misplaced slice cannot match by accident."""
    rng = np.random.default_rng(seed)
    lead = [int(v) for v in rng.integers(20, 80, 5)]
    cluster = [int(v) for v in rng.integers(100, 401, 9 if long_last else 14)] + ([9000] if long_last else [])
    tail = [int(v) for v in rng.integers(20, 80, 11)]
    gaps = [5000] + [31000] * (len(lead) - 1)
    end_of_lead = sum(gaps) + sum(burst_len(n) for n in lead)
    gaps += [3 * STEP + 1500 - end_of_lead] + [300] * (len(cluster) - 1) + [31000] * len(tail)
    payloads = [rng.integers(0, 256, n).astype(np.uint8).tobytes() for n in lead + cluster + tail]
    return payloads, gaps, range(len(lead), len(lead) + len(cluster))


def received_stream(pkg, clean, delta, seed):
    """delta zero samples, the bursts, three batches of silence; then a small frequency offset and AWGN at Es/N0 = 20 dB
    (as test_packet_transmitter.py's loopback)"""
    z = lambda k: torch.zeros(k, dtype=torch.complex64, device=clean.device)
    x = pkg.Rotator(np.float32(0.01)).process_bulk(torch.cat([z(delta), clean, z(3 * N)]))
    n0 = 0.32 * 4 * 10.0 ** (-0.1 * 20.0)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    noise = torch.complex(torch.randn(x.numel(), generator=g, device="cuda"),
                          torch.randn(x.numel(), generator=g, device="cuda")) * np.float32(np.sqrt(n0 / 2.0))
    return (x + noise).to(torch.complex64)


def on_host(r):
    """what the checks need of a result, copied at once (with output_ring the tensors are recycled)"""
    if r["status"] != 0:
        return {"status": r["status"], "error": r["error"], "consumed": r["consumed"]}
    return {"status": 0, "error": "", "consumed": r["consumed"], "lengths": [int(v) for v in r["packet_lengths"]],
            "packets": r["packets"].cpu().numpy().tobytes(), "n_llr": r["n_llr"], "llr_tags": r["llr_tags"],
            "n_pay": r["n_payload_llr"], "pay_tags": r["payload_tags"], "header_mismatches": r["header_mismatches"]}


def run_pair(pkg, x, packets_only, output_ring):
    """two pipelined decode_headers receivers on identical chunks: rx with packets_cap=CAP, ok without"""
    chunks = [x[p:p + N] for p in range(0, x.numel() - N + 1, STEP)]
    kw = dict(max_items=N, tags_cap=256, pipelined=True, decode_headers=True, packets_only=packets_only,
              output_ring=output_ring)
    rx = pkg.NativePacketReceiver(packets_cap=CAP, **kw)
    ok = pkg.NativePacketReceiver(**kw)
    out, ref = [], []
    for c in chunks:
        for rcv, dst in ((rx, out), (ok, ref)):
            r = rcv.process_bulk(c)
            if r is not None:
                dst.append(on_host(r))
    out += [on_host(r) for r in rx.flush()]
    ref += [on_host(r) for r in ok.flush()]
    assert len(out) == len(ref) == len(chunks)
    return out, ref


def packets_of(ref):
    """every packet of the undisturbed receiver: [start, payload bits, batch that delivered it], start in the payload LLR
    stream counted from the first batch; and per batch the end of its payload and LLR streams, and the header starts"""
    pk, pay_end, llr_end, hdr = [], [], [], []
    P = L = 0
    for i, b in enumerate(ref):
        assert b["status"] == 0 and b["header_mismatches"] == 0, (i, b["error"])
        pk += [[P + int(t["index"]), int(t["payload_bits"]), None] for t in b["pay_tags"]]
        hdr += [L + int(t["index"]) for t in b["llr_tags"] if t["kind"] == PKT_HEADER_START]
        P += b["n_pay"]
        L += b["n_llr"]
        pay_end.append(P)
        llr_end.append(L)
    for p in pk:
        p[2] = next(i for i, e in enumerate(pay_end) if p[0] + p[1] <= e)
    for i, b in enumerate(ref):  # the model matches what the receiver delivered
        assert len(b["lengths"]) == sum(p[2] == i for p in pk), i
    return pk, pay_end, llr_end, hdr


def check_recovery(payloads, cluster, out, ref):
    """the checks of one stream; returns (f, where the end of batch f fell, R)"""
    pk, pay_end, llr_end, hdr = packets_of(ref)
    assert len(pk) == len(payloads), "every header decodes at 20 dB"
    assert [p[1] for p in pk] == [8 * (len(b) + 4) for b in payloads]
    # where rx must fail: a batch whose packets -- those that started behind the end of the last failed batch -- need more
    # than CAP bytes (the packet cut by a failed batch is lost with it)
    want_failed, cut_at = [], None
    for i in range(len(ref)):
        need = sum(p[1] // 8 for p in pk if p[2] == i and (cut_at is None or p[0] >= cut_at))
        if need > CAP:
            want_failed.append(i)
            cut_at = pay_end[i]
    failed = [i for i, r in enumerate(out) if r["status"] != 0]
    assert failed == want_failed, (failed, want_failed, [r["error"] for r in out if r["status"]])
    assert failed and all("packets_cap" in out[i]["error"] for i in failed)
    assert all(any(pk[k][2] == i for k in cluster) for i in failed), "a batch failed that holds no packet of the cluster"
    f = failed[-1]
    P_f, L_f = pay_end[f], llr_end[f]
    cut = [k for k, p in enumerate(pk) if p[0] < P_f < p[0] + p[1]]
    R = pk[cut[0]][0] + pk[cut[0]][1] - P_f if cut else 0
    where = "payload" if R else ("header" if any(h < L_f < h + HEADER_LLRS for h in hdr) else "between packets")
    # batch by batch: the undisturbed receiver's packets, less those that started before the end of the last failed batch
    last_fail = None
    for i, (a, b) in enumerate(zip(out, ref)):
        assert a["consumed"] == b["consumed"], i
        if a["status"] != 0:
            last_fail = pay_end[i]
            continue
        drop = sum(1 for p in pk if p[2] == i and last_fail is not None and p[0] < last_fail)
        assert a["lengths"] == b["lengths"][drop:], (i, drop, a["lengths"], b["lengths"])
        assert a["packets"] == b["packets"][sum(b["lengths"][:drop]):], (i, drop)
        if i == f + 1 and len(b["lengths"]) > drop:
            assert a["lengths"], "the first batch behind the failure delivered nothing"
        assert a["header_mismatches"] == (0 if i > f else b["header_mismatches"]), i
    # and against the transmitter's input: every packet whose payload starts behind the end of batch f, byte for byte
    m0 = sum(1 for p in pk if p[0] < P_f)
    got = [out[i] for i in range(f + 1, len(out))]
    assert sum((r["lengths"] for r in got), []) == [len(p) for p in payloads[m0:]]
    assert b"".join(r["packets"] for r in got) == b"".join(payloads[m0:])
    return f, where, R, (pay_end[f + 1] - P_f)


def sweep(pkg, seed, long_last, deltas, packets_only, output_ring):
    payloads, gaps, cluster = layout(seed, long_last)
    clean, _, _ = pkg.PacketTransmitter(max_packets=len(payloads)).process_bulk(payloads, gaps=gaps)
    seen, wrong = [], []
    for d in deltas:
        x = received_stream(pkg, clean, d, 1000 + d)
        out, ref = run_pair(pkg, x, packets_only, output_ring)
        try:
            f, where, R, n_next = check_recovery(payloads, cluster, out, ref)
        except (AssertionError, pkg.Gr4pmError) as e:
            wrong.append(f"delta {d}: {str(e)[:300]}")
            continue
        seen.append((d, f, where, R, n_next))
        print(f"delta {d:5d}: last failed batch {f}, its end {where}, R = {R} (R mod 8 = {R % 8}), "
              f"next batch {n_next} payload LLRs")
    assert not wrong, "\n".join(wrong)
    return seen


@pytest.mark.parametrize("packets_only,output_ring", [(False, False), (True, False), (True, True)])
def test_the_packet_cut_by_a_failed_batch_does_not_shift_the_ones_behind_it(pkg, packets_only, output_ring):
    # 24 offsets 212 samples apart: one burst period of the cluster; 212 is 53 symbols, so the end of the failed batch
    # moves by one symbol modulo 4 = two LLRs modulo 8 from one offset to the next (16 samples: one payload byte)
    seen = sweep(pkg, 1, False, range(0, 24 * 212, 212), packets_only, output_ring)
    where = {s[2] for s in seen}
    r8 = {s[3] % 8 for s in seen if s[3] > 0}
    assert {"header", "between packets", "payload"} <= where and {0, 2, 4, 6} <= r8, (where, r8)


@pytest.mark.parametrize("packets_only", [False, True])
def test_a_cut_packet_longer_than_a_batch_is_skipped_over_several_batches(pkg, packets_only):
    # the cluster ends with a 9000-byte packet: the failed batch cuts it, and what is left of it fills the next batch and more
    seen = sweep(pkg, 1, True, range(0, 8 * 636, 636), packets_only, False)
    assert all(s[2] == "payload" and s[3] > s[4] for s in seen), seen
    assert {s[3] % 8 for s in seen} == {0, 2, 4, 6}, seen


def stream_of_batches(pkg, n_batches, seed):
    rng = np.random.default_rng(seed)
    payloads = [rng.integers(0, 256, int(n)).astype(np.uint8).tobytes() for n in rng.integers(50, 600, 12 * n_batches)]
    x, _, _ = pkg.PacketTransmitter(max_packets=len(payloads)).process_bulk(
        payloads, gaps=[int(g) for g in rng.integers(1500, 3000, len(payloads))])
    x = torch.cat([x, torch.zeros(N * (n_batches + 1), dtype=torch.complex64, device=x.device)])
    return [x[p:p + N] for p in range(0, STEP * n_batches, STEP)]


def same_bits(a, b):
    """bit for bit (a noise-free stimulus can leave NaN symbols, which torch.equal never calls equal)"""
    return a.numel() == b.numel() and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_output_ring_covers_every_batch_in_flight(pkg):
    """output_ring=True: with the library's maximum of batches in flight, no two of them share an output tensor"""
    M = int(pkg.lib().gr4pm_packet_receiver_max_inflight())
    assert M >= 1
    chunks = stream_of_batches(pkg, M, 5)
    results, keep = {}, []
    for ring in (True, False):
        rx = pkg.NativePacketReceiver(max_items=N, tags_cap=1024, pipelined=True, decode_headers=True, output_ring=ring)
        for c in chunks:
            rx.submit(c)
        assert pkg.lib().gr4pm_packet_receiver_inflight(rx._h) == M
        with pytest.raises(pkg.Gr4pmError):  # the library's limit: one more is refused
            rx.submit(chunks[0])
        results[ring] = [rx.collect() for _ in chunks]
        torch.cuda.synchronize()
        keep.append(rx)  # (the receiver, and with it the ring, stays alive until compared)
    n_packets = 0
    for i, (a, b) in enumerate(zip(results[True], results[False])):
        assert a["status"] == b["status"] == 0, i
        for key in ("symbols", "llr", "packets"):
            assert same_bits(a[key], b[key]), (i, key)
        n_packets += int(np.sum(b["packet_lengths"] > 0))
    assert n_packets >= 3 * M  # packets in every batch


def test_multichannel_output_ring_covers_every_batch_in_flight(pkg):
    """the same for NativeMultiChannelReceiver's ring of symbol buffers"""
    C = 2
    rows = [stream_of_batches(pkg, 6, 20 + c) for c in range(C)]
    results, keep = {}, []
    for ring in (True, False):
        rx = pkg.NativeMultiChannelReceiver(C, max_items=N, output_ring=ring)
        k = 0
        while True:
            x = torch.stack([rows[c][k] for c in range(C)])
            try:
                rx.submit(x)
            except pkg.Gr4pmError:  # the library's limit
                break
            k += 1
        assert k >= 2 and rx.in_flight() == k
        results[ring] = [rx.collect() for _ in range(k)]
        torch.cuda.synchronize()
        keep.append(rx)
    assert len(results[True]) == len(results[False])
    for i, (a, b) in enumerate(zip(results[True], results[False])):
        for c in range(C):
            assert a[c]["symbols"].numel() > 0 and same_bits(a[c]["symbols"], b[c]["symbols"]), (i, c)
