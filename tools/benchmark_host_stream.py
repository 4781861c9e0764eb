#!/usr/bin/env python3
"""The receiver fed from pinned host memory, with the upload in an integer IQ format.

  tools/benchmark_host_stream.py [--format cf32 sc16 sc8] [--log2-chunk 25] [--log2-total 29]

The scheme of bench.py's host_stream_leg: a pinned host ring of four chunks, every chunk copied to one of six device
slots on a copy stream two chunks ahead of the pipelined native receiver.  Here the ring and the slots hold the chosen
format (8, 4 or 2 bytes per sample) and an iq_unpack() into the receiver's complex64 slot sits between the copy and the
submit.  Per format one JSON line: Msamples/s through the receiver, the link-only figure (the same copies with nothing
behind them) and the copies with only the unpack behind them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg(bench, pkg, torch, device, rrc, fmt, chunk, host_chunks, total):
    n_slots = 6
    x, n_pkt = bench.burst_stream(pkg, chunk * host_chunks, rrc, seed=77, device=device)
    item = {"cf32": 8, "sc16": 4, "sc8": 2, "cu8": 2}[fmt]
    if fmt == "cf32":
        dev_src, shape, dtype = x, (chunk,), torch.complex64
    else:
        peak = float(torch.view_as_real(x).abs().max().item())
        gain = 0.5 * (32768.0 if fmt == "sc16" else 128.0) / peak
        dev_src = pkg.iq_pack(x, fmt, gain)
        shape, dtype = (chunk, 2), dev_src.dtype
    host = torch.empty((chunk * host_chunks,) + shape[1:], dtype=dtype).pin_memory()
    host.copy_(dev_src)
    del x, dev_src
    slots = [torch.empty(shape, dtype=dtype, device=device) for _ in range(n_slots)]
    work = slots if fmt == "cf32" else [torch.empty(chunk, dtype=torch.complex64, device=device) for _ in range(n_slots)]
    copy_stream = torch.cuda.Stream()
    events = [torch.cuda.Event() for _ in range(n_slots)]
    n_chunks = total // chunk

    def upload(i, unpack=True):
        src = host[(i % host_chunks) * chunk:(i % host_chunks + 1) * chunk]
        with torch.cuda.stream(copy_stream):
            slots[i % n_slots].copy_(src, non_blocking=True)
            if fmt != "cf32" and unpack:
                pkg.iq_unpack(slots[i % n_slots], 1.0 / gain, out=work[i % n_slots])
            events[i % n_slots].record(copy_stream)

    def timed_uploads(unpack):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n_chunks):
            upload(i, unpack)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    dt_link = timed_uploads(False)   # the link alone: the copies, nothing behind them
    dt_conv = timed_uploads(True)    # the copies with the unpack behind each (cf32: the copies again)
    rx = pkg.NativePacketReceiver(bench.SPS, bench.BINS, 9.5, "QPSK", max_items=chunk, tags_cap=max(64, 2 * n_pkt + 64),
                                  pipelined=True, output_ring=True)

    def run(n):
        done = tags = 0
        upload(0)
        upload(1)
        for i in range(n):
            if i + 2 < n:
                upload(i + 2)
            events[i % n_slots].synchronize()
            res = rx.process_bulk(work[i % n_slots], 1500)
            if res is not None:
                done += res["consumed"]
                tags += res["tags"].size
        for res in rx.flush():
            done += res["consumed"]
            tags += res["tags"].size
        return done, tags
    run(n_slots)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done, tags = run(n_chunks)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del rx
    return {"tool": "benchmark_host_stream", "format": fmt, "bytes_per_sample": item, "chunks": n_chunks, "chunk": chunk,
            "msamples_per_s": round(done / dt / 1e6, 2), "h2d_gbs": round(item * done / dt / 1e9, 2), "tags": tags,
            "link_only_msamples_per_s": round(n_chunks * chunk / dt_link / 1e6, 2),
            "link_only_h2d_gbs": round(item * n_chunks * chunk / dt_link / 1e9, 2),
            "copy_and_unpack_msamples_per_s": round(n_chunks * chunk / dt_conv / 1e6, 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--format", nargs="+", choices=["cf32", "sc16", "sc8", "cu8"], default=["cf32", "sc16", "sc8"])
    ap.add_argument("--log2-chunk", type=int, default=25)
    ap.add_argument("--log2-total", type=int, default=29)
    args = ap.parse_args()
    import torch
    import bench
    pkg = bench.ge.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    device = torch.device("cuda", 0)
    rrc = bench.unit_norm_rrc(pkg)
    for fmt in args.format:
        print(json.dumps(leg(bench, pkg, torch, device, rrc, fmt, 1 << args.log2_chunk, 4, 1 << args.log2_total)), flush=True)


if __name__ == "__main__":
    main()
