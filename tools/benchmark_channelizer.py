#!/usr/bin/env python3
"""Rate of the Channelizer (csrc/channelizer.hip) against a copy of the same bytes in the same process.

  tools/benchmark_channelizer.py [--channels 64] [--taps 12] [--log2-items 28] [--iters 20] [--form fast|generic]
                                 [--format cf32|sc16|sc8|cu8]

One process_bulk() call of 2^log2-items wideband samples per iteration, timed with device events; the median over the
iterations, in Gsamples/s of input.  The yardstick is torch's device-to-device copy of a tensor of the same size (8 B
read and 8 B written per sample, what the channelizer moves), timed the same way.  Prints one JSON line.  Asserts the
one floor that can be derived: real time for the README's operating point, 64 x 3.2 Msps = 0.2048 Gsamples/s.

--format sc16 | sc8 | cu8 (integer IQ in) prints a second JSON line with three figures side by side: the fused call
(process_bulk on the integer tensor), iq_unpack followed by process_bulk (two launches, the complex64 stream written and
read back in between), and process_bulk on samples that were unpacked beforehand."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REAL_TIME_GSPS = 64 * 3.2e6 / 1e9


def median_ms(fn, iters, torch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--taps", type=int, default=12, help="taps per branch")
    ap.add_argument("--log2-items", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--form", choices=["fast", "generic"], default="fast")
    ap.add_argument("--format", choices=["cf32", "sc16", "sc8", "cu8"], default="cf32")
    args = ap.parse_args()
    os.environ["GR4PM_CHANNELIZER"] = args.form
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    n = 1 << args.log2_items
    M = args.channels
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((n, 2), dtype=torch.float32, device="cuda", generator=g))
    ch = pkg.Channelizer(M, taps_per_branch=args.taps, max_frames=n // M)
    out = torch.empty((M, n // M), dtype=torch.complex64, device="cuda")
    ms = median_ms(lambda: ch.process_bulk(x, out=out), args.iters, torch)
    flat = out.reshape(-1)
    ms_copy = median_ms(lambda: flat.copy_(x), args.iters, torch)
    gsps, copy_gsps = n / ms / 1e6, n / ms_copy / 1e6
    res = {"tool": "benchmark_channelizer", "channels": M, "taps_per_branch": args.taps, "form": args.form,
           "items": n, "ms": round(ms, 4), "gsamples_per_s": round(gsps, 2), "copy_ms": round(ms_copy, 4),
           "copy_gsamples_per_s": round(copy_gsps, 2), "copy_tb_per_s": round(16 * copy_gsps / 1e3, 3),
           "share_of_copy": round(gsps / copy_gsps, 3), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    assert gsps > REAL_TIME_GSPS, f"{gsps} Gsamples/s is below real time for 64 x 3.2 Msps"
    if args.format != "cf32":
        xi = pkg.iq_pack(x, args.format, 0.25 * (32768.0 if args.format == "sc16" else 128.0))
        xc = torch.empty_like(x)
        ms_fused = median_ms(lambda: ch.process_bulk(xi, out=out), args.iters, torch)
        ms_two = median_ms(lambda: ch.process_bulk(pkg.iq_unpack(xi, out=xc), out=out), args.iters, torch)
        ms_pre = median_ms(lambda: ch.process_bulk(xc, out=out), args.iters, torch)
        print(json.dumps({"tool": "benchmark_channelizer", "format": args.format, "channels": M, "taps_per_branch": args.taps,
                          "form": args.form, "items": n,
                          "fused_ms": round(ms_fused, 4), "fused_gsamples_per_s": round(n / ms_fused / 1e6, 2),
                          "unpack_then_process_ms": round(ms_two, 4),
                          "unpack_then_process_gsamples_per_s": round(n / ms_two / 1e6, 2),
                          "complex64_ms": round(ms_pre, 4), "complex64_gsamples_per_s": round(n / ms_pre / 1e6, 2),
                          "fused_over_two_launches": round(ms_two / ms_fused, 3)}))


if __name__ == "__main__":
    main()
