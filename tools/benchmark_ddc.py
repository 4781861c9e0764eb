#!/usr/bin/env python3
"""Rate of the Ddc (csrc/ddc.hip) against a copy of the same bytes in the same process.

  tools/benchmark_ddc.py [--log2-items 28] [--iters 20] [--shape traffic|issue|both] [--format cf32|sc16|sc8|cu8]
                         [--rational | --interpolation I]

One process_bulk() call of 2^log2-items wideband samples per iteration, timed with device events; the median over the
iterations, in Gsamples/s of input.  One JSON line per shape:

  traffic  K = 1, D = 4, L = 48: 8 B read and 2 B written per input sample, 48 FMAs per sample.  The yardstick is torch's
           device-to-device copy that moves the same number of bytes (5 B read and 5 B written per sample), timed the
           same way; the aim is half the copy's rate.
  issue    K = 8, D = 16, L = 192: 4 K L / D = 384 FMAs per input sample; the ceiling is the vector peak of 157.3 TFLOPS
           = 78.6 T FMA/s (reached only with packed FMAs) over 384 = 204.8 Gsamples/s.  Also, for information, the
           grid-aligned setting (f_k = k / 16, the channelizer's taps) against Channelizer(16, select = 8 rows) on the
           same input.

--format sc16 | sc8 | cu8 adds the fused integer ingest of each shape (process_bulk on the integer tensor).

--rational (off by default; give --iters 10 for the median of 10 that DESIGN.md quotes) runs instead the rational Ddc beside the integer Ddc of the
same process, one JSON line per shape with time, Gsamples/s of input and T FMA/s of both:
  traffic  K = 1, I / D = 4 / 25, the default taps (L = 300, 75 per branch), beside K = 1, D = 4, L = 48
  issue    K = 8, I / D = 3 / 49, L = 588 (196 MACs per item and channel), beside K = 8, D = 16, L = 192
The two shapes are fixed; --shape picks one of them.  --interpolation I with any positive I is another spelling of
--rational: the shapes bring their own I."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FMA_PER_S = 157.3e12 / 2
SHAPES = {"traffic": dict(K=1, D=4, L=48), "issue": dict(K=8, D=16, L=192)}
RATIONAL_SHAPES = {"traffic": dict(K=1, I=4, D=25, L=300), "issue": dict(K=8, I=3, D=49, L=588)}
FREQS = [0.1234, -0.31, 0.02, 0.47, -0.05, 0.29, -0.44, 0.18]


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


def rational_legs(pkg, torch, args, x, n):
    """--rational: each rational shape beside the integer Ddc of the same process"""
    names = ["traffic", "issue"] if args.shape == "both" else [args.shape]
    for name in names:
        K, I, D, L = (RATIONAL_SHAPES[name][k] for k in "KIDL")
        Ki, Di, Li = (SHAPES[name][k] for k in "KDL")
        items = n * I // D
        d = pkg.Ddc(FREQS[:K], D, interpolation=I, taps=pkg.ddc_rational_taps(I, D, L // D), max_frames=items + I)
        # the calls continue one stream: a call makes floor or ceil of n I / D items, by the handle's position
        out = torch.empty((K, items + 1), dtype=torch.complex64, device="cuda")
        ms = median_ms(lambda: d.process_bulk(x, out=out), args.iters, torch)
        del d, out
        di = pkg.Ddc(FREQS[:Ki], Di, taps_per_phase=Li // Di, max_frames=n // Di)
        out = torch.empty((Ki, n // Di), dtype=torch.complex64, device="cuda")
        ms_i = median_ms(lambda: di.process_bulk(x, out=out), args.iters, torch)
        del di, out
        # real FMAs: four per complex MAC, ceil(L / I) MACs per item and channel (the integer Ddc: L)
        fma = 4.0 * K * -(-L // I) * items
        fma_i = 4.0 * Ki * Li * (n // Di)
        res = {"tool": "benchmark_ddc", "shape": name + "_rational", "channels": K, "interpolation": I, "decimation": D,
               "taps": L, "items": n, "ms": round(ms, 4), "gsamples_per_s": round(n / ms / 1e6, 2),
               "tfma_per_s": round(fma / ms / 1e9, 2),
               "integer": {"channels": Ki, "decimation": Di, "taps": Li, "ms": round(ms_i, 4),
                           "gsamples_per_s": round(n / ms_i / 1e6, 2), "tfma_per_s": round(fma_i / ms_i / 1e9, 2)},
               "fma_rate_against_integer": round((fma / ms) / (fma_i / ms_i), 3),
               "device": torch.cuda.get_device_name(0)}
        print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2-items", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shape", choices=["traffic", "issue", "both"], default="both")
    ap.add_argument("--format", choices=["cf32", "sc16", "sc8", "cu8"], default="cf32")
    ap.add_argument("--interpolation", type=int, default=0, metavar="I", help="any positive I: the same as --rational")
    ap.add_argument("--rational", action="store_true",
                    help="the rational Ddc's two shapes beside the integer Ddc instead (see above)")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    n = 1 << args.log2_items
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((n, 2), dtype=torch.float32, device="cuda", generator=g))
    if args.rational or args.interpolation > 0:
        return rational_legs(pkg, torch, args, x, n)
    xi = None
    if args.format != "cf32":
        xi = pkg.iq_pack(x, args.format, 0.25 * (32768.0 if args.format == "sc16" else 128.0))
    for name in (["traffic", "issue"] if args.shape == "both" else [args.shape]):
        K, D, L = (SHAPES[name][k] for k in "KDL")
        d = pkg.Ddc(FREQS[:K], D, taps_per_phase=L // D, max_frames=n // D)
        out = torch.empty((K, n // D), dtype=torch.complex64, device="cuda")
        ms = median_ms(lambda: d.process_bulk(x, out=out), args.iters, torch)
        gsps = n / ms / 1e6
        fma_per_sample = 4 * K * L // D
        res = {"tool": "benchmark_ddc", "shape": name, "channels": K, "decimation": D, "taps": L, "items": n,
               "ms": round(ms, 4), "gsamples_per_s": round(gsps, 2), "fma_per_sample": fma_per_sample,
               "tfma_per_s": round(gsps * fma_per_sample / 1e3, 2),
               "fma_ceiling_gsamples_per_s": round(PEAK_FMA_PER_S / fma_per_sample / 1e9, 1),
               "share_of_fma_ceiling": round(gsps * 1e9 * fma_per_sample / PEAK_FMA_PER_S, 3)}
        # the copy that moves as many bytes as the call: (8 + 8 K / D) n in all, half of them read, half written
        nbytes = (8 * n + 8 * K * (n // D)) // 2
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        ms_copy = median_ms(lambda: dst.copy_(src), args.iters, torch)
        res.update({"bytes_per_sample": 8 + 8 * K / D, "copy_ms": round(ms_copy, 4),
                    "copy_tb_per_s": round(2 * nbytes / ms_copy / 1e9, 3), "tb_per_s": round((8 + 8 * K / D) * gsps / 1e3, 3),
                    "share_of_copy": round(ms_copy / ms, 3)})
        del src, dst
        if xi is not None:
            ms_fused = median_ms(lambda: d.process_bulk(xi, out=out), args.iters, torch)
            res.update({"format": args.format, "fused_ms": round(ms_fused, 4),
                        "fused_gsamples_per_s": round(n / ms_fused / 1e6, 2)})
        if name == "issue":  # on the channelizer's grid: the same rows two ways
            M = D
            h = pkg.channelizer_taps(M, L // M)
            da = pkg.Ddc([k / M for k in range(K)], M, taps=h, max_frames=n // M)
            ch = pkg.Channelizer(M, taps=h, select=list(range(K)), max_frames=n // M)
            ms_a = median_ms(lambda: da.process_bulk(x, out=out), args.iters, torch)
            ms_c = median_ms(lambda: ch.process_bulk(x, out=out), args.iters, torch)
            res.update({"grid_aligned_ms": round(ms_a, 4), "channelizer_select8_ms": round(ms_c, 4),
                        "channelizer_select8_gsamples_per_s": round(n / ms_c / 1e6, 2)})
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res))
        del d, out


if __name__ == "__main__":
    main()
