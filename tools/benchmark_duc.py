#!/usr/bin/env python3
"""Rate of the Duc (csrc/duc.hip) against a copy of the output's bytes and against the Ddc, in the same process.

  tools/benchmark_duc.py [--log2-items 28] [--iters 10] [--shape store|issue|both] [--rational] [--format sc16|sc8|cu8]

One process_bulk() call that makes 2^log2-items wideband samples per iteration, timed with device events; the median
over the iterations, in Gsamples/s of OUTPUT.  One JSON line per shape:

  store  K = 1, I = 4, L = 48: 2 B read and 8 B written per output sample, 48 FMAs per sample.  The yardstick is torch's
         device-to-device copy of 2^log2-items complex64 (the output's bytes), timed the same way; the aim is half the
         copy's rate.
  issue  K = 8, I = 16, L = 192: 4 K L / I = 384 FMAs per output sample; the ceiling is the vector peak of 157.3 TFLOPS
         = 78.6 T FMA/s over 384 = 204.8 Gsamples/s.  Also the Ddc's issue-bound shape (K = 8, D = 16, L = 192) on as
         many wideband samples: the same arithmetic per wideband sample.

--rational: the Duc that resamples by I / D (gr4pm_duc_create_rational) instead, each shape beside
the integer Duc at the same I, K and L in the same process (`integer_*` in the JSON line; both make 2^log2-items
samples per call):
  store  K = 1, 25 / 4, L = 300: 8 B written and 8 * 4 / 25 B read per output sample, 2 K P = 24 FMAs for the filter
         and 8 K for the rotator and the mix; against the copy of the output's bytes, as above.
  issue  K = 8, 16 / 3, L = 192: 2 K P + 8 K = 256 FMAs per output sample (the real-tap loop does half the FMAs per tap of
         k_duc, the rotator comes per output sample instead of per input item); against the vector FMA peak.

--format F: per shape also the integer output (gr4pm_duc_process_iq), three more figures from the same
process (tools/iq_out_timing.py): the fused call that writes F, the complex64 call again, and that call followed by
iq_pack()."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iq_out_timing import iq_out_figures  # noqa: E402

PEAK_FMA_PER_S = 157.3e12 / 2
SHAPES = {"store": dict(K=1, I=4, L=48), "issue": dict(K=8, I=16, L=192)}
RATIONAL_SHAPES = {"store": dict(K=1, I=25, D=4, L=300), "issue": dict(K=8, I=16, D=3, L=192)}
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2-items", type=int, default=28)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shape", choices=["store", "issue", "both"], default="both")
    ap.add_argument("--rational", action="store_true", help="the Duc resampling by I / D beside the integer Duc")
    ap.add_argument("--format", choices=["sc16", "sc8", "cu8"], help="also the integer output: fused, complex64, complex64 + iq_pack")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    n = 1 << args.log2_items
    g = torch.Generator(device="cuda").manual_seed(1)
    out = torch.empty(n, dtype=torch.complex64, device="cuda")
    for name in (["store", "issue"] if args.shape == "both" else [args.shape]) if args.rational else []:
        K, I, D, L = (RATIONAL_SHAPES[name][k] for k in "KIDL")
        P = L // I
        n_in = n * D // I  # a call makes floor or ceil of n_in I / D samples, by the handle's position: at most n
        v = torch.view_as_complex(torch.randn((K, n_in, 2), dtype=torch.float32, device="cuda", generator=g))
        d = pkg.Duc(FREQS[:K], I, decimation=D, taps_per_phase=P, max_items=n_in)
        made = n_in * I / D  # per call, on average
        ms = median_ms(lambda: d.process_bulk(v, out=out), args.iters, torch)
        gsps = made / ms / 1e6
        fma_per_sample = 2 * K * P + 8 * K
        nbytes = 8 + 8 * K * D / I
        res = {"tool": "benchmark_duc", "rational": True, "shape": name, "channels": K, "interpolation": I, "decimation": D,
               "taps": L, "items": round(made, 2), "ms": round(ms, 4), "gsamples_per_s": round(gsps, 2),
               "bytes_per_sample": round(nbytes, 3), "tb_per_s": round(nbytes * gsps / 1e3, 3),
               "fma_per_sample": fma_per_sample, "tfma_per_s": round(gsps * fma_per_sample / 1e3, 2),
               "fma_ceiling_gsamples_per_s": round(PEAK_FMA_PER_S / fma_per_sample / 1e9, 1),
               "share_of_fma_ceiling": round(gsps * 1e9 * fma_per_sample / PEAK_FMA_PER_S, 3)}
        if args.format:
            res.update(iq_out_figures(pkg, torch, median_ms, args.iters, args.format, n, lambda **kw: d.process_bulk(v, **kw)))
        del d, v
        # the integer Duc at the same I, K and L, as many output samples
        vi = torch.view_as_complex(torch.randn((K, n // I, 2), dtype=torch.float32, device="cuda", generator=g))
        di = pkg.Duc(FREQS[:K], I, taps_per_phase=P, max_items=n // I)
        ms_int = median_ms(lambda: di.process_bulk(vi, out=out), args.iters, torch)
        n_int = n // I * I
        res.update({"integer_ms": round(ms_int, 4), "integer_gsamples_per_s": round(n_int / ms_int / 1e6, 2),
                    "time_per_sample_over_integer": round((ms / made) / (ms_int / n_int), 3)})
        del di, vi
        if name == "store":  # the copy of the output's bytes
            src = torch.empty(n, dtype=torch.complex64, device="cuda")
            ms_copy = median_ms(lambda: out.copy_(src), args.iters, torch)
            res.update({"copy_ms": round(ms_copy, 4), "copy_tb_per_s": round(2 * 8 * n / ms_copy / 1e9, 3),
                        "share_of_copy": round((ms_copy / n) / (ms / made), 3)})
            del src
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res))
    for name in ([] if args.rational else ["store", "issue"] if args.shape == "both" else [args.shape]):
        K, I, L = (SHAPES[name][k] for k in "KIL")
        v = torch.view_as_complex(torch.randn((K, n // I, 2), dtype=torch.float32, device="cuda", generator=g))
        d = pkg.Duc(FREQS[:K], I, taps_per_phase=L // I, max_items=n // I)
        ms = median_ms(lambda: d.process_bulk(v, out=out), args.iters, torch)
        gsps = n / ms / 1e6
        fma_per_sample = 4 * K * L // I
        nbytes = 8 + 8 * K / I
        res = {"tool": "benchmark_duc", "shape": name, "channels": K, "interpolation": I, "taps": L, "items": n,
               "ms": round(ms, 4), "gsamples_per_s": round(gsps, 2), "bytes_per_sample": nbytes,
               "tb_per_s": round(nbytes * gsps / 1e3, 3), "fma_per_sample": fma_per_sample,
               "tfma_per_s": round(gsps * fma_per_sample / 1e3, 2),
               "fma_ceiling_gsamples_per_s": round(PEAK_FMA_PER_S / fma_per_sample / 1e9, 1),
               "share_of_fma_ceiling": round(gsps * 1e9 * fma_per_sample / PEAK_FMA_PER_S, 3)}
        if args.format:
            res.update(iq_out_figures(pkg, torch, median_ms, args.iters, args.format, n, lambda **kw: d.process_bulk(v, **kw)))
        if name == "store":  # the copy of the output's bytes
            src = torch.empty(n, dtype=torch.complex64, device="cuda")
            ms_copy = median_ms(lambda: out.copy_(src), args.iters, torch)
            res.update({"copy_ms": round(ms_copy, 4), "copy_tb_per_s": round(2 * 8 * n / ms_copy / 1e9, 3),
                        "share_of_copy": round(ms_copy / ms, 3)})
            del src
        else:  # the Ddc's issue-bound shape on the same number of wideband samples
            dd = pkg.Ddc(FREQS[:K], I, taps_per_phase=L // I, max_frames=n // I)
            x = out  # any wideband samples: the last call's
            y = torch.empty((K, n // I), dtype=torch.complex64, device="cuda")
            ms_ddc = median_ms(lambda: dd.process_bulk(x, out=y), args.iters, torch)
            res.update({"ddc_ms": round(ms_ddc, 4), "ddc_gsamples_per_s": round(n / ms_ddc / 1e6, 2),
                        "ddc_time_over_duc_time": round(ms_ddc / ms, 3)})
            del dd, y
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res))
        del d, v


if __name__ == "__main__":
    main()
