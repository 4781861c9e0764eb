#!/usr/bin/env python3
"""Rate of the Spectrum block (csrc/spectrum.hip) against a copy of the same bytes and the one-bin correlator, all in
the same process.

  tools/benchmark_spectrum.py [--log2-items 28] [--iters 20]

One process_bulk() call of 2^log2-items wideband samples per iteration, timed with device events; the median over the
iterations, in Gsamples/s of input, for hop 2048 and 1024 and for complex64 and sc16 input.  Beside each: torch's
device-to-device copy of the input's bytes (8 or 4 read and as many written per sample; the Spectrum only reads), and
SyncwordDetection.correlate_only with one frequency bin (two transforms per 1752 samples where the Spectrum runs one per
hop) on complex64 samples.  Prints one JSON line per (hop, format).  Expected from the code, not asserted: at hop 2048
the kernel is bound by reading 8 (sc16: 4) bytes per sample, at hop 1024 by vector issue at about twice the correlator's
rate per sample."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_channelizer import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2-items", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    import bench
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    n = 1 << args.log2_items
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((n, 2), dtype=torch.float32, device="cuda", generator=g))
    xi = pkg.iq_pack(x, "sc16", 0.125 * 32768.0)
    rrc = bench.unit_norm_rrc(pkg)
    sd = pkg.SyncwordDetection(rrc, bench.SYNCWORD, np.array([1, -1], dtype=np.complex64), 0, 0, power_threshold=9.5, max_items=n)
    ms_corr = median_ms(lambda: sd.correlate_only(x), args.iters, torch)
    copies = {}
    for name, src in (("cf32", x), ("sc16", xi)):
        dst = torch.empty_like(src)
        copies[name] = median_ms(lambda: dst.copy_(src), args.iters, torch)
        del dst
    for hop in (2048, 1024):
        sp = pkg.Spectrum(hop=hop)
        for name, src, item_bytes in (("cf32", x, 8), ("sc16", xi, 4)):
            ms = median_ms(lambda: sp.process_bulk(src), args.iters, torch)
            gsps = n / ms / 1e6
            print(json.dumps({"tool": "benchmark_spectrum", "hop": hop, "format": name, "items": n, "ms": round(ms, 4),
                              "gsamples_per_s": round(gsps, 2), "read_tb_per_s": round(item_bytes * gsps / 1e3, 3),
                              "copy_ms": round(copies[name], 4), "copy_gsamples_per_s": round(n / copies[name] / 1e6, 2),
                              "copy_tb_per_s": round(2 * item_bytes * n / copies[name] / 1e9, 3),
                              "one_bin_correlator_ms": round(ms_corr, 4),
                              "one_bin_correlator_gsamples_per_s": round(n / ms_corr / 1e6, 2),
                              "over_correlator": round(ms_corr / ms, 3), "device": torch.cuda.get_device_name(0)}))
        assert sp.read()["segments"] > 0


if __name__ == "__main__":
    main()
