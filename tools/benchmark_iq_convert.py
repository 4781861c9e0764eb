#!/usr/bin/env python3
"""Rate of the integer IQ converters (csrc/iq_format.hip) against a copy of the same bytes in the same process.

  tools/benchmark_iq_convert.py [--log2-items 28] [--iters 20]

For each of sc16, sc8 and cu8: one iq_unpack() and one iq_pack() call of 2^log2-items items per iteration, timed with
device events, the median over the iterations.  The yardstick is the one tools/benchmark_channelizer.py uses: torch's
device-to-device copy of as many bytes as the call reads plus writes (half of them read, half written), timed the same
way.  Prints one JSON line per call: Gsamples/s, TB/s and the share of the copy."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from benchmark_channelizer import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2-items", type=int, default=28)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    n = 1 << args.log2_items
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((n, 2), dtype=torch.float32, device="cuda", generator=g) * 0.3)
    y = torch.empty_like(x)
    clipped = torch.zeros(1, dtype=torch.int64, device="cuda")
    for fmt, item in (("sc16", 4), ("sc8", 2), ("cu8", 2)):
        total = (8 + item) * n  # bytes read plus written, either direction
        a = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
        b = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
        ms_copy = median_ms(lambda: b.copy_(a), args.iters, torch)
        del a, b
        v = pkg.iq_pack(x, fmt)
        calls = (("unpack", lambda: pkg.iq_unpack(v, out=y)), ("pack", lambda: pkg.iq_pack(x, fmt, out=v, clipped=clipped)))
        for name, fn in calls:
            ms = median_ms(fn, args.iters, torch)
            print(json.dumps({"tool": "benchmark_iq_convert", "call": name, "format": fmt, "items": n, "ms": round(ms, 4),
                              "gsamples_per_s": round(n / ms / 1e6, 2), "tb_per_s": round(total / ms / 1e9, 3),
                              "copy_ms": round(ms_copy, 4), "copy_tb_per_s": round(total / ms_copy / 1e9, 3),
                              "share_of_copy": round(ms_copy / ms, 3), "device": torch.cuda.get_device_name(0)}))
        del v


if __name__ == "__main__":
    main()
