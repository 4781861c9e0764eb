#!/usr/bin/env python3
"""gr4pm_noise_source throughput: NoiseSource<c64> Gaussian (or another item / type) at 2^k items per call, noise
alone and added in place into a signal (out = in + noise, the Add block fused in).

    benchmark_noise_source.py [--log2-items 20 24 28] [--item c64] [--type gaussian] [--iters 10] [--json out.json]

Every call is timed whole (the jump pre-pass, count, scan and write kernels) with device events, after two warm-up
calls of the same shape.  "of_store_ceiling" sets the bytes moved per item (8 written for c64 noise; 8 read + 8
written in place) against 6.0 TB/s."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

CEILING = 6.0e12  # bytes/s


def run(pkg, item, typ, n, add, iters):
    src = pkg.NoiseSource(typ, 0.05, 1, item, max_items=n)
    dt = torch.complex64 if item == "c64" else torch.float32
    out = torch.zeros(n, dtype=dt, device="cuda")
    for _ in range(2):
        src.process_bulk(n, add_to=out if add else None, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        src.process_bulk(n, add_to=out if add else None, out=out)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    t = float(np.median(times))
    bytes_per = out.element_size() * (2 if add else 1)
    return {"item": item, "type": typ, "add": add, "items_per_call": n, "seconds_median": t,
            "seconds_min": float(np.min(times)), "gsamples_per_s": n / t / 1e9,
            "of_store_ceiling": bytes_per * n / t / CEILING}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log2-items", nargs="+", type=int, default=[20, 24, 28])
    ap.add_argument("--item", default="c64")
    ap.add_argument("--type", default="gaussian")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", help="also write the results here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("benchmark_noise_source.py needs a GPU")
    pkg = ge.load_package()
    results = []
    for lg in a.log2_items:
        for add in (False, True):
            r = run(pkg, a.item, a.type, 1 << lg, add, a.iters)
            results.append(r)
            print(f"{a.item} {a.type} {'in + noise' if add else 'noise     '}  2^{lg} items/call  "
                  f"{r['seconds_median'] * 1e3:9.3f} ms  {r['gsamples_per_s']:8.2f} Gsps  "
                  f"{100 * r['of_store_ceiling']:5.1f} % of 6 TB/s", flush=True)
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
