#!/usr/bin/env python3
"""Ddc.extract beside the streaming Ddc on one recording.

A recording of 2^28 samples (--log2-samples), complex64 and sc16, seeded noise on the device.  Two shapes:
    K = 8, D = 16, L = 192     K = 1, D = 4, L = 48
For each, Ddc.process_bulk of the whole recording (every frame of every channel), and Ddc.extract at the duties
1/16, 1/4 and 1: every carrier is on the air that share of the time, in 64 equal spans per call, spread evenly over
the channels and over the recording.  Each is timed by device events around the one call, median of 10 (--repeat) after 2
warm-up calls, the stream's reset outside the timed window, the output allocated once.  The crossover is the duty at which
the extract takes the stream's time, interpolated linearly between the measured duties.

Rates are recording samples per second for the stream (n / t) and, for the extract, the samples the spans stand for
(duty x n / t): the work a user asked for, not a share of any peak.

Needs the GPU: there is no fallback.  Prints a table and one JSON line; --json writes the line to a file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

SHAPES = [dict(K=8, D=16, L=192), dict(K=1, D=4, L=48)]
DUTIES = [(1, 16), (1, 4), (1, 1)]
SPANS = 64


def timed(torch, fn, before, repeat, warmup=2):
    """median, min and max milliseconds of fn() by device events; before() runs outside the window"""
    ms = []
    for i in range(warmup + repeat):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def spans_of(K, F, num, den):
    """64 equal spans: span b on channel b mod K, the channel's spans evenly spread over its F frames, together num / den
    of them"""
    per_channel = SPANS // K
    n = F * num // den // per_channel
    return [(b % K, (b // K) * (F // per_channel), n) for b in range(SPANS)], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-samples", type=int, default=28)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--json")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "benchmark_ddc_extract.py needs a GPU"
    pkg = ge.load_package()
    n = 1 << a.log2_samples
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.view_as_complex(torch.randn((n, 2), dtype=torch.float32, device="cuda", generator=g))
    xi = torch.randint(-2048, 2048, (n, 2), dtype=torch.int16, device="cuda", generator=g)
    result = {"samples": n, "repeat": a.repeat, "device": torch.cuda.get_device_name(0), "shapes": []}
    print(f"recording: 2^{a.log2_samples} samples, median of {a.repeat} by device events (min .. max)")
    for s in SHAPES:
        K, D, L = s["K"], s["D"], s["L"]
        F = n // D
        freqs = [(-0.4 + 0.8 * (k + 0.37) / K) for k in range(K)]
        taps = np.asarray(pkg.ddc_taps(D, L // D))
        d = pkg.Ddc(freqs, D, taps=taps, max_frames=F)
        shape = {"K": K, "D": D, "L": L, "formats": {}}
        for name, rec in (("complex64", x), ("sc16", xi)):
            out = torch.empty((K, F), dtype=torch.complex64, device="cuda")
            t_stream = timed(torch, lambda: d.process_bulk(rec, out=out), d.reset, a.repeat)
            del out
            row = {"stream_ms": t_stream, "stream_gsps": n / t_stream[0] / 1e6, "extract": []}
            print(f"K = {K}, D = {D}, L = {L}, {name}: stream {t_stream[0]:.3f} ms ({t_stream[1]:.3f} .. {t_stream[2]:.3f}), "
                  f"{row['stream_gsps']:.1f} Gsamples/s")
            points = []
            for num, den in DUTIES:
                spans, n_cols = spans_of(K, F, num, den)
                spans = np.array([(k, m, f) for k, f, m in spans], dtype=pkg.Ddc.SPAN_DTYPE)  # converted once, not per call
                rows = torch.empty((SPANS, n_cols), dtype=torch.complex64, device="cuda")
                t = timed(torch, lambda: d.extract(rec, spans, n_cols=n_cols, out=rows), lambda: None, a.repeat)
                del rows
                duty = num / den
                points.append((duty, t[0]))
                row["extract"].append({"duty": duty, "frames_per_span": n_cols, "ms": t, "gsps_of_spans": duty * n / t[0] / 1e6,
                                       "over_stream": t[0] / t_stream[0]})
                print(f"    extract, duty {num}/{den}: 64 spans of {n_cols} frames, {t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f}), "
                      f"{t[0] / t_stream[0]:.3f} of the stream, {duty * n / t[0] / 1e6:.1f} Gsamples/s of spans")
            cross = None
            for (d0, t0), (d1, t1) in zip(points[:-1], points[1:]):
                if t0 <= t_stream[0] <= t1 and t1 > t0:
                    cross = d0 + (d1 - d0) * (t_stream[0] - t0) / (t1 - t0)
            if cross is None:
                cross = "below 1/16" if points[0][1] > t_stream[0] else "above 1"
            row["crossover_duty"] = cross
            print(f"    crossover duty: {cross if isinstance(cross, str) else f'{cross:.3f}'}")
            shape["formats"][name] = row
        result["shapes"].append(shape)
        del d
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
