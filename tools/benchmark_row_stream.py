#!/usr/bin/env python3
"""Rate of the StreamRowResampler block (csrc/row_stream.hip) beside the one-shot RowResampler on the same rows, in the same
process.

  tools/benchmark_row_stream.py [--rows 64] [--log2-cols 22] [--iters 20]

Calls of gr4pm_row_stream_process into a preallocated output, timed with device events; the median over the iterations.
Shapes: [rows, 2^log2-cols] complex64 at steps of 0.893 and 2.27 input items per output item in one call (a frequency word
on every row), then 64 rows of 4096 items per call over 64 calls, timed as one stretch.  The yardstick is
gr4pm_row_resampler_process on the same rows (64 calls of it for the small shape): the kernel the stream kernel restates,
not the code under test.  Prints one JSON line per (shape, step).  Expected from the code, not
asserted: the same work per output item, P - 1 history items more per tile of 1024, and one more launch of a workgroup per
row: a ratio of 1.00 to 1.02 at the large shapes, and up to twice the one-shot where a call is two launches of a few
microseconds each."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_channelizer import median_ms  # noqa: E402

TWO32 = 1 << 32


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--log2-cols", type=int, default=22)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    lib = pkg.lib()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(1)
    one = pkg.RowResampler()
    for rows, cols, steps, calls in ((args.rows, 1 << args.log2_cols, (0.893, 2.27), 1), (64, 4096, (0.893, 2.27), 64)):
        x = torch.view_as_complex(torch.randn((rows, cols, 2), dtype=torch.float32, device="cuda", generator=g))
        for step in steps:
            q = [round(step * TWO32)] * rows
            freqs = [round(0.003 * TWO32) * (1 - 2 * (r % 2)) for r in range(rows)]
            longest = int(one.output_lengths([cols] * rows, q).max())
            n_cols = -(-(longest + 1) // 2048) * 2048  # a call of the stream makes one item more or fewer than the last
            out = torch.empty((rows, n_cols), dtype=torch.complex64, device="cuda")
            lens = np.zeros(rows, dtype=np.uint64)
            lp = lens.ctypes.data_as(C.c_void_p)
            # the C entries with the records made once: a call of the small shape is shorter than the classes' bookkeeping
            rec = one._records(rows, q, None, freqs)
            rp, h1 = rec.ctypes.data_as(C.c_void_p), one._handle()
            rs = pkg.StreamRowResampler(q, freqs)

            def stream():
                for _ in range(calls):
                    lib.gr4pm_row_stream_process(rs._h, x.data_ptr(), cols, cols, None, out.data_ptr(), n_cols, n_cols, lp)

            def one_shot():
                for _ in range(calls):
                    lib.gr4pm_row_resampler_process(h1, x.data_ptr(), cols, cols, None, rp, rows, out.data_ptr(), n_cols, n_cols, lp)

            assert lib.gr4pm_row_stream_process(rs._h, x.data_ptr(), cols, cols, None, out.data_ptr(), n_cols, n_cols, lp) == 0
            made = int(lens.max())
            one_ms = median_ms(one_shot, args.iters, torch)
            ms = median_ms(stream, args.iters, torch)
            one_ms_2 = median_ms(one_shot, args.iters, torch)  # the yardstick again: its own spread in this process
            print(json.dumps({"tool": "benchmark_row_stream", "rows": rows, "cols": cols, "calls": calls, "step": step,
                              "out_cols": n_cols, "items_first_call": made, "ms": round(ms, 4),
                              "gitems_out_per_s": round(calls * rows * longest / ms / 1e6, 2),
                              "one_shot_ms": round(one_ms, 4), "one_shot_ms_again": round(one_ms_2, 4),
                              "over_one_shot": round(ms / min(one_ms, one_ms_2), 3),
                              "device": torch.cuda.get_device_name(0)}), flush=True)
            del out, rs
        del x


if __name__ == "__main__":
    main()
