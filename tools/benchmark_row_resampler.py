#!/usr/bin/env python3
"""Rate of the RowResampler block (csrc/row_resampler.hip) beside a copy of the same bytes, in the same process.

  tools/benchmark_row_resampler.py [--rows 64] [--log2-cols 22] [--iters 20]

One gr4pm_row_resampler_process call into a preallocated output per iteration, timed with device events; the median over the
iterations.  Shapes: [rows, 2^log2-cols] complex64 at steps of 0.893 and 2.27 input items per output item (a frequency
word on every row), then the shape Ddc.extract makes, 64 rows of 6144 items, at 0.893.  Beside each: torch's
device-to-device copy of as many bytes as the call reads and writes (8 per input item, 8 per output column), so the ratio
says how far the kernel is from a pass that only moves its data.  Prints one JSON line per (shape, step).  Expected from
the code, not asserted: 12 multiply-accumulates of three fmaf and two 8-byte LDS reads each, and a
double-precision rotator, per output item: vector-issue-bound at 0.893, close to the copy at 2.27."""
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
    rs = pkg.RowResampler()
    for rows, cols, steps in ((args.rows, 1 << args.log2_cols, (0.893, 2.27)), (64, 6144, (0.893,))):
        x = torch.view_as_complex(torch.randn((rows, cols, 2), dtype=torch.float32, device="cuda", generator=g))
        for step in steps:
            q = [round(step * TWO32)] * rows
            freqs = [round(0.003 * TWO32) * (1 - 2 * (r % 2)) for r in range(rows)]
            longest = int(rs.output_lengths([cols] * rows, q).max())
            n_cols = -(-longest // 2048) * 2048
            out = torch.empty((rows, n_cols), dtype=torch.complex64, device="cuda")
            # the C entry with the records made once: a call of the small shape is shorter than the class's bookkeeping
            rec = rs._records(rows, q, None, freqs)
            lens = np.zeros(rows, dtype=np.uint64)
            rp, lp, h = rec.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), rs._handle()
            call = lambda: lib.gr4pm_row_resampler_process(h, x.data_ptr(), cols, cols, None, rp, rows, out.data_ptr(), n_cols,
                                                           n_cols, lp)
            assert call() == 0 and int(lens.max()) == longest
            ms = median_ms(call, args.iters, torch)
            moved = rows * (cols + n_cols)  # items read plus items written
            src = torch.empty(moved // 2, dtype=torch.complex64, device="cuda")
            dst = torch.empty_like(src)
            copy_ms = median_ms(lambda: dst.copy_(src), args.iters, torch)
            del src, dst, out
            print(json.dumps({"tool": "benchmark_row_resampler", "rows": rows, "cols": cols, "step": step, "out_cols": n_cols,
                              "tile_items": rs.tile_items(q), "ms": round(ms, 4),
                              "gitems_out_per_s": round(rows * longest / ms / 1e6, 2),
                              "moved_tb_per_s": round(8 * moved / ms / 1e9, 3), "copy_ms": round(copy_ms, 4),
                              "copy_tb_per_s": round(8 * moved / copy_ms / 1e9, 3), "over_copy": round(ms / copy_ms, 3),
                              "device": torch.cuda.get_device_name(0)}), flush=True)
        del x


if __name__ == "__main__":
    main()
