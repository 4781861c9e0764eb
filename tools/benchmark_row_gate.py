#!/usr/bin/env python3
"""Rate of the RowBurstGate block (csrc/row_gate.hip) beside a device copy of the same rows, in the same process.

  tools/benchmark_row_gate.py [--rows 64] [--log2-cols 22] [--iters 20]

[rows, 2^log2-cols] complex64: noise of 0.05 with bursts of 2420 items of amplitude 1, on the air 1/16 of the time (one
every 38 720 items) and 3/4 of it (one every 3227 items).  The C entries into preallocated outputs, timed with device
events; the median over the iterations.  Per duty: gr4pm_row_gate_block_power alone; a whole gr4pm_row_gate_process call
(reset first, which is host only: every call is the same call), which is the power pass, the copy of the block sums to the
host and the wait for them, the host's plan over them, and the copies of the burst rows and of what the rows retain; and,
before and after, a device copy of the rows' bytes: the yardstick, not the code under test.  Prints one JSON line per duty.
Expected from the code, not asserted: the power pass reads 8 bytes per item and writes 1 / 64 of
that, where the copy reads and writes 8; the gather moves the duty's share; so a call at duty 1/16 should take less than
the copy."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark_channelizer import median_ms  # noqa: E402

BURST = 2420


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
    rows, cols = args.rows, 1 << args.log2_cols
    g = torch.Generator(device="cuda").manual_seed(1)
    for duty, period in (("1/16", 16 * BURST), ("3/4", 3227)):
        x = torch.randn((rows, cols, 2), dtype=torch.float32, device="cuda", generator=g) * 0.05
        on = (torch.arange(cols, device="cuda") % period) < BURST
        phase = torch.rand((rows, cols), device="cuda", generator=g) * (2 * np.pi)
        x[..., 0] += on * torch.cos(phase)
        x[..., 1] += on * torch.sin(phase)
        del phase
        x = torch.view_as_complex(x)
        y = torch.empty_like(x)
        gate = pkg.RowBurstGate(rows)  # the defaults: blocks of 64, burst rows of 4096 columns
        gate.set_floor([2 * 0.05 ** 2] * rows)
        lens = np.full(rows, cols, dtype=np.uint64)
        lp = lens.ctypes.data_as(C.c_void_p)
        count = C.c_size_t(0)
        status = lib.gr4pm_row_gate_process(gate._h, x.data_ptr(), cols, lp, None, 0, 0, None, C.byref(count))
        assert status == -5 and count.value > 0, (status, count.value)  # the capacity refusal reports the count
        cap = count.value
        out = torch.empty((cap, gate.n_cols), dtype=torch.complex64, device="cuda")
        rec = np.zeros(cap, dtype=pkg._abi.ROW_GATE_RECORD_DTYPE)
        rp = rec.ctypes.data_as(C.c_void_p)
        sums = torch.empty((rows, cols // gate.block), dtype=torch.float32, device="cuda")

        def power():
            lib.gr4pm_row_gate_block_power(gate._h, x.data_ptr(), cols, lp, sums.data_ptr(), cols // gate.block)

        def process():
            lib.gr4pm_row_gate_reset(gate._h)
            lib.gr4pm_row_gate_process(gate._h, x.data_ptr(), cols, lp, out.data_ptr(), gate.n_cols, cap, rp, C.byref(count))

        def copy():
            y.copy_(x)

        assert lib.gr4pm_row_gate_process(gate._h, x.data_ptr(), cols, lp, out.data_ptr(), gate.n_cols, cap, rp, C.byref(count)) == 0
        assert count.value == cap
        burst_items = int(rec["n_items"].sum())
        copy_ms = median_ms(copy, args.iters, torch)
        power_ms = median_ms(power, args.iters, torch)
        ms = median_ms(process, args.iters, torch)
        copy_ms_2 = median_ms(copy, args.iters, torch)  # the yardstick again: its own spread in this process
        best = min(copy_ms, copy_ms_2)
        print(json.dumps({"tool": "benchmark_row_gate", "rows": rows, "cols": cols, "duty": duty, "bursts": cap,
                          "burst_items": burst_items, "out_gbytes": round(cap * gate.n_cols * 8 / 1e9, 3),
                          "block_power_ms": round(power_ms, 4), "block_power_gitems_per_s": round(rows * cols / power_ms / 1e6, 1),
                          "process_ms": round(ms, 4), "process_gitems_per_s": round(rows * cols / ms / 1e6, 1),
                          "copy_ms": round(copy_ms, 4), "copy_ms_again": round(copy_ms_2, 4),
                          "block_power_over_copy": round(power_ms / best, 3), "process_over_copy": round(ms / best, 3),
                          "device": torch.cuda.get_device_name(0)}), flush=True)
        del x, y, out, sums, gate


if __name__ == "__main__":
    main()
