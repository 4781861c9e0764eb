"""tests/_row_gate_ref.py alone, without a GPU: the NumPy statement of the RowBurstGate's definition is cut-invariant on
seeded rows, its block sum follows the stated order, and the edge cases of tests/test_row_gate.py give the records that are
written out here, on hand-written block sums."""
import numpy as np

import _row_gate_ref as ref
from _row_stream_ref import cutting

KW = dict(hold=1, min_blocks=2, pre=1, post=1, max_blocks=8)
LO, MID, HI = 1.0, 3.0, 5.0  # against close_sum 2 and open_sum 4


def records(sums, n_items=None, B=16, **kw):
    kw = {**KW, **kw}
    n_items = len(sums) * B if n_items is None else n_items
    rec, dropped = ref.gate(sums, n_items, B, 4.0, 2.0, **kw)
    return [(r["first_item"], r["n_items"], r["first_active_item"], r["active_items"], r["flags"], float(r["peak"]), r["power"])
            for r in rec], dropped


def test_block_sum_order():
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(np.complex64)
    p = ref.item_power(x)
    assert p.dtype == np.float32
    # B = 16: folds only
    t = p[:16].copy()
    for off in (8, 4, 2, 1):
        t = t[:off] + t[off:2 * off]
    assert ref.block_sums(x, 16)[0] == t[0]
    # B = 256: four items per lane in ascending order, then six folds
    t = p[256:512].reshape(4, 64)
    lane = ((t[0] + t[1]) + t[2]) + t[3]
    for off in (32, 16, 8, 4, 2, 1):
        lane = lane[:off] + lane[off:2 * off]
    assert ref.block_sums(x, 256)[1] == lane[0]
    assert ref.block_sums(x[:100], 64).size == 1 and ref.block_sums(x[:100], 64, pad=True).size == 2
    assert ref.block_sums(x[:100], 64, pad=True)[1] == ref.block_sums(np.concatenate([x[64:100], np.zeros(28, np.complex64)]), 64)[0]


def test_one_block_is_dropped_and_min_blocks_is_kept():
    assert records([LO, LO, HI, LO, LO, LO]) == ([], 1)
    # two active blocks 2, 3: closed at block 5 (hold 1: the second inactive one), span [1, 4]
    assert records([LO, LO, HI, HI, LO, LO, LO]) == ([(16, 64, 32, 32, 0, 5.0, 10.0 / 32)], 0)


def test_gap_of_hold_merges_and_of_hold_plus_one_splits():
    got, dropped = records([LO, HI, HI, LO, HI, HI, LO, LO, LO])
    assert got == [(0, 112, 16, 80, 0, 5.0, 20.0 / 80)] and dropped == 0  # one inactive block inside, not in the power
    got, dropped = records([LO, HI, HI, LO, LO, HI, HI, LO, LO, LO])
    assert got == [(0, 64, 16, 32, 0, 5.0, 10.0 / 32), (64, 64, 80, 32, 0, 5.0, 10.0 / 32)] and dropped == 0


def test_burst_at_item_zero_clips_the_pre_margin():
    assert records([HI, HI, LO, LO]) == ([(0, 48, 0, 32, 0, 5.0, 10.0 / 32)], 0)


def test_between_the_thresholds_neither_opens_nor_closes():
    assert records([MID, MID, MID, LO]) == ([], 0)
    got, _ = records([LO, HI, MID, MID, MID, LO, LO])
    assert got == [(0, 96, 16, 64, 0, 5.0, 14.0 / 64)]


def test_flush_closes_an_open_burst_with_a_partial_block():
    # blocks 2, 3 and 8 of 16 items of a fourth: the zero-completed block is active, the margins are clipped to 56 items
    got, dropped = records([LO, LO, HI, HI], n_items=56)
    assert got == [(16, 40, 32, 24, ref.AT_END, 5.0, 10.0 / 24)] and dropped == 0
    # the partial block below close: it is the first inactive one, flush closes; post reaches into it
    got, _ = records([LO, HI, HI, LO], n_items=50)
    assert got == [(0, 50, 16, 32, ref.AT_END, 5.0, 10.0 / 32)]
    # without flush nothing closes
    assert ref.gate([LO, HI, HI, LO], 64, 16, 4.0, 2.0, flush=False, **KW)[0] == []


def test_forced_split_gives_a_truncated_piece_and_a_successor():
    # opens at block 2, start 1; block 8 completes max_blocks = 8; block 9 opens again, its pre margin is block 8
    got, dropped = records([LO, LO] + [HI] * 9 + [LO, LO])
    assert got == [(16, 128, 32, 112, ref.TRUNCATED, 5.0, 35.0 / 112), (128, 64, 144, 32, 0, 5.0, 10.0 / 32)] and dropped == 0
    # a truncated piece is emitted whatever its active extent; the successor of one block is dropped
    got, dropped = records([HI, LO, HI, LO], max_blocks=3, min_blocks=2, pre=0, post=1)
    assert got == [(0, 48, 0, 48, ref.TRUNCATED, 5.0, 10.0 / 48)] and dropped == 0


def test_thresholds_per_block():
    opens = np.array([4, 4, 4, 2.5, 2.5, 2.5, 2.5], np.float32)
    closes = np.array([2, 2, 2, 0.5, 0.5, 0.5, 0.5], np.float32)
    rec, _ = ref.gate([MID, MID, MID, MID, LO, 0.25, 0.25], 7 * 16, 16, opens, closes, **KW)
    assert [(r["first_item"], r["n_items"], r["first_active_item"], r["active_items"]) for r in rec] == [(32, 64, 48, 32)]


def test_cut_invariant_on_seeded_rows():
    rng = np.random.default_rng(2030)
    for B in (16, 64):
        n = 5000
        x = 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        for lo, hi in ((0, 3 * B), (10 * B + 5, 13 * B), (20 * B, 20 * B + B // 2), (30 * B, 45 * B), (n - 3 * B - 7, n)):
            x[lo:hi] += np.exp(2j * np.pi * rng.random(hi - lo))
        x = x.astype(np.complex64)
        kw = dict(hold=1, min_blocks=2, pre=2, post=2, max_blocks=12)
        floor = 2 * 0.05 ** 2 * B
        whole = ref.Row(B, 10 * floor, 4 * floor, **kw)
        rec, dropped = whole.process(x)
        tail, dropped, rows = whole.flush(12 * B)
        rec = rec + tail
        assert len(rec) >= 5 and any(r["flags"] & ref.TRUNCATED for r in rec) and rec[-1]["flags"] == ref.AT_END
        for shift in (0, 13, 41):
            row = ref.Row(B, 10 * floor, 4 * floor, **kw)
            got, pos = [], 0
            for c in cutting(12, n, shift):
                got += row.process(x[pos:pos + c])[0]
                pos += c
            last, d2, _ = row.flush()
            assert got + last == rec and d2 == dropped
