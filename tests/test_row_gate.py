"""The RowBurstGate on the GPU against tests/_row_gate_ref.py: six rows of 5000 seeded items, B in {16, 64, 1024}, n_cols =
max_blocks * B, every row cut differently into 47 calls (tests/_row_stream_ref.py's cutting) and flushed.  The rows are noise
of 0.05 with block-aligned stretches of amplitude 1 and 0.45 (between the thresholds), laid out so that a one-block burst is
dropped, a burst has exactly min_blocks, gaps of hold blocks merge and of hold + 1 split, a burst at item 0 clips its pre
margin, a burst is open at the end and flush closes it with a partial block, a burst longer than max_blocks gives a
truncated piece and a successor, and a stretch between the thresholds neither opens nor closes.  block_power and the sums
the stream form works with are the NumPy restatement's bits; records and burst rows are the reference's bytes and the
one-call run's; +0 stands behind n_items in an output pre-filled with NaN, which stays NaN beyond the count; a second pass
behind the flush gives the same bytes; a cap one too small refuses and the next call delivers everything."""
import numpy as np
import pytest

import _row_gate_ref as ref
from _frontend import load_package
from _row_stream_ref import cutting

pytestmark = pytest.mark.gpu

N, ROWS, SIGMA = 5000, 6, 0.05
L, M, H = 0, 1, 2
# per B: hold, min, pre, post, max
SHAPES = {16: dict(hold=2, min_blocks=2, pre=2, post=2, max_blocks=16),
          64: dict(hold=1, min_blocks=2, pre=1, post=1, max_blocks=8),
          1024: dict(hold=0, min_blocks=2, pre=0, post=1, max_blocks=3)}
FIELDS = ("first_item", "n_items", "first_active_item", "active_items", "flags", "peak", "power")


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def layout(B):
    """the level of every block of the six rows (the last entry is the partial block's)"""
    nb = -(-N // B)
    if B == 1024:
        rows = [[H, L, L, L, L], [H, H, L, L, L], [H, H, H, H, H], [M, M, M, M, M], [L, H, M, L, L], [L, L, L, H, H]]
        assert all(len(r) == nb for r in rows)
        return rows
    s = SHAPES[B]
    h, mn, mx = s["hold"], s["min_blocks"], s["max_blocks"]
    quiet = [L] * (h + 3)
    rows = [
        [H] * mn + quiet + [H] + quiet,                                      # at item 0 with exactly min_blocks; one block: dropped
        [L] * 3 + [H, H] + [L] * h + [H, H] + [L] * (h + 1) + [H, H] + quiet,  # a gap of hold merges, of hold + 1 splits
        [L] * 2 + [H] * (mx + 3) + quiet,                                    # longer than max_blocks
        [L] * 2 + [M] * 4 + [L] * 2 + [H, H] + [M] * (h + 2) + quiet,        # between the thresholds
        [],                                                                  # open at the end
        [],                                                                  # noise only
    ]
    rows = [r + [L] * (nb - len(r)) for r in rows]
    rows[4][nb - 3:] = [H, H, H]
    assert all(len(r) == nb for r in rows)
    return rows


SCENES = {}


def scene(B):
    """(x [6, 5000] complex64, open_sum, close_sum, per row: the reference's records, dropped count and burst rows)"""
    if B in SCENES:
        return SCENES[B]
    rng = np.random.default_rng(100 + B)
    x = SIGMA * (rng.standard_normal((ROWS, N)) + 1j * rng.standard_normal((ROWS, N)))
    for r, levels in enumerate(layout(B)):
        amp = np.repeat(np.array([0.0, 0.45, 1.0])[levels], B)[:N]
        x[r] += amp * np.exp(2j * np.pi * rng.random(N))
    x = x.astype(np.complex64)
    # the floor is 2 sigma^2 = 0.005 per item: 0.05 is 10 dB above it, 0.45^2 + 0.005 lies between, 1 above
    open_sum, close_sum = np.float32(0.5 * B), np.float32(0.05 * B)
    want = []
    for r in range(ROWS):
        row = ref.Row(B, open_sum, close_sum, **SHAPES[B])
        rec, _ = row.process(x[r])
        tail, dropped = row._run(True)  # (the flush, with the items still there for rows_of)
        all_rec = rec + tail
        want.append((all_rec, dropped, row.rows_of(all_rec, SHAPES[B]["max_blocks"] * B)))
    SCENES[B] = (x, open_sum, close_sum, want)
    return SCENES[B]


def make_gate(pkg, B, open_sum, close_sum, **kw):
    s = {**SHAPES[B], **kw}
    g = pkg.RowBurstGate(ROWS, s["max_blocks"] * B, B, s["hold"], s["min_blocks"], s["pre"], s["post"], s["max_blocks"])
    for r in range(ROWS):
        g.set_thresholds(r, open_sum, close_sum)
    return g


def run(gate, x, cuts, cap=64):
    """the rows in the given calls, then the flush: per row (records, burst rows), and checks the NaN pre-fill"""
    import torch
    rec, rows, pos = [[] for _ in range(ROWS)], [[] for _ in range(ROWS)], [0] * ROWS
    out = torch.empty((cap, gate.n_cols), dtype=torch.complex64, device="cuda")

    def collect(res):
        burst_rows, lengths, records = res
        got = out.cpu().numpy()
        n = len(records)
        assert burst_rows.shape == (n, gate.n_cols) and list(lengths) == list(records["n_items"])
        assert not np.isnan(got[:n].view(np.float32)).any() and np.isnan(got[n:].view(np.float32)).all()
        assert list(records["row"]) == sorted(records["row"])  # the order (row, time)
        for j in range(n):
            rec[records["row"][j]].append(records[j])
            rows[records["row"][j]].append(got[j].copy())

    for i in range(len(cuts[0])):
        lens = [cuts[r][i] for r in range(ROWS)]
        chunk = np.zeros((ROWS, max(max(lens), 1)), np.complex64)
        for r in range(ROWS):
            chunk[r, :lens[r]] = x[r, pos[r]:pos[r] + lens[r]]
            pos[r] += lens[r]
        out.fill_(complex(float("nan"), float("nan")))
        collect(gate.process_rows(torch.from_numpy(chunk).cuda(), lens, cap=cap, out=out))
    assert pos == [x.shape[1]] * ROWS
    out.fill_(complex(float("nan"), float("nan")))
    collect(gate.flush(cap=cap, out=out))
    return rec, rows


def same_as_reference(got, want, B):
    rec, rows = got
    for r in range(ROWS):
        w_rec, _, w_rows = want[r]
        assert len(rec[r]) == len(w_rec), (B, r, len(rec[r]), len(w_rec))
        for a, b in zip(rec[r], w_rec):
            for f in FIELDS:
                assert a[f] == b[f], (B, r, f, a, b)
        if w_rec:
            assert np.stack(rows[r]).tobytes() == w_rows.tobytes(), (B, r)


@pytest.mark.parametrize("B", [16, 64, 1024])
def test_the_scene_holds_every_case(B):
    """(the reference alone) the layout does what the docstring says"""
    _, _, _, want = scene(B)
    flags = [[r["flags"] for r in w[0]] for w in want]
    dropped = [w[1] for w in want]
    if B == 1024:
        assert flags == [[], [0], [ref.TRUNCATED, ref.AT_END], [], [0], [ref.AT_END]] and dropped == [1, 0, 0, 0, 0, 0]
        assert want[2][0][1]["n_items"] == N - 3 * B and want[5][0][0]["n_items"] == N - 3 * B
        return
    s = SHAPES[B]
    assert flags == [[0], [0, 0], [ref.TRUNCATED, 0], [0], [ref.AT_END], []] and dropped == [1, 0, 0, 0, 0, 0]
    assert want[0][0][0]["first_item"] == 0 and want[0][0][0]["active_items"] == s["min_blocks"] * B
    assert want[1][0][0]["active_items"] == (4 + s["hold"]) * B and want[1][0][1]["active_items"] == 2 * B
    assert want[2][0][0]["n_items"] == s["max_blocks"] * B
    assert want[2][0][1]["first_item"] < want[2][0][0]["first_item"] + want[2][0][0]["n_items"]  # the pre margin overlaps
    assert want[3][0][0]["active_items"] == (4 + s["hold"]) * B
    last = want[4][0][0]
    assert last["first_item"] + last["n_items"] == N and N % B and last["active_items"] == 2 * B + N % B


@pytest.mark.parametrize("B", [16, 64, 1024])
def test_block_power_bit_for_bit(pkg, B):
    import torch
    x, _, _, _ = scene(B)
    gate = make_gate(pkg, B, 1.0, 1.0)
    lengths = [N, N - 1, N // 2, B, B - 1, 0]
    got = gate.block_power(torch.from_numpy(x).cuda(), lengths)
    for r in range(ROWS):
        want = ref.block_sums(x[r, :lengths[r]], B)
        assert got[r].dtype == np.float32 and got[r].tobytes() == want.tobytes(), (B, r)
    # the sums of the stream form, in the cutting: every block opens a burst that its own block ends (max_blocks = 1),
    # so the records' peaks are the block sums the calls worked with
    every = make_gate(pkg, B, 1e-30, 1e-30, hold=0, min_blocks=1, pre=0, post=0, max_blocks=1)
    rec, _ = run(every, x, [cutting(B, N, 7 * r) for r in range(ROWS)], cap=2 * (N // B + 1))
    for r in range(ROWS):
        want = ref.block_sums(x[r], B, pad=True)
        assert np.array([a["peak"] for a in rec[r]], np.float32).tobytes() == want.tobytes(), (B, r)
        assert [a["flags"] for a in rec[r]] == [ref.TRUNCATED] * want.size
        assert every.state(r)["truncated"] == want.size


@pytest.mark.parametrize("B", [16, 64, 1024])
def test_records_and_burst_rows_in_any_cutting(pkg, B):
    x, open_sum, close_sum, want = scene(B)
    gate = make_gate(pkg, B, open_sum, close_sum)
    cuts = [cutting(B, N, 7 * r) for r in range(ROWS)]
    assert all(len(c) == 47 for c in cuts)
    first = run(gate, x, cuts)
    same_as_reference(first, want, B)
    for r in range(ROWS):
        s = gate.state(r)
        assert (s["items"], s["blocks"], s["open"], s["emitted"], s["dropped"]) == (0, 0, False, len(want[r][0]), want[r][1])
    second = run(gate, x, cuts)  # behind the flush the rows count from 0 again
    same_as_reference(second, want, B)
    one = run(gate, x, [[N]] * ROWS)
    same_as_reference(one, want, B)
    for r in range(ROWS):
        assert [a.tobytes() for a in one[0][r]] == [a.tobytes() for a in first[0][r]]
        assert [a.tobytes() for a in one[1][r]] == [a.tobytes() for a in first[1][r]]


def test_a_cap_one_too_small_refuses_and_the_next_call_delivers(pkg):
    import torch
    B = 64
    x, open_sum, close_sum, want = scene(B)
    gate = make_gate(pkg, B, open_sum, close_sum)
    dev = torch.from_numpy(x).cuda()
    in_call = sum(sum(1 for a in w[0] if a["flags"] != ref.AT_END) for w in want)
    assert in_call >= 4
    with pytest.raises(pkg.Gr4pmError, match="more bursts"):
        gate.process_rows(dev, cap=in_call - 1)
    assert all(gate.state(r) == dict(items=0, blocks=0, open=False, emitted=0, dropped=0, truncated=0) for r in range(ROWS))
    burst_rows, lengths, records = gate.process_rows(dev)
    assert len(records) == in_call and burst_rows.shape[0] == in_call
    # the default cap is a guess: a call that emits more is made once more with the library's count
    every = make_gate(pkg, B, 1e-30, 1e-30, hold=0, min_blocks=1, pre=0, post=0, max_blocks=1)
    many = every.process_rows(dev)
    assert len(many[2]) == ROWS * (N // B) and many[0].shape == (ROWS * (N // B), B)
    assert many[0].cpu().numpy().tobytes() == x[:, :N // B * B].tobytes()
    tail_rows, _, tail = gate.flush()
    got = np.concatenate([burst_rows.cpu().numpy(), tail_rows.cpu().numpy()])
    rec = np.concatenate([records, tail])
    for r in range(ROWS):
        mine = got[rec["row"] == r]
        assert mine.shape[0] == len(want[r][0])
        if mine.shape[0]:
            assert mine.tobytes() == want[r][2].tobytes()


def test_refusals(pkg):
    import torch
    with pytest.raises(pkg.Gr4pmError, match="rows"):
        pkg.RowBurstGate(65)
    with pytest.raises(pkg.Gr4pmError, match="power of two"):
        pkg.RowBurstGate(2, block=48)
    with pytest.raises(pkg.Gr4pmError, match="post_blocks"):
        pkg.RowBurstGate(2, hold_blocks=3, post_blocks=5)
    with pytest.raises(pkg.Gr4pmError, match="max_blocks"):
        pkg.RowBurstGate(2, n_cols=4096, max_blocks=65)
    with pytest.raises(pkg.Gr4pmError, match="max_blocks"):
        pkg.RowBurstGate(2, max_blocks=9)
    gate = pkg.RowBurstGate(2)
    with pytest.raises(pkg.Gr4pmError, match="close_sum"):
        gate.set_thresholds(0, 1.0, 2.0)
    gate.set_floor([0.005, 0.005])
    x = torch.zeros((2, 100), dtype=torch.complex64, device="cuda")
    with pytest.raises(pkg.Gr4pmError, match="stride"):
        gate.process_rows(x, [100, 101])
    assert gate.state(0)["items"] == 0 and gate.state(1)["items"] == 0
    gate.process_rows(x, [100, 7])
    assert [gate.state(r)["items"] for r in range(2)] == [100, 7] and gate.state(0)["blocks"] == 1
    gate.reset()
    assert gate.state(0) == dict(items=0, blocks=0, open=False, emitted=0, dropped=0, truncated=0)
