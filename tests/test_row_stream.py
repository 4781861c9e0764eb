"""The StreamRowResampler on the GPU (gr4pm_row_stream) beside the one-shot RowResampler, bit for bit.
The two are fronts of one kernel body (csrc/row_kernel.hpp: k_row_stream and k_row_resample instantiate it), so these
comparisons show that carrying a row across calls changes nothing, not that two implementations agree: the float64 bound of
test_row_resampler.py holds the values, and the recorded digests of test_row_resampler_digests.py hold the bits.

One handle of six rows (steps 2^26 .. 2^38), cut into calls differently per row -- forty calls of 1 item, then
P - 2, P - 1, P, 0, 255, 257 and the rest, rotated per row so that every call is ragged -- and flushed, gives the bytes of
RowResampler.process_rows on the whole rows; +0 behind every call's counts in an output pre-filled with NaN; items_for is
what each call reports; a second pass behind the flush gives the same bytes.  A start_index beyond 2^33 gives the one-
shot's bytes at the phase0 the test computes in Python integers.  A set_row after 2000 items stays within the derived bound
of the float64 restatement.  Every refusal is followed by calls that show the state did not move.

Rows are seeded random complex64 of 5000 items."""
import ctypes as C

import numpy as np
import pytest

import _row_resampler_ref as ref
import _row_stream_ref as sref
from _frontend import bits, dev, host, load_package

pytestmark = pytest.mark.gpu

TWO32 = 1 << 32
N = 5000
SIZES = [(32, 12), (2, 1), (256, 16), (64, 3)]
STEPS = [1 << 26, int(0.893 * TWO32), TWO32, TWO32 + 1, int(2.27 * TWO32), 1 << 38]
WORDS = [0, 1, -(1 << 31), 12345678]
R = len(STEPS)


@pytest.fixture(scope="module")
def pkg():
    return load_package()


def make_rows():
    rng = np.random.default_rng(29)
    return (rng.standard_normal((R, N)) + 1j * rng.standard_normal((R, N))).astype(np.complex64)


@pytest.fixture(scope="module")
def rows():
    return make_rows()


def taps_of(Q, P):
    """the design with something random mixed in: every tap matters"""
    rng = np.random.default_rng(Q + P)
    return (ref.kaiser_taps64(Q, P) + 0.05 * rng.standard_normal(Q * P)).astype(np.float32)


def phases_of(P):
    """none, one with a fraction, one beyond P items"""
    return [0, TWO32 // 2 + 3, (P + 5) * TWO32 + TWO32 // 4]


def cuts_of(P):
    """row r starts the list's seven special lengths at call 7 r, so in most of the 47 calls the rows' lengths differ"""
    return [sref.cutting(P, N, 40 - 7 * r) for r in range(R)]


def feed(b, x, cuts, out_columns=None):
    """the rows through the handle, row r cut by cuts[r], then the flush: per row the concatenated items"""
    import torch
    got, at = [[] for _ in range(R)], [0] * R
    n_calls = len(cuts[0])
    for c in range(n_calls + 1):
        last = c == n_calls
        if last:
            want = b.flush_lengths()
        else:
            lengths = [cuts[r][c] for r in range(R)]
            part = np.zeros((R, max(max(lengths), 1)), np.complex64)
            for r in range(R):
                part[r, :lengths[r]] = x[r, at[r]:at[r] + lengths[r]]
                at[r] += lengths[r]
            want = b.items_for(lengths)
        columns = -(-int(want.max()) // 2048) * 2048
        out = torch.full((R, columns), float("nan"), dtype=torch.complex64, device="cuda")
        y, lens = b.flush(out=out) if last else b.process_rows(dev(part), lengths, out=out)
        assert lens.tolist() == want.tolist(), c
        y = host(y)
        assert y.shape == (R, columns)
        for r in range(R):
            assert not bits(y[r, lens[r]:]).any(), f"call {c}, row {r}: an item behind the count {lens[r]} is not +0"
            got[r].append(y[r, :lens[r]].copy())
    assert at == [N] * R
    return [np.concatenate(g) for g in got]


def one_shot(pkg, Q, h, x, steps, phase0, freqs):
    y, lens = pkg.RowResampler(phases=Q, taps=h).process_rows(dev(x), [x.shape[1]] * x.shape[0], steps, phase0, freqs)
    y = host(y)
    return [y[r, :lens[r]] for r in range(x.shape[0])]


def cutting_case(pkg, Q, P, k):
    """the handle of the comparison's case k (phases_of(P)[k], the frequency words rotated by k) and its words"""
    freqs = [WORDS[(r + k) % len(WORDS)] for r in range(R)]
    return pkg.StreamRowResampler(STEPS, freqs, [phases_of(P)[k]] * R, phases=Q, taps=taps_of(Q, P)), freqs


def cutting_output(Q, P, k):
    """per row, what the 47 ragged calls and the flush of case k deliver"""
    return feed(cutting_case(load_package(), Q, P, k)[0], make_rows(), cuts_of(P))


@pytest.mark.parametrize("Q,P", SIZES)
def test_any_cutting_gives_the_one_shot_blocks_bytes(pkg, rows, Q, P):
    h = taps_of(Q, P)
    cuts = cuts_of(P)
    assert all(any(cuts[r][c] == 0 for r in range(R)) and any(cuts[r][c] > 0 for r in range(R)) for c in (3, 10, 17, 24, 31, 38)), \
        "calls in which some rows get nothing while others get items"
    assert sum(len({cuts[r][c] for r in range(R)}) > 1 for c in range(len(cuts[0]))) >= 30, "ragged calls"  # (a special length of 1 beside rows that get 1 is not ragged)
    for k, phase in enumerate(phases_of(P)):
        b, freqs = cutting_case(pkg, Q, P, k)
        want = one_shot(pkg, Q, h, rows, STEPS, [phase] * R, freqs)
        got = feed(b, rows, cuts)
        for r in range(R):
            assert want[r].size == ref.output_items(N, P, STEPS[r], phase) > 0
            assert got[r].tobytes() == want[r].tobytes(), (Q, P, phase, r)
            assert b.state(r) == (0, 0)  # as created
        if k == 1:  # behind the flush the handle is as created: the same rows again, the same bytes
            again = feed(b, rows, cuts[::-1])
            for r in range(R):
                assert again[r].tobytes() == want[r].tobytes(), (Q, P, r)


FAR_START = (1 << 33) + 20480
FAR_FREQS = [(3 << 20) * (1 if r % 2 else -1) for r in range(R)]
FAR_PHASE0 = [12345 + 1000003 * r for r in range(R)]


def far_output(rows=None):
    """per row, what a handle that starts at FAR_START delivers over the ragged calls and the flush"""
    Q, P = 32, 12
    b = load_package().StreamRowResampler(STEPS, FAR_FREQS, FAR_PHASE0, [FAR_START] * R, phases=Q, taps=taps_of(Q, P))
    return feed(b, make_rows() if rows is None else rows, cuts_of(P))


def test_far_positions_give_the_one_shot_blocks_bytes(pkg, rows):
    Q, P = 32, 12
    h = taps_of(Q, P)
    start, freqs, phase0 = FAR_START, FAR_FREQS, FAR_PHASE0
    assert all((f * start) % TWO32 == 0 for f in freqs)
    # the first item's position from the row's first item, in Python integers
    first = [sref.Row(h, Q, STEPS[r], phase0[r], freqs[r], start).next_pos - (start << 32) for r in range(R)]
    assert all(0 <= first[r] < STEPS[r] for r in range(R))
    want = one_shot(pkg, Q, h, rows, STEPS, first, freqs)
    got = far_output(rows)
    for r in range(R):
        assert got[r].tobytes() == want[r].tobytes(), r


SET_ROW_FREQS = [WORDS[r % len(WORDS)] for r in range(R)]
SET_ROW_NEW_STEPS = [min(1 << 38, s + s // 8 + 1) for s in STEPS]
SET_ROW_NEW_FREQS = [-7654321, 0, 1 << 30, -1, 99, -(1 << 31)]


def set_row_calls(rows):
    """2000 items, a set_row on every row, the other 3000 and the flush: the three calls' arrays and counts"""
    Q, P = 32, 12
    b = load_package().StreamRowResampler(STEPS, SET_ROW_FREQS, None, phases=Q, taps=taps_of(Q, P))
    x = dev(rows)
    a, la = b.process_rows(x[:, :2000].contiguous())
    a = host(a)
    for r in range(R):
        b.set_row(r, SET_ROW_NEW_STEPS[r], SET_ROW_NEW_FREQS[r])
    c, lc = b.process_rows(x[:, 2000:].contiguous())
    f, lf = b.flush()
    return (a, host(c), host(f)), (la, lc, lf)


def set_row_output():
    """per row, the items of the three calls one after the other"""
    parts, lens = set_row_calls(make_rows())
    return [np.concatenate([y[r, :n[r]] for y, n in zip(parts, lens)]) for r in range(R)]


def test_set_row_within_the_derived_bound_of_float64(pkg, rows):
    Q, P = 32, 12
    h = taps_of(Q, P)
    freqs, new_steps, new_freqs = SET_ROW_FREQS, SET_ROW_NEW_STEPS, SET_ROW_NEW_FREQS
    (a, c, f), (la, lc, lf) = set_row_calls(rows)
    worst = 0.0
    for r in range(R):
        row = sref.Row(h, Q, STEPS[r], 0, freqs[r], bits=64)
        want = [row.process(rows[r, :2000])]
        p_star = row.next_pos
        row.set_row(new_steps[r], new_freqs[r])
        want += [row.process(rows[r, 2000:]), row.flush()]
        assert [la[r], lc[r], lf[r]] == [w.size for w in want], r
        got = np.concatenate([a[r, :la[r]], c[r, :lc[r]], f[r, :lf[r]]]).astype(np.complex128)
        # the items in front of p* are the one-shot's at the old step, those from p* on the one-shot's at the new step from
        # p*: tests/_row_resampler_ref.py's bound as it is, on either side
        bound = np.concatenate([ref.error_bound(rows[r], N, h, Q, STEPS[r], 0)[:la[r]],
                                ref.error_bound(rows[r], N, h, Q, new_steps[r], p_star)])
        assert bound.size == got.size
        err = np.abs(got - np.concatenate(want))
        live = bound > 0
        worst = max(worst, float(np.max(err[live] / bound[live])))
        assert np.all(err <= bound), (r, float(np.max(err[live] / bound[live])))
    print(f"StreamRowResampler with set_row: worst error / bound = {worst:.3f}")


def test_refusals_leave_the_state(pkg, rows):
    import torch
    Q, P = 32, 12
    h = taps_of(Q, P)
    L = pkg.lib()
    invalid, overflow = -1, -5  # GR4PM_ERR_INVALID, GR4PM_ERR_OVERFLOW
    steps, n = STEPS[1:3], 1000
    want = one_shot(pkg, Q, h, rows[:2, :n], steps, [0, 0], [5, -5])
    b = pkg.StreamRowResampler(steps, [5, -5], phases=Q, taps=h)
    x = dev(rows[:2, :n])
    first, lens = b.process_rows(x[:, :300].contiguous())
    first = host(first)
    state = [b.state(r) for r in range(2)]
    part = x[:, 300:].contiguous()
    counts = b.items_for([700, 700])
    cols = int(counts.max())
    out = torch.full((2, cols), float("nan"), dtype=torch.complex64, device="cuda")
    ol = np.full(2, 99, dtype=np.uint64)
    olp = ol.ctypes.data_as(C.c_void_p)

    def call(xp=part.data_ptr(), stride=700, n_cols=700, lengths=None, outp=out.data_ptr(), out_stride=cols, n_cols_out=cols,
             lens=olp):
        lp = None if lengths is None else np.array(lengths, dtype=np.uint64)
        return L.gr4pm_row_stream_process(b._h, xp, stride, n_cols, None if lp is None else lp.ctypes.data_as(C.c_void_p), outp,
                                          out_stride, n_cols_out, lens)

    refused = [(call(n_cols_out=cols - 1, out_stride=cols), overflow),  # one column too few: nothing is cut
               (call(lengths=[700, 701]), invalid), (call(stride=699), invalid), (call(out_stride=cols - 1), invalid),
               (call(lens=None), invalid), (call(outp=None), invalid), (call(xp=None), invalid),
               (call(n_cols_out=(1 << 31) + 1, out_stride=1 << 32), overflow),
               (call(n_cols=1 << 32, stride=1 << 32, lengths=[1, (1 << 32) - P + 1]), overflow),
               (L.gr4pm_row_stream_flush(b._h, out.data_ptr(), cols, 0, olp), overflow),
               (L.gr4pm_row_stream_set_row(b._h, 2, TWO32, 0), invalid),
               (L.gr4pm_row_stream_set_row(b._h, 0, (1 << 26) - 1, 0), invalid),
               (L.gr4pm_row_stream_set_row(b._h, 0, (1 << 38) + 1, 0), invalid)]
    for k, (status, code) in enumerate(refused):
        assert status == code, k
    assert L.gr4pm_last_error()
    assert ol.tolist() == [99, 99] and torch.isnan(host_real(out)).all(), "a refused call wrote something"
    assert [b.state(r) for r in range(2)] == state and b.items_for([700, 700]).tolist() == counts.tolist()
    with pytest.raises(pkg.Gr4pmError):
        b.process_rows(part, [700, 700], out=out[:, :cols - 1])
    with pytest.raises(TypeError):
        b.process_rows(x[:1])
    # the state did not move: the call itself, and the flush, finish the one-shot's bytes
    assert call() == 0 and ol.tolist() == counts.tolist()
    rest = host(out)
    tail, lt = b.flush()
    tail = host(tail)
    for r in range(2):
        got = np.concatenate([first[r, :lens[r]], rest[r, :counts[r]], tail[r, :lt[r]]])
        assert got.tobytes() == want[r].tobytes(), r
    # nothing in, no column: fine, and nothing moves
    assert call(xp=None, lengths=[0, 0], outp=None, n_cols_out=0, out_stride=0) == 0 and ol.tolist() == [0, 0]


def host_real(t):
    import torch
    torch.cuda.synchronize()
    return t.real.cpu()
