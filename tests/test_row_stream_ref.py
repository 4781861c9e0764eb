"""The StreamRowResampler's definition on the CPU (no GPU): tests/_row_stream_ref.py's restatement with Python integers for
positions and theta, fed through a dozen cuttings, equals tests/_row_resampler_ref.py's one-shot float32 restatement of the
whole row with ==; a start_index beyond 2^33 equals the one-shot on the same items with the phase0 computed in Python
integers; set_row keeps p* and the phase there; and the host-only calls of blocks.StreamRowResampler (the constructor's
checks, items_for, set_row, state, reset) agree with the restatement without a GPU."""
import numpy as np
import pytest

import _row_resampler_ref as ref
import _row_stream_ref as sref

N = 700
STEPS = [1 << 26, int(0.893 * 2 ** 32), 1 << 32, (1 << 32) + 1, int(2.27 * 2 ** 32), 1 << 38]


def pkg():
    import __graft_entry__ as ge
    return ge.load_package()


def row_items(seed, n=N):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def cuttings(P, n):
    rng = np.random.default_rng(P)
    base = sref.cutting(P, n)
    cuts = [[n], [0, n], [1, n - 1], [n - 1, 1], [P - 1, n - P + 1], [P, n - P], [7] * (n // 7) + [n % 7], base, base[::-1],
            sref.cutting(P, n, 17), sref.cutting(P, n, 43)]
    r, left = [], n
    while left:
        k = min(left, int(rng.integers(0, 2 * P + 3)))
        r.append(k)
        left -= k
    cuts.append(r)
    assert len(cuts) >= 12 and all(sum(c) == n for c in cuts)
    return cuts


def same_bytes(a, b):
    a, b = np.asarray(a, np.complex64), np.asarray(b, np.complex64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("Q,P", [(32, 12), (2, 1), (64, 3)])
def test_any_cutting_equals_the_one_shot_restatement(Q, P):
    rng = np.random.default_rng(Q * P)
    h = rng.standard_normal(Q * P).astype(np.float32)
    x = row_items(Q + P)
    cuts = cuttings(P, N)
    for k, step in enumerate(STEPS):
        phase0 = [0, (3 << 32) + (1 << 30) + 5, ((P + 7) << 32) + 12345][k % 3]
        freq = [0, 1, -(1 << 31), 12345678][k % 4]
        want = ref.resample32(x, N, h, Q, step, phase0, freq)
        assert want.size == ref.output_items(N, P, step, phase0) > 0
        for cut in cuts:
            row = sref.Row(h, Q, step, phase0, freq)
            parts, at = [], 0
            for n in cut:
                parts.append(row.process(x[at:at + n]))
                at += n
            parts.append(row.flush())
            got = np.concatenate(parts)
            assert same_bytes(got, want), (step, cut[:8])
            assert row.A == 0 and row.next_pos == phase0  # back in the created state


def test_positions_and_theta_are_the_unbounded_definitions():
    Q, P = 32, 12
    h = np.random.default_rng(1).standard_normal(Q * P).astype(np.float32)
    x = row_items(2)
    for step in STEPS:
        for start in (0, 1, (1 << 32) - 1, (1 << 33) + 20480, 1 << 63):
            phase0, freq = (5 << 32) + 77, -12884902
            row = sref.Row(h, Q, step, phase0, freq, start)
            assert row.next_pos >= start << 32 and (row.next_m == 0 or row.next_pos - step < start << 32)
            for n in sref.cutting(P, N):
                at = row.A - start
                row.process(x[at:at + n])
            made = len(row.positions)
            assert row.positions == [phase0 + (row.next_m - made + k) * step for k in range(made)]
            assert all(t == ref.theta(freq, p) for p, t in zip(row.positions, row.thetas))
            assert all((p >> 32) <= start + N - 1 for p in row.positions) and row.next_pos >> 32 >= start + N


def test_far_start_equals_the_one_shot_on_the_same_items():
    Q, P = 32, 12
    h = np.random.default_rng(3).standard_normal(Q * P).astype(np.float32)
    x = row_items(4)
    start = (1 << 33) + 20480
    for step in STEPS:
        for freq in (3 << 20, -(3 << 20)):
            assert (freq * start) % (1 << 32) == 0
            row = sref.Row(h, Q, step, 12345, freq, start)
            phase0 = row.next_pos - (start << 32)  # the first item's position from the row's first item
            assert 0 <= phase0 < step
            parts, at = [], 0
            for n in sref.cutting(P, N, 3):
                parts.append(row.process(x[at:at + n]))
                at += n
            parts.append(row.flush())
            assert same_bytes(np.concatenate(parts), ref.resample32(x, N, h, Q, step, phase0, freq)), (step, freq)


def test_set_row_keeps_the_position_and_the_phase():
    Q, P = 32, 12
    h = np.random.default_rng(5).standard_normal(Q * P).astype(np.float32)
    x = row_items(6)
    for step in STEPS:
        row = sref.Row(h, Q, step, 1 << 31, 12345678)
        untouched = sref.Row(h, Q, step, 1 << 31, 12345678)
        a = row.process(x[:300])
        assert same_bytes(a, untouched.process(x[:300]))
        p_star, m_star, before = row.next_pos, row.next_m, row.theta(row.next_pos)
        new_step = min(1 << 38, step + step // 8 + 1)
        row.set_row(new_step, -7654321)
        assert row.next_pos == p_star and row.next_m == m_star
        assert row.theta(p_star) == before  # continuous to 2^-32 cycles: the very word
        row.process(x[300:])
        made = row.positions[-(row.next_m - m_star):]
        assert made[0] == p_star and made == [p_star + k * new_step for k in range(len(made))]
        assert row.thetas[-len(made):] == [(before + ((-7654321 * (p - p_star)) >> 32)) % (1 << 32) for p in made]


def test_the_blocks_host_only_calls_without_a_gpu():
    m = pkg()
    Q, P = 32, 12
    h = m.row_resampler_taps(Q, P)
    starts = [0, 1, (1 << 32) - 1, (1 << 33) + 20480, 1 << 63, 5]
    phase0 = [0, 1 << 31, (20 << 32) + 9, 77, (1 << 63) - 1, 3]
    b = m.StreamRowResampler(STEPS, [0, 1, -(1 << 31), 12345678, -5, 9], phase0, starts, phases=Q, taps=h)
    assert b.n_rows == 6 and b.taps_per_phase == P
    rows = [sref.Row(h, Q, STEPS[r], phase0[r], 0, starts[r]) for r in range(6)]
    for r in range(6):
        assert b.state(r) == (starts[r], rows[r].next_m % (1 << 64)), r
    lengths = [0, 1, P - 1, 255, 5000, (1 << 32) - P]
    assert list(b.items_for(lengths)) == [rows[r].count(lengths[r]) for r in range(6)]
    assert list(b.items_for(lengths)) == [rows[r].count(lengths[r]) for r in range(6)]  # no state moved
    assert list(b.flush_lengths()) == [rows[r].count(P - 1) for r in range(6)]
    b.set_row(1, step=1 << 30)
    rows[1].set_row(1 << 30, 1)
    b.set_rate(2, 0.2, 0.001)
    rows[2].set_row(m.RowResampler.steps_for([0.2])[0], 0)
    assert list(b.items_for(lengths)) == [rows[r].count(lengths[r]) for r in range(6)]
    b.reset()
    assert b.state(3) == (starts[3], rows[3].next_m % (1 << 64))
    with pytest.raises(m.Gr4pmError):
        b.items_for([0, 0, 0, 0, 0, (1 << 32) - P + 1])
    with pytest.raises(m.Gr4pmError):
        b.items_for([1, 2, 3])
    for bad in (dict(steps=[]), dict(steps=[1 << 32] * 65), dict(steps=[(1 << 26) - 1]), dict(steps=[(1 << 38) + 1]),
                dict(steps=[1 << 32], phase0=[1 << 63]), dict(steps=[1 << 32], start_index=[1 << 64]),
                dict(steps=[1 << 32], start_index=[0, 0]), dict(steps=[1 << 32], freqs=[1 << 31]),
                dict(steps=[1 << 32], phases=3), dict(steps=[1 << 32], phases=256, taps_per_phase=17)):
        with pytest.raises(m.Gr4pmError):
            m.StreamRowResampler(**bad)
    for bad in (dict(r=6), dict(r=0, step=(1 << 26) - 1), dict(r=0, step=(1 << 38) + 1)):
        with pytest.raises(m.Gr4pmError):
            b.set_row(**bad)
    c = m.StreamRowResampler.for_rates([0.2, 0.11], [0.001, -0.002])
    assert c._steps == m.RowResampler.steps_for([0.2, 0.11]) and c._freqs == [c._freq_word(0.001), c._freq_word(-0.002)] == [4294967, -8589935]
