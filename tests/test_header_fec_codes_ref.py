"""The LDPC test codes of tests/_ldpc_codes.py and the inputs tests/test_header_fec_codes.py decodes on the GPU, held
to what they are chosen for -- on the CPU, with the serial decoder of oracle/ alone.  An edit of a fixture under
tests/golden/ldpc/ that loses a property fails here and does not thin the GPU test silently."""
import numpy as np
import pytest

import _ldpc_codes as lc
import _oracle as orc

# steps of the greedy layering per code; the decoder's table holds 24 (csrc/header_blocks.hip: kMaxSteps)
STEPS = {"c16_8": 2, "c48_8": 3, "c80_16": 3, "c136_128": 17, "c200_136": 17, "c256_192_mixed": 23, "shipped": 8,
         "c256_192_all8": 38}
# (n, m, lowest row weight, highest row weight)
SHAPE = {"c16_8": (16, 8, 3, 4), "c48_8": (48, 8, 7, 8), "c80_16": (80, 16, 8, 8), "c136_128": (136, 128, 3, 3),
         "c200_136": (200, 136, 5, 7), "c256_192_mixed": (256, 192, 4, 8), "shipped": (128, 96, 3, 5),
         "c256_192_all8": (256, 192, 8, 8)}


@pytest.mark.parametrize("name", lc.ACCEPTED + (lc.REFUSED,))
def test_code_shape_and_layering(name):
    code = lc.load(name)
    n, m, lo, hi = SHAPE[name]
    weights = [len(r) for r in code.rows]
    assert (code.n, code.m, min(weights), max(weights)) == (n, m, lo, hi)
    assert set(weights) == set(range(lo, hi + 1)), "every weight of the range occurs"
    assert all(len(set(r)) == len(r) and all(0 <= v < n for v in r) for r in code.rows)
    assert set(v for r in code.rows for v in r) == set(range(n)), "every variable is checked"
    assert code.k % 8 == 0 and code.k <= 64
    passes = lc.greedy_layers(code.n, code.rows)
    assert sorted(c for p in passes for c in p) == list(range(m))
    for p in passes:  # a pass: at most 64 edges, no variable twice
        vs = [v for c in p for v in code.rows[c]]
        assert len(vs) <= 64 and len(set(vs)) == len(vs)
    assert len(passes) == STEPS[name]
    if name == lc.REFUSED:
        assert len(passes) > 24
    else:
        assert len(passes) <= 24
    assert lc.read_alist(lc.write_alist(code.n, code.m, code.rows)) == (code.n, code.m, code.rows)


def test_codes_reach_the_untested_paths():
    """what each code is in the set for (csrc/header_blocks.hip: k_header_fec)"""
    codes = {name: lc.load(name) for name in lc.ACCEPTED}
    assert max(STEPS[name] for name in lc.ACCEPTED) >= 23, "a layering next to the 24-step table"
    assert sorted(set(c.k for c in codes.values())) == [8, 32, 40, 64], "one header byte, four, five, eight"
    assert codes["c16_8"].n < 64 and codes["c136_128"].n % 64 and codes["c200_136"].n % 64 == 8
    # edges 5, 6 and 7 come from the table, not from the schedule entry: every check of c48_8, parity variables too
    assert all(len(r) > 5 for r in codes["c48_8"].rows)
    for name in ("c48_8", "c80_16", "c256_192_mixed"):
        c = codes[name]
        for edge in (5, 6, 7):
            assert any(len(r) > edge and r[edge] >= c.k for r in c.rows), (name, edge)
            assert any(len(r) > edge and r[edge] < c.k for r in c.rows), (name, edge)
    # a step with all 64 lanes busy: eight checks of weight 8
    c = codes["c80_16"]
    assert any(len(p) == 8 and sum(len(c.rows[i]) for i in p) == 64 for p in lc.greedy_layers(c.n, c.rows))
    # check indices that need the 8th bit of their field, on both paths
    assert any(len(r) >= 6 for r in codes["c200_136"].rows[128:])
    mixed = codes["c256_192_mixed"]
    assert any(len(r) >= 6 for r in mixed.rows[128:]), "a check >= 128 on the table path"
    assert any(255 in r[5:] for r in mixed.rows), "variable 255 (the table's unused mark as a byte) behind edge 4"


@pytest.mark.parametrize("name", lc.ACCEPTED)
def test_encode_satisfies_every_check(name):
    code = lc.load(name)
    info = np.random.default_rng(5).integers(0, 2, (64, code.k)).astype(np.uint8)
    info[0], info[1] = 0, 1
    cw = code.encode(info)
    assert cw.shape == (64, code.n) and np.array_equal(cw[:, :code.k], info)
    for row in code.rows:
        assert not (cw[:, row].sum(axis=1) & 1).any()
    assert cw[1:].any(axis=1).all()


@pytest.mark.parametrize("arithmetic", (0, 1))
@pytest.mark.parametrize("name", lc.ACCEPTED)
def test_oracle_decodes_noiseless_words_without_iterating(name, arithmetic):
    code = lc.load(name)
    info, llr = lc.family(code, "noiseless")
    assert code.syndrome_free((llr[:, :code.n] < 0).astype(np.uint8))
    dec = orc.HeaderFecDecoder(code.alist)
    for i in range(0, lc.N_WORDS, 7):
        bits, it = dec.decode(llr[i, :code.n] + llr[i, code.n:], 0, arithmetic)
        assert it == 0 and np.array_equal(bits, info[i])
    hb, invalid = lc.oracle_decode(code, llr, arithmetic, 0)
    assert not invalid.any() and np.array_equal(hb, lc.header_bytes(info))


@pytest.mark.parametrize("arithmetic", (0, 1))
@pytest.mark.parametrize("name", lc.ACCEPTED)
def test_esn0_points_are_what_they_are_chosen_for(name, arithmetic):
    """high: the oracle decodes all 300 to the sent word; waterfall: at least 20 valid and 20 invalid verdicts"""
    code = lc.load(name)
    high, mid, waterfall = lc.ESN0_DB[name]
    assert waterfall < mid < high
    info, llr = lc.family(code, "high")
    hb, invalid = lc.oracle_decode(code, llr, arithmetic, 25)
    assert not invalid.any() and np.array_equal(hb, lc.header_bytes(info))
    _, llr = lc.family(code, "waterfall")
    _, invalid = lc.oracle_decode(code, llr, arithmetic, 25)
    print(name, arithmetic, "waterfall", waterfall, "dB: valid", int((~invalid).sum()), "invalid", int(invalid.sum()))
    assert invalid.sum() >= 20 and (~invalid).sum() >= 20


@pytest.mark.parametrize("name", lc.ACCEPTED)
def test_edge_families_are_what_they_are_chosen_for(name):
    code = lc.load(name)
    _, ties = lc.family(code, "ties")
    assert set(np.unique(np.abs(ties))) == {0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0}
    zero = ties == 0
    assert (np.signbit(ties) & zero).any() and (~np.signbit(ties) & zero).any(), "+0.0 and -0.0"
    acc = ties[:, :code.n] + ties[:, code.n:]
    # the two copies cancel with probability 1/49 (both zero) + 6/49 x 12/49 (equal magnitudes, one sign flipped) = 0.050
    assert (acc == 0).mean() > 0.03, "posteriors of exactly zero"
    assert (np.signbit(acc) & (acc == 0)).any() and (~np.signbit(acc) & (acc == 0)).any()
    # a sum takes one of 13 magnitudes, none likelier than 1/7: two of a check's three or more agree one time in four
    mags = np.abs(acc)
    tie = np.mean([[len(set(w[r])) < len(r) for r in code.rows] for w in mags[:50]])
    assert tie > 0.2, "equal magnitudes within a check"
    _, sat = lc.family(code, "saturation")
    assert np.isfinite(sat).all() and np.abs(sat).max() <= 1e6
    acc = np.abs(sat[:, :code.n] + sat[:, code.n:])
    # past the table's cut and the 8-bit clamp of channel LLRs and messages.  (The 16-bit clamp of a posterior cannot
    # bind: a posterior is a channel LLR plus one message per check of its variable, at most 127 x (1 + 192) < 32767.)
    assert (acc >= 8.0).mean() > 0.9 and (8.0 * acc > 127.0).mean() > 0.9
    _, rnd = lc.family(code, "noncodewords")
    for arithmetic in (0, 1):
        _, invalid = lc.oracle_decode(code, rnd, arithmetic, 25)
        if code.m >= 16:  # (a code with 8 checks accepts one word in 256 outright, and converges to many more)
            assert invalid.mean() > 0.5
