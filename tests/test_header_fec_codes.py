"""The header LDPC decoder (csrc/header_blocks.hip: k_header_fec) bit for bit against the serial decoder of oracle/ on
every shape of code gr4pm_header_fec_decoder_create accepts -- tests/_ldpc_codes.py; what each code reaches and the
Es/N0 points are held on the CPU by tests/test_header_fec_codes_ref.py.

The kernel does a layer's checks at once, one lane per edge; its claim is that this IS the serial layered decoder that
visits those checks one by one in float32 (ldpc_decode_impl, oracle/gr4pm_oracle.cpp).  The decoder is no smooth
function of its inputs (a table read at int(8 x), the first of equal minima, 25 iterations that feed every flip back),
so nothing but identity of every header byte and every verdict separates right from wrong.  That the SENT word comes
back is asserted besides, against tests/_ldpc_codes.py's own encoder: kernel and oracle cannot be wrong the same way
about bit order or byte packing."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import _ldpc_codes as lc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GR4PM_ERR_INVALID = -1


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ge.load_package()


@functools.lru_cache(maxsize=None)
def _code(name):
    return lc.load(name)


@functools.lru_cache(maxsize=None)
def _family(name, family):
    info, llr = lc.family(_code(name), family)
    llr.setflags(write=False)
    return info, llr


@functools.lru_cache(maxsize=None)
def _want(name, family, arithmetic, max_iterations):
    """the oracle's header bytes and verdicts: computed once, shared, never written"""
    hb, invalid = lc.oracle_decode(_code(name), _family(name, family)[1], arithmetic, max_iterations)
    hb.setflags(write=False)
    invalid.setflags(write=False)
    return hb, invalid


def _dev(llr):
    return torch.from_numpy(np.array(llr, dtype=np.float32)).cuda()  # (a copy: the shared arrays are read-only)


def _same(got, want, what):
    (got_hb, got_inv), (want_hb, want_inv) = got, want
    assert got_hb.shape == want_hb.shape and got_inv.shape == want_inv.shape, what
    differ = np.flatnonzero((got_inv != want_inv) | (got_hb != want_hb).any(axis=1))
    assert differ.size == 0, (f"{what}: {differ.size} of {want_inv.size} codewords differ from the oracle, the first at {differ[0]}: "
                              f"header {got_hb[differ[0]].tolist()} / {want_hb[differ[0]].tolist()}, "
                              f"invalid {got_inv[differ[0]]} / {want_inv[differ[0]]}")


@pytest.mark.parametrize("max_iterations", (0, 1, 2, 25))
@pytest.mark.parametrize("arithmetic", (0, 1))
@pytest.mark.parametrize("name", lc.ACCEPTED)
def test_decoder_is_the_serial_decoder_bit_for_bit(pkg, name, arithmetic, max_iterations):
    code = _code(name)
    dec = pkg.HeaderFecDecoder(code.alist, max_iterations=max_iterations, arithmetic=arithmetic)
    assert (dec.llrs_per_codeword, dec.header_bytes) == (2 * code.n, code.k // 8)
    for family in lc.FAMILIES:
        info, llr = _family(name, family)
        want = _want(name, family, arithmetic, max_iterations)
        got = dec.process_bulk(_dev(llr))
        _same(got, want, f"{name} arithmetic {arithmetic} max_iterations {max_iterations} {family}")
        if family == "noiseless":  # a codeword is accepted before the first iteration, and it is the word that was sent
            assert not got[1].any() and np.array_equal(got[0], lc.header_bytes(info))
        if max_iterations == 25 and family == "high":
            assert not got[1].any() and np.array_equal(got[0], lc.header_bytes(info))
        if max_iterations == 25 and family == "waterfall":  # (on the oracle's verdicts: both outcomes are compared)
            assert want[1].sum() >= 20 and (~want[1]).sum() >= 20


@pytest.mark.parametrize("name", ("c16_8", "c80_16", "c256_192_mixed"))
def test_output_buffers_grow_and_are_reused(pkg, name):
    """1, then 300, then 1 codewords on one handle"""
    code = _code(name)
    _, llr = _family(name, "waterfall")
    want_hb, want_inv = _want(name, "waterfall", 0, 25)
    dec = pkg.HeaderFecDecoder(code.alist)
    for first, last in ((0, 1), (0, lc.N_WORDS), (lc.N_WORDS - 1, lc.N_WORDS)):
        got = dec.process_bulk(_dev(llr[first:last]))
        _same(got, (want_hb[first:last], want_inv[first:last]), f"{name} codewords {first}..{last}")


def test_two_handles_of_different_codes_used_alternately(pkg):
    names = ("c80_16", "c136_128")
    decs = [pkg.HeaderFecDecoder(_code(n).alist, arithmetic=a) for n, a in zip(names, (0, 1))]
    dev = [_dev(_family(n, "waterfall")[1]) for n in names]
    alone = [d.process_bulk(x) for d, x in zip(decs, dev)]
    for rnd in range(3):
        for i in (0, 1):
            got = decs[i].process_bulk(dev[i])
            _same(got, alone[i], f"{names[i]} round {rnd} against its own single run")
            _same(got, _want(names[i], "waterfall", i, 25), f"{names[i]} round {rnd}")


def test_no_codewords_is_ok_and_touches_nothing(pkg):
    code = _code("c80_16")
    dec = pkg.HeaderFecDecoder(code.alist)
    headers = np.full(64, 0xA5, dtype=np.uint8)
    invalid = np.full(8, 0xA5, dtype=np.uint8)
    x = torch.zeros(2 * code.n, dtype=torch.float32, device="cuda")
    st = pkg.lib().gr4pm_header_fec_decoder_process(dec._h, x.data_ptr(), 0, headers.ctypes.data_as(C.c_void_p),
                                                    invalid.ctypes.data_as(C.c_void_p))
    assert st == 0 and (headers == 0xA5).all() and (invalid == 0xA5).all()
    assert pkg.lib().gr4pm_header_fec_decoder_process(dec._h, None, 0, None, None) == 0
    hb, inv = dec.process_bulk(torch.empty(0, dtype=torch.float32, device="cuda"))
    assert hb.shape == (0, 8) and inv.shape == (0,)
    _same(dec.process_bulk(_dev(_family("c80_16", "mid")[1])), _want("c80_16", "mid", 0, 25), "afterwards")


# ------------------------------------------------------------------ what create refuses
def _staircase(n, m, weight=3):
    return lc.write_alist(n, m, lc.staircase_rows(n, m, [weight] * m, 1))


def _edited(name, edit):
    """the alist of a committed code with its checks changed by edit(rows)"""
    code = _code(name)
    rows = [list(r) for r in code.rows]
    edit(rows)
    return lc.write_alist(code.n, code.m, rows)


def _nine(rows):
    rows[3] = list(range(9))


def _nine_under_a_stated_maximum_of_eight(name):
    lines = _edited(name, _nine).splitlines()
    lines[1] = lines[1].split()[0] + " 8"
    return "\n".join(lines) + "\n"


def _first_tokens(text, count):
    return " ".join(text.split()[:count]) + "\n"


REFUSALS = {
    "all8_256_192": (lambda: _code(lc.REFUSED).alist, "schedule steps do not fit"),
    "n_257": (lambda: _staircase(257, 193), "unsupported code dimensions"),
    "m_193": (lambda: _staircase(249, 193), "unsupported code dimensions"),
    "row_weight_9": (lambda: _edited("c48_8", _nine), "unsupported code dimensions"),
    "row_weight_9_stated_as_8": (lambda: _nine_under_a_stated_maximum_of_eight("c48_8"), "bad row entry"),
    "k_72": (lambda: _staircase(80, 8), "unsupported code dimensions"),
    "k_12": (lambda: _staircase(20, 8), "unsupported code dimensions"),
    "m_equals_n": (lambda: "8 8\n1 1\n" + "1 " * 16 + "\n" + "\n".join(str(i + 1) for i in range(8)) * 2 + "\n",
                   "unsupported code dimensions"),
    "m_above_n": (lambda: "8 16\n1 1\n" + "1 " * 24 + "\n", "unsupported code dimensions"),
    "truncated_in_the_weights": (lambda: _first_tokens(_code("c16_8").alist, 4 + 16 + 5), "truncated"),
    "truncated_in_the_lists": (lambda: _first_tokens(_code("c16_8").alist, len(_code("c16_8").alist.split()) - 3),
                               "list entries"),
    "row_entry_above_n": (lambda: _edited("c16_8", lambda rows: rows[2].__setitem__(1, 16)), "bad row entry"),
    "variable_twice_in_a_row": (lambda: _edited("c48_8", lambda rows: rows[4].__setitem__(6, rows[4][1])),
                                r"check 5 names variable \d+ twice"),
    "variable_twice_on_adjacent_edges": (lambda: _edited("c16_8", lambda rows: rows[0].__setitem__(1, rows[0][0])),
                                         r"check 1 names variable \d+ twice"),
    # a check without variables: among others in the first pass of the layering, as the last check, and as the only
    # check of a code (alone in its pass)
    "zero_weight_row_sharing_a_pass": (lambda: _edited("c16_8", lambda rows: rows.__setitem__(3, [])),
                                       "check 4 has no variables"),
    "zero_weight_row_last": (lambda: _edited("c136_128", lambda rows: rows.__setitem__(127, [])),
                             "check 128 has no variables"),
    "zero_weight_row_alone": (lambda: "9 1\n0 0\n" + "0 " * 9 + "\n0\n", "check 1 has no variables"),
    "zero_weight_row_zero_padded": (lambda: "9 1\n1 2\n" + "0 " * 9 + "\n2\n" + "0\n" * 9 + "0 0\n",
                                    "check 1 has no variables"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_create_refuses(pkg, case):
    make, message = REFUSALS[case]
    alist = make()
    p = pkg._abi.HeaderFecDecoderParams(alist.encode(), 25, None, 0)
    h = C.c_void_p()
    st = pkg.lib().gr4pm_header_fec_decoder_create(C.byref(p), C.byref(h))
    assert st == GR4PM_ERR_INVALID and not h.value
    with pytest.raises(pkg.Gr4pmError, match="status -1: .*" + message):
        pkg.HeaderFecDecoder(alist)
    # and a good create afterwards works
    _, llr = _family("c16_8", "noiseless")
    _same(pkg.HeaderFecDecoder(_code("c16_8").alist).process_bulk(_dev(llr[:4])),
          tuple(a[:4] for a in _want("c16_8", "noiseless", 0, 25)), "a good create after " + case)


# ------------------------------------------------------------------ the callers that are built for 256 LLRs -> 4 bytes
@pytest.mark.parametrize("name, sizes", (("c16_8", "32 LLRs -> 1 header bytes"), ("c80_16", "160 LLRs -> 8 header bytes")))
def test_native_receiver_refuses_a_header_code_of_other_sizes(pkg, name, sizes):
    """an alist the decoder accepts as `header_alist`: create fails cleanly (its buffers hold 4 bytes a codeword),
    and a create with the shipped alist works afterwards"""
    L = pkg.lib()
    for packets_only in (0, 1):
        p = pkg._abi.PacketReceiverParams(4, 4, 9.5, 2, 1 << 16, 256, 0, 1, 1, _code(name).alist.encode(), packets_only)
        h = C.c_void_p()
        assert L.gr4pm_packet_receiver_create(C.byref(p), C.byref(h)) == GR4PM_ERR_INVALID and not h.value
        assert sizes in L.gr4pm_last_error().decode() and "256 -> 4" in L.gr4pm_last_error().decode()
    p = pkg._abi.PacketReceiverParams(4, 4, 9.5, 2, 1 << 16, 256, 0, 1, 1, _code("shipped").alist.encode(), 0)
    assert L.gr4pm_packet_receiver_create(C.byref(p), C.byref(h)) == 0 and h.value
    L.gr4pm_packet_receiver_destroy(h)


def test_gr4_block_refuses_a_header_code_of_other_sizes(tmp_path):
    """HeaderFecDecoder::start() of host/gr4pm_gr4_blocks.hpp through tests/gr4_blocks_driver.cpp: an exception that
    names the sizes; the shipped code starts"""
    ge.build_gr4_driver()
    for name, sizes in (("c16_8", "32 LLRs -> 1 header bytes"), ("c80_16", "160 LLRs -> 8 header bytes")):
        path = tmp_path / (name + ".alist")
        path.write_text(_code(name).alist)
        r = subprocess.run([ge.GR4_DRIVER, "fec_alist", str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and sizes in r.stderr and "256 -> 4" in r.stderr, r.stderr
    path = tmp_path / "shipped.alist"
    path.write_text(_code("shipped").alist)
    r = subprocess.run([ge.GR4_DRIVER, "fec_alist", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "started" in r.stdout, r.stderr
