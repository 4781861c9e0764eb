"""Small LDPC codes that reach every path of the header decoder (csrc/header_blocks.hip: k_header_fec), with an encoder
that needs no generator matrix.

Construction: the first k = n - m variables are the information bits; check c holds parity variable k + c and, for c > 0,
k + c - 1 (a staircase: encoding is one running XOR), plus deg[c] minus those distinct information variables drawn from
repeated random permutations of 0..k-1 (every information bit is covered); the order of the variables within a row is
shuffled, so the parity variables land on every edge position.

The alists are committed under tests/golden/ldpc/ (written by tests/golden/make_ldpc_codes.py): the tests read those,
a change of numpy's random stream does not move the codes.

Test infrastructure only.
"""
import os

import numpy as np

LDPC_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ldpc")


def staircase_rows(n, m, deg, seed, draw_order=None):
    """rows[c]: the 0-based variables of check c in edge order.  deg: one weight per check.  draw_order: the order in
    which the checks take their information variables from the stream of permutations (default: index order; checks
    that draw next to each other from one permutation share no information variable)"""
    k = n - m
    rng = np.random.default_rng(seed)
    pool = []
    rows = [None] * m
    for c in (draw_order or range(m)):
        row = [k + c] + ([k + c - 1] if c else [])
        info = []
        while len(info) < deg[c] - len(row):
            if not pool:
                pool = [int(v) for v in rng.permutation(k)]
            # the first of the stream that this row does not hold yet (a row that spans two permutations)
            at = next((i for i, v in enumerate(pool) if v not in info), None)
            if at is None:
                pool += [int(v) for v in rng.permutation(k)]
                continue
            info.append(pool.pop(at))
        row += info
        rows[c] = [row[i] for i in rng.permutation(len(row))]
    return rows


def write_alist(n, m, rows):
    """alist text (unpadded lists, 1-based) of the code whose checks are `rows`"""
    cols = [[] for _ in range(n)]
    for c, row in enumerate(rows):
        for v in row:
            if 0 <= v < n:
                cols[v].append(c)
    lines = [f"{n} {m}", f"{max(len(c) for c in cols)} {max(len(r) for r in rows)}",
             " ".join(str(len(c)) for c in cols), " ".join(str(len(r)) for r in rows)]
    lines += [" ".join(str(c + 1) for c in col) for col in cols]
    lines += [" ".join(str(v + 1) for v in row) for row in rows]
    return "\n".join(lines) + "\n"


def read_alist(text):
    """(n, m, rows) of an unpadded or zero-padded alist"""
    v = [int(t) for t in text.split()]
    n, m, max_col, max_row = v[:4]
    colw, roww = v[4:4 + n], v[4 + n:4 + n + m]
    rest = v[4 + n + m:]
    padded = len(rest) == n * max_col + m * max_row
    assert padded or len(rest) == sum(colw) + sum(roww)
    at = n * max_col if padded else sum(colw)
    rows = []
    for c in range(m):
        cnt = max_row if padded else roww[c]
        rows.append([x - 1 for x in rest[at:at + cnt] if x > 0])
        at += cnt
    return n, m, rows


def greedy_layers(n, rows):
    """the decoder's layering restated: scan the checks not yet placed in index order, take every one that shares no
    variable with those already taken in this pass, at most 64 edges a pass.  Returns the passes (lists of checks)."""
    placed = [False] * len(rows)
    passes = []
    while not all(placed):
        used, lanes, taken = set(), 0, []
        for c, row in enumerate(rows):
            if placed[c] or lanes + len(row) > 64 or used & set(row):
                continue
            used |= set(row)
            lanes += len(row)
            placed[c] = True
            taken.append(c)
        assert taken, "a check wider than a pass"
        passes.append(taken)
    return passes


def greedy_steps(n, rows):
    return len(greedy_layers(n, rows))


class Code:
    def __init__(self, name, text):
        self.name, self.alist = name, text
        self.n, self.m, self.rows = read_alist(text)
        self.k = self.n - self.m

    def encode(self, info_bits):
        """[N, k] bits -> [N, n] codewords: p_0 = the XOR of check 0's information bits, p_c = p_(c-1) ^ check c's"""
        info = np.asarray(info_bits, dtype=np.uint8).reshape(-1, self.k)
        cw = np.zeros((info.shape[0], self.n), dtype=np.uint8)
        cw[:, :self.k] = info
        run = np.zeros(info.shape[0], dtype=np.uint8)
        for c, row in enumerate(self.rows):
            for v in row:
                if v < self.k:
                    run = run ^ info[:, v]
            cw[:, self.k + c] = run
        return cw

    def syndrome_free(self, codewords):
        cw = np.asarray(codewords, dtype=np.uint8).reshape(-1, self.n)
        return all(not (cw[:, row].sum(axis=1) & 1).any() for row in self.rows)

    def steps(self):
        return greedy_steps(self.n, self.rows)


class ShippedCode(Code):
    """the package's (128, 32) header code: no staircase, encoded with its dense generator
    (tests/golden/header_ldpc_generator.npy: parity bit j = parity(info word & generator[j]), info MSB first)"""

    def encode(self, info_bits):
        gen = np.load(os.path.join(os.path.dirname(LDPC_DIR), "header_ldpc_generator.npy")).astype(np.uint32)
        g = ((gen[:, None] >> (31 - np.arange(32, dtype=np.uint32))[None, :]) & 1).astype(np.uint8)  # [96, 32]
        info = np.asarray(info_bits, dtype=np.uint8).reshape(-1, 32)
        return np.concatenate([info, (info.astype(np.int64) @ g.T.astype(np.int64) & 1).astype(np.uint8)], axis=1)


def load(name):
    """a committed code: tests/golden/ldpc/<name>.alist ("shipped": the package's (128, 32) header code)"""
    if name == "shipped":
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        with open(os.path.join(root, "gr4-packet-modem_amd", "data", "header_ldpc_128_32.alist")) as f:
            return ShippedCode(name, f.read())
    with open(os.path.join(LDPC_DIR, name + ".alist")) as f:
        return Code(name, f.read())


# the codes the decoder accepts, smallest first, and the one it must refuse
ACCEPTED = ("c16_8", "c48_8", "c80_16", "c136_128", "c200_136", "c256_192_mixed", "shipped")
REFUSED = "c256_192_all8"

# ------------------------------------------------------------------ the inputs both test files decode
N_WORDS = 300
LLR_SCALE = 2.0 / 0.7**2  # the receiver's fixed noise_sigma, packet_receiver.hpp:129
# Es/N0 in dB per code: (every word decodes, between, inside the waterfall: >= 20 valid and >= 20 invalid verdicts of
# the 300 in either arithmetic).  Chosen with the oracle alone; tests/test_header_fec_codes_ref.py holds them to that.
ESN0_DB = {
    "c16_8": (8.0, 1.0, -6.0),
    "c48_8": (9.0, 5.0, 1.0),
    "c80_16": (9.0, 5.0, 1.0),
    "c136_128": (8.0, 0.0, -8.0),
    "c200_136": (8.0, 2.0, -3.0),
    "c256_192_mixed": (8.0, 2.0, -3.0),
    "shipped": (8.0, 2.0, -4.0),
}
FAMILIES = ("noiseless", "high", "mid", "waterfall", "ties", "saturation", "noncodewords")


def _rng(code, family):
    return np.random.default_rng(7000 + 100 * ACCEPTED.index(code.name) + FAMILIES.index(family))


def _awgn(code, rng, esn0_db):
    info = rng.integers(0, 2, (N_WORDS, code.k)).astype(np.uint8)
    tx = np.tile(1.0 - 2.0 * code.encode(info), 2) * np.sqrt(0.5)  # the codeword twice: the header's repetition code
    sigma = np.sqrt(0.5 / 10 ** (esn0_db / 10))
    return info, (LLR_SCALE * (tx + sigma * rng.standard_normal(tx.shape))).astype(np.float32)


def family(code, name):
    """(information bits [N_WORDS, k] or None where no word was sent, LLRs [N_WORDS, 2 n] float32)"""
    rng = _rng(code, name)
    high, mid, waterfall = ESN0_DB[code.name]
    if name == "noiseless":
        info = rng.integers(0, 2, (N_WORDS, code.k)).astype(np.uint8)
        return info, np.tile(1.0 - 2.0 * code.encode(info), 2).astype(np.float32)
    if name in ("high", "mid", "waterfall"):
        return _awgn(code, rng, {"high": high, "mid": mid, "waterfall": waterfall}[name])
    if name == "ties":
        # multiples of 0.5 in [-3, 3] with both zeros, signed like an encoded word but for one LLR in seven: many equal
        # magnitudes within a check (the first minimum wins) and sums of the two copies that are exactly +0 or -0
        info = rng.integers(0, 2, (N_WORDS, code.k)).astype(np.uint8)
        sign = np.tile(1.0 - 2.0 * code.encode(info), 2) * np.where(rng.random((N_WORDS, 2 * code.n)) < 1 / 7, -1.0, 1.0)
        return None, (sign * 0.5 * rng.integers(0, 7, sign.shape)).astype(np.float32)  # (-1 * 0 = -0.0)
    if name == "saturation":
        # far past the correction table's cut (x >= 8) and, in the 8-bit form, the +-127 and 16-bit clamps; finite
        _, llr = _awgn(code, rng, mid)
        llr = llr * np.float32(40.0)
        assert np.abs(llr).max() <= 1e6
        return None, llr
    if name == "noncodewords":
        _, llr = _awgn(code, rng, mid)
        return None, (np.abs(llr) * np.where(rng.random(llr.shape) < 0.5, -1.0, 1.0)).astype(np.float32)
    raise KeyError(name)


def header_bytes(info_bits):
    """k bits -> k / 8 bytes, MSB first (header_fec_decoder.hpp:329-335)"""
    return np.packbits(np.asarray(info_bits, dtype=np.uint8), axis=-1)


_ORACLE = {}


def oracle_decode(code, llrs, arithmetic, max_iterations):
    """the serial decoder of oracle/ over [N, 2 n] LLRs: (header bytes [N, k / 8], invalid [N] bool).  The two copies
    of a codeword are added here, in float32 (header_fec_decoder.hpp:308-312)"""
    import _oracle as orc
    if code.name not in _ORACLE:
        _ORACLE[code.name] = orc.HeaderFecDecoder(code.alist)
    dec = _ORACLE[code.name]
    x = np.asarray(llrs, dtype=np.float32).reshape(-1, 2 * code.n)
    acc = x[:, :code.n] + x[:, code.n:]
    assert acc.dtype == np.float32
    bits = np.empty((x.shape[0], code.k), dtype=np.uint8)
    invalid = np.empty(x.shape[0], dtype=bool)
    for i in range(x.shape[0]):
        bits[i], it = dec.decode(acc[i], max_iterations, arithmetic)
        invalid[i] = it < 0
    return header_bytes(bits), invalid
