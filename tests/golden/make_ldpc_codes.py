#!/usr/bin/env python3
"""Writes tests/golden/ldpc/*.alist: the codes of tests/_ldpc_codes.py (construction and reasons there and in
tests/test_header_fec_codes_ref.py).  Needs nothing but numpy.  The committed files are what the tests read; run this
only to add a code -- another numpy may draw other codes, and the Es/N0 points pinned in the tests belong to these.

For every code the first seed is taken at which the stated condition holds.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _ldpc_codes as lc  # noqa: E402


def weights(m, lo, hi, seed):
    """one weight per check, lo..hi, every value present"""
    rng = np.random.default_rng(1000 + seed)
    deg = rng.integers(lo, hi + 1, m)
    deg[rng.permutation(m)[: hi - lo + 1]] = np.arange(lo, hi + 1)
    return [int(d) for d in deg]


def steps_in(lo, hi):
    return lambda n, rows: lo <= lc.greedy_steps(n, rows) <= hi


def table_edges(n, rows):
    """edges 5, 6 and 7 (read from the table, not from the schedule entry) each hold a parity and an information variable"""
    k = n - len(rows)
    return lc.greedy_steps(n, rows) <= 24 and all(
        any(len(r) > e and r[e] >= k for r in rows) and any(len(r) > e and r[e] < k for r in rows) for e in (5, 6, 7))


def full_step(n, rows):
    """a pass of eight weight-8 checks: all 64 lanes of a step busy"""
    return table_edges(n, rows) and any(sum(len(rows[c]) for c in p) == 64 for p in lc.greedy_layers(n, rows))


def mixed_limits(n, rows):
    """23 or 24 steps; variable 255 on the table path (edge >= 5); a check >= 128 of weight >= 6"""
    return (23 <= lc.greedy_steps(n, rows) <= 24 and table_edges(n, rows) and any(255 in row[5:] for row in rows)
            and any(len(row) >= 6 for row in rows[128:]))


# c80_16 draws for its even checks first: they are no staircase neighbours and take 7 + 7 x 6 = 49 information variables
# of one permutation of 64, so the first pass holds all eight of them
EVEN_FIRST = list(range(0, 16, 2)) + list(range(1, 16, 2))
CODES = [  # name, n, m, lowest and highest row weight, condition, draw order
    ("c16_8", 16, 8, 3, 4, steps_in(1, 24), None),
    ("c48_8", 48, 8, 7, 8, table_edges, None),
    ("c80_16", 80, 16, 8, 8, full_step, EVEN_FIRST),
    ("c136_128", 136, 128, 3, 3, steps_in(1, 24), None),
    ("c200_136", 200, 136, 5, 7, lambda n, rows: steps_in(1, 24)(n, rows) and any(len(r) >= 6 for r in rows[128:]), None),
    ("c256_192_mixed", 256, 192, 4, 8, mixed_limits, None),
    ("c256_192_all8", 256, 192, 8, 8, steps_in(25, 192), None),
]


def main():
    os.makedirs(lc.LDPC_DIR, exist_ok=True)
    for name, n, m, lo, hi, ok, order in CODES:
        for seed in range(200):
            rows = lc.staircase_rows(n, m, weights(m, lo, hi, seed), seed, order)
            if ok(n, rows):
                break
        else:
            raise SystemExit(f"{name}: no seed below 200 meets the condition")
        with open(os.path.join(lc.LDPC_DIR, name + ".alist"), "w") as f:
            f.write(lc.write_alist(n, m, rows))
        print(f"{name}: seed {seed}, {lc.greedy_steps(n, rows)} steps, weights {min(map(len, rows))}-{max(map(len, rows))}")


if __name__ == "__main__":
    main()
