#!/usr/bin/env python3
"""Regenerates tests/golden/row_resampler_digests.json: the SHA-256 of the raw output bytes of the RowResampler and the
StreamRowResampler on the inputs that tests/test_row_resampler_digests.py names.

Needs the built library and an MI355X.  The cases, their inputs and the order of the bytes are the test's own (OUTPUTS
and digest() there), run through the public classes; only the digests are written, with the commit whose library made
them (the first argument).  The file was first written from the commit before k_row_resample and k_row_stream became two
instantiations of one body, and a run on a later tree must rewrite its digests byte for byte.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import test_row_resampler_digests as cases  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: make_row_resampler_digests.py COMMIT")
    digests = {}
    for key in sorted(cases.OUTPUTS):
        digests[key] = cases.digest(key)
        print(key, digests[key], flush=True)
    with open(cases.GOLDEN, "w") as f:
        json.dump({"device": "MI355X", "commit": sys.argv[1], "digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
