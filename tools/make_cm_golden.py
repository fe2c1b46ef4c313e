#!/usr/bin/env python3
"""Generate tests/golden/cm: small Kaldi compressed matrices ('CM ' records) and what the reference's reader makes of them.

    python tools/make_cm_golden.py --reference /path/to/pytorch-kaldi-resnet

Each case is a seeded matrix (tests/cm_ref.py: make_matrix) compressed by tests/cm_ref.py: compress and written as one record of
cases.ark; cases.json holds per case the key, the kind, the shape and the byte offset of the record's \\0B flag (what an scp line
points at); expected.npz holds the float32 matrix that the reference's scripts/kaldi_io.py: read_mat returns for that record.
The reference's reader divides each segment's width before it multiplies by the code, this project multiplies first (Kaldi's
order): the two differ in the last bits, by at most a few ulp of the matrix's largest magnitude (tests/test_cm_cpu.py).
Only data goes into the fixture."""
import argparse
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "cm")

import cm_ref  # noqa: E402

CASES = [   # kind, rows, cols: rows over {1, 2, 3, 4, 5, 7, 9, 33, 203}, cols over {1, 3, 23, 40, 80}
    ("logmel", 1, 1), ("logmel", 2, 3), ("logmel", 3, 23), ("logmel", 4, 40), ("logmel", 5, 80), ("logmel", 7, 1),
    ("logmel", 9, 3), ("logmel", 33, 23), ("logmel", 203, 80),
    ("cmn", 5, 3), ("cmn", 33, 80), ("cmn", 203, 40),
    ("ties", 4, 3), ("ties", 9, 40), ("ties", 203, 23),
    ("const", 1, 1), ("const", 7, 3), ("const", 33, 23),
    ("constcol", 33, 40), ("constcol", 203, 3),
    ("tight", 3, 3), ("tight", 9, 23), ("tight", 33, 1), ("tight", 203, 40),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (holds scripts/kaldi_io.py)")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_kaldi_io", os.path.join(args.reference, "scripts", "kaldi_io.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261017)
    ark = os.path.join(OUT, "cases.ark")
    index, expected = [], {}
    with open(ark, "wb") as f:
        for kind, rows, cols in CASES:
            key = "%s_%dx%d" % (kind, rows, cols)
            m = cm_ref.make_matrix(kind, rows, cols, rng)
            f.write((key + " ").encode())
            off = f.tell()
            f.write(cm_ref.record(*cm_ref.compress(m)))
            index.append({"key": key, "kind": kind, "rows": rows, "cols": cols, "offset": off})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)      # np.reshape(newshape=) in the reference's reader
        for c in index:
            got = np.asarray(ref.read_mat("%s:%d" % (ark, c["offset"])), dtype=np.float32)
            assert got.shape == (c["rows"], c["cols"]), (c, got.shape)
            expected[c["key"]] = got
    np.savez_compressed(os.path.join(OUT, "expected.npz"), **expected)
    json.dump(index, open(os.path.join(OUT, "cases.json"), "w"), indent=1)
    for n in ("cases.ark", "cases.json", "expected.npz"):
        print(n, os.path.getsize(os.path.join(OUT, n)), "bytes")


if __name__ == "__main__":
    main()
