#!/usr/bin/env python3
"""Generate tests/golden/resample/*.npz: Kaldi's LinearResample as the reference's kaldi.py computes it (resample_waveform) on
seeded int16 test signals, pinning tests/resample_ref.py.

    python tools/make_resample_golden.py --reference /path/to/pytorch-kaldi-resnet

kaldi.py is loaded as tools/make_fbank_golden.py loads it; it also calls fractions.gcd, which Python 3.9 removed: math.gcd is put
in its place.  The default dtype is float64 (kaldi.py builds its filter table in the default dtype).  Every case is written as
int16 samples and the float64 output.  The lengths are chosen so that both branches of the output-length rule occur: n * ou
divisible by iu (the last tick falls on the end of the interval and is dropped) and not."""
import argparse
import fractions
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "resample")

from make_fbank_golden import load_reference_kaldi, speechlike  # noqa: E402

CASES = [
    # name, input rate, output rate, samples (exact: n * ou % iu == 0)
    ("r44100_16000", 44100, 16000, 4410),        # exact: 10 units
    ("r44100_16000_odd", 44100, 16000, 5003),
    ("r48000_16000", 48000, 16000, 4800),        # exact
    ("r48000_16000_odd", 48000, 16000, 4801),
    ("r22050_16000", 22050, 16000, 3001),
    ("r11025_16000", 11025, 16000, 2205),        # exact: 5 units
    ("r11025_16000_odd", 11025, 16000, 2500),
    ("r8000_16000", 8000, 16000, 2000),          # upsampling by 2: always exact
    ("r16000_8000", 16000, 8000, 4000),          # exact
    ("r16000_8000_odd", 16000, 8000, 4001),
    ("r14400_16000", 14400, 16000, 3600),        # speed 0.9; exact
    ("r14400_16000_odd", 14400, 16000, 3607),
    ("r17600_16000", 17600, 16000, 4400),        # speed 1.1; exact
    ("r17600_16000_odd", 17600, 16000, 4405),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (holds kaldi.py)")
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    if not hasattr(fractions, "gcd"):
        fractions.gcd = math.gcd
    K = load_reference_kaldi(args.reference)
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261017)
    index = []
    for name, fi, fo, n in CASES:
        x = speechlike(rng, fi, (n + 0.5) / fi)
        assert len(x) == n, (name, len(x), n)
        y = K.resample_waveform(torch.from_numpy(x.astype(np.float64))[None, :], float(fi), float(fo))[0].numpy()
        g = math.gcd(fi, fo)
        exact = (n * (fo // g)) % (fi // g) == 0
        np.savez_compressed(os.path.join(OUT, name + ".npz"), wave=x, out=y.astype(np.float64))
        index.append({"name": name, "fi": fi, "fo": fo, "n": n, "n_out": int(y.shape[0]), "exact_division": bool(exact)})
        print(name, n, "->", y.shape[0], "exact" if exact else "inexact", os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")
    json.dump(index, open(os.path.join(OUT, "cases.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
