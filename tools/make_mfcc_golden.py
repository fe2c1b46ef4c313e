#!/usr/bin/env python3
"""Generate tests/golden/mfcc/*.npz: Kaldi MFCCs computed by the reference's kaldi.py mfcc() (a copy of torchaudio's
Kaldi-compliance module) on seeded int16 test signals, pinning tests/mfcc_ref.py.

    python tools/make_mfcc_golden.py --reference /path/to/pytorch-kaldi-resnet

As tools/make_fbank_golden.py: a stub torchaudio module and an adapter for the removed torch.rfft are injected, and the default dtype
is float64.  kaldi.py takes its DCT from torchaudio.functional.create_dct(n, n, 'ortho'), which the stub supplies from
scipy.fft.dct(eye(n), norm='ortho') (the same orthonormal DCT-II, as a right-multiply matrix).  Dither is 0; every case is written as
int16 samples, float64 expected MFCCs and the options as JSON."""
import argparse
import json
import os
import sys
import types

import numpy as np
import scipy.fft
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_fbank_golden import load_reference_kaldi, speechlike  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mfcc")


def stub_torchaudio():
    ta = sys.modules.setdefault("torchaudio", types.ModuleType("torchaudio"))
    fn = types.ModuleType("torchaudio.functional")

    def create_dct(n_mfcc, n_mels, norm):
        assert norm == "ortho"
        # [n_mels, n_mfcc]: column k is basis k of the DCT-II
        return torch.from_numpy(scipy.fft.dct(np.eye(n_mels), type=2, norm="ortho", axis=0).T[:, :n_mfcc].copy())
    fn.create_dct = create_dct
    ta.functional = fn
    sys.modules["torchaudio.functional"] = fn


CASES = [
    # name, fs, seconds, mfcc options (dither 0 throughout; use_energy and htk_compat always stated)
    ("conf16k_c40", 16000, 0.61, dict(num_mel_bins=40, num_ceps=40, snip_edges=False, high_freq=7600,
                                      use_energy=True, htk_compat=False)),                               # conf/mfcc.conf
    ("default_c13", 16000, 0.5, dict(num_mel_bins=23, num_ceps=13, use_energy=True, htk_compat=False)),
    ("htk_f80_c72", 16000, 0.45, dict(num_mel_bins=80, num_ceps=72, use_energy=False, htk_compat=True)),
    ("nolifter_c30", 16000, 0.503, dict(num_mel_bins=30, num_ceps=30, cepstral_lifter=0.0, use_energy=False, htk_compat=False,
                                        energy_floor=1.0)),
    ("htk_c1", 16000, 0.4, dict(num_mel_bins=24, num_ceps=1, use_energy=True, htk_compat=True)),
    ("htk_energy_c30", 16000, 0.52, dict(num_mel_bins=40, num_ceps=30, use_energy=True, htk_compat=True)),
    ("fs8k_c20", 8000, 0.8, dict(num_mel_bins=40, num_ceps=20, use_energy=False, htk_compat=False, high_freq=-200)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (holds kaldi.py)")
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    stub_torchaudio()
    K = load_reference_kaldi(args.reference)
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261019)
    index = []
    for name, fs, sec, opts in CASES:
        x = speechlike(rng, fs, sec)
        kw = dict(dither=0.0, sample_frequency=float(fs), cepstral_lifter=22.0)
        kw.update(opts)
        feats = K.mfcc(torch.from_numpy(x.astype(np.float64))[None, :], **kw)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, wave=x, mfcc=feats.numpy().astype(np.float64), options=json.dumps(kw))
        index.append(name)
        print(name, tuple(feats.shape), os.path.getsize(path), "bytes")
    json.dump(index, open(os.path.join(OUT, "cases.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
