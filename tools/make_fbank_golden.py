#!/usr/bin/env python3
"""Generate tests/golden/fbank/*.npz: Kaldi fbank + raw log energy computed by the reference's kaldi.py (a copy of torchaudio's
Kaldi-compliance module) on seeded int16 test signals, pinning tests/frontend_ref.py.

    python tools/make_fbank_golden.py --reference /path/to/pytorch-kaldi-resnet

kaldi.py imports torchaudio (only needed for its MFCC DCT) and calls the removed torch.rfft: a stub module and an adapter over
torch.fft.rfft are injected.  The default dtype is float64, because kaldi.py builds its window and mel tables in the default dtype
(in float32 the tables alone differ from fp64 by ~1.5e-4).  Dither is 0 (deterministic); every case is written as int16 samples
and float32 expected outputs."""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "fbank")


def load_reference_kaldi(ref_dir):
    sys.modules.setdefault("torchaudio", types.ModuleType("torchaudio"))
    if not hasattr(torch, "rfft"):
        def rfft(x, signal_ndim, normalized=False, onesided=True):
            assert signal_ndim == 1 and not normalized and onesided
            return torch.view_as_real(torch.fft.rfft(x, dim=-1))
        torch.rfft = rfft
    spec = importlib.util.spec_from_file_location("ref_kaldi", os.path.join(ref_dir, "kaldi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def speechlike(rng, fs, seconds):
    """voiced-like harmonic bursts with noise, a digital-zero stretch, a DC-offset quiet stretch and a clipped loud stretch"""
    n = int(fs * seconds)
    t = np.arange(n) / fs
    x = np.zeros(n)
    f0 = 120 + 30 * np.sin(2 * np.pi * 1.5 * t)
    ph = 2 * np.pi * np.cumsum(f0) / fs
    for h in range(1, 12):
        x += (0.6 / h) * np.sin(h * ph)
    env = (np.sin(2 * np.pi * 2.0 * t) > -0.2).astype(float)
    x = 3000 * x * env + rng.normal(0, 200, n)
    q = n // 8
    x[q:2 * q] = 0.0                                     # digital zero
    x[3 * q:4 * q] = 2000.0 + rng.normal(0, 3, q)        # quiet with a DC offset
    x[5 * q:6 * q] *= 20.0                               # clipped below
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


CASES = [
    # name, fs, seconds, fbank options (dither 0 throughout)
    ("conf16k_f40", 16000, 0.61, dict(num_mel_bins=40, high_freq=7600, snip_edges=False)),   # conf/fbank.conf
    ("snip_f80", 16000, 0.5, dict(num_mel_bins=80, snip_edges=True)),
    ("nosnip_f80", 16000, 0.503, dict(num_mel_bins=80, snip_edges=False)),
    ("hamming_f40", 16000, 0.4, dict(num_mel_bins=40, window_type="hamming")),
    ("hanning_f40", 16000, 0.4, dict(num_mel_bins=40, window_type="hanning", snip_edges=False)),
    ("rect_f40", 16000, 0.4, dict(num_mel_bins=40, window_type="rectangular")),
    ("blackman_f40", 16000, 0.4, dict(num_mel_bins=40, window_type="blackman", snip_edges=False)),
    ("fs8k_f40", 8000, 0.8, dict(num_mel_bins=40, sample_frequency=8000.0, low_freq=20, high_freq=-200)),
    ("fs8k_snip_f23", 8000, 0.6, dict(sample_frequency=8000.0, snip_edges=True, energy_floor=1.0)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (holds kaldi.py)")
    args = ap.parse_args()
    torch.set_default_dtype(torch.float64)
    K = load_reference_kaldi(args.reference)
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261016)
    index = []
    for name, fs, sec, opts in CASES:
        x = speechlike(rng, fs, sec)
        kw = dict(dither=0.0, sample_frequency=float(fs))
        kw.update(opts)
        wav = torch.from_numpy(x.astype(np.float64))[None, :]
        feats = K.fbank(wav, **kw)
        wf, shift, size, padded = K._get_waveform_and_window_properties(
            wav, -1, kw["sample_frequency"], kw.get("frame_shift", 10.0), kw.get("frame_length", 25.0), True,
            kw.get("preemphasis_coefficient", 0.97))
        _, loge = K._get_window(wf, padded, size, shift, kw.get("window_type", "povey"), kw.get("blackman_coeff", 0.42),
                                kw.get("snip_edges", True), True, kw.get("energy_floor", 0.0), 0.0, True,
                                kw.get("preemphasis_coefficient", 0.97))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), wave=x, fbank=feats.numpy().astype(np.float32),
                            log_energy=loge.numpy().astype(np.float32), options=json.dumps(kw))
        index.append(name)
        print(name, tuple(feats.shape), os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")
    json.dump(index, open(os.path.join(OUT, "cases.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
