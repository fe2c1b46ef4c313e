#!/usr/bin/env python3
"""spk_mfcc_fwd against spk_fbank_fwd at the same options and batch (MFCC, Cost): --calls alternating calls of
features.fbank and features.mfcc on a resident batch (512 utterances x 3 s, the framing of conf/fbank.conf / conf/mfcc.conf, 40 mel
bins, 40 cepstra, dither on; --num-ceps / --num-mel-bins / --dither for other points).  Run it under the profiler, the program after
`--`, for the kernel times (fbank_kernel, mfcc_kernel):

    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python tools/mfcc_trace.py

Prints one JSON line: CUDA-event times around the Python calls (they include the small H2D copies of the per-row counts and ids;
the kernel times are the profiler's), and the largest difference between the log energies of the two (0: the same frames)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--num-mel-bins", type=int, default=40)
    ap.add_argument("--num-ceps", type=int, default=40)
    ap.add_argument("--dither", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features
    from wav_extract_bench import synth
    fs, B = 16000, args.batch
    N = int(args.seconds * fs)
    rng = np.random.default_rng(1)
    base = np.stack([synth(rng, N, fs) for _ in range(8)]).astype(np.float32)
    wave = torch.from_numpy(base[np.arange(B) % 8] + rng.normal(0, 20, (B, 1)).astype(np.float32)).cuda()
    nsamp = np.full(B, N, dtype=np.int64)
    ids = np.arange(B, dtype=np.int64)
    common = dict(num_mel_bins=args.num_mel_bins, high_freq=7600, snip_edges=False, dither=args.dither)
    fb = features.FbankOptions(**common)
    mf = features.MfccOptions(num_ceps=args.num_ceps, **common)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_fb, t_mf = [], []
    for _ in range(args.calls):
        ev[0].record()
        _, _, e_fb = features.fbank(wave, nsamp, fb, ids, 0)
        ev[1].record()
        _, _, e_mf = features.mfcc(wave, nsamp, mf, ids, 0)
        ev[2].record()
        torch.cuda.synchronize()
        t_fb.append(ev[0].elapsed_time(ev[1]))
        t_mf.append(ev[1].elapsed_time(ev[2]))
    print(json.dumps({"batch": B, "seconds": args.seconds, "num_mel_bins": args.num_mel_bins, "num_ceps": args.num_ceps,
                      "dither": args.dither, "calls": args.calls,
                      "fbank_call_ms_min": min(t_fb[1:]), "fbank_call_ms_median": float(np.median(t_fb[1:])),
                      "mfcc_call_ms_min": min(t_mf[1:]), "mfcc_call_ms_median": float(np.median(t_mf[1:])),
                      "log_energy_max_abs_diff": float((e_fb - e_mf).abs().max()),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
