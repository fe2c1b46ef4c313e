#!/usr/bin/env python3
"""The workload of profiles/r07_resample/: 10 calls of the resampler (512 utterances x 3 s, 44.1 kHz -> 16 kHz) each followed by the
fbank of its output (conf/fbank.conf, dither on), on a resident batch.  Run it under the profiler, the program after `--`:

    rocprofv3 --kernel-trace --stats -d OUT --output-format csv -- python tools/resample_trace.py

Prints one JSON line: CUDA-event times around the Python calls (they include the small H2D copies of the per-row counts; the kernel
times are the profiler's), the bytes the resampler has to move and the time those take at the chip's measured streaming rate."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STREAM_TBS = 6.0        # streaming reads / writes of this chip, measured


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--input-rate", type=int, default=44100)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features
    from wav_extract_bench import synth
    fi, fo, B = args.input_rate, 16000, args.batch
    N = int(args.seconds * fi)
    rng = np.random.default_rng(1)
    base = np.stack([synth(rng, N, fi) for _ in range(8)]).astype(np.float32)
    wave = torch.from_numpy(base[np.arange(B) % 8] + rng.normal(0, 20, (B, 1)).astype(np.float32)).cuda()
    nsamp = np.full(B, N, dtype=np.int64)
    ids = np.arange(B, dtype=np.int64)
    fb = features.FbankOptions(num_mel_bins=40, high_freq=7600, snip_edges=False)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_rs, t_fb = [], []
    for _ in range(args.calls):
        ev[0].record()
        w16, n16 = features.resample(wave, nsamp, fi, fo)
        ev[1].record()
        features.fbank(w16, n16, fb, ids, 0)
        ev[2].record()
        torch.cuda.synchronize()
        t_rs.append(ev[0].elapsed_time(ev[1]))
        t_fb.append(ev[1].elapsed_time(ev[2]))
    nbytes = 4 * B * (N + int(n16[0]))
    print(json.dumps({"batch": B, "seconds": args.seconds, "fi": fi, "fo": fo, "calls": args.calls,
                      "resample_call_ms_min": min(t_rs[1:]), "fbank_call_ms_min": min(t_fb[1:]),
                      "bytes_in": 4 * B * N, "bytes_out": 4 * B * int(n16[0]),
                      "byte_floor_us_at_%.1f_TBs" % STREAM_TBS: nbytes / (STREAM_TBS * 1e12) * 1e6,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
