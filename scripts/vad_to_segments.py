#!/usr/bin/env python3
"""VAD decisions -> a Kaldi segments file: reads the vad.scp that compute_fbank.py / compute_mfcc.py
--vad-config write (one 0/1 vector per recording) and writes '<recording>-<start:08d>-<end:08d> <recording> <start s> <end s>' lines
(frame indices of the recording, end exclusive) - the file `decode.py --segments` takes.  The rule (include/spkhip.h:
spk_vad_segments): every run of voiced frames padded by --seg-padding, padded runs at most --seg-max-gap apart joined, segments shorter
than --seg-min-length dropped.  --backend host runs it in numpy (ingest.segments_from_vad), --backend hip on the GPU
(features.vad_segments); both write the same bytes."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("vad_scp")
    ap.add_argument("out", help="the segments file to write")
    ap.add_argument("--backend", choices=["host", "hip"], default="host")
    ap.add_argument("--frame-shift", type=float, default=0.01, help="seconds per frame, for the times written (default 0.01)")
    ap.add_argument("--seg-padding", type=int, default=None, help="frames added on both sides of a voiced run (default 10)")
    ap.add_argument("--seg-max-gap", type=int, default=None, help="padded runs at most this many frames apart are joined (default 30)")
    ap.add_argument("--seg-min-length", type=int, default=None, help="segments shorter than this are dropped (default 50)")
    ap.add_argument("--batch-size", type=int, default=64, help="recordings per launch with --backend hip")
    a = ap.parse_args(argv)
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features, ingest, kaldi_io
    d = features.SegmentOptions()
    try:
        opts = features.SegmentOptions(padding=d.padding if a.seg_padding is None else a.seg_padding,
                                       max_gap=d.max_gap if a.seg_max_gap is None else a.seg_max_gap,
                                       min_length=d.min_length if a.seg_min_length is None else a.seg_min_length)
    except ValueError as e:
        ap.error(str(e))
    if a.frame_shift <= 0 or a.batch_size < 1:
        ap.error("--frame-shift must be positive and --batch-size at least 1")
    try:
        tab = [l.split(None, 1) for l in open(a.vad_scp) if l.strip()]
        names = [k for k, _ in tab]
        vads = [(kaldi_io.read_vec_flt(rx.strip()) != 0).astype(np.int32) for _, rx in tab]
    except (OSError, ValueError) as e:
        ap.error("%s: %s" % (a.vad_scp, e))
    nseg = 0
    with open(a.out, "w") as f:
        for i in range(0, len(names), a.batch_size):
            rows = vads[i:i + a.batch_size]
            T = np.array([len(v) for v in rows], dtype=np.int64)
            v = np.zeros((len(rows), max(int(T.max()), 1)), dtype=np.int32)
            for b, r in enumerate(rows):
                v[b, :len(r)] = r
            if a.backend == "hip":
                import torch
                row, start, end = features.vad_segments(torch.from_numpy(v).cuda(), T, opts)
            else:
                row, start, end = ingest.segments_from_vad(v, T, opts)
            for b, s, e in zip(row, start, end):
                k = names[i + b]
                f.write("%s-%08d-%08d %s %.3f %.3f\n" % (k, s, e, k, s * a.frame_shift, e * a.frame_shift))
            nseg += len(row)
    print("vad_to_segments: %d segments of %d recordings to %s" % (nseg, len(names), a.out))


if __name__ == "__main__":
    main()
