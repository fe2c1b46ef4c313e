#!/usr/bin/env python3
"""wav.scp -> Kaldi MFCC archives on the GPU: what `local/make_mfcc.sh --mfcc-config conf/mfcc.conf` of the reference's recipe makes
with compute-mfcc-feats (feature_pre.sh:92-103, run.sh:74-85: the data/<set>_mfcc directory), and with --vad-config the vad.ark /
vad.scp that compute_vad_decision.sh computes on it - the file the recipe copies next to the fbank features, and what
compute_fbank.py --egs --vad-scp consumes.

The sibling of scripts/compute_fbank.py, with --mfcc-config in place of --fbank-config (without it: compute-mfcc-feats' defaults);
every other flag, the files written (feats.ark, feats.scp, utt2num_frames; vad.ark, vad.scp), the skipping rules, resampling, speed
perturbation, augmented entries and --compress are that script's (the code is shared: scripts/_compute_feats.py).  The frames, the
dither draws and the raw log energy are the fbank's for the same framing options and --seed, so the VAD decisions are the same.

    python scripts/compute_mfcc.py data/train/wav.scp data/train_mfcc --mfcc-config conf/mfcc.conf --vad-config conf/vad.conf
    python scripts/compute_fbank.py data/train/wav.scp out --fbank-config conf/fbank.conf --egs --vad-scp data/train_mfcc/vad.scp
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _compute_feats  # noqa: E402

if __name__ == "__main__":
    _compute_feats.main("mfcc")
