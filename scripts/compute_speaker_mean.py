#!/usr/bin/env python3
"""usage: compute_speaker_mean.py [--backend host|hip] <ark> <utt2spk> <out>  -> per-speaker mean vectors, the S-norm cohort
(reference scripts/compute_speaker_mean.py: same arguments, same output file, same two print lines)"""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_kaldi_resnet_amd  # noqa: E402,F401
from pytorch_kaldi_resnet_amd import scoring  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["host", "hip"], default="host", help="hip: the per-speaker accumulation runs on the GPU")
    ap.add_argument("ark_file")
    ap.add_argument("utt2spk_file")
    ap.add_argument("mean_file")
    a = ap.parse_args()
    vecs = scoring.read_embeddings(a.ark_file)
    means = scoring.speaker_mean(vecs, a.utt2spk_file, a.mean_file, backend=a.backend)
    print("speakers: {}, feat-dim: {}".format(len(means), vecs.mat.shape[1]))
    print("saved speaker mean in {}".format(a.mean_file))
