#!/usr/bin/env python3
"""PLDA on the projected, length-normalised training embeddings: the work of Kaldi's `ivector-subtract-global-mean | transform-vec |
ivector-normalize-length | ivector-compute-plda` in the reference's recipes.  Writes Kaldi's binary Plda object."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_kaldi_resnet_amd  # noqa: E402,F401
from pytorch_kaldi_resnet_amd import kaldi_io, plda, scoring  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-em-iters", type=int, default=10)
    ap.add_argument("--mean", type=str, default=None, help="global mean to subtract (default: the mean of the archive itself)")
    ap.add_argument("--backend", choices=["host", "hip"], default="host", help="hip: projection, class means, scatter matrices and the EM passes on the GPU")
    ap.add_argument("ark")
    ap.add_argument("utt2spk")
    ap.add_argument("transform")
    ap.add_argument("plda")
    a = ap.parse_args()
    mean = kaldi_io.read_vec_flt(a.mean) if a.mean else None
    m, T, psi = plda.compute_plda(scoring.read_embeddings(a.ark), plda.read_utt2spk(a.utt2spk), plda.read_transform(a.transform),
                                  a.num_em_iters, mean, a.backend, a.plda)
    print("PLDA: {} dimensions, psi {} ... {}; wrote {}".format(len(psi), psi[0], psi[-1], a.plda))
