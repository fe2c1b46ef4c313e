#!/usr/bin/env python3
"""LDA on the training embeddings: the work of Kaldi's `ivector-subtract-global-mean | ivector-compute-lda` in the reference's
recipes (run_aam_v2.sh: --total-covariance-factor=0.0 --dim=200).  Writes a Kaldi binary matrix [dim][D+1]."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_kaldi_resnet_amd  # noqa: E402,F401
from pytorch_kaldi_resnet_amd import kaldi_io, plda, scoring  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--total-covariance-factor", type=float, default=0.0)
    ap.add_argument("--covariance-floor", type=float, default=1e-6)
    ap.add_argument("--mean", type=str, default=None, help="global mean to subtract (default: the mean of the archive itself)")
    ap.add_argument("--backend", choices=["host", "hip"], default="host", help="hip: class sums and both scatter matrices on the GPU")
    ap.add_argument("ark")
    ap.add_argument("utt2spk")
    ap.add_argument("transform")
    a = ap.parse_args()
    mean = kaldi_io.read_vec_flt(a.mean) if a.mean else None
    T, ev = plda.compute_lda(scoring.read_embeddings(a.ark), plda.read_utt2spk(a.utt2spk), a.dim, a.total_covariance_factor,
                             a.covariance_floor, mean, a.backend, a.transform)
    print("LDA: kept {} of {} dimensions, eigenvalues {} ... {}; wrote {}".format(T.shape[0], T.shape[1] - 1, ev[0], ev[T.shape[0] - 1],
                                                                              a.transform))
