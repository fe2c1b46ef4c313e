#!/usr/bin/env python3
"""PLDA scoring: the work of the reference's test.sh pipeline `ivector-subtract-global-mean | transform-vec |
ivector-normalize-length` into `ivector-plda-scoring` (with `ivector-copy-plda --smoothing`), same score file format as
cosine_score.py."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_kaldi_resnet_amd  # noqa: E402,F401
from pytorch_kaldi_resnet_amd import kaldi_io, plda, scoring  # noqa: E402


def _bool(v):
    if v.lower() in ("true", "1", "yes"):
        return True
    if v.lower() in ("false", "0", "no"):
        return False
    raise argparse.ArgumentTypeError("true or false, got %r" % v)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--normalize-length", type=_bool, default=True)
    ap.add_argument("--simple-length-normalization", type=_bool, default=False)
    ap.add_argument("--smoothing", type=float, default=0.0)
    ap.add_argument("--num-utts", type=str, default=None, help="'<utt> <count>' lines: utterances behind each enrolment vector")
    ap.add_argument("--mean", type=str, required=True)
    ap.add_argument("--transform", type=str, required=True)
    ap.add_argument("--plda", type=str, required=True)
    ap.add_argument("--enroll", type=str, required=True)
    ap.add_argument("--test", type=str, required=True)
    ap.add_argument("--trials", type=str, required=True)
    ap.add_argument("--score-file", type=str, required=True)
    ap.add_argument("--backend", choices=["host", "hip"], default="host", help="hip: projection, normalisation and the trial loop on the GPU")
    a = ap.parse_args()
    mean = kaldi_io.read_vec_flt(a.mean)
    en = scoring.read_embeddings(a.enroll)
    te = en if a.test == a.enroll else scoring.read_embeddings(a.test)
    plda.plda_score(en, te, a.trials, mean, plda.read_transform(a.transform), plda.read_plda(a.plda),
                    num_utts=plda.read_num_utts(a.num_utts) if a.num_utts else None, normalize_length=a.normalize_length,
                    simple_length_normalization=a.simple_length_normalization, smoothing=a.smoothing, score_path=a.score_file,
                    backend=a.backend)
    print("saved scores of {} in {}".format(a.trials, a.score_file))
