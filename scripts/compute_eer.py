#!/usr/bin/env python3
"""usage: compute_eer.py [--backend host|hip] <scores> <trials>  -> prints EER as 'x.xx%' (reference scripts/compute_eer.py);
--backend hip: the sort and the error-rate sweep run on the GPU (scoring.error_rates), the same number"""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_kaldi_resnet_amd  # noqa: E402,F401
from pytorch_kaldi_resnet_amd import scoring  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["host", "hip"], default="host")
    ap.add_argument("scores_filename")
    ap.add_argument("trials_filename")
    a = ap.parse_args()
    scores, labels = scoring.read_scored_trials(a.scores_filename, a.trials_filename)
    eer = scoring.compute_eer(scores, labels) if a.backend == "host" else scoring.error_rates(scores, labels, (), "hip")["eer"]
    sys.stdout.write("{0:.2%}\n".format(eer))
    sys.stderr.write("eer is {0:.2%}\n".format(eer))
