#!/usr/bin/env python3
"""usage: compute_min_dcf.py [--p-target P] [--c-miss C] [--c-fa C] [--backend host|hip] <scores> <trials>
-> prints the minimum detection cost as 'x.xxxx' (reference local/compute_min_dcf.py: same options, same output)"""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_kaldi_resnet_amd  # noqa: E402,F401
from pytorch_kaldi_resnet_amd import scoring  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--p-target", type=float, dest="p_target", default=0.01, help="The prior probability of the target speaker in a trial.")
    ap.add_argument("--c-miss", type=float, dest="c_miss", default=1, help="Cost of a missed detection.  This is usually not changed.")
    ap.add_argument("--c-fa", type=float, dest="c_fa", default=1, help="Cost of a spurious detection.  This is usually not changed.")
    ap.add_argument("--backend", choices=["host", "hip"], default="host", help="hip: sort and error-rate sweep run on the GPU")
    ap.add_argument("scores_filename", help="Input scores file, with columns of the form <utt1> <utt2> <score>")
    ap.add_argument("trials_filename", help="Input trials file, with columns of the form <utt1> <utt2> <target/nontarget>")
    sys.stderr.write(" ".join(sys.argv) + "\n")
    a = ap.parse_args()
    scores, labels = scoring.read_scored_trials(a.scores_filename, a.trials_filename)
    mindcf, threshold = scoring.min_dcf(scores, labels, a.p_target, a.c_miss, a.c_fa, backend=a.backend)
    sys.stdout.write("{0:.4f}\n".format(mindcf))
    sys.stderr.write("minDCF is {0:.4f} at threshold {1:.4f} (p-target={2}, c-miss={3},"
                     "c-fa={4})\n".format(mindcf, threshold, a.p_target, a.c_miss, a.c_fa))
