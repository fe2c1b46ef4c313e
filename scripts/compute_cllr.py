#!/usr/bin/env python3
"""usage: compute_cllr.py [--p-target P]... [--c-miss C] [--c-fa C] [--backend host|hip] <scores> <trials>
-> prints 'Cllr: x.xxxx', 'minCllr: x.xxxx' and one 'actDCF(p-target=P): x.xxxx' line per prior (default 0.01 and 0.001): the scores
read as log-likelihood ratios"""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_kaldi_resnet_amd  # noqa: E402,F401
from pytorch_kaldi_resnet_amd import calibration  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--p-target", type=float, dest="p_target", action="append", default=None,
                    help="The prior probability of the target speaker in a trial; may be given up to 8 times (default: 0.01 and 0.001)")
    ap.add_argument("--c-miss", type=float, dest="c_miss", default=1, help="Cost of a missed detection.")
    ap.add_argument("--c-fa", type=float, dest="c_fa", default=1, help="Cost of a spurious detection.")
    ap.add_argument("--backend", choices=["host", "hip"], default="host", help="hip: every sum, count and the pooling run on the GPU")
    ap.add_argument("scores_filename", help="Input scores file, with columns of the form <utt1> <utt2> <score>")
    ap.add_argument("trials_filename", help="Input trials file, with columns of the form <utt1> <utt2> <target/nontarget>")
    a = ap.parse_args()
    priors = a.p_target if a.p_target else [0.01, 0.001]
    try:
        costs = calibration._costs([(p, a.c_miss, a.c_fa) for p in priors])
        pairs, cols = calibration.read_score_files([a.scores_filename])
        labels = calibration.trial_labels(pairs, a.trials_filename)
        rep = calibration.evaluate(cols[0], labels, costs, backend=a.backend)
        mc = calibration.min_cllr(cols[0], labels, backend=a.backend)[0]
    except (calibration.ScoreFileError, ValueError, OSError) as e:
        sys.stderr.write("compute_cllr.py: error: %s\n" % e)
        sys.exit(2)
    sys.stdout.write("Cllr: {0:.4f}\nminCllr: {1:.4f}\n".format(rep["cllr"], mc))
    for p, r in zip(priors, rep["act_dcf"]):
        sys.stdout.write("actDCF(p-target={0}): {1:.4f}\n".format(p, r["act_dcf"]))
        sys.stderr.write("actDCF {0:.4f} at threshold {1:.4f}: {2} misses, {3} false alarms\n".format(r["act_dcf"], r["threshold"], r["miss"], r["fa"]))
