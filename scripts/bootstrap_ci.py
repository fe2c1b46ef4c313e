#!/usr/bin/env python3
"""usage: bootstrap_ci.py [--scores-b F] [--utt2spk FILE] [--replicates R] [--seed S] [--alpha A] [--p-target P]... [--c-miss C] [--c-fa C]
                       [--llr] [--backend host|hip] [--write-replicates FILE] <scores> <trials>
-> prints 'EER: x% [lo, hi]', one 'minDCF(p-target=P): x [lo, hi]' line per prior (default 0.01 and 0.001), with --llr (the scores are
log-likelihood ratios) also one 'actDCF(p-target=P): x [lo, hi]' line per prior, then the count of degenerate replicates; with
--scores-b (a second system on the same trials, in any line order) the same lines for the difference A - B with the share of
replicates below zero.  The intervals are percentile intervals of a speaker-level bootstrap."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_kaldi_resnet_amd  # noqa: E402,F401
from pytorch_kaldi_resnet_amd import bootstrap, calibration  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--scores-b", dest="scores_b", default=None, help="Scores of a second system on the same trials: report the difference A - B")
    ap.add_argument("--utt2spk", default=None, help="'<id> <speaker>' lines: the speakers that are resampled (default: every id is its own unit)")
    ap.add_argument("--replicates", type=int, default=1000, help="Bootstrap replicates")
    ap.add_argument("--seed", type=int, default=0, help="Seed of the counts table")
    ap.add_argument("--alpha", type=float, default=0.05, help="The intervals cover 1 - alpha")
    ap.add_argument("--max-degenerate", type=float, dest="max_degenerate", default=0.05,
                    help="Largest share of replicates without a target or without a non-target trial")
    ap.add_argument("--p-target", type=float, dest="p_target", action="append", default=None,
                    help="The prior probability of the target speaker in a trial; may be given up to 8 times (default: 0.01 and 0.001)")
    ap.add_argument("--c-miss", type=float, dest="c_miss", default=1, help="Cost of a missed detection.")
    ap.add_argument("--c-fa", type=float, dest="c_fa", default=1, help="Cost of a spurious detection.")
    ap.add_argument("--llr", action="store_true", help="The scores are log-likelihood ratios: report actDCF too")
    ap.add_argument("--backend", choices=["host", "hip"], default="host", help="hip: every replicate is swept on the GPU")
    ap.add_argument("--write-replicates", dest="write_replicates", default=None, help="Write the per-replicate values of system A here")
    ap.add_argument("scores_filename", help="Input scores file, with columns of the form <utt1> <utt2> <score>")
    ap.add_argument("trials_filename", help="Input trials file, with columns of the form <utt1> <utt2> <target/nontarget>")
    a = ap.parse_args()
    priors = a.p_target if a.p_target else [0.01, 0.001]
    try:
        if a.replicates < 2:
            raise ValueError("--replicates must be at least 2")
        costs = bootstrap._costs([(p, a.c_miss, a.c_fa) for p in priors], "--p-target")
        pairs, cols = calibration.read_score_files([a.scores_filename])
        labels = calibration.trial_labels(pairs, a.trials_filename)
        ua, ub, names = bootstrap.trial_units(pairs, a.utt2spk)
        kw = dict(costs=costs, act_costs=costs if a.llr else (), replicates=a.replicates, seed=a.seed, alpha=a.alpha,
                  max_degenerate=a.max_degenerate, backend=a.backend, units=len(names))
        if a.scores_b is None:
            rep, diff = bootstrap.bootstrap_report(cols[0], labels, ua, ub, **kw), None
        else:
            pairs_b, cols_b = calibration.read_score_files([a.scores_b])
            both = bootstrap.bootstrap_compare(cols[0], bootstrap.match_scores(pairs, cols[0], pairs_b, cols_b[0]), labels, ua, ub, **kw)
            rep, diff = both["a"], both["diff"]
        if a.write_replicates:
            bootstrap.write_replicates(a.write_replicates, rep["values"])
    except (calibration.ScoreFileError, ValueError, OSError) as e:
        sys.stderr.write("bootstrap_ci.py: error: %s\n" % e)
        sys.exit(2)
    sys.stdout.write("\n".join(bootstrap.report_lines(rep, diff)) + "\n")
