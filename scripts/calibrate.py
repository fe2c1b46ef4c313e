#!/usr/bin/env python3
"""usage: calibrate.py train --scores F [F ...] --trials FILE --out MODEL [--p-target P] [--l2 L] [--epsilon E] [--max-iters N]
                             [--backend host|hip]
          calibrate.py apply --model MODEL --scores F [F ...] --score-out OUT [--backend host|hip]
Affine calibration (one score file) or fusion (several) of '<utt1> <utt2> <score>' files that list the same trials in the same
order, trained by prior-weighted logistic regression on a development trial list.
exit status: 0; 2 = bad arguments or files (the message names the file and the line); 3 = the model was written but the training did
not converge"""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_kaldi_resnet_amd  # noqa: E402,F401
from pytorch_kaldi_resnet_amd import calibration  # noqa: E402


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="command")
    tr = sub.add_parser("train")
    tr.add_argument("--scores", nargs="+", required=True, help="one score file per system")
    tr.add_argument("--trials", required=True, help="<utt1> <utt2> target|nontarget")
    tr.add_argument("--out", required=True, help="the model file")
    tr.add_argument("--p-target", type=float, dest="p_target", default=0.01)
    tr.add_argument("--l2", type=float, default=0.0)
    tr.add_argument("--epsilon", type=float, default=1e-18)
    tr.add_argument("--max-iters", type=int, dest="max_iters", default=100)
    tr.add_argument("--backend", choices=["host", "hip"], default="host")
    apl = sub.add_parser("apply")
    apl.add_argument("--model", required=True)
    apl.add_argument("--scores", nargs="+", required=True)
    apl.add_argument("--score-out", dest="score_out", required=True)
    apl.add_argument("--backend", choices=["host", "hip"], default="host")
    a = ap.parse_args(argv)
    if a.command is None:
        ap.error("a command is needed: train or apply")
    try:
        if a.command == "train":
            if len(a.scores) > calibration.MAX_K:
                ap.error("--scores: at most %d systems" % calibration.MAX_K)
            if not 0.0 < a.p_target < 1.0:
                ap.error("--p-target must be greater than 0 and less than 1")
            if not a.l2 >= 0.0:
                ap.error("--l2 must not be negative")
            if not a.epsilon >= 0.0:
                ap.error("--epsilon must not be negative")
            if not 1 <= a.max_iters <= 10000:
                ap.error("--max-iters must lie in [1, 10000]")
            pairs, cols = calibration.read_score_files(a.scores)
            labels = calibration.trial_labels(pairs, a.trials)
            model = calibration.train(cols, labels, a.p_target, a.l2, a.epsilon, a.max_iters, backend=a.backend)
            calibration.save(model, a.out)
            sys.stderr.write("%s after %d evaluations: objective %.17g\n" % (model.status, model.evaluations, model.objective))
            if model.status != "converged":
                sys.stderr.write("calibrate.py: the training ended %s; the model was written to %s\n" % (model.status, a.out))
                return 3
            return 0
        model = calibration.load(a.model)
        if len(a.scores) != len(model.weights):
            ap.error("--scores: %d files for a model of %d systems" % (len(a.scores), len(model.weights)))
        pairs, cols = calibration.read_score_files(a.scores)
        llr = calibration.apply(model, cols, backend=a.backend)
        with open(a.score_out, "w") as f:
            for (u, v), x in zip(pairs, llr.tolist()):
                f.write("{} {} {}\n".format(u, v, x))
        return 0
    except (calibration.ScoreFileError, ValueError, OSError) as e:
        sys.stderr.write("calibrate.py: error: %s\n" % e)
        return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
