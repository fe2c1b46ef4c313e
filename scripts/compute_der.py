#!/usr/bin/env python3
"""Diarization error rate of a hypothesis RTTM against a reference RTTM (the role of md-eval.pl, restated as
this project's contract in integer ticks).  Prints '<recording> <miss> <fa> <conf> <scored> <DER %>' per recording (counts in ticks)
and an OVERALL line over the summed counts."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("ref", help="reference RTTM")
    ap.add_argument("hyp", help="hypothesis RTTM")
    ap.add_argument("--uem", default=None, help="the regions to score: '<recording> <channel> <start s> <end s>' (default: the reference's extent)")
    ap.add_argument("--collar", type=float, default=0.25, help="seconds not scored on each side of a reference turn boundary")
    ap.add_argument("--ignore-overlap", action="store_true", help="leave out where two or more reference speakers talk")
    ap.add_argument("--tick", type=float, default=0.001, help="seconds per tick")
    ap.add_argument("--backend", choices=["host", "hip"], default="host", help="hip: the counts and the assignment on the GPU")
    a = ap.parse_args(argv)
    if not a.collar >= 0:
        ap.error("--collar must not be negative, got %r" % a.collar)
    if not a.tick > 0:
        ap.error("--tick must be positive, got %r" % a.tick)
    return ap, a


if __name__ == "__main__":
    ap, a = parse()
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize
    try:
        res = diarize.der(a.ref, a.hyp, uem=a.uem, collar=a.collar, ignore_overlap=a.ignore_overlap, tick=a.tick, backend=a.backend)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    rows = [(r, res["per_recording"][r]) for r in res["recordings"]] + [("OVERALL", res["total"])]
    for r, p in rows:
        print("%s %d %d %d %d %.2f" % (r, p["miss"], p["fa"], p["conf"], p["scored"], 100.0 * p["der"]))
