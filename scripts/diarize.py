#!/usr/bin/env python3
"""Diarization from sliding-window embeddings: what Kaldi's callhome_diarization recipe runs behind extract_xvectors.sh -
ivector-plda-scoring-dense (or cosine), agglomerative-cluster and make_rttm.py - on what `decode.py --window W --period P` wrote
(DESIGN.md section 6n).  Writes <out-dir>/labels ('<window-key> <label>' lines), <out-dir>/rttm and, with --write-scores, one text
matrix per recording in <out-dir>/scores.<recording>.  With --vbx the clustering is the first pass of VBx resegmentation (section
6o): labels and rttm then hold the VBx result and <out-dir>/labels.ahc the first pass.  With --target-energy E the PLDA scores take
ivector-plda-scoring-dense's per-recording PCA (section 6p) and <out-dir>/pca_dim lists '<recording> <dim>'; VBx is unaffected.
With --ref-rttm F the result is scored against the reference (section 6r) and <out-dir>/der holds one line per recording and an
OVERALL line, as compute_der.py prints them.  With --tune-threshold LO:HI:STEP (in place of --threshold; needs --ref-rttm) the
recordings are clustered once, every threshold of the grid is scored, <out-dir>/threshold_der lists '<threshold> <miss> <fa> <conf>
<scored> <DER>' and <out-dir>/best_threshold the winner, and every other file is that of the best threshold."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _bool(v):
    if v.lower() in ("true", "1", "yes"):
        return True
    if v.lower() in ("false", "0", "no"):
        return False
    raise argparse.ArgumentTypeError("true or false, got %r" % v)


def threshold_grid(text):
    """LO:HI:STEP -> LO, LO + STEP, ... up to HI (HI included where it lies on the grid, give or take a billionth of a step)"""
    try:
        lo, hi, step = (float(v) for v in text.split(":"))
    except ValueError:
        raise argparse.ArgumentTypeError("LO:HI:STEP (three numbers), got %r" % text)
    if not (step > 0 and hi >= lo and (hi - lo) / step < 1e6):
        raise argparse.ArgumentTypeError("LO:HI:STEP needs STEP > 0, HI >= LO and fewer than a million thresholds, got %r" % text)
    return [lo + i * step for i in range(int((hi - lo) / step + 1e-9) + 1)]


def der_lines(res):
    """'<recording> <miss> <fa> <conf> <scored> <DER>' per recording and an OVERALL line (ticks; DER in percent, nan where nothing is scored)"""
    rows = [(r, res["per_recording"][r]) for r in res["recordings"]] + [("OVERALL", res["total"])]
    return ["%s %d %d %d %d %.2f" % (r, p["miss"], p["fa"], p["conf"], p["scored"], 100.0 * p["der"]) for r, p in rows]


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--embeddings", required=True, help="the vectors decode.py --window wrote (text or binary), one per window")
    ap.add_argument("--segments", required=True, help="segments.<name> of the same run: '<key> <recording> <start s> <end s>'")
    ap.add_argument("--backend-score", choices=["cosine", "plda"], default="cosine")
    ap.add_argument("--mean", default=None, help="global mean to subtract (default: the mean of --embeddings)")
    ap.add_argument("--transform", default=None, help="LDA transform (required with plda, optional with cosine)")
    ap.add_argument("--plda", default=None)
    ap.add_argument("--smoothing", type=float, default=0.0)
    ap.add_argument("--normalize-length", type=_bool, default=True)
    ap.add_argument("--simple-length-normalization", type=_bool, default=False)
    ap.add_argument("--threshold", type=float, default=None,
                    help="stop merging when the average score of the best pair of clusters falls below this")
    ap.add_argument("--reco2num-spk", default=None, help="'<recording> <speakers>' lines: cluster every recording down to its count")
    ap.add_argument("--recordings", default=None, help="optional list of the recordings expected: one with no window is an error")
    ap.add_argument("--backend", choices=["host", "hip"], default="host", help="hip: scores and clustering on the GPU")
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--rttm-channel", type=int, default=0)
    ap.add_argument("--write-scores", action="store_true")
    ap.add_argument("--target-energy", type=float, default=None,
                    help="per-recording PCA of ivector-plda-scoring-dense: keep this share of each recording's energy, in (0, 1) "
                         "(needs --backend-score plda; also writes <out-dir>/pca_dim)")
    ap.add_argument("--vbx", action="store_true", help="resegment with VBx, seeded by the clustering (needs --backend-score plda)")
    ap.add_argument("--vbx-fa", type=float, default=0.3)
    ap.add_argument("--vbx-fb", type=float, default=17.0)
    ap.add_argument("--vbx-loop-prob", type=float, default=0.99)
    ap.add_argument("--vbx-max-iters", type=int, default=40)
    ap.add_argument("--vbx-epsilon", type=float, default=1e-6)
    ap.add_argument("--vbx-init-smoothing", type=float, default=7.0)
    ap.add_argument("--ref-rttm", default=None, help="reference RTTM: score the result (writes <out-dir>/der; DESIGN.md section 6r)")
    ap.add_argument("--uem", default=None, help="with --ref-rttm: the regions to score, '<recording> <channel> <start s> <end s>'")
    ap.add_argument("--der-collar", type=float, default=0.25, help="with --ref-rttm: seconds not scored on each side of a reference boundary")
    ap.add_argument("--der-ignore-overlap", action="store_true", help="with --ref-rttm: leave out where two reference speakers talk")
    ap.add_argument("--tune-threshold", type=threshold_grid, default=None, metavar="LO:HI:STEP",
                    help="in place of --threshold: cluster once, score every threshold of the grid against --ref-rttm, use the best")
    a = ap.parse_args(argv)
    if a.tune_threshold is not None:
        if a.threshold is not None or a.reco2num_spk is not None:
            ap.error("--tune-threshold takes the place of --threshold and --reco2num-spk")
        if a.ref_rttm is None:
            ap.error("--tune-threshold needs --ref-rttm")
    elif (a.threshold is None) == (a.reco2num_spk is None):
        ap.error("give exactly one of --threshold and --reco2num-spk")
    if a.ref_rttm is None and (a.uem is not None or a.der_ignore_overlap or a.der_collar != 0.25):
        ap.error("--uem, --der-collar and --der-ignore-overlap need --ref-rttm")
    if not a.der_collar >= 0:
        ap.error("--der-collar must not be negative, got %r" % a.der_collar)
    if a.backend_score == "plda" and (a.plda is None or a.transform is None):
        ap.error("--backend-score plda needs --plda and --transform")
    if a.backend_score == "cosine" and a.plda is not None:
        ap.error("--plda is only used with --backend-score plda")
    if a.vbx and a.backend_score != "plda":
        ap.error("--vbx needs --backend-score plda")
    if a.target_energy is not None:
        if a.backend_score != "plda":
            ap.error("--target-energy needs --backend-score plda")
        if not 0.0 < a.target_energy < 1.0:
            ap.error("--target-energy must lie strictly between 0 and 1, got %r" % a.target_energy)
    return ap, a


if __name__ == "__main__":
    ap, a = parse()
    import numpy as np
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize, kaldi_io, plda, scoring
    try:
        segments = diarize.read_segments(a.segments)
        emb = scoring.read_embeddings(a.embeddings)
        extra = {}
        if a.backend_score == "plda":
            extra = dict(plda=plda.read_plda(a.plda), smoothing=a.smoothing, normalize_length=a.normalize_length,
                         simple_length_normalization=a.simple_length_normalization)
        if a.ref_rttm is not None:
            extra.update(ref=diarize.read_rttm(a.ref_rttm), uem=diarize.read_uem(a.uem) if a.uem else None, tune=a.tune_threshold,
                         der_collar=a.der_collar, der_ignore_overlap=a.der_ignore_overlap)
        res = diarize.diarize(emb, segments, a.backend_score, threshold=a.threshold,
                              reco2num_spk=diarize.read_reco2num_spk(a.reco2num_spk) if a.reco2num_spk else None,
                              recordings=[l.split()[0] for l in open(a.recordings) if l.strip()] if a.recordings else None,
                              backend=a.backend, channel=a.rttm_channel, return_scores=a.write_scores,
                              vbx=dict(Fa=a.vbx_fa, Fb=a.vbx_fb, loop_prob=a.vbx_loop_prob, max_iters=a.vbx_max_iters,
                                       epsilon=a.vbx_epsilon, init_smoothing=a.vbx_init_smoothing) if a.vbx else None,
                              target_energy=a.target_energy, mean=kaldi_io.read_vec_flt(a.mean) if a.mean else None,
                              transform=plda.read_transform(a.transform) if a.transform else None, **extra)
    except ValueError as e:
        ap.error(str(e))
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "labels"), "w") as f:
        for k, l in zip(res["keys"], res["labels"]):
            f.write("%s %d\n" % (k, l))
    if a.vbx:
        with open(os.path.join(a.out_dir, "labels.ahc"), "w") as f:
            for k, l in zip(res["keys"], res["ahc_labels"]):
                f.write("%s %d\n" % (k, l))
    if a.target_energy is not None:
        with open(os.path.join(a.out_dir, "pca_dim"), "w") as f:
            for reco, d in zip(res["recordings"], res["pca_dim"]):
                f.write("%s %d\n" % (reco, d))
    with open(os.path.join(a.out_dir, "rttm"), "w") as f:
        f.write("".join(l + "\n" for l in res["rttm"]))
    if a.ref_rttm is not None:
        with open(os.path.join(a.out_dir, "der"), "w") as f:
            f.write("".join(l + "\n" for l in der_lines(res["der"])))
    if a.tune_threshold is not None:
        with open(os.path.join(a.out_dir, "threshold_der"), "w") as f:
            for t, miss, fa, conf, scored, d in res["der_table"]:
                f.write("%.9g %d %d %d %d %.2f\n" % (t, miss, fa, conf, scored, 100.0 * d))
        with open(os.path.join(a.out_dir, "best_threshold"), "w") as f:
            f.write("%.9g\n" % res["best_threshold"])
    if a.write_scores:
        ro, mo = res["rec_off"], res["mat_off"]
        for r, reco in enumerate(res["recordings"]):
            n = int(ro[r + 1] - ro[r])
            np.savetxt(os.path.join(a.out_dir, "scores." + reco), res["scores"][mo[r]:mo[r + 1]].reshape(n, n), fmt="%.9g")
    print("diarized {} recordings ({} windows, {} segments) into {}".format(len(res["recordings"]), len(res["keys"]),
                                                                           len(res["rttm"]), a.out_dir))
    if a.tune_threshold is not None:
        print("best threshold {:.9g} of {} ({} jobs scored on the host)".format(res["best_threshold"], len(res["der_table"]), res["der_host_jobs"]))
    if a.ref_rttm is not None:
        print(der_lines(res["der"])[-1])
