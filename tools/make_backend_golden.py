#!/usr/bin/env python3
"""Fixtures of the scoring stage (tests/golden/backend/), produced by the REFERENCE's own programs:
scripts/compute_mean.py, compute_speaker_mean.py, cosine_score.py, compute_topk_mean_std.py, adaptive_snorm.py, compute_eer.py
and local/compute_min_dcf.py, run unmodified as subprocesses (their functions ComputeErrorRates / ComputeMinDcf imported for the
sweep cases).  Only data is written: text arks, score files, recorded stdout, one .npz of doubles.

usage: make_backend_golden.py <reference checkout>      (needs the reference; never needs a GPU)
"""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "backend")
COSTS = [(0.01, 1.0, 1.0), (0.001, 1.0, 1.0), (0.05, 10.0, 1.0)]


def _module(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_ark(path, keys, mat):
    with open(path, "w") as f:
        for k, v in zip(keys, mat):
            f.write(k + " [ " + " ".join(map(str, v)) + " ]\n")


def stage_files(ref):
    """a small train / test set through the reference's stages 11-13; every program runs inside OUT on relative names, so the
    recorded stdout holds no path of the machine that made it"""
    rng = np.random.RandomState(20)
    D, S = 16, 8
    centres = rng.randn(S, D)
    # 40 training utterances, speakers interleaved (the archive is not grouped by speaker), 2 to 9 utterances per speaker
    per = [2, 9, 5, 3, 7, 4, 6, 4]
    spk_of = np.concatenate([[s] * n for s, n in enumerate(per)])
    rng.shuffle(spk_of)
    count = [0] * S
    train_keys = []
    for s in spk_of:
        train_keys.append("id%02d-u%d" % (s, count[s]))
        count[s] += 1
    train = (centres[spk_of] + 0.6 * rng.randn(len(spk_of), D)).astype(np.float32)
    _write_ark(os.path.join(OUT, "train.iv"), train_keys, train)
    with open(os.path.join(OUT, "utt2spk"), "w") as f:
        for k in sorted(train_keys):
            f.write("%s %s\n" % (k, k.split("-")[0]))
    # 12 test utterances of 4 unseen speakers and all 66 pairs
    tc = rng.randn(4, D)
    test_keys = ["t%d-u%d" % (s, u) for s in range(4) for u in range(3)]
    test = (np.repeat(tc, 3, axis=0) + 1.7 * rng.randn(12, D)).astype(np.float32)
    _write_ark(os.path.join(OUT, "test.iv"), test_keys, test)
    with open(os.path.join(OUT, "trials"), "w") as f:
        for i, a in enumerate(test_keys):
            for b in test_keys[i + 1:]:
                f.write("%s %s %s\n" % (a, b, "target" if a.split("-")[0] == b.split("-")[0] else "nontarget"))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=os.path.join(ref, "scripts"))
    sc, py = os.path.join(ref, "scripts"), sys.executable

    def run(args, stdout_file=None):
        out = subprocess.check_output([py] + args, env=env, cwd=OUT, stderr=subprocess.DEVNULL)
        if stdout_file:
            open(os.path.join(OUT, stdout_file), "wb").write(out)
        return out.decode()

    run([os.path.join(sc, "compute_mean.py"), "train.iv", "mean.vec"])
    run([os.path.join(sc, "compute_speaker_mean.py"), "train.iv", "utt2spk", "spk_mean.vec"], "spk_mean.stdout")
    run([os.path.join(sc, "cosine_score.py"), "--mean", "mean.vec", "--enroll", "test.iv", "--test", "test.iv", "--trials", "trials",
         "--score-file", "scores"])
    # the reference's top-k is hard-wired to 300: its statistics come from the 320-vector cohort of tests/golden/io (same D)
    run([os.path.join(sc, "compute_topk_mean_std.py"), "--mean", "mean.vec", "--ark-file", "test.iv", "--cohort-file",
         os.path.join("..", "io", "cohort.iv"), "--mean-std-file", "topk_mean_std"])
    run([os.path.join(sc, "adaptive_snorm.py"), "--enroll", "topk_mean_std", "--test", "topk_mean_std", "--score-in", "scores",
         "--score-out", "scores_snorm"])
    # the three-line report of test.sh:65-74, for the cosine and the snorm back end
    for scores, report in (("scores", "eer_cosine"), ("scores_snorm", "eer_snorm_adapt_snorm")):
        eer = run([os.path.join(sc, "compute_eer.py"), scores, "trials"]).strip()
        d1 = run([os.path.join(ref, "local", "compute_min_dcf.py"), "--p-target", "0.01", scores, "trials"],
                 "min_dcf_0.01_%s.stdout" % report).strip()
        d2 = run([os.path.join(ref, "local", "compute_min_dcf.py"), "--p-target", "0.001", scores, "trials"]).strip()
        with open(os.path.join(OUT, report), "w") as f:
            f.write("EER: %s%%\nminDCF(p-target=0.01): %s\nminDCF(p-target=0.001): %s\n" % (eer, d1, d2))
    run([os.path.join(ref, "local", "compute_min_dcf.py"), "--p-target", "0.05", "--c-miss", "10", "--c-fa", "2", "scores",
         "trials"], "min_dcf_0.05_10_2.stdout")


def sweep_cases(ref):
    """score / label lists with the reference's EER, minDCF and threshold as exact doubles"""
    eer_mod = _module(os.path.join(ref, "scripts", "compute_eer.py"), "ref_compute_eer")
    dcf_mod = _module(os.path.join(ref, "local", "compute_min_dcf.py"), "ref_compute_min_dcf")
    rng = np.random.RandomState(21)
    out = {"costs": np.array(COSTS, dtype=np.float64)}
    cases = []
    for n in (2, 3, 5, 17, 64, 100, 255, 256, 257, 400):
        for kind in ("random", "tied", "zeros"):
            lab = (rng.rand(n) < 0.3).astype(np.int64)
            lab[rng.randint(n)] = 1
            lab[(np.flatnonzero(lab)[0] + 1) % n] = 0
            s = rng.randn(n) + 1.5 * lab
            if kind == "tied":
                s = np.round(s * 2) / 2
            if kind == "zeros":
                s = np.round(s)
                s[s == 0] *= np.where(rng.rand(int((s == 0).sum())) < 0.5, -1.0, 1.0)     # both zeros
            cases.append((s, lab))
    # all targets below all non-targets (EER 1), all above (EER 0), one constant score
    cases.append((np.array([0.1, 0.2, 0.8, 0.9]), np.array([1, 1, 0, 0])))
    cases.append((np.array([0.9, 0.8, 0.1, 0.0]), np.array([1, 1, 0, 0])))
    cases.append((np.zeros(9), np.array([1, 0, 0, 1, 0, 0, 0, 1, 0])))
    for k, (s, lab) in enumerate(cases):
        scores, labels = [float(v) for v in s], [int(v) for v in lab]
        fnrs, fprs, thresholds = eer_mod.ComputeErrorRates(scores, labels)
        i = np.nanargmin(np.absolute((np.array(fnrs) - np.array(fprs))))
        exp = [max(fprs[i], fnrs[i])]
        fnrs, fprs, thresholds = dcf_mod.ComputeErrorRates(scores, labels)
        for p_target, c_miss, c_fa in COSTS:
            exp.extend(dcf_mod.ComputeMinDcf(fnrs, fprs, thresholds, p_target, c_miss, c_fa))
        out["scores_%02d" % k] = np.array(scores, dtype=np.float64)
        out["labels_%02d" % k] = np.array(labels, dtype=np.uint8)
        out["expect_%02d" % k] = np.array(exp, dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "sweep_cases.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    os.makedirs(OUT, exist_ok=True)
    stage_files(os.path.abspath(sys.argv[1]))
    sweep_cases(os.path.abspath(sys.argv[1]))
    print("wrote", OUT, sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT)), "bytes")
