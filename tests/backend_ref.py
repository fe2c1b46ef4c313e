"""Own numpy / Python restatement of the reference's scoring stage, the yardstick of tests/test_backend_{cpu,gpu}.py:
speaker means (scripts/compute_speaker_mean.py:15-27), adaptive S-norm (scripts/adaptive_snorm.py:28-35), the stable sort and
the error-rate sweep (scripts/compute_eer.py:35-70,101-102, local/compute_min_dcf.py:54-106).  Reads nothing outside the
repository; checked against the reference-made fixtures of tests/golden/backend in test_backend_cpu.py."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backend")


def speaker_mean(keys, mat, utt2spk):
    """spk -> float32 mean, speakers in order of first appearance: a float32 accumulator that takes float64 rows in order"""
    acc, num = {}, {}
    for k, v in zip(keys, mat):
        if k not in utt2spk:
            raise Exception("{} not specified to any speaker".format(k))
        spk = utt2spk[k]
        if spk not in acc:
            acc[spk] = np.zeros(len(v), dtype=np.float32)
            num[spk] = 0
        acc[spk] += np.asarray(v, dtype=np.float64)
        num[spk] += 1
    for spk in acc:
        acc[spk] /= num[spk]
    return acc


def speaker_mean_text(means):
    return "".join(spk + " [ " + " ".join(map(str, v)) + " ]\n" for spk, v in means.items())


def snorm(scores, ia, ib, e_mean, e_std, t_mean, t_std):
    """per trial in Python floats, as the reference's loop"""
    out = []
    for s, a, b in zip(scores, ia, ib):
        s = float(s)
        out.append((s - float(e_mean[a])) / max(float(e_std[a]), 1e-8) / 2 + (s - float(t_mean[b])) / max(float(t_std[b]), 1e-8) / 2)
    return np.array(out, dtype=np.float64)


def sort_order(scores):
    """ascending, equal scores (-0.0 == +0.0) in index order: Python's stable sorted(..., key=itemgetter(1))"""
    s = np.asarray(scores, dtype=np.float64)
    return np.lexsort((np.arange(len(s)), s + 0.0))


def sweep(scores, labels, costs):
    """-> (eer, eer position, [(min_dcf, threshold, position) per (p_target, c_miss, c_fa)])"""
    s = np.asarray(scores, dtype=np.float64)
    order = sort_order(s)
    lab = (np.asarray(labels)[order] != 0).astype(np.int64)
    ct = np.cumsum(lab)
    cn = np.cumsum(1 - lab)
    fnr = ct / float(ct[-1])
    fpr = 1 - cn / float(cn[-1])
    i = int(np.nanargmin(np.absolute(fnr - fpr)))
    out = []
    for p, c_miss, c_fa in costs:
        c = c_miss * fnr * p + c_fa * fpr * (1 - p)
        j = int(np.argmin(c))                # first minimum: the strict `<` of ComputeMinDcf
        out.append((float(c[j] / min(c_miss * p, c_fa * (1 - p))), float(s[order[j]]), j))
    return float(max(fpr[i], fnr[i])), i, out


def sweep_loop(scores, labels, costs):
    """the same in plain Python, operation by operation as the reference writes it (small lists only)"""
    idx = sorted(range(len(scores)), key=lambda i: scores[i])
    lab = [int(labels[i]) for i in idx]
    fn, fp = [], []
    for i, l in enumerate(lab):
        fn.append((fn[-1] if i else 0) + l)
        fp.append((fp[-1] if i else 0) + 1 - l)
    n_tar = sum(lab)
    n_non = len(lab) - n_tar
    fnr = [x / float(n_tar) for x in fn]
    fpr = [1 - x / float(n_non) for x in fp]
    e = int(np.nanargmin(np.absolute(np.array(fnr) - np.array(fpr))))
    out = []
    for p, c_miss, c_fa in costs:
        best, at = float("inf"), 0
        for i in range(len(fnr)):
            c = c_miss * fnr[i] * p + c_fa * fpr[i] * (1 - p)
            if c < best:
                best, at = c, i
        out.append((best / min(c_miss * p, c_fa * (1 - p)), float(scores[idx[at]]), at))
    return max(fpr[e], fnr[e]), e, out


def golden_sweep_cases():
    """[(scores, labels, costs, expected [eer, dcf0, thr0, dcf1, thr1, ...])] recorded from the reference's two functions"""
    z = np.load(os.path.join(GOLD, "sweep_cases.npz"))
    costs = [tuple(c) for c in z["costs"].tolist()]
    n = sum(1 for f in z.files if f.startswith("scores_"))
    return [(z["scores_%02d" % k], z["labels_%02d" % k], costs, z["expect_%02d" % k]) for k in range(n)]


def read_text_ark(path):
    keys, rows = [], []
    for line in open(path):
        p = line.split()
        keys.append(p[0])
        rows.append([float(v) for v in p[2:-1]])
    return keys, np.array(rows, dtype=np.float64)


def read_utt2spk(path):
    return dict(line.split() for line in open(path))
