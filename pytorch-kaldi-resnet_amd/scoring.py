"""Cosine scoring back end (the step after the path): global mean, mean-subtracted cosine per trial, EER,
cohort top-k statistics and adaptive S-norm.

Behaviour of the reference's scripts/compute_mean.py:9-33, scripts/cosine_score.py:52-68,
scripts/compute_eer.py:35-105, scripts/compute_topk_mean_std.py:10-23 and scripts/adaptive_snorm.py:14-40 (same file
formats, same numbers).  Two back ends with the same results to fp32 rounding: `host` (numpy, vectorised instead of a
per-trial Python/torch loop) and `hip` (csrc/score.hip through ops.py: embeddings stay in HBM, one launch per stage).

The rest of the stage (reference run_aam_v2.sh:139-181, test.sh): per-speaker means of the training embeddings - the S-norm
cohort (scripts/compute_speaker_mean.py:9-30), the minimum detection cost (local/compute_min_dcf.py:43-106) and the whole stage in
one call (score_and_report).  These are exact: `host` and `hip` (csrc/eval.hip) return the reference's numbers bit for bit.
"""
import numpy as np

from . import kaldi_io


def read_embeddings(ark_path):
    """utt -> float64 vector from the ark written by decode (text 'utt [ v0 ... ]' lines or binary FV records): an
    vecark.EmbTable - a dict like the one kaldi_io.read_vec_flt_ark yields, parsed natively (libspkio), that also carries the
    [n][D] matrix the vectorised paths below work on."""
    from . import vecark
    return vecark.load(ark_path)


def compute_mean(ark_path, mean_path=None):
    """float32 mean over all vectors (compute_mean.py builds a FloatTensor and torch.mean's it)."""
    from . import vecark
    mat = vecark.load(ark_path).mat.astype(np.float32)
    import torch
    mean = torch.from_numpy(mat).mean(dim=0).numpy()   # same reduction as the reference (torch.mean over rows)
    if mean_path:
        with open(mean_path, "w") as f:
            f.write(" [ " + " ".join(map(str, mean)) + " ]\n")
    return mean


def _table(vecs, mean):
    """dict utt -> vector  =>  (key -> row index, float32 [N][D] of mean-subtracted vectors).  The subtraction is done
    in float64 and cast to float32, as the reference does (numpy float64 ark values minus the mean, then FloatTensor).
    An EmbTable (read_embeddings) is converted in one vectorised pass over its matrix."""
    m = np.zeros(1) if mean is None else np.asarray(mean, dtype=np.float64)
    if hasattr(vecs, "mat") and len(vecs) == len(vecs.keys_list):       # (no duplicate keys: dict and matrix agree)
        return vecs.index, (vecs.mat - m).astype(np.float32)
    keys = list(vecs)
    mat = np.stack([(np.asarray(vecs[k], dtype=np.float64) - m).astype(np.float32) for k in keys])
    return {k: i for i, k in enumerate(keys)}, mat


def _device_rows(mat, eps):
    import torch
    from . import ops
    return ops.center_normalize(torch.from_numpy(np.ascontiguousarray(mat)).cuda(), None, eps)


def _read_trials(trials_path, enroll, test, mean):
    """the trial list against the two tables: (pairs, labels, enrol rows ia, test rows ib, enrol matrix, test matrix)"""
    pairs, labels = [], []
    for line in open(trials_path):
        a, b, t = line.strip().split()
        pairs.append((a, b))
        labels.append(1 if t == "target" else 0)
    ie, me = _table(enroll, mean)
    it, mt = (ie, me) if test is enroll else _table(test, mean)
    ia = np.fromiter((ie[a] for a, _ in pairs), dtype=np.int32, count=len(pairs))    # KeyError = unknown utterance
    ib = np.fromiter((it[b] for _, b in pairs), dtype=np.int32, count=len(pairs))
    return pairs, labels, ia, ib, me, mt


def _device_cosine(me, mt, ia, ib, same):
    """float32 device tensor of the trial cosines; embeddings and indices go up, nothing comes down"""
    import torch
    from . import ops
    en = _device_rows(me, 1e-8)
    te = en if same else _device_rows(mt, 1e-8)
    return ops.trial_cosine(en, te, torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda())


def cosine_score(enroll, test, trials_path, mean=None, score_path=None, backend="host"):
    """scores for '<enroll> <test> target|nontarget' lines; vectors are mean-subtracted in float64, cast to
    float32, cosine = a.b / (max(|a|,eps) * max(|b|,eps)) with eps 1e-8 (F.cosine_similarity)."""
    pairs, labels, ia, ib, me, mt = _read_trials(trials_path, enroll, test, mean)
    if backend == "hip":
        scores = _device_cosine(me, mt, ia, ib, test is enroll).cpu().numpy()
    else:
        assert backend == "host", backend
        # the same arithmetic as before, gathered in chunks so that 10^7 trials do not materialise two [T][D] matrices at once
        ne = np.maximum(np.linalg.norm(me, axis=1), 1e-8)
        nt = ne if test is enroll else np.maximum(np.linalg.norm(mt, axis=1), 1e-8)
        scores = np.empty(len(pairs), dtype=np.float32)
        for lo in range(0, len(pairs), 1 << 18):
            ja, jb = ia[lo:lo + (1 << 18)], ib[lo:lo + (1 << 18)]
            num = (me[ja] * mt[jb]).sum(1, dtype=np.float32)
            scores[lo:lo + len(ja)] = (num / (ne[ja] * nt[jb])).astype(np.float32)
    if score_path:
        with open(score_path, "w") as f:
            for (a, b), s in zip(pairs, scores):
                f.write("{} {} {}\n".format(a, b, s))
    return scores, np.array(labels)


def compute_eer(scores, labels):
    """EER as a fraction: sort by score, cumulative miss / false-alarm rates, argmin |fnr - fpr|, max of the two."""
    order = np.argsort(np.asarray(scores), kind="stable")
    lab = np.asarray(labels, dtype=np.float64)[order]
    fnrs = np.cumsum(lab) / lab.sum()
    fprs = 1.0 - np.cumsum(1.0 - lab) / (len(lab) - lab.sum())
    i = int(np.nanargmin(np.abs(fnrs - fprs)))
    return float(max(fprs[i], fnrs[i]))


def topk_mean_std(vecs, cohort, mean=None, topk=300, backend="host"):
    """utt -> (mean, std) of the `topk` largest cosine scores of the utterance against the cohort vectors
    (compute_topk_mean_std.py:10-23: both sides mean-subtracted and L2-normalised, unbiased std)."""
    iv, mv = _table(vecs, mean)
    _, mc = _table(cohort, mean)
    if topk > len(mc):
        raise RuntimeError("selected index k out of range: topk=%d > %d cohort vectors" % (topk, len(mc)))
    if backend == "hip":
        from . import ops
        v, c = _device_rows(mv, 1e-12), _device_rows(mc, 1e-12)
        scores = ops.gemm(v, c, v.shape[0], c.shape[0], v.shape[1], v.stride(0), 1, 1, c.stride(0))
        mu, sd = ops.topk_mean_std(scores, topk)
        mu, sd = mu.cpu().numpy(), sd.cpu().numpy()
    else:
        assert backend == "host", backend
        v = mv / np.maximum(np.linalg.norm(mv, axis=1, keepdims=True), 1e-12)
        c = mc / np.maximum(np.linalg.norm(mc, axis=1, keepdims=True), 1e-12)
        top = -np.sort(-(v @ c.T), axis=1)[:, :topk]
        mu = top.mean(axis=1, dtype=np.float32)
        sd = top.std(axis=1, ddof=1, dtype=np.float32)
    return {k: (np.float32(mu[i]), np.float32(sd[i])) for k, i in iv.items()}


def write_mean_std(stats, path):
    with open(path, "w") as f:
        for k, (m, s) in stats.items():
            f.write("{} {} {}\n".format(k, m, s))


def read_mean_std(path):
    out = {}
    for line in open(path):
        k, m, s = line.strip().split()
        out[k] = (float(m), float(s))
    return out


def _stats_tables(stats, names):
    """(name -> row, mean [n] float64, std [n] float64) over the names a trial list uses; KeyError = no statistics for a name"""
    index = {}
    for k in names:
        if k not in index:
            index[k] = len(index)
    mu = np.fromiter((stats[k][0] for k in index), dtype=np.float64, count=len(index))
    sd = np.fromiter((stats[k][1] for k in index), dtype=np.float64, count=len(index))
    return index, mu, sd


def _snorm_host(scores, ia, ib, emu, esd, tmu, tsd):
    """adaptive_snorm.py:33-34 on float64 arrays: the same IEEE operations in the same order as the Python expression"""
    s = np.asarray(scores, dtype=np.float64)
    return (s - emu[ia]) / np.maximum(esd[ia], 1e-8) / 2 + (s - tmu[ib]) / np.maximum(tsd[ib], 1e-8) / 2


def _snorm_device(scores, ia, ib, emu, esd, tmu, tsd):
    """scores: a float32 / float64 device tensor, or host values (uploaded as float64) -> float64 device tensor"""
    import torch
    from . import ops
    if not torch.is_tensor(scores):
        scores = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float64)).cuda()
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()      # noqa: E731
    return ops.trial_snorm(scores, up(ia.astype(np.int32)), up(ib.astype(np.int32)), up(emu), up(esd), up(tmu), up(tsd))


def adaptive_snorm(enroll_stats, test_stats, score_in, score_out=None, backend="host"):
    """adaptive_snorm.py:28-36: half the enrol-side plus half the test-side z-normalised score, in Python floats
    (`hip`: the same fp64 expression per trial in one launch, csrc/eval.hip)."""
    if backend == "hip":
        trials, sc = [], []
        for line in open(score_in):
            a, b, v = line.strip().split()
            trials.append((a, b))
            sc.append(float(v))
        ie, emu, esd = _stats_tables(enroll_stats, (a for a, _ in trials))
        it, tmu, tsd = _stats_tables(test_stats, (b for _, b in trials))
        ia = np.fromiter((ie[a] for a, _ in trials), dtype=np.int32, count=len(trials))
        ib = np.fromiter((it[b] for _, b in trials), dtype=np.int32, count=len(trials))
        out = _snorm_device(np.array(sc, dtype=np.float64), ia, ib, emu, esd, tmu, tsd).cpu().numpy().tolist()
        if score_out:
            with open(score_out, "w") as f:
                f.write("\n".join("{} {} {}".format(a, b, v) for (a, b), v in zip(trials, out)) + "\n")
        return out
    assert backend == "host", backend
    lines, out = [], []
    for line in open(score_in):
        a, b, sc = line.strip().split()
        sc = float(sc)
        v = (sc - enroll_stats[a][0]) / max(enroll_stats[a][1], 1e-8) / 2 + (sc - test_stats[b][0]) / max(test_stats[b][1], 1e-8) / 2
        out.append(v)
        lines.append("{} {} {}".format(a, b, v))
    if score_out:
        with open(score_out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return out


# ---- the rest of the scoring stage: speaker-mean cohort, minDCF, one-process report -------------------------------------
def _archive_rows(vecs):
    """(keys in archive order, [n][D] float64): every record, duplicates included, as kaldi_io.read_vec_flt_ark yields them"""
    if hasattr(vecs, "mat"):
        return vecs.keys_list, vecs.mat
    keys = list(vecs)
    return keys, np.stack([np.asarray(vecs[k], dtype=np.float64) for k in keys]) if keys else np.zeros((0, 0))


def speaker_mean(vecs, utt2spk_path, out_path=None, backend="host"):
    """spk -> float32 mean of its utterances' vectors, speakers in order of first appearance in the archive
    (compute_speaker_mean.py:9-30: a float32 accumulator that takes every float64 vector in archive order, then `/= count`).
    The text output is the reference's: 'spk [ v0 v1 ... ]' with str(np.float32) values."""
    utt2spk = {}
    for line in open(utt2spk_path):
        utt, spk = line.strip().split()
        utt2spk[utt] = spk
    keys, mat = _archive_rows(vecs)
    spk_index, spk_of = {}, np.empty(len(keys), dtype=np.int64)
    for r, utt in enumerate(keys):
        if utt not in utt2spk:
            raise Exception("{} not specified to any speaker".format(utt))
        spk_of[r] = spk_index.setdefault(utt2spk[utt], len(spk_index))
    S = len(spk_index)
    if backend == "hip":
        import torch
        from . import ops
        rows = np.argsort(spk_of, kind="stable").astype(np.int32)              # grouped by speaker, archive order inside
        seg_off = np.concatenate([[0], np.cumsum(np.bincount(spk_of, minlength=S))]).astype(np.int32)
        means = ops.segment_mean(torch.from_numpy(np.ascontiguousarray(mat, dtype=np.float64)).cuda(), torch.from_numpy(rows).cuda(),
                                 torch.from_numpy(seg_off).cuda()).cpu().numpy()
    else:
        assert backend == "host", backend
        means = np.zeros((S, mat.shape[1] if S else 0), dtype=np.float32)
        for r in range(len(keys)):
            means[spk_of[r]] += mat[r]                      # float32 += float64: added in float64, rounded to float32
        means /= np.bincount(spk_of, minlength=S).astype(np.float32)[:, None] if S else 1
    out = {spk: means[i] for spk, i in spk_index.items()}
    if out_path:
        with open(out_path, "w") as f:
            for spk, v in out.items():
                f.write(spk + " [ " + " ".join(map(str, v)) + " ]\n")
    return out


def read_scored_trials(scores_path, trials_path):
    """(scores, labels) of a score file against a trial list, looked up by '<utt1> <utt2>' as compute_eer.py:80-97 and
    compute_min_dcf.py:119-136 do (the last label of a repeated trial wins; a scored pair without a trial raises)"""
    trials = {}
    for line in open(trials_path):
        a, b, t = line.rstrip().split()
        trials[a + " " + b] = t
    scores, labels = [], []
    for line in open(scores_path):
        a, b, s = line.rstrip().split()
        if a + " " + b not in trials:
            raise Exception("Missing entry for " + a + " and " + b + " " + scores_path)
        scores.append(float(s))
        labels.append(1 if trials[a + " " + b] == "target" else 0)
    return scores, labels


DEFAULT_COSTS = ((0.01, 1, 1), (0.001, 1, 1))


def _check_costs(costs):
    """compute_min_dcf.py:43-50"""
    for p_target, c_miss, c_fa in costs:
        if c_fa <= 0:
            raise ValueError("--c-fa must be greater than 0")
        if c_miss <= 0:
            raise ValueError("--c-miss must be greater than 0")
        if p_target <= 0 or p_target >= 1:
            raise ValueError("--p-target must be greater than 0 and less than 1")


def _sweep_host(s, lab, costs):
    """ComputeErrorRates / ComputeMinDcf in numpy: stable sort (-0.0 equals +0.0), exact integer counts, rates and costs in
    float64 in the reference's order of operations, first minimum wins."""
    T = len(s)
    order = np.lexsort((np.arange(T), s + 0.0))
    ct = np.cumsum(lab[order], dtype=np.int64)
    cn = np.arange(1, T + 1, dtype=np.int64) - ct
    n_tar, n_non = int(ct[-1]), int(cn[-1])
    fnr = ct / float(n_tar)
    fpr = 1 - cn / float(n_non)
    i = int(np.nanargmin(np.abs(fnr - fpr)))
    dcf = []
    for p_target, c_miss, c_fa in costs:
        c = c_miss * fnr * p_target + c_fa * fpr * (1 - p_target)
        j = int(np.argmin(c))
        dcf.append((float(c[j] / min(c_miss * p_target, c_fa * (1 - p_target))), float(s[order[j]]), j))
    return {"eer": float(max(fpr[i], fnr[i])), "eer_index": i, "n_target": n_tar, "n_nontarget": n_non, "min_dcf": dcf}


def _sweep_device(scores, lab, costs):
    """scores: float64 device tensor; labels go up, 2 + 3 P numbers come down"""
    import torch
    from . import ops
    order = ops.sort_trials(scores)                                     # ValueError on NaN
    out_d, out_i = ops.error_sweep(scores, torch.from_numpy(lab).cuda(), order, costs)
    d, i = out_d.cpu().tolist(), out_i.cpu().tolist()
    return {"eer": d[0], "eer_index": i[0], "n_target": i[1], "n_nontarget": i[2],
            "min_dcf": [(d[1 + 2 * k], d[2 + 2 * k], i[3 + k]) for k in range(len(costs))]}


def error_rates(scores, labels, costs=DEFAULT_COSTS, backend="host"):
    """The EER and every minimum detection cost from one sort of the trial scores (compute_eer.py:35-70,101-102,
    compute_min_dcf.py:54-106).  costs: triples (p_target, c_miss, c_fa).  -> {'eer', 'eer_index', 'n_target', 'n_nontarget',
    'min_dcf': [(min_dcf, threshold, index), ...]}, the same doubles from both back ends.  `scores` may be a float64 device tensor
    on `hip`."""
    costs = [tuple(float(v) for v in c) for c in costs]
    _check_costs(costs)
    lab = np.ascontiguousarray(np.asarray(labels) != 0, dtype=np.uint8)
    n_tar = int(lab.sum())
    if n_tar == 0 or n_tar == len(lab):
        raise ValueError("error rates need at least one target and one non-target trial")
    if backend == "hip":
        import torch
        if not torch.is_tensor(scores):
            s = np.ascontiguousarray(scores, dtype=np.float64)
            if np.isnan(s).any():
                raise ValueError("a score is NaN")
            scores = torch.from_numpy(s).cuda()
        if scores.numel() != len(lab):
            raise ValueError("%d scores for %d labels" % (scores.numel(), len(lab)))
        return _sweep_device(scores, lab, costs)
    assert backend == "host", backend
    s = np.ascontiguousarray(scores, dtype=np.float64)
    if len(s) != len(lab):
        raise ValueError("%d scores for %d labels" % (len(s), len(lab)))
    if np.isnan(s).any():
        raise ValueError("a score is NaN")
    return _sweep_host(s, lab, costs)


def min_dcf(scores, labels, p_target=0.01, c_miss=1, c_fa=1, backend="host"):
    """(minDCF, threshold) of compute_min_dcf.py"""
    d, thr, _ = error_rates(scores, labels, ((p_target, c_miss, c_fa),), backend)["min_dcf"][0]
    return d, thr


def _calibrated(report, scores, labels, costs, calibration, backend):
    """the report with 'cllr', 'min_cllr' and 'act_dcf' (one per cost triple) of the scores through a one-system calibration model
    (calibration.Model or its file); on `hip` the scores and the log-likelihood ratios stay on the device"""
    from . import calibration as cal
    model = cal.load(calibration) if isinstance(calibration, str) else calibration
    if len(model.weights) != 1:
        raise ValueError("score_and_report calibrates one system, the model has %d" % len(model.weights))
    llr = cal.apply(model, scores, backend)
    ev = cal.evaluate(llr, labels, costs, backend)
    report["cllr"] = ev["cllr"]
    report["min_cllr"] = cal.min_cllr(llr, labels, backend)[0]
    report["act_dcf"] = [a["act_dcf"] for a in ev["act_dcf"]]
    return report


def _trial_pairs(trials_path):
    return [tuple(line.split()[:2]) for line in open(trials_path)]


def _bootstrap_ci(pairs, scores, labels, costs, calibration, backend, options):
    """score_and_report's 'ci': {'eer', 'min_dcf', 'act_dcf' (of the calibrated scores; empty without a model), 'replicates',
    'degenerate', 'alpha', 'units'}, each entry {'value', 'lo', 'hi', 'mean', 'std'}"""
    from . import bootstrap as boot
    opt = dict(options)
    ua, ub, names = boot.trial_units(pairs, opt.pop("utt2spk", None))
    if opt.get("counts") is None:
        opt["counts"] = boot.bootstrap_counts(len(names), opt.pop("replicates", 1000), opt.pop("seed", 0))
    opt.pop("replicates", None)
    opt.pop("seed", None)
    ci = boot.bootstrap_report(scores, labels, ua, ub, costs, (), backend=backend, units=len(names), **opt)
    if calibration is not None:
        from . import calibration as cal
        model = cal.load(calibration) if isinstance(calibration, str) else calibration
        act = boot.bootstrap_report(cal.apply(model, scores, backend), labels, ua, ub, (), costs, backend=backend, units=len(names), **opt)
        ci["act_dcf"], ci["act_costs"] = act["act_dcf"], act["act_costs"]
    del ci["values"]
    return ci


def score_and_report(enroll, test, trials_path, mean, enroll_stats=None, test_stats=None, costs=DEFAULT_COSTS, backend="host",
                     score_path=None, plda=None, transform=None, num_utts=None, calibration=None, bootstrap=None):
    """The whole scoring stage in one process: cosine per trial, adaptive S-norm when both statistics tables are given
    (utt -> (mean, std), topk_mean_std / read_mean_std), error-rate sweep.  -> the error_rates report.  On `hip` the embeddings
    and the index arrays go up and only the report comes down (and the scores, if score_path asks for them).
    plda = (mean, transform, psi) with the LDA `transform` (and optionally num_utts: utt -> enrolment count) scores the trials with
    the PLDA back end instead of the cosine (plda.plda_score); S-norm does not apply to it.
    calibration: a one-system calibration.Model (or its file): the report gains 'cllr', 'min_cllr' and 'act_dcf' of the calibrated
    scores (section 6s); without it the report is what it was.
    bootstrap: a dict of bootstrap_report's options (replicates, seed, alpha, max_degenerate, counts) and `utt2spk` (a dict or a file:
    the speakers that are resampled; without it every id is its own unit): the report gains 'ci', the speaker-level bootstrap
    intervals of the EER and every minDCF - and of every actDCF when `calibration` is given (section 6t); without it the report is
    what it was."""
    if plda is not None:
        from . import plda as plda_mod
        assert transform is not None, "the plda back end needs the LDA transform"
        assert enroll_stats is None and test_stats is None, "S-norm is a cosine back end"
        scores, labels = plda_mod.plda_score(enroll, test, trials_path, mean, transform, plda, num_utts=num_utts,
                                             score_path=score_path, backend=backend, return_device=True)
        if backend == "hip":
            import torch
            scores = scores.to(torch.float64)            # (widening: exact)
        else:
            scores = scores.astype(np.float64)
        report = error_rates(scores, labels, costs, backend)
        if calibration is not None:
            report = _calibrated(report, scores, labels, costs, calibration, backend)
        if bootstrap is not None:
            report["ci"] = _bootstrap_ci(_trial_pairs(trials_path), scores, labels, costs, calibration, backend, bootstrap)
        return report
    pairs, labels, ia, ib, me, mt = _read_trials(trials_path, enroll, test, mean)
    snorm = enroll_stats is not None or test_stats is not None
    if snorm:
        assert enroll_stats is not None and test_stats is not None, "S-norm needs both statistics tables"
        ie, emu, esd = _stats_tables(enroll_stats, (a for a, _ in pairs))
        it, tmu, tsd = _stats_tables(test_stats, (b for _, b in pairs))
        ja = np.fromiter((ie[a] for a, _ in pairs), dtype=np.int32, count=len(pairs))
        jb = np.fromiter((it[b] for _, b in pairs), dtype=np.int32, count=len(pairs))
    if backend == "hip":
        import torch
        scores = _device_cosine(me, mt, ia, ib, test is enroll)
        scores = _snorm_device(scores, ja, jb, emu, esd, tmu, tsd) if snorm else scores.to(torch.float64)   # (widening: exact)
    else:
        assert backend == "host", backend
        scores = cosine_score(enroll, test, trials_path, mean)[0].astype(np.float64)
        if snorm:
            scores = _snorm_host(scores, ja, jb, emu, esd, tmu, tsd)
    report = error_rates(scores, labels, costs, backend)
    if calibration is not None:
        report = _calibrated(report, scores, labels, costs, calibration, backend)
    if bootstrap is not None:
        report["ci"] = _bootstrap_ci(pairs, scores, labels, costs, calibration, backend, bootstrap)
    if score_path:
        host = scores.cpu().numpy() if backend == "hip" else scores
        with open(score_path, "w") as f:
            for (a, b), v in zip(pairs, host.tolist()):
                f.write("{} {} {}\n".format(a, b, v))
    return report


# ---- speaker-level bootstrap intervals of the report (bootstrap.py) ------------------------------------------
from .bootstrap import (bootstrap_compare, bootstrap_counts, bootstrap_replicates, bootstrap_report, match_scores,  # noqa: E402,F401
                        trial_units)
