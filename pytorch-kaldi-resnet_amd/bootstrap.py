"""Speaker-level bootstrap of the evaluation report: percentile intervals for the EER, every minDCF and every actDCF, and for the
difference of two systems scored on the same trials.

Speakers are the independent units, so speakers are resampled: a replicate is a row of counts c [U] (how often each unit was drawn) and
a trial between units a and b weighs c[a] c[b], or c[a] when a = b.  One replicate is scoring._sweep_host with these weights in place
of ones: exact integer counts, rates and costs in float64 in the same order of operations, the lowest position winning every tie.  Two
back ends give the same doubles and integers for every replicate: `host` (numpy, one vectorised sweep per replicate) and `hip`
(csrc/boot.hip through ops.py: the sorted list stays on the device and groups of replicates sweep it together).  The intervals come
from one host function for both.
"""
import numpy as np

MAX_UNITS = 65535
MAX_COUNT = 65535
MAX_COSTS = 8
_M64 = (1 << 64) - 1
_NAN = float("nan")


# ---- the counts table -------------------------------------------------------------------------------------------------------------
def _splitmix64(x):
    """SplitMix64's output function on uint64 arrays (arithmetic modulo 2^64)"""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def bootstrap_counts(U, R, seed=0):
    """int64 [R][U]: row r is the histogram of U draws with replacement from U units.  Draw j of row r is unit
    (high 32 bits of h * U) >> 32 with h = mix(mix(mix(seed) + r) + j), mix = SplitMix64, everything modulo 2^64: a counter-based hash,
    so the table depends on (U, R, seed) alone and row r does not depend on R."""
    U, R = int(U), int(R)
    if not 1 <= U <= MAX_UNITS:
        raise ValueError("U=%d units, must lie in [1, %d]" % (U, MAX_UNITS))
    if R < 1:
        raise ValueError("replicates=%d, at least 1" % R)
    with np.errstate(over="ignore"):
        s = _splitmix64(np.array([int(seed) & _M64], dtype=np.uint64))
        rows = _splitmix64(s + np.arange(R, dtype=np.uint64))
        out = np.empty((R, U), dtype=np.int64)
        j = np.arange(U, dtype=np.uint64)
        for r in range(R):
            h = _splitmix64(rows[r] + j)
            unit = ((h >> np.uint64(32)) * np.uint64(U)) >> np.uint64(32)
            out[r] = np.bincount(unit.astype(np.int64), minlength=U)
    return out


# ---- units ------------------------------------------------------------------------------------------------------------------------
def read_utt2spk(path):
    m = {}
    for ln, line in enumerate(open(path), 1):
        w = line.split()
        if not w:
            continue
        if len(w) != 2:
            raise ValueError("%s:%d: expected '<id> <speaker>'" % (path, ln))
        m[w[0]] = w[1]
    return m


def trial_units(pairs, utt2spk=None):
    """(ua, ub, unit_names): the unit of the enrolment and of the test id of every trial, int32 in [0, U), both sides in one unit space,
    units numbered in order of first appearance.  utt2spk: a dict id -> speaker or such a file; without it every id is its own unit."""
    if isinstance(utt2spk, str):
        utt2spk = read_utt2spk(utt2spk)
    index, names = {}, []

    def unit(utt):
        if utt2spk is None:
            spk = utt
        else:
            spk = utt2spk.get(utt)
            if spk is None:
                raise ValueError("%s is not assigned to any speaker" % utt)
        k = index.get(spk)
        if k is None:
            k = index[spk] = len(names)
            names.append(spk)
        return k
    ua = np.empty(len(pairs), dtype=np.int32)
    ub = np.empty(len(pairs), dtype=np.int32)
    for t, (a, b) in enumerate(pairs):
        ua[t] = unit(a)
        ub[t] = unit(b)
    if len(names) > MAX_UNITS:
        raise ValueError("%d units, at most %d" % (len(names), MAX_UNITS))
    return ua, ub, names


# ---- checks -----------------------------------------------------------------------------------------------------------------------
def _costs(costs, what):
    costs = [tuple(float(v) for v in c) for c in costs]
    if len(costs) > MAX_COSTS:
        raise ValueError("at most %d %s cost triples per call (P <= %d)" % (MAX_COSTS, what, MAX_COSTS))
    for p, c_miss, c_fa in costs:
        if not (0.0 < p < 1.0) or not c_miss > 0 or not c_fa > 0:
            raise ValueError("a cost triple needs 0 < p_target < 1, c_miss > 0 and c_fa > 0")
    return costs


def _is_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "is_cuda")


def _check(scores, labels, ua, ub, counts):
    """-> (T, lab uint8, ua, ub int32, counts int64 [R][U], largest count); every refusal of section 6t that needs no score value"""
    lab = np.ascontiguousarray(np.asarray(labels) != 0, dtype=np.uint8).reshape(-1)
    T = lab.size
    n = scores.numel() if _is_tensor(scores) else np.asarray(scores).size
    if n != T:
        raise ValueError("%d scores for %d labels" % (n, T))
    if T < 2 or T >= 1 << 31:
        raise ValueError("T=%d trials, must lie in [2, 2^31)" % T)
    n_tar = int(lab.sum())
    if n_tar == 0 or n_tar == T:
        raise ValueError("the bootstrap needs at least one target and one non-target trial")
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[0] < 1 or c.dtype.kind not in "iu":
        raise ValueError("counts must be an integer table [R][U]")
    c = np.ascontiguousarray(c, dtype=np.int64)
    U = c.shape[1]
    if not 1 <= U <= MAX_UNITS:
        raise ValueError("U=%d units, must lie in [1, %d]" % (U, MAX_UNITS))
    cmax = int(c.max())
    if int(c.min()) < 0 or cmax > MAX_COUNT:
        raise ValueError("a count lies outside [0, %d]" % MAX_COUNT)
    if cmax * cmax * T >= 1 << 53:
        raise ValueError("max(counts)^2 * T = %d^2 * %d reaches 2^53: the weighted counts would not be exact in a double" % (cmax, T))
    ua = np.ascontiguousarray(ua, dtype=np.int64).reshape(-1)
    ub = np.ascontiguousarray(ub, dtype=np.int64).reshape(-1)
    if ua.size != T or ub.size != T:
        raise ValueError("%d / %d unit ids for %d trials" % (ua.size, ub.size, T))
    if min(int(ua.min()), int(ub.min())) < 0 or max(int(ua.max()), int(ub.max())) >= U:
        raise ValueError("a unit id lies outside [0, %d)" % U)
    return T, lab, ua.astype(np.int32), ub.astype(np.int32), c, cmax


# ---- the replicates ---------------------------------------------------------------------------------------------------------------
def _replicates_host(s, lab, ua, ub, counts, costs, act_costs):
    from . import calibration as cal
    T, R, P, Pa = len(s), counts.shape[0], len(costs), len(act_costs)
    order = np.lexsort((np.arange(T), s + 0.0))
    sa, sb, sl = ua[order].astype(np.int64), ub[order].astype(np.int64), lab[order].astype(np.int64)
    same = sa == sb
    q = [int(np.count_nonzero(s < cal.bayes_threshold(*c))) for c in act_costs]
    out_d = np.full((R, 1 + P + Pa), _NAN, dtype=np.float64)
    out_i = np.full((R, 4 + P + 2 * Pa), -1, dtype=np.int64)
    for r in range(R):
        c = counts[r]
        w = np.where(same, c[sa], c[sa] * c[sb])
        wt = w * sl
        ct = np.cumsum(wt, dtype=np.int64)
        cn = np.cumsum(w - wt, dtype=np.int64)
        n_tar, n_non = int(ct[-1]), int(cn[-1])
        out_i[r, 1], out_i[r, 2] = n_tar, n_non
        if n_tar == 0 or n_non == 0:
            out_i[r, 0] = 1
            continue
        fnr = ct / float(n_tar)
        fpr = 1 - cn / float(n_non)
        i = int(np.argmin(np.abs(fnr - fpr)))
        out_d[r, 0] = max(fpr[i], fnr[i])
        out_i[r, 0], out_i[r, 3] = 0, i
        for m, (p, c_miss, c_fa) in enumerate(costs):
            cost = c_miss * fnr * p + c_fa * fpr * (1 - p)
            j = int(np.argmin(cost))
            out_d[r, 1 + m] = cost[j] / min(c_miss * p, c_fa * (1 - p))
            out_i[r, 4 + m] = j
        for m, (p, c_miss, c_fa) in enumerate(act_costs):
            miss = int(ct[q[m] - 1]) if q[m] else 0
            fa = n_non - (int(cn[q[m] - 1]) if q[m] else 0)
            out_d[r, 1 + P + m] = cal._act_dcf_value(miss, fa, n_tar, n_non, p, c_miss, c_fa)
            out_i[r, 4 + P + m], out_i[r, 4 + P + Pa + m] = miss, fa
    return out_d, out_i


def _replicates_device(scores, lab, ua, ub, counts, cmax, costs, act_costs, chunk):
    import torch
    from . import calibration as cal, ops
    dev = scores.device
    order = ops.sort_trials(scores)                                    # ValueError on NaN
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)    # noqa: E731
    U = counts.shape[1]
    rec, q = ops.boot_pack(scores, up(lab), order, up(ua), up(ub), [cal.bayes_threshold(*c) for c in act_costs], U)
    out_d, out_i = ops.boot_sweep(rec, q, ops.boot_table(counts, dev), U, cmax, costs, act_costs, chunk=chunk)
    return out_d.cpu().numpy(), out_i.cpu().numpy()


def bootstrap_replicates(scores, labels, ua, ub, counts, costs=None, act_costs=(), backend="host", chunk=None):
    """Every replicate of the weighted sweep.  scores [T] float64 without NaN (on `hip` possibly a float64 device tensor), labels [T],
    ua / ub [T] in [0, U), counts [R][U] of integers in [0, 65 535] with max(counts)^2 T < 2^53; costs: P <= 8 triples (p_target,
    c_miss, c_fa) of the minimum costs, act_costs: Pa <= 8 triples of the actual costs (the scores read as log-likelihood ratios).
    -> {'d': float64 [R][1 + P + Pa] = EER, minDCF [P], actDCF [Pa]; 'i': int64 [R][4 + P + 2 Pa] = flag, n_target, n_nontarget, EER
    position, minDCF positions [P], miss [Pa], fa [Pa]} and the same columns by name.  A flagged (degenerate) replicate has no target
    or no non-target weight: its doubles are NaN, its positions and counts -1.  chunk: replicates per launch sequence on `hip`."""
    from . import scoring
    if backend not in ("host", "hip"):
        raise ValueError("backend must be host or hip, not %r" % (backend,))
    costs = _costs(scoring.DEFAULT_COSTS if costs is None else costs, "minDCF")
    act_costs = _costs(act_costs, "actDCF")
    T, lab, ua, ub, counts, cmax = _check(scores, labels, ua, ub, counts)
    if backend == "hip":
        import torch
        if not torch.is_tensor(scores):
            s = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
            if np.isnan(s).any():
                raise ValueError("a score is NaN")
            scores = torch.from_numpy(s).cuda()
        if scores.dtype != torch.float64 or not scores.is_cuda:
            raise ValueError("the hip back end takes float64 device tensors")
        d, i = _replicates_device(scores.reshape(-1).contiguous(), lab, ua, ub, counts, cmax, costs, act_costs, chunk)
    else:
        s = np.ascontiguousarray(scores.cpu().numpy() if _is_tensor(scores) else scores, dtype=np.float64).reshape(-1)
        if np.isnan(s).any():
            raise ValueError("a score is NaN")
        d, i = _replicates_host(s, lab, ua, ub, counts, costs, act_costs)
    P, Pa = len(costs), len(act_costs)
    return {"d": d, "i": i, "costs": costs, "act_costs": act_costs, "degenerate": i[:, 0] != 0, "n_target": i[:, 1], "n_nontarget": i[:, 2],
            "eer": d[:, 0], "eer_index": i[:, 3], "min_dcf": d[:, 1:1 + P], "min_dcf_index": i[:, 4:4 + P], "act_dcf": d[:, 1 + P:],
            "miss": i[:, 4 + P:4 + P + Pa], "fa": i[:, 4 + P + Pa:]}


# ---- intervals --------------------------------------------------------------------------------------------------------------------
def interval(values, valid, alpha=0.05):
    """percentile interval of the valid replicates: numpy.quantile at alpha / 2 and 1 - alpha / 2 (linear interpolation), with the
    bootstrap mean and standard deviation"""
    v = np.asarray(values, dtype=np.float64)[np.asarray(valid, dtype=bool)]
    lo, hi = np.quantile(v, [alpha / 2, 1 - alpha / 2])
    return {"lo": float(lo), "hi": float(hi), "mean": float(np.mean(v)), "std": float(np.std(v))}


def _guard(rep, alpha, max_degenerate):
    if not 0.0 < alpha < 1.0:
        raise ValueError("alpha must lie in (0, 1), not %r" % (alpha,))
    R, bad = len(rep["degenerate"]), int(rep["degenerate"].sum())
    if R - bad < 2:
        raise ValueError("%d of %d replicates are degenerate (no target or no non-target weight): fewer than 2 are left" % (bad, R))
    if bad > max_degenerate * R:
        raise ValueError("%d of %d replicates are degenerate (no target or no non-target weight), more than the share %g allowed"
                         % (bad, R, max_degenerate))
    return R, bad


def _table(counts, replicates, seed, U):
    if counts is None:
        return bootstrap_counts(U, replicates, seed)
    return counts


def bootstrap_report(scores, labels, ua, ub, costs=None, act_costs=(), replicates=1000, seed=0, alpha=0.05, max_degenerate=0.05,
                     counts=None, backend="host", units=None):
    """Point estimates (scoring.error_rates / calibration.evaluate, unchanged) with the bootstrap interval of each:
    {'eer', 'min_dcf': [...], 'act_dcf': [...]: {'value', 'lo', 'hi', 'mean', 'std'}, 'replicates', 'degenerate', 'alpha', 'units',
    'values': the bootstrap_replicates result}.  counts: an explicit table instead of bootstrap_counts(units, replicates, seed); units
    (default: largest unit id + 1).  ValueError when more than max_degenerate of the replicates are degenerate or fewer than 2 are valid."""
    from . import calibration as cal, scoring
    costs = _costs(scoring.DEFAULT_COSTS if costs is None else costs, "minDCF")
    act_costs = _costs(act_costs, "actDCF")
    U = int(units) if units is not None else int(max(np.max(ua), np.max(ub))) + 1
    counts = _table(counts, replicates, seed, U)
    rep = bootstrap_replicates(scores, labels, ua, ub, counts, costs, act_costs, backend)
    R, bad = _guard(rep, alpha, max_degenerate)
    point = scoring.error_rates(scores, labels, costs, backend)
    ok = ~rep["degenerate"]
    out = {"eer": dict(value=point["eer"], **interval(rep["eer"], ok, alpha)),
           "min_dcf": [dict(value=point["min_dcf"][m][0], **interval(rep["min_dcf"][:, m], ok, alpha)) for m in range(len(costs))],
           "act_dcf": [], "replicates": R, "degenerate": bad, "alpha": alpha, "units": int(np.asarray(counts).shape[1]),
           "costs": costs, "act_costs": act_costs, "values": rep}
    if act_costs:
        ev = cal.evaluate(scores, labels, act_costs, backend)
        out["act_dcf"] = [dict(value=ev["act_dcf"][m]["act_dcf"], **interval(rep["act_dcf"][:, m], ok, alpha)) for m in range(len(act_costs))]
    return out


def match_scores(pairs_a, scores_a, pairs_b, scores_b):
    """scores_b in the order of pairs_a: the two lists are matched by (utt1, utt2); a pair that one list lacks is an error"""
    where = {}
    for t, p in enumerate(pairs_b):
        if p in where:
            raise ValueError("trial '%s %s' appears twice in the second score list" % p)
        where[p] = t
    if len(pairs_a) != len(set(pairs_a)):
        raise ValueError("a trial appears twice in the first score list")
    idx = np.empty(len(pairs_a), dtype=np.int64)
    for t, p in enumerate(pairs_a):
        if p not in where:
            raise ValueError("trial '%s %s' is missing from the second score list" % p)
        idx[t] = where[p]
    if len(pairs_b) != len(pairs_a):
        extra = next(p for p in pairs_b if p not in set(pairs_a))
        raise ValueError("trial '%s %s' is missing from the first score list" % extra)
    return np.asarray(scores_b, dtype=np.float64)[idx]


def bootstrap_compare(scores_a, scores_b, labels, ua, ub, costs=None, act_costs=(), replicates=1000, seed=0, alpha=0.05,
                      max_degenerate=0.05, counts=None, backend="host", units=None):
    """Two systems on the same trials (same order: match_scores) under the same table: {'a', 'b': bootstrap_report of each, 'diff':
    {'eer', 'min_dcf': [...], 'act_dcf': [...]: {'value', 'lo', 'hi', 'mean', 'std', 'below_zero'}} of the per-replicate difference
    A - B; below_zero: the share of valid replicates with a difference < 0}"""
    U = int(units) if units is not None else int(max(np.max(ua), np.max(ub))) + 1
    counts = _table(counts, replicates, seed, U)
    kw = dict(costs=costs, act_costs=act_costs, alpha=alpha, max_degenerate=max_degenerate, counts=counts, backend=backend)
    a = bootstrap_report(scores_a, labels, ua, ub, **kw)
    b = bootstrap_report(scores_b, labels, ua, ub, **kw)
    ok = ~(a["values"]["degenerate"] | b["values"]["degenerate"])

    def diff(pa, pb, va, vb):
        d = np.where(ok, va, 0.0) - np.where(ok, vb, 0.0)
        return dict(value=pa - pb, below_zero=float(np.mean(d[ok] < 0)), **interval(d, ok, alpha))
    out = {"eer": diff(a["eer"]["value"], b["eer"]["value"], a["values"]["eer"], b["values"]["eer"]), "min_dcf": [], "act_dcf": []}
    for key in ("min_dcf", "act_dcf"):
        for m in range(len(a[key])):
            out[key].append(diff(a[key][m]["value"], b[key][m]["value"], a["values"][key][:, m], b["values"][key][:, m]))
    return {"a": a, "b": b, "diff": out}


# ---- text -------------------------------------------------------------------------------------------------------------------------
def report_lines(rep, diff=None):
    """the lines scripts/bootstrap_ci.py prints: the report's percent / four-digit formats with '[lo, hi]' behind each value"""
    pc = lambda e: "%.4f%% [%.4f, %.4f]" % (100 * e["value"], 100 * e["lo"], 100 * e["hi"])      # noqa: E731
    ab = lambda e: "%.4f [%.4f, %.4f]" % (e["value"], e["lo"], e["hi"])                           # noqa: E731
    lines = ["EER: " + pc(rep["eer"])]
    lines += ["minDCF(p-target=%s): %s" % (_g(c[0]), ab(e)) for c, e in zip(rep["costs"], rep["min_dcf"])]
    lines += ["actDCF(p-target=%s): %s" % (_g(c[0]), ab(e)) for c, e in zip(rep["act_costs"], rep["act_dcf"])]
    lines.append("degenerate replicates: %d of %d (%d units, %g%% intervals)" % (rep["degenerate"], rep["replicates"], rep["units"],
                                                                                100 * (1 - rep["alpha"])))
    if diff is not None:
        tail = lambda e: " P(<0)=%.4f" % e["below_zero"]                                           # noqa: E731
        lines.append("EER(A-B): " + pc(diff["eer"]) + tail(diff["eer"]))
        lines += ["minDCF(A-B, p-target=%s): %s" % (_g(c[0]), ab(e) + tail(e)) for c, e in zip(rep["costs"], diff["min_dcf"])]
        lines += ["actDCF(A-B, p-target=%s): %s" % (_g(c[0]), ab(e) + tail(e)) for c, e in zip(rep["act_costs"], diff["act_dcf"])]
    return lines


def _g(p):
    return repr(float(p))


def write_replicates(path, rep):
    """one line per replicate: flag, n_target, n_nontarget, then every double as repr (round-trips), under a header line"""
    P, Pa = len(rep["costs"]), len(rep["act_costs"])
    with open(path, "w") as f:
        f.write("# degenerate n_target n_nontarget eer" + "".join(" min_dcf_%d" % m for m in range(P))
                + "".join(" act_dcf_%d" % m for m in range(Pa)) + "\n")
        for r in range(rep["d"].shape[0]):
            f.write("%d %d %d %s\n" % (rep["i"][r, 0], rep["i"][r, 1], rep["i"][r, 2], " ".join(repr(float(v)) for v in rep["d"][r])))
