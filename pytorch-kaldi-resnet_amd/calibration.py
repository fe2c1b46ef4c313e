"""Calibration and fusion of trial scores: an affine map llr = w . s + b of K systems' scores trained by
prior-weighted logistic regression, and what judges the result as log-likelihood ratios: Cllr, minCllr (pool-adjacent-violators)
and the detection cost at the Bayes threshold (actDCF).

Two back ends of one rule.  `host` is numpy fp64.  `hip` (csrc/cal.hip through ops.py) takes float64 device tensors or numpy arrays;
apply, the miss / false-alarm counts, the actDCF doubles and the PAV pools are the host's bit for bit and integer for integer,
the sums that pass through exp / log1p (Cllr, minCllr, training) agree to the bounds of section 6s.
"""
import math

import numpy as np

MAX_K = 8
MAX_COSTS = 8
LN2 = math.log(2.0)
STATUS = ("running", "converged", "not_converged", "singular")
MODEL_VERSION = "spk-calibration 1"


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _is_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "is_cuda")


def _labels(labels, T):
    lab = np.ascontiguousarray(np.asarray(labels) != 0, dtype=np.uint8).reshape(-1)
    if lab.size != T:
        raise ValueError("%d labels for %d trials" % (lab.size, T))
    n_tar = int(lab.sum())
    if n_tar == 0 or n_tar == T:
        raise ValueError("calibration needs at least one target and one non-target trial")
    return lab, n_tar


def _host_columns(columns):
    """-> float64 [K][T], finite"""
    if _is_tensor(columns):
        columns = columns.cpu().numpy()
    if isinstance(columns, (list, tuple)):
        columns = [c.cpu().numpy() if _is_tensor(c) else c for c in columns]
    c = np.ascontiguousarray(columns, dtype=np.float64)
    if c.ndim == 1:
        c = c[None]
    if c.ndim != 2 or not 1 <= c.shape[0] <= MAX_K:
        raise ValueError("columns must be [K][T] with 1 <= K <= %d, got shape %s" % (MAX_K, c.shape))
    if not np.isfinite(c).all():
        raise ValueError("a score is NaN or infinite")
    return c


def _device_columns(columns):
    """-> float64 device tensor [K][T], finite"""
    import torch
    if isinstance(columns, (list, tuple)) and any(_is_tensor(c) for c in columns):
        columns = torch.stack([c if _is_tensor(c) else torch.from_numpy(np.asarray(c, dtype=np.float64)).cuda() for c in columns])
    if not _is_tensor(columns):
        return torch.from_numpy(_host_columns(columns)).cuda()
    c = columns if columns.dim() == 2 else columns.reshape(1, -1)
    if c.dtype != torch.float64 or not c.is_cuda:
        raise ValueError("the hip back end takes float64 device tensors")
    if not 1 <= c.shape[0] <= MAX_K:
        raise ValueError("columns must be [K][T] with 1 <= K <= %d, got shape %s" % (MAX_K, tuple(c.shape)))
    if not bool(torch.isfinite(c).all()):
        raise ValueError("a score is NaN or infinite")
    return c.contiguous()


def _vector(x, backend):
    """one float64 column [T] on the back end's side"""
    c = _device_columns(x) if backend == "hip" else _host_columns(x)
    if c.shape[0] != 1:
        raise ValueError("one column of numbers is needed, got %d" % c.shape[0])
    return c[0]


def _check_backend(backend):
    if backend not in ("host", "hip"):
        raise ValueError("backend must be host or hip, not %r" % (backend,))


def _costs(costs):
    costs = [tuple(float(v) for v in c) for c in costs]
    if len(costs) > MAX_COSTS:
        raise ValueError("at most %d cost triples per call" % MAX_COSTS)
    for p, c_miss, c_fa in costs:
        if not (0.0 < p < 1.0) or not c_miss > 0 or not c_fa > 0:
            raise ValueError("a cost triple needs 0 < p_target < 1, c_miss > 0 and c_fa > 0")
    return costs


def bayes_threshold(p_target, c_miss=1.0, c_fa=1.0):
    """eta = log(c_fa (1 - p)) - log(c_miss p): computed here, once, and handed to either back end as these bits"""
    return math.log(c_fa * (1.0 - p_target)) - math.log(c_miss * p_target)


def logit(p):
    return math.log(p / (1.0 - p))


# ---- the model -------------------------------------------------------------------------------------------------------------------------
class Model:
    """llr = ((weights[0] s0 + weights[1] s1) + ...) + bias"""

    def __init__(self, weights, bias, p_target=0.01, l2=0.0, status="loaded", evaluations=0, objective=float("nan")):
        self.weights = [float(w) for w in weights]
        self.bias = float(bias)
        self.p_target = float(p_target)
        self.l2 = float(l2)
        self.status = status
        self.evaluations = int(evaluations)
        self.objective = float(objective)
        if not 1 <= len(self.weights) <= MAX_K:
            raise ValueError("a model has 1 to %d weights, not %d" % (MAX_K, len(self.weights)))

    @property
    def theta(self):
        return np.array(self.weights + [self.bias], dtype=np.float64)

    def __repr__(self):
        return "Model(weights=%r, bias=%r, p_target=%r, l2=%r, status=%r, evaluations=%d)" % (
            self.weights, self.bias, self.p_target, self.l2, self.status, self.evaluations)


def save(model, path):
    with open(path, "w") as f:
        f.write(MODEL_VERSION + "\n")
        f.write("p_target %.17g\nl2 %.17g\nsystems %d\n" % (model.p_target, model.l2, len(model.weights)))
        for w in model.weights:
            f.write("weight %.17g\n" % w)
        f.write("bias %.17g\n" % model.bias)


def load(path):
    lines = [l.strip() for l in open(path)]
    lines = [l for l in lines if l]

    def field(i, name, conv):
        if i >= len(lines) or lines[i].split()[0] != name or len(lines[i].split()) != 2:
            raise ValueError("%s: line %d should be '%s <value>'" % (path, i + 1, name))
        try:
            return conv(lines[i].split()[1])
        except ValueError:
            raise ValueError("%s: line %d: bad value for %s" % (path, i + 1, name))
    if not lines or lines[0] != MODEL_VERSION:
        raise ValueError("%s: not a calibration model (first line should be %r)" % (path, MODEL_VERSION))
    p, l2, K = field(1, "p_target", float), field(2, "l2", float), field(3, "systems", int)
    if not 1 <= K <= MAX_K:
        raise ValueError("%s: systems %d outside [1, %d]" % (path, K, MAX_K))
    weights = [field(4 + k, "weight", float) for k in range(K)]
    bias = field(4 + K, "bias", float)
    if len(lines) != 5 + K:
        raise ValueError("%s: %d lines after the bias" % (path, len(lines) - 5 - K))
    return Model(weights, bias, p, l2)


def _theta(model_or_theta, K):
    th = model_or_theta.theta if isinstance(model_or_theta, Model) else np.ascontiguousarray(model_or_theta, dtype=np.float64).reshape(-1)
    if th.size != K + 1:
        raise ValueError("%d columns for a model of %d systems" % (K, th.size - 1))
    if not np.isfinite(th).all():
        raise ValueError("a model parameter is NaN or infinite")
    return th


# ---- apply -----------------------------------------------------------------------------------------------------------------------------
def _apply_host(c, th):
    z = th[0] * c[0]
    for k in range(1, c.shape[0]):
        z = z + th[k] * c[k]
    return z + th[-1]


def apply(model, columns, backend="host"):
    """columns [K][T] (or one column [T]) -> llr [T] float64: a device tensor on `hip` when device tensors came in, else numpy"""
    _check_backend(backend)
    if backend == "hip":
        from . import ops
        c = _device_columns(columns)
        out = ops.cal_apply(c, _theta(model, c.shape[0]))
        return out if _is_tensor(columns) or (isinstance(columns, (list, tuple)) and any(_is_tensor(x) for x in columns)) else out.cpu().numpy()
    c = _host_columns(columns)
    return _apply_host(c, _theta(model, c.shape[0]))


# ---- Cllr and actDCF -------------------------------------------------------------------------------------------------------------------
def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _act_dcf_value(miss, fa, n_tar, n_non, p, c_miss, c_fa):
    """the order of operations of scoring._sweep_host"""
    fnr, fpr = miss / float(n_tar), fa / float(n_non)
    return float((c_miss * fnr * p + c_fa * fpr * (1 - p)) / min(c_miss * p, c_fa * (1 - p)))


def evaluate(llr, labels, costs=(), backend="host"):
    """One pass: {'cllr', 'sum_target', 'sum_nontarget', 'n_target', 'n_nontarget', 'act_dcf': [{'act_dcf', 'miss', 'fa', 'threshold'}]}"""
    _check_backend(backend)
    costs = _costs(costs)
    eta = [bayes_threshold(*c) for c in costs]
    x = _vector(llr, backend)
    lab, n_tar = _labels(labels, x.shape[0])
    if x.shape[0] < 2:
        raise ValueError("at least two trials are needed")
    if backend == "hip":
        import torch
        from . import ops
        out_d, out_i = ops.cal_cllr(x, torch.from_numpy(lab).to(x.device), costs, eta)
        d, i = out_d.cpu().tolist(), out_i.cpu().tolist()
        P = len(costs)
        st, sn, n_t, n_n = d[0], d[1], i[0], i[1]
        act = [{"act_dcf": d[2 + m], "miss": i[2 + m], "fa": i[2 + P + m], "threshold": eta[m]} for m in range(P)]
    else:
        tar = lab != 0
        st, sn = float(np.sum(_softplus(-x[tar]))), float(np.sum(_softplus(x[~tar])))
        n_t, n_n = n_tar, x.size - n_tar
        act = []
        for (p, c_miss, c_fa), e in zip(costs, eta):
            miss, fa = int(np.count_nonzero(x[tar] < e)), int(np.count_nonzero(x[~tar] >= e))
            act.append({"act_dcf": _act_dcf_value(miss, fa, n_t, n_n, p, c_miss, c_fa), "miss": miss, "fa": fa, "threshold": e})
    return {"cllr": (st / n_t + sn / n_n) / (2 * LN2), "sum_target": st, "sum_nontarget": sn, "n_target": n_t, "n_nontarget": n_n,
            "act_dcf": act}


def cllr(llr, labels, backend="host"):
    """(mean over targets of softplus(-llr) + mean over non-targets of softplus(llr)) / (2 ln 2)"""
    return evaluate(llr, labels, (), backend)["cllr"]


def act_dcf(llr, labels, p_target=0.01, c_miss=1, c_fa=1, backend="host"):
    """the detection cost at the Bayes threshold of (p_target, c_miss, c_fa), normalised as minDCF is"""
    return evaluate(llr, labels, ((p_target, c_miss, c_fa),), backend)["act_dcf"][0]["act_dcf"]


# ---- minCllr ----------------------------------------------------------------------------------------------------------------------------
def tie_pools(scores, labels):
    """host: (pools int64 [P0][2] = (targets, trials) of every run of equal scores in ascending order, order, first position of each)"""
    s = _vector(scores, "host")
    lab, _ = _labels(labels, s.size)
    order = np.lexsort((np.arange(s.size), s + 0.0))                 # stable; -0.0 equals +0.0
    ss = s[order]
    flag = np.ones(s.size, dtype=bool)
    flag[1:] = ss[1:] != ss[:-1]
    start = np.flatnonzero(flag)
    ct = np.concatenate([[0], np.cumsum(lab[order], dtype=np.int64)])
    bounds = np.concatenate([start, [s.size]])
    pools = np.stack([ct[bounds[1:]] - ct[bounds[:-1]], bounds[1:] - bounds[:-1]], axis=1).astype(np.int64)
    return pools, order, start


def pav_pools(pools):
    """The rule on a list of pools (t, n): adjacent pools merge while t_prev n_next >= t_next n_prev (int64 products) -> the unique
    list with strictly increasing t / n.  Whole runs of violating neighbours merge per round: the order of merging does not change
    the answer (tests/cal_ref.py states it as the minimax formula)."""
    p = np.ascontiguousarray(pools, dtype=np.int64).reshape(-1, 2)
    while p.shape[0] > 1:
        viol = p[:-1, 0] * p[1:, 1] >= p[1:, 0] * p[:-1, 1]          # pool i + 1 joins pool i
        if not viol.any():
            break
        head = np.flatnonzero(np.concatenate([[True], ~viol]))
        p = np.add.reduceat(p, head, axis=0)
    return p


def _min_cllr_value(pools, n_tar, n_non):
    t, n = pools[:, 0], pools[:, 1]
    m = (t > 0) & (t < n)
    dt, dn = t[m].astype(np.float64), (n[m] - t[m]).astype(np.float64)
    d_tar, d_non = float(n_tar), float(n_non)
    a = float(np.sum(dt * np.log1p((dn / dt) * (d_tar / d_non))))
    b = float(np.sum(dn * np.log1p((dt / dn) * (d_non / d_tar))))
    return ((1.0 / d_tar) * a + (1.0 / d_non) * b) / (2.0 * LN2)


def min_cllr(scores, labels, backend="host", details=False):
    """-> (minCllr, pools int64 [P][2] = (targets, trials) with t / n strictly increasing, pool index of every trial); details: a
    fourth item {'tie_pools', 'counts'}: the pools of equal scores and the pool count after every stage"""
    _check_backend(backend)
    s = _vector(scores, backend)
    lab, n_tar = _labels(labels, s.shape[0])
    if backend == "hip":
        import torch
        from . import ops
        order = ops.sort_trials(s)
        r = ops.cal_pav(s, torch.from_numpy(lab).to(s.device), order)
        counts = r["counts"].cpu().tolist()
        pools = r["pools"][:counts[3]].cpu().numpy()
        pool_of = r["pool_of"] if _is_tensor(scores) else r["pool_of"].cpu().numpy()
        out = (float(r["min_cllr"].cpu()[0]), pools, pool_of)
        return out + ({"tie_pools": r["tie"][:counts[0]].cpu().numpy(), "counts": counts[:4]},) if details else out
    tie, order, start = tie_pools(s, lab)
    pools = pav_pools(tie)
    cum = np.concatenate([[0], np.cumsum(pools[:, 1])])
    pool_of = np.empty(s.size, dtype=np.int32)
    pool_of[order] = np.searchsorted(cum, np.arange(s.size), side="right") - 1
    out = (_min_cllr_value(pools, n_tar, s.size - n_tar), pools, pool_of)
    return out + ({"tie_pools": tie, "counts": [tie.shape[0], tie.shape[0], tie.shape[0], pools.shape[0]]},) if details else out


# ---- training --------------------------------------------------------------------------------------------------------------------------
def objective_terms(c, lab, theta, p_target, l2, n_tar=None):
    """host: (f, g [K + 1], H [K + 1][K + 1]) of the objective of section 6s at theta, the evaluation pass of the state machine"""
    K, T = c.shape
    n_tar = int(lab.sum()) if n_tar is None else n_tar
    tau = logit(p_target)
    tar = lab != 0
    x = _apply_host(c, theta) + tau
    y = np.where(tar, -x, x)
    e = np.exp(-np.abs(y))
    den = 1.0 + e
    sig = np.where(y >= 0, 1.0, e) / den
    cw = np.where(tar, p_target / float(n_tar), (1.0 - p_target) / float(T - n_tar))
    cd, ch = cw * np.where(tar, -sig, sig), cw * (e / (den * den))
    S = np.concatenate([c, np.ones((1, T))])
    w = theta[:K]
    ww = 0.0
    for k in range(K):
        ww = ww + w[k] * w[k]
    f = float(np.sum(cw * (np.maximum(y, 0.0) + np.log1p(e)))) + 0.5 * l2 * ww
    g = np.array([float(np.sum(cd * S[j])) for j in range(K + 1)])
    H = np.zeros((K + 1, K + 1))
    for j in range(K + 1):
        chj = ch * S[j]
        for k in range(j + 1):
            H[j, k] = H[k, j] = float(np.sum(chj * S[k]))
    g[:K] = g[:K] + l2 * w
    H[np.arange(K), np.arange(K)] += l2
    return f, g, H


def _newton_direction(g, H):
    """Cholesky by rows, then the two triangular solves -> (x = H^-1 g, lambda2 = g . x), or None at a pivot that is not > 0"""
    D = g.size
    L = np.zeros((D, D))
    for j in range(D):
        for k in range(j + 1):
            s = H[j, k]
            for m in range(k):
                s = s - L[j, m] * L[k, m]
            if k == j:
                if not s > 0.0:
                    return None
                L[j, j] = math.sqrt(s)
            else:
                L[j, k] = s / L[k, k]
    x = np.zeros(D)
    for j in range(D):
        s = g[j]
        for m in range(j):
            s = s - L[j, m] * x[m]
        x[j] = s / L[j, j]
    for j in range(D - 1, -1, -1):
        s = x[j]
        for m in range(j + 1, D):
            s = s - L[m, j] * x[m]
        x[j] = s / L[j, j]
    lam = 0.0
    for j in range(D):
        lam = lam + g[j] * x[j]
    return x, lam


def _train_host(c, lab, n_tar, p_target, l2, epsilon, max_iters):
    D = c.shape[0] + 1
    theta, acc, d = np.zeros(D), np.zeros(D), np.zeros(D)
    f_acc, status, evals = float("inf"), 0, 0
    for it in range(max_iters):
        f, g, H = objective_terms(c, lab, theta, p_target, l2, n_tar)
        evals += 1
        if not f <= f_acc:                                   # 1: half the step
            d = 0.5 * d
            theta = acc + d
        else:                                                # 2: accept
            f_acc, acc = f, theta.copy()
            r = _newton_direction(g, H)
            if r is None:
                status = 3
            elif r[1] <= epsilon:                            # 3
                status = 1
            else:                                            # 4
                d = -r[0]
                theta = theta + d
        if status == 0 and it == max_iters - 1:
            status = 2
        if status:
            break
    return acc, status, evals, f_acc


def train(columns, labels, p_target=0.01, l2=0.0, epsilon=1e-18, max_iters=100, backend="host"):
    """Prior-weighted logistic regression of labels on columns [K][T] from theta = 0 (section 6s) -> Model with weights, bias,
    p_target, l2, status ('converged', 'not_converged', 'singular'), evaluations and objective (f at the returned parameters)."""
    _check_backend(backend)
    if not 0.0 < p_target < 1.0 or not l2 >= 0.0 or not epsilon >= 0.0 or not 1 <= int(max_iters) <= 10000:
        raise ValueError("train needs 0 < p_target < 1, l2 >= 0, epsilon >= 0 and 1 <= max_iters <= 10000")
    c = _device_columns(columns) if backend == "hip" else _host_columns(columns)
    lab, n_tar = _labels(labels, c.shape[1])
    if c.shape[1] < 2:
        raise ValueError("at least two trials are needed")
    if backend == "hip":
        import torch
        from . import ops
        state, istate = ops.cal_train(c, torch.from_numpy(lab).to(c.device), n_tar, p_target, logit(p_target), l2, epsilon, int(max_iters))
        st, ist = state.cpu().numpy(), istate.cpu().tolist()
        D = c.shape[0] + 1
        theta, status, evals, f_acc = st[9:9 + D], ist[0], ist[1], float(st[27])
    else:
        theta, status, evals, f_acc = _train_host(c, lab, n_tar, float(p_target), float(l2), float(epsilon), int(max_iters))
    return Model(theta[:-1].tolist(), float(theta[-1]), p_target, l2, STATUS[status], evals, f_acc)


# ---- score files ---------------------------------------------------------------------------------------------------------------------
class ScoreFileError(ValueError):
    pass


def read_score_files(paths):
    """'<utt1> <utt2> <score>' files that list the same trials in the same order -> (pairs, float64 [K][T]); a mismatch names the
    file and the line"""
    pairs, cols = None, []
    for path in paths:
        mine, col = [], []
        with open(path) as f:
            for ln, line in enumerate(f, 1):
                w = line.split()
                if not w:
                    continue
                if len(w) != 3:
                    raise ScoreFileError("%s:%d: expected '<utt1> <utt2> <score>'" % (path, ln))
                try:
                    v = float(w[2])
                except ValueError:
                    raise ScoreFileError("%s:%d: the score %r is not a number" % (path, ln, w[2]))
                if not math.isfinite(v):
                    raise ScoreFileError("%s:%d: the score is NaN or infinite" % (path, ln))
                if pairs is not None and (len(mine) >= len(pairs) or pairs[len(mine)] != (w[0], w[1])):
                    raise ScoreFileError("%s:%d: trial '%s %s' is not the trial at this place in %s" % (path, ln, w[0], w[1], paths[0]))
                mine.append((w[0], w[1]))
                col.append(v)
        if pairs is None:
            pairs = mine
            if not pairs:
                raise ScoreFileError("%s:1: no trials" % path)
        elif len(mine) != len(pairs):
            raise ScoreFileError("%s:%d: the file ends after %d trials, %s has %d" % (path, len(mine) + 1, len(mine), paths[0], len(pairs)))
        cols.append(col)
    return pairs, np.array(cols, dtype=np.float64)


def trial_labels(pairs, trials_path):
    """labels of the pairs from a '<utt1> <utt2> target|nontarget' list, looked up as scoring.read_scored_trials does"""
    trials = {}
    for line in open(trials_path):
        a, b, t = line.rstrip().split()
        trials[(a, b)] = t
    lab = []
    for ln, p in enumerate(pairs, 1):
        if p not in trials:
            raise ScoreFileError("%s: no entry for trial '%s %s' (score line %d)" % (trials_path, p[0], p[1], ln))
        lab.append(1 if trials[p] == "target" else 0)
    return np.array(lab, dtype=np.uint8)
