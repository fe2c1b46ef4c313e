"""Independent numpy fp64 restatement of the PLDA back end: Kaldi's ivector-compute-lda, transform-vec,
ivector-normalize-length, ivector-compute-plda, ivector-copy-plda --smoothing and ivector-plda-scoring as the section states them,
written with plain Python loops over utterances, classes and trials.  `rounded=False` removes every fl32(...) stage rounding (the
archive values themselves stay the float32 data they are).  Also the fp64 references of the csrc/plda.hip kernels with their
per-element error bounds, and the seeded synthetic set both test files use."""
import numpy as np

U53 = 2.0 ** -53


def fl32(a, rounded=True):
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if rounded else a


# ---- the synthetic set ------------------------------------------------------------------------------------------------------------
D, LDA_DIM, EM_ITERS = 24, 16, 10
COUNTS = [1, 1, 2, 2, 3, 3, 3, 5, 7, 7] * 4


def synthetic(seed=11):
    """40 training speakers (136 vectors) and 12 test speakers x 3, D = 24: a rank-10 speaker factor with column scales 2 ... 0.3,
    noise 0.7 with per-dimension scale 0.5 ... 1.5, offset 3, float32 values.  -> dict of train / test keys and matrices, utt2spk,
    mean (float32, of the training set) and trials [(enrol, test, 'target' | 'nontarget')] over all test pairs."""
    rng = np.random.RandomState(seed)
    F = rng.randn(D, 10) * np.linspace(2.0, 0.3, 10)
    ns = np.linspace(0.5, 1.5, D)

    def speaker(n):
        h = rng.randn(10)
        return [(3.0 + F @ h + 0.7 * ns * rng.randn(D)).astype(np.float32) for _ in range(n)]

    tk, tx, utt2spk = [], [], {}
    for s, n in enumerate(COUNTS):
        for u, v in enumerate(speaker(n)):
            tk.append("s%02d-u%d" % (s, u))
            tx.append(v)
            utt2spk[tk[-1]] = "s%02d" % s
    ek, ex = [], []
    for s in range(12):
        for u, v in enumerate(speaker(3)):
            ek.append("t%02d-u%d" % (s, u))
            ex.append(v)
    trials = [(a, b, "target" if a[:3] == b[:3] else "nontarget") for i, a in enumerate(ek) for b in ek[i + 1:]]
    tx, ex = np.stack(tx), np.stack(ex)
    return {"train_keys": tk, "train": tx, "test_keys": ek, "test": ex, "utt2spk": utt2spk,
            "mean": tx.astype(np.float64).mean(axis=0).astype(np.float32), "trials": trials}


def write_text_ark(path, keys, mat):
    with open(path, "w") as f:
        for k, v in zip(keys, mat):
            f.write(k + " [ " + " ".join(str(x) for x in v) + " ]\n")


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def center(x, mean, rounded=True):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    m = x.sum(axis=0) / len(x) if mean is None else np.asarray(mean).astype(np.float32).astype(np.float64)
    return fl32(x - m, rounded)


def _by_speaker(keys, utt2spk):
    spk = {}
    for i, k in enumerate(keys):
        if k in utt2spk:
            spk.setdefault(utt2spk[k], []).append(i)
    return spk


def lda(keys, x0, utt2spk, dim, factor=0.0, floor=1e-6, rounded=True):
    """-> (transform [dim][D+1], eigenvalues descending, within-class covariance)"""
    spk = _by_speaker(keys, utt2spk)
    used = [i for rows in spk.values() for i in rows]
    N, Dd = len(used), x0.shape[1]
    mu = np.zeros(Dd)
    for i in used:
        mu += x0[i]
    mu /= N
    tot, bet = np.zeros((Dd, Dd)), np.zeros((Dd, Dd))
    for i in used:
        tot += np.outer(x0[i] - mu, x0[i] - mu)
    for rows in spk.values():
        a = np.zeros(Dd)
        for i in rows:
            a += x0[i] - mu
        a /= len(rows)
        bet += len(rows) * np.outer(a, a)
    total, within = tot / N, (tot - bet) / N
    between = total - within
    s, U = np.linalg.eigh(factor * total + (1 - factor) * within)
    s = np.maximum(s, s.max() * floor)
    T = np.diag(s ** -0.5) @ U.T
    ev, V = np.linalg.eigh(T @ between @ T.T)
    order = np.argsort(-ev)
    A = V[:, order[:dim]].T @ T
    return fl32(np.concatenate([A, -(A @ mu)[:, None]], axis=1), rounded), ev[order], within


def project(x0, transform, rounded=True):
    out = []
    for x in x0:
        y = fl32(transform @ np.concatenate([x, [1.0]]), rounded)
        nrm = np.sqrt((y * y).sum())
        out.append(fl32(y * np.sqrt(len(y)) / nrm, rounded) if nrm > 0 else y)
    return np.stack(out)


def plda_train(keys, z, utt2spk, iters):
    """-> (mean, transform, psi, W, B): PldaStats + PldaEstimator + GetOutput with a loop over the classes"""
    spk = _by_speaker(keys, utt2spk)
    L = z.shape[1]
    K, N = len(spk), sum(len(r) for r in spk.values())
    off, gsum, cls = np.zeros((L, L)), np.zeros(L), []
    for rows in spk.values():
        m = np.zeros(L)
        for i in rows:
            m += z[i]
            off += np.outer(z[i], z[i])
        m /= len(rows)
        off -= len(rows) * np.outer(m, m)
        gsum += m
        cls.append((len(rows), m))
    W, B = np.eye(L), np.eye(L)
    for _ in range(iters):
        Ws, Wc, Bs, Bc = off.copy(), N - K, np.zeros((L, L)), 0
        Wi, Bi = np.linalg.inv(W), np.linalg.inv(B)
        for n, mk in cls:
            m = mk - gsum / K
            mixed = np.linalg.inv(Bi + n * Wi)
            w = mixed @ (n * (Wi @ m))
            Bs += mixed + np.outer(w, w)
            Bc += 1
            Ws += n * mixed + n * np.outer(m - w, m - w)
            Wc += 1
        W, B = Ws / Wc, Bs / Bc
    C = np.linalg.cholesky(W)
    T1 = np.linalg.inv(C)
    psi, U = np.linalg.eigh(T1 @ B @ T1.T)
    order = np.argsort(-psi)
    return gsum / K, U[:, order].T @ T1, np.maximum(psi[order], 0.0), W, B


def smooth(plda, smoothing):
    mean, T, psi = plda
    c = 1.0 + smoothing * psi
    return mean, np.diag(c ** -0.5) @ T, psi / c


def transform_ivector(z, plda, n=1, normalize_length=True, simple=False):
    mean, T, psi = plda
    u = T @ z - T @ mean
    if normalize_length:
        ss = (u * u).sum() if simple else (u * u / (psi + 1.0 / n)).sum()
        if ss > 0:
            u = u * np.sqrt(len(u) / ss)
    return u


def llr(e, t, psi, n=1):
    c = n * psi / (n * psi + 1.0)
    v = 1.0 + psi / (n * psi + 1.0)
    return -0.5 * (np.log(v).sum() + ((t - c * e) ** 2 / v).sum()) + 0.5 * (np.log(psi + 1.0).sum() + (t * t / (psi + 1.0)).sum())


def score(ekeys, ex, tkeys, tx, trials, mean, transform, plda, num_utts=None, normalize_length=True, simple=False, smoothing=0.0,
          rounded=True):
    """-> float64 scores (fl32 values when rounded) in trial order"""
    plda = smooth(plda, smoothing)
    ze = project(center(ex, mean, rounded), transform, rounded)
    zt = project(center(tx, mean, rounded), transform, rounded)
    ie, it = {k: i for i, k in enumerate(ekeys)}, {k: i for i, k in enumerate(tkeys)}
    out = []
    for a, b, _ in trials:
        n = 1 if num_utts is None else num_utts.get(a, 1)
        e = transform_ivector(ze[ie[a]], plda, n, normalize_length, simple)
        t = transform_ivector(zt[it[b]], plda, 1, normalize_length, simple)
        out.append(llr(e, t, plda[2], n))
    return fl32(np.array(out), rounded)


def stage(S, rounded=True, **kw):
    """the whole stage on the synthetic set S -> dict(lda, lda_ev, within, plda (mean, transform, psi), W, B, scores)"""
    x0 = center(S["train"], S["mean"], rounded)
    T, ev, within = lda(S["train_keys"], x0, S["utt2spk"], LDA_DIM, rounded=rounded)
    z = project(x0, T, rounded)
    mean, tr, psi, W, B = plda_train(S["train_keys"], z, S["utt2spk"], EM_ITERS)
    sc = score(S["test_keys"], S["test"], S["test_keys"], S["test"], S["trials"], S["mean"], T, (mean, tr, psi), rounded=rounded, **kw)
    return {"lda": T, "lda_ev": ev, "within": within, "plda": (mean, tr, psi), "W": W, "B": B, "scores": sc}


def invariants(plda):
    """what a Plda object defines without the sign of its rows: (psi, T^T T, T^T diag(psi) T)"""
    _, T, psi = plda
    return psi, T.T @ T, T.T @ np.diag(psi) @ T


def error_rates(scores, labels):
    """(EER, minDCF at 0.01, minDCF at 0.001) by the plain threshold sweep"""
    order = sorted(range(len(scores)), key=lambda i: scores[i])
    lab = [labels[i] for i in order]
    n_tar, n_non = sum(lab), len(lab) - sum(lab)
    fnr, fpr, miss, rej = [], [], 0, 0
    for l in lab:
        miss += l
        rej += 1 - l
        fnr.append(miss / float(n_tar))
        fpr.append(1 - rej / float(n_non))
    i = min(range(len(lab)), key=lambda j: abs(fnr[j] - fpr[j]))
    out = [max(fnr[i], fpr[i])]
    for p in (0.01, 0.001):
        out.append(min(fnr[j] * p + fpr[j] * (1 - p) for j in range(len(lab))) / min(p, 1 - p))
    return tuple(out)


# ---- kernel references and bounds -----------------------------------------------------------------------------------------------------
def scatter(X, mu=None, w=None):
    """(C, bound): |C - ref| <= (N + 8) 2^-53 sum_i |w_i| |c_ia| |c_ib| - a sum of N products in any order, plus the roundings of the
    centring and of the weight"""
    c = np.asarray(X, dtype=np.float64) - (0.0 if mu is None else mu)
    ww = np.ones(len(c)) if w is None else np.asarray(w, dtype=np.float64)
    return (c * ww[:, None]).T @ c, (len(c) + 8) * U53 * (np.abs(c) * np.abs(ww)[:, None]).T @ np.abs(c)


def segment_sum(X, rows, seg_off):
    """(sums, counts, bound): n_k 2^-53 sum |x|"""
    X = np.asarray(X, dtype=np.float64)
    K = len(seg_off) - 1
    out, bound, cnt = np.zeros((K, X.shape[1])), np.zeros((K, X.shape[1])), np.zeros(K, dtype=np.int32)
    for k in range(K):
        r = rows[seg_off[k]:seg_off[k + 1]] if rows is not None else np.arange(seg_off[k], seg_off[k + 1])
        out[k] = X[r].sum(axis=0)
        cnt[k] = len(r)
        bound[k] = len(r) * U53 * np.abs(X[r]).sum(axis=0)
    return out, cnt, bound


def affine(X, A, b=None, q=None, scale=False):
    """(Y, bound) in fp64.  Unscaled: the dot-product bound e = (Di + 8) 2^-53 (|x| |A|^T + |b|).  Scaled by s = sqrt(Do / ss),
    ss = sum_j y_j^2 q_j: d(ss) <= sum_j 2 |y_j| e_j q_j + (Do + 4) 2^-53 ss, d(s) / s <= d(ss) / (2 ss) + 3 * 2^-53 (the division,
    the root, the product), so |out - s y| <= s e + |s y| (d(ss) / (2 ss) + 3 * 2^-53)."""
    X = np.asarray(X, dtype=np.float64)
    Di = X.shape[1]
    A = np.eye(Di) if A is None else A
    Do = len(A)
    bb = np.zeros(Do) if b is None else b
    y = X @ A.T + bb
    e = (Di + 8) * U53 * (np.abs(X) @ np.abs(A).T + np.abs(bb))
    if not scale:
        return y, e
    qq = np.ones(Do) if q is None else q
    ss = (y * y * qq).sum(axis=1)
    dss = (2 * np.abs(y) * e * qq).sum(axis=1) + (Do + 4) * U53 * ss
    ok = ss > 0
    s = np.where(ok, np.sqrt(Do / np.where(ok, ss, 1.0)), 1.0)
    rel = np.where(ok, dss / (2 * np.where(ok, ss, 1.0)), 0.0) + 3 * U53
    return y * s[:, None], s[:, None] * e + np.abs(y * s[:, None]) * rel[:, None]


def llr_table(en, te, ia, ib, psi, count=None):
    """(scores fp64, bound): (D + 8) 2^-53 sum |terms| for the fp64 sum, then one float32 rounding of the result"""
    out, bound = np.zeros(len(ia)), np.zeros(len(ia))
    for t in range(len(ia)):
        n = 1 if count is None else int(count[ia[t]])
        e, x = en[ia[t]], te[ib[t]]
        c = n * psi / (n * psi + 1.0)
        v = 1.0 + psi / (n * psi + 1.0)
        terms = np.concatenate([0.5 * x * x / (psi + 1.0), -0.5 * (x - c * e) ** 2 / v, [0.5 * np.log(psi + 1.0).sum(), -0.5 * np.log(v).sum()]])
        out[t] = llr(e, x, psi, n)
        b64 = (len(psi) + 8) * U53 * np.abs(terms).sum()
        bound[t] = b64 + 2.0 ** -24 * (abs(out[t]) + b64) + 2.0 ** -149
    return out, bound
