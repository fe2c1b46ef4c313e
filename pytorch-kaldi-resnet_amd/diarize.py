"""Diarization back end: the consumer of the sliding-window embeddings decode.py --window writes.  Per
recording an all-pairs score matrix (Kaldi's ivector-plda-scoring-dense, or cosine), average-linkage agglomerative clustering with a
threshold or a known speaker count (agglomerative-cluster) and RTTM output (make_rttm.py).  No Kaldi binary is involved: the contract
is the rule as section 6n states it, pinned by the independent restatement in tests/diar_ref.py.  With target_energy the PLDA scores
take ivector-plda-scoring-dense's per-recording PCA (--target-energy; section 6p, pinned by tests/pca_ref.py): the PLDA model is
projected onto the leading principal directions of each recording's own rows and diagonalised again before that recording is scored.

Two back ends.  `host` is numpy in fp64.  `hip` keeps the embeddings, the scores and the clustering on the GPU (csrc/diar.hip through
ops.py, the projections through csrc/plda.hip).  A batch of recordings is one [Ntot][D] table with rec_off [R + 1]: recording r owns
the rows rec_off[r] .. rec_off[r + 1] - 1, and its n x n score matrix lies at mat_off[r] = sum of the earlier n^2 in one flat array.
pca_rows, cluster, vbx and vbx_init take that layout as a RecBatch (recbatch.py) in place of rec_off; diarize() builds one per call."""
import numpy as np

from . import plda as _plda
from .recbatch import RecBatch


def plda_dense_terms(psi):
    """(g [D], k [D], K) of the dense form of Plda::LogLikelihoodRatio(u_i, 1, u_j):
    llr = q_i + q_j + K + sum_d g_d u_id u_jd with q_i = -0.5 sum_d k_d u_id^2"""
    psi = np.asarray(psi, dtype=np.float64)
    g = psi / (2.0 * psi + 1.0)
    k = psi * psi / ((psi + 1.0) * (2.0 * psi + 1.0))
    K = 0.5 * float((np.log(psi + 1.0) - np.log(1.0 + psi / (psi + 1.0))).sum())
    return g, k, K


def _center(emb, mean):
    """x0 = fl32(x - m) as plda._center takes it: values and mean as float32; mean None: the fp64 mean of the rows themselves"""
    x = np.asarray(emb).astype(np.float32).astype(np.float64)
    m = x.mean(axis=0) if mean is None else np.asarray(mean).astype(np.float32).astype(np.float64)
    if x.ndim != 2 or x.shape[1] != m.shape[0]:
        raise ValueError("the mean has %d dimensions, the embeddings %s" % (m.shape[0], x.shape[1:]))
    return (x - m).astype(np.float32)


def dense_inputs(emb, kind, mean=None, transform=None, plda=None, smoothing=0.0, normalize_length=True,
                 simple_length_normalization=False, backend="host"):
    """-> (U [Ntot][D'] fp64, q [Ntot] fp64, g [D'] fp64, K): the operands of the dense score, numpy on `host`, device tensors on
    `hip`.  cosine: rows of norm sqrt(D) (ivector-normalize-length's scaling, spk_affine_lennorm) with g = 1 / D - the cosine of the
    centred embeddings; q = 0 and K = 0.  plda: the rows Plda::TransformIvector gives for one utterance per side."""
    if kind == "plda":
        z, model = _plda_z(emb, mean, transform, plda, smoothing, backend)
        return _plda_rows(z, model, normalize_length, simple_length_normalization, backend)
    if kind != "cosine":
        raise ValueError("kind must be cosine or plda, got %r" % (kind,))
    x0 = _center(emb, mean)
    N = x0.shape[0]
    z = x0 if transform is None else _plda.project(x0, transform, backend)
    D = z.shape[1]
    if backend == "hip":
        import torch
        from . import ops
        U = ops.affine_lennorm(z if torch.is_tensor(z) else _plda._up(z), None, None, None, True, torch.float64)
        return U, torch.zeros(N, device=U.device, dtype=torch.float64), _plda._up(np.full(D, 1.0 / D)), 0.0
    assert backend == "host", backend
    y = z.astype(np.float64)
    ss = (y * y).sum(axis=1)
    U = y * np.where(ss > 0, np.sqrt(D / np.where(ss > 0, ss, 1.0)), 1.0)[:, None]
    return U, np.zeros(N), np.full(D, 1.0 / D), 0.0


def _plda_z(emb, mean, transform, plda, smoothing, backend):
    """where every PLDA path starts, once per call -> (z [Ntot][L] float32: the centred, projected rows of plda.project, the smoothed model)"""
    if plda is None or transform is None:
        raise ValueError("plda scoring needs the transform and the Plda object")
    return _plda.project(_center(emb, mean), transform, backend), _plda.smooth(plda, smoothing)


def _plda_rows(z, model, normalize_length, simple_length_normalization, backend):
    """z and the smoothed model of _plda_z -> (U, q, g, K) of dense_inputs(kind="plda")"""
    g, k, K = plda_dense_terms(model[2])
    counts = np.ones(z.shape[0], dtype=np.int64)
    if backend == "hip":
        from . import ops
        U = _plda._side_hip(z, model, counts, normalize_length, simple_length_normalization)
        return U, ops.score_dense_q(U, _plda._up(k), -0.5), _plda._up(g), K
    assert backend == "host", backend
    U = _plda._side_host(z, model, counts, normalize_length, simple_length_normalization)
    return U, -0.5 * (k[None, :] * U * U).sum(axis=1), g, K


# ---- per-recording PCA ---------------------------------------------------------------------------------------
def _check_energy(target_energy, kind):
    if kind != "plda":
        raise ValueError("target_energy needs kind='plda' (the PCA adapts the PLDA model), got %r" % (kind,))
    if not 0.0 < float(target_energy) < 1.0:
        raise ValueError("target_energy must lie strictly between 0 and 1, got %r" % (target_energy,))
    return float(target_energy)


def pca_dim_rule(s, n, E):
    """s [L] descending and >= 0, n rows -> the retained dimension of section 6p, or None where the recording skips the PCA"""
    L = len(s)
    cum = np.cumsum(s)                                              # (in index order)
    tot = cum[-1]
    if n == 1 or not tot > 0:
        return None
    over = np.nonzero(cum / tot > E)[0]
    k = int(over[0]) + 1 if over.size else L
    return min(k + 1, L, n - 1)


def _pca_rec_host(z, W, B, model, E):
    """steps 1-5 of section 6p for the rows z [n][L] of one recording -> (dim, s [L], psi_r [L], A_r [L][L], b_r [L], info), zero
    padded at and beyond dim"""
    mean, T, psi = model
    n, L = z.shape
    x = z.astype(np.float64)
    mu = x.sum(axis=0) / n
    C = np.triu((x.T @ x) / n - np.outer(mu, mu))
    C = C + np.triu(C, 1).T
    s, P = _plda._sym_eig_desc(C)
    s = np.maximum(s, 0.0)
    dim = pca_dim_rule(s, n, E)
    if dim is None:
        return L, s, psi.copy(), T.copy(), -(T @ mean), 0
    Pr = P[:, :dim].T
    Wr, Br = Pr @ W @ Pr.T, Pr @ B @ Pr.T
    A, b, pr = np.zeros((L, L)), np.zeros(L), np.zeros(L)
    try:
        G = np.linalg.cholesky(np.tril(Wr) + np.tril(Wr, -1).T)
    except np.linalg.LinAlgError:
        return dim, s, pr, A, b, 2
    T1 = np.linalg.inv(G)
    p, U = _plda._sym_eig_desc(T1 @ Br @ T1.T)
    pr[:dim] = np.maximum(p, 0.0)
    A[:dim] = U.T @ T1 @ Pr
    b[:dim] = -(A[:dim] @ mean)
    return dim, s, pr, A, b, 0


def pca_inputs(emb, rec_off, target_energy, mean=None, transform=None, plda=None, smoothing=0.0, normalize_length=True,
               simple_length_normalization=False, backend="host", ws_budget_bytes=1 << 31):
    """The operands of the dense score with the per-recording PCA of section 6p: the embeddings centred and projected as
    dense_inputs(kind="plda") does, then pca_rows on the smoothed model"""
    E = _check_energy(target_energy, "plda")
    z, model = _plda_z(emb, mean, transform, plda, smoothing, backend)
    return pca_rows(z, rec_off, model, E, normalize_length, simple_length_normalization, backend, ws_budget_bytes)


def _pca_rows_host(z, rec, model, W, B, E, normalize_length, simple_length_normalization):
    ro, R, L = rec.rec_off, rec.R, z.shape[1]
    z = np.asarray(z, dtype=np.float32)
    dim, info = np.empty(R, dtype=np.int32), np.empty(R, dtype=np.int32)
    s, psi_r, A_r, b_r = np.zeros((R, L)), np.zeros((R, L)), np.zeros((R, L, L)), np.zeros((R, L))
    for r in range(R):
        dim[r], s[r], psi_r[r], A_r[r], b_r[r], info[r] = _pca_rec_host(z[ro[r]:ro[r + 1]], W, B, model, E)
    # (a recording in error has zeros in A_r, b_r and psi_r: what follows is defined for it, and pca_rows raises)
    g, k, K = (np.array(t) for t in zip(*(plda_dense_terms(p) for p in psi_r)))
    qn = None if (simple_length_normalization or not normalize_length) else 1.0 / (psi_r + 1.0)
    U = np.zeros((z.shape[0], L))
    for r in range(R):
        u = z[ro[r]:ro[r + 1]].astype(np.float64) @ A_r[r].T + b_r[r]
        if normalize_length:
            ss = (u * u * (1.0 if qn is None else qn[r][None, :])).sum(axis=1)
            u = u * np.where(ss > 0, np.sqrt(dim[r] / np.where(ss > 0, ss, 1.0)), 1.0)[:, None]
        U[ro[r]:ro[r + 1]] = u
    q = np.concatenate([-0.5 * (k[r][None, :] * U[ro[r]:ro[r + 1]] ** 2).sum(axis=1) for r in range(R)])
    return {"U": U, "q": q, "g": g, "K": K, "dim": dim, "s": s, "psi_r": psi_r, "info": info}


def _pca_rows_hip(z, rec, model, W, B, E, normalize_length, simple_length_normalization, ws_budget_bytes):
    import torch
    from . import ops
    up = _plda._up
    z = (z if torch.is_tensor(z) else up(z, np.float32)).contiguous()
    m, T, psi = model                                               # (more than syevj_max_dim() dimensions: pca_plda_batch raises)
    dim, s, psi_r, A_r, b_r, info = ops.pca_plda_batch(z, rec, up(W), up(B), up(T), up(psi), up(m), E, ws_budget_bytes)
    g, k, qn, K = ops.pca_score_terms(psi_r)
    plain = simple_length_normalization or not normalize_length
    U = ops.affine_lennorm_rec(z, rec, A_r, b_r, None if plain else qn, dim, normalize_length)
    q = ops.score_dense_q(U, k, -0.5, rec)
    # (the one synchronisation of the chain, after its kernels are queued; a recording in error has zeros in A_r, b_r and psi_r)
    return {"U": U, "q": q, "g": g, "K": K, "dim": dim.cpu().numpy(), "s": s.cpu().numpy(), "psi_r": psi_r.cpu().numpy(),
            "info": info.cpu().numpy()}


def pca_rows(z, rec_off, model, target_energy, normalize_length=True, simple_length_normalization=False, backend="host",
             ws_budget_bytes=1 << 31):
    """z [Ntot][L] float32 (numpy, or on `hip` a device tensor): the rows plda.project gives; rec_off [R + 1] or a RecBatch; model =
    (mean, T, psi), already smoothed -> dict(U [Ntot][L] fp64 (zeros beyond dim[r]), q [Ntot], g [R][L], K [R], dim [R], s [R][L],
    psi_r [R][L], info [R]); U, q, g and K are device tensors on `hip`, the rest numpy.  A recording whose factorisation failed
    (info != 0) raises ValueError naming it."""
    E = _check_energy(target_energy, "plda")
    rec = RecBatch.of(rec_off, z.shape[0])
    model = m, T, psi = tuple(np.asarray(v, dtype=np.float64) for v in model)
    if z.shape[1] != len(psi):
        raise ValueError("the rows have %d dimensions, the PLDA model %d" % (z.shape[1], len(psi)))
    Ti = np.linalg.inv(T)
    W, B = Ti @ Ti.T, (Ti * psi[None, :]) @ Ti.T
    if backend == "hip":
        p = _pca_rows_hip(z, rec, model, W, B, E, normalize_length, simple_length_normalization, ws_budget_bytes)
    else:
        assert backend == "host", backend
        p = _pca_rows_host(z, rec, model, W, B, E, normalize_length, simple_length_normalization)
    info = p["info"]
    bad = np.nonzero(info)[0]
    if bad.size:
        raise ValueError("the per-recording PCA failed for recording %d (info = %d: %s)" % (
            bad[0], info[bad[0]], "a Cholesky pivot was not positive" if info[bad[0]] == 2 else "an eigendecomposition did not converge"))
    return p


def _inputs(emb, rec, kind, target_energy=None, vbx_rows=False, mean=None, transform=None, plda=None, smoothing=0.0,
            normalize_length=True, simple_length_normalization=False, backend="host", ws_budget_bytes=1 << 31):
    """The one way from the embeddings to the operands of the dense score -> (U, q, g, K, extra).  plda: the embeddings are centred
    and projected once and the model is smoothed once, whatever follows.  target_energy: the operands are pca_rows' (g [R][D], K [R])
    and extra holds pca_dim; vbx_rows: extra holds X and Phi for VBx: the global rows and psi, with or without the PCA."""
    if target_energy is not None:
        _check_energy(target_energy, kind)
    if kind != "plda":
        return dense_inputs(emb, kind, mean, transform, backend=backend) + ({},)
    z, model = _plda_z(emb, mean, transform, plda, smoothing, backend)
    norm = (normalize_length, simple_length_normalization)
    U, q, g, K = _plda_rows(z, model, *norm, backend) if target_energy is None or vbx_rows else (None,) * 4
    extra = {"X": U, "Phi": model[2]} if vbx_rows else {}
    if target_energy is not None:
        p = pca_rows(z, rec, model, target_energy, *norm, backend, ws_budget_bytes)
        U, q, g, K = p["U"], p["q"], p["g"], p["K"]
        extra["pca_dim"] = [int(d) for d in p["dim"]]
    return U, q, g, K, extra


def score_dense(emb, rec_off, kind="cosine", mean=None, transform=None, plda=None, smoothing=0.0, normalize_length=True,
                simple_length_normalization=False, backend="host", return_device=False, target_energy=None):
    """emb [Ntot][D] (the rows of all recordings, recording after recording), rec_off [R + 1] -> (scores float32 [sum n^2], mat_off
    int64 [R + 1]): recording r's matrix S[i][j] = (float)(q_i + q_j + K + sum_d g_d U_id U_jd) at scores[mat_off[r]:], symmetric
    bit for bit.  `hip` with return_device: the scores stay on the GPU (what cluster(..., backend="hip") takes).  target_energy (a
    number in (0, 1), kind plda): every recording is scored with its own PCA-adapted model (section 6p)."""
    emb = np.asarray(emb)
    rec = RecBatch.of(rec_off, emb.shape[0])
    U, q, g, K, _ = _inputs(emb, rec, kind, target_energy, False, mean, transform, plda, smoothing, normalize_length,
                            simple_length_normalization, backend)
    return _score_rows(U, q, g, K, rec, backend, return_device), rec.mat_off


def _score_rows(U, q, g, K, rec, backend, return_device):
    """the dense scores of the operands dense_inputs made (g [D], K a number) or pca_rows did (g [R][D], K [R]: every recording's
    own terms); rec: rec_off [R + 1] or a RecBatch.  On `hip`: device tensors in, and with return_device a device tensor out."""
    rec = RecBatch.of(rec, U.shape[0])
    if backend == "hip":
        from . import ops
        out = ops.score_dense(U, rec, q, g, K)[0]
        return out if return_device else out.cpu().numpy()
    ro, mat_off = rec.rec_off, rec.mat_off
    g, K = np.broadcast_to(g, (rec.R, U.shape[1])), np.broadcast_to(K, (rec.R,))
    out = np.empty(int(mat_off[-1]), dtype=np.float32)
    for r in range(rec.R):
        u, qq = U[ro[r]:ro[r + 1]], q[ro[r]:ro[r + 1]]
        s = np.triu(((u * g[r][None, :]) @ u.T + qq[:, None]) + qq[None, :] + K[r])
        s = s + np.triu(s, 1).T                                     # the upper triangle, mirrored
        out[mat_off[r]:mat_off[r + 1]] = s.astype(np.float32).ravel()
    return out


# ---- clustering -------------------------------------------------------------------------------------------------------------------
def _ahc_host(S, min_clusters, threshold):
    """One recording by the rule of section 6n, with the cached row minima the kernel keeps (csrc/diar.hip): the minimum of row a over
    the active b > a, refreshed only where a merge can have changed it.  -> (labels, merges, costs)"""
    n = S.shape[0]
    C = np.triu(-S.astype(np.float64), 1)
    C = C + C.T
    m = np.ones(n)
    active = np.ones(n, dtype=bool)
    root = np.arange(n)
    val = np.full(n, np.inf)
    col = np.full(n, -1, dtype=np.int64)

    def scan(a):
        b = np.arange(a + 1, n)
        b = b[active[b]]
        val[a], col[a] = np.inf, -1
        if b.size:
            c = C[a, b] / (m[a] * m[b])
            c = np.where(c == c, c, np.inf)                        # a NaN never wins
            k = int(np.argmin(c))                                  # the first of equal costs
            if c[k] < np.inf:
                val[a], col[a] = c[k], b[k]

    for a in range(n - 1):
        scan(a)
    target = max(min(int(min_clusters), n), 1)
    merges, costs = [], []
    nactive = n
    with np.errstate(all="ignore"):
        while nactive > target:
            cand = np.where(active & (col >= 0), val, np.inf)
            i = int(np.argmin(cand))
            if not cand[i] < np.inf:
                break
            c, j = cand[i], int(col[i])
            if not c <= -threshold:
                break
            merges.append((i, j))
            costs.append(c)
            k = active.copy()
            k[[i, j]] = False
            C[i, k] = C[i, k] + C[j, k]
            C[k, i] = C[i, k]
            m[i] += m[j]
            active[j] = False
            root[root == j] = i
            for a in np.nonzero(active[:j])[0]:
                if a == i or col[a] == i or col[a] == j:
                    scan(a)
                elif a < i:
                    ci = C[a, i] / (m[a] * m[i])
                    if ci < val[a] or (ci == val[a] and i < col[a]) or (col[a] < 0 and ci < np.inf):
                        val[a], col[a] = ci, i
            nactive -= 1
    rank = np.cumsum(active)
    return rank[root].astype(np.int32), merges, costs


def _per_recording(v, R, dtype, default, name):
    if v is None:
        return np.full(R, default, dtype=dtype)
    a = np.asarray(v, dtype=dtype)
    if a.ndim == 0:
        return np.full(R, a, dtype=dtype)
    if a.shape != (R,):
        raise ValueError("%s must be one value or one per recording (%d), got %s" % (name, R, a.shape))
    return a


def cluster(scores, rec_off, threshold=None, num_speakers=None, backend="host", ws_budget_bytes=1 << 31):
    """scores: the flat float32 matrices of score_dense (numpy, or on `hip` a device tensor), rec_off [R + 1].  threshold: stop when
    the next merge's cost c does not satisfy c <= -threshold, i.e. when the average score of the best pair falls below it (one value
    or one per recording; None or -inf: none).  num_speakers: clusters to stop at (one value or one per recording; values above n
    clamp to n; None: 1).  -> (labels int32 [Ntot] from 1, numbered by lowest member window; merges int32 [Ntot][2] and merge_cost
    float64 [Ntot], recording r in the slots from rec_off[r]; n_merges int32 [R]) as numpy arrays.  The merge list of a correct
    implementation is unique: both back ends give the same bits."""
    rec = RecBatch.of(rec_off)
    ro, mat_off, R, Ntot = rec.rec_off, rec.mat_off, rec.R, rec.Ntot
    minc = _per_recording(num_speakers, R, np.int64, 1, "num_speakers")
    if (minc < 1).any():
        raise ValueError("num_speakers must be at least 1")
    thr = _per_recording(threshold, R, np.float64, -np.inf, "threshold")
    if np.isnan(thr).any():
        raise ValueError("a threshold is NaN")
    minc = np.minimum(minc, rec.n)                                  # (fits int32)
    if backend == "hip":
        import torch
        from . import ops
        sd = scores if torch.is_tensor(scores) else torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).cuda()
        return tuple(t.cpu().numpy() for t in ops.ahc_batch(sd, rec, minc.astype(np.int32), thr, ws_budget_bytes))
    assert backend == "host", backend
    s = np.asarray(scores.cpu().numpy() if hasattr(scores, "cpu") else scores, dtype=np.float32)
    if s.size < mat_off[-1]:
        raise ValueError("the scores hold %d values, rec_off asks for %d" % (s.size, mat_off[-1]))
    labels, nm = np.empty(Ntot, dtype=np.int32), np.empty(R, dtype=np.int32)
    merges, cost = np.zeros((Ntot, 2), dtype=np.int32), np.zeros(Ntot, dtype=np.float64)
    for r in range(R):
        lab, mer, cs = _ahc_host(s[mat_off[r]:mat_off[r + 1]].reshape(rec.n[r], rec.n[r]), minc[r], thr[r])
        labels[ro[r]:ro[r + 1]] = lab
        nm[r] = len(mer)
        if mer:
            merges[ro[r]:ro[r] + len(mer)] = mer
            cost[ro[r]:ro[r] + len(mer)] = cs
    return labels, merges, cost, nm


# ---- VBx resegmentation ------------------------------------------------------------------------------------
VBX_DEFAULTS = dict(Fa=0.3, Fb=17.0, loop_prob=0.99, max_iters=40, epsilon=1e-6, init_smoothing=7.0)
VBX_PI_FLOOR = 2.0 ** -900      # a state whose prior is below this is taken to have prior 0 (csrc/diar.hip)


def vbx_inputs(emb, mean=None, transform=None, plda=None, smoothing=0.0, normalize_length=True, simple_length_normalization=False,
               backend="host"):
    """-> (X [Ntot][D'] fp64, Phi [D'] fp64): the rows of dense_inputs(kind="plda") - Plda::TransformIvector for one utterance per
    side, the space where the within-class covariance is I - and the between-class variances psi of the smoothed model.  numpy on
    `host`, device tensors on `hip`."""
    z, model = _plda_z(emb, mean, transform, plda, smoothing, backend)
    U = _plda_rows(z, model, normalize_length, simple_length_normalization, backend)[0]
    return U, (_plda._up(model[2]) if backend == "hip" else model[2])


def vbx_init(init_labels, rec_off, init_smoothing=7.0):
    """first-pass labels [Ntot] -> (gamma [Ntot][Smax], pi [R][Smax], n_states [R]): per recording S = its number of distinct labels
    (state s: the s-th smallest), gamma_ts = softmax_s(init_smoothing [label_t == s]) over its S states, pi_s = 1 / S; the columns
    at or beyond S are 0"""
    lab = np.asarray(init_labels)
    rec = RecBatch.of(rec_off, lab.shape[0])
    ro, R = rec.rec_off, rec.R
    idx = [np.unique(lab[ro[r]:ro[r + 1]], return_inverse=True)[1] for r in range(R)]
    ns = np.array([int(i.max()) + 1 for i in idx], dtype=np.int32)
    Smax = int(ns.max())
    gamma = np.zeros((lab.shape[0], Smax))
    pi = np.zeros((R, Smax))
    for r in range(R):
        S = int(ns[r])
        z = float(init_smoothing) * (idx[r][:, None] == np.arange(S)[None, :])
        e = np.exp(z - z.max(axis=1, keepdims=True))
        gamma[ro[r]:ro[r + 1], :S] = e / e.sum(axis=1, keepdims=True)
        pi[r, :S] = 1.0 / S
    return gamma, pi, ns


def vbx_labels(gamma, rec_off, n_states):
    """the window label: argmax_s gamma_ts over the recording's states, ties to the lowest s, renumbered 1, 2, ... by lowest member
    window (section 6n's rule) -> int32 [Ntot]"""
    ro = np.asarray(rec_off, dtype=np.int64)
    out = np.empty(gamma.shape[0], dtype=np.int32)
    for r in range(ro.size - 1):
        a = np.argmax(gamma[ro[r]:ro[r + 1], :int(n_states[r])], axis=1)
        _, first, inv = np.unique(a, return_index=True, return_inverse=True)
        out[ro[r]:ro[r + 1]] = (np.argsort(np.argsort(first)) + 1)[inv]
    return out


def _vbx_host(X, Phi, gamma, pi, Fa, Fb, loopP, max_iters, epsilon):
    """One recording by the rule of section 6o in numpy fp64, with the forward-backward pass in the scaled form the kernel uses
    (csrc/diar.hip): a_t = e^{lfw_t} / sum_i e^{lfw_ti}, gamma_t = a_t b_t.  -> (gamma, pi, elbo list)"""
    T, D = X.shape
    rho = X * np.sqrt(Phi)[None, :]
    G = -0.5 * ((X * X).sum(axis=1) + D * np.log(2 * np.pi))
    FaFb = Fa / Fb
    pi = np.where(pi >= VBX_PI_FLOOR, pi, 0.0)
    elbo = []
    with np.errstate(all="ignore"):
        for it in range(max_iters):
            N = gamma.sum(axis=0)
            invL = 1.0 / (1.0 + FaFb * N[:, None] * Phi[None, :])
            alpha = FaFb * invL * (gamma.T @ rho)
            logp = Fa * (rho @ alpha.T - 0.5 * ((invL + alpha ** 2) @ Phi)[None, :] + G[:, None])
            live = pi > 0
            M = np.where(live[None, :], logp, -np.inf).max(axis=1)
            p = np.where(live[None, :], np.exp(logp - M[:, None]), 0.0)
            a = np.empty_like(p)
            c = np.empty(T)
            u = p[0] * pi
            c[0] = u.sum()
            a[0] = u / c[0]
            for t in range(1, T):
                u = p[t] * (loopP * a[t - 1] + (1.0 - loopP) * pi)
                c[t] = u.sum()
                a[t] = u / c[t]
            gamma = np.empty_like(p)
            gamma[T - 1] = a[T - 1]
            b = np.ones(p.shape[1])
            acc = np.zeros(p.shape[1])
            for t in range(T - 1, 0, -1):
                x = p[t] * b / c[t]
                y = pi * x
                acc += y
                b = loopP * x + (1.0 - loopP) * y.sum()
                gamma[t - 1] = a[t - 1] * b
            elbo.append(float((M + np.log(c)).sum() + 0.5 * Fb * (np.log(invL) - invL - alpha ** 2 + 1.0).sum()))
            pi = gamma[0] + (1.0 - loopP) * acc
            pi = pi / pi.sum()
            pi = np.where(pi >= VBX_PI_FLOOR, pi, 0.0)
            if it > 0 and elbo[-1] - elbo[-2] < epsilon:
                break
    return gamma, pi, elbo


def vbx(X, Phi, rec_off, init_labels=None, gamma=None, pi=None, n_states=None, Fa=0.3, Fb=17.0, loop_prob=0.99, max_iters=40,
        epsilon=1e-6, init_smoothing=7.0, backend="host", ws_budget_bytes=1 << 31):
    """VBx (section 6o) over the rows X [Ntot][D] (vbx_inputs) of the recordings rec_off [R + 1], Phi [D] >= 0.  The start is either
    init_labels [Ntot] (first-pass labels: vbx_init) or gamma [Ntot][Smax] with optional pi [R][Smax] (default 1 / n_states) and
    n_states [R] (default Smax).  epsilon = -inf always runs max_iters iterations.  On `hip` X and Phi may be device tensors.
    -> dict(labels int32 [Ntot] (vbx_labels), gamma [Ntot][Smax], pi [R][Smax], elbo [R][max_iters] (NaN past n_iters), n_iters
    int32 [R], n_states int32 [R]) as numpy arrays."""
    if not (Fa > 0 and np.isfinite(Fa) and Fb > 0 and np.isfinite(Fb)):
        raise ValueError("Fa and Fb must be positive and finite, got %r and %r" % (Fa, Fb))
    if not 0.0 < loop_prob < 1.0:
        raise ValueError("loop_prob must lie strictly between 0 and 1, got %r" % (loop_prob,))
    if int(max_iters) != max_iters or max_iters < 1:
        raise ValueError("max_iters must be an integer of at least 1, got %r" % (max_iters,))
    if not epsilon < np.inf:
        raise ValueError("epsilon must be a number below +inf, got %r" % (epsilon,))
    Ntot, D = X.shape
    rec = RecBatch.of(rec_off, Ntot)
    ro, R = rec.rec_off, rec.R
    if (init_labels is None) == (gamma is None):
        raise ValueError("give exactly one of init_labels and gamma")
    if init_labels is not None:
        if pi is not None or n_states is not None:
            raise ValueError("pi and n_states go with gamma, not with init_labels")
        if np.shape(init_labels) != (Ntot,):
            raise ValueError("init_labels must hold one label per window (%d), got %s" % (Ntot, np.shape(init_labels)))
        gamma, pi, ns = vbx_init(init_labels, rec, init_smoothing)
    else:
        gamma = np.array(gamma, dtype=np.float64)
        if gamma.ndim != 2 or gamma.shape[0] != Ntot or gamma.shape[1] < 1:
            raise ValueError("gamma must be [Ntot = %d][Smax], got %s" % (Ntot, gamma.shape))
        ns = _per_recording(n_states, R, np.int32, gamma.shape[1], "n_states")
        if (ns < 1).any() or (ns > gamma.shape[1]).any():
            raise ValueError("n_states must lie in [1, Smax = %d]" % gamma.shape[1])
        if pi is None:
            pi = (np.arange(gamma.shape[1])[None, :] < ns[:, None]) / ns[:, None].astype(np.float64)
        pi = np.array(pi, dtype=np.float64)
        if pi.shape != (R, gamma.shape[1]):
            raise ValueError("pi must be [R = %d][Smax = %d], got %s" % (R, gamma.shape[1], pi.shape))
    Smax = gamma.shape[1]
    phi_host = np.asarray(Phi.cpu().numpy() if hasattr(Phi, "cpu") else Phi, dtype=np.float64)
    if phi_host.shape != (D,) or not (phi_host >= 0).all():
        raise ValueError("Phi must hold %d values >= 0" % D)
    elbo = np.full((R, int(max_iters)), np.nan)
    if backend == "hip":
        import torch
        from . import ops
        if Smax > ops.vbx_max_states():
            raise ValueError("the hip back end takes at most %d states per recording, got %d" % (ops.vbx_max_states(), Smax))
        if int(rec.n.max()) > ops.ahc_max_n():
            raise ValueError("vbx: a recording has %d windows, the cap is %d" % (int(rec.n.max()), ops.ahc_max_n()))
        Xd = X if torch.is_tensor(X) else _plda._up(np.asarray(X, dtype=np.float64))
        Pd = Phi if torch.is_tensor(Phi) else _plda._up(phi_host)
        gd, pd = _plda._up(gamma), _plda._up(pi)
        ed, nd = ops.vbx_batch(Xd.contiguous(), Pd, rec, ns, gd, pd, Fa, Fb, loop_prob, int(max_iters), epsilon,
                               ws_budget_bytes=ws_budget_bytes)
        gamma, pi, elbo, nit = gd.cpu().numpy(), pd.cpu().numpy(), ed.cpu().numpy(), nd.cpu().numpy()
    else:
        assert backend == "host", backend
        Xh = np.asarray(X.cpu().numpy() if hasattr(X, "cpu") else X, dtype=np.float64)
        nit = np.empty(R, dtype=np.int32)
        for r in range(R):
            S = int(ns[r])
            g, p, el = _vbx_host(Xh[ro[r]:ro[r + 1]], phi_host, gamma[ro[r]:ro[r + 1], :S], pi[r, :S], float(Fa), float(Fb),
                                 float(loop_prob), int(max_iters), float(epsilon))
            gamma[ro[r]:ro[r + 1]] = 0.0
            gamma[ro[r]:ro[r + 1], :S] = g
            pi[r] = 0.0
            pi[r, :S] = p
            elbo[r, :len(el)] = el
            nit[r] = len(el)
    return {"labels": vbx_labels(gamma, ro, ns), "gamma": gamma, "pi": pi, "elbo": elbo, "n_iters": nit, "n_states": ns}


_vbx = vbx      # (diarize() has a parameter of that name)


# ---- RTTM -------------------------------------------------------------------------------------------------------------------------
def read_segments(path):
    """'<key> <recording> <start s> <end s>' lines (decode.py --window's segments.<name>) -> [(key, recording, start, end)]"""
    out = []
    for ln, line in enumerate(open(path), 1):
        f = line.split()
        if not f:
            continue
        if len(f) != 4:
            raise ValueError("%s:%d: expected '<key> <recording> <start> <end>', got %r" % (path, ln, line.strip()))
        out.append((f[0], f[1], float(f[2]), float(f[3])))
    return out


def make_rttm(segments, labels, channel=0):
    """segments: (key, recording, start, end) per window; labels: key -> label, or one label per window in the same order.  Per
    recording (in order of first appearance) the windows sorted by (start, end); every adjacent pair with different labels that
    overlaps is cut at the midpoint of the overlap; consecutive windows of one label that touch or overlap are merged; empty pieces
    are dropped.  Only adjacent pairs are cut: with a period below half the window deeper overlaps stay.  -> the RTTM lines."""
    if not isinstance(labels, dict):
        labels = list(labels)
        if len(labels) != len(segments):
            raise ValueError("%d labels for %d windows" % (len(labels), len(segments)))
        labels = {s[0]: l for s, l in zip(segments, labels)}
    recs = {}
    for key, reco, start, end in segments:
        recs.setdefault(reco, []).append([float(start), float(end), int(labels[key])])
    lines = []
    for reco, w in recs.items():
        w.sort(key=lambda p: (p[0], p[1]))
        for cur, nxt in zip(w[:-1], w[1:]):
            if cur[2] != nxt[2] and nxt[0] < cur[1]:
                mid = 0.5 * (nxt[0] + cur[1])
                cur[1] = nxt[0] = mid
        pieces = []
        for p in w:
            if pieces and pieces[-1][2] == p[2] and p[0] <= pieces[-1][1]:
                pieces[-1][1] = max(pieces[-1][1], p[1])
            else:
                pieces.append(list(p))
        for start, end, lab in pieces:
            if end > start:
                lines.append("SPEAKER %s %s %.3f %.3f <NA> <NA> %d <NA> <NA>" % (reco, channel, start, end - start, lab))
    return lines


# ---- one call -----------------------------------------------------------------------------------------------------------------------
def group_windows(emb_keys, segments, recordings=None):
    """The batch layout of a segments list against the embedding keys: (recordings in order of first appearance, the windows of
    each in file order as indices into `segments`, rec_off).  Raises ValueError naming what is wrong: a key of one file that the other
    lacks, a key listed twice, a recording (of `recordings`, when given) with no window."""
    seg_keys = [s[0] for s in segments]
    have, want = set(emb_keys), set(seg_keys)
    if len(want) != len(seg_keys):
        seen, dup = set(), []
        for k in seg_keys:
            if k in seen:
                dup.append(k)
            seen.add(k)
        raise ValueError("segments lists a window twice: " + " ".join(dup[:5]))
    if want - have:
        raise ValueError("windows of the segments file without an embedding: " + " ".join(sorted(want - have)[:5]))
    if have - want:
        raise ValueError("embeddings without a line in the segments file: " + " ".join(sorted(have - want)[:5]))
    order, rows = [], {}
    for i, s in enumerate(segments):
        if s[1] not in rows:
            order.append(s[1])
            rows[s[1]] = []
        rows[s[1]].append(i)
    if recordings is not None:
        empty = [r for r in recordings if r not in rows]
        if empty:
            raise ValueError("recordings with no window: " + " ".join(empty[:5]))
    if not order:
        raise ValueError("recordings with no window: the segments file is empty")
    rec_off = np.concatenate([[0], np.cumsum([len(rows[r]) for r in order])]).astype(np.int64)
    return order, [rows[r] for r in order], rec_off


def read_reco2num_spk(path):
    out = {}
    for line in open(path):
        f = line.split()
        if not f:
            continue
        if len(f) != 2 or int(f[1]) < 1:
            raise ValueError("%s: expected '<recording> <speakers >= 1>', got %r" % (path, line.strip()))
        out[f[0]] = int(f[1])
    return out


def diarize(embeddings, segments, kind="cosine", threshold=None, reco2num_spk=None, recordings=None, backend="host", channel=0,
            return_scores=False, vbx=None, target_energy=None, ws_budget_bytes=1 << 31, **score_args):
    """embeddings: key -> vector (scoring.read_embeddings), segments: read_segments' list; exactly one of threshold and
    reco2num_spk (recording -> speakers).  -> dict(recordings, rec_off, mat_off, keys (batch order), labels, scores (numpy with
    return_scores, else None: on `hip` the matrices then never leave the device), rttm (lines), merges, merge_cost, n_merges).
    vbx: None, or a dict with any of Fa, Fb, loop_prob, max_iters, epsilon, init_smoothing (VBX_DEFAULTS): the clustering's labels
    then seed VBx (section 6o; kind must be plda), `labels` and `rttm` hold its result and the dict gains ahc_labels, vbx_elbo,
    vbx_n_iters and vbx_pi; on `hip` the rows stay on the device between scoring and VBx.  target_energy: None, or the energy in
    (0, 1) of the per-recording PCA (section 6p; kind must be plda): the clustering then runs on the adapted scores and the dict gains
    pca_dim (one int per recording); VBx keeps the global rows and the global psi.  ws_budget_bytes: as in pca_rows, cluster, vbx."""
    if (threshold is None) == (reco2num_spk is None):
        raise ValueError("give exactly one of threshold and reco2num_spk")
    if vbx is not None:
        if kind != "plda":
            raise ValueError("vbx needs kind='plda' (its rows and variances are the PLDA's), got %r" % (kind,))
        unknown = sorted(set(vbx) - set(VBX_DEFAULTS))
        if unknown:
            raise ValueError("unknown vbx parameters: " + " ".join(unknown))
    emb_keys = embeddings.keys_list if hasattr(embeddings, "keys_list") else list(embeddings)
    order, rows, rec_off = group_windows(emb_keys, segments, recordings)
    num = None
    if reco2num_spk is not None:
        absent = [r for r in reco2num_spk if r not in set(order)]
        if absent:
            raise ValueError("recordings of reco2num-spk that are absent from the segments file: " + " ".join(absent[:5]))
        missing = [r for r in order if r not in reco2num_spk]
        if missing:
            raise ValueError("recordings without a speaker count in reco2num-spk: " + " ".join(missing[:5]))
        num = np.array([reco2num_spk[r] for r in order], dtype=np.int64)
    flat = [i for rr in rows for i in rr]
    keys = [segments[i][0] for i in flat]
    if hasattr(embeddings, "mat") and hasattr(embeddings, "index"):
        emb = embeddings.mat[[embeddings.index[k] for k in keys]]
    else:
        emb = np.stack([np.asarray(embeddings[k], dtype=np.float64) for k in keys])
    rec = RecBatch(rec_off, emb.shape[0])                           # (the one layout every stage below takes)
    U, q, g, K, extra = _inputs(np.asarray(emb), rec, kind, target_energy, vbx is not None, backend=backend,
                                ws_budget_bytes=ws_budget_bytes, **score_args)
    scores = _score_rows(U, q, g, K, rec, backend, backend == "hip")
    labels, merges, cost, nm = cluster(scores, rec, threshold, num, backend, ws_budget_bytes)
    segs = [segments[i] for i in flat]
    if vbx is not None:
        res = _vbx(extra.pop("X"), extra.pop("Phi"), rec, init_labels=labels, backend=backend, ws_budget_bytes=ws_budget_bytes, **vbx)
        extra.update({"ahc_labels": labels, "vbx_elbo": res["elbo"], "vbx_n_iters": res["n_iters"], "vbx_pi": res["pi"]})
        labels = res["labels"]
    out = {"recordings": order, "rec_off": rec_off, "mat_off": rec.mat_off, "keys": keys, "labels": labels,
           "scores": None if not return_scores else (scores.cpu().numpy() if hasattr(scores, "cpu") else scores), "rttm": make_rttm(segs, labels.tolist(), channel),
           "merges": merges, "merge_cost": cost, "n_merges": nm}
    out.update(extra)
    return out
