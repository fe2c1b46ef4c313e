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
            return_scores=False, vbx=None, target_energy=None, ws_budget_bytes=1 << 31, ref=None, tune=None, uem=None, der_collar=0.25,
            der_ignore_overlap=False, der_tick=0.001, **score_args):
    """embeddings: key -> vector (scoring.read_embeddings), segments: read_segments' list; exactly one of threshold and
    reco2num_spk (recording -> speakers).  -> dict(recordings, rec_off, mat_off, keys (batch order), labels, scores (numpy with
    return_scores, else None: on `hip` the matrices then never leave the device), rttm (lines), merges, merge_cost, n_merges).
    vbx: None, or a dict with any of Fa, Fb, loop_prob, max_iters, epsilon, init_smoothing (VBX_DEFAULTS): the clustering's labels
    then seed VBx (section 6o; kind must be plda), `labels` and `rttm` hold its result and the dict gains ahc_labels, vbx_elbo,
    vbx_n_iters and vbx_pi; on `hip` the rows stay on the device between scoring and VBx.  target_energy: None, or the energy in
    (0, 1) of the per-recording PCA (section 6p; kind must be plda): the clustering then runs on the adapted scores and the dict gains
    pca_dim (one int per recording); VBx keeps the global rows and the global psi.  ws_budget_bytes: as in pca_rows, cluster, vbx.
    ref: None, or the reference (an RTTM path or parse_rttm's dict): the dict gains `der`, der()'s result for the RTTM lines returned
    (section 6r; uem, der_collar, der_ignore_overlap and der_tick are der()'s uem, collar, ignore_overlap and tick).  tune: None, or
    thresholds to sweep in place of `threshold` (needs ref): the recordings are clustered once, tune_threshold scores every cut, and
    every output is that of the best threshold; the dict gains der_table, best_threshold and der_host_jobs."""
    if tune is not None:
        if threshold is not None or reco2num_spk is not None:
            raise ValueError("tune takes the place of threshold and reco2num_spk")
        if ref is None:
            raise ValueError("tune needs the reference (ref)")
    elif (threshold is None) == (reco2num_spk is None):
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
    segs = [segments[i] for i in flat]
    der_args = dict(uem=uem, collar=der_collar, ignore_overlap=der_ignore_overlap, tick=der_tick)
    if tune is None:
        labels, merges, cost, nm = cluster(scores, rec, threshold, num, backend, ws_budget_bytes)
    else:
        ref = _load(ref, read_rttm)
        _, merges, cost, nm = cluster(scores, rec, None, None, backend, ws_budget_bytes)
        tt = tune_threshold((merges, cost, nm), segs, ref, tune, backend=backend, ws_budget_bytes=ws_budget_bytes, **der_args)
        labels, nm = tt["labels"][tt["best_index"]].copy(), tt["prefix"][:, tt["best_index"]].astype(np.int32)
        past = np.arange(rec.Ntot) - np.repeat(rec.rec_off[:-1], rec.n) >= np.repeat(nm, rec.n)
        merges, cost = np.where(past[:, None], 0, merges).astype(np.int32), np.where(past, 0.0, cost)   # (as a run at that threshold leaves them)
        extra.update({"der_table": tt["table"], "best_threshold": tt["best_threshold"], "der_host_jobs": tt["host_jobs"]})
    if vbx is not None:
        res = _vbx(extra.pop("X"), extra.pop("Phi"), rec, init_labels=labels, backend=backend, ws_budget_bytes=ws_budget_bytes, **vbx)
        extra.update({"ahc_labels": labels, "vbx_elbo": res["elbo"], "vbx_n_iters": res["n_iters"], "vbx_pi": res["pi"]})
        labels = res["labels"]
    out = {"recordings": order, "rec_off": rec_off, "mat_off": rec.mat_off, "keys": keys, "labels": labels,
           "scores": None if not return_scores else (scores.cpu().numpy() if hasattr(scores, "cpu") else scores), "rttm": make_rttm(segs, labels.tolist(), channel),
           "merges": merges, "merge_cost": cost, "n_merges": nm}
    out.update(extra)
    if ref is not None:
        out["der"] = der(ref, parse_rttm(out["rttm"], "the result"), backend=backend, ws_budget_bytes=ws_budget_bytes, **der_args)
    return out


# ---- scoring: the diarization error rate -----------------------------------------------------------------------
def to_ticks(t, tick=0.001):
    """tick(t) = floor(t / tick_s + 0.5) as int64 (a number or an array)"""
    return np.floor(np.asarray(t, dtype=np.float64) / float(tick) + 0.5).astype(np.int64)


def _rttm_fields(f, where):
    """the fields of one SPEAKER line -> (recording, speaker, start, dur)"""
    if len(f) < 8:
        raise ValueError("%s: expected 'SPEAKER <recording> <channel> <start> <dur> <NA> <NA> <speaker> ...', got %r" % (where, " ".join(f)))
    try:
        start, dur = float(f[3]), float(f[4])
    except ValueError:
        raise ValueError("%s: start and duration must be numbers, got %r and %r" % (where, f[3], f[4]))
    if not (np.isfinite(start) and np.isfinite(dur)) or dur < 0:
        raise ValueError("%s: start must be finite and the duration finite and not negative, got %r and %r" % (where, f[3], f[4]))
    return f[1], f[7], start, dur


def parse_rttm(lines, name="rttm"):
    """RTTM lines -> {recording: [(speaker, start s, dur s)]} in order of first appearance; lines of another type than SPEAKER and
    empty lines are skipped; a bad line raises ValueError naming it as <name>:<line>"""
    out = {}
    for ln, line in enumerate(lines, 1):
        f = line.split()
        if not f or f[0] != "SPEAKER":
            continue
        reco, spk, start, dur = _rttm_fields(f, "%s:%d" % (name, ln))
        out.setdefault(reco, []).append((spk, start, dur))
    return out


def read_rttm(path):
    with open(path) as fh:
        return parse_rttm(fh, path)


def read_uem(path):
    """'<recording> <channel> <start s> <end s>' lines -> {recording: [(start, end)]}; a bad line raises ValueError naming it"""
    out = {}
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            f = line.split()
            if not f:
                continue
            if len(f) != 4:
                raise ValueError("%s:%d: expected '<recording> <channel> <start> <end>', got %r" % (path, ln, line.strip()))
            try:
                start, end = float(f[2]), float(f[3])
            except ValueError:
                raise ValueError("%s:%d: start and end must be numbers, got %r and %r" % (path, ln, f[2], f[3]))
            if not (np.isfinite(start) and np.isfinite(end)) or end < start:
                raise ValueError("%s:%d: the region must be finite and must not end before it starts, got %r and %r" % (path, ln, f[2], f[3]))
            out.setdefault(f[0], []).append((start, end))
    return out


def _union(s, e):
    """intervals [s, e) (int64 arrays; empty ones dropped) -> (starts, ends) of their union, sorted and disjoint (touching ones joined)"""
    s, e = np.asarray(s, dtype=np.int64), np.asarray(e, dtype=np.int64)
    keep = e > s
    s, e = s[keep], e[keep]
    if s.size == 0:
        return s, e
    o = np.argsort(s, kind="stable")
    s, e = s[o], e[o]
    run = np.maximum.accumulate(e)
    new = np.concatenate([[True], s[1:] > run[:-1]])
    first = np.nonzero(new)[0]
    return s[first], run[np.concatenate([first[1:] - 1, [s.size - 1]])]


def _covers(s, e, a):
    """is point a[k] inside the sorted disjoint intervals [s, e)? -> (bool [len(a)], index of the interval or -1)"""
    if s.size == 0:
        return np.zeros(a.shape, dtype=bool), np.full(a.shape, -1, dtype=np.int64)
    i = np.searchsorted(s, a, side="right") - 1
    ok = (i >= 0) & (a < e[np.maximum(i, 0)])
    return ok, np.where(ok, i, -1)


def der_reference(turns, uem=None, collar=0.25, ignore_overlap=False, tick=0.001):
    """The reference side of one recording, prepared once: turns [(speaker, start s, dur s)], uem [(start s, end s)] or None ->
    dict(speakers (names in order of first appearance), cs, ce int64 [nc]: the scored set S cut into cells - sorted disjoint intervals
    on each of which the set of active reference speakers is constant -, act bool [Sr][nc], nr int64 [nc])"""
    names = []
    for t in turns:
        if t[0] not in names:
            names.append(t[0])
    spk = np.array([names.index(t[0]) for t in turns], dtype=np.int64)
    ts = to_ticks([t[1] for t in turns], tick) if turns else np.zeros(0, np.int64)
    te = ts + (to_ticks([t[2] for t in turns], tick) if turns else np.zeros(0, np.int64))
    keep = te > ts
    spk, ts, te = spk[keep], ts[keep], te[keep]
    c = int(to_ticks(collar, tick))
    if uem is not None:
        Ss, Se = _union(to_ticks([u[0] for u in uem], tick), to_ticks([u[1] for u in uem], tick))
    elif ts.size:
        Ss, Se = np.array([ts.min()]), np.array([te.max()])
    else:
        Ss, Se = np.zeros(0, np.int64), np.zeros(0, np.int64)
    uni = [_union(ts[spk == i], te[spk == i]) for i in range(len(names))]
    b = np.concatenate([ts, te])
    Xs, Xe = _union(b - c, b + c) if c > 0 else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    pts = np.unique(np.concatenate([Ss, Se, Xs, Xe] + [v for u in uni for v in u]))
    a, z = pts[:-1], pts[1:]
    keep = _covers(Ss, Se, a)[0] & ~_covers(Xs, Xe, a)[0] if a.size else np.zeros(0, dtype=bool)
    a, z = a[keep], z[keep]
    act = np.array([_covers(u[0], u[1], a)[0] for u in uni], dtype=bool).reshape(len(names), a.size)
    nr = act.sum(axis=0).astype(np.int64)
    if ignore_overlap:
        keep = nr < 2
        a, z, act, nr = a[keep], z[keep], act[:, keep], nr[keep]
    # (adjacent cells with the same speakers are joined: fewer cells, the same sums)
    if a.size > 1:
        same = (a[1:] == z[:-1]) & (act[:, 1:] == act[:, :-1]).all(axis=0)
        first = np.nonzero(np.concatenate([[True], ~same]))[0]
        last = np.concatenate([first[1:] - 1, [a.size - 1]])
        a, z, act, nr = a[first], z[last], act[:, first], nr[first]
    return {"speakers": names, "cs": a, "ce": z, "act": act, "nr": nr}


def _assign(C):
    """C int64 [a][b] >= 0 -> (opt, [(i, j)]): a one-to-one partial assignment that maximises the sum of C[i][j] (shortest augmenting
    paths with potentials on -C, the smaller side as rows; exact in int64); pairs with C[i][j] = 0 are not reported"""
    if C.shape[0] == 0 or C.shape[1] == 0:
        return 0, []
    tr = C.shape[0] > C.shape[1]
    A = -(C.T if tr else C).astype(np.int64)
    n, m = A.shape
    INF = np.int64(1) << 61
    u, v = np.zeros(n + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    p, way = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv = np.full(m + 1, INF, dtype=np.int64)
        used = np.zeros(m + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = A[i0 - 1] - u[i0] - v[1:]
            upd = ~used[1:] & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            cand = np.where(used[1:], INF, minv[1:])
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    pairs = [((j - 1, int(p[j]) - 1) if tr else (int(p[j]) - 1, j - 1)) for j in range(1, m + 1) if p[j]]
    pairs = sorted(q for q in pairs if C[q] > 0)
    return int(sum(int(C[q]) for q in pairs)), pairs


def _disjoint_pieces(lab, ps, pe):
    """pieces (dense label, start, end) -> the same ticks per label as pieces that are disjoint within a label: sorted by (label,
    start), a piece starts where the earlier pieces of its label end; empty ones are dropped"""
    keep = pe > ps
    lab, ps, pe = lab[keep], ps[keep], pe[keep]
    if lab.size == 0:
        return lab, ps, pe
    o = np.lexsort((ps, lab))
    lab, ps, pe = lab[o], ps[o], pe[o]
    lo = int(min(ps.min(), 0))
    big = int(pe.max()) - lo + 1
    run = np.maximum.accumulate((pe - lo) + lab * big)              # the running end within a label (labels ascend)
    prev = np.concatenate([[-1], run[:-1]])
    cs = np.maximum(ps, np.where(prev >= lab * big, prev - lab * big + lo, ps))
    keep = pe > cs
    return lab[keep], cs[keep], pe[keep]


def _score_host(prep, lab, ps, pe):
    """One job by the rule of section 6r: the reference side of der_reference, hypothesis pieces (label, start, end: int arrays, any
    labels, any order, overlapping freely) -> ((scored, miss, fa, conf, opt), [(reference speaker index, label)])"""
    cs, ce, act, nr = prep["cs"], prep["ce"], prep["act"], prep["nr"]
    uniq, inv = np.unique(np.asarray(lab, dtype=np.int64), return_inverse=True)
    dl, ds, de = _disjoint_pieces(inv.astype(np.int64), np.asarray(ps, dtype=np.int64), np.asarray(pe, dtype=np.int64))
    pts = np.unique(np.concatenate([cs, ce, ds, de]))
    a = pts[:-1]
    ln = np.diff(pts)
    inS, cell = _covers(cs, ce, a) if a.size else (np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int64))
    ln = np.where(inS, ln, 0)
    r = np.where(inS, nr[np.maximum(cell, 0)], 0) if nr.size else np.zeros(a.size, dtype=np.int64)
    h = np.searchsorted(np.sort(ds), a, side="right") - np.searchsorted(np.sort(de), a, side="right")
    scored = int((ln * r).sum())
    miss = int((ln * np.maximum(r - h, 0)).sum())
    fa = int((ln * np.maximum(h - r, 0)).sum())
    both = int((ln * np.minimum(r, h)).sum())
    C = np.zeros((act.shape[0], uniq.size), dtype=np.int64)
    if ds.size and act.shape[0] and a.size:
        k0, k1 = np.searchsorted(pts, ds), np.searchsorted(pts, de)          # the piece covers the elementary intervals k0 .. k1 - 1
        cnt = k1 - k0
        k = np.repeat(k0 - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(int(cnt.sum()))
        j = np.repeat(dl, cnt)
        sel = inS[k]
        k, j = k[sel], j[sel]
        np.add.at(C.T, j, (act[:, cell[k]] * ln[k][None, :]).T)
    opt, pairs = _assign(C)
    return (scored, miss, fa, both - opt, opt), [(i, int(uniq[j])) for i, j in pairs]


def _der_value(miss, fa, conf, scored):
    return float("nan") if scored == 0 else float(np.float64(miss + fa + conf) / np.float64(scored))


def _prep_table(preps, max_ref):
    """the reference sides as spk_der_batch takes them -> (rec_tab [R][4], cells [ncells][3]); a recording with more than max_ref
    speakers gets Sr = -1 (its jobs are the host's)"""
    rec_tab = np.zeros((len(preps), 4), dtype=np.int64)
    cells, off = [], 0
    for r, p in enumerate(preps):
        Sr, nc = p["act"].shape
        if Sr > max_ref:
            rec_tab[r] = (off, 0, -1, 0)
            continue
        mask = np.zeros(nc, dtype=np.uint64)
        for i in range(Sr):
            mask |= p["act"][i].astype(np.uint64) << np.uint64(i)
        cells.append(np.stack([p["cs"], p["ce"], mask.view(np.int64)], axis=1) if nc else np.zeros((0, 3), dtype=np.int64))
        rec_tab[r] = (off, nc, Sr, 0)
        off += nc
    return rec_tab, (np.concatenate(cells) if cells else np.zeros((0, 3), dtype=np.int64))


def score_jobs(preps, jobs, backend="host", ws_budget_bytes=1 << 31):
    """preps: der_reference's dict per recording; jobs: [(recording index, labels, starts, ends)] (int arrays in ticks) -> (ints int64
    [J][5] = scored, miss, fa, conf, opt; mappings: per job [(reference speaker index, label)]; host_jobs: how many jobs the `hip` back
    end left to the host rule because they exceed the device limits).  Both back ends give the same integers."""
    J = len(jobs)
    ints, maps, on_host = np.zeros((J, 5), dtype=np.int64), [None] * J, list(range(J))
    if backend == "hip" and J:
        import torch
        from . import ops
        max_ref, max_hyp, max_turns = ops.der_limits()
        rec_tab, cells = _prep_table(preps, max_ref)
        dev_jobs, tab, labs, off, uniqs = [], [], [], 0, {}
        for x, (r, lab, ps, pe) in enumerate(jobs):
            uniq, inv = np.unique(np.asarray(lab, dtype=np.int64), return_inverse=True)
            if rec_tab[r, 2] < 0 or uniq.size > max_hyp or inv.size > max_turns:
                continue
            dev_jobs.append(x)
            uniqs[x] = uniq
            tab.append((r, off, inv.size, uniq.size))
            labs.append((inv + 1, ps, pe))
            off += inv.size
        on_host = [x for x in range(J) if x not in uniqs]
        if dev_jobs:
            rec_tab[rec_tab[:, 2] < 0, 2] = 0
            cat = [np.concatenate([t[c] for t in labs]) for c in range(3)]
            up = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).cuda()
            out, mp = ops.der_batch(rec_tab, cells, tab, up(cat[0], np.int32), up(cat[1], np.int64), up(cat[2], np.int64), ws_budget_bytes)
            out, mp = out.cpu().numpy(), mp.cpu().numpy()
            for y, x in enumerate(dev_jobs):
                ints[x] = out[y]
                maps[x] = [(i, int(uniqs[x][l - 1])) for i, l in enumerate(mp[y][:preps[jobs[x][0]]["act"].shape[0]]) if l > 0]
    else:
        assert backend == "host" or not J, backend
    for x in on_host:
        r, lab, ps, pe = jobs[x]
        ints[x], maps[x] = _score_host(preps[r], lab, ps, pe)
    return ints, maps, (len(on_host) if backend == "hip" else 0)


def _turn_ticks(turns, tick):
    """[(speaker, start s, dur s)] -> (dense labels from 1 in order of first appearance, names, starts, ends in ticks)"""
    names = []
    for t in turns:
        if t[0] not in names:
            names.append(t[0])
    lab = np.array([names.index(t[0]) + 1 for t in turns], dtype=np.int64)
    s = to_ticks([t[1] for t in turns], tick) if turns else np.zeros(0, np.int64)
    return lab, names, s, s + (to_ticks([t[2] for t in turns], tick) if turns else np.zeros(0, np.int64))


def _summary(order, ints, maps=None):
    per = {}
    for x, reco in enumerate(order):
        scored, miss, fa, conf, opt = (int(v) for v in ints[x])
        per[reco] = {"scored": scored, "miss": miss, "fa": fa, "conf": conf, "opt": opt, "der": _der_value(miss, fa, conf, scored)}
        if maps is not None:
            per[reco]["mapping"] = maps[x]
    tot = {k: sum(p[k] for p in per.values()) for k in ("scored", "miss", "fa", "conf", "opt")}
    tot["der"] = _der_value(tot["miss"], tot["fa"], tot["conf"], tot["scored"])
    return per, tot


def _load(v, reader):
    return reader(v) if isinstance(v, (str, bytes)) or hasattr(v, "__fspath__") else v


def der(ref, hyp, uem=None, collar=0.25, ignore_overlap=False, tick=0.001, backend="host", ws_budget_bytes=1 << 31):
    """The diarization error rate of section 6r.  ref, hyp: an RTTM path or {recording: [(speaker, start s, dur s)]}; uem: a UEM path,
    {recording: [(start s, end s)]} or None.  -> dict(recordings; per_recording: recording -> dict(scored, miss, fa, conf, opt: ints in
    ticks, der, mapping: {reference speaker: hypothesis speaker}); total: the integers summed and their der; host_jobs).  A recording
    the hypothesis lacks is all miss; one the reference lacks raises ValueError unless the UEM covers it (it is then all false alarm)."""
    ref, hyp, uem = _load(ref, read_rttm), _load(hyp, read_rttm), (None if uem is None else _load(uem, read_uem))
    if not tick > 0:
        raise ValueError("tick must be positive, got %r" % (tick,))
    if not collar >= 0:
        raise ValueError("collar must not be negative, got %r" % (collar,))
    extra = [r for r in hyp if r not in ref and not (uem is not None and r in uem)]
    if extra:
        raise ValueError("recordings of the hypothesis that the reference lacks: " + " ".join(extra[:5]))
    order = list(ref) + [r for r in hyp if r not in ref]
    preps = [der_reference(ref.get(r, []), None if uem is None else uem.get(r), collar, ignore_overlap, tick) for r in order]
    jobs, names = [], []
    for x, r in enumerate(order):
        lab, nm, s, e = _turn_ticks(hyp.get(r, []), tick)
        jobs.append((x, lab, s, e))
        names.append(nm)
    ints, maps, host_jobs = score_jobs(preps, jobs, backend, ws_budget_bytes)
    maps = [{preps[x]["speakers"][i]: names[x][l - 1] for i, l in m} for x, m in enumerate(maps)]
    per, tot = _summary(order, ints, maps)
    return {"recordings": order, "per_recording": per, "total": tot, "host_jobs": host_jobs}


# ---- cutting one merge list at many thresholds ------------------------------------------------------------------------------------------
def _prefix_len(cost, nm, th):
    """per threshold of th [K]: the merges of the longest prefix of cost[:nm] whose costs all satisfy c <= -t -> int64 [K]"""
    if nm <= 0:
        return np.zeros(th.size, dtype=np.int64)
    bad = ~(cost[:nm, None] <= -th[None, :])
    return np.where(bad.any(axis=0), bad.argmax(axis=0), nm).astype(np.int64)


def _thresholds(thresholds):
    th = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
    if th.ndim != 1 or th.size < 1 or np.isnan(th).any():
        raise ValueError("thresholds must be one or more numbers, none of them NaN")
    return th


def cut_merges(merges, merge_cost, n_merges, rec_off, thresholds, backend="host"):
    """merges [Ntot][2], merge_cost [Ntot], n_merges [R] as cluster returns them (numpy, or on `hip` device tensors) -> labels int32
    [K][Ntot]: row k equals the labels of cluster(scores, rec_off, threshold=thresholds[k]) bit for bit - the merge sequence does not
    depend on the threshold, so a cut applies a prefix of it."""
    rec = RecBatch.of(rec_off)
    th = _thresholds(thresholds)
    if backend == "hip":
        import torch
        from . import ops
        up = lambda v, dt: v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).cuda()
        return ops.ahc_cut_batch(up(merges, np.int32), up(merge_cost, np.float64), up(n_merges, np.int32), rec, th).cpu().numpy()
    assert backend == "host", backend
    host = lambda v: np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v)
    merges, cost, nm = host(merges).astype(np.int64), host(merge_cost).astype(np.float64), host(n_merges)
    ro = rec.rec_off
    out = np.empty((th.size, rec.Ntot), dtype=np.int32)
    for r in range(rec.R):
        n = int(rec.n[r])
        for k, L in enumerate(_prefix_len(cost[ro[r]:ro[r + 1]], min(max(int(nm[r]), 0), n - 1), th)):
            parent = np.arange(n)
            parent[merges[ro[r]:ro[r] + L, 1]] = merges[ro[r]:ro[r] + L, 0]
            while True:
                nxt = parent[parent]
                if (nxt == parent).all():
                    break
                parent = nxt
            out[k, ro[r]:ro[r + 1]] = np.cumsum(parent == np.arange(n))[parent]
    return out


def cut_pieces(wstart, wend, labels):
    """The hypothesis of a cut for one recording: windows in ticks sorted by (start, end) and their labels -> (starts, ends) with
    make_rttm's adjacent-pair cut at (a + b) // 2"""
    s, e = np.array(wstart, dtype=np.int64), np.array(wend, dtype=np.int64)
    lab = np.asarray(labels)
    if s.size > 1:
        cut = (lab[1:] != lab[:-1]) & (wstart[1:] < wend[:-1])
        mid = (np.asarray(wstart[1:], dtype=np.int64) + np.asarray(wend[:-1], dtype=np.int64)) >> 1
        s[1:] = np.where(cut, mid, s[1:])
        e[:-1] = np.where(cut, mid, e[:-1])
    return s, e


def _segment_batch(segments):
    """segments in batch order -> (recordings, rec_off); the windows of a recording must follow one another"""
    order, counts = [], []
    for s in segments:
        if order and s[1] == order[-1]:
            counts[-1] += 1
        else:
            if s[1] in order:
                raise ValueError("the windows of recording %s do not follow one another" % s[1])
            order.append(s[1])
            counts.append(1)
    if not order:
        raise ValueError("no windows")
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def tune_threshold(scores_or_merges, segments, ref, thresholds, uem=None, collar=0.25, ignore_overlap=False, tick=0.001,
                   backend="host", ws_budget_bytes=1 << 31):
    """Sweeps the stopping threshold: one clustering, K cuts, R x K scorings.  scores_or_merges: the flat scores of score_dense (the
    recordings are then clustered once, to one cluster) or cluster's (merges, merge_cost, n_merges); segments: (key, recording, start s,
    end s) per window in batch order; ref: an RTTM path or dict; thresholds: K numbers.  -> dict(table: [(threshold, miss, fa, conf,
    scored, DER)] over all recordings; best_threshold, best_index: the smallest miss + fa + conf, ties to the first; per_recording
    int64 [R][K][5]; labels int32 [K][Ntot] (the cuts); prefix int32 [R][K] (merges applied); host_jobs: jobs the `hip` back end left
    to the host rule).  Thresholds that apply the same prefix to a recording share one scoring.  On `hip` the labels and the pieces
    stay on the device between the cut and the scoring."""
    th = _thresholds(thresholds)
    order, rec_off = _segment_batch(segments)
    rec = RecBatch(rec_off, len(segments))
    ref, uem = _load(ref, read_rttm), (None if uem is None else _load(uem, read_uem))
    absent = [r for r in order if r not in ref and not (uem is not None and r in uem)]
    if absent:
        raise ValueError("recordings that the reference lacks: " + " ".join(absent[:5]))
    if isinstance(scores_or_merges, (tuple, list)) and len(scores_or_merges) == 3:
        merges, cost, nm = scores_or_merges
    else:
        merges, cost, nm = cluster(scores_or_merges, rec, None, None, backend, ws_budget_bytes)[1:]
    host = lambda v: np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v)
    cost_h, nm_h = host(cost).astype(np.float64), host(nm)
    R, K, ro = rec.R, th.size, rec.rec_off
    prefix = np.array([_prefix_len(cost_h[ro[r]:ro[r + 1]], min(max(int(nm_h[r]), 0), int(rec.n[r]) - 1), th) for r in range(R)],
                      dtype=np.int32)
    preps = [der_reference(ref.get(r, []), None if uem is None else uem.get(r), collar, ignore_overlap, tick) for r in order]
    ws = to_ticks([s[2] for s in segments], tick)
    we = to_ticks([s[3] for s in segments], tick)
    perm = np.concatenate([ro[r] + np.lexsort((we[ro[r]:ro[r + 1]], ws[ro[r]:ro[r + 1]])) for r in range(R)])
    ws, we = ws[perm], we[perm]
    ints = np.zeros((R, K, 5), dtype=np.int64)
    host_jobs = 0
    if backend == "hip":
        import torch
        from . import ops
        up = lambda v, dt: v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, dtype=dt)).cuda()
        lab_d = ops.ahc_cut_batch(up(merges, np.int32), up(cost, np.float64), up(nm, np.int32), rec, th)
        srt_d = lab_d if (perm == np.arange(perm.size)).all() else lab_d.index_select(1, up(perm, np.int64)).contiguous()
        ps_d, pe_d = ops.der_pieces(srt_d, up(ws, np.int64), up(we, np.int64), rec)
        max_ref, max_hyp, max_turns = ops.der_limits()
        rec_tab, cells = _prep_table(preps, max_ref)
        Sh = rec.n[:, None] - prefix
        dev = (rec_tab[:, 2] >= 0)[:, None] & (Sh <= max_hyp) & (rec.n <= max_turns)[:, None]
        first = np.array([(lambda u: u[1][u[2]])(np.unique(prefix[r], return_index=True, return_inverse=True)) for r in range(R)])
        own = first == np.arange(K)[None, :]                         # (thresholds with the same prefix share one job)
        rk = np.argwhere(dev & own)
        labels = None
        if rk.size:
            rec_tab[rec_tab[:, 2] < 0, 2] = 0
            tab = np.stack([rk[:, 0], rk[:, 1] * rec.Ntot + ro[rk[:, 0]], rec.n[rk[:, 0]], Sh[rk[:, 0], rk[:, 1]]], axis=1)
            out = ops.der_batch(rec_tab, cells, tab, srt_d.view(-1), ps_d.view(-1), pe_d.view(-1), ws_budget_bytes)[0]
            ints[rk[:, 0], rk[:, 1]] = out.cpu().numpy()
        rest = np.argwhere(~dev & own)
        host_jobs = len(rest)
        labels = lab_d.cpu().numpy()
        for r, k in rest:
            lab = labels[k, perm[ro[r]:ro[r + 1]]]
            s, e = cut_pieces(ws[ro[r]:ro[r + 1]], we[ro[r]:ro[r + 1]], lab)
            ints[r, k] = _score_host(preps[r], lab, s, e)[0]
        ints = ints[np.arange(R)[:, None], first]
    else:
        assert backend == "host", backend
        labels = cut_merges(merges, cost, nm, rec, th, "host")
        for r in range(R):
            seen = {}
            for k in range(K):
                if prefix[r, k] not in seen:                        # (thresholds with the same prefix have the same hypothesis)
                    lab = labels[k, perm[ro[r]:ro[r + 1]]]
                    s, e = cut_pieces(ws[ro[r]:ro[r + 1]], we[ro[r]:ro[r + 1]], lab)
                    seen[prefix[r, k]] = _score_host(preps[r], lab, s, e)[0]
                ints[r, k] = seen[prefix[r, k]]
    tot = ints.sum(axis=0)
    table = [(float(th[k]), int(tot[k, 1]), int(tot[k, 2]), int(tot[k, 3]), int(tot[k, 0]),
              _der_value(int(tot[k, 1]), int(tot[k, 2]), int(tot[k, 3]), int(tot[k, 0]))) for k in range(K)]
    err = tot[:, 1] + tot[:, 2] + tot[:, 3]
    best = int(np.argmin(err))                                      # (the first of equal sums)
    return {"table": table, "best_threshold": float(th[best]), "best_index": best, "per_recording": ints, "labels": labels,
            "prefix": prefix, "recordings": order, "host_jobs": host_jobs}
