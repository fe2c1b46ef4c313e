"""PLDA back end: the last stage of the reference's recipes - an LDA trained on the training embeddings
(Kaldi's ivector-subtract-global-mean | ivector-compute-lda), a PLDA trained on the projected, length-normalised embeddings
(transform-vec | ivector-normalize-length | ivector-compute-plda) and the trial scores (ivector-plda-scoring behind the same
pipeline, with ivector-copy-plda's smoothing).  No Kaldi binary is involved: the contract is Kaldi's published algorithm as section
6j states it, pinned by the independent restatement in tests/plda_ref.py.

Two back ends.  `host` is numpy in fp64.  `hip` runs every pass over an [N][D] or [K][D] table and the trial loop on the GPU
(csrc/plda.hip through ops.py); the D x D factorisations (eigendecompositions, Cholesky, inverses) stay in numpy.linalg on both.
Stage roundings (the float32 values Kaldi's BaseFloat pipeline hands from one binary to the next) are the same on both:
x0 = fl32(x - m), y = fl32(A [x0; 1]), z = fl32(y sqrt(L) / |y|); everything after z is fp64."""
import re
import struct
import sys

import numpy as np

from . import kaldi_io, scoring


# ---- files ----------------------------------------------------------------------------------------------------------------------
def write_transform(path, mat):
    """Kaldi binary 'FM ' matrix (\\0B header), float32"""
    kaldi_io.write_mat(path, np.ascontiguousarray(mat, dtype=np.float32))


def read_transform(path):
    """[dim][D+1] float64 of a binary or text Kaldi matrix"""
    return np.asarray(kaldi_io.read_mat(path), dtype=np.float64)


def write_plda(path, mean, transform, psi):
    """Kaldi's binary Plda object: \\0B <Plda> DV(mean) DM(transform) DV(psi) </Plda>"""
    mean, transform, psi = (np.ascontiguousarray(v, dtype="<f8") for v in (mean, transform, psi))
    with open(path, "wb") as f:
        f.write(b"\0B<Plda> ")
        f.write(b"DV \x04" + struct.pack("<i", mean.shape[0]) + mean.tobytes())
        f.write(b"DM \x04" + struct.pack("<i", transform.shape[0]) + b"\x04" + struct.pack("<i", transform.shape[1]) + transform.tobytes())
        f.write(b"DV \x04" + struct.pack("<i", psi.shape[0]) + psi.tobytes())
        f.write(b"</Plda> ")


def read_plda(path):
    """-> (mean [D], transform [D][D], psi [D]) float64 of Kaldi's binary or text Plda object"""
    raw = open(path, "rb").read()
    if raw[:2] == b"\0B":
        pos = 2

        def take(tok):
            nonlocal pos
            if raw[pos:pos + len(tok)] != tok:
                raise kaldi_io.UnknownHeader("%s: expected %r at byte %d, got %r" % (path, tok, pos, raw[pos:pos + len(tok)]))
            pos += len(tok)

        def take_int():
            nonlocal pos
            take(b"\x04")
            pos += 4
            return struct.unpack("<i", raw[pos - 4:pos])[0]

        def take_f64(n):
            nonlocal pos
            pos += 8 * n
            return np.frombuffer(raw[pos - 8 * n:pos], dtype="<f8").copy()

        take(b"<Plda> ")
        take(b"DV ")
        mean = take_f64(take_int())
        take(b"DM ")
        r, c = take_int(), take_int()
        transform = take_f64(r * c).reshape(r, c)
        take(b"DV ")
        psi = take_f64(take_int())
        take(b"</Plda> ")
    else:
        text = raw.decode()
        m = re.match(r"\s*<Plda>(.*)</Plda>\s*$", text, re.S)
        if not m:
            raise kaldi_io.UnknownHeader("%s is not a Plda object" % path)
        groups = re.findall(r"\[(.*?)\]", m.group(1), re.S)
        if len(groups) != 3:
            raise kaldi_io.UnknownHeader("%s: a Plda object holds a vector, a matrix and a vector" % path)
        mean = np.array(groups[0].split(), dtype=np.float64)
        transform = np.array([l.split() for l in groups[1].splitlines() if l.strip()], dtype=np.float64)
        psi = np.array(groups[2].split(), dtype=np.float64)
    if transform.shape != (len(mean), len(mean)) or len(psi) != len(mean):
        raise ValueError("%s: inconsistent Plda dimensions %s %s %s" % (path, mean.shape, transform.shape, psi.shape))
    return mean, transform, psi


def read_utt2spk(path):
    out = {}
    for line in open(path):
        utt, spk = line.strip().split()
        out[utt] = spk
    return out


def read_num_utts(path):
    """'<utt> <count>' lines of ivector-plda-scoring's --num-utts"""
    out = {}
    for line in open(path):
        utt, n = line.strip().split()
        out[utt] = int(n)
        if out[utt] < 1:
            raise ValueError("%s: the count of %s must be at least 1" % (path, utt))
    return out


# ---- the stages every script shares ---------------------------------------------------------------------------------------------
def _center(vecs, mean):
    """(keys, x0 [N][D] float32): archive values taken as float32, x0 = fl32(x - m); m: the given mean (its values taken as float32
    too, as Kaldi's BaseFloat reader takes them), or the fp64 mean of the archive itself"""
    keys, mat = scoring._archive_rows(vecs)
    x = np.asarray(mat).astype(np.float32).astype(np.float64)
    m = x.mean(axis=0) if mean is None else np.asarray(mean).astype(np.float32).astype(np.float64)
    if x.shape[1] != m.shape[0]:
        raise ValueError("the mean has %d dimensions, the archive %d" % (m.shape[0], x.shape[1]))
    return keys, (x - m).astype(np.float32)


def _classes(keys, x0, utt2spk):
    """The rows that have a speaker, grouped: (x0 without the other rows, rows [N] int32 into it grouped by speaker - speakers in
    order of first appearance, archive order inside - and seg_off [K+1] int32).  Utterances without a speaker are skipped with a
    warning; a speaker without a vector never shows up."""
    index, spk_of, kept = {}, [], []
    for r, utt in enumerate(keys):
        if utt not in utt2spk:
            sys.stderr.write("WARNING: %s has no speaker in utt2spk: skipped\n" % utt)
            continue
        kept.append(r)
        spk_of.append(index.setdefault(utt2spk[utt], len(index)))
    if not kept:
        raise ValueError("no utterance of the archive has a speaker")
    if len(kept) != len(keys):
        x0 = np.ascontiguousarray(x0[kept])
    spk_of = np.asarray(spk_of, dtype=np.int64)
    rows = np.argsort(spk_of, kind="stable").astype(np.int32)
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(spk_of, minlength=len(index)))]).astype(np.int32)
    return x0, rows, seg_off


def _up(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _sym_eig_desc(M):
    s, U = np.linalg.eigh((M + M.T) / 2)
    order = np.argsort(-s, kind="stable")
    return s[order], U[:, order]


# ---- LDA ------------------------------------------------------------------------------------------------------------------------
def lda_from_stats(tot, bet, mu, N, dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    """The D x D part of ivector-compute-lda: (transform [dim][D+1] float64 = [A | -A mu], eigenvalues [D] descending)"""
    total = tot / N
    within = (tot - bet) / N
    between = total - within
    f = total_covariance_factor
    s, U = np.linalg.eigh(f * total + (1 - f) * within)
    s = np.maximum(s, s.max() * covariance_floor)
    T = (U / np.sqrt(s)).T
    ev, V = _sym_eig_desc(T @ between @ T.T)
    if not 1 <= dim <= len(mu):
        raise ValueError("--dim=%d must lie in [1, %d]" % (dim, len(mu)))
    A = V[:, :dim].T @ T
    return np.concatenate([A, -(A @ mu)[:, None]], axis=1), ev


def compute_lda(vecs, utt2spk, dim=200, total_covariance_factor=0.0, covariance_floor=1e-6, mean=None, backend="host", out_path=None):
    """-> (transform [dim][D+1] float32, eigenvalues of the between-class covariance in the whitened space, descending)"""
    keys, x0 = _center(vecs, mean)
    x0, rows, seg_off = _classes(keys, x0, utt2spk)
    N, K = len(rows), len(seg_off) - 1
    if backend == "hip":
        from . import ops
        xd, rd, sd = _up(x0), _up(rows), _up(seg_off)
        sums = ops.segment_sum_f64(xd, sd, rd)[0]
        mu = ops.segment_sum_f64(sums, _up(np.array([0, K], dtype=np.int32)))[0][0].cpu().numpy() / N
        mud = _up(mu)
        tot = ops.scatter_f64(xd, mud).cpu().numpy()
        means = ops.segment_sum_f64(xd, sd, rd, mean=True)[0]
        bet = ops.scatter_f64(means, mud, _up(np.diff(seg_off), np.float64)).cpu().numpy()
    else:
        assert backend == "host", backend
        c = x0[rows].astype(np.float64)
        mu = c.mean(axis=0)
        c -= mu
        tot = c.T @ c
        n = np.diff(seg_off).astype(np.float64)
        a = np.add.reduceat(c, seg_off[:-1], axis=0) / n[:, None]
        bet = (a * n[:, None]).T @ a
    T, ev = lda_from_stats(tot, bet, mu, N, dim, total_covariance_factor, covariance_floor)
    T = T.astype(np.float32)
    if out_path:
        write_transform(out_path, T)
    return T, ev


# ---- projection and length normalisation ---------------------------------------------------------------------------------------
def project(x0, transform, backend="host"):
    """x0 [N][D] float32, transform [L][D+1] (or [L][D]) -> z [N][L] float32: y = fl32(A [x0; 1]), z = fl32(y sqrt(L) / |y|) with
    the norm of the float32 y taken in fp64; a zero row is kept.  On `hip` the result is a device tensor."""
    transform = np.asarray(transform, dtype=np.float64)
    D = x0.shape[1]
    if transform.shape[1] not in (D, D + 1):
        raise ValueError("the transform has %d columns, the vectors %d dimensions" % (transform.shape[1], D))
    A = np.ascontiguousarray(transform[:, :D])
    b = np.ascontiguousarray(transform[:, D]) if transform.shape[1] == D + 1 else np.zeros(len(A))
    if backend == "hip":
        import torch
        from . import ops
        xd = x0 if torch.is_tensor(x0) else _up(x0)
        y = ops.affine_lennorm(xd, _up(A), _up(b), None, False, torch.float32)
        return ops.affine_lennorm(y, None, None, None, True, torch.float32)
    assert backend == "host", backend
    y = (x0.astype(np.float64) @ A.T + b).astype(np.float32).astype(np.float64)
    ss = (y * y).sum(axis=1)
    f = np.where(ss > 0, np.sqrt(len(A) / np.where(ss > 0, ss, 1.0)), 1.0)
    return (y * f[:, None]).astype(np.float32)


# ---- PLDA estimation ------------------------------------------------------------------------------------------------------------
def _simdiag(W, B):
    """T with T W T^T = I and T B T^T = diag(psi): W = C C^T, T1 = C^-1, T1 B T1^T = U diag(psi) U^T (psi floored at 0, descending)"""
    C = np.linalg.cholesky((W + W.T) / 2)
    T1 = np.linalg.inv(C)
    psi, U = _sym_eig_desc(T1 @ B @ T1.T)
    return np.maximum(psi, 0.0), U.T @ T1


def _em_host(off, means, n, gsum, iters):
    """the class loop as section 6j writes it, vectorised over the classes that share a count"""
    K, D = means.shape
    N = float(n.sum())
    W, B = np.eye(D), np.eye(D)
    mc = means - gsum / K
    groups = [(float(c), mc[n == c]) for c in np.unique(n)]
    for _ in range(iters):
        Wstats, Wcount, Bstats, Bcount = off.copy(), N - K, np.zeros((D, D)), 0.0
        Winv, Binv = np.linalg.inv(W), np.linalg.inv(B)
        for c, M in groups:
            mixed = np.linalg.inv(Binv + c * Winv)
            w = (c * M @ Winv.T) @ mixed.T                # rows: mixed (n W^-1 m)
            r = M - w
            Bstats += len(M) * mixed + w.T @ w
            Bcount += len(M)
            Wstats += c * len(M) * mixed + c * (r.T @ r)
            Wcount += len(M)
        W, B = Wstats / Wcount, Bstats / Bcount
    return W, B


def _em_hip(off, means_d, n_d, n, gsum, iters):
    """The same iteration in the basis where W = I and B = diag(psi): there (B^-1 + n W^-1)^-1 = diag(psi / (n psi + 1)), so the
    class loop is one projection of the class means (spk_affine_lennorm), their two posterior row tables
    (spk_plda_posterior_rows) and one scatter of each (spk_scatter_f64); the diagonal terms depend on the counts alone."""
    from . import ops
    import torch
    K, D = means_d.shape
    N = float(n.sum())
    W, B = np.eye(D), np.eye(D)
    mean = gsum / K
    counts, mult = np.unique(n, return_counts=True)
    nw = _up(n, np.float64)
    for _ in range(iters):
        psi, T = _simdiag(W, B)
        mt = ops.affine_lennorm(means_d, _up(T), _up(-(T @ mean)), None, False, torch.float64)
        w, r = ops.plda_posterior_rows(mt, n_d, _up(psi))
        Sw = ops.scatter_f64(w).cpu().numpy()
        Sr = ops.scatter_f64(r, None, nw).cpu().numpy()
        mixed = psi[None, :] / (counts[:, None] * psi[None, :] + 1.0)                     # [distinct counts][D]
        Bt = np.diag((mult[:, None] * mixed).sum(axis=0)) + Sw
        Wt = T @ off @ T.T + np.diag(((mult * counts)[:, None] * mixed).sum(axis=0)) + Sr
        Ti = np.linalg.inv(T)
        W, B = Ti @ (Wt / N) @ Ti.T, Ti @ (Bt / K) @ Ti.T                                  # Wcount = (N - K) + K
    return W, B


def compute_plda(vecs, utt2spk, transform, num_em_iters=10, mean=None, backend="host", out_path=None):
    """-> (mean [L], transform [L][L], psi [L]) float64, Kaldi's Plda object"""
    keys, x0 = _center(vecs, mean)
    x0, rows, seg_off = _classes(keys, x0, utt2spk)
    K = len(seg_off) - 1
    n = np.diff(seg_off).astype(np.int64)
    z = project(x0, transform, backend)
    if backend == "hip":
        from . import ops
        rd, sd = _up(rows), _up(seg_off)
        means_d, n_d = ops.segment_sum_f64(z, sd, rd, mean=True)
        off = ops.scatter_f64(z).cpu().numpy() - ops.scatter_f64(means_d, None, _up(n, np.float64)).cpu().numpy()
        gsum = ops.segment_sum_f64(means_d, _up(np.array([0, K], dtype=np.int32)))[0][0].cpu().numpy()
        W, B = _em_hip(off, means_d, n_d, n, gsum, num_em_iters)
    else:
        z = z[rows].astype(np.float64)
        means = np.add.reduceat(z, seg_off[:-1], axis=0) / n[:, None]
        off = z.T @ z - (means * n[:, None]).T @ means
        gsum = means.sum(axis=0)
        W, B = _em_host(off, means, n, gsum, num_em_iters)
    psi, T = _simdiag(W, B)
    out = (gsum / K, T, psi)
    if out_path:
        write_plda(out_path, *out)
    return out


# ---- scoring --------------------------------------------------------------------------------------------------------------------
def smooth(plda, smoothing):
    """ivector-copy-plda --smoothing: psi /= c, transform rows *= c^-1/2 with c = 1 + smoothing psi (0.0 changes nothing) -> float64"""
    mean, T, psi = (np.asarray(v, dtype=np.float64) for v in plda)
    if smoothing == 0.0:
        return mean, T, psi
    c = 1.0 + smoothing * psi
    return mean, T / np.sqrt(c)[:, None], psi / c


def _log_table(psi, counts):
    """per distinct count n: (sum_j log v_j, sum_j log(psi_j + 1)), v_j = 1 + psi_j / (n psi_j + 1)"""
    return np.array([[np.log(1.0 + psi / (c * psi + 1.0)).sum(), np.log(psi + 1.0).sum()] for c in counts], dtype=np.float64)


def _side_host(z, plda, counts, normalize_length, simple):
    mean, T, psi = plda
    u = z.astype(np.float64) @ T.T - T @ mean
    if normalize_length:
        q = np.ones_like(u) if simple else 1.0 / (psi[None, :] + 1.0 / counts[:, None])
        ss = (u * u * q).sum(axis=1)
        u = u * np.where(ss > 0, np.sqrt(u.shape[1] / np.where(ss > 0, ss, 1.0)), 1.0)[:, None]
    return u


def _side_hip(z, plda, counts, normalize_length, simple):
    """u = s (T z - T mean) on the device, fp64; one fused launch per distinct count (its q), on rows grouped by count"""
    import torch
    from . import ops
    mean, T, psi = plda
    Td, bd = _up(T), _up(-(T @ mean))
    if not normalize_length or simple or (counts == counts[0]).all():
        q = None if (simple or not normalize_length) else _up(1.0 / (psi + 1.0 / counts[0]))
        return ops.affine_lennorm(z, Td, bd, q, normalize_length, torch.float64)
    u = torch.empty(z.shape[0], len(psi), device=z.device, dtype=torch.float64)
    for c in np.unique(counts):                                  # (the caller sorted the rows by count)
        lo, hi = np.searchsorted(counts, c, "left"), np.searchsorted(counts, c, "right")
        ops.affine_lennorm(z[lo:hi], Td, bd, _up(1.0 / (psi + 1.0 / c)), True, torch.float64, out=u[lo:hi])
    return u


def plda_score(enroll, test, trials_path, mean, transform, plda, num_utts=None, normalize_length=True,
               simple_length_normalization=False, smoothing=0.0, score_path=None, backend="host", return_device=False):
    """scores (float32) and labels for '<enroll> <test> target|nontarget' lines.  num_utts: utt -> enrolment count (default 1);
    the test side always counts 1.  An unknown key raises KeyError."""
    plda = smooth(plda, smoothing)
    psi = plda[2]
    pairs, labels = [], []
    for line in open(trials_path):
        a, b, t = line.strip().split()
        pairs.append((a, b))
        labels.append(1 if t == "target" else 0)
    ke, xe = _center(enroll, mean)
    ce = np.array([1 if num_utts is None else int(num_utts.get(k, 1)) for k in ke], dtype=np.int64)
    if (ce != ce[0]).any():                                     # rows grouped by count: one row range per distinct count
        order = np.argsort(ce, kind="stable")
        ke, xe, ce = [ke[i] for i in order], np.ascontiguousarray(xe[order]), ce[order]
    ie = {k: i for i, k in enumerate(ke)}
    if test is enroll:
        kt, xt, it = ke, xe, ie
    else:
        kt, xt = _center(test, mean)
        it = {k: i for i, k in enumerate(kt)}
    ia = np.fromiter((ie[a] for a, _ in pairs), dtype=np.int32, count=len(pairs))          # KeyError = unknown utterance
    ib = np.fromiter((it[b] for _, b in pairs), dtype=np.int32, count=len(pairs))
    ct = np.ones(len(kt), dtype=np.int64)
    distinct = np.unique(ce)
    logs = _log_table(psi, distinct)
    if backend == "hip":
        from . import ops
        ze = project(xe, transform, "hip")
        zt = ze if test is enroll else project(xt, transform, "hip")
        ue = _side_hip(ze, plda, ce, normalize_length, simple_length_normalization)
        ut = ue if (test is enroll and (ce == 1).all()) else _side_hip(zt, plda, ct, normalize_length, simple_length_normalization)
        scores_d = ops.plda_llr(ue, ut, _up(ia), _up(ib), _up(psi), None if (ce == 1).all() else _up(ce, np.int32),
                                _up(distinct, np.int32), _up(logs))
        scores = scores_d.cpu().numpy()
    else:
        assert backend == "host", backend
        ze = project(xe, transform, "host")
        zt = ze if test is enroll else project(xt, transform, "host")
        ue = _side_host(ze, plda, ce, normalize_length, simple_length_normalization)
        ut = _side_host(zt, plda, ct, normalize_length, simple_length_normalization)
        slot = np.searchsorted(distinct, ce)
        scores = np.empty(len(pairs), dtype=np.float32)
        for lo in range(0, len(pairs), 1 << 16):
            ja, jb = ia[lo:lo + (1 << 16)], ib[lo:lo + (1 << 16)]
            nn = ce[ja].astype(np.float64)[:, None]
            den = nn * psi[None, :] + 1.0
            c, v = nn * psi[None, :] / den, 1.0 + psi[None, :] / den
            t = ut[jb]
            d = t - c * ue[ja]
            quad = (0.5 * (t * t / (psi[None, :] + 1.0) - d * d / v)).sum(axis=1)
            scores[lo:lo + len(ja)] = (quad + 0.5 * (logs[slot[ja], 1] - logs[slot[ja], 0])).astype(np.float32)
    if score_path:
        with open(score_path, "w") as f:
            for (a, b), s in zip(pairs, scores):
                f.write("{} {} {}\n".format(a, b, s))
    if return_device and backend == "hip":
        return scores_d, np.array(labels)
    return scores, np.array(labels)
