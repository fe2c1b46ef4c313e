"""fp64 restatements, engineered inputs and per-element error bounds for the kernels around the trunk
(csrc/head.hip, pool.hip, gemm.hip, sgd.hip, score.hip) - test infrastructure only.

tests/test_small_kernels_cpu.py pins these restatements against the reference-generated goldens and shows that float32 torch
on the CPU stays inside every bound on every input below; tests/test_small_kernels_gpu.py runs the kernels on the same inputs
against the same bounds.

Two rules hold throughout:
  * float32 decisions, fp64 values: wherever the reference (which runs in float32) decides something - (cos - th) > 0,
    0 <= 1 - c^2 <= 1, norm >= eps, logit > target, the top-k selection - the decision is taken in float32 arithmetic on the
    float32 inputs; the value of the chosen branch is then computed in fp64.
  * per-element bounds, derived from the summation structure of the kernel source: with u = 2^-24,
    bound = (roundings + 1) * u * sum|terms|.  The kernels that call expf / logf or divide by a small sine use the tolerance
    tests/test_kernels_gpu.py already states for them, applied per row / per element with the conditioning term explicit.
"""
import math

import numpy as np
import torch

from oracle import spk_oracle as O
from oracle import weights as W

U = 2.0 ** -24
F32 = np.float32


def rnd(seed, *shape, scale=1.0, shift=0.0):
    """seeded float32 tensor, uniform in shift + (-scale, scale)"""
    n = int(np.prod(shape))
    return torch.from_numpy(((W.hash_uniform(seed, 1, n) * 2 - 1) * scale + shift).astype(np.float32).reshape(shape))


def uni(seed, *shape):
    """seeded float32 tensor, uniform in [0, 1)"""
    n = int(np.prod(shape))
    return torch.from_numpy(W.hash_uniform(seed, 2, n).astype(np.float32).reshape(shape))


def ints(seed, n, hi):
    return torch.from_numpy(np.minimum((W.hash_uniform(seed, 3, n) * hi).astype(np.int64), hi - 1))


RATIOS = {}     # kernel -> largest error / bound seen in this process (the GPU run prints it)


def check(name, got, ref, bound, skip=None):
    """|got - ref| <= bound on every element where ref is finite; where ref is not finite got has the same value (NaN where
    NaN, the same signed infinity).  `skip`: boolean mask of elements the caller has named and checks itself.
    -> largest error / bound."""
    ref = torch.as_tensor(ref).double()
    bound = torch.broadcast_to(torch.as_tensor(bound).double(), ref.shape).reshape(-1)
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    ref = ref.reshape(-1)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    keep = torch.ones_like(ref, dtype=torch.bool) if skip is None else ~torch.as_tensor(skip).reshape(-1)
    fin = torch.isfinite(ref)
    nf = keep & ~fin
    assert torch.equal(torch.isnan(got[nf]), torch.isnan(ref[nf])), "%s: NaN pattern differs" % name
    inf = nf & torch.isinf(ref)
    assert torch.equal(got[inf], ref[inf]), "%s: infinities differ" % name
    ok = keep & fin
    assert bool(torch.isfinite(got[ok]).all()), "%s: non-finite value where the reference is finite" % name
    err = (got[ok] - ref[ok]).abs()
    b = bound[ok]
    assert bool((b >= 0).all()), name
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), worst)
    if not worst <= 1.0:
        i = int(torch.argmax(ratio))
        raise AssertionError("%s: error / bound = %.3g (error %.3g, bound %.3g, ref %.6g) at kept element %d of %d" % (
            name, worst, float(err[i]), float(b[i]), float(ref[ok][i]), i, int(ok.sum())))
    return worst


# ---- l2norm (F.normalize, scripts/model.py:485) ---------------------------------------------------------------------------
L2_SHAPES = [(1, 1), (5, 63), (6, 65), (7, 256), (37, 512), (5994, 256)]
L2_EPS = 1e-12


def l2_chain(D):
    """roundings of one row reduction in l2norm_* / center_normalize: a per-lane fma chain of ceil(D/64) steps, then six
    shuffle-tree additions"""
    return -(-D // 64) + 6


def l2norm_inputs(R, D):
    """x, dy, dx_prev.  From R >= 5 on: row 1 all zero (y = 0, dx = dy / eps), row 2 of norm ~1e-13 (below eps: clamped), row 3
    of norm ~1e-10 (above eps)."""
    x, dy, prev = rnd(1000 + R, R, D), rnd(1100 + R, R, D), rnd(1200 + R, R, D)
    if R >= 5:
        x[1] = 0.0
        for row, norm in ((2, 1e-13), (3, 1e-10)):
            v = x[row].double()
            x[row] = (v * (norm / float(v.norm()))).float()
    return x, dy, prev


def l2norm_ref(x, dy, eps=L2_EPS):
    """y = x / max(||x||, eps) and the gradient dx of <y, dy> with respect to x, in fp64, as torch differentiates it: a clamped
    row has the constant denominator eps (clamp_min passes no gradient, norm's subgradient at 0 is 0), so dx = dy / eps.

    The decision norm >= eps is the float32 one; a norm within 1e-3 (relative) of eps would make it depend on the float32
    summation order, and is refused here.

    Bounds (ns = l2_chain(D) roundings of a row reduction):
      y   the squared norm carries ns roundings on all-positive terms (relative ns u); sqrt halves that and adds one, the
          reciprocal one, the product one:                         |y - ref| <= (ns/2 + 3 + 1) u |y|
      dx  = inv (dy - y dot), dot = sum y dy.  dot: ns roundings on sum|y dy| plus the relative error ey = (ns/2 + 4) u of
          every y; the factor y again ey; product, subtraction, product by inv three more; inv itself (ns/2 + 2) u:
                                                                  |dx - ref| <= (2.5 ns + 15) u inv (|dy| + |y| sum|y dy|)
      the all-zero and the clamped rows are the special case dot = 0, inv = 1 / eps of the same formula."""
    xd, gd = x.double(), dy.double()
    D = x.shape[1]
    ns = l2_chain(D)
    n = xd.pow(2).sum(1).sqrt()
    e32 = float(F32(eps))
    assert bool(((n - e32).abs() > 1e-3 * e32).all()), "a row norm too close to eps for a float32 decision"
    clamped = n.float() < F32(eps)
    den = torch.where(clamped, torch.full_like(n, e32), n)[:, None]
    y = xd / den
    ybound = (ns / 2 + 4) * U * y.abs()
    ydy = (y * gd).sum(1, keepdim=True)
    dx = torch.where(clamped[:, None], gd / den, (gd - y * ydy) / den)
    dxbound = (2.5 * ns + 15) * U * (gd.abs() + y.abs() * (y * gd).abs().sum(1, keepdim=True)) / den
    return y, ybound, dx, dxbound, clamped


# ---- AAM margin (AAMLayer.forward from `cosine` on, scripts/model.py:487-499) ----------------------------------------------
AAM_SHAPES = [(1, 1), (3, 255), (4, 256), (5, 257), (6, 5994)]
AAM_MS = [(0.2, 30.0), (0.3, 15.0)]


def aam_consts(m):
    """cos_m, sin_m, th, mm as float32 roundings of the Python doubles (what the library passes to its kernels and what
    torch's scalar * float32-tensor arithmetic uses)"""
    return (F32(math.cos(m)), F32(math.sin(m)), F32(math.cos(math.pi - m)), F32(math.sin(math.pi - m) * m))


def aam_label_values(m):
    """the label-column cosines of the issue: th and both float32 neighbours, ordinary values, and the three values around
    +1 and around -1"""
    th = aam_consts(m)[2]
    one = F32(1.0)
    return [th, np.nextafter(th, F32(1)), np.nextafter(th, F32(-2)), F32(0.0), F32(0.5), F32(-0.5), F32(0.999),
            np.nextafter(one, F32(0)), one, np.nextafter(one, F32(2)),
            np.nextafter(-one, F32(0)), -one, np.nextafter(-one, F32(-2))]


def aam_inputs(B, S, m):
    """-> list of (cosv [B][S], label [B], dlogits [B][S]): as many rounds as it takes to put every value of aam_label_values on
    a label column.  Labels include 0 and S - 1; the other columns are uniform in (-1, 1), with one +1.0 and one -1.0 on
    non-label columns when the row has room."""
    vals = aam_label_values(m)
    out = []
    for r0 in range(0, len(vals), B):
        cosv = rnd(2000 + S + r0, B, S, scale=0.999)
        lab = ints(2100 + S + r0, B, S)
        lab[0] = 0
        if B > 1:
            lab[1] = S - 1
        if S >= 3:
            for b in range(B):
                free = [j for j in (1, S // 2, S - 2, 0, S - 1) if j != int(lab[b])]
                cosv[b, free[0]] = 1.0 if b % 2 == 0 else -1.0
        for b in range(B):
            cosv[b, lab[b]] = float(vals[(r0 + b) % len(vals)])
        dl = rnd(2200 + S + r0, B, S, scale=1.0 / B)
        dl[dl == 0] = 1e-3           # no 0 * inf: the sign of an infinite gradient is the sign of dlogits
        out.append((cosv, lab, dl))
    return out


def aam_ref(cosv, label, dlogits, m, s):
    """logits = s (j == label ? phi(c) : c) and dcos = dlogits dlogits/dc in fp64 with float32 decisions.

    Decisions, on float32 arithmetic: take_phi = (c - th) > 0;  neg = 1 - c c < 0 (the clamp to [0, 1]; 1 - c c > 1 cannot
    happen).  The sign of 1 - c c is the same in float32 and fp64 (it is exactly 0 at |c| = 1, and float32 neighbours of 1 are
    2^-24 away).  Values: sine = sqrt(clamp(1 - c^2)), phi = c cos_m - sine sin_m, else c - mm.

    Gradient (torch autograd of the same expression): on the label column with take_phi, dphi/dc = cos_m + sin_m c / sine when
    0 <= 1 - c^2 <= 1 - +inf at c = 1 exactly - and cos_m when the clamp cut 1 - c^2 < 0; everywhere else 1.

    Bounds:
      logits  rtol 2e-5 / atol 5e-5 (test_aam_head_golden), per element; on a label column that took phi with sine > 0, plus the
              first-order term of the cancellation in 1 - c^2: d sine = d(1 - c^2) / (2 sine) with |d(1 - c^2)| <= 2 u c^2, times
              s sin_m, i.e. s sin_m c^2 / sine u.
      dcos    g = s dlogits: one rounding, 2 u |g| off the phi branch (3 u |g cos_m| under the clamp).  On the phi branch the
              product g dphi with dphi = cos_m + sin_m c / sine: six roundings (c c, 1 - ., sqrt, 2 sine, reciprocal, two
              products, one sum) on |dphi|, plus the cancellation: relative error of sine = u c^2 / (2 sine^2), times the
              sin_m |c| / sine term:       |g| (8 u (cos_m + sin_m |c| / sine) + sin_m |c|^3 u / (2 sine^3))."""
    cos_m, sin_m, th, mm = aam_consts(m)
    c32 = cosv.numpy().astype(F32)
    take_phi = (c32 - th) > F32(0)
    u32 = F32(1.0) - c32 * c32
    neg = u32 < F32(0)
    assert not (u32 > F32(1)).any()
    c = c32.astype(np.float64)
    cm, sm, s64 = float(cos_m), float(sin_m), float(F32(s))
    u64 = np.where(neg, 0.0, 1.0 - c * c)
    assert (u64 >= 0).all() and ((u64 == 0) == (neg | (u32 == 0))).all()
    sine = np.sqrt(u64)
    onehot = np.zeros(c.shape, dtype=bool)
    onehot[np.arange(c.shape[0]), label.numpy()] = True
    phi = np.where(take_phi, c * cm - sine * sm, c - float(mm))
    logits = s64 * np.where(onehot, phi, c)
    onphi = onehot & take_phi
    with np.errstate(divide="ignore", invalid="ignore"):
        cancel = np.where(onphi & (sine > 0), s64 * sm * c * c / sine * U, 0.0)
        lbound = 5e-5 + 2e-5 * np.abs(logits) + cancel
        g = dlogits.numpy().astype(np.float64) * s64
        dphi = np.where(neg, cm, cm + sm * c / sine)
        dcos = np.where(onphi, g * dphi, g)
        dbound = np.where(onphi & ~neg, np.abs(g) * (8 * U * (cm + sm * np.abs(c) / sine) + sm * np.abs(c) ** 3 * U / (2 * sine ** 3)),
                          np.where(onphi, 3 * U * np.abs(g) * cm, 2 * U * np.abs(g)))
    dbound = np.where(np.isfinite(dcos), dbound, 0.0)
    return (torch.from_numpy(logits), torch.from_numpy(lbound), torch.from_numpy(dcos), torch.from_numpy(dbound),
            torch.from_numpy(onehot), torch.from_numpy(take_phi))


# ---- softmax cross-entropy, rank, mean ---------------------------------------------------------------------------------------
CE_SHAPES = [(1, 1), (2, 2), (3, 255), (3, 256), (3, 257), (64, 5994), (5, 16385)]
CE_KINDS = ("uniform", "aam", "equal", "huge", "neginf", "ties")
MEAN_SIZES = [1, 255, 256, 257, 1000]


def ce_inputs(B, S):
    """-> list of (logits [B][S], label [B], kinds): rounds until every row kind of the issue has been used.  uniform: scale 12;
    aam: the target 30, the rest in +-6; equal: one value (loss = log S, rank 0); huge: uniform in +-1e4 with the target at
    -1e4 and one +1e4 (no overflow; loss ~ max - target); neginf: every third non-target column -inf; ties: copies of the
    target value on both sides of the label and two strictly larger entries.  Labels include 0 and S - 1."""
    out = []
    for r0 in range(0, len(CE_KINDS), B):
        lg = rnd(3000 + S + r0, B, S, scale=12.0)
        lab = ints(3100 + S + r0, B, S)
        kinds = []
        for b in range(B):
            kind = CE_KINDS[(r0 + b) % len(CE_KINDS)]
            kinds.append(kind)
            lab[b] = (0, S - 1, int(lab[b]))[(r0 + b) % 3]
            t = int(lab[b])
            if kind == "aam":
                lg[b] *= 0.5
                lg[b, t] = 30.0
            elif kind == "equal":
                lg[b] = 3.25
            elif kind == "huge":
                lg[b] = (lg[b].double() * (1e4 / 12.0)).float()
                lg[b, t] = -1e4
                if S > 1:
                    lg[b, (t + 1) % S] = 1e4
            elif kind == "neginf":
                idx = torch.arange(S)
                lg[b, (idx % 3 == 0) & (idx != t)] = float("-inf")
            elif kind == "ties":
                for d in (-2, -1, 1, 2, 5):
                    if 0 <= t + d < S:
                        lg[b, t + d] = lg[b, t]
                for d in (-3, 3):
                    if 0 <= t + d < S:
                        lg[b, t + d] = lg[b, t] + 1.0
        out.append((lg, lab, kinds))
    return out


def ce_ref(logits, label, grad_scale):
    """loss_row = logsumexp(row) - row[label], dlogits = (softmax - onehot) grad_scale, rank = #{j: row[j] > row[label]}.
    O.cross_entropy on .double() inputs states the loss (its mean); the per-row values here are the same expression.

    Bounds: the project's 1e-5 (test_softmax_ce_large), per row:
      loss     1e-5 |loss| plus the conditioning of the final difference lse - target: both are rounded float32 numbers of
               magnitude up to |max| + log S and |target|, so 4 u (|max| + |target|) of absolute error is there however small the
               loss is (an AAM row with the target at 30 has a loss of 1e-9).
      dlogits  1e-5 of the row's own max |dlogits|, plus 2 u grad_scale softmax_j: the probability is a rounded float32 number
               before the one-hot is subtracted, so a target with p = 1 - 1e-8 keeps an absolute error of u however small
               p - 1 is.
      rank     exact (a float32 comparison)."""
    x = logits.double()
    t = x.gather(1, label.view(-1, 1)).squeeze(1)
    lse = torch.logsumexp(x, dim=1)
    loss = lse - t
    lbound = 1e-5 * loss.abs() + 4 * U * (x.max(1).values.abs() + t.abs())
    d = torch.softmax(x, dim=1)
    prob = d.clone()
    d[torch.arange(x.shape[0]), label] -= 1.0
    d = d * float(F32(grad_scale))
    dbound = 1e-5 * d.abs().max(1, keepdim=True).values + 2 * U * float(F32(grad_scale)) * prob
    rank = (logits > logits.gather(1, label.view(-1, 1))).sum(1).to(torch.int32)
    return loss, lbound, d, dbound, rank


def mean_ref(v):
    """mean_kernel adds in fp64 and rounds the quotient once: (1 + 1) u mean|v|"""
    return v.double().mean(), 2 * U * v.double().abs().mean()


# ---- relu_bwd, colsum -------------------------------------------------------------------------------------------------------
RELU_SIZES = [1, 255, 257, 100003]
COLSUM_SHAPES = [(1, 1), (37, 257), (256, 5994)]


def relu_inputs(n):
    """y with 0.0, -0.0, the smallest normal and the smallest subnormal float32 sprinkled in; dy"""
    y, dy = rnd(4000 + n, n), rnd(4100 + n, n)
    special = torch.tensor([0.0, -0.0, 1.1754944e-38, 1e-45, -1e-45], dtype=torch.float32)
    for i in range(0, n, 7):
        y[i] = special[(i // 7) % 5]
    return y, dy


def relu_ref(y, dy):
    return torch.where(y > 0, dy, torch.zeros_like(dy))


def colsum_ref(dy, prev=None):
    """colsum_kernel adds the M rows one after the other in float32: M - 1 roundings (one more with accumulate):
    (M + 1) u (sum|dy| + |prev|)"""
    M = dy.shape[0]
    s = dy.double().sum(0)
    a = dy.double().abs().sum(0)
    if prev is not None:
        s, a = s + prev.double(), a + prev.double().abs()
    return s, (M + 1) * U * a


# ---- GEMM -------------------------------------------------------------------------------------------------------------------
GBM, GBK = 64, 32
GEMM_FORMS = ("NT", "NN", "TN")        # linear_fwd (x w^T), linear_bwd dx (dy w), linear_bwd dw (dy^T x)
GEMM_MN = [(1, 1), (63, 65), (64, 64), (65, 63), (130, 1), (1, 130), (130, 130)]
GEMM_K = [1, 31, 32, 33, 64, 129, 5994]
# (A layout, B layout) pairs of a sweep case; a layout is (base offset in floats, row stride % 4 != 0)
GEMM_LAYOUTS = [(0, 0), (1, 0), (0, 1), (1, 1)]
GEMM_LAYOUT_PAIRS = [(0, 0), (1, 2), (2, 1), (3, 3), (0, 3), (3, 0)]


def gemm_splitk(M, N, K):
    """host restatement of spk_gemm_splitk (the GPU test checks it against the library)"""
    tiles = -(-M // GBM) * -(-N // GBM)
    chunks = -(-K // GBK)
    return max(1, min(-(-512 // tiles), chunks // 2, 32))


def gemm_kper(M, N, K):
    ns = gemm_splitk(M, N, K)
    return -(-(-(-K // ns)) // GBK) * GBK


def stage_paths(off, s_row, s_k, rows, K, kper):
    """which of gemm_stage's four paths the tiles of one operand take: pointer of tile (r0, k0) = base + r0 s_row + k0 s_k with
    base = off floats past a 16-byte boundary"""
    paths = set()
    for r0 in range(0, rows, GBM):
        nr = min(GBM, rows - r0)
        for kbeg in range(0, K, kper):
            kend = min(K, kbeg + kper)
            for k0 in range(kbeg, kend, GBK):
                ks = min(GBK, kend - k0)
                al = (off + r0 * s_row + k0 * s_k) % 4 == 0
                if s_k == 1 and al and s_row % 4 == 0 and ks == GBK:
                    paths.add("vec_k")
                elif s_row == 1 and al and s_k % 4 == 0 and nr == GBM:
                    paths.add("vec_rows")
                elif s_row == 1:
                    paths.add("scalar_rows")
                else:
                    paths.add("scalar_k")
    return paths


def _store(mat, layout):
    """mat [rows][inner] float32 -> (flat buffer, offset, ld): element (r, i) at buffer[offset + r ld + i]; the buffer's base is
    16-byte aligned, ld is a multiple of 4 or one more"""
    off, odd = layout
    rows, inner = mat.shape
    ld = -(-inner // 4) * 4 + (1 if odd else 0)
    buf = torch.full((off + rows * ld,), 7.5, dtype=torch.float32)      # the padding is never a zero
    buf[off:].view(rows, ld)[:, :inner] = mat
    return buf, off, ld


def gemm_problem(form, M, N, K, la=(0, 0), lb=(0, 0), seed=0):
    """operands of C[M][N] = sum_k A(m,k) B(k,n) in the memory layout of one of the three call forms of ops.linear_*.
    -> dict: abuf / bbuf (flat host buffers), aoff / boff, the four strides, A / Bm (the logical float32 matrices)"""
    A = rnd(5000 + seed, M, K)
    Bm = rnd(5001 + seed, K, N, scale=0.1)
    if form == "TN":
        abuf, aoff, lda = _store(A.t().contiguous(), la)
        sam, sak = 1, lda
    else:
        abuf, aoff, lda = _store(A, la)
        sam, sak = lda, 1
    if form == "NT":
        bbuf, boff, ldb = _store(Bm.t().contiguous(), lb)
        sbk, sbn = 1, ldb
    else:
        bbuf, boff, ldb = _store(Bm, lb)
        sbk, sbn = ldb, 1
    return dict(form=form, M=M, N=N, K=K, A=A, Bm=Bm, abuf=abuf, aoff=aoff, bbuf=bbuf, boff=boff, sam=sam, sak=sak, sbk=sbk,
                sbn=sbn)


# (M, N, K, alpha, bias, accumulate, out is a column slice of a wider tensor): K = 31 is the direct path, 129 split-K 2,
# 256 split-K 4, 5994 split-K 32
GEMM_EPILOGUES = [(37, 70, 129, 0.37, False, False, False), (37, 70, 129, 1.0, True, True, False),
                  (65, 63, 31, 1.0, False, False, True), (65, 63, 129, 1.0, False, False, True),
                  (65, 63, 256, 0.37, True, True, True), (65, 63, 5994, 0.37, True, True, True),
                  (1, 1, 1, 0.37, True, True, True)]


def gemm_sweep():
    for form in GEMM_FORMS:
        for M, N in GEMM_MN:
            for K in GEMM_K:
                yield form, M, N, K


def gemm_paths(p):
    kper = gemm_kper(p["M"], p["N"], p["K"])
    return (stage_paths(p["aoff"], p["sam"], p["sak"], p["M"], p["K"], kper),
            stage_paths(p["boff"], p["sbn"], p["sbk"], p["N"], p["K"], kper))


def gemm_ref(A, Bm, alpha=1.0, bias=None, prev=None):
    """C = alpha A B (+ bias) (+ prev) in fp64 from the float32 operands.

    Bound: one K slice (min(kper, K) steps) runs through v_mfma_f32_32x32x2_f32 with at most one rounding per k step; the
    slices are folded in fp64 and rounded once; alpha, bias and accumulate add one rounding each.  The staging path only chooses
    how a tile reaches LDS, never the order of the sum.   (kslice + 4 + 1) u (|alpha| (|A| |B|)[m][n] + |bias[n]| + |prev[m][n]|)"""
    M, K = A.shape
    N = Bm.shape[1]
    a = float(F32(alpha))
    C = a * (A.double() @ Bm.double())
    mag = abs(a) * (A.double().abs() @ Bm.double().abs())
    if bias is not None:
        C, mag = C + bias.double(), mag + bias.double().abs()
    if prev is not None:
        C, mag = C + prev.double(), mag + prev.double().abs()
    return C, (min(gemm_kper(M, N, K), K) + 5) * U * mag


def head_gemm_calls(B, S, D=256, seed=0):
    """the three GEMM calls of the AAM head exactly as engine.py writes them (forward_train / backward): name, A, Bm (contiguous
    float32 tensors), the ops.gemm argument tuple (M, N, K, sam, sak, sbk, sbn), and the logical A [M][K] / B [K][N]"""
    hn, wn, dcos = rnd(5100 + seed, B, D, scale=0.1), rnd(5101 + seed, S, D, scale=0.1), rnd(5102 + seed, B, S, scale=1.0 / B)
    return [("cos", hn, wn, (B, S, D, D, 1, 1, D), hn, wn.t()),
            ("dhn", dcos, wn, (B, D, S, S, 1, D, 1), dcos, wn),
            ("dwn", dcos, hn, (S, D, B, 1, S, D, 1), dcos.t(), hn)]


# ---- statistics pooling -----------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 10, 2, 256), (1, 3, 1, 32), (2, 5, 38, 96), (1, 10, 375, 256), (2, 10, 13, 1024), (3, 1, 7, 33)]    # B, H, W, C
POOL_OFFSET_SHAPE = (1, 10, 375, 256)      # 100 + 0.01 uniform: variance 1e-8 of the mean square


def pool_inputs(B, H, Wd, C, mode, offset=False):
    """x NCHW [B][C][H][W] >= 0 (as after ReLU), gout [B][C H (2)]"""
    x = uni(6000 + Wd + C, B, C, H, Wd)
    if offset:
        x = (100.0 + 0.01 * x.double()).float()
    gout = rnd(6100 + Wd + C, B, C * H * (2 if mode else 1))
    return x, gout


def pool_ref(x, gout, mode):
    """O.stats_pool on the .double() input, flattened as nn.Flatten(1, -1), and its fp64 autograd gradient.

    Bounds: rtol 2e-6 / atol 1e-7 forward and rtol 2e-5 / atol 1e-7 backward (test_stats_pool_golden_and_random), per element,
    plus the one conditioning term of the two-pass form: the mean is a running float32 sum of W terms, |d mean| <= dm =
    (W/2 + 1) u max|x| (each addition rounds at the size of the partial sum).  A shifted mean moves the centred second moment by
    exactly W dm^2 (the cross term vanishes), so the variance by W/(W-1) dm^2; it moves every x - mean of the backward by dm,
    so dx by |2 g_var / (W - 1)| dm.  For ordinary data these terms are ~1e-12; for 100 + 0.01 uniform at W = 375 they allow up to
    20 % of the variance (8e-6), where a one-pass sum of squares is off by several times the variance itself."""
    name = "mean+std" if mode else "mean"
    B, C, H, Wd = x.shape
    xd = x.double().requires_grad_(True)
    y = O.stats_pool(xd, name).flatten(1)
    dx, = torch.autograd.grad(y, [xd], grad_outputs=gout.double())
    y = y.detach()
    dm = (Wd / 2 + 1) * U * x.double().abs().amax(dim=3)                 # [B][C][H]
    ybound = 2e-6 * y.abs() + 1e-7
    dxbound = 2e-5 * dx.abs() + 1e-7
    if mode and Wd > 1:
        extra = torch.cat([Wd / (Wd - 1.0) * dm * dm, torch.zeros_like(dm)], dim=-1).flatten(1)     # [B][C][2H]: var half only
        ybound = ybound + extra
        gvar = gout.double().view(B, C, 2 * H)[:, :, :H]
        dxbound = dxbound + (2.0 * gvar.abs() / (Wd - 1) * dm)[..., None]
    return y, ybound, dx, dxbound


# ---- SGD --------------------------------------------------------------------------------------------------------------------
SGD_SIZES = [1, 2, 3, 4, 5, 1023, 10007, 4194304 + 1024 + 3]
SGD_HYPER = [(0.1, 0.9, 5e-4, 1.0), (0.05, 0.9, 1e-4, 0.125), (0.1, 0.0, 0.0, 1.0)]      # lr, momentum, wd, grad_scale


def sgd_inputs(n):
    return rnd(7000 + n % 9973, n), rnd(7001 + n % 9973, n), rnd(7002 + n % 9973, n)      # p0, g1, g2


def sgd_ref(p, g, buf, lr, mom, wd, gs, first):
    """one step of g' = g gs + wd p;  buf = first ? g' : mom buf + g';  p -= lr buf in fp64 from float32 p, g, buf (the state the
    code under test holds before the step) and the float32 roundings of the scalars.

    Bounds: g' is two products and a sum (3 roundings), buf one product and a sum more (5 in all), the update one product and a
    difference:     |buf - ref| <= (5 + 1) u (|g gs| + |wd p| + |mom buf|)
                    |p - ref|   <= lr times that, plus (2 + 1) u (|p| + lr |buf'|)"""
    lr, mom, wd, gs = (float(F32(v)) for v in (lr, mom, wd, gs))
    p, g = p.double(), g.double()
    gp = g * gs + wd * p
    mag = (g * gs).abs() + (wd * p).abs()
    if first:
        b = gp
    else:
        b = mom * buf.double() + gp
        mag = mag + (mom * buf.double()).abs()
    bbound = 6 * U * mag
    pn = p - lr * b
    pbound = lr * bbound + 3 * U * (p.abs() + lr * b.abs())
    return pn, pbound, b, bbound


# ---- scoring ----------------------------------------------------------------------------------------------------------------
CN_SHAPES = [(1, 1), (5, 63), (6, 256), (3001, 256)]
TC_D = [3, 63, 64, 256, 260, 512]
TC_T = [1, 5, 20000]
TOPK_M = [2, 3, 255, 256, 257, 5994, 8192, 8193, 16384]


def cn_inputs(N, D, with_mean):
    emb = rnd(8000 + N + D, N, D)
    mean = rnd(8100 + D, D, scale=0.1) if with_mean else None
    emb[N // 2] = mean if with_mean else 0.0          # centred to exactly zero: the output row is 0
    return emb, mean


def cn_ref(emb, mean, eps):
    """v = emb - mean; out = v / max(||v||, eps).  v carries one rounding; the squared norm ns + 2 more than l2norm's (the
    product is not fused, v itself is rounded), so    |out - ref| <= (ns/2 + 6) u |out|.  The zero row is exact."""
    v = emb.double() - (mean.double() if mean is not None else 0.0)
    n = v.pow(2).sum(1).sqrt()
    e32 = float(F32(eps))
    assert bool(((n - e32).abs() > 1e-3 * e32).all())
    out = v / torch.clamp(n, min=e32)[:, None]
    return out, (l2_chain(emb.shape[1]) / 2 + 6) * U * out.abs()


def tc_inputs(D, T, same):
    n_en, n_te = 50, (50 if same else 70)
    en = rnd(8200 + D, n_en, D, scale=0.2)
    te = en if same else rnd(8300 + D, n_te, D, scale=0.2)
    ia, ib = ints(8400 + T, T, n_en).to(torch.int32), ints(8500 + T, T, n_te).to(torch.int32)
    ia[0], ib[0] = 0, n_te - 1
    ia[-1], ib[-1] = n_en - 1, 0
    if T >= 5:
        ia[1:4], ib[1:4] = 7, 7            # repeated trials
    return en, te, ia, ib


def tc_ref(en, te, ia, ib):
    """out[t] = <en[ia[t]], te[ib[t]]>.  D % 4 == 0: a lane adds four products and the running sum per 256-wide step
    (5 roundings each), else one product and one sum per 64-wide step; six shuffle-tree additions:
    (n + 1) u sum|a b| with n = 5 ceil(D/256) + 6 or 2 ceil(D/64) + 6."""
    a, b = en.double()[ia.long()], te.double()[ib.long()]
    D = en.shape[1]
    n = 5 * -(-D // 256) + 6 if D % 4 == 0 else 2 * -(-D // 64) + 6
    return (a * b).sum(1), (n + 1) * U * (a * b).abs().sum(1)


def topk_ks(M):
    return sorted({2, min(300, M), M})


def topk_inputs(M):
    """scores [3][M + 3] whose first M columns are the problem (ld > M; the 3 columns beyond are a 1e30 sentinel): row 0 random,
    row 1 all equal (0.5: every partial sum is exact, std = 0), row 2 quantised to 7 levels (many duplicates around the k-th)"""
    full = torch.full((3, M + 3), 1e30, dtype=torch.float32)
    full[0, :M] = rnd(8600 + M, M)
    full[1, :M] = 0.5
    full[2, :M] = torch.floor(uni(8700 + M, M) * 7) / 8
    return full


def topk_ref(scores, k):
    """mean and unbiased std of the k largest entries of each row: np.sort in fp64 (the selection is exact on float32 values).

    Bounds: the mean is a per-thread chain of ceil(k/256) additions, six shuffle steps, three additions and a division:
    nm = ceil(k/256) + 10 roundings,  |mu - ref| <= dmu = (nm + 1) u mean|top|.  The squared deviations add the same way with
    two more roundings per term; sqrt halves the relative error: (nm/2 + 3) u std.  A shifted mean adds exactly k dmu^2 to
    the sum of squares (the cross term vanishes), so at most sqrt(k / (k - 1)) dmu to the std."""
    top = -np.sort(-scores.numpy().astype(np.float64), axis=1)[:, :k]
    mu = top.mean(1)
    sd = top.std(1, ddof=1)
    nm = -(-k // 256) + 10
    dmu = (nm + 1) * U * np.abs(top).mean(1)
    return (torch.from_numpy(mu), torch.from_numpy(dmu), torch.from_numpy(sd),
            torch.from_numpy((nm / 2 + 3) * U * sd + math.sqrt(k / (k - 1.0)) * dmu))
