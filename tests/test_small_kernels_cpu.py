"""Pins tests/small_kernels_ref.py without the code it will judge (no GPU, no library):
  * its fp64 restatements reproduce tests/golden/kernels.npz, which the reference generated, to the goldens' own tolerances;
  * float32 torch on the CPU - the reference's own arithmetic - stays inside every bound on every engineered input that
    tests/test_small_kernels_gpu.py feeds the kernels, with the same NaN / inf pattern, so the reference alone passes each
    of those tests;
  * the known places where torch autograd and the kernels' rule differ are stated and checked here."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_kernels_ref as R
from oracle import spk_oracle as O


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ---- goldens ------------------------------------------------------------------------------------------------------------------
def test_restatements_reproduce_the_aam_head_golden(gold_dir):
    g = np.load(os.path.join(gold_dir, "kernels.npz"))
    e, w, lab = torch.from_numpy(g["aam_e"]), torch.from_numpy(g["aam_w"]), torch.from_numpy(g["aam_lab"])
    B = e.shape[0]
    en = R.l2norm_ref(e, torch.zeros_like(e))[0]
    wn = R.l2norm_ref(w, torch.zeros_like(w))[0]
    cosv = (en @ wn.t()).float()
    logits, _, _, _, _, _ = R.aam_ref(cosv, lab, torch.ones_like(cosv), 0.2, 30.0)
    np.testing.assert_allclose(logits.numpy(), g["aam_logits"], rtol=2e-5, atol=5e-5)
    loss, _, dl, _, rank = R.ce_ref(logits.float(), lab, 1.0 / B)
    assert abs(float(loss.mean()) - float(g["aam_loss"])) < 1e-4
    assert abs(float(loss.mean()) - float(O.cross_entropy(logits.float().double(), lab))) < 1e-12
    dcos = R.aam_ref(cosv, lab, dl.float(), 0.2, 30.0)[2]
    de = R.l2norm_ref(e, (dcos @ wn).float())[2]
    dw = R.l2norm_ref(w, (dcos.t() @ en).float())[2]
    assert relerr(de, torch.from_numpy(g["aam_ge"])) < 1e-4
    assert relerr(dw, torch.from_numpy(g["aam_gw"])) < 1e-4
    acc1, acc5 = O.accuracy(torch.from_numpy(g["aam_logits"]), lab, (1, 5))
    assert abs(float((rank < 1).float().mean() * 100) - float(acc1)) < 1e-4
    assert abs(float((rank < 5).float().mean() * 100) - float(acc5)) < 1e-4


def test_restatements_reproduce_the_pool_golden(gold_dir):
    g = np.load(os.path.join(gold_dir, "kernels.npz"))
    x = torch.from_numpy(g["pool_x"])
    for mode, name in [(0, "mean"), (1, "mean+std")]:
        gy = torch.from_numpy(g["pool_%s_gy" % name].reshape(2, -1))
        y, _, dx, _ = R.pool_ref(x, gy, mode)
        np.testing.assert_allclose(y.numpy(), g["pool_%s_y" % name].reshape(2, -1), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(dx.numpy(), g["pool_%s_gx" % name], rtol=1e-5, atol=1e-7)


# ---- float32 torch inside every bound ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.L2_SHAPES)
def test_torch_l2norm_is_inside_the_bounds(shape):
    x, dy, prev = R.l2norm_inputs(*shape)
    y, yb, dx, dxb, clamped = R.l2norm_ref(x, dy)
    if shape[0] >= 5:
        assert clamped.tolist()[:4] == [False, True, True, False]
        assert float(y[1].abs().max()) == 0.0 and bool(torch.isfinite(dx[1]).all()) and float(dx[1].abs().max()) > 1e9
    xt = x.clone().requires_grad_(True)
    yt = F.normalize(xt, eps=R.L2_EPS)
    R.check("l2norm_fwd", yt, y, yb)
    gt, = torch.autograd.grad(yt, [xt], grad_outputs=dy)
    R.check("l2norm_bwd", gt, dx, dxb)
    R.check("l2norm_bwd+acc", prev + gt, prev.double() + dx, dxb + R.U * (prev.double() + dx).abs())


def test_l2norm_squares_that_overflow_float32_are_left_out():
    """known non-agreement, left out of the GPU inputs: a row whose squares overflow float32 (|x| > 1.8e19) has an infinite
    float32 norm, so the reference (and the kernel) returns y = 0 where the exact answer is a unit vector"""
    x = torch.full((1, 4), 3e19)
    assert float(F.normalize(x).abs().max()) == 0.0
    assert abs(float(R.l2norm_ref(x, torch.zeros_like(x))[0][0, 0]) - 0.5) < 1e-12
    for shape in R.L2_SHAPES:
        assert float(R.l2norm_inputs(*shape)[0].abs().max()) < 1e18


def aam_torch(cosine, label, m, s):
    """AAMLayer.forward from `cosine` on (oracle/spk_oracle.py aam_logits, scripts/model.py:487-499), any dtype"""
    import math
    cos_m, sin_m = math.cos(m), math.sin(m)
    th = math.cos(math.pi - m)
    mm = math.sin(math.pi - m) * m
    sine = torch.sqrt((1.0 - cosine * cosine).clamp(0, 1))
    phi = cosine * cos_m - sine * sin_m
    phi = torch.where((cosine - th) > 0, phi, cosine - mm)
    one_hot = torch.zeros_like(cosine)
    one_hot.scatter_(1, label.view(-1, 1), 1)
    return (one_hot * phi + (1.0 - one_hot) * cosine) * s


def aam_autograd_nan(cosv, onehot):
    """the elements where torch autograd of the reference expression returns NaN although the chosen branch has a derivative:
    1 - c^2 == 0 exactly (|c| == 1) on a column whose phi receives a ZERO gradient - every non-label column (one_hot * phi) and a
    label column that took c - mm (where() routes 0 to phi) - because sqrt's backward turns that 0 into 0 / 0."""
    return (cosv.abs() == 1.0) & ~(onehot & (cosv == 1.0))


@pytest.mark.parametrize("ms", R.AAM_MS)
@pytest.mark.parametrize("shape", R.AAM_SHAPES)
def test_torch_aam_margin_is_inside_the_bounds(shape, ms):
    m, s = ms
    seen = set()
    for cosv, lab, dl in R.aam_inputs(*shape, m):
        logits, lb, dcos, db, onehot, take_phi = R.aam_ref(cosv, lab, dl, m, s)
        ct = cosv.clone().requires_grad_(True)
        lt = aam_torch(ct, lab, m, s)
        R.check("aam_margin_fwd", lt, logits, lb)
        gt, = torch.autograd.grad(lt, [ct], grad_outputs=dl)
        nanset = aam_autograd_nan(cosv, onehot)
        assert bool(torch.isnan(gt[nanset]).all()), "torch autograd is expected to give NaN on these elements"
        # the restatement (and the kernel) give the derivative of the branch that was taken there: s * dlogits
        assert torch.equal(dcos[nanset], dl.double()[nanset] * s)
        R.check("aam_margin_bwd", gt, dcos, db, skip=nanset)
        labv = cosv[onehot]
        seen |= set(labv.tolist())
        # the branch float32 decides: th and the value below take c - mm, the value above takes phi
        th = R.aam_consts(m)[2]
        for v, phi in ((th, False), (np.nextafter(th, R.F32(-2)), False), (np.nextafter(th, R.F32(1)), True)):
            sel = onehot & (cosv == float(v))
            assert bool((take_phi[sel] == phi).all())
        one = onehot & (cosv == 1.0)
        assert bool(torch.isinf(dcos[one]).all()) and torch.equal(torch.sign(dcos[one]), torch.sign(dl.double()[one]))
    assert seen >= set(float(v) for v in R.aam_label_values(m)), "every engineered label value is used"
    assert shape[1] < 3 or (bool((cosv == 1.0).any()) and bool((cosv == -1.0).any()))


def test_aam_threshold_and_clamp_decisions_in_float32():
    """the float32 facts the engineered label values rest on (m = 0.2)"""
    cos_m, sin_m, th, mm = R.aam_consts(0.2)
    assert abs(float(th) + 0.9800666) < 1e-7
    one = R.F32(1)
    assert one - one * one == 0
    up, dn = np.nextafter(one, R.F32(2)), np.nextafter(one, R.F32(0))
    assert abs(float(one - up * up) + 2.38e-7) < 1e-9 and abs(float(one - dn * dn) - 1.19e-7) < 1e-9
    assert 1.0 - float(up) ** 2 < 0 < 1.0 - float(dn) ** 2
    # the two branches differ by ~0.02 at th: far above any tolerance on the logit
    c = float(th)
    assert abs((c * float(cos_m) - np.sqrt(1 - c * c) * float(sin_m)) - (c - float(mm))) > 0.015


@pytest.mark.parametrize("shape", R.CE_SHAPES)
def test_torch_softmax_ce_is_inside_the_bounds(shape):
    B, S = shape
    kinds_seen = set()
    for lg, lab, kinds in R.ce_inputs(B, S):
        kinds_seen |= set(kinds)
        for gs in (1.0 / B, 1.0 / (8 * B)):
            loss, lb, d, db, rank = R.ce_ref(lg, lab, gs)
            lt = lg.clone().requires_grad_(True)
            rows = F.cross_entropy(lt, lab, reduction="none")
            R.check("softmax_ce loss", rows, loss, lb)
            gt, = torch.autograd.grad(rows.sum() * R.F32(gs), [lt])
            R.check("softmax_ce dlogits", gt, d, db)
        assert bool(torch.isfinite(loss).all())
        for b, kind in enumerate(kinds):
            t = int(lab[b])
            if kind == "equal":
                assert abs(float(loss[b]) - np.log(S)) < 1e-12 and int(rank[b]) == 0
            if kind == "huge" and S > 1:
                assert abs(float(loss[b]) - 2e4) <= np.log(S)
            if kind == "ties" and S >= 8:
                # known non-agreement: the kernel counts strictly greater entries, topk breaks ties by index - with equal
                # entries left of the label the reference's top-k places the target later than `rank` says.  Harmless: exact
                # float32 ties between logits of different classes do not happen in training, and rank is the optimistic
                # (and order-independent) reading of "correct@k".
                assert int(rank[b]) == int((lg[b] > lg[b, t]).sum())
                ties_left = int((lg[b, :t] == lg[b, t]).sum())
                assert ties_left > 0 or t < 1
                pos = int((torch.sort(lg[b], descending=True, stable=True).indices == t).nonzero()[0])
                assert pos == int(rank[b]) + ties_left
                assert int((torch.topk(lg[b], S).indices == t).nonzero()[0]) >= int(rank[b])
        mu, mb = R.mean_ref(loss.float())
        R.check("mean", loss.float().mean(), mu, mb)
    assert kinds_seen == set(R.CE_KINDS)


@pytest.mark.parametrize("n", R.MEAN_SIZES)
def test_torch_mean_is_inside_the_bound(n):
    v = R.uni(3500 + n, n) * 10
    mu, mb = R.mean_ref(v)
    R.check("mean", v.mean(), mu, mb)


def test_torch_relu_bwd_and_colsum():
    for n in R.RELU_SIZES:
        y, dy = R.relu_inputs(n)
        yt = y.clone().requires_grad_(True)
        # threshold_backward of F.relu's OUTPUT > 0, as the engine differentiates the stored activation
        gt = torch.where(yt.detach() > 0, dy, torch.zeros_like(dy))
        assert torch.equal(gt, R.relu_ref(y, dy))
        assert float(R.relu_ref(torch.tensor([1e-45, -0.0, 0.0]), torch.ones(3)).sum()) == 1.0
    for M, N in R.COLSUM_SHAPES:
        dy, prev = R.rnd(4200 + N, M, N), R.rnd(4300 + N, N)
        s, b = R.colsum_ref(dy)
        R.check("colsum", dy.sum(0), s, b)
        s, b = R.colsum_ref(dy, prev)
        R.check("colsum+acc", prev + dy.sum(0), s, b)


def test_gemm_table_reaches_every_staging_path_and_split():
    """pure host logic: the problem table of the GPU test takes each of gemm_stage's four paths for A and for B, and reaches
    split-K counts 1, 2, 4 and 32"""
    pa, pb, splits = set(), set(), set()
    for form, M, N, K in R.gemm_sweep():
        for ia, ib in R.GEMM_LAYOUT_PAIRS:
            p = R.gemm_problem(form, M, N, 1 if K > 1000 else K, R.GEMM_LAYOUTS[ia], R.GEMM_LAYOUTS[ib])   # strides only
            p["K"] = K
            a, b = R.gemm_paths(p)
            pa |= a
            pb |= b
        splits.add(R.gemm_splitk(M, N, K))
    allp = {"vec_k", "vec_rows", "scalar_rows", "scalar_k"}
    assert pa == allp and pb == allp, (pa, pb)
    for c in R.GEMM_EPILOGUES:
        splits.add(R.gemm_splitk(*c[:3]))
    assert splits >= {1, 2, 4, 32}, splits
    assert [R.gemm_splitk(*c[3][:3]) for c in R.head_gemm_calls(6, 5994)] == [4, 32, 1]
    # the head's strided forms at S = 5994: sak = S with S % 4 = 2 is a scalar path, K = 5994 leaves a 10-wide tail chunk
    assert 5994 % 4 == 2 and 5994 % 32 == 10
    assert "scalar_rows" in R.stage_paths(0, 1, 5994, 5994, 6, R.gemm_kper(5994, 256, 6))


@pytest.mark.parametrize("form", R.GEMM_FORMS)
def test_torch_gemm_is_inside_the_bound(form):
    for f, M, N, K in R.gemm_sweep():
        if f != form:
            continue
        p = R.gemm_problem(form, M, N, K)
        C, b = R.gemm_ref(p["A"], p["Bm"])
        R.check("gemm", p["A"] @ p["Bm"], C, b)
    for M, N, K, alpha, bias, acc, _ in R.GEMM_EPILOGUES:
        p = R.gemm_problem("NT", M, N, K, seed=7)
        bv = R.rnd(5200, N) if bias else None
        prev = R.rnd(5201, M, N) if acc else None
        C, b = R.gemm_ref(p["A"], p["Bm"], alpha, bv, prev)
        out = (p["A"] @ p["Bm"]) * alpha
        out = out + bv if bias else out
        out = out + prev if acc else out
        R.check("gemm epilogue", out, C, b)


@pytest.mark.parametrize("B,S", [(6, 1211), (37, 1211), (6, 5994), (37, 5994)])
def test_torch_head_gemms_are_inside_the_bound(B, S):
    for name, _, _, _, A, Bm in R.head_gemm_calls(B, S):
        C, b = R.gemm_ref(A, Bm)
        R.check("gemm head " + name, A @ Bm, C, b)


@pytest.mark.parametrize("shape", R.POOL_SHAPES + ["offset"])
@pytest.mark.parametrize("mode", [0, 1])
def test_torch_stats_pool_is_inside_the_bounds(shape, mode):
    offset = shape == "offset"
    B, H, Wd, C = R.POOL_OFFSET_SHAPE if offset else shape
    x, gout = R.pool_inputs(B, H, Wd, C, mode, offset)
    assert float(x.min()) >= 0.0
    y, yb, dx, dxb = R.pool_ref(x, gout, mode)
    xt = x.clone().requires_grad_(True)
    yt = O.stats_pool(xt, "mean+std" if mode else "mean").flatten(1)
    R.check("stats_pool_fwd", yt, y, yb)
    gt, = torch.autograd.grad(yt, [xt], grad_outputs=gout)
    R.check("stats_pool_bwd", gt, dx, dxb)
    if mode and Wd == 1:            # 0 / 0: the variance half is NaN, the sqrt(mean) half finite
        yv = y.view(B, C, 2 * H)
        assert bool(torch.isnan(yv[:, :, :H]).all()) and bool(torch.isfinite(yv[:, :, H:]).all())
    if offset and mode:
        # the bound separates the two-pass form from a one-pass sum of squares: float32 sum x^2 - W mean^2, scaled to unbiased
        x32 = x.numpy()
        s1 = np.cumsum(x32, axis=3, dtype=np.float32)[..., -1]
        s2 = np.cumsum(x32 * x32, axis=3, dtype=np.float32)[..., -1]
        mean = s1 / np.float32(Wd)
        onepass = (s2 / np.float32(Wd) - mean * mean) * np.float32(Wd / (Wd - 1.0))
        var, vb = y.view(B, C, 2 * H)[:, :, :H].numpy(), yb.view(B, C, 2 * H)[:, :, :H].numpy()
        assert float((vb / var).max()) < 0.25
        assert float(np.median(np.abs(onepass - var) / vb)) > 5.0


@pytest.mark.parametrize("hyper", R.SGD_HYPER)
@pytest.mark.parametrize("n", R.SGD_SIZES)
def test_torch_sgd_is_inside_the_bounds(n, hyper):
    lr, mom, wd, gs = hyper
    p0, g1, g2 = R.sgd_inputs(n)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([p], lr=lr, momentum=mom, weight_decay=wd)
    buf = None
    for first, g in ((True, g1), (False, g2)):
        before = p.detach().clone()
        pr, pb, br, bb = R.sgd_ref(before, g, buf, lr, mom, wd, gs, first)
        p.grad = g * R.F32(gs)        # 1 and 0.125: exact products, so torch sees the same g gs the kernel forms
        opt.step()
        R.check("sgd p", p.detach(), pr, pb)
        if mom != 0:
            buf = opt.state[p]["momentum_buffer"].clone()
            R.check("sgd buf", buf, br, bb)
        else:
            buf = br.float()


@pytest.mark.parametrize("shape", R.CN_SHAPES)
def test_torch_center_normalize_is_inside_the_bound(shape):
    for with_mean in (False, True):
        for eps in (1e-8, 1e-12):
            emb, mean = R.cn_inputs(*shape, with_mean)
            out, b = R.cn_ref(emb, mean, eps)
            assert float(out[shape[0] // 2].abs().max()) == 0.0
            R.check("center_normalize", F.normalize(emb - mean if with_mean else emb, eps=eps), out, b)


@pytest.mark.parametrize("D", R.TC_D)
def test_torch_trial_cosine_is_inside_the_bound(D):
    for T in R.TC_T:
        for same in (True, False):
            en, te, ia, ib = R.tc_inputs(D, T, same)
            assert T < 2 or int(ia.min()) == 0 and int(ia.max()) == en.shape[0] - 1 and int(ib.min()) == 0 and int(ib.max()) == te.shape[0] - 1
            s, b = R.tc_ref(en, te, ia, ib)
            R.check("trial_cosine", (en[ia.long()] * te[ib.long()]).sum(1), s, b)


@pytest.mark.parametrize("M", R.TOPK_M)
def test_torch_topk_mean_std_is_inside_the_bounds(M):
    full = R.topk_inputs(M)
    sc = full[:, :M]
    for k in R.topk_ks(M):
        mu, mb, sd, sb = R.topk_ref(sc, k)
        top = torch.topk(sc, k, dim=1).values
        sdt, mut = torch.std_mean(top, dim=1)
        R.check("topk mean", mut, mu, mb)
        R.check("topk std", sdt, sd, sb)
        assert float(sd[1]) == 0.0 and float(mu[1]) == 0.5          # the all-equal row
        if k < M and M >= 255:
            srt = np.sort(sc[2].numpy())[::-1]
            assert srt[k - 1] == srt[k], "the quantised row has duplicates across the k-th place"
