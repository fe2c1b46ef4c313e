"""Parity of the kernels around the trunk (csrc/head.hip, pool.hip, gemm.hip, sgd.hip, score.hip) on a real MI355X against the
fp64 restatements of tests/small_kernels_ref.py: per-element bounds derived there, on the engineered inputs built there - the
same inputs on which tests/test_small_kernels_cpu.py shows float32 torch to stay inside those bounds.  Every comparison goes
through small_kernels_ref.check: |got - ref64| <= bound(element), identical NaN / inf pattern, nothing masked unless named."""
import numpy as np
import pytest
import torch

import small_kernels_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops as _ops
    yield _ops
    print("\nlargest error / bound per kernel: " + ", ".join("%s %.3g" % kv for kv in sorted(R.RATIOS.items())))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(x):
    return x.cpu().permute(0, 3, 1, 2).contiguous()


# ---- l2norm -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.L2_SHAPES)
def test_l2norm_fwd_bwd(ops, shape):
    x, dy, prev = R.l2norm_inputs(*shape)
    y, yb, dx, dxb, clamped = R.l2norm_ref(x, dy)
    yg, inv = ops.l2norm_fwd(x.cuda())
    R.check("l2norm_fwd", yg, y, yb)
    if shape[0] >= 5:
        assert float(yg[1].abs().max()) == 0.0                      # the all-zero row
        assert float(inv[1]) == float(inv[2]) == float(np.float32(1) / np.float32(R.L2_EPS))      # clamped rows: 1 / eps
    dxg = ops.l2norm_bwd(yg, inv, dy.cuda())
    R.check("l2norm_bwd", dxg, dx, dxb)                            # the zero row's dy / eps is a value check like any other
    acc = prev.cuda()
    out = ops.l2norm_bwd(yg, inv, dy.cuda(), out=acc, accumulate=True)
    assert out.data_ptr() == acc.data_ptr()
    R.check("l2norm_bwd+acc", acc, prev.double() + dx, dxb + R.U * (prev.double() + dx).abs())


# ---- AAM margin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms", R.AAM_MS)
@pytest.mark.parametrize("shape", R.AAM_SHAPES)
def test_aam_margin_fwd_bwd(ops, shape, ms):
    m, s = ms
    for cosv, lab, dl in R.aam_inputs(*shape, m):
        logits, lb, dcos, db, onehot, take_phi = R.aam_ref(cosv, lab, dl, m, s)
        lg = ops.aam_margin_fwd(cosv.cuda(), lab.cuda(), m, s)
        # the rows one ulp either side of th land on the branch float32 decides: the branches differ by ~0.02 s there
        R.check("aam_margin_fwd", lg, logits, lb)
        dg = ops.aam_margin_bwd(cosv.cuda(), lab.cuda(), dl.cuda(), m, s)
        # Nothing is masked.  Where torch autograd of the reference expression gives NaN - |c| == 1 exactly on a non-label column
        # or on a label column that took c - mm: sqrt's backward turns the ZERO gradient routed to the unused phi into 0 / 0
        # (tests/test_small_kernels_cpu.py checks that) - the kernel returns the derivative of the branch that was taken,
        # s * dlogits, which is what the restatement states.  Harmless: that NaN is an artefact of differentiating an unused
        # expression, and a cosine of exactly +-1 off the label does not survive a float32 GEMM of normalised rows anyway.
        R.check("aam_margin_bwd", dg, dcos, db)
        one = onehot & (cosv == 1.0)                               # label at exactly 1: +-inf with the sign of dlogits
        assert bool(torch.isinf(dg.cpu()[one]).all()) and torch.equal(torch.sign(dg.cpu()[one]), torch.sign(dl[one]))


# ---- softmax cross-entropy, rank, mean -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.CE_SHAPES)
def test_softmax_ce_rank_and_mean(ops, shape):
    B, S = shape
    for lg, lab, kinds in R.ce_inputs(B, S):
        lgg, labg = lg.cuda(), lab.cuda()
        for gs in (1.0 / B, 1.0 / (8 * B)):                         # one process, and the world-size-8 scale
            loss, lb, d, db, rank = R.ce_ref(lg, lab, gs)
            loss_row, dl, rk = ops.softmax_ce(lgg, labg, grad_scale=gs)
            R.check("softmax_ce loss", loss_row, loss, lb)
            R.check("softmax_ce dlogits", dl, d, db)
            # rank counts strictly greater entries (exact); the reference's topk orders ties by index, which can only place
            # the target later (tests/test_small_kernels_cpu.py) - pinned as the kernel's rule
            assert torch.equal(rk.cpu(), rank)
        loss_only, none_dl, none_rk = ops.softmax_ce(lgg, labg, grad_scale=None, want_rank=False)      # NULL dlogits / rank
        assert none_dl is None and none_rk is None
        assert torch.equal(loss_only, loss_row)
        mu, mb = R.mean_ref(loss_row.cpu())
        R.check("mean", ops.mean(loss_row), mu, mb)


@pytest.mark.parametrize("n", R.MEAN_SIZES)
def test_mean(ops, n):
    v = R.uni(3500 + n, n) * 10
    mu, mb = R.mean_ref(v)
    R.check("mean", ops.mean(v.cuda()), mu, mb)


# ---- relu_bwd, colsum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.RELU_SIZES)
def test_relu_bwd(ops, n):
    y, dy = R.relu_inputs(n)
    assert torch.equal(ops.relu_bwd(y.cuda(), dy.cuda()).cpu(), R.relu_ref(y, dy))


@pytest.mark.parametrize("M,N", R.COLSUM_SHAPES)
def test_colsum(ops, M, N):
    dy, prev = R.rnd(4200 + N, M, N), R.rnd(4300 + N, N)
    dyg = dy.cuda()
    for acc in (False, True):
        db = prev.cuda() if acc else torch.full((N,), float("nan"), device="cuda")
        ops.call("spk_colsum", ops.ptr(dyg), ops.ptr(db), M, N, 1 if acc else 0, ops.stream())
        s, b = R.colsum_ref(dy, prev if acc else None)
        R.check("colsum+acc" if acc else "colsum", db, s, b)


# ---- GEMM -----------------------------------------------------------------------------------------------------------------------
def run_gemm(ops, p, **kw):
    a, b = p["abuf"].cuda()[p["aoff"]:], p["bbuf"].cuda()[p["boff"]:]
    assert a.data_ptr() % 16 == 4 * (p["aoff"] % 4) and b.data_ptr() % 16 == 4 * (p["boff"] % 4)
    return ops.gemm(a, b, p["M"], p["N"], p["K"], p["sam"], p["sak"], p["sbk"], p["sbn"], **kw)


@pytest.mark.parametrize("form", R.GEMM_FORMS)
def test_gemm_staging_paths_sizes_and_splits(ops, form):
    """M, N in {1, 63, 64, 65, 130} x K in {1, 31, 32, 33, 64, 129, 5994} in each call form of ops.linear_*, every problem in six
    memory layouts (base pointer aligned / one float off, row stride % 4 == 0 / != 0, for A and B independently): the layouts
    choose between the vector staging paths and their scalar twins (test_gemm_table_reaches_every_staging_path_and_split shows
    that all four are reached for A and for B); the LDS tile they fill is the same, so the results must be bit-identical."""
    from pytorch_kaldi_resnet_amd import hip
    for f, M, N, K in R.gemm_sweep():
        if f != form:
            continue
        assert hip.lib().spk_gemm_splitk(M, N, K) == R.gemm_splitk(M, N, K)
        first = None
        for ia, ib in R.GEMM_LAYOUT_PAIRS:
            p = R.gemm_problem(form, M, N, K, R.GEMM_LAYOUTS[ia], R.GEMM_LAYOUTS[ib])
            out = run_gemm(ops, p).cpu()
            if first is None:
                first = out
                C, b = R.gemm_ref(p["A"], p["Bm"])
                R.check("gemm", out, C, b)
            else:
                assert torch.equal(out, first), ("staging path changed the result", form, M, N, K, ia, ib)


@pytest.mark.parametrize("case", R.GEMM_EPILOGUES)
def test_gemm_alpha_bias_accumulate_and_wide_destination(ops, case):
    """alpha != 1, bias with accumulate, and `out` as a column slice of a wider tensor (ldc > N, unaligned) on the direct path
    (K = 31) and on the split-K path: everything outside the slice keeps its sentinel."""
    M, N, K, alpha, bias, acc, wide = case
    p = R.gemm_problem("NT", M, N, K, seed=7)
    bv = R.rnd(5200, N) if bias else None
    prev = R.rnd(5201, M, N) if acc else None
    C, b = R.gemm_ref(p["A"], p["Bm"], alpha, bv, prev)
    if wide:
        full = torch.full((M, N + 9), -7777.0, device="cuda")
        out = full[:, 5:5 + N]
    else:
        full = out = torch.full((M, N), -7777.0, device="cuda")
    if acc:
        out.copy_(prev)
    run_gemm(ops, p, bias=bv.cuda() if bias else None, out=out, alpha=alpha, accumulate=acc)
    R.check("gemm epilogue", out, C, b)
    if wide:
        assert out.stride(0) == N + 9
        assert bool((full[:, :5] == -7777.0).all()) and bool((full[:, 5 + N:] == -7777.0).all())


@pytest.mark.parametrize("B,S", [(6, 1211), (37, 1211), (6, 5994), (37, 5994)])
def test_gemm_head_calls(ops, B, S):
    """the cosine GEMM and its two gradient GEMMs exactly as engine.py writes them (split-K 4 / 32 / 1 at B = 6, S = 5994; the
    strided forms take the scalar paths at S % 4 = 2 and leave a 10-wide K tail), and scoring.topk_mean_std's call shape"""
    for name, a, bm, args, A, Bm in R.head_gemm_calls(B, S):
        C, b = R.gemm_ref(A, Bm)
        R.check("gemm head " + name, ops.gemm(a.cuda(), bm.cuda(), *args), C, b)
    v, c = R.rnd(5300, B, 256, scale=0.1).cuda(), R.rnd(5301, S, 256, scale=0.1).cuda()
    C, b = R.gemm_ref(v.cpu(), c.cpu().t())
    R.check("gemm scoring", ops.gemm(v, c, v.shape[0], c.shape[0], v.shape[1], v.stride(0), 1, 1, c.stride(0)), C, b)


# ---- statistics pooling -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.POOL_SHAPES + ["offset"])
@pytest.mark.parametrize("mode", [0, 1])
def test_stats_pool_fwd_bwd(ops, shape, mode):
    """`offset`: 100 + 0.01 uniform at W = 375 - the variance is 1e-8 of the mean square and the bound (pool_ref) admits the
    two-pass form only.  W = 1 in mean+std: the variance half is NaN as torch's, the sqrt(mean) half finite and checked."""
    offset = shape == "offset"
    B, H, Wd, C = R.POOL_OFFSET_SHAPE if offset else shape
    x, gout = R.pool_inputs(B, H, Wd, C, mode, offset)
    y, yb, dx, dxb = R.pool_ref(x, gout, mode)
    xg = nhwc(x)
    R.check("stats_pool_fwd", ops.stats_pool_fwd(xg, mode), y, yb)
    slot = torch.zeros(1, device="cuda", dtype=torch.int32)
    dxg = nchw(ops.stats_pool_bwd(xg, gout.cuda(), mode, amax_out=slot))
    R.check("stats_pool_bwd", dxg, dx, dxb)
    fin = dxg[torch.isfinite(dxg)]
    want = float(fin.abs().max()) if fin.numel() else 0.0
    assert float(slot.cpu().view(torch.float32)[0]) == want          # absmax hand-off: max finite |dx|, bit for bit


# ---- SGD ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hyper", R.SGD_HYPER)
@pytest.mark.parametrize("n", R.SGD_SIZES)
def test_sgd_two_steps(ops, n, hyper):
    """n < 4 is the tail alone; the largest n runs the grid-stride loop (more than 4096 blocks of 256 float4) and the tail.  Each
    step is judged against the fp64 recurrence from the float32 state the kernel itself held before that step."""
    lr, mom, wd, gs = hyper
    p0, g1, g2 = R.sgd_inputs(n)
    pad = 4
    p, buf = torch.full((n + pad,), 12345.0, device="cuda"), torch.full((n + pad,), 54321.0, device="cuda")
    p[:n].copy_(p0)
    for first, g in ((True, g1), (False, g2)):
        before, bbefore = p[:n].cpu(), buf[:n].cpu()
        pr, pb, br, bb = R.sgd_ref(before, g, bbefore, lr, mom, wd, gs, first)
        ops.sgd_step(p[:n], g.cuda(), buf[:n], lr, mom, wd, gs, first)
        R.check("sgd p", p[:n], pr, pb)
        R.check("sgd buf", buf[:n], br, bb)
    assert bool((p[n:] == 12345.0).all()) and bool((buf[n:] == 54321.0).all())      # nothing written beyond n


# ---- scoring --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.CN_SHAPES)
def test_center_normalize(ops, shape):
    for with_mean in (False, True):
        for eps in (1e-8, 1e-12):
            emb, mean = R.cn_inputs(*shape, with_mean)
            out, b = R.cn_ref(emb, mean, eps)
            got = ops.center_normalize(emb.cuda(), mean.cuda() if with_mean else None, eps)
            R.check("center_normalize", got, out, b)
            assert float(got[shape[0] // 2].abs().max()) == 0.0       # the row equal to the mean


@pytest.mark.parametrize("D", R.TC_D)
def test_trial_cosine(ops, D):
    for T in R.TC_T:
        for same in (True, False):
            en, te, ia, ib = R.tc_inputs(D, T, same)
            eg = en.cuda()
            tg = eg if same else te.cuda()
            s, b = R.tc_ref(en, te, ia, ib)
            R.check("trial_cosine", ops.trial_cosine(eg, tg, ia.cuda(), ib.cuda()), s, b)


@pytest.mark.parametrize("M", R.TOPK_M)
def test_topk_mean_std(ops, M):
    """M = 16384 is the documented limit: 64 KiB of dynamic LDS next to 16 B of static LDS in one launch"""
    full = R.topk_inputs(M).cuda()
    sc = full[:, :M]                                                 # ld = M + 3 > M; a 1e30 sentinel beyond column M
    assert sc.stride(0) == M + 3
    for k in R.topk_ks(M):
        mu, mb, sd, sb = R.topk_ref(sc.cpu(), k)
        mg, sg = ops.topk_mean_std(sc, k)
        R.check("topk mean", mg, mu, mb)
        R.check("topk std", sg, sd, sb)
        assert float(sg[1]) == 0.0 and float(mg[1]) == 0.5            # the all-equal row


def test_topk_mean_std_refuses_more_than_16384_columns(ops):
    """a host check before any launch"""
    with pytest.raises(RuntimeError):
        ops.topk_mean_std(torch.zeros(1, 16385, device="cuda"), 2)
