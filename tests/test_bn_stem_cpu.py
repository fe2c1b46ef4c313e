"""Pins tests/bn_stem_ref.py without the code it will judge (no GPU, no library):
  * float32 torch on the CPU - F.batch_norm in training and in eval mode, F.conv2d, autograd - stays inside every bound on
    every engineered input that tests/test_bn_stem_gpu.py feeds the kernels, so a correct implementation passes each of those
    tests and no bound is too tight;
  * the fp64 restatements agree with fp64 autograd;
  * the host restatements of the launch geometry, of the operand scale and of the fp16 window counter are checked against
    hand-computed values."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_stem_ref as R
import helpers


def close64(a, b, rel=1e-10):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert float((a - b).abs().max()) <= rel * float(b.abs().max()) + 1e-300, float((a - b).abs().max())


# ---- geometry ---------------------------------------------------------------------------------------------------------------
def test_reduction_geometry():
    """the shapes of the issue reach what they are there for"""
    C, N = R.STATS_BIG
    nb, rpb = R.stats_blocks(N), R.rows_per_block(N)
    assert (nb, rpb) == (4096, 257)                      # 4081 full blocks, one of 16 rows, 14 blocks without a row
    last = N // rpb
    assert last == 4081 and 0 < N - last * rpb < rpb and (last + 1) * rpb >= N and last + 1 < nb
    assert R.bn_chain(N, 4) == 2 + 256 + 1 and R.bn_chain(1000, 1024) == 250 + 1 + 1 and R.bn_chain(1, 4) == 1 + 256 + 1
    assert R.stats_blocks(1000) == 4                     # C = 1024: 32 finalize blocks, 4 partial rows
    C, N = R.BWD_BIG_APPLY
    assert N * C // 4 > 2048 * 256 and (N * C // 4) % 256 != 0
    # spk_absmax: both lengths hit the cap of 8192 blocks and have a scalar tail; only ABSMAX_LOOP makes a thread loop
    for n, loops in ((R.ABSMAX_BIG, False), (R.ABSMAX_LOOP, True)):
        assert R.absmax_blocks(n) == 8192 and n % 4 == 3 and n * 4 < 34e6
        assert ((n >> 2) > R.absmax_blocks(n) * 256) == loops
    assert R.absmax_blocks(1) == 1 and R.absmax_blocks(1025) == 2
    B, Fd, T = R.STEM_SHAPES[-1]
    assert B * Fd * T > 2048 * 64 and R.stem_chain(B * Fd * T, 2048) == 2 + 8 and R.stem_chain(B * Fd * T, 1024) == 3 + 8
    for C in R.APPLY_C:                                  # one, two and three groups past the end of the four per thread
        past = set()
        for N in R.apply_rows(C):
            nq = N * C // 4
            stride = -(-nq // 1024) * 256
            past |= {sum(i0 + stride * u >= nq for u in range(4)) for i0 in range(min(stride, nq))}
        assert past == {0, 1, 2, 3}, (C, past)


# ---- 1. forward statistics ------------------------------------------------------------------------------------------------
def torch_stats(x, gamma, beta, rm, rv):
    rm, rv = rm.clone(), rv.clone()
    out, mean, inv = torch.native_batch_norm(x, gamma, beta, rm, rv, True, 0.1, 1e-5)
    return out, mean, inv, rm, rv


@pytest.mark.parametrize("C", R.STATS_C)
def test_torch_batch_norm_statistics_are_inside_the_bounds(C):
    for N in R.STATS_N:
        for off in R.STATS_OFFSETS:
            x, gamma, beta, rm, rv = R.stats_inputs(C, N, off)
            ref = R.stats_ref(x, gamma, beta, rm, rv)
            if N == 1:
                with pytest.raises(ValueError):          # the reference refuses one value per channel
                    F.batch_norm(x, rm.clone(), rv.clone(), gamma, beta, True, 0.1, 1e-5)
                assert bool((ref["invstd"][0].float() == np.float32(R.INV_SQRT_EPS)).all())
                continue
            out, mean, inv, rmn, rvn = torch_stats(x, gamma, beta, rm, rv)
            R.check("torch mean", mean, *ref["mean"])
            R.check("torch invstd", inv, *ref["invstd"])
            R.check("torch running_mean", rmn, *ref["running_mean"])
            R.check("torch running_var", rvn, *ref["running_var"])
            sc = gamma * inv
            R.check("torch scale", sc, *ref["scale"])
            R.check("torch shift", beta - mean * sc, *ref["shift"])
            (s, bs), (h, bh) = ref["scale"], ref["shift"]
            by = R.apply_ref(x, s.float(), h.float())[1]          # the output through the chain: coefficient errors + the apply
            R.check("torch batch_norm train", out, x.double() * s + h, x.double().abs() * (bs + R.U * s.abs()) + bh + R.U * h.abs() + by)
            assert float(ref["var"][0][0]) == 0.0 and float(ref["var"][0][1]) < 1e-15      # the constant channels
            assert abs(float(ref["var"][0][2]) - 25.0 * (N - 1) / N ** 2) < 1e-12            # one value among zeros


def test_torch_batch_norm_statistics_big_and_limit():
    C, N = R.STATS_BIG
    x, gamma, beta, rm, rv = R.stats_inputs(C, N, 3.0)
    ref = R.stats_ref(x, gamma, beta, rm, rv)
    # F.batch_norm adds the million rows of a channel one after the other in float32 (its mean of the constant 0.1 is off by
    # 1e-3 relative): a chain of N, where the bound describes per-block float32 sums of 257 rows folded in fp64.  The float32
    # implementation shown to be inside the bound is therefore torch's float32 sum per block of rows_per_block rows.
    nb, rpb = R.stats_blocks(N), R.rows_per_block(N)
    xp = torch.cat([x, torch.zeros(nb * rpb - N, C)]).reshape(nb, rpb, C)
    s1, s2 = xp.sum(1).double().sum(0), (xp * xp).sum(1).double().sum(0)
    R.check("blocked sum", s1, *ref["sum"])
    R.check("blocked sumsq", s2, *ref["sumsq"])
    mean = s1 / N
    var = (s2 / N - mean * mean).clamp_min(0.0)
    R.check("blocked mean", mean.float(), *ref["mean"])
    R.check("blocked var", var, *ref["var"])
    R.check("blocked invstd", (1.0 / torch.sqrt(var + R.EPS)).float(), *ref["invstd"])
    xe = R.stats_inputs(C, N, 0.0, exact=True)[0]
    assert torch.equal(xe.sum(0).double(), xe.double().sum(0))               # the exact case is exact in float32
    # the limit case: the bound of the variance reaches the variance; the interval image stays finite and positive
    x, gamma, beta, rm, rv = R.stats_inputs(256, 1000, R.STATS_LIMIT_OFFSET)
    ref = R.stats_ref(x, gamma, beta, rm, rv)
    var, bvar = ref["var"]
    inv, binv = ref["invstd"]
    assert float((bvar[3:] / var[3:]).max()) > 0.5
    assert bool(torch.isfinite(binv).all()) and bool((binv > 0).all()) and bool((inv <= 1.0 / np.sqrt(R.EPS)).all())


def test_torch_batch_norm_eval_is_inside_the_bounds():
    for C in R.STATS_C:
        x, gamma, beta, rm, rv = R.stats_inputs(C, 257, 3.0)
        (sc, bsc), (sh, bsh) = R.eval_coeffs_ref(gamma, beta, rm, rv)
        by = R.apply_ref(x, sc.float(), sh.float())[1]
        got = F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, 1e-5)
        R.check("torch batch_norm eval", got, x.double() * sc + sh, x.double().abs() * (bsc + R.U * sc.abs()) + bsh + R.U * sh.abs() + by)
        inv32 = 1.0 / torch.sqrt(rv + np.float32(1e-5))
        R.check("torch eval scale", gamma * inv32, sc, bsc)
        R.check("torch eval shift", beta - rm * (gamma * inv32), sh, bsh)


def test_affine_estimate_restatement():
    assert float(R.fma32(np.float32(3.0), np.float32(1.0 / 3.0), np.float32(-1.0))) == 2.0 ** -25          # one rounding
    assert float(np.float32(3.0) * np.float32(1.0 / 3.0) + np.float32(-1.0)) == 0.0                         # two
    sc, sh = R.rnd(1, 64, scale=2.0), R.rnd(2, 64)
    e = R.affine_est32(sc, sh, 3.7)
    exact = float((sc.double().abs() * float(np.float32(3.7)) + sh.double().abs()).max())
    assert abs(e - exact) <= R.U * exact


# ---- 2. bn_apply ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.APPLY_C)
def test_torch_affine_is_inside_the_apply_bounds(C):
    for N in R.apply_rows(C):
        raw, sc, sh, res, rs, rh = R.apply_inputs(C, N)
        for form in R.APPLY_FORMS:
            for relu in (False, True):
                v = raw * sc + sh
                if form == "res":
                    v = v + res
                elif form == "res_affine":
                    v = v + (res * rs + rh)
                ref, b = R.apply_ref(raw, sc, sh, res if form != "plain" else None, rs if form == "res_affine" else None,
                                     rh if form == "res_affine" else None, relu)
                R.check("torch affine " + form, torch.relu(v) if relu else v, ref, b)


def test_sign_mask_words_and_ties():
    out = torch.zeros(2, 64)
    out[0, 0] = 1.0
    out[0, 31] = 2.0
    out[1, 33] = 1e-45
    out[1, 40] = -1.0
    assert R.sign_mask_words(out).tolist() == [1 + (1 << 31) - (1 << 32), 0, 0, 2]
    raw, scale, shift, dy = R.tie_inputs()
    sep = raw * scale + shift
    fused = torch.tensor([[float(R.fma32(r, s, -1.0)) for r, s in zip(row, scale.tolist())] for row in raw.tolist()])
    assert int(((sep > 0) != (fused > 0)).sum()) >= 8          # the two arithmetics decide differently on these inputs
    assert bool((dy != 0).all())


# ---- 3. BatchNorm backward ------------------------------------------------------------------------------------------------
def autograd_bwd(raw, dy, res, gamma, beta, mode, dtype):
    x = raw.to(dtype).requires_grad_(True)
    g, b = gamma.to(dtype).requires_grad_(True), beta.to(dtype).requires_grad_(True)
    y = F.batch_norm(x, None, None, g, b, True, 0.1, R.EPS)          # (the float32 eps in both precisions)
    if mode in (R.MASK_ACT, R.MASK_BITS):
        y = F.relu(y + res.to(dtype))
    elif mode == R.MASK_RAW:
        y = F.relu(y)
    gx, gg, gb = torch.autograd.grad(y, [x, g, b], grad_outputs=dy.to(dtype))
    mask = None if mode == R.MASK_NONE else (y.detach() > 0)
    return gx, gg, gb, mask


@pytest.mark.parametrize("C", R.BWD_C)
def test_backward_restatement_is_fp64_autograd_and_float32_autograd_is_inside_the_bounds(C):
    for N in R.BWD_N[1:] + [2]:                             # (the reference refuses N = 1)
        raw, dy, res, gamma, beta = R.bwd_inputs(C, N)
        for mode in (R.MASK_NONE, R.MASK_ACT, R.MASK_RAW):
            gx, gg, gb, mask = autograd_bwd(raw, dy, res, gamma, beta, mode, torch.float64)
            ref = R.bwd_ref(dy, raw, mask, gamma)
            close64(ref["draw"][0], gx, 1e-9)
            close64(ref["dgamma"][0], gg, 1e-9)
            close64(ref["dbeta"][0], gb, 1e-9)
            gx, gg, gb, mask = autograd_bwd(raw, dy, res, gamma, beta, mode, torch.float32)
            ref = R.bwd_ref(dy, raw, mask, gamma)          # the float32 forward's own decision
            R.check("torch draw", gx, *ref["draw"])
            R.check("torch dgamma", gg, *ref["dgamma"])
            R.check("torch dbeta", gb, *ref["dbeta"])


def test_backward_float32_closed_form_on_the_rounded_rows_is_inside_the_bounds():
    """the arithmetic of the kernels, written with float32 torch operations on the float32 rows of bn_rows"""
    for C, N in ((32, 1000), (4, 255), (1024, 1), R.BWD_BIG_APPLY):
        raw, dy, res, gamma, beta = R.bwd_inputs(C, N)
        bn4 = R.bn_rows(raw, gamma, beta)
        mask = (raw * bn4[2] + bn4[3] + res) > 0
        ref = R.bwd_ref(dy, raw, mask, gamma)
        dz = torch.where(mask, dy, torch.zeros(()))
        xh = (raw - bn4[0]) * bn4[1]
        dbeta, dgamma = dz.sum(0), (dz * xh).sum(0)
        k1, m1, m2 = gamma * bn4[1], dbeta / N, dgamma / N
        R.check("f32 dbeta", dbeta, *ref["dbeta"])
        R.check("f32 dgamma", dgamma, *ref["dgamma"])
        R.check("f32 k1", k1, *ref["k1"])
        R.check("f32 m1", m1, *ref["m1"])
        R.check("f32 m2", m2, *ref["m2"])
        R.check("f32 draw", k1 * (dz - m1 - xh * m2), *ref["draw"])
    raw, dy, res, gamma, beta = R.bwd_inputs(32, 1000, exact=True)
    mask = res > 0
    ref = R.bwd_ref(dy, raw, mask, gamma)
    assert torch.equal(torch.where(mask, dy, torch.zeros(())).sum(0).double(), ref["dbeta"][0])      # exact in float32


def test_masks_are_selects():
    """an inf / NaN gradient at a masked-off position (the pooling layer's sqrt'(0)) must not reach any sum: the restatement
    selects, and a product with the mask would not do"""
    raw, dy, res, gamma, beta = R.bwd_inputs(32, 255)
    mask = res > 0
    bad, zeroed = R.nonfinite_dy(dy, mask)
    assert int(torch.isinf(bad).sum()) > 100 and int(torch.isnan(bad).sum()) > 100
    a, b = R.bwd_ref(bad, raw, mask, gamma), R.bwd_ref(zeroed, raw, mask, gamma)
    for name in a:
        assert torch.equal(a[name][0], b[name][0]) and bool(torch.isfinite(a[name][0]).all()), name
    assert not bool(torch.isfinite((bad * mask).sum(0)).all())
    raw, dy, gamma, beta = R.pooling_scenario()
    assert float(dy[:, 5].abs().max()) > 1e5 and float(gamma[5]) == float(np.float32(1e-6))


# ---- 4. hand-off helpers ----------------------------------------------------------------------------------------------------
def test_absmax_cases():
    for n in R.ABSMAX_N:
        for name, x, want in R.absmax_cases(n):
            assert x.shape == (n,)
            fin = x[torch.isfinite(x)]
            assert float(fin.abs().max()) == want, (n, name)
            if name == "nonfinite" and n >= 4:
                assert int(torch.isinf(x).sum()) >= 1 and int(torch.isnan(x).sum()) == 1


def test_sigma_restatements():
    """helpers.sigma_of carries the device function's exponent clamp"""
    for bits in R.SIGMA_SLOTS:
        slot = torch.from_numpy(np.array([bits], dtype=np.uint32).view(np.int32).copy())
        assert helpers.sigma_of(slot) == R.sigma_from_bits(bits), hex(bits)
    assert R.sigma_from_bits(0x3F800000) == 2.0 ** 14 and R.sigma_from_bits(0x407FFFFF) == 2.0 ** 13
    assert R.sigma_from_bits(0x40800000) == 2.0 ** 12 and R.sigma_from_bits(0x7F7FFFFF) == 2.0 ** -113
    assert R.sigma_from_bits(R.f32_bits(2.0 ** -120)) == 2.0 ** 127 == R.sigma_from_bits(R.f32_bits(2.0 ** -113))
    for bits in (0, 1, 0x007FFFFF, 0x7F800000, 0x7FC00000):
        assert R.sigma_from_bits(bits) == 1.0


def test_window_counter_restatement():
    sig = 2.0 ** 14
    x = R.window_values(sig)
    assert x.numel() % 4 == 0 and x.numel() >= 32
    n, sat, lo_sub, hi_sub = R.window_count_ref(x, sig)
    # +-(65504 / sig) does not saturate, the next float does; +-2^-14 / sig has a normal high term and so has the float32 below
    # it (it rounds up to 2^-14 as an fp16), 2^-14 - 2^-24 and 3 2^-20 have a subnormal one, 2^-25 rounds to zero; the low term
    # is subnormal for +-(1 + 2^-14 - 2^-23) / sig only
    assert (n, sat, lo_sub, hi_sub) == (x.numel(), 2, 2, 4), (n, sat, lo_sub, hi_sub)
    pairs = R.encode_pairs(x.reshape(-1, 4), sig)
    np_, satp, lop, hip = R.window_count_ref(pairs, sig, pairs=True)
    # the pair form reads saturation from the stored high term: +-65504 itself, the clamped next float and 65490 -> 65504 count
    assert (np_, lop, hip) == (n, lo_sub, hi_sub) and satp == 6
    for bits in R.SIGMA_SLOTS:
        s = R.sigma_from_bits(bits)
        v = R.window_values(s)
        assert bool(torch.isfinite(v).all()) and v.numel() >= 8
        assert bool((((v.double() * s).float().double()) == v.double() * s).all())          # v sigma is exact


# ---- 5. stem ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.STEM_SHAPES)
def test_torch_stem_is_inside_the_bounds(shape):
    B, Fd, T = shape
    x, w, esc, esh, dy, prev = R.stem_inputs(*shape)
    v, bv = R.stem_ref(x, w)
    out = F.conv2d(x[:, None], w, None, 1, 1)
    R.check("torch stem", out.permute(0, 2, 3, 1), v, bv)
    v2, bv2 = R.stem_ref(x, w, esc, esh, relu=True)
    R.check("torch stem epilogue", F.relu(out * esc.view(1, -1, 1, 1) + esh.view(1, -1, 1, 1)).permute(0, 2, 3, 1), v2, bv2)
    (s1, b1), (s2, b2) = R.stem_stats_ref(v, bv)
    o2 = out.permute(0, 2, 3, 1).reshape(-1, 32)
    R.check("torch stem sum", o2.sum(0), s1, b1)
    R.check("torch stem sumsq", (o2 * o2).sum(0), s2, b2)
    # weight gradient: restatement = fp64 autograd, float32 autograd inside the bound
    dw, bdw = R.stem_wgrad_ref(x, dy)
    wd = w.double().requires_grad_(True)
    g64, = torch.autograd.grad(F.conv2d(x.double()[:, None], wd, None, 1, 1), [wd], grad_outputs=dy.double())
    close64(dw, g64, 1e-12)
    wf = w.clone().requires_grad_(True)
    g32, = torch.autograd.grad(F.conv2d(x[:, None], wf, None, 1, 1), [wf], grad_outputs=dy)
    R.check("torch stem wgrad", g32, dw, bdw)
    dwa, bdwa = R.stem_wgrad_ref(x, dy, prev)
    R.check("torch stem wgrad+acc", prev + g32, dwa, bdwa)
    # length-masked form: the padding may hold anything
    lens = R.stem_lengths(B, T)
    xn = x.clone()
    for b in range(B):
        xn[b, :, int(lens[b]):] = float("nan")
    vm, bm = R.stem_ref(xn, w, lens=lens)
    assert bool(torch.isfinite(vm).all())
    for b in range(B):
        assert float(vm[b, :, int(lens[b]):].abs().max() if int(lens[b]) < T else 0.0) == 0.0
    # integer-exact case: float32 is exact
    xe, we, _, _, dye, _ = R.stem_inputs(*shape, exact=True)
    ve, _ = R.stem_ref(xe, we)
    assert torch.equal(F.conv2d(xe[:, None], we, None, 1, 1).permute(0, 2, 3, 1).double(), ve)
    assert float(ve.abs().max()) <= 81.0 and float(R.stem_wgrad_ref(xe, dye)[0].abs().max()) < 2.0 ** 24
