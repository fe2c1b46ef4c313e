"""The BatchNorm, stem and operand-scale kernels (csrc/bn.hip, csrc/stem.hip) on a real MI355X against the fp64 restatements of
tests/bn_stem_ref.py: per-element bounds derived there from the kernels' summation structure, on the engineered inputs built
there - the inputs on which tests/test_bn_stem_cpu.py shows float32 torch to stay inside those bounds - and, for every
reduction, an integer-valued case that must come out exactly.  Comparisons go through small_kernels_ref.check.
The largest error / bound per kernel is printed when the module finishes: run with `-s` to see the line
(python -m pytest tests/test_bn_stem_gpu.py -m gpu -q -s)."""
import numpy as np
import pytest
import torch

import bn_stem_ref as R
from helpers import sigma_of, slot, slot_value

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops as _ops
    yield _ops
    mine = sorted(kv for kv in R.RATIOS.items() if kv[0].startswith(("bn_", "stem_")))
    print("\nlargest error / bound per kernel: " + ", ".join("%s %.3g" % kv for kv in mine))


def bits_slot(bits):
    return torch.from_numpy(np.array([bits], dtype=np.uint32).view(np.int32).copy()).cuda()


def filled(*shape):
    return torch.full(shape, NAN, device="cuda")


# ---- 1. forward statistics: spk_bn_stats_partial + spk_bn_finalize --------------------------------------------------------
def run_stats(ops, x, gamma, beta, rm, rv, est=None):
    xg = x.cuda()
    N, C = x.shape
    part = ops.bn_stats_partial(xg)
    assert part.shape[0] == R.stats_blocks(N)
    bn4, rmg, rvg = filled(4, C), rm.cuda(), rv.cuda()
    nbt = torch.full((), 7, dtype=torch.int64, device="cuda")
    amax = ops.absmax_into(xg, slot()) if est is not None else None
    ops.bn_finalize(part, N, gamma.cuda(), beta.cuda(), rmg, rvg, nbt, bn4, amax_in=amax, est_out=est)
    assert int(nbt) == 8                                   # += 1 exactly once, however many blocks the finalize launches
    return part.double().sum(0).cpu(), bn4.cpu(), rmg.cpu(), rvg.cpu(), amax


def check_stats(tot, bn4, rmg, rvg, ref, N):
    R.check("bn_stats_partial sum", tot[:, 0], *ref["sum"])
    R.check("bn_stats_partial sumsq", tot[:, 1], *ref["sumsq"])
    for i, name in enumerate(("mean", "invstd", "scale", "shift")):
        R.check("bn_finalize " + name, bn4[i], *ref[name])
    R.check("bn_finalize running_mean", rmg, *ref["running_mean"])
    if N > 1:
        R.check("bn_finalize running_var", rvg, *ref["running_var"])
    else:                                                  # running_var at N = 1: the reference refuses the call - finite, no more
        assert bool(torch.isfinite(rvg).all())
        assert bool((bn4[1] == np.float32(R.INV_SQRT_EPS)).all()) and bool(torch.isfinite(bn4).all())


@pytest.mark.parametrize("C", R.STATS_C)
def test_bn_statistics(ops, C):
    for N in R.STATS_N:
        for off in R.STATS_OFFSETS:
            x, gamma, beta, rm, rv = R.stats_inputs(C, N, off)
            ref = R.stats_ref(x, gamma, beta, rm, rv)
            est = slot()
            tot, bn4, rmg, rvg, amax = run_stats(ops, x, gamma, beta, rm, rv, est)
            check_stats(tot, bn4, rmg, rvg, ref, N)
            assert float(bn4[1, 0]) == float(np.float32(R.INV_SQRT_EPS))         # the constant-0 channel: variance exactly 0
            # est_out: max_c |scale_c| A + |shift_c| in float32 from the kernel's own rows, an upper bound of what gets staged
            A, e = slot_value(amax), slot_value(est)
            assert A == float(x.abs().max())
            assert e == R.affine_est32(bn4[2], bn4[3], A), (C, N, off)
            assert e >= float((x.double() * bn4[2].double() + bn4[3].double()).clamp_min(0).max())
            e2 = slot_value(ops.affine_estimate(bn4[2].cuda(), bn4[3].cuda(), amax, slot()))
            assert e2 >= e
            big = bits_slot(R.f32_bits(1e30))                                    # a slot that already holds more keeps it
            run_stats(ops, x, gamma, beta, rm, rv, big)
            assert slot_value(big) == float(np.float32(1e30))
        xe, gamma, beta, rm, rv = R.stats_inputs(C, N, 0.0, exact=True)          # integer-valued: every partial sum is exact
        tot = run_stats(ops, xe, gamma, beta, rm, rv)[0]
        assert torch.equal(tot[:, 0], xe.double().sum(0)) and torch.equal(tot[:, 1], (xe.double() ** 2).sum(0)), (C, N)


def test_bn_statistics_more_than_256_rows_per_block(ops):
    C, N = R.STATS_BIG
    x, gamma, beta, rm, rv = R.stats_inputs(C, N, 3.0)
    tot, bn4, rmg, rvg, _ = run_stats(ops, x, gamma, beta, rm, rv)
    check_stats(tot, bn4, rmg, rvg, R.stats_ref(x, gamma, beta, rm, rv), N)
    xe = R.stats_inputs(C, N, 0.0, exact=True)[0]
    tot = run_stats(ops, xe, gamma, beta, rm, rv)[0]
    assert torch.equal(tot[:, 0], xe.double().sum(0)) and torch.equal(tot[:, 1], (xe.double() ** 2).sum(0))


def test_bn_statistics_limit_case(ops):
    """mean / sigma = 1000: sumsq / n - mean^2 from float32 partial sums has lost the variance; what the
    design guarantees is a finite result and an invstd in (0, 1 / sqrt(eps)]"""
    x, gamma, beta, rm, rv = R.stats_inputs(256, 1000, R.STATS_LIMIT_OFFSET)
    tot, bn4, rmg, rvg, _ = run_stats(ops, x, gamma, beta, rm, rv)
    for t in (bn4, rmg, rvg):
        assert bool(torch.isfinite(t).all())
    assert bool((bn4[1] > 0).all()) and bool((bn4[1] <= np.float32(R.INV_SQRT_EPS)).all())


def test_bn_eval_coeffs(ops):
    for C in R.STATS_C:
        x, gamma, beta, rm, rv = R.stats_inputs(C, 2, 0.0)
        ev = filled(2, C)
        ops.bn_eval_coeffs(gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), ev)
        (sc, bsc), (sh, bsh) = R.eval_coeffs_ref(gamma, beta, rm, rv)
        R.check("bn_eval_coeffs scale", ev[0], sc, bsc)
        R.check("bn_eval_coeffs shift", ev[1], sh, bsh)


# ---- 2. spk_bn_apply --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.APPLY_C)
def test_bn_apply(ops, C):
    for N in R.apply_rows(C):
        raw, sc, sh, res, rs, rh = R.apply_inputs(C, N)
        rawg, scg, shg, resg, rsg, rhg = (t.cuda() for t in (raw, sc, sh, res, rs, rh))
        for form in R.APPLY_FORMS:
            for relu in (False, True):
                use_res, use_aff = form != "plain", form == "res_affine"
                ref, b = R.apply_ref(raw, sc, sh, res if use_res else None, rs if use_aff else None, rh if use_aff else None, relu)
                sl, outg = slot(), filled(N, C)
                got = ops.bn_apply(rawg, scg, shg, res=resg if use_res else None, res_affine=(rsg, rhg) if use_aff else None,
                                   relu=relu, out=outg, mask=C % 32 == 0, amax_out=sl)
                out = outg.cpu()
                R.check("bn_apply " + form, out, ref, b)
                assert slot_value(sl) == float(out.abs().max()), (C, N, form, relu)          # the bits of max|out|
                if C % 32 == 0:
                    assert torch.equal(got[1].cpu(), R.sign_mask_words(out)), (C, N, form, relu)


def test_bn_apply_refusals(ops):
    t, out = torch.zeros(8, 2048, device="cuda"), torch.zeros(8, 2048, device="cuda")
    words = torch.zeros(8 * 64, device="cuda", dtype=torch.int32)

    def call(C, mask=None, res=None, raff=None):
        ops.call("spk_bn_apply", ops.ptr(t), ops.ptr(t), ops.ptr(t), ops.ptr(res), ops.ptr(raff), ops.ptr(raff), ops.ptr(out),
                 ops.ptr(mask), 8, C, 1, None, ops.stream())

    call(32, mask=words, res=t, raff=t)                    # the accepted form of each argument
    for kw in (dict(C=16, mask=words), dict(C=32, raff=t), dict(C=24), dict(C=2048)):
        with pytest.raises(RuntimeError, match=r"rc=-\d+\): spk_bn_apply"):
            call(**kw)
    torch.cuda.synchronize()


def test_relu_decisions_agree_on_near_ties(ops):
    """raw scale + shift within a rounding of zero: the output, its sign bit and the MASK_RAW recomputation of both backward
    kernels must take the same decision on every element (they must round the same way)"""
    raw, scale, shift, dy = R.tie_inputs()
    N, C = raw.shape
    rawg, dyg = raw.cuda(), dy.cuda()
    out, mk = ops.bn_apply(rawg, scale.cuda(), shift.cuda(), relu=True, mask=True)
    pos = out.cpu() > 0
    assert 0 < int(pos[:3].sum()) < 3 * C                  # both decisions occur among the near ties
    assert torch.equal(mk.cpu(), R.sign_mask_words(out.cpu()))
    bn4 = torch.stack([torch.zeros(C), torch.ones(C), scale, shift]).cuda()
    want = torch.where(pos, dy, torch.zeros(()))
    ones = torch.ones(C, device="cuda")
    for mode, act in ((R.MASK_RAW, None), (R.MASK_BITS, mk), (R.MASK_ACT, out)):
        part = ops.bn_bwd_partial(dyg, rawg, act, bn4, mode)
        assert torch.equal(part.double().sum(0)[:, 0].cpu(), want.double().sum(0)), mode          # the reduction's decision
        dz = filled(N, C)
        ops.bn_backward(dyg, rawg, act, bn4, ones, filled(C), filled(C), mode, dz_out=dz)
        assert torch.equal(dz.cpu(), want), mode                                                  # the apply's decision


# ---- 3. spk_bn_bwd_reduce / _finalize / _apply ------------------------------------------------------------------------------
def forward_for_backward(ops, raw, res, bn4):
    """the float32 forward whose decisions the backward differentiates: relu(bn(raw) + res) with its sign bits (C >= 32), and
    relu(bn(raw)) for MASK_RAW -> {mode: (act argument, mask on the host)}"""
    C = raw.shape[1]
    got = ops.bn_apply(raw, bn4[2], bn4[3], res=res, relu=True, mask=C >= 32)
    out, mk = got if C >= 32 else (got, None)
    plain = ops.bn_apply(raw, bn4[2], bn4[3], relu=True)
    modes = {R.MASK_NONE: (None, None), R.MASK_ACT: (out, out.cpu() > 0), R.MASK_RAW: (None, plain.cpu() > 0)}
    if mk is not None:
        assert torch.equal(mk.cpu(), R.sign_mask_words(out.cpu()))
        modes[R.MASK_BITS] = (mk, out.cpu() > 0)
    return modes


def run_backward(ops, dyg, rawg, act, bn4, gammag, mode):
    """-> dict of host tensors: partial rows, their fp64 column sums, dgamma, dbeta, coef, draw, dz, chan_amax, slot"""
    N, C = rawg.shape
    ca = torch.zeros(C, device="cuda", dtype=torch.int32)
    part = ops.bn_bwd_partial(dyg, rawg, act, bn4, mode, chan_amax=ca)
    assert part.shape[0] == R.stats_blocks(N)
    dg, db, dz, sl = filled(C), filled(C), filled(N, C), slot()
    draw = ops.bn_backward(dyg, rawg, act, bn4, gammag, dg, db, mode, dz_out=dz, amax_out=sl)
    dg2, db2 = filled(C), filled(C)
    coef = ops.bn_bwd_coef(part, N, gammag, bn4, dg2, db2)
    assert torch.equal(dg2, dg) and torch.equal(db2, db)
    return {"part": part.cpu(), "tot": part.double().sum(0).cpu(), "dgamma": dg.cpu(), "dbeta": db.cpu(), "coef": coef.cpu(),
            "draw": draw.cpu(), "dz": dz.cpu(), "chan_amax": ca.cpu().view(torch.float32), "slot": slot_value(sl)}


def check_backward(got, ref, tag=""):
    R.check("bn_bwd_reduce sum dz", got["tot"][:, 0], *ref["dbeta"])
    R.check("bn_bwd_reduce sum dz xhat", got["tot"][:, 1], *ref["dgamma"])
    R.check("bn_bwd_finalize dbeta", got["dbeta"], *ref["dbeta"])
    R.check("bn_bwd_finalize dgamma", got["dgamma"], *ref["dgamma"])
    for i, name in enumerate(("k1", "m1", "m2")):
        R.check("bn_bwd_finalize " + name, got["coef"][i], *ref[name])
    R.check("bn_bwd_apply draw", got["draw"], *ref["draw"])
    dz = ref["dz"][0]
    assert torch.equal(got["dz"].double(), dz), tag                                    # dz_out == dy mask, exactly
    assert got["slot"] == float(got["draw"].abs().max()), tag                          # amax_out: the bits of max|draw|
    assert torch.equal(got["chan_amax"].double(), dz.abs().amax(0)), tag               # per-channel max |dz|, exactly


@pytest.mark.parametrize("C", R.BWD_C)
def test_bn_backward(ops, C):
    for N in R.BWD_N:
        raw, dy, res, gamma, beta = R.bwd_inputs(C, N)
        bn4 = R.bn_rows(raw, gamma, beta).cuda()
        rawg, dyg, gammag = raw.cuda(), dy.cuda(), gamma.cuda()
        modes = forward_for_backward(ops, rawg, res.cuda(), bn4)
        assert len(modes) == (4 if C >= 32 else 3)
        got = {}
        for mode, (act, mask) in modes.items():
            ref = R.bwd_ref(dy, raw, mask, gamma)
            got[mode] = run_backward(ops, dyg, rawg, act, bn4, gammag, mode)
            check_backward(got[mode], ref, (C, N, mode))
        if C >= 32:                                         # MASK_BITS is MASK_ACT read from one bit per value: bit-identical
            for name in ("part", "draw", "dz", "dgamma", "dbeta", "coef"):
                assert torch.equal(got[R.MASK_BITS][name], got[R.MASK_ACT][name]), (C, N, name)
        # accumulate = 1: previous + new, one more rounding
        mode = R.MASK_BITS if C >= 32 else R.MASK_ACT
        act, mask = modes[mode]
        ref = R.bwd_ref(dy, raw, mask, gamma)
        pg, pb = R.rnd(350 + C, C), R.rnd(351 + C, C)
        dg, db = pg.cuda(), pb.cuda()
        ops.bn_bwd_coef(got[mode]["part"].cuda(), N, gammag, bn4, dg, db, accumulate=True)
        for name, acc, prev in (("dgamma", dg, pg), ("dbeta", db, pb)):
            want = prev.double() + ref[name][0]
            R.check("bn_bwd_finalize %s+acc" % name, acc, want, ref[name][1] + R.U * want.abs())
        # integer-valued gradient: sum dz and dbeta are exact
        dye = R.bwd_inputs(C, N, exact=True)[1]
        e = run_backward(ops, dye.cuda(), rawg, act, bn4, gammag, mode)
        want = torch.where(mask, dye, torch.zeros(())).double().sum(0)
        assert torch.equal(e["tot"][:, 0], want) and torch.equal(e["dbeta"].double(), want), (C, N)


@pytest.mark.parametrize("shape", [R.BWD_BIG_APPLY, R.BWD_BIG_REDUCE])
def test_bn_backward_beyond_the_block_caps(ops, shape):
    """(32, 65541): the grid-stride loop of bn_bwd_apply_kernel (2048 persistent blocks) with a ragged tail;
    (4, 4096 256 + 257): more than 256 rows per reduction block"""
    C, N = shape
    raw, dy, res, gamma, beta = R.bwd_inputs(C, N, exact=True)
    bn4 = R.bn_rows(raw, gamma, beta).cuda()
    rawg, dyg, gammag = raw.cuda(), dy.cuda(), gamma.cuda()
    modes = forward_for_backward(ops, rawg, res.cuda(), bn4)
    for mode in ((R.MASK_BITS, R.MASK_RAW) if C >= 32 else (R.MASK_ACT,)):
        act, mask = modes[mode]
        ref = R.bwd_ref(dy, raw, mask, gamma)
        got = run_backward(ops, dyg, rawg, act, bn4, gammag, mode)
        check_backward(got, ref, (C, N, mode))
        assert torch.equal(got["tot"][:, 0], ref["dbeta"][0]) and torch.equal(got["dbeta"].double(), ref["dbeta"][0])


@pytest.mark.parametrize("C,N", [(32, 1000), (64, 255)])
def test_bn_backward_drops_non_finite_gradients_at_masked_positions(ops, C, N):
    """the pooling layer's sqrt'(0) puts an inf into a gradient that the ReLU mask then drops (csrc/spk_common.h,
    spk_finite_abs): the masks are selects, and nothing non-finite may reach a sum, a bound or a scale slot"""
    raw, dy, res, gamma, beta = R.bwd_inputs(C, N)
    bn4 = R.bn_rows(raw, gamma, beta).cuda()
    rawg, gammag = raw.cuda(), gamma.cuda()
    modes = forward_for_backward(ops, rawg, res.cuda(), bn4)
    for mode in (R.MASK_ACT, R.MASK_RAW, R.MASK_BITS):
        act, mask = modes[mode]
        bad, zeroed = R.nonfinite_dy(dy, mask)
        assert int((~torch.isfinite(bad)).sum()) == int((~mask).sum()) > N
        a = run_backward(ops, bad.cuda(), rawg, act, bn4, gammag, mode)
        b = run_backward(ops, zeroed.cuda(), rawg, act, bn4, gammag, mode)
        for name in a:
            ta, tb = torch.as_tensor(a[name]), torch.as_tensor(b[name])
            assert bool(torch.isfinite(ta).all()) and torch.equal(ta, tb), (mode, name)
        check_backward(a, R.bwd_ref(bad, raw, mask, gamma), (C, N, mode))
        assert torch.equal(a["chan_amax"], torch.where(mask, dy, torch.zeros(())).abs().amax(0))
        fin = bad[torch.isfinite(bad)]
        assert slot_value(ops.absmax_into(bad.cuda(), slot())) == float(fin.abs().max())          # the tensor slot


def test_bn_backward_bounds(ops):
    """the rigorous operand-scale bound of the BatchNorm-backward values: the same bits from the finalize and from the
    stand-alone kernel, never below the truth; with one channel of tiny gamma and a huge gradient the per-channel form is
    tighter than the tensor-wide one, and the pair tensor written under it does not saturate"""
    for scenario in ("ordinary", "pooling"):
        if scenario == "pooling":
            raw, dy, gamma, beta = R.pooling_scenario()
        else:
            raw, dy, _, gamma, beta = R.bwd_inputs(64, 1000)
        N, C = raw.shape
        bn4 = R.bn_rows(raw, gamma, beta).cuda()
        rawg, dyg, gammag = raw.cuda(), dy.cuda(), gamma.cuda()
        mask = ops.bn_apply(rawg, bn4[2], bn4[3], relu=True).cpu() > 0
        truth = float(R.bwd_ref(dy, raw, mask, gamma)["draw"][0].abs().max())
        g_amax, raw_amax = ops.absmax_into(dyg, slot()), ops.absmax_into(rawg, slot())
        ca = torch.zeros(C, device="cuda", dtype=torch.int32)
        part = ops.bn_bwd_partial(dyg, rawg, None, bn4, R.MASK_RAW, chan_amax=ca)
        est_t, est_c = slot(), slot()
        coef = ops.bn_bwd_coef(part, N, gammag, bn4, filled(C), filled(C), amax_in=g_amax, raw_amax=raw_amax, est_out=est_t)
        est_k = ops.bnbwd_estimate(coef, bn4, g_amax, raw_amax)
        assert int(est_k.cpu()) == int(est_t.cpu())
        ops.bn_bwd_coef(part, N, gammag, bn4, filled(C), filled(C), amax_in=g_amax, raw_amax=raw_amax, est_out=est_c, chan_amax=ca)
        tensor_wide, per_channel = slot_value(est_t), slot_value(est_c)
        print("%s: truth %.4g, per-channel bound %.4g, tensor-wide bound %.4g" % (scenario, truth, per_channel, tensor_wide))
        assert truth <= per_channel <= tensor_wide
        if scenario == "pooling":
            assert per_channel < 1e-3 * tensor_wide         # the coupling of channels the per-channel form removes
        est_p = slot()
        ca2 = torch.zeros(C, device="cuda", dtype=torch.int32)
        draw_p = ops.bn_backward(dyg, rawg, None, bn4, gammag, filled(C), filled(C), R.MASK_RAW, pair=(g_amax, raw_amax, est_p),
                                 chan_amax=ca2)
        assert int(est_p.cpu()) == int(est_c.cpu())
        cnt = torch.zeros(4, device="cuda", dtype=torch.int64)
        ops.f16_window_count(draw_p, est_p, cnt, pairs=True)
        assert int(cnt[0]) == N * C and int(cnt[1]) == 0, cnt.tolist()
        draw_f = ops.bn_backward(dyg, rawg, None, bn4, gammag, filled(C), filled(C), R.MASK_RAW)
        assert torch.equal(draw_p.cpu().view(torch.int32), R.encode_pairs(draw_f.cpu(), sigma_of(est_p)).view(torch.int32))


# ---- 4. hand-off helpers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ABSMAX_N)
def test_absmax(ops, n):
    for name, x, want in R.absmax_cases(n):
        xg = x.cuda()
        assert xg.data_ptr() % 16 == 0
        assert slot_value(ops.absmax_into(xg, slot())) == want, (n, name)
        prior = bits_slot(R.f32_bits(1e9))                  # a larger prior value is kept
        assert slot_value(ops.absmax_into(xg, prior)) == 1e9
    wide = torch.zeros(n + 1, device="cuda")
    with pytest.raises(RuntimeError, match="16-byte aligned"):      # a pointer off by one float
        ops.absmax_into(wide[1:], slot())


@pytest.mark.parametrize("n", [R.ABSMAX_BIG, R.ABSMAX_LOOP])
def test_absmax_at_and_beyond_the_block_cap(ops, n):
    """8192 blocks x 256 float4 and the scalar tail: with ABSMAX_BIG every thread makes exactly one trip, with ABSMAX_LOOP the
    last float4 is read by the second trip of thread 0 of block 0 and by nothing else"""
    nq = n >> 2
    assert (nq > R.absmax_blocks(n) * 256) == (n == R.ABSMAX_LOOP)
    x = torch.full((n,), 0.5, device="cuda")
    assert slot_value(ops.absmax_into(x, slot())) == 0.5
    x[4 * (nq - 1) + 1] = -2.0                              # the last float4
    assert slot_value(ops.absmax_into(x, slot())) == 2.0
    x[5] = float("inf")
    x[n - 1] = 3.0                                          # the scalar tail (n % 4 = 3)
    assert slot_value(ops.absmax_into(x, slot())) == 3.0


def window_counts(ops, x, sl, **kw):
    cnt = torch.zeros(4, device="cuda", dtype=torch.int64)
    ops.f16_window_count(x, sl, cnt, **kw)
    return cnt.tolist()


@pytest.mark.parametrize("bits", R.SIGMA_SLOTS)
def test_sigma_and_window_counter(ops, bits):
    """spk_sigma_from_amax_bits observed through spk_f16_window_count: the inputs sit on the saturation and subnormal boundaries
    of the sigma the host restatement expects, so another sigma gives other counts"""
    sl = bits_slot(bits)
    sig = R.sigma_from_bits(bits)
    assert sigma_of(sl) == sig
    x = R.window_values(sig).reshape(-1, 4)
    assert window_counts(ops, x.cuda(), sl) == R.window_count_ref(x, sig), hex(bits)
    pairs = R.encode_pairs(x, sig)
    assert window_counts(ops, pairs.cuda(), sl, pairs=True) == R.window_count_ref(pairs, sig, pairs=True), hex(bits)
    if 2.0 ** -20 <= sig <= 2.0 ** 20:                      # the affine form: relu(x scale + shift), exact by construction
        scale, shift = torch.tensor([1.0, 2.0, 0.5, -1.0]), torch.zeros(4)
        assert window_counts(ops, x.cuda(), sl, affine=(scale.cuda(), shift.cuda())) == R.window_count_ref(x, sig, scale, shift)


def test_window_counter_boundaries(ops):
    """the counts themselves at sigma = 2^14 (slot 1.0), spelled out"""
    sl, sig = bits_slot(0x3F800000), 2.0 ** 14
    v = torch.tensor([65504.0, 65504.0, 0.0, 0.0]) / sig
    assert window_counts(ops, v.view(1, 4).cuda(), sl) == [4, 0, 0, 0]                       # exactly 65504 / sigma: no saturation
    v[1] = float(np.nextafter(np.float32(65504.0 / sig), np.float32(np.inf)))
    assert window_counts(ops, v.view(1, 4).cuda(), sl) == [4, 1, 0, 0]                       # the next float: one
    # ... as a pair tensor the stored high terms are +65504 twice: both count as saturated
    assert window_counts(ops, R.encode_pairs(v.view(1, 4), sig).cuda(), sl, pairs=True) == [4, 2, 0, 0]
    v = torch.tensor([2.0 ** -14, 2.0 ** -14 - 2.0 ** -24, 1.0 + 2.0 ** -14, 1.0 + 2.0 ** -14 - 2.0 ** -23]) / sig
    assert window_counts(ops, v.view(1, 4).cuda(), sl) == [4, 0, 1, 1]
    assert window_counts(ops, torch.zeros(2, 4).cuda(), sl) == [8, 0, 0, 0]


# ---- 5. stem ----------------------------------------------------------------------------------------------------------------
def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


@pytest.mark.parametrize("shape", R.STEM_SHAPES)
def test_stem(ops, shape):
    B, Fd, T = shape
    NP = B * Fd * T
    x, w, esc, esh, dy, prev = R.stem_inputs(*shape)
    xg, wg = x.cuda(), w.cuda()
    v, bv = R.stem_ref(x, w)
    sl = slot()
    out, st = ops.stem_fwd(xg, wg, stats=True, amax_out=sl)
    assert st.shape[0] == min(-(-NP // 64), 2048)
    R.check("stem_fwd", out, v, bv)
    assert slot_value(sl) == float(out.abs().max())
    (s1, b1), (s2, b2) = R.stem_stats_ref(v, bv)
    tot = st.double().sum(0).cpu()
    R.check("stem_fwd stats sum", tot[:, 0], s1, b1)
    R.check("stem_fwd stats sumsq", tot[:, 1], s2, b2)
    v2, bv2 = R.stem_ref(x, w, esc, esh, relu=True)
    sl2 = slot()
    out2, _ = ops.stem_fwd(xg, wg, epi_affine=(esc.cuda(), esh.cuda()), relu=True, amax_out=sl2)
    R.check("stem_fwd epilogue", out2, v2, bv2)
    assert slot_value(sl2) == float(out2.abs().max())
    # length-masked form: NaN in the padding, statistics over the valid frames, +0 beyond them
    lens = R.stem_lengths(B, T)
    xn = x.clone()
    for b in range(B):
        xn[b, :, int(lens[b]):] = NAN
    vm, bm = R.stem_ref(xn, w, lens=lens)
    sl3 = slot()
    out3, st3 = ops.stem_fwd(xn.cuda(), wg, stats=True, amax_out=sl3, wlen=lens.cuda())
    R.check("stem_fwd_len", out3, vm, bm)
    for b in range(B):
        assert int(out3[b, :, int(lens[b]):].contiguous().view(torch.int32).abs().max() if int(lens[b]) < T else 0) == 0      # +0
    assert slot_value(sl3) == float(out3.abs().max())
    (s1, b1), (s2, b2) = R.stem_stats_ref(vm, bm)
    tot = st3.double().sum(0).cpu()
    R.check("stem_fwd_len stats sum", tot[:, 0], s1, b1)
    R.check("stem_fwd_len stats sumsq", tot[:, 1], s2, b2)
    # weight gradient, and accumulate = 1 onto a previous dw
    dyg = nhwc(dy)
    dw = filled(32, 1, 3, 3)
    ops.stem_wgrad(xg, dyg, dw)
    R.check("stem_wgrad", dw, *R.stem_wgrad_ref(x, dy))
    acc = prev.cuda()
    ops.stem_wgrad(xg, dyg, acc, accumulate=True)
    R.check("stem_wgrad+acc", acc, *R.stem_wgrad_ref(x, dy, prev))
    # integer-valued x, w, dy: outputs, per-block statistics and the weight gradient are exact
    xe, we, _, _, dye, _ = R.stem_inputs(*shape, exact=True)
    ve, _ = R.stem_ref(xe, we)
    oute, ste = ops.stem_fwd(xe.cuda(), we.cuda(), stats=True)
    assert torch.equal(oute.cpu().double(), ve)
    tot = ste.double().sum(0).cpu()
    assert torch.equal(tot[:, 0], ve.reshape(-1, 32).sum(0)) and torch.equal(tot[:, 1], (ve * ve).reshape(-1, 32).sum(0))
    dwe = filled(32, 1, 3, 3)
    ops.stem_wgrad(xe.cuda(), nhwc(dye), dwe)
    assert torch.equal(dwe.cpu().double(), R.stem_wgrad_ref(xe, dye)[0])
