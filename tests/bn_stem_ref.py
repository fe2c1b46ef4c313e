"""fp64 restatements, engineered inputs and per-element error bounds for the kernels inside the trunk that are not matrix
kernels (csrc/bn.hip, csrc/stem.hip) - test infrastructure only.

tests/test_bn_stem_cpu.py shows that float32 torch on the CPU stays inside every bound on every input below and that the
restatements agree with fp64 autograd; tests/test_bn_stem_gpu.py runs the kernels on the same inputs against the same bounds.

The rules are those of tests/small_kernels_ref.py (whose check / rnd / uni / U / RATIOS are used here):
  * float32 decisions, fp64 values: a ReLU mask is what the float32 forward decided - `out > 0` of the forward output the
    caller hands in - never a recomputation in fp64;
  * per-element bounds from the summation structure of the kernel source: with u = 2^-24,
    bound = (roundings + 1) u sum|terms|; nothing is fitted to what a kernel returns.
Those worst-case bounds are loose against random rounding (a few hundred roundings are allowed where a handful happen), so
every reduction also has an EXACT case: small-integer inputs (-3 ... 3) make every float32 partial sum exact and the
comparison is `==` - that is what catches a dropped or doubled row.
"""
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

from helpers import encode_pairs      # noqa: F401  (re-exported)
from oracle import weights as W
from small_kernels_ref import F32, RATIOS, U, check, rnd, uni      # noqa: F401  (re-exported to the two test files)

EPS = float(F32(1e-5))                      # the float32 eps the library passes, as every kernel widens it
MOM = float(F32(0.1))
INV_SQRT_EPS = float(F32(1.0 / math.sqrt(EPS)))      # invstd of a channel without variance, to float32
MASK_NONE, MASK_ACT, MASK_RAW, MASK_BITS = 0, 1, 2, 3


def small_ints(seed, *shape):
    """seeded float32 tensor of integers in -3 ... 3"""
    n = int(np.prod(shape))
    return torch.from_numpy((np.minimum(np.floor(W.hash_uniform(seed, 4, n) * 7), 6) - 3).astype(np.float32).reshape(shape))


def f32_bits(v):
    """bit pattern of float32(v) as a Python int"""
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def bits_f32(bits):
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


def fma32(a, b, c):
    """float32(a b + c) with ONE rounding (v_fma_f32), exact rational arithmetic on the float32 inputs"""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    r = np.float32(float(exact))
    cands = [r, np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), f32_bits(v) & 1))


# ---- launch geometry of the two-level reductions (bn_stats_partial_kernel, bn_bwd_reduce_kernel) ---------------------------
def stats_blocks(N):
    """host restatement of spk_bn_stats_blocks"""
    return max(1, min(-(-N // 256), 4096))


def rows_per_block(N):
    return -(-N // stats_blocks(N))


def bn_chain(N, C):
    """roundings on the way of one value into a per-block float32 partial sum: a thread owns one float4 of channels and walks
    rows r0 + prow, + rstep, ... of its block (rstep = 1024 / C rows are in flight per block): ceil(rows_per_block / rstep)
    additions; thread `quad` then folds the rstep LDS rows of its channels one after the other: rstep additions; the products
    x x and dz xhat carry one rounding of their own (fused or not).  The blocks are folded in fp64 (2^-53: nothing)."""
    rstep = 1024 // C
    return -(-rows_per_block(N) // rstep) + rstep + 1


# ---- 1. forward statistics --------------------------------------------------------------------------------------------------
STATS_C = [4, 8, 32, 256, 1024]
STATS_N = [1, 2, 255, 257, 1000]
STATS_OFFSETS = [0.0, 3.0, 30.0]            # mean / sigma
STATS_LIMIT_OFFSET = 1000.0
STATS_BIG = (4, 4096 * 256 + 257)           # rows_per_block = 257 > 256, ragged last block, 16 MB


def stats_inputs(C, N, offset, exact=False):
    """x [N][C], gamma, beta, running_mean, running_var.  Channel c has sigma_c in [0.5, 2) and mean = offset sigma_c;
    channel 0 is the constant 0, channel 1 the constant 0.1, channel 2 one nonzero value among zeros.
    exact: integers in -3 ... 3 instead (every float32 partial sum of x and of x^2 is exact)."""
    if exact:
        x = small_ints(120 + C + N % 1000, N, C)
    else:
        sig = (0.5 + 1.5 * uni(100 + C, C)).double()
        x = ((rnd(110 + C + N % 1000, N, C).double() * math.sqrt(3.0) + offset) * sig).float()
        x[:, 0] = 0.0
        x[:, 1] = 0.1
        x[:, 2] = 0.0
        x[N // 2, 2] = 5.0
    return (x, rnd(130 + C, C, scale=0.3, shift=1.0), rnd(131 + C, C, scale=0.2), rnd(132 + C, C, scale=0.1),
            rnd(133 + C, C, scale=0.2, shift=1.0))


def invstd_interval(var, bvar):
    """1 / sqrt(v + eps) and the image of [var - bvar, var + bvar] under v -> 1 / sqrt(max(v, 0) + eps), plus 2 u relative (the
    fp64 value is rounded to float32 once; u more for the float32 rsqrt of an implementation that works in float32) of the
    largest value in the interval.  Valid also when bvar reaches var itself (constant channels, the limit case)."""
    inv = 1.0 / torch.sqrt(var + EPS)
    lo = 1.0 / torch.sqrt(var + bvar + EPS)
    hi = 1.0 / torch.sqrt((var - bvar).clamp_min(0.0) + EPS)
    return inv, torch.maximum(hi - inv, inv - lo) + 2 * U * hi


def stats_ref(x, gamma, beta, rm, rv):
    """-> {name: (fp64 value, bound)} for sum / sumsq (the column sums of the partial rows), mean, var, invstd, scale, shift,
    running_mean, running_var (unbiased, momentum 0.1) of nn.BatchNorm in training mode.

    k = (bn_chain + 1) u.  Bounds:
      sum, sumsq    k sum|x|,  k sum x^2
      mean          k sum|x| / n + u |mean|                       (the fp64 quotient is stored as float32)
      var           absolute: [k sum x^2 + 2 |mean| k sum|x|] / n   (sumsq / n - mean^2: the second term is the conditioning -
                    relative to the variance it is k (1 + mean^2 / sigma^2) and no better)
      invstd        invstd_interval
      scale         |gamma| b_invstd + u |scale|                  (one float32 product)
      shift         |mean| b_scale + |scale| b_mean + u (|beta| + 2 |mean scale|)     (product and difference, fused or not)
      running_*     5 u (|(1 - m) old| + |m new|) + m b_new       (1 - m, two products, one sum: 4 roundings)"""
    N, C = x.shape
    xd = x.double()
    k = (bn_chain(N, C) + 1) * U
    s1, a1, s2 = xd.sum(0), xd.abs().sum(0), (xd * xd).sum(0)
    mean = s1 / N
    var = ((xd - mean) ** 2).mean(0)
    bs1, bs2 = k * a1, k * s2
    bmean = bs1 / N + U * mean.abs()
    bvar = (bs2 + 2 * mean.abs() * bs1) / N
    inv, binv = invstd_interval(var, bvar)
    g, b = gamma.double(), beta.double()
    sc = g * inv
    bsc = g.abs() * binv + U * sc.abs()
    sh = b - mean * sc
    bsh = mean.abs() * bsc + sc.abs() * bmean + U * (b.abs() + 2 * (mean * sc).abs())
    unb = var * (N / (N - 1.0)) if N > 1 else var
    bunb = bvar * (N / (N - 1.0)) if N > 1 else bvar
    rmn = (1 - MOM) * rm.double() + MOM * mean
    rvn = (1 - MOM) * rv.double() + MOM * unb
    return {"sum": (s1, bs1), "sumsq": (s2, bs2), "mean": (mean, bmean), "var": (var, bvar), "invstd": (inv, binv),
            "scale": (sc, bsc), "shift": (sh, bsh),
            "running_mean": (rmn, 5 * U * (((1 - MOM) * rm.double()).abs() + (MOM * mean).abs()) + MOM * bmean),
            "running_var": (rvn, 5 * U * (((1 - MOM) * rv.double()).abs() + (MOM * unb).abs()) + MOM * bunb)}


def eval_coeffs_ref(gamma, beta, rm, rv):
    """eval-mode coefficients from the running statistics: scale = gamma / sqrt(rv + eps), shift = beta - rm scale.
    Bounds: sum, rsqrt (2 u for a float32 one), product: 4 (+ 1) u |scale|; shift: |rm| b_scale + 2 u (|beta| + |rm scale|)"""
    sc = gamma.double() / torch.sqrt(rv.double() + EPS)
    bsc = 5 * U * sc.abs()
    sh = beta.double() - rm.double() * sc
    return (sc, bsc), (sh, rm.double().abs() * bsc + 2 * U * (beta.double().abs() + (rm.double() * sc).abs()))


def affine_est32(scale, shift, A):
    """float32 restatement of the est_out of bn_finalize_kernel: max_c fma(|scale_c|, A, |shift_c|) (the device compiler
    contracts a b + c into one v_fma_f32), on the kernel's own float32 scale / shift rows"""
    return max(float(fma32(abs(float(s)), A, abs(float(h)))) for s, h in zip(scale.tolist(), shift.tolist()))


# ---- 2. bn_apply --------------------------------------------------------------------------------------------------------------
APPLY_C = [4, 32, 64, 1024]
APPLY_QUADS = [1, 255, 257, 1023, 1025, 4 * 256 * 3 + 1]     # N C / 4: bn_apply_kernel takes four 16-byte groups per thread from a
#                                                            covering grid - these leave one, two and three groups past the end
APPLY_FORMS = ("plain", "res", "res_affine")


def apply_rows(C):
    """the N whose N C / 4 are the lengths of APPLY_QUADS - for C > 4 the whole rows on either side of each of them"""
    q = C // 4
    return sorted({max(1, L // q) for L in APPLY_QUADS} | {-(-L // q) for L in APPLY_QUADS})


def apply_inputs(C, N):
    """raw, scale, shift, res, rscale, rshift"""
    return (rnd(200 + C + N, N, C, scale=2.0, shift=0.3), rnd(201 + C, C, scale=0.8, shift=0.9), rnd(202 + C, C, scale=0.5),
            rnd(203 + C + N, N, C), rnd(204 + C, C, scale=0.8, shift=0.9), rnd(205 + C, C, scale=0.5))


def apply_ref(raw, scale, shift, res=None, rscale=None, rshift=None, relu=False):
    """[relu](raw scale + shift [+ res | + res rscale + rshift]) in fp64 from the float32 operands.
    Bound: one fused multiply-add, a second one for the residual affine, one addition for the residual: (ops + 1) u sum|terms|
    (an evaluation with separately rounded products has at most 2 ops - 1 roundings, each on a partial sum of the same terms:
    inside the same bound).  ReLU is 1-Lipschitz: the bound of the pre-activation holds for the output."""
    v = raw.double() * scale.double() + shift.double()
    mag = (raw.double() * scale.double()).abs() + shift.double().abs()
    ops = 1
    if res is not None:
        r = res.double()
        ops += 1
        if rscale is not None:
            mag = mag + (r * rscale.double()).abs() + rshift.double().abs()
            r = r * rscale.double() + rshift.double()
            ops += 1
        else:
            mag = mag + r.abs()
        v = v + r
    return (v.clamp_min(0.0) if relu else v), (ops + 1) * U * mag


def sign_mask_words(out):
    """[N][C] float32 -> the int32 words spk_bn_apply(mask_out=) writes for it: [N][C / 32], bit k of word j = out[n][32 j + k] > 0"""
    N, C = out.shape
    bits = (out.reshape(N, C // 32, 32) > 0).numpy().astype(np.uint64)
    words = (bits << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32).reshape(-1))


def tie_inputs():
    """raw [4][32], scale, shift, dy: channel c has scale = float32(1 / k), k = c + 3, and shift = -1; the rows are raw = k, its
    two float32 neighbours and -k.  raw scale + shift is 0 or +-2^-25-ish depending on whether the product is rounded before
    the addition (k = 3: 0 with separate rounding, 2^-25 fused): every implementation of the decision `> 0` must use the same
    arithmetic as the forward.  dy is 1, 2 or 3 (never 0: dz shows the decision)."""
    k = torch.arange(3, 35, dtype=torch.float32)
    up = torch.from_numpy(np.nextafter(k.numpy(), F32(np.inf)))
    dn = torch.from_numpy(np.nextafter(k.numpy(), F32(0)))
    raw = torch.stack([k, up, dn, -k]).contiguous()
    scale = (1.0 / k.double()).float()
    shift = torch.full((32,), -1.0)
    dy = small_ints(290, 4, 32).abs().clamp_min(1.0)
    return raw, scale, shift, dy


# ---- 3. BatchNorm backward ----------------------------------------------------------------------------------------------------
BWD_C = [4, 32, 64, 256, 1024]
BWD_N = [1, 255, 1000]
BWD_BIG_APPLY = (32, 65541)                # 524 328 groups: beyond the 2048 x 256 of bn_bwd_apply_kernel, with a ragged tail
BWD_BIG_REDUCE = STATS_BIG                 # more than 4096 reduction blocks' worth of rows


def bwd_inputs(C, N, exact=False):
    """raw [N][C] (channel c: sigma_c in [0.5, 2), mean / sigma = 0, 3, 30 by c % 3), dy, res, gamma, beta.
    exact: dy holds integers in -3 ... 3 (sum dz is exact in float32)."""
    sig = (0.5 + 1.5 * uni(300 + C, C)).double()
    off = torch.tensor([0.0, 3.0, 30.0], dtype=torch.float64)[torch.arange(C) % 3]
    raw = ((rnd(310 + C + N % 1000, N, C).double() * math.sqrt(3.0) + off) * sig).float()
    dy = small_ints(320 + C + N % 1000, N, C) if exact else rnd(320 + C + N % 1000, N, C)
    return raw, dy, rnd(330 + C + N % 1000, N, C), rnd(340 + C, C, scale=0.3, shift=1.0), rnd(341 + C, C, scale=0.2)


def bn_rows(raw, gamma, beta):
    """the float32 rows [mean, invstd, scale, shift] a forward pass hands to the backward kernels, here the fp64 statistics of
    raw rounded once (the kernels under test in part 3 take them as inputs; the forward statistics are part 1's subject)"""
    xd = raw.double()
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    inv = (1.0 / torch.sqrt(var + EPS)).float()
    mean = mean.float()
    scale = gamma * inv
    shift = beta - mean * scale
    return torch.stack([mean, inv, scale, shift]).contiguous()


def bwd_ref(dy, raw, mask, gamma):
    """The fp64 closed form of the gradient of relu(batch_norm(raw) [+ res]) in training mode with respect to raw, gamma, beta:
        dz = mask ? dy : 0 (a select: dy may hold anything where the mask is 0),  xhat = (raw - mean) invstd,
        dbeta = sum dz, dgamma = sum dz xhat, k1 = gamma invstd, m1 = dbeta / n, m2 = dgamma / n,
        draw = k1 (dz - m1 - xhat m2)
    with the fp64 statistics of raw; `mask` (bool [N][C], or None) is the float32 forward's decision.
    -> {name: (value, bound)} for dz (exact), dbeta, dgamma, k1, m1, m2, draw.

    k = (bn_chain + 1) u.  Bounds:
      xhat     the kernels take mean and invstd as float32 rows: the rounded mean moves xhat by u |mean| invstd - stated here
               because it does not shrink with |xhat| - and the rounded invstd, the difference and the product by 3 u |xhat|:
                                                                ex = u |mean| invstd + 3 u |xhat|
      dbeta    k sum|dz|
      dgamma   k sum|dz xhat| + sum |dz| ex
      k1       2 u |k1|                                         (float32 invstd, one product)
      m1, m2   b / n + u |m|                                    (fp64 quotient stored as float32)
      draw     inner = dz - m1 - xhat m2: three operations (+ 1) on T = |dz| + |m1| + |xhat m2|, and the errors of m1, xhat,
               m2 carried through; the product with k1 another three (+ 1):
                                                                |k1| (b_m1 + ex |m2| + |xhat| b_m2 + 8 u T)"""
    N, C = raw.shape
    k = (bn_chain(N, C) + 1) * U
    xd, g = raw.double(), gamma.double()
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    inv = 1.0 / torch.sqrt(var + EPS)
    dz = dy.double() if mask is None else torch.where(mask, dy.double(), torch.zeros((), dtype=torch.float64))
    xhat = (xd - mean) * inv
    ex = U * mean.abs() * inv + 3 * U * xhat.abs()
    dbeta, bdbeta = dz.sum(0), k * dz.abs().sum(0)
    dgamma = (dz * xhat).sum(0)
    bdgamma = k * (dz * xhat).abs().sum(0) + (dz.abs() * ex).sum(0)
    k1 = g * inv
    m1, m2 = dbeta / N, dgamma / N
    bm1, bm2 = bdbeta / N + U * m1.abs(), bdgamma / N + U * m2.abs()
    T = dz.abs() + m1.abs() + (xhat * m2).abs()
    draw = k1 * (dz - m1 - xhat * m2)
    bdraw = k1.abs() * (bm1 + ex * m2.abs() + xhat.abs() * bm2 + 8 * U * T)
    return {"dz": (dz, torch.zeros_like(dz)), "dbeta": (dbeta, bdbeta), "dgamma": (dgamma, bdgamma), "k1": (k1, 2 * U * k1.abs()),
            "m1": (m1, bm1), "m2": (m2, bm2), "draw": (draw, bdraw)}


def nonfinite_dy(dy, mask):
    """dy with +inf, -inf and NaN (in turn) wherever the mask is 0, and the same tensor with zeros there"""
    bad = torch.tensor([float("inf"), float("-inf"), float("nan")])[torch.arange(dy.numel()) % 3].reshape(dy.shape)
    return torch.where(mask, dy, bad), torch.where(mask, dy, torch.zeros(()))


def pooling_scenario(C=64, N=777):
    """the scenario of include/spkhip.h: one channel (5) with a tiny gamma and a huge gradient - sqrt'(mean) of the pooling
    layer at a tiny mean - next to ordinary channels.  -> raw, dy, gamma, beta"""
    raw, dy, _, gamma, beta = bwd_inputs(C, N)
    gamma[5] = 1e-6
    dy[:, 5] *= 1e6
    return raw, dy, gamma, beta


# ---- 4. operand-scale hand-offs ---------------------------------------------------------------------------------------------
ABSMAX_N = [1, 2, 3, 4, 5, 7, 1023, 1025]
ABSMAX_BIG = 4 * 256 * 8192 + 3            # absmax_kernel runs at most 8192 blocks of 256 float4: exactly one trip of every thread
ABSMAX_LOOP = 4 * (256 * 8192 + 1) + 3     # one float4 more: thread 0 of block 0 makes a second trip of the grid-stride loop; 33.5 MB


def absmax_blocks(n):
    """host restatement of the grid of spk_absmax: stream_grid(n / 4 + 1), at most 8192 blocks of 256 threads"""
    return max(1, min(-(-(n // 4 + 1) // 256), 8192))


def absmax_cases(n):
    """-> [(name, x [n], expected slot value)]: the maximum first, last (in the scalar tail when n % 4 != 0), negative; inf / NaN
    present and left out; -0.0 and all zeros give 0"""
    base = rnd(400 + n, n, scale=0.9)
    out = []
    for name, idx, val in (("first", 0, 3.5), ("last", n - 1, 2.5), ("negative", n // 2, -4.25)):
        x = base.clone()
        x[idx] = val
        out.append((name, x, abs(val)))
    x = base.clone()
    x[n - 1] = 1.5
    for i, bad in enumerate((float("inf"), float("-inf"), float("nan"))):
        if n > i + 1:
            x[(i * 2) % (n - 1)] = bad
    out.append(("nonfinite", x, float(x[torch.isfinite(x)].abs().max())))
    z = torch.zeros(n)
    out.append(("zeros", z.clone(), 0.0))
    z[n - 1] = -0.0
    z[0] = -0.0
    out.append(("negative zero", z, 0.0))
    return out


# slots (bit patterns) of the issue: 0, a subnormal, inf, NaN, 2^-120 (the upper exponent clamp: sigma = 2^127, not 2^134),
# 1.0, just below and at a power of two, FLT_MAX
SIGMA_SLOTS = [0x00000000, 0x00000001, 0x007FFFFF, 0x7F800000, 0x7FC00000, f32_bits(2.0 ** -120), f32_bits(2.0 ** -113),
               f32_bits(2.0 ** -114), 0x3F800000, 0x407FFFFF, 0x40800000, f32_bits(1e-3), f32_bits(3e4), 0x7F7FFFFF]


def sigma_from_bits(bits):
    """host restatement of spk_sigma_from_amax_bits: 2^(14 - floor(log2 amax)), exponent clamped to a finite normal float32
    (biased 1 ... 254); 1 for zero / subnormal / inf / NaN slots"""
    e = (bits >> 23) & 0xFF
    if e in (0, 255):
        return 1.0
    se = min(max(127 + 14 - (e - 127), 1), 254)
    return 2.0 ** (se - 127)


def window_values(sig):
    """float32 inputs that sit on every boundary of the two-term fp16 window under the scale sig (a power of two, so v sig is
    exact): 65504 / sig (the largest value that does not saturate) and the next float above it; 2^-14 / sig (the smallest
    normal high term), the float32 below it (as an fp16 it rounds back up) and 2^-14 - 2^-24 (the largest subnormal fp16);
    (1 + 2^-14) / sig (low term 2^-14: the smallest normal one) and the float below it (low term 2^-14 - 2^-23: subnormal);
    their negatives; zeros; ordinary values.  Values that are no normal finite float32 under this sig are left out (FLT_MAX's
    sigma cannot reach saturation, 2^127 cannot reach a subnormal high term).  -> [n] float32, n % 4 == 0."""
    tiny = np.float32(2.0 ** -14)
    marks = [np.float32(65504.0), np.nextafter(np.float32(65504.0), F32(np.inf)), np.float32(65488.0), np.float32(65490.0),
             tiny, np.nextafter(tiny, F32(0)), np.float32(2.0 ** -14 - 2.0 ** -24),
             np.float32(1.0 + 2.0 ** -14), np.float32(1.0 + 2.0 ** -14 - 2.0 ** -23),
             np.float32(1.0), np.float32(100.5), np.float32(3.0 * 2.0 ** -20), np.float32(2.0 ** -25), np.float32(32768.0)]
    vals = [0.0, -0.0]
    for m in marks:
        v = float(m) / sig
        if math.isfinite(v) and 2.0 ** -126 <= abs(v) <= 3.4028234e38 and float(np.float32(v)) == v:
            vals += [v, -v]
    vals += [0.0] * (-len(vals) % 4)
    return torch.tensor(vals, dtype=torch.float64).float()


def window_count_ref(x, sig, scale=None, shift=None, pairs=False):
    """host restatement of f16_window_count_kernel on top of helpers.encode_pairs: [values, saturating, low term subnormal,
    high term subnormal].  x [n/4][4] float32, or the pair tensor of it with pairs=True (saturation is then read from the stored
    high term: +-65504 counts).  The affine form relu(x scale + shift) is restated for scale / shift rows whose results are
    exact in float32 (powers of two, zero shift) - what the test uses."""
    if pairs:
        tp = x
        sat = None
    else:
        v = x
        if scale is not None:
            vd = (x.double() * scale.double() + shift.double()).clamp_min(0.0)
            v = vd.float()
            assert torch.equal(v.double(), vd), "the affine form of the test must be exact in float32"
        u = (v.double() * sig).float()
        sat = int((u.abs() > 65504.0).sum())
        tp = encode_pairs(v.reshape(-1, 4), sig)
    h = tp.reshape(-1).view(torch.float16).reshape(-1, 8).float()
    hi, lo = h[:, :4], h[:, 4:]
    if sat is None:
        sat = int((hi.abs() >= 65504.0).sum())
    tiny = 2.0 ** -14
    return [hi.numel(), sat, int(((lo != 0) & (lo.abs() < tiny)).sum()), int(((hi != 0) & (hi.abs() < tiny)).sum())]


# ---- 5. stem ------------------------------------------------------------------------------------------------------------------
STEM_SHAPES = [(1, 1, 1), (1, 1, 5), (1, 3, 1), (2, 2, 2), (1, 80, 1), (2, 7, 9), (3, 80, 547)]      # the last: 131 280 pixels,
#                                                            beyond 2048 x 64 (stem_fwd_kernel) and 1024 x 64 (stem_wgrad_kernel)


def stem_chain(NP, cap):
    """roundings of one value into a per-block sum of stem_fwd_kernel's statistics (cap 2048) / stem_wgrad_kernel (cap 1024):
    a thread owns pixels pl, + blocks 64, ...: ceil(NP / (blocks 64)) fused multiply-adds (additions for the statistics), four
    shuffle steps over the 16 pixel lanes of a wave, three additions over the four waves; one more for the rounding of the
    product v v"""
    blocks = min(-(-NP // 64), cap)
    return -(-NP // (blocks * 64)) + 4 + 3 + 1


def stem_inputs(B, Fd, T, exact=False):
    """x [B][F][T], w [32][1][3][3], epilogue scale / shift [32], dy [B][32][F][T], previous dw.  exact: integers in -3 ... 3"""
    s = 500 + B + 3 * Fd + 7 * T
    if exact:
        return (small_ints(s, B, Fd, T), small_ints(s + 1, 32, 1, 3, 3), None, None, small_ints(s + 4, B, 32, Fd, T),
                small_ints(s + 5, 32, 1, 3, 3))
    return (rnd(s, B, Fd, T), rnd(s + 1, 32, 1, 3, 3, scale=0.5), rnd(s + 2, 32, scale=0.5, shift=1.0), rnd(s + 3, 32, scale=0.3),
            rnd(s + 4, B, 32, Fd, T), rnd(s + 5, 32, 1, 3, 3))


def stem_lengths(B, T):
    """utterance lengths [B] int32: the first is T, the others shorter (at least 1)"""
    return torch.tensor([max(1, T - (3 * b + 2) % T) if b else T for b in range(B)], dtype=torch.int32)


def stem_ref(x, w, esc=None, esh=None, relu=False, lens=None):
    """Conv2d(1, 32, 3, stride 1, pad 1) [+ per-channel affine] [+ ReLU] in fp64, NHWC [B][F][T][32].  lens: frames t >= lens[b]
    are read as zero (whatever x holds there) and the outputs there are +0.
    Bound: nine fused multiply-adds, 10 u sum|x w|; the epilogue one more: |es| 10 u sum|x w| + 2 u (|v es| + |eh|)."""
    B, Fd, T = x.shape
    xd = x.double()
    valid = None
    if lens is not None:
        valid = (torch.arange(T)[None, :] < lens[:, None].long())[:, None, :].expand(B, Fd, T)
        xd = torch.where(valid, xd, torch.zeros((), dtype=torch.float64))
    wd = w.double()
    v = F.conv2d(xd[:, None], wd, None, 1, 1)
    bound = 10 * U * F.conv2d(xd.abs()[:, None], wd.abs(), None, 1, 1)
    if esc is not None:
        es, eh = esc.double().view(1, -1, 1, 1), esh.double().view(1, -1, 1, 1)
        bound = es.abs() * bound + 2 * U * ((v * es).abs() + eh.abs())
        v = v * es + eh
    if relu:
        v = v.clamp_min(0.0)
    if valid is not None:
        v = torch.where(valid[:, None], v, torch.zeros((), dtype=torch.float64))
        bound = torch.where(valid[:, None], bound, torch.zeros((), dtype=torch.float64))
    return v.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


def stem_stats_ref(v, bv):
    """fp64 sums of the fp64 output v (with its element bounds bv) over all pixels, per channel, and their bounds: the summation
    (stem_chain + 1) u sum|v| resp. sum v^2, plus the element errors carried through: sum b and sum 2 |v| b
    -> (sum, bound), (sumsq, bound)"""
    NP = v.numel() // 32
    k = (stem_chain(NP, 2048) + 1) * U
    v2, b2 = v.reshape(-1, 32), bv.reshape(-1, 32)
    return ((v2.sum(0), k * v2.abs().sum(0) + b2.sum(0)),
            ((v2 * v2).sum(0), k * (v2 * v2).sum(0) + (2 * v2.abs() * b2 + b2 * b2).sum(0)))


def stem_wgrad_ref(x, dy, prev=None):
    """dw[c][kh][kw] = sum_p x[p + tap] dy[p][c] in fp64 (+ prev).  Bound: (stem_chain + 1) u sum|x dy| - the per-block partials
    are folded in fp64 and stored as float32 once - plus one rounding of the sum with accumulate."""
    B, Fd, T = x.shape
    xp = F.pad(x.double(), (1, 1, 1, 1))
    dyd = dy.double()
    dw = torch.zeros(32, 1, 3, 3, dtype=torch.float64)
    mag = torch.zeros_like(dw)
    for kh in range(3):
        for kw in range(3):
            win = xp[:, None, kh:kh + Fd, kw:kw + T]
            dw[:, 0, kh, kw] = (win * dyd).sum((0, 2, 3))
            mag[:, 0, kh, kw] = (win * dyd).abs().sum((0, 2, 3))
    bound = (stem_chain(B * Fd * T, 1024) + 1) * U * mag
    if prev is not None:
        dw = dw + prev.double()
        bound = bound + U * dw.abs()
    return dw, bound
