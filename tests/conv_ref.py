"""fp64 restatement, engineered inputs, operand-mode emulations and per-element error bounds for the convolution kernels
(csrc/conv_kernel.h with conv_mfma / conv_split / conv_pipe.hip, pack.hip and the conv_wgrad*.hip family) - test infrastructure
only.  The two streaming kernels, conv1x1_stream.hip and conv3x3_c32_stream.hip, are the same tap-table launches with their own
tiling of the pixel axis and their own statistics mechanism: the last part of this file holds their statistics chains, the
partition of the pixels into partial rows and their case lists (tests/test_conv_stream_edges_cpu.py and _gpu.py).

tests/test_conv_edges_cpu.py shows that the restatement agrees with F.conv2d and autograd in float64, that float32 torch on the
CPU stays inside the `f32` bound, that the numpy emulation of every operand mode stays inside that mode's representation term
and that the integer inputs are exact under every emulation; tests/test_conv_edges_gpu.py runs the kernels on the same inputs
against the same bounds.  check / rnd / U / RATIOS are those of tests/small_kernels_ref.py.

The convolution is restated the way ops._conv_launch describes it to the kernel, as a TAP TABLE: for the logical output pixel
(oy, ox) and the tap (dy, dx, wi) the input pixel is (oy IS + dy, ox IS + dx), 0 outside the input, and the weight is plane wi
of the packed tensor; the logical pixel lands at (oy OS + ooy, ox OS + oox) of the physical output.  A forward convolution is
one such launch (a strided 1x1 reads its input through a strided view, ips = IS: the same sum), a stride-1 data gradient one
with mirrored taps and transposed weights, a stride-2 data gradient four of them (the parity classes of the input pixel).

Everything here is NCHW on the CPU; the GPU file converts.  Rules:
  * values in fp64 from the float32 inputs; a ReLU on a VALUE needs no decision (relu is 1-Lipschitz: the bound of its argument
    is the bound of its result); a MASK that gates another tensor (sign bits, act > 0, raw scale + shift > 0) is the float32
    decision, and an input on which fused and unfused float32 arithmetic could decide differently is refused (mask_from_raw);
  * per-element bounds with u = 2^-24, nothing fitted to what a kernel returns.  For a sum of K products the accumulation term
    is (K + 1) u sum|a w|: ANY order of adding K terms puts at most K - 1 roundings on the path of one term, the products are
    exact in the fp32 accumulator of the split modes and carry one rounding (fused: none) in the f32 mode, and one more covers the
    store.  The operand-representation terms of DESIGN.md section 3a are added per mode (rep_term), every fused transform and
    epilogue step adds its own roundings on its own terms (stage, Conv.finish), and errors of staged values propagate through
    sum e_a |w|;
  * integer inputs (x in -2 .. 2, w in -1 .. 1, integer vectors): every operand has one term in every mode and every partial sum
    is an integer below sum|a w|, so wherever that stays below 2^24 (exact_ok) the comparison is `==`.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import weights as W
from small_kernels_ref import F32, RATIOS, U, check, rnd      # noqa: F401  (re-exported to the two test files)

SPLITS = {"f32": 0, "bf16x6": 6, "bf16x9": 9, "f16x3": 3}
MODE_OF = {v: k for k, v in SPLITS.items()}
SLACK = 1.0 + 2.0 ** -20          # second-order terms of the first-order bounds below


def split_for(mode, ksize):
    """operand mode of a launch (ops.split_for): the bf16-term modes cover the 3x3 convolutions, 1x1 run on fp32 operands there"""
    s = SPLITS[mode]
    return s if (ksize == 3 or s == 3) else 0


def ints(seed, lo, hi, *shape):
    """seeded float32 tensor of integers in lo .. hi"""
    n = int(np.prod(shape))
    v = np.minimum(np.floor(W.hash_uniform(seed, 5, n) * (hi - lo + 1)), hi - lo) + lo
    return torch.from_numpy(v.astype(np.float32).reshape(shape))


def v4(t):
    return t.double().view(1, -1, 1, 1)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def conv_inputs(seed, B, Cin, Cout, H, Wd, k, exact=False):
    """x [B][Cin][H][W], w [Cout][Cin][k][k].  Random: uniform magnitudes, except input channel 3 at 2^-20 of the rest (below
    the f16x3 scale window: the absolute floor of section 3a is in play) and output channel 5 at 2^-10 (a low-magnitude channel
    that a max-norm yardstick cannot see)."""
    if exact:
        return ints(seed, -2, 2, B, Cin, H, Wd), ints(seed + 1, -1, 1, Cout, Cin, k, k)
    x, w = rnd(seed, B, Cin, H, Wd), rnd(seed + 1, Cout, Cin, k, k, scale=0.2)
    x[:, 3] *= 2.0 ** -20
    w[5] *= 2.0 ** -10
    return x, w


def vec_affine(seed, C, exact=False):
    """(scale, shift) of a fused input transform or an epilogue affine"""
    if exact:
        return ints(seed, -1, 2, C), ints(seed + 1, -1, 1, C)
    return rnd(seed, C, scale=0.5, shift=1.0), rnd(seed + 1, C, scale=0.3)


def vec_bn4(seed, C, exact=False):
    """[mean, invstd, scale, shift] rows of a BatchNorm"""
    if exact:
        return torch.stack([ints(seed, -1, 1, C), ints(seed + 1, 1, 2, C), ints(seed + 2, -1, 2, C), ints(seed + 3, -1, 1, C)])
    return torch.stack([rnd(seed, C, scale=0.3), rnd(seed + 1, C, scale=0.2, shift=1.0), rnd(seed + 2, C, scale=0.5, shift=1.0),
                        rnd(seed + 3, C, scale=0.4)])


def vec_coef(seed, C, exact=False):
    """[k1, m1, m2] rows of spk_bn_bwd_finalize"""
    if exact:
        return torch.stack([ints(seed, -2, 2, C), ints(seed + 1, -1, 1, C), ints(seed + 2, -1, 1, C)])
    return torch.stack([rnd(seed, C, scale=0.3, shift=1.0), rnd(seed + 1, C, scale=0.05), rnd(seed + 2, C, scale=0.05)])


def tensor(seed, exact, *shape, scale=1.0, shift=0.0):
    return ints(seed, -2, 2, *shape) if exact else rnd(seed, *shape, scale=scale, shift=shift)


def sign_bits(mask):
    """[B][C][H][W] bool -> the int32 sign-mask words of spk_bn_apply(mask=True): [B H W][C / 32], bit k = channel 32 j + k"""
    B, C, H, Wd = mask.shape
    bits = mask.permute(0, 2, 3, 1).reshape(-1, C // 32, 32).numpy().astype(np.uint64)
    words = (bits << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32).reshape(-1).copy())


def mask_from_raw(raw, scale, shift):
    """the float32 decision raw scale + shift > 0 (the kernels recompute a ReLU mask this way).  Float32 evaluates the
    expression with one or two roundings (fused or not), each below u (|raw scale| + |shift|): a non-zero value closer to 0 than
    4 u of that would make the decision depend on the instruction selection, and such an input is refused.  (An exact 0 - the
    integer inputs have many - is 0 either way.)"""
    p, h = raw.double() * v4(scale), v4(shift)
    m = p + h
    amb = (m != 0) & (m.abs() <= 4 * U * (p.abs() + h.abs()))
    assert not bool(amb.any()), "a recomputed ReLU mask within rounding of 0: choose another seed"
    return m > 0


# ---- the tap table ------------------------------------------------------------------------------------------------------------
def out_hw(h, w, k, s):
    pad = 1 if k == 3 else 0
    return (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1


def fwd_taps(k):
    return [(kh - 1, kw - 1, kh * 3 + kw) for kh in range(3) for kw in range(3)] if k == 3 else [(0, 0, 0)]


def dgrad_taps(k):
    return [(1 - kh, 1 - kw, kh * 3 + kw) for kh in range(3) for kw in range(3)] if k == 3 else [(0, 0, 0)]


def dgrad_classes(k, IH, IW):
    """stride-2 data gradient -> [(cy, cx, LH, LW, taps)]: input pixel (2 ly + cy, 2 lx + cx) receives the taps kh with
    cy + 1 - kh even, from dy pixel (ly + (cy + 1 - kh) / 2, ..).  A class without pixels (H or W of 1) is no launch.  1x1: only
    the even pixels receive anything."""
    if k == 1:
        return [(0, 0, (IH + 1) // 2, (IW + 1) // 2, [(0, 0, 0)])]
    out = []
    for cy in range(2):
        for cx in range(2):
            LH, LW = (IH - cy + 1) // 2, (IW - cx + 1) // 2
            if LH <= 0 or LW <= 0:
                continue
            taps = [((cy + 1 - kh) // 2, (cx + 1 - kw) // 2, kh * 3 + kw) for kh in range(3) if (cy + 1 - kh) % 2 == 0
                    for kw in range(3) if (cx + 1 - kw) % 2 == 0]
            out.append((cy, cx, LH, LW, taps))
    return out


def tap_conv(a, w3, taps, IS, OH, OW):
    """out[b][o][oy][ox] = sum_t sum_c a[b][c][oy IS + dy_t][ox IS + dx_t] w3[o][c][wi_t], a = 0 outside; fp64"""
    dys, dxs = [t[0] for t in taps], [t[1] for t in taps]
    _, _, IH, IW = a.shape
    pt, pb = max(0, -min(dys)), max(0, (OH - 1) * IS + max(dys) - (IH - 1))
    pl, pr = max(0, -min(dxs)), max(0, (OW - 1) * IS + max(dxs) - (IW - 1))
    ap = F.pad(a, (pl, pr, pt, pb))
    out = torch.zeros(a.shape[0], w3.shape[0], OH, OW, dtype=torch.float64)
    for dy, dx, wi in taps:
        sl = ap[:, :, pt + dy: pt + dy + (OH - 1) * IS + 1: IS, pl + dx: pl + dx + (OW - 1) * IS + 1: IS]
        out += torch.einsum("bchw,oc->bohw", sl, w3[:, :, wi])
    return out


# ---- staging: what the kernel multiplies ------------------------------------------------------------------------------------
def stage(x, in_affine=None, in_bnbwd=None):
    """-> a (fp64 staged values), e (bound of their float32 evaluation), B (the scale-slot value the library derives when the
    caller passes none: ops._amax_fwd_fallback / _amax_fallback, times SLACK for its float32 evaluation), and for in_bnbwd the
    side outputs.  Padding pixels are 0 AFTER the transform (tap_conv pads the staged tensor), never relu(shift).

    in_affine = (scale, shift): a = relu(x scale + shift); product and sum round once each: e = 2 u (|x scale| + |shift|).
    in_bnbwd = (raw, mask, bn4, coef): dz = x mask (exact), a = k1 (dz - m1 - ((raw - mean) invstd) m2) as conv_kernel.h writes
      it: six float32 operations (fewer when the compiler fuses), each result no larger than
      T = |k1| (|dz| + |m1| + (|raw| + |mean|) |invstd| |m2|), so e = 6 u T.  a is also the side output `draw`, dz the side
      output `dz` (bit-exact: a select)."""
    xd = x.double()
    if in_bnbwd is not None:
        raw, mask, bn4, coef = in_bnbwd
        dz = xd * mask
        xh_abs = (raw.double().abs() + v4(bn4[0]).abs()) * v4(bn4[1]).abs()
        a = v4(coef[0]) * (dz - v4(coef[1]) - ((raw.double() - v4(bn4[0])) * v4(bn4[1])) * v4(coef[2]))
        T = v4(coef[0]).abs() * (dz.abs() + v4(coef[1]).abs() + xh_abs * v4(coef[2]).abs())
        e = 6 * U * T * SLACK
        # spk_bnbwd_estimate: max_c |k1| (A + |m1| + (R + |mean|) invstd |m2|) (1 + 2^-16)
        A, R = float(xd.abs().max()), float(raw.abs().max())
        est = coef[0].double().abs() * (A + coef[1].double().abs() + (R + bn4[0].double().abs()) * bn4[1].double().abs() * coef[2].double().abs())
        return {"a": a, "e": e, "B": float(est.max()) * (1 + 2.0 ** -16) * SLACK, "dz": dz}
    if in_affine is not None:
        sc, sh = in_affine
        p = xd * v4(sc)
        a = torch.relu(p + v4(sh))
        e = 2 * U * (p.abs() + v4(sh).abs()) * SLACK
        # spk_affine_estimate: max_c |scale_c| absmax(x) + max_c |shift_c|
        return {"a": a, "e": e, "B": (float(sc.abs().max()) * float(xd.abs().max()) + float(sh.abs().max())) * SLACK}
    return {"a": xd, "e": None, "B": float(xd.abs().max())}


# ---- operand-representation terms ----------------------------------------------------------------------
REP6 = 2.0 ** -23 + 2.0 ** -32      # bf16x6: x = x1 + x2 + x3 exactly with |x2| <= 2^-8 |x|, |x3| <= 2^-16 |x|; the dropped cross
#                                     terms x2 w3 + x3 w2 + x3 w3 are below (2 2^-24 + 2^-32) |x w|
REP3 = 2.0 ** -21                   # f16x3: 2^-23 per operand (two 11-bit terms) + the dropped h2 g2 at 2^-22
FLOOR_REL, FLOOR_ABS = 2.0 ** -18, 2.0 ** -39     # ... and below B 2^-18 of the tensor's scale B an absolute B 2^-39 per operand


def floor_of(v_abs, B):
    """absolute representation floor of the f16x3 operands: B 2^-39 for non-zero values below B 2^-18 (their low term is an
    fp16 subnormal), nothing for the rest (covered by the relative 2^-23) and for exact zeros"""
    return ((v_abs > 0) & (v_abs < B * FLOOR_REL)).double() * (B * FLOOR_ABS)


def rep_term(split, S, bilinear, a_abs, w_abs, Ba, Bw):
    """representation error of sum a w in a mode: S = sum|a||w|, bilinear(p, q) = the same sum on other operands"""
    if split in (0, 9):
        return 0.0
    if split == 6:
        return REP6 * S
    return REP3 * S + (bilinear(floor_of(a_abs, Ba), w_abs) + bilinear(a_abs, floor_of(w_abs, Bw))) * SLACK


class Conv:
    """One launch of the tap-table convolution in fp64: acc = sum a w, S = sum (|a| + e)|w|, E = sum e |w|, K products."""

    def __init__(self, x, w3, taps, IS, OH, OW, in_affine=None, in_bnbwd=None):
        self.st = stage(x, in_affine, in_bnbwd)
        self.w = w3.double()
        self.geo = (taps, IS, OH, OW)
        self.K = len(taps) * x.shape[1]
        a, e = self.st["a"], self.st["e"]
        self.acc = self.bil(a, self.w)
        self.a_abs = a.abs() if e is None else a.abs() + e
        self.S = self.bil(self.a_abs, self.w.abs())
        self.E = 0.0 if e is None else self.bil(e, self.w.abs())
        self._rep = {}

    def bil(self, p, q):
        return tap_conv(p, q, *self.geo)

    def acc_bound(self, split, amax=None):
        """(K + 1) u S + E + the mode's representation term.  amax: the scale-slot value the caller hands the kernel (f16x3),
        default the library's own estimate"""
        key = (split, amax)
        if key not in self._rep:
            self._rep[key] = rep_term(split, self.S, self.bil, self.a_abs, self.w.abs(), amax or self.st["B"], float(self.w.abs().max()))
        return (self.K + 1) * U * self.S + self.E + self._rep[key]

    def exact_ok(self):
        """integer inputs: every partial sum of the accumulation is an integer of magnitude <= S"""
        return float(self.S.max()) < 2.0 ** 24

    def finish(self, split, epi_affine=None, add=None, add_gate=None, relu=False, amax=None):
        """the epilogue in the kernel's order: affine, add (where add_gate), ReLU -> (stored value, bound).
        affine v es + eh: two roundings on |v es| and |v es| + |eh|; the add one rounding on |v| + |add|; relu none."""
        v, b = self.acc, self.acc_bound(split, amax)
        if epi_affine is not None:
            es, eh = v4(epi_affine[0]), v4(epi_affine[1])
            b = b * es.abs() + 2 * U * ((v.abs() + b) * es.abs() + eh.abs()) * SLACK
            v = v * es + eh
        if add is not None:
            ad = add.double() if add_gate is None else add.double() * add_gate
            b = b + U * (v.abs() + b + ad.abs()) * SLACK
            v = v + ad
        if relu:
            v = torch.relu(v)
        return v, b


def stats_chain(MT, NT):
    """roundings on the way of one stored value into a partial-statistics row of conv_body (csrc/conv_kernel.h, epilogue): a lane
    owns one channel quad of one pixel row per pass, 4 NT passes per m-tile, MT m-tiles: 4 MT NT additions; then the lanes with
    the same quad fold by shuffles over the strides 8 NT .. 32: log2(8 / NT) more.  The rows (one per wave and tile) are summed in
    fp64 by the tests.  The square / the product dz xhat is a fused multiply-add: its rounding is the addition's."""
    return 4 * MT * NT + int(math.log2(8 // NT))


def stats_ref(v, b, chain):
    """EPI_STATS over the stored values: per channel (sum, bound, sum of squares, bound).  Every stored value v' = v + d, |d| <= b:
    sum: sum b + chain u sum|v'|; squares: sum (2 |v| b + b^2) + chain u sum v'^2."""
    va = v.abs() + b
    dims = (0, 2, 3)
    return (v.sum(dims), (b.sum(dims) + chain * U * va.sum(dims)) * SLACK,
            (v * v).sum(dims), ((2 * v.abs() * b + b * b).sum(dims) + chain * U * (va * va).sum(dims)) * SLACK)


def bnbwd_stats_ref(v, b, raw, mask, bn4, chain):
    """EPI_BNBWD: dz = v mask; per channel (sum dz, bound, sum dz xhat, bound), xhat = (raw - mean) invstd in float32: two
    roundings, |error| <= 2 u (|raw| + |mean|) |invstd| =: ex."""
    dz, bz = v * mask, b * mask
    xh = (raw.double() - v4(bn4[0])) * v4(bn4[1])
    ex = 2 * U * (raw.double().abs() + v4(bn4[0]).abs()) * v4(bn4[1]).abs()
    za, xa = dz.abs() + bz, xh.abs() + ex
    dims = (0, 2, 3)
    return (dz.sum(dims), (bz.sum(dims) + chain * U * za.sum(dims)) * SLACK,
            (dz * xh).sum(dims), ((bz * xa + dz.abs() * ex).sum(dims) + chain * U * (za * xa).sum(dims)) * SLACK)


# ---- forward, data gradient, weight gradient --------------------------------------------------------------------------------
def fwd(x, w, k, s, in_affine=None):
    """the launch of ops.conv_fwd: Conv over the forward taps at input stride s"""
    OH, OW = out_hw(x.shape[2], x.shape[3], k, s)
    return Conv(x, w.reshape(w.shape[0], w.shape[1], k * k), fwd_taps(k), s, OH, OW, in_affine=in_affine)


def dgrad1(dy, w, k, in_bnbwd=None):
    """the launch of a stride-1 ops.conv_dgrad: mirrored taps, weights with the channel roles swapped"""
    wt = w.permute(1, 0, 2, 3).reshape(w.shape[1], w.shape[0], k * k)
    return Conv(dy, wt, dgrad_taps(k), 1, dy.shape[2], dy.shape[3], in_bnbwd=in_bnbwd)


def dgrad(dy, w, k, s, in_hw, split, add=None, amax=None):
    """ops.conv_dgrad without fused BatchNorm forms -> (dx, bound, exact_ok).  add: the shortcut gradient or, for
    accumulate=True, the previous content of dx.  Stride 2: one launch per parity class, every launch adds its own pixels of
    `add`; a strided 1x1 leaves the odd pixels at exactly `add` (or 0)."""
    IH, IW = in_hw
    if s == 1:
        c = dgrad1(dy, w, k)
        v, b = c.finish(split, add=add, amax=amax)
        return v, b, c.exact_ok()
    wt = w.permute(1, 0, 2, 3).reshape(w.shape[1], w.shape[0], k * k)
    base = torch.zeros(dy.shape[0], w.shape[1], IH, IW, dtype=torch.float64) if add is None else add.double()
    out, bound, ok = base.clone(), torch.zeros_like(base), True
    for cy, cx, LH, LW, taps in dgrad_classes(k, IH, IW):
        c = Conv(dy, wt, taps, 1, LH, LW)
        # (the strided 1x1 launch always adds: onto `add`, or onto the zeros ops.conv_dgrad wrote - exact)
        v, b = c.finish(split, add=base[:, :, cy::2, cx::2] if (add is not None or k == 1) else None, amax=amax)
        out[:, :, cy::2, cx::2], bound[:, :, cy::2, cx::2] = v, b
        ok = ok and c.exact_ok()
    return out, bound, ok


def wgrad(x, dy, k, s, split, in_affine=None, prev=None, x_amax=None, dy_amax=None):
    """ops.conv_wgrad -> (dw, bound, exact_ok): dw[o][c][kh][kw] = sum over (b, oy, ox) of a[b][c][oy s + kh - pad][ox s + kw - pad]
    dy[b][o][oy][ox], a = the staged x (stage), n = B OH OW products per element.  The kernels sum a region in k-steps inside the
    matrix instruction, regions one after the other in a block's accumulators, blocks into slabs, slabs in spk_wgrad_reduce: a
    summation order of the n products that depends on tile, nsplit and kernel family - and any order stays inside (n + 1) u S
    (module docstring; padding pixels of a k-step multiply zeros).  accumulate adds dw_prev with one more rounding."""
    st = stage(x, in_affine)
    a, e = st["a"], st["e"]
    pad = 1 if k == 3 else 0
    B, C, _, _ = x.shape
    _, O, OH, OW = dy.shape
    dyd = dy.double()

    def bil(p, q):
        pp = F.pad(p, (pad, pad, pad, pad))
        g = torch.zeros(O, C, k, k, dtype=torch.float64)
        for kh in range(k):
            for kw in range(k):
                sl = pp[:, :, kh: kh + (OH - 1) * s + 1: s, kw: kw + (OW - 1) * s + 1: s]
                g[:, :, kh, kw] = torch.einsum("bchw,bohw->oc", sl, q)
        return g

    g = bil(a, dyd)
    a_abs = a.abs() if e is None else a.abs() + e
    S = bil(a_abs, dyd.abs())
    E = 0.0 if e is None else bil(e, dyd.abs())
    n = B * OH * OW
    b = (n + 1) * U * S + E + rep_term(split, S, bil, a_abs, dyd.abs(), x_amax or st["B"], dy_amax or float(dyd.abs().max()))
    ok = float(S.max()) < 2.0 ** 24
    if prev is not None:
        b = b + U * (prev.double().abs() + g.abs() + b) * SLACK
        ok = ok and float((prev.double().abs() + S).max()) < 2.0 ** 24
        g = g + prev.double()
    return g, b, ok


# ---- numpy / torch emulation of the operand modes: the same bilinear sum on the terms, accumulated in fp64 ---------------------
def bf16_terms(v):
    """float32 -> its three bf16 terms (round to nearest even, as pack_bf16x2) and the residual (0: the split is exact)"""
    r, t = v.double(), []
    for _ in range(3):
        h = r.float().bfloat16().double()       # the residual of a float32 against its bf16 rounding is a float32
        t.append(h)
        r = r - h
    return t, r


def sigma_of_value(B):
    """host copy of spk_sigma_from_amax_bits on the float32 B: B sigma in [2^14, 2^15)"""
    B = float(F32(B))
    if B == 0.0 or not math.isfinite(B) or B < 2.0 ** -126:
        return 1.0
    return 2.0 ** (14 - (math.frexp(B)[1] - 1))


def f16_terms(v, B):
    """float32, scale-slot value -> the two fp16 terms of v sigma (split2h), divided by sigma again"""
    sig = sigma_of_value(B)
    u = (v.double() * sig).float().clamp(-65504.0, 65504.0)
    h1 = u.half()
    h2 = (u - h1.float()).half()
    return [h1.double() / sig, h2.double() / sig]


def emulate(bilinear, a, w, split, Ba=None, Bw=None):
    """sum a w as the matrix cores of a mode receive it: the kept cross terms of the operand splits, each product and the sum
    in fp64 (the accumulation error is NOT emulated: this isolates the representation error).  a, w: float32."""
    if split == 0:
        return bilinear(a.double(), w.double())
    if split in (6, 9):
        ta, tw = bf16_terms(a)[0], bf16_terms(w)[0]
        keep = [(i, j) for i in range(3) for j in range(3) if split == 9 or i + j <= 2]
    else:
        ta = f16_terms(a, float(a.abs().max()) if Ba is None else Ba)
        tw = f16_terms(w, float(w.abs().max()) if Bw is None else Bw)
        keep = [(0, 0), (0, 1), (1, 0)]
    out = None
    for i, j in keep:
        t = bilinear(ta[i], tw[j])
        out = t if out is None else out + t
    return out


# ---- the register tiles the GPU file forces, and the C ABI's limits on them (csrc/conv_mfma.hip: conv_mfma_entry) -------------
TILE_MAP = (21, 27)                 # B = 2, 64 -> 128 channels, 3x3 stride 1
TILE_B, TILE_CIN, TILE_COUT = 2, 64, 128
# per MT a tile of more than (4 MT - 1) 32 pixels - pixel q of a tile belongs to m-tile (q / 32) % MT of wave q / (32 MT), so the
# last m-tile of the last wave works - that leaves a ragged last tile on both axes of the 21 x 27 map
TILE_OF_MT = {1: (8, 16), 2: (16, 16), 3: (16, 24), 4: (20, 25)}
TILES_F32 = [(1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (2, 2), (3, 2), (4, 2), (1, 4), (2, 4)]
TILES_SPLIT = [(1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (2, 2), (3, 2), (1, 4)]
TILES_PIPE = [(2, 1), (3, 1), (1, 2), (2, 2), (3, 2), (1, 4)]
PIX_BYTES = {0: 144, 6: 112, 9: 112, 3: 80}      # LDS bytes per halo pixel (ConvCfg<SPLIT>::LP4 * 16)
LDS_LIMIT = 160 * 1024


def tile_violations(TH, TW, MT, NT, OH, OW, Cout, IS, kspan, split, kc=1, pipe=False, m16=False):
    """the limits spk_conv_mfma states for a tile, restated: -> list of violated ones (empty: the launch is legal)"""
    bad = []
    halo = ((TH - 1) * IS + kspan) * ((TW - 1) * IS + kspan)
    if not (TH >= 1 and TW >= 1 and TH * TW <= 128 * MT):
        bad.append("tile pixels")
    if Cout % (32 * NT):
        bad.append("Cout % (32 NT)")
    if max(kc * halo * PIX_BYTES[split], 4 * 32 * (NT * 32 + 4) * 4) > LDS_LIMIT:
        bad.append("LDS")
    if pipe:
        if split != 3 or kc != 1 or (MT, NT) not in TILES_PIPE:
            bad.append("pipelined form")
        if halo > 576:
            bad.append("pipelined halo")
        if (2 * halo + 1) * PIX_BYTES[3] > LDS_LIMIT:
            bad.append("pipelined LDS")
    if m16 and not (pipe and (MT, NT) == (3, 2) and halo <= 512):
        bad.append("16x16x32 form")
    return bad


# ---- the cases the two test files share -------------------------------------------------------------------------------------
GEOM_MAPS = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (4, 6), (5, 4)]      # the last three: stride 2 meets all four parities of (H, W)
GEOM_B, GEOM_CIN, GEOM_COUT = 2, 64, 32
DISPATCH_COUT, DISPATCH_CIN, DISPATCH_MAPS = [32, 64, 96, 128, 256], [32, 64, 128], [(3, 5), (9, 11), (10, 38)]
DISPATCH_B = 2
# single-tap launches: kc channel planes per barrier (ops.KC_CANDIDATES: the first of 4, 2 whose 32 kc divides Cin), and a strided one
ONE_BY_ONE = [(32, 64, 1, 1), (64, 128, 1, 2), (128, 64, 1, 4), (64, 128, 2, 2)]      # Cin, Cout, stride, kc (Cin != Cout: not the streaming 1x1 kernel)
ONE_BY_ONE_MAP, ONE_BY_ONE_B = (9, 13), 2


# ---- weight gradients: the region loop (B = 1) --------------------------------------------------------------------------------
WG_MAP = (4, 13)             # output map: tiles (4, 6) -> 3 regions (the last one ragged: odd OW under the even-TW rule), (4, 2) -> 7
WG_TILES = [((4, 6), 3), ((4, 2), 7)]
WG_SMALL = ((3, 5), (3, 6))  # a map of 15 pixels and its tile: most of a k-step is padding
WG_FAMILIES = [
    # mode, ksize, Cin, Cout, WN, label of the kernel, dy as an f16 pair tensor.  One (input-channel, output-channel) block per slab,
    # so the number of slabs is the lowered block target itself
    ("f32", 3, 32, 32, 1, "conv_wgrad_kernel<9,4,1>", False),
    ("f32", 3, 32, 64, 2, "conv_wgrad_kernel<9,2,2>", False),
    ("f32", 3, 32, 128, 4, "conv_wgrad_kernel<9,1,4>", False),
    ("bf16x6", 3, 32, 64, 2, "conv_wgrad_split_kernel<9,2,2,6,", False),
    ("bf16x9", 3, 32, 64, 2, "conv_wgrad_split_kernel<9,2,2,9,", False),
    ("f16x3", 3, 32, 64, 2, "conv_wgrad_split_kernel<9,2,2,3,", False),
    ("f16x3", 1, 64, 64, 2, "conv_wgrad_1x1_kernel<2,2,2>", False),
    ("f16x3", 1, 128, 64, 2, "conv_wgrad_1x1_kernel<2,2,4>", False),
    ("f16x3", 3, 64, 64, 2, "conv_wgrad_wm_kernel", False),
    ("f16x3", 3, 64, 64, 2, "conv_wgrad_wm16_kernel", True),
    ("f16x3", 3, 32, 32, 1, "conv_wgrad_c32m16_kernel", True),
]


def wgrad_runs():
    """(tile, block target, input map, stride, regions) of every launch the GPU file makes per family"""
    runs = [(tile, target, WG_MAP, 1, nreg) for tile, nreg in WG_TILES for target in (1, 2, 3)]
    tile = WG_TILES[1][0]
    runs.append((tile, 2, (2 * WG_MAP[0], 2 * WG_MAP[1]), 2, WG_TILES[1][1]))
    runs.append((WG_SMALL[1], 1, WG_SMALL[0], 1, 1))
    return runs


def wgrad_tile_violations(fam, tile, in_hw, stride):
    """the limits spk_conv_wgrad and its launchers state for a tile (csrc/conv_wgrad*.hip), restated, plus the conditions under which
    ops.conv_wgrad takes the family's kernel -> list of violated ones"""
    mode, k, Cin, Cout, WN, label, pairs = fam
    TH, TW = tile
    halo = ((TH - 1) * stride + k) * ((TW - 1) * stride + k)
    pix16, pix32 = -(-(TH * TW) // 16) * 16, -(-(TH * TW) // 32) * 32
    bad = []
    if TW < 2 or TW % 2:
        bad.append("TW even")
    if Cout % (32 * WN) or Cin % 32:
        bad.append("channels")
    if "c32m16" in label:
        if halo > 32 * 6 or halo * 192 + 2 * pix32 * 128 > 80 * 1024:
            bad.append("32-channel-group window / LDS")
    elif "wm" in label:
        if Cin % 64 or Cout % 64 or halo > 16 * 7 or TH * TW > 64 or halo * 384 + pix16 * 448 > 80 * 1024:
            bad.append("2 x 2 wave windows / LDS")
        if "wm16" in label and halo * 416 + 2 * pix32 * 256 > 80 * 1024:
            bad.append("16x16x32 LDS")
    elif "1x1" in label:
        cg = int(label[-2])
        if k != 1 or Cin % (32 * cg) or TH * TW > 64 or pix16 * (cg * 192 + WN * 192 + 64) > 80 * 1024:
            bad.append("grouped 1x1")
    else:
        if halo > 32 * 5:
            bad.append("halo prefetch window")
        if TH * TW > (256 // (8 * WN)) * 4:
            bad.append("dY prefetch window")
    return bad


# ---- the two streaming kernels (csrc/conv1x1_stream.hip, csrc/conv3x3_c32_stream.hip) ------------------------------------------
# Both are one tap-table launch (fwd / dgrad1 above) in the f16x3 mode: the outputs are Conv.finish(3, ...).  What is their own:
# which pixels form a tile, which tiles a persistent block walks, and how the statistics are reduced.
#
# Statistics, conv1x1_stream_kernel (epilogue, read line by line): a lane holds one output channel of 2 row tiles x 16 accumulator
# registers = 32 pixels of a tile.  `float ts = 0, tq = 0` per tile; every live pixel does `ts += val` (`ts += dz`) and
# `tq += val * val` (`tq += dz * ((rw - bmu) * bis)`): 32 float32 additions into each, and the square / product is a plain C
# expression - a rounding of its own unless the compiler contracts it, so the bound counts it: 33.  (xhat = (rw - bmu) * bis has two
# more roundings: bnbwd_stats_ref's ex.)  Then `s_sum += (double)ts` across the tiles of the block, the fold of the lane pair
# l, l + 32 by __shfl_xor on the doubles (2^-53: inside SLACK), and ONE cast `(float)s_sum` of the row.
# conv3x3_c32_stream_kernel: a lane holds one channel of 16 pixels of a tile (2 tile rows of its wave x 8 columns); `ts += val`
# and `tq = __builtin_fmaf(val, val, tq)`: 16 additions, the square inside the fused operation; the same fp64 tail and cast.
# The cast rounds the ROW'S TOTAL: its term is u |row sum| per row and statistic, stated on the row (stream_stats), not folded
# into the per-element chain - |row sum| can be far below sum|v|, and a per-element chain would have to be 1 larger for every
# row an element is not even in.
STREAM_CHAINS = {"1x1": (32, 33), "3x3": (16, 16)}       # (additions into the sum, roundings into the sum of squares / products)


def stream1_tile(C):
    """conv1x1_stream_kernel<C>: (TP pixels per tile, PPP pixels per staging pass, WM pixel wave groups = partial rows per block)"""
    return 8192 // C, 1024 // C, 128 // C


def stream1_rows(P, C, G):
    """partial-statistics row of every pixel of the flattened [B H W] axis on a grid of G blocks: tile p / TP belongs to block
    tile % G, pixel wave group (p % TP) / 64 -> (row [P], number of rows)"""
    TP, _, WM = stream1_tile(C)
    p = torch.arange(P)
    return ((p // TP) % G) * WM + (p % TP) // 64, G * WM


def stream3_tiles(B, H, Wd):
    return B * (-(-H // 8)) * (-(-Wd // 16))


def stream3_rows(B, H, Wd, G):
    """conv3x3_c32_stream_kernel: tiles of 8 x 16 pixels numbered x fastest, then y, then image; VIRTUAL block tile % G (the XCD
    band permutation renames blocks, tile sets and rows go by the virtual id); wave (y % 8) / 2 -> (row [B H W], number of rows)"""
    ty, tx = -(-H // 8), -(-Wd // 16)
    b, y, x = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(Wd), indexing="ij")
    tile = (b * ty + y // 8) * tx + x // 16
    return ((tile % G) * 4 + (y % 8) // 2).reshape(-1), 4 * G


def stream_stats(v, b, rows, nrows, chains, bnbwd=None):
    """the partial rows of a streaming kernel's statistics -> (value, bound, magnitude), each [nrows][C][2]: per row stats_ref
    (bnbwd = (raw, mask, bn4): bnbwd_stats_ref) over the row's own pixels with the chain of the kernel, plus the cast of the row:
    u (|row sum| + its bound).  magnitude: sum |terms| of the row (integer inputs: exact while it stays below 2^24).  A row
    without pixels (a wave group past the tail) is 0, exactly.  The fp64 sum of the rows a test forms has the sum of the bounds."""
    C = v.shape[1]

    def px(t):
        return t.permute(0, 2, 3, 1).reshape(-1, C)
    vp, bp = px(v), px(b)
    if bnbwd is not None:
        rawp, maskp = px(bnbwd[0]), px(bnbwd[1])
    val, bnd, mag = (torch.zeros(nrows, C, 2, dtype=torch.float64) for _ in range(3))

    def img(t, idx):
        return t[idx].t().reshape(1, C, -1, 1)
    for r in range(nrows):
        idx = torch.nonzero(rows == r).reshape(-1)
        if idx.numel() == 0:
            continue
        vr, br = img(vp, idx), img(bp, idx)
        if bnbwd is None:
            s0, b0, _, _ = stats_ref(vr, br, chains[0])
            _, _, s1, b1 = stats_ref(vr, br, chains[1])
            m0, m1 = vr.abs().sum((0, 2, 3)), (vr * vr).sum((0, 2, 3))
        else:
            rr, mr = img(rawp, idx), img(maskp, idx)
            s0, b0, _, _ = bnbwd_stats_ref(vr, br, rr, mr, bnbwd[2], chains[0])
            _, _, s1, b1 = bnbwd_stats_ref(vr, br, rr, mr, bnbwd[2], chains[1])
            xh = (rr.double() - v4(bnbwd[2][0])) * v4(bnbwd[2][1])
            m0, m1 = (vr * mr).abs().sum((0, 2, 3)), (vr * mr * xh).abs().sum((0, 2, 3))
        val[r, :, 0], val[r, :, 1] = s0, s1
        bnd[r, :, 0], bnd[r, :, 1] = b0 + U * (s0.abs() + b0), b1 + U * (s1.abs() + b1)
        mag[r, :, 0], mag[r, :, 1] = m0, m1
    return val, bnd, mag


def stream1(x, w, transpose=False, in_affine=None):
    """the launch of the streaming 1x1 kernel on a C -> C weight tensor [C][C][1][1]: fwd(), or - transpose - the stride-1 data
    gradient dgrad1() (the same single tap, the matrix transposed: what pack_conv_weight(transpose=True) hands the kernel), with
    any staging the entry accepts"""
    return fwd(x, w.permute(1, 0, 2, 3) if transpose else w, 1, 1, in_affine=in_affine)


# -- case lists shared by the CPU and the GPU file
STREAM1_C = (32, 64, 128)
STREAM1_BATCH = (3, 5, 7)         # a real batch: image borders inside a tile (a 1x1 convolution must not see them)


def stream1_pixels(C):
    """pixel counts at every boundary of the tiling: one pixel; one short of a staging pass; the last row tile of a tile empty,
    holding one pixel, one short of full; exactly a tile; a tile and a pixel; two tiles, a staging pass and three pixels; three
    tiles (a grid of 2: block 0 walks two tiles, block 1 one) - and the batch of STREAM1_BATCH"""
    TP, PPP, _ = stream1_tile(C)
    return [1, PPP - 1, TP - 32, TP - 31, TP - 1, TP, TP + 1, 2 * TP + PPP + 3, 3 * TP, int(np.prod(STREAM1_BATCH))]


def stream1_layout(P):
    """P pixels as B x H x W: three images where 3 divides P (else two, else one), H the largest divisor of the rest below its root"""
    if P == int(np.prod(STREAM1_BATCH)):
        return STREAM1_BATCH
    B = 3 if P % 3 == 0 else (2 if P % 2 == 0 else 1)
    n = P // B
    H = max(d for d in range(1, int(math.isqrt(n)) + 1) if n % d == 0)
    return B, H, n // H


def stream1_grids(P, C):
    """ops.STREAM_1X1_BLOCKS of a case: 1, 2 and the tile count (the planner clamps a grid to the tile count)"""
    nt = -(-P // stream1_tile(C)[0])
    return sorted({min(g, nt) for g in (1, 2, nt)})


def stream1_sweep_pixels(C):
    TP, PPP, _ = stream1_tile(C)
    return 2 * TP + PPP + 3


# the variants: (input, add, add mask, statistics, BatchNorm backward).  input: "f32" | "aff" (fused BatchNorm + ReLU) | "pair"
# (f16 pair tensor); BatchNorm backward: None | "raw" (mask recomputed) | "bits".  A variant with a pair input, a mask or the
# BatchNorm-backward statistics is a data gradient (transposed weights); the others are forwards.
STREAM1_EPILOGUES = [(False, False, False, None), (False, False, True, None), (True, False, False, None), (True, True, False, None),
                     (False, False, True, "raw"), (False, False, True, "bits"), (True, True, True, "bits"), (True, False, True, "raw")]
STREAM1_VARIANTS = [(inp,) + e for inp in ("f32", "aff", "pair") for e in STREAM1_EPILOGUES]
STREAM1_P_SWEEP = [("aff", False, False, True, None), ("pair", True, True, True, "bits")]
# the five compile-time instances of spk_conv1x1_stream's PICK; every other variant takes the generic instance
STREAM1_COMPILED = [("aff", False, False, True, None), ("f32", False, False, True, None), ("pair", False, False, True, "raw"),
                    ("pair", True, True, False, None), ("pair", True, True, True, "bits")]


def stream1_is_dgrad(variant):
    inp, add, addmask, stats, bnb = variant
    return inp == "pair" or addmask or bnb is not None


def edge_bits(shape, seed):
    """a ReLU decision [B][C][H][W] whose sign-mask words include all-zero, all-one and single-bit words (bit 0, bit 31), the
    last pixel's last word being the single bit 31 where there are three pixels or more, and seeded words elsewhere"""
    B, C, H, Wd = shape
    P, nw = B * H * Wd, C // 32
    m = (ints(seed, 0, 1, P, nw, 32) > 0)
    pat = [torch.zeros(32, dtype=torch.bool), torch.ones(32, dtype=torch.bool), torch.arange(32) == 0, torch.arange(32) == 31]
    for i in range(min(P, 4) * nw):
        m.view(-1, 32)[i] = pat[i % 4]
    if P >= 3:
        m[P - 1, nw - 1] = pat[3]
        m[P - 1, 0] = pat[3] if nw == 1 else pat[1]
    return m.reshape(B, H, Wd, C).permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def stream1_case(C, P, variant, exact):
    """inputs and fp64 references of one case (computed once; grids and tests share it; never modified) -> dict"""
    inp, add, addmask, stats, bnb = variant
    B, H, Wd = stream1_layout(P)
    seed = 700 + C + 7 * P
    c = {"shape": (B, H, Wd), "dgrad": stream1_is_dgrad(variant)}
    c["x"], c["w"] = conv_inputs(seed, B, C, C, H, Wd, 1, exact)
    c["ia"] = vec_affine(seed + 2, C, exact) if inp == "aff" else None
    c["add"] = tensor(seed + 4, exact, B, C, H, Wd) if add else None
    c["gate"] = edge_bits((B, C, H, Wd), seed + 5) if addmask else None
    c["conv"] = stream1(c["x"], c["w"], c["dgrad"], c["ia"])
    c["out"] = c["conv"].finish(3, add=c["add"], add_gate=c["gate"])
    if bnb is not None:
        c["raw"], c["bn4"] = tensor(seed + 6, exact, B, C, H, Wd, scale=2.0, shift=0.3), vec_bn4(seed + 7, C, exact)
        c["mask"] = edge_bits((B, C, H, Wd), seed + 11) if bnb == "bits" else mask_from_raw(c["raw"], c["bn4"][2], c["bn4"][3])
    return c


def stream1_stats(c, G, exact):
    """partial rows of case c on a grid of G blocks (stream_stats; integer inputs: no element bound)"""
    if ("stats", G) not in c:
        v, b = c["out"]
        rows, nrows = stream1_rows(v.shape[0] * v.shape[2] * v.shape[3], v.shape[1], G)
        bn = (c["raw"], c["mask"], c["bn4"]) if "raw" in c else None
        c["stats", G] = stream_stats(v, torch.zeros_like(b) if exact else b, rows, nrows, STREAM_CHAINS["1x1"], bn)
    return c["stats", G]


STREAM3_MAPS = [(1, 1), (1, 16), (8, 1), (8, 16), (8, 17), (9, 16), (7, 15), (9, 33), (17, 17), (25, 49)]
STREAM3_B = (1, 2)
STREAM3_SWEEP_MAP = (25, 49)          # 4 x 4 tiles per image: interior tiles without a bounds test, ragged edges one pixel wide
STREAM3_GRIDS = (1, 5, 7, 8, 15, 16, 24)      # and the tile count; 8, 16, 24, 32: the XCD band permutation


def stream3_grids(B, H, Wd):
    """ops.STREAM_C32_BLOCKS of a case: the tile count (the default grid on a small map), and on the sweep map the grids that
    leave some blocks a tile more than others in the two-tiles-in-flight loop"""
    nt = stream3_tiles(B, H, Wd)
    return sorted({g for g in STREAM3_GRIDS if g <= nt} | {nt}) if (H, Wd) == STREAM3_SWEEP_MAP else [nt]


@functools.lru_cache(maxsize=None)
def stream3_case(B, H, Wd, aff, exact):
    c = {}
    seed = 800 + 100 * B + 3 * H + Wd
    c["x"], c["w"] = conv_inputs(seed, B, 32, 32, H, Wd, 3, exact)
    c["ia"] = vec_affine(seed + 2, 32, exact) if aff else None
    c["conv"] = fwd(c["x"], c["w"], 3, 1, in_affine=c["ia"])
    c["out"] = c["conv"].finish(3)
    return c


def stream3_stats(c, G, exact):
    if ("stats", G) not in c:
        v, b = c["out"]
        rows, nrows = stream3_rows(v.shape[0], v.shape[2], v.shape[3], G)
        c["stats", G] = stream_stats(v, torch.zeros_like(b) if exact else b, rows, nrows, STREAM_CHAINS["3x3"])
    return c["stats", G]


# operand scales far apart: inputs near 2^40, weights near 2^-50 (exact power-of-two scalings of the usual inputs), and the scale
# slot the caller hands in a loose bound 2^3 above the true maximum.  Outputs near 2^-10: normal floats.
FAR_X, FAR_W, FAR_LOOSE = 2.0 ** 40, 2.0 ** -50, 8.0


def far_case(C, H, Wd, k):
    x, w = conv_inputs(900 + C + k, 2, C, C, H, Wd, k)
    x, w = x * FAR_X, w * FAR_W
    amax = float(x.abs().max()) * FAR_LOOSE
    c = fwd(x, w, k, 1)
    return x, w, amax, c.finish(3, amax=amax)
