"""The numeric contract of the half-precision extraction path (precision="f16", DESIGN.md section 6l, csrc/half.hip) restated in
fp64 torch / numpy on the CPU - test infrastructure only.

Rules (independent of the kernels: nothing here imports the package):
  1. every trunk convolution weight except the stem's is rounded once to fp16 (nearest even); eval BatchNorm stays an fp32
     (scale, shift) pair per channel, scale = gamma / sqrt(var + eps), shift = beta - mean * scale; fc1 stays fp32;
  2. the stem is fp32 arithmetic (conv, affine, ReLU, length mask), rounded to fp16 on store;
  3. a convolution sums exact products of fp16 values; v = acc * scale + shift (+ add) -> ReLU -> length mask (+0) -> ONE rounding
     to fp16, nearest even, subnormals kept;
  4. a value outside fp16's range is stored as the conversion gives it (+-inf) and counted per utterance; nothing is clamped;
  5. pooling reads fp16, computes in fp32 with StatsPooling's formulas (var / sqrt(mean) swapped as in the reference);
  6. masking as in the fp32 length-masked forward (the emulation below crops the utterance instead, which is what masking means).
Here the accumulations run in fp64 (acc32=True: the convolution sums in fp32 instead), so the emulation differs from a kernel by
the kernel's fp32 accumulation error and by whatever rounding flips that causes downstream.

The per-element kernel bound: with y the exact result on the same fp16 inputs, S = |scale| sum|a w| + |shift| + |add| and
K = KH KW Cin,
    |gpu - y| <= 2^-11 |y| + 2^-25 + (K + 4) 2^-24 S (1 + 2^-10)
(half an fp16 ulp; half the fp16 subnormal spacing; K - 1 fp32 additions of the accumulation in any order, the fused multiply-add
of the affine, the residual add, and slack for the rounding of the fp32 value itself, each at most 2^-24 of a partial result that S
bounds; the last factor covers the half ulp being taken of the computed instead of the exact value).  The stem uses the same
formula with K = 9: its products are rounded too, but a fused multiply-add chain of 9 terms commits 9 roundings of at most
2^-24 sum|x w| each.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle.weights import ARCH_LAYERS, STAGE_STRIDE, STAGE_WIDTH, make_input, make_state

BN_EPS = 1e-5
F16_MAX = 65504.0


def round16(t):
    """fp64 / fp32 tensor -> the same dtype holding the nearest fp16 values: ties to even, subnormals kept, overflow -> +-inf"""
    a = t.detach().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        return torch.from_numpy(a.astype(np.float16).astype(a.dtype))


def not_finite_rows(t):
    """stored values of each batch row that are not finite -> int64 [B]"""
    return (~torch.isfinite(t)).reshape(t.shape[0], -1).sum(dim=1)


def kernel_bound(y, S, K):
    return 2.0 ** -11 * y.abs() + 2.0 ** -25 + (K + 4) * 2.0 ** -24 * S * (1 + 2.0 ** -10)


def _mask_w(y, wlen):
    """y [B][H][W][C]: columns x >= wlen[b] -> +0"""
    if wlen is None:
        return y
    W = y.shape[2]
    keep = (torch.arange(W)[None, :] < torch.as_tensor(wlen, dtype=torch.int64)[:, None])[:, None, :, None]
    return torch.where(keep, y, torch.zeros_like(y))


# ---- per-kernel references -----------------------------------------------------------------------------------------------------
def stem_ref(x, w, scale, shift, wlen=None):
    """x [B][F][T] fp32, w [32][1][3][3] fp32 -> (y exact fp64 [B][F][T][32] before the rounding, S, stored fp16 values, ovf [B]).
    With wlen the frames t >= wlen[b] are read as 0 and stored as +0."""
    xd = x.double()
    if wlen is not None:
        T = x.shape[2]
        keep = torch.arange(T)[None, :] < torch.as_tensor(wlen, dtype=torch.int64)[:, None]
        xd = torch.where(keep[:, None, :], xd, torch.zeros_like(xd))
    acc = F.conv2d(xd[:, None], w.double(), None, 1, 1)
    sab = F.conv2d(xd[:, None].abs(), w.double().abs(), None, 1, 1)
    sc, sh = scale.double()[None, :, None, None], shift.double()[None, :, None, None]
    y = torch.relu(acc * sc + sh).permute(0, 2, 3, 1).contiguous()
    S = (sab * sc.abs() + sh.abs()).permute(0, 2, 3, 1).contiguous()
    y = _mask_w(y, wlen)
    st = round16(y)
    return y, S, st, not_finite_rows(st)


def conv_sums(x16, w, ksize, stride):
    """x16 [B][IH][IW][Cin] (fp16 values in any float dtype), w OIHW fp32 (rounded to fp16 here, rule 1) -> the exact sums over
    (tap, Cin) in fp64, NCHW: (sum a w, sum |a w|).  3x3 pads by 1, 1x1 by 0."""
    w16 = round16(w.double())
    xin = x16.double().permute(0, 3, 1, 2)
    pad = 1 if ksize == 3 else 0
    return F.conv2d(xin, w16, None, stride, pad), F.conv2d(xin.abs(), w16.abs(), None, stride, pad)


def conv_ref(sums, scale, shift, add16=None, relu=True, wlen=None):
    """sums: conv_sums(...); add16 [B][OH][OW][Cout] or None -> (y exact fp64 NHWC before the rounding, S, stored fp16 values,
    ovf [B])"""
    acc, sab = sums
    sc, sh = scale.double()[None, :, None, None], shift.double()[None, :, None, None]
    y = (acc * sc + sh).permute(0, 2, 3, 1)
    S = (sab * sc.abs() + sh.abs()).permute(0, 2, 3, 1)
    if add16 is not None:
        y = y + add16.double()
        S = S + add16.double().abs()
    if relu:
        y = torch.relu(y)
    y = _mask_w(y.contiguous(), wlen)
    st = round16(y)
    return y, S.contiguous(), st, not_finite_rows(st)


def pool_ref(x16, mode, wlen=None):
    """x16 [B][H][W][C] fp16 values -> (fp64 [B][C H (1 + mode)] in nn.Flatten order, bound).  Row b pools over its first wlen[b]
    frames; one frame gives NaN in the variance half ('mean+std').  Bound: tests/small_kernels_ref.pool_ref's (rtol 2e-6, atol
    1e-7, plus the conditioning term of the two-pass variance W / (W - 1) dm^2, dm = (W / 2 + 1) 2^-24 max|x|)."""
    B, H, W, C = x16.shape
    ys, bs = [], []
    for b in range(B):
        Wb = W if wlen is None else max(1, min(int(wlen[b]), W))
        xb = x16[b, :, :Wb].double().permute(2, 0, 1)            # [C][H][Wb]
        mean = xb.mean(dim=2)
        if mode == 0:
            y = mean
            bound = 2e-6 * y.abs() + 1e-7
        else:
            var = ((xb - mean[..., None]) ** 2).sum(dim=2) / (Wb - 1) if Wb > 1 else torch.full_like(mean, float("nan"))
            y = torch.cat([var, torch.sqrt(mean)], dim=-1)        # [C][2H]
            bound = 2e-6 * y.abs() + 1e-7
            if Wb > 1:
                dm = (Wb / 2 + 1) * 2.0 ** -24 * xb.abs().amax(dim=2)
                bound = bound + torch.cat([Wb / (Wb - 1.0) * dm * dm, torch.zeros_like(dm)], dim=-1)
        ys.append(y.reshape(-1))
        bs.append(bound.reshape(-1))
    return torch.stack(ys), torch.stack(bs)


def pack_ref(w):
    """OIHW fp32 -> the packed fp16 image of spk_h16_pack_conv_weight (include/spkhip.h): [tap][Cin/32][Cout/16][lane 64][8],
    lane l element j = w[16 m + (l & 15)][32 s + 8 (l >> 4) + j][tap] -> numpy float16, flat"""
    Cout, Cin, KH, KW = w.shape
    with np.errstate(over="ignore"):
        w16 = w.numpy().astype(np.float16).reshape(Cout // 16, 16, Cin // 32, 4, 8, KH * KW)     # m, r, s, q, j, t
    return np.ascontiguousarray(w16.transpose(5, 2, 0, 3, 1, 4)).reshape(-1)                      # t, s, m, q, r, j  (lane = 16 q + r)


def packed_bytes(Cout, Cin, KH, KW):
    return 2 * Cout * Cin * KH * KW


# ---- whole-model emulation -----------------------------------------------------------------------------------------------------
def _bn_rows(st, p):
    g, b = st[p + ".weight"].double(), st[p + ".bias"].double()
    rm, rv = st[p + ".running_mean"].double(), st[p + ".running_var"].double()
    scale = g / torch.sqrt(rv + BN_EPS)
    return scale, b - rm * scale


def embed(np_state, x, arch, pooling, half=True, acc32=False):
    """Eval-mode embedding of x [B][F][T] (numpy fp32).  half=False: the exact network in fp64 (no rounding anywhere).
    half=True: the contract above with fp64 accumulation (acc32: fp32 convolution sums).
    -> (embedding fp64 [B][256], ovf int64 [B], largest stored finite |value|)"""
    st = {k: torch.from_numpy(np.asarray(v).copy()) for k, v in np_state.items() if np.asarray(v).shape != ()}
    kind, layers = ARCH_LAYERS[arch]
    B = x.shape[0]
    ovf = torch.zeros(B, dtype=torch.int64)
    peak = [0.0]

    def store(t):
        if not half:
            return t
        r = round16(t)
        ovf.add_(not_finite_rows(r))
        fin = r[torch.isfinite(r)]
        if fin.numel():
            peak[0] = max(peak[0], float(fin.abs().max()))
        return r

    def conv(h, key, bn, stride, pad, add=None, relu=True):
        w = st[key].double()
        if half:
            w = round16(w)
        if half and acc32:
            acc = F.conv2d(h.float(), w.float(), None, stride, pad).double()
        else:
            acc = F.conv2d(h, w, None, stride, pad)
        sc, sh = _bn_rows(st, bn)
        v = acc * sc[None, :, None, None] + sh[None, :, None, None]
        if add is not None:
            v = v + add
        return store(torch.relu(v) if relu else v)

    xd = torch.from_numpy(x).double()[:, None]
    sc, sh = _bn_rows(st, "res.bn1")
    h = store(torch.relu(F.conv2d(xd, st["res.conv1.weight"].double(), None, 1, 1) * sc[None, :, None, None]
                         + sh[None, :, None, None]))
    inplanes = 32
    for li, (planes, nblk, stride) in enumerate(zip(STAGE_WIDTH, layers, STAGE_STRIDE)):
        for bi in range(nblk):
            p = "res.layer%d.%d" % (li + 1, bi)
            s = stride if bi == 0 else 1
            res = h
            if bi == 0 and (stride != 1 or inplanes != planes):
                res = conv(h, p + ".downsample.0.weight", p + ".downsample.1", s, 0, relu=False)
            if kind == "basic":
                o = conv(h, p + ".conv1.weight", p + ".bn1", s, 1)
                h = conv(o, p + ".conv2.weight", p + ".bn2", 1, 1, add=res)
            else:
                o = conv(h, p + ".conv1.weight", p + ".bn1", 1, 0)
                o = conv(o, p + ".conv2.weight", p + ".bn2", s, 1)
                h = conv(o, p + ".conv3.weight", p + ".bn3", 1, 0, add=res)
        inplanes = planes
    if pooling == "mean":
        pooled = h.mean(dim=3, keepdim=True)
    else:
        W = h.shape[3]
        mean = h.mean(dim=3)
        var = ((h - mean[..., None]) ** 2).sum(dim=3) / (W - 1) if W > 1 else torch.full_like(mean, float("nan"))
        pooled = torch.cat([var, torch.sqrt(mean)], dim=-1)
    emb = F.linear(pooled.flatten(1), st["fc1.weight"].double(), st["fc1.bias"].double())
    return emb, ovf, peak[0]


def distance(e, e64):
    """-> (max over rows of |e - e64| / |e64|, max over rows of 1 - cos)"""
    e, e64 = e.double(), e64.double()
    rel = ((e - e64).norm(dim=1) / e64.norm(dim=1)).max()
    cos = (e * e64).sum(dim=1) / (e.norm(dim=1) * e64.norm(dim=1))
    return float(rel), float((1.0 - cos).max())


# the four cases that stay inside fp16's range, and the two that do not: name -> (arch, seed, F, T, B, pooling, loss)
CASES = {
    "r34_s11": ("resnet34", 11, 80, 224, 3, "mean+std", "AAM"),
    "r34_s12": ("resnet34", 12, 40, 224, 3, "mean", "softmax"),
    "r18_s21": ("resnet18", 21, 40, 104, 3, "mean+std", "AAM"),
    "r50_s22": ("resnet50", 22, 40, 104, 3, "mean+std", "AAM"),
}
PEAKS = {"r34_s11": 267.0, "r34_s12": 112.0, "r18_s21": 4.4, "r50_s22": 315.0}      # largest stored |value| of the emulation
OVERFLOW_CASE = ("resnet101", 13, 40, 104, 4, "mean+std", "AAM")                   # input seed 14: every row leaves the range
SCALED_CASE = ("resnet34", 11, 80, 104, 3, "mean+std", "AAM")                      # input seed 12, row 1 times 1e4
SPK_NUM = 10


def case_state(case):
    arch, seed, Fd, T, B, pooling, loss = case
    return make_state(seed, SPK_NUM, feat_dim=Fd, pooling=pooling, loss=loss, arch=arch)


def case_input(case, input_seed=None):
    arch, seed, Fd, T, B, pooling, loss = case
    return make_input(seed + 1 if input_seed is None else input_seed, B, Fd, T, SPK_NUM)[0]


@functools.lru_cache(maxsize=None)
def case_yardstick(name):
    """-> dict: x, e64 (exact fp64 embedding), emu (emulation), ovf, peak, relL2 and cosd of the emulation against e64.
    Computed once per process and shared by the tests; callers must not modify it."""
    case = CASES[name]
    st, x = case_state(case), case_input(case)
    e64, _, _ = embed(st, x, case[0], case[5], half=False)
    emu, ovf, peak = embed(st, x, case[0], case[5], half=True)
    rel, cosd = distance(emu, e64)
    return {"case": case, "x": x, "e64": e64, "emu": emu, "ovf": ovf, "peak": peak, "relL2": rel, "cosd": cosd}
