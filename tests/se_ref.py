"""Squeeze-and-excitation reference (test infrastructure only): the SE-ResNet-34 trunk restated on the oracle's functions, and
fp64 restatements with per-element error bounds of the kernels in csrc/se.hip.

Model level.  oracle/ does not know this architecture, so the trunk is restated here from the reference's SEBasicBlock / SELayer
(scripts/model.py:17-33, 67-97, factory :300-302) with oracle.spk_oracle's _bn, stats_pool and heads.  Every ReLU goes through
`O.F.relu`, so oracle.masked can record and prescribe masks; the SE hidden ReLU is a mask of its own ([B, C/16]), in call order
between the block's two.  `oracle_knows_se()` makes oracle.spk_oracle.trunk dispatch "se_resnet34" here for the length of a
`with` block, which is all that oracle.masked and tests/helpers.py need.

Kernel level.  One function per kernel: fp64 values from the float32 inputs the kernel gets, and a bound per element from the
kernel's arithmetic: (roundings + 1) u sum|terms| with u = 2^-24, the rule of tests/bn_stem_ref.py.  Inputs that a kernel takes
from an earlier kernel (q, u, g, da, ...) are the float32 tensors of that kernel; where a kernel chains several small products
the bound of one stage is carried through the next one's |weights|.  Nothing is fitted to what a kernel returns.
"""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import spk_oracle as O
from oracle import weights as W

U = 2.0 ** -24
TINY = 2.0 ** -50            # the fp64 accumulations of the kernels, against sum|terms|
ARCH = "se_resnet34"
LAYERS = [3, 4, 6, 3]        # scripts/model.py:300-302
REDUCTION = 16
SE_ROWS = 512                # csrc/se.hip: pixels of one utterance per reduction block
FC0_GAIN, FC2_GAIN = 2.0, 6.0


# ---- state -------------------------------------------------------------------------------------------------------------------
def state_spec(spk_num, feat_dim=80, pooling="mean+std", loss="AAM"):
    """[(key, shape, kind, stream, gain)] in the reference's state-dict order: the resnet34 entries keep their fill stream
    (index in the resnet34 spec); the two SE tensors follow each block's bn2 (SEBasicBlock registers se before downsample) and
    take stream 10000 + their index in THIS list."""
    out = []
    for i, (key, shape, kind) in enumerate(W.state_spec(spk_num, feat_dim, pooling, loss, "resnet34")):
        out.append((key, shape, kind, i, 1.0))
        if key.startswith("res.layer") and key.endswith(".bn2.num_batches_tracked"):
            p = key[:-len(".bn2.num_batches_tracked")]
            c = W.STAGE_WIDTH[int(p[len("res.layer")]) - 1]
            out.append((p + ".se.fc.0.weight", (c // REDUCTION, c), "linear_w", None, FC0_GAIN))
            out.append((p + ".se.fc.2.weight", (c, c // REDUCTION), "linear_w", None, FC2_GAIN))
    return [(k, s, kd, st if st is not None else 10000 + i, g) for i, (k, s, kd, st, g) in enumerate(out)]


def make_state(seed, spk_num, feat_dim=80, pooling="mean+std", loss="AAM"):
    """oracle.weights.make_state(..., "resnet34") for the shared keys; the SE matrices are nn.Linear-like fills scaled x2 (fc.0)
    and x6 (fc.2) so that the gates span (0, 1) instead of sitting near 0.5"""
    st = {}
    for key, shape, kind, stream, gain in state_spec(spk_num, feat_dim, pooling, loss):
        v = W.fill_tensor(seed, stream, shape, kind)
        st[key] = (v * np.float32(gain)).astype(np.float32) if gain != 1.0 else v
    return st


# ---- trunk -------------------------------------------------------------------------------------------------------------------
def se_layer(st, p, x):
    """SELayer.forward, scripts/model.py:28-33 -> (x * gate, gate [B, C])"""
    y = x.mean(dim=(2, 3))                                       # AdaptiveAvgPool2d(1) :30
    y = O.F.relu(F.linear(y, st[p + ".fc.0.weight"]))            # :22-23
    y = torch.sigmoid(F.linear(y, st[p + ".fc.2.weight"]))       # :24-25
    return x * y[:, :, None, None], y


def se_basic_block(st, p, x, stride, has_ds, train, gates=None):
    """SEBasicBlock.forward, scripts/model.py:81-97"""
    out = F.conv2d(x, st[p + ".conv1.weight"], None, stride, 1)
    out = O.F.relu(O._bn(st, p + ".bn1", out, train))
    out = F.conv2d(out, st[p + ".conv2.weight"], None, 1, 1)
    out = O._bn(st, p + ".bn2", out, train)
    out, g = se_layer(st, p + ".se", out)
    if gates is not None:
        gates.append(g.detach())
    res = x
    if has_ds:
        res = F.conv2d(x, st[p + ".downsample.0.weight"], None, stride, 0)
        res = O._bn(st, p + ".downsample.1", res, train)
    return O.F.relu(out + res)


def trunk(st, x, arch=ARCH, train=False, gates=None):
    """ResNet.forward (scripts/model.py:246-269) over SEBasicBlocks"""
    assert arch == ARCH
    x = x.view(x.size(0), 1, x.size(1), x.size(2))
    x = F.conv2d(x, st["res.conv1.weight"], None, 1, 1)
    x = O.F.relu(O._bn(st, "res.bn1", x, train))
    inplanes = 32
    for li, (planes, nblk, stride) in enumerate(zip(W.STAGE_WIDTH, LAYERS, W.STAGE_STRIDE)):
        for bi in range(nblk):
            s = stride if bi == 0 else 1
            has_ds = bi == 0 and (stride != 1 or inplanes != planes)
            x = se_basic_block(st, "res.layer%d.%d" % (li + 1, bi), x, s, has_ds, train, gates)
        inplanes = planes
    return x


@contextlib.contextmanager
def oracle_knows_se():
    """oracle.spk_oracle.trunk(st, x, "se_resnet34", train) -> this module's trunk, inside the block only"""
    real = O.trunk

    def dispatch(st, x, arch="resnet34", train=False):
        return trunk(st, x, arch, train) if arch == ARCH else real(st, x, arch, train)

    O.trunk = dispatch
    try:
        yield
    finally:
        O.trunk = real


def embed(st, x, pooling="mean+std", train=False):
    with oracle_knows_se():
        return O.embed(st, x, pooling, ARCH, train)


def forward(st, x, y=None, pooling="mean+std", loss="AAM", train=False):
    with oracle_knows_se():
        return O.forward(st, x, y, pooling, loss, ARCH, train)


# ---- kernels -----------------------------------------------------------------------------------------------------------------
def chain(HW, C):
    """float32 additions on the way of one value into a per-block partial sum of se_reduce_kernel: a thread owns one float4 of
    channels and walks every rstep-th pixel of its SE_ROWS block, then one thread folds the rstep LDS rows (rstep = 1024 / C)"""
    rstep = 1024 // C
    return -(-min(HW, SE_ROWS) // rstep) + rstep


def squeeze_ref(x, wlen=None):
    """x [B,H,W,C] float32 -> (sums [B,C] fp64, bound).  The block partials are float32, everything after them fp64."""
    B, H, Wd, C = x.shape
    xd = x.double()
    if wlen is not None:
        keep = (torch.arange(Wd)[None, :] < torch.as_tensor(wlen)[:, None]).double()[:, None, :, None]
        xd = xd * keep
    return xd.sum((1, 2)), (chain(H * Wd, C) + 1) * U * xd.abs().sum((1, 2))


def excite_ref(sums, scale, shift, w1, w2, H, Wd, wlen=None):
    """sums [B,C] fp64 (as handed to the kernel) -> {name: (value, bound)} for q, u, g.
    q: the quotient is rounded to float32, then one multiply-add (fused or not): 3 u (|scale m| + |shift|).
    u: fp64 dot product of W1 with the kernel's own float32 q (|W1| b_q), rounded once; ReLU is 1-Lipschitz.
    g: the same through W2, the sigmoid's slope is at most 1/4, rounded once."""
    cnt = (H * (torch.as_tensor(wlen).double() if wlen is not None else torch.full((sums.shape[0],), float(Wd)).double()))[:, None]
    m = sums.double() / cnt
    w1d, w2d = w1.double(), w2.double()
    if scale is None:
        q, bq = m, U * m.abs()
    else:
        q = scale.double() * m + shift.double()
        bq = 3 * U * ((scale.double() * m).abs() + shift.double().abs())
    pre = q @ w1d.t()
    bu = bq @ w1d.abs().t() + U * pre.abs() + TINY * (q.abs() @ w1d.abs().t())
    u = pre.clamp_min(0)
    a = u @ w2d.t()
    ba = bu @ w2d.abs().t() + TINY * (u.abs() @ w2d.abs().t())
    g = torch.sigmoid(a)
    bg = 0.25 * ba + 2 * U * g + 1e-14
    return {"q": (q, bq), "u": (u, bu), "g": (g, bg)}


def apply_ref(raw, scale, shift, g, res=None, rscale=None, rshift=None, relu=True, wlen=None):
    """out = relu(g (raw scale + shift) + res [rscale + rshift]), 0 at width >= wlen[b]  -> (value, bound).
    float32: z (2 roundings), g z (1), the residual affine (2), the sum (1): 4 u (|g| (|raw scale| + |shift|) + |res rscale| +
    |rshift|) covers them; ReLU is 1-Lipschitz and the width mask exact."""
    rd = raw.double()
    gd = g.double()[:, None, None, :]
    if scale is None:
        za = rd.abs()
        z = rd
    else:
        z = rd * scale.double() + shift.double()
        za = (rd * scale.double()).abs() + shift.double().abs()
    v = gd * z
    mag = gd.abs() * za
    if res is not None:
        r = res.double()
        if rscale is not None:
            mag = mag + (r * rscale.double()).abs() + rshift.double().abs()
            r = r * rscale.double() + rshift.double()
        else:
            mag = mag + r.abs()
        v = v + r
    if relu:
        v = v.clamp_min(0)
    bound = 4 * U * mag
    if wlen is not None:
        keep = (torch.arange(raw.shape[2])[None, :] < torch.as_tensor(wlen)[:, None])[:, None, :, None]
        v = v * keep
        bound = bound * keep
    return v, bound


def bwd_reduce_ref(dout, mask, raw):
    """mask: bool [B,H,W,C], what the float32 forward decided (out > 0) -> {S1, S2: (value [B,C], bound)}"""
    B, H, Wd, C = raw.shape
    e = dout.double() * mask
    er = e * raw.double()
    k = (chain(H * Wd, C) + 2) * U
    return {"S1": (e.sum((1, 2)), k * e.abs().sum((1, 2))), "S2": (er.sum((1, 2)), k * er.abs().sum((1, 2)))}


def gate_ref(S1, S2, sums, q, u, g, w1, w2, mean, invstd, scale, shift, gamma, HW, prior=None):
    """The gate's backward chain and the BatchNorm-backward finalize from the [B,C] tables (spk_se_bwd_gate).
    S1, S2, sums: fp64 tables as handed to the kernel; q, u, g: the forward's float32 tables.
    -> {name: (value, bound)} for da, du, dq, dqs, dW1 [Cr,C], dW2 [C,Cr], dbeta, dgamma, k1, m1, m2.
    prior = (dW1, dW2, dgamma, dbeta) float32: the accumulate form (one more float32 addition each)."""
    B, C = q.shape
    S1, S2, sums = S1.double(), S2.double(), sums.double()
    qd, ud, gd, w1d, w2d = q.double(), u.double(), g.double(), w1.double(), w2.double()
    mu, inv, sc, sh, ga = mean.double(), invstd.double(), scale.double(), shift.double(), gamma.double()
    dg = sc * S2 + sh * S1
    bdg = U * dg.abs() + TINY * ((sc * S2).abs() + (sh * S1).abs())
    gg = gd * (1 - gd)
    da = dg * gg
    bda = gg.abs() * bdg + 3 * U * da.abs()                      # 1 - g, g (1 - g), dg * that
    live = (ud > 0).double()
    du = (da @ w2d) * live
    bdu = (bda @ w2d.abs() + U * du.abs() + TINY * (da.abs() @ w2d.abs())) * live
    dq = du @ w1d
    bdq = bdu @ w1d.abs() + U * dq.abs() + TINY * (du.abs() @ w1d.abs())
    dqs = dq / HW
    bdqs = (bdu @ w1d.abs() + TINY * (du.abs() @ w1d.abs())) / HW + U * dqs.abs()
    dW2 = da.t() @ ud
    bdW2 = bda.t() @ ud.abs() + U * dW2.abs() + TINY * (da.abs().t() @ ud.abs())
    dW1 = du.t() @ qd
    bdW1 = bdu.t() @ qd.abs() + U * dW1.abs() + TINY * (du.abs().t() @ qd.abs())
    n = B * HW
    s = (gd * S1 + dq).sum(0)
    s_mag = ((gd * S1).abs() + dq.abs()).sum(0)
    bs_core = bdq.sum(0) + TINY * s_mag                          # before the float32 rounding of the stored / divided value
    rm = sums / HW - mu
    ss = (inv * (gd * (S2 - mu * S1) + dq * rm)).sum(0)
    ss_mag = (inv * (gd * (S2.abs() + (mu * S1).abs()) + dq.abs() * ((sums / HW).abs() + mu.abs()))).sum(0)
    bss_core = (inv * bdq * rm.abs()).sum(0) + TINY * ss_mag
    k1 = ga * inv
    out = {"da": (da, bda), "du": (du, bdu), "dq": (dq, bdq), "dqs": (dqs, bdqs),
           "k1": (k1, U * k1.abs()), "m1": (s / n, bs_core / n + U * (s / n).abs()),
           "m2": (ss / n, bss_core / n + U * (ss / n).abs())}
    for name, v, b, i in (("dW1", dW1, bdW1, 0), ("dW2", dW2, bdW2, 1), ("dgamma", ss, bss_core + U * ss.abs(), 2),
                          ("dbeta", s, bs_core + U * s.abs(), 3)):
        if prior is not None:
            p = prior[i].double()
            out[name] = (p + v, b + U * (p.abs() + v.abs()))
        else:
            out[name] = (v, b)
    return out


def bwd_apply_ref(dout, mask, raw, g, dqs, mean, invstd, coef):
    """draw = k1 (g e + dqs - m1 - xhat m2), e = dout [mask]  -> (draw, bound, e).  g, dqs, coef: the float32 tables the kernel
    reads.  float32 roundings: g e, + dqs, raw - mean, * invstd, xhat m2, - m1, - xhat m2, * k1 = 8: 9 u |k1| (|g e| + |dqs| + |m1|
    + |xhat m2|).  e itself is a select: exact."""
    e = dout.double() * mask
    gd, qd = g.double()[:, None, None, :], dqs.double()[:, None, None, :]
    k1, m1, m2 = coef[0].double(), coef[1].double(), coef[2].double()
    xh = (raw.double() - mean.double()) * invstd.double()
    dz = gd * e + qd
    o = k1 * (dz - m1 - xh * m2)
    mag = k1.abs() * ((gd * e).abs() + qd.abs() + m1.abs() + (xh * m2).abs())
    return o, 9 * U * mag, e


def draw_bound_ref(coef, dqs, mean, invstd, A, R):
    """the operand-scale bound of |draw| spk_se_bwd_gate writes (float64 evaluation of its formula, without its rounding slack):
    max_c |k1| (A + max_b |dqs| + |m1| + (R + |mean|) invstd |m2|)"""
    k1, m1, m2 = coef[0].double().abs(), coef[1].double().abs(), coef[2].double().abs()
    xh = (R + mean.double().abs()) * invstd.double().abs()
    return float((k1 * (A + dqs.double().abs().max(0).values + m1 + xh * m2)).max())


def block_tail_autograd(raw2, r, gamma, beta, w1, w2, dout, eps=1e-5):
    """fp64 autograd of z = bn2(raw2) (batch statistics), out = relu(gate(z) z + r), L = sum(dout out) on NHWC leaves
    -> dict of out, mask and the gradients wrt raw2, r, gamma, beta, w1, w2"""
    leaves = [t.double().clone().requires_grad_(True) for t in (raw2, r, gamma, beta, w1, w2)]
    x, rr, ga, be, a1, a2 = leaves
    mu = x.mean((0, 1, 2))
    var = ((x - mu) ** 2).mean((0, 1, 2))
    z = (x - mu) / torch.sqrt(var + eps) * ga + be
    q = z.mean((1, 2))
    g = torch.sigmoid(torch.relu(q @ a1.t()) @ a2.t())
    out = torch.relu(g[:, None, None, :] * z + rr)
    gs = torch.autograd.grad((out * dout.double()).sum(), leaves)
    return dict(out=out.detach(), mask=(out > 0).detach(), mean=mu.detach(), invstd=(1 / torch.sqrt(var + eps)).detach(),
                g=g.detach(), draw=gs[0], dr=gs[1], dgamma=gs[2], dbeta=gs[3], dW1=gs[4], dW2=gs[5])


def block_tail_tables(raw2, mask, gamma, beta, w1, w2, dout, eps=1e-5):
    """the same gradients from the per-kernel formulas, fp64 throughout: reduce -> gate (the [B,C]-table form of bn2's
    statistics) -> apply"""
    B, H, Wd, C = raw2.shape
    HW = H * Wd
    x = raw2.double()
    mu = x.mean((0, 1, 2))
    inv = 1 / torch.sqrt(((x - mu) ** 2).mean((0, 1, 2)) + eps)
    sc = gamma.double() * inv
    sh = beta.double() - mu * sc
    sums = x.sum((1, 2))
    ex = excite_ref(sums, sc, sh, w1, w2, H, Wd)
    q, u, g = ex["q"][0], ex["u"][0], ex["g"][0]
    rd = bwd_reduce_ref(dout, mask, raw2)
    gt = gate_ref(rd["S1"][0], rd["S2"][0], sums, q, u, g, w1, w2, mu, inv, sc, sh, gamma, HW)
    coef = torch.stack([gt["k1"][0], gt["m1"][0], gt["m2"][0]])
    draw, _, e = bwd_apply_ref(dout, mask, raw2, g, gt["dqs"][0], mu, inv, coef)
    return dict(draw=draw, dr=e, dgamma=gt["dgamma"][0], dbeta=gt["dbeta"][0], dW1=gt["dW1"][0], dW2=gt["dW2"][0], g=g)


def check(name, got, ref, bound):
    """|got - ref| <= bound on every element -> largest error / bound"""
    got = torch.as_tensor(got).detach().cpu().double()
    ref = torch.as_tensor(ref).double()
    bound = torch.broadcast_to(torch.as_tensor(bound).double(), ref.shape)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s: non-finite value" % name
    err = (got - ref).abs()
    bad = err > bound
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    assert not bool(bad.any()), "%s: %d of %d elements outside their bound, worst error / bound %.3g" % (
        name, int(bad.sum()), bad.numel(), worst)
    return worst
