"""The squeeze-and-excitation kernels (csrc/se.hip) through the C ABI against the fp64 restatements and per-element bounds of
tests/se_ref.py.  Every kernel gets the float32 / fp64 tensors the kernel before it wrote, so each comparison judges one
kernel's arithmetic.  Shapes: C in {32, 64, 128, 256}; maps 1x1, 5x7, 10x38 and one 80x300 (47 reduction blocks per utterance);
B in {1, 3}; valid widths 1 and W; gates of exactly 0 and 1; an all-zero gradient; accumulate against overwrite; f16 pair output
under the bound the gate kernel writes, with one utterance's dq 10^6 times the others'.  Every kernel twice: bit-identical."""
import numpy as np
import pytest
import torch

import se_ref as R
from helpers import decode_pairs, sigma_of, slot, slot_value
from oracle import weights as W

pytestmark = pytest.mark.gpu

MASK_ACT, MASK_BITS = 1, 3
SHAPES = [(1, 1, 1, 32), (3, 1, 1, 256), (3, 5, 7, 32), (3, 5, 7, 64), (1, 5, 7, 128), (1, 10, 38, 128), (3, 10, 38, 256),
          (3, 10, 38, 32), (1, 80, 300, 32)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops
    return ops


def rnd(seed, *shape, scale=1.0, shift=0.0):
    n = int(np.prod(shape))
    return torch.from_numpy(((W.hash_uniform(seed, 1, n) * 2 - 1) * scale + shift).astype(np.float32).reshape(shape))


def widths(B, Wd):
    return [1, Wd, max(1, Wd // 2)][:B]


def bn_rows(raw, seed):
    """mean, invstd, scale, shift, gamma (float32) of a training-mode BatchNorm over raw [B,H,W,C]"""
    C = raw.shape[-1]
    x = raw.double().reshape(-1, C)
    mean = x.mean(0)
    inv = 1 / torch.sqrt(((x - mean) ** 2).mean(0) + 1e-5)
    gamma, beta = rnd(seed, C, scale=0.5, shift=1.0), rnd(seed + 1, C, scale=0.3)
    mean, inv = mean.float(), inv.float()
    scale = gamma * inv
    return mean, inv, scale, beta - mean * scale, gamma


def twice(fn):
    """run a launch twice: the results must be bit-identical -> the first result"""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        if x is not None:
            assert torch.equal(x, y), "two runs differ"
    return a


@pytest.mark.parametrize("B,H,Wd,C", SHAPES)
@pytest.mark.parametrize("masked", [False, True])
def test_squeeze(ops, B, H, Wd, C, masked):
    x = rnd(1, B, H, Wd, C, scale=1.5, shift=0.3)
    wl = widths(B, Wd) if masked else None
    wlg = torch.tensor(wl, dtype=torch.int32, device="cuda") if masked else None
    got = twice(lambda: ops.se_squeeze(x.cuda(), wlg))
    ref, bound = R.squeeze_ref(x, wl)
    print("squeeze worst error / bound", R.check("sums", got, ref, bound))
    # small integers: every float32 partial sum is exact
    xi = torch.from_numpy((np.floor(W.hash_uniform(2, 4, x.numel()) * 7) - 3).astype(np.float32).reshape(x.shape))
    ref, _ = R.squeeze_ref(xi, wl)
    assert torch.equal(ops.se_squeeze(xi.cuda(), wlg).cpu(), ref)


@pytest.mark.parametrize("B,H,Wd,C", SHAPES)
@pytest.mark.parametrize("affine,masked", [(True, False), (False, True)])
def test_excite(ops, B, H, Wd, C, affine, masked):
    Cr = C // 16
    sums = (rnd(3, B, C, scale=1.0, shift=0.2).double() * H * Wd)
    scale, shift = (rnd(4, C, scale=0.5, shift=1.0), rnd(5, C, scale=0.3)) if affine else (None, None)
    w1, w2 = rnd(6, Cr, C, scale=0.5), rnd(7, C, Cr, scale=2.0)
    wl = widths(B, Wd) if masked else None
    wlg = torch.tensor(wl, dtype=torch.int32, device="cuda") if masked else None
    q, u, g = twice(lambda: ops.se_excite(sums.cuda(), (scale.cuda(), shift.cuda()) if affine else None, w1.cuda(), w2.cuda(),
                                          H, Wd, wlg))
    ref = R.excite_ref(sums, scale, shift, w1, w2, H, Wd, wl)
    for name, got in (("q", q), ("u", u), ("g", g)):
        print(name, "worst error / bound", R.check(name, got, *ref[name]))
    assert float(g.min()) >= 0 and float(g.max()) <= 1


def test_excite_gates_of_exactly_zero_and_one(ops):
    """a pre-activation of +-10^4: the gate is exactly 1 / exactly 0, and the backward gate kernel's da there is exactly 0"""
    B, C, Cr, H, Wd = 3, 32, 2, 5, 7
    sums = (rnd(8, B, C, scale=0.4, shift=1.0).double() * H * Wd)           # q > 0
    w1 = rnd(9, Cr, C, scale=0.005, shift=0.01)                             # > 0: u > 0, about 0.3
    w2 = rnd(10, C, Cr, scale=2.0)
    w2[0], w2[1] = 1e4, -1e4
    q, u, g = ops.se_excite(sums.cuda(), None, w1.cuda(), w2.cuda(), H, Wd)
    assert bool((u > 0).all())
    assert bool((g[:, 0] == 1.0).all()) and bool((g[:, 1] == 0.0).all())
    assert bool(((g[:, 2:] > 0) & (g[:, 2:] < 1)).all())
    S = rnd(11, B, 2, C, scale=3.0).double()
    raw = rnd(12, B, H, Wd, C, scale=1.5, shift=0.3)
    mean, inv, scale, shift, gamma = bn_rows(raw, 13)
    bn4 = torch.stack([mean, inv, scale, shift]).cuda()
    dw1, dw2 = torch.zeros(Cr, C, device="cuda"), torch.zeros(C, Cr, device="cuda")
    dga, dbe = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    coef, dq, da, du = ops.se_bwd_gate(S.cuda(), sums.cuda(), q, u, g, w1.cuda(), w2.cuda(), bn4, gamma.cuda(), dw1, dw2, dga, dbe,
                                       H * Wd)
    assert bool((da[:, :2] == 0).all()) and bool((da[:, 2:] != 0).any())
    assert bool((dw2[:2] == 0).all())


@pytest.mark.parametrize("B,H,Wd,C", SHAPES)
@pytest.mark.parametrize("form", ["plain", "identity_res", "affine_res_masked", "no_affine_masked"])
def test_apply(ops, B, H, Wd, C, form):
    raw = rnd(14, B, H, Wd, C, scale=1.5, shift=0.3)
    g = rnd(15, B, C, scale=0.5, shift=0.5)
    g[0, 0], g[0, 1] = 0.0, 1.0
    scale, shift = rnd(16, C, scale=0.5, shift=1.0), rnd(17, C, scale=0.3)
    res = rnd(18, B, H, Wd, C) if form != "plain" else None
    rs, rh = (rnd(19, C, scale=0.5, shift=1.0), rnd(20, C, scale=0.3)) if form == "affine_res_masked" else (None, None)
    if form == "no_affine_masked":
        scale = shift = None
    wl = widths(B, Wd) if form.endswith("masked") else None
    wlg = torch.tensor(wl, dtype=torch.int32, device="cuda") if wl else None
    am = slot()
    out, bits = twice(lambda: ops.se_apply(raw.cuda(), (scale.cuda(), shift.cuda()) if scale is not None else None, g.cuda(),
                                           res=res.cuda() if res is not None else None,
                                           res_affine=(rs.cuda(), rh.cuda()) if rs is not None else None, relu=True, mask=True,
                                           amax_out=am, wlen=wlg))
    ref, bound = R.apply_ref(raw, scale, shift, g, res, rs, rh, True, wl)
    print("apply worst error / bound", R.check("out", out, ref, bound))
    oc = out.cpu()
    if wl:
        for b in range(B):
            assert bool((oc[b, :, wl[b]:] == 0).all())
    assert slot_value(am) == float(oc.abs().max())
    # the sign bits are those of the stored output: word [pixel][C/32], bit c % 32
    words = bits.cpu().view(B * H * Wd, C // 32).numpy().astype(np.uint32)
    unpacked = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B, H, Wd, C).astype(bool)
    assert np.array_equal(unpacked, (oc > 0).numpy())
    # without the ReLU: the signed value
    lin = ops.se_apply(raw.cuda(), (scale.cuda(), shift.cuda()) if scale is not None else None, g.cuda(),
                       res=res.cuda() if res is not None else None, res_affine=(rs.cuda(), rh.cuda()) if rs is not None else None,
                       relu=False, wlen=wlg)
    ref, bound = R.apply_ref(raw, scale, shift, g, res, rs, rh, False, wl)
    R.check("out (no relu)", lin, ref, bound)


def block_inputs(ops, B, H, Wd, C, seed=30):
    """one SE block tail on the device: raw, BatchNorm rows, gate matrices, the forward tables and the block output with its
    sign bits, and a gradient dout"""
    raw = rnd(seed, B, H, Wd, C, scale=1.5, shift=0.3)
    mean, inv, scale, shift, gamma = bn_rows(raw, seed + 1)
    w1, w2 = rnd(seed + 3, C // 16, C, scale=0.5), rnd(seed + 4, C, C // 16, scale=2.0)
    res = rnd(seed + 5, B, H, Wd, C)
    dout = rnd(seed + 6, B, H, Wd, C, scale=2.0)
    d = dict(raw=raw, mean=mean, inv=inv, scale=scale, shift=shift, gamma=gamma, w1=w1, w2=w2, res=res, dout=dout)
    dev = {k: v.cuda() for k, v in d.items()}
    sums = ops.se_squeeze(dev["raw"])
    q, u, g = ops.se_excite(sums, (dev["scale"], dev["shift"]), dev["w1"], dev["w2"], H, Wd)
    out, bits = ops.se_apply(dev["raw"], (dev["scale"], dev["shift"]), g, res=dev["res"], relu=True, mask=True)
    dev.update(sums=sums, q=q, u=u, g=g, out=out, bits=bits, bn4=torch.stack([dev["mean"], dev["inv"], dev["scale"], dev["shift"]]))
    d["mask"] = (out > 0).cpu()
    return d, dev


@pytest.mark.parametrize("B,H,Wd,C", SHAPES)
def test_bwd_reduce(ops, B, H, Wd, C):
    d, dev = block_inputs(ops, B, H, Wd, C)
    assert 0 < float(d["mask"].double().mean()) < 1
    ca = torch.zeros(C, dtype=torch.int32, device="cuda")
    S = twice(lambda: ops.se_bwd_reduce(dev["dout"], dev["raw"], dev["bits"], MASK_BITS, chan_amax=ca))
    S_act = ops.se_bwd_reduce(dev["dout"], dev["raw"], dev["out"], MASK_ACT)
    assert torch.equal(S, S_act)                     # the two mask sources select the same values
    ref = R.bwd_reduce_ref(d["dout"], d["mask"], d["raw"])
    print("S1", R.check("S1", S[:, 0], *ref["S1"]), "S2", R.check("S2", S[:, 1], *ref["S2"]))
    e = d["dout"] * d["mask"]
    assert torch.equal(ca.cpu().view(torch.float32), e.abs().amax((0, 1, 2)))
    zero = ops.se_bwd_reduce(torch.zeros_like(dev["dout"]), dev["raw"], dev["bits"], MASK_BITS)
    assert bool((zero == 0).all())


@pytest.mark.parametrize("B,H,Wd,C", SHAPES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_bwd_gate(ops, B, H, Wd, C, accumulate):
    d, dev = block_inputs(ops, B, H, Wd, C)
    Cr, HW = C // 16, H * Wd
    S = ops.se_bwd_reduce(dev["dout"], dev["raw"], dev["bits"], MASK_BITS)
    prior = [rnd(40 + i, *s, scale=5.0) for i, s in enumerate([(Cr, C), (C, Cr), (C,), (C,)])]

    def run():
        bufs = [p.clone().cuda() for p in prior]
        r = ops.se_bwd_gate(S, dev["sums"], dev["q"], dev["u"], dev["g"], dev["w1"], dev["w2"], dev["bn4"], dev["gamma"],
                            bufs[0], bufs[1], bufs[2], bufs[3], HW, accumulate=accumulate)
        return r + tuple(bufs)

    coef, dq, da, du, dw1, dw2, dga, dbe = twice(run)
    ref = R.gate_ref(S[:, 0].cpu(), S[:, 1].cpu(), dev["sums"].cpu(), dev["q"].cpu(), dev["u"].cpu(), dev["g"].cpu(), d["w1"],
                     d["w2"], d["mean"], d["inv"], d["scale"], d["shift"], d["gamma"], HW, prior=prior if accumulate else None)
    got = {"da": da, "du": du, "dq": dq[0], "dqs": dq[1], "dW1": dw1, "dW2": dw2, "dgamma": dga, "dbeta": dbe, "k1": coef[0],
           "m1": coef[1], "m2": coef[2]}
    print({k: round(R.check(k, v, *ref[k]), 3) for k, v in got.items()})
    # the tables reproduce a plain BatchNorm-backward reduction over dz = g e + dq / HW (one value per channel has no variance:
    # xhat is then the float32 rounding of the mean times 1 / sqrt(eps), nothing to compare)
    if B * HW == 1:
        return
    dz = dev["g"].double()[:, None, None, :].cpu() * (d["dout"].double() * d["mask"]) + dq[1].double().cpu()[:, None, None, :]
    xh = (d["raw"].double() - d["mean"].double()) * d["inv"].double()
    n = B * HW
    assert torch.allclose(coef[1].double().cpu(), dz.sum((0, 1, 2)) / n, rtol=0, atol=1e-5 * float(dz.abs().sum((0, 1, 2)).max()) / n)
    assert torch.allclose(coef[2].double().cpu(), (dz * xh).sum((0, 1, 2)) / n, rtol=0,
                          atol=1e-5 * float((dz * xh).abs().sum((0, 1, 2)).max()) / n)


def test_bwd_gate_all_zero_gradient(ops):
    B, H, Wd, C = 3, 5, 7, 64
    d, dev = block_inputs(ops, B, H, Wd, C)
    S = ops.se_bwd_reduce(torch.zeros_like(dev["dout"]), dev["raw"], dev["bits"], MASK_BITS)
    bufs = [torch.full(s, 7.0, device="cuda") for s in [(C // 16, C), (C, C // 16), (C,), (C,)]]
    coef, dq, da, du = ops.se_bwd_gate(S, dev["sums"], dev["q"], dev["u"], dev["g"], dev["w1"], dev["w2"], dev["bn4"], dev["gamma"],
                                       *bufs, H * Wd)
    for t in (dq, da, du, coef[1:], *bufs):
        assert bool((t == 0).all())
    draw = ops.se_bwd_apply(torch.zeros_like(dev["dout"]), dev["raw"], dev["bits"], MASK_BITS, dev["g"], dq[1], dev["bn4"], coef)
    assert bool((draw == 0).all())


@pytest.mark.parametrize("B,H,Wd,C", SHAPES)
@pytest.mark.parametrize("pairs", [False, True])
def test_bwd_apply(ops, B, H, Wd, C, pairs):
    d, dev = block_inputs(ops, B, H, Wd, C)
    HW = H * Wd
    S = ops.se_bwd_reduce(dev["dout"], dev["raw"], dev["bits"], MASK_BITS)
    dev["u"] = dev["u"].abs() + 0.1                  # every hidden unit live, so that dq cannot vanish (u is only an input here)
    if B > 1:
        S[1] *= 1e6              # this utterance's dg, da, du and dq become 10^6 times the others'
    A, Rr, est = slot(), slot(), slot()
    ops.absmax_into(dev["dout"], A)
    ops.absmax_into(dev["raw"], Rr)
    bufs = [torch.zeros(s, device="cuda") for s in [(C // 16, C), (C, C // 16), (C,), (C,)]]
    coef, dq, _, _ = ops.se_bwd_gate(S, dev["sums"], dev["q"], dev["u"], dev["g"], dev["w1"], dev["w2"], dev["bn4"], dev["gamma"],
                                     *bufs, HW, pair=(A, Rr, est))
    if B > 1:
        rest = float(torch.cat([dq[1, :1], dq[1, 2:]]).abs().max()) if B > 2 else float(dq[1, 0].abs().max())
        assert float(dq[1, 1].abs().max()) > 1e4 * rest
    am = slot()

    def run():
        e = dev["dout"].clone()
        draw = ops.se_bwd_apply(e, dev["raw"], dev["bits"], MASK_BITS, dev["g"], dq[1], dev["bn4"], coef, e_out=e, amax_out=am,
                                pair_scale=est if pairs else None)
        return draw, e

    draw, e = twice(run)
    ref, bound, e_ref = R.bwd_apply_ref(d["dout"], d["mask"], d["raw"], dev["g"].cpu(), dq[1].cpu(), d["mean"], d["inv"], coef.cpu())
    assert torch.equal(e.cpu().double(), e_ref)                      # the shortcut gradient, in place
    true_amax = float(ref.abs().max())
    # the bound slot: the formula of the issue, evaluated from the kernel's own tables, and above every value
    formula = R.draw_bound_ref(coef.cpu(), dq[1].cpu(), d["mean"], d["inv"], slot_value(A), slot_value(Rr))
    assert formula <= slot_value(est) <= formula * (1 + 2.0 ** -14), (formula, slot_value(est))
    assert slot_value(est) >= true_amax
    if pairs:
        sig = sigma_of(est)
        got = decode_pairs(draw.cpu(), sig)
        bound = bound + 2.0 ** -22 * ref.abs() + 2.0 ** -25 / sig
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        ops.f16_window_count(draw, est, counts, pairs=True)
        assert int(counts[0]) == draw.numel() and int(counts[1]) == 0, counts
    else:
        got = draw
    print("draw worst error / bound", R.check("draw", got, ref, bound))
    assert abs(slot_value(am) - true_amax) <= float(bound.max())
    # the activated tensor as the mask source: the same values
    draw_act = ops.se_bwd_apply(dev["dout"], dev["raw"], dev["out"], MASK_ACT, dev["g"], dq[1], dev["bn4"], coef,
                                pair_scale=est if pairs else None)
    assert torch.equal(draw_act, draw)


def test_bad_arguments_are_refused(ops):
    x = torch.zeros(1, 2, 2, 48, device="cuda")
    with pytest.raises(RuntimeError):
        ops.se_squeeze(x)                                            # C is no power of two
    y = torch.zeros(1, 2, 2, 32, device="cuda")
    with pytest.raises(RuntimeError):
        ops.se_bwd_reduce(y, y, y, 2)                                # MASK_RAW has no meaning here
