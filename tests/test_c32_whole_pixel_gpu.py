"""The whole-pixel form of the 32-channel fused BatchNorm-backward data gradient (csrc/conv_kernel.h, CKP = 32: one 32-channel
plane of 144-byte LDS pixels, staged once, the K loop walking 2 x 9 (16-channel group, tap) steps) on a real MI355X:

  * against the fp64 restatement of tests/conv_ref.py, inside the bounds test_fused_batchnorm_backward_on_every_register_tile
    uses (tests/test_conv_edges_gpu.py), with random inputs (per-element bounds) and integer inputs (bit for bit; dz is a select
    and exact in both);
  * against the 16-channel-plane instances of the same launch (ops.C32_PLANE = 16, the switch SPK_C32_PLANE reads): the
    accumulators see the same products in the same order, so dx, the side tensors, the statistics rows and both absmax slots
    are required to be equal bit for bit.

Shapes: B = 2, 32 -> 32 channels, 3x3, f16x3.  17 x 19 with a 16 x 16 tile: four tiles, ragged right and bottom, all four
borders inside one halo; 5 x 7: smaller than the tile; 9 x 18 with the 128-pixel tile 8 x 16 of the (1, 1) register tile.
Flag sets: the two compile-time variants of the training step (conv2's gradient: in-mask bits, pair side output, statistics with
the mask recomputed; conv1's: masked shortcut add, statistics by sign bits, in-mask recomputed) and one generic combination
(activation tensor as the in-mask, both fp32 side outputs).

The pair side output is compared after decoding.  Its bound is that of the fp32 side output plus the two-term fp16
representation: round-to-nearest to 11 bits leaves a residual of at most 2^-11 |u|, its own rounding 2^-11 of that: 2^-22 |u|;
below the fp16 normal range the low term moves in steps of 2^-24 of the scaled value, which is at most B 2^-39 for the slot
value B (the scaled B lies in [2^14, 2^15)).  Integer inputs have one term and decode exactly."""
import contextlib
import functools

import pytest
import torch

import conv_ref as R
from helpers import decode_pairs, sigma_of, slot, slot_value

pytestmark = pytest.mark.gpu

NAN = float("nan")
KINDS = [False, True]        # random inputs (bounds), integer inputs (exact)
B, C = 2, 32
SHAPES = [((17, 19), (16, 16, 2, 1)), ((5, 7), (16, 16, 2, 1)), ((9, 18), (8, 16, 1, 1))]
SETS = ["conv2", "conv1", "generic"]
CK32_FLAG = 1 << 23


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops as _ops
    assert _ops.CONV_CK32 == CK32_FLAG
    yield _ops
    mine = sorted(kv for kv in R.RATIOS.items() if kv[0].startswith("c32 whole pixel"))
    print("\nlargest error / bound: " + ", ".join("%s %.3g" % kv for kv in mine))


@pytest.fixture(scope="module")
def tiling(ops):
    from pytorch_kaldi_resnet_amd import tiling as _tiling
    return _tiling


def G(t):
    return R.nhwc(t).cuda()


def Cn(t):
    return R.nchw(t.detach().cpu())


def filled(*shape):
    return torch.full(shape, NAN, device="cuda")


@contextlib.contextmanager
def patched(obj, **kw):
    old = {k: getattr(obj, k) for k in kw}
    for k, v in kw.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


@contextlib.contextmanager
def forced(table, key, val):
    old = table.get(key)
    table[key] = val
    try:
        yield
    finally:
        if old is None:
            table.pop(key, None)
        else:
            table[key] = old


@contextlib.contextmanager
def launches(ops):
    rec, real = [], ops.call

    def call(name, *args, label=None, flops=0.0, nbytes=0.0):
        rec.append((name, args, label))
        return real(name, *args, label=label, flops=flops, nbytes=nbytes)
    ops.call = call
    try:
        yield rec
    finally:
        ops.call = real


def compare(name, got, ref, bound, exact):
    got = got.detach().cpu().double()
    if exact:
        assert got.shape == ref.shape and torch.equal(got, ref), "%s: integer case not exact (%d of %d elements differ, largest %g)" % (
            name, int((got != ref).sum()), ref.numel(), float((got - ref).abs().max()))
        R.RATIOS.setdefault(name, 0.0)
    else:
        R.check(name, got, ref, bound)


def compare_sums(name, got, ref, bound, abs_sum, exact):
    compare(name, got, ref, bound, exact and float(abs_sum.max()) < 2.0 ** 24)


@functools.lru_cache(maxsize=None)
def case(hw, exact):
    """inputs and fp64 references of one map size (shared by the flag sets, never modified)"""
    H, Wd = hw
    s = 1000 + 37 * H
    c = {}
    c["wd"] = R.conv_inputs(s, 1, C, C, 1, 1, 3, exact)[1]
    c["dy"] = R.tensor(s + 3, exact, B, C, H, Wd)
    c["addt"], c["gate"] = R.tensor(s + 4, exact, B, C, H, Wd), R.tensor(s + 5, exact, B, C, H, Wd) > 0
    c["raw_i"], c["act_i"] = R.tensor(s + 11, exact, B, C, H, Wd, scale=2.0, shift=0.3), R.tensor(s + 12, exact, B, C, H, Wd)
    c["bn4_i"], c["coef"] = R.vec_bn4(s + 13, C, exact), R.vec_coef(s + 17, C, exact)
    c["raw_o"], c["act_o"] = R.tensor(s + 21, exact, B, C, H, Wd, scale=2.0, shift=0.3), R.tensor(s + 22, exact, B, C, H, Wd)
    c["bn4_o"] = R.vec_bn4(s + 23, C, exact)
    c["mask_i"] = {"raw": R.mask_from_raw(c["raw_i"], c["bn4_i"][2], c["bn4_i"][3]), "act": c["act_i"] > 0}
    c["mask_o"] = {"raw": R.mask_from_raw(c["raw_o"], c["bn4_o"][2], c["bn4_o"][3]), "act": c["act_o"] > 0}
    for src in ("raw", "act"):
        c["in_" + src] = R.dgrad1(c["dy"], c["wd"], 3, in_bnbwd=(c["raw_i"], c["mask_i"][src], c["bn4_i"], c["coef"]))
        assert c["in_" + src].exact_ok() or not exact
    return c


def run_set(ops, c, fs, hw):
    """one launch of flag set fs -> dict of device results"""
    H, Wd = hw
    wpk_t = ops.pack_conv_weight(c["wd"].cuda(), transpose=True)
    dyg = G(c["dy"])
    raw_i, bn4_i, coef = G(c["raw_i"]), c["bn4_i"].cuda(), c["coef"].cuda()
    raw_o, bn4_o = G(c["raw_o"]), c["bn4_o"].cuda()
    amax = ops._amax_fallback(dyg, (raw_i, None, bn4_i, coef))
    o_amax, s_amax = slot(), slot()
    sd = filled(B, H, Wd, C)
    r = {"in_amax": amax, "out_amax": o_amax, "side_amax": s_amax, "sd": sd}
    kw = dict(in_amax=amax, out_amax=o_amax, side_amax=s_amax, out=filled(B, H, Wd, C))
    if fs == "conv2":
        inb = (raw_i, None, bn4_i, coef, R.sign_bits(c["mask_i"]["act"]).cuda())
        r["dx"], r["part"] = ops.conv_dgrad(dyg, wpk_t, C, 3, 1, hw, in_bnbwd=inb, side=(sd, None), side_presplit=True,
                                            bn_bwd=(raw_o, None, bn4_o), **kw)
    elif fs == "conv1":
        inb = (raw_i, None, bn4_i, coef)
        r["dx"], r["part"] = ops.conv_dgrad(dyg, wpk_t, C, 3, 1, hw, in_bnbwd=inb, side=(sd, None), side_presplit=True,
                                            add=G(c["addt"]), add_mask=R.sign_bits(c["gate"]).cuda(),
                                            bn_bwd=(raw_o, None, bn4_o, R.sign_bits(c["mask_o"]["act"]).cuda()), **kw)
    else:
        inb = (raw_i, G(c["act_i"]), bn4_i, coef)
        r["sz"] = filled(B, H, Wd, C)
        r["dx"] = ops.conv_dgrad(dyg, wpk_t, C, 3, 1, hw, in_bnbwd=inb, side=(sd, r["sz"]), **kw)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("exact", KINDS)
@pytest.mark.parametrize("fs", SETS)
@pytest.mark.parametrize("hw,tile", SHAPES)
def test_whole_pixel_staging_against_fp64_and_the_16_channel_planes(ops, tiling, hw, tile, fs, exact):
    H, Wd = hw
    TH, TW, MT, NT = tile
    c = case(hw, exact)
    name = "c32 whole pixel %s" % fs
    got = {}
    with patched(ops, SPLIT=3, SPLIT_BWD=None), forced(tiling.FORCE_CONV_SPLIT, (H, Wd, 1, 3, 3, 9, C), tile):
        for plane in (32, 16):
            with patched(ops, C32_PLANE=plane), launches(ops) as rec:
                got[plane] = run_set(ops, c, fs, hw)
            conv = [(a, lab) for n, a, lab in rec if n == "spk_conv_mfma"]
            assert len(conv) == 1 and conv[0][1].startswith("conv_mfma_kernel<%d,%d,true,3>" % (MT, NT)), conv
            args = conv[0][0]
            assert tuple(args[-12:-8]) == tile, "the forced tile is the one launched"
            assert bool(args[-6] & CK32_FLAG) == (plane == 32), "plane width of the launch"
    r, r16 = got[32], got[16]

    # ---- against the 16-channel instances: bit for bit
    for k in ("dx", "sd", "sz", "part"):
        if k in r:
            assert torch.equal(r[k].view(torch.int32), r16[k].view(torch.int32)), "%s differs from the 16-channel planes" % k
    for k in ("in_amax", "out_amax", "side_amax"):
        assert int(r[k].cpu()[0]) == int(r16[k].cpu()[0]), "%s differs from the 16-channel planes" % k

    # ---- against the fp64 reference
    in_src = {"conv2": "act", "conv1": "raw", "generic": "act"}[fs]
    cv = c["in_" + in_src]
    assert slot_value(r["in_amax"]) <= cv.st["B"], "the scale slot is the estimate the bounds assume"
    add = dict(add=c["addt"], add_gate=c["gate"]) if fs == "conv1" else {}
    v, b = cv.finish(3, **add)
    compare(name + " dx", Cn(r["dx"]), v, b, exact)
    if fs == "generic":
        compare(name + " side draw", Cn(r["sd"]), cv.st["a"], cv.st["e"], exact)
        assert torch.equal(Cn(r["sz"]).double(), cv.st["dz"]), "side dz is a select: exact"
    else:
        Bs = slot_value(r["in_amax"])
        dec = R.nchw(decode_pairs(r["sd"].cpu(), sigma_of(r["in_amax"])))
        aa = cv.st["a"].abs() + cv.st["e"]
        compare(name + " pair side draw", dec, cv.st["a"], (cv.st["e"] + 2.0 ** -22 * aa + Bs * R.FLOOR_ABS) * R.SLACK, exact)
        mask = c["mask_o"]["raw" if fs == "conv2" else "act"]
        s0, b0, s1, b1 = R.bnbwd_stats_ref(v, torch.zeros_like(b) if exact else b, c["raw_o"], mask, c["bn4_o"], R.stats_chain(MT, NT))
        assert r["part"].shape[0] == 4 * B * -(-H // TH) * -(-Wd // TW), "one partial row per wave and tile"
        tot = r["part"].double().sum(0).cpu()
        xh = (c["raw_o"].double() - R.v4(c["bn4_o"][0])) * R.v4(c["bn4_o"][1])
        compare_sums(name + " sum dz", tot[:, 0], s0, b0, (v * mask).abs().sum((0, 2, 3)), exact)
        compare_sums(name + " sum dz xhat", tot[:, 1], s1, b1, (v * mask * xh).abs().sum((0, 2, 3)), exact)
    # the absmax slots hold the largest stored magnitudes
    assert slot_value(r["out_amax"]) == float(r["dx"].abs().max())
    side32 = Cn(r["sd"]).double() if fs == "generic" else dec
    assert abs(slot_value(r["side_amax"]) - float(side32.abs().max())) <= 2.0 ** -22 * float(side32.abs().max())


def test_other_launches_keep_their_16_channel_planes(ops, tiling):
    """a fused data gradient at 64 input channels, and one at 32 on a register tile without a whole-pixel instance, do not carry
    the flag; a forced 32-channel plane on a shape the kernel does not have is refused by the entry, not launched"""
    from pytorch_kaldi_resnet_amd import hip
    H, Wd = 5, 7
    for Ci, tile in ((64, (16, 16, 2, 1)), (32, (5, 7, 3, 1))):
        dy, raw = torch.randn(B, H, Wd, Ci, device="cuda"), torch.randn(B, H, Wd, Ci, device="cuda")
        bn4, coef = R.vec_bn4(5, Ci).cuda(), R.vec_coef(9, Ci).cuda()
        wpk_t = ops.pack_conv_weight(torch.randn(Ci, C, 3, 3, device="cuda") * 0.1, transpose=True)
        with patched(ops, SPLIT=3, SPLIT_BWD=None, C32_PLANE=32), forced(tiling.FORCE_CONV_SPLIT, (H, Wd, 1, 3, 3, 9, C), tile), \
                launches(ops) as rec:
            ops.conv_dgrad(dy, wpk_t, C, 3, 1, (H, Wd), in_bnbwd=(raw, None, bn4, coef), side=(torch.empty_like(dy), None))
            torch.cuda.synchronize()
        flags = [a[-6] for n, a, _ in rec if n == "spk_conv_mfma"]
        assert flags and not any(f & CK32_FLAG for f in flags), (Ci, tile, flags)
    # the C entry: the flag without the fused BatchNorm backward
    x = torch.randn(1, 4, 4, 32, device="cuda")
    wpk = ops.pack_conv_weight(torch.randn(32, 32, 3, 3, device="cuda"))
    taps = [(kh - 1, kw - 1, kh * 3 + kw) for kh in range(3) for kw in range(3)]
    ia = ops._iarr
    with pytest.raises(RuntimeError, match="CONV_CK32"):
        hip.call("spk_conv_mfma", x.data_ptr(), wpk.data_ptr(), torch.empty_like(x).data_ptr(), *([None] * 18), 1, 4, 4, 32, 4, 4, 4, 4, 32,
                 1, 1, 0, 0, 9, ia([t[0] for t in taps]), ia([t[1] for t in taps]), ia([t[2] for t in taps]), 4, 4, 2, 1, 1, 1,
                 CK32_FLAG, 3, slot().data_ptr(), None, None, None)
