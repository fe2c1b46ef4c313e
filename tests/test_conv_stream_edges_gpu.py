"""The two streaming convolution kernels (csrc/conv1x1_stream.hip, csrc/conv3x3_c32_stream.hip) on a real MI355X against the
fp64 restatement of tests/conv_ref.py, with the helpers of tests/test_conv_edges_gpu.py: outputs per element (integer inputs
bit for bit), the partial statistics per ROW and in total against the chains read off the two epilogues, the out_amax slot,
guard pixels behind the output, every tail at a tile / row-tile / staging-pass boundary, every grid that leaves blocks uneven
tile counts, every flag combination the 1x1 entry accepts, and one case with operand scales 2^90 apart.  Then the ReLU decisions
the convolutions take themselves - the fused input BatchNorm + ReLU of every kernel form, the recomputed masks of EPI_BNBWD and
IN_BNBWD - on inputs within one rounding of the tie, against the decision of spk_bn_apply.  tests/test_conv_stream_edges_cpu.py
shows without a GPU that the cases plan to these kernels and that the bounds hold for the emulated arithmetic.
The largest error / bound per form is printed when the module finishes: python -m pytest tests/test_conv_stream_edges_gpu.py -m gpu -q -s"""
import contextlib

import pytest
import torch

import bn_stem_ref as BR
import conv_ref as R
from helpers import encode_pairs, sigma_of, slot, slot_value
from test_conv_edges_gpu import (C, G, KINDS, NAN, bits_slot, compare, compare_sums, filled, forced, launches, ops, patched,  # noqa: F401
                                 tiling, vecs)

pytestmark = pytest.mark.gpu

SENTINEL = -77.25          # behind every output: no case stores it
GUARD_PIXELS = 64          # 1x1: more than a row tile behind the last pixel


def stream_launches(rec):
    return [(n, a) for n, a, _ in rec if n.startswith("spk_conv")]


def check_rows(name, st, ref, exact, labels):
    """the partial rows one by one (a row written by the wrong block, or past the tail, shows here and not in the total), then
    their fp64 sum"""
    val, bnd, mag = ref
    got = st.detach().cpu().double()
    assert got.shape == val.shape, "%s: %s partial rows, the planner promised %s" % (name, tuple(got.shape), tuple(val.shape))
    for j, lab in enumerate(labels):
        compare_sums("%s %s rows" % (name, lab), got[:, :, j], val[:, :, j], bnd[:, :, j], mag[:, :, j], exact)
        compare_sums("%s %s" % (name, lab), got.sum(0)[:, j], val.sum(0)[:, j], bnd.sum(0)[:, j], mag.sum(0)[:, j], exact)


# ---- 1. conv1x1_stream_kernel -------------------------------------------------------------------------------------------------
def run_1x1(ops, Cn, P, variant, grid, exact):
    """one launch of a case on a grid of `grid` blocks, through ops.conv_fwd / ops.conv_dgrad where they can express the variant
    and ops._conv_launch where they cannot; every check of the file on it"""
    inp, add, addmask, stats, bnb = variant
    c = R.stream1_case(Cn, P, variant, exact)
    B, H, Wd = c["shape"]
    name = "conv1x1_stream " + ("dgrad" if c["dgrad"] else "fwd") + (" fused input" if inp == "aff" else "") + (" + add" if add else "")
    xg = G(c["x"])
    wpk = ops.pack_conv_weight(c["w"].cuda(), transpose=c["dgrad"])
    ia = vecs(c["ia"]) if c["ia"] is not None else None
    if inp == "pair":        # the f16 pair tensor of x under the slot of its absmax
        amax = ops.absmax_into(xg, slot())
        xin = encode_pairs(R.nhwc(c["x"]), sigma_of(amax)).cuda()
    else:
        amax, xin = ops._amax_fwd_fallback(xg, ia), xg
    buf = torch.full(((P + GUARD_PIXELS) * Cn,), SENTINEL, device="cuda")
    out = buf[:P * Cn].view(B, H, Wd, Cn)
    out.fill_(NAN)
    addg = G(c["add"]) if add else None
    gate = R.sign_bits(c["gate"]).cuda() if addmask else None
    bn = None
    if bnb is not None:
        bn = (G(c["raw"]), None, c["bn4"].cuda()) + ((R.sign_bits(c["mask"]).cuda(),) if bnb == "bits" else ())
    oa = slot()
    with patched(ops, SPLIT=3, SPLIT_BWD=None, STREAM_1X1=True, STREAM_1X1_BLOCKS=grid), launches(ops) as rec:
        if inp != "pair" and bnb is None and not addmask:
            st = ops.conv_fwd(xin, wpk, Cn, 1, 1, in_affine=ia, epi_add=addg, stats=stats, out=out, in_amax=amax, out_amax=oa)[1]
        elif inp != "aff" and (bnb is not None or not stats):
            got = ops.conv_dgrad(xin, wpk, Cn, 1, 1, (H, Wd), add=addg, out=out, bn_bwd=bn, add_mask=gate, in_amax=amax, out_amax=oa,
                                 in_presplit=inp == "pair")
            st = got[1] if bn is not None else None
        else:
            st = ops._conv_launch(xin, wpk, out, Cn, [(0, 0, 0)], 1, 1, 0, 0, H, Wd, ia, None, addg, False, stats, bn, None, None,
                                  split=3, add_mask=gate, in_amax=amax, out_amax=oa, in_presplit=inp == "pair")
        torch.cuda.synchronize()
    (entry, args), = stream_launches(rec)
    want_flags = ((ops.IN_AFFINE_RELU if inp == "aff" else 0) | (ops.IN_PRESPLIT if inp == "pair" else 0) | (ops.EPI_ADD if add else 0)
                  | (ops.EPI_STATS if stats else 0) | (ops.EPI_BNBWD if bnb else 0))
    assert entry == "spk_conv1x1_stream" and (args[11], args[12], args[13], args[16]) == (P, Cn, want_flags, grid), (entry, args[11:17])
    assert (args[6] is not None) == addmask and (args[8] is not None) == (bnb == "bits"), "the mask pointers select the instance"
    assert bool((buf[P * Cn:] == SENTINEL).all()), "%s: a tail row was stored behind the tensor" % name
    compare(name, C(out), *c["out"], exact)            # (a NaN left from the fill fails here: every element is defined)
    assert slot_value(oa) == float(out.abs().max()), "%s: out_amax is not the largest stored magnitude (tail rows?)" % name
    assert (st is not None) == stats
    if stats:
        labels = ("sum dz", "sum dz xhat") if bnb else ("stats sum", "stats sumsq")
        check_rows("conv1x1_stream", st, R.stream1_stats(c, grid, exact), exact, labels)


@pytest.mark.parametrize("variant", R.STREAM1_P_SWEEP, ids=["fwd-affine-stats", "dgrad-pair-add-mask-bnbwd-bits"])
@pytest.mark.parametrize("Cn", R.STREAM1_C)
def test_streaming_1x1_tails_and_grids(ops, Cn, variant):
    """every pixel count at a boundary of the tiling (R.stream1_pixels) on grids of 1, 2 and the tile count"""
    for P in R.stream1_pixels(Cn):
        for grid in R.stream1_grids(P, Cn):
            for exact in KINDS:
                run_1x1(ops, Cn, P, variant, grid, exact)


@pytest.mark.parametrize("inp", ["f32", "aff", "pair"])
@pytest.mark.parametrize("Cn", R.STREAM1_C)
def test_streaming_1x1_every_flag_combination(ops, Cn, inp):
    """the 24 combinations the entry accepts - the five compile-time instances and the generic one for the rest - at two tiles,
    a staging pass and three pixels on two blocks"""
    for variant in R.STREAM1_VARIANTS:
        if variant[0] == inp:
            for exact in KINDS:
                run_1x1(ops, Cn, R.stream1_sweep_pixels(Cn), variant, 2, exact)


# ---- 2. conv3x3_c32_stream_kernel ---------------------------------------------------------------------------------------------
def run_3x3(ops, B, H, Wd, aff, grid, exact):
    c = R.stream3_case(B, H, Wd, aff, exact)
    name = "conv3x3_c32_stream " + ("fused fwd" if aff else "fwd")
    buf = torch.full((B + 1, H, Wd, 32), SENTINEL, device="cuda")
    out = buf[:B]
    out.fill_(NAN)
    oa = slot()
    with patched(ops, SPLIT=3, SPLIT_BWD=None, STREAM_C32=True, STREAM_C32_BLOCKS=grid), launches(ops) as rec:
        st = ops.conv_fwd(G(c["x"]), ops.pack_conv_weight(c["w"].cuda()), 32, 3, 1, in_affine=vecs(c["ia"]) if aff else None, stats=True,
                          out=out, out_amax=oa)[1]
        torch.cuda.synchronize()
    (entry, args), = stream_launches(rec)
    assert entry == "spk_conv3x3_c32_stream" and args[6:10] == (B, H, Wd, ops.EPI_STATS | (ops.IN_AFFINE_RELU if aff else 0)), args[6:10]
    assert args[12] == grid
    assert bool((buf[B] == SENTINEL).all()), "%s: a ragged tile stored behind the tensor" % name
    compare(name, C(out), *c["out"], exact)
    assert slot_value(oa) == float(out.abs().max()), "%s: out_amax is not the largest stored magnitude" % name
    check_rows("conv3x3_c32_stream" + (" fused" if aff else ""), st, R.stream3_stats(c, grid, exact), exact, ("stats sum", "stats sumsq"))


@pytest.mark.parametrize("H,Wd", R.STREAM3_MAPS)
def test_streaming_3x3_maps(ops, H, Wd):
    """maps from one pixel to 4 x 4 tiles, ragged by one pixel and by all but one, one and two images, plain and fused input, on
    the default grid (one block per tile)"""
    for B in R.STREAM3_B:
        for aff in (False, True):
            for exact in KINDS:
                run_3x3(ops, B, H, Wd, aff, R.stream3_tiles(B, H, Wd), exact)


@pytest.mark.parametrize("aff", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("B", R.STREAM3_B)
def test_streaming_3x3_grids_with_uneven_tile_counts(ops, B, aff):
    """16 and 32 tiles on 1, 5, 7, 8, 15, 16, 24 blocks: the two-tiles-in-flight loop with one, two, three and four tiles per
    block, an odd tile left over, and the XCD band permutation on the multiples of 8 - the rows go by the virtual block"""
    H, Wd = R.STREAM3_SWEEP_MAP
    for grid in R.stream3_grids(B, H, Wd):
        for exact in KINDS:
            run_3x3(ops, B, H, Wd, aff, grid, exact)


@pytest.mark.parametrize("k", [1, 3])
def test_operand_scales_far_apart(ops, k):
    """inputs near 2^40 under a slot 2^3 above their maximum, weights near 2^-50: the accumulator is scaled back by two factors
    whose product is far from both; the bound is the one of the slot handed in"""
    B, H, Wd = 2, 9, 13
    x, w, amax, (v, b) = R.far_case(32, H, Wd, k)
    with patched(ops, SPLIT=3, SPLIT_BWD=None, STREAM_1X1=True, STREAM_C32=True), launches(ops) as rec:
        out = ops.conv_fwd(G(x), ops.pack_conv_weight(w.cuda()), 32, k, 1, stats=True, out=filled(B, H, Wd, 32), in_amax=bits_slot(amax))[0]
        torch.cuda.synchronize()
    (entry, _), = stream_launches(rec)
    assert entry == ("spk_conv1x1_stream" if k == 1 else "spk_conv3x3_c32_stream")
    compare("conv%dx%d stream scales far apart" % (k, k), C(out), v, b, False)


# ---- 3. ReLU decisions on near ties, convolution side -------------------------------------------------------------------------
TIE_MAP = (8, 16)          # 128 pixels: pixel p holds row p % 4 of bn_stem_ref.tie_inputs()


def tie_case(Cn):
    """raw, scale, shift, dy of tie_inputs() tiled to Cn channels and to the pixels of TIE_MAP (NHWC, on the card), the identity
    weights, and the decision of spk_bn_apply on exactly these tensors"""
    raw, scale, shift, dy = BR.tie_inputs()
    H, Wd = TIE_MAP
    rep = Cn // 32

    def px(t):
        return t.repeat(H * Wd // 4, rep).reshape(1, H, Wd, Cn).contiguous().cuda()
    return px(raw), scale.repeat(rep).cuda(), shift.repeat(rep).cuda(), px(dy)


def identity(ops, Cn, k, transpose=False):
    w = torch.zeros(Cn, Cn, k, k)
    w[torch.arange(Cn), torch.arange(Cn), k // 2, k // 2] = 1.0
    return ops.pack_conv_weight(w.cuda(), transpose=transpose)


def reference_decision(ops, raw, scale, shift):
    Cn = raw.shape[-1]
    out, mk = ops.bn_apply(raw.view(-1, Cn), scale, shift, relu=True, mask=True)
    pos = out > 0
    assert torch.equal(mk.cpu(), BR.sign_mask_words(out.cpu()))
    assert 0 < int(pos[:3].sum()) < 3 * Cn, "both decisions occur among the near ties"
    return pos.view(raw.shape)


# kernel form -> (channels, ksize, module switches, forced tile or None, statistics, label the launch must carry)
TIE_FORWARD_FORMS = {
    "conv_mfma f32": (32, 3, dict(SPLIT=0), None, False, "conv_mfma_kernel<"),
    "conv_mfma f16x3": (32, 3, dict(SPLIT=3), None, False, "conv_mfma_kernel<"),
    "conv_mfma f16x3 1x1 wide staging": (64, 1, dict(SPLIT=3, STREAM_1X1=False), None, False, "conv_mfma_kernel<"),
    "conv_pipe": (64, 3, dict(SPLIT=3, PIPE_CONV=True, PIPE_M16=False), (8, 16, 2, 1), False, "conv_pipe_kernel<2,1,"),
    "conv1x1_stream": (32, 1, dict(SPLIT=3, STREAM_1X1=True), None, False, "conv1x1_stream_kernel<32>"),
    "conv3x3_c32_stream": (32, 3, dict(SPLIT=3, STREAM_C32=True), None, True, "conv3x3_c32_stream_kernel"),
}


@pytest.mark.parametrize("form", sorted(TIE_FORWARD_FORMS))
def test_fused_input_relu_decides_near_ties_like_bn_apply(ops, tiling, form):
    """IN_AFFINE_RELU staging in front of identity weights (the centre tap of a 3x3): the output is the staged value - 0 or
    about 2^-23, kept apart by a scale slot of 2^-21 that the test owns - and out > 0 must be spk_bn_apply's decision on every
    element"""
    Cn, k, switches, tile, stats, label = TIE_FORWARD_FORMS[form]
    H, Wd = TIE_MAP
    raw, scale, shift, _ = tie_case(Cn)
    pos = reference_decision(ops, raw, scale, shift)
    table = tiling.FORCE_CONV_SPLIT if switches["SPLIT"] else tiling.FORCE_CONV
    key = (H, Wd, 1, k, k, k * k, Cn)
    if tile is not None:
        assert R.tile_violations(*tile, H, Wd, Cn, 1, 3, 3, pipe=True) == []
    with patched(ops, SPLIT_BWD=None, **switches), (forced(table, key, tile) if tile else contextlib.nullcontext()), launches(ops) as rec:
        out = ops.conv_fwd(raw, identity(ops, Cn, k), Cn, k, 1, in_affine=(scale, shift), stats=stats, out=filled(1, H, Wd, Cn),
                           in_amax=bits_slot(2.0 ** -21))[0]
        torch.cuda.synchronize()
    (lab,) = [lb for n, _, lb in rec if n.startswith("spk_conv")]
    assert lab.startswith(label), (lab, label)
    bad = (out > 0) != pos
    assert not bool(bad.any()), "%s: %d of %d ReLU decisions differ from spk_bn_apply's on near ties" % (form, int(bad.sum()), bad.numel())


@pytest.mark.parametrize("form", ["conv_mfma f32", "conv_mfma f16x3", "conv1x1_stream"])
def test_recomputed_mask_of_the_bnbwd_epilogue_decides_near_ties_like_bn_apply(ops, form):
    """EPI_BNBWD without a mask operand: identity weights and integer dy in 1 .. 3, so dx = dy exactly and sum dz per channel
    is the sum of dy over the pixels the kernel decided for: that of spk_bn_apply's pixels, and of bn_bwd_partial(MASK_RAW)"""
    Cn, k = 32, (1 if form == "conv1x1_stream" else 3)
    H, Wd = TIE_MAP
    raw, scale, shift, dy = tie_case(Cn)
    pos = reference_decision(ops, raw, scale, shift)
    bn4 = torch.stack([torch.zeros(Cn), torch.ones(Cn), scale.cpu(), shift.cpu()]).cuda()
    with patched(ops, SPLIT=0 if form.endswith("f32") else 3, SPLIT_BWD=None, STREAM_1X1=True), launches(ops) as rec:
        dx, part = ops.conv_dgrad(dy, identity(ops, Cn, k, transpose=True), Cn, k, 1, (H, Wd), bn_bwd=(raw, None, bn4),
                                  out=filled(1, H, Wd, Cn))
        torch.cuda.synchronize()
    (lab,) = [lb for n, _, lb in rec if n.startswith("spk_conv")]
    assert lab.startswith("conv1x1_stream_kernel" if k == 1 else "conv_mfma_kernel<"), lab
    assert torch.equal(dx, dy)
    want = torch.where(pos, dy, torch.zeros((), device="cuda")).double().sum((0, 1, 2))
    ref = ops.bn_bwd_partial(dy.view(-1, Cn), raw.view(-1, Cn), None, bn4, BR.MASK_RAW).double().sum(0)[:, 0]
    got = part.double().sum(0)[:, 0]
    assert torch.equal(ref, want), "bn_bwd_partial(MASK_RAW) against bn_apply (tests/test_bn_stem_gpu.py pins this)"
    assert torch.equal(got, want), "%s: sum dz differs on %d channels: the recomputed mask rounds another way" % (form, int((got != want).sum()))


@pytest.mark.parametrize("Cn", [32, 64])
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_recomputed_mask_of_the_fused_input_bnbwd_decides_near_ties_like_bn_apply(ops, mode, Cn):
    """IN_BNBWD without a mask operand (conv_mfma_kernel; 32 channels in the f16x3 mode: its whole-pixel staging): the side
    output dz = dy where the kernel decided for the pixel, else 0 - compared exactly"""
    H, Wd = TIE_MAP
    raw, scale, shift, dy = tie_case(Cn)
    pos = reference_decision(ops, raw, scale, shift)
    bn4 = torch.stack([torch.zeros(Cn), torch.ones(Cn), scale.cpu(), shift.cpu()]).cuda()
    coef = torch.stack([torch.ones(Cn), torch.zeros(Cn), torch.zeros(Cn)]).cuda()
    with patched(ops, SPLIT=R.SPLITS[mode], SPLIT_BWD=None), launches(ops) as rec:
        sd, sz = filled(1, H, Wd, Cn), filled(1, H, Wd, Cn)
        ops.conv_dgrad(dy, identity(ops, Cn, 3, transpose=True), Cn, 3, 1, (H, Wd), in_bnbwd=(raw, None, bn4, coef), side=(sd, sz),
                       out=filled(1, H, Wd, Cn))
        torch.cuda.synchronize()
    assert all(lb.startswith("conv_mfma_kernel<") and ",true," in lb for n, _, lb in rec if n == "spk_conv_mfma"), [lb for _, _, lb in rec]
    want = torch.where(pos, dy, torch.zeros((), device="cuda"))
    assert torch.equal(sz, want), "IN_BNBWD %s C=%d: %d of %d recomputed ReLU decisions differ from spk_bn_apply's" % (
        mode, Cn, int((sz != want).sum()), want.numel())
    assert torch.equal(sd, want), "k1 = 1, m1 = m2 = 0: draw is dz"
