"""The convolution kernels (csrc/conv_kernel.h in its conv_mfma / conv_split / conv_pipe instantiations, the 16x16x32 form, and
the conv_wgrad*.hip family) on a real MI355X against the fp64 restatement of tests/conv_ref.py: every compiled register tile,
the default dispatch on shapes outside the model, degenerate maps, the region loop of the weight gradients, and the absmax
hand-offs.  Every case runs with integer inputs (compared bit for bit wherever tests/test_conv_edges_cpu.py proves the partial
sums exact) and with random inputs (per-element bounds derived in conv_ref.py).  The largest error / bound per kernel form is
printed when the module finishes: python -m pytest tests/test_conv_edges_gpu.py -m gpu -q -s"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import conv_ref as R
from helpers import encode_pairs, sigma_of, slot, slot_value

pytestmark = pytest.mark.gpu

NAN = float("nan")
KINDS = [False, True]        # random inputs (bounds), integer inputs (exact)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops as _ops
    yield _ops
    mine = sorted(kv for kv in R.RATIOS.items() if kv[0].startswith("conv"))
    print("\nlargest error / bound per kernel form: " + ", ".join("%s %.3g" % kv for kv in mine))


@pytest.fixture(scope="module")
def tiling(ops):
    from pytorch_kaldi_resnet_amd import tiling as _tiling
    return _tiling


def G(t):
    """NCHW on the CPU -> NHWC on the card"""
    return R.nhwc(t).cuda()


def C(t):
    return R.nchw(t.detach().cpu())


def filled(*shape):
    return torch.full(shape, NAN, device="cuda")


def vecs(pair):
    return tuple(v.cuda() for v in pair)


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
    """pass-through recorder of ops.call: (entry, arguments, label) of every launch"""
    rec, real = [], ops.call

    def call(name, *args, label=None, flops=0.0, nbytes=0.0):
        rec.append((name, args, label))
        return real(name, *args, label=label, flops=flops, nbytes=nbytes)
    ops.call = call
    try:
        yield rec
    finally:
        ops.call = real


def conv_labels(rec):
    return [lab for name, _, lab in rec if name == "spk_conv_mfma"]


def compare(name, got, ref, bound, exact):
    """integer inputs: bit for bit; random inputs: |got - ref| <= bound per element"""
    got = got.detach().cpu().double()
    if exact:
        assert got.shape == ref.shape and torch.equal(got, ref), "%s: integer case not exact (%d of %d elements differ, largest %g)" % (
            name, int((got != ref).sum()), ref.numel(), float((got - ref).abs().max()))
        R.RATIOS.setdefault(name, 0.0)
    else:
        R.check(name, got, ref, bound)


def compare_sums(name, got, ref, bound, abs_sum, exact):
    """a per-channel sum over pixels: exact for integer inputs while the sum of magnitudes stays below 2^24, else its bound"""
    compare(name, got, ref, bound, exact and float(abs_sum.max()) < 2.0 ** 24)


# ---- a. every compiled register tile ------------------------------------------------------------------------------------------
TILE_KEY = R.TILE_MAP + (1, 3, 3, 9, R.TILE_COUT)
CONFIGS = ([("f32", mt, nt, False, False) for mt, nt in R.TILES_F32]
           + [(m, mt, nt, False, False) for m in ("bf16x6", "bf16x9", "f16x3") for mt, nt in R.TILES_SPLIT]
           + [("f16x3", mt, nt, True, False) for mt, nt in R.TILES_PIPE] + [("f16x3", 3, 2, True, True)])


def form_name(mode, pipe, m16):
    return "conv_pipe 16x16x32" if m16 else ("conv_pipe" if pipe else "conv_mfma " + mode)


@functools.lru_cache(maxsize=None)
def tile_case(exact):
    """inputs and fp64 references of the tile sweep (shared by all configurations, never modified): a 64 -> 128 forward, and the
    data gradient of a 128 -> 64 convolution - the launch with the same 64 -> 128 shape and mirrored taps"""
    B, Ci, Co, (H, Wd) = R.TILE_B, R.TILE_CIN, R.TILE_COUT, R.TILE_MAP
    c = {}
    c["x"], c["w"] = R.conv_inputs(101, B, Ci, Co, H, Wd, 3, exact)
    c["ia"], c["ea"] = R.vec_affine(111, Ci, exact), R.vec_affine(113, Co, exact)
    c["res"] = R.tensor(115, exact, B, Co, H, Wd)
    c["wd"] = R.conv_inputs(121, 1, Co, Ci, 1, 1, 3, exact)[1]            # [Ci][Co][3][3]
    c["dy"] = R.tensor(123, exact, B, Ci, H, Wd)
    c["addt"], c["gate"] = R.tensor(124, exact, B, Co, H, Wd), R.tensor(125, exact, B, Co, H, Wd) > 0
    c["plain"] = R.fwd(c["x"], c["w"], 3, 1)
    c["fused"] = R.fwd(c["x"], c["w"], 3, 1, in_affine=c["ia"])
    c["dg"] = R.dgrad1(c["dy"], c["wd"], 3)
    # fused BatchNorm backward while staging dy (IN_BNBWD), and its statistics in the epilogue (EPI_BNBWD)
    c["raw_i"], c["act_i"] = R.tensor(131, exact, B, Ci, H, Wd, scale=2.0, shift=0.3), R.tensor(132, exact, B, Ci, H, Wd)
    c["bn4_i"], c["coef"] = R.vec_bn4(133, Ci, exact), R.vec_coef(137, Ci, exact)
    c["raw_o"], c["act_o"] = R.tensor(141, exact, B, Co, H, Wd, scale=2.0, shift=0.3), R.tensor(142, exact, B, Co, H, Wd)
    c["bn4_o"] = R.vec_bn4(143, Co, exact)
    for src, mask in (("raw", R.mask_from_raw(c["raw_i"], c["bn4_i"][2], c["bn4_i"][3])), ("act", c["act_i"] > 0)):
        c["in_" + src] = R.dgrad1(c["dy"], c["wd"], 3, in_bnbwd=(c["raw_i"], mask, c["bn4_i"], c["coef"]))
    c["mask_o"] = {"raw": R.mask_from_raw(c["raw_o"], c["bn4_o"][2], c["bn4_o"][3]), "act": c["act_o"] > 0}
    assert all(c[k].exact_ok() for k in ("plain", "fused", "dg", "in_raw", "in_act")) or not exact
    return c


@contextlib.contextmanager
def tile_config(ops, tiling, mode, MT, NT, pipe, m16):
    split = R.SPLITS[mode]
    table = tiling.FORCE_CONV_SPLIT if split else tiling.FORCE_CONV
    with patched(ops, SPLIT=split, SPLIT_BWD=None, PIPE_CONV=pipe, PIPE_M16=m16), \
            forced(table, TILE_KEY, R.TILE_OF_MT[MT] + (MT, NT)), launches(ops) as rec:
        yield split, rec
    want = "conv_pipe_kernel<%d,%d," % (MT, NT) if pipe else "conv_mfma_kernel<%d,%d," % (MT, NT)
    labels = conv_labels(rec)
    assert labels and all(lab.startswith(want) for lab in labels), (want, labels)
    assert all(lab.endswith(",true>") == m16 for lab in labels if "false,false" in lab), labels


@pytest.mark.parametrize("exact", KINDS)
@pytest.mark.parametrize("mode,MT,NT,pipe,m16", CONFIGS)
def test_every_register_tile(ops, tiling, mode, MT, NT, pipe, m16, exact):
    """plain forward, forward with statistics, forward with the fused input transform and the full epilogue, stride-1 data
    gradient with add + sign mask - on the forced tile, whose launches are checked to be the kernel form meant"""
    c, name = tile_case(exact), form_name(mode, pipe, m16)
    B, Co, (H, Wd) = R.TILE_B, R.TILE_COUT, R.TILE_MAP
    TH, TW = R.TILE_OF_MT[MT]
    with tile_config(ops, tiling, mode, MT, NT, pipe, m16) as (split, _):
        xg = G(c["x"])
        wpk = ops.pack_conv_weight(c["w"].cuda())
        wpk_t = ops.pack_conv_weight(c["wd"].cuda(), transpose=True)
        out = ops.conv_fwd(xg, wpk, Co, 3, 1, out=filled(B, H, Wd, Co))[0]
        out2, st = ops.conv_fwd(xg, wpk, Co, 3, 1, stats=True, out=filled(B, H, Wd, Co))
        out3 = ops.conv_fwd(xg, wpk, Co, 3, 1, in_affine=vecs(c["ia"]), epi_affine=vecs(c["ea"]), epi_add=G(c["res"]), relu=True,
                            out=filled(B, H, Wd, Co))[0]
        dx = ops.conv_dgrad(G(c["dy"]), wpk_t, Co, 3, 1, (H, Wd), add=G(c["addt"]), add_mask=R.sign_bits(c["gate"]).cuda(),
                            out=filled(B, H, Wd, Co))
        torch.cuda.synchronize()
    v, b = c["plain"].finish(split)
    compare(name + " fwd", C(out), v, b, exact)
    assert torch.equal(out2, out)
    assert st.shape[0] == 4 * B * -(-H // TH) * -(-Wd // TW), "one partial row per wave and tile: the forced tile is the one launched"
    tot = st.double().sum(0).cpu()
    s0, b0, s1, b1 = R.stats_ref(v, torch.zeros_like(b) if exact else b, R.stats_chain(MT, NT))
    compare_sums(name + " stats sum", tot[:, 0], s0, b0, v.abs().sum((0, 2, 3)), exact)
    compare_sums(name + " stats sumsq", tot[:, 1], s1, b1, s1, exact)
    compare(name + " fused fwd", C(out3), *c["fused"].finish(split, epi_affine=c["ea"], add=c["res"], relu=True), exact)
    compare(name + " dgrad add+mask", C(dx), *c["dg"].finish(split, add=c["addt"], add_gate=c["gate"]), exact)


BNBWD_CONFIGS = ([("f32", mt, nt, False) for mt, nt in R.TILES_F32] + [("f16x3", mt, nt, False) for mt, nt in R.TILES_SPLIT]
                 + [("f16x3", mt, nt, True) for mt, nt in R.TILES_PIPE])


@pytest.mark.parametrize("exact", KINDS)
@pytest.mark.parametrize("mode,MT,NT,pipe", BNBWD_CONFIGS)
def test_fused_batchnorm_backward_on_every_register_tile(ops, tiling, mode, MT, NT, pipe, exact):
    """the IN_BNBWD instantiation with both side outputs and EPI_BNBWD, each with its three mask sources (recomputed from the raw
    tensor, an activation tensor, sign bits).  IN_BNBWD stays on conv_mfma_kernel in the default build, so the pipelined
    configurations run EPI_BNBWD only."""
    c, name = tile_case(exact), form_name(mode, pipe, False)
    B, Ci, Co, (H, Wd) = R.TILE_B, R.TILE_CIN, R.TILE_COUT, R.TILE_MAP
    chain = R.stats_chain(MT, NT)
    got = {}
    with tile_config(ops, tiling, mode, MT, NT, pipe, False) as (split, _):
        wpk_t = ops.pack_conv_weight(c["wd"].cuda(), transpose=True)
        dyg, addg = G(c["dy"]), G(c["addt"])
        for src in ("raw", "act", "bits"):
            if not pipe:
                inb = (G(c["raw_i"]), G(c["act_i"]) if src == "act" else None, c["bn4_i"].cuda(), c["coef"].cuda())
                if src == "bits":
                    inb = inb + (R.sign_bits(c["act_i"] > 0).cuda(),)
                sd, sz = filled(B, H, Wd, Ci), filled(B, H, Wd, Ci)
                dx = ops.conv_dgrad(dyg, wpk_t, Co, 3, 1, (H, Wd), add=addg, in_bnbwd=inb, side=(sd, sz), out=filled(B, H, Wd, Co))
                got["in", src] = (dx, sd, sz)
            bnb = (G(c["raw_o"]), G(c["act_o"]) if src == "act" else None, c["bn4_o"].cuda())
            if src == "bits":
                bnb = bnb + (R.sign_bits(c["act_o"] > 0).cuda(),)
            got["epi", src] = ops.conv_dgrad(dyg, wpk_t, Co, 3, 1, (H, Wd), add=addg, bn_bwd=bnb, out=filled(B, H, Wd, Co))
        torch.cuda.synchronize()
    for src in ("raw", "act", "bits"):
        key = "raw" if src == "raw" else "act"
        if not pipe:
            cv = c["in_" + key]
            dx, sd, sz = got["in", src]
            compare(name + " IN_BNBWD dx", C(dx), *cv.finish(split, add=c["addt"]), exact)
            compare(name + " IN_BNBWD side draw", C(sd), cv.st["a"], cv.st["e"], exact)
            assert torch.equal(C(sz).double(), cv.st["dz"]), "side dz is a select: exact"
        dx, part = got["epi", src]
        v, b = c["dg"].finish(split, add=c["addt"])
        compare(name + " EPI_BNBWD dx", C(dx), v, b, exact)
        mask = c["mask_o"][key]
        s0, b0, s1, b1 = R.bnbwd_stats_ref(v, torch.zeros_like(b) if exact else b, c["raw_o"], mask, c["bn4_o"], chain)
        tot = part.double().sum(0).cpu()
        xh = (c["raw_o"].double() - R.v4(c["bn4_o"][0])) * R.v4(c["bn4_o"][1])
        compare_sums(name + " EPI_BNBWD sum dz", tot[:, 0], s0, b0, (v * mask).abs().sum((0, 2, 3)), exact)
        compare_sums(name + " EPI_BNBWD sum dz xhat", tot[:, 1], s1, b1, (v * mask * xh).abs().sum((0, 2, 3)), exact)


@pytest.mark.parametrize("exact", KINDS)
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("Cin,Cout,s,kc", R.ONE_BY_ONE)
def test_single_tap_launches(ops, Cin, Cout, s, kc, mode, exact):
    """1x1 convolutions on the general kernel: kc = 1, 2, 4 channel planes per barrier, and the strided view (ips = 2)"""
    B, (H, Wd) = R.ONE_BY_ONE_B, R.ONE_BY_ONE_MAP
    x, w = R.conv_inputs(201, B, Cin, Cout, H, Wd, 1, exact)
    ia, ea = R.vec_affine(203, Cin, exact), R.vec_affine(205, Cout, exact)
    OH, OW = R.out_hw(H, Wd, 1, s)
    res, dy, addt = R.tensor(207, exact, B, Cout, OH, OW), R.tensor(208, exact, B, Cout, OH, OW), R.tensor(209, exact, B, Cin, H, Wd)
    split, name = R.split_for(mode, 1), "conv_mfma 1x1 " + mode
    with patched(ops, SPLIT=R.SPLITS[mode], SPLIT_BWD=None), launches(ops) as rec:
        xg = G(x)
        wpk, wpk_t = ops.pack_conv_weight(w.cuda()), ops.pack_conv_weight(w.cuda(), transpose=True)
        out, st = ops.conv_fwd(xg, wpk, Cout, 1, s, stats=True, out=filled(B, OH, OW, Cout))
        out3 = ops.conv_fwd(xg, wpk, Cout, 1, s, in_affine=vecs(ia), epi_affine=vecs(ea), epi_add=G(res), relu=True)[0]
        dx = ops.conv_dgrad(G(dy), wpk_t, Cin, 1, s, (H, Wd), add=G(addt))
        torch.cuda.synchronize()
    fwd_args = [a for n, a, _ in rec if n == "spk_conv_mfma"][0]
    assert (fwd_args[-8], fwd_args[-7]) == (kc, s), "kc, ips of the forward launch"
    c = R.fwd(x, w, 1, s)
    v, b = c.finish(split)
    compare(name + " fwd", C(out), v, b, exact)
    compare_sums(name + " stats sum", st.double().sum(0).cpu()[:, 0], v.sum((0, 2, 3)), R.stats_ref(v, b, R.stats_chain(4, 2))[1],
                 v.abs().sum((0, 2, 3)), exact)
    compare(name + " fused fwd", C(out3), *R.fwd(x, w, 1, s, in_affine=ia).finish(split, epi_affine=ea, add=res, relu=True), exact)
    compare(name + " dgrad", C(dx), *R.dgrad(dy, w, 1, s, (H, Wd), split, add=addt)[:2], exact)


@pytest.mark.parametrize("exact", KINDS)
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_single_tap_tile_one_pixel_wide_on_a_wider_map(ops, tiling, mode, exact):
    """A forced (6, 1) tile of a 1x1 convolution on a 6 x 5 map: the halo is one pixel wide, which has no 32-bit reciprocal
    (csrc/conv_mfma.hip stages a second column for it - here real pixels of the neighbouring tile, which no tap reads and which
    the side outputs of a fused BatchNorm backward must not write twice).  Forward, and the IN_BNBWD data gradient with both side
    outputs into NaN-filled tensors."""
    B, Ci, Co, H, Wd = 2, R.TILE_CIN, R.TILE_COUT, 6, 5
    x, w = R.conv_inputs(221, B, Ci, Co, H, Wd, 1, exact)
    wd = R.conv_inputs(223, 1, Co, Ci, 1, 1, 1, exact)[1]               # [Ci][Co][1][1]: dy has Ci channels, dx has Co
    dy, raw = R.tensor(225, exact, B, Ci, H, Wd), R.tensor(226, exact, B, Ci, H, Wd, scale=2.0, shift=0.3)
    bn4, coef = R.vec_bn4(227, Ci, exact), R.vec_coef(231, Ci, exact)
    split, name = R.split_for(mode, 1), "conv_mfma 1x1 TW=1 " + mode
    table = tiling.FORCE_CONV_SPLIT if split else tiling.FORCE_CONV
    assert R.tile_violations(H, 1, 1, 1, H, Wd, Co, 1, 1, split, kc=2) == []
    with patched(ops, SPLIT=R.SPLITS[mode], SPLIT_BWD=None), forced(table, (H, Wd, 1, 1, 1, 1, Co), (H, 1, 1, 1)), launches(ops) as rec:
        out = ops.conv_fwd(G(x), ops.pack_conv_weight(w.cuda()), Co, 1, 1, out=filled(B, H, Wd, Co))[0]
        sd, sz = filled(B, H, Wd, Ci), filled(B, H, Wd, Ci)
        dx = ops.conv_dgrad(G(dy), ops.pack_conv_weight(wd.cuda(), transpose=True), Co, 1, 1, (H, Wd),
                            in_bnbwd=(G(raw), None, bn4.cuda(), coef.cuda()), side=(sd, sz), out=filled(B, H, Wd, Co))
        torch.cuda.synchronize()
    tiles = [a[-12:-8] for n, a, _ in rec if n == "spk_conv_mfma"]
    assert tiles == [(H, 1, 1, 1)] * 2, tiles
    compare(name + " fwd", C(out), *R.fwd(x, w, 1, 1).finish(split), exact)
    cv = R.dgrad1(dy, wd, 1, in_bnbwd=(raw, R.mask_from_raw(raw, bn4[2], bn4[3]), bn4, coef))
    compare(name + " IN_BNBWD dx", C(dx), *cv.finish(split), exact)
    compare(name + " IN_BNBWD side draw", C(sd), cv.st["a"], cv.st["e"], exact)
    assert torch.equal(C(sz).double(), cv.st["dz"])


# ---- b. the default dispatch never refuses a legal shape ----------------------------------------------------------------------
def dispatch_case(ops, Cin, Cout, H, Wd, modes, exact):
    B = R.DISPATCH_B
    x, w = R.conv_inputs(301, B, Cin, Cout, H, Wd, 3, exact)
    ref = R.fwd(x, w, 3, 1)
    for mode in modes:
        with patched(ops, SPLIT=R.SPLITS[mode], SPLIT_BWD=None):
            out = ops.conv_fwd(G(x), ops.pack_conv_weight(w.cuda()), Cout, 3, 1, out=filled(B, H, Wd, Cout))[0]
            torch.cuda.synchronize()
        compare("conv default dispatch " + mode, C(out), *ref.finish(R.SPLITS[mode]), exact)


def test_64_to_32_channels_on_a_9x11_map_in_the_default_mode(ops, tiling):
    """The named regression: tiling hands this shape the (1, 1) register tile, which csrc/conv_pipe.hip does not build; before
    ops.PIPE_TILES the launch carried CONV_PIPE and failed with "unsupported pipelined tile config"."""
    assert tiling.conv_tile(9, 11, 1, 3, 3, 9, 32, split=3)[2:] == (1, 1) and ops.PIPE_CONV
    for exact in KINDS:
        dispatch_case(ops, 64, 32, 9, 11, ["f16x3"], exact)


@pytest.mark.parametrize("H,Wd", R.DISPATCH_MAPS)
def test_default_dispatch_never_refuses_a_legal_shape(ops, H, Wd):
    for Cin in R.DISPATCH_CIN:
        for Cout in R.DISPATCH_COUT:
            for exact in KINDS:
                dispatch_case(ops, Cin, Cout, H, Wd, ("f16x3", "f32"), exact)


# ---- c. degenerate geometry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Wd", R.GEOM_MAPS)
def test_degenerate_maps(ops, H, Wd):
    """forward, data gradient (plain into a NaN-filled tensor - every element must come out defined, also where a stride-2
    parity class is empty - with add, accumulating) and weight gradient on maps down to 1 x 1, in every operand mode"""
    B, Cin, Cout = R.GEOM_B, R.GEOM_CIN, R.GEOM_COUT
    for k in (1, 3):
        for s in (1, 2):
            OH, OW = R.out_hw(H, Wd, k, s)
            for exact in KINDS:
                x, w = R.conv_inputs(401, B, Cin, Cout, H, Wd, k, exact)
                dy, addt = R.tensor(403, exact, B, Cout, OH, OW), R.tensor(404, exact, B, Cin, H, Wd)
                prev = R.tensor(405, exact, Cout, Cin, k, k)
                cf, done = R.fwd(x, w, k, s), set()
                for mode in R.SPLITS:
                    split = R.split_for(mode, k)
                    if split in done:
                        continue
                    done.add(split)
                    name = "conv %dx%d s%d %s" % (k, k, s, R.MODE_OF[split])
                    with patched(ops, SPLIT=R.SPLITS[mode], SPLIT_BWD=None):
                        xg, dyg = G(x), G(dy)
                        wpk, wpk_t = ops.pack_conv_weight(w.cuda()), ops.pack_conv_weight(w.cuda(), transpose=True)
                        out = ops.conv_fwd(xg, wpk, Cout, k, s, out=filled(B, OH, OW, Cout))[0]
                        dx = ops.conv_dgrad(dyg, wpk_t, Cin, k, s, (H, Wd), out=filled(B, H, Wd, Cin))
                        dx2 = ops.conv_dgrad(dyg, wpk_t, Cin, k, s, (H, Wd), add=G(addt), out=filled(B, H, Wd, Cin))
                        dx3 = ops.conv_dgrad(dyg, wpk_t, Cin, k, s, (H, Wd), out=G(addt), accumulate=True)
                        dw = ops.conv_wgrad(xg, dyg, filled(Cout, Cin, k, k), k, s)
                        dw2 = ops.conv_wgrad(xg, dyg, prev.cuda(), k, s, accumulate=True)
                        torch.cuda.synchronize()
                    compare(name + " fwd", C(out), *cf.finish(split), exact)
                    compare(name + " dgrad", C(dx), *R.dgrad(dy, w, k, s, (H, Wd), split)[:2], exact)
                    ref_add = R.dgrad(dy, w, k, s, (H, Wd), split, add=addt)[:2]
                    compare(name + " dgrad add", C(dx2), *ref_add, exact)
                    compare(name + " dgrad accumulate", C(dx3), *ref_add, exact)
                    if k == 1 and s == 2:       # the odd pixels are exactly `add`
                        odd = torch.ones(H, Wd, dtype=torch.bool)
                        odd[::2, ::2] = False
                        assert torch.equal(C(dx2)[:, :, odd], addt[:, :, odd]) and not bool(C(dx)[:, :, odd].any())
                    compare(name + " wgrad", dw.cpu(), *R.wgrad(x, dy, k, s, split)[:2], exact)
                    # accumulate: dw_prev + g within the bound of g alone (+ the one rounding of the addition)
                    compare(name + " wgrad accumulate", dw2.cpu(), *R.wgrad(x, dy, k, s, split, prev=prev)[:2], exact)


# ---- d. weight gradients: the region loop ---------------------------------------------------------------------------------------
def run_wgrad(ops, tiling, fam, tile, target, in_hw, stride, nreg, exact, in_affine=None, prev=None):
    """one weight gradient with the tile forced and the block targets lowered to `target`: the launch must be the family's kernel
    on that tile with min(regions, target) slabs, whatever the stride or the fusion; then the result"""
    mode, k, Cin, Cout, WN, label, pairs = fam
    split = R.split_for(mode, k)
    H, Wd = in_hw
    OH, OW = R.out_hw(H, Wd, k, stride)
    x = R.tensor(501, exact, 1, Cin, H, Wd)
    dy = R.tensor(502, exact, 1, Cout, OH, OW)
    key = (OH, OW, Cin, Cout, k, stride)
    table = tiling.FORCE_WGRAD_C32M16 if "c32m16" in label else (tiling.FORCE_WGRAD_SPLIT if split else tiling.FORCE_WGRAD)
    with patched(ops, SPLIT=R.SPLITS[mode], SPLIT_BWD=None, GROUPED_1X1_BLOCKS=target), patched(tiling, WGRAD_TARGET_BLOCKS=target), \
            forced(table, key, tile + (WN,)), launches(ops) as rec:
        xg, dyg, kw = G(x), G(dy), {}
        if pairs:
            kw["dy_amax"] = ops.absmax_into(dyg, slot())
            dyg = encode_pairs(R.nhwc(dy), sigma_of(kw["dy_amax"])).cuda()
            kw["dy_presplit"] = True
        dw = filled(Cout, Cin, k, k) if prev is None else prev.cuda()
        ops.conv_wgrad(xg, dyg, dw, k, stride, in_affine=None if in_affine is None else vecs(in_affine), accumulate=prev is not None, **kw)
        torch.cuda.synchronize()
    (args, lab), = [(a, lb) for n, a, lb in rec if n == "spk_conv_wgrad"]
    nsplit = min(nreg, target)
    assert -(-OH // tile[0]) * -(-OW // tile[1]) == nreg and args[15:19] == tile + (WN, nsplit), (args[15:19], tile, WN, nsplit)
    assert lab.startswith(label), (lab, label)
    name = "conv_wgrad " + label.split("<")[0].replace("conv_wgrad_", "").replace("kernel", mode) + (" WN=%d" % WN if mode == "f32" else "")
    compare(name, dw.cpu(), *R.wgrad(x, dy, k, stride, split, in_affine=in_affine, prev=prev)[:2], exact)


@pytest.mark.parametrize("exact", KINDS)
@pytest.mark.parametrize("fam", R.WG_FAMILIES, ids=lambda f: "%s-%s" % (f[5].split("<")[0], f[0]) + ("-WN%d" % f[4] if f[0] == "f32" else "") + ("-C%d" % f[2] if f[1] == 1 else ""))
def test_weight_gradient_region_loop(ops, tiling, fam, exact):
    """nsplit = 1, 2, 3 slabs over 3 and 7 pixel regions: a block walks 1 .. 7 regions, prefetching the next while it reduces
    this one, with a remainder where nsplit does not divide the regions, and a single slab goes through spk_wgrad_reduce.  Then
    on the 7-region tile with 2 slabs: stride 2, the fused input transform, accumulate = dw_prev + g, and a map of 15 pixels
    (most of a k-step is padding)."""
    mode, k, Cin, Cout = fam[:4]
    for tile, target, in_hw, stride, nreg in R.wgrad_runs():
        run_wgrad(ops, tiling, fam, tile, target, in_hw, stride, nreg, exact)
    tile, nreg = R.WG_TILES[1]
    run_wgrad(ops, tiling, fam, tile, 2, R.WG_MAP, 1, nreg, exact, in_affine=R.vec_affine(511, Cin, exact))
    run_wgrad(ops, tiling, fam, tile, 2, R.WG_MAP, 1, nreg, exact, prev=R.tensor(513, exact, Cout, Cin, k, k))


# ---- e. hand-offs and locality ------------------------------------------------------------------------------------------------
def bits_slot(value):
    return torch.from_numpy(np.array([value], dtype=np.float32).view(np.int32).copy()).cuda()


NAN_STAGED_AS = -65504.0      # v_med3_f32(NaN, -65504, 65504) = min of the other two (split2h, csrc/spk_common.h)


def finite_absmax(t):
    a = t.abs()
    return float(a[torch.isfinite(a)].max())


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_absmax_handoffs_hold_exactly_the_largest_stored_magnitude(ops, mode):
    """out_amax / side_amax: the float bits of max|stored tensor| (max is order-independent: exact); a slot already above keeps
    its value"""
    B, Cin, Cout, H, Wd = 2, 64, 64, 9, 11
    x, w = R.conv_inputs(601, B, Cin, Cout, H, Wd, 3)
    dy, raw = R.rnd(603, B, Cout, H, Wd), R.rnd(604, B, Cout, H, Wd, scale=2.0, shift=0.3)
    bn4, coef = R.vec_bn4(605, Cout), R.vec_coef(609, Cout)
    with patched(ops, SPLIT=R.SPLITS[mode], SPLIT_BWD=None):
        wpk, wpk_t = ops.pack_conv_weight(w.cuda()), ops.pack_conv_weight(w.cuda(), transpose=True)
        s1, big = slot(), bits_slot(1e30)
        out = ops.conv_fwd(G(x), wpk, Cout, 3, 1, out_amax=s1)[0]
        ops.conv_fwd(G(x), wpk, Cout, 3, 1, out_amax=big)
        s2, s3 = slot(), slot()
        sd = filled(B, H, Wd, Cout)
        dx = ops.conv_dgrad(G(dy), wpk_t, Cin, 3, 1, (H, Wd), in_bnbwd=(G(raw), None, bn4.cuda(), coef.cuda()), side=(sd, None),
                            out_amax=s2, side_amax=s3)
        torch.cuda.synchronize()
    assert slot_value(s1) == float(out.abs().max()) and slot_value(big) == float(np.float32(1e30))
    assert slot_value(s2) == float(dx.abs().max()) and slot_value(s3) == float(sd.abs().max())


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_non_finite_inputs_stay_local_and_out_of_the_slots(ops, mode):
    """One inf and one NaN planted in the input: every output outside their two 3x3 receptive fields is bit-identical to the
    clean run, and the out_amax slot holds the largest FINITE stored magnitude (the hand-offs leave
    non-finite values out - an inf in the slot would turn the operand scale of the whole tensor into 1).  This test found the
    convolution epilogues taking fabsf of what they store into the slot, infinities included.
    Inside the receptive fields the f32 mode stores non-finite values, as the reference would.  The f16x3 mode does NOT, and that
    is deliberate (csrc/spk_common.h, split2h: the scaled operand is saturated to the fp16 range by a median-of-three while it
    is split): an inf operand is staged as +-65504 / sigma, and a NaN operand - the median instruction answers a NaN with the
    smallest of its other two operands - as -65504 / sigma.  Both are pinned here: the run with the inf alone and the run with
    the NaN alone equal, bit for bit, the clean run with that finite value in the same place, so every output inside the two
    receptive fields of the combined run is finite and differs from the clean run.  (the tensors these
    kernels stage get their non-finite values masked before a convolution reads them; a NaN that did reach one would not show.)"""
    B, Cin, Cout, H, Wd = 2, 64, 64, 9, 11
    x, w = R.conv_inputs(611, B, Cin, Cout, H, Wd, 3)
    spots = [(0, 7, 2, 3, float("inf")), (1, 40, 6, 8, NAN)]
    inside = torch.zeros(B, H, Wd, dtype=torch.bool)
    xb = x.clone()
    for b, c, y, xx, val in spots:
        xb[b, c, y, xx] = val
        inside[b, y - 1:y + 2, xx - 1:xx + 2] = True
    with patched(ops, SPLIT=R.SPLITS[mode], SPLIT_BWD=None):
        wpk = ops.pack_conv_weight(w.cuda())
        amax = ops.absmax_into(G(x), slot())         # the scale of the clean tensor, for every run
        s0, s1 = slot(), slot()
        clean = ops.conv_fwd(G(x), wpk, Cout, 3, 1, in_amax=amax, out_amax=s0)[0].cpu()
        bad = ops.conv_fwd(G(xb), wpk, Cout, 3, 1, in_amax=amax, out_amax=s1)[0].cpu()
        pinned = []
        if mode == "f16x3":
            for (b, c, y, xx, val), staged in zip(spots, (65504.0, NAN_STAGED_AS)):
                xi, xs = x.clone(), x.clone()
                xi[b, c, y, xx], xs[b, c, y, xx] = val, staged / sigma_of(amax)
                pinned.append([ops.conv_fwd(G(t), wpk, Cout, 3, 1, in_amax=amax)[0].cpu() for t in (xi, xs)])
        torch.cuda.synchronize()
    assert torch.equal(bad[~inside].view(torch.int32), clean[~inside].view(torch.int32)), "outputs outside the receptive fields changed"
    assert slot_value(s0) == float(clean.abs().max())
    assert slot_value(s1) == finite_absmax(bad), "a stored non-finite value reached the slot"
    if mode == "f32":
        assert not bool(torch.isfinite(bad[inside]).any()), "outputs inside the receptive fields must be non-finite"
    else:
        for got, want in pinned:
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "a non-finite operand is staged as the pinned finite value"
        assert bool(torch.isfinite(bad[inside]).all()) and bool((bad[inside] != clean[inside]).any(-1).all())


@pytest.mark.parametrize("Cin,Cout,k,stats", [(64, 64, 3, False), (32, 32, 3, True), (64, 64, 1, False)],
                         ids=["general-or-pipelined", "conv3x3_c32_stream", "conv1x1_stream"])
def test_overflowing_outputs_stay_out_of_the_slot_in_the_f16x3_kernels(ops, Cin, Cout, k, stats):
    """The f16x3-only forms (pipelined kernel, the two streaming kernels) never see an inf operand (split2h saturates), but a
    finite 2^100 times weights of up to 0.2 * 2^31 overflows in about a third of the outputs it reaches when the accumulator is
    scaled back: those are stored as inf, and the slot still holds the largest finite stored magnitude."""
    B, H, Wd = 2, 9, 11
    x, w = R.conv_inputs(621, B, Cin, Cout, H, Wd, k)
    x[1, 9, 4, 5] = 2.0 ** 100
    w[:, 9] *= 2.0 ** 31
    with patched(ops, SPLIT=R.SPLITS["f16x3"], SPLIT_BWD=None), launches(ops) as rec:
        s1 = slot()
        out = ops.conv_fwd(G(x), ops.pack_conv_weight(w.cuda()), Cout, k, 1, stats=stats, out_amax=s1)[0].cpu()
        torch.cuda.synchronize()
    names = [n for n, _, _ in rec if n.startswith("spk_conv")]
    assert names == ["spk_conv3x3_c32_stream" if stats else ("spk_conv1x1_stream" if k == 1 else "spk_conv_mfma")], names
    assert bool(torch.isinf(out).any()) and finite_absmax(out) > 0, "the case needs stored infinities next to finite values"
    assert slot_value(s1) == finite_absmax(out), "a stored non-finite value reached the slot"
