"""tests/conv_ref.py against torch on the CPU: the fp64 restatement of the tap-table convolution agrees with F.conv2d and
autograd in float64 (1e-12 relative) on every case tests/test_conv_edges_gpu.py runs, float32 torch stays inside the `f32` bound
everywhere, the emulation of every operand mode stays inside that mode's representation term, the integer inputs are exact
under every emulation with every partial sum below 2^24, and the register tiles the GPU file forces satisfy the limits the C
ABI states (a wrong table entry fails here, not on a card)."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

REL = 1e-12
MODES = ["f32", "bf16x6", "bf16x9", "f16x3"]


def close(got, ref, what):
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= REL * max(scale, 1e-300), what


def autograd_refs(x, w, k, s):
    """F.conv2d and its two gradients under a seeded dy, in float64"""
    pad = 1 if k == 3 else 0
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(xr, wr, None, s, pad)
    dy = R.rnd(77, *y.shape)
    gx, gw = torch.autograd.grad((y * dy.double()).sum(), [xr, wr])
    return y.detach(), dy, gx, gw


def geom_cases():
    for H, Wd in R.GEOM_MAPS:
        for k in (1, 3):
            for s in (1, 2):
                yield H, Wd, k, s


def all_shapes():
    """(B, Cin, Cout, H, W, k, s) of every case of the GPU file"""
    yield (R.TILE_B, R.TILE_CIN, R.TILE_COUT) + R.TILE_MAP + (3, 1)
    for H, Wd, k, s in geom_cases():
        yield (R.GEOM_B, R.GEOM_CIN, R.GEOM_COUT, H, Wd, k, s)
    for Cin, Cout, s, _ in R.ONE_BY_ONE:
        yield (R.ONE_BY_ONE_B, Cin, Cout) + R.ONE_BY_ONE_MAP + (1, s)
    for H, Wd in R.DISPATCH_MAPS:
        for Cin in R.DISPATCH_CIN:
            for Cout in R.DISPATCH_COUT:
                yield (R.DISPATCH_B, Cin, Cout, H, Wd, 3, 1)


def test_restatement_agrees_with_conv2d_and_autograd_in_float64():
    for B, Cin, Cout, H, Wd, k, s in all_shapes():
        x, w = R.conv_inputs(11, B, Cin, Cout, H, Wd, k)
        y, dy, gx, gw = autograd_refs(x, w, k, s)
        tag = (B, Cin, Cout, H, Wd, k, s)
        close(R.fwd(x, w, k, s).acc, y, ("fwd",) + tag)
        close(R.dgrad(dy, w, k, s, (H, Wd), 0)[0], gx, ("dgrad",) + tag)
        addt = R.rnd(78, B, Cin, H, Wd)
        dx, _, _ = R.dgrad(dy, w, k, s, (H, Wd), 0, add=addt)
        close(dx, gx + addt.double(), ("dgrad + add",) + tag)
        if s == 2 and k == 1:        # the odd pixels of a strided 1x1 data gradient are exactly `add`
            odd = torch.ones(H, Wd, dtype=torch.bool)
            odd[::2, ::2] = False
            assert torch.equal(dx[:, :, odd], addt.double()[:, :, odd])
        close(R.wgrad(x, dy, k, s, 0)[0], gw, ("wgrad",) + tag)
        prev = R.rnd(79, Cout, Cin, k, k)
        close(R.wgrad(x, dy, k, s, 0, prev=prev)[0], gw + prev.double(), ("wgrad accumulate",) + tag)


def fused_forward(x, w, k, s, exact):
    """the fused forward of the GPU file: input relu(x scale + shift), epilogue affine + add + ReLU"""
    B, Cin = x.shape[:2]
    Cout = w.shape[0]
    OH, OW = R.out_hw(x.shape[2], x.shape[3], k, s)
    ia, ea = R.vec_affine(21, Cin, exact), R.vec_affine(23, Cout, exact)
    res = R.tensor(25, exact, B, Cout, OH, OW)
    return ia, ea, res


@pytest.mark.parametrize("exact", [False, True])
def test_fused_forms_agree_with_torch_in_float64(exact):
    B, Cin, Cout, (H, Wd) = R.TILE_B, R.TILE_CIN, R.TILE_COUT, R.TILE_MAP
    for k, s in ((3, 1), (3, 2), (1, 1), (1, 2)):
        x, w = R.conv_inputs(12, B, Cin, Cout, H, Wd, k, exact)
        pad = 1 if k == 3 else 0
        ia, ea, res = fused_forward(x, w, k, s, exact)
        c = R.fwd(x, w, k, s, in_affine=ia)
        v, b = c.finish(0, epi_affine=ea, add=res, relu=True)
        xa = torch.relu(x.double() * R.v4(ia[0]) + R.v4(ia[1]))
        ref = torch.relu(F.conv2d(xa, w.double(), None, s, pad) * R.v4(ea[0]) + R.v4(ea[1]) + res.double())
        close(v, ref, ("fused fwd", k, s))
        # float32 torch with the same fusions stays inside the f32 bound
        x32 = torch.relu(x * ia[0].view(1, -1, 1, 1) + ia[1].view(1, -1, 1, 1))
        y32 = torch.relu(F.conv2d(x32, w, None, s, pad) * ea[0].view(1, -1, 1, 1) + ea[1].view(1, -1, 1, 1) + res)
        R.check("cpu fused fwd", y32, v, b)
        # statistics of the stored tensor
        s0, b0, s1, b1 = R.stats_ref(v, b, R.stats_chain(4, 2))
        close(s0, ref.sum((0, 2, 3)), "stats sum")
        close(s1, (ref * ref).sum((0, 2, 3)), "stats sumsq")
        assert bool((b0 >= 0).all()) and bool((b1 >= 0).all())
        # weight gradient with the fused input transform
        dy = R.tensor(26, exact, *ref.shape)
        gw_ref = torch.nn.grad.conv2d_weight(xa, w.shape, dy.double(), stride=s, padding=pad)
        g, gb, ok = R.wgrad(x, dy, k, s, 0, in_affine=ia)
        close(g, gw_ref, ("wgrad fused", k, s))
        g32 = torch.nn.grad.conv2d_weight(x32, w.shape, dy, stride=s, padding=pad)
        R.check("cpu wgrad fused", g32, g, gb)
        if exact:
            assert c.exact_ok() and ok
            assert torch.equal(y32.double(), v) and torch.equal(g32.double(), g)


def bnbwd_inputs(B, C, H, Wd, exact, seed=31):
    """raw, act, bn4, coef of a fused BatchNorm backward on a [B][C][H][W] tensor"""
    raw = R.tensor(seed, exact, B, C, H, Wd, scale=2.0, shift=0.3)
    act = R.tensor(seed + 1, exact, B, C, H, Wd)
    return raw, act, R.vec_bn4(seed + 2, C, exact), R.vec_coef(seed + 6, C, exact)


@pytest.mark.parametrize("exact", [False, True])
def test_fused_batchnorm_backward_forms_agree_with_torch_in_float64(exact):
    # (the data gradient of a 128 -> 64 convolution: the launch has the 64 -> 128 shape of the tile sweep)
    B, Cl, Ck, (H, Wd) = R.TILE_B, R.TILE_COUT, R.TILE_CIN, R.TILE_MAP
    x, w = R.conv_inputs(13, B, Cl, Ck, H, Wd, 3, exact)        # w [Ck][Cl][3][3]: dy has Ck channels, dx has Cl
    dy = R.tensor(14, exact, B, Ck, H, Wd)
    # IN_BNBWD: the staged value is the BatchNorm backward of dy, with its side outputs
    raw, act, bn4, coef = bnbwd_inputs(B, Ck, H, Wd, exact)
    for mask in (R.mask_from_raw(raw, bn4[2], bn4[3]), act > 0):
        c = R.dgrad1(dy, w, 3, in_bnbwd=(raw, mask, bn4, coef))
        dz = dy.double() * mask
        xh = (raw.double() - R.v4(bn4[0])) * R.v4(bn4[1])
        draw = R.v4(coef[0]) * (dz - R.v4(coef[1]) - xh * R.v4(coef[2]))
        close(c.st["a"], draw, "side draw")
        assert torch.equal(c.st["dz"], dz)
        xr = x.double().requires_grad_(True)
        gx, = torch.autograd.grad(F.conv2d(xr, w.double(), None, 1, 1), [xr], grad_outputs=draw)
        close(c.acc, gx, "dgrad IN_BNBWD")
        d32 = coef[0].view(1, -1, 1, 1) * (dy * mask - coef[1].view(1, -1, 1, 1)
                                           - ((raw - bn4[0].view(1, -1, 1, 1)) * bn4[1].view(1, -1, 1, 1)) * coef[2].view(1, -1, 1, 1))
        R.check("cpu side draw", d32, c.st["a"], c.st["e"])
        xr32 = x.clone().requires_grad_(True)
        g32, = torch.autograd.grad(F.conv2d(xr32, w, None, 1, 1), [xr32], grad_outputs=d32)
        R.check("cpu dgrad IN_BNBWD", g32, *c.finish(0))
        if exact:
            assert c.exact_ok() and torch.equal(g32.double(), c.acc) and torch.equal(d32.double(), draw)
    # EPI_BNBWD: the statistics of the BatchNorm backward of dx, masked add in front
    raw, act, bn4, _ = bnbwd_inputs(B, Cl, H, Wd, exact, seed=41)
    addt, gate = R.tensor(49, exact, B, Cl, H, Wd), R.tensor(50, exact, B, Cl, H, Wd) > 0
    c = R.dgrad1(dy, w, 3)
    v, b = c.finish(0, add=addt, add_gate=gate)
    xr = x.double().requires_grad_(True)
    gx, = torch.autograd.grad(F.conv2d(xr, w.double(), None, 1, 1), [xr], grad_outputs=dy.double())
    close(v, gx + addt.double() * gate, "dgrad + masked add")
    for mask in (R.mask_from_raw(raw, bn4[2], bn4[3]), act > 0):
        s0, b0, s1, b1 = R.bnbwd_stats_ref(v, b, raw, mask, bn4, R.stats_chain(4, 2))
        dz = v * mask
        close(s0, dz.sum((0, 2, 3)), "sum dz")
        close(s1, (dz * (raw.double() - R.v4(bn4[0])) * R.v4(bn4[1])).sum((0, 2, 3)), "sum dz xhat")
        assert bool((b0 >= 0).all()) and bool((b1 >= 0).all())
        if exact:        # sum dz is exact; sum dz xhat too while its absolute sum stays below 2^24
            assert float(dz.abs().sum((0, 2, 3)).max()) < 2.0 ** 24


def test_float32_torch_stays_inside_the_f32_bound():
    for B, Cin, Cout, H, Wd, k, s in all_shapes():
        x, w = R.conv_inputs(15, B, Cin, Cout, H, Wd, k)
        pad = 1 if k == 3 else 0
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = F.conv2d(xr, wr, None, s, pad)
        dy = R.rnd(77, *y.shape)
        gx, gw = torch.autograd.grad((y * dy).sum(), [xr, wr])
        R.check("cpu fwd", y.detach(), *R.fwd(x, w, k, s).finish(0))
        R.check("cpu dgrad", gx, *R.dgrad(dy, w, k, s, (H, Wd), 0)[:2])
        R.check("cpu wgrad", gw, *R.wgrad(x, dy, k, s, 0)[:2])


def small_shapes():
    yield (R.TILE_B, R.TILE_CIN, R.TILE_COUT) + R.TILE_MAP + (3, 1)
    for H, Wd, k, s in geom_cases():
        yield (R.GEOM_B, R.GEOM_CIN, R.GEOM_COUT, H, Wd, k, s)
    for Cin, Cout, s, _ in R.ONE_BY_ONE:
        yield (R.ONE_BY_ONE_B, Cin, Cout) + R.ONE_BY_ONE_MAP + (1, s)


@pytest.mark.parametrize("mode", MODES)
def test_mode_emulations_stay_inside_their_representation_terms(mode):
    """sum of the kept cross terms in fp64 against the exact sum: within rep_term alone (no accumulation term; 2^-50 of S for the
    fp64 arithmetic of the emulation itself)"""
    split = R.SPLITS[mode]
    for B, Cin, Cout, H, Wd, k, s in small_shapes():
        x, w = R.conv_inputs(16, B, Cin, Cout, H, Wd, k)
        c = R.fwd(x, w, k, s)
        w3 = w.reshape(Cout, Cin, k * k)
        if split in (6, 9):
            assert not bool(R.bf16_terms(x)[1].any()) and not bool(R.bf16_terms(w)[1].any()), "three bf16 terms are exact"
        got = R.emulate(c.bil, x, w3, split)
        rep = R.rep_term(split, c.S, c.bil, c.a_abs, c.w.abs(), c.st["B"], float(w.abs().max()))
        R.check("emulation " + mode, got, c.acc, rep + 2.0 ** -50 * c.S)
        if split == 6:       # the six-term form differs from the nine-term form: the bound is not vacuous
            assert float((got - c.acc).abs().max()) > 0 or k == 1
        dy = R.rnd(77, *c.acc.shape)
        g, _, _ = R.wgrad(x, dy, k, s, 0)

        def bil(p, q):
            return R.wgrad(p.float(), q.float(), k, s, 0)[0]
        if (H, Wd) != R.TILE_MAP:
            continue
        # weight gradient: the operands are x and dy; the emulated terms are float32-representable, so bil's casts are exact
        gb = R.rep_term(split, R.wgrad(x.abs(), dy.abs(), k, s, 0)[0], bil, x.double().abs(), dy.double().abs(),
                        float(x.abs().max()), float(dy.abs().max()))
        R.check("emulation wgrad " + mode, R.emulate(bil, x, dy, split), g, gb + 2.0 ** -50 * g.abs().max())


@pytest.mark.parametrize("mode", MODES)
def test_integer_inputs_are_exact_under_every_emulation(mode):
    """x in -2 .. 2 and w in -1 .. 1 have one term in every mode (the others are 0), every product is an integer and every partial
    sum stays below sum|a w| < 2^24: a float32 accumulator holds each of them exactly, in any order"""
    split = R.SPLITS[mode]
    for B, Cin, Cout, H, Wd, k, s in all_shapes():
        x, w = R.conv_inputs(17, B, Cin, Cout, H, Wd, k, exact=True)
        c = R.fwd(x, w, k, s)
        assert c.exact_ok(), (Cin, Cout, H, Wd, k, s, float(c.S.max()))
        assert torch.equal(R.emulate(c.bil, x, w.reshape(Cout, Cin, k * k), split), c.acc)
        assert float(c.acc_bound(split).max()) > 0          # (the bound is still there: the GPU file checks `==` instead)
        if split == 3:
            t = R.f16_terms(x, 2.0)
            assert torch.equal(t[0], x.double()) and not bool(t[1].any())
        elif split:
            t = R.bf16_terms(x)[0]
            assert torch.equal(t[0], x.double()) and not bool(t[1].any()) and not bool(t[2].any())
        dy = R.ints(18, -2, 2, *c.acc.shape)
        for add in (None, R.ints(19, -2, 2, B, Cin, H, Wd)):
            assert R.dgrad(dy, w, k, s, (H, Wd), split, add=add)[2]
        assert R.wgrad(x, dy, k, s, split, prev=R.ints(20, -2, 2, Cout, Cin, k, k))[2]
        # statistics: the sum of the stored values is exact; the sum of squares where it stays below 2^24 (else: its bound)
        assert float(c.acc.abs().sum((0, 2, 3)).max()) < 2.0 ** 24


def test_forced_tiles_satisfy_the_c_abi():
    OH, OW = R.TILE_MAP
    for split, tiles in ((0, R.TILES_F32), (6, R.TILES_SPLIT), (9, R.TILES_SPLIT), (3, R.TILES_SPLIT)):
        for MT, NT in tiles:
            TH, TW = R.TILE_OF_MT[MT]
            assert R.tile_violations(TH, TW, MT, NT, OH, OW, R.TILE_COUT, 1, 3, split) == [], (split, MT, NT)
            assert TH * TW > (4 * MT - 1) * 32 and OH % TH and OW % TW, "last m-tile of the last wave works; ragged on both axes"
            assert TH < OH and TW < OW, "more than one tile per axis"
    for MT, NT in R.TILES_PIPE:
        TH, TW = R.TILE_OF_MT[MT]
        assert R.tile_violations(TH, TW, MT, NT, OH, OW, R.TILE_COUT, 1, 3, 3, pipe=True, m16=(MT, NT) == (3, 2)) == []
        assert (2 * (TH + 2) * (TW + 2) + 1) * 80 <= 80 * 1024, "within the default PIPE_MAX_LDS: nothing to raise"
    assert sorted(R.TILES_PIPE) == sorted(t for t in R.TILES_SPLIT if t not in ((1, 1), (4, 1)))
    # single-tap launches: the kc planes of the whole map fit
    for Cin, Cout, s, kc in R.ONE_BY_ONE:
        assert kc == next((c for c in (4, 2) if Cin % (32 * c) == 0), 1)
    # a tile the chooser may return but the pipelined translation unit does not build: the dispatch regression of the GPU file
    assert R.tile_violations(9, 11, 1, 1, 9, 11, 32, 1, 3, 3, pipe=True) == ["pipelined form"]
    assert R.tile_violations(9, 11, 1, 1, 9, 11, 32, 1, 3, 3) == []


def test_default_chooser_returns_tiles_outside_the_pipelined_set():
    """tiling._conv_tile hands a 9 x 11 map with 32 output channels the (1, 1) register tile - legal for conv_mfma_kernel, not
    instantiated by conv_pipe.hip - and ops._conv_launch must keep such a launch off the pipelined kernel (PIPE_TILES)."""
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops, tiling
    assert tiling._conv_tile(9, 11, 1, 3, 3, 9, 32) == (9, 11, 1, 1)
    assert sorted(ops.PIPE_TILES) == sorted(R.TILES_PIPE)
    src = open(ops.__file__.replace("ops.py", "csrc/conv_pipe.hip")).read()
    built = src.split("spk_launch_conv_pipe(")[1]
    assert sorted(ops.PIPE_TILES) == sorted((int(m), int(n)) for m, n in __import__("re").findall(r"CASE\((\d), (\d)\)", built))
    # the plan of that launch (64 input channels: PIPE_MIN_CIN is not what decides it) stays on conv_mfma_kernel
    p = ops._plan_conv(1, 9, 11, 64, 9, 11, 9, 11, 32, ops.FWD_TAPS, 1, 1, 0, 0, 3, False)
    assert ops.PIPE_CONV and 64 >= ops.PIPE_MIN_CIN and (p.TH, p.TW, p.MT, p.NT) == (9, 11, 1, 1)
    assert not p.flags & ops.CONV_PIPE and p.label.startswith("conv_mfma_kernel<1,1,"), p


def test_forced_weight_gradient_tiles_satisfy_the_c_abi_and_the_restatement_covers_their_shapes():
    """every (family, tile, map, stride) the GPU file launches: within the limits of spk_conv_wgrad and of the family's launcher,
    the region count the GPU file expects, and the restatement against autograd in float64 on exactly these shapes"""
    seen = set()
    for fam in R.WG_FAMILIES:
        mode, k, Cin, Cout, WN, label, pairs = fam
        for tile, target, (H, Wd), stride, nreg in R.wgrad_runs():
            assert R.wgrad_tile_violations(fam, tile, (H, Wd), stride) == [], (label, tile, stride)
            OH, OW = R.out_hw(H, Wd, k, stride)
            assert -(-OH // tile[0]) * -(-OW // tile[1]) == nreg
            assert (Cin // (32 * (int(label[-2]) if "1x1" in label else 2 if "wm" in label else 1))) * (Cout // (32 * WN)) == 1, "one block per slab"
            if (k, Cin, Cout, H, Wd, stride) in seen:
                continue
            seen.add((k, Cin, Cout, H, Wd, stride))
            for exact in (False, True):
                x, dy = R.tensor(501, exact, 1, Cin, H, Wd), R.tensor(502, exact, 1, Cout, OH, OW)
                ref = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, k, k), dy.double(), stride=stride, padding=1 if k == 3 else 0)
                g, b, ok = R.wgrad(x, dy, k, stride, 0)
                close(g, ref, ("wgrad", k, Cin, Cout, H, Wd, stride))
                g32 = torch.nn.grad.conv2d_weight(x, (Cout, Cin, k, k), dy, stride=stride, padding=1 if k == 3 else 0)
                R.check("cpu wgrad region shapes", g32, g, b)
                assert ok and torch.equal(g32.double(), g) or not exact
    # the limits bite: a tile one pixel too wide for the prefetch windows, and an odd width
    assert R.wgrad_tile_violations(R.WG_FAMILIES[2], (4, 10), R.WG_MAP, 1) and R.wgrad_tile_violations(R.WG_FAMILIES[0], (4, 3), R.WG_MAP, 1)
