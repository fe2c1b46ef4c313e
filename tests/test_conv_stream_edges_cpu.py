"""The cases tests/test_conv_stream_edges_gpu.py runs on the two streaming convolution kernels, checked without a GPU: every
case plans (ops._plan_conv) to the streaming entry with the grid and the statistics rows the reference partitions the pixels
into - and to spk_conv_mfma with the module switch off; the numpy emulation of the f16x3 operands, stored as float32 and summed
into float32 rows, stays inside the bounds the kernels will be held to (outputs per element, statistics per row); every integer
case is exact with every sum below 2^24; no random case lies within rounding of a recomputed ReLU decision (the seeds are
fixed here); the engineered sign masks and integer affine vectors hold what the GPU file needs of them."""
import pytest
import torch

import conv_ref as R

KINDS = [False, True]


@pytest.fixture(scope="module")
def ops():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops as _ops
    return _ops


def stream1_cases():
    """(C, P, variant) of every 1x1 case of the GPU file: the pixel sweep on its two variants, the variant sweep at its size"""
    for C in R.STREAM1_C:
        for variant in R.STREAM1_P_SWEEP:
            for P in R.stream1_pixels(C):
                yield C, P, variant
        for variant in R.STREAM1_VARIANTS:
            yield C, R.stream1_sweep_pixels(C), variant


def stream1_sweep_grids(C, P, variant):
    return R.stream1_grids(P, C) if variant in R.STREAM1_P_SWEEP else [2]


def stream3_cases():
    for H, Wd in R.STREAM3_MAPS:
        for B in R.STREAM3_B:
            for aff in (False, True):
                yield B, H, Wd, aff


class switched:
    def __init__(self, obj, **kw):
        self.obj, self.kw = obj, kw

    def __enter__(self):
        self.old = {k: getattr(self.obj, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.obj, k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(self.obj, k, v)


def test_case_lists_are_the_boundaries_they_claim():
    assert [R.stream1_tile(C) for C in R.STREAM1_C] == [(256, 32, 4), (128, 16, 2), (64, 8, 1)]
    for C in R.STREAM1_C:
        TP, PPP, WM = R.stream1_tile(C)
        Ps = R.stream1_pixels(C)
        assert Ps[:9] == [1, PPP - 1, TP - 32, TP - 31, TP - 1, TP, TP + 1, 2 * TP + PPP + 3, 3 * TP] and Ps[9] == 105
        assert max(Ps) * C <= 768 * 32
        for P in Ps:
            B, H, Wd = R.stream1_layout(P)
            assert B * H * Wd == P
            rows, n = R.stream1_rows(P, C, 2 if P > TP else 1)
            assert n == (2 if P > TP else 1) * WM and int(rows.max()) < n
        assert R.stream1_layout(105) == (3, 5, 7) and R.stream1_layout(3 * TP)[0] == 3
        assert R.stream1_grids(3 * TP, C) == [1, 2, 3] and R.stream1_grids(TP, C) == [1]
        # three tiles on two blocks: block 0 walks two tiles, block 1 one
        rows, _ = R.stream1_rows(3 * TP, C, 2)
        assert int((rows < WM).sum()) == 2 * TP and int((rows >= WM).sum()) == TP
    assert len(R.STREAM1_VARIANTS) == 24 and len(set(R.STREAM1_VARIANTS)) == 24
    assert all(v in R.STREAM1_VARIANTS for v in R.STREAM1_COMPILED + R.STREAM1_P_SWEEP) and len(R.STREAM1_COMPILED) == 5
    # 3x3: the sweep map is 4 x 4 tiles with interior tiles and one-pixel edges; the grids leave uneven tile counts
    H, Wd = R.STREAM3_SWEEP_MAP
    assert (-(-H // 8), -(-Wd // 16)) == (4, 4) and H % 8 == 1 and Wd % 16 == 1 and R.STREAM3_SWEEP_MAP in R.STREAM3_MAPS
    assert R.stream3_grids(1, H, Wd) == [1, 5, 7, 8, 15, 16] and R.stream3_grids(2, H, Wd) == [1, 5, 7, 8, 15, 16, 24, 32]
    assert 2 * H * Wd * 32 == max(B * h * w * 32 for B in R.STREAM3_B for h, w in R.STREAM3_MAPS)
    for B in R.STREAM3_B:
        for G in R.stream3_grids(B, H, Wd):
            rows, n = R.stream3_rows(B, H, Wd, G)
            assert n == 4 * G and rows.numel() == B * H * Wd and int(rows.max()) < n
    rows, _ = R.stream3_rows(1, H, Wd, 5)            # 16 tiles on 5 blocks: block 0 walks four (3 G + 1), the others three
    per_block = torch.bincount(rows // 4, minlength=5)
    assert int(per_block[0]) > int(per_block[1:].max())


def test_engineered_masks_and_integer_vectors_hold_what_the_gpu_file_needs():
    for C in R.STREAM1_C:
        for P in (1, 3, 105):
            m = R.edge_bits((1, C, 1, P), 5)
            words = R.sign_bits(m).view(P, C // 32).numpy().view("uint32")
            flat = set(int(w) for w in words.reshape(-1)[:4 * (C // 32)])
            if P * (C // 32) >= 4:
                assert {0, 0xFFFFFFFF, 1, 0x80000000} <= flat
            if P >= 3:
                assert int(words[P - 1, -1]) == 0x80000000, "bit 31 of the last word of the last pixel, alone"
    # a positive integer shift on some channels: a padded halo pixel staged as relu(shift) instead of 0 shows in the exact case
    for B, H, Wd, aff in stream3_cases():
        if aff:
            sc, sh = R.stream3_case(B, H, Wd, True, True)["ia"]
            assert bool((sh > 0).any()) and bool((sh <= 0).any())
    for C, P, variant in stream1_cases():
        if variant[0] == "aff":
            assert bool((R.stream1_case(C, P, variant, True)["ia"][1] > 0).any())


def test_transposed_stream_launch_is_the_stride_1_data_gradient():
    x, w = R.conv_inputs(5, 2, 64, 64, 3, 5, 1)
    assert torch.equal(R.stream1(x, w, transpose=True).acc, R.dgrad1(x, w, 1).acc)
    assert torch.equal(R.stream1(x, w).acc, R.fwd(x, w, 1, 1).acc)


def plan1(ops, C, P, variant):
    inp, add, addmask, stats, bnb = variant
    B, H, Wd = R.stream1_layout(P)
    return ops._plan_conv(B, H, Wd, C, H, Wd, H, Wd, C, [(0, 0, 0)], 1, 1, 0, 0, 3, False, in_affine=inp == "aff", epi_add=add,
                          want_stats=stats, bn_bwd={None: None, "raw": "raw", "bits": "sign"}[bnb], add_mask=addmask,
                          in_presplit=inp == "pair")


def flags1(ops, variant):
    inp, add, addmask, stats, bnb = variant
    return ((ops.IN_AFFINE_RELU if inp == "aff" else 0) | (ops.IN_PRESPLIT if inp == "pair" else 0) | (ops.EPI_ADD if add else 0)
            | (ops.EPI_STATS if stats else 0) | (ops.EPI_BNBWD if bnb else 0))


def test_every_case_plans_to_the_streaming_entry(ops):
    from pytorch_kaldi_resnet_amd import hip
    for C, P, variant in stream1_cases():
        TP, _, WM = R.stream1_tile(C)
        for G in stream1_sweep_grids(C, P, variant):
            with switched(ops, STREAM_1X1=True, STREAM_1X1_BLOCKS=G):
                p = plan1(ops, C, P, variant)
            assert (p.entry, p.nblocks, p.flags) == ("spk_conv1x1_stream", G, flags1(ops, variant)), (C, P, variant, G, p)
            assert p.stats_rows is None and hip.lib().spk_conv1x1_stream_rows(G, C) == G * WM == R.stream1_rows(P, C, G)[1]
        with switched(ops, STREAM_1X1=True, STREAM_1X1_BLOCKS=512):
            assert plan1(ops, C, P, variant).nblocks == -(-P // TP), "the default grid is the tile count on these sizes"
        with switched(ops, STREAM_1X1=False):
            assert plan1(ops, C, P, variant).entry == "spk_conv_mfma"
    for B, H, Wd, aff in stream3_cases():
        def plan():
            return ops._plan_conv(B, H, Wd, 32, H, Wd, H, Wd, 32, ops.FWD_TAPS, 1, 1, 0, 0, 3, False, in_affine=aff, want_stats=True)
        for G in R.stream3_grids(B, H, Wd):
            with switched(ops, STREAM_C32=True, STREAM_C32_BLOCKS=G):
                p = plan()
            assert (p.entry, p.nblocks, p.stats_rows) == ("spk_conv3x3_c32_stream", G, 4 * G), (B, H, Wd, G, p)
            assert p.stats_rows == R.stream3_rows(B, H, Wd, G)[1]
            assert p.flags == (ops.EPI_STATS | (ops.IN_AFFINE_RELU if aff else 0))
        with switched(ops, STREAM_C32=True, STREAM_C32_BLOCKS=512):
            assert plan().nblocks == R.stream3_tiles(B, H, Wd)
        with switched(ops, STREAM_C32=False):
            assert plan().entry == "spk_conv_mfma"


def stored_as_float32(c, gate_add=True):
    """what a kernel with exact accumulation would store: the f16x3 emulation of the float32-staged operands in fp64, rounded to
    float32, the (masked) add in float32"""
    cv = c["conv"]
    x = c["x"]
    if c.get("ia") is not None:
        sc, sh = c["ia"]
        x = torch.relu(x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))          # float32, product and sum rounded separately
    acc = R.emulate(cv.bil, x, cv.w.float(), 3, Ba=cv.st["B"], Bw=float(cv.w.abs().max())).float()
    if c.get("add") is not None:
        ad = c["add"] if c.get("gate") is None else torch.where(c["gate"], c["add"], torch.zeros(()))
        acc = acc + ad
    return acc


def rows_as_float32(out32, rows, nrows, bn=None):
    """per-row statistics of stored float32 values the way the kernels end them: fp64 totals, one cast to float32"""
    C = out32.shape[1]
    o = out32.permute(0, 2, 3, 1).reshape(-1, C).double()
    if bn is None:
        a, q = o, o * o
    else:
        raw, mask, bn4 = bn
        px = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)      # noqa: E731
        xh = ((px(raw) - bn4[0]) * bn4[1]).double()              # float32 xhat
        a = o * px(mask)
        q = a * xh
    got = torch.zeros(nrows, C, 2, dtype=torch.float64)
    got[:, :, 0].index_add_(0, rows, a)
    got[:, :, 1].index_add_(0, rows, q)
    return got.float().double()


def check_case(name, c, stats_of, rows_of, grids, exact, bn=None):
    v, b = c["out"]
    out32 = stored_as_float32(c)
    if exact:
        assert c["conv"].exact_ok() and torch.equal(out32.double(), v), name
        assert float((c["conv"].S + (0 if c.get("add") is None else c["add"].double().abs())).max()) < 2.0 ** 24
    else:
        R.check("emulated " + name, out32, v, b)
    for G in grids:
        val, bnd, mag = stats_of(c, G, exact)
        rows = rows_of(G)
        got = rows_as_float32(out32, rows[0], rows[1], bn)
        if exact:
            assert float(mag.max()) < 2.0 ** 24 and torch.equal(got, val), (name, G)
            assert torch.equal(got.sum(0), val.sum(0)) and float(mag.sum(0).max()) < 2.0 ** 24
        else:
            R.check("emulated " + name + " statistics rows", got, val, bnd)
            R.check("emulated " + name + " statistics totals", got.sum(0), val.sum(0), bnd.sum(0))
        empty = torch.bincount(rows[0], minlength=rows[1]) == 0
        assert bool((bnd >= 0).all()) and not bool(bnd[empty].any()) and not bool(val[empty].any()), "a row without pixels is 0, exactly"


@pytest.mark.parametrize("exact", KINDS)
@pytest.mark.parametrize("C", R.STREAM1_C)
def test_streaming_1x1_cases_stay_inside_their_own_bounds(C, exact):
    """building a case also takes every recomputed ReLU decision through mask_from_raw: a seed within rounding of 0 fails here"""
    for Cc, P, variant in stream1_cases():
        if Cc != C:
            continue
        c = R.stream1_case(C, P, variant, exact)
        grids = stream1_sweep_grids(C, P, variant) if variant[3] else []
        bn = (c["raw"], c["mask"], c["bn4"]) if variant[4] else None
        check_case("conv1x1_stream %s" % (variant,), c, R.stream1_stats, lambda G, P=P: R.stream1_rows(P, C, G), grids, exact, bn)


@pytest.mark.parametrize("exact", KINDS)
@pytest.mark.parametrize("H,Wd", R.STREAM3_MAPS)
def test_streaming_3x3_cases_stay_inside_their_own_bounds(H, Wd, exact):
    for B in R.STREAM3_B:
        for aff in (False, True):
            c = R.stream3_case(B, H, Wd, aff, exact)
            check_case("conv3x3_c32_stream", c, R.stream3_stats, lambda G, B=B: R.stream3_rows(B, H, Wd, G), R.stream3_grids(B, H, Wd), exact)


def test_far_apart_operand_scales_stay_normal_and_inside_the_bound():
    for C, k in ((32, 1), (32, 3)):
        x, w, amax, (v, b) = R.far_case(C, 9, 13, k)
        assert amax == 8 * float(x.abs().max()) and 2.0 ** 39 < float(x.abs().max()) < 2.0 ** 41
        assert 2.0 ** -53 < float(w.abs().max()) < 2.0 ** -51
        assert float(v.abs().max()) < 1.0 and float(v.abs()[v != 0].min()) > 2.0 ** -100, "outputs are normal floats"
        cv = R.fwd(x, w, k, 1)
        got = R.emulate(cv.bil, x, cv.w.float(), 3, Ba=amax, Bw=float(w.abs().max())).float()
        R.check("emulated far-apart scales", got, v, b)
        # the operand scales: the two reciprocals are far from 1, on opposite sides
        assert R.sigma_of_value(amax) < 2.0 ** -25 and R.sigma_of_value(float(w.abs().max())) > 2.0 ** 60
