"""Half-precision extraction on the GPU (csrc/half.hip) against tests/half_ref.py.

Kernel level: every element of every output inside the contract's bound
    |gpu - y| <= 2^-11 |y| + 2^-25 + (K + 4) 2^-24 S (1 + 2^-10)
(half_ref.kernel_bound; y exact on the same fp16 inputs), masked columns +0 bit for bit, overflow counts equal to the reference's;
with small-integer data, where every partial sum is exact, bit-for-bit equality - that is what pins the lane maps of the matrix
instruction, the nearest-even rounding (2049 -> 2048, 2051 -> 2052) and the overflow threshold (65519 stays finite, 65520 is inf).
Model level: the distance of predict(precision="f16") to the exact fp64 embedding within 2 x the distance of the CPU emulation of
the contract (the project's factor: test_fullsize_gpu.py holds a mode to 2 x its yardstick); a direct comparison with the emulation
is no test, since the network amplifies single rounding flips to that same distance (tests/test_half_cpu.py).
"""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import half_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Cin, Cout, ksize, stride, IH, IW
SHAPES = [(32, 32, 3, 1, 5, 19), (64, 64, 3, 1, 1, 1), (256, 256, 3, 1, 3, 5), (32, 64, 3, 2, 11, 13), (64, 128, 1, 2, 8, 9),
          (128, 128, 1, 1, 4, 6), (128, 256, 3, 2, 20, 75)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def h16(t):
    """fp16 values held in any float dtype -> device float16"""
    return t.to(torch.float16).cuda()


def bits(t):
    return t.contiguous().view(torch.int16)


def run_conv(x16, w, scale, shift, k, stride, add16=None, relu=True, wlen=None):
    from pytorch_kaldi_resnet_amd import ops
    B = x16.shape[0]
    ovf = torch.zeros(B, dtype=torch.int32, device="cuda")
    wpk = ops.h16_pack_conv_weight(w.cuda())
    out = ops.h16_conv_fwd(h16(x16), wpk, w.shape[0], k, stride, scale.cuda(), shift.cuda(), ovf,
                           add=None if add16 is None else h16(add16), relu=relu,
                           wlen=None if wlen is None else torch.tensor(wlen, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    return out.cpu(), ovf.cpu()


# ---- exact integer data ---------------------------------------------------------------------------------------------------------
def integer_case(shape, B, rows=None):
    """inputs in {-4..4}, weights in {-2..2}, scale 1 or 2, integer shift: every partial sum is an exact fp32 integer.  The residual
    (an fp16 tensor of integers) places chosen results in every image: 2049 and 2051 (ties of the rounding), two values >= 65520
    (stored as inf) and, where some y0 = 15 mod 32 exists, 65519 - the largest result that stays finite.  rows: the images that
    get planted values (default: all)."""
    Cin, Cout, k, stride, IH, IW = shape
    g = gen(100 + Cin + Cout + k + stride + B)
    x = torch.randint(-4, 5, (B, IH, IW, Cin), generator=g).double()
    w = torch.randint(-2, 3, (Cout, Cin, k, k), generator=g).float()
    scale = torch.tensor([1.0, 2.0])[torch.randint(0, 2, (Cout,), generator=g)]
    shift = torch.randint(-3, 4, (Cout,), generator=g).float()
    sums = R.conv_sums(x, w, k, stride)
    assert float(sums[1].max()) * 2 + 3 + 65504 < 2 ** 24
    y0 = R.conv_ref(sums, scale, shift, relu=False)[0]
    add = torch.randint(-8, 9, y0.shape, generator=g).double()
    flat, addf = y0.reshape(B, -1), add.reshape(B, -1)
    for b in (range(B) if rows is None else rows):
        cand = torch.nonzero((flat[b] >= 16) & (flat[b] <= 2000)).flatten().tolist()
        assert len(cand) >= 4, "too few candidates to plant the ties and the overflow"
        for i, target in zip(cand[:4], (2049.0, 2051.0, None, None)):
            addf[b, i] = 65504.0 if target is None else target - float(flat[b, i])
        edge = [i for i in torch.nonzero((flat[b] >= 15) & (flat[b] <= 2000) & (flat[b] % 32 == 15)).flatten().tolist()
                if i not in cand[:4]]
        if edge:
            addf[b, edge[0]] = 65519.0 - float(flat[b, edge[0]])
    assert (add == R.round16(add)).all()
    return x, w, scale, shift, sums, add


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dto%d_k%d_s%d_%dx%d" % s)
def test_conv_is_exact_on_integer_data(shape, B):
    Cin, Cout, k, stride, IH, IW = shape
    x, w, scale, shift, sums, add = integer_case(shape, B)
    y, _, want, want_ovf = R.conv_ref(sums, scale, shift, add16=add, relu=True)
    flat = y.reshape(B, -1)
    for b in range(B):
        assert (flat[b] == 2049.0).any() and (flat[b] == 2051.0).any() and int((flat[b] >= 65520.0).sum()) >= 2
        assert want_ovf[b] == int((flat[b] >= 65520.0).sum())
    got, ovf = run_conv(x, w, scale, shift, k, stride, add16=add, relu=True)
    want16 = want.to(torch.float16)
    assert torch.equal(bits(got), bits(want16)), "not bit-equal: %d of %d differ" % (int((bits(got) != bits(want16)).sum()),
                                                                                  got.numel())
    assert ovf.tolist() == want_ovf.tolist()


@pytest.mark.parametrize("Cin,Cout,k,stride", [(32, 32, 3, 1), (64, 64, 3, 1), (32, 64, 3, 2), (64, 64, 1, 1)])
def test_conv_is_exact_when_a_block_runs_several_tiles(Cin, Cout, k, stride):
    """from a tile count on, a block runs several consecutive tiles with its loads pipelined across the tile boundaries: three
    tiles per image and a tile count that is no multiple of the tiles per block, so blocks straddle images and the last one is
    short; with Cin = 32 at stride 1 the weight images are staged once per block"""
    from pytorch_kaldi_resnet_amd import ops
    th, tw = ops.h16_conv_tile()
    tpb, tmin = ops.h16_conv_tiles_per_block()
    OW = 2 * tw + 1                                       # three column tiles, the last one pixel wide
    nzc = max(1, Cout // 64)
    B = -(-tmin // (3 * nzc))
    while (3 * B) % tpb == 0:
        B += 1
    assert 3 * B * nzc >= tmin and tpb > 1
    shape = (Cin, Cout, k, stride, 1, OW if stride == 1 else 2 * OW - 1)
    rows = [0, 1, B // 2, B - 2, B - 1]
    x, w, scale, shift, sums, add = integer_case(shape, B, rows=rows)
    y, _, want, want_ovf = R.conv_ref(sums, scale, shift, add16=add, relu=True)
    assert y.shape == (B, 1, OW, Cout) and all(want_ovf[b] >= 2 for b in rows) and int(want_ovf.sum()) == int(want_ovf[rows].sum())
    got, ovf = run_conv(x, w, scale, shift, k, stride, add16=add, relu=True)
    assert torch.equal(bits(got), bits(want.to(torch.float16)))
    assert ovf.tolist() == want_ovf.tolist()


# ---- random data ----------------------------------------------------------------------------------------------------------------
def _tile_shape():
    from pytorch_kaldi_resnet_amd import ops
    th, tw = ops.h16_conv_tile()
    return (64, 32, 3, 1, th + 1, tw + 1)


@pytest.mark.parametrize("idx", range(len(SHAPES) + 1))
def test_conv_random_within_the_bound(idx):
    from pytorch_kaldi_resnet_amd import ops
    th, tw = ops.h16_conv_tile()
    Cin, Cout, k, stride, IH, IW = SHAPES[idx] if idx < len(SHAPES) else _tile_shape()
    OH, OW = (IH + stride - 1) // stride, (IW + stride - 1) // stride
    wl = sorted({1, OW, max(1, OW // 2)} | {v for v in (tw - 1, tw + 1) if 1 <= v <= OW})
    B = len(wl)
    g = gen(200 + idx)
    x = R.round16(torch.randn(B, IH, IW, Cin, generator=g).double())
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (k * Cin ** 0.5)).float()
    # per-channel scales from 2^-16 to 2^6: the small channels store fp16 subnormals
    e = torch.linspace(-16, 6, Cout)[torch.randperm(Cout, generator=g)]
    sign = torch.where(torch.rand(Cout, generator=g) < 0.5, -1.0, 1.0)
    scale = (sign * 2.0 ** e).float()
    shift = (torch.randn(Cout, generator=g) * 2.0 ** e * 0.5).float()
    add = R.round16(torch.randn(B, OH, OW, Cout, generator=g).double() * (2.0 ** e).double())
    sums = R.conv_sums(x, w, k, stride)
    K = k * k * Cin
    worst, subnormals = 0.0, 0
    for use_add, relu, use_wl in itertools.product((False, True), repeat=3):
        y, S, _, want_ovf = R.conv_ref(sums, scale, shift, add16=add if use_add else None, relu=relu, wlen=wl if use_wl else None)
        got, ovf = run_conv(x, w, scale, shift, k, stride, add16=add if use_add else None, relu=relu, wlen=wl if use_wl else None)
        assert want_ovf.tolist() == [0] * B and ovf.tolist() == [0] * B
        assert got.shape == y.shape
        err = (got.double() - y).abs()
        bound = R.kernel_bound(y, S, K)
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (idx, use_add, relu, use_wl, ratio)
        subnormals += int(((got != 0) & (got.abs() < 2.0 ** -14)).sum())
        if use_wl:
            for b, l in enumerate(wl):
                assert (bits(got[b, :, l:]) == 0).all(), "masked columns must be +0 bit for bit"
    print("h16 conv %dto%d k%d s%d %dx%d: worst error / bound %.3f, %d subnormal outputs" % (Cin, Cout, k, stride, IH, IW, worst,
                                                                                            subnormals))
    assert subnormals > 0


# ---- stem, pooling, pack ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,T", [(1, 1), (5, 17), (40, 65)])
@pytest.mark.parametrize("masked", [False, True])
def test_stem(F, T, masked):
    from pytorch_kaldi_resnet_amd import ops
    g = gen(300 + F + T)
    x = torch.randn(2, F, T, generator=g)
    w = (torch.randn(32, 1, 3, 3, generator=g) / 3).float()
    scale = (torch.rand(32, generator=g) + 0.5).float()
    shift = (torch.randn(32, generator=g) * 0.3).float()
    wl = [T, max(1, T // 2)] if masked else None
    xin = x.clone()
    if masked:
        xin[1, :, wl[1]:] = float("nan")               # the padding is never read
    y, S, _, want_ovf = R.stem_ref(x, w, scale, shift, wl)
    ovf = torch.zeros(2, dtype=torch.int32, device="cuda")
    got = ops.h16_stem_fwd(xin.cuda(), w.cuda(), scale.cuda(), shift.cuda(), ovf,
                           wlen=None if wl is None else torch.tensor(wl, dtype=torch.int32, device="cuda")).cpu()
    ratio = float(((got.double() - y).abs() / R.kernel_bound(y, S, 9)).max())
    print("h16 stem F %d T %d masked %s: worst error / bound %.3f" % (F, T, masked, ratio))
    assert ratio <= 1.0
    assert ovf.cpu().tolist() == want_ovf.tolist() == [0, 0]
    if masked:
        assert (bits(got[1, :, wl[1]:]) == 0).all()


def test_stem_counts_overflow_per_utterance():
    from pytorch_kaldi_resnet_amd import ops
    x = torch.ones(3, 4, 9)
    x[1] *= 3e4
    w = torch.ones(32, 1, 3, 3)
    scale, shift = torch.ones(32), torch.zeros(32)
    _, _, want, want_ovf = R.stem_ref(x, w, scale, shift)
    ovf = torch.zeros(3, dtype=torch.int32, device="cuda")
    got = ops.h16_stem_fwd(x.cuda(), w.cuda(), scale.cuda(), shift.cuda(), ovf).cpu()
    assert torch.equal(bits(got), bits(want.to(torch.float16)))
    assert ovf.cpu().tolist() == want_ovf.tolist() and want_ovf[0] == 0 and want_ovf[1] == 4 * 9 * 32 and want_ovf[2] == 0


@pytest.mark.parametrize("W", [1, 2, 38, 75])
@pytest.mark.parametrize("mode", [0, 1])
def test_pooling(W, mode):
    from pytorch_kaldi_resnet_amd import ops
    B, H, C = 3, 3, 64
    x = R.round16(torch.randn(B, H, W, C, generator=gen(400 + W)).abs().double())
    for wl in (None, [W, 1, max(1, W // 2)]):
        want, bound = R.pool_ref(x, mode, wl)
        got = ops.h16_stats_pool_fwd(h16(x), mode, wlen=None if wl is None else torch.tensor(wl, dtype=torch.int32, device="cuda")).cpu()
        assert got.shape == want.shape
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)                    # the unbiased variance of one frame, in the same entries
        assert bool(nan.any()) == (mode == 1 and (W == 1 or wl is not None))
        ratio = float(((got.double() - want).abs()[~nan] / bound[~nan]).max())
        print("h16 pooling W %d mode %d wlen %s: worst error / bound %.3f" % (W, mode, wl, ratio))
        assert ratio <= 1.0


def test_pack_rounds_ties_to_even_and_keeps_inf():
    from pytorch_kaldi_resnet_amd import ops
    w = torch.randn(64, 32, 3, 3, generator=gen(500))
    special = [2049.0, 2051.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 65519.0, 65520.0, 1e5, -7e4]
    w.view(-1)[:len(special)] = torch.tensor(special)
    got = ops.h16_pack_conv_weight(w.cuda()).cpu().numpy()
    want = R.pack_ref(w)
    assert got.dtype == np.float16 and got.nbytes == R.packed_bytes(64, 32, 3, 3)
    assert np.array_equal(got.view(np.int16), want.view(np.int16))
    with np.errstate(over="ignore"):
        r = w.view(-1)[:len(special)].numpy().astype(np.float16).astype(np.float64).tolist()
    assert r == [2048.0, 2052.0, 1.0, 1 + 2.0 ** -9, 0.0, 2.0 ** -23, 65504.0, float("inf"), float("inf"), float("-inf")]


# ---- model level ------------------------------------------------------------------------------------------------------------------
def make_model(case, seed=None):
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    arch, s, Fd, T, B, pooling, loss = case
    npst = R.make_state(s if seed is None else seed, R.SPK_NUM, feat_dim=Fd, pooling=pooling, loss=loss, arch=arch)
    m = NeuralSpeakerModel(R.SPK_NUM, Fd, pooling, loss, 0.2, 30, arch=arch)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()}, strict=True)
    return m.cuda().eval(), npst


def half_predict(m, x, lengths=None):
    e = m.predict(torch.as_tensor(x).cuda(), lengths=lengths, precision="f16")
    torch.cuda.synchronize()
    return e.cpu(), m.engine().half_overflow.cpu()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_distance_to_the_exact_embedding(name):
    y = R.case_yardstick(name)
    m, _ = make_model(y["case"])
    e, ovf = half_predict(m, y["x"])
    rel, cosd = R.distance(e, y["e64"])
    print("%s: half predict vs fp64 relL2 %.3e 1-cos %.3e; emulation %.3e %.3e" % (name, rel, cosd, y["relL2"], y["cosd"]))
    assert ovf.dtype == torch.int32 and ovf.tolist() == [0] * y["case"][4]
    assert rel <= 2.0 * y["relL2"] and cosd <= 2.0 * y["cosd"]


@pytest.mark.parametrize("name", ["r34_s11", "r50_s22"])
def test_lengths(name):
    arch, seed, Fd, _, _, pooling, loss = R.CASES[name]
    T = 104
    L = [T, T - 1, T - 7, 53, 17, 9]
    case = (arch, seed, Fd, T, len(L), pooling, loss)
    m, npst = make_model(case)
    x0 = torch.from_numpy(R.case_input(case))
    outs = []
    for fill in ("zero", "noise", "nan"):
        x = x0.clone()
        for b, l in enumerate(L):
            if fill == "zero":
                x[b, :, l:] = 0
            elif fill == "noise":
                x[b, :, l:] = (torch.rand(Fd, T - l, generator=gen(b)) * 2 - 1) * 1e3
            else:
                x[b, :, l:] = float("nan")
        e, ovf = half_predict(m, x, L)
        assert ovf.tolist() == [0] * len(L)
        outs.append(e)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])          # the padding content does not matter
    plain, _ = half_predict(m, x0)
    full, _ = half_predict(m, x0, [T] * len(L))
    assert torch.equal(plain, full)
    for b, l in enumerate(L):
        xb = x0[b:b + 1, :, :l].numpy()
        e64, _, _ = R.embed(npst, xb, arch, pooling, half=False)
        emu, _, _ = R.embed(npst, xb, arch, pooling, half=True)
        rel_e, cos_e = R.distance(emu, e64)
        rel, cosd = R.distance(outs[0][b:b + 1], e64)
        print("%s row %d L %d: half predict vs fp64 %.3e %.3e; emulation %.3e %.3e" % (name, b, l, rel, cosd, rel_e, cos_e))
        assert rel <= 2.0 * rel_e and cosd <= 2.0 * cos_e, (b, l)
    # one frame: the unbiased variance of the pooling is NaN - that row only, where the fp32 path has it
    x2 = x0[:2].contiguous()
    e, _ = half_predict(m, x2, [T, 1])
    e32 = m.predict(x2.cuda(), lengths=[T, 1]).cpu()
    assert torch.isfinite(e[0]).all() and torch.equal(torch.isnan(e), torch.isnan(e32))
    assert torch.isnan(e[1]).any() == (pooling == "mean+std")


def test_overflow_is_reported_per_row():
    case = R.OVERFLOW_CASE
    m, _ = make_model(case)
    _, ovf = half_predict(m, R.case_input(case, 14))
    assert (ovf > 0).all(), ovf.tolist()
    case = R.SCALED_CASE
    m, _ = make_model(case)
    x = torch.from_numpy(R.case_input(case, 12))
    base, ovf0 = half_predict(m, x)
    xs = x.clone()
    xs[1] *= 1e4
    e, ovf = half_predict(m, xs)
    assert ovf0.tolist() == [0, 0, 0]
    assert ovf[0] == 0 and ovf[1] > 0 and ovf[2] == 0, ovf.tolist()
    assert torch.equal(e[0], base[0]) and torch.equal(e[2], base[2])


def test_packs_follow_the_weights():
    case = R.CASES["r18_s21"]
    x = R.case_input(case)
    m, _ = make_model(case)
    first, _ = half_predict(m, x)
    other = R.make_state(31, R.SPK_NUM, feat_dim=case[2], pooling=case[5], loss=case[6], arch=case[0])
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in other.items()}, strict=True)
    second, _ = half_predict(m, x)
    fresh, _ = half_predict(make_model(case, seed=31)[0], x)
    assert torch.equal(second, fresh) and not torch.equal(first, second)


def test_refusals():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    case = R.CASES["r18_s21"]
    m, _ = make_model(case)
    x = torch.from_numpy(R.case_input(case)).cuda()
    with pytest.raises(ValueError, match="precision"):
        m.predict(x, precision="bf16")
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.predict(x, precision="f16")
    se = NeuralSpeakerModel(R.SPK_NUM, 40, "mean", "softmax", 0.2, 30, arch="se_resnet34").cuda().eval()
    with pytest.raises(NotImplementedError, match="se_resnet34"):
        se.predict(x, precision="f16")


def test_the_default_path_is_untouched():
    case = R.CASES["r18_s21"]
    m, _ = make_model(case)
    x = torch.from_numpy(R.case_input(case)).cuda()
    before = m.predict(x).cpu()
    half_predict(m, x)
    after = m.predict(x).cpu()
    named = m.predict(x, precision="f32").cpu()
    assert torch.equal(before, after) and torch.equal(after, named)


# ---- decode.py --half -----------------------------------------------------------------------------------------------------------
def _read_text_vectors(path):
    out = {}
    for line in open(path):
        key, rest = line.split(" ", 1)
        out[key] = np.array(rest.strip().strip("[]").split(), dtype=np.float32)
    return out


def test_decode_half(tmp_path):
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import kaldi_io
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    Fd = 40
    rng = np.random.RandomState(7)
    lens = rng.choice(np.arange(40, 121), size=8, replace=False)
    ark, scp = str(tmp_path / "feats.ark"), str(tmp_path / "feats.scp")
    with open(ark, "wb") as f, open(scp, "w") as s:
        for i, n in enumerate(lens):
            key = "utt%03d" % i
            f.write(key.encode() + b" ")
            off = f.tell()
            kaldi_io.write_mat(f, rng.randn(int(n), Fd).astype(np.float32))
            s.write("%s %s:%d\n" % (key, ark, off))
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT

    def decode(arch, seed, pooling, loss, half, tag):
        npst = R.make_state(seed, R.SPK_NUM, feat_dim=Fd, pooling=pooling, loss=loss, arch=arch)
        m = NeuralSpeakerModel(R.SPK_NUM, Fd, pooling, loss, 0.2, 30, arch=arch)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
        ckpt = str(tmp_path / ("%s.pth.tar" % arch))
        torch.save({"state_dict": m.state_dict(), "epoch": 1}, ckpt)
        out = str(tmp_path / tag)
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "decode.py"), "--spk_num", str(R.SPK_NUM), "--arch", arch,
               "--input-dim", str(Fd), "--pooling", pooling, "--model-path", ckpt, "--decode-scp", scp, "--out-path", out,
               "--native-reader", "--pad-batches", "--batch-size", "16"] + (["--half"] if half else [])
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return os.path.join(out, "alone"), r.stdout

    y = R.case_yardstick("r34_s12")
    arch, seed, _, _, _, pooling, loss = y["case"]
    p32, out32 = decode(arch, seed, pooling, loss, False, "r34_f32")
    p16, out16 = decode(arch, seed, pooling, loss, True, "r34_f16")
    assert "left the fp16 range" not in out32
    assert "=> 0 of 8 utterances left the fp16 range and were extracted in fp32" in out16
    a, b = _read_text_vectors(p16), _read_text_vectors(p32)
    assert sorted(a) == sorted(b) == ["utt%03d" % i for i in range(8)]
    for k in sorted(a):
        rel, cosd = R.distance(torch.from_numpy(a[k][None]), torch.from_numpy(b[k][None]))
        print("decode --half %s: %.3e %.3e against fp32 (yardstick %.3e %.3e)" % (k, rel, cosd, y["relL2"], y["cosd"]))
        assert rel <= 2.0 * y["relL2"] and cosd <= 2.0 * y["cosd"], k
    arch, seed, _, _, _, pooling, loss = R.OVERFLOW_CASE
    p32, _ = decode(arch, seed, pooling, loss, False, "r101_f32")
    p16, out16 = decode(arch, seed, pooling, loss, True, "r101_f16")
    assert "=> 8 of 8 utterances left the fp16 range and were extracted in fp32" in out16
    assert open(p16, "rb").read() == open(p32, "rb").read()
