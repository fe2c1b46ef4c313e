"""Length-masked predict: predict(x, lengths=L) over a padded batch gives, for every row, the embedding of that utterance run alone.

Model level (three operand modes, the tolerances of test_model_gpu.py::test_forward_parity): every row against the CPU oracle's solo
embedding of x[b:b+1, :, :L[b]] and against the HIP solo predict of the cropped utterance; the padding content does not matter (bitwise);
lengths = [T] * B is the plain predict (bitwise); a pooled width of one frame gives NaN in that row only.  Kernel level: the masked
stem / convolution forms / pooling against the unmasked kernels on zero-padded input.  Extraction: decode.py --pad-batches against the
length-bucketed run.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import spk_oracle as O  # noqa: E402
from oracle import weights as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["bf16x6", "f32", "f16x3"]


@pytest.fixture(params=MODES)
def mfma_mode(request):
    from pytorch_kaldi_resnet_amd import ops
    old = ops.SPLIT
    ops.SPLIT = ops.MFMA_MODES[request.param]
    yield request.param
    ops.SPLIT = old


def cos_dist(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float((1 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))).max())


def srel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())


def close(a, b):
    """test_forward_parity's bar for eval-mode embeddings"""
    return cos_dist(a, b) < 1e-6 and srel(a, b) < 2e-5


CASES = {     # name: (seed, spk_num, feat_dim, pooling, loss, arch, T)
    "r34_aam": (11, 10, 80, "mean+std", "AAM", "resnet34", 224),
    "r34_softmax_mean_f40": (12, 12, 40, "mean", "softmax", "resnet34", 224),
    "r101_aam": (13, 10, 40, "mean+std", "AAM", "resnet101", 224),
}


def lengths_for(T):
    return [T, T - 1, T - 7, 203, 150, 17, 9]


def make_model(name):
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    seed, S, F, pooling, loss, arch, _ = CASES[name]
    npst = W.make_state(seed, S, F, pooling, loss, arch)
    m = NeuralSpeakerModel(S, F, pooling, loss, 0.2, 30, arch=arch)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()}, strict=True)
    return m.cuda().eval(), npst


def padded_input(name, L, fill="zero"):
    seed, S, F, _, _, _, T = CASES[name]
    x, _ = W.make_input(seed + 1, len(L), F, T, S)
    x = torch.from_numpy(x)
    for b, l in enumerate(L):
        if fill == "zero":
            x[b, :, l:] = 0
        elif fill == "random":
            x[b, :, l:] = (torch.rand(F, T - l, generator=torch.Generator().manual_seed(b)) * 2 - 1) * 1e3
        else:
            x[b, :, l:] = float("nan")
    return x


_ORACLE = {}


def oracle_rows(name, npst, x, L):
    """CPU oracle embedding of every utterance alone (cached: it does not depend on the operand mode)"""
    key = (name, tuple(L))
    if key not in _ORACLE:
        _, _, _, pooling, _, arch, _ = CASES[name]
        st = O.to_torch_state(npst)
        with torch.no_grad():
            _ORACLE[key] = np.concatenate([O.embed(st, x[b:b + 1, :, :l], pooling, arch, train=False).numpy()
                                           for b, l in enumerate(L)])
    return _ORACLE[key]


@pytest.mark.parametrize("name", list(CASES))
def test_padded_batch_matches_solo_runs(mfma_mode, name):
    m, npst = make_model(name)
    T = CASES[name][6]
    L = lengths_for(T)
    x = padded_input(name, L)
    with torch.no_grad():
        emb = m.predict(x.cuda(), lengths=L).cpu().numpy()
        solo = np.concatenate([m.predict(x[b:b + 1, :, :l].contiguous().cuda()).cpu().numpy() for b, l in enumerate(L)])
    ref = oracle_rows(name, npst, x, L)
    assert np.isfinite(emb).all()
    for b, l in enumerate(L):
        assert close(emb[b:b + 1], ref[b:b + 1]), (name, mfma_mode, l, cos_dist(emb[b:b + 1], ref[b:b + 1]), srel(emb[b:b + 1], ref[b:b + 1]))
        assert close(emb[b:b + 1], solo[b:b + 1]), (name, mfma_mode, l)


@pytest.mark.parametrize("name", ["r34_aam", "r101_aam"])
def test_padding_content_is_irrelevant(mfma_mode, name):
    m, _ = make_model(name)
    L = lengths_for(CASES[name][6])
    Lt = torch.tensor(L, dtype=torch.int32, device="cuda")        # an int tensor on the device works as well as a list
    with torch.no_grad():
        outs = [m.predict(padded_input(name, L, fill).cuda(), lengths=Lt) for fill in ("zero", "random", "nan")]
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("name", ["r34_aam", "r34_softmax_mean_f40"])
def test_full_lengths_is_the_plain_predict(mfma_mode, name):
    m, _ = make_model(name)
    seed, S, F, _, _, _, T = CASES[name]
    x, _ = W.make_input(seed + 1, 5, F, T, S)
    xg = torch.from_numpy(x).cuda()
    with torch.no_grad():
        a = m.predict(xg)
        b = m.predict(xg, lengths=torch.full((5,), T, dtype=torch.int64))
    assert torch.equal(a, b)


def test_one_pooled_frame_is_nan_in_its_row_only(mfma_mode):
    name = "r34_aam"
    m, npst = make_model(name)
    T = CASES[name][6]
    L = lengths_for(T)[:-1] + [5]           # ceil(5 / 8) = 1 pooled frame: unbiased variance 0/0
    x = padded_input(name, L)
    with torch.no_grad():
        emb = m.predict(x.cuda(), lengths=L).cpu().numpy()
    st = O.to_torch_state(npst)
    with torch.no_grad():
        ref5 = O.embed(st, x[-1:, :, :5], "mean+std", "resnet34", train=False).numpy()
    assert np.isnan(ref5).any()
    np.testing.assert_array_equal(np.isnan(emb[-1:]), np.isnan(ref5))
    assert np.isfinite(emb[:-1]).all()
    ref = oracle_rows(name, npst, x, lengths_for(T))
    for b in range(len(L) - 1):
        assert close(emb[b:b + 1], ref[b:b + 1]), (mfma_mode, L[b])


def test_argument_errors():
    m, _ = make_model("r34_softmax_mean_f40")
    T = 64
    x = torch.randn(3, 40, T, device="cuda")
    with torch.no_grad():
        for bad, exc in (([T, 0, 5], ValueError), ([T, T + 1, 5], ValueError), ([T, 5], ValueError), ([T, 5, 5, 5], ValueError),
                         (torch.tensor([5.0, 6.0, 7.0]), TypeError)):
            with pytest.raises(exc):
                m.predict(x, lengths=bad)
        m.train()
        with pytest.raises(RuntimeError, match="eval"):
            m.predict(x, lengths=[T, 5, 5])
        m.eval()
        assert m.predict(x, lengths=[T, 5, 5]).shape == (3, 256)


# ---- kernel level ------------------------------------------------------------------------------------------------------------

def _bits_to_float(slot):
    return float(slot.view(torch.float32).item())


def test_masked_stem_kernel():
    from pytorch_kaldi_resnet_amd import ops
    torch.manual_seed(0)
    B, F, T = 3, 40, 77
    L = [77, 40, 3]
    wl = torch.tensor(L, dtype=torch.int32, device="cuda")
    x = torch.randn(B, F, T, device="cuda")
    for b, l in enumerate(L):
        x[b, :, l:] = 0
    xn = x.clone()
    for b, l in enumerate(L):
        xn[b, :, l:] = float("nan")
    w = torch.randn(32, 1, 3, 3, device="cuda") * 0.3
    sc, sh = torch.rand(32, device="cuda") + 0.5, torch.rand(32, device="cuda") + 0.1      # shift > 0: the unmasked tail is not 0
    s0 = torch.zeros(1, dtype=torch.int32, device="cuda")
    s1 = torch.zeros(1, dtype=torch.int32, device="cuda")
    ref, _ = ops.stem_fwd(x, w, epi_affine=(sc, sh), relu=True, amax_out=s0)
    got, _ = ops.stem_fwd(xn, w, epi_affine=(sc, sh), relu=True, amax_out=s1, wlen=wl)
    for b, l in enumerate(L):
        assert torch.equal(got[b, :, :l], ref[b, :, :l])
        assert (got[b, :, l:] == 0).all()
        if l < T:
            assert (ref[b, :, l:] != 0).any()
    assert _bits_to_float(s1) == float(got.abs().max())


FORMS = [("f32", "mfma"), ("bf16x6", "mfma"), ("f16x3", "mfma"), ("f16x3", "pipe"), ("f16x3", "m16")]


@pytest.mark.parametrize("k,stride,add", [(3, 1, False), (3, 1, True), (3, 2, False), (1, 1, False), (1, 2, False)])
@pytest.mark.parametrize("mode,form", FORMS)
def test_masked_conv_forms(mode, form, k, stride, add):
    from pytorch_kaldi_resnet_amd import ops, tiling
    torch.manual_seed(1)
    B, H, W, Cin, Cout = 3, 10, 40, 64, 64
    Lin = [40, 23, 5]
    Lout = [-(-l // stride) for l in Lin]
    x = torch.randn(B, H, W, Cin, device="cuda")
    for b, l in enumerate(Lin):
        x[b, :, l:] = 0
    w = torch.randn(Cout, Cin, k, k, device="cuda") * 0.05
    sc, sh = torch.rand(Cout, device="cuda") + 0.5, torch.rand(Cout, device="cuda") + 0.1
    OH, OW = ops.conv_out_hw(H, W, k, stride)
    res = torch.randn(B, OH, OW, Cout, device="cuda") if add else None
    old = (ops.SPLIT, ops.PIPE_CONV, ops.PIPE_M16, ops.PROFILE)
    key = (OH, OW, stride if k == 3 else 1, k, k, k * k, Cout)
    forced = k == 3 and stride == 1
    try:
        ops.SPLIT = ops.MFMA_MODES[mode]
        ops.PIPE_CONV = form != "mfma"
        ops.PIPE_M16 = form == "m16"
        if forced:                     # a (3, 2) register tile whose halo fits both pipelined forms
            tiling.FORCE_CONV[key] = tiling.FORCE_CONV_SPLIT[key] = (8, 32, 3, 2)
        wpk = ops.pack_conv_weight(w)
        s0 = torch.zeros(1, dtype=torch.int32, device="cuda")
        s1 = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.PROFILE = []
        ref, _ = ops.conv_fwd(x, wpk, Cout, k, stride, epi_affine=(sc, sh), epi_add=res, relu=True, out_amax=s0)
        got, _ = ops.conv_fwd(x, wpk, Cout, k, stride, epi_affine=(sc, sh), epi_add=res, relu=True, out_amax=s1,
                              wlen=torch.tensor(Lout, dtype=torch.int32, device="cuda"))
        labels = [p[0] for p in ops.PROFILE]
        torch.cuda.synchronize()
    finally:
        ops.SPLIT, ops.PIPE_CONV, ops.PIPE_M16, ops.PROFILE = old
        if forced:
            tiling.FORCE_CONV.pop(key, None)
            tiling.FORCE_CONV_SPLIT.pop(key, None)
    if form == "mfma":
        assert labels[-1].startswith("conv_mfma_kernel"), labels
    elif forced and form == "m16":
        assert labels[-1].startswith("conv_pipe_kernel<3,2,false,false,false,true>"), labels
    elif forced:
        assert labels[-1].startswith("conv_pipe_kernel<3,2,false,false>"), labels
    for b, l in enumerate(Lout):
        assert torch.equal(got[b, :, :l], ref[b, :, :l]), (b, l)
        assert (got[b, :, l:] == 0).all()
        if l < OW:
            assert (ref[b, :, l:] != 0).any()
    assert _bits_to_float(s1) == float(got.abs().max())


@pytest.mark.parametrize("mode", [0, 1])
def test_masked_stats_pool(mode):
    from pytorch_kaldi_resnet_amd import ops
    torch.manual_seed(2)
    B, H, W, C = 4, 5, 19, 64
    L = [19, 7, 2, 1]
    x = torch.rand(B, H, W, C, device="cuda")
    for b, l in enumerate(L):
        x[b, :, l:] = float("nan")
    got = ops.stats_pool_fwd(x, mode, wlen=torch.tensor(L, dtype=torch.int32, device="cuda"))
    for b, l in enumerate(L):
        ref = ops.stats_pool_fwd(x[b:b + 1, :, :l].contiguous(), mode)
        torch.testing.assert_close(got[b:b + 1], ref, rtol=0, atol=0, equal_nan=True)
    assert torch.isfinite(got[:3]).all()
    assert torch.isnan(got[3]).any() == (mode == 1)


def test_conv_entry_refuses_the_mask_on_forms_without_it():
    from pytorch_kaldi_resnet_amd import hip, ops
    x = torch.randn(2, 8, 16, 64, device="cuda")
    w = ops.pack_conv_weight(torch.randn(64, 64, 3, 3, device="cuda") * 0.05)
    wl = torch.tensor([16, 3], dtype=torch.int32, device="cuda")
    raw = torch.randn_like(x)
    with pytest.raises(RuntimeError, match="WMASK"):       # the fused BatchNorm-backward form has no length mask
        ops._conv_launch(x, w, torch.empty_like(x), 64, [(kh - 1, kw - 1, kh * 3 + kw) for kh in range(3) for kw in range(3)],
                         1, 1, 0, 0, 8, 16, None, None, None, False, False,
                         in_bnbwd=(raw, None, torch.ones(4, 64, device="cuda"), torch.ones(3, 64, device="cuda")),
                         side=(torch.empty_like(x), None), split=ops.split_for(3, True),
                         in_amax=ops._amax_fwd_fallback(x, None), wlen=wl)
    lib = hip.lib()
    assert lib.spk_stem_conv_fwd(1, 1, 1, None, None, None, 1, 8, 8, hip.EPI_WMASK, None, None) < 0
    assert b"WMASK" in lib.spk_last_error()


# ---- extraction -------------------------------------------------------------------------------------------------------------

def _read_vectors(path, fmt):
    from pytorch_kaldi_resnet_amd import kaldi_io
    if fmt == "fv":
        return {k: np.asarray(v, dtype=np.float32) for k, v in kaldi_io.read_vec_flt_ark(path)}
    out = {}
    for line in open(path):
        key, rest = line.split(" ", 1)
        assert key not in out, key
        out[key] = np.array(rest.strip().strip("[]").split(), dtype=np.float32)
    return out


def test_decode_pad_batches_matches_bucketed(tmp_path):
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import kaldi_io
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    F, S = 40, 12
    rng = np.random.RandomState(5)
    lens = rng.choice(np.arange(120, 421), size=60, replace=False)
    ark, scp = str(tmp_path / "feats.ark"), str(tmp_path / "feats.scp")
    with open(ark, "wb") as f, open(scp, "w") as s:
        for i, n in enumerate(lens):
            key = "utt%03d" % i
            f.write(key.encode() + b" ")
            off = f.tell()
            kaldi_io.write_mat(f, rng.randn(int(n), F).astype(np.float32))
            s.write("%s %s:%d\n" % (key, ark, off))
    npst = W.make_state(21, S, F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    ckpt = str(tmp_path / "model.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 1}, ckpt)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    for fmt in ("text", "fv"):
        res = {}
        for mode in ("bucketed", "padded"):
            out = str(tmp_path / ("%s_%s" % (mode, fmt)))
            cmd = [sys.executable, os.path.join(ROOT, "scripts", "decode.py"), "--spk_num", str(S), "--arch", "resnet34",
                   "--input-dim", str(F), "--pooling", "mean+std", "--model-path", ckpt, "--decode-scp", scp, "--out-path", out,
                   "--native-reader", "--batch-size", "16", "--out-format", fmt] + (["--pad-batches"] if mode == "padded" else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            res[mode] = _read_vectors(os.path.join(out, "alone"), fmt)
        assert sorted(res["padded"]) == sorted(res["bucketed"]) == sorted("utt%03d" % i for i in range(60))
        keys = sorted(res["bucketed"])
        a = np.stack([res["padded"][k] for k in keys])
        b = np.stack([res["bucketed"][k] for k in keys])
        for i in range(len(keys)):
            assert close(a[i:i + 1], b[i:i + 1]), (fmt, keys[i])
    # without --native-reader the flag is an error
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "decode.py"), "--arch", "resnet34", "--input-dim", str(F),
                        "--pooling", "mean+std", "--pad-batches"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--native-reader" in r.stderr
