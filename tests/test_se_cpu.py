"""SE-ResNet-34 without a GPU: the restated trunk of tests/se_ref.py against the fixtures recorded from the reference, the
per-kernel backward formulas of csrc/se.hip against fp64 autograd, and the host side of the model (key list, arena layout,
loadParameters)."""
import json
import os

import numpy as np
import pytest
import torch

import se_ref
from oracle import masked
from oracle import spk_oracle as O
from oracle import weights as W

NAME = "se_r34_aam"


@pytest.fixture(scope="module")
def case(gold_dir):
    meta = json.load(open(os.path.join(gold_dir, NAME + ".json")))
    g = np.load(os.path.join(gold_dir, NAME + ".npz"))
    npst = se_ref.make_state(meta["seed"], meta["spk_num"], meta["feat_dim"], meta["pooling"], meta["loss"])
    x, y = W.make_input(meta["seed"] + 1, meta["batch"], meta["feat_dim"], meta["frames"], meta["spk_num"])
    return meta, g, npst, x, y


def close(a, b, rel):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.abs(a - b).max() <= rel * np.abs(b).max(), (np.abs(a - b).max(), np.abs(b).max())


def test_state_spec_is_the_reference_key_list(gold_dir):
    keys = json.load(open(os.path.join(gold_dir, "state_keys_se_resnet34_AAM.json")))
    spec = se_ref.state_spec(7, 80, "mean+std", "AAM")
    assert [k for k, *_ in spec] == [k for k, _ in keys]
    assert [list(s) for _, s, *_ in spec] == [s for _, s in keys]
    assert len(keys) == 251 and sum(".se.fc." in k for k, _ in keys) == 32


def test_se_ref_reproduces_the_reference(case):
    """tolerances of tests/test_oracle_golden.py::test_forward_backward_vs_reference"""
    meta, g, npst, x, y = case
    assert meta["gate_range"]["eval"][0] < 0.1 and meta["gate_range"]["eval"][1] > 0.9
    st = O.to_torch_state(npst)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    with torch.no_grad():
        close(se_ref.embed(st, xt, meta["pooling"], train=False).numpy(), g["emb_eval"], 2e-6)
        close(se_ref.forward(st, xt, yt, meta["pooling"], meta["loss"], train=False).numpy(), g["logits_eval"], 2e-6)
    keys = O.trainable_keys(st)
    assert keys == meta["param_names"]
    for k in keys:
        st[k].requires_grad_(True)
    logits = se_ref.forward(st, xt, yt, meta["pooling"], meta["loss"], train=True)
    lv = O.cross_entropy(logits, yt)
    close(logits.detach().numpy(), g["logits_train"], 2e-6)
    assert abs(float(lv.detach()) - float(g["loss_train"])) <= 1e-5
    gs = torch.autograd.grad(lv, [st[k] for k in keys])
    for i, (n, gi) in enumerate(zip(keys, gs)):
        ref_norm = float(g["grad_norm"][i])
        assert abs(float(gi.double().norm()) - ref_norm) <= 1e-4 * ref_norm + 1e-5, n
    for key in g.files:
        if key.startswith("rm:"):
            np.testing.assert_allclose(st[key[3:] + ".running_mean"].numpy(), g[key], rtol=1e-5, atol=1e-6)
        if key.startswith("rv:"):
            np.testing.assert_allclose(st[key[3:] + ".running_var"].numpy(), g[key], rtol=1e-5, atol=1e-6)
    assert "rm:res.layer1.0.bn2" in g.files and "rm:res.layer4.2.bn2" in g.files


def test_masks_include_the_hidden_relu(case):
    """oracle.masked records one mask per ReLU call: the stem, and per block bn1's, the gate's hidden one [B, C/16], the output's"""
    meta, g, npst, x, y = case
    st = O.to_torch_state(npst)
    with se_ref.oracle_knows_se():
        lo, masks = masked.record_masks(st, torch.from_numpy(x), torch.from_numpy(y), meta["pooling"], meta["loss"], se_ref.ARCH)
        assert len(masks) == 1 + 3 * 16
        assert tuple(masks[2].shape) == (meta["batch"], 2) and tuple(masks[-2].shape) == (meta["batch"], 16)
        lv, _ = masked.grads(npst, x, y, meta["pooling"], meta["loss"], se_ref.ARCH, masks, dtype=torch.float32)
    assert abs(lv - float(g["loss_train"])) <= 1e-5
    with pytest.raises(KeyError):
        O.trunk(st, torch.from_numpy(x), se_ref.ARCH)           # the patch is gone outside the block


@pytest.mark.parametrize("B,H,Wd,C", [(3, 5, 7, 32), (2, 3, 4, 64), (1, 1, 1, 32)])
def test_table_formulas_equal_autograd(B, H, Wd, C):
    """reduce -> gate -> apply, with bn2's backward statistics taken from the [B,C] tables, is the fp64 autograd gradient"""
    torch.manual_seed(B * 100 + C)
    raw2 = torch.randn(B, H, Wd, C, dtype=torch.float64) * 1.5 + 0.3
    r = torch.randn(B, H, Wd, C, dtype=torch.float64)
    gamma, beta = torch.rand(C, dtype=torch.float64) + 0.5, torch.randn(C, dtype=torch.float64) * 0.3
    w1 = torch.randn(C // 16, C, dtype=torch.float64) * 0.5
    w2 = torch.randn(C, C // 16, dtype=torch.float64) * 2.0
    dout = torch.randn(B, H, Wd, C, dtype=torch.float64)
    ag = se_ref.block_tail_autograd(raw2, r, gamma, beta, w1, w2, dout)
    tb = se_ref.block_tail_tables(raw2, ag["mask"], gamma, beta, w1, w2, dout)
    assert 0 < float(ag["mask"].double().mean()) < 1
    for k in ("g", "draw", "dr", "dgamma", "dbeta", "dW1", "dW2"):
        scale = float(ag[k].abs().max())
        assert float((tb[k] - ag[k]).abs().max()) <= 1e-11 * max(scale, 1e-3), k


@pytest.fixture(scope="module")
def hip_model():
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    return NeuralSpeakerModel(10, 80, "mean+std", "AAM", arch="se_resnet34")


def test_model_has_the_reference_keys(hip_model, gold_dir):
    keys = json.load(open(os.path.join(gold_dir, "state_keys_se_resnet34_AAM.json")))
    sd = hip_model.state_dict()
    assert list(sd.keys()) == [k for k, _ in keys]
    for k, shape in keys:
        want = [10, 256] if k == "last.weight" else shape          # the key list was recorded with 7 speakers
        assert list(sd[k].shape) == want, k
    meta = json.load(open(os.path.join(gold_dir, NAME + ".json")))
    assert [n for n, _ in hip_model.named_parameters()] == meta["param_names"]


def test_se_parameters_lie_inside_their_stage_slice(hip_model):
    """the flat arenas are cut per ResNet stage (parallel.stage_slices: the all-reduce buckets): the slices stay disjoint and
    cover the arena, every se.fc.* tensor sits inside the slice of its own stage, and is initialised like nn.Linear
    (|w| <= 1 / sqrt(fan_in))"""
    from pytorch_kaldi_resnet_amd.parallel import stage_slices
    m = hip_model
    flat = m.flat_parameters()
    sl = stage_slices(m)
    spans = sorted(sl.values())
    assert spans[0][0] == 0 and spans[-1][1] == flat.numel()
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    seen = 0
    for n, p in m.named_parameters():
        if ".se.fc." not in n:
            continue
        o = (p.data_ptr() - flat.data_ptr()) // 4
        lo, hi = sl[n.split(".")[1]]
        assert lo <= o and o + p.numel() <= hi, n
        assert 0 < float(p.abs().max()) <= 1.0 / np.sqrt(p.shape[1]), n
        seen += 1
    assert seen == 32


def test_load_parameters_takes_module_prefixed_keys(hip_model, case, capsys):
    meta, g, npst, x, y = case
    hip_model.loadParameters({"module." + k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    assert "is not in the model" not in capsys.readouterr().out
    sd = hip_model.state_dict()
    for k, v in npst.items():
        assert np.array_equal(sd[k].numpy(), v), k


def test_other_archs_unchanged_and_unknown_refused():
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    assert len(NeuralSpeakerModel(7, 80, "mean+std", "AAM").state_dict()) == 219
    with pytest.raises(NotImplementedError):
        NeuralSpeakerModel(7, 80, "mean+std", "AAM", arch="thin_resnet34")
