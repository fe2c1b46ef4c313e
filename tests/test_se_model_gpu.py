"""SE-ResNet-34 end to end on the GPU: parity with the fixtures recorded from the reference (tests/golden/se_r34_aam.*, written
by tools/make_se_golden.py) and with the restated trunk of tests/se_ref.py, at the tolerances of tests/test_model_gpu.py and
tests/test_masked_predict_gpu.py, in the three operand modes."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import se_ref  # noqa: E402
from helpers import ROOT, assert_samemask_parity, hip_relu_masks, oracle_reference  # noqa: E402
from oracle import spk_oracle as O  # noqa: E402
from oracle import weights as W  # noqa: E402

NAME = "se_r34_aam"
ARCH = se_ref.ARCH


@pytest.fixture(autouse=True, params=["bf16x6", "f32", "f16x3"])
def mfma_mode(request):
    from pytorch_kaldi_resnet_amd import ops
    old = ops.SPLIT
    ops.SPLIT = ops.MFMA_MODES[request.param]
    yield request.param
    ops.SPLIT = old


@pytest.fixture(scope="module")
def case(gold_dir):
    assert torch.cuda.is_available()
    meta = json.load(open(os.path.join(gold_dir, NAME + ".json")))
    g = np.load(os.path.join(gold_dir, NAME + ".npz"))
    npst = se_ref.make_state(meta["seed"], meta["spk_num"], meta["feat_dim"], meta["pooling"], meta["loss"])
    return meta, g, npst


def build(npst, S, F, pooling="mean+std", loss="AAM"):
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    m = NeuralSpeakerModel(S, F, pooling, loss, 0.2, 30, arch=ARCH)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()}, strict=True)
    return m.cuda()


def build_case(case):
    meta, _, npst = case
    return build(npst, meta["spk_num"], meta["feat_dim"], meta["pooling"], meta["loss"])


def batch(meta, s=0):
    x, y = W.make_input(meta["seed"] + 1 + s, meta["batch"], meta["feat_dim"], meta["frames"], meta["spk_num"])
    return x, y, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


def cos_dist(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float((1 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))).max())


def srel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())


def curve_tol(meta):
    """tests/test_model_gpu.py::loss_curve_tol on the self-distances of the reference recorded in this fixture's json: 1e-4 at
    step 0, then 3x the larger of (1-ulp input noise, fp64 against fp32), never below 1e-4"""
    ent = meta["ref_sensitivity"]
    own = [max(a, abs(b)) for a, b in zip(ent["perturb_ulp"]["max_abs_dloss"], ent["fp64_minus_recorded"])]
    return [1e-4] + [max(1e-4, 3.0 * v) for v in own[1:]]


def step_with_masks(m, xg, yg):
    """helpers.hip_step_with_masks with the SE hidden ReLU masks (u > 0, [B, C/16]) in the reference's call order: per block
    bn1's mask, the gate's hidden mask, the block output's"""
    from pytorch_kaldi_resnet_amd import ops
    eng = m.engine()
    m.attach_grads()
    for p in m.parameters():
        p.grad = None
    with torch.no_grad():
        logits, saved = eng.forward_train(xg.contiguous(), yg)
        plain = hip_relu_masks(eng, saved)                 # stem, then (bn1, out) per block
        masks = [plain[0]]
        for i, rec in enumerate(saved["blocks"]):
            masks += [plain[1 + 2 * i], (rec["se"][2] > 0).cpu(), plain[2 + 2 * i]]
        loss_row, dl, _ = ops.softmax_ce(logits, yg, grad_scale=1.0 / logits.shape[0])
        loss = float(ops.mean(loss_row))
        lg = logits.detach().cpu()
    eng.backward(saved, dl)
    torch.cuda.synchronize()
    return loss, {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}, masks, lg


def test_forward_parity(case, gold_dir):
    meta, g, _ = case
    m = build_case(case)
    keys = json.load(open(os.path.join(gold_dir, "state_keys_se_resnet34_AAM.json")))
    assert list(m.state_dict().keys()) == [k for k, _ in keys]
    x, y, xg, yg = batch(meta)
    m.eval()
    with torch.no_grad():
        emb = m.predict(xg).cpu().numpy()
        lg = m(xg, yg).cpu().numpy()
    print("eval: 1-cos %.3e srel %.3e logits srel %.3e" % (cos_dist(emb, g["emb_eval"]), srel(emb, g["emb_eval"]),
                                                          srel(lg, g["logits_eval"])))
    assert cos_dist(emb, g["emb_eval"]) < 1e-6
    assert srel(emb, g["emb_eval"]) < 2e-5
    assert srel(lg, g["logits_eval"]) < 5e-5
    m.train()
    logits = m(xg, yg)
    loss = torch.nn.functional.cross_entropy(logits, yg)
    print("train: logits srel %.3e |dloss| %.3e" % (srel(logits.detach().cpu().numpy(), g["logits_train"]),
                                                    abs(float(loss) - float(g["loss_train"]))))
    assert srel(logits.detach().cpu().numpy(), g["logits_train"]) < 2e-4
    assert abs(float(loss) - float(g["loss_train"])) < 1e-4
    sd = m.state_dict()
    seen = 0
    for key in g.files:
        if key.startswith("rm:"):
            np.testing.assert_allclose(sd[key[3:] + ".running_mean"].cpu().numpy(), g[key], rtol=1e-4, atol=1e-5)
            seen += 1
        if key.startswith("rv:"):
            np.testing.assert_allclose(sd[key[3:] + ".running_var"].cpu().numpy(), g[key], rtol=1e-4, atol=1e-5)
        if key.startswith("nbt:"):
            assert int(sd[key[4:] + ".num_batches_tracked"]) == int(g[key])
    assert seen == 5


_REF = {}


def same_mask_reference(key, npst, x, y, pooling, loss):
    """the implementation-independent part of the yardstick (CPU fp32 against fp64), once per input"""
    if key not in _REF:
        with se_ref.oracle_knows_se():
            _REF[key] = oracle_reference(npst, x, y, pooling, loss, ARCH)
    return _REF[key]


def test_backward_same_mask(case):
    """the HIP gradient against the fp64 gradient of the function the HIP forward differentiated (its own ReLU masks, the gate's
    hidden ones included) within 3x the CPU fp32 path's error under the same yardstick, overall and per tensor
    (helpers.assert_samemask_parity: the assertions and the floor of test_backward_parity); gradient norms against the reference's"""
    meta, g, npst = case
    m = build_case(case).train()
    x, y, xg, yg = batch(meta)
    assert [n for n, _ in m.named_parameters()] == meta["param_names"]
    loss, hip, masks, lg = step_with_masks(m, xg, yg)
    ref = same_mask_reference("case", npst, x, y, meta["pooling"], meta["loss"])
    with se_ref.oracle_knows_se():
        out = assert_samemask_parity(ref, npst, x, y, meta["pooling"], meta["loss"], ARCH, hip, masks, logits_hip=lg, bound=3.0,
                                     tag="se_resnet34")
    tol = max(2e-2, 1.5 * ref["e_free_cpu"])
    for i, n in enumerate(meta["param_names"]):
        rn = float(g["grad_norm"][i])
        assert abs(float(hip[n].norm()) - rn) <= tol * rn + 1e-5, n
    assert abs(loss - float(g["loss_train"])) < 1e-4
    print(out)


def test_window_counts_see_no_saturation(case, mfma_mode):
    """f16x3: every tensor a matrix-core kernel stages sits inside the fp16 window of its scale slot - the pair tensors written by
    spk_se_bwd_apply under the gate kernel's bound included"""
    if mfma_mode != "f16x3":
        return
    meta, _, _ = case
    m = build_case(case).train()
    _, _, xg, yg = batch(meta)
    eng = m.engine()
    eng.window_counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    eng.loss_and_grad(xg, yg)
    c = eng.window_counts.cpu()
    assert int(c[0]) > 0 and int(c[1]) == 0, c


def test_loss_curve_and_graph_replay(case):
    """3 SGD steps: the eager losses stay within the budget of the reference's own self-distance, and the graphed step equals
    the eager step bit for bit - losses, gradients and the weights after every update"""
    from pytorch_kaldi_resnet_amd.engine import GraphedTrainStep
    from pytorch_kaldi_resnet_amd.optim import FlatSGD
    meta, g, _ = case
    me, mg = build_case(case).train(), build_case(case).train()
    oe = FlatSGD(me, meta["lr"], momentum=0.9, weight_decay=meta["wd"])
    og = FlatSGD(mg, meta["lr"], momentum=0.9, weight_decay=meta["wd"])
    step = GraphedTrainStep(mg.engine(), meta["batch"], meta["frames"], warmup=1)
    assert torch.equal(mg.flat_parameters(), me.flat_parameters())
    losses = []
    for s in range(meta["steps"]):
        _, _, xs, ys = batch(meta, s)
        oe.zero_grad(set_to_none=True)
        l1, _, _ = me.engine().loss_and_grad(xs, ys)
        l2, _, _ = step(xs, ys)
        assert float(l1) == float(l2), (s, float(l1), float(l2))
        assert torch.equal(me.flat_grads(), mg.flat_grads()), s
        oe.step()
        og.step()
        assert torch.equal(me.flat_parameters(), mg.flat_parameters()), s
        losses.append(float(l1))
    tol = curve_tol(meta)
    print("losses", losses, "recorded", list(g["loss_curve"]), "budget", tol)
    for i, (a, b) in enumerate(zip(losses, g["loss_curve"])):
        assert abs(a - b) <= tol[i], (i, a, b)
    assert step.pack_table.launches_captured == 1
    # SGD reaches the gate matrices through the arena: in every stage some of them moved (a block whose hidden units are all dead
    # has zero gradients, as in the reference, and weight decay alone is below float32 resolution at this learning rate)
    npst = se_ref.make_state(meta["seed"], meta["spk_num"], meta["feat_dim"], meta["pooling"], meta["loss"])
    se_moved = [n for n, p in me.named_parameters() if ".se.fc." in n and not np.array_equal(p.detach().cpu().numpy(), npst[n])]
    assert {n.split(".")[1] for n in se_moved} == {"layer1", "layer2", "layer3", "layer4"}, se_moved


def test_autograd_path_and_accumulation(case):
    """loss.backward() through the autograd bridge fills the same arena as loss_and_grad; a second backward accumulates"""
    meta, _, _ = case
    _, _, xg, yg = batch(meta)
    m1 = build_case(case).train()
    torch.nn.functional.cross_entropy(m1(xg, yg), yg).backward()
    g1 = m1.flat_grads().clone()
    m2 = build_case(case).train()
    m2.engine().loss_and_grad(xg, yg)
    g2 = m2.flat_grads().clone()
    assert float((g1 - g2).norm() / g1.norm()) < 1e-5
    m2.engine().loss_and_grad(xg, yg)
    assert float((m2.flat_grads() - 2 * g2).norm() / g2.norm()) < 1e-5


def test_odd_shape_against_se_ref():
    """F 30 (ceil at every stride-2 stage), T 37, B 3: eval embeddings, train logits and the same-mask backward against se_ref.
    Tolerances of test_model_gpu.py::test_odd_shapes_against_oracle, its x4 on the gradient bound for mean+std pooling over a last
    stage of <= 5 frames included (the pooled sqrt(row mean) at a mean near 0 carries most of the gradient)."""
    S, F, T, B = 7, 30, 37, 3
    npst = se_ref.make_state(21, S, F, "mean+std", "AAM")
    m = build(npst, S, F)
    x, y = W.make_input(22, B, F, T, S)
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    st = O.to_torch_state(npst)
    m.eval()
    with torch.no_grad():
        e = m.predict(xg).cpu().numpy()
        eo = se_ref.embed(st, torch.from_numpy(x), "mean+std", train=False).numpy()
    assert e.shape == (B, 256) and cos_dist(e, eo) < 1e-6 and srel(e, eo) < 3e-5
    m.train()
    _, hip, masks, lg = step_with_masks(m, xg, yg)
    lo = se_ref.forward(st, torch.from_numpy(x), torch.from_numpy(y), "mean+std", "AAM", train=True)
    assert srel(lg.numpy(), lo.detach().numpy()) < 2e-4
    assert all(bool(torch.isfinite(v).all()) for v in hip.values())
    ref = same_mask_reference("odd", npst, x, y, "mean+std", "AAM")
    with se_ref.oracle_knows_se():
        assert_samemask_parity(ref, npst, x, y, "mean+std", "AAM", ARCH, hip, masks, bound=3.0 * 4.0, tag="se_resnet34 F30 T37 B3")


LENGTHS = [75, 41, 9, 1]


def test_masked_predict(case):
    """predict(x, lengths=): row b is the solo predict of x[b:b+1, :, :L[b]] at test_masked_predict_gpu.py's bar (cosine 1e-6,
    values 2e-5 scale-relative; L = 1 pools one frame: the unbiased variance is NaN in the reference too - the same entries
    must be NaN), against se_ref as well, and bitwise whatever the padding holds"""
    meta, _, npst = case
    m = build_case(case).eval()
    x, _, _, _ = batch(meta)
    x = torch.from_numpy(x)
    st = O.to_torch_state(npst)

    def padded(fill):
        xp = x.clone()
        for b, l in enumerate(LENGTHS):
            if fill == "zero":
                xp[b, :, l:] = 0
            elif fill == "random":
                xp[b, :, l:] = (torch.rand(x.shape[1], x.shape[2] - l, generator=torch.Generator().manual_seed(b)) * 2 - 1) * 1e3
            else:
                xp[b, :, l:] = float("nan")
        return xp.cuda()

    with torch.no_grad():
        outs = [m.predict(padded(f), lengths=LENGTHS) for f in ("zero", "random", "nan")]
        solo = [m.predict(x[b:b + 1, :, :l].contiguous().cuda()).cpu().numpy() for b, l in enumerate(LENGTHS)]
        ref = [se_ref.embed(st, x[b:b + 1, :, :l], meta["pooling"], train=False).numpy() for b, l in enumerate(LENGTHS)]
    assert torch.equal(outs[0].isnan(), outs[1].isnan()) and torch.equal(outs[0].isnan(), outs[2].isnan())
    assert torch.equal(outs[0].nan_to_num(), outs[1].nan_to_num()) and torch.equal(outs[0].nan_to_num(), outs[2].nan_to_num())
    emb = outs[0].cpu().numpy()
    for b, l in enumerate(LENGTHS):
        row = emb[b:b + 1]
        if np.isnan(ref[b]).any():
            assert l == 1 and np.array_equal(np.isnan(row), np.isnan(ref[b])) and np.array_equal(np.isnan(row), np.isnan(solo[b]))
            continue
        assert np.isfinite(row).all(), l
        assert cos_dist(row, solo[b]) < 1e-6 and srel(row, solo[b]) < 2e-5, (l, cos_dist(row, solo[b]), srel(row, solo[b]))
        assert cos_dist(row, ref[b]) < 1e-6 and srel(row, ref[b]) < 2e-5, (l, cos_dist(row, ref[b]), srel(row, ref[b]))
    with torch.no_grad():
        full = m.predict(x.cuda(), lengths=[x.shape[2]] * x.shape[0])
        assert torch.equal(full, m.predict(x.cuda()))


def test_checkpoint_round_trip(case, tmp_path):
    """scripts/train_resnet.py's checkpoint (save_checkpoint: 'module.'-prefixed state dict as a distributed run writes it + the
    optimizer state) read back the way its --resume branch does (loadParameters, FlatSGD.load_state_dict): the resumed model
    continues bit-identically - weights, BatchNorm buffers and the momentum buffers of the SE matrices included"""
    from pytorch_kaldi_resnet_amd.optim import FlatSGD
    spec = importlib.util.spec_from_file_location("spk_train_script", os.path.join(ROOT, "scripts", "train_resnet.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    meta, _, npst = case
    a = build_case(case).train()
    oa = FlatSGD(a, 1e-2, momentum=0.9, weight_decay=meta["wd"])
    for s in range(2):
        _, _, xs, ys = batch(meta, s)
        oa.zero_grad(set_to_none=True)
        a.engine().loss_and_grad(xs, ys)
        oa.step()
    path = str(tmp_path / "checkpoint_epoch0.pth.tar")
    script.save_checkpoint({"epoch": 1, "arch": ARCH, "state_dict": {"module." + k: v for k, v in a.state_dict().items()},
                            "best_acc1": torch.as_tensor(0.0), "optimizer": oa.state_dict()}, False, path)
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert ckpt["arch"] == ARCH and len(ckpt["state_dict"]) == 251
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    b = NeuralSpeakerModel(meta["spk_num"], meta["feat_dim"], meta["pooling"], meta["loss"], 0.2, 30, arch=ARCH)
    b.loadParameters(ckpt["state_dict"])
    b = b.cuda().train()
    ob = FlatSGD(b, 1e-2, momentum=0.9, weight_decay=meta["wd"])
    ob.load_state_dict(ckpt["optimizer"])
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    _, _, xs, ys = batch(meta, 2)
    for m, o in ((a, oa), (b, ob)):
        o.zero_grad(set_to_none=True)
        m.engine().loss_and_grad(xs, ys)
        o.step()
    assert torch.equal(a.flat_parameters(), b.flat_parameters())
    sa, sb = oa.state_dict(), ob.state_dict()
    names = [n for n, _ in a.named_parameters()]
    se_idx = [i for i, n in enumerate(names) if ".se.fc." in n]
    assert len(se_idx) == 32
    for i, ent in sa["state"].items():
        assert torch.equal(ent["momentum_buffer"], sb["state"][i]["momentum_buffer"]), names[i]
    assert all(float(sa["state"][i]["momentum_buffer"].abs().max()) > 0 for i in se_idx)
