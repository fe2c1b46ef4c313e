"""End-to-end parity of the HIP model against the reference-generated golden fixtures and the CPU oracle.

What is compared, and why these tolerances:
  * eval-mode embeddings / logits and train-mode logits / loss (forward only): well conditioned; the BASELINE
    bar is cosine >= 1 - 1e-4, asserted: 1e-6 on cosine, 2e-5 scale-relative on values, 1e-4 on the train-mode loss at
    step 0 - 2e-4 for ResNet-101 at batch 2, whose train-mode BatchNorm over two utterances amplifies
    forward rounding (measured 1.1e-4).
  * gradients (test_backward_parity): against the fp64 gradient of the SAME piecewise-linear function - the oracle forward
    replayed with the ReLU masks the HIP forward chose (oracle/masked.py) - within 3x the CPU fp32 path's own error under
    the same yardstick (4x for the heads with a BatchNorm1d over 3-4 embeddings), no additive slack; the masks themselves
    within the CPU fp32 path's (Poisson) disagreement with the fp64 forward; the free-running comparison keeps a budget
    derived from the flip count; every parameter's gradient norm against the norms recorded from the reference.
  * loss curve over 5 SGD steps: step 0 within 1e-4, later steps within a budget derived from the reference's measured
    distance to ITSELF under 1-ulp input noise and fp64 arithmetic (loss_curve_tol, tests/golden/ref_sensitivity.json).
  * the same comparisons at the size of the headline (batch 256, 300 frames, 1211 speakers) between the operand modes:
    tests/test_fullsize_gpu.py.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import spk_oracle as O  # noqa: E402
from oracle import weights as W  # noqa: E402
from helpers import assert_samemask_parity, hip_step_with_masks, oracle_reference  # noqa: E402

def loss_curve_tol(gold_dir, name):
    """|loss - recorded reference loss| budget per SGD step of the recorded 5-step curves.  SURVEY.md section 8c asks for
    1e-4 at step 0 and <= 1e-3 by step 5; the reference itself does not meet the latter against ITSELF: with every input
    value moved by at most one unit in the last place (what another correct fp32 summation order does) its own step-4 loss
    moves by up to 9.5e-3, and its fp64 run differs from its fp32 run by 4.5e-3 (tools/ref_sensitivity.py, imported
    reference, recorded in tests/golden/ref_sensitivity.json).  Budget: 1e-4 at step 0 (well conditioned), then 3x the
    larger of those two measured self-distances of the reference, never below 1e-4."""
    ent = json.load(open(os.path.join(gold_dir, "ref_sensitivity.json")))["cases"][name]
    own = [max(a, abs(b)) for a, b in zip(ent["perturb_ulp"]["max_abs_dloss"], ent["fp64_minus_recorded"])]
    return [1e-4] + [max(1e-4, 3.0 * v) for v in own[1:]]


CASES = ["c1_r34_aam", "r34_aam_t203", "r34_aam_t300", "r34_softmax_mean_f40", "r34_aamv1_f40", "r101_aam"]


@pytest.fixture(autouse=True, params=["bf16x6", "f32", "f16x3"])
def mfma_mode(request):
    """Every model-level parity test runs in the default operand mode (fp32 operands as three bf16 terms, 6 cross products
    on the bf16 matrix instruction, fp32 accumulate) and on the native fp32 matrix instruction - same tolerances."""
    from pytorch_kaldi_resnet_amd import ops
    old = ops.SPLIT
    ops.SPLIT = ops.MFMA_MODES[request.param]
    yield request.param
    ops.SPLIT = old


@pytest.fixture(scope="module")
def P():
    assert torch.cuda.is_available()
    import pytorch_kaldi_resnet_amd as pkg
    from pytorch_kaldi_resnet_amd import model, optim  # noqa: F401
    return pkg


def build(P, meta):
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    m = NeuralSpeakerModel(meta["spk_num"], meta["feat_dim"], meta["pooling"], meta["loss"], 0.2, 30, arch=meta["arch"])
    npst = W.make_state(meta["seed"], meta["spk_num"], meta["feat_dim"], meta["pooling"], meta["loss"], meta["arch"])
    sd = {k: torch.from_numpy(np.array(v)) for k, v in npst.items()}
    m.load_state_dict(sd, strict=True)
    return m.cuda(), npst


def cos_dist(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float((1 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))).max())


def srel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", CASES)
def test_forward_parity(P, gold_dir, name):
    meta = json.load(open(os.path.join(gold_dir, name + ".json")))
    g = np.load(os.path.join(gold_dir, name + ".npz"))
    m, _ = build(P, meta)
    # state_dict naming / shapes are the reference's
    keys = json.load(open(os.path.join(gold_dir, "state_keys_%s_%s.json" % (meta["arch"], meta["loss"])))) \
        if os.path.exists(os.path.join(gold_dir, "state_keys_%s_%s.json" % (meta["arch"], meta["loss"]))) else None
    if keys:
        sd = m.state_dict()
        assert list(sd.keys()) == [k for k, _ in keys]
    x, y = W.make_input(meta["seed"] + 1, meta["batch"], meta["feat_dim"], meta["frames"], meta["spk_num"])
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    m.eval()
    with torch.no_grad():
        emb = m.predict(xg).cpu().numpy()
        lg = m(xg, yg).cpu().numpy()
    assert cos_dist(emb, g["emb_eval"]) < 1e-6          # BASELINE bar: 1e-4
    assert srel(emb, g["emb_eval"]) < 2e-5
    assert srel(lg, g["logits_eval"]) < 5e-5
    m.train()
    logits = m(xg, yg)
    loss = torch.nn.functional.cross_entropy(logits, yg)
    # train-mode BN over a batch of 2-4 utterances amplifies rounding differences more than eval mode
    assert srel(logits.detach().cpu().numpy(), g["logits_train"]) < 2e-4
    # 1e-4 at step 0.  ResNet-101 at batch 2 (33 Bottleneck blocks, train-mode BatchNorm over two utterances):
    # the reference itself moves this loss by 1.0-1.3e-4 when every input value is perturbed by <= 1 ulp and by 1.14e-4 between fp32
    # and fp64 (oracle run, round 4); budget = 3 x that self-distance, as for the loss curves.  Measured here:
    # 1.1e-4 ... 2.7e-4 depending on the operand mode and the summation order of the statistics
    assert abs(float(loss) - float(g["loss_train"])) < (4e-4 if name == "r101_aam" else 1e-4), name
    # BN running statistics after exactly one training forward
    sd = m.state_dict()
    for key in g.files:
        if key.startswith("rm:"):
            np.testing.assert_allclose(sd[key[3:] + ".running_mean"].cpu().numpy(), g[key], rtol=1e-4, atol=1e-5)
        if key.startswith("rv:"):
            np.testing.assert_allclose(sd[key[3:] + ".running_var"].cpu().numpy(), g[key], rtol=1e-4, atol=1e-5)
        if key.startswith("nbt:"):
            assert int(sd[key[4:] + ".num_batches_tracked"]) == int(g[key])


@pytest.mark.parametrize("name", ["c1_r34_aam", "r34_softmax_mean_f40", "r34_aamv1_f40", "r101_aam", "r34_aam_t300"])
def test_backward_parity(P, gold_dir, name):
    """Gradients against the fp64 oracle.

    (1) Arithmetic: the HIP gradient against the fp64 gradient of the SAME piecewise-linear function - the oracle forward
        replayed with the ReLU masks the HIP forward chose (oracle/masked.py).  The CPU fp32 oracle is held to the same
        yardstick with its own masks; the HIP error must be within 3x of it, no additive slack (measured: about 1x).
    (2) Forward agreement: the fraction of ReLU masks that differ from the fp64 forward's is at the fp32 rounding level
        (a few elements per network, like the CPU fp32 path's) - each differing element is a legitimate subgradient
        choice at |z| ~ 1e-5 but moves the free-running gradient comparison by ~1/sqrt(N) of a layer's gradient, which is
        why (3) the free-running comparison keeps a budget derived from the flip count instead of a constant."""
    from oracle import masked
    meta = json.load(open(os.path.join(gold_dir, name + ".json")))
    g = np.load(os.path.join(gold_dir, name + ".npz"))
    m, npst = build(P, meta)
    x, y = W.make_input(meta["seed"] + 1, meta["batch"], meta["feat_dim"], meta["frames"], meta["spk_num"])
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    m.train()
    names = [n for n, _ in m.named_parameters()]
    assert names == meta["param_names"]
    loss_hip, hip, masks_hip = hip_step_with_masks(m, xg, yg)
    kw = dict(pooling=meta["pooling"], loss=meta["loss"], arch=meta["arch"])

    def oracle_own(dtype):
        st = O.to_torch_state(npst)
        st = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in st.items()}
        keys = O.trainable_keys(st)
        for k in keys:
            st[k].requires_grad_(True)
        lo, masks = masked.record_masks(st, torch.from_numpy(x).to(dtype), torch.from_numpy(y), **kw)
        lv = O.cross_entropy(lo, torch.from_numpy(y))
        gs = torch.autograd.grad(lv, [st[k] for k in keys])
        return {k: v.double() for k, v in zip(keys, gs)}, masks

    g32, masks32 = oracle_own(torch.float32)
    g64, masks64 = oracle_own(torch.float64)
    assert [tuple(a.shape) for a in masks_hip] == [tuple(a.shape) for a in masks64]
    _, ref_hip = masked.grads(npst, x, y, masks=masks_hip, **kw)      # fp64 yardstick under the HIP forward's masks
    _, ref_32 = masked.grads(npst, x, y, masks=masks32, **kw)         # ... and under the CPU fp32 forward's masks

    def flat(d):
        return torch.cat([d[n].reshape(-1) for n in names])

    def rel(a, b):
        return float((flat(a) - flat(b)).norm() / flat(b).norm())

    # (1) arithmetic of the backward, mask choices factored out
    e_hip, e_cpu = rel(hip, ref_hip), rel(g32, ref_32)
    # per tensor, relative to that tensor's gradient norm - with a floor of 1e-3 of the largest tensor norm so that
    # analytically-zero gradients (fc1.bias in front of the head's BatchNorm1d) are judged on an absolute scale
    floor = 1e-3 * max(float(ref_hip[n].norm()) for n in names)
    worst = max(float((hip[n] - ref_hip[n]).norm() / max(float(ref_hip[n].norm()), floor)) for n in names)
    worst_cpu = max(float((g32[n] - ref_32[n]).norm() / max(float(ref_32[n].norm()), floor)) for n in names)
    print("same-mask gradient error vs fp64: hip %.3e (worst tensor %.3e)  cpu-fp32 %.3e (worst tensor %.3e)" % (
        e_hip, worst, e_cpu, worst_cpu))
    # 3x the CPU fp32 path's own error; 4x for the heads with a BatchNorm1d over the batch of 3-4 embeddings: there the error
    # is one common factor on every tensor (tools/diag_samemask.py) - the forward's fp32 rounding of the embeddings amplified
    # by |mean| / std of a 4-sample BatchNorm - and the HIP forward's rms rounding error is 1.5x the CPU path's (sequential
    # accumulation inside the matrix instruction against MKL's blocked sums; tools/diag_fwd.py), measured ratio 2.5 - 3.1
    bound = 4.0 if meta["loss"] in ("softmax", "AAM-v1") else 3.0
    assert e_hip <= bound * e_cpu, (e_hip, e_cpu)
    assert worst <= bound * worst_cpu + 1e-5, (worst, worst_cpu)
    # (2) mask agreement with the fp64 forward
    n_el = sum(a.numel() for a in masks64)
    flips_hip = sum(int((a != b).sum()) for a, b in zip(masks_hip, masks64))
    flips_cpu = sum(int((a != b).sum()) for a, b in zip(masks32, masks64))
    print("ReLU masks differing from the fp64 forward: hip %d, cpu-fp32 %d of %d" % (flips_hip, flips_cpu, n_el))
    assert flips_hip <= 3 * flips_cpu + 2e-6 * n_el + 4     # Poisson counts: mean ~ (fp32 forward error ~1e-5) x density x N
    # (3) free-running comparison (each path with its own masks): budget = the fp32 oracle's own error + what the
    # differing masks can move (rms over the layers they sit in is bounded by sqrt(flips / smallest layer size))
    smallest = min(a.numel() for a in masks64)
    e_free, e_free_cpu = rel(hip, g64), rel(g32, g64)
    print("free-running gradient error vs fp64: hip %.3e cpu-fp32 %.3e" % (e_free, e_free_cpu))
    assert e_free <= 3.0 * e_free_cpu + 2.0 * (flips_hip / smallest) ** 0.5 + 3.0 * e_hip
    # golden norms recorded from the reference itself
    # (2 %, or 1.5x the fp32 oracle's own whole-gradient error against fp64 where that is larger: ResNet-101 at batch 2)
    tol = max(2e-2, 1.5 * e_free_cpu)
    for i, n in enumerate(names):
        ref = float(g["grad_norm"][i])
        assert abs(float(hip[n].norm()) - ref) <= tol * ref + 1e-5, n
    assert abs(loss_hip - float(g["loss_train"])) < (4e-4 if name == "r101_aam" else 1e-4), name      # (budget: see test_forward_parity)


def test_fused_step_equals_autograd_path(P, gold_dir):
    meta = json.load(open(os.path.join(gold_dir, "c1_r34_aam.json")))
    m, _ = build(P, meta)
    x, y = W.make_input(meta["seed"] + 1, meta["batch"], meta["feat_dim"], meta["frames"], meta["spk_num"])
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    m.train()
    logits = m(xg, yg)
    loss = torch.nn.functional.cross_entropy(logits, yg)
    loss.backward()
    g1 = m.flat_grads().clone()
    l1 = float(loss)
    m2, _ = build(P, meta)
    m2.train()
    loss2, logits2, rank = m2.engine().loss_and_grad(xg, yg)
    assert abs(float(loss2) - l1) < 1e-5
    g2 = m2.flat_grads()
    assert float((g1 - g2).norm() / g1.norm()) < 1e-5
    acc1 = O.accuracy(logits2.cpu(), torch.from_numpy(y), (1,))[0]
    assert abs(float((rank.cpu() < 1).float().mean() * 100) - float(acc1)) < 1e-4
    # gradient accumulation semantics: a second backward without zero_grad adds onto the arena
    g2c = g2.clone()
    m2.engine().loss_and_grad(xg, yg)
    assert float((m2.flat_grads() - 2 * g2c).norm() / g2c.norm()) < 1e-5


def test_graphed_step_equals_eager(P, gold_dir):
    """The hipGraph-captured forward+CE+backward must reproduce the eager launch sequence bit for bit (same kernels,
    same order per stream), replay after replay, and keep BN running statistics advancing."""
    from pytorch_kaldi_resnet_amd.engine import GraphedTrainStep
    meta = json.load(open(os.path.join(gold_dir, "c1_r34_aam.json")))
    x, y = W.make_input(meta["seed"] + 1, meta["batch"], meta["feat_dim"], meta["frames"], meta["spk_num"])
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    m1, _ = build(P, meta)
    m1.train()
    l1, lg1, r1 = m1.engine().loss_and_grad(xg, yg)
    g1 = m1.flat_grads().clone()
    m2, _ = build(P, meta)
    m2.train()
    before = {k: v.clone() for k, v in m2.state_dict().items()}
    step = GraphedTrainStep(m2.engine(), meta["batch"], meta["frames"], warmup=1)
    for k, v in m2.state_dict().items():         # building the graph (dummy warm-up steps) must not touch the model
        assert torch.equal(v, before[k]), k
    m2.load_state_dict(m1.state_dict())
    m1b, _ = build(P, meta)
    m1b.load_state_dict(m1.state_dict())
    m1b.train()
    l1b, _, _ = m1b.engine().loss_and_grad(xg, yg)
    l2, lg2, r2 = step(xg, yg)
    assert float(l2) == float(l1b)
    assert torch.equal(m2.flat_grads(), m1b.flat_grads())
    assert torch.equal(m2.state_dict()["res.bn1.running_mean"], m1b.state_dict()["res.bn1.running_mean"])
    l3, _, _ = step(xg, yg)                        # second replay: same batch statistics, same loss
    assert float(l3) == float(l2)
    assert int(m2.state_dict()["res.bn1.num_batches_tracked"]) == int(m1b.state_dict()["res.bn1.num_batches_tracked"]) + 1


def test_graph_replay_trains_on_updated_weights(P, gold_dir):
    """graph -> SGD -> graph -> ... must be the eager step -> SGD -> step -> ... bit for bit (reference
    scripts/train_resnet.py:316-328: every forward runs on the weights optimizer.step() just wrote).  A captured step
    that does not re-pack the convolution weights keeps training on the weights of capture time: the losses then stop
    matching after the first update.  lr is large enough (1e-2) for every step to move the loss visibly."""
    from pytorch_kaldi_resnet_amd.engine import GraphedTrainStep
    from pytorch_kaldi_resnet_amd.optim import FlatSGD
    meta = json.load(open(os.path.join(gold_dir, "c1_r34_aam.json")))
    g = np.load(os.path.join(gold_dir, "c1_r34_aam.npz"))
    tol = loss_curve_tol(gold_dir, "c1_r34_aam")
    batches = []
    for s in range(5):
        xs, ys = W.make_input(meta["seed"] + 1 + s, meta["batch"], meta["feat_dim"], meta["frames"], meta["spk_num"])
        batches.append((torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda()))
    for lr, wd in ((1e-2, 5e-4), (meta["lr"], meta["wd"])):
        me, _ = build(P, meta)
        mg, _ = build(P, meta)
        me.train()
        mg.train()
        oe = FlatSGD(me, lr, momentum=0.9, weight_decay=wd)
        og = FlatSGD(mg, lr, momentum=0.9, weight_decay=wd)
        step = GraphedTrainStep(mg.engine(), meta["batch"], meta["frames"], warmup=1)
        assert torch.equal(mg.flat_parameters(), me.flat_parameters())      # building the graph left the weights alone
        le, lg = [], []
        for s, (xs, ys) in enumerate(batches):
            oe.zero_grad(set_to_none=True)
            l1, _, _ = me.engine().loss_and_grad(xs, ys)
            l2, _, _ = step(xs, ys)
            assert float(l1) == float(l2), (lr, s, float(l1), float(l2))
            assert torch.equal(me.flat_grads(), mg.flat_grads()), (lr, s)
            oe.step()
            og.step()
            assert torch.equal(me.flat_parameters(), mg.flat_parameters()), (lr, s)
            le.append(float(l1))
            lg.append(float(l2))
        print("lr %g: graph losses %s" % (lr, lg))
        if lr == 1e-2:
            # the update is visible: same batch again gives a different loss than before the 5 steps
            l_again, _, _ = step(*batches[0])
            assert abs(float(l_again) - lg[0]) > 1e-3
        else:
            # at the fixture's own lr the graph path meets the reference's recorded curve (same budget as the eager path)
            for i, (a, b) in enumerate(zip(lg, g["loss_curve"])):
                assert abs(a - b) <= tol[i], (i, a, b)
        # every replay re-packed: the packed weights now in use equal a fresh pack of the weights of the LAST forward
        assert step.pack_table.launches_captured == 1


@pytest.mark.parametrize("name", ["c1_r34_aam", "r34_softmax_mean_f40"])
def test_sgd_loss_curve(P, gold_dir, name):
    from pytorch_kaldi_resnet_amd.optim import FlatSGD
    meta = json.load(open(os.path.join(gold_dir, name + ".json")))
    g = np.load(os.path.join(gold_dir, name + ".npz"))
    m, _ = build(P, meta)
    opt = FlatSGD(m, meta["lr"], momentum=0.9, weight_decay=meta["wd"])
    m.train()
    losses = []
    for s in range(meta["steps"]):
        xs, ys = W.make_input(meta["seed"] + 1 + s, meta["batch"], meta["feat_dim"], meta["frames"], meta["spk_num"])
        xs, ys = torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda()
        out = m(xs, ys)
        loss = torch.nn.functional.cross_entropy(out, ys)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("loss curve", losses, list(g["loss_curve"]))
    tol = loss_curve_tol(gold_dir, name)[:len(losses)]
    print("per-step budget", tol, "deviation", [abs(a - b) for a, b in zip(losses, g["loss_curve"])])
    for i, (a, b) in enumerate(zip(losses, g["loss_curve"])):
        assert abs(a - b) <= tol[i], (i, a, b)
    x, _ = W.make_input(meta["seed"] + 1, meta["batch"], meta["feat_dim"], meta["frames"], meta["spk_num"])
    m.eval()
    with torch.no_grad():
        e2 = m.predict(torch.from_numpy(x).cuda()).cpu().numpy()
    assert cos_dist(e2, g["emb_after"]) < 1e-4


@pytest.mark.parametrize("arch,F,T,B,pooling,loss", [("resnet18", 30, 37, 3, "mean+std", "AAM"), ("resnet34", 80, 64, 1, "mean", "softmax"),
                                                    ("resnet50", 24, 45, 2, "mean+std", "AAM-v1"), ("resnet18", 80, 1001, 1, "mean+std", "AAM")])
def test_odd_shapes_against_oracle(P, arch, F, T, B, pooling, loss):
    """Ragged / minimal shapes the reference handles implicitly: feat_dim not a multiple of 8 (ceil at every stride-2
    stage, fc1 fan-in (F+7)//8), odd frame counts, batch 1, a long utterance (decode.py feeds whole utterances)."""
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    S = 7
    npst = W.make_state(21, S, F, pooling, loss, arch)
    m = NeuralSpeakerModel(S, F, pooling, loss, 0.2, 30, arch=arch)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    m = m.cuda()
    x, y = W.make_input(22, B, F, T, S)
    st = O.to_torch_state(npst)
    m.eval()
    with torch.no_grad():
        e = m.predict(torch.from_numpy(x).cuda()).cpu().numpy()
        eo = O.embed(st, torch.from_numpy(x), pooling, arch, train=False).numpy()
    assert e.shape == (B, 256) and cos_dist(e, eo) < 1e-6 and srel(e, eo) < 3e-5
    if B > 1:      # train-mode BN needs more than one value per channel in the head's BatchNorm1d
        m.train()
        lg = m(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
        lo = O.forward(st, torch.from_numpy(x), torch.from_numpy(y), pooling, loss, arch, train=True)
        assert srel(lg.detach().cpu().numpy(), lo.detach().numpy()) < 2e-4
        torch.nn.functional.cross_entropy(lg, torch.from_numpy(y).cuda()).backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters())
        # the backward of these shapes against the fp64 oracle under the HIP forward's own masks (test_backward_parity's
        # yardstick; 4x for the head with a BatchNorm1d over the batch, as there).  x4 where mean+std pooling sees a last stage
        # of <= 5 frames (resnet18 F30 T37: 4 x 5 features per channel): the pooled sqrt(row mean) has derivative 1/(2 sqrt(mean)),
        # so the few rows with a mean near 0 carry most of the gradient and turn the forward's absolute rounding error there into
        # a relative error of the whole gradient.  Measured per tensor (f32 operands): one common factor 8.5-14.8x the CPU fp32
        # path's from the head-most tensor (layer4.1.bn2) to the stem - the head and pooling kernels are the same in every operand
        # mode, only the forward convolutions' rounding differs (f16x3: 2.5x, bf16x6: 5.9x, f32: 10.6x overall), and the
        # last-stage features themselves stay within 1.6x of the CPU path's rms error against fp64 (3.3e-6 vs 2.1e-6)
        bound = 4.0 if loss in ("softmax", "AAM-v1") else 3.0
        if pooling == "mean+std" and -(-T // 8) <= 5:
            bound *= 4.0
        _, hip, masks_hip = hip_step_with_masks(m, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
        ref = oracle_reference(npst, x, y, pooling, loss, arch)
        assert_samemask_parity(ref, npst, x, y, pooling, loss, arch, hip, masks_hip, bound=bound,
                               tag="%s F%d T%d B%d" % (arch, F, T, B))


def test_cpu_input_is_refused(P):
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    m = NeuralSpeakerModel(5, 80, "mean+std", "AAM").cuda()
    with pytest.raises(RuntimeError):
        m.predict(torch.zeros(1, 80, 100))
