#!/usr/bin/env python3
"""Generate the SE-ResNet-34 fixtures under tests/golden/ by running the REFERENCE itself on the CPU (build container only).

Like tools/make_golden.py: imports the reference's scripts/model.py unmodified, puts its own `se_resnet34()` trunk into
NeuralSpeakerModel (the reference parses --arch but always builds resnet34, scripts/train_resnet.py:42,152), loads the
hash-filled state of tests/se_ref.py through load_state_dict(strict=True) and records the same fields as make_golden's
record_case, the running statistics of the first and the last SE block's bn2, and how far the reference's OWN loss curve moves
under 1-ulp input noise and in fp64 (the method of tools/ref_sensitivity.py) - the budget of the loss-curve tests.
Only arrays and names are written; no reference source travels.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_se_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "scripts"))
sys.dont_write_bytecode = True

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import se_ref  # noqa: E402
from oracle import weights as W  # noqa: E402
from tools.make_golden import sample_idx  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.manual_seed(0)
torch.set_num_threads(8)
RUNNING = ["res.bn1", "res.layer1.0.bn1", "res.layer2.0.downsample.1", "res.layer1.0.bn2", "res.layer4.2.bn2"]


def ref_model(spk_num, feat_dim, pooling, loss, seed, dtype=torch.float32):
    import model as refmodel
    m = refmodel.NeuralSpeakerModel(spk_num=spk_num, feat_dim=feat_dim, pooling=pooling, loss=loss, m=0.2, s=30)
    m.res = refmodel.se_resnet34()
    st = se_ref.make_state(seed, spk_num, feat_dim, pooling, loss)
    assert list(m.state_dict().keys()) == list(st.keys()), "tests/se_ref.py does not restate the reference's key order"
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()}, strict=True)
    return m.to(dtype)


def gate_range(m, x, train):
    """smallest and largest SE gate of one forward (forward hooks on the Sigmoid modules; the state is put back afterwards)"""
    gates = []
    hooks = [mod.register_forward_hook(lambda _m, _i, o: gates.append(o.detach())) for mod in m.modules()
             if isinstance(mod, nn.Sigmoid)]
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.train(train)
    with torch.no_grad():
        m.predict(x)
    for h in hooks:
        h.remove()
    m.load_state_dict(sd)
    return min(float(g.min()) for g in gates), max(float(g.max()) for g in gates)


def curve(meta, dtype=torch.float32, eps=0.0, pseed=0):
    """the loop of scripts/train_resnet.py:304-328 (tools/ref_sensitivity.py: curve)"""
    m = ref_model(meta["spk_num"], meta["feat_dim"], meta["pooling"], meta["loss"], meta["seed"], dtype).train()
    crit = nn.CrossEntropyLoss()
    opt = torch.optim.SGD(m.parameters(), meta["lr"], momentum=0.9, weight_decay=meta["wd"])
    rng = np.random.RandomState(1000 + pseed)
    losses = []
    for s in range(meta["steps"]):
        xs, ys = W.make_input(meta["seed"] + 1 + s, meta["batch"], meta["feat_dim"], meta["frames"], meta["spk_num"])
        if eps:
            xs = (xs.astype(np.float64) * (1.0 + eps * rng.uniform(-1, 1, xs.shape))).astype(np.float32)
        xs, ys = torch.from_numpy(xs).to(dtype), torch.from_numpy(ys)
        loss = crit(m(xs, ys), ys)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return np.array(losses)


def record_case(name, spk_num, feat_dim, frames, batch, pooling, loss, seed, steps, lr=2e-5, wd=5e-4):
    print("case", name)
    m = ref_model(spk_num, feat_dim, pooling, loss, seed)
    x_np, y_np = W.make_input(seed + 1, batch, feat_dim, frames, spk_num)
    x, y = torch.from_numpy(x_np), torch.from_numpy(y_np)
    # the two forwards the fixture records: eval mode (running statistics of the fill: the squeezed means are far from beta) and
    # training mode (batch statistics: the squeezed means stay near beta, the gates nearer 0.5)
    ranges = {"eval": gate_range(m, x, False), "train": gate_range(m, x, True)}
    print("SE gates span", ranges)
    gmin, gmax = min(r[0] for r in ranges.values()), max(r[1] for r in ranges.values())
    assert gmin < 0.1 and gmax > 0.9, "the gates do not span (0, 1): a kernel that ignored them would nearly pass"
    out = {}
    m.eval()
    with torch.no_grad():
        out["emb_eval"] = m.predict(x).numpy()
        out["logits_eval"] = m(x, y).numpy()
    m.train()
    crit = nn.CrossEntropyLoss()
    opt = torch.optim.SGD(m.parameters(), lr, momentum=0.9, weight_decay=wd)
    logits = m(x, y)
    lossv = crit(logits, y)
    opt.zero_grad()
    lossv.backward()
    out["logits_train"] = logits.detach().numpy()
    out["loss_train"] = np.array(float(lossv))
    names = [n for n, _ in m.named_parameters()]
    gnorm, gsamp = [], []
    for i, (n, p) in enumerate(m.named_parameters()):
        g = p.grad.detach().reshape(-1).numpy()
        gnorm.append(np.sqrt((g.astype(np.float64) ** 2).sum()))
        gsamp.append(g[sample_idx(g.size, i)])
    out["grad_norm"] = np.array(gnorm)
    out["grad_samples"] = np.stack(gsamp).astype(np.float32)
    sd = m.state_dict()
    for key in RUNNING:
        out["rm:" + key] = sd[key + ".running_mean"].numpy().copy()
        out["rv:" + key] = sd[key + ".running_var"].numpy().copy()
        out["nbt:" + key] = sd[key + ".num_batches_tracked"].numpy().copy()
    losses = [float(lossv)]
    opt.step()
    for s in range(1, steps):
        xs, ys = W.make_input(seed + 1 + s, batch, feat_dim, frames, spk_num)
        xs, ys = torch.from_numpy(xs), torch.from_numpy(ys)
        l = crit(m(xs, ys), ys)
        opt.zero_grad()
        l.backward()
        opt.step()
        losses.append(float(l))
    out["loss_curve"] = np.array(losses)
    m.eval()
    with torch.no_grad():
        out["emb_after"] = m.predict(x).numpy()
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    meta = dict(name=name, spk_num=spk_num, feat_dim=feat_dim, frames=frames, batch=batch, pooling=pooling, loss=loss,
                arch=se_ref.ARCH, seed=seed, steps=steps, lr=lr, wd=wd, param_names=names, gate_range=ranges,
                torch=torch.__version__, numpy=np.__version__)
    # the reference against itself (tools/ref_sensitivity.py): fp64, and fp32 with every input value moved by <= 1 ulp, 8 seeds
    rec = out["loss_curve"]
    base = curve(meta)
    assert np.abs(base - rec).max() < 1e-6, "the recorded curve is not reproduced: %s vs %s" % (base, rec)
    d = np.stack([np.abs(curve(meta, eps=2.0 ** -23, pseed=ps) - rec) for ps in range(8)])
    meta["ref_sensitivity"] = {"recorded": rec.tolist(), "fp64_minus_recorded": (curve(meta, torch.float64) - rec).tolist(),
                               "perturb_ulp": {"eps": 2.0 ** -23, "max_abs_dloss": d.max(0).tolist()}}
    print("reference against itself:", meta["ref_sensitivity"])
    with open(os.path.join(GOLD, name + ".json"), "w") as f:
        json.dump(meta, f, indent=1)


def record_keys():
    import model as refmodel
    m = refmodel.NeuralSpeakerModel(spk_num=7, feat_dim=80, pooling="mean+std", loss="AAM")
    m.res = refmodel.se_resnet34()
    keys = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert len(keys) == 251
    with open(os.path.join(GOLD, "state_keys_se_resnet34_AAM.json"), "w") as f:
        json.dump(keys, f)


if __name__ == "__main__":
    record_keys()
    record_case("se_r34_aam", 10, 80, 75, 4, "mean+std", "AAM", 31, steps=3)
