#!/usr/bin/env python3
"""What squeeze-and-excitation costs: se_resnet34 against resnet34 on one GPU, alternating, at this commit.

  * the training step (weight re-pack + forward + CE + backward as one hipGraph, then the fused SGD) at batch 256 x 300 frames x
    80 mel bins, 1211 speakers - the shape of the bench.py headline;
  * predict() in eval mode at batch 512 x 300 frames;
  * one eager, instrumented SE training step: time and algorithmic bytes of every spk_se_* launch (ops.PROFILE).

The two architectures take turns (--rounds rounds of --steps steps each) so that clock and temperature drift hits both alike;
the median round is reported with the spread.  Prints one JSON line per architecture; --out also writes them to a file.
Inputs are seeded noise; nothing is read from disk.

Run:  python tools/se_bench.py --out profiles/se_bench.json
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ARCHS = ("se_resnet34", "resnet34")


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--predict-batch", type=int, default=512)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--speakers", type=int, default=1211)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops
    from pytorch_kaldi_resnet_amd.engine import GraphedTrainStep
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    from pytorch_kaldi_resnet_amd.optim import FlatSGD
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.randn(args.batch, 80, args.frames, device=dev, generator=gen)
    y = torch.randint(0, args.speakers, (args.batch,), device=dev, generator=gen)
    xp = torch.randn(args.predict_batch, 80, args.frames, device=dev, generator=gen)
    runs = {}
    for arch in ARCHS:
        with contextlib.redirect_stdout(sys.stderr):
            m = NeuralSpeakerModel(args.speakers, 80, "mean+std", "AAM", 0.2, 30, arch=arch).to(dev).train()
        opt = FlatSGD(m, 0.1, momentum=0.9, weight_decay=5e-4)
        graph = GraphedTrainStep(m.engine(), args.batch, args.frames)

        def train_step(graph=graph, opt=opt):
            graph(x, y)
            opt.step()

        def predict_step(m=m):
            with torch.no_grad():
                m.predict(xp)

        runs[arch] = dict(model=m, train=train_step, predict=predict_step, train_ms=[], predict_ms=[])
        timed(train_step, 3)                                       # warm-up
    for _ in range(args.rounds):
        for arch in ARCHS:
            runs[arch]["train_ms"].append(timed(runs[arch]["train"], args.steps))
    for arch in ARCHS:
        runs[arch]["model"].eval()
        timed(runs[arch]["predict"], 2)
    for _ in range(args.rounds):
        for arch in ARCHS:
            runs[arch]["predict_ms"].append(timed(runs[arch]["predict"], args.steps))
    # the SE kernels inside one eager training step
    m = runs["se_resnet34"]["model"].train()
    for p in m.parameters():
        p.grad = None
    m.engine().loss_and_grad(x, y)
    torch.cuda.synchronize()
    ops.PROFILE = []
    for p in m.parameters():
        p.grad = None
    m.engine().loss_and_grad(x, y)
    torch.cuda.synchronize()
    recs, ops.PROFILE = ops.PROFILE, None
    kern, step_ms = {}, 0.0
    for label, _, e0, e1, nbytes in recs:
        ms = e0.elapsed_time(e1)
        step_ms += ms
        if label.startswith("spk_se_"):
            k = kern.setdefault(label, {"launches": 0, "ms": 0.0, "algorithmic_bytes": 0.0})
            k["launches"] += 1
            k["ms"] += ms
            k["algorithmic_bytes"] += nbytes
    for k in kern.values():
        k["ms"] = round(k["ms"], 4)
        k["gb_per_s"] = round(k["algorithmic_bytes"] / (k["ms"] * 1e6), 1) if k["ms"] > 0 and k["algorithmic_bytes"] else None
    lines = []
    for arch in ARCHS:
        r = runs[arch]
        line = {"arch": arch, "batch": args.batch, "frames": args.frames, "speakers": args.speakers, "mfma": os.environ.get("SPK_MFMA", "f16x3"),
                "rounds": args.rounds, "steps_per_round": args.steps,
                "train_step_ms": {"median": round(statistics.median(r["train_ms"]), 3), "min": round(min(r["train_ms"]), 3),
                                  "max": round(max(r["train_ms"]), 3)},
                "predict_batch": args.predict_batch,
                "predict_ms": {"median": round(statistics.median(r["predict_ms"]), 3), "min": round(min(r["predict_ms"]), 3),
                               "max": round(max(r["predict_ms"]), 3)}}
        if arch == "se_resnet34":
            base = runs["resnet34"]
            line["train_ratio_vs_resnet34"] = round(statistics.median(r["train_ms"]) / statistics.median(base["train_ms"]), 4)
            line["predict_ratio_vs_resnet34"] = round(statistics.median(r["predict_ms"]) / statistics.median(base["predict_ms"]), 4)
            line["se_kernels_eager_step"] = kern
            line["se_kernels_ms"] = round(sum(k["ms"] for k in kern.values()), 3)
            line["eager_step_kernel_ms"] = round(step_ms, 3)
        lines.append(json.dumps(line))
        print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
