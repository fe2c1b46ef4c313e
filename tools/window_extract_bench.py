#!/usr/bin/env python3
"""Windowed extraction against the plain predict: ResNet-34 (mean+std, 80 mel), 64 utterances of 3 000 frames, a window of 300 frames
every 150 (19 windows per utterance, 1 216 in all), eval mode, in ONE GPU process.

Timing: the two paths alternate - three pairs of (plain leg, windowed leg), each leg `--calls` timed calls after `--warmup` warm-up
calls, device events around the calls, the leg ending in a synchronise.  Two more legs per pair split the difference: the
length-masked predict alone on the batches of windows gathered beforehand (what is left is the window machinery), and the masked
predict on unpadded rows (lengths = 300 at width 300: the masked kernels without the padding to a multiple of 8).  The windowed leg
is model.predict_windows(x, None, 300, 150, batch_size=--batch): plan, gather, the length-masked predict per batch of windows, plan order restored.  The plain leg is the
yardstick: model.predict() over the same number of 300-frame rows, already laid out as a [N][80][300] tensor, in batches of the same
size.  A separate pass takes the time of every launch of one predict_windows(average=True) from device events around each launch
(ops.PROFILE) and sums the spk_window_gather and spk_window_mean launches.
Prints one JSON line; --out writes it to a file (profiles/window_extract_bench.json is the committed run).
usage: python tools/window_extract_bench.py [--batch 256] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls        # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--period", type=int, default=150)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "window_extract_bench needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from oracle import weights as Wt
    from pytorch_kaldi_resnet_amd import ingest, ops
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    F, S, U, T, W, P, bs = 80, 1211, args.utts, args.frames, args.window, args.period, args.batch
    npst = Wt.make_state(3, S, F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    m = m.cuda().eval()
    x = torch.randn(U, F, T, generator=torch.Generator().manual_seed(4)).cuda()
    plan = ingest.plan_windows([T] * U, W, P, 1)
    N = int(plan.utt.size)
    rows = torch.randn(N, F, W, generator=torch.Generator().manual_seed(5)).cuda()      # the plain leg's input: N rows of W frames

    def plain():
        return [m.predict(rows[i:i + bs]) for i in range(0, N, bs)]

    def windowed():
        return m.predict_windows(x, None, W, P, batch_size=bs)

    # the length-masked predict alone, on the batches predict_windows forms (gathered once, outside the timed calls)
    batches = ingest.window_batches(plan.length, bs)
    gathered = [(ops.window_gather(x, plan.utt[i], plan.start[i], plan.length[i], wcap), plan.length[i].tolist()) for i, wcap in batches]

    def masked():
        return [m.predict(xw, lengths=lw) for xw, lw in gathered]

    def masked_unpadded():      # the masked kernels at the plain leg's width: lengths = W on rows of W frames
        return [m.predict(rows[i:i + bs], lengths=[W] * min(bs, N - i)) for i in range(0, N, bs)]

    def by_kernel(fn):
        """ms per kernel of one call, from device events around every launch, summed by the kernel's name without its template"""
        ops.PROFILE = []
        fn()
        torch.cuda.synchronize()
        prof, ops.PROFILE = ops.PROFILE, None
        out = {}
        for label, _, e0, e1, _ in prof:
            k = label.split("<")[0]
            out[k] = out.get(k, 0.0) + e0.elapsed_time(e1)
        return dict(sorted(out.items(), key=lambda kv: -kv[1]))

    pairs = []
    with torch.no_grad():
        for _ in range(args.pairs):
            tp = leg(plain, args.warmup, args.calls)
            tw = leg(windowed, args.warmup, args.calls)
            tm = leg(masked, args.warmup, args.calls)
            tu = leg(masked_unpadded, args.warmup, args.calls)
            pairs.append({"plain_ms": tp, "windowed_ms": tw, "masked_ms": tm, "masked_unpadded_ms": tu, "plain_rows_per_s": N / tp * 1e3,
                          "windows_per_s": N / tw * 1e3, "ratio": tp / tw})
        plain_kernels, masked_kernels = by_kernel(plain), by_kernel(masked)
        ops.PROFILE = []
        m.predict_windows(x, None, W, P, average=True, batch_size=bs)
        torch.cuda.synchronize()
        prof, ops.PROFILE = ops.PROFILE, None
    kinds = {}
    for label, _, e0, e1, nbytes in prof:
        if label in ("spk_window_gather", "spk_window_mean"):
            k = kinds.setdefault(label, {"launches": 0, "ms": 0.0, "bytes": 0.0})
            k["launches"] += 1
            k["ms"] += e0.elapsed_time(e1)
            k["bytes"] += nbytes
    plain_rates = [p["plain_rows_per_s"] for p in pairs]
    res = {
        "metric": "predict_windows against predict on as many rows, ResNet-34 mean+std, 80 mel, eval mode, one process, device events",
        "utterances": U, "frames": T, "window": W, "period": P, "windows": N, "batch": bs, "pairs": pairs,
        "calls_per_leg": args.calls, "warmup_per_leg": args.warmup,
        "windows_per_s_median": float(np.median([p["windows_per_s"] for p in pairs])),
        "plain_rows_per_s_median": float(np.median(plain_rates)),
        "plain_spread": (max(plain_rates) - min(plain_rates)) / float(np.median(plain_rates)),
        "ratio_median": float(np.median([p["ratio"] for p in pairs])),
        "padded_width": sorted({int(wcap) for _, wcap in batches}),
        "plain_kernels_ms": plain_kernels, "masked_kernels_ms": masked_kernels,
        "window_kernels": kinds, "window_kernels_ms": sum(k["ms"] for k in kinds.values()),
        "profiled_call_launch_ms_total": sum(e0.elapsed_time(e1) for _, _, e0, e1, _ in prof),
        "operand_mode": os.environ.get("SPK_MFMA", "f16x3"), "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
