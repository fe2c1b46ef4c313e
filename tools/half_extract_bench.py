#!/usr/bin/env python3
"""Half-precision extraction against the fp32 path: ResNet-34 (mean+std, 80 mel) predict at batch 512 x 300 frames, eval mode, in
ONE GPU process.

Timing: the two paths alternate - three pairs of (fp32 predict, half predict), each leg 20 timed calls after 5 warm-up calls, device
events around the calls, the leg ending in a synchronise.  The fp32 leg is model.predict(x): the default path, unchanged.
A separate pass then takes the time of every launch of one half predict from device events around each launch (ops.PROFILE), summed
by launch kind, with the ALGORITHMIC bytes and FLOP of the kind computed from the shapes (every tensor read or written once; no halo
or re-read factor): achieved TB/s and TFLOP/s, and which of the two limits the kind sits closer to (HBM_TBS / MFMA_TFLOPS below).
Prints one JSON line; --out writes it to a file (profiles/half_extract_bench.json is the committed run).
usage: python tools/half_extract_bench.py [--batch 512] [--frames 300] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0            # the two ceilings of DESIGN.md section 3b (datasheet): HBM3E bandwidth ...
MFMA_TFLOPS = 2500.0     # ... and the dense fp16 matrix peak, one product per multiply-accumulate


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
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "half_extract_bench needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from oracle import weights as W
    from pytorch_kaldi_resnet_amd import ops
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    F, S, B, T = 80, 1211, args.batch, args.frames
    npst = W.make_state(3, S, F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    m = m.cuda().eval()
    x = torch.from_numpy(W.make_input(4, B, F, T, S)[0]).cuda()
    pairs = []
    with torch.no_grad():
        for _ in range(args.pairs):
            t32 = leg(lambda: m.predict(x), args.warmup, args.calls)
            t16 = leg(lambda: m.predict(x, precision="f16"), args.warmup, args.calls)
            pairs.append({"f32_ms": t32, "f16_ms": t16, "f32_utt_per_s": B / t32 * 1e3, "f16_utt_per_s": B / t16 * 1e3,
                          "ratio": t32 / t16})
        e32 = m.predict(x).double()
        e16 = m.predict(x, precision="f16").double()
        overflow_rows = int((m.engine().half_overflow > 0).sum())
        # per-launch pass: device events around every launch of one half predict
        ops.PROFILE = []
        m.predict(x, precision="f16")
        torch.cuda.synchronize()
        prof, ops.PROFILE = ops.PROFILE, None
    kinds = {}
    for label, flops, e0, e1, nbytes in prof:
        k = kinds.setdefault(label, {"launches": 0, "ms": 0.0, "flop": 0.0, "bytes": 0.0})
        k["launches"] += 1
        k["ms"] += e0.elapsed_time(e1)
        k["flop"] += flops
        k["bytes"] += nbytes
    for k in kinds.values():
        k["tb_per_s"] = k["bytes"] / (k["ms"] * 1e-3) / 1e12 if k["bytes"] else 0.0
        k["tflop_per_s"] = k["flop"] / (k["ms"] * 1e-3) / 1e12
        k["bound"] = "memory" if k["bytes"] / (HBM_TBS * 1e12) >= k["flop"] / (MFMA_TFLOPS * 1e12) else "compute"
        k["of_bound"] = max(k["tb_per_s"] / HBM_TBS, k["tflop_per_s"] / MFMA_TFLOPS)
    cos = 1 - (e32 * e16).sum(1) / (e32.norm(dim=1) * e16.norm(dim=1))
    best = max(pairs, key=lambda p: p["f16_utt_per_s"])
    res = {
        "metric": "predict, ResNet-34 mean+std, 80 mel, eval mode, one process, device events",
        "batch": B, "frames": T, "pairs": pairs, "calls_per_leg": args.calls, "warmup_per_leg": args.warmup,
        "f32_utt_per_s": max(p["f32_utt_per_s"] for p in pairs), "f16_utt_per_s": best["f16_utt_per_s"],
        "ratio_median": float(np.median([p["ratio"] for p in pairs])),
        "max_cos_dist_f16_vs_f32": float(cos.max()), "overflow_rows": overflow_rows,
        "half_launch_kinds": dict(sorted(kinds.items(), key=lambda kv: -kv[1]["ms"])),
        "half_launch_ms_total": sum(k["ms"] for k in kinds.values()),
        "limits": {"hbm_tb_per_s": HBM_TBS, "fp16_mfma_tflop_per_s": MFMA_TFLOPS},
        "operand_mode_f32_path": os.environ.get("SPK_MFMA", "f16x3"), "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
