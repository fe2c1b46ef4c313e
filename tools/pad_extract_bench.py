#!/usr/bin/env python3
"""Whole-utterance extraction: length-bucketed batches (decode.py --native-reader) against padded, length-masked batches
(decode.py --native-reader --pad-batches), in ONE GPU process.

A seeded synthetic ark (2 000 utterances x 80 mel, log-normal lengths clipped to [400, 3000] frames, about 800 on average) is
extracted by both modes alternately, twice each, after a warm-up pass of both.  A pass is read (libspkio, pinned) + H2D + predict +
D2H of every utterance, sequential, timed with a host clock around work that ends in a device synchronise.  Prints one JSON line:
utt/s of each mode (each pass and the best), padding overhead (padded / real frames) and the largest cosine distance between
the two modes' embeddings.
usage: python tools/pad_extract_bench.py [--n 2000] [--batch-size 64] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_ark(d, n, F, seed):
    from pytorch_kaldi_resnet_amd import kaldi_io
    rng = np.random.RandomState(seed)
    lens = np.clip(rng.lognormal(np.log(750), 0.4, n), 400, 3000).astype(np.int64)
    ark = os.path.join(d, "feats.ark")
    rx = []
    with open(ark, "wb") as f:
        for i, T in enumerate(lens):
            f.write(b"u%05d " % i)
            off = kaldi_io.write_mat(f, rng.randn(int(T), F).astype(np.float32))
            rx.append("%s:%d" % (ark, off))
    return rx, lens


def run(model, table, batches, padded, F):
    """one pass over every batch: -> (seconds, {utterance index: embedding})"""
    out = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for idx, T in batches:
        buf = torch.empty(len(idx), F, T).pin_memory()
        if padded:
            table.read_padded(idx, T, buf)
            e = model.predict(buf.cuda(non_blocking=True), lengths=table.rows[idx])
        else:
            table.read_crop(idx, [0] * len(idx), T, buf)
            e = model.predict(buf.cuda(non_blocking=True))
        e = e.cpu().numpy()
        for j, i in enumerate(idx):
            out[int(i)] = e[j]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--max-pad-ratio", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pad_extract_bench needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from oracle import weights as W
    from pytorch_kaldi_resnet_amd import ingest, ops
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    F, S = 80, 1211
    npst = W.make_state(3, S, F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    m = m.cuda().eval()
    with tempfile.TemporaryDirectory() as d:
        rx, lens = make_ark(d, args.n, F, args.seed)
        table = ingest.ArkTable(rx)
        # bucketed: equal frame counts share a batch (decode.py --native-reader)
        order = np.argsort(lens, kind="stable")
        bucketed, i = [], 0
        while i < len(order):
            j = i
            while j < len(order) and j - i < args.batch_size and lens[order[j]] == lens[order[i]]:
                j += 1
            bucketed.append((order[i:j], int(lens[order[i]])))
            i = j
        padded = ingest.pad_batches(lens, args.batch_size, max_pad_ratio=args.max_pad_ratio)
        pad_frames = sum(len(b) * T for b, T in padded)
        times = {"bucketed": [], "padded": []}
        with torch.no_grad():
            run(m, table, bucketed, False, F)          # warm-up of both (code objects, allocator, pinned pages)
            run(m, table, padded, True, F)
            for _ in range(2):
                tb, eb = run(m, table, bucketed, False, F)
                tp, ep = run(m, table, padded, True, F)
                times["bucketed"].append(tb)
                times["padded"].append(tp)
    a = np.stack([eb[i] for i in range(args.n)]).astype(np.float64)
    b = np.stack([ep[i] for i in range(args.n)]).astype(np.float64)
    cos = 1 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    ups = {k: [args.n / t for t in v] for k, v in times.items()}
    res = {
        "metric": "whole-utterance extraction, ResNet-34 mean+std, 80 mel, read + predict + D2H, one process",
        "utterances": args.n, "frames_mean": float(lens.mean()), "frames_min": int(lens.min()), "frames_max": int(lens.max()),
        "distinct_lengths": int(len(np.unique(lens))), "batch_size": args.batch_size, "operand_mode": os.environ.get("SPK_MFMA", "f16x3"),
        "bucketed_batches": len(bucketed), "padded_batches": len(padded),
        "padding_overhead": pad_frames / float(lens.sum()),
        "bucketed_utt_per_s": max(ups["bucketed"]), "padded_utt_per_s": max(ups["padded"]),
        "speedup": max(ups["padded"]) / max(ups["bucketed"]),
        "bucketed_utt_per_s_passes": ups["bucketed"], "padded_utt_per_s_passes": ups["padded"],
        "max_cos_dist_padded_vs_bucketed": float(cos.max()),
        "device": torch.cuda.get_device_name(0), "split": ops.SPLIT,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
