#!/usr/bin/env python3
"""Training ingest from a float32 ('FM ') archive against Kaldi's one-byte compressed form ('CM ') of the same corpus (DESIGN.md
section 6g): one seeded synthetic corpus written twice, then NativeTrainLoader(device=cuda) alone and in front of the ResNet-34
training step at 256 x 300, FM and CM alternating in one process (`--pairs` pairs), per leg the utterances per second, the
process's CPU seconds (os.times: user + system, reader threads included), the bytes the batches read from the archives and the
bytes copied to the device per batch.

    python tools/cm_ingest_bench.py --out profiles/r09_cm_ingest.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/cm_ingest_bench.py --pairs 1 --no-step     # spk_cm_decode's time

The 'CM ' corpus is compressed on the GPU (features.compress); the 'FM ' corpus holds the ORIGINAL values, as a user who never
compressed would have it (the two loaders therefore yield slightly different numbers: the format is lossy).  Prints one JSON line."""
import argparse
import contextlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FEAT, SPK = 80, 1211


def write_corpora(d, n, lo, hi, seed):
    from pytorch_kaldi_resnet_amd import features, kaldi_io
    rs = np.random.RandomState(seed)
    out = {}
    fm, cm = os.path.join(d, "fm.ark"), os.path.join(d, "cm.ark")
    lines = {"fm": [], "cm": []}
    u2s = []
    with open(fm, "wb") as ff, open(cm, "wb") as fc:
        for i0 in range(0, n, 64):
            T = rs.randint(lo, hi + 1, min(64, n - i0))
            x = (rs.standard_normal((len(T), FEAT, int(T.max()))) * 3 + 8).astype(np.float32)      # log-mel-like
            mr, hd, cd = (t.cpu().numpy() for t in features.compress(torch.from_numpy(x).cuda(), T))
            for r, t in enumerate(T):
                utt = "utt%06d" % (i0 + r)
                lines["fm"].append("%s %s:%d" % (utt, fm, kaldi_io.write_mat(ff, np.ascontiguousarray(x[r, :, :t].T), key=utt)))
                lines["cm"].append("%s %s:%d" % (utt, cm, kaldi_io.write_cm(fc, mr[r, 0], mr[r, 1], hd[r], cd[r, :, :t], key=utt)))
                u2s.append("%s %d" % (utt, (i0 + r) % SPK))
    open(os.path.join(d, "utt2spkid"), "w").write("\n".join(u2s) + "\n")
    for k in ("fm", "cm"):
        open(os.path.join(d, k + ".scp"), "w").write("\n".join(lines[k]) + "\n")
        out[k] = {"scp": os.path.join(d, k + ".scp"), "ark_bytes": os.path.getsize(fm if k == "fm" else cm)}
    return out, os.path.join(d, "utt2spkid")


def batch_bytes(loader, T, B):
    """(bytes a batch reads from the archive, bytes it copies to the device), from the reader's rule (csrc_io/ark_reader.cpp): an
    'FM ' crop reads T x F floats; a 'CM ' crop reads the headers and either the span of the F strips (rows <= 4 T) or F strips.
    The read figure is the mean over the corpus at batch size B."""
    rows = loader.table.rows.astype(np.int64)
    if loader.table.all_cm:
        per = 16 + FEAT * 8 + np.where(rows <= 4 * T, (FEAT - 1) * rows + T, FEAT * T)
        return float(per.mean()) * B, B * FEAT * T + B * FEAT * 16 + B * 8
    return float(T * FEAT * 4) * B, B * FEAT * T * 4 + B * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=4000)
    ap.add_argument("--min-frames", type=int, default=400)
    ap.add_argument("--max-frames", type=int, default=1200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--no-step", action="store_true", help="loader-alone legs only")
    ap.add_argument("--out")
    args = ap.parse_args()
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd.ingest import NativeTrainLoader
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    from pytorch_kaldi_resnet_amd.optim import FlatSGD
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    d = tempfile.mkdtemp(prefix="spk_cm_ingest_")
    t0 = time.perf_counter()
    corp, u2s = write_corpora(d, args.utts, args.min_frames, args.max_frames, 7)
    sys.stderr.write("wrote %d utterances: FM %.0f MB, CM %.0f MB in %.1f s\n" % (args.utts, corp["fm"]["ark_bytes"] / 1e6,
                                                                                 corp["cm"]["ark_bytes"] / 1e6, time.perf_counter() - t0))
    loaders = {}
    with contextlib.redirect_stdout(sys.stderr):
        for k in ("fm", "cm"):
            loaders[k] = NativeTrainLoader(corp[k]["scp"], u2s, args.frames, args.batch, seed=5, threads=args.threads, drop_last=True,
                                           prefetch=3, device=str(dev))
        step = None
        if not args.no_step:
            from pytorch_kaldi_resnet_amd.engine import GraphedTrainStep
            torch.manual_seed(0)
            model = NeuralSpeakerModel(SPK, FEAT, "mean+std", "AAM", 0.2, 30, arch="resnet34").to(dev)
            model.train()
            opt = FlatSGD(model, 0.1, momentum=0.9, weight_decay=5e-4)
            graphed = GraphedTrainStep(model.engine(), args.batch, args.frames)

            def step(xb, yb):
                loss, _, _ = graphed(xb, yb, None)
                opt.step()
                return loss
    assert loaders["cm"].table.all_cm and not loaders["fm"].table.all_cm

    def batches(loader):
        ep = 0
        while True:
            loader.set_epoch(ep)
            ep += 1
            for xb, yb in loader:
                yield xb, yb

    its = {k: batches(loaders[k]) for k in loaders}      # one stream of batches per corpus for the whole run

    def leg(kind, with_step):
        it = its[kind]
        for _ in range(args.warmup):
            xb, yb = next(it)
            if with_step:
                step(xb, yb)
        torch.cuda.synchronize()
        c0, t1 = os.times(), time.perf_counter()
        for _ in range(args.steps):
            xb, yb = next(it)
            if with_step:
                step(xb, yb)
            else:
                xb.sum()                  # a consumer on the current stream, ordered after the copy (and the decode)
        torch.cuda.synchronize()
        dt, c1 = time.perf_counter() - t1, os.times()
        rd, h2d = batch_bytes(loaders[kind], args.frames, args.batch)
        return {"kind": kind, "with_step": with_step, "ms_per_batch": dt / args.steps * 1e3, "utt_per_s": args.batch * args.steps / dt,
                "cpu_s": (c1.user - c0.user) + (c1.system - c0.system), "read_bytes_per_batch": rd, "h2d_bytes_per_batch": h2d}

    legs = []
    for with_step in ([False] if args.no_step else [False, True]):
        for p in range(args.pairs):
            for kind in (("fm", "cm") if p % 2 == 0 else ("cm", "fm")):
                legs.append(leg(kind, with_step))
                sys.stderr.write(json.dumps(legs[-1]) + "\n")

    def med(kind, with_step, key):
        return float(np.median([l[key] for l in legs if l["kind"] == kind and l["with_step"] == with_step]))
    res = {"tool": "cm_ingest_bench", "utts": args.utts, "frames": [args.min_frames, args.max_frames], "batch": args.batch,
           "chunk": args.frames, "steps": args.steps, "pairs": args.pairs, "threads": args.threads,
           "ark_bytes": {k: corp[k]["ark_bytes"] for k in corp}, "legs": legs, "median": {}}
    for with_step in ([False] if args.no_step else [False, True]):
        name = "loader_and_step" if with_step else "loader_alone"
        res["median"][name] = {k: {key: med(k, with_step, key) for key in ("ms_per_batch", "utt_per_s", "cpu_s")} for k in ("fm", "cm")}
    shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    if args.out:
        open(args.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
