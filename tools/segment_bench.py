#!/usr/bin/env python3
"""Kernel against host for VAD decisions -> speech segments, recorded and not gated:

  workload   64 rows of 360 000 frames (an hour at 10 ms), voiced runs and pauses of geometric length with a mean of 100 frames
             each - about one run per 200 frames - as int32 decisions in HBM, where spk_vad_count leaves them; default
             SegmentOptions;
  legs       `kernel`: spk_vad_segments alone, timed by device events; `wrapper`: features.vad_segments (the launch, the counts
             and the written pairs downloaded), timed by the host clock; `host`: the VAD tensor downloaded, then
             ingest.segments_from_vad, timed by the host clock (the download is also given on its own).  The legs alternate
             `--reps` times in one process after one warm-up.

Needs a GPU.    python tools/segment_bench.py --out profiles/segment_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(rows, frames, mean_run, rng):
    v = np.zeros((rows, frames), dtype=np.int32)
    for b in range(rows):
        n = rng.geometric(1.0 / mean_run, size=2 * frames // mean_run + 64)
        bit = (np.arange(n.size) + b) % 2                        # alternate, rows start voiced or silent in turn
        v[b] = np.repeat(bit, n)[:frames]
    return v


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--frames", type=int, default=360000)
    ap.add_argument("--mean-run", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "segment_bench measures the device path: it needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features, hip, ingest
    B, T = a.rows, a.frames
    v = synth(B, T, a.mean_run, np.random.RandomState(7))
    runs = int((np.diff(v, axis=1) == 1).sum() + v[:, 0].sum())
    vg = torch.from_numpy(v).cuda()
    lengths = np.full(B, T, dtype=np.int64)
    tg = torch.from_numpy(lengths.astype(np.int32)).cuda()
    o = features.SegmentOptions()
    want = ingest.segments_from_vad(v, lengths, o)
    cap = int(np.bincount(want[0], minlength=B).max())
    seg = torch.empty(B, cap, 2, dtype=torch.int32, device="cuda")
    nseg = torch.empty(B, dtype=torch.int32, device="cuda")

    def kernel_leg():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        hip.call("spk_vad_segments", hip.ptr(vg), hip.ptr(tg), B, T, o.padding, o.max_gap, o.min_length, hip.ptr(seg), cap, hip.ptr(nseg),
                 hip.stream())
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def wrapper_leg():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = features.vad_segments(vg, lengths, o)
        return (time.perf_counter() - t0) * 1e3, res

    def host_leg():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vh = vg.cpu().numpy()
        t1 = time.perf_counter()
        res = ingest.segments_from_vad(vh, lengths, o)
        t2 = time.perf_counter()
        return (t2 - t0) * 1e3, (t1 - t0) * 1e3, res

    kernel_leg()                                                 # warm-up: the code object, the allocator
    wrapper_leg()
    host_leg()
    t = {"kernel": [], "wrapper": [], "host": [], "host_download": []}
    for _ in range(a.reps):
        t["kernel"].append(kernel_leg())
        ms, got = wrapper_leg()
        t["wrapper"].append(ms)
        ms, dl, host = host_leg()
        t["host"].append(ms)
        t["host_download"].append(dl)
    res = {"tool": "segment_bench", "device": torch.cuda.get_device_name(0), "rows": B, "frames": T, "mean_run": a.mean_run, "runs": runs,
           "frames_per_run": B * T / max(runs, 1), "segments": int(want[0].size), "most_segments_in_a_row": cap,
           "options": [o.padding, o.max_gap, o.min_length], "vad_bytes": int(v.nbytes)}
    res.update({k: stats(x) for k, x in t.items()})
    res["host_over_kernel"] = res["host"]["median_ms"] / res["kernel"]["median_ms"]
    res["host_over_wrapper"] = res["host"]["median_ms"] / res["wrapper"]["median_ms"]
    res["kernel_gb_per_s"] = v.nbytes / (res["kernel"]["median_ms"] * 1e-3) / 1e9
    res["same_segments"] = bool(all(np.array_equal(g, w) and np.array_equal(h, w) for g, h, w in zip(got, host, want)))
    res["note"] = ("kernel: device events around spk_vad_segments, decisions in HBM; wrapper: wall clock of features.vad_segments (launch, "
                   "counts and written pairs downloaded); host: wall clock of the VAD tensor's download plus ingest.segments_from_vad")
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
