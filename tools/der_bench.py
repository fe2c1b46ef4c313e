#!/usr/bin/env python3
"""The threshold sweep of diarization scoring on both back ends, recorded and not gated:

  workload   64 recordings of 800 sliding windows (1.5 s every 0.75 s: ten minutes each), 4 reference speakers in turns of 3 - 20 s,
             window embeddings planted near their speaker's centre, cosine scores; clustered once on the device (not timed: the
             merge list is the sweep's input); K = 41 thresholds from -1 to 1: 2 624 jobs of 800 pieces, of which those that apply
             the same prefix to a recording are scored once (`distinct_jobs`), on both back ends;
  legs       `hip`: diarize.tune_threshold(backend="hip"), wall clock around the call with a device synchronise at both ends, and
             inside it the three kernels by device events (spk_ahc_cut_batch, spk_der_pieces, spk_der_batch; a run of its own with
             the events on); `host`: diarize.tune_threshold(backend="host") on the same merge list, wall clock.  The legs alternate
             `--reps` times in one process after one warm-up of each.
The host leg is the host side of the same code base, not an outside scorer: it is the only comparison there is.

Needs a GPU.    python tools/der_bench.py --out profiles/der_bench.json
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


def synth(R, n, speakers, rng, dim=32, window=1.5, period=0.75, noise=0.8):
    segs, emb, ref = [], [], {}
    for r in range(R):
        reco = "rec%03d" % r
        centres = rng.randn(speakers, dim)
        end, t, turns = (n - 1) * period + window, 0.0, []
        while t < end:
            d = round(rng.uniform(3.0, 20.0), 2)
            turns.append((rng.randint(speakers), t, min(round(t + d, 2), end)))
            t = round(t + d, 2)
        ref[reco] = [("spk%d" % s, a, round(b - a, 2)) for s, a, b in turns]
        starts = np.array([tt[1] for tt in turns])
        for w in range(n):
            a = round(w * period, 2)
            who = turns[int(np.searchsorted(starts, a + 0.5 * window, side="right")) - 1][0]
            segs.append(("%s-%08d-%08d" % (reco, round(a * 100), round((a + window) * 100)), reco, a, round(a + window, 2)))
            emb.append(centres[who] + noise * rng.randn(dim))
    return segs, np.array(emb), ref


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--windows", type=int, default=800)
    ap.add_argument("--speakers", type=int, default=4)
    ap.add_argument("--thresholds", type=int, default=41)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "der_bench measures the device path: it needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize as D, ops
    R, n, K = a.recordings, a.windows, a.thresholds
    segs, emb, ref = synth(R, n, a.speakers, np.random.RandomState(11))
    rec_off = np.arange(R + 1, dtype=np.int64) * n
    scores = D.score_dense(emb, rec_off, "cosine", backend="hip", return_device=True)[0]
    merges = D.cluster(scores, rec_off, backend="hip")[1:]
    th = np.linspace(-1.0, 1.0, K)

    def leg(backend):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = D.tune_threshold(merges, segs, ref, th, backend=backend)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    leg("hip")                                                   # warm-up: the code objects, the allocator
    leg("host")
    t = {"hip": [], "host": []}
    for _ in range(a.reps):
        ms, g = leg("hip")
        t["hip"].append(ms)
        ms, h = leg("host")
        t["host"].append(ms)
    kern = {}
    for _ in range(a.reps):                                      # the kernels by device events, in runs of their own
        ops.PROFILE = []
        D.tune_threshold(merges, segs, ref, th, backend="hip")
        torch.cuda.synchronize()
        seen = {}
        for name, _, e0, e1, _ in ops.PROFILE:
            seen[name] = seen.get(name, 0.0) + e0.elapsed_time(e1)
        ops.PROFILE = None
        for name, v in seen.items():
            kern.setdefault(name, []).append(v)
    res = {"tool": "der_bench", "device": torch.cuda.get_device_name(0), "recordings": R, "windows": n, "reference_speakers": a.speakers,
           "thresholds": K, "jobs": R * K,
           "distinct_jobs": int(sum(np.unique(row).size for row in g["prefix"])), "pieces_per_job": n, "labels_per_job": [int(g["labels"].max(axis=1).min()), int(g["labels"].max())],
           "host_jobs": g["host_jobs"], "best_threshold": g["best_threshold"], "best_der": g["table"][g["best_index"]][5]}
    res.update({"sweep_" + k: stats(v) for k, v in t.items()})
    res["kernels"] = {k: stats(v) for k, v in kern.items()}
    res["kernels_total_ms"] = float(sum(s["median_ms"] for s in res["kernels"].values()))
    res["hip_host_share"] = 1.0 - res["kernels_total_ms"] / res["sweep_hip"]["median_ms"]
    res["host_over_hip"] = res["sweep_host"]["median_ms"] / res["sweep_hip"]["median_ms"]
    res["same_table"] = bool(g["table"] == h["table"] and np.array_equal(g["per_recording"], h["per_recording"]))
    res["note"] = ("sweep_hip / sweep_host: wall clock of diarize.tune_threshold on one merge list (clustering not included); kernels: device "
                   "events around each launch, summed per call of tune_threshold, in runs apart from the wall-clock ones; hip_host_share: the "
                   "part of a hip sweep that is not kernel time (reference preparation, tables, uploads, the download of labels and counts); "
                   "the host leg is this project's own host back end - the only comparison there is")
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
