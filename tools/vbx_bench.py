#!/usr/bin/env python3
"""Host against hip for VBx resegmentation, recorded and not gated:

  workload   64 recordings of 800 windows, D = 128, four planted speakers per recording, the first pass an average-linkage
             clustering down to eight clusters (S = 8), 20 fixed iterations (epsilon = -inf);
  legs       `hip`: spk_vbx_batch from the rows, gamma and pi already in HBM, timed by device events; `host`: diarize.vbx's numpy
             fp64 back end, timed by the host clock.  The two legs alternate `--reps` times in one process after one warm-up;
  chain      the same launch at D = 1, where the two GEMM-shaped sums all but vanish: the forward-backward chain with the
             per-window passes around it.  Its share of the D = 128 time is an upper estimate of the chain's share.

Needs a GPU.    python tools/vbx_bench.py --out profiles/vbx_bench.json
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


def synth(ns, D, rng, speakers=4):
    rows, planted = [], []
    for n in ns:
        centres = rng.randn(speakers, D) * 1.5
        who = np.repeat(np.concatenate([np.arange(speakers), rng.randint(0, speakers, size=n)]), 8)[:n]
        rows.append(centres[who] + 0.5 * rng.randn(n, D))
        planted.append(who)
    return np.concatenate(rows).astype(np.float32), planted


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": len(v)}


def same_partition(a, b):
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--windows", type=int, default=800)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "vbx_bench measures the device path: it needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize, ops
    D, R, S = a.dim, a.recordings, 8
    rng = np.random.RandomState(3)
    model = (np.zeros(D), np.eye(D), np.linspace(20.0, 0.5, D))
    transform = np.concatenate([np.linalg.qr(rng.randn(D, D))[0], np.zeros((D, 1))], axis=1)
    ns = [a.windows] * R
    emb, planted = synth(ns, D, rng)
    rec_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    scores, _ = diarize.score_dense(emb, rec_off, "plda", transform=transform, plda=model, backend="hip", return_device=True)
    first = diarize.cluster(scores, rec_off, num_speakers=S, backend="hip")[0]
    del scores
    Xd, Pd = diarize.vbx_inputs(emb, None, transform, model, backend="hip")
    Xh, Ph = Xd.cpu().numpy(), Pd.cpu().numpy()
    gamma0, pi0, n_states = diarize.vbx_init(first, rec_off)
    rec = diarize.RecBatch(rec_off)                                 # the layout, as diarize() builds one per call
    kw = dict(Fa=0.3, Fb=17.0, loop_prob=0.99, max_iters=a.iters, epsilon=-np.inf)

    def hip_leg(X, Phi):
        g, p = torch.from_numpy(gamma0).cuda(), torch.from_numpy(pi0).cuda()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        ops.vbx_batch(X, Phi, rec, n_states, g, p, **kw)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), g.cpu().numpy()

    def host_leg():
        t0 = time.perf_counter()
        res = diarize.vbx(Xh, Ph, rec_off, gamma=gamma0, pi=pi0, n_states=n_states, backend="host", **kw)
        return (time.perf_counter() - t0) * 1e3, res["gamma"]

    X1, P1 = Xd[:, :1].contiguous(), Pd[:1].contiguous()
    hip_leg(Xd, Pd)                                                 # warm-up: code objects, allocator, the layout's device table
    hip_leg(X1, P1)
    t = {"hip": [], "host": [], "hip_dim1": []}
    for _ in range(a.reps):
        ms, g_hip = hip_leg(Xd, Pd)
        t["hip"].append(ms)
        ms, g_host = host_leg()
        t["host"].append(ms)
        t["hip_dim1"].append(hip_leg(X1, P1)[0])
    res = {"tool": "vbx_bench", "device": torch.cuda.get_device_name(0), "dim": D, "recordings": R, "windows": a.windows, "speakers": 4,
           "initial_states": [int(n_states.min()), int(n_states.max())], "iterations": a.iters, "workgroup_threads": ops.vbx_threads()}
    res.update({k: stats(v) for k, v in t.items()})
    res["host_over_hip"] = res["host"]["median_ms"] / res["hip"]["median_ms"]
    res["chain_share_upper_estimate"] = res["hip_dim1"]["median_ms"] / res["hip"]["median_ms"]
    res["hip_us_per_recording_iteration"] = 1e3 * res["hip"]["median_ms"] / a.iters       # the recordings run side by side
    lab_hip = diarize.vbx_labels(g_hip, rec_off, n_states)
    lab_host = diarize.vbx_labels(g_host, rec_off, n_states)
    res["recovers_planted_hip"] = all(same_partition(lab_hip[rec_off[r]:rec_off[r + 1]], planted[r]) for r in range(R))
    res["same_labels_host_hip"] = bool((lab_hip == lab_host).all())
    res["largest_gamma_difference_host_hip"] = float(np.abs(g_hip - g_host).max())
    res["note"] = ("hip: device events around spk_vbx_batch, inputs in HBM; host: wall clock of diarize.vbx(backend='host'); hip_dim1: "
                   "the same launch on the first dimension only")
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
