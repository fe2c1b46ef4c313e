#!/usr/bin/env python3
"""Host against hip for the diarization back end, recorded and not gated:

  workloads  64 recordings of 800 windows, and one recording of 4 800 windows; D = 128, PLDA scores, four planted speakers per
             recording, clustered down to four;
  legs       `hip`: spk_score_dense_q + spk_score_dense + spk_ahc_batch from the projected rows already in HBM, timed by device
             events; `host`: the same expression in numpy fp64 and scipy's average linkage (diarize.cluster's host back end where
             scipy does not import), timed by the host clock.  The two legs alternate `--reps` times in one process after one warm-up;
  run        one diarize.diarize(..., backend="hip") call over the 64 x 800 workload from raw embeddings: wall time, and the share
             of each kernel by device events around every launch (a second call, so that the events do not sit in the first one).

Needs a GPU.    python tools/diarize_bench.py --out profiles/diarize_bench.json
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
        who = np.concatenate([np.arange(speakers), rng.randint(0, speakers, size=n - speakers)])
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "diarize_bench measures the device path: it needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize, ops
    try:
        from scipy.cluster import hierarchy
    except ImportError:
        hierarchy = None
    D = a.dim
    rng = np.random.RandomState(3)
    model = (np.zeros(D), np.eye(D), np.linspace(20.0, 0.5, D))
    transform = np.concatenate([np.linalg.qr(rng.randn(D, D))[0], np.zeros((D, 1))], axis=1)
    res = {"tool": "diarize_bench", "device": torch.cuda.get_device_name(0), "dim": D, "speakers": 4,
           "host_clustering": "scipy.cluster.hierarchy.linkage(average)" if hierarchy else "diarize.cluster(backend='host')",
           "workloads": {}}
    for name, ns in (("64x800", [800] * 64), ("1x4800", [4800])):
        emb, planted = synth(ns, D, rng)
        rec_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        R = len(ns)
        rec = diarize.RecBatch(rec_off)                             # the layout, as diarize() builds one per call
        Ud, qd_unused, gd, K = diarize.dense_inputs(emb, "plda", transform=transform, plda=model, backend="hip")
        Uh, qh_unused, gh, Kh = diarize.dense_inputs(emb, "plda", transform=transform, plda=model, backend="host")
        kd = torch.from_numpy(diarize.plda_dense_terms(model[2])[1]).cuda()
        kh = diarize.plda_dense_terms(model[2])[1]
        four, none = np.full(R, 4, dtype=np.int32), np.full(R, -np.inf)

        def hip_leg():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            q = ops.score_dense_q(Ud, kd, -0.5)
            scores, _ = ops.score_dense(Ud, rec, q, gd, K)
            ev[1].record()
            out = ops.ahc_batch(scores, rec, four, none)
            ev[2].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), out[0].cpu().numpy()

        def host_leg():
            t0 = time.perf_counter()
            q = -0.5 * (kh[None, :] * Uh * Uh).sum(axis=1)
            mats = []
            for r in range(R):
                u, qq = Uh[rec_off[r]:rec_off[r + 1]], q[rec_off[r]:rec_off[r + 1]]
                mats.append((((u * gh[None, :]) @ u.T + qq[:, None]) + qq[None, :] + Kh).astype(np.float32))
            t1 = time.perf_counter()
            labels = []
            if hierarchy:
                for s in mats:
                    y = -s[np.triu_indices(len(s), 1)].astype(np.float64)      # the condensed form, row-major
                    Z = hierarchy.linkage(y - y.min() + 1.0, "average")         # distances: a shift moves every average alike
                    labels.append(hierarchy.fcluster(Z, 4, "maxclust"))
            else:
                flat = np.concatenate([m.ravel() for m in mats])
                lab = diarize.cluster(flat, rec_off, num_speakers=4, backend="host")[0]
                labels = [lab[rec_off[r]:rec_off[r + 1]] for r in range(R)]
            t2 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, labels

        hip_leg()                                                   # warm-up: code objects, allocator, the layout's device table
        t = {"hip_scores": [], "hip_cluster": [], "host_scores": [], "host_cluster": []}
        for _ in range(a.reps):
            s, c, lab_hip = hip_leg()
            t["hip_scores"].append(s)
            t["hip_cluster"].append(c)
            s, c, lab_host = host_leg()
            t["host_scores"].append(s)
            t["host_cluster"].append(c)
        w = {k: stats(v) for k, v in t.items()}
        w["hip_total_median_ms"] = w["hip_scores"]["median_ms"] + w["hip_cluster"]["median_ms"]
        w["host_total_median_ms"] = w["host_scores"]["median_ms"] + w["host_cluster"]["median_ms"]
        w["recovers_planted_hip"] = all(same_partition(lab_hip[rec_off[r]:rec_off[r + 1]], planted[r]) for r in range(R))
        w["same_partition_host_hip"] = all(same_partition(lab_hip[rec_off[r]:rec_off[r + 1]], np.asarray(lab_host[r])) for r in range(R))
        res["workloads"][name] = w
        print(name, json.dumps(w), flush=True)
        if name == "64x800":                                       # one whole diarize() call from raw embeddings
            keys = ["rec%02d-%08d-%08d" % (r, 20 * i, 20 * i + 40) for r, n in enumerate(ns) for i in range(n)]
            segs = [(k, k[:5], 0.2 * int(k[6:14]) / 20, 0.2 * int(k[6:14]) / 20 + 0.4) for k in keys]
            table = dict(zip(keys, emb))
            kw = dict(threshold=None, reco2num_spk={"rec%02d" % r: 4 for r in range(R)}, backend="hip", transform=transform, plda=model)
            diarize.diarize(table, segs, "plda", **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            diarize.diarize(table, segs, "plda", **kw)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            ops.PROFILE = []
            diarize.diarize(table, segs, "plda", **kw)
            torch.cuda.synchronize()
            per = {}
            for label, _, e0, e1, _ in ops.PROFILE:
                per[label] = per.get(label, 0.0) + e0.elapsed_time(e1)
            ops.PROFILE = None
            res["diarize_call_64x800"] = {"wall_ms": wall, "kernel_ms": per, "ahc_share_of_wall": per.get("spk_ahc_batch", 0.0) / wall,
                                          "note": "wall: embeddings as a dict in memory to labels and RTTM lines, host grouping and "
                                                  "uploads included; kernel_ms: device events of a separate call"}
            print("diarize", json.dumps(res["diarize_call_64x800"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
