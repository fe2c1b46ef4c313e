#!/usr/bin/env python3
"""Host against hip for the per-recording PCA of the dense PLDA scores, recorded and not gated:

  workload   64 recordings of 800 windows, L = 128, four planted speakers per recording, E = 0.1 and E = 0.9;
  legs       `hip`: spk_pca_plda_batch, then spk_pca_score_terms, spk_affine_lennorm_rec, spk_score_dense_q_rec and
             spk_score_dense_rec, from the projected rows and the batch's offset table already in HBM, timed by device events; `host`: diarize.pca_rows and the
             numpy scores, timed by the host clock.  The two legs alternate `--reps` times in one process after one warm-up;
  alone      the same `hip` leg on the first recording only: one workgroup per recording, so this is the slowest workgroup's time;
  eig        spk_syevj_batch alone on the 64 covariances (order L) and on 64 matrices Q diag(psi_r) Q^T of the retained orders (the
             spectrum and order of the second eigendecomposition in a random basis): their sum over the spk_pca_plda_batch time
             estimates the share of the two eigendecompositions.

Needs a GPU.    python tools/pca_bench.py --out profiles/pca_bench.json
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


def synth(R, n, L, rng, speakers=4):
    scale = 0.97 ** np.arange(L)
    rows = []
    for _ in range(R):
        spk = 2.0 * rng.randn(speakers, L) * scale
        rows.append(spk[rng.randint(0, speakers, size=n)] + rng.randn(n, L) * scale)
    return np.concatenate(rows).astype(np.float32)


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": len(v)}


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    out = fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--recordings", type=int, default=64)
    ap.add_argument("--windows", type=int, default=800)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pca_bench measures the device path: it needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize, ops
    from pytorch_kaldi_resnet_amd.plda import _up
    L, R, n = a.dim, a.recordings, a.windows
    rng = np.random.RandomState(3)
    model = (0.1 * rng.randn(L), np.eye(L) + rng.randn(L, L) / np.sqrt(L), np.sort(rng.uniform(0.05, 8.0, L))[::-1].copy())
    m, T, psi = model
    Ti = np.linalg.inv(T)
    dev_model = tuple(_up(v) for v in (Ti @ Ti.T, (Ti * psi[None, :]) @ Ti.T, T, psi, m))
    Zh = synth(R, n, L, rng)
    Zd = torch.from_numpy(Zh).cuda()
    ro = np.arange(R + 1, dtype=np.int64) * n
    res = {"tool": "pca_bench", "device": torch.cuda.get_device_name(0), "dim": L, "recordings": R, "windows": n, "speakers": 4,
           "sweep_bound": ops.syevj_max_sweeps()}

    def hip_leg(Z, rec_off, E):
        t_pca, (dim, s, psi_r, A_r, b_r, info) = timed(lambda: ops.pca_plda_batch(Z, rec_off, *dev_model, E))

        def rest():
            g, k, qn, K = ops.pca_score_terms(psi_r)
            U = ops.affine_lennorm_rec(Z, rec_off, A_r, b_r, qn, dim, True)
            return ops.score_dense(U, rec_off, ops.score_dense_q(U, k, -0.5, rec_off), g, K)[0]

        t_rest, scores = timed(rest)
        assert int(info.abs().max()) == 0
        return t_pca, t_rest, dim.cpu().numpy(), psi_r.cpu().numpy(), scores

    def host_leg(E):
        t0 = time.perf_counter()
        p = diarize.pca_rows(Zh, ro, model, E, backend="host")
        t1 = time.perf_counter()
        s = diarize._score_rows(p["U"], p["q"], p["g"], p["K"], ro, "host", False)
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, p["dim"], s

    rec, rec1 = diarize.RecBatch(ro), diarize.RecBatch(ro[:2])     # the layouts, as diarize() builds one per call
    hip_leg(Zd, rec, 0.9)                                           # warm-up: code objects, allocator, the layouts' device tables
    hip_leg(Zd[:n], rec1, 0.9)
    for E in (0.1, 0.9):
        t = {k: [] for k in ("hip_pca", "hip_rows_scores", "host_pca", "host_rows_scores", "hip_pca_one_recording")}
        for _ in range(a.reps):
            tp, tr, dim_hip, psi_hip, s_hip = hip_leg(Zd, rec, E)
            t["hip_pca"].append(tp)
            t["hip_rows_scores"].append(tr)
            hp, hr, dim_host, s_host = host_leg(E)
            t["host_pca"].append(hp)
            t["host_rows_scores"].append(hr)
            t["hip_pca_one_recording"].append(hip_leg(Zd[:n], rec1, E)[0])
        leg = {k: stats(v) for k, v in t.items()}
        leg["host_over_hip_pca"] = leg["host_pca"]["median_ms"] / leg["hip_pca"]["median_ms"]
        leg["host_over_hip_all"] = ((leg["host_pca"]["median_ms"] + leg["host_rows_scores"]["median_ms"])
                                    / (leg["hip_pca"]["median_ms"] + leg["hip_rows_scores"]["median_ms"]))
        leg["dims"] = [int(dim_hip.min()), int(dim_hip.max())]
        leg["same_dims_host_hip"] = bool((dim_hip == dim_host).all())
        leg["largest_score_difference_host_hip"] = float(np.abs(s_hip.cpu().numpy().astype(np.float64) - s_host).max())
        # the two eigendecompositions alone
        x = Zh.astype(np.float64).reshape(R, n, L)
        mu = x.mean(axis=1)
        C = np.einsum("rni,rnj->rij", x, x) / n - mu[:, :, None] * mu[:, None, :]
        Cd = torch.from_numpy(np.ascontiguousarray(C)).cuda()
        Md = np.zeros((R, L, L))
        for r in range(R):
            d = int(dim_hip[r])
            Q = np.linalg.qr(rng.randn(d, d))[0]
            Md[r, :d, :d] = (Q * psi_hip[r, :d][None, :]) @ Q.T
        Md = torch.from_numpy(Md).cuda()
        ops.syevj_batch(Cd)
        e1, e2, sw1, sw2 = [], [], None, None
        for _ in range(a.reps):
            ms, out = timed(lambda: ops.syevj_batch(Cd))
            e1.append(ms)
            sw1 = out[2].cpu().numpy()
            ms, out = timed(lambda: ops.syevj_batch(Md, dim_hip))
            e2.append(ms)
            sw2 = out[2].cpu().numpy()
        leg["syevj_covariances"] = stats(e1)
        leg["syevj_retained_order"] = stats(e2)
        leg["sweeps_covariances"] = [int(sw1.min()), int(sw1.max())]
        leg["sweeps_retained_order"] = [int(sw2.min()), int(sw2.max())]
        leg["eigendecomposition_share_of_hip_pca"] = (leg["syevj_covariances"]["median_ms"] + leg["syevj_retained_order"]["median_ms"]) \
            / leg["hip_pca"]["median_ms"]
        res["E=%g" % E] = leg
    res["note"] = ("hip_pca: device events around spk_pca_plda_batch, rows in HBM; hip_rows_scores: events around the score terms and the three "
                   "per-recording kernels; host_*: wall clock of diarize.pca_rows(backend='host') "
                   "and of the numpy scores; hip_pca_one_recording: the first recording alone")
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
