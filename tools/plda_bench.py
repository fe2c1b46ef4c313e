#!/usr/bin/env python3
"""Host against hip for the PLDA back end at VoxCeleb scale, on one machine:

  workload   synthetic float32 embeddings (default 1.2 M x 256) of 6 000 speakers with unequal counts, LDA to 200 dimensions, 10 EM
             iterations, 5 x 10^5 trials over 20 000 test embeddings;
  steps      wall time of plda.compute_lda, plda.compute_plda and plda.plda_score on `host` and on `hip` from the same in-memory
             tables (a host clock around work that ends in a device synchronise; host and hip alternate `--reps` times after one
             warm-up of hip);
  scatter    per-launch time of spk_scatter_f64 over the whole table by device events, against its flop count 2 N D^2 and the
             N D 4 bytes it must read: achieved fp64 FLOP/s and bytes/s.  This is the method, not a gate.

Needs a GPU.    python tools/plda_bench.py --out profiles/plda_bench.json
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


class Table:
    """what plda.py reads of an embedding archive: keys in file order and the [n][D] matrix"""

    def __init__(self, keys, mat):
        self.keys_list, self.mat = keys, mat

    def __len__(self):
        return len(self.keys_list)


def synth(N, D, K, n_test, rng):
    rank = 64
    F = (rng.randn(D, rank) * np.linspace(2.0, 0.3, rank)).astype(np.float32)
    ns = np.linspace(0.5, 1.5, D).astype(np.float32)
    w = rng.gamma(2.0, 1.0, K) + 0.2                                            # unequal counts
    counts = np.maximum(1, np.floor(w / w.sum() * N)).astype(np.int64)
    counts[0] += N - counts.sum()
    spk = np.repeat(np.arange(K), counts)
    x = np.empty((N, D), dtype=np.float32)
    H = rng.randn(K, rank).astype(np.float32)
    for lo in range(0, N, 1 << 16):
        s = spk[lo:lo + (1 << 16)]
        x[lo:lo + len(s)] = 3.0 + H[s] @ F.T + 0.7 * ns * rng.randn(len(s), D).astype(np.float32)
    keys = ["u%07d" % i for i in range(N)]
    utt2spk = {k: "s%05d" % s for k, s in zip(keys, spk)}
    tspk = rng.randint(0, 1000, n_test)
    Ht = rng.randn(1000, rank).astype(np.float32)
    xt = (3.0 + Ht[tspk] @ F.T + 0.7 * ns * rng.randn(n_test, D).astype(np.float32)).astype(np.float32)
    return Table(keys, x), utt2spk, Table(["t%06d" % i for i in range(n_test)], xt), tspk


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1200000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--speakers", type=int, default=6000)
    ap.add_argument("--lda-dim", type=int, default=200)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--trials", type=int, default=500000)
    ap.add_argument("--test-utts", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skip-host", action="store_true", help="time only the hip back end")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "plda_bench measures the device path: it needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops, plda
    rng = np.random.RandomState(1)
    train, utt2spk, test, tspk = synth(a.n, a.dim, a.speakers, a.test_utts, rng)
    mean = train.mat.mean(axis=0, dtype=np.float64).astype(np.float32)
    ia, ib = rng.randint(0, a.test_utts, a.trials), rng.randint(0, a.test_utts, a.trials)
    ib[::20] = ia[::20]                                                          # at least 5 % targets
    tf = tempfile.NamedTemporaryFile("w", suffix=".trials", delete=False)
    tf.write("".join("%s %s %s\n" % (test.keys_list[i], test.keys_list[j], "target" if tspk[i] == tspk[j] else "nontarget")
                     for i, j in zip(ia, ib)))
    tf.close()
    res = {"tool": "plda_bench", "device": torch.cuda.get_device_name(0), "n": a.n, "dim": a.dim, "speakers": a.speakers,
           "lda_dim": a.lda_dim, "em_iters": a.iters, "trials": a.trials, "steps": {}}
    models = {}

    def lda(backend):
        return plda.compute_lda(train, utt2spk, a.lda_dim, mean=mean, backend=backend)[0]

    def train_plda(backend):
        return plda.compute_plda(train, utt2spk, models["lda"], a.iters, mean, backend=backend)

    def score(backend):
        return plda.plda_score(test, test, tf.name, mean, models["lda"], models["plda"], backend=backend)[0]

    backends = ["hip"] if a.skip_host else ["hip", "host"]
    for name, fn, key in (("compute_lda", lda, "lda"), ("compute_plda", train_plda, "plda"), ("plda_score", score, "scores")):
        models[key] = fn("hip")                                                  # warm-up: code objects, allocator
        t = {b: [] for b in backends}
        out = {}
        for _ in range(a.reps):
            for b in backends:
                ms, out[b] = wall(lambda: fn(b))
                t[b].append(ms)
        res["steps"][name] = {b: stats(t[b]) for b in backends}
        if "host" in out and key == "scores":
            res["steps"][name]["max_abs_host_minus_hip"] = float(np.abs(out["host"].astype(np.float64) - out["hip"]).max())
        if "host" in out and key == "plda":
            res["steps"][name]["max_rel_psi_host_minus_hip"] = float((np.abs(out["host"][2] - out["hip"][2]) / out["hip"][2]).max())
        print(name, json.dumps(res["steps"][name]), flush=True)
    # the scatter kernel alone: device events around each launch, the table already in HBM
    xd = torch.from_numpy(train.mat).cuda()
    mu = torch.from_numpy(mean.astype(np.float64)).cuda()
    ops.scatter_f64(xd, mu)
    ev = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.scatter_f64(xd, mu)
        e1.record()
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    flops, nbytes = 2.0 * a.n * a.dim * a.dim, 4.0 * a.n * a.dim
    med = float(np.median(ev))
    res["scatter"] = {"launch_ms": stats(ev), "flops": flops, "bytes_read_once": nbytes, "tflops_fp64": flops / med / 1e9,
                      "tbytes_per_s": nbytes / med / 1e9, "slab_rows": ops.scatter_slab_rows(a.n),
                      "note": "launch = slab kernel + slab reduce; bytes are the table read once (tile pairs re-read it through the caches)"}
    print("scatter", json.dumps(res["scatter"]), flush=True)
    os.unlink(tf.name)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
