#!/usr/bin/env python3
"""Host against hip for the evaluation stage on synthetic trial lists of 10^6 and 10^7 trials:

  error_rates       scoring.error_rates (EER + two minDCFs from one sort) from host arrays: `host` is numpy, `hip` uploads the
                    scores and labels, sorts and sweeps on the device and brings the report down;
  sort_sweep_device the device part alone (spk_sort_trials + spk_error_sweep on scores already in HBM), by device events;
  snorm             the adaptive S-norm expression on arrays (what score_and_report runs): numpy against spk_trial_snorm;
  snorm_file        scoring.adaptive_snorm from a score file to a score file (at --file-trials trials, 10^6 by default: both back
                    ends spend their time parsing and formatting text, the per-trial Python loop of the host is what `hip` removes).

Every leg is warmed up once, then host and hip alternate `--reps` times; medians and the spread (min, max) are reported, and the
two reports are checked to be equal.  Needs a GPU.

    python tools/backend_bench.py --out profiles/backend_eval_bench.json
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


def timed(fn, sync):
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--file-trials", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--utts", type=int, default=20000, help="utterances the trials are drawn from (S-norm statistics tables)")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "backend_bench measures the device path: it needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops, scoring
    res = {"tool": "backend_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "sizes": {}}
    for T in a.trials:
        rng = np.random.RandomState(T % 1000 + 1)
        lab = (rng.rand(T) < 0.05).astype(np.uint8)
        s = (rng.randn(T) * 0.15 + 0.5 * lab).astype(np.float32).astype(np.float64)       # cosine-like float32 scores, widened
        ia, ib = rng.randint(a.utts, size=T).astype(np.int32), rng.randint(a.utts, size=T).astype(np.int32)
        mu, sd = rng.randn(a.utts) * 0.05, np.abs(rng.randn(a.utts)) * 0.05 + 0.02
        legs = {k: [] for k in ("error_rates_host", "error_rates_hip", "sort_device", "sweep_device", "snorm_host", "snorm_hip_upload",
                                "snorm_hip_device")}
        sdev, ldev = torch.from_numpy(s).cuda(), torch.from_numpy(lab).cuda()
        dv = [torch.from_numpy(v).cuda() for v in (ia, ib, mu, sd)]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for rep in range(-1, a.reps):                       # rep -1: warm-up of every leg at this size
            t_host, r_host = timed(lambda: scoring.error_rates(s, lab, backend="host"), False)
            t_hip, r_hip = timed(lambda: scoring.error_rates(s, lab, backend="hip"), True)
            assert r_host == r_hip, (r_host, r_hip)
            ev[0].record()
            order = ops.sort_trials(sdev)
            ev[1].record()
            ops.error_sweep(sdev, ldev, order, scoring.DEFAULT_COSTS)
            ev[2].record()
            torch.cuda.synchronize()
            t_sn_host, sn_host = timed(lambda: scoring._snorm_host(s, ia, ib, mu, sd, mu, sd), False)
            t_sn_up, sn_dev = timed(lambda: scoring._snorm_device(s, ia, ib, mu, sd, mu, sd), True)
            t_sn_dev, _ = timed(lambda: ops.trial_snorm(sdev, dv[0], dv[1], dv[2], dv[3], dv[2], dv[3]), True)
            assert np.array_equal(sn_dev.cpu().numpy(), sn_host)
            if rep >= 0:
                for k, v in (("error_rates_host", t_host), ("error_rates_hip", t_hip), ("sort_device", ev[0].elapsed_time(ev[1])),
                             ("sweep_device", ev[1].elapsed_time(ev[2])), ("snorm_host", t_sn_host), ("snorm_hip_upload", t_sn_up),
                             ("snorm_hip_device", t_sn_dev)):
                    legs[k].append(v)
        entry = {k: stats(v) for k, v in legs.items()}
        entry["report"] = r_hip
        entry["sort_workspace_bytes"] = int(pytorch_kaldi_resnet_amd.hip.lib().spk_sort_trials_workspace(T))
        res["sizes"][str(T)] = entry
        sys.stderr.write("%d trials: %s\n" % (T, json.dumps(entry)))
    # file to file, as scripts/adaptive_snorm.py runs it
    T = a.file_trials
    if T > 0:
        rng = np.random.RandomState(9)
        d = tempfile.mkdtemp(prefix="spk_backend_bench_")
        names = ["utt%06d" % i for i in range(a.utts)]
        st = {k: (float(m), float(v)) for k, m, v in zip(names, rng.randn(a.utts) * 0.05, np.abs(rng.randn(a.utts)) * 0.05 + 0.02)}
        ia, ib, sc = rng.randint(a.utts, size=T), rng.randint(a.utts, size=T), (rng.randn(T) * 0.15).astype(np.float32)
        with open(os.path.join(d, "scores"), "w") as f:
            for x, y, v in zip(ia, ib, sc):
                f.write("%s %s %s\n" % (names[x], names[y], v))
        legs = {"snorm_file_host": [], "snorm_file_hip": []}
        for rep in range(-1, a.reps):
            th, _ = timed(lambda: scoring.adaptive_snorm(st, st, os.path.join(d, "scores"), os.path.join(d, "out_host")), False)
            tg, _ = timed(lambda: scoring.adaptive_snorm(st, st, os.path.join(d, "scores"), os.path.join(d, "out_hip"), backend="hip"), True)
            if rep >= 0:
                legs["snorm_file_host"].append(th)
                legs["snorm_file_hip"].append(tg)
        assert open(os.path.join(d, "out_host")).read() == open(os.path.join(d, "out_hip")).read()
        res["snorm_file"] = dict({k: stats(v) for k, v in legs.items()}, trials=T)
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
