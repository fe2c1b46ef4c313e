#!/usr/bin/env python3
"""Calibration on both back ends, recorded and not gated:

  workload   synthetic trial lists of 10^5 and 10^7 trials, 10 % targets, llr ~ N(+-3, 6); K = 1: the scores (llr - 1.5) / 4; K = 3:
             two more noisy affine views of the same llr; p_target 0.01, l2 0, epsilon 1e-18;
  legs       `hip`, by device events around the calls of ops.py, inputs resident on the device: train (max_iters 100: every launch
             pair the call enqueues, those after the stop included), train with max_iters = the evaluations it needs, one
             evaluation (max_iters 1: init, the pass over the trials, the step - its bytes/s counts the K * 8 + 1 bytes a trial is
             read as), cllr with two cost triples, sort_trials, and spk_cal_pav stopped after the tie pools, after the tiles and run
             whole: the differences are the stages; `host`: the same calls of calibration.py on numpy arrays, wall clock.  The legs
             alternate in one process after one warm-up of each.
The host leg is the host side of the same code base, not an outside toolkit: it is the only comparison there is.

Needs a GPU.    python tools/cal_bench.py --out profiles/cal_bench.json
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


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": len(v)}


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, nargs="+", default=[100000, 10000000])
    ap.add_argument("--systems", type=int, nargs="+", default=[1, 3])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2, help="repetitions of the host leg at more than 10^6 trials")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "cal_bench measures the device path: it needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import calibration as C, ops
    P, EPS, COSTS = 0.01, 1e-18, [(0.01, 1, 1), (0.001, 1, 1)]
    eta = [C.bayes_threshold(*c) for c in COSTS]
    result = {"device": torch.cuda.get_device_name(0), "p_target": P, "sizes": dict(zip(("block", "pav_tile", "state", "threads"), ops.cal_sizes())),
              "cases": []}
    for T in a.trials:
        for K in a.systems:
            rng = np.random.RandomState(T % 1000 + K)
            lab = (rng.rand(T) < 0.1).astype(np.uint8)
            llr = np.where(lab > 0, 3.0, -3.0) + np.sqrt(6.0) * rng.randn(T)
            cols = [(llr - 1.5) / 4] + [(llr + (1.0 + k) * rng.randn(T)) / (2.0 + k) + 0.25 * k for k in range(1, K)]
            cols = np.ascontiguousarray(cols)
            n_tar = int(lab.sum())
            cd, ld = torch.from_numpy(cols).cuda(), torch.from_numpy(lab).cuda()
            tau = C.logit(P)
            reps = a.reps
            hreps = a.reps if T <= 1000000 else a.host_reps
            case = {"trials": T, "systems": K, "targets": n_tar}
            # warm-up of both legs; the models the timed runs must reproduce
            dev = C.train(cd, lab, P, 0.0, EPS, 100, backend="hip")
            host = C.train(cols, lab, P, 0.0, EPS, 100)
            case.update(status=dev.status, evaluations=dev.evaluations, host_status=host.status, host_evaluations=host.evaluations,
                        theta=dev.theta.tolist(), theta_max_difference=float(np.abs(dev.theta - host.theta).max()))
            s_dev = cd[0].contiguous()
            order = ops.sort_trials(s_dev)
            ops.cal_pav(s_dev, ld, order)
            ops.cal_cllr(s_dev, ld, COSTS, eta)
            legs = {k: [] for k in ("train", "train_exact", "evaluation", "cllr", "sort", "pav_ties", "pav_tiles", "pav_all",
                                    "host_train", "host_evaluation", "host_cllr", "host_min_cllr")}
            for rep in range(reps):
                legs["train"].append(device_ms(lambda: ops.cal_train(cd, ld, n_tar, P, tau, 0.0, EPS, 100))[0])
                legs["train_exact"].append(device_ms(lambda: ops.cal_train(cd, ld, n_tar, P, tau, 0.0, EPS, dev.evaluations))[0])
                legs["evaluation"].append(device_ms(lambda: ops.cal_train(cd, ld, n_tar, P, tau, 0.0, EPS, 1))[0])
                legs["cllr"].append(device_ms(lambda: ops.cal_cllr(s_dev, ld, COSTS, eta))[0])
                legs["sort"].append(device_ms(lambda: ops.sort_trials(s_dev))[0])
                legs["pav_ties"].append(device_ms(lambda: ops.cal_pav(s_dev, ld, order, upto=1))[0])
                legs["pav_tiles"].append(device_ms(lambda: ops.cal_pav(s_dev, ld, order, upto=2))[0])
                ms, r = device_ms(lambda: ops.cal_pav(s_dev, ld, order))
                legs["pav_all"].append(ms)
                if rep < hreps:
                    legs["host_train"].append(host_ms(lambda: C.train(cols, lab, P, 0.0, EPS, 100))[0])
                    legs["host_evaluation"].append(host_ms(lambda: C.objective_terms(cols, lab, host.theta, P, 0.0, n_tar))[0])
                    legs["host_cllr"].append(host_ms(lambda: C.evaluate(cols[0], lab, COSTS))[0])
                    ms, hm = host_ms(lambda: C.min_cllr(cols[0], lab))
                    legs["host_min_cllr"].append(ms)
            counts = r["counts"].cpu().tolist()
            case["pools"] = {"tie": counts[0], "after_tiles": counts[1], "after_second_tiles": counts[2], "final": counts[3]}
            case["min_cllr"] = float(r["min_cllr"].cpu()[0])
            case["host_min_cllr_value"] = hm[0]
            case["same_pools"] = bool(np.array_equal(r["pools"][:counts[3]].cpu().numpy(), hm[1]))
            case["times"] = {k: stats(v) for k, v in legs.items()}
            med = lambda k: case["times"][k]["median_ms"]                                # noqa: E731
            case["pav_stages_ms"] = {"sort": med("sort"), "tie_pools": med("pav_ties"), "tiles": med("pav_tiles") - med("pav_ties"),
                                     "final_merge_and_index": med("pav_all") - med("pav_tiles")}
            nbytes = (8.0 * K + 1) * T
            case["evaluation_bytes"] = nbytes
            case["evaluation_bytes_per_s"] = nbytes / (med("evaluation") * 1e-3)
            print(json.dumps({k: case[k] for k in ("trials", "systems", "evaluations", "pools", "pav_stages_ms")}), flush=True)
            print({k: round(v["median_ms"], 3) for k, v in case["times"].items()}, flush=True)
            result["cases"].append(case)
            del cd, ld, s_dev, order, r
            torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
