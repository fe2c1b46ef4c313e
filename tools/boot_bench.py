#!/usr/bin/env python3
"""Speaker-level bootstrap of the error-rate sweep on both back ends, recorded and not gated:

  workload   synthetic trial lists of 10^5 and 10^7 trials over U = 1 251 speakers (half the trials inside a speaker: targets, the rest
             across two speakers: non-targets), scores N(+-2, 1), R = 1 000 replicates of bootstrap_counts(U, R, 0), two minimum-cost
             and two actual-cost triples;
  legs       `hip`, by device events around the calls of ops.py, the sorted list resident on the device: the pack (once per system), the
             whole sweep of R replicates, and the sweep stopped after each phase (`upto`): the differences are the phases; `host`: the
             same replicates by bootstrap.py's numpy sweep, wall clock, on the first --host-replicates rows of the same table and scaled
             to R (the sort counted once, the rest times R / rows) - the file states the factor.  The rows the host ran are compared with the device's, bit for bit.
  rates      per phase against the bytes it streams (8-byte records once per group of G replicates and pass; the per-tile partials
             written and read) and, for the rates phase, the fp64 divisions done (2 per weighted position).
The host leg is the host side of the same code base, not an outside toolkit: no other time has been measured for this workload, so it
is the only yardstick there is.

Needs a GPU.    python tools/boot_bench.py --out profiles/boot_bench.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, nargs="+", default=[100000, 10000000])
    ap.add_argument("--units", type=int, default=1251)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-replicates", type=int, nargs="+", default=[50, 3], help="rows of the table the host leg runs, per --trials entry")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "boot_bench measures the device path: it needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import bootstrap as B, calibration as C, hip, ops
    COSTS = [(0.01, 1.0, 1.0), (0.001, 1.0, 1.0)]
    U, R = a.units, a.replicates
    G, pitch = ops.boot_sizes(U)
    eta = [C.bayes_threshold(*c) for c in COSTS]
    counts = B.bootstrap_counts(U, R, 0)
    cmax = int(counts.max())
    result = {"device": torch.cuda.get_device_name(0), "units": U, "replicates": R, "cost_triples": len(COSTS), "act_triples": len(COSTS),
              "sizes": dict(zip(("tile", "max_units", "max_count", "max_costs", "max_group", "threads"), ops.boot_sizes())),
              "group": G, "pitch": pitch, "largest_count": cmax,
              "yardstick": "the host back end of this same code (bootstrap.py, numpy) on rows of the same table; no other time exists",
              "cases": []}
    for T, hr in zip(a.trials, a.host_replicates):
        rng = np.random.RandomState(T % 1000)
        ua = rng.randint(0, U, size=T).astype(np.int32)
        ub = np.where(rng.rand(T) < 0.5, ua, rng.randint(0, U, size=T)).astype(np.int32)
        lab = (ua == ub).astype(np.uint8)
        s = rng.randn(T) + np.where(lab > 0, 2.0, -2.0)
        sd, ld = torch.from_numpy(s).cuda(), torch.from_numpy(lab).cuda()
        uad, ubd = torch.from_numpy(ua).cuda(), torch.from_numpy(ub).cuda()
        table = ops.boot_table(counts, sd.device)
        tile = ops.boot_sizes()[0]
        nb = -(-T // tile)
        per = hip.lib().spkb_sweep_ws_elems(T, 2, 2, 1)
        chunk = max(1, ops.BOOT_WS_BYTES // (8 * per) // G) * G
        case = {"trials": T, "targets": int(lab.sum()), "tiles": nb, "replicates_per_chunk": min(chunk, R)}
        # warm-up of both legs; the rows the host runs are the device's, bit for bit
        order = ops.sort_trials(sd)
        rec, q = ops.boot_pack(sd, ld, order, uad, ubd, eta, U)
        out_d, out_i = ops.boot_sweep(rec, q, table, U, cmax, COSTS, COSTS)
        dd, di = out_d.cpu().numpy(), out_i.cpu().numpy()
        t0 = time.perf_counter()
        np.lexsort((np.arange(T), s + 0.0))                            # the host's sort alone: it is paid once, not per replicate
        host_sort_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        host = B.bootstrap_replicates(s, lab, ua, ub, counts[:hr], COSTS, COSTS)
        host_ms = (time.perf_counter() - t0) * 1e3
        case["host_rows_equal_device"] = bool(host["d"].tobytes() == dd[:hr].tobytes() and host["i"].tobytes() == di[:hr].tobytes())
        case["degenerate"] = int((di[:, 0] != 0).sum())
        times = {"sort": [], "pack": [], "sweep": [], "upto_counts": [], "upto_offsets": [], "upto_rates": []}
        for _ in range(a.reps):
            times["sort"].append(device_ms(lambda: ops.sort_trials(sd))[0])
            times["pack"].append(device_ms(lambda: ops.boot_pack(sd, ld, order, uad, ubd, eta, U))[0])
            times["sweep"].append(device_ms(lambda: ops.boot_sweep(rec, q, table, U, cmax, COSTS, COSTS))[0])
            for k, name in ((1, "upto_counts"), (2, "upto_offsets"), (3, "upto_rates")):
                times[name].append(device_ms(lambda: ops.boot_sweep(rec, q, table, U, cmax, COSTS, COSTS, upto=k))[0])
        case["times"] = {k: stats(v) for k, v in times.items()}
        med = {k: case["times"][k]["median_ms"] for k in times}
        phases = {"counts": med["upto_counts"], "offsets": med["upto_offsets"] - med["upto_counts"],
                  "rates": med["upto_rates"] - med["upto_offsets"], "final": med["sweep"] - med["upto_rates"]}
        groups = -(-R // G)
        partial_bytes = 32.0 * 3 * nb * R
        sums_bytes = 16.0 * (nb + 1) * R
        byts = {"counts": 8.0 * T * groups + 2.0 * pitch * G * nb * groups + sums_bytes, "offsets": 2 * sums_bytes,
                "rates": 8.0 * T * groups + 2.0 * pitch * G * nb * groups + sums_bytes + partial_bytes, "final": partial_bytes}
        # (a phase shorter than the spread of the runs it is a difference of has no rate)
        case["phases"] = {k: {"ms": phases[k], "bytes": byts[k], "GB_per_s": byts[k] / phases[k] / 1e6 if phases[k] > 0.01 else None}
                          for k in phases}
        case["phases"]["rates"]["fp64_divisions"] = 2.0 * T * R
        case["phases"]["rates"]["Gdiv_per_s"] = 2.0 * T * R / phases["rates"] / 1e6
        case["weighted_positions_per_s"] = float(T) * R / (med["sweep"] * 1e-3)
        scaled = host_sort_ms + max(host_ms - host_sort_ms, 0.0) * R / hr
        case["host"] = {"replicates_run": hr, "ms": host_ms, "sort_alone_ms": host_sort_ms, "scale_factor": R / float(hr),
                        "ms_scaled_to_all_replicates": scaled,
                        "note": "wall clock of one sort and %d replicates; scaled = the sort once + the rest times %g" % (hr, R / float(hr))}
        case["host_over_device"] = case["host"]["ms_scaled_to_all_replicates"] / (med["pack"] + med["sweep"])
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        del sd, ld, uad, ubd, rec, q, table, out_d, out_i, order
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
