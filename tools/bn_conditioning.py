#!/usr/bin/env python3
"""How far the BatchNorm inputs of the golden states sit from the conditioning limit of sumsq / n - mean^2:
the largest mean^2 / sigma^2 over all BatchNorm inputs and channels of a training-mode forward of the CPU oracle on the golden
batch, statistics in fp64.  CPU only.

  python tools/bn_conditioning.py [golden case ...]        (default: c1_r34_aam r34_aam_t300 r101_aam)
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import spk_oracle as O  # noqa: E402
from oracle import weights as W  # noqa: E402


def ratios(name):
    """-> [(largest mean^2 / sigma^2 of the layer, its channel, C, values per channel)] in the order of the forward"""
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", name + ".json")))
    kw = dict(pooling=meta["pooling"], loss=meta["loss"], arch=meta["arch"])
    st = O.to_torch_state(W.make_state(meta["seed"], meta["spk_num"], meta["feat_dim"], **kw))
    x, y = W.make_input(meta["seed"] + 1, meta["batch"], meta["feat_dim"], meta["frames"], meta["spk_num"])
    rec, real = [], F.batch_norm

    def bn(x, *a, **k):
        xd = x.detach().double()
        dims = [d for d in range(xd.dim()) if d != 1]
        r = xd.mean(dims) ** 2 / xd.var(dims, unbiased=False)
        rec.append((float(r.max()), int(r.argmax()), xd.shape[1], xd.numel() // xd.shape[1]))
        return real(x, *a, **k)

    O.F.batch_norm = bn
    try:
        with torch.no_grad():
            O.forward(st, torch.from_numpy(x), torch.from_numpy(y), train=True, **kw)
    finally:
        O.F.batch_norm = real
    return meta, rec


if __name__ == "__main__":
    for name in sys.argv[1:] or ["c1_r34_aam", "r34_aam_t300", "r101_aam"]:
        meta, rec = ratios(name)
        worst = max(rec)
        print("%s (%s, batch %d, %d frames): %d BatchNorm layers, largest mean^2/sigma^2 %.2f (layer %d, channel %d of %d, %d values "
              "per channel), median over layers of the per-layer maximum %.2f" % (
                  name, meta["arch"], meta["batch"], meta["frames"], len(rec), worst[0], rec.index(worst), worst[1], worst[2],
                  worst[3], float(np.median([r[0] for r in rec]))))
