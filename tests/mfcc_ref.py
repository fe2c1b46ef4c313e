"""Independent numpy implementation of Kaldi's compute-mfcc-feats for one utterance, on top of the fbank
oracle tests/frontend_ref.py: log-mel energies, the DCT-II with Kaldi's first row, the cepstral lifter, the energy in C0 and the
HTK order.

fp64 is the oracle.  dtype=np.float32 is the float32 restatement (the DCT and lifter tables built in fp64 and rounded once, as the
GPU path does; float32 arithmetic): its error against fp64 is the yardstick of the GPU tolerances."""
import math

import numpy as np

import frontend_ref as R

DEFAULTS = dict(R.DEFAULTS, num_ceps=13, use_energy=True, cepstral_lifter=22.0, htk_compat=False)


def dct_matrix(C, F):
    """[C, F]: D[0][n] = sqrt(1 / F), D[k][n] = sqrt(2 / F) cos(pi / F (n + 0.5) k)"""
    d = np.empty((C, F))
    for k in range(C):
        for n in range(F):
            d[k, n] = math.sqrt(1.0 / F) if k == 0 else math.sqrt(2.0 / F) * math.cos(math.pi / F * (n + 0.5) * k)
    return d


def lifter(C, Q):
    return np.array([1.0 + 0.5 * Q * math.sin(math.pi * k / Q) if Q != 0 else 1.0 for k in range(C)])


def mfcc(x, noise=None, dtype=np.float64, **kw):
    """x: int16-scale samples [N].  Returns (mfcc [T, C], raw log energy [T] floored by log(energy_floor)) in `dtype`."""
    o = dict(DEFAULTS, **kw)
    C, F, Q = o["num_ceps"], o["num_mel_bins"], o["cepstral_lifter"]
    fb_kw = {k: v for k, v in o.items() if k in R.DEFAULTS}
    lm, e = R.fbank(x, noise=noise, dtype=dtype, **fb_kw)
    c = (lm @ dct_matrix(C, F).astype(dtype).T).astype(dtype)
    c = c * lifter(C, Q).astype(dtype)[None, :]
    if o["use_energy"]:
        c[:, 0] = e
    if o["htk_compat"]:
        c0 = c[:, :1] if o["use_energy"] else c[:, :1] * dtype(math.sqrt(2.0))
        c = np.concatenate([c[:, 1:], c0], 1)
    return c.astype(dtype), e
