"""Independent numpy implementation of the resampler (DESIGN.md "Feature front end", "Resampling"): Kaldi's LinearResample /
ResampleWaveform for one utterance - the counterpart of tests/frontend_ref.py.

fp64 is the oracle, pinned by tests/golden/resample/ (outputs of the reference's kaldi.py: resample_waveform).  dtype=np.float32 runs
the same sums in float32: tables built in fp64 and rounded once, as the GPU path does, products and sums rounded to float32 tap by
tap in index order (no FMA); its error against fp64 is the yardstick of the GPU tolerances."""
import math

import numpy as np

ZEROS = 6          # lowpass_filter_width: zero crossings of the windowed sinc


def num_resampled(n, fi, fo):
    """LinearResample::GetNumOutputSamples, in ticks of 1 / lcm(fi, fo)"""
    if n <= 0:
        return 0
    tick = fi * fo // math.gcd(fi, fo)
    length = n * (tick // fi)
    per_out = tick // fo
    last = length // per_out
    if last * per_out == length:
        last -= 1
    return last + 1


def tables(fi, fo):
    """(iu, ou, K, first [ou] int64, w [ou][K] fp64)"""
    g = math.gcd(fi, fo)
    iu, ou = fi // g, fo // g
    fc = 0.99 * 0.5 * min(fi, fo)
    ww = ZEROS / (2 * fc)
    first = np.zeros(ou, dtype=np.int64)
    last = np.zeros(ou, dtype=np.int64)
    for p in range(ou):
        t = np.float64(p) / fo
        first[p] = int(np.ceil((t - ww) * fi))
        last[p] = int(np.floor((t + ww) * fi))
    K = int((last - first + 1).max())
    w = np.zeros((ou, K))
    for p in range(ou):
        t = np.float64(p) / fo
        dt = (first[p] + np.arange(K)).astype(np.float64) / fi - t
        win = np.zeros(K)
        inside = np.abs(dt) < ww
        win[inside] = 0.5 * (1 + np.cos(2 * math.pi * fc / ZEROS * dt[inside]))
        nz = dt != 0
        sinc = np.full(K, 2 * fc)
        sinc[nz] = np.sin(2 * math.pi * fc * dt[nz]) / (math.pi * dt[nz])
        w[p] = win * sinc / fi
    return iu, ou, K, first, w


def resample(x, fi, fo, dtype=np.float64):
    """x: samples [n] -> [num_resampled(n)] in `dtype`; x is taken as 0 outside [0, n)"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    iu, ou, K, first, w = tables(fi, fo)
    n_out = num_resampled(n, fi, fo)
    lo, hi = int(min(first.min(), 0)), int(first.max()) + ((max(n_out, 1) - 1) // ou) * iu + K
    pad = np.zeros(hi - lo + 1, dtype=dtype)
    pad[-lo:-lo + n] = x.astype(dtype)
    wd = w.astype(dtype)
    j = np.arange(n_out)
    p, u = j % ou, j // ou
    base = first[p] + u * iu - lo
    y = np.zeros(n_out, dtype=dtype)
    for k in range(K):                       # taps in index order; in float32 every product and sum rounds to float32
        y = (y + wd[p, k] * pad[base + k]).astype(dtype)
    return y
