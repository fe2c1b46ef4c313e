"""Windowed extraction restated on the CPU - test infrastructure only, nothing here imports the package.

The window rule one frame at a time, the gather as numpy slicing, the length-weighted mean in fp64 with the bound of the fp32 kernel:
a chain of K fused multiply-adds (one rounding each, of a partial sum that sum_r w_r |e_r| bounds), the correctly rounded reciprocal
of the exact weight total (the weights are window lengths: their sums are exact in fp32) and the final multiply - K + 2 roundings of
at most 2^-24 relative, each of a quantity bounded by sum w |e| / tot:
    |gpu - mean| <= (K + 2) 2^-24 sum_r w_r |e_r| / tot
"""
import numpy as np


def brute_windows(n, W, P, M):
    """windows of an utterance of n frames -> list of (start, length), or None when the utterance is skipped (n < M)"""
    if n < M:
        return None
    out, k = [], 0
    while True:
        frames = [t for t in range(k * P, k * P + W) if t < n]          # one frame at a time
        last = k * P + W >= n
        if not last or len(frames) >= M or k == 0:
            out.append((k * P, len(frames)))
        if last:
            return out
        k += 1


def brute_plan(lengths, W, P, M):
    """-> (utt, start, length, skipped) as lists, utterance order then window order"""
    utt, start, length, skipped = [], [], [], []
    for u, n in enumerate(lengths):
        w = brute_windows(int(n), W, P, M)
        if w is None:
            skipped.append(u)
            continue
        for s, l in w:
            utt.append(u)
            start.append(s)
            length.append(l)
    return utt, start, length, skipped


def gather_ref(src, row, start, length, Wcap):
    """src [B][F][T] numpy -> [N][F][Wcap]: the slices, +0 past each length"""
    out = np.zeros((len(row), src.shape[1], Wcap), dtype=src.dtype)
    for i, (r, s, l) in enumerate(zip(row, start, length)):
        out[i, :, :l] = src[r, :, s:s + l]
    return out


def mean_ref(emb, seg_off, weight):
    """emb [N][D], seg_off [U+1], weight [N] -> (fp64 mean [U][D], bound [U][D])"""
    e, w = np.asarray(emb, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    means, bounds = [], []
    for u in range(len(seg_off) - 1):
        a, b = int(seg_off[u]), int(seg_off[u + 1])
        tot = w[a:b].sum()
        means.append((w[a:b, None] * e[a:b]).sum(0) / tot)
        bounds.append((b - a + 2) * 2.0 ** -24 * (w[a:b, None] * np.abs(e[a:b])).sum(0) / tot)
    return np.stack(means), np.stack(bounds)
