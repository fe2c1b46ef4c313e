"""Independent numpy implementation of the augmentation contract: reverberation and additive noise as the
recipe's wav-reverberate entries ask for them, for one utterance - the counterpart of tests/frontend_ref.py and tests/resample_ref.py.

fp64 (`augment`) is the oracle: the formulas as they stand, the convolutions by their definition.  `augment32` restates the arithmetic of
csrc/augment.hip in float32: the uniformly partitioned overlap-save convolution with blocks of 1024 samples and a radix-2
decimation-in-time FFT of 2048 points written out here (numpy.fft is another factorisation, and more accurate), the bin products
summed in ascending partition order, float32 twiddles rounded once from fp64; sums of squares and the scalars they give in fp64;
one rounding to float32 per sample operation.  Its error against fp64 is the yardstick of the GPU tolerances - it never sees the
kernel's output."""
import numpy as np

P = 1024
L = 2 * P
LOGL = 11


def early_window(h, fs):
    """(s, e0, e1): the peak (first maximum of the signed value) and the early part h[e0:e1] of an impulse response"""
    h = np.asarray(h)
    s = int(np.argmax(h))
    return s, max(0, s - int(0.001 * fs)), min(len(h), s + int(0.05 * fs))


def fill(r, duration, fs):
    """the additive signal as it is added: repeated or cut to int(fs * duration) samples, or as it is"""
    r = np.asarray(r)
    if duration is None:
        return r
    D = int(fs * duration)
    return r[np.arange(D) % len(r)]


def convolve(x, h):
    """full linear convolution in fp64 by its definition, y[i] = sum_t h[t] x[i - t]: one shifted, scaled copy of x per tap"""
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    y = np.zeros(len(x) + len(h) - 1)
    for t in range(len(h)):
        y[t:t + len(x)] += h[t] * x
    return y


def augment(x, h=None, noises=(), fs=16000, quantize=False, conv=convolve, detail=None):
    """x [N] -> out [N] (fp64), or (out, clipped count) with quantize.  noises: (samples, duration or None, start seconds, snr dB).
    detail: a dict that receives p_before, p_sig, p_after, M, s, g, the scales a and the powers q, and y before the gain."""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    p_before = (x ** 2).sum() / N
    if h is not None:
        h = np.asarray(h, dtype=np.float64)
        s, e0, e1 = early_window(h, fs)
        p_sig = (conv(x, h[e0:e1]) ** 2).mean()
        y = conv(x, h).copy()
    else:
        s, p_sig, y = 0, p_before, x.copy()
    M = len(y)
    scales, powers = [], []
    for r, duration, start, snr in noises:
        n = fill(np.asarray(r, dtype=np.float64), duration, fs)
        q = (n ** 2).sum() / len(n)
        a = np.sqrt(10.0 ** (-snr / 10.0) * p_sig / q)
        o = int(start * fs)
        scales.append(a)
        powers.append(q)
        if o < M:
            k = min(len(n), M - o)
            y[o:o + k] += a * n[:k]
    p_after = (y ** 2).sum() / M
    plain = h is None and len(noises) == 0
    g = 1.0 if (plain or p_after == 0) else np.sqrt(p_before / p_after)
    out = g * y[s:s + N]
    if detail is not None:
        detail.update(p_before=p_before, p_sig=p_sig, p_after=p_after, M=M, s=s, g=g, a=scales, q=powers, y=y)
    if not quantize:
        return out
    t = np.trunc(out)
    return np.clip(t, -32768, 32767), int(((t > 32767) | (t < -32768)).sum())


# ---- the kernel's arithmetic in float32 ----
def _twiddles():
    k = np.arange(L // 2, dtype=np.float64)
    return (np.cos(-2 * np.pi * k / L).astype(np.float32), np.sin(-2 * np.pi * k / L).astype(np.float32))


_BREV = np.array([int(format(n, "011b")[::-1], 2) for n in range(L)])


def fft32(re, im):
    """radix-2 decimation-in-time FFT of rows of L points, every product and sum rounded to float32 (no FMA)"""
    wr, wi = _twiddles()
    zr = np.zeros(re.shape, dtype=np.float32)
    zi = np.zeros(im.shape, dtype=np.float32)
    zr[..., _BREV] = re
    zi[..., _BREV] = im
    k = np.arange(L // 2)
    for st in range(LOGL):
        half = 1 << st
        pos = k & (half - 1)
        i0 = ((k >> st) << (st + 1)) + pos
        i1 = i0 + half
        tr, ti = wr[pos << (LOGL - 1 - st)], wi[pos << (LOGL - 1 - st)]
        ur, ui, vr, vi = zr[..., i0], zi[..., i0], zr[..., i1], zi[..., i1]
        br = (vr * tr).astype(np.float32) - (vi * ti).astype(np.float32)
        bi = (vr * ti).astype(np.float32) + (vi * tr).astype(np.float32)
        zr[..., i0], zi[..., i0] = ur + br, ui + bi
        zr[..., i1], zi[..., i1] = ur - br, ui - bi
    return zr, zi


def conv32(x, h):
    """x * h in float32 by partitioned overlap-save, as aug_spectra_kernel / aug_conv_kernel compute it"""
    x = np.asarray(x, dtype=np.float32)
    h = np.asarray(h, dtype=np.float32)
    N, R = len(x), len(h)
    M = N + R - 1
    nwx, npart, nb = -(-N // P) + 1, -(-R // P), -(-M // P)
    xp = np.zeros((nwx + 1) * P, dtype=np.float32)
    xp[P:P + N] = x                                          # window w holds x[(w - 1) P .. (w + 1) P)
    win = np.stack([xp[w * P:w * P + L] for w in range(nwx)])
    hp = np.zeros((npart, L), dtype=np.float32)
    hp.reshape(-1)[np.arange(R) // P * L + np.arange(R) % P] = h
    Xr, Xi = fft32(win, np.zeros_like(win))
    Hr, Hi = fft32(hp, np.zeros_like(hp))
    y = np.zeros(nb * P, dtype=np.float32)
    for m in range(nb):
        ar = np.zeros(P + 1, dtype=np.float32)
        ai = np.zeros(P + 1, dtype=np.float32)
        for p in range(max(0, m - (nwx - 1)), min(npart - 1, m) + 1):
            xr, xi, hr, hi = Xr[m - p, :P + 1], Xi[m - p, :P + 1], Hr[p, :P + 1], Hi[p, :P + 1]
            ar = (ar + xr * hr).astype(np.float32)
            ar = (ar - xi * hi).astype(np.float32)
            ai = (ai + xr * hi).astype(np.float32)
            ai = (ai + xi * hr).astype(np.float32)
        zr = np.zeros(L, dtype=np.float32)
        zi = np.zeros(L, dtype=np.float32)
        zr[:P + 1], zi[:P + 1] = ar, -ai                     # the conjugate spectrum: its forward FFT is conj(inverse FFT)
        zr[P + 1:], zi[P + 1:] = ar[P - 1:0:-1], ai[P - 1:0:-1]
        yr, _ = fft32(zr, zi)
        y[m * P:(m + 1) * P] = yr[P:] * np.float32(1.0 / L)
    return y[:M]


def augment32(x, h=None, noises=(), fs=16000):
    """the float32 run (quantize=False): out [N] float32"""
    x = np.asarray(x, dtype=np.float32)
    N = len(x)
    p_before = (x.astype(np.float64) ** 2).sum() / N
    if h is not None:
        h = np.asarray(h, dtype=np.float32)
        s, e0, e1 = early_window(h, fs)
        p_sig = (conv32(x, h[e0:e1]).astype(np.float64) ** 2).mean()
        y = conv32(x, h)
    else:
        s, p_sig, y = 0, p_before, x.copy()
    M = len(y)
    for r, duration, start, snr in noises:
        n = fill(np.asarray(r, dtype=np.float32), duration, fs)
        q = (n.astype(np.float64) ** 2).sum() / len(n)
        a = np.sqrt(10.0 ** (-snr / 10.0) * p_sig / q)
        o = int(start * fs)
        if o < M:
            k = min(len(n), M - o)
            y[o:o + k] = (y[o:o + k].astype(np.float64) + a * n[:k].astype(np.float64)).astype(np.float32)
    p_after = (y.astype(np.float64) ** 2).sum() / M
    plain = h is None and len(noises) == 0
    g = 1.0 if (plain or p_after == 0) else np.sqrt(p_before / p_after)
    return (g * y[s:s + N].astype(np.float64)).astype(np.float32)


# ---- seeded synthetic signals of the tests ----
def speech(n, seed, amp=3000.0):
    """low-pass filtered noise with a slow envelope, at int16 scale (whole numbers, as a 16-bit file holds them)"""
    rng = np.random.default_rng(seed)
    v = np.convolve(rng.normal(0, 1, n + 31), np.hanning(32) / np.hanning(32).sum())[31:31 + n]
    env = 0.55 + 0.45 * np.sin(2 * np.pi * np.arange(n) / 7001.0 + seed)
    v = v / np.abs(v).max() * amp * env
    return np.round(v).astype(np.float32)


def impulse_response(seconds, seed, fs=16000, peak_ms=3.0, negative_larger=False):
    """exponentially decaying noise, the peak a few ms in; negative_larger: a negative sample after the peak is larger in magnitude"""
    rng = np.random.default_rng(seed)
    n = int(seconds * fs)
    s = int(peak_ms * 0.001 * fs)
    h = np.zeros(n)
    t = np.arange(n - s)
    h[s:] = 0.35 * rng.normal(0, 1, n - s) * np.exp(-t / (0.12 * seconds * fs))
    h[:s] = 0.02 * rng.normal(0, 1, s)
    h[s] = 1.0
    h = np.clip(h, -0.95, 0.95)
    h[s] = 1.0
    if negative_larger:
        h[s + 5] = -1.4
    return h.astype(np.float32)


def noise(n, seed, amp=900.0):
    rng = np.random.default_rng(seed)
    return np.round(rng.normal(0, amp, n)).astype(np.float32)
