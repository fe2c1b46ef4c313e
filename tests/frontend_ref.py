"""Independent numpy implementation of the feature front end (DESIGN.md "Feature front end"): Kaldi's compute-fbank-feats (raw log
energy included), compute-vad, apply-cmvn-sliding --norm-vars=false --center=true and select-voiced-frames, for one utterance.

fp64 is the oracle.  dtype=np.float32 runs the same algorithm in float32 (tables built in fp64 and rounded once, as the GPU path
does; FFT by torch.fft.rfft on float32): its error against fp64 is the yardstick of the GPU tolerances.  Dither is an argument: the
noise [T, L] to add (times dither), e.g. the noise the kernel exports."""
import math

import numpy as np
import torch

FLT_EPSILON = 1.1920928955078125e-07


def frame_params(fs, frame_length_ms, frame_shift_ms):
    L = int(fs * frame_length_ms * 0.001)
    S = int(fs * frame_shift_ms * 0.001)
    return L, S, 2 ** (L - 1).bit_length()


def num_frames(N, L, S, snip_edges):
    return 1 + (N - L) // S if snip_edges else (N + S // 2) // S


def frames(x, L, S, snip_edges):
    """[T, L] sample indices -> samples; snip_edges=false reflects once: s < 0 -> -s-1, s >= N -> 2N-1-s"""
    N = len(x)
    T = num_frames(N, L, S, snip_edges)
    off = 0 if snip_edges else L // 2 - S // 2
    s = np.arange(T)[:, None] * S - off + np.arange(L)[None, :]
    s = np.where(s < 0, -s - 1, s)
    s = np.where(s >= N, 2 * N - 1 - s, s)
    assert s.min() >= 0 and s.max() < N
    return np.asarray(x, dtype=np.float64)[s]


def window(kind, L, blackman_coeff=0.42):
    n = np.arange(L, dtype=np.float64)
    c = np.cos(2 * math.pi * n / (L - 1))
    if kind == "povey":
        return (0.5 - 0.5 * c) ** 0.85
    if kind == "hanning":
        return 0.5 - 0.5 * c
    if kind == "hamming":
        return 0.54 - 0.46 * c
    if kind == "rectangular":
        return np.ones(L)
    if kind == "blackman":
        return blackman_coeff - 0.5 * c + (0.5 - blackman_coeff) * np.cos(4 * math.pi * n / (L - 1))
    raise ValueError(kind)


def mel_weights(F, P, fs, low_freq, high_freq):
    """[F, P/2] Kaldi triangular filters over FFT bins 0 .. P/2-1"""
    nyq = fs / 2.0
    if high_freq <= 0:
        high_freq += nyq

    def mel(f):
        return 1127.0 * np.log1p(np.asarray(f, dtype=np.float64) / 700.0)
    ml, mh = mel(low_freq), mel(high_freq)
    d = (mh - ml) / (F + 1)
    out = np.zeros((F, P // 2))
    m = mel(np.arange(P // 2) * (fs / P))
    for i in range(F):
        l, c, r = ml + i * d, ml + (i + 1) * d, ml + (i + 2) * d
        out[i] = np.maximum(0.0, np.minimum((m - l) / (c - l), (r - m) / (r - c)))
    return out


DEFAULTS = dict(sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0, dither=1.0, preemphasis_coefficient=0.97,
                remove_dc_offset=True, window_type="povey", blackman_coeff=0.42, snip_edges=True, num_mel_bins=23,
                low_freq=20.0, high_freq=0.0, energy_floor=0.0)


def fbank(x, noise=None, dtype=np.float64, **kw):
    """x: int16-scale samples [N].  Returns (log-mel [T, F], raw log energy [T]) in `dtype`."""
    o = dict(DEFAULTS, **kw)
    L, S, P = frame_params(o["sample_frequency"], o["frame_length"], o["frame_shift"])
    fr = frames(x, L, S, o["snip_edges"]).astype(dtype)
    if noise is not None and o["dither"] != 0:
        fr = fr + (o["dither"] * np.asarray(noise, dtype=np.float64)[:fr.shape[0], :L]).astype(dtype)
    if o["remove_dc_offset"]:
        fr = fr - fr.mean(1, keepdims=True, dtype=dtype).astype(dtype)
    e = np.log(np.maximum((fr * fr).sum(1, dtype=dtype), dtype(FLT_EPSILON)))
    if o["energy_floor"] > 0:
        e = np.maximum(e, dtype(math.log(o["energy_floor"])))
    c = dtype(o["preemphasis_coefficient"])
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], 1)
    fr = fr - c * prev
    fr = fr * window(o["window_type"], L, o["blackman_coeff"]).astype(dtype)[None, :]
    pad = np.zeros((fr.shape[0], P), dtype=dtype)
    pad[:, :L] = fr
    if dtype == np.float64:
        spec = np.fft.rfft(pad, axis=1)
        pw = (spec.real ** 2 + spec.imag ** 2)[:, :P // 2]
    else:
        spec = torch.fft.rfft(torch.from_numpy(pad), dim=1)
        pw = (spec.real * spec.real + spec.imag * spec.imag).numpy()[:, :P // 2]
    mw = mel_weights(o["num_mel_bins"], P, o["sample_frequency"], o["low_freq"], o["high_freq"]).astype(dtype)
    mel = pw @ mw.T
    return np.log(np.maximum(mel, dtype(FLT_EPSILON))).astype(dtype), e.astype(dtype)


def vad(loge, vad_energy_threshold=5.0, vad_energy_mean_scale=0.5, vad_frames_context=0, vad_proportion_threshold=0.6):
    """compute-vad decisions [T] (int32 0/1) from raw log energies [T]"""
    e = np.asarray(loge)
    T = len(e)
    if T == 0:                  # an utterance without frames: no decisions (and no mean to divide for)
        return np.zeros(0, dtype=np.int32)
    thr = vad_energy_threshold + vad_energy_mean_scale * float(np.asarray(e, dtype=np.float64).sum()) / T
    above = e.astype(np.float64) > thr
    out = np.zeros(T, dtype=np.int32)
    c = vad_frames_context
    for t in range(T):
        lo, hi = max(0, t - c), min(T, t + c + 1)
        out[t] = int(above[lo:hi].sum() >= (hi - lo) * vad_proportion_threshold)
    return out


def cmn_window(t, T, W):
    """[start, end) of the centred sliding window of frame t"""
    start = t - W // 2
    end = start + W
    if start < 0:
        end -= start
        start = 0
    if end > T:
        start -= end - T
        end = T
        start = max(start, 0)
    return start, end


def sliding_cmn(x, W):
    """x [T, F] -> x[t] - mean(x[start:end]) in fp64"""
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    out = np.empty_like(x)
    for t in range(T):
        s, e = cmn_window(t, T, W)
        out[t] = x[t] - x[s:e].mean(0)
    return out


def select_voiced(x, v):
    return np.asarray(x)[np.asarray(v) != 0]
