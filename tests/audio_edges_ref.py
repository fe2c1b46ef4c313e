"""Case lists and helpers of the edge tests of the audio path: csrc/frontend.hip (framing, MFCC epilogue, VAD, sliding CMN and
selection), csrc/augment.hip (overlap-save reverberation, additive noise) and csrc/resample.hip.  This module builds inputs and
expectations only - it never sees a kernel's output.  tests/test_audio_edges_cpu.py proves, without a GPU, the premises the lists rest
on (which size lands on which boundary, which identity holds in the oracle, which yardstick is non-zero);
tests/test_audio_edges_gpu.py runs the kernels on them.

The fp64 oracles are the ones the feature tests use: frontend_ref.py, mfcc_ref.py, augment_ref.py, resample_ref.py.  Signals are drawn
here from numpy.random.default_rng(seed) at int16 scale and rounded to whole numbers, as a 16-bit file holds them.

Tile sizes that the library chooses (frames per framing tile, outputs per resampler tile) are asked of the library - the functions
are host code and run without a GPU.  The compile-time constants of the kernels are named below with the line they mirror."""
import functools
import math

import numpy as np

import augment_ref as A
import frontend_ref as R
import mfcc_ref as M
import resample_ref as RS

# ---- the kernels' compile-time constants ----
WAVE = 64               # frontend.hip:326 vad_kernel `t0 += 64`, :356 cmn_prefix_kernel `t0 += 64`, :234 the cepstral lane loop `k += 64`
FE_WAVES = 4            # frontend.hip:27  frames of a tile computed per round (`r += FE_WAVES`)
DCT_UNROLL = 8          # frontend.hip:238 the eight-wide DCT loop `n + 8 <= a.F`
CMN_ROWS = 4            # frontend.hip:349 rows of the prefix scan per workgroup (`blockIdx.x * 4 + (threadIdx.x >> 6)`)
CMN_THREADS = 256       # frontend.hip:376 outputs of cmn_select_kernel per workgroup; nj = ceil(Tout / 256) at :613
AUG_P = 1024            # augment.hip:37   samples per block and taps per partition of the overlap-save convolution
AUG_CHUNK = 4096        # augment.hip:41   samples per partial sum of squares
RS_NT = 8               # resample.hip:28  tiles one resampler workgroup takes at the most

RATIOS = {}             # group -> largest error / bound seen by the GPU tests (printed when the module finishes)


def note(group, ratio):
    RATIOS[group] = max(RATIOS.get(group, 0.0), float(ratio))


def lib():
    from pytorch_kaldi_resnet_amd import hip
    return hip.lib()


def whole(rng, n, amp):
    """n whole-numbered samples at int16 scale"""
    return np.clip(np.round(rng.normal(0.0, amp, n)), -32768, 32767).astype(np.float64)


# ---- A. framing: spk_fbank_fwd, spk_mfcc_fwd ----
# (kind, options besides snip_edges and dither).  A1: the recipe's shape, FT = 32.  A2: FT = 16 and two lane rounds in the cepstral
# epilogue (C = 72 > 64).  A3: L = 40, S = 20, P = 64 - an FFT of 32 points, fewer than a wave.  A4: F % 8 = 1, C = F = 65, one
# cepstrum past a wave.
FRAME_CONFIGS = {
    "A1": ("fbank", dict(sample_frequency=16000.0, num_mel_bins=40)),
    "A2": ("mfcc", dict(sample_frequency=16000.0, num_mel_bins=80, num_ceps=72)),
    "A3": ("fbank", dict(sample_frequency=8000.0, frame_length=5.0, frame_shift=2.5, num_mel_bins=8)),
    "A4": ("mfcc", dict(sample_frequency=16000.0, num_mel_bins=65, num_ceps=65, htk_compat=True, use_energy=False)),
}
FRAME_SEEDS = {"A1": 101, "A2": 102, "A3": 103, "A4": 104}
FRAME_UTT = 4242        # the utterance id every row of the dither-on launches carries


def frame_sizes(name):
    """(L, S, P) of a configuration"""
    kw = dict(R.DEFAULTS, **FRAME_CONFIGS[name][1])
    return R.frame_params(kw["sample_frequency"], kw["frame_length"], kw["frame_shift"])


def frame_tile(name):
    """FT: frames per workgroup, as the library reports it for the configuration"""
    kind, kw = FRAME_CONFIGS[name]
    L, S, P = frame_sizes(name)
    if kind == "mfcc":
        return int(lib().spk_mfcc_tile_frames(L, S, P, kw["num_mel_bins"], kw["num_ceps"]))
    return int(lib().spk_fbank_tile_frames(L, S, P, kw["num_mel_bins"]))


def length_range(T, L, S, snip_edges):
    """(shortest, longest) sample count of an utterance of at least L samples with T frames, or None when there is none"""
    if snip_edges:
        lo, hi = L + (T - 1) * S, L + (T - 1) * S + S - 1
    else:
        lo, hi = T * S - S // 2, T * S - S // 2 + S - 1
    lo = max(lo, L)
    return (lo, hi) if lo <= hi else None


def frame_counts(FT, L, S, snip_edges):
    """the frame counts of a ragged batch: around the wave rounds (1 .. 5), around one tile and two"""
    want = sorted({1, 2, 3, 4, 5, FT - 1, FT, FT + 1, 2 * FT, 2 * FT + 1})
    return [T for T in want if T >= 1 and length_range(T, L, S, snip_edges) is not None]


def frame_rows(name, snip_edges):
    """[(T, N)] of the batch of a configuration, in ascending N.  snip_edges: every T at its shortest length, T = 1 and T = FT at
    their longest as well; otherwise every T at its shortest and at its longest length"""
    FT = frame_tile(name)
    L, S, _ = frame_sizes(name)
    rows = []
    for T in frame_counts(FT, L, S, snip_edges):
        lo, hi = length_range(T, L, S, snip_edges)
        rows.append((T, lo))
        if (not snip_edges or T in (1, FT)) and hi != lo:
            rows.append((T, hi))
    return sorted(rows, key=lambda r: r[1])


@functools.lru_cache(maxsize=None)
def frame_signal(name):
    """the one signal whose prefixes are the rows of a configuration (long enough for either snip_edges)"""
    n = max(N for snip in (True, False) for _, N in frame_rows(name, snip))
    return whole(np.random.default_rng(FRAME_SEEDS[name]), n, 3000.0)


def frame_options(name, snip_edges, dither):
    """(kind, keyword options) as FbankOptions / MfccOptions and the oracles take them"""
    kind, kw = FRAME_CONFIGS[name]
    return kind, dict(kw, snip_edges=snip_edges, dither=dither)


def frame_oracle(name, snip_edges, x, dtype=np.float64):
    """(features [T, R], raw log energy [T]) of one row, dither off"""
    kind, kw = frame_options(name, snip_edges, 0.0)
    return (M.mfcc if kind == "mfcc" else R.fbank)(x, dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def frame_oracles(name, snip_edges):
    """[(fp64 features, fp64 energies, float32 features)] per row of frame_rows - computed once, shared, never written to"""
    x = frame_signal(name)
    out = []
    for _, N in frame_rows(name, snip_edges):
        ref, eref = frame_oracle(name, snip_edges, x[:N])
        r32, _ = frame_oracle(name, snip_edges, x[:N], dtype=np.float32)
        for a in (ref, eref, r32):
            a.setflags(write=False)
        out.append((ref, eref, r32))
    return out


def pooled_yardstick(oracles):
    """(max, rms) error of the float32 restatement against fp64 over all rows of a launch"""
    d = np.concatenate([(r32.astype(np.float64) - ref).reshape(-1) for ref, _, r32 in oracles])
    return np.abs(d).max(), math.sqrt((d ** 2).mean())


def reflect(x, T, L, S):
    """the signal whose snip_edges=true frames are the snip_edges=false frames of x (T of them): L/2 - S/2 mirrored samples in
    front, mirrored samples behind up to L + (T - 1) S.  Returns (signal, samples appended)."""
    x = np.asarray(x)
    N = len(x)
    off = L // 2 - S // 2
    right = L + (T - 1) * S - off - N
    assert 0 <= off <= N and 0 <= right <= N, (N, T, off, right)
    return np.concatenate([x[:off][::-1], x, x[N - right:][::-1]]), right


# ---- B. VAD: spk_vad_count ----
VAD_T = (0, 1, 2, 3, 63, 64, 65, 128, 129)
VAD_TCAPS = (129, 192)
VAD_CONTEXTS = (0, 2, 70)
VAD_PROPORTIONS = (0.12, 0.6)
VAD_MARGIN = 1e-6       # every energy is at least this far from its row's threshold: the order of an fp64 sum cannot flip a decision


def vad_row(T, seed):
    """float32 log energies around the default threshold 5 + 0.5 mean: a loud start (two fifths of the frames, so that a clipped
    window of context 70 holds more than 0.6 of them at the start and none at the end), a quiet rest, and from 63 frames on a few
    swapped pairs - isolated frames of either kind.  At context 0 both decisions occur in every row of three frames or more; a
    context wider than a row gives every frame the same window, so there both occur in the rows of 128 and 129 frames"""
    rng = np.random.default_rng(seed)
    k = -(-2 * T // 5)
    e = np.concatenate([rng.normal(14.0, 1.2, k), rng.normal(7.0, 1.2, T - k)])
    if T >= 63:
        for i in rng.choice(T // 2, 6, replace=False):
            e[i], e[T - 1 - i] = e[T - 1 - i], e[i]
    return e.astype(np.float32)


def vad_rows():
    return [vad_row(T, 200 + i) for i, T in enumerate(VAD_T)]


def vad_threshold(e, energy_threshold=5.0, mean_scale=0.5):
    return energy_threshold + mean_scale * float(np.asarray(e, dtype=np.float64).sum()) / len(e)


def vad_expected(e, **kw):
    """(decisions [T] int32, voiced frame indices) from the oracle"""
    v = R.vad(e, **kw)
    return v, np.nonzero(v)[0].astype(np.int32)


VAD_TIE_T = (64, 65, 129)
VAD_TIE_ENERGY = np.float32(9.7)
VAD_TIE_OPTIONS = dict(vad_energy_threshold=0.0, vad_energy_mean_scale=1.0)


def vad_all_voiced_rows():
    """T = 129 and T = 128, every frame far above 5 + 0.5 mean: idx is 0 .. T - 1, the carry runs across three ballots"""
    return [np.random.default_rng(230 + i).normal(20.0, 1.0, T).astype(np.float32) for i, T in enumerate((129, 128))]


# ---- C. sliding CMN and selection: spk_cmn_select ----
CMN_B, CMN_F = 3, 5     # 15 rows: the last prefix workgroup has one idle wave
CMN_BATCHES = ((1, 64, 300), (2, 63, 65))
CMN_SELECT_WINDOWS = (3, 600)


def cmn_windows(Ts):
    return sorted({w for w in [1, 2, 3, 64, 65, 600] + [T + d for T in Ts for d in (-1, 0, 1)] if w >= 1})


def cmn_input(Ts, seed):
    """[B, F, Tcap] float32, log-mel-like, garbage past each row's count"""
    rng = np.random.default_rng(seed)
    x = rng.normal(8.0, 3.0, (CMN_B, CMN_F, max(Ts))).astype(np.float32)
    for b, T in enumerate(Ts):
        x[b, :, T:] = 1.0e30
    return x


def cmn_expected(x, T, W):
    """e = float32(x - mean64) [F, T] of one row x [F, Tcap], the window from the oracle's cmn_window, the mean in fp64"""
    x64 = x[:, :T].astype(np.float64)
    out = np.empty((x.shape[0], T), dtype=np.float32)
    for t in range(T):
        s, e = R.cmn_window(t, T, W)
        out[:, t] = (x64[:, t] - x64[:, s:e].mean(1)).astype(np.float32)
    return out


def select_patterns(Ts):
    """name -> per-row voiced frame lists"""
    return {
        "none": [np.zeros(0, dtype=np.int32) for T in Ts],
        "all": [np.arange(T, dtype=np.int32) for T in Ts],
        "every_other": [np.arange(0, T, 2, dtype=np.int32) for T in Ts],
        "last": [np.array([T - 1], dtype=np.int32) for T in Ts],
    }


# ---- D. reverberation and noise: spk_augment_fwd ----
FS = 16000
CONV_ROWS = ((1, 5), (100, 5), (1023, 2), (1024, 1), (1024, 1025), (1025, 1024), (2047, 2), (2048, 2049), (4096, 1),
             (4097, 1500), (1, 1025), (700, 2049))          # (N, R); M = N + R - 1
CONV_RIR_SEED = 31
PEAK = 48               # the peak of A.impulse_response(0.2, seed) at 16 kHz: int(3 ms * fs)


@functools.lru_cache(maxsize=None)
def base_rir():
    h = A.impulse_response(0.2, CONV_RIR_SEED)
    h.setflags(write=False)
    return h


def conv_rows():
    """[(speech, impulse response, noises)]: CONV_ROWS with the first R samples of one response, then a response whose peak is its
    last sample and one whose peak is its first"""
    h = base_rir()
    rows = [(A.speech(N, 300 + i), np.ascontiguousarray(h[:Rn]), []) for i, (N, Rn) in enumerate(CONV_ROWS)]
    rows.append((A.speech(1500, 320), np.ascontiguousarray(h[:PEAK + 1]), []))
    rows.append((A.speech(2000, 321), np.ascontiguousarray(h[PEAK:PEAK + 1000]), []))
    return rows


EARLY_SIZES = (1024, 1025, 2448, 4096)
EARLY_SPEECH = {1024: 3000, 1025: 3500, 2448: 4096, 4096: 5000}


def early_size(fs, seconds=0.2, peak_ms=3.0):
    """E of A.impulse_response(seconds, seed, fs=fs) at fs Hz, from the formulas of early_window"""
    n, s = int(seconds * fs), int(peak_ms * 0.001 * fs)
    return min(n, s + int(0.05 * fs)) - max(0, s - int(0.001 * fs))


@functools.lru_cache(maxsize=None)
def early_rate(E):
    """the lowest whole rate at which a 0.2 s response has an early part of E samples"""
    for fs in range(8000, 200000):
        if early_size(fs) == E:
            return fs
    raise ValueError(E)


def early_rows():
    """[(sample rate, speech, impulse response, noises)] per early-part size: the noise is what makes the output depend on the
    power of the early part (its scale is sqrt(10^(-snr / 10) p_sig / q))"""
    rows = []
    for i, E in enumerate(EARLY_SIZES):
        fs = early_rate(E)
        n = EARLY_SPEECH[E]
        rows.append((fs, A.speech(n, 340 + i), A.impulse_response(0.2, 350 + i, fs=fs), [(A.noise(1500, 360 + i), None, 0.01, 3.0)]))
    return rows


def seconds(samples, fs=FS):
    """a time whose int(fs * t) is `samples` whatever the rounding of the product"""
    return (samples + 0.5) / fs


def noise_rows():
    """[(speech, impulse response or None, noises, what)] - the descriptor edges, on rows with and without a response"""
    h = base_rir()
    shared = A.noise(512, 380)
    return [
        (A.speech(4096, 370), None, [(np.array([700.0], dtype=np.float32), None, seconds(10), 10.0),
                                     (A.noise(1000, 381), seconds(4096), 0.0, 8.0)],
         "raw length 1; fill 4096 = M exactly (and no multiple of the raw length)"),
        (A.speech(3000, 371), None, [(A.noise(500, 382), None, seconds(2999), 0.0), (A.noise(400, 383), None, seconds(3000), 0.0),
                                     (A.noise(2000, 384), None, seconds(2000), 6.0)],
         "start at M - 1: one sample lands; start = M: none lands; start + fill past M: cut"),
        (A.speech(3072, 372), np.ascontiguousarray(h[:1025]), [(A.noise(1500, 385), seconds(4097), 0.0, 9.0),
                                                               (A.noise(5000, 386), seconds(1234), seconds(100), 12.0)],
         "M = 4096; fill 4097, cut by one; fill shorter than the raw noise"),
        (A.speech(2044, 373), np.ascontiguousarray(h[:5]), [(shared, seconds(2048), 0.0, 7.0)],
         "M = 2048 = fill = 4 x raw, the array shared with the next row"),
        (A.speech(1100, 374), None, [(shared, None, seconds(300), 4.0)], "the shared array as it is"),
        (A.speech(2000, 375), np.ascontiguousarray(h[:100]), [(A.noise(300, 387), None, seconds(2098), 5.0),
                                                              (A.noise(300, 388), None, seconds(2099), 5.0)],
         "with a response, M = 2099: start at M - 1 and at M"),
    ]


def aug_yardstick(x, h, noises, fs=FS):
    """(fp64 oracle, float32 restatement) of one row"""
    return A.augment(x, h, noises, fs=fs), A.augment32(x, h, noises, fs=fs)


# ---- E. resampler: spk_resample_fwd ----
RESAMPLE_PAIRS = ((44100, 16000), (8000, 16000))


def resample_tile(fi, fo):
    iu, ou, K, _, _ = RS.tables(fi, fo)
    return int(lib().spk_resample_tile(iu, ou, K))


def resample_lengths(fi, fo):
    """[(input length, output count)] for output counts TO - 1, TO, TO + 1, 8 TO, 8 TO + 1 (8 = RS_NT).  A count that no input
    length gives (2 n is never odd) is replaced by the nearest count on the same side of the tile edge that one does give."""
    TO = resample_tile(fi, fo)
    out = []
    for want, step in ((TO - 1, -1), (TO, 0), (TO + 1, 1), (RS_NT * TO, 0), (RS_NT * TO + 1, 1)):
        while True:
            n = want * fi // fo
            hit = [m for m in range(max(n - 2, 1), n + 3) if RS.num_resampled(m, fi, fo) == want]
            if hit:
                out.append((hit[0], want))
                break
            assert step != 0, (fi, fo, want)
            want += step
    return out


def resample_signal(fi, fo):
    n = max(n for n, _ in resample_lengths(fi, fo))
    return np.random.default_rng(fi + fo).integers(-20000, 20001, n).astype(np.float64)


# ---- oracles computed once and shared (read-only) ----
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def conv_oracles():
    return [_frozen(*aug_yardstick(x, h, nz)) for x, h, nz in conv_rows()]


@functools.lru_cache(maxsize=None)
def noise_oracles():
    return [_frozen(*aug_yardstick(x, h, nz)) for x, h, nz, _ in noise_rows()]


@functools.lru_cache(maxsize=None)
def early_oracles():
    return [_frozen(*aug_yardstick(x, h, nz, fs)) for fs, x, h, nz in early_rows()]


@functools.lru_cache(maxsize=None)
def resample_oracles(fi, fo):
    x = resample_signal(fi, fo)
    return [_frozen(RS.resample(x[:n], fi, fo), RS.resample(x[:n], fi, fo, dtype=np.float32)) for n, _ in resample_lengths(fi, fo)]


def errors(got, ref):
    """(max, rms) of got - ref"""
    d = np.asarray(got, dtype=np.float64) - ref
    return np.abs(d).max(), math.sqrt((d ** 2).mean())


def short_pool(rows, oracles, outputs):
    """the rows with N < AUG_P judged together: (max, rms) over the pool of (outputs - fp64) / peak |fp64| per row.
    outputs: per row the values to judge (the float32 restatement for the yardstick, the kernel's for the test)"""
    d = [(np.asarray(o, dtype=np.float64) - ref) / np.abs(ref).max()
         for (x, *_), (ref, _), o in zip(rows, oracles, outputs) if len(x) < AUG_P]
    d = np.concatenate(d)
    return np.abs(d).max(), math.sqrt((d ** 2).mean()), d.size
