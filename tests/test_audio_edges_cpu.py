"""The premises of the audio edge cases (tests/audio_edges_ref.py), proved without a GPU: every size said to lie on a tile, wave,
partition or chunk boundary lies on it for the tile sizes the library reports; the identities the GPU tests hold the kernels to
hold in the fp64 oracles; every float32 yardstick that a bound is doubled from is non-zero; and the oracles of all cases together
take a few seconds."""
import time

import numpy as np
import pytest

import audio_edges_ref as E
import augment_ref as A
import frontend_ref as R
import resample_ref as RS
import pytorch_kaldi_resnet_amd  # noqa: F401
from pytorch_kaldi_resnet_amd import features

CONFIGS = sorted(E.FRAME_CONFIGS)


def test_frame_tiles_and_configurations():
    assert {n: E.frame_tile(n) for n in CONFIGS} == {"A1": 32, "A2": 16, "A3": 32, "A4": 32}
    assert E.frame_sizes("A1") == (400, 160, 512) and E.frame_sizes("A3") == (40, 20, 64)
    assert E.frame_sizes("A3")[2] // 2 < E.WAVE                        # an FFT of 32 points: half a wave idles in every stage
    a2, a4 = E.FRAME_CONFIGS["A2"][1], E.FRAME_CONFIGS["A4"][1]
    assert E.WAVE < a2["num_ceps"] <= 2 * E.WAVE                       # the lane loop over C runs twice
    assert a4["num_mel_bins"] % E.DCT_UNROLL == 1 and a4["num_ceps"] == E.WAVE + 1 == a4["num_mel_bins"]
    L, S, P = E.frame_sizes("A3")
    kw = dict(R.DEFAULTS, **E.FRAME_CONFIGS["A3"][1])
    banks = R.mel_weights(kw["num_mel_bins"], P, kw["sample_frequency"], kw["low_freq"], kw["high_freq"])
    assert (banks.max(1) > 0).all()                                    # no empty filter: no log(FLT_EPSILON) plateau in the oracle
    for n in CONFIGS:                                                  # the options are ones the front end takes
        kind, kw = E.frame_options(n, False, 1.0)
        opts = (features.MfccOptions if kind == "mfcc" else features.FbankOptions)(**kw)
        assert (opts.frame_len, opts.frame_sh, opts.padded_len) == E.frame_sizes(n)


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("name", CONFIGS)
def test_frame_rows_sit_on_the_tile_edges(name, snip):
    FT = E.frame_tile(name)
    L, S, _ = E.frame_sizes(name)
    rows = E.frame_rows(name, snip)
    counts = {T for T, _ in rows}
    assert {FT - 1, FT, FT + 1, 2 * FT, 2 * FT + 1, 3, 4, 5} <= counts
    assert min(counts) == (1 if snip else (3 if name != "A3" else 2))  # what an utterance of at least L samples can have
    assert max(counts) == 2 * FT + 1 and (2 * FT + 1) % FT == 1        # Tcap = longest T: the last tile holds one frame
    assert 3 * FT >= max(counts) and (3 * FT) % FT == 0
    assert min(N for _, N in rows) == L                                # a row at the minimum length
    x = E.frame_signal(name)
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 32768 and max(N for _, N in rows) <= len(x) <= 10700
    for T, N in rows:
        assert N >= L and R.num_frames(N, L, S, snip) == T
        lo, hi = E.length_range(T, L, S, snip)
        assert N in (lo, hi)
        assert lo == L or R.num_frames(lo - 1, L, S, snip) == T - 1    # the shortest and the longest length with T frames
        assert R.num_frames(hi + 1, L, S, snip) == T + 1
    if snip:
        assert sorted({T for T, _ in rows if sum(t == T for t, _ in rows) == 2}) == [1, FT]
    else:
        assert all(sum(t == T for t, _ in rows) == 2 for T in counts)


@pytest.mark.parametrize("name", CONFIGS)
def test_reflection_identity_holds_in_the_oracle(name):
    """the frames of snip_edges=false are the frames of snip_edges=true of the reflected signal, first and last frame included"""
    L, S, _ = E.frame_sizes(name)
    x = E.frame_signal(name)
    for T, N in E.frame_rows(name, False):
        xr, right = E.reflect(x[:N], T, L, S)
        assert 0 <= right <= N and len(xr) == L + (T - 1) * S and R.num_frames(len(xr), L, S, True) == T
        assert np.array_equal(R.frames(x[:N], L, S, False), R.frames(xr, L, S, True))


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("name", CONFIGS)
def test_frame_yardsticks_are_non_zero(name, snip):
    e_max, e_rms = E.pooled_yardstick(E.frame_oracles(name, snip))
    assert e_max > 0 and e_rms > 0
    assert sum(ref.size for ref, _, _ in E.frame_oracles(name, snip)) > 1000         # thousands of values under each maximum
    for (T, _), (ref, eref, _) in zip(E.frame_rows(name, snip), E.frame_oracles(name, snip)):
        assert ref.shape[0] == T == eref.shape[0]


def test_vad_rows():
    rows = E.vad_rows()
    assert [len(e) for e in rows] == list(E.VAD_T) and max(E.VAD_T) == E.VAD_TCAPS[0] < E.VAD_TCAPS[1]
    assert {E.WAVE - 1, E.WAVE, E.WAVE + 1, 2 * E.WAVE, 2 * E.WAVE + 1, 0} <= set(E.VAD_T)
    assert max(E.VAD_CONTEXTS) > E.WAVE and sum(T <= max(E.VAD_CONTEXTS) for T in E.VAD_T) > len(E.VAD_T) // 2
    assert R.vad(rows[0]).shape == (0,)                                 # T = 0: no decisions
    for e in rows[1:]:
        thr = E.vad_threshold(e)
        assert np.abs(e.astype(np.float64) - thr).min() > E.VAD_MARGIN
        if len(e) >= 3:                                                 # context 0: a decision is the frame's own comparison
            v = R.vad(e, vad_frames_context=0)
            assert 0 < v.sum() < len(e)
    for ctx in E.VAD_CONTEXTS:                                          # wider contexts: both decisions in the rows of two waves
        for prop in E.VAD_PROPORTIONS:
            for e in rows[-2:]:
                v = R.vad(e, vad_frames_context=ctx, vad_proportion_threshold=prop)
                assert 0 < v.sum() < len(e), (ctx, prop, len(e))
    # a clipped window: context 70 clips every window of the rows up to 129 frames at one end at least, most at both
    assert all(t - 70 < 0 or t + 70 > T - 1 for T in E.VAD_T for t in range(T))


def test_vad_tie_and_all_voiced_rows():
    for T in E.VAD_TIE_T:
        e = np.full(T, E.VAD_TIE_ENERGY, dtype=np.float32)
        thr = E.vad_threshold(e, 0.0, 1.0)
        assert thr == float(E.VAD_TIE_ENERGY)                           # exact: T e is an fp64 number, and so is (T e) / T
        for ctx in E.VAD_CONTEXTS:
            assert not R.vad(e, vad_frames_context=ctx, **E.VAD_TIE_OPTIONS).any()      # the comparison is strict
    assert E.WAVE in E.VAD_TIE_T
    for e in E.vad_all_voiced_rows():
        for ctx in E.VAD_CONTEXTS:
            for prop in E.VAD_PROPORTIONS:
                assert R.vad(e, vad_frames_context=ctx, vad_proportion_threshold=prop).all()
        assert np.abs(e.astype(np.float64) - E.vad_threshold(e)).min() > E.VAD_MARGIN
    assert len(E.vad_all_voiced_rows()[0]) == 2 * E.WAVE + 1            # three ballots


def test_cmn_cases():
    assert (E.CMN_B * E.CMN_F) % E.CMN_ROWS == 3                        # the last prefix workgroup: three rows, one idle wave
    seen = set()
    for i, Ts in enumerate(E.CMN_BATCHES):
        seen |= set(Ts)
        ws = E.cmn_windows(Ts)
        assert {1, 2, 3, 64, 65, 600} <= set(ws) and min(ws) == 1
        assert all(w in ws for T in Ts for w in (T - 1, T, T + 1) if w >= 1)
        x = E.cmn_input(Ts, 400 + i)
        assert x.shape == (E.CMN_B, E.CMN_F, max(Ts)) and x.dtype == np.float32
        for b, T in enumerate(Ts):
            v = np.abs(x[b, :, :T].astype(np.float64))
            # every fp64 prefix sum of the row is exact (no value below 2^-16, no sum near 2^13: under 53 bits), so a window of one
            # frame has the frame itself as its mean and W = 1 gives exactly 0
            assert v.min() >= 2.0 ** -16 and v.sum(1).max() < 2.0 ** 13
            assert (E.cmn_expected(x[b], T, 1) == 0).all()
            assert np.array_equal(E.cmn_expected(x[b], T, 600), (x[b, :, :T] - x[b, :, :T].astype(np.float64).mean(1, keepdims=True))
                                  .astype(np.float32))
            ref = R.sliding_cmn(x[b, :, :T].T.astype(np.float64), 3).T
            assert np.array_equal(E.cmn_expected(x[b], T, 3), ref.astype(np.float32))
    assert {1, 2, E.WAVE - 1, E.WAVE, E.WAVE + 1, 300} == seen
    pats = E.select_patterns(E.CMN_BATCHES[0])
    assert max(len(v) for v in pats["none"]) == 0 and max(len(v) for v in pats["all"]) == 300
    assert -(-300 // E.CMN_THREADS) == 2                                # nj = 2
    assert [v.tolist() for v in pats["last"]] == [[0], [63], [299]]
    assert pats["every_other"][2][-1] == 298 and len(pats["every_other"][0]) == 1


def test_convolution_rows_sit_on_the_partition_edges():
    P, C = E.AUG_P, E.AUG_CHUNK
    M = [N + Rn - 1 for N, Rn in E.CONV_ROWS]
    assert M == [5, 104, 1024, 1024, 2048, 2048, 2048, 4096, 4096, 5596, 1025, 2748]
    assert sum(m % P == 0 for m in M) == 7 and sum(m % C == 0 for m in M) == 2 and 1025 in M
    assert {1, P, P + 1} <= {Rn for _, Rn in E.CONV_ROWS} and {1, P - 1, P, P + 1, 2 * P, C, C + 1} <= {N for N, _ in E.CONV_ROWS}
    h = E.base_rir()
    assert int(np.argmax(h)) == E.PEAK and len(h) == 3200
    rows = E.conv_rows()
    assert [(len(x), len(hh)) for x, hh, _ in rows[:len(E.CONV_ROWS)]] == list(E.CONV_ROWS)
    for x, hh, _ in rows:
        assert np.array_equal(x, np.round(x)) and A.early_window(hh, E.FS)[2] - A.early_window(hh, E.FS)[1] <= P      # nep = 1 here
    s, _, _ = A.early_window(rows[-2][1], E.FS)
    assert s == len(rows[-2][1]) - 1                                    # the peak is the last sample
    assert A.early_window(rows[-1][1], E.FS)[0] == 0                    # the peak is the first
    assert len(rows[-2][0]) >= P and len(rows[-1][0]) >= P


def test_early_parts_span_one_to_four_partitions():
    lib = E.lib()
    assert lib.spk_augment_max_early() == 4 * E.AUG_P == max(E.EARLY_SIZES)
    assert E.early_rate(2448) == 48000 and E.early_rate(4096) == 80320
    got = []
    for (fs, x, h, nz), size in zip(E.early_rows(), E.EARLY_SIZES):
        s, e0, e1 = A.early_window(h, fs)
        assert (s, e0, e1) == features.early_window(h, fs) and e1 - e0 == size
        assert 3000 <= len(x) <= 5000 and len(nz) == 1
        got.append(-(-size // E.AUG_P))
    assert got == [1, 2, 3, 4]
    fs = E.early_rate(4097)
    h = A.impulse_response(0.2, 1, fs=fs)
    s, e0, e1 = features.early_window(h, fs)
    assert e1 - e0 == lib.spk_augment_max_early() + 1


def test_noise_descriptors_sit_on_their_edges():
    rows = E.noise_rows()
    fills = []
    for x, h, nz, what in rows:
        Mrow = len(x) + (len(h) - 1 if h is not None else 0)
        for r, dur, start, snr in nz:
            fills.append((len(r), len(A.fill(r, dur, E.FS)), int(start * E.FS), Mrow))
    assert fills == [(1, 1, 10, 4096), (1000, 4096, 0, 4096), (500, 500, 2999, 3000), (400, 400, 3000, 3000), (2000, 2000, 2000, 3000),
                     (1500, 4097, 0, 4096), (5000, 1234, 100, 4096), (512, 2048, 0, 2048), (512, 512, 300, 1100),
                     (300, 300, 2098, 2099), (300, 300, 2099, 2099)]
    assert E.seconds(4096) * E.FS != 4096                               # the durations are not on a rounding edge of int(fs * t)
    assert rows[3][2][0][0] is rows[4][2][0][0]                         # one array, two descriptors on different rows
    assert {r[1] is None for r in rows} == {True, False}
    assert all(len(r[0]) >= E.AUG_P for r in rows)                      # every row is judged by the per-row rule
    assert {4096, 4097} <= {f[1] for f in fills} and 4096 == E.AUG_CHUNK


def test_augment_yardsticks_are_non_zero():
    for rows, oracles in ((E.conv_rows(), E.conv_oracles()), (E.noise_rows(), E.noise_oracles()),
                          ([r[1:] for r in E.early_rows()], E.early_oracles())):
        for row, (ref, r32) in zip(rows, oracles):
            assert len(ref) == len(row[0]) == len(r32)
            if len(row[0]) >= E.AUG_P:
                e_max, e_rms = E.errors(r32, ref)
                assert e_max > 0 and e_rms > 0
    rows, oracles = E.conv_rows(), E.conv_oracles()
    p_max, p_rms, n = E.short_pool(rows, oracles, [r32 for _, r32 in oracles])
    assert p_max > 0 and p_rms > 0 and n == 1 + 100 + 1023 + 1 + 700
    for (x, *_), (ref, r32) in zip(rows, oracles):                      # per row, in units of the row's scale
        if len(x) < E.AUG_P:
            assert 1e-8 < E.errors(r32, ref)[0] / np.abs(ref).max() < 1e-6


@pytest.mark.parametrize("fi,fo", E.RESAMPLE_PAIRS)
def test_resampler_lengths_give_the_counts_claimed(fi, fo):
    TO = E.resample_tile(fi, fo)
    assert TO == 1024
    lens = E.resample_lengths(fi, fo)
    counts = [c for _, c in lens]
    for n, c in lens:
        assert RS.num_resampled(n, fi, fo) == c == features.num_resampled(n, fi, fo) and c >= 255
        assert n == 1 or RS.num_resampled(n - 1, fi, fo) < c            # the shortest input with that count
    if fo % fi:
        assert counts == [TO - 1, TO, TO + 1, E.RS_NT * TO, E.RS_NT * TO + 1]
    else:       # 2 n is never odd: the nearest counts on the same side of the tile edge
        assert counts == [TO - 2, TO, TO + 2, E.RS_NT * TO, E.RS_NT * TO + 2]
    x = E.resample_signal(fi, fo)
    assert np.array_equal(x, np.round(x)) and len(x) == max(n for n, _ in lens) <= 23000
    for (n, c), (ref, r32) in zip(lens, E.resample_oracles(fi, fo)):
        assert len(ref) == c
        e_max, e_rms = E.errors(r32, ref)
        assert e_max > 0 and e_rms > 0


def test_oracles_take_a_few_seconds():
    """every fp64 oracle and float32 restatement of the GPU module, computed afresh"""
    for f in (E.frame_oracles, E.conv_oracles, E.noise_oracles, E.early_oracles, E.resample_oracles, E.frame_signal):
        f.cache_clear()
    t = time.perf_counter()
    for n in CONFIGS:
        for snip in (True, False):
            E.frame_oracles(n, snip)
    E.conv_oracles(), E.noise_oracles(), E.early_oracles()
    for fi, fo in E.RESAMPLE_PAIRS:
        E.resample_oracles(fi, fo)
    for i, Ts in enumerate(E.CMN_BATCHES):
        x = E.cmn_input(Ts, 400 + i)
        for W in E.cmn_windows(Ts):
            for b, T in enumerate(Ts):
                E.cmn_expected(x[b], T, W)
    dt = time.perf_counter() - t
    print("oracles of the audio edge cases: %.1f s" % dt)
    assert dt < 30.0
