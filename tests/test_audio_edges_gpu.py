"""The audio kernels on a real MI355X at their tile and block edges: csrc/frontend.hip (spk_fbank_fwd, spk_mfcc_fwd, spk_vad_count,
spk_cmn_select), csrc/augment.hip (spk_augment_fwd) and csrc/resample.hip (spk_resample_fwd) through
pytorch_kaldi_resnet_amd.features, on the case lists of tests/audio_edges_ref.py (whose premises tests/test_audio_edges_cpu.py proves).

Identities, held bit for bit: frame counts, zero tails, Tcap invariance, the prefix identity (a frame depends on its own samples
and its index only), the reflection identity (snip_edges=false is snip_edges=true on the mirrored signal), VAD decisions / lists /
counts against the oracle, W = 1 of the sliding CMN, voiced-frame selection against host column selection, row invariance of the
augmentation, quantisation as trunc-and-clip of the unquantised output, output counts of the resampler.
Bounds: the project's rule - at most twice the error of the oracle's own float32 restatement against fp64, maximum and rms - for
the features (pooled over the rows of a launch, with the floors of test_frontend_gpu.py), the augmentation (per row from 1024
samples on, shorter rows pooled in units of each row's peak) and the resampler (per row); one float32 ulp for the sliding CMN.
The largest error / bound per group is printed when the module finishes: python -m pytest tests/test_audio_edges_gpu.py -m gpu -q -s"""
import numpy as np
import pytest
import torch

import audio_edges_ref as E
import augment_ref as A
import frontend_ref as R

pytestmark = pytest.mark.gpu

CONFIGS = sorted(E.FRAME_CONFIGS)
NAN = float("nan")


@pytest.fixture(scope="module")
def features():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features as _features
    yield _features
    print("\nlargest error / bound per group: " + ", ".join("%s %.3g" % kv for kv in sorted(E.RATIOS.items())))


def _batch(waves, nmax=None, fill=0.0):
    """rows of a [B, nmax] float32 batch; everything that is not signal holds `fill`"""
    nmax = nmax or max(len(w) for w in waves)
    buf = np.full((len(waves), nmax), fill, dtype=np.float32)
    for r, w in enumerate(waves):
        buf[r, :len(w)] = w
    return torch.from_numpy(buf).cuda(), np.asarray([len(w) for w in waves], dtype=np.int64)


# ---- A. framing ----
def _frames(features, name, snip, dither, waves, Tcap=None):
    """(feats [B, R, Tcap], T, log energy [B, Tcap]) on the host; the padding of the batch holds garbage"""
    kind, kw = E.frame_options(name, snip, dither)
    opts = (features.MfccOptions if kind == "mfcc" else features.FbankOptions)(**kw)
    w, n = _batch(waves, nmax=max(len(v) for v in waves) + 37, fill=12345.0)
    ids = [E.FRAME_UTT] * len(waves) if dither else None
    f, T, e = (features.mfcc if kind == "mfcc" else features.fbank)(w, n, opts, utt_ids=ids, seed=7, Tcap=Tcap)
    return f.cpu().numpy(), T, e.cpu().numpy()


@pytest.mark.parametrize("snip", [True, False], ids=["snip", "nosnip"])
@pytest.mark.parametrize("name", CONFIGS)
def test_frame_counts_padding_tcap_and_oracle(features, name, snip):
    FT = E.frame_tile(name)
    rows = E.frame_rows(name, snip)
    x = E.frame_signal(name)
    waves = [x[:N] for _, N in rows]
    oracles = E.frame_oracles(name, snip)
    Tmax = max(T for T, _ in rows)
    f1, T1, e1 = _frames(features, name, snip, 0.0, waves, Tcap=Tmax)           # the last tile holds one frame
    f2, T2, e2 = _frames(features, name, snip, 0.0, waves, Tcap=3 * FT)         # an exact tile multiple
    assert f1.shape[2] == Tmax == 2 * FT + 1 and f2.shape[2] == 3 * FT
    d = []
    for b, ((T, N), (ref, eref, _)) in enumerate(zip(rows, oracles)):
        assert T1[b] == T2[b] == T == ref.shape[0], (b, N)
        for f, e in ((f1, e1), (f2, e2)):
            assert (f[b, :, T:] == 0).all() and (e[b, T:] == 0).all(), (b, N)    # exactly 0 past T, in every Tcap form
        assert np.array_equal(f1[b, :, :T], f2[b, :, :T]) and np.array_equal(e1[b, :T], e2[b, :T]), (b, N)
        d.append((f1[b, :, :T].T.astype(np.float64) - ref).reshape(-1))
        assert np.abs(e1[b, :T] - eref).max() <= 1e-5 * np.abs(eref).max(), (b, N)
    assert np.isfinite(f1).all() and np.isfinite(f2).all()
    d = np.concatenate(d)
    e32_max, e32_rms = E.pooled_yardstick(oracles)
    dmax, drms = np.abs(d).max(), np.sqrt((d ** 2).mean())
    bmax, brms = max(2 * e32_max, 2e-4), max(2 * e32_rms, 2e-5)                   # the rule of test_frontend_gpu.py, floors included
    print("%s snip_edges=%s: max %.3e / float32 %.3e = %.2f, rms %.3e / float32 %.3e = %.2f (%d values)"
          % (name, snip, dmax, e32_max, dmax / e32_max, drms, e32_rms, drms / e32_rms, d.size))
    E.note("framing " + name, max(dmax / bmax, drms / brms))
    assert dmax <= bmax, (name, snip, dmax, e32_max)
    assert drms <= brms, (name, snip, drms, e32_rms)


@pytest.mark.parametrize("name", CONFIGS)
def test_prefix_identity_with_dither(features, name):
    """snip_edges=true, dither 1.0, one utterance id: every row's columns are the first T columns of the longest row, bit for bit"""
    rows = E.frame_rows(name, True)
    x = E.frame_signal(name)
    waves = [x[:N] for _, N in rows]
    f, T, e = _frames(features, name, True, 1.0, waves)
    f0, _, _ = _frames(features, name, True, 0.0, waves)
    last = len(rows) - 1
    assert T[last] == max(T) and not np.array_equal(f, f0)                        # the dither is on
    for b, (Tb, N) in enumerate(rows):
        assert T[b] == Tb
        assert np.array_equal(f[b, :, :Tb], f[last, :, :Tb]), (b, N)
        assert np.array_equal(e[b, :Tb], e[last, :Tb]), (b, N)
        assert (f[b, :, Tb:] == 0).all() and (e[b, Tb:] == 0).all()


@pytest.mark.parametrize("name", CONFIGS)
def test_reflection_identity_with_dither(features, name):
    """snip_edges=false on x is snip_edges=true on x mirrored about both ends, bit for bit: the reflect-on-load code, first and
    last frame included"""
    L, S, _ = E.frame_sizes(name)
    rows = E.frame_rows(name, False)
    x = E.frame_signal(name)
    waves = [x[:N] for _, N in rows]
    f, T, e = _frames(features, name, False, 1.0, waves)
    g, Tg, eg = _frames(features, name, True, 1.0, [E.reflect(w, Tb, L, S)[0] for w, (Tb, _) in zip(waves, rows)])
    for b, (Tb, N) in enumerate(rows):
        assert T[b] == Tg[b] == Tb
        assert np.array_equal(f[b, :, :Tb], g[b, :, :Tb]), (b, N)
        assert np.array_equal(e[b, :Tb], eg[b, :Tb]), (b, N)


# ---- B. VAD ----
def _vad(features, rows, Tcap, fill, **kw):
    buf = np.full((len(rows), Tcap), fill, dtype=np.float32)
    for b, r in enumerate(rows):
        buf[b, :len(r)] = r
    v, idx, cnt = features.vad(torch.from_numpy(buf).cuda(), [len(r) for r in rows], features.VadOptions(**kw))
    return v.cpu().numpy(), idx.cpu().numpy(), cnt


def _check_vad(rows, got, Tcap, **kw):
    v, idx, cnt = got
    assert v.shape == (len(rows), Tcap) and cnt.shape == (len(rows),)
    for b, r in enumerate(rows):
        T = len(r)
        want, keep = E.vad_expected(r, **kw)
        assert np.array_equal(v[b, :T], want), (b, T, kw)
        assert (v[b, T:] == 0).all(), (b, T)
        assert cnt[b] == len(keep) and np.array_equal(idx[b, :cnt[b]], keep), (b, T, kw)


@pytest.mark.parametrize("prop", E.VAD_PROPORTIONS)
@pytest.mark.parametrize("ctx", E.VAD_CONTEXTS)
def test_vad_at_the_wave_edges(features, ctx, prop):
    rows = E.vad_rows()
    kw = dict(vad_frames_context=ctx, vad_proportion_threshold=prop)
    a = _vad(features, rows, E.VAD_TCAPS[0], 1.0e30, **kw)
    b = _vad(features, rows, E.VAD_TCAPS[1], NAN, **kw)           # NaN in every column at or past T
    _check_vad(rows, a, E.VAD_TCAPS[0], **kw)
    _check_vad(rows, b, E.VAD_TCAPS[1], **kw)
    assert a[2][0] == 0 and np.array_equal(a[2], b[2])              # the row without frames: count 0


def test_vad_tie_and_all_voiced_rows(features):
    for ctx in E.VAD_CONTEXTS:
        kw = dict(E.VAD_TIE_OPTIONS, vad_frames_context=ctx)
        rows = [np.full(T, E.VAD_TIE_ENERGY, dtype=np.float32) for T in E.VAD_TIE_T]
        got = _vad(features, rows, max(E.VAD_TIE_T), NAN, **kw)
        _check_vad(rows, got, max(E.VAD_TIE_T), **kw)
        assert not got[0].any() and not got[2].any()               # energy == threshold: the comparison is strict
        for prop in E.VAD_PROPORTIONS:
            kw = dict(vad_frames_context=ctx, vad_proportion_threshold=prop)
            rows = E.vad_all_voiced_rows()
            v, idx, cnt = got = _vad(features, rows, 129, NAN, **kw)
            _check_vad(rows, got, 129, **kw)
            assert cnt.tolist() == [129, 128] and np.array_equal(idx[0], np.arange(129))      # the carry across three ballots


# ---- C. sliding CMN and selection ----
@pytest.mark.parametrize("which", range(len(E.CMN_BATCHES)))
def test_sliding_cmn_within_one_ulp(features, which):
    Ts = E.CMN_BATCHES[which]
    x = E.cmn_input(Ts, 400 + which)
    xd = torch.from_numpy(x).cuda()
    worst = 0.0
    for W in E.cmn_windows(Ts):
        got = features.sliding_cmn(xd, list(Ts), features.CmnOptions(cmn_window=W)).cpu().numpy()
        assert got.shape == x.shape
        for b, T in enumerate(Ts):
            e = E.cmn_expected(x[b], T, W)
            err = np.abs(got[b, :, :T].astype(np.float64) - e.astype(np.float64))
            ulp = np.spacing(np.abs(e)).astype(np.float64)          # one float32 ulp: the fp64 means agree to ~T 2^-53
            worst = max(worst, (err / ulp).max())
            assert (err <= ulp).all(), (W, b, T, (err / ulp).max())
            assert (got[b, :, T:] == 0).all(), (W, b, T)
            if W == 1:
                assert (got[b, :, :T] == 0).all()                   # a window of one frame: x - x
    print("sliding CMN, T =", Ts, ": largest error %.3g ulp" % worst)
    E.note("sliding CMN (ulp)", worst)


@pytest.mark.parametrize("W", E.CMN_SELECT_WINDOWS)
def test_selection_is_host_column_selection(features, W):
    Ts = E.CMN_BATCHES[0]
    x = E.cmn_input(Ts, 400)
    xd = torch.from_numpy(x).cuda()
    cmn = features.CmnOptions(cmn_window=W)
    cm = features.sliding_cmn(xd, list(Ts), cmn).cpu().numpy()
    for name, keep in E.select_patterns(Ts).items():
        idx = np.zeros((len(Ts), max(Ts)), dtype=np.int32)          # past count: frame 0, which selection must not copy
        for b, k in enumerate(keep):
            idx[b, :len(k)] = k
        count = np.asarray([len(k) for k in keep], dtype=np.int64)
        sel, lengths = features.select_voiced(xd, list(Ts), torch.from_numpy(idx).cuda(), count, cmn)
        sel = sel.cpu().numpy()
        assert sel.shape == (len(Ts), x.shape[1], count.max()) and np.array_equal(lengths, count), name
        for b, k in enumerate(keep):
            assert np.array_equal(sel[b, :, :len(k)], cm[b][:, k]), (name, b)
            assert (sel[b, :, len(k):] == 0).all(), (name, b)


# ---- D. reverberation and noise ----
def _augment(features, rows, fs=E.FS, quantize=False, nmax=None):
    w, n = _batch([r[0] for r in rows], nmax=nmax, fill=NAN)
    out, clipped = features.augment(w, n, [r[1] for r in rows], [r[2] for r in rows], quantize=quantize, sample_rate=fs)
    return out.cpu().numpy(), clipped


def _check_rows(features, group, rows, oracles, fs=E.FS):
    """zeros, the oracle rule and row invariance of one batch; returns the batch's output"""
    out, clipped = _augment(features, rows, fs, nmax=max(len(r[0]) for r in rows) + 37)
    assert not clipped.any() and not np.isnan(out).any()
    for b, ((x, h, nz), (ref, r32)) in enumerate(zip(rows, oracles)):
        N = len(x)
        assert (out[b, N:] == 0).all(), (group, b)
        alone, _ = _augment(features, [rows[b]], fs)
        assert np.array_equal(alone[0], out[b, :N]), (group, b, N)            # the row alone: the same bits
        if N >= E.AUG_P:
            (dmax, drms), (e_max, e_rms) = E.errors(out[b, :N], ref), E.errors(r32, ref)
            print("%s row %d N %d R %d: max %.3e / float32 %.3e = %.2f, rms %.3e / float32 %.3e = %.2f" % (
                group, b, N, 0 if h is None else len(h), dmax, e_max, dmax / e_max, drms, e_rms, drms / e_rms))
            E.note(group, max(dmax / (2 * e_max), drms / (2 * e_rms)))
            assert dmax <= 2 * e_max, (group, b, dmax, e_max)
            assert drms <= 2 * e_rms, (group, b, drms, e_rms)
    return out


def test_convolution_at_the_partition_edges(features):
    rows, oracles = E.conv_rows(), E.conv_oracles()
    out = _check_rows(features, "augment convolution", rows, oracles)
    # the rows shorter than a partition, judged together in units of each row's peak
    e_max, e_rms, n = E.short_pool(rows, oracles, [r32 for _, r32 in oracles])
    dmax, drms, _ = E.short_pool(rows, oracles, [out[b, :len(r[0])] for b, r in enumerate(rows)])
    print("augment convolution, %d samples of rows under %d: max %.3e / float32 %.3e = %.2f, rms %.3e / float32 %.3e = %.2f"
          % (n, E.AUG_P, dmax, e_max, dmax / e_max, drms, e_rms, drms / e_rms))
    E.note("augment short rows", max(dmax / (2 * e_max), drms / (2 * e_rms)))
    assert dmax <= 2 * e_max and drms <= 2 * e_rms, (dmax, e_max, drms, e_rms)


def test_noise_descriptors_at_their_edges(features):
    _check_rows(features, "augment noise", [r[:3] for r in E.noise_rows()], E.noise_oracles())


def test_early_part_over_several_partitions(features):
    mate = (A.speech(2000, 390), None, [(A.noise(700, 391), None, 0.02, 6.0)])
    for (fs, x, h, nz), oracle, size in zip(E.early_rows(), E.early_oracles(), E.EARLY_SIZES):
        assert features.early_window(h, fs)[2] - features.early_window(h, fs)[1] == size
        rows = [mate, (x, h, nz)]
        _check_rows(features, "augment early part", rows, [E.aug_yardstick(*mate, fs=fs), oracle], fs)
    fs = E.early_rate(max(E.EARLY_SIZES) + 1)                       # one sample more than the kernel is built for: refused
    w, n = _batch([A.speech(3000, 392)])
    with pytest.raises(ValueError, match="early part .* has %d samples" % (max(E.EARLY_SIZES) + 1)):
        features.augment(w, n, [A.impulse_response(0.2, 393, fs=fs)], sample_rate=fs)


def test_quantisation_is_trunc_and_clip(features):
    conv = E.conv_rows()[E.CONV_ROWS.index((2048, 2049))]
    fs, x, h, nz = E.early_rows()[E.EARLY_SIZES.index(2448)]
    for rows, rate in (([conv], E.FS), ([(x, h, nz)], fs)):
        plain, c0 = _augment(features, rows, rate)
        quant, c1 = _augment(features, rows, rate, quantize=True)
        t = np.trunc(plain)
        assert np.array_equal(quant, np.clip(t, -32768, 32767)) and not np.array_equal(quant, plain)
        assert np.array_equal(c1, ((t > 32767) | (t < -32768)).sum(1)) and not c0.any()


# ---- E. resampler ----
@pytest.mark.parametrize("fi,fo", E.RESAMPLE_PAIRS)
def test_resampler_at_the_tile_edges(features, fi, fo):
    lens = E.resample_lengths(fi, fo)
    x = E.resample_signal(fi, fo)
    w, n = _batch([x[:m] for m, _ in lens], nmax=len(x) + 37, fill=12345.0)
    out, n_out = features.resample(w, n, fi, fo)
    out = out.cpu().numpy()
    assert out.shape == (len(lens), max(c for _, c in lens))        # Nmax_out is the longest count: no slack column
    for b, ((m, c), (ref, r32)) in enumerate(zip(lens, E.resample_oracles(fi, fo))):
        assert n_out[b] == c == len(ref)
        assert (out[b, c:] == 0).all(), (b, c)
        (dmax, drms), (e_max, e_rms) = E.errors(out[b, :c], ref), E.errors(r32, ref)
        print("resample %d -> %d, %d outputs: max %.3e / float32 %.3e = %.2f, rms %.3e / float32 %.3e = %.2f"
              % (fi, fo, c, dmax, e_max, dmax / e_max, drms, e_rms, drms / e_rms))
        E.note("resample", max(dmax / (2 * e_max), drms / (2 * e_rms)))
        assert dmax <= 2 * e_max, (b, c, dmax, e_max)
        assert drms <= 2 * e_rms, (b, c, drms, e_rms)
