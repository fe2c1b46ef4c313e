"""Training from audio on the GPU: the span form of the fbank / MFCC kernels against the whole-utterance
launches bit for bit, spk_pcm16_to_f32, features.AugmentPool against features.augment bit for bit, ingest.WavTrainLoader against
the offline chain run in-process on whole utterances (one fp32 ulp of the offline value per element: the only difference is the
origin of the fp64 prefix sums of the sliding CMN, which can move a value across one rounding boundary), and
scripts/train_resnet.py --wav-scp against --native-reader on the archives compute_fbank.py writes.  The tests print how many
elements differ at all."""
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import augment_ref as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000
RVB = 'cat {wav} | wav-reverberate --shift-output=true --impulse-response="{rir}" - - |'
NOISE = "wav-reverberate --shift-output=true --additive-signals='{items}' --start-times='{starts}' --snrs='{snrs}' {wav} - |"
BG = 'wav-reverberate --duration={dur} "{wav}" - |'


def _write_wav(path, samples, rate=FS):
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(np.asarray(samples).astype("<i2").tobytes())
    return str(path)


def _speech(n, seed):
    """bursts of low-pass noise between near-silence: the energy VAD finds voiced and unvoiced frames"""
    rng = np.random.default_rng(seed)
    v = np.convolve(rng.normal(0, 1, n + 15), np.hanning(16) / np.hanning(16).sum())[15:15 + n]
    env = 0.03 + 0.97 * (np.sin(2 * np.pi * np.arange(n) / (3100.0 + 97 * (seed % 7)) + seed) > -0.55)
    return np.round(v / np.abs(v).max() * 6000.0 * env).astype(np.int16)


# ---- the span kernels ----
def _configs():
    from pytorch_kaldi_resnet_amd import features
    return {
        "fbank16k_f40_nosnip": features.FbankOptions(num_mel_bins=40, snip_edges=False),
        "fbank8k_f23_snip": features.FbankOptions(sample_frequency=8000.0, num_mel_bins=23, snip_edges=True),
        "mfcc16k_f40_c13": features.MfccOptions(num_mel_bins=40, num_ceps=13, snip_edges=False),
    }


_WHOLE = {}


def _whole(name, dither):
    """the utterances of a configuration and their whole-utterance features, computed once: (opts, [int16 samples], feats [B, R, T]
    cuda, log energies, frame counts, utt ids)"""
    from pytorch_kaldi_resnet_amd import features
    if (name, dither) not in _WHOLE:
        import dataclasses
        opts = dataclasses.replace(_configs()[name], dither=float(dither))
        L, S = opts.frame_len, opts.frame_sh
        lens = [L, L + 33 * S + 7, 5 * S + L + 1, 70 * S + 3, 129 * S + L - 1, 41 * S]       # the first: exactly one frame length
        utts = [_speech(n, 100 + i) for i, n in enumerate(lens)]
        buf = np.zeros((len(utts), max(lens)), dtype=np.float32)
        for b, u in enumerate(utts):
            buf[b, :len(u)] = u
        ids = [features.utt_id("utt%d" % i) for i in range(len(utts))]
        fn = features.mfcc if isinstance(opts, features.MfccOptions) else features.fbank
        feats, T, loge = fn(torch.from_numpy(buf).cuda(), lens, opts, ids, seed=7)
        _WHOLE[(name, dither)] = (opts, utts, feats, loge, T, ids)
    return _WHOLE[(name, dither)]


def _check_spans(name, dither, spans, odd_first=False, tcap_extra=0):
    """spans: (utterance, frame0, nframes).  Every row is torch.equal to the column slice of the whole-utterance call, zero behind"""
    from pytorch_kaldi_resnet_amd import features
    opts, utts, feats, loge, T, ids = _whole(name, dither)
    u = np.array([s[0] for s in spans])
    f0 = np.array([s[1] for s in spans])
    nf = np.array([s[2] for s in spans])
    total = np.array([len(utts[i]) for i in u])
    first, last = features.span_samples(opts, f0, np.maximum(f0 + nf, f0 + 1), total)
    first = np.where(nf > 0, first, 0)
    last = np.where(nf > 0, last, 1)
    if odd_first:           # one more sample in front where that makes the row start at an odd sample
        first = np.where((first % 2 == 0) & (first > 0), first - 1, first)
    Nmax = int((last - first).max()) + 5
    buf = np.full((len(spans), Nmax), 12345.0, dtype=np.float32)        # garbage behind the span must not be read
    for b, i in enumerate(u):
        buf[b, :last[b] - first[b]] = utts[i][first[b]:last[b]]
    fn = features.mfcc_span if isinstance(opts, features.MfccOptions) else features.fbank_span
    Tcap = int(nf.max()) + tcap_extra
    out, n_out, le = fn(torch.from_numpy(buf).cuda(), last - first, first, total, f0, nf, opts, [ids[i] for i in u], seed=7, Tcap=Tcap)
    assert list(n_out) == list(nf) and out.shape == (len(spans), feats.shape[1], Tcap)
    for b, i in enumerate(u):
        assert torch.equal(out[b, :, :nf[b]], feats[i, :, f0[b]:f0[b] + nf[b]]), (name, dither, spans[b])
        assert torch.equal(le[b, :nf[b]], loge[i, f0[b]:f0[b] + nf[b]]), (name, dither, spans[b])
        assert not out[b, :, nf[b]:].any() and not le[b, nf[b]:].any(), (name, dither, spans[b])
    return first


@pytest.mark.parametrize("dither", [0, 1])
@pytest.mark.parametrize("name", ["fbank16k_f40_nosnip", "fbank8k_f23_snip", "mfcc16k_f40_c13"])
def test_span_frames_are_the_whole_utterance_frames_bit_for_bit(name, dither):
    opts, utts, feats, loge, T, ids = _whole(name, dither)
    assert T[0] == (3 if not opts.snip_edges else 1) and T[4] >= 129
    # the whole utterance, every utterance (rows of different lengths; the utterance of exactly frame_len samples among them)
    _check_spans(name, dither, [(i, 0, int(T[i])) for i in range(len(utts))])
    # frames [0, 1), the last frame alone - of the one-frame-length utterance too
    _check_spans(name, dither, [(4, 0, 1), (4, int(T[4]) - 1, 1), (0, 0, 1), (0, int(T[0]) - 1, 1), (1, int(T[1]) - 1, 1)])
    # frame0 around the 32-frame tile, spans longer than a tile, an odd first sample
    first = _check_spans(name, dither, [(4, 31, 40), (4, 32, 33), (4, 33, 64), (3, 31, 1), (3, 32, 2), (3, 33, 5)], odd_first=True)
    assert (first % 2 == 1).any()
    # rows of different spans in one batch, a row past its last frame (no frames: zeros), columns past every row's span
    _check_spans(name, dither, [(4, 100, int(T[4]) - 100), (1, 2, 9), (5, int(T[5]), 0), (2, 1, 3), (0, 0, int(T[0]))], tcap_extra=37)


def test_span_refusals_need_no_launch():
    """the wrapper's refusals, checked on the host: nothing here reaches the kernel but the last call, whose `out` is taken"""
    from pytorch_kaldi_resnet_amd import features
    opts = _configs()["fbank16k_f40_nosnip"]
    N = 16000
    w = torch.zeros(1, N, device="cuda")
    ok = dict(nsamp=[N], first=[0], total=[N], frame0=[0], nframes=[100])
    for change, msg in [(dict(nframes=[101]), "frames outside"), (dict(first=[1], nsamp=[N - 1]), "outside the row"),
                        (dict(nsamp=[N - 1]), "outside the row"), (dict(total=[399], nsamp=[399]), "shorter than one frame")]:
        a = dict(ok, **change)
        with pytest.raises(ValueError, match=msg):
            features.fbank_span(w, a["nsamp"], a["first"], a["total"], a["frame0"], a["nframes"], opts)
    with pytest.raises(ValueError, match="utt_ids"):
        features.fbank_span(w, *[ok[k] for k in ("nsamp", "first", "total", "frame0", "nframes")], opts)          # dither 1
    with pytest.raises(ValueError, match="MfccOptions"):
        features.mfcc_span(w, *[ok[k] for k in ("nsamp", "first", "total", "frame0", "nframes")], opts)
    with pytest.raises(ValueError, match="float32 cuda"):
        features.fbank_span(w.cpu(), *[ok[k] for k in ("nsamp", "first", "total", "frame0", "nframes")], opts)
    # out is [B, num_ceps, Tcap] exactly: a tensor one row short is refused, not written past its end
    mo = features.MfccOptions(num_mel_bins=40, num_ceps=13, snip_edges=False, dither=0.0)
    span = [ok[k] for k in ("nsamp", "first", "total", "frame0", "nframes")]
    with pytest.raises(ValueError, match="out must be"):
        features.mfcc_span(w, *span, mo, out=torch.empty(1, mo.num_ceps - 1, 100, device="cuda"))
    out = torch.empty(1, mo.num_ceps, 100, device="cuda")
    assert features.mfcc_span(w, *span, mo, out=out)[0] is out


def test_pcm16_to_f32():
    from pytorch_kaldi_resnet_amd import features
    rng = np.random.default_rng(0)
    for Nmax in (4096 + 40, 2048 + 37, 8, 3):          # vector rows (Nmax % 8 == 0, two blocks), scalar rows, one thread's worth
        x = rng.integers(-32768, 32768, size=(4, Nmax)).astype(np.int16)
        x[0, :2] = (-32768, 32767)
        count = np.array([Nmax, 0, Nmax // 2 + 1, max(Nmax - 9, 1)], dtype=np.int32)
        out = features.pcm16_to_f32(torch.from_numpy(x).cuda(), torch.from_numpy(count).cuda()).cpu().numpy()
        ref = np.where(np.arange(Nmax)[None, :] < count[:, None], x.astype(np.float32), 0.0)
        assert out.dtype == np.float32 and np.array_equal(out, ref), Nmax


# ---- the corpus of the pool, loader and entry-point tests ----
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """24 WAVs of 0.4 - 4 s under 4 speakers, their VAD vectors (features.vad on the whole utterances, dither 0 and the dithered
    fbank of the tests share them), impulse responses and noises"""
    from pytorch_kaldi_resnet_amd import features, ingest, kaldi_io
    d = tmp_path_factory.mktemp("wav_train")
    rng = np.random.default_rng(1)
    secs = np.concatenate([[0.4, 4.0], rng.uniform(0.4, 4.0, 22)])
    keys = ["s%d-u%02d" % (i % 4, i) for i in range(24)]
    wavs = {k: _write_wav(d / (k + ".wav"), _speech(int(s * FS), 200 + i)) for i, (k, s) in enumerate(zip(keys, secs))}
    opts = features.FbankOptions(num_mel_bins=24, snip_edges=False, dither=0.0)
    conf = str(d / "fbank.conf")
    open(conf, "w").write("--num-mel-bins=24\n--snip-edges=false\n--dither=0\n")
    open(str(d / "vad.conf"), "w").write("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n")
    vad_opts = features.VadOptions(vad_energy_threshold=5.5)
    table = ingest.WavTable([wavs[k] for k in keys], FS)
    nmax = int(table.nsamp.max())
    buf = torch.empty(24, nmax)
    table.read_padded(np.arange(24), nmax, buf, 2)
    wave_all = buf.cuda()
    feats, T, loge = features.fbank(wave_all, table.nsamp, opts)
    v, vidx, cnt = features.vad(loge, T, vad_opts)
    v = v.cpu().numpy()
    lines = []
    with open(str(d / "vad.ark"), "wb") as f:
        for b, k in enumerate(keys):
            f.write((k + " ").encode())
            lines.append((k, "%s:%d" % (d / "vad.ark", f.tell())))
            kaldi_io.write_vec_flt(f, v[b, :T[b]].astype(np.float32))
    long_enough = [b for b in range(24) if cnt[b] >= 64]
    assert 8 <= len(long_enough) < 24 and (cnt < T).any(), (cnt, T)
    rir = {k: _write_wav(d / ("rir_%s.wav" % k), np.round(20000 * A.impulse_response(sec, 80 + i)))
           for i, (k, sec) in enumerate({"a": 0.3, "b": 0.6}.items())}
    nz = {k: _write_wav(d / ("noise_%s.wav" % k), A.noise(n, 90 + i)) for i, (k, n) in enumerate({"a": 6000, "b": 9000, "c": 30000}.items())}
    return dict(dir=d, keys=keys, wavs=wavs, opts=opts, conf=conf, vad_opts=vad_opts, vad_lines=dict(lines), table=table,
                wave_all=wave_all, T=T, vad=v, vidx=vidx, cnt=cnt, long=long_enough, rir=rir, nz=nz)


def _scp(c, name, rows, entries=None, vad_keys=None):
    """wav.scp, vad.scp and utt2spkid of the keys `rows` (entries: {key: (written key, wav.scp value)} for augmented copies)"""
    d = c["dir"]
    wav, vad, u2s = [], [], []
    for b in rows:
        k = c["keys"][b]
        wk, val = (entries or {}).get(k, (k, c["wavs"][k]))
        wav.append("%s %s\n" % (wk, val))
        vad.append("%s %s\n" % (wk, c["vad_lines"][k]))          # the recipe copies the clean file's vector under the copy's key
        u2s.append("%s %d\n" % (wk, int(k[1])))
    paths = [str(d / (name + ext)) for ext in (".wav.scp", ".vad.scp", ".utt2spkid")]
    for p, lines in zip(paths, (wav, vad, u2s)):
        open(p, "w").writelines(lines)
    return paths


def _aug_entries(c, rows):
    """every second key of `rows` as an augmented copy: reverb, one noise, several noises (one with --duration), reverb"""
    kinds = [lambda w: RVB.format(wav=w, rir=c["rir"]["a"]),
             lambda w: NOISE.format(items=c["nz"]["a"], starts="0.1", snrs="12", wav=w),
             lambda w: NOISE.format(items=",".join([c["nz"]["b"], BG.format(dur=1.5, wav=c["nz"]["c"]), c["nz"]["a"]]), starts="0,0,0.3",
                                    snrs="15,10,8", wav=w),
             lambda w: RVB.format(wav=w, rir=c["rir"]["b"])]
    out = {}
    for j, b in enumerate(rows[::2]):
        k = c["keys"][b]
        out[k] = ("aug%d-%s" % (j % 4, k), kinds[j % 4](c["wavs"][k]))
    return out


def test_augment_pool_is_features_augment_bit_for_bit(corpus):
    from pytorch_kaldi_resnet_amd import features, ingest
    c = corpus
    rows = c["long"][:8]
    wav_scp, _, _ = _scp(c, "pool", rows, _aug_entries(c, rows))
    keys, entries = features.read_wav_scp(wav_scp)
    assert [e.augmented for e in entries] == [True, False] * 4
    assert [bool(e.rir_path) for e in entries][::2] == [True, False, False, True] and len(entries[4].noises) == 3
    table = ingest.WavTable([e.path for e in entries], FS)
    pool = features.AugmentPool(features.WavAugmentation(table, entries), "cuda", FS)
    idx = np.arange(8)
    first = np.array([0, 5, 1001, 16, 333, 0, 4000, 77])
    count = np.minimum(table.nsamp - first, 14000 + 100 * idx)
    Nmax = int(-(-count.max() // 8) * 8)
    pcm = torch.empty(8, Nmax, dtype=torch.int16)
    table.read_span(idx, first, count, Nmax, pcm)
    cdev = torch.from_numpy(count.astype(np.int32)).cuda()
    wave_t = features.pcm16_to_f32(pcm.cuda(), cdev)
    plan = pool.plan(idx)
    assert list(plan.rows) == [0, 2, 4, 6] and plan.desc_file.size == 4
    sel = torch.from_numpy(plan.rows).cuda()
    got = wave_t.clone()
    got[sel] = pool.apply(wave_t[sel], cdev[sel], plan)
    assert pool.reads == 5                      # two impulse responses, three noises
    again = pool.apply(wave_t[sel], cdev[sel], plan)
    assert pool.reads == 5 and torch.equal(again, got[sel])          # a second call reads no file
    ref_aug = features.WavAugmentation(table, entries)
    rir, noises, names = ref_aug.inputs(idx)
    ref, clipped = features.augment(wave_t, count, rir, noises, quantize=True, sample_rate=FS, names=names)
    assert torch.equal(got, ref)
    assert not torch.equal(got[sel], wave_t[sel]) and torch.equal(got[1], wave_t[1])
    assert int(pool.clipped) == 2 * int(clipped.sum())              # the counts stay on the device, accumulated per call
    assert pool.plan(np.array([1, 3, 5])) is None


# ---- the loader against the offline chain ----
def _offline(c, opts, cmn, use_vad, seed, ids):
    """the matrices compute_fbank.py --egs --vad-scp (use_vad) / sliding CMN alone write, for every utterance of the corpus, in one
    whole-utterance batch: ([24, F, Tmax] cuda, lengths)"""
    from pytorch_kaldi_resnet_amd import features
    feats, T, _ = features.fbank(c["wave_all"], c["table"].nsamp, opts, ids, seed)
    if not use_vad:
        return features.sliding_cmn(feats, T, cmn), T
    return features.select_voiced(feats, T, c["vidx"], c["cnt"], cmn)


def _ulp_check(what, got, ref):
    got, ref = got.cpu().numpy(), ref.cpu().numpy()
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    differ = int((got != ref).sum())
    worst = float((d / np.spacing(np.abs(ref)).astype(np.float64)).max())
    print("%s: %d of %d elements differ, worst %.2f ulp" % (what, differ, got.size, worst))
    assert (d <= np.spacing(np.abs(ref))).all(), what
    return differ


@pytest.mark.parametrize("case", ["vad", "dither", "novad", "lengths"])
def test_loader_gives_the_offline_columns(corpus, case):
    import dataclasses
    from pytorch_kaldi_resnet_amd import features, ingest
    c = corpus
    rows = c["long"]
    wav_scp, vad_scp, u2s = _scp(c, "loader", rows)
    opts = dataclasses.replace(c["opts"], dither=1.0 if case == "dither" else 0.0)
    cmn = features.CmnOptions(cmn_window=30)
    ids = [features.utt_id(k) for k in c["keys"]]
    off, lens = _offline(c, opts, cmn, case != "novad", 11, ids)
    loader = ingest.WavTrainLoader(wav_scp, u2s, 48, 8, opts, cmn, vad_scp=None if case == "novad" else vad_scp, feat_seed=11, seed=3,
                                   threads=2, chunk_range=(48, 64, 16) if case == "lengths" else None)
    n_el = differ = 0
    seen_T = set()
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        draws = list(loader.draws())
        batches = list(loader)
        assert len(batches) == len(draws) == len(loader)
        for (k, sel, r, T, starts), (x, y) in zip(draws, batches):
            assert x.shape == (len(sel), 24, T) and x.dtype == torch.float32 and x.is_cuda
            assert torch.equal(y.cpu(), torch.from_numpy(loader.labels[sel]))
            ref = torch.stack([off[rows[i], :, s:s + T] for i, s in zip(r, starts)])
            assert all(s + T <= lens[rows[i]] for i, s in zip(r, starts))
            differ += _ulp_check("%s epoch %d batch %d" % (case, epoch, k), x, ref)
            n_el += x.numel()
            seen_T.add(T)
    print("loader %s: %d of %d elements differ from the offline chain" % (case, differ, n_el))
    assert seen_T == ({48, 64} if case == "lengths" else {48})


def test_loader_augmented_rows_are_the_augmented_span(corpus):
    """an augmented entry is applied to the span that is read: features.augment on the span, then the span
    front end and the CMN selection through the functional API"""
    from pytorch_kaldi_resnet_amd import features, ingest
    c = corpus
    rows = c["long"][:8]
    wav_scp, vad_scp, u2s = _scp(c, "augloader", rows, _aug_entries(c, rows))
    opts, cmn = c["opts"], features.CmnOptions(cmn_window=30)
    loader = ingest.WavTrainLoader(wav_scp, u2s, 48, 8, opts, cmn, vad_scp=vad_scp, feat_seed=0, seed=5, threads=2)
    assert loader.pool is not None
    draws = list(loader.draws())
    batches = list(loader)
    ref_aug = features.WavAugmentation(loader.table, loader.pool.aug.entries)
    off, _ = _offline(c, opts, cmn, True, 0, None)
    differ = n_el = 0
    for (k, sel, r, T, starts), (x, y) in zip(draws, batches):
        p = loader.plan(r, starts, T)
        B, Nmax = len(r), int(-(-p.count.max() // 8) * 8)
        pcm = torch.empty(B, Nmax, dtype=torch.int16)
        loader.table.read_span(r, p.first, p.count, Nmax, pcm)
        wave_t = features.pcm16_to_f32(pcm.cuda(), torch.from_numpy(p.count.astype(np.int32)).cuda())
        rir, noises, names = ref_aug.inputs(r)
        wave_t, _ = features.augment(wave_t, p.count, rir, noises, quantize=True, sample_rate=FS, names=names)
        nf = p.frame_hi - p.frame_lo
        feats, _, _ = features.fbank_span(wave_t, p.count, p.first, loader.table.nsamp[r], p.frame_lo, nf, opts)
        rel = np.zeros((B, feats.shape[2]), dtype=np.int32)
        rel[:, :T] = p.rel
        ref, _ = features.select_voiced(feats, nf, torch.from_numpy(rel).cuda(), np.full(B, T), cmn)
        differ += _ulp_check("augmented batch %d" % k, x, ref)
        n_el += x.numel()
        aug_rows = [j for j, i in enumerate(r) if loader.pool.aug.entries[i].augmented]
        clean = [j for j in range(B) if j not in aug_rows]
        assert aug_rows and clean
        # the clean rows are the offline columns; the augmented rows are not their clean file's
        for j in range(B):
            col = off[rows[r[j]], :, starts[j]:starts[j] + T]
            if j in clean:
                _ulp_check("clean row %d" % j, x[j], col)
            else:
                assert not torch.equal(x[j], col)
    print("augmented loader: %d of %d elements differ from augment-on-the-span" % (differ, n_el))


# ---- the entry point ----
def _run(script, cmd, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT, SPK_AUTOTUNE="0")
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + cmd, env=env, capture_output=True, text=True,
                          timeout=timeout)


def _first_loss(stdout):
    m = re.search(r"Epoch: \[0\]\[\s*0/\s*\d+\].*?Loss (\S+) ", stdout)
    assert m, stdout[-3000:]
    return float(m.group(1))


def test_train_resnet_from_audio_against_the_archives(corpus):
    c = corpus
    d = str(c["dir"])
    wav_scp, _, u2s = _scp(c, "train", c["long"])
    common = ["--fbank-config", c["conf"], "--seed", "4"]
    r = _run("compute_fbank.py", [wav_scp, os.path.join(d, "raw"), "--vad-config", os.path.join(d, "vad.conf")] + common)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    vad_scp = os.path.join(d, "raw", "vad.scp")
    r = _run("compute_fbank.py", [wav_scp, os.path.join(d, "egs"), "--egs", "--vad-scp", vad_scp, "--cmn-window", "30"] + common)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    feats_scp = os.path.join(d, "egs", "feats.scp")
    train = ["--utt2spkid", u2s, "--cv-list", feats_scp, "--input-dim", "24", "--spk-num", "4", "-a", "resnet18", "-b", "8",
             "--max-chunk-size", "48", "--max-steps", "3", "--epochs", "1", "--no-graph", "--seed", "2", "-j", "1", "--gpu", "0"]
    a = _run("train_resnet.py", train + ["--train-list", feats_scp, "--native-reader", "--log-dir", os.path.join(d, "log_ark")])
    assert a.returncode == 0, a.stdout[-2000:] + a.stderr[-3000:]
    audio = ["--wav-scp", wav_scp, "--vad-scp", vad_scp, "--fbank-config", c["conf"], "--cmn-window", "30", "--feat-seed", "4"]
    b = _run("train_resnet.py", train + audio + ["--log-dir", os.path.join(d, "log_wav")])
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-3000:]
    for log in ("log_ark", "log_wav"):
        assert os.path.isfile(os.path.join(d, log, "checkpoint_epoch0.pth.tar")), log
    la, lb = _first_loss(a.stdout), _first_loss(b.stdout)
    print("first loss: archives %.6e, audio %.6e, relative difference %.3g" % (la, lb, abs(la - lb) / abs(la)))
    assert abs(la - lb) <= 1e-4 * abs(la)
    # refusals: non-zero exit before the first step, naming the file / the key and the option
    hi = _write_wav(os.path.join(d, "hi44.wav"), np.zeros(44100, dtype=np.int16), rate=44100)
    lines = open(wav_scp).read().splitlines()
    bad_scp = os.path.join(d, "bad.wav.scp")
    open(bad_scp, "w").write("\n".join(lines[:-1] + ["%s %s" % (lines[-1].split()[0], hi)]) + "\n")
    r = _run("train_resnet.py", train + ["--wav-scp", bad_scp] + audio[2:] + ["--log-dir", os.path.join(d, "log_bad")])
    assert r.returncode != 0 and "hi44.wav" in r.stderr and "44100" in r.stderr and "Epoch: [0]" not in r.stdout, r.stderr[-2000:]
    short_vad = os.path.join(d, "short.vad.scp")
    open(short_vad, "w").write("\n".join(open(vad_scp).read().splitlines()[1:]) + "\n")
    r = _run("train_resnet.py", train + ["--wav-scp", wav_scp, "--vad-scp", short_vad] + audio[4:] + ["--log-dir", os.path.join(d, "log_bad")])
    key0 = lines[0].split()[0]
    assert r.returncode != 0 and key0 in r.stderr and "--vad-scp" in r.stderr and "Epoch: [0]" not in r.stdout, r.stderr[-2000:]
