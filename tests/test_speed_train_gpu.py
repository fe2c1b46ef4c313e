"""Training from audio with speed perturbation on the GPU (DESIGN.md sections 6e "Resampling" and 6k): the span form of the
resampler (include/spkwav.h) against features.resample on the whole utterance bit for bit - every alignment of the window in the
row, every tile edge, row lists, garbage behind the counts -, features.ChunkFrontend with speed rows against Frontend(speed=F) on the
whole file, ingest.WavTrainLoader against the archive compute_fbank.py writes for the same wav.scp (one fp32 ulp of the offline value:
the sliding CMN's prefix sums start elsewhere, section 6k; the resampler adds nothing), and scripts/train_resnet.py --wav-scp against
--native-reader on that archive.  The tests print how many elements differ at all."""
import dataclasses
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import augment_ref as A
import resample_span_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000
SOX = "sox -t wav %s -t wav - speed %s |"
RVB = 'cat {wav} | wav-reverberate --shift-output=true --impulse-response="{rir}" - - |'
BIG = 1e30


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


def _ulp_check(what, got, ref):
    """the criterion of tests/test_wav_train_gpu.py: every element within one ulp of the offline value"""
    got, ref = got.cpu().numpy(), ref.cpu().numpy()
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    differ = int((got != ref).sum())
    worst = float((d / np.spacing(np.abs(ref)).astype(np.float64)).max())
    print("%s: %d of %d elements differ, worst %.2f ulp" % (what, differ, got.size, worst))
    assert (d <= np.spacing(np.abs(ref))).all(), what
    return differ


# ---- 1. the span kernel against the whole-utterance launch ----
def _tile256_rates():
    """a rate pair whose table leaves room for tiles of 256 outputs only, found on the host (spk_resample_tile launches nothing)"""
    from pytorch_kaldi_resnet_amd import features, hip
    for ou in range(880, 1100):
        iu = ou - 1
        if hip.lib().spk_resample_tile(iu, ou, features._resample_first(iu, ou)[2]) == 256:
            return iu, ou
    return None


LENS = [20011, 23456, 24999]
_WHOLE = {}


def _whole(fi, fo):
    """three utterances and their whole-utterance resampling, computed once per rate pair: (x [3, Nmax] numpy, y cuda, n_out)"""
    from pytorch_kaldi_resnet_amd import features
    if (fi, fo) not in _WHOLE:
        rng = np.random.default_rng(fi + fo)
        x = np.zeros((len(LENS), max(LENS)), dtype=np.float32)
        for b, n in enumerate(LENS):
            x[b, :n] = np.round(rng.normal(0, 3000, n))
        y, n_out = features.resample(torch.from_numpy(x).cuda(), LENS, fi, fo)
        _WHOLE[(fi, fo)] = (x, y, n_out)
    return _WHOLE[(fi, fo)]


def _run_spans(fi, fo, spans, front=None, rows=None, offset_view=False):
    """spans: (utterance, ofirst, ocount); front: per span, samples the row holds in front of what the rule names (where the file
    has them).  1e30 behind every icount and all over the output buffer before the launch.  Every row of the list equals the
    whole-utterance samples bit for bit and is 0 behind them; the others keep the 1e30.  Returns (ifirst, window starts a(ofirst))"""
    from pytorch_kaldi_resnet_amd import features, ingest
    x, y, n_out = _whole(fi, fo)
    iu, ou, K, first, _ = features.resample_tables(fi, fo)
    u = np.array([s[0] for s in spans])
    o = np.array([s[1] for s in spans])
    m = np.array([s[2] for s in spans])
    N = np.array([LENS[i] for i in u])
    f, c = ingest.resample_input_span(o, m, N, fi, fo)
    if front is not None:
        f2 = np.maximum(f - np.asarray(front), 0)
        f, c = f2, c + (f - f2)
    B, Nmax_in, Nmax_out = len(spans), int(c.max()) + 3, int(m.max()) + 5
    buf = np.full(B * Nmax_in + 1, BIG, dtype=np.float32)
    rowsv = buf[1:].reshape(B, Nmax_in) if offset_view else buf[:-1].reshape(B, Nmax_in)
    for b in range(B):
        rowsv[b, :c[b]] = x[u[b], f[b]:f[b] + c[b]]
    base = torch.from_numpy(buf).cuda()
    wave_in = (base[1:] if offset_view else base[:-1]).view(B, Nmax_in)
    assert wave_in.is_contiguous() and (wave_in.data_ptr() % 16 == 4) == offset_view
    out = torch.full((B, Nmax_out), BIG, device="cuda")
    got = features.resample_span(wave_in, c, f, N, o, m, fi, fo, rows=rows, out=out)
    assert got is out
    for b in range(B):
        if rows is not None and b not in rows:
            assert bool((out[b] == BIG).all()), (fi, fo, spans[b], "a row outside the list was touched")
            continue
        assert torch.equal(out[b, :m[b]], y[u[b], o[b]:o[b] + m[b]]), (fi, fo, spans[b], int(f[b]))
        assert not out[b, m[b]:].any(), (fi, fo, spans[b])
    return f, first[o % ou] + (o // ou) * iu


def _span_cases(fi, fo):
    from pytorch_kaldi_resnet_amd import features, hip
    iu, ou, K, first, _ = features.resample_tables(fi, fo)
    TO = hip.lib().spk_resample_tile(iu, ou, K)
    NT = min(max(-(-2 * ou * K // TO), 1), 8)         # tiles per workgroup, where the row has that many (csrc/resample.hip)
    x, y, n_out = _whole(fi, fo)
    assert all(NT * TO + 1 < n for n in n_out)
    counts = [1, TO, TO + 1, NT * TO + 1]
    # ofirst = 0: the window starts below 0 and is zero-filled; spans ending at N'
    f, a = _run_spans(fi, fo, [(i % 3, 0, cnt) for i, cnt in enumerate(counts)] + [(2 - i % 3, int(n_out[2 - i % 3]) - cnt, cnt)
                                                                                  for i, cnt in enumerate(counts)])
    assert (a[:4] < 0).all() and (f[:4] == 0).all()
    # ofirst in every residue mod 4, both parities of the window start; rows of different spans and utterances in one launch
    spans = [(r % 3, 5000 + 37 * r, TO + 1 + r) for r in range(8)]
    f, a = _run_spans(fi, fo, spans)
    assert {s[1] % 4 for s in spans} == {0, 1, 2, 3} and set(a % 2) == {0, 1}
    # ifirst in every residue mod 4 (and with it every phase of the window in the 16-byte staging)
    f, a = _run_spans(fi, fo, [(1, 7001, TO + 1)] * 4 + [(0, 9000, 2 * TO + 3)] * 4, front=[0, 1, 2, 3] * 2)
    assert set(f[:4] % 4) == set(f[4:] % 4) == {0, 1, 2, 3}
    # a view offset by one float: the element-load path
    _run_spans(fi, fo, spans[:4] + [(0, 0, TO + 1), (2, int(n_out[2]) - TO - 1, TO + 1)], offset_view=True)
    # the whole utterance as a span; a row list that is a strict subset
    _run_spans(fi, fo, [(i, 0, int(n_out[i])) for i in range(3)])
    _run_spans(fi, fo, spans, rows=[6, 1, 3])
    return TO


@pytest.mark.parametrize("speed,tile", [("0.9", 1024), ("1.1", 1024), ("0.999", 512)])
def test_span_equals_whole_bit_for_bit(speed, tile):
    from pytorch_kaldi_resnet_amd import features
    assert _span_cases(*features.speed_rates(speed, FS)) == tile


def test_span_equals_whole_at_the_256_tile():
    rates = _tile256_rates()
    assert rates is not None, "no coprime pair (ou - 1, ou), 880 <= ou < 1100, leaves room for tiles of 256 only"
    assert _span_cases(*rates) == 256


def test_a_sample_the_row_lacks_reads_as_zero():
    """the launch without the host check: a sample inside the utterance but outside the row is not read - the result is that of
    the utterance with zeros there (tests/resample_span_ref.py: zero_outside_row), bit for bit, and nothing of the 1e30 around the
    row's samples survives"""
    from pytorch_kaldi_resnet_amd import features, ingest
    fi, fo = features.speed_rates("0.9", FS)
    x, y, n_out = _whole(fi, fo)
    spans = [(0, 4000, 3000), (1, 0, 2000), (2, int(n_out[2]) - 2500, 2500)]
    u, o, m = (np.array(v) for v in zip(*spans))
    N = np.array([LENS[i] for i in u])
    f, c = ingest.resample_input_span(o, m, N, fi, fo)
    f, c = f + np.array([2, 5, 0]), c - np.array([2 + 3, 5, 4])          # short at the front, at the end, or both
    z = np.zeros((3, max(LENS)), dtype=np.float32)
    for b in range(3):
        z[b] = R.zero_outside_row(x[u[b]], f[b], c[b])
    ref, _ = features.resample(torch.from_numpy(z).cuda(), N, fi, fo)
    Nmax_in, Nmax_out = int(c.max()) + 4, int(m.max())
    buf = np.full((3, Nmax_in), BIG, dtype=np.float32)
    for b in range(3):
        buf[b, :c[b]] = x[u[b], f[b]:f[b] + c[b]]
    with pytest.raises(ValueError, match="row 0 .*outside the row"):
        features.resample_span(torch.from_numpy(buf).cuda(), c, f, N, o, m, fi, fo)

    def dv(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
    out = torch.full((3, Nmax_out), BIG, device="cuda")
    features._resample_span_launch(torch.from_numpy(buf).cuda(), dv(f, np.int64), dv(c, np.int32), dv(N, np.int64), dv(o, np.int64),
                                   dv(m, np.int32), None, fi, fo, out)
    for b in range(3):
        assert torch.equal(out[b, :m[b]], ref[b, o[b]:o[b] + m[b]]) and not out[b, m[b]:].any(), spans[b]
        assert not torch.equal(out[b, :m[b]], y[u[b], o[b]:o[b] + m[b]])
    # the copy of the rows that are not resampled: the counted samples, zeros behind, other rows untouched
    cp = torch.full((3, Nmax_in + 7), BIG, device="cuda")
    features._copy_rows_launch(torch.from_numpy(buf).cuda(), dv(c, np.int32), dv([2, 0], np.int32), cp)
    for b in (0, 2):
        assert torch.equal(cp[b, :c[b]], torch.from_numpy(buf[b, :c[b]]).cuda()) and not cp[b, c[b]:].any()
    assert bool((cp[1] == BIG).all())


# ---- 2. ChunkFrontend with speed rows against Frontend(speed=F) on the whole file ----
def _configs():
    from pytorch_kaldi_resnet_amd import features
    return {
        "fbank16k_f40_nosnip": features.FbankOptions(num_mel_bins=40, snip_edges=False),
        "fbank8k_f23_snip": features.FbankOptions(sample_frequency=8000.0, num_mel_bins=23, snip_edges=True),
        "mfcc16k_f40_c13": features.MfccOptions(num_mel_bins=40, num_ceps=13, snip_edges=False),
    }


ROW_SPEED = [None, "0.9", "1.1", "0.9", None, "1.1"]


@pytest.mark.parametrize("dither", [0, 1])
@pytest.mark.parametrize("name", ["fbank16k_f40_nosnip", "fbank8k_f23_snip", "mfcc16k_f40_c13"])
def test_chunk_frontend_with_speed_rows(name, dither):
    from pytorch_kaldi_resnet_amd import features, ingest
    opts = dataclasses.replace(_configs()[name], dither=float(dither))
    fs = int(opts.sample_frequency)
    lens = [20000 + 831 * i for i in range(6)]
    utts = [_speech(n, 300 + i) for i, n in enumerate(lens)]
    ids = [features.utt_id("sp-utt%d" % i) for i in range(6)]
    B, T, seed = 6, 40, 9
    x = np.zeros((B, max(lens)), dtype=np.float32)
    for b, v in enumerate(utts):
        x[b, :len(v)] = v
    xg = torch.from_numpy(x).cuda()
    rates = {sp: features.speed_rates(sp, fs) for sp in ("0.9", "1.1")}
    n_out = np.array([lens[b] if sp is None else int(features.num_resampled(lens[b], *rates[sp])) for b, sp in enumerate(ROW_SPEED)])
    frames = np.array([opts.num_frames(int(n)) for n in n_out])
    differ = n_el = 0
    for cmn in (None, features.CmnOptions(cmn_window=30)):
        ref = [None] * B            # the whole-file features of every row: Frontend(speed=F), sliding CMN over all frames
        for sp in (None, "0.9", "1.1"):
            sel = [b for b in range(B) if ROW_SPEED[b] == sp]
            feats, Tw = features.Frontend(opts, cmn=cmn, speed=sp)(xg[sel], [lens[b] for b in sel], [ids[b] for b in sel], seed)
            for j, b in enumerate(sel):
                assert Tw[j] == frames[b]
                ref[b] = feats[j, :, :Tw[j]]
        W = 30 if cmn is not None else 0
        for v0 in ([0] * B, list(frames - T), [17, 5, 33, 60, 41, 8]):      # head (ofirst = 0), tail (up to N'), interior
            p = ingest.plan_spans([None] * B, v0, T, W, frames, opts, n_out)
            ifirst, icount = p.first.copy(), p.count.copy()
            for b, sp in enumerate(ROW_SPEED):
                if sp is not None:
                    ifirst[b], icount[b] = ingest.resample_input_span(p.first[b], p.count[b], lens[b], *rates[sp])
            Nmax = -(-int(icount.max()) // 8) * 8
            pcm = np.zeros((B, Nmax), dtype=np.int16)
            for b in range(B):
                pcm[b, :icount[b]] = utts[b][ifirst[b]:ifirst[b] + icount[b]]
            Tcap = int((p.frame_hi - p.frame_lo).max())
            rel = np.zeros((B, Tcap), dtype=np.int32)
            rel[:, :T] = p.rel

            def dv(a, dtype):
                return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
            order = [0, 4, 1, 3, 2, 5]                      # plain rows, then the rows of 0.9, then those of 1.1
            sb = features.SpeedBatch(dv(p.first, np.int64), dv(n_out, np.int64), dv(p.count, np.int32), dv(order, np.int32),
                                     [rates["0.9"] + (2, 4), rates["1.1"] + (4, 6)], (0, 2), -(-int(p.count.max()) // 4) * 4)
            times = {}
            got = features.ChunkFrontend(opts, cmn, seed)(dv(pcm, np.int16), dv(icount, np.int32), dv(ifirst, np.int64),
                                                          dv(lens, np.int64), dv(p.frame_lo, np.int32),
                                                          dv(p.frame_hi - p.frame_lo, np.int32), dv(rel, np.int32), T, dv(ids, np.int64),
                                                          None, times, sb)
            assert "resample" in times and got.shape == (B, ref[0].shape[0], T)
            want = torch.stack([ref[b][:, v0[b]:v0[b] + T] for b in range(B)])
            if cmn is None:
                assert torch.equal(got, want), (name, dither, v0)
            else:
                differ += _ulp_check("%s dither %d v0 %s" % (name, dither, v0[:2]), got, want)
                n_el += got.numel()
    print("chunk front end %s dither %d: %d of %d CMN'd elements differ from the whole file" % (name, dither, differ, n_el))


# ---- 3. and 4. the loader and the entry point against the archive of the same wav.scp ----
def _run(script, cmd, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT, SPK_AUTOTUNE="0")
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + cmd, env=env, capture_output=True, text=True,
                          timeout=timeout)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """12 files of 1.5 - 3 s under 4 speakers; wav.scp with each file plain, as sp0.9- and as sp1.1- (new speakers) and one
    reverberated copy; vad.scp from compute_fbank.py --vad-config on that wav.scp, the --egs archive from it"""
    d = tmp_path_factory.mktemp("speed_train")
    rng = np.random.default_rng(2)
    secs = np.concatenate([[1.5, 3.0], rng.uniform(1.5, 3.0, 10)])
    names = ["s%d-u%02d" % (i % 4, i) for i in range(12)]
    wavs = {k: _write_wav(d / (k + ".wav"), _speech(int(s * FS), 400 + i)) for i, (k, s) in enumerate(zip(names, secs))}
    rir = _write_wav(d / "rir.wav", np.round(20000 * A.impulse_response(0.3, 80)))
    lines, u2s = [], []
    for k in names:
        for sp, base in ((None, 0), ("0.9", 4), ("1.1", 8)):
            key = k if sp is None else "sp%s-%s" % (sp, k)
            lines.append((key, wavs[k] if sp is None else SOX % (wavs[k], sp)))
            u2s.append((key, int(k[1]) + base))
    aug_key = "rvb-" + names[5]
    lines.append((aug_key, RVB.format(wav=wavs[names[5]], rir=rir)))
    u2s.append((aug_key, int(names[5][1])))
    paths = {n: str(d / n) for n in ("wav.scp", "plain.scp", "clean.scp", "utt2spkid", "clean.utt2spkid", "fbank.conf", "vad.conf")}
    open(paths["wav.scp"], "w").writelines("%s %s\n" % l for l in lines)
    open(paths["plain.scp"], "w").writelines("%s %s\n" % (k, wavs[k]) for k in names)
    open(paths["clean.scp"], "w").writelines("%s %s\n" % l for l in lines[:-1])
    open(paths["utt2spkid"], "w").writelines("%s %d\n" % l for l in u2s)
    open(paths["clean.utt2spkid"], "w").writelines("%s %d\n" % l for l in u2s[:-1])
    open(paths["fbank.conf"], "w").write("--num-mel-bins=24\n--snip-edges=false\n")          # dither 1: keyed by the written key
    open(paths["vad.conf"], "w").write("--vad-energy-threshold=5.5\n--vad-energy-mean-scale=0.5\n")
    common = ["--fbank-config", paths["fbank.conf"], "--seed", "4"]
    r = _run("compute_fbank.py", [paths["wav.scp"], str(d / "raw"), "--vad-config", paths["vad.conf"]] + common)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    vad_scp = str(d / "raw" / "vad.scp")
    r = _run("compute_fbank.py", [paths["wav.scp"], str(d / "egs"), "--egs", "--vad-scp", vad_scp, "--cmn-window", "30"] + common)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return dict(dir=d, names=names, keys=[k for k, _ in lines], aug_key=aug_key, paths=paths, vad_scp=vad_scp, common=common,
                feats_scp=str(d / "egs" / "feats.scp"))


def _read_scp(scp):
    from pytorch_kaldi_resnet_amd import kaldi_io
    return {k: kaldi_io.read_mat(v.strip()) for k, v in (l.split(None, 1) for l in open(scp) if l.strip())}


def test_speed_matrices_are_those_of_the_speed_flag(corpus):
    """one command on the combined wav.scp writes, under the sp0.9- keys, the bits compute_fbank.py --speed 0.9 writes for the plain
    lines: same key, same dither stream, same resampling"""
    c = corpus
    r = _run("compute_fbank.py", [c["paths"]["plain.scp"], str(c["dir"] / "sp09"), "--speed", "0.9"] + c["common"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw, sp = _read_scp(str(c["dir"] / "raw" / "feats.scp")), _read_scp(str(c["dir"] / "sp09" / "feats.scp"))
    assert sorted(sp) == sorted("sp0.9-" + k for k in c["names"]) and len(raw) == 37
    for k, m in sp.items():
        assert m.shape == raw[k].shape and np.array_equal(m, raw[k]), k
    n = {k: int(v) for k, v in (l.split() for l in open(str(c["dir"] / "raw" / "utt2num_frames")))}
    assert all(n["sp0.9-" + k] > n[k] > n["sp1.1-" + k] for k in c["names"])


def test_loader_gives_the_columns_of_the_archive(corpus):
    from pytorch_kaldi_resnet_amd import features, ingest
    c = corpus
    opts = features.FbankOptions.from_kaldi_config(c["paths"]["fbank.conf"])
    cmn = features.CmnOptions(cmn_window=30)
    arch = {k: torch.from_numpy(np.ascontiguousarray(m.T)).cuda() for k, m in _read_scp(c["feats_scp"]).items()}
    times = []
    loader = ingest.WavTrainLoader(c["paths"]["wav.scp"], c["paths"]["utt2spkid"], 48, 8, opts, cmn, vad_scp=c["vad_scp"], feat_seed=4,
                                   seed=3, threads=2, times=times)
    assert loader.has_speed and loader.pool is not None and [loader.rows[i] for i in range(37)] == [arch[k].shape[1] for k in c["keys"]]
    ref_aug = features.WavAugmentation(loader.table, loader.pool.aug.entries)
    aug_row = c["keys"].index(c["aug_key"])
    differ = n_el = aug_seen = 0
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        draws = list(loader.draws())
        batches = list(loader)
        assert len(batches) == len(draws) == len(loader)
        for (k, sel, r, T, starts), (x, y) in zip(draws, batches):
            assert x.shape == (len(sel), 24, T) and torch.equal(y.cpu(), torch.from_numpy(loader.labels[sel]))
            keep = [j for j, i in enumerate(r) if i != aug_row]
            ref = torch.stack([arch[c["keys"][r[j]]][:, starts[j]:starts[j] + T] for j in keep])
            differ += _ulp_check("epoch %d batch %d" % (epoch, k), x[keep], ref)
            n_el += ref.numel()
            for j in [j for j, i in enumerate(r) if i == aug_row]:
                # the augmented line is applied to the span that is read: features.augment on the span, then the span front end
                p = loader.plan(r[j:j + 1], starts[j:j + 1], T)
                Nmax = int(-(-p.count.max() // 8) * 8)
                pcm = torch.empty(1, Nmax, dtype=torch.int16)
                loader.table.read_span(r[j:j + 1], p.first, p.count, Nmax, pcm)
                w = features.pcm16_to_f32(pcm.cuda(), torch.from_numpy(p.count.astype(np.int32)).cuda())
                rir, noises, names = ref_aug.inputs(r[j:j + 1])
                w, _ = features.augment(w, p.count, rir, noises, quantize=True, sample_rate=FS, names=names)
                nf = p.frame_hi - p.frame_lo
                feats, _, _ = features.fbank_span(w, p.count, p.first, loader.table.nsamp[r[j:j + 1]], p.frame_lo, nf, opts,
                                                  [loader.utt_ids[aug_row]], seed=4)
                rel = np.zeros((1, feats.shape[2]), dtype=np.int32)
                rel[:, :T] = p.rel
                want, _ = features.select_voiced(feats, nf, torch.from_numpy(rel).cuda(), np.full(1, T), cmn)
                _ulp_check("augmented row", x[j:j + 1], want)
                aug_seen += 1
    assert aug_seen >= 1 and any("resample" in t for t in times)
    print("loader with speed lines: %d of %d elements differ from the archive" % (differ, n_el))


def _first_loss(stdout):
    m = re.search(r"Epoch: \[0\]\[\s*0/\s*\d+\].*?Loss (\S+) ", stdout)
    assert m, stdout[-3000:]
    return float(m.group(1))


def test_train_resnet_from_speed_lines_against_the_archive(corpus):
    c = corpus
    d = str(c["dir"])
    clean = os.path.join(d, "clean.feats.scp")           # the archive without the reverberated line (applied to the span, section 6k)
    open(clean, "w").writelines(l for l in open(c["feats_scp"]) if not l.startswith(c["aug_key"] + " "))
    train = ["--utt2spkid", c["paths"]["clean.utt2spkid"], "--cv-list", clean, "--input-dim", "24", "--spk-num", "12", "-a", "resnet18",
             "-b", "8", "--max-chunk-size", "48", "--max-steps", "3", "--epochs", "1", "--no-graph", "--seed", "2", "-j", "1", "--gpu", "0"]
    a = _run("train_resnet.py", train + ["--train-list", clean, "--native-reader", "--log-dir", os.path.join(d, "log_ark")])
    assert a.returncode == 0, a.stdout[-2000:] + a.stderr[-3000:]
    audio = ["--wav-scp", c["paths"]["clean.scp"], "--vad-scp", c["vad_scp"], "--fbank-config", c["paths"]["fbank.conf"], "--cmn-window", "30",
             "--feat-seed", "4"]
    b = _run("train_resnet.py", train + audio + ["--log-dir", os.path.join(d, "log_wav")])
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-3000:]
    la, lb = _first_loss(a.stdout), _first_loss(b.stdout)
    print("first loss: archive %.6e, audio with speed lines %.6e, relative difference %.3g" % (la, lb, abs(la - lb) / abs(la)))
    assert abs(la - lb) <= 1e-4 * abs(la)
