"""Feature front end on the GPU (csrc/frontend.hip through pytorch_kaldi_resnet_amd.features) against the fp64 oracle
tests/frontend_ref.py: fbank and raw log energy on ragged batches of the fixture signals, row / batch invariance with dither on, the
exported dither noise, VAD / sliding CMN / voiced-frame compaction, Frontend + length-masked predict against the CPU oracle model, and
decode.py --wav-scp against compute_fbank.py --egs + decode.py --native-reader --pad-batches."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import frontend_ref as R
from oracle import spk_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB = os.path.join(ROOT, "tests", "golden", "fbank")
CASES = json.load(open(os.path.join(FB, "cases.json")))
EPS_LOG = np.float32(np.log(np.float32(R.FLT_EPSILON)))


def _case(name):
    z = np.load(os.path.join(FB, name + ".npz"))
    return z["wave"].astype(np.float64), json.loads(str(z["options"]))


def _opts(kw, **over):
    from pytorch_kaldi_resnet_amd import features
    d = dict(kw)
    d.update(over)
    return features.FbankOptions(**d)


def _ragged(x):
    """the signal, a prefix of it and a longer version (signal + its reverse): three utterances of different lengths"""
    return [x, x[: int(len(x) * 0.7)], np.concatenate([x, x[::-1]])]


def _batch(waves, nmax=None, rows=None):
    nmax = nmax or max(len(w) for w in waves)
    B = len(waves) if rows is None else max(rows) + 1
    buf = np.zeros((B, nmax), dtype=np.float32)
    rows = rows or list(range(len(waves)))
    n = np.full(B, nmax, dtype=np.int64)
    for r, w in zip(rows, waves):
        buf[r, :len(w)] = w
        n[r] = len(w)
    return torch.from_numpy(buf).cuda(), n


@pytest.mark.parametrize("name", CASES)
def test_fbank_matches_fp64_oracle(name):
    from pytorch_kaldi_resnet_amd import features
    x, kw = _case(name)
    opts = _opts(kw)
    waves = _ragged(x)
    wave_t, n = _batch(waves)
    feats, T, loge = features.fbank(wave_t, n, opts)
    feats, loge = feats.cpu().numpy(), loge.cpu().numpy()
    for b, w in enumerate(waves):
        ref, eref = R.fbank(w, **kw)
        r32, _ = R.fbank(w, dtype=np.float32, **kw)
        assert T[b] == ref.shape[0]
        e32_max, e32_rms = np.abs(r32 - ref).max(), np.sqrt(((r32 - ref) ** 2).mean())
        got = feats[b, :, :T[b]].T
        d = got - ref
        assert np.abs(d).max() <= max(2 * e32_max, 2e-4), (name, b, np.abs(d).max(), e32_max)
        assert np.sqrt((d ** 2).mean()) <= max(2 * e32_rms, 2e-5), (name, b, np.sqrt((d ** 2).mean()), e32_rms)
        assert np.abs(loge[b, :T[b]] - eref).max() <= 1e-5 * np.abs(eref).max()
        assert (feats[b, :, T[b]:] == 0).all() and (loge[b, T[b]:] == 0).all()      # padding is exactly 0
        if opts.energy_floor == 0:
            zero = np.nonzero((np.abs(R.frames(w, opts.frame_len, opts.frame_sh, opts.snip_edges)).max(1) == 0))[0]
            assert zero.size > 0
            assert (got[zero] == EPS_LOG).all() and (loge[b, zero] == EPS_LOG).all()    # digital zero: log(FLT_EPSILON)


@pytest.mark.parametrize("fs", [11025.0, 22050.0])
def test_fbank_other_sample_rates(fs):
    """rates whose LDS span is an odd number of floats ((FT - 1) * S + L: 3685 at 11.025 kHz, 3851 at 22.05 kHz)"""
    from pytorch_kaldi_resnet_amd import features
    x, _ = _case("snip_f80")
    kw = dict(sample_frequency=fs, num_mel_bins=40, dither=0.0, snip_edges=False)
    opts = _opts(kw)
    waves = _ragged(x)
    wave_t, n = _batch(waves)
    feats, T, loge = features.fbank(wave_t, n, opts)
    feats, loge = feats.cpu().numpy(), loge.cpu().numpy()
    for b, w in enumerate(waves):
        ref, eref = R.fbank(w, **kw)
        r32, _ = R.fbank(w, dtype=np.float32, **kw)
        assert T[b] == ref.shape[0]
        d = feats[b, :, :T[b]].T - ref
        assert np.abs(d).max() <= max(2 * np.abs(r32 - ref).max(), 2e-4), (fs, b, np.abs(d).max())
        assert np.sqrt((d ** 2).mean()) <= max(2 * np.sqrt(((r32 - ref) ** 2).mean()), 2e-5)
        assert np.abs(loge[b, :T[b]] - eref).max() <= 1e-5 * np.abs(eref).max()


def test_row_and_batch_invariance_with_dither():
    from pytorch_kaldi_resnet_amd import features
    x, kw = _case("conf16k_f40")
    opts = _opts(kw, dither=1.0)
    others = _ragged(_case("snip_f80")[0])
    w1, n1 = _batch([x, others[0]])
    w2, n2 = _batch([others[1], others[2], x], nmax=len(others[2]) + 5000)
    f1, T1, e1 = features.fbank(w1, n1, opts, utt_ids=[77, 5], seed=3)
    f2, T2, e2 = features.fbank(w2, n2, opts, utt_ids=[9, 8, 77], seed=3, Tcap=int(max(T1.max(), 0) + 400))
    t = T1[0]
    assert T2[2] == t
    assert torch.equal(f1[0, :, :t], f2[2, :, :t]) and torch.equal(e1[0, :t], e2[2, :t])
    f3, _, _ = features.fbank(w1, n1, opts, utt_ids=[77, 5], seed=4)
    assert not torch.equal(f1[0, :, :t], f3[0, :, :t])       # the seed matters


def test_dither_against_oracle_with_exported_noise():
    from pytorch_kaldi_resnet_amd import features
    x, kw = _case("nosnip_f80")
    opts = _opts(kw, dither=1.0)
    w, n = _batch([x])
    f, T, e = features.fbank(w, n, opts, utt_ids=[1234], seed=11)
    noise = features.dither_noise(1234, 11, 0, int(T[0]), opts.frame_len).cpu().numpy().astype(np.float64)
    ref, eref = R.fbank(x, noise=noise, **dict(kw, dither=1.0))
    r32, _ = R.fbank(x, noise=noise, dtype=np.float32, **dict(kw, dither=1.0))
    got = f[0, :, :T[0]].cpu().numpy().T
    e32_max, e32_rms = np.abs(r32 - ref).max(), np.sqrt(((r32 - ref) ** 2).mean())
    assert np.abs(got - ref).max() <= max(2 * e32_max, 2e-4)
    assert np.sqrt(((got - ref) ** 2).mean()) <= max(2 * e32_rms, 2e-5)
    assert np.abs(e[0, :T[0]].cpu().numpy() - eref).max() <= 1e-5 * np.abs(eref).max()
    big = features.dither_noise(99, 1, 0, 2000, 400).cpu().numpy().astype(np.float64).reshape(-1)     # 800 000 draws
    n_ = big.size
    assert abs(big.mean()) < 5 / np.sqrt(n_)
    assert abs(big.var() - 1) < 5 * np.sqrt(2 / n_)
    assert abs(np.corrcoef(big[:-1], big[1:])[0, 1]) < 5 / np.sqrt(n_)
    np.testing.assert_array_equal(features.dither_noise(99, 1, 5, 1, 400).cpu().numpy().reshape(-1), big[5 * 400:6 * 400])


def test_vad_cmn_and_selection():
    from pytorch_kaldi_resnet_amd import features
    x, kw = _case("conf16k_f40")
    opts = _opts(kw, dither=1.0)
    vo = features.VadOptions.from_kaldi_config(os.path.join(FB, "vad.conf"))
    cmn = features.CmnOptions(cmn_window=30)
    long = np.concatenate([x] * 6)                   # 366 frames; the others 61, 50 and 200 (all > W = 30 here; W >= T below)
    silent = np.zeros(8000)
    waves = [long, x, silent, x[: 200 * 160]]
    w, n = _batch(waves)
    ids = [1, 2, 3, 4]
    feats, T, loge = features.fbank(w, n, opts, ids, seed=0)
    v, idx, cnt = features.vad(loge, T, vo)
    v, idx = v.cpu().numpy(), idx.cpu().numpy()
    le = loge.cpu().numpy()
    ff = feats.cpu().numpy()
    cm = features.sliding_cmn(feats, T, cmn).cpu().numpy()
    sel, lengths = features.select_voiced(feats, T, torch.from_numpy(idx).cuda(), cnt, cmn)
    sel = sel.cpu().numpy()
    assert sel.shape[2] == cnt.max()
    for b in range(len(waves)):
        ref_v = R.vad(le[b, :T[b]], vo.vad_energy_threshold, vo.vad_energy_mean_scale, vo.vad_frames_context,
                      vo.vad_proportion_threshold)
        assert np.array_equal(v[b, :T[b]], ref_v), b
        assert (v[b, T[b]:] == 0).all()
        assert cnt[b] == ref_v.sum() == lengths[b]
        ref_c = R.sliding_cmn(ff[b, :, :T[b]].T.astype(np.float64), 30).T
        assert np.abs(cm[b, :, :T[b]] - ref_c).max() <= 1e-5, b
        assert (cm[b, :, T[b]:] == 0).all()
        keep = np.nonzero(ref_v)[0]
        assert np.array_equal(sel[b, :, :cnt[b]], cm[b][:, keep])     # compaction bit-identical to host column selection
        assert (sel[b, :, cnt[b]:] == 0).all()
    assert cnt[2] == 0 and cnt[0] > 0 and cnt[1] > 0               # the all-silent utterance: length 0
    # windows as long as or longer than the utterance: W = 61 = T of row 1, W = 300 > T of rows 1-3 (end clamped to T, start to 0)
    for Wn in (61, 300):
        cw = features.sliding_cmn(feats, T, features.CmnOptions(cmn_window=Wn)).cpu().numpy()
        for b in range(len(waves)):
            ref_c = R.sliding_cmn(ff[b, :, :T[b]].T.astype(np.float64), Wn).T
            assert np.abs(cw[b, :, :T[b]] - ref_c).max() <= 1e-5, (Wn, b)
            assert (cw[b, :, T[b]:] == 0).all()
    fe = features.Frontend(opts, vo, cmn)
    f2, l2 = fe(w, n, ids, 0)
    assert np.array_equal(l2, lengths) and np.array_equal(f2.cpu().numpy(), sel)


def test_frontend_then_masked_predict_matches_oracle():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    x, kw = _case("conf16k_f40")
    opts = _opts(kw, dither=0.0)
    vo = features.VadOptions.from_kaldi_config(os.path.join(FB, "vad.conf"))
    cmn = features.CmnOptions(cmn_window=300)
    y = _case("nosnip_f80")[0]
    waves = [np.concatenate([x] * 4), np.concatenate([y, x, y]), np.concatenate([x, y] * 3)]
    w, n = _batch(waves)
    feats, lengths = features.Frontend(opts, vo, cmn)(w, n, None, 0)
    S, F = 10, 40
    npst = W.make_state(31, S, F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    m = m.cuda().eval()
    with torch.no_grad():
        emb = m.predict(feats, lengths=lengths).cpu().numpy()
    st = O.to_torch_state(npst)
    for b, wv in enumerate(waves):
        f64, e64 = R.fbank(wv, **dict(kw, dither=0.0))
        v = R.vad(e64, vo.vad_energy_threshold, vo.vad_energy_mean_scale, vo.vad_frames_context, vo.vad_proportion_threshold)
        ref_in = R.select_voiced(R.sliding_cmn(f64, 300), v).T.astype(np.float32)
        with torch.no_grad():
            ref = O.embed(st, torch.from_numpy(np.ascontiguousarray(ref_in))[None], "mean+std", "resnet34", train=False).numpy()
        a, r = emb[b].astype(np.float64), ref[0].astype(np.float64)
        cosd = 1 - (a @ r) / (np.linalg.norm(a) * np.linalg.norm(r))
        assert cosd <= 1e-4, (b, cosd, lengths[b], ref_in.shape)


def _write_wavs(d, n=24, seed=3):
    rng = np.random.default_rng(seed)
    x = _case("conf16k_f40")[0]
    y = _case("nosnip_f80")[0]
    lines = []
    for i in range(n):
        parts = [x if rng.random() < 0.5 else y for _ in range(int(rng.integers(2, 7)))]
        s = np.concatenate(parts)[: int(rng.integers(16000, 60000))]
        s = np.clip(s + rng.normal(0, 30, s.size), -32768, 32767).astype(np.int16)
        if i == 5:
            s = np.zeros(20000, dtype=np.int16)        # all silent: skipped
        p = os.path.join(d, "u%02d.wav" % i)
        with wave.open(p, "wb") as wf:
            wf.setnchannels(1)
            wf.setsampwidth(2)
            wf.setframerate(16000)
            wf.writeframes(s.tobytes())
        lines.append("utt%02d %s\n" % (i, p))
    scp = os.path.join(d, "wav.scp")
    open(scp, "w").writelines(lines)
    return scp


def _read_text(path):
    out = {}
    for line in open(path):
        k, rest = line.split(None, 1)
        out[k] = np.array(rest.strip().strip("[]").split(), dtype=np.float64)
    return out


def test_compute_fbank_archives_read_back(tmp_path):
    """compute_fbank.py writes each batch as it comes (batches smaller than the set): feats.scp / vad.scp / utt2num_frames in
    wav.scp order point at matrices equal to the front end run directly"""
    from pytorch_kaldi_resnet_amd import features, kaldi_io
    scp = _write_wavs(str(tmp_path), n=13, seed=8)
    out = str(tmp_path / "fb")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "compute_fbank.py"), scp, out, "--batch-size", "4", "--seed",
                        "5", "--fbank-config", os.path.join(FB, "fbank.conf"), "--vad-config", os.path.join(FB, "vad.conf")],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    keys = [l.split()[0] for l in open(scp)]
    paths = [l.split()[1] for l in open(scp)]
    fscp = [l.split() for l in open(os.path.join(out, "feats.scp"))]
    vscp = [l.split() for l in open(os.path.join(out, "vad.scp"))]
    nfr = [l.split() for l in open(os.path.join(out, "utt2num_frames"))]
    assert [k for k, _ in fscp] == [k for k, _ in vscp] == [k for k, _ in nfr] == keys
    fb, vo, _ = features.options_from_configs(os.path.join(FB, "fbank.conf"), os.path.join(FB, "vad.conf"))
    for i in range(len(keys)):
        with wave.open(paths[i], "rb") as wf:
            s = np.frombuffer(wf.readframes(wf.getnframes()), "<i2").astype(np.float32)
        f, T, e = features.fbank(torch.from_numpy(s)[None].cuda(), [s.size], fb, [features.utt_id(keys[i])], 5)
        v, _, _ = features.vad(e, T, vo)
        m = kaldi_io.read_mat(fscp[i][1])
        assert m.shape == (T[0], fb.num_mel_bins) and int(nfr[i][1]) == T[0]
        assert np.array_equal(m, f[0].cpu().numpy().T)                  # bit-identical: the features do not depend on the batch
        assert np.array_equal(kaldi_io.read_vec_flt(vscp[i][1]), v[0].cpu().numpy().astype(np.float32))


def test_decode_wav_scp_matches_compute_fbank_then_decode(tmp_path):
    """same keys and embeddings; the output ORDER differs by design: --wav-scp sorts its batches by sample count (the voiced frame
    count is known only after the front end), --native-reader --pad-batches by the frame count of the archive"""
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    scp = _write_wavs(str(tmp_path))
    S, F = 10, 40
    npst = W.make_state(41, S, F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    ckpt = str(tmp_path / "model.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 1}, ckpt)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    cfg = ["--fbank-config", os.path.join(FB, "fbank.conf"), "--vad-config", os.path.join(FB, "vad.conf")]
    feats = str(tmp_path / "feats")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "compute_fbank.py"), scp, feats, "--egs", "--cmn-window",
                        "300", "--batch-size", "8"] + cfg, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "utt05" in r.stdout and "no voiced frames" in r.stdout
    base = [sys.executable, os.path.join(ROOT, "scripts", "decode.py"), "--spk_num", str(S), "--arch", "resnet34", "--input-dim",
            str(F), "--pooling", "mean+std", "--model-path", ckpt, "--batch-size", "8"]
    r1 = subprocess.run(base + ["--decode-scp", os.path.join(feats, "feats.scp"), "--out-path", str(tmp_path / "a"),
                                "--native-reader", "--pad-batches"], env=env, capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    r2 = subprocess.run(base + ["--wav-scp", scp, "--out-path", str(tmp_path / "b"), "--cmn-window", "300"] + cfg, env=env,
                        capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert "utt05" in r2.stdout and "no voiced frames" in r2.stdout
    a, b = _read_text(str(tmp_path / "a" / "alone")), _read_text(str(tmp_path / "b" / "alone"))
    assert sorted(a) == sorted(b) == sorted("utt%02d" % i for i in range(24) if i != 5)
    for k in a:
        cosd = 1 - (a[k] @ b[k]) / (np.linalg.norm(a[k]) * np.linalg.norm(b[k]))
        assert cosd <= 1e-6, (k, cosd)
    r3 = subprocess.run(base + ["--wav-scp", scp, "--decode-scp", "x", "--out-path", str(tmp_path / "c")], env=env,
                        capture_output=True, text=True, timeout=300)
    assert r3.returncode != 0 and "mutually exclusive" in r3.stderr
