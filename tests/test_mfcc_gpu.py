"""MFCC front end on the GPU (spk_mfcc_fwd of csrc/frontend.hip through pytorch_kaldi_resnet_amd.features.mfcc) against the fp64
oracle tests/mfcc_ref.py: every fixture case on a ragged batch written into a poisoned buffer, the log energy against the fbank's
bit for bit, the inverse DCT against the fbank's log-mels, dither with the exported noise and its row / batch invariance, digital
zero frames, Frontend + length-masked predict on a 30-dimensional model against the CPU oracle model, and the entry points
scripts/compute_mfcc.py and scripts/decode.py --mfcc-config.

The bounds of the cepstra: max|d| <= max(2 e32_max, 2e-4 g) and rms(d) <= max(2 e32_rms, 2e-5 g), e32 the error of the float32
restatement of the oracle against fp64 on the same input, 2e-4 / 2e-5 the floors of the fbank test (its log-mel values are this
kernel's input), g = 1 + cepstral_lifter / 2 the largest lifter gain (the DCT rows are orthonormal: the lifter is the only gain).
A wrong DCT row, lifter index or row order gives errors of order 1."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import frontend_ref as R
import mfcc_ref as M
from oracle import spk_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MF = os.path.join(ROOT, "tests", "golden", "mfcc")
FB = os.path.join(ROOT, "tests", "golden", "fbank")
CASES = json.load(open(os.path.join(MF, "cases.json")))
EPS_LOG = float(np.log(np.float32(R.FLT_EPSILON)))
CEPSTRAL = ("num_ceps", "cepstral_lifter", "use_energy", "htk_compat")


def _case(name):
    z = np.load(os.path.join(MF, name + ".npz"))
    return z["wave"].astype(np.float64), json.loads(str(z["options"]))


def _ragged(x):
    """the signal, a prefix of it and a longer version (signal + its reverse): three utterances of different lengths"""
    return [x, x[: int(len(x) * 0.7)], np.concatenate([x, x[::-1]])]


def _batch(waves, nmax=None):
    nmax = nmax or max(len(w) for w in waves)
    buf = np.zeros((len(waves), nmax), dtype=np.float32)
    for r, w in enumerate(waves):
        buf[r, :len(w)] = w
    return torch.from_numpy(buf).cuda(), np.asarray([len(w) for w in waves], dtype=np.int64)


def _gain(kw):
    return 1.0 + 0.5 * dict(M.DEFAULTS, **kw)["cepstral_lifter"]


def _bounds(x, kw, noise=None):
    """(fp64 oracle [T, C], its energies, max bound, rms bound) of one utterance"""
    ref, eref = M.mfcc(x, noise=noise, **kw)
    r32, _ = M.mfcc(x, noise=noise, dtype=np.float32, **kw)
    g = _gain(kw)
    e32_max, e32_rms = np.abs(r32 - ref).max(), np.sqrt(((r32 - ref) ** 2).mean())
    return ref, eref, max(2 * e32_max, 2e-4 * g), max(2 * e32_rms, 2e-5 * g)


def _energy_row(kw):
    o = dict(M.DEFAULTS, **kw)
    return o["num_ceps"] - 1 if o["htk_compat"] else 0


@pytest.mark.parametrize("name", CASES)
def test_mfcc_matches_fp64_oracle(name):
    from pytorch_kaldi_resnet_amd import features
    x, kw = _case(name)
    opts = features.MfccOptions(**kw)
    waves = _ragged(x)
    wave_t, n = _batch(waves)
    C = opts.num_ceps
    Tcap = max(opts.num_frames(len(w)) for w in waves) + 3
    out = torch.full((len(waves), C, Tcap), float("nan"), device="cuda")
    feats, T, loge = features.mfcc(wave_t, n, opts, Tcap=Tcap, out=out)
    assert feats.data_ptr() == out.data_ptr()
    feats, loge = feats.cpu().numpy(), loge.cpu().numpy()
    worst = 0.0
    for b, w in enumerate(waves):
        ref, eref, bmax, brms = _bounds(w, kw)
        assert T[b] == ref.shape[0] and ref.shape[1] == C
        got = feats[b, :, :T[b]].T
        d = got - ref
        dmax, drms = np.abs(d).max(), np.sqrt((d ** 2).mean())
        worst = max(worst, dmax / bmax, drms / brms)
        print("%s row %d: max|d| %.3e (bound %.3e) rms %.3e (bound %.3e)" % (name, b, dmax, bmax, drms, brms))
        assert dmax <= bmax, (name, b, dmax, bmax)
        assert drms <= brms, (name, b, drms, brms)
        etol = 1e-5 * np.abs(eref).max()
        assert np.abs(loge[b, :T[b]] - eref).max() <= etol             # written also with use_energy=false: the VAD's input
        if opts.use_energy:
            assert np.array_equal(got[:, _energy_row(kw)], loge[b, :T[b]])
            assert np.abs(got[:, _energy_row(kw)] - eref).max() <= etol
        # padding is exactly 0 in all C rows and the energies (partial last tiles, tiles wholly past the short row): no NaN left
        assert (feats[b, :, T[b]:] == 0).all() and (loge[b, T[b]:] == 0).all()
    assert np.isfinite(feats).all()
    print("%s: largest error over bound %.3f" % (name, worst))


def test_log_energy_is_the_fbanks_bit_for_bit():
    """the same frames, dither draws and energy arithmetic: VAD decisions on either are identical"""
    from pytorch_kaldi_resnet_amd import features
    for name, over in (("conf16k_c40", {}), ("default_c13", dict(energy_floor=3.0)), ("htk_f80_c72", {})):
        x, kw = _case(name)
        fkw = {k: v for k, v in kw.items() if k not in CEPSTRAL}
        waves = _ragged(x)
        wave_t, n = _batch(waves)
        for dither in (0.0, 1.0):
            mo = features.MfccOptions(**dict(kw, dither=dither, **over))
            fo = features.FbankOptions(**dict(fkw, dither=dither, **over))
            _, Tm, em = features.mfcc(wave_t, n, mo, utt_ids=[5, 6, 7], seed=9)
            _, Tf, ef = features.fbank(wave_t, n, fo, utt_ids=[5, 6, 7], seed=9)
            assert np.array_equal(Tm, Tf) and torch.equal(em, ef), (name, dither)
            vo = features.VadOptions.from_kaldi_config(os.path.join(FB, "vad.conf"))
            assert torch.equal(features.vad(em, Tm, vo)[0], features.vad(ef, Tf, vo)[0])


def test_inverse_dct_gives_the_fbank_log_mels():
    """independent of the oracle: C = F, no lifter, no energy, no HTK order - the orthonormal DCT inverted on the host in fp64"""
    from pytorch_kaldi_resnet_amd import features
    x, kw = _case("conf16k_c40")
    kw = dict(kw, cepstral_lifter=0.0, use_energy=False, htk_compat=False)
    fkw = {k: v for k, v in kw.items() if k not in CEPSTRAL}
    mo, fo = features.MfccOptions(**kw), features.FbankOptions(**fkw)
    assert mo.num_ceps == mo.num_mel_bins == 40
    waves = _ragged(x)
    wave_t, n = _batch(waves)
    c, T, _ = features.mfcc(wave_t, n, mo)
    f, Tf, _ = features.fbank(wave_t, n, fo)
    assert np.array_equal(T, Tf)
    D = features.dct_matrix(mo)
    c, f = c.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.float64)
    for b, w in enumerate(waves):
        _, _, bmax, brms = _bounds(w, kw)              # g = 1
        d = D.T @ c[b, :, :T[b]] - f[b, :, :T[b]]
        assert np.abs(d).max() <= bmax, (b, np.abs(d).max(), bmax)
        assert np.sqrt((d ** 2).mean()) <= brms, (b, np.sqrt((d ** 2).mean()), brms)


def test_dither_against_oracle_and_row_batch_invariance():
    from pytorch_kaldi_resnet_amd import features
    x, kw = _case("htk_energy_c30")
    kw = dict(kw, dither=1.0)
    opts = features.MfccOptions(**kw)
    others = _ragged(_case("default_c13")[0])
    w1, n1 = _batch([x, others[0]])
    f1, T1, e1 = features.mfcc(w1, n1, opts, utt_ids=[1234, 5], seed=11)
    t = int(T1[0])
    noise = features.dither_noise(1234, 11, 0, t, opts.frame_len).cpu().numpy().astype(np.float64)
    ref, eref, bmax, brms = _bounds(x, kw, noise=noise)
    d = f1[0, :, :t].cpu().numpy().T - ref
    assert np.abs(d).max() <= bmax, (np.abs(d).max(), bmax)
    assert np.sqrt((d ** 2).mean()) <= brms
    assert np.abs(e1[0, :t].cpu().numpy() - eref).max() <= 1e-5 * np.abs(eref).max()
    # another row, other batch-mates, a longer Nmax and a larger Tcap: the same bits
    w2, n2 = _batch([others[1], others[2], x], nmax=len(others[2]) + 5000)
    f2, T2, e2 = features.mfcc(w2, n2, opts, utt_ids=[9, 8, 1234], seed=11, Tcap=int(T1.max()) + 70)
    assert T2[2] == t
    assert torch.equal(f1[0, :, :t], f2[2, :, :t]) and torch.equal(e1[0, :t], e2[2, :t])
    assert (f2[2, :, t:] == 0).all() and (e2[2, t:] == 0).all()
    f3, _, _ = features.mfcc(w1, n1, opts, utt_ids=[1234, 5], seed=12)
    assert not torch.equal(f1[0, :, :t], f3[0, :, :t])       # the seed matters


def test_digital_zero_frames_and_the_energy_floor():
    from pytorch_kaldi_resnet_amd import features
    x, _ = _case("default_c13")
    sig = np.concatenate([x[:4000], np.zeros(4000), x[:2000]])
    base = dict(sample_frequency=16000.0, dither=0.0, num_mel_bins=24, num_ceps=13)
    wave_t, n = _batch([sig, sig[:7000]])
    L, S = 400, 160
    zero = np.nonzero(np.abs(R.frames(sig, L, S, True)).max(1) == 0)[0]
    assert zero.size >= 10
    c, T, e = features.mfcc(wave_t, n, features.MfccOptions(use_energy=True, energy_floor=1.0, **base))
    c, e = c.cpu().numpy(), e.cpu().numpy()
    assert (c[0, 0, zero] == 0.0).all() and (e[0, zero] == 0.0).all()        # log(1), exactly
    assert (c[0, 0, :T[0]] >= 0.0).all()
    for htk in (False, True):
        kw = dict(base, use_energy=False, htk_compat=htk)
        c, T, e = features.mfcc(wave_t, n, features.MfccOptions(**kw))
        c, e = c.cpu().numpy(), e.cpu().numpy()
        _, _, bmax, _ = _bounds(sig, kw)
        want = np.sqrt(24.0) * EPS_LOG * (np.sqrt(2.0) if htk else 1.0)
        c0 = c[0, 12 if htk else 0, zero]
        assert np.abs(c0 - want).max() <= bmax, (htk, np.abs(c0 - want).max(), bmax)
        rest = np.delete(c[0][:, zero], 12 if htk else 0, axis=0)
        assert np.abs(rest).max() <= bmax                    # a constant log-mel vector has no higher cepstra
        assert (e[0, zero] == np.float32(EPS_LOG)).all()     # no floor: log(FLT_EPSILON)


def test_mfcc_frontend_then_masked_predict_matches_oracle():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    x, y = _case("conf16k_c40")[0], _case("nolifter_c30")[0]
    kw = dict(sample_frequency=16000.0, dither=0.0, num_mel_bins=30, num_ceps=30, snip_edges=False)
    opts = features.MfccOptions(**kw)
    vo = features.VadOptions.from_kaldi_config(os.path.join(FB, "vad.conf"))
    cmn = features.CmnOptions(cmn_window=300)
    waves = [np.concatenate([x] * 4), np.concatenate([y, x, y]), np.concatenate([x, y] * 3)]
    w, n = _batch(waves)
    feats, lengths = features.Frontend(opts, vo, cmn)(w, n, None, 0)
    S, F = 10, 30                                    # map heights 30 -> 15 -> 8 -> 4
    assert feats.shape[1] == F
    npst = W.make_state(31, S, F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    m = m.cuda().eval()
    with torch.no_grad():
        emb = m.predict(feats, lengths=lengths).cpu().numpy()
    st = O.to_torch_state(npst)
    for b, wv in enumerate(waves):
        c64, e64 = M.mfcc(wv, **kw)
        v = R.vad(e64, vo.vad_energy_threshold, vo.vad_energy_mean_scale, vo.vad_frames_context, vo.vad_proportion_threshold)
        ref_in = R.select_voiced(R.sliding_cmn(c64, 300), v).T.astype(np.float32)
        assert lengths[b] == ref_in.shape[1] > 0
        with torch.no_grad():
            ref = O.embed(st, torch.from_numpy(np.ascontiguousarray(ref_in))[None], "mean+std", "resnet34", train=False).numpy()
        a, r = emb[b].astype(np.float64), ref[0].astype(np.float64)
        cosd = 1 - (a @ r) / (np.linalg.norm(a) * np.linalg.norm(r))
        assert cosd <= 1e-4, (b, cosd, lengths[b], ref_in.shape)


# ---- entry points ----
def _write_wavs(d):
    x, y = _case("conf16k_c40")[0], _case("htk_energy_c30")[0]
    rng = np.random.default_rng(4)
    lines, paths = [], []
    for i, s in enumerate((np.concatenate([x, y, x]), np.concatenate([y, y, x, y]), np.concatenate([x, x]))):
        s = np.clip(s + rng.normal(0, 30, s.size), -32768, 32767).astype(np.int16)
        p = os.path.join(d, "u%d.wav" % i)
        with wave.open(p, "wb") as wf:
            wf.setnchannels(1)
            wf.setsampwidth(2)
            wf.setframerate(16000)
            wf.writeframes(s.tobytes())
        lines.append("utt%d %s\n" % (i, p))
        paths.append(p)
    scp = os.path.join(d, "wav.scp")
    open(scp, "w").writelines(lines)
    return scp, ["utt%d" % i for i in range(3)], paths


def _run(script, args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + args, env=env, capture_output=True, text=True,
                          timeout=300)


def _read_wav(path):
    with wave.open(path, "rb") as wf:
        return np.frombuffer(wf.readframes(wf.getnframes()), "<i2").astype(np.float32)


def test_compute_mfcc_archives_read_back(tmp_path):
    """feats / vad archives equal the in-process call bit for bit, --compress archives read back through the native reader as the
    in-process compression of the same features, and vad.ark is compute_fbank.py's byte for byte"""
    from pytorch_kaldi_resnet_amd import features, ingest, kaldi_io
    scp, keys, paths = _write_wavs(str(tmp_path))
    mconf, vconf = os.path.join(MF, "mfcc.conf"), os.path.join(FB, "vad.conf")
    common = ["--vad-config", vconf, "--seed", "5", "--batch-size", "2"]
    plain, comp, fb = str(tmp_path / "mfcc"), str(tmp_path / "mfcc_cm"), str(tmp_path / "fbank")
    for script, out, extra in (("compute_mfcc.py", plain, ["--mfcc-config", mconf]),
                               ("compute_mfcc.py", comp, ["--mfcc-config", mconf, "--compress"]),
                               ("compute_fbank.py", fb, ["--fbank-config", os.path.join(FB, "fbank.conf")])):
        r = _run(script, [scp, out] + common + extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert script[:-3] + ": wrote 3 of 3" in r.stdout
    fscp = [l.split() for l in open(os.path.join(plain, "feats.scp"))]
    cscp = [l.split() for l in open(os.path.join(comp, "feats.scp"))]
    vscp = [l.split() for l in open(os.path.join(plain, "vad.scp"))]
    nfr = [l.split() for l in open(os.path.join(plain, "utt2num_frames"))]
    assert [k for k, _ in fscp] == [k for k, _ in cscp] == [k for k, _ in vscp] == [k for k, _ in nfr] == keys
    mo, vo, _ = features.options_from_configs(vad_config=vconf, mfcc_config=mconf)
    tab = ingest.ArkTable([r for _, r in cscp])
    assert tab.all_cm and (tab.cols == 40).all()
    for i, k in enumerate(keys):
        s = _read_wav(paths[i])
        c, T, e = features.mfcc(torch.from_numpy(s)[None].cuda(), [s.size], mo, [features.utt_id(k)], 5)
        v, _, _ = features.vad(e, T, vo)
        m = kaldi_io.read_mat(fscp[i][1])
        assert m.shape == (T[0], 40) and int(nfr[i][1]) == T[0] == tab.rows[i]
        assert np.array_equal(m, c[0].cpu().numpy().T)
        assert np.array_equal(kaldi_io.read_vec_flt(vscp[i][1]), v[0].cpu().numpy().astype(np.float32))
        mr, hd, cd = features.compress(c, T)
        want = features.decompress(cd, torch.from_numpy(features.column_headers(mr, hd)).cuda(), T).cpu()
        got = tab.read_padded(np.asarray([i]), int(T[0]), torch.empty(1, 40, int(T[0])), 1)
        assert torch.equal(got, want)
        assert np.abs(got[0].numpy().T - m).max() <= (m.max() - m.min()) / 200      # one-byte codes of the same matrix
    assert open(os.path.join(plain, "vad.ark"), "rb").read() == open(os.path.join(fb, "vad.ark"), "rb").read()
    assert [l.split()[1].rsplit(":", 1)[1] for l in open(os.path.join(plain, "vad.scp"))] == \
        [l.split()[1].rsplit(":", 1)[1] for l in open(os.path.join(fb, "vad.scp"))]


def _read_text(path):
    out = {}
    for line in open(path):
        k, rest = line.split(None, 1)
        out[k] = np.array(rest.strip().strip("[]").split(), dtype=np.float64)
    return out


def test_decode_mfcc_config_matches_compute_mfcc_then_decode(tmp_path):
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    scp, keys, _ = _write_wavs(str(tmp_path))
    S, F = 10, 40
    npst = W.make_state(41, S, F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    ckpt = str(tmp_path / "model.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 1}, ckpt)
    cfg = ["--mfcc-config", os.path.join(MF, "mfcc.conf"), "--vad-config", os.path.join(FB, "vad.conf")]
    feats = str(tmp_path / "feats")
    r = _run("compute_mfcc.py", [scp, feats, "--egs", "--cmn-window", "300", "--batch-size", "2"] + cfg)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    base = ["--spk_num", str(S), "--arch", "resnet34", "--pooling", "mean+std", "--model-path", ckpt, "--batch-size", "2"]
    r1 = _run("decode.py", base + ["--input-dim", str(F), "--decode-scp", os.path.join(feats, "feats.scp"), "--out-path",
                                   str(tmp_path / "a"), "--native-reader", "--pad-batches"])
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    r2 = _run("decode.py", base + ["--input-dim", str(F), "--wav-scp", scp, "--out-path", str(tmp_path / "b"), "--cmn-window",
                                   "300"] + cfg)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    a, b = _read_text(str(tmp_path / "a" / "alone")), _read_text(str(tmp_path / "b" / "alone"))
    assert sorted(a) == sorted(b) == keys
    for k in a:
        cosd = 1 - (a[k] @ b[k]) / (np.linalg.norm(a[k]) * np.linalg.norm(b[k]))
        assert cosd <= 1e-6, (k, cosd)
    # refusals, before the model is built
    r3 = _run("decode.py", base + ["--input-dim", str(F), "--wav-scp", scp, "--out-path", str(tmp_path / "c"), "--fbank-config",
                                   os.path.join(FB, "fbank.conf")] + cfg)
    assert r3.returncode != 0 and "mutually exclusive" in r3.stderr
    r4 = _run("decode.py", base + ["--input-dim", "30", "--wav-scp", scp, "--out-path", str(tmp_path / "d")] + cfg)
    assert r4.returncode != 0 and "--input-dim 30" in r4.stderr and "num-ceps 40" in r4.stderr
    assert not os.path.exists(str(tmp_path / "c")) and not os.path.exists(str(tmp_path / "d"))
