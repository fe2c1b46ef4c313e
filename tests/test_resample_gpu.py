"""The GPU resampler (csrc/resample.hip through pytorch_kaldi_resnet_amd.features) against the fp64 oracle tests/resample_ref.py:
every fixture rate pair on a ragged batch, output counts and zero tails, row / batch invariance, the refusals, Frontend with an
input rate and a speed factor, and compute_fbank.py / decode.py with --allow-downsample and --speed.

The accuracy bound is the one test_frontend_gpu.py uses for the fbank: twice the error of the oracle's own float32 run against
its fp64 run on the same input (the kernel is a different but equally long fp32 summation; FMA contraction only helps).  No
absolute floor is needed: where the input is all zero the float32 oracle and the kernel both give exact zeros, and the bound is
taken over a whole utterance, which always holds signal."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import frontend_ref as R
import resample_ref as RS
from oracle import weights as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GR = os.path.join(ROOT, "tests", "golden", "resample")
FB = os.path.join(ROOT, "tests", "golden", "fbank")
CASES = json.load(open(os.path.join(GR, "cases.json")))


def _case(c):
    return np.load(os.path.join(GR, c["name"] + ".npz"))["wave"].astype(np.float64)


def _batch(waves, nmax=None, rows=None, fill=0.0):
    """rows of a [B, nmax] float32 batch; everything that is not signal holds `fill`"""
    nmax = nmax or max(len(w) for w in waves)
    rows = rows or list(range(len(waves)))
    B = max(rows) + 1
    buf = np.full((B, nmax), fill, dtype=np.float32)
    n = np.full(B, nmax, dtype=np.int64)
    for r, w in zip(rows, waves):
        buf[r, :len(w)] = w
        n[r] = len(w)
    return torch.from_numpy(buf).cuda(), n


def _ragged(x):
    """the case, two truncated copies and a longer one - rows long enough for the float32 yardstick (see _TINY)"""
    return [x, x[: int(len(x) * 0.63)], x[: int(len(x) * 0.31)], np.concatenate([x, x[::-1], x])]


# Rows of a few samples (shorter than the filter, a single sample) ride in the same batch.  The float32 yardstick compares the
# maxima of two different realisations of rounding error, which means something over hundreds of outputs and nothing over the 1 - 8
# outputs such a row has; these rows get the a-priori bound of a K-term float32 dot product instead (Higham, Accuracy and Stability
# of Numerical Algorithms, section 3.1: |error| <= gamma_K sum |w_k x_k|, in any summation order and with or without FMA), plus one
# unit roundoff for the table's rounding to float32: (K + 1) u sum_k |w_k x_k| / (1 - (K + 1) u), u = 2^-24.
_TINY = [1, 7]


def _abs_sum(x, fi, fo):
    """sum_k |w[p][k] x[.]| per output"""
    iu, ou, K, first, w = RS.tables(fi, fo)
    n_out = RS.num_resampled(len(x), fi, fo)
    out = np.zeros(n_out)
    for j in range(n_out):
        idx = first[j % ou] + (j // ou) * iu + np.arange(K)
        ok = (idx >= 0) & (idx < len(x))
        out[j] = (np.abs(w[j % ou][ok]) * np.abs(x[idx[ok]])).sum()
    return out, K


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_resample_matches_fp64_oracle(c):
    from pytorch_kaldi_resnet_amd import features
    fi, fo = c["fi"], c["fo"]
    x = _case(c)
    waves = _ragged(x) + [x[100:100 + m] for m in _TINY]
    # 37 extra columns of padding that hold garbage: samples past a row's count must not be read as signal
    wave_t, n = _batch(waves, nmax=max(len(w) for w in waves) + 37, fill=12345.0)
    out, n_out = features.resample(wave_t, n, fi, fo)
    out = out.cpu().numpy()
    assert out.shape == (len(waves), n_out.max())
    for b, w in enumerate(waves):
        ref = RS.resample(w, fi, fo)
        assert n_out[b] == len(ref) == RS.num_resampled(len(w), fi, fo) == features.num_resampled(len(w), fi, fo)
        assert (out[b, n_out[b]:] == 0).all()                   # exactly 0 past the row's count
        d = out[b, :n_out[b]] - ref
        if len(w) in _TINY:
            s, K = _abs_sum(w, fi, fo)
            u = 2.0 ** -24
            bound = (K + 1) * u / (1 - (K + 1) * u) * s
            print(c["name"], b, len(w), "tiny: max |d| / bound", (np.abs(d) / bound).max())
            assert len(ref) < 64 and (np.abs(d) <= bound).all(), (c["name"], b, np.abs(d), bound)
            continue
        r32 = RS.resample(w, fi, fo, dtype=np.float32)
        e32_max, e32_rms = np.abs(r32 - ref).max(), np.sqrt(((r32 - ref) ** 2).mean())
        print(c["name"], b, len(w), "max", np.abs(d).max(), "e32_max", e32_max, "rms", np.sqrt((d ** 2).mean()), "e32_rms", e32_rms,
              "scale", np.abs(ref).max())
        assert len(ref) >= 256
        assert np.abs(d).max() <= 2 * e32_max, (c["name"], b, np.abs(d).max(), e32_max)
        assert np.sqrt((d ** 2).mean()) <= 2 * e32_rms, (c["name"], b, np.sqrt((d ** 2).mean()), e32_rms)


def test_nsamp_out_on_device_and_zero_tail():
    """the kernel writes its own counts (device int32) and zeros up to the Nmax_out it is given, whatever the buffers held"""
    from pytorch_kaldi_resnet_amd import features, hip
    fi, fo = 44100, 16000
    rng = np.random.default_rng(0)
    lens = [5003, 441, 1, 4410, 3000]
    waves = [rng.integers(-20000, 20000, n).astype(np.float64) for n in lens]
    wave_t, n = _batch(waves, nmax=6000, fill=-777.0)
    iu, ou, K, first, w = features.resample_tables(fi, fo, wave_t.device)
    tab = features._resample_cached(fi, fo, wave_t.device)
    Nout = 2500
    out = torch.full((len(lens), Nout), 99.0, device="cuda")
    nd = torch.full((len(lens),), -1, dtype=torch.int32, device="cuda")
    ns = torch.from_numpy(n.astype(np.int32)).cuda()
    hip.call("spk_resample_fwd", hip.ptr(wave_t), hip.ptr(ns), len(lens), 6000, hip.ptr(tab.first_dev), hip.ptr(tab.wq_dev), fi, fo,
             K, hip.ptr(out), hip.ptr(nd), Nout, hip.stream())
    want = np.array([features.num_resampled(v, fi, fo) for v in lens])
    assert np.array_equal(nd.cpu().numpy(), want)
    o = out.cpu().numpy()
    for b in range(len(lens)):
        assert (o[b, want[b]:] == 0).all() and np.abs(o[b, :want[b]]).max() > 0
    o2, n2 = features.resample(wave_t, n, fi, fo)
    assert np.array_equal(n2, want)
    for b in range(len(lens)):
        assert np.array_equal(o2.cpu().numpy()[b, :want[b]], o[b, :want[b]])


@pytest.mark.parametrize("fi,fo", [(44100, 16000), (11025, 16000), (14400, 16000), (48000, 16000)])
def test_row_batch_invariance(fi, fo):
    """an utterance's output does not depend on its row, the batch around it, Nmax or what the padding holds - bit for bit"""
    from pytorch_kaldi_resnet_amd import features
    rng = np.random.default_rng(fi)
    x = rng.integers(-30000, 30000, 23457).astype(np.float64)
    others = [rng.integers(-30000, 30000, n).astype(np.float64) for n in (30011, 999, 12000)]
    a, na = features.resample(*_batch([x]), fi, fo)
    wb, nb = _batch(others[:2] + [x] + others[2:], nmax=31003, fill=555.0)
    b, nob = features.resample(wb, nb, fi, fo)
    wc, nc = _batch([x, others[1]], nmax=23459, rows=[3, 0], fill=-1.0)
    c, noc = features.resample(wc, nc, fi, fo)
    assert na[0] == nob[2] == noc[3]
    a0 = a[0, :na[0]].cpu().numpy()
    assert np.array_equal(a0, b[2, :na[0]].cpu().numpy())
    assert np.array_equal(a0, c[3, :na[0]].cpu().numpy())
    # a view that does not start on a 16-byte boundary takes the element-load path: same values
    wd = torch.as_strided(torch.zeros(23457 + 1, device="cuda"), (1, 23457), (23457, 1), 1)
    wd.copy_(torch.from_numpy(x.astype(np.float32))[None])
    assert wd.data_ptr() % 16 != 0 and wd.is_contiguous()
    d, nd = features.resample(wd, [23457], fi, fo)
    assert np.array_equal(a0, d[0, :nd[0]].cpu().numpy())


def test_equal_rates_and_refusals():
    from pytorch_kaldi_resnet_amd import features, hip
    w, n = _batch([np.arange(100.0)])
    o, no = features.resample(w, n, 16000, 16000)
    assert o is w and no is n                              # equal rates: not a launch
    # 44100 -> 22051: gcd 1, 22 051 phases - refused by the host before any launch, naming the pair
    with pytest.raises(ValueError, match=r"44100 -> 22051"):
        features.resample(w, n, 44100, 22051)
    # ... and by the library's own check, should a caller go past the Python layer (dummy tables: nothing is launched)
    dummy_i = torch.zeros(8, dtype=torch.int32, device="cuda")
    dummy_f = torch.zeros(8, device="cuda")
    out = torch.full((1, 64), 7.0, device="cuda")
    with pytest.raises(RuntimeError, match=r"44100 -> 22051"):
        hip.call("spk_resample_fwd", hip.ptr(w), hip.ptr(dummy_i), 1, 100, hip.ptr(dummy_i), hip.ptr(dummy_f), 44100, 22051, 25,
                 hip.ptr(out), hip.ptr(dummy_i), 64, hip.stream())
    torch.cuda.synchronize()
    assert (out == 7.0).all()                              # nothing ran
    assert hip.lib().spk_resample_tile(44100, 22051, 25) == 0 and hip.lib().spk_resample_tile(441, 160, 34) > 0
    with pytest.raises(ValueError, match="float32 cuda"):
        features.resample(w.cpu(), n, 44100, 16000)
    with pytest.raises(ValueError, match="float32 cuda"):
        features.resample(w.double(), n, 44100, 16000)
    with pytest.raises(ValueError, match="float32 cuda"):
        features.resample(w[0], n, 44100, 16000)
    with pytest.raises(ValueError, match="2 sample counts for 1 rows"):
        features.resample(w, [100, 100], 44100, 16000)
    with pytest.raises(ValueError, match="row 0 has 101 samples"):
        features.resample(w, [101], 44100, 16000)
    with pytest.raises(ValueError, match="row 0 has 0 samples"):
        features.resample(w, [0], 44100, 16000)
    with pytest.raises(ValueError, match="whole number of Hz"):
        features.resample(w, n, 44100.5, 16000)


def _long_signal(rate_case, reps, seed):
    """a few of the fixture signals of one rate in a row, with a little noise so that no two utterances are equal"""
    rng = np.random.default_rng(seed)
    cs = [c for c in CASES if c["fi"] == rate_case]
    x = np.concatenate([_case(cs[int(rng.integers(len(cs)))]) for _ in range(reps)])
    return np.clip(np.round(x + rng.normal(0, 30, x.size)), -32768, 32767)


def test_frontend_input_rate_and_speed():
    """Frontend(input_rate=44100) is fbank(resample(...)) bit for bit, and stays within the fbank's own bound of the fp64 oracle of
    both steps; a speed factor is one more resampling ratio"""
    from pytorch_kaldi_resnet_amd import features
    kw = json.loads(str(np.load(os.path.join(FB, "conf16k_f40.npz"))["options"]))
    opts = features.FbankOptions(**kw)
    waves = [_long_signal(44100, 6, 1), _long_signal(44100, 4, 2), _long_signal(44100, 9, 3)]
    wave_t, n = _batch(waves)
    fe = features.Frontend(opts, input_rate=44100)
    feats, T = fe(wave_t, n)
    r, nr = features.resample(wave_t, n, 44100, 16000)
    f2, T2, _ = features.fbank(r, nr, opts)
    assert np.array_equal(T, T2) and torch.equal(feats, f2)
    f3, T3 = features.Frontend(opts)(wave_t, n, input_rate=44100)           # the rate given per call
    assert np.array_equal(T, T3) and torch.equal(feats, f3)
    feats = feats.cpu().numpy()
    for b, w in enumerate(waves):
        ref, _ = R.fbank(RS.resample(w, 44100, 16000), **kw)
        r32, _ = R.fbank(RS.resample(w, 44100, 16000, dtype=np.float32), dtype=np.float32, **kw)
        assert T[b] == ref.shape[0] == opts.num_frames(features.num_resampled(len(w), 44100, 16000))
        e32_max, e32_rms = np.abs(r32 - ref).max(), np.sqrt(((r32 - ref) ** 2).mean())
        d = feats[b, :, :T[b]].T - ref
        print("frontend 44100", b, "max", np.abs(d).max(), "e32_max", e32_max, "rms", np.sqrt((d ** 2).mean()), "e32_rms", e32_rms)
        assert np.abs(d).max() <= max(2 * e32_max, 2e-4), (b, np.abs(d).max(), e32_max)
        assert np.sqrt((d ** 2).mean()) <= max(2 * e32_rms, 2e-5), (b, np.sqrt((d ** 2).mean()), e32_rms)
    # speed 0.9 on 16 kHz audio: 14400 -> 16000, 1 / 0.9 times as long; combined with an input rate of 48 kHz (the same samples,
    # declared as such): 43200 -> 16000, one launch
    x16 = [_long_signal(16000, 5, 4), _long_signal(16000, 3, 5)]
    w16, n16 = _batch(x16)
    fs, Ts = features.Frontend(opts, speed="0.9")(w16, n16)
    rs_, nrs = features.resample(w16, n16, 14400, 16000)
    assert np.array_equal(nrs, [-(-len(w) * 10 // 9) for w in x16])
    f4, T4, _ = features.fbank(rs_, nrs, opts)
    assert np.array_equal(Ts, T4) and torch.equal(fs, f4)
    fc, Tc = features.Frontend(opts, input_rate=48000, speed="0.9")(wave_t, n)
    rc, nrc = features.resample(wave_t, n, 43200, 16000)
    f5, T5, _ = features.fbank(rc, nrc, opts)
    assert np.array_equal(Tc, T5) and torch.equal(fc, f5)
    # 44100 x 0.9 = 39690 -> 16000 has a common divisor of 10 only: 1 600 phases, beyond the LDS budget - refused, not approximated
    with pytest.raises(ValueError, match=r"39690 -> 16000"):
        features.Frontend(opts, input_rate=44100, speed="0.9")(wave_t, n)
    # defaults: today's behaviour, no resampling
    f0, T0 = features.Frontend(opts)(w16, n16)
    f6, T6, _ = features.fbank(w16, n16, opts)
    assert np.array_equal(T0, T6) and torch.equal(f0, f6)


def _write_wavs(d, rate, n, seed, silent=None):
    rng = np.random.default_rng(seed)
    lines, sig = [], {}
    for i in range(n):
        s = _long_signal(rate, int(rng.integers(14, 24)), seed * 100 + i)
        s = s[: int(rng.integers(int(1.0 * rate), len(s)))].astype(np.int16)
        if i == silent:
            s = np.zeros(int(1.2 * rate), dtype=np.int16)
        p = os.path.join(d, "u%02d.wav" % i)
        with wave.open(p, "wb") as wf:
            wf.setnchannels(1)
            wf.setsampwidth(2)
            wf.setframerate(rate)
            wf.writeframes(s.tobytes())
        lines.append("utt%02d %s\n" % (i, p))
        sig["utt%02d" % i] = s.astype(np.float32)
    scp = os.path.join(d, "wav.scp")
    open(scp, "w").writelines(lines)
    return scp, sig


def _run(cmd, **kw):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    return subprocess.run([sys.executable] + cmd, env=env, capture_output=True, text=True, timeout=300, **kw)


CFG = ["--fbank-config", os.path.join(FB, "fbank.conf"), "--vad-config", os.path.join(FB, "vad.conf")]


def test_compute_fbank_allow_downsample(tmp_path):
    """44.1 kHz files: refused without the flag (naming the file), with it the archives equal the functional API bit for bit"""
    from pytorch_kaldi_resnet_amd import features, kaldi_io
    scp, sig = _write_wavs(str(tmp_path), 44100, 9, 11)
    out = str(tmp_path / "fb")
    script = os.path.join(ROOT, "scripts", "compute_fbank.py")
    r = _run([script, scp, out, "--batch-size", "4"] + CFG)
    assert r.returncode != 0 and "u00.wav" in r.stderr and "--allow-downsample" in r.stderr
    r = _run([script, scp, out, "--batch-size", "4", "--allow-upsample"] + CFG)
    assert r.returncode != 0 and "u00.wav" in r.stderr
    r = _run([script, scp, out, "--batch-size", "4", "--seed", "5", "--allow-downsample"] + CFG)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    fb, vo, _ = features.options_from_configs(os.path.join(FB, "fbank.conf"), os.path.join(FB, "vad.conf"))
    fscp = [l.split() for l in open(os.path.join(out, "feats.scp"))]
    vscp = [l.split() for l in open(os.path.join(out, "vad.scp"))]
    nfr = dict(l.split() for l in open(os.path.join(out, "utt2num_frames")))
    assert [k for k, _ in fscp] == [k for k, _ in vscp] == list(sig)
    for (k, loc), (_, vloc) in zip(fscp, vscp):
        s = sig[k]
        w, nw = features.resample(torch.from_numpy(s)[None].cuda(), [s.size], 44100, 16000)
        f, T, e = features.fbank(w, nw, fb, [features.utt_id(k)], 5)
        v, _, _ = features.vad(e, T, vo)
        m = kaldi_io.read_mat(loc)
        assert int(nfr[k]) == T[0] == fb.num_frames(features.num_resampled(s.size, 44100, 16000)) == m.shape[0]
        assert np.array_equal(m, f[0].cpu().numpy().T)
        assert np.array_equal(kaldi_io.read_vec_flt(vloc), v[0].cpu().numpy().astype(np.float32))


def test_compute_fbank_speed(tmp_path):
    """--speed 0.9 --utt2spk on 16 kHz files: sp0.9- keys, the side files of perturb_data_dir_speed.sh, features of the audio
    resampled 14400 -> 16000 with the dither of the written key"""
    from pytorch_kaldi_resnet_amd import features, kaldi_io
    scp, sig = _write_wavs(str(tmp_path), 16000, 7, 12)
    u2s = str(tmp_path / "utt2spk")
    open(u2s, "w").writelines("%s spk%d\n" % (k, i % 3) for i, k in enumerate(sig))
    out = str(tmp_path / "sp")
    script = os.path.join(ROOT, "scripts", "compute_fbank.py")
    r = _run([script, scp, out, "--speed", "1.0"] + CFG)
    assert r.returncode != 0 and "no perturbation" in r.stderr
    r = _run([script, scp, out, "--utt2spk", u2s] + CFG)
    assert r.returncode != 0 and "--utt2spk needs --speed" in r.stderr
    r = _run([script, scp, out, "--batch-size", "3", "--seed", "2", "--speed", "0.9", "--utt2spk", u2s] + CFG)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    fb, vo, _ = features.options_from_configs(os.path.join(FB, "fbank.conf"), os.path.join(FB, "vad.conf"))
    fscp = [l.split() for l in open(os.path.join(out, "feats.scp"))]
    nfr = dict(l.split() for l in open(os.path.join(out, "utt2num_frames")))
    assert [k for k, _ in fscp] == ["sp0.9-" + k for k in sig] == list(nfr)
    assert open(os.path.join(out, "utt2spk")).read() == "".join("sp0.9-%s sp0.9-spk%d\n" % (k, i % 3) for i, k in enumerate(sig))
    assert open(os.path.join(out, "utt2uniq")).read() == "".join("sp0.9-%s %s\n" % (k, k) for k in sig)
    for (k, loc), orig in zip(fscp, sig):
        s = sig[orig]
        w, nw = features.resample(torch.from_numpy(s)[None].cuda(), [s.size], 14400, 16000)
        assert nw[0] == -(-s.size * 10 // 9)
        f, T, e = features.fbank(w, nw, fb, [features.utt_id(k)], 2)             # the dither of the WRITTEN key
        m = kaldi_io.read_mat(loc)
        assert int(nfr[k]) == T[0] == fb.num_frames(features.num_resampled(s.size, 14400, 16000)) == m.shape[0]
        assert np.array_equal(m, f[0].cpu().numpy().T)
        f0, _, _ = features.fbank(w, nw, fb, [features.utt_id(orig)], 2)
        assert not np.array_equal(m, f0[0].cpu().numpy().T)                      # another key, another noise


def _read_text(path):
    out = {}
    for line in open(path):
        k, rest = line.split(None, 1)
        out[k] = np.array(rest.strip().strip("[]").split(), dtype=np.float64)
    return out


def test_decode_wav_scp_allow_downsample(tmp_path):
    """decode.py --wav-scp --allow-downsample on 44.1 kHz files equals compute_fbank.py --egs --allow-downsample followed by decode.py
    on the archives (same keys and embeddings; the order differs by design, as at 16 kHz)"""
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    scp, sig = _write_wavs(str(tmp_path), 44100, 12, 13, silent=5)
    S, F = 10, 40
    npst = W.make_state(41, S, F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    ckpt = str(tmp_path / "model.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 1}, ckpt)
    feats = str(tmp_path / "feats")
    r = _run([os.path.join(ROOT, "scripts", "compute_fbank.py"), scp, feats, "--egs", "--cmn-window", "300", "--batch-size", "8",
              "--allow-downsample"] + CFG)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "utt05" in r.stdout and "no voiced frames" in r.stdout
    base = [os.path.join(ROOT, "scripts", "decode.py"), "--spk_num", str(S), "--arch", "resnet34", "--input-dim", str(F), "--pooling",
            "mean+std", "--model-path", ckpt, "--batch-size", "8"]
    r1 = _run(base + ["--decode-scp", os.path.join(feats, "feats.scp"), "--out-path", str(tmp_path / "a"), "--native-reader",
                      "--pad-batches"])
    assert r1.returncode == 0, r1.stdout[-2000:] + r1.stderr[-2000:]
    r2 = _run(base + ["--wav-scp", scp, "--out-path", str(tmp_path / "b"), "--cmn-window", "300", "--allow-downsample"] + CFG)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert "utt05" in r2.stdout and "no voiced frames" in r2.stdout
    a, b = _read_text(str(tmp_path / "a" / "alone")), _read_text(str(tmp_path / "b" / "alone"))
    assert sorted(a) == sorted(b) == sorted(k for k in sig if k != "utt05")
    for k in a:
        cosd = 1 - (a[k] @ b[k]) / (np.linalg.norm(a[k]) * np.linalg.norm(b[k]))
        assert cosd <= 1e-6, (k, cosd)
    r3 = _run(base + ["--wav-scp", scp, "--out-path", str(tmp_path / "c"), "--cmn-window", "300"] + CFG)
    assert r3.returncode != 0 and "u00.wav" in r3.stderr and "above sample_frequency" in r3.stderr
    r4 = _run(base + ["--decode-scp", os.path.join(feats, "feats.scp"), "--out-path", str(tmp_path / "d"), "--allow-downsample"])
    assert r4.returncode != 0 and "need --wav-scp" in r4.stderr
