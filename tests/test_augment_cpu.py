"""Augmentation without a GPU: the fp64 oracle tests/augment_ref.py against independent code (scipy's FFT convolution, numpy's
convolve, SNRs measured on its output), its edge cases, its float32 restatement of the kernel's arithmetic, the grammar of
features.parse_wav_entry against entries built with the format strings of the recipe's two scripts, wav_scp_batches on augmented
entries, and the argument errors of scripts/compute_fbank.py."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import scipy.signal

import augment_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000


# ---- the oracle against independent code ----
@pytest.mark.parametrize("n,r", [(4000, 1), (3000, 700), (9000, 3300), (1500, 5000)])
def test_oracle_convolution_is_the_convolution(n, r):
    x, h = A.speech(n, 1).astype(np.float64), A.impulse_response(0.4, 2)[:r].astype(np.float64)
    y = A.convolve(x, h)
    assert len(y) == n + r - 1
    for other in (scipy.signal.fftconvolve(x, h), np.convolve(x, h)):
        err = np.abs(y - other).max() / np.abs(y).max()
        print(n, r, "%.2e" % err)
        assert err <= 1e-12
    # the float32 restatement of the kernel: a float32 computation, close to fp64 but not equal to it
    y32 = A.conv32(x, h)
    assert y32.dtype == np.float32 and len(y32) == len(y)
    assert 0 < np.abs(y32 - y).max() <= 1e-5 * np.abs(y).max()


def test_requested_snr_is_the_measured_snr():
    x = A.speech(20000, 3)
    for snr in (15.0, 0.0, -3.5):
        d = {}
        A.augment(x, None, [(A.noise(7000, 4), len(x) / FS, 0.0, snr)], detail=d)
        added = d["y"] - x.astype(np.float64)
        measured = 10 * np.log10((x.astype(np.float64) ** 2).mean() / (added ** 2).mean())
        print(snr, measured)
        assert abs(measured - snr) <= 1e-9


def test_snr_with_reverberation_refers_to_the_early_energy():
    x, h = A.speech(12000, 5), A.impulse_response(0.4, 6)
    s, e0, e1 = A.early_window(h, FS)
    assert s == 48 and e0 == 32 and e1 == 848
    early = (scipy.signal.fftconvolve(x.astype(np.float64), h[e0:e1].astype(np.float64)) ** 2).mean()
    d = {}
    A.augment(x, h, [(A.noise(5000, 7), None, 0.1, 10.0), (A.noise(30000, 8), 0.5, 0.0, 5.0)], detail=d)
    for a, q, snr in zip(d["a"], d["q"], (10.0, 5.0)):
        assert abs(a * a * q * 10 ** (snr / 10) / early - 1) <= 1e-12
    assert abs(d["p_sig"] / early - 1) <= 1e-12


def test_output_power_is_the_input_power():
    x, h = A.speech(12000, 9), A.impulse_response(0.3, 10)
    for rir, noises in ((h, []), (None, [(A.noise(3000, 11), None, 0.2, 3.0)]), (h, [(A.noise(3000, 11), 2.0, 0.0, 8.0)])):
        d = {}
        out = A.augment(x, rir, noises, detail=d)
        assert d["M"] == len(x) + (len(h) - 1 if rir is not None else 0) and len(out) == len(x)
        assert abs(((d["g"] * d["y"]) ** 2).sum() / d["M"] / d["p_before"] - 1) <= 1e-12
        assert np.array_equal(out, d["g"] * d["y"][d["s"]:d["s"] + len(x)])


def test_peak_is_the_first_signed_maximum():
    h = A.impulse_response(0.25, 12, negative_larger=True)
    assert np.abs(h).argmax() == 53 and h[53] < 0
    assert A.early_window(h, FS) == (48, 32, 848)
    h2 = h.copy()
    h2[200] = h2[48]                                       # a second, equal maximum: the first one counts
    assert A.early_window(h2, FS)[0] == 48
    assert A.early_window(h[:500], FS) == (48, 32, 500)    # the window stops at the end
    assert A.early_window(h[40:], FS) == (8, 0, 808)       # ... and at the start


def test_edge_cases():
    x = A.speech(8000, 13)
    x64 = x.astype(np.float64)
    nz = A.noise(3000, 14)
    # a start past the end adds nothing; without anything added the gain is 1
    assert np.array_equal(A.augment(x, None, [(nz, None, 0.5, 0.0)]), x64)
    assert np.array_equal(A.augment(x, None, [(nz, None, 7.0, 0.0)]), x64)
    # a noise longer than the remainder is cut
    d = {}
    A.augment(x, None, [(nz, None, 0.4, 0.0)], detail=d)
    added = d["y"] - x64
    assert not added[:6400].any() and np.allclose(added[6400:], d["a"][0] * nz[:1600], rtol=0, atol=1e-9) and added[6400:].any()
    # --duration: repeats the signal to fill, or trims it; the power is that of what is added
    assert np.array_equal(A.fill(nz, 0.5, FS), np.concatenate([nz, nz, nz[:2000]]))
    assert np.array_equal(A.fill(nz, 0.1, FS), nz[:1600])
    assert A.fill(nz, None, FS) is nz
    d = {}
    A.augment(x, None, [(nz, 0.1, 0.0, 0.0)], detail=d)
    assert d["q"][0] == (nz[:1600].astype(np.float64) ** 2).mean()
    assert not (d["y"] - x64)[1600:].any()
    # h = delta at s: the input comes back, shifted back by s.  A one-tap h returns it as it is; behind a longer h the same
    # energy is spread over M = N + R - 1 samples, so the contract's divisor M scales it by sqrt(M / N) - nothing else changes
    assert np.allclose(A.augment(x, np.ones(1, dtype=np.float32)), x64, rtol=1e-15, atol=0)
    for s in (0, 37):
        h = np.zeros(300, dtype=np.float32)
        h[s] = 1.0
        k = np.sqrt((8000 + 299) / 8000)
        assert np.allclose(A.augment(x, h), k * x64, rtol=1e-13, atol=0)
        assert np.allclose(A.augment(x, 0.25 * h), k * x64, rtol=1e-13, atol=0)          # the scale of h cancels in g
    # quantisation: truncation toward zero, clipping, the count
    out, clipped = A.augment(np.array([1.9, -1.9, 40000.0, -40000.0, 32767.9, -32768.9], dtype=np.float32), quantize=True)
    assert list(out) == [1, -1, 32767, -32768, 32767, -32768] and clipped == 2


def test_float32_restatement_follows_the_oracle():
    x, h = A.speech(9000, 15), A.impulse_response(0.3, 16)
    noises = [(A.noise(2500, 17), None, 0.1, 12.0), (A.noise(2500, 18), 0.5, 0.0, 6.0)]
    for rir, nz in ((h, noises), (None, noises), (h, []), (None, [])):
        ref, r32 = A.augment(x, rir, nz), A.augment32(x, rir, nz)
        assert r32.dtype == np.float32 and np.abs(r32 - ref).max() <= 1e-5 * np.abs(ref).max()
    assert np.array_equal(A.augment32(x), x)


# ---- the grammar: entries as the recipe's scripts format them (the format strings are data copied from the scripts) ----
RVB_ENTRY = "{0} wav-reverberate --shift-output={1} {2} - - |"          # reverberate_data_dir.py:365
RVB_CAT = "cat {0} |"                                                   # reverberate_data_dir.py:345
RVB_IR = '--impulse-response="{0}" '                                    # reverberate_data_dir.py:262
RVB_ADD = "--additive-signals='{0}' "                                   # reverberate_data_dir.py:292-294
RVB_START = "--start-times='{0}' "
RVB_SNR = "--snrs='{0}' "


def _augment_data_dir_entry(wav, items, starts, snrs):
    """AugmentWav of augment_data_dir.py:103-118, from its lists"""
    start_times_str = "--start-times='" + ",".join([str(i) for i in starts]) + "'"
    snrs_str = "--snrs='" + ",".join([str(i) for i in snrs]) + "'"
    noises_str = "--additive-signals='" + ",".join(items).strip() + "'"
    if wav.strip()[-1] != "|":
        return "wav-reverberate --shift-output=true " + noises_str + " " + start_times_str + " " + snrs_str + " " + wav + " - |"
    return wav + " wav-reverberate --shift-output=true " + noises_str + " " + start_times_str + " " + snrs_str + " - - |"


def _bg(dur, path, quotes=True):
    q = '"' if quotes else ""
    return "wav-reverberate --duration=" + str(dur) + " " + q + path + q + " - |"       # augment_data_dir.py:87-88


def test_accepted_entry_shapes():
    from pytorch_kaldi_resnet_amd import features
    e = features.parse_wav_entry("/data/vox/id1/a.wav")
    assert e == features.WavEntry("/data/vox/id1/a.wav", None, [], False) and not e.augmented
    e = features.parse_wav_entry(RVB_ENTRY.format(RVB_CAT.format("/d/a.wav"), "true", RVB_IR.format("/rirs/small/Room001-00001.wav")))
    assert e == features.WavEntry("/d/a.wav", "/rirs/small/Room001-00001.wav", [], True)
    opts = RVB_IR.format("r.wav") + RVB_ADD.format("n1.wav,n2.wav") + RVB_START.format("0,1.5") + RVB_SNR.format("20,10")
    e = features.parse_wav_entry(RVB_ENTRY.format(RVB_CAT.format("a.wav"), "true", opts))
    assert e == features.WavEntry("a.wav", "r.wav", [("n1.wav", None, 0.0, 20.0), ("n2.wav", None, 1.5, 10.0)], True)
    # noise set: foreground noises every few seconds
    e = features.parse_wav_entry(_augment_data_dir_entry("/d/a.wav", ["/musan/noise/free-sound/noise-free-sound-0000.wav",
                                                                     "/musan/noise/n2.wav"], [0, 6.25], [15, 0]))
    assert e == features.WavEntry("/d/a.wav", None, [("/musan/noise/free-sound/noise-free-sound-0000.wav", None, 0.0, 15.0),
                                                     ("/musan/noise/n2.wav", None, 6.25, 0.0)], True)
    # music / babble: background items with --duration, with and without the quotes
    items = [_bg(8.12, "/musan/speech/s%d.wav" % i, quotes=i % 2 == 0) for i in range(7)]
    e = features.parse_wav_entry(_augment_data_dir_entry("/d/a.wav", items, [0] * 7, [13, 15, 17, 20, 13, 15, 17]))
    assert e.path == "/d/a.wav" and e.rir_path is None and e.augmented and len(e.noises) == 7
    assert e.noises[3] == ("/musan/speech/s3.wav", 8.12, 0.0, 20.0)
    # a mix of both kinds, and the pipe form of augment_data_dir.py:116 over a `cat` entry
    e = features.parse_wav_entry(_augment_data_dir_entry("cat /d/a.wav |", [_bg(3, "m.wav"), "n.wav"], [0, 2], [5, 10]))
    assert e == features.WavEntry("/d/a.wav", None, [("m.wav", 3.0, 0.0, 5.0), ("n.wav", None, 2.0, 10.0)], True)


REFUSED = [
    "sox a.flac -t wav - |",
    "ffmpeg -i a.m4a -f wav - |",
    _augment_data_dir_entry("sox a.flac -t wav - |", ["n.wav"], [0], [5]),                                # :116 over a non-cat pipe
    RVB_ENTRY.format("sox a.flac -t wav - |", "true", RVB_IR.format("r.wav")),
    RVB_ENTRY.format(RVB_CAT.format("a.wav"), "false", RVB_IR.format("r.wav")),
    RVB_ENTRY.format(RVB_CAT.format("a.wav"), "true", RVB_IR.format("r.wav") + "--duration=3 "),           # top-level --duration
    "cat a.wav | wav-reverberate --impulse-response=\"r.wav\" - - |",                                      # --shift-output defaults to false
    RVB_ENTRY.format(RVB_CAT.format("a.wav"), "true", ""),                                                 # nothing to apply
    RVB_ENTRY.format(RVB_CAT.format("a.wav"), "true", RVB_IR.format("r.wav") + "--volume=0.5 "),
    RVB_ENTRY.format(RVB_CAT.format("a.wav"), "true", RVB_IR.format("r.wav") + "--multi-channel-output=true "),
    RVB_ENTRY.format(RVB_CAT.format("a.wav"), "true", RVB_IR.format("r.wav") + RVB_IR.format("r2.wav")),
    _augment_data_dir_entry("a.wav", ['wav-reverberate --impulse-response="r.wav" --duration=3 "n.wav" - |'], [0], [5]),
    _augment_data_dir_entry("a.wav", ['wav-reverberate --impulse-response="r.wav" "n.wav" - |'], [0], [5]),
    _augment_data_dir_entry("a.wav", ["sox n.flac -t wav - |"], [0], [5]),
    _augment_data_dir_entry("a.wav", ["n1.wav", "n2.wav"], [0], [5, 10]),
    _augment_data_dir_entry("a.wav", ["n1.wav", "n2.wav"], [0, 1], [5]),
    _augment_data_dir_entry("a.wav", ["n1.wav"], [0, 1], [5, 10]),
    _augment_data_dir_entry("a.wav", ["n1.wav"], ["x"], [5]),
    "wav-reverberate --shift-output=true --additive-signals='n.wav' --start-times='0' a.wav - |",          # no --snrs
    "wav-reverberate --shift-output=true --snrs='5' --start-times='0' a.wav - |",
    "wav-reverberate --shift-output=true --impulse-response=\"r.wav\" a.wav - |",
    "wav-reverberate --shift-output=true --additive-signals='n.wav' --start-times='0' --snrs='5' a.wav b.wav |",
    "cat a.wav | wav-reverberate --shift-output=true --impulse-response=\"r.wav\" - - | sox - -t wav - |",
    "cat a.wav | wav-reverberate --shift-output=true --impulse-response='unterminated - - |",
]


@pytest.mark.parametrize("text", REFUSED)
def test_refused_entry_shapes(text):
    from pytorch_kaldi_resnet_amd import features
    with pytest.raises(ValueError, match="pipe") as ei:
        features.parse_wav_entry(text)
    assert text in str(ei.value) or repr(text) in str(ei.value)


def test_wav_table_still_refuses_every_pipe():
    from pytorch_kaldi_resnet_amd import ingest
    for text in ("sox a.flac -t wav - |", RVB_ENTRY.format(RVB_CAT.format("a.wav"), "true", RVB_IR.format("r.wav"))):
        with pytest.raises(ValueError, match="pipe"):
            ingest.WavTable([text], 16000)


# ---- wav_scp_batches ----
def _write(path, samples, rate=FS):
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(np.asarray(samples).astype(np.int16).tobytes())
    return str(path)


def test_wav_scp_batches_with_augmented_entries(tmp_path):
    from pytorch_kaldi_resnet_amd import features
    fb = features.FbankOptions(num_mel_bins=40)
    sp = [_write(tmp_path / ("s%d.wav" % i), A.speech(9000 + 1500 * i, 20 + i)) for i in range(4)]
    rir = _write(tmp_path / "rir.wav", 20000 * A.impulse_response(0.2, 30))
    nz = _write(tmp_path / "noise.wav", A.noise(5000, 31))
    nz8 = _write(tmp_path / "noise8k.wav", A.noise(5000, 32), rate=8000)
    plain = str(tmp_path / "plain.scp")
    open(plain, "w").writelines("u%d %s\n" % (i, p) for i, p in enumerate(sp))
    lines = ["u0 %s\n" % sp[0],
             "rvb-u1 %s\n" % RVB_ENTRY.format(RVB_CAT.format(sp[1]), "true", RVB_IR.format(rir)),
             "noise-u2 %s\n" % _augment_data_dir_entry(sp[2], [nz, nz], [0, 0.3], [10, 5]),
             "babble-u3 %s\n" % _augment_data_dir_entry(sp[3], [_bg(0.75, nz)] * 3, [0, 0, 0], [13, 15, 17])]
    scp = str(tmp_path / "aug.scp")
    open(scp, "w").writelines(lines)
    # a wav.scp without augmented entries: the table and the batches of before, with or without the new argument
    k0, t0, b0, s0 = features.wav_scp_batches(plain, fb, 2)
    k1, t1, b1, s1 = features.wav_scp_batches(plain, fb, 2, augment=True)
    assert k0 == k1 and t0.paths == t1.paths and not hasattr(t1, "augmentation")
    assert [(list(i), n) for i, n in b0] == [(list(i), n) for i, n in b1]
    # augmented entries are not handed to a caller that would not apply them
    with pytest.raises(ValueError, match="pipe"):
        features.wav_scp_batches(scp, fb, 2)
    keys, table, batches, short = features.wav_scp_batches(features.read_wav_scp(scp), fb, 2, augment=True)       # parsed once
    assert keys == ["u0", "rvb-u1", "noise-u2", "babble-u3"] and table.paths == sp
    assert [(list(i), n) for i, n in batches] == [(list(i), n) for i, n in b0] and len(short) == 0       # by the speech length
    assert isinstance(table.augmentation, features.WavAugmentation) and sorted(table.augmentation.aux.paths) == sorted([rir, nz])                                            # each distinct file once
    rirs, noises, names = features.augment_inputs(table, np.arange(4))
    assert rirs[0] is None and rirs[2] is None and noises[0] == [] and noises[1] == []
    assert np.array_equal(rirs[1], np.trunc(20000 * A.impulse_response(0.2, 30)))
    assert [(d, st, snr) for _, d, st, snr in noises[2]] == [(None, 0.0, 10.0), (None, 0.3, 5.0)]
    assert [(d, st, snr) for _, d, st, snr in noises[3]] == [(0.75, 0.0, 13.0), (0.75, 0.0, 15.0), (0.75, 0.0, 17.0)]
    assert all(v[0] is noises[2][0][0] for v in noises[2] + noises[3])                             # one read, one array
    features.augment_inputs(table, np.arange(4))
    assert table.augmentation.reads == 2
    assert rir in names[1] and sp[1] in names[1]
    # every impulse-response and noise file must have its speech file's rate: refused naming both
    bad = str(tmp_path / "bad.scp")
    open(bad, "w").writelines(lines[:2] + ["noise-u2 %s\n" % _augment_data_dir_entry(sp[2], [nz8], [0], [10])])
    with pytest.raises(ValueError) as ei:
        features.wav_scp_batches(bad, fb, 2, augment=True)
    assert nz8 in str(ei.value) and sp[2] in str(ei.value) and "8000" in str(ei.value)


# ---- compute_fbank.py: argument errors (before any GPU use) ----
def _run(cmd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "compute_fbank.py")] + cmd, env=env, capture_output=True,
                          text=True, timeout=300)


def test_compute_fbank_argument_errors(tmp_path):
    scp = str(tmp_path / "wav.scp")
    open(scp, "w").write("u0 a.wav\nrvb-u0 %s\n" % RVB_ENTRY.format(RVB_CAT.format("a.wav"), "true", RVB_IR.format("r.wav")))
    vad = str(tmp_path / "vad.scp")
    open(vad, "w").write("")
    out = str(tmp_path / "out")
    r = _run([scp, out, "--speed", "0.9"])
    assert r.returncode == 2 and "--speed does not combine with wav-reverberate entries" in r.stderr
    r = _run([scp, out, "--vad-scp", vad])
    assert r.returncode == 2 and "--vad-scp needs --egs" in r.stderr
    r = _run([scp, out, "--egs"])
    assert r.returncode == 2 and "--egs needs --vad-config" in r.stderr
    sox = str(tmp_path / "sox.scp")
    open(sox, "w").write("u0 sox a.flac -t wav - |\n")
    r = _run([sox, out])
    assert r.returncode == 2 and "pipe" in r.stderr
    assert not os.path.exists(out)
