"""The GPU augmentation (csrc/augment.hip through pytorch_kaldi_resnet_amd.features.augment) against the fp64 oracle
tests/augment_ref.py: a ragged batch with every kind of row, zero tails, row / batch / padding invariance bit for bit, the 16-bit
quantisation and its clipped counts, the refusals, and compute_fbank.py on a wav.scp of wav-reverberate entries against the same
script on plain files that hold features.augment's quantised output.

The accuracy bound is the project's rule for the fbank and the resampler: per row, twice the error of the oracle's own float32
run against its fp64 run on the same input.  That float32 run (augment_ref.augment32) restates the kernel's arithmetic - the same
partition size, a radix-2 float32 FFT written in numpy, the same order of the bin products, fp64 sums of squares - and never sees
the kernel's output.  The test prints the measured ratios."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import augment_ref as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB = os.path.join(ROOT, "tests", "golden", "fbank")
FS = 16000


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


def _rows():
    """(speech, impulse response or None, noises) per row: reverberation only; foreground noises only (one running past the end,
    one starting past it); one background noise with --duration (repeated); babble with 7 backgrounds shorter and longer than the
    speech; reverberation plus noise, the impulse response with a negative sample larger than its peak; no augmentation"""
    fg = [(A.noise(5000, 40), None, 0.0, 15.0), (A.noise(7000, 41), None, 0.7, 10.0), (A.noise(4000, 42), None, 1.2, 5.0),
          (A.noise(9000, 43), None, 1.6, 0.0), (A.noise(3000, 44), None, 2.5, 0.0)]
    babble = [(A.noise(n, 50 + i), 35000 / FS, 0.0, snr) for i, (n, snr) in enumerate(
        [(9000, 13.0), (50000, 15.0), (21000, 17.0), (35000, 20.0), (1234, 13.0), (70001, 15.0), (16000, 17.0)])]
    return [
        (A.speech(40000, 1), A.impulse_response(0.6, 2), []),
        (A.speech(30011, 3), None, fg),
        (A.speech(25000, 4), None, [(A.noise(7000, 45), 25000 / FS, 0.0, 8.0)]),
        (A.speech(35000, 5), None, babble),
        (A.speech(48000, 6), A.impulse_response(1.0, 7, negative_larger=True),
         [(A.noise(6000, 46), None, 0.25, 12.0), (A.noise(20000, 47), 3.0, 0.0, 9.0)]),
        (A.speech(20000, 8), None, []),
    ]


def test_augment_matches_fp64_oracle():
    from pytorch_kaldi_resnet_amd import features
    rows = _rows()
    assert len(rows[0][1]) != len(rows[4][1])
    waves = [r[0] for r in rows]
    wave_t, n = _batch(waves, nmax=max(len(w) for w in waves) + 37, fill=12345.0)       # 37 columns of garbage
    out, clipped = features.augment(wave_t, n, [r[1] for r in rows], [r[2] for r in rows])
    out = out.cpu().numpy()
    assert out.shape == tuple(wave_t.shape) and out.dtype == np.float32
    assert clipped.dtype == np.int64 and not clipped.any()
    for b, (x, h, nz) in enumerate(rows):
        ref = A.augment(x, h, nz)
        assert A.augment(x, h, nz, quantize=True)[1] == 0           # the oracle itself clips nothing on these inputs
        r32 = A.augment32(x, h, nz)
        assert (out[b, len(x):] == 0).all()                         # exactly 0 past the row's count
        d = out[b, :len(x)] - ref
        e32_max, e32_rms = np.abs(r32 - ref).max(), np.sqrt(((r32 - ref) ** 2).mean())
        dmax, drms = np.abs(d).max(), np.sqrt((d ** 2).mean())
        print("row", b, "max", dmax, "e32_max", e32_max, "ratio", dmax / e32_max if e32_max else 0.0, "rms", drms, "e32_rms", e32_rms,
              "ratio", drms / e32_rms if e32_rms else 0.0, "scale", np.abs(ref).max())
        assert dmax <= 2 * e32_max, (b, dmax, e32_max)
        assert drms <= 2 * e32_rms, (b, drms, e32_rms)
    assert np.array_equal(out[5, :20000], rows[5][0])               # a row with neither comes back as it went in


def test_longest_impulse_response_and_short_speech():
    """R = 32 768 (32 partitions) on speech shorter than it, and a short utterance behind a 5-tap response"""
    from pytorch_kaldi_resnet_amd import features
    h = A.impulse_response(32768 / FS, 9)
    assert len(h) == 32768 == features.hip.lib().spk_augment_max_rir()
    rows = [(A.speech(20000, 10), h, [(A.noise(3000, 48), None, 0.1, 10.0)]),
            (A.speech(1500, 11), np.array([0.1, 1.0, -0.5, 0.25, 0.1], dtype=np.float32), [])]
    wave_t, n = _batch([r[0] for r in rows], fill=-7.0)
    out, _ = features.augment(wave_t, n, [r[1] for r in rows], [r[2] for r in rows])
    out = out.cpu().numpy()
    for b, (x, hh, nz) in enumerate(rows):
        ref, r32 = A.augment(x, hh, nz), A.augment32(x, hh, nz)
        d = out[b, :len(x)] - ref
        e32_max, e32_rms = np.abs(r32 - ref).max(), np.sqrt(((r32 - ref) ** 2).mean())
        print("row", b, "max ratio", np.abs(d).max() / e32_max, "rms ratio", np.sqrt((d ** 2).mean()) / e32_rms)
        assert np.abs(d).max() <= 2 * e32_max and np.sqrt((d ** 2).mean()) <= 2 * e32_rms
        assert (out[b, len(x):] == 0).all()


def test_row_batch_padding_invariance():
    """a row's output does not depend on its batch, its index, its batch-mates' impulse responses and noises, Nmax or what the
    padding holds (NaN included) - bit for bit"""
    from pytorch_kaldi_resnet_amd import features
    rows = _rows()
    for pick in (4, 3, 0):
        x, h, nz = rows[pick]
        a, _ = features.augment(*_batch([x]), [h], [nz])
        a0 = a[0, :len(x)].cpu().numpy()
        others = [rows[i] for i in range(6) if i != pick][:3]
        mates = others[:2] + [rows[pick]] + others[2:]
        wb, nb = _batch([r[0] for r in mates], nmax=48000 + 1003, fill=float("nan"))
        b, _ = features.augment(wb, nb, [r[1] for r in mates], [r[2] for r in mates])
        assert np.array_equal(a0, b[2, :len(x)].cpu().numpy())
        assert (b[2, len(x):] == 0).all()
        wc, nc = _batch([x, rows[1][0]], nmax=len(x) + 2, rows=[3, 0], fill=-1.0)
        c, _ = features.augment(wc, nc, [None, None, None, h], [rows[1][2], [], [], nz])
        assert np.array_equal(a0, c[3, :len(x)].cpu().numpy())
        assert not torch.isnan(b).any()


def test_quantisation_and_clipped_counts():
    from pytorch_kaldi_resnet_amd import features
    rows = _rows()
    loud = (np.clip(4 * A.speech(30000, 12, amp=30000.0), -32000, 32000), A.impulse_response(0.3, 13),      # heavily compressed
            [(A.noise(8000, 49), 30000 / FS, 0.0, 0.0)])
    rows = rows + [loud]
    wave_t, n = _batch([r[0] for r in rows], fill=99999.0)
    args = ([r[1] for r in rows], [r[2] for r in rows])
    plain, c0 = features.augment(wave_t, n, *args)
    quant, c1 = features.augment(wave_t, n, *args, quantize=True)
    plain, quant = plain.cpu().numpy(), quant.cpu().numpy()
    t = np.trunc(plain)
    assert np.array_equal(quant, np.clip(t, -32768, 32767))
    want = ((t > 32767) | (t < -32768)).sum(1)
    print("clipped", c1, want)
    assert np.array_equal(c1, want) and not c0.any()
    assert not c1[:6].any() and c1[6] > 0                                         # only the loud row clips
    assert abs(int(c1[6]) - A.augment(*loud, quantize=True)[1]) <= max(2, int(0.02 * c1[6]))      # the oracle clips as many
    # without anything to apply, quantisation alone is applied
    x = np.array([[1.9, -1.9, 40000.0, -40000.0, 32767.9, -32768.9, 0.5, 5.0]], dtype=np.float32)
    q, c = features.augment(torch.from_numpy(x).cuda(), [6], quantize=True)
    assert q.cpu().numpy().tolist() == [[1, -1, 32767, -32768, 32767, -32768, 0, 0]] and c.tolist() == [2]


def test_refusals_come_before_any_launch(tmp_path):
    from pytorch_kaldi_resnet_amd import features, hip
    w, n = _batch([A.speech(5000, 14), A.speech(4000, 15)])
    nz = A.noise(1000, 60)
    limit = hip.lib().spk_augment_max_rir()
    with pytest.raises(ValueError, match=r"row 1 \(b\.wav\) has %d samples, more than the %d" % (limit + 1, limit)):
        features.augment(w, n, [None, np.ones(limit + 1, dtype=np.float32)], names=["a.wav", "b.wav"])
    sizes = (hip.ctypes.c_longlong * 3)()
    with pytest.raises(RuntimeError, match="Rmax=%d" % (limit + 1)):            # ... and by the library's own check
        hip.call("spk_augment_workspace", 2, 5000, limit + 1, 100, 0, 0, sizes)
    with pytest.raises(ValueError, match="all zero"):
        features.augment(w, n, None, [[], [(np.zeros(100, dtype=np.float32), None, 0.0, 5.0)]])
    lead = np.concatenate([np.zeros(800, dtype=np.float32), nz])           # q_k is the power of what is added, after --duration
    with pytest.raises(ValueError, match="all zero over the 800 samples"):
        features.augment(w, n, None, [[(nz, None, 0.0, 5.0), (lead, 0.05, 0.0, 5.0)], []])
    features.augment(w, n, None, [[(lead, 0.06, 0.0, 5.0), (lead, None, 0.0, 5.0)], []])
    with pytest.raises(ValueError, match="is empty"):
        features.augment(w, n, None, [[(np.zeros(0, dtype=np.float32), None, 0.0, 5.0)], []])
    with pytest.raises(ValueError, match="is empty"):
        features.augment(w, n, [np.zeros(0, dtype=np.float32), None])
    with pytest.raises(ValueError, match="non-finite SNR"):
        features.augment(w, n, None, [[(nz, None, 0.0, float("nan"))], []])
    with pytest.raises(ValueError, match="non-finite SNR"):
        features.augment(w, n, None, [[(nz, None, 0.0, float("inf"))], []])
    with pytest.raises(ValueError, match="starts at -0.5"):
        features.augment(w, n, None, [[(nz, None, -0.5, 5.0)], []])
    with pytest.raises(ValueError, match="gives 0 samples"):
        features.augment(w, n, None, [[(nz, 0.0, 0.0, 5.0)], []])
    with pytest.raises(ValueError, match="1 impulse responses and 2 noise lists for 2 rows"):
        features.augment(w, n, [None], [[], []])
    with pytest.raises(ValueError, match="2 impulse responses and 3 noise lists for 2 rows"):
        features.augment(w, n, None, [[], [], []])
    with pytest.raises(ValueError, match="3 sample counts for 2 rows"):
        features.augment(w, [5000, 4000, 1])
    with pytest.raises(ValueError, match="float32 array"):
        features.augment(w, n, [np.ones(10), None])
    with pytest.raises(ValueError, match="float32 cuda"):
        features.augment(w.cpu(), n)
    # a noise file at another rate than its speech file: refused naming both
    sp = _write_wav(tmp_path / "s.wav", A.speech(9000, 16))
    n8 = _write_wav(tmp_path / "n8.wav", A.noise(3000, 61), rate=8000)
    scp = str(tmp_path / "wav.scp")
    open(scp, "w").write("noise-u %s\n" % NOISE.format(items=n8, starts="0", snrs="10", wav=sp))
    with pytest.raises(ValueError) as ei:
        features.wav_scp_batches(scp, features.FbankOptions(num_mel_bins=40), 4, augment=True)
    assert n8 in str(ei.value) and sp in str(ei.value)


# ---- end to end: scripts/compute_fbank.py ----
RVB = 'cat {wav} | wav-reverberate --shift-output=true --impulse-response="{rir}" {more} - - |'
NOISE = "wav-reverberate --shift-output=true --additive-signals='{items}' --start-times='{starts}' --snrs='{snrs}' {wav} - |"
BG = 'wav-reverberate --duration={dur} "{wav}" - |'


def _write_wav(path, samples, rate=FS):
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(np.asarray(samples).astype(np.int16).tobytes())
    return str(path)


def _run(cmd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "compute_fbank.py")] + cmd, env=env, capture_output=True,
                          text=True, timeout=300)


def _write_vad(path_base, frames, seed):
    """vad.ark / vad.scp of seeded 0/1 vectors: {key: frame count} -> the scp path"""
    from pytorch_kaldi_resnet_amd import kaldi_io
    rng = np.random.default_rng(seed)
    ark = path_base + ".ark"
    lines = []
    with open(ark, "wb") as f:
        for k, T in frames.items():
            v = (rng.random(T) < 0.7).astype(np.float32)
            f.write((k + " ").encode())
            lines.append("%s %s:%d\n" % (k, ark, f.tell()))
            kaldi_io.write_vec_flt(f, v)
    open(path_base + ".scp", "w").writelines(lines)
    return path_base + ".scp"


def test_compute_fbank_on_augmented_entries(tmp_path):
    from pytorch_kaldi_resnet_amd import features, kaldi_io
    d = str(tmp_path)
    lens = {"plain": 21000, "rvb": 26000, "rvbnoise": 30000, "noise": 24000, "babble": 33000}
    sp = {k: _write_wav(tmp_path / (k + ".wav"), A.speech(n, 70 + i)) for i, (k, n) in enumerate(lens.items())}
    rir = {k: _write_wav(tmp_path / ("rir_%s.wav" % k), np.round(20000 * A.impulse_response(sec, 80 + i)))
           for i, (k, sec) in enumerate({"a": 0.5, "b": 0.9}.items())}
    nz = {k: _write_wav(tmp_path / ("noise_%s.wav" % k), A.noise(n, 90 + i)) for i, (k, n) in enumerate(
        {"a": 6000, "b": 9000, "c": 40000, "d": 15000}.items())}
    entries = {
        "plain": sp["plain"],
        "rvb": RVB.format(wav=sp["rvb"], rir=rir["a"], more=""),
        "rvbnoise": RVB.format(wav=sp["rvbnoise"], rir=rir["b"], more="--additive-signals='%s,%s' --start-times='0,1.0' --snrs='20,10'"
                               % (nz["a"], nz["b"])),
        "noise": NOISE.format(items=",".join([nz["a"], nz["b"], nz["a"]]), starts="0,0.5,1.25", snrs="15,10,5", wav=sp["noise"]),
        "babble": NOISE.format(items=",".join(BG.format(dur=33000 / FS, wav=nz[k]) for k in "cdacdab"), starts="0,0,0,0,0,0,0",
                               snrs="13,15,17,20,13,15,17", wav=sp["babble"]),
    }
    scp = os.path.join(d, "aug.scp")
    open(scp, "w").writelines("%s %s\n" % kv for kv in entries.items())
    fb, _, _ = features.options_from_configs(os.path.join(FB, "fbank.conf"))
    vad = _write_vad(os.path.join(d, "vad"), {k: fb.num_frames(n) for k, n in lens.items()}, 5)
    opts = ["--fbank-config", os.path.join(FB, "fbank.conf"), "--egs", "--vad-scp", vad, "--cmn-window", "300", "--seed", "3",
            "--batch-size", "4"]
    r = _run([scp, os.path.join(d, "o1")] + opts)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "samples clipped" in r.stdout and "wrote 5 of 5" in r.stdout
    # the same augmentation through the functional API, written as plain 16-bit files under the same keys
    keys, table, _, _ = features.wav_scp_batches(scp, fb, 8, augment=True)
    idx = np.arange(len(keys))
    nmax = int(table.nsamp.max())
    buf = torch.empty(len(keys), nmax)
    table.read_padded(idx, nmax, buf, 2)
    rirs, noises, names = features.augment_inputs(table, idx)
    out, clipped = features.augment(buf.cuda(), table.nsamp, rirs, noises, quantize=True, sample_rate=FS, names=names)
    assert ("%d samples clipped" % clipped.sum()) in r.stdout
    out = out.cpu().numpy()
    assert np.array_equal(out, np.trunc(out)) and np.abs(out).max() <= 32768
    assert np.array_equal(out[0, :lens["plain"]], A.speech(lens["plain"], 70))
    for b, k in enumerate(keys[1:], 1):                    # every augmented row differs from its speech, and follows the oracle
        x = A.speech(lens[k], 70 + b)
        assert not np.array_equal(out[b, :lens[k]], x)
        ref, _ = A.augment(x, rirs[b], noises[b], quantize=True)
        assert np.abs(out[b, :lens[k]] - ref).max() <= 1.0          # truncation may fall on the other side of a whole number
    os.makedirs(os.path.join(d, "q"))
    scp2 = os.path.join(d, "quant.scp")
    open(scp2, "w").writelines("%s %s\n" % (k, _write_wav(os.path.join(d, "q", k + ".wav"), out[b, :lens[k]]))
                               for b, k in enumerate(keys))
    r2 = _run([scp2, os.path.join(d, "o2")] + opts)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert "samples clipped" not in r2.stdout
    assert open(os.path.join(d, "o1", "utt2num_frames")).read() == open(os.path.join(d, "o2", "utt2num_frames")).read()
    a = {k: m for k, m in kaldi_io.read_mat_scp(os.path.join(d, "o1", "feats.scp"))}
    b2 = {k: m for k, m in kaldi_io.read_mat_scp(os.path.join(d, "o2", "feats.scp"))}
    assert list(a) == list(b2) == list(entries)
    for k in a:
        assert a[k].dtype == np.float32 and np.array_equal(a[k], b2[k]), k
    assert open(os.path.join(d, "o1", "feats.ark"), "rb").read() == open(os.path.join(d, "o2", "feats.ark"), "rb").read()
    # the plain entry's features are those of a run with only that entry
    scp3 = os.path.join(d, "plain.scp")
    open(scp3, "w").write("plain %s\n" % sp["plain"])
    r3 = _run([scp3, os.path.join(d, "o3")] + opts)
    assert r3.returncode == 0, r3.stdout[-2000:] + r3.stderr[-2000:]
    (k3, m3), = list(kaldi_io.read_mat_scp(os.path.join(d, "o3", "feats.scp")))
    assert k3 == "plain" and np.array_equal(m3, a["plain"])
    # the voiced frames are the file's: the frame count is the number of ones
    nfr = dict(l.split() for l in open(os.path.join(d, "o1", "utt2num_frames")))
    for line in open(vad):
        k, loc = line.split()
        assert int(nfr[k]) == int(kaldi_io.read_vec_flt(loc).sum()) == a[k].shape[0]
    # ... and they are the frames where the vector is 1: the sliding CMN over all frames of the quantised audio's fbank (dither of
    # the written key), picked with the vector itself
    _, _, cmn = features.options_from_configs(os.path.join(FB, "fbank.conf"), None, 300)
    vec = {l.split()[0]: kaldi_io.read_vec_flt(l.split()[1]) for l in open(vad)}
    for b, k in enumerate(keys):
        f, T, _ = features.fbank(torch.from_numpy(out[b:b + 1, :lens[k]].copy()).cuda(), [lens[k]], fb, [features.utt_id(k)], 3)
        want = features.sliding_cmn(f, T, cmn)[0].cpu().numpy().T[vec[k] == 1]
        assert 0 < want.shape[0] < T[0] and np.array_equal(a[k], want), k
    # a vector of the wrong length, a missing key: errors that name the utterance
    frames = {k: fb.num_frames(n) for k, n in lens.items()}
    frames["noise"] += 1
    bad = _write_vad(os.path.join(d, "vad_bad"), frames, 5)
    r4 = _run([scp, os.path.join(d, "o4")] + opts[:3] + ["--vad-scp", bad])
    assert r4.returncode != 0 and "noise" in r4.stderr and "frames" in r4.stderr
    frames["noise"] -= 1
    del frames["babble"]
    r5 = _run([scp, os.path.join(d, "o5")] + opts[:3] + ["--vad-scp", _write_vad(os.path.join(d, "vad_missing"), frames, 5)])
    assert r5.returncode != 0 and "babble has no entry" in r5.stderr
