"""Training from audio, the host half: the span reader of libspkio against Python's wave module, the span
planner against a brute-force fp64 CMN of the whole utterance (tests/frontend_ref.py), and the draws of WavTrainLoader against
NativeTrainLoader's over the archive of the same entries.  No GPU."""
import os
import struct
import sys
import wave

import numpy as np
import pytest
import torch

import pytorch_kaldi_resnet_amd  # noqa: F401
from pytorch_kaldi_resnet_amd import features, ingest, kaldi_io

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frontend_ref  # noqa: E402


def write_wav(path, x, rate=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(x, dtype="<i2").tobytes())


def write_extensible(path, x, rate=16000):
    """WAVE_FORMAT_EXTENSIBLE with a LIST chunk of odd size in front of the data"""
    x = np.asarray(x, dtype="<i2")
    guid = struct.pack("<H", 1) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    fmt = struct.pack("<HHIIHHHHI", 0xFFFE, 1, rate, rate * 2, 2, 16, 22, 16, 4) + guid
    assert len(fmt) == 40
    lst = b"LIST" + struct.pack("<I", 5) + b"abcde" + b"\x00"
    body = b"WAVE" + b"fmt " + struct.pack("<I", 40) + fmt + lst + b"data" + struct.pack("<I", x.nbytes) + x.tobytes()
    open(str(path), "wb").write(b"RIFF" + struct.pack("<I", len(body)) + body)


def wave_module_read(path, first, count):
    with wave.open(str(path), "rb") as w:
        w.setpos(first)
        return np.frombuffer(w.readframes(count), dtype="<i2")


# ---- reader ----
@pytest.fixture(scope="module")
def wav_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("span_reader")
    rs = np.random.RandomState(11)
    files = []
    for i, n in enumerate([4000, 1, 777, 12345]):
        p = d / ("f%d.wav" % i)
        x = rs.randint(-32768, 32768, size=n).astype(np.int16)
        (write_extensible if i == 2 else write_wav)(p, x)
        files.append((str(p), x))
    return files


def test_read_span_is_bit_exact_against_the_wave_module(wav_files):
    tab = ingest.WavTable([p for p, _ in wav_files], 16000)
    assert list(tab.nsamp) == [len(x) for _, x in wav_files]
    #        interior     first sample  last sample   count 1   a file of one sample   EXTENSIBLE      whole file   empty span
    spans = [(0, 100, 900), (0, 0, 50), (0, 3950, 50), (3, 5000, 1), (1, 0, 1), (2, 3, 770), (3, 0, 12345), (0, 17, 0)]
    idx = np.array([s[0] for s in spans])
    first = np.array([s[1] for s in spans])
    count = np.array([s[2] for s in spans])
    for threads in (1, 3):
        Nmax = 12352
        out = torch.full((len(spans), Nmax), 7, dtype=torch.int16)
        tab.read_span(idx, first, count, Nmax, out, nthreads=threads)
        got = out.numpy()
        for b, (i, f, c) in enumerate(spans):
            if i != 2:          # the wave module does not read WAVE_FORMAT_EXTENSIBLE before Python 3.12: compare with what was written
                np.testing.assert_array_equal(got[b, :c], wave_module_read(wav_files[i][0], f, c))
            np.testing.assert_array_equal(got[b, :c], wav_files[i][1][f:f + c])
            assert not got[b, c:].any()


def test_read_span_refusals_name_the_file(wav_files):
    tab = ingest.WavTable([p for p, _ in wav_files], 16000)
    out = torch.zeros(1, 64, dtype=torch.int16)
    name = os.path.basename(wav_files[0][0])
    with pytest.raises(RuntimeError, match=name):           # first < 0
        tab.read_span([0], [-1], [10], 64, out)
    with pytest.raises(RuntimeError, match=name):           # first + count > nsamp
        tab.read_span([0], [3990], [11], 64, out)
    with pytest.raises(RuntimeError, match=name + ".*Nmax"):  # count > Nmax
        tab.read_span([0], [0], [65], 64, out)
    assert not out.numpy().any()                            # refused before anything is read
    tab.read_span([0], [3990], [10], 64, out)               # the span up to the last sample is fine
    np.testing.assert_array_equal(out.numpy()[0, :10], wav_files[0][1][3990:])


# ---- planner ----
def _opts(snip):
    return features.FbankOptions(sample_frequency=8000.0, frame_length=1.0, frame_shift=0.5, num_mel_bins=4, snip_edges=snip)


def _frame_samples(opts, N, lo, hi):
    """the samples of an utterance of N samples that frames [lo, hi) read (tests/frontend_ref.py: frames)"""
    L, S = opts.frame_len, opts.frame_sh
    off = 0 if opts.snip_edges else L // 2 - S // 2
    s = np.arange(lo, hi)[:, None] * S - off + np.arange(L)[None, :]
    s = np.where(s < 0, -s - 1, s)
    s = np.where(s >= N, 2 * N - 1 - s, s)
    assert s.min() >= 0 and s.max() < N
    return s


def _voiced(pattern, Ttot, rs, need):
    """ascending voiced frames of an utterance of Ttot >= need frames, at least `need` of them"""
    k = max(need, Ttot // 3)
    if pattern == "dense":
        return np.arange(Ttot)
    if pattern == "sparse":
        return np.sort(rs.permutation(Ttot)[:k])
    return np.arange(k) if pattern == "head" else np.arange(Ttot - k, Ttot)


def test_plan_spans_gives_the_whole_utterance_cmn():
    """200 seeded draws: the fp64 sliding CMN of the selected frames, computed on the span with span-relative indices, equals the
    whole-utterance one; the span is no longer than the utterance nor than t_last - t_first + 1 + 2 W; the sample range holds
    every sample the span's frames read."""
    rs = np.random.RandomState(2024)
    seen, done, worst = set(), 0, 0.0
    combos = [(W, T, pat) for W in (1, 2, 30, 31) for T in sorted({1, 7, W // 2, W, 2 * W}) if T >= 1
              for pat in ("dense", "sparse", "head", "tail")]
    while done < 200:
        W, T, pat = combos[done % len(combos)]
        Ttot = max(int(rs.randint(1, 3 * W + 1)), T)       # 1 .. 3 W frames, and room for the chunk
        vi = _voiced(pat, Ttot, rs, T)
        snip = bool(done % 2)
        opts = _opts(snip)
        L, S = opts.frame_len, opts.frame_sh
        N = L + (Ttot - 1) * S + int(rs.randint(0, S)) if snip else Ttot * S - S // 2 + int(rs.randint(0, S))
        v0 = int(rs.randint(0, vi.size - T + 1))
        if done % 7 == 0:
            v0 = 0
        if done % 7 == 1:
            v0 = vi.size - T
        dense_as_none = pat == "dense" and done % 3 == 0
        p = ingest.plan_spans([None if dense_as_none else vi.astype(np.int32)], [v0], T, W, [Ttot], opts, [max(N, L)])
        lo, hi = int(p.frame_lo[0]), int(p.frame_hi[0])
        sel = vi[v0:v0 + T]
        assert 0 <= lo < hi <= Ttot
        assert hi - lo <= sel[-1] - sel[0] + 1 + 2 * W
        np.testing.assert_array_equal(p.rel[0] + lo, sel)
        x = rs.randn(Ttot, 3) * 10 + rs.randn(1, 3) * 100
        whole = frontend_ref.sliding_cmn(x, W)[sel]
        span = frontend_ref.sliding_cmn(x[lo:hi], W)[p.rel[0]]
        worst = max(worst, float(np.abs(whole - span).max()))
        assert np.abs(whole - span).max() <= 1e-12, (W, T, pat, Ttot, v0, lo, hi)
        if N >= L and opts.num_frames(N) == Ttot:
            s = _frame_samples(opts, N, lo, hi)
            assert p.first[0] <= s.min() and s.max() < p.first[0] + p.count[0], (snip, N, lo, hi, p.first[0], p.count[0])
            assert p.first[0] >= 0 and p.first[0] + p.count[0] <= N
            features.check_spans("test", opts, p.count, p.first, [N], [lo], [hi - lo], int(p.count[0]))      # the wrapper agrees
        seen.add((W, T, pat))
        done += 1
    assert seen == set(combos)
    print("plan_spans: worst |whole - span| = %.3g over 200 draws" % worst)


def test_plan_spans_without_cmn_is_the_selected_range():
    opts = _opts(True)
    vi = np.array([3, 4, 9, 20, 21], dtype=np.int32)
    p = ingest.plan_spans([vi, None], [1, 5], 3, 0, [30, 30], opts, [opts.frame_len + 29 * opts.frame_sh] * 2)
    assert list(p.frame_lo) == [4, 5] and list(p.frame_hi) == [21, 8]
    np.testing.assert_array_equal(p.rel, [[0, 5, 16], [0, 1, 2]])


def test_span_wrapper_refusals_on_the_host():
    opts = _opts(False)
    L, S = opts.frame_len, opts.frame_sh
    N = 40 * S
    ok = dict(nsamp=[N], first=[0], total=[N], frame0=[0], nframes=[40])
    features.check_spans("t", opts, Nmax=N, **ok)
    for change, msg in [(dict(nframes=[41]), "frames outside"), (dict(frame0=[-1]), "frames outside"),
                        (dict(first=[1], nsamp=[N - 1]), "outside the row"),          # frame 0 reflects into sample 0
                        (dict(nsamp=[N - 1]), "outside the row"),                      # the last frame reflects about `total`
                        (dict(first=[5], nsamp=[N]), "not a part"), (dict(total=[L - 1], nsamp=[L - 1]), "shorter than one frame"),
                        (dict(nsamp=[N + 1]), "Nmax")]:
        with pytest.raises(ValueError, match=msg):
            features.check_spans("t", opts, Nmax=N, **dict(ok, **change))
    # an interior span needs only its own samples
    first, last = features.span_samples(opts, [10], [12], [N])
    features.check_spans("t", opts, [last[0] - first[0]], first, [N], [10], [2], N)
    with pytest.raises(ValueError, match="outside the row"):
        features.check_spans("t", opts, [last[0] - first[0] - 1], first, [N], [10], [2], N)


# ---- draws ----
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """a wav.scp with vad.scp and the feats.scp of an archive whose entries have as many rows as their wav has voiced frames"""
    d = tmp_path_factory.mktemp("draws")
    rs = np.random.RandomState(5)
    opts = features.FbankOptions(num_mel_bins=4, snip_edges=False, dither=0.0)
    wav, vad, feats, u2s = [], [], [], []
    with open(str(d / "vad.ark"), "wb") as fv, open(str(d / "feats.ark"), "wb") as fa:
        for s in range(4):
            for u in range(2 if s else 12):         # speaker 0 has six times the utterances: the balancing lists the others 3 times
                key = "s%d-u%d" % (s, u)
                n = int(rs.randint(8000, 20000))
                p = d / (key + ".wav")
                write_wav(p, rs.randint(-3000, 3000, size=n))
                T = opts.num_frames(n)
                v = (rs.rand(T) < 0.7).astype(np.float32)
                v[:40] = 1
                fv.write((key + " ").encode())
                off = fv.tell()
                kaldi_io.write_vec_flt(fv, v)
                vad.append("%s %s:%d" % (key, d / "vad.ark", off))
                foff = kaldi_io.write_mat(fa, np.zeros((int(v.sum()), 4), dtype=np.float32), key=key)
                feats.append("%s %s:%d" % (key, d / "feats.ark", foff))
                wav.append("%s %s" % (key, p))
                u2s.append("%s %d" % (key, s))
    for name, lines in (("wav.scp", wav), ("vad.scp", vad), ("feats.scp", feats), ("utt2spkid", u2s)):
        open(str(d / name), "w").write("\n".join(lines) + "\n")
    return d, opts


@pytest.mark.parametrize("chunk_range", [None, (24, 40, 8)])
def test_draws_equal_native_train_loader(corpus, chunk_range):
    d, opts = corpus
    n, lengths = 0, set()
    for seed in (0, 3):
        for world, rank in ((1, 0), (2, 0), (2, 1)):
            kw = dict(rank=rank, world=world, seed=seed, chunk_range=chunk_range)
            a = ingest.NativeTrainLoader(str(d / "feats.scp"), str(d / "utt2spkid"), 40, 8, **kw)
            b = ingest.WavTrainLoader(str(d / "wav.scp"), str(d / "utt2spkid"), 40, 8, opts, features.CmnOptions(cmn_window=30),
                                      vad_scp=str(d / "vad.scp"), **kw)
            assert len(a) == len(b)
            np.testing.assert_array_equal(a.labels, b.labels)
            for epoch in (0, 1):
                a.set_epoch(epoch)
                b.set_epoch(epoch)
                da, db = list(a.draws()), list(b.draws())
                assert len(da) == len(db) == len(a)
                for (ka, sa, ra, Ta, sta), (kb, sb, rb, Tb, stb) in zip(da, db):
                    np.testing.assert_array_equal(sa, sb)
                    assert (ka, Ta, sta) == (kb, Tb, stb)
                    # the same utterance: the archive table is sorted by rxfile, the audio table is in wav.scp order
                    assert [a.table.rows[i] for i in ra] == [b.rows[i] for i in rb]
                    n += len(sta)
                lengths |= {T for _, _, _, T, _ in da}
                assert len(b.labels) == 12 + 3 * 3 * 2          # the repetition rule: cap 6, speakers of 2 utterances 3 times each
    assert n > 0 and (len(lengths) > 1) == (chunk_range is not None)


def test_loader_refusals(corpus, tmp_path):
    d, opts = corpus
    args = (str(d / "utt2spkid"), 40, 8, opts)
    lines = open(str(d / "wav.scp")).read().splitlines()
    # a 44.1 kHz file
    write_wav(tmp_path / "hi.wav", np.zeros(44100, dtype=np.int16), rate=44100)
    open(str(tmp_path / "w1.scp"), "w").write("\n".join(lines[:-1] + ["%s %s" % (lines[-1].split()[0], tmp_path / "hi.wav")]) + "\n")
    with pytest.raises(ValueError, match=r"hi\.wav.*44100"):
        ingest.WavTrainLoader(str(tmp_path / "w1.scp"), *args, vad_scp=str(d / "vad.scp"))
    # a key without a VAD line / without a label
    open(str(tmp_path / "v.scp"), "w").write("\n".join(open(str(d / "vad.scp")).read().splitlines()[1:]) + "\n")
    with pytest.raises(ValueError, match="s0-u0 has no entry in --vad-scp"):
        ingest.WavTrainLoader(str(d / "wav.scp"), *args, vad_scp=str(tmp_path / "v.scp"))
    open(str(tmp_path / "u"), "w").write("\n".join(open(str(d / "utt2spkid")).read().splitlines()[1:]) + "\n")
    with pytest.raises(ValueError, match="s0-u0 has no label"):
        ingest.WavTrainLoader(str(d / "wav.scp"), str(tmp_path / "u"), 40, 8, opts, vad_scp=str(d / "vad.scp"))
    # a VAD vector of another length
    vl = open(str(d / "vad.scp")).read().splitlines()
    open(str(tmp_path / "v2.scp"), "w").write("\n".join(["s0-u0 " + vl[1].split()[1]] + vl[1:]) + "\n")
    with pytest.raises(ValueError, match=r"s0-u0.*frames but its vector"):
        ingest.WavTrainLoader(str(d / "wav.scp"), *args, vad_scp=str(tmp_path / "v2.scp"))
    # a pipe entry of another shape
    open(str(tmp_path / "w2.scp"), "w").write("\n".join(lines[:-1] + ["x sox %s -t wav - |" % lines[-1].split()[1]]) + "\n")
    with pytest.raises(ValueError, match="pipe"):
        ingest.WavTrainLoader(str(tmp_path / "w2.scp"), *args, vad_scp=str(d / "vad.scp"))
    # fewer voiced frames than the chunk: NativeTrainLoader's assertion
    with pytest.raises(AssertionError, match="shorter than the chunk size"):
        ingest.WavTrainLoader(str(d / "wav.scp"), str(d / "utt2spkid"), 4000, 8, opts, vad_scp=str(d / "vad.scp"))


def test_new_exports_are_declared_and_bound():
    import re
    from pytorch_kaldi_resnet_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "spkhip.h")).read()
    for name in ("spk_fbank_span_fwd", "spk_mfcc_span_fwd", "spk_pcm16_to_f32"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in hip.exported_symbols() and hasattr(hip.lib(), name), name
    assert re.search(r"\bspk_wav_read_span\s*\(", open(os.path.join(root, "include", "spkio.h")).read())
    assert hasattr(ingest.lib(), "spk_wav_read_span")
    # host-side validation before any launch
    assert hip.lib().spk_pcm16_to_f32(None, None, 1, 8, None, None) < 0 and b"spk_pcm16_to_f32" in hip.lib().spk_last_error()
