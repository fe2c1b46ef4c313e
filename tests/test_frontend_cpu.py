"""Feature front end, CPU side: the fp64 oracle (tests/frontend_ref.py) against the fixtures tools/make_fbank_golden.py computed
with the reference's kaldi.py, the VAD and sliding-CMN oracles on hand-derived cases, the Kaldi config parser on the recipe's conf
files, the WAV reader against the stdlib `wave` module, and the host-side argument refusals of the new C-ABI entries."""
import ctypes
import json
import os
import struct
import wave

import numpy as np
import pytest
import torch

import frontend_ref as R
import pytorch_kaldi_resnet_amd  # noqa: F401
from pytorch_kaldi_resnet_amd import features, hip, ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB = os.path.join(ROOT, "tests", "golden", "fbank")
CASES = json.load(open(os.path.join(FB, "cases.json")))


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference_fixtures(name):
    z = np.load(os.path.join(FB, name + ".npz"))
    kw = json.loads(str(z["options"]))
    f, e = R.fbank(z["wave"].astype(np.float64), **kw)
    assert f.shape == z["fbank"].shape
    assert np.abs(f - z["fbank"]).max() <= 1e-5
    assert np.abs(e - z["log_energy"]).max() <= 1e-5 * np.abs(z["log_energy"]).max()


def test_fixtures_cover_the_issue_cases():
    opts = [json.loads(str(np.load(os.path.join(FB, n + ".npz"))["options"])) for n in CASES]
    assert {o.get("snip_edges", True) for o in opts} == {True, False}
    assert {o.get("window_type", "povey") for o in opts} == set(features.WINDOWS)
    assert {o["sample_frequency"] for o in opts} == {8000.0, 16000.0}
    assert {40, 80} <= {o.get("num_mel_bins", 23) for o in opts}
    for n in CASES:
        assert os.path.getsize(os.path.join(FB, n + ".npz")) < 64 * 1024


def test_frames_reflect_once_at_both_ends():
    x = np.arange(10, dtype=np.float64)
    fr = R.frames(x, 6, 4, snip_edges=False)      # off = 3 - 2 = 1, T = (10 + 2) // 4 = 3
    assert fr.shape == (3, 6)
    assert list(fr[0]) == [0, 0, 1, 2, 3, 4]
    assert list(fr[2]) == [7, 8, 9, 9, 8, 7]
    assert R.frames(x, 6, 4, snip_edges=True).shape == (2, 6)


def test_vad_oracle_hand_cases():
    e = np.array([0.0, 10.0, 10.0, 0.0, 0.0, 10.0])   # mean 5: thr = 1 + 0.5 * 5 = 3.5
    assert list(R.vad(e, 1.0, 0.5, 0, 0.6)) == [0, 1, 1, 0, 0, 1]
    # context 1, proportion 0.5: windows clipped at the edges count only the frames inside
    # t=0 window [0,1]: 1 >= 0.5 * 2; t=3 window [2,4]: 1 < 0.5 * 3
    assert list(R.vad(e, 1.0, 0.5, 1, 0.5)) == [1, 1, 1, 0, 0, 1]
    # context 2, proportion 0.6: t=0 window [0,2]: 2 >= 1.8; t=1 window [0,3]: 2 < 2.4; t=3 window [1,5]: 3 >= 3.0
    assert list(R.vad(e, 1.0, 0.5, 2, 0.6)) == [1, 0, 0, 1, 0, 0]
    assert list(R.vad(np.zeros(4), 5.0, 0.5, 0, 0.6)) == [0, 0, 0, 0]


def test_cmn_window_rule():
    assert R.cmn_window(0, 1000, 300) == (0, 300)           # shifted right at the start
    assert R.cmn_window(500, 1000, 300) == (350, 650)
    assert R.cmn_window(999, 1000, 300) == (700, 1000)      # shifted left at the end
    assert R.cmn_window(10, 100, 300) == (0, 100)           # T < W: the whole utterance
    assert R.cmn_window(299, 300, 300) == (0, 300)          # T = W
    assert R.cmn_window(0, 300, 300) == (0, 300)
    x = np.arange(5, dtype=np.float64)[:, None] * np.ones((1, 2))
    np.testing.assert_allclose(R.sliding_cmn(x, 3), np.array([[-1, 0, 0, 0, 1]]).T * np.ones((1, 2)))
    np.testing.assert_allclose(R.sliding_cmn(x, 10), x - 2.0)


def test_kaldi_config_parser_on_recipe_confs():
    fb = features.FbankOptions.from_kaldi_config(os.path.join(FB, "fbank.conf"))
    assert (fb.sample_frequency, fb.frame_length, fb.low_freq, fb.high_freq, fb.num_mel_bins, fb.snip_edges) == \
        (16000.0, 25.0, 20.0, 7600.0, 40, False)
    assert fb.dither == 1.0 and fb.window_type == "povey"
    v = features.VadOptions.from_kaldi_config(os.path.join(FB, "vad.conf"))
    assert (v.vad_energy_threshold, v.vad_energy_mean_scale, v.vad_proportion_threshold, v.vad_frames_context) == \
        (5.5, 0.5, 0.12, 2)


def test_kaldi_config_parser_refusals(tmp_path):
    p = tmp_path / "bad.conf"
    p.write_text("--num-mel-bins=40\n--no-such-option=1  # comment\n")
    with pytest.raises(ValueError, match="unknown option --no-such-option"):
        features.FbankOptions.from_kaldi_config(str(p))
    for bad in (dict(vtln_warp=0.9), dict(use_energy=True), dict(htk_compat=True), dict(subtract_mean=True),
                dict(use_power=False), dict(use_log_fbank=False), dict(frame_length=80.0)):
        with pytest.raises(ValueError):
            features.FbankOptions(**bad)
    with pytest.raises(ValueError):
        features.CmnOptions(center=False)
    with pytest.raises(ValueError):
        features.CmnOptions(norm_vars=True)


def test_host_tables_match_oracle():
    o = features.FbankOptions(num_mel_bins=40, high_freq=7600)
    np.testing.assert_allclose(features.window_function(o), R.window("povey", 400), rtol=0, atol=1e-15)
    np.testing.assert_allclose(features.mel_banks(o), R.mel_weights(40, 512, 16000.0, 20.0, 7600.0), rtol=0, atol=1e-12)


# ---- WAV reader ----
def _wav(path, x, fs=16000, width=2, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(fs)
        w.writeframes(x.tobytes())


def _chunked(path, x, fs=16000, extensible=False, list_chunk=True, tag=1, bits=16, channels=1):
    if extensible:
        guid = struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, channels, fs, fs * 2 * channels, 2 * channels, bits, 22, bits, 4) + guid
    else:
        fmt = struct.pack("<HHIIHH", tag, channels, fs, fs * 2 * channels, 2 * channels, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if list_chunk:
        info = b"INFOISFT\x05\x00\x00\x00test\x00"        # odd size: padded to even
        body += b"LIST" + struct.pack("<I", len(info)) + info + b"\x00"
    data = x.astype("<i2").tobytes()
    body += b"data" + struct.pack("<I", len(data)) + data
    open(path, "wb").write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_wav_reader_against_stdlib_wave(tmp_path):
    rng = np.random.default_rng(0)
    xs = [rng.integers(-32768, 32767, n).astype(np.int16) for n in (1000, 1601, 400)]
    paths = []
    for i, x in enumerate(xs):
        p = tmp_path / ("u%d.wav" % i)
        if i == 0:
            _wav(p, x)
        elif i == 1:
            _chunked(p, x, list_chunk=True)
        else:
            _chunked(p, x, extensible=True, list_chunk=True)
        paths.append(str(p))
        if i < 2:           # the stdlib reader of this Python does not take WAVE_FORMAT_EXTENSIBLE
            with wave.open(str(p), "rb") as w:
                assert np.array_equal(np.frombuffer(w.readframes(w.getnframes()), "<i2"), x)
    tab = ingest.WavTable(paths, 16000)
    assert list(tab.nsamp) == [len(x) for x in xs] and list(tab.rate) == [16000] * 3
    out = torch.full((3, 2000), 7.0)
    tab.read_padded(np.arange(3), 2000, out, nthreads=2)
    for i, x in enumerate(xs):
        assert np.array_equal(out[i, :len(x)].numpy(), x.astype(np.float32))
        assert (out[i, len(x):] == 0).all()


def test_wav_reader_refusals(tmp_path):
    x = np.zeros(100, dtype=np.int16)
    cases = {"stereo.wav": dict(channels=2), "u8.wav": dict(bits=8), "float.wav": dict(tag=3),
             "ext_float.wav": dict(extensible=True, tag=3)}
    for name, kw in cases.items():
        _chunked(tmp_path / name, x, **kw)
        with pytest.raises(RuntimeError, match=name):
            ingest.WavTable([str(tmp_path / name)], 16000)
    _wav(tmp_path / "w24.wav", np.zeros(300, dtype=np.uint8), width=3)
    with pytest.raises(RuntimeError, match="w24.wav.*24-bit"):
        ingest.WavTable([str(tmp_path / "w24.wav")], 16000)
    _wav(tmp_path / "r8k.wav", x, fs=8000)
    with pytest.raises(RuntimeError, match="r8k.wav.*8000"):
        ingest.WavTable([str(tmp_path / "r8k.wav")], 16000)
    assert ingest.WavTable([str(tmp_path / "r8k.wav")], 8000).nsamp[0] == 100
    (tmp_path / "junk.wav").write_bytes(b"RIFX0000WAVE")
    with pytest.raises(RuntimeError, match="junk.wav"):
        ingest.WavTable([str(tmp_path / "junk.wav")], 16000)
    with pytest.raises(ValueError, match="pipe"):
        ingest.WavTable(["sox a.flac -t wav - |"], 16000)


# ---- C-ABI refusals (host-side checks, before any launch) ----
_POINTERS = ("wave", "nsamp", "first", "total", "frame0", "nframes", "utt_ids", "window", "twiddle", "mel_w", "mel_lo", "mel_off", "dct",
             "lifter", "feats", "log_energy", "T_out")


def _frontend_call(lib, mfcc, span, null=(), F=40, C=13, P=512, L=400, S=160, dither=0.0):
    """(export name, rc) of spk_{fbank,mfcc}[_span]_fwd on dummy pointers (`null`: the ones passed as NULL), B = 1, Nmax = 1000,
    Tcap = 10; nothing is dereferenced as long as the call fails a host-side check"""
    p = {k: None if k in null else ctypes.c_void_p(16) for k in _POINTERS}
    name = "spk_%s%s_fwd" % ("mfcc" if mfcc else "fbank", "_span" if span else "")
    args = ([p["wave"], p["nsamp"]] + ([p[k] for k in ("first", "total", "frame0", "nframes")] if span else [])
            + [p["utt_ids"], 1, 1000] + [p[k] for k in ("window", "twiddle", "mel_w", "mel_lo", "mel_off")]
            + ([p["dct"], p["lifter"]] if mfcc else []) + [L, S, P, F] + ([C] if mfcc else []) + [1, dither, 0.97, 1, 0.0]
            + ([1, 0] if mfcc else []) + [0, p["feats"], p["log_energy"], p["T_out"], 10, None])
    return name, getattr(lib, name)(*args)


# (the forms a case applies to, arguments, the word its refusal carries)
REFUSALS = [
    ("all", dict(P=500), b"power of two"), ("all", dict(P=2048), b"power of two"),
    ("all", dict(dither=1.0, null=("utt_ids",)), b"utt_ids"), ("all", dict(null=("mel_off",)), b"null"),
    ("all", dict(L=1024, S=4000, P=1024), b"LDS"),
    ("span", dict(null=("first",)), b"null"), ("span", dict(null=("total",)), b"null"), ("span", dict(null=("frame0",)), b"null"),
    ("span", dict(null=("nframes",)), b"null"),
    ("mfcc", dict(C=41), b"num_ceps"), ("mfcc", dict(C=0), b"num_ceps"), ("mfcc", dict(C=-3), b"num_ceps"),
    ("mfcc", dict(null=("dct",)), b"null"), ("mfcc", dict(null=("lifter",)), b"null"), ("mfcc", dict(F=600, C=13), b"num_mel_bins"),
    ("mfcc", dict(F=128, C=128), b"LDS"),
    # F > P: the MFCC forms refuse it (the log-mels reuse the FFT buffer); fbank allows F <= 1024 and gets as far as the tile test
    # (the shift of 4000 samples is there so that no tile fits: with the default shift a tile of 8 frames would, and launch)
    ("mfcc", dict(F=600, S=4000), b"num_mel_bins"), ("fbank", dict(F=600, S=4000), b"LDS"),
]


@pytest.mark.parametrize("mfcc, span", [(False, False), (True, False), (False, True), (True, True)])
def test_frontend_exports_refuse_bad_arguments_without_a_gpu(mfcc, span):
    """one table over the four exports: each refusal returns rc < 0 and names the export that was called"""
    lib = hip.lib()
    applies = {"all": True, "span": span, "mfcc": mfcc, "fbank": not mfcc}
    ran = 0
    for forms, kw, word in REFUSALS:
        if applies[forms]:
            name, rc = _frontend_call(lib, mfcc, span, **kw)
            err = lib.spk_last_error()
            assert rc < 0 and name.encode() + b":" in err and word in err, (name, kw, rc, err)
            ran += 1
    assert ran == 5 + 4 * span + (8 if mfcc else 1)


def test_frontend_argtypes_are_the_declared_parameter_lists():
    """the ctypes signatures of the four exports, written out: include/spkhip.h's parameter lists, type by type"""
    lib = hip.lib()
    P, I, L, F, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_ulonglong
    assert lib.spk_fbank_fwd.argtypes == [P, P, P, I, L, P, P, P, P, P, I, I, I, I, I, F, F, I, F, U, P, P, P, I, P]
    assert lib.spk_mfcc_fwd.argtypes == [P, P, P, I, L, P, P, P, P, P, P, P, I, I, I, I, I, I, F, F, I, F, I, I, U, P, P, P, I, P]
    assert lib.spk_fbank_span_fwd.argtypes == [P, P, P, P, P, P, P, I, L, P, P, P, P, P, I, I, I, I, I, F, F, I, F, U, P, P, P, I, P]
    assert lib.spk_mfcc_span_fwd.argtypes == [P, P, P, P, P, P, P, I, L, P, P, P, P, P, P, P, I, I, I, I, I, I, F, F, I, F, I, I, U, P,
                                              P, P, I, P]


def test_frontend_entries_refuse_bad_arguments_without_a_gpu():
    """the other entries of csrc/frontend.hip (the four frame launches: the table above)"""
    lib = hip.lib()
    P = ctypes.c_void_p(16)      # never dereferenced: every call below fails its host-side checks
    assert lib.spk_fbank_tile_frames(400, 160, 512, 80) == 32
    assert lib.spk_fbank_tile_frames(1024, 4000, 1024, 80) == 0
    assert lib.spk_fbank_dither_noise(P, 0, 0, 0, 0, 400, None) < 0
    assert lib.spk_vad_count(P, P, 1, 10, 5.0, 0.5, -1, 0.6, P, P, P, None) < 0
    assert b"frames_context" in lib.spk_last_error()
    assert lib.spk_cmn_select(P, P, P, None, P, P, 1, 40, 10, 10, 300, None) < 0
    assert b"idx and count" in lib.spk_last_error()
    assert lib.spk_cmn_select(P, P, None, None, None, P, 1, 40, 10, 10, 300, None) < 0
    assert b"prefix" in lib.spk_last_error()
    assert lib.spk_cmn_select(P, P, None, None, P, P, 1, 40, 10, 11, 300, None) < 0


class _FakeCudaWave:
    """stands in for a float32 cuda tensor [2, 1000]: the length checks of features.fbank come before any device work"""
    dtype = torch.float32
    is_cuda = True
    shape = (2, 1000)

    def dim(self):
        return 2

    def contiguous(self):
        return self


def test_fbank_api_refuses_short_utterances():
    with pytest.raises(ValueError, match="row 1 has 399 samples, outside \\[frame length 400"):
        features.fbank(_FakeCudaWave(), [1000, 399], features.FbankOptions(), utt_ids=[1, 2])
    with pytest.raises(ValueError, match="utt_ids"):
        features.fbank(_FakeCudaWave(), [1000, 1000], features.FbankOptions())
