"""Resampling without a GPU: the fp64 oracle tests/resample_ref.py against the fixtures made with the reference's kaldi.py
(tools/make_resample_golden.py), the output-length rule, the host tables of pytorch_kaldi_resnet_amd.features, the speed-factor
parsing, wav_scp_batches on files of mixed sample rates, and the key / utt2spk / utt2uniq text of a speed-perturbed copy."""
import json
import os
import wave
from fractions import Fraction

import numpy as np
import pytest

import resample_ref as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GR = os.path.join(ROOT, "tests", "golden", "resample")
CASES = json.load(open(os.path.join(GR, "cases.json")))
PAIRS = sorted({(c["fi"], c["fo"]) for c in CASES})
# ou and K of the fixture pairs, worked out by hand from the formula: window half-width ww = 6 / (0.99 min(fi, fo)) seconds, i.e.
# 2 ww fi input samples; K is that count rounded to the lattice (the largest over the phases)
OU_K = {(44100, 16000): (160, 34), (48000, 16000): (1, 37), (22050, 16000): (320, 17), (11025, 16000): (640, 13),
        (8000, 16000): (2, 13), (16000, 8000): (1, 25), (14400, 16000): (10, 13), (17600, 16000): (10, 14)}


def test_fixture_pairs_cover_the_issue():
    assert set(PAIRS) == set(OU_K)
    for p in PAIRS:        # both branches of the length rule, except for 8 -> 16 kHz (always exact) and 22050 (one case)
        kinds = {c["exact_division"] for c in CASES if (c["fi"], c["fo"]) == p}
        assert kinds == {True, False} or p in ((8000, 16000), (22050, 16000))
    assert {c["exact_division"] for c in CASES} == {True, False}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_oracle_matches_reference_fixture(c):
    z = np.load(os.path.join(GR, c["name"] + ".npz"))
    x, ref = z["wave"], z["out"]
    assert x.dtype == np.int16 and ref.dtype == np.float64 and len(x) == c["n"] and len(ref) == c["n_out"]
    y = RS.resample(x.astype(np.float64), c["fi"], c["fo"])
    assert len(y) == len(ref) == RS.num_resampled(c["n"], c["fi"], c["fo"])
    g = np.gcd(c["fi"], c["fo"])
    assert c["exact_division"] == ((c["n"] * (c["fo"] // g)) % (c["fi"] // g) == 0)
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print(c["name"], "max |oracle - fixture| / max |fixture| = %.2e" % err)
    assert err <= 1e-12
    # the float32 run of the oracle is a float32 computation (the yardstick of the GPU test), close to fp64 but not equal to it
    y32 = RS.resample(x.astype(np.float64), c["fi"], c["fo"], dtype=np.float32)
    assert y32.dtype == np.float32 and 0 < np.abs(y32 - y).max() <= 1e-5 * np.abs(ref).max()


@pytest.mark.parametrize("fi,fo", PAIRS + [(44100, 22051), (16000, 48000)])
def test_num_resampled_is_the_brute_force_count(fi, fo):
    from pytorch_kaldi_resnet_amd import features
    n = np.arange(1, 2001)
    # outputs j with j / fo < n / fi, i.e. j * fi < n * fo: counted one by one
    j = np.arange(0, 2000 * fo // fi + 3)
    brute = ((j[None, :] * fi) < (n[:, None] * fo)).sum(1)
    assert np.array_equal(features.num_resampled(n, fi, fo), brute)
    assert [features.num_resampled(int(v), fi, fo) for v in n[:300]] == list(brute[:300])
    assert [RS.num_resampled(int(v), fi, fo) for v in n] == list(brute)
    assert features.num_resampled(0, fi, fo) == 0 and RS.num_resampled(0, fi, fo) == 0


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_tables_equal_the_oracle(fi, fo):
    from pytorch_kaldi_resnet_amd import features
    iu, ou, K, first, w = features.resample_tables(fi, fo)
    riu, rou, rK, rfirst, rw = RS.tables(fi, fo)
    assert (iu, ou, K) == (riu, rou, rK) and (ou, K) == OU_K[(fi, fo)]
    g = np.gcd(fi, fo)
    assert iu == fi // g and ou == fo // g
    assert first.dtype == np.int64 and np.array_equal(first, rfirst)
    assert w.dtype == np.float64 and w.shape == (ou, K) and np.array_equal(w, rw)
    assert features.resample_tables(fi, fo)[4] is w            # cached
    # the taps of a phase sum to about 1 (a low-pass filter of unit DC gain)
    assert np.abs(w.sum(1) - 1).max() < 2e-2


def test_speed_parsing():
    from pytorch_kaldi_resnet_amd import features
    assert features.speed_rates("0.9", 16000) == (14400, 16000)
    assert features.speed_rates("1.1", 16000.0) == (17600, 16000)
    assert features.speed_rates(Fraction(9, 10), 16000) == (14400, 16000)
    assert features.speed_rates("0.9", 16000, 44100) == (39690, 16000)        # combined with an input rate: one resampling
    assert features.speed_rates("1.1", 8000) == (8800, 8000)
    for bad in ("1.0", "1", Fraction(1)):
        with pytest.raises(ValueError, match="no perturbation"):
            features.speed_rates(bad, 16000)
    with pytest.raises(ValueError, match="not a whole number of Hz"):
        features.speed_rates("0.9", 11025)
    with pytest.raises(ValueError, match="not a whole number of Hz"):
        features.speed_rates("0.93337", 16000)
    with pytest.raises(ValueError, match="decimal string"):
        features.speed_rates(0.9, 16000)
    with pytest.raises(ValueError, match="not a decimal factor"):
        features.speed_rates("fast", 16000)
    with pytest.raises(ValueError, match="positive"):
        features.speed_rates("-0.9", 16000)
    # the length of a 0.9x copy is 1 / 0.9 times the original's
    assert features.num_resampled(14400, *features.speed_rates("0.9", 16000)) == 16000
    fe = features.Frontend(features.FbankOptions(), speed="0.9")
    assert fe.rates() == (14400, 16000) and fe.rates(44100) == (39690, 16000)
    assert features.Frontend(features.FbankOptions(), input_rate=44100).rates() == (44100, 16000)
    assert features.Frontend(features.FbankOptions()).rates() == (None, None)
    assert features.Frontend(features.FbankOptions()).rates(8000) == (8000, 16000)
    with pytest.raises(ValueError, match="no perturbation"):
        features.Frontend(features.FbankOptions(), speed="1.0")
    with pytest.raises(ValueError, match="whole number of Hz"):
        features.Frontend(features.FbankOptions(), input_rate=44100.5)


def _wav(path, rate, n, rng):
    with wave.open(path, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(rng.integers(-3000, 3000, n).astype(np.int16).tobytes())


def _mixed_set(d):
    rng = np.random.default_rng(5)
    spec = [("a16", 16000, 20000), ("b44", 44100, 50000), ("c16", 16000, 16000), ("d8", 8000, 9000), ("e44", 44100, 30000),
            ("f44short", 44100, 900),       # 900 samples at 44.1 kHz = 327 at 16 kHz (363 at 0.9x) < one frame (400); 900 >= 400 before
            ("g8", 8000, 250),              # 250 at 8 kHz = 500 at 16 kHz: a frame after resampling, though not before
            ("h44", 44100, 51000), ("i16", 16000, 399)]
    lines = []
    for k, r, n in spec:
        p = os.path.join(d, k + ".wav")
        _wav(p, r, n, rng)
        lines.append("%s %s\n" % (k, p))
    scp = os.path.join(d, "wav.scp")
    open(scp, "w").writelines(lines)
    return scp, spec


def test_wav_scp_batches_mixed_rates(tmp_path):
    from pytorch_kaldi_resnet_amd import features
    scp, spec = _mixed_set(str(tmp_path))
    fb = features.FbankOptions()
    with pytest.raises(ValueError, match=r"b44\.wav: sample rate 44100 is above sample_frequency 16000"):
        features.wav_scp_batches(scp, fb, 4)
    with pytest.raises(ValueError, match=r"b44\.wav: sample rate 44100 is above"):
        features.wav_scp_batches(scp, fb, 4, allow_upsample=True)           # only the wrong flag
    with pytest.raises(ValueError, match=r"d8\.wav: sample rate 8000 is below"):
        features.wav_scp_batches(scp, fb, 4, allow_downsample=True)
    keys, table, batches, short = features.wav_scp_batches(scp, fb, 2, allow_downsample=True, allow_upsample=True)
    assert keys == [k for k, _, _ in spec]
    assert list(table.rate) == [r for _, r, _ in spec] and list(table.nsamp) == [n for _, _, n in spec]
    assert sorted(keys[i] for i in short) == ["f44short", "i16"]            # judged on the resampled length
    seen = []
    for idx, nmax in batches:
        assert len(idx) <= 2 and len({int(table.rate[i]) for i in idx}) == 1          # rate-pure
        assert nmax == table.nsamp[idx].max() and list(table.nsamp[idx]) == sorted(table.nsamp[idx])
        seen += [keys[i] for i in idx]
    assert sorted(seen) == sorted(k for k, _, _ in spec if k not in ("f44short", "i16"))
    # with a speed factor the length after perturbation decides: 399 samples played at 0.9x are 444 >= 400
    _, _, b2, short2 = features.wav_scp_batches(scp, fb, 2, True, True, speed="0.9")
    assert sorted(keys[i] for i in short2) == ["f44short"]
    assert sum(len(i) for i, _ in b2) == len(spec) - 1
    # a set at the fbank's rate behaves as before: no flag needed, length-sorted (two batches: 20 000 samples next to 16 000
    # would be more than 10 % padding)
    scp16 = os.path.join(str(tmp_path), "wav16.scp")
    open(scp16, "w").writelines(l for l in open(scp) if l.split()[0] in ("a16", "c16", "i16"))
    k16, t16, b16, s16 = features.wav_scp_batches(scp16, fb, 8)
    assert [k16[i] for i in s16] == ["i16"] and [[k16[i] for i in b] for b, _ in b16] == [["c16"], ["a16"]]
    assert [n for _, n in b16] == [16000, 20000]


def test_speed_side_files():
    from pytorch_kaldi_resnet_amd import features
    keys = ["id001-a", "id002-b", "id001-c"]
    u2s = {"id001-a": "id001", "id002-b": "id002", "id001-c": "id001", "unused": "x"}
    assert features.speed_key("0.9", "id001-a") == "sp0.9-id001-a"
    s, u = features.speed_side_files("0.9", keys, u2s)
    assert s == "sp0.9-id001-a sp0.9-id001\nsp0.9-id002-b sp0.9-id002\nsp0.9-id001-c sp0.9-id001\n"
    assert u == "sp0.9-id001-a id001-a\nsp0.9-id002-b id002-b\nsp0.9-id001-c id001-c\n"
    s, u = features.speed_side_files("1.1", keys[:1])
    assert s is None and u == "sp1.1-id001-a id001-a\n"
    with pytest.raises(ValueError, match="no speaker for id002-b"):
        features.speed_side_files("0.9", keys, {"id001-a": "id001"})
    # the copies of an utterance draw different dither: the noise is keyed by the written key
    assert len({features.utt_id(k) for k in ("id001-a", "sp0.9-id001-a", "sp1.1-id001-a")}) == 3
