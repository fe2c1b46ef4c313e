"""MFCC front end, CPU side: the fp64 oracle (tests/mfcc_ref.py) against the fixtures tools/make_mfcc_golden.py computed with the
reference's kaldi.py mfcc(), MfccOptions (the recipe's conf/mfcc.conf, the refusals), the host DCT and lifter tables against the
oracle's, and the tile heights of spk_mfcc_tile_frames (the argument refusals of spk_mfcc_fwd: test_frontend_cpu.py)."""
import json
import os

import numpy as np
import pytest

import frontend_ref as R
import mfcc_ref as M
import pytorch_kaldi_resnet_amd  # noqa: F401
from pytorch_kaldi_resnet_amd import features, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MF = os.path.join(ROOT, "tests", "golden", "mfcc")
CASES = json.load(open(os.path.join(MF, "cases.json")))


def _case(name):
    z = np.load(os.path.join(MF, name + ".npz"))
    return z["wave"].astype(np.float64), json.loads(str(z["options"])), z["mfcc"]


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference_fixtures(name):
    x, kw, want = _case(name)
    c, _ = M.mfcc(x, **kw)
    assert c.shape == want.shape and want.dtype == np.float64
    assert np.abs(c - want).max() <= 1e-9, np.abs(c - want).max()


def test_fixtures_cover_the_issue_cases():
    got = set()
    for n in CASES:
        _, kw, _ = _case(n)
        o = dict(M.DEFAULTS, **kw)
        assert o["dither"] == 0
        got.add((o["num_mel_bins"], o["num_ceps"], o["cepstral_lifter"], o["use_energy"], o["htk_compat"], o["sample_frequency"],
                 o["snip_edges"], o["high_freq"], o["energy_floor"]))
        assert os.path.getsize(os.path.join(MF, n + ".npz")) < 100 * 1024
    assert got == {(40, 40, 22.0, True, False, 16000.0, False, 7600, 0.0),
                   (23, 13, 22.0, True, False, 16000.0, True, 0.0, 0.0),
                   (80, 72, 22.0, False, True, 16000.0, True, 0.0, 0.0),
                   (30, 30, 0.0, False, False, 16000.0, True, 0.0, 1.0),
                   (24, 1, 22.0, True, True, 16000.0, True, 0.0, 0.0),
                   (40, 30, 22.0, True, True, 16000.0, True, 0.0, 0.0),
                   (40, 20, 22.0, False, False, 8000.0, True, -200, 0.0)}


def test_every_fixture_builds_mfcc_options():
    for n in CASES:
        _, kw, want = _case(n)
        o = features.MfccOptions(**kw)
        assert o.num_ceps == want.shape[1]


def test_mfcc_options_defaults_and_recipe_conf():
    d = features.MfccOptions()
    assert (d.num_mel_bins, d.num_ceps, d.use_energy, d.energy_floor, d.raw_energy, d.cepstral_lifter, d.htk_compat) == \
        (23, 13, True, 0.0, True, 22.0, False)
    assert (d.frame_len, d.frame_sh, d.padded_len, d.num_frames(16000), d.sample_frequency) == (400, 160, 512, 98, 16000.0)
    o = features.MfccOptions.from_kaldi_config(os.path.join(MF, "mfcc.conf"))
    assert (o.sample_frequency, o.frame_length, o.low_freq, o.high_freq, o.num_mel_bins, o.num_ceps, o.snip_edges) == \
        (16000.0, 25.0, 20.0, 7600.0, 40, 40, False)
    assert o.use_energy and o.cepstral_lifter == 22.0 and o.num_frames(16000) == 100
    fb = features.FbankOptions(snip_edges=False)
    for n in (400, 16000, 16079, 16080):
        assert o.num_frames(n) == fb.num_frames(n)
    mo, vo, cmn = features.options_from_configs(mfcc_config=os.path.join(MF, "mfcc.conf"), cmn_window=300)
    assert isinstance(mo, features.MfccOptions) and mo == o and vo is None and cmn.cmn_window == 300
    assert isinstance(features.options_from_configs()[0], features.FbankOptions)
    with pytest.raises(ValueError, match="mutually exclusive"):
        features.options_from_configs(fbank_config=os.path.join(MF, "mfcc.conf"), mfcc_config=os.path.join(MF, "mfcc.conf"))


@pytest.mark.parametrize("bad, word", [
    (dict(num_ceps=0), "num_ceps"), (dict(num_ceps=24), "num_ceps"), (dict(num_ceps=41, num_mel_bins=40), "num_ceps"),
    (dict(cepstral_lifter=-1.0), "cepstral_lifter"), (dict(vtln_warp=0.9), "vtln_warp"), (dict(raw_energy=False), "raw_energy"),
    (dict(round_to_power_of_two=False), "round_to_power_of_two"), (dict(subtract_mean=True), "subtract_mean"),
    (dict(frame_length=80.0), "1024")])
def test_mfcc_options_refusals(bad, word):
    with pytest.raises(ValueError, match=word):
        features.MfccOptions(**bad)


def test_mfcc_config_parser_refuses_unknown_options(tmp_path):
    p = tmp_path / "bad.conf"
    p.write_text("--num-ceps=20\n--use-power=false\n")       # a compute-fbank-feats option, not one of compute-mfcc-feats
    with pytest.raises(ValueError, match="unknown option --use-power"):
        features.MfccOptions.from_kaldi_config(str(p))
    p.write_text("--num-ceps=20\n--num-mel-bins=30\n--htk-compat=true # comment\n--use-energy=false\n--cepstral-lifter=0\n")
    o = features.MfccOptions.from_kaldi_config(str(p))
    assert (o.num_ceps, o.num_mel_bins, o.htk_compat, o.use_energy, o.cepstral_lifter) == (20, 30, True, False, 0.0)


@pytest.mark.parametrize("F, C, Q", [(40, 40, 22.0), (23, 13, 22.0), (80, 72, 22.0), (30, 30, 0.0), (24, 1, 22.0), (40, 30, 7.5)])
def test_host_tables_match_oracle(F, C, Q):
    o = features.MfccOptions(num_mel_bins=F, num_ceps=C, cepstral_lifter=Q)
    d, l = features.dct_matrix(o), features.lifter_coeffs(o)
    assert d.shape == (C, F) and l.shape == (C,) and d.dtype == np.float64 and l.dtype == np.float64
    assert np.abs(d.astype(np.float32) - M.dct_matrix(C, F).astype(np.float32)).max() <= 2.0 ** -24      # |D| < 1: one ulp at most
    np.testing.assert_allclose(d, M.dct_matrix(C, F), rtol=0, atol=1e-15)
    np.testing.assert_allclose(l, M.lifter(C, Q), rtol=0, atol=1e-14)
    assert np.abs(l.astype(np.float32) - M.lifter(C, Q).astype(np.float32)).max() <= 2.0 ** -24 * (1 + Q / 2)
    np.testing.assert_allclose(d @ d.T, np.eye(C), rtol=0, atol=1e-13)      # orthonormal rows: the lifter is the only gain
    assert l.max() <= 1 + Q / 2 and l[0] == 1.0
    # the mel tables are the fbank's, whatever htk_compat says
    h = features.MfccOptions(num_mel_bins=F, num_ceps=C, cepstral_lifter=Q, htk_compat=True)
    assert np.array_equal(features.mel_banks(o), features.mel_banks(h))
    np.testing.assert_allclose(features.mel_banks(o), R.mel_weights(F, 512, 16000.0, 20.0, 0.0), rtol=0, atol=1e-12)


# ---- C-ABI (host side; the refusals of spk_mfcc_fwd and spk_mfcc_span_fwd: the table of test_frontend_cpu.py over the four exports) ----
def test_mfcc_entry_refuses_bad_arguments_without_a_gpu():
    lib = hip.lib()
    # the tile height comes from the LDS budget: C + 1 rows and the DCT copy
    assert lib.spk_mfcc_tile_frames(400, 160, 512, 40, 40) == 32
    assert lib.spk_mfcc_tile_frames(400, 160, 512, 23, 13) == 32
    assert lib.spk_mfcc_tile_frames(400, 160, 512, 80, 72) == 16
    assert lib.spk_mfcc_tile_frames(400, 160, 512, 128, 128) == 0
    assert lib.spk_mfcc_tile_frames(1024, 4000, 1024, 40, 13) == 0
    assert lib.spk_fbank_tile_frames(400, 160, 512, 80) == 32       # the fbank's tile is what it was


class _FakeCudaWave:
    """stands in for a float32 cuda tensor [2, 1000]: the length checks of features.mfcc come before any device work"""
    import torch as _t
    dtype = _t.float32
    is_cuda = True
    shape = (2, 1000)

    def dim(self):
        return 2

    def contiguous(self):
        return self


def test_mfcc_api_refusals_before_any_launch():
    with pytest.raises(ValueError, match="mfcc: row 1 has 399 samples, outside \\[frame length 400"):
        features.mfcc(_FakeCudaWave(), [1000, 399], features.MfccOptions(), utt_ids=[1, 2])
    with pytest.raises(ValueError, match="mfcc: dither != 0 needs utt_ids"):
        features.mfcc(_FakeCudaWave(), [1000, 1000], features.MfccOptions())
    with pytest.raises(ValueError, match="MfccOptions"):
        features.mfcc(_FakeCudaWave(), [1000, 1000], features.FbankOptions(), utt_ids=[1, 2])
    with pytest.raises(ValueError, match="mfcc: Tcap 2 < longest"):
        features.mfcc(_FakeCudaWave(), [1000, 1000], features.MfccOptions(dither=0.0), Tcap=2)
