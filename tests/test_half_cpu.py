"""Half-precision extraction, the part that needs no GPU: the emulation premises the GPU tests stand on (tests/half_ref.py: which
seeded models stay inside fp16's range, which do not, and how far the fp16 contract itself sits from the exact embedding - the
yardstick of tests/test_half_gpu.py), the rounding helper, the host-side argument validation and the packed layout of the new
exports, and decode.py's refusal of --half with se_resnet34."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import half_ref as R
import pytorch_kaldi_resnet_amd  # noqa: F401
from pytorch_kaldi_resnet_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_seeded_models_stay_inside_fp16_and_the_yardstick(name):
    y = R.case_yardstick(name)
    print("%s: emulation vs fp64 relL2 %.3e  1-cos %.3e  largest stored |value| %.4g" % (name, y["relL2"], y["cosd"], y["peak"]))
    assert y["ovf"].tolist() == [0] * y["case"][4]
    assert y["peak"] == pytest.approx(R.PEAKS[name], rel=0.02)        # the table of DESIGN.md section 6l (two to three digits)
    assert y["peak"] < R.F16_MAX
    # the fp16 contract is a per-layer relative error of 2^-11: far from the fp32 oracle (1e-6), far from a wrong result (O(1))
    assert 1e-5 < y["relL2"] < 1e-2 and y["cosd"] < 1e-5


def test_accumulation_order_moves_the_emulation_as_much_as_fp16_does():
    """why the GPU is not compared with the emulation element by element: summing the convolutions in fp32 instead of fp64 leaves
    the distance to the exact embedding where it was, but moves the embedding itself by about that distance"""
    name = "r18_s21"
    y = R.case_yardstick(name)
    case = y["case"]
    e32, ovf, _ = R.embed(R.case_state(case), y["x"], case[0], case[5], half=True, acc32=True)
    rel32, _ = R.distance(e32, y["e64"])
    apart, _ = R.distance(e32, y["emu"])
    print("%s: fp64-sum emulation %.3e, fp32-sum emulation %.3e from fp64; %.3e from each other" % (name, y["relL2"], rel32, apart))
    assert ovf.tolist() == [0, 0, 0]
    assert 0.5 * y["relL2"] < rel32 < 2.0 * y["relL2"]
    assert apart > 0.1 * y["relL2"]


def test_resnet101_leaves_the_range_in_every_row():
    case = R.OVERFLOW_CASE
    st, x = R.case_state(case), R.case_input(case, 14)
    e64, _, _ = R.embed(st, x, case[0], case[5], half=False)
    _, ovf, _ = R.embed(st, x, case[0], case[5], half=True)
    print("resnet101 seed 13: fp64 embedding max |e| %.3g, overflow counts %s" % (float(e64.abs().max()), ovf.tolist()))
    assert float(e64.abs().max()) > 1e8
    assert (ovf > 0).all()


def test_a_scaled_row_overflows_alone():
    case = R.SCALED_CASE
    st, x = R.case_state(case), R.case_input(case, 12).copy()
    x[1] *= 1e4
    _, ovf, _ = R.embed(st, x, case[0], case[5], half=True)
    assert ovf[0] == 0 and ovf[1] > 0 and ovf[2] == 0


def test_round16_ties_to_even_and_keeps_subnormals():
    v = torch.tensor([2049.0, 2051.0, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, 65519.99, 65520.0, -65520.0, 1e-9],
                     dtype=torch.float64)
    r = R.round16(v)
    assert r.tolist() == [2048.0, 2052.0, 0.0, 2.0 ** -23, 2.0 ** -24, 65504.0, float("inf"), float("-inf"), 0.0]
    assert R.not_finite_rows(r[None]).tolist() == [2]


def _err():
    return hip.lib().spk_last_error().decode()


def test_conv_arguments_are_validated_on_the_host():
    lib = hip.lib()
    p = ctypes.c_void_p(64)          # never dereferenced: validation comes before any launch
    good = dict(B=1, IH=4, IW=4, Cin=32, Cout=32, ksize=3, stride=1)
    for bad in (dict(Cin=48), dict(ksize=2), dict(stride=3), dict(Cout=512), dict(Cin=16), dict(B=0)):
        a = dict(good, **bad)
        rc = lib.spk_h16_conv_fwd(p, p, p, p, None, p, None, p, a["B"], a["IH"], a["IW"], a["Cin"], a["Cout"], a["ksize"],
                                  a["stride"], 1, None)
        assert rc < 0 and "spk_h16_conv_fwd" in _err(), (bad, rc, _err())
    rc = lib.spk_h16_conv_fwd(None, p, p, p, None, p, None, p, 1, 4, 4, 32, 32, 3, 1, 1, None)
    assert rc < 0 and "spk_h16_conv_fwd" in _err()
    assert lib.spk_h16_stem_fwd(p, p, p, p, p, None, None, 1, 4, 4, None) < 0 and "spk_h16_stem_fwd" in _err()
    assert lib.spk_h16_stats_pool_fwd(p, p, None, 1, 4, 4, 32, 2, None) < 0 and "spk_h16_stats_pool_fwd" in _err()
    assert lib.spk_h16_pack_conv_weight(p, p, 32, 32, 3, 1, None) < 0 and "spk_h16_pack_conv_weight" in _err()


def test_packed_bytes_follow_the_documented_layout():
    lib = hip.lib()
    for Cout, Cin, k in ((32, 32, 3), (64, 32, 1), (256, 128, 3), (256, 256, 1)):
        assert lib.spk_h16_packed_bytes(Cout, Cin, k, k) == R.packed_bytes(Cout, Cin, k, k)
        # [tap][Cin / 32][Cout / 16] fragment images of 64 lanes x 8 halfs
        assert R.packed_bytes(Cout, Cin, k, k) == k * k * (Cin // 32) * (Cout // 16) * 64 * 8 * 2
    assert lib.spk_h16_packed_bytes(48, 32, 3, 3) < 0 and "spk_h16_packed_bytes" in _err()
    assert lib.spk_h16_packed_bytes(32, 32, 5, 5) < 0
    # the reference restatement of the layout: element (lane, j) of image (tap, s, m)
    w = torch.arange(64 * 32 * 9, dtype=torch.float32).reshape(64, 32, 3, 3) % 1021
    pk = R.pack_ref(w).reshape(9, 1, 4, 64, 8)
    for t, m, lane, j in ((0, 0, 0, 0), (4, 3, 17, 5), (8, 1, 63, 7)):
        assert pk[t, 0, m, lane, j] == w[16 * m + (lane & 15), 8 * (lane >> 4) + j, t // 3, t % 3]
    th, tw = lib.spk_h16_conv_tile(0), lib.spk_h16_conv_tile(1)
    assert th > 0 and tw > 0 and tw % 16 == 0


def test_decode_refuses_half_with_se_resnet34(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "decode.py"), "--arch", "se_resnet34", "--input-dim", "40",
                        "--pooling", "mean", "--half", "--out-path", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 2
    assert "--half" in r.stderr and "se_resnet34" in r.stderr


def test_predict_refuses_an_unknown_precision_before_touching_the_input():
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    m = NeuralSpeakerModel(spk_num=4, feat_dim=40, pooling="mean", loss="softmax", arch="resnet18")
    with pytest.raises(ValueError, match="precision"):
        m.predict(torch.zeros(1, 40, 16), precision="bf16")
