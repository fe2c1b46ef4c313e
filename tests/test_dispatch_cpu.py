"""ops._plan_conv / ops._plan_wgrad against the launch record (tests/golden/dispatch/*.json, tools/make_dispatch_golden.py) on a
machine without a GPU: for every recorded convolution the planner arguments are rebuilt from the stored planner-level inputs
and the plan is compared field by field with the C ABI scalars, the entry and the label the recorded launch carried.  The
files were written at the revision before the planners existed; the library is never loaded here."""
import glob
import os
import sys

import pytest

from conftest import GOLD, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_dispatch_golden import load  # noqa: E402  (the reader of the files' one-line-per-record form; imports no library)

FILES = sorted(glob.glob(os.path.join(GOLD, "dispatch", "*.json")))
# label prefixes bench.py's mfma_peak() tells apart, as counted in the files when they were recorded: the forms the default
# build reaches in these runs (conv_ws_kernel, conv_wgrad_ws_kernel, conv_wgrad_pipe_kernel are opt-in; the engine hands every
# f16x3 weight gradient a pair-tensor dy, so conv_wgrad_wm_kernel gives way to conv_wgrad_wm16_kernel) ...
PEAK_PREFIXES = ["conv_mfma_kernel", "conv_pipe_kernel", "conv_wgrad_split_kernel", "conv_wgrad_wm16_kernel",
                 "conv_wgrad_c32m16_kernel", "conv_wgrad_1x1_kernel"]
# ... and the labels it rates at the fp32 matrix peak
OTHER_PREFIXES = ["conv1x1_stream_kernel", "conv3x3_c32_stream_kernel", "conv_wgrad_kernel", "spk_wgrad_reduce"]


@pytest.fixture(scope="module")
def ops():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops
    return ops


def mask_form(t, n):
    """the None pattern and length of a stored bn_bwd (n = 3) / in_bnbwd (n = 4) tuple -> how it carries its ReLU mask"""
    return None if t is None else "sign" if len(t) > n else "raw" if t[1] is None else "act"


def check_conv(ops, rec, experimental):
    i = rec["inputs"]
    (launch,) = rec["launches"]
    a, entry = launch["args"], launch["entry"]
    B, IH, IW, Cin = i["x"]
    p = ops._plan_conv(B, IH, IW, Cin, i["OH"], i["OW"], i["out"][1], i["out"][2], i["Cout"], [tuple(t) for t in i["taps"]],
                       i["IS"], i["OS"], i["ooy"], i["oox"], i["split"], experimental, in_affine=i["in_affine"] is not None,
                       epi_affine=i["epi_affine"] is not None, epi_add=i["epi_add"] is not None, relu=i["relu"],
                       want_stats=i["want_stats"], bn_bwd=mask_form(i["bn_bwd"], 3), in_bnbwd=mask_form(i["in_bnbwd"], 4),
                       side=i["side"] is not None, add_mask=i["add_mask"] is not None, in_presplit=i["in_presplit"],
                       side_presplit=i["side_presplit"], wlen=i["wlen"] is not None, out_is_x=i["out_is_x"])
    shape = " C%d %dx%d%s" % (i["Cout"], i["OH"], i["OW"], " plane32" if a["flags"] & ops.CONV_CK32 else "") if ops.LABEL_SHAPES else ""
    assert (p.entry, p.label, p.flags) == (entry, launch["label"] + shape, a["flags"])
    assert bool(p.flags & ops.EPI_STATS) == (a["stats"] != 0)
    if entry in ("spk_conv3x3_c32_stream", "spk_conv1x1_stream"):
        assert p.nblocks == a["nblocks"]
        assert entry == "spk_conv1x1_stream" or p.stats_rows == 4 * a["nblocks"]
    else:
        assert entry == ("spk_conv_mfma" if i["wlen"] is None else "spk_conv_mfma_len")
        assert (p.TH, p.TW, p.MT, p.NT, p.kc, p.ips, p.IS) == tuple(a[k] for k in ("TH", "TW", "MT", "NT", "kc", "ips", "IS"))
        assert p.WC == ({0: 1, 1: 2, 2: 4}[(a["flags"] >> 8) & 3] if a["flags"] & ops.CONV_WS else 1)
        assert p.stats_rows == (4 // p.WC) * B * -(-a["OH"] // a["TH"]) * -(-a["OW"] // a["TW"])
        # the launcher's own marshalling of the plan-independent scalars, as recorded
        assert (a["ntaps"], a["split"], a["OS"], a["ooy"], a["oox"]) == (len(i["taps"]), i["split"], i["OS"], i["ooy"], i["oox"])
        assert [list(t) for t in zip(a["tap_dy"], a["tap_dx"], a["tap_w"])] == i["taps"]


def check_wgrad(ops, rec):
    i = rec["inputs"]
    launch, reduce = rec["launches"]
    a = launch["args"]
    assert (launch["entry"], reduce["entry"]) == ("spk_conv_wgrad", "spk_wgrad_reduce")
    B, _, _, Cin = i["x"]
    _, OH, OW, Cout = i["dy"]
    split = ops.split_for(i["ksize"], True)
    assert split == a["split"]
    p = ops._plan_wgrad(B, Cin, OH, OW, Cout, i["ksize"], i["stride"], split, in_affine=i["in_affine"] is not None,
                        dy_presplit=i["dy_presplit"])
    shape = " C%d %dx%d" % (Cout, OH, OW) if ops.LABEL_SHAPES else ""
    assert (p.TH, p.TW, p.WN, p.nsplit, p.flags, p.label) == (a["TH"], a["TW"], a["WN"], a["nsplit"], a["flags"], launch["label"] + shape)
    assert p.cg == ({1: 2, 2: 4}[(a["flags"] >> 12) & 3] if a["flags"] & ops.WGRAD_GROUPS else 0)
    assert p.label.startswith({"f32": "conv_wgrad_kernel<", "split": "conv_wgrad_split_kernel<"}.get(p.family, "conv_wgrad_%s_kernel" % p.family))
    assert reduce["args"]["nslab"] == p.nsplit


@pytest.mark.parametrize("shapes", [False, True], ids=["plain", "label_shapes"])
@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(f)[:-5] for f in FILES])
def test_plans_equal_the_record(ops, path, shapes, monkeypatch):
    """shapes: with the diagnostic LABEL_SHAPES switch the same label carries the layer's shape (and `plane32`) behind it"""
    d = load(path)
    assert d["records"], "empty record"
    monkeypatch.setattr(ops, "SPLIT", ops.MFMA_MODES[d["config"]["mode"]])       # conv_wgrad reads the operand mode from it
    monkeypatch.setattr(ops, "LABEL_SHAPES", shapes)
    seen = set()
    for rec in d["records"]:
        seen.add(rec["fn"])
        if rec["fn"] == "_conv_launch":
            check_conv(ops, rec, d["experimental"])
        else:
            check_wgrad(ops, rec)
    assert seen == ({"_conv_launch"} if d["config"].get("run") == "predict" else {"_conv_launch", "conv_wgrad"})


def test_the_record_covers_the_label_families():
    assert len(FILES) == 9
    labels = set()
    for path in FILES:
        labels |= {ln["label"].split("<")[0] for rec in load(path)["records"] for ln in rec["launches"]}
    assert sorted(labels) == sorted(PEAK_PREFIXES + OTHER_PREFIXES)


def test_opt_in_forms_the_record_does_not_reach(ops, monkeypatch):
    """No recorded run reaches conv_ws_kernel (the engine's fused data gradients leave their side output as a pair tensor, which
    that kernel does not take, so the variant-library record equals the default one but for `experimental`), conv_wgrad_wm_kernel
    (every f16x3 weight gradient of the engine gets a pair-tensor dy), conv_wgrad_ws_kernel or conv_wgrad_pipe_kernel (opt-in).
    Their branches against expectations worked out by hand from csrc's limits, on a 128 -> 128 fused data gradient of the 20 x 75
    map and a 64 -> 64 weight gradient of the 40 x 150 map."""
    monkeypatch.setattr(ops, "LABEL_SHAPES", False)
    from pytorch_kaldi_resnet_amd import tiling
    dgrad = (2, 20, 75, 128, 20, 75, 20, 75, 128, [(1 - kh, 1 - kw, kh * 3 + kw) for kh in range(3) for kw in range(3)], 1, 1, 0, 0, 3)
    fused = dict(in_bnbwd="raw", side=True)
    assert tiling.ws_tile(20, 75, 1, 3, 3, 9, 128) == (10, 19, 6, 1, 4)
    # "auto": the wave-specialised kernel only where the library has it
    p = ops._plan_conv(*dgrad, False, **fused)
    assert (p.label, p.flags, p.WC) == ("conv_mfma_kernel<3,2,true,3>", ops.IN_BNBWD, 1)
    p = ops._plan_conv(*dgrad, True, **fused)
    assert (p.label, p.flags) == ("conv_ws_kernel<6,1,4,true,3>", ops.IN_BNBWD | ops.CONV_WS | (2 << 8))
    assert (p.TH, p.TW, p.MT, p.NT, p.WC, p.stats_rows) == (10, 19, 6, 1, 4, 1 * 2 * 2 * 4)
    # ... not below WS_AUTO_MIN_COUT output channels, not for a plain input, not with a pair-tensor side output
    assert ops._plan_conv(*dgrad[:8], 64, *dgrad[9:], True, **fused).label.startswith("conv_mfma_kernel<")
    assert ops._plan_conv(*dgrad, True).label.startswith("conv_pipe_kernel<")
    assert ops._plan_conv(*dgrad, True, side_presplit=True, **fused).label.startswith("conv_mfma_kernel<")
    # "1": every eligible 3x3 launch, whatever the library says; "0": never
    monkeypatch.setattr(ops, "WS_CONV", "1")
    assert ops._plan_conv(*dgrad, False).label == "conv_ws_kernel<6,1,4,false,3>"
    monkeypatch.setattr(ops, "WS_CONV", "0")
    assert ops._plan_conv(*dgrad, True, **fused).label == "conv_mfma_kernel<3,2,true,3>"
    # weight gradient, 8 x 8 tile (halo 10 x 10 = 100 pixels: NX = 4; four k-steps of 16 pixels), two waves per pixel group
    wg = (2, 64, 40, 150, 64, 3, 1, 3)
    p = ops._plan_wgrad(*wg)
    assert (p.TH, p.TW, p.WN, p.family, p.cg, p.label) == (8, 8, 2, "wm", 2, "conv_wgrad_wm_kernel")
    assert p.flags == ops.WGRAD_GROUPS | (1 << 12) and p.nsplit <= 2 * 5 * 19
    monkeypatch.setattr(ops, "WM_SHIFT", False)
    assert ops._plan_wgrad(*wg).flags == ops.WGRAD_GROUPS | (1 << 12) | ops.hip.WGRAD_NOSHIFT
    monkeypatch.setattr(ops, "PIPE_WGRAD", True)        # 2 x (2 x 100 x 64 + 2 x 2 x 64 x 64) + 128 = 58 496 bytes <= PIPE_MAX_LDS
    p = ops._plan_wgrad(*wg)
    assert (p.family, p.cg, p.flags, p.label) == ("pipe", 0, ops.CONV_PIPE, "conv_wgrad_pipe_kernel<2,2,4,2>")
    monkeypatch.setattr(ops, "WS_WGRAD", True)          # takes precedence; 2 x (100 x 192 + 64 x 448) = 95 744 bytes <= 160 KiB
    p = ops._plan_wgrad(*wg)
    assert (p.family, p.cg, p.flags, p.label) == ("ws", 0, ops.CONV_WS, "conv_wgrad_ws_kernel<9,2,2,4>")
    assert ops._plan_wgrad(*wg, dy_presplit=True).label == "conv_wgrad_wm16_kernel"       # neither takes a pair-tensor dy
