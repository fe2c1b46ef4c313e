"""The stem without two tensor passes, and the pooling kernels that read each row once: every new kernel against the
kernels it replaces, bit for bit (torch.equal).

  * spk_stem_stats / spk_stem_fwd_apply against spk_stem_conv_fwd(EPI_STATS) + spk_bn_apply(relu, mask, amax_out);
  * spk_stem_bwd_wgrad against spk_bn_bwd_apply(MASK_RAW) + spk_stem_conv_wgrad, with accumulate 0 and 1, with d untouched, and
    with inf / NaN in d under the ReLU mask (the pooling backward hands those down under dead rows);
  * one training step with SPK_STEM_FUSED=0 and =1, each in a child process: loss and the whole gradient arena;
  * the row-in-registers pooling forward against the serial two-pass kernel (spk_stats_pool_row_form), with and without
    lengths, modes 0 and 1, including a width above the cap.  (The same form of the pooling backward was measured, was not
    faster and is not in the library.)

Shapes (B, F, T) of the stem: (1,1,1) every tap but the centre out of bounds; (2,5,7) 70 pixels = one ragged block, all four
borders; (3,80,33) 124 blocks, no grid-stride step; (6,80,300) 144 000 pixels > 2048 x 64 > 1024 x 64: both the statistics
grid and the weight-gradient grid take a second grid-stride step.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEM_SHAPES = [(1, 1, 1), (2, 5, 7), (3, 80, 33), (6, 80, 300)]
MASK_RAW = 2


def _slot():
    return torch.zeros(1, device="cuda", dtype=torch.int32)


_stem_cache = {}


def _stem_case(shape):
    """x, w, BatchNorm parameters and the two-kernel forward (the reference of every stem test), computed once per shape"""
    if shape in _stem_cache:
        return _stem_cache[shape]
    from pytorch_kaldi_resnet_amd import ops
    B, F, T = shape
    g = torch.Generator().manual_seed(1000 * B + 10 * F + T)
    x = torch.randn(B, F, T, generator=g).cuda()
    w = (torch.randn(32, 1, 3, 3, generator=g) * 0.3).cuda()
    gamma = (0.5 + torch.rand(32, generator=g)).cuda()
    gamma[5] = -gamma[5]                         # a negative scale: the mask follows z = raw*scale + shift, not raw
    beta = (torch.randn(32, generator=g) * 0.2).cuda()
    raw, st = ops.stem_fwd(x, w, stats=True)
    t4 = torch.empty(4, 32, device="cuda")
    ops.bn_finalize(st, B * F * T, gamma, beta, torch.zeros(32, device="cuda"), torch.ones(32, device="cuda"),
                    torch.zeros((), device="cuda", dtype=torch.int64), t4)
    amax = _slot()
    act, mask = ops.bn_apply(raw, t4[2], t4[3], relu=True, mask=True, amax_out=amax)
    torch.cuda.synchronize()
    c = dict(x=x, w=w, gamma=gamma, raw=raw, st=st, t4=t4, act=act, mask=mask, amax=amax, gen=g)
    _stem_cache[shape] = c
    return c


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_forward_pair_is_the_two_kernel_forward(shape):
    from pytorch_kaldi_resnet_amd import ops
    c = _stem_case(shape)
    st = ops.stem_stats(c["x"], c["w"])
    assert st.shape == c["st"].shape and torch.equal(st, c["st"])
    amax = _slot()
    raw, act, mask = ops.stem_fwd_apply(c["x"], c["w"], c["t4"][2], c["t4"][3], mask=True, amax_out=amax)
    assert torch.equal(raw, c["raw"])
    assert torch.equal(act, c["act"])
    assert torch.equal(mask, c["mask"])
    assert torch.equal(amax, c["amax"]) and int(amax) != 0
    # without the sign words and the slot (no-grad training-mode forward)
    raw2, act2, none = ops.stem_fwd_apply(c["x"], c["w"], c["t4"][2], c["t4"][3])
    assert none is None and torch.equal(raw2, c["raw"]) and torch.equal(act2, c["act"])


def _two_kernel_wgrad(c, d, coef, dw, accumulate):
    from pytorch_kaldi_resnet_amd import hip, ops
    t4, raw = c["t4"], c["raw"]
    draw = torch.empty_like(raw)
    hip.call("spk_bn_bwd_apply", hip.ptr(d), hip.ptr(raw), None, hip.ptr(t4[0]), hip.ptr(t4[1]), hip.ptr(t4[2]), hip.ptr(t4[3]),
             hip.ptr(coef), hip.ptr(draw), None, raw.numel() // 32, 32, MASK_RAW, None, None, hip.stream())
    return ops.stem_wgrad(c["x"], draw, dw, accumulate=accumulate)


def _backward_case(c, d):
    from pytorch_kaldi_resnet_amd import ops
    t4, raw = c["t4"], c["raw"]
    part = ops.bn_bwd_partial(d, raw, None, t4, MASK_RAW)
    coef = ops.bn_bwd_coef(part, raw.numel() // 32, c["gamma"], t4, torch.empty(32, device="cuda"), torch.empty(32, device="cuda"))
    keep = d.clone()
    for accumulate in (False, True):
        init = torch.randn(32, 1, 3, 3, generator=c["gen"]).cuda()
        dw_a = _two_kernel_wgrad(c, d, coef, init.clone(), accumulate)
        dw_b = ops.stem_bwd_wgrad(c["x"], d, raw, t4, coef, init.clone(), accumulate=accumulate)
        assert torch.isfinite(dw_a).all() and torch.equal(dw_a, dw_b), accumulate
        assert accumulate or not torch.equal(dw_b, init)
    # d is only read (bit patterns: NaN != NaN)
    assert torch.equal(d.view(torch.int32), keep.view(torch.int32))


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_backward_fused_is_apply_then_wgrad(shape):
    c = _stem_case(shape)
    d = (torch.randn(c["raw"].shape, generator=c["gen"]) * 0.1).cuda()
    _backward_case(c, d)


def test_stem_backward_drops_inf_and_nan_under_the_mask():
    c = _stem_case((3, 80, 33))
    d = (torch.randn(c["raw"].shape, generator=c["gen"]) * 0.1).cuda()
    dead = (c["raw"] * c["t4"][2] + c["t4"][3]) < -1e-3            # clearly below zero: z <= 0 whatever the contraction
    idx = dead.reshape(-1).nonzero().reshape(-1)
    assert idx.numel() > 1000
    flat = d.reshape(-1)
    flat[idx[0::3]] = float("inf")
    flat[idx[1::3]] = float("-inf")
    flat[idx[2::3]] = float("nan")
    _backward_case(c, d)


# ---- one training step with and without the fused stem, each in a child process ---------------------------------------------
def _child(out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    from helpers import VARLEN_F
    from oracle import weights as W
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    S = 10
    npst = W.make_state(41, S, VARLEN_F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, VARLEN_F, "mean+std", "AAM", 0.2, 30, arch="resnet34")
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()}, strict=True)
    m = m.cuda().train()
    x, y = W.make_input(1032, 2, VARLEN_F, 32, S)
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    eng = m.engine()
    want = os.environ["SPK_STEM_FUSED"] == "1"
    assert eng.stem_fused_fwd == want and eng.stem_fused_bwd == want
    m.attach_grads()
    with torch.no_grad():
        logits, saved = eng.forward_train(xg, yg)
        loss, dl, _ = ops.softmax_ce(logits, yg, grad_scale=0.5)
    eng.backward(saved, dl)
    torch.cuda.synchronize()
    torch.save({"loss": loss.cpu(), "grads": m.flat_grads().cpu()}, out)


def test_training_step_is_identical_with_and_without_the_fused_stem(tmp_path):
    res = []
    for v in ("0", "1"):
        out = str(tmp_path / ("step%s.pt" % v))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, SPK_STEM_FUSED=v),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        res.append(torch.load(out))
    assert torch.isfinite(res[0]["grads"]).all() and res[0]["grads"].abs().max() > 0
    assert torch.equal(res[0]["loss"], res[1]["loss"])
    assert torch.equal(res[0]["grads"], res[1]["grads"])


# ---- pooling ----------------------------------------------------------------------------------------------------------------
class _serial_pooling:
    """the serial two-pass pooling forward at every width"""

    def __enter__(self):
        from pytorch_kaldi_resnet_amd import hip
        self.lib = hip.lib()
        self.prev = self.lib.spk_stats_pool_row_form(0)

    def __exit__(self, *exc):
        self.lib.spk_stats_pool_row_form(self.prev)


def _pool_shapes():
    from pytorch_kaldi_resnet_amd import hip
    cap = hip.lib().spk_stats_pool_row_cap()
    assert cap >= 50
    # W - 1 = 1; 96 threads = a partial block; the 400-frame chunk at 256 channels; one width above the cap (the fallback)
    return [(1, 1, 2, 32), (1, 3, 38, 32), (2, 10, 50, 256), (1, 2, cap + 1, 32), (1, 2, cap, 32)]


@pytest.mark.parametrize("mode", [0, 1])
def test_pooling_rows_in_registers_are_the_serial_kernels(mode):
    from pytorch_kaldi_resnet_amd import ops
    g = torch.Generator().manual_seed(7)
    for shape in _pool_shapes():
        B, H, W, C = shape
        x = torch.rand(shape, generator=g).cuda()                 # post-ReLU values
        x[0, 0, :, 3] = 0.0                                       # a dead row
        with _serial_pooling():
            y0 = ops.stats_pool_fwd(x, mode)
        y1 = ops.stats_pool_fwd(x, mode)
        assert torch.isfinite(y1).all(), shape
        assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)), shape


@pytest.mark.parametrize("mode", [0, 1])
def test_pooling_with_lengths_rows_in_registers(mode):
    from pytorch_kaldi_resnet_amd import ops
    g = torch.Generator().manual_seed(11)
    for W in (7, 38, 50):
        x = torch.rand(3, 10, W, 64, generator=g).cuda()
        x[:, :, 7:] = float("nan")                                # frames past the shortest lengths may hold anything
        x[0] = torch.rand(10, W, 64, generator=g).cuda()
        wlen = torch.tensor([W, 1, 7], dtype=torch.int32).cuda()
        with _serial_pooling():
            y0 = ops.stats_pool_fwd(x, mode, wlen=wlen)
        y1 = ops.stats_pool_fwd(x, mode, wlen=wlen)
        assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)), W
        assert torch.isfinite(y1[0]).all() and torch.isfinite(y1[2]).all(), W
        full = ops.stats_pool_fwd(x[:1].contiguous(), mode)       # wlen = W is the plain kernel
        assert torch.equal(full[0], y1[0]), W


if __name__ == "__main__":
    _child(sys.argv[1])
