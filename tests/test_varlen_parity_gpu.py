"""Variable-length training (scripts/train_resnet.py --var-chunk, BASELINE configs[3]) against the fp64 oracle.

Away from 300 frames most convolutions run on tiles the cost model in tiling.py chooses (tile_table.json only holds the shapes of
300 frames), and the tile selects the kernel form: pipelined or 16x16x32, channel planes per barrier, the weight-gradient kernel,
ragged last tiles.  This file
  * records the launch configuration of every convolution launch (helpers.record_conv_launches) of a training step at every
    chunk length of the production set P (helpers.VARLEN_*: ResNet-34 / ResNet-101, F = 80, 200..400 step 8, f16x3) and checks
    that the committed parity lengths below reach every configuration P reaches (test_sweep_covers_the_production_set);
  * checks the whole network's gradient at each committed length against the fp64 gradient of the same piecewise-linear
    function (test_model_gpu.test_backward_parity's yardstick, helpers.assert_samemask_parity), plus the f32 and bf16x6 operand
    modes at two ragged lengths;
  * checks that the per-length graph cache of variable-length training (engine.GraphedStepCache, with eviction) is the eager
    step bit for bit.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import (VARLEN_ARCHS, VARLEN_F, VARLEN_LENGTHS, assert_samemask_parity, hip_step_with_masks,  # noqa: E402
                     oracle_reference, record_conv_launches)
from oracle import weights as W  # noqa: E402

S = 10                  # speakers
POOLING, LOSS = "mean+std", "AAM"
STATE_SEED = 41

# Parity lengths, chosen by a greedy cover over the launch configurations recorded at every length of P (ResNet-34 first, then
# ResNet-101 for the configurations ResNet-34 does not reach) and pruned so that no length is redundant: dropping any one of
# them leaves a configuration unreached (test_sweep_covers_the_production_set names it).  The tiles follow the stage widths
# T, T/2, T/4, T/8, so at this quantum every length of P reaches configurations of its own, in both archs (ResNet-34: 2 to 16
# per length, ResNet-101 - Bottleneck 1x1 convolutions, stride-2 3x3 convolutions inside the block - 6 to 31; 1400 in all).
SWEEP = {
    "resnet34": [200, 208, 216, 224, 232, 240, 248, 256, 264, 272, 280, 288, 296, 304, 312, 320, 328, 336, 344, 352, 360, 368,
                 376, 384, 392, 400],
    "resnet101": [200, 208, 216, 224, 232, 240, 248, 256, 264, 272, 280, 288, 296, 304, 312, 320, 328, 336, 344, 352, 360, 368,
                  376, 384, 392, 400],
}
# the other operand modes at two ragged lengths of the ResNet-34 sweep (T / 8 = 29 and 43 frames in the last stage)
OTHER_MODES = {"f32": (232, 344), "bf16x6": (232, 344)}


def _model(arch):
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    npst = W.make_state(STATE_SEED, S, VARLEN_F, POOLING, LOSS, arch)
    m = NeuralSpeakerModel(S, VARLEN_F, POOLING, LOSS, 0.2, 30, arch=arch)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()}, strict=True)
    return m.cuda().train(), npst


def _input(B, T):
    return W.make_input(1000 + T, B, VARLEN_F, T, S)


class _mode:
    """operand mode of the convolutions for the models built inside (packed weights carry the mode)"""

    def __init__(self, name):
        from pytorch_kaldi_resnet_amd import ops
        self.ops, self.split = ops, ops.MFMA_MODES[name]

    def __enter__(self):
        self.old = self.ops.SPLIT
        self.ops.SPLIT = self.split

    def __exit__(self, *exc):
        self.ops.SPLIT = self.old


def step_keys(m, B, T):
    """launch configurations of one eager training step (forward_train + CE + backward) at batch B, T frames"""
    from pytorch_kaldi_resnet_amd import ops
    x, y = _input(B, T)
    xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    keys = set()
    eng = m.engine()
    m.attach_grads()
    with record_conv_launches(keys):
        with torch.no_grad():
            logits, saved = eng.forward_train(xg, yg)
            _, dl, _ = ops.softmax_ce(logits, yg, grad_scale=1.0 / B)
        eng.backward(saved, dl)
    torch.cuda.synchronize()
    return keys


def record_production_set():
    """{arch: {T: launch configurations}} over P at batch 2"""
    out = {}
    with _mode("f16x3"):
        for arch in VARLEN_ARCHS:
            m, _ = _model(arch)
            out[arch] = {T: step_keys(m, 2, T) for T in VARLEN_LENGTHS}
            del m
            torch.cuda.empty_cache()
    return out


def uncovered(per_len, lengths):
    """configurations of P that `lengths` do not reach -> {key: [lengths of P that reach it]}"""
    have = set().union(*(per_len[T] for T in lengths)) if lengths else set()
    miss = {}
    for T, ks in per_len.items():
        for k in ks - have:
            miss.setdefault(k, []).append(T)
    return miss


def test_sweep_lists_are_in_the_production_set():
    for arch in VARLEN_ARCHS:
        assert SWEEP[arch] and set(SWEEP[arch]) <= set(VARLEN_LENGTHS) and len(set(SWEEP[arch])) == len(SWEEP[arch]), arch
    for mode, lengths in OTHER_MODES.items():
        assert len(lengths) == 2 and set(lengths) <= set(SWEEP["resnet34"]), mode


def test_sweep_covers_the_production_set():
    rec = record_production_set()
    # ResNet-101 shares its stem and 3x3 layer shapes with ResNet-34: the two sweeps together cover the union of both archs
    per_len = {}
    for arch in VARLEN_ARCHS:
        for T, ks in rec[arch].items():
            per_len.setdefault((arch, T), set()).update(ks)
    committed = [(arch, T) for arch in VARLEN_ARCHS for T in SWEEP[arch]]
    miss = uncovered(per_len, committed)
    n_all = len(set().union(*per_len.values()))
    print("launch configurations over P: %d; reached by the %d committed lengths: %d" % (n_all, len(committed), n_all - len(miss)))
    for c in committed:     # what each committed length alone adds (a length that adds nothing is redundant)
        print("  %s T=%d: %d configurations only it reaches" % (c[0], c[1], len(uncovered(per_len, [d for d in committed if d != c]))))
    assert not miss, "launch configurations no committed parity length reaches:\n" + "\n".join(
        "  %s  <- %s" % (k, ", ".join("%s T=%d" % t for t in sorted(v))) for k, v in sorted(miss.items()))


@pytest.mark.parametrize("arch", VARLEN_ARCHS)
def test_launch_configurations_do_not_depend_on_the_batch(arch):
    """the sweep records at batch 2; training runs at 256: the launch configuration must not change with the batch"""
    T = 264
    with _mode("f16x3"):
        m, _ = _model(arch)
        k2 = step_keys(m, 2, T)
        k256 = step_keys(m, 256, T)
    assert k2 == k256, ("only at batch 2:", sorted(k2 - k256), "only at batch 256:", sorted(k256 - k2))


# ---- whole-network gradient parity at every committed length
_REF = {}


def _reference(arch, T, npst, x, y):
    """oracle parts shared by every operand mode at (arch, T); only the latest (arch, T) is kept (the parameters below run
    the modes of one length back to back)"""
    if (arch, T) not in _REF:
        _REF.clear()
        _REF[(arch, T)] = oracle_reference(npst, x, y, POOLING, LOSS, arch)
    return _REF[(arch, T)]


def _cases():
    out = []
    for arch in VARLEN_ARCHS:
        for T in SWEEP[arch]:
            out.append(pytest.param(arch, T, "f16x3", id="%s-T%d-f16x3" % (arch, T)))
            for mode, lengths in OTHER_MODES.items():
                if arch == "resnet34" and T in lengths:
                    out.append(pytest.param(arch, T, mode, id="%s-T%d-%s" % (arch, T, mode)))
    return out


@pytest.mark.parametrize("arch,T,mode", _cases())
def test_varlen_gradient_parity(arch, T, mode):
    B = 2
    x, y = _input(B, T)
    with _mode(mode):
        m, npst = _model(arch)
        _, hip, masks_hip, logits = hip_step_with_masks(m, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(),
                                                        return_logits=True)
    ref = _reference(arch, T, npst, x, y)
    assert_samemask_parity(ref, npst, x, y, POOLING, LOSS, arch, hip, masks_hip, logits_hip=logits,
                           tag="%s T=%d %s" % (arch, T, mode))


# ---- the per-length graph cache of variable-length training
def test_graph_cache_equals_eager_step():
    """engine.GraphedStepCache with room for two graphs against an eager twin, SGD between batches, over a length sequence that
    evicts a graph and captures that length again: loss, gradient arena, parameters after the update and a BatchNorm running
    mean bit for bit after every step; the owner of the shared memory pool is never evicted."""
    from pytorch_kaldi_resnet_amd.engine import GraphedStepCache
    from pytorch_kaldi_resnet_amd.optim import FlatSGD
    B, arch = 2, "resnet34"
    seq = [200, 304, 200, 256, 304, 200]
    # LRU with two slots, the first graph (the pool owner) re-queued instead of dropped: 304 is evicted by 256, 256 by 304
    captures = [1, 2, 2, 3, 4, 4]
    resident = [{200}, {200, 304}, {200, 304}, {200, 256}, {200, 304}, {200, 304}]
    with _mode("f16x3"):
        me, _ = _model(arch)
        mg, _ = _model(arch)
        oe = FlatSGD(me, 1e-2, momentum=0.9, weight_decay=5e-4)
        og = FlatSGD(mg, 1e-2, momentum=0.9, weight_decay=5e-4)
        cache = GraphedStepCache(mg.engine(), max_graphs=2, warmup=1)
        owner = None
        for s, T in enumerate(seq):
            x, y = W.make_input(2000 + s, B, VARLEN_F, T, S)
            xg, yg = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
            oe.zero_grad(set_to_none=True)
            l1, _, _ = me.engine().loss_and_grad(xg, yg)
            l2, _, _ = cache(xg, yg)
            assert float(l1) == float(l2), (s, T, float(l1), float(l2))
            assert torch.equal(me.flat_grads(), mg.flat_grads()), (s, T)
            oe.step()
            og.step()
            assert torch.equal(me.flat_parameters(), mg.flat_parameters()), (s, T)
            rm = "res.layer4.2.bn2.running_mean"
            assert torch.equal(me.state_dict()[rm], mg.state_dict()[rm]), (s, T)
            if owner is None:
                owner = cache._pool_owner
            assert cache._pool_owner is owner and owner in cache.steps.values(), s
            assert cache.captures == captures[s], (s, cache.captures)
            assert {k[1] for k in cache.steps} == resident[s], (s, list(cache.steps))
            assert len(cache) <= 2
