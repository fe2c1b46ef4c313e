"""The CPU launch record (tests/golden/step/, tests/step_trace.py) against what the card really gets: one eager training step
of the recorded resnet18 / f16x3 / default configuration, with the weight gradients on the main stream and on the side stream.
The ordered (entry, label) list of both runs must be the first step of the recorded trace - the fake library and the stubs of
the CPU recording change no decision - and the two runs must agree bit for bit."""
import json
import os

import pytest
import torch

import step_trace as S
from conftest import GOLD

NAME = "resnet18-f16x3-default"


def _step(side_stream):
    from pytorch_kaldi_resnet_amd import ops
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    cfg = S.CONFIGS[NAME]
    assert ops.SPLIT == ops.MFMA_MODES["f16x3"] and ops.SPLIT_BWD is None, "the suite runs in the default operand mode"
    torch.manual_seed(11)
    m = NeuralSpeakerModel(S.SPEAKERS, S.F, cfg["head"][0], cfg["head"][1], 0.2, 30, arch=cfg["arch"]).cuda().train()
    x = torch.randn(S.B, S.F, S.T, generator=torch.Generator().manual_seed(5)).cuda()
    y = (torch.arange(S.B) % S.SPEAKERS).cuda()
    eng = m.engine()
    eng.use_side_stream = side_stream
    log = []
    with S.launch_labels(log):
        logits, loss_row = S.train_step(eng, x, y)
    torch.cuda.synchronize()
    return log, loss_row.clone(), logits.clone(), m.flat_grads().clone()


@pytest.mark.gpu
def test_eager_step_launches_the_recorded_sequence():
    want = S.first_step(json.load(open(os.path.join(GOLD, "step", NAME + ".trace.json"))))
    runs = [_step(False), _step(True)]
    for log, _, _, _ in runs:
        i = next((i for i, (a, b) in enumerate(zip(log, want)) if a != b), min(len(log), len(want)))
        assert log == want, "first difference at launch %d: launched %s, recorded %s" % (
            i, log[i] if i < len(log) else "(end)", want[i] if i < len(want) else "(end)")
    (_, loss0, logits0, g0), (_, loss1, logits1, g1) = runs
    assert torch.isfinite(g0).all() and float(g0.abs().max()) > 0
    assert torch.equal(loss0, loss1) and torch.equal(logits0, logits1) and torch.equal(g0, g1)
