"""The launch sequence of the training step and the forwards against the record (tests/golden/step/, tools/make_step_golden.py)
on a machine without a GPU: every configuration of tests/step_trace.py is recorded again - the engine and the ops wrappers run
on CPU tensors, nothing is launched, the library is never loaded - and its trace must equal the recorded one: every launch in
order with every scalar, the identity class of every pointer, and the markers where the side stream is joined.  The files were
written at the revision before the engine's unused path selectors were removed."""
import json
import os

import pytest

import step_trace as S
from conftest import GOLD

INDEX = json.load(open(os.path.join(GOLD, "step", "index.json")))


def test_the_record_covers_the_configurations():
    assert list(INDEX) == list(S.CONFIGS)
    assert sorted(f for f in os.listdir(os.path.join(GOLD, "step")) if f.endswith(".trace.json")) == \
        sorted(n + ".trace.json" for n in S.FULL)
    assert sum(os.path.getsize(os.path.join(GOLD, "step", f)) for f in os.listdir(os.path.join(GOLD, "step"))) < 300 * 1024


@pytest.mark.parametrize("name", list(S.CONFIGS))
def test_trace_equals_the_record(name):
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip, ops
    before = (hip.lib, ops.call, ops.ptr, ops.SPLIT, ops.SPLIT_BWD)
    trace = S.record(name)
    assert before == (hip.lib, ops.call, ops.ptr, ops.SPLIT, ops.SPLIT_BWD), "the recorder left a stub behind"
    got, want = S.summary(trace), INDEX[name]
    if got == want:
        if name in S.FULL:      # the full trace file is the one the digest was taken from
            assert trace == json.load(open(os.path.join(GOLD, "step", name + ".trace.json")))
        return
    if name in S.FULL:
        gold = json.load(open(os.path.join(GOLD, "step", name + ".trace.json")))
        i = next((i for i, (a, b) in enumerate(zip(trace, gold)) if a != b), min(len(trace), len(gold)))
        pytest.fail("%s: first difference at element %d of %d (recorded %d)\n  now:      %s\n  recorded: %s" % (
            name, i, len(trace), len(gold), json.dumps(trace[i]) if i < len(trace) else "(end)",
            json.dumps(gold[i]) if i < len(gold) else "(end)"))
    diff = {e: (want["entries"].get(e, 0), got["entries"].get(e, 0)) for e in sorted(set(want["entries"]) | set(got["entries"]))
            if want["entries"].get(e, 0) != got["entries"].get(e, 0)}
    pytest.fail("%s: sha256 %s, recorded %s; launches %d, recorded %d; entries whose count changed (recorded, now): %s\n"
                "the whole trace, to diff against the same dump of the parent revision: python tools/make_step_golden.py --dump %s"
                % (name, got["sha256"], want["sha256"], got["launches"], want["launches"], diff or "none (order or arguments)", name))
