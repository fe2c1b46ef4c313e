"""Launch trace of whole training steps and forwards, recorded on a machine without a GPU and without libspkhip.so (test
infrastructure only; tools/make_step_golden.py writes tests/golden/step/ from it, tests/test_step_trace_cpu.py and
tests/test_step_trace_gpu.py hold engine.py and ops.py to those files).

The engine and the real ops wrappers run end to end on CPU tensors while `stubbed()` replaces, for the duration of one recording,
the few module globals that need a device or the library.  A trace is a list of [entry, label, [args...]] in launch order: the
integers and floats as they are, the tap arrays as lists, the stream dropped, and every pointer as the identity class of its
address - 0 = NULL, then 1, 2, ... by first appearance over the whole recording - so that the trace holds the data flow between
launches (which buffer feeds which launch, in-place aliasing, the AmaxPool slot each launch gets) and no address.  Two kinds of
marker elements sit in the same list: [JOIN, "", []] every time Engine._join_wgrad is called and [STAGE, name, []] every time
the on_stage_done callback fires - where the side stream is joined relative to the launches.

Only module globals are hooked, so this file records any revision of engine.py and ops.py."""
import contextlib
import ctypes
import hashlib
import itertools
import json

import torch

from helpers import header_params

B, F, T, SPEAKERS = 3, 30, 37, 5            # odd shapes (tests/test_model_gpu.py::test_odd_shapes_against_oracle): every stride-2
LENGTHS = [37, 11, 24]                      # stage rounds up; B = 3 tells per-utterance SE tables from per-batch ones
JOIN, STAGE = "@join_wgrad", "@stage_done"

# What the fake library answers.  These values only size scratch and partial-sum buffers; no engine decision reads them.
LIB_CONSTANTS = {"spk_pack_job_bytes": 48, "spk_build_flags": 0}
LIB_DEFAULT = 4                             # every other helper; spk_conv1x1_stream_rows(n, c) -> n


class _FakeLib:
    def __getattr__(self, name):
        if not name.startswith("spk_"):
            raise AttributeError(name)
        if name == "spk_conv1x1_stream_rows":
            return lambda n, c: n
        return lambda *a: LIB_CONSTANTS.get(name, LIB_DEFAULT)


# ---- configurations ----------------------------------------------------------------------------------------------------------
ARCHS = ("resnet18", "resnet50", "se_resnet34")
MODES = {"f16x3": ("f16x3", None), "f32": ("f32", None), "bf16x6": ("bf16x6", None), "f16x3_bwdf32": ("f16x3", "f32")}
SETTINGS = {
    "default": {},
    "nochan": {"chan_amax": False},
    "stem00": {"stem_fused_fwd": False, "stem_fused_bwd": False},
    "stem10": {"stem_fused_fwd": True, "stem_fused_bwd": False},
    "stem01": {"stem_fused_fwd": False, "stem_fused_bwd": True},
    "maxc": {"fuse_apply_max_c": 1000000},              # (f16x3 only: the other modes have no limit to lift)
}
HEADS = {"mean_softmax": ("mean", "softmax"), "aamv1": ("mean+std", "AAM-v1")}      # besides the default ("mean+std", "AAM")


def _configs():
    out = {}
    for arch, mode, setting in itertools.product(ARCHS, MODES, SETTINGS):
        if setting == "maxc" and mode != "f16x3":
            continue
        out["%s-%s-%s" % (arch, mode, setting)] = dict(arch=arch, mode=mode, setting=setting, head=("mean+std", "AAM"))
    for hname, head in HEADS.items():
        out["resnet18-f16x3-default-%s" % hname] = dict(arch="resnet18", mode="f16x3", setting="default", head=head)
    return out


CONFIGS = _configs()
FULL = ("resnet18-f16x3-default", "resnet18-f32-default")        # configurations whose whole trace is kept, not only its digest


# ---- recording -----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def stubbed(trace, mode="f16x3"):
    """Everything inside runs the engine on CPU tensors and appends to `trace` instead of launching.  Replaced and restored on
    exit: hip.lib, ops.call, ops.ptr, ops._ptr_rows, ops.stream, ops._check_wlen (it insists on a device tensor),
    torch.cuda.current_stream, torch.cuda.is_current_stream_capturing, ops.SPLIT / ops.SPLIT_BWD (set from `mode`) and the
    content of ops' workspace caches (emptied first: the class numbering must not depend on what ran earlier in the process)."""
    from pytorch_kaldi_resnet_amd import hip, ops
    fwd, bwd = MODES[mode]
    classes, alive, params = {}, [], {}

    def ptr(t):
        if t is None:
            return None
        assert t.is_contiguous(), "libspkhip takes contiguous tensors only"
        return _cls(t)

    def _cls(t):
        alive.append(t)                  # no address is reused within a recording
        return classes.setdefault(t.data_ptr(), len(classes) + 1)

    def call(name, *args, label=None, flops=0.0, nbytes=0.0):
        if name not in params:
            params[name] = header_params(name)
            assert len(params[name]) == len(hip._SIGS[name]), (name, len(params[name]), len(hip._SIGS[name]))
        assert len(args) == len(params[name]), (name, len(args), len(params[name]))
        vals = []
        for pn, ct, v in zip(params[name], hip._SIGS[name], args):
            if pn == "stream":
                continue
            if ct is ctypes.c_void_p:
                vals.append(0 if v is None else int(v))
            elif ct in (ctypes.c_int, ctypes.c_longlong):
                vals.append(int(v))
            elif ct in (ctypes.c_float, ctypes.c_double):
                vals.append(float(v))
            else:
                vals.append([int(e) for e in v])
        trace.append([name, label or name, vals])

    class _Stream:
        cuda_stream = 0

    new = [(hip, "lib", lambda: _FakeLib()), (ops, "call", call), (ops, "ptr", ptr), (ops, "_ptr_rows", _cls),
           (ops, "stream", lambda: 0), (ops, "_check_wlen", lambda wlen, B: None),
           (torch.cuda, "current_stream", lambda *a: _Stream()), (torch.cuda, "is_current_stream_capturing", lambda: False),
           (ops, "SPLIT", ops.MFMA_MODES[fwd]), (ops, "SPLIT_BWD", None if bwd is None else ops.MFMA_MODES[bwd])]
    old = [(o, n, getattr(o, n)) for o, n, _ in new]
    caches = [(c, c.copy()) for c in (ops._ws_cache, ops._ws64_cache, ops._ws_retired)]
    try:
        for o, n, v in new:
            setattr(o, n, v)
        for c, _ in caches:
            c.clear()
        yield trace
    finally:
        for o, n, v in old:
            setattr(o, n, v)
        for c, saved in caches:
            c.clear()
            c.update(saved) if isinstance(c, dict) else c.extend(saved)


def train_step(eng, x, y, trace=None):
    """forward_train, cross entropy and backward of one batch, as an eager step runs them; with `trace` the markers go there
    -> (logits, loss rows)"""
    from pytorch_kaldi_resnet_amd import ops
    with torch.no_grad():
        logits, saved = eng.forward_train(x, y)
        loss_row, dl, _ = ops.softmax_ce(logits, y, grad_scale=1.0 / logits.shape[0])
    eng.backward(saved, dl, None if trace is None else (lambda name: trace.append([STAGE, name, []])))
    return logits, loss_row


def record(name):
    """configuration `name` -> its trace: two training steps on one model (the first backward attaches the gradient views and
    overwrites, the second takes every accumulate path), one no-grad training-mode forward, one eval forward and one
    length-masked eval forward"""
    from pytorch_kaldi_resnet_amd.engine import Engine
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    cfg = CONFIGS[name]
    trace = []
    with stubbed(trace, cfg["mode"]), contextlib.redirect_stdout(None):
        m = NeuralSpeakerModel(SPEAKERS, F, cfg["head"][0], cfg["head"][1], 0.2, 30, arch=cfg["arch"]).train()
        eng = m.engine()
        eng.use_side_stream = False
        for k, v in SETTINGS[cfg["setting"]].items():
            setattr(eng, k, v)
        join = eng._join_wgrad
        eng._join_wgrad = lambda: (trace.append([JOIN, "", []]), join())[1]
        x = torch.zeros(B, F, T)
        y = torch.arange(B) % SPEAKERS
        for _ in range(2):
            train_step(eng, x, y, trace)
        with torch.no_grad():
            eng._embed_train(x, save=False)
            eng.embed_eval(x)
            eng.embed_eval(x, Engine.stage_widths(LENGTHS, B, T, "cpu"))
    return trace


def first_step(trace):
    """the (entry, label) column of the first training step of a trace: up to the first time the stem stage is reported done"""
    end = trace.index([STAGE, "stem", []])
    return [(e, lab) for e, lab, _ in trace[:end] if not e.startswith("@")]


@contextlib.contextmanager
def launch_labels(log):
    """pass-through wrapper around ops.call: every launch still runs and adds its (entry, label) to the list `log`"""
    from pytorch_kaldi_resnet_amd import ops
    real = ops.call

    def call(name, *args, label=None, flops=0.0, nbytes=0.0):
        log.append((name, label or name))
        return real(name, *args, label=label, flops=flops, nbytes=nbytes)

    ops.call = call
    try:
        yield log
    finally:
        ops.call = real


# ---- the golden files ------------------------------------------------------------------------------------------------------------
def summary(trace):
    """what is kept of every configuration: the sha256 of the canonical JSON of the trace, the launch count, the count per entry"""
    entries = {}
    for e, _, _ in trace:
        if not e.startswith("@"):
            entries[e] = entries.get(e, 0) + 1
    digest = hashlib.sha256(json.dumps(trace, separators=(",", ":")).encode()).hexdigest()
    return {"sha256": digest, "launches": sum(entries.values()), "entries": dict(sorted(entries.items()))}


def dump_trace(trace, path):
    """one launch (or marker) per line"""
    with open(path, "w") as f:
        f.write("[\n%s\n]\n" % ",\n".join(json.dumps(el, separators=(",", ":")) for el in trace))
