#!/usr/bin/env python3
"""Launch record of the convolution dispatch: tests/golden/dispatch/<config>.json.

For every ops._conv_launch / ops.conv_wgrad call of one model run this stores the planner-level inputs of the call (operand
shapes or None, tuple lengths and None patterns, ints and bools, whether `out` is `x`, whether the add operand is `out`) and
every C ABI launch issued inside it: entry, label and every argument named by include/spkhip.h - integers as they are, the tap
arrays as lists, the stream dropped, pointers reduced to an identity class within the call (0 = NULL, then 1, 2, ... by first
appearance of a distinct address: NULL patterns and aliasing without addresses).  Each file holds the unique records of its
config in first-seen order.  Only module globals of ops are hooked (call, _conv_launch, conv_wgrad), so the same tool records
any revision of ops.py: the committed files were written at the revision before dispatch was split from launch, and
tests/test_dispatch_cpu.py / tests/test_dispatch_gpu.py hold every later revision to them.

    python tools/make_dispatch_golden.py [config ...]        # every config, each in a fresh child process under a time limit
"""
import argparse
import contextlib
import ctypes
import inspect
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
GOLD = os.path.join(ROOT, "tests", "golden", "dispatch")
EXP_LIB = os.path.join(ROOT, "pytorch-kaldi-resnet_amd", "variants", "libspkhip_exp.so")
B, F, S = 2, 80, 10
CHILD_TIMEOUT = 300

# run: "train" = one eager AAM training step (forward, cross entropy, backward), "predict" = predict(x, lengths=...).
# lib "exp": the variant library with the experimental kernel forms (SPK_LIB), where ops._experimental() is true.
CONFIGS = {
    "r34_t300_f16x3": dict(arch="resnet34", T=300, mode="f16x3"),
    "r34_t203_f16x3": dict(arch="resnet34", T=203, mode="f16x3"),
    "r34_t300_f32": dict(arch="resnet34", T=300, mode="f32"),
    "r34_t300_bf16x6": dict(arch="resnet34", T=300, mode="bf16x6"),
    "r34_predict_len": dict(arch="resnet34", T=203, mode="f16x3", run="predict", lengths=[203, 57]),
    "r50_t300_f16x3": dict(arch="resnet50", T=300, mode="f16x3"),
    "se_r34_t300_f16x3": dict(arch="se_resnet34", T=300, mode="f16x3"),
    "r34_t300_f16x3_exp": dict(arch="resnet34", T=300, mode="f16x3", lib="exp"),
    "r34_t300_f16x3_b256": dict(arch="resnet34", T=300, mode="f16x3", B=256),       # block and slab caps; no test runs it
}


def _enc(v):
    """planner-level image of one argument: a tensor is its shape"""
    import torch
    if isinstance(v, torch.Tensor):
        return list(v.shape)
    if isinstance(v, (tuple, list)):
        return [_enc(e) for e in v]
    assert v is None or isinstance(v, (bool, int)), type(v)
    return v


@contextlib.contextmanager
def recorder(records):
    """appends the unique records of every convolution issued inside to the list `records`"""
    from helpers import header_params
    from pytorch_kaldi_resnet_amd import hip, ops
    real = {n: getattr(ops, n) for n in ("call", "_conv_launch", "conv_wgrad")}
    seen = {json.dumps(r, sort_keys=True) for r in records}
    open_calls = []           # (record, {address: class}) of the convolution calls in flight
    params = {}

    def call(name, *args, label=None, flops=0.0, nbytes=0.0):
        if open_calls:
            if name not in params:
                params[name] = header_params(name)
                assert len(params[name]) == len(hip._SIGS[name]), (name, len(params[name]), len(hip._SIGS[name]))
            assert len(args) == len(params[name]), (name, len(args), len(params[name]))
            rec, ids = open_calls[-1]
            named = {}
            for pn, ct, v in zip(params[name], hip._SIGS[name], args):
                if pn == "stream":
                    continue
                if ct is ctypes.c_void_p:
                    named[pn] = 0 if v is None else ids.setdefault(v, len(ids) + 1)
                elif ct in (ctypes.c_int, ctypes.c_longlong):
                    named[pn] = int(v)
                elif ct in (ctypes.c_float, ctypes.c_double):
                    named[pn] = float(v)
                else:
                    named[pn] = [int(e) for e in v]
            rec["launches"].append({"entry": name, "label": label or name, "args": named})
        return real["call"](name, *args, label=label, flops=flops, nbytes=nbytes)

    def wrap(fn):
        sig = inspect.signature(real[fn])

        def wrapped(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            v = b.arguments
            rec = {"fn": fn, "inputs": {n: _enc(t) for n, t in v.items()}, "launches": []}
            if fn == "_conv_launch":
                rec["inputs"]["out_is_x"] = v["out"] is v["x"]
                rec["inputs"]["add_is_out"] = v["epi_add"] is v["out"]
            open_calls.append((rec, {}))
            try:
                ret = real[fn](*a, **k)
            finally:
                open_calls.pop()
            key = json.dumps(rec, sort_keys=True)
            if key not in seen:
                seen.add(key)
                records.append(rec)
            return ret
        return wrapped

    ops.call, ops._conv_launch, ops.conv_wgrad = call, wrap("_conv_launch"), wrap("conv_wgrad")
    try:
        yield records
    finally:
        for n, f in real.items():
            setattr(ops, n, f)


def record(name):
    """run config `name` in this process -> the content of its golden file"""
    import torch
    from pytorch_kaldi_resnet_amd import hip, ops
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    cfg = CONFIGS[name]
    assert cfg.get("lib") != "exp" or os.path.abspath(hip.LIB_PATH) == EXP_LIB, "the variant library is chosen by SPK_LIB"
    nb, T = cfg.get("B", B), cfg["T"]
    old, ops.SPLIT = ops.SPLIT, ops.MFMA_MODES[cfg["mode"]]         # packed weights carry the mode: before the first forward
    try:
        m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30, arch=cfg["arch"]).cuda()
        g = torch.Generator().manual_seed(7)
        x = torch.randn(nb, F, T, generator=g).cuda()
        y = (torch.arange(nb) % S).cuda()
        records = []
        if cfg.get("run", "train") == "train":
            m.train()
            eng = m.engine()
            m.attach_grads()
            with recorder(records):
                with torch.no_grad():
                    logits, saved = eng.forward_train(x, y)
                    _, dl, _ = ops.softmax_ce(logits, y, grad_scale=1.0 / nb)
                eng.backward(saved, dl)
        else:
            m.eval()
            with recorder(records), torch.no_grad():
                m.predict(x, lengths=cfg["lengths"])
        torch.cuda.synchronize()
    finally:
        ops.SPLIT = old
    return {"config": dict(cfg, name=name), "experimental": bool(ops._experimental()), "records": records}


def dump(content, path):
    """Write a golden file.  Argument names are written once per file (the parameter names of the two hooked functions and,
    per C ABI entry, the names include/spkhip.h gives); a record is one line [function, input values, [[entry, label,
    argument values], ...]] with the values in the order of those names."""
    inputs, args = {}, {}
    lines = []
    for r in content["records"]:
        assert inputs.setdefault(r["fn"], list(r["inputs"])) == list(r["inputs"])
        for ln in r["launches"]:
            assert args.setdefault(ln["entry"], list(ln["args"])) == list(ln["args"])
        lines.append(json.dumps([r["fn"], list(r["inputs"].values()),
                                 [[ln["entry"], ln["label"], list(ln["args"].values())] for ln in r["launches"]]],
                                separators=(",", ":")))
    with open(path, "w") as f:
        f.write('{"config": %s,\n"experimental": %s,\n"inputs": %s,\n"args": %s,\n"records": [\n%s\n]}\n' % (
            json.dumps(content["config"], sort_keys=True), json.dumps(content["experimental"]), json.dumps(inputs),
            json.dumps(args), ",\n".join(lines)))


def load(path):
    """a golden file -> the content record() returns: every record with its inputs and launch arguments by name"""
    d = json.load(open(path))
    recs = [{"fn": fn, "inputs": dict(zip(d["inputs"][fn], vals)),
             "launches": [{"entry": e, "label": lab, "args": dict(zip(d["args"][e], a))} for e, lab, a in launches]}
            for fn, vals, launches in d["records"]]
    return {"config": d["config"], "experimental": d["experimental"], "records": recs}


def run_child(name, out_path, timeout=CHILD_TIMEOUT):
    """config `name` in a fresh child process under its own time limit -> its golden content, also written to out_path"""
    env = dict(os.environ)
    env.pop("SPK_LIB", None)
    if CONFIGS[name].get("lib") == "exp":
        env["SPK_LIB"] = EXP_LIB
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__), "--child", name, "--out", out_path]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, "%s: exit %d\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return load(out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=list(CONFIGS))
    ap.add_argument("--out-dir", default=GOLD)
    ap.add_argument("--child", default=None, help="(internal) record this config in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        import pytorch_kaldi_resnet_amd  # noqa: F401
        dump(record(a.child), a.out)
        return
    os.makedirs(a.out_dir, exist_ok=True)
    for name in a.configs:
        got = run_child(name, os.path.join(a.out_dir, name + ".json"))
        print("%s: %d unique records, %d launches, experimental=%s" % (
            name, len(got["records"]), sum(len(r["launches"]) for r in got["records"]), got["experimental"]), flush=True)


if __name__ == "__main__":
    main()
