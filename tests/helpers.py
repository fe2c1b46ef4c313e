"""Helpers shared by the GPU parity tests (test infrastructure only)."""
import contextlib
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The production set of variable-length training that tests/test_varlen_parity_gpu.py sweeps: scripts/train_resnet.py
# --var-chunk at its default --min-chunk-size / --max-chunk-size / --chunk-quantum (tests/test_varlen_range_cpu.py pins them),
# F = 80, f16x3 operands, AAM head, mean+std pooling.
VARLEN_MIN, VARLEN_MAX, VARLEN_QUANTUM = 200, 400, 8
VARLEN_LENGTHS = tuple(range(VARLEN_MIN, VARLEN_MAX + 1, VARLEN_QUANTUM))
VARLEN_ARCHS = ("resnet34", "resnet101")
VARLEN_F = 80


def hip_relu_masks(eng, saved):
    """The ReLU masks the HIP training forward chose, in the call order of the reference forward (scripts/model.py:250,
    48-64 / 115-135 per block, head :361-363) - the masks the backward kernels differentiate with.  Inner masks come from the
    same fused multiply-add the kernels use (spk_bn_apply); block-output masks from the stored block outputs."""
    from pytorch_kaldi_resnet_amd import ops
    nchw = lambda t: (t > 0).permute(0, 3, 1, 2).cpu()      # noqa: E731
    masks = [nchw(saved["blocks"][0]["x"])]
    for b, rec in zip(eng.blocks, saved["blocks"]):
        for raw, bn in zip(rec["raws"][:-1], b.bns[:-1]):
            masks.append(nchw(ops.bn_apply(raw, bn.t4[2], bn.t4[3], relu=True)))
        masks.append(nchw(rec["out"]))
    if "h" in saved["head"]:
        masks.append((saved["head"]["h"] > 0).cpu())
    return masks


def hip_step_with_masks(m, xg, yg, return_logits=False):
    """forward + CE + backward through the engine, also returning the ReLU masks the HIP forward chose, in the call
    order of the reference forward (scripts/model.py:250, 48-64 / 115-135 per block, head :361-363): the masks the
    backward kernels differentiate with.  Inner masks come from the same fused multiply-add the kernels use
    (spk_bn_apply); block-output masks from the stored block outputs.
    -> (loss, {name: grad (float64, CPU)}, masks) (+ the train-mode logits on the CPU with return_logits)."""
    from pytorch_kaldi_resnet_amd import ops
    eng = m.engine()
    m.attach_grads()
    for p in m.parameters():
        p.grad = None
    with torch.no_grad():
        logits, saved = eng.forward_train(xg.contiguous(), yg)
        masks = hip_relu_masks(eng, saved)
        loss_row, dl, _ = ops.softmax_ce(logits, yg, grad_scale=1.0 / logits.shape[0])
        loss = float(ops.mean(loss_row))
        lg = logits.detach().cpu() if return_logits else None
    eng.backward(saved, dl)
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}
    return (loss, grads, masks, lg) if return_logits else (loss, grads, masks)


# ---- same-mask fp64 gradient parity (the yardstick of test_model_gpu.test_backward_parity, without the golden norms)
def oracle_reference(npst, x, y, pooling, loss, arch):
    """The parts of the yardstick that do not depend on the implementation under test: the CPU fp32 oracle with its own
    masks, measured against the fp64 gradient under those masks, and the fp64 forward with its own masks.  The fp32 / fp64
    gradient dicts are reduced to the scalars the assertions need; the fp64 gradient and masks are kept."""
    from oracle import masked
    from oracle import spk_oracle as O
    kw = dict(pooling=pooling, loss=loss, arch=arch)

    def own(dtype):
        st = O.to_torch_state(npst)
        st = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in st.items()}
        keys = O.trainable_keys(st)
        for k in keys:
            st[k].requires_grad_(True)
        lo, mk = masked.record_masks(st, torch.from_numpy(x).to(dtype), torch.from_numpy(y), **kw)
        lv = O.cross_entropy(lo, torch.from_numpy(y))
        gs = torch.autograd.grad(lv, [st[k] for k in keys])
        return {k: v.double() for k, v in zip(keys, gs)}, mk, lo.detach().double()

    g32, masks32, _ = own(torch.float32)
    g64, masks64, logits64 = own(torch.float64)
    _, ref_32 = masked.grads(npst, x, y, masks=masks32, **kw)
    names = list(g64)
    floor = 1e-3 * max(float(ref_32[n].norm()) for n in names)
    return {
        "names": names, "g64": g64, "masks64": masks64, "logits64": logits64,
        "e_cpu": rel_err(g32, ref_32, names),
        "worst_cpu": max(float((g32[n] - ref_32[n]).norm() / max(float(ref_32[n].norm()), floor)) for n in names),
        "e_free_cpu": rel_err(g32, g64, names),
        "flips_cpu": sum(int((a != b).sum()) for a, b in zip(masks32, masks64)),
    }


def rel_err(a, b, names):
    fa = torch.cat([a[n].reshape(-1) for n in names])
    fb = torch.cat([b[n].reshape(-1) for n in names])
    return float((fa - fb).norm() / fb.norm())


def assert_samemask_parity(ref, npst, x, y, pooling, loss, arch, hip, masks_hip, logits_hip=None, bound=3.0, tag=""):
    """test_backward_parity's assertions (1)-(3) against `ref` = oracle_reference(...) for a HIP step (hip_step_with_masks):
    (1) the HIP gradient against the fp64 gradient under the HIP forward's own masks within `bound` x the CPU fp32 path's error
        under the same yardstick, overall and per tensor, no additive slack beyond test_backward_parity's 1e-5 on the per-tensor
        ratio; (2) the ReLU-mask flip count against the fp64 forward; (3) the free-running budget.  With logits_hip: the
        train-mode logits within 2e-4 (scale-relative) of the fp64 oracle.  -> the measured figures."""
    from oracle import masked
    names = ref["names"]
    assert sorted(hip) == sorted(names), tag
    masks64 = ref["masks64"]
    assert [tuple(a.shape) for a in masks_hip] == [tuple(a.shape) for a in masks64], tag
    _, ref_hip = masked.grads(npst, x, y, masks=masks_hip, pooling=pooling, loss=loss, arch=arch)
    e_hip = rel_err(hip, ref_hip, names)
    floor = 1e-3 * max(float(ref_hip[n].norm()) for n in names)
    per = {n: float((hip[n] - ref_hip[n]).norm() / max(float(ref_hip[n].norm()), floor)) for n in names}
    worst_name = max(per, key=per.get)
    worst = per[worst_name]
    print("%s same-mask gradient error vs fp64: hip %.3e (worst tensor %.3e, %s)  cpu-fp32 %.3e (worst tensor %.3e)" % (
        tag, e_hip, worst, worst_name, ref["e_cpu"], ref["worst_cpu"]))
    assert e_hip <= bound * ref["e_cpu"], (tag, e_hip, ref["e_cpu"])
    assert worst <= bound * ref["worst_cpu"] + 1e-5, (tag, worst_name, worst, ref["worst_cpu"])
    n_el = sum(a.numel() for a in masks64)
    flips_hip = sum(int((a != b).sum()) for a, b in zip(masks_hip, masks64))
    print("%s ReLU masks differing from the fp64 forward: hip %d, cpu-fp32 %d of %d" % (tag, flips_hip, ref["flips_cpu"], n_el))
    assert flips_hip <= 3 * ref["flips_cpu"] + 2e-6 * n_el + 4, (tag, flips_hip, ref["flips_cpu"], n_el)
    smallest = min(a.numel() for a in masks64)
    e_free = rel_err(hip, ref["g64"], names)
    print("%s free-running gradient error vs fp64: hip %.3e cpu-fp32 %.3e" % (tag, e_free, ref["e_free_cpu"]))
    assert e_free <= 3.0 * ref["e_free_cpu"] + 2.0 * (flips_hip / smallest) ** 0.5 + 3.0 * e_hip, (tag, e_free)
    out = {"e_hip": e_hip, "worst": worst, "flips": flips_hip, "e_free": e_free}
    if logits_hip is not None:
        lo = ref["logits64"]
        out["logits_srel"] = float((logits_hip.double() - lo).abs().max() / lo.abs().max())
        assert out["logits_srel"] < 2e-4, (tag, out["logits_srel"])
    return out


# ---- launch-configuration recorder: which kernel form, tile and edge case every convolution launch of a step takes
CONV_LAUNCHES = ("spk_conv_mfma", "spk_conv_mfma_len", "spk_conv1x1_stream", "spk_conv3x3_c32_stream", "spk_conv_wgrad",
                 "spk_stem_conv_fwd", "spk_stem_conv_fwd_len", "spk_stem_conv_wgrad")


def header_params(name):
    """parameter names of `int name(...)` in include/spkhip.h, in order"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spkhip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m is not None, "%s is not declared in include/spkhip.h" % name
    return [re.findall(r"\w+", p)[-1] for p in m.group(1).split(",")]


def conv_launch_key(name, a, label):
    """Launch configuration of one convolution launch (`a`: argument name -> value, named by include/spkhip.h): the kernel and
    its template (the ops label), channels, taps, strides, tile, register tile, form / fusion flags, operand mode and whether
    the last tile row / column is ragged.  B, pointers, grid sizes and the weight gradient's slab count stay out: they do not
    select code."""
    lab = label or name
    if name in ("spk_conv_mfma", "spk_conv_mfma_len"):
        f = [("Cin", a["Cin"]), ("Cout", a["Cout"]), ("taps", a["ntaps"]), ("IS", a["IS"]), ("OS", a["OS"]), ("ips", a["ips"]),
             ("oo", "%d%d" % (a["ooy"], a["oox"])), ("TH", a["TH"]), ("TW", a["TW"]), ("MT", a["MT"]), ("NT", a["NT"]),
             ("kc", a["kc"]), ("flags", hex(a["flags"])), ("split", a["split"]),
             ("ragH", int(a["OH"] % a["TH"] != 0)), ("ragW", int(a["OW"] % a["TW"] != 0))]
    elif name == "spk_conv_wgrad":
        f = [("Cin", a["Cin"]), ("Cout", a["Cout"]), ("k", a["ksize"]), ("IS", a["stride"]), ("TH", a["TH"]), ("TW", a["TW"]),
             ("WN", a["WN"]), ("flags", hex(a["flags"])), ("split", a["split"]),
             ("ragH", int(a["OH"] % a["TH"] != 0)), ("ragW", int(a["OW"] % a["TW"] != 0))]
    elif name == "spk_conv3x3_c32_stream":          # 8 x 16 pixel tiles (ops._plan_conv)
        f = [("Cin", 32), ("Cout", 32), ("k", 3), ("flags", hex(a["flags"])),
             ("ragH", int(a["H"] % 8 != 0)), ("ragW", int(a["W"] % 16 != 0))]
    elif name == "spk_conv1x1_stream":              # pixel-linear tiles over B * H * W: the ragged tail depends on B
        f = [("Cin", a["C"]), ("Cout", a["C"]), ("k", 1), ("flags", hex(a["flags"]))]
    else:                                           # stem: pixel-linear blocks over B * F * T
        f = [("flags", hex(a["flags"]))] if "flags" in a else []
    return " ".join([name, lab] + ["%s=%s" % kv for kv in f])


@contextlib.contextmanager
def record_conv_launches(keys):
    """Pass-through wrapper around ops.call: every launch still runs; each convolution launch adds its conv_launch_key to the
    set `keys`.  The argument count of every recorded entry is checked against include/spkhip.h (and the ctypes binding), so a
    signature change fails here instead of being mis-parsed; a convolution entry this recorder does not know fails too."""
    from pytorch_kaldi_resnet_amd import hip, ops
    params = {n: header_params(n) for n in CONV_LAUNCHES}
    for n, p in params.items():
        assert len(p) == len(hip._SIGS[n]), (n, len(p), len(hip._SIGS[n]))
    real = ops.call

    def call(name, *args, label=None, flops=0.0, nbytes=0.0):
        if name in params:
            assert len(args) == len(params[name]), (name, len(args), len(params[name]))
            keys.add(conv_launch_key(name, dict(zip(params[name], args)), label))
        else:
            assert not name.startswith(("spk_conv", "spk_stem_conv")), "convolution launch unknown to the recorder: " + name
        return real(name, *args, label=label, flops=flops, nbytes=nbytes)

    ops.call = call
    try:
        yield keys
    finally:
        ops.call = real


# ---- f16 pair tensors and scale slots of the f16x3 operand mode (host restatements used by the kernel tests)
def slot():
    return torch.zeros(1, device="cuda", dtype=torch.int32)


def sigma_of(slot_t):
    """host copy of spk_sigma_from_amax_bits"""
    bits = int(slot_t.cpu().view(torch.int32)[0]) & 0xFFFFFFFF
    e = (bits >> 23) & 0xFF
    if e in (0, 255):
        return 1.0
    se = min(max(127 + 14 - (e - 127), 1), 254)          # the result stays a finite normal float32 (amax < 2^-113: 2^127)
    return 2.0 ** (se - 127)


def slot_value(slot_t):
    return float(slot_t.cpu().view(torch.float32)[0])


def encode_pairs(t32, sig):
    """host restatement of split2h + the pair layout: [.., 4k..4k+3] floats -> [4 x fp16 hi][4 x fp16 lo] of value * sigma"""
    u = (t32.double() * sig).float().clamp(-65504.0, 65504.0)       # sigma is a power of two: exact
    hi = u.half()
    lo = (u - hi.float()).half()
    g = t32.shape[-1] // 4
    hi = hi.reshape(-1, g, 4)
    lo = lo.reshape(-1, g, 4)
    return torch.cat([hi, lo], dim=-1).reshape(-1).view(torch.float32).reshape(t32.shape)


def decode_pairs(tp, sig):
    h = tp.reshape(-1).view(torch.float16).reshape(-1, 8)
    return ((h[:, :4].double() + h[:, 4:].double()) / sig).reshape(tp.shape)
