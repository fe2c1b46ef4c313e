"""The compile-time flag variants of the downsample-block launches (csrc/conv_split.hip, conv_pipe.hip, conv_wgrad_split.hip) and
the slab reduce (csrc/conv_wgrad.hip) on a real MI355X.

Every case is the smallest launch that reaches one variant with the flag word the training step gives it: batch 2, 32 -> 64 and
64 -> 128 channels, 9 x 11 and 10 x 12 maps (odd and even extents under the stride-2 ceil, unequal parity classes), a 4 x 4 tile
that leaves the last tile partial on both axes, the register tile forced to the one the step runs.  The same cases run in this
process (variants on) and in ONE child process with SPK_FL_VARIANTS=0 (every launch generic): outputs, statistics rows and absmax
slots are compared byte for byte, each launch is asked which instance it takes (spk_conv_variant_of / spk_wgrad_variant_of), and
every output is held to the fp64 restatement of tests/conv_ref.py with the bounds of tests/test_conv_edges_gpu.py - a variant and
a generic instance that are wrong together do not pass.  (None of these variants has a side output: those belong to the fused
BatchNorm-backward variants, which tests/test_c32_whole_pixel_gpu.py and tests/test_conv_edges_gpu.py cover.)

The slab reduce is compared byte for byte with a float32 numpy emulation of its four chains (exact: tolerance zero).

    python tests/test_flag_variants_gpu.py OUT.npz        # the child: runs the cases in this process, writes every array"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import conv_ref as R  # noqa: E402
from helpers import encode_pairs, header_params, sigma_of, slot  # noqa: E402

pytestmark = pytest.mark.gpu

B = 2
MAPS = [(9, 11), (10, 12)]
TILE = (4, 4)            # output map 5 x 6 (5 x 5, 4 x 6, 4 x 5 for the parity classes): the last tile is partial on both axes
EPI_ADD, EPI_STATS, IN_PRESPLIT = 4, 16, 1 << 14
NSLABS = (1, 3, 4, 5, 15, 16, 17, 33, 256)
# ksize, Cin, Cout of the reduce: 9 * 32 * 32 weights, the 1x1 32 -> 64 shortcut, and 135 weights (no multiple of the 256-thread block)
REDUCE_SIZES = [(3, 32, 32), (1, 32, 64), (3, 3, 5)]


def conv_cases():
    """(kind, Cin, Cout, register tile, pipelined kernel allowed, kernel, FL of the variant).  Cin / Cout: of the CONVOLUTION (a data
    gradient launches with the roles swapped)."""
    return [
        # 3x3 stride 2 forward with statistics: (1, 2) at 64 channels, (1, 4) at 128 on conv_mfma_kernel (where the pipelined kernel
        # takes that launch it runs generic: its variant was measured and dropped)
        ("fwd3", 32, 64, (1, 2), True, "conv_mfma_kernel<1,2,", EPI_STATS),
        ("fwd3", 64, 128, (1, 4), False, "conv_mfma_kernel<1,4,", EPI_STATS),
        # 1x1 stride 2 forward with statistics (the shortcut): (1, 2), and the (3, 2) tile of the 256-channel block
        ("fwd1", 32, 64, (1, 2), True, "conv_mfma_kernel<1,2,", EPI_STATS),
        ("fwd1", 64, 128, (3, 2), True, "conv_mfma_kernel<3,2,", EPI_STATS),
        # 3x3 stride 2 data gradient, pair input: four parity launches each
        ("dgrad3", 32, 64, (2, 1), True, "conv_mfma_kernel<2,1,", IN_PRESPLIT),
        ("dgrad3", 64, 128, (2, 2), True, "conv_mfma_kernel<2,2,", IN_PRESPLIT),
        ("dgrad3", 64, 128, (3, 2), True, "conv_mfma_kernel<3,2,", IN_PRESPLIT),
        # 1x1 stride 2 data gradient accumulated onto a pre-filled dx
        ("dgrad1", 32, 64, (2, 1), True, "conv_mfma_kernel<2,1,", EPI_ADD),
        ("dgrad1", 64, 128, (2, 2), True, "conv_mfma_kernel<2,2,", EPI_ADD),
        ("dgrad1", 64, 128, (3, 2), True, "conv_mfma_kernel<3,2,", EPI_ADD),
    ]


def wgrad_cases():
    """(kind, Cin, Cout, (TH, TW, WN), kernel, VAR).  3x3 stride 2 with a pair dY on the large prefetch window (halo 9 x 17 = 153 and
    11 x 13 = 143 pixels: the step's two tiles), 1x1 stride 2 with a plain dY on the small one (64 -> 128 goes to the grouped 1x1
    kernel: another family)."""
    return [
        ("wgrad3", 32, 64, (4, 8, 2), "conv_wgrad_split_kernel<9,2,2,3,5>", 2),
        ("wgrad3", 32, 64, (5, 6, 2), "conv_wgrad_split_kernel<9,2,2,3,5>", 2),
        ("wgrad3", 64, 128, (4, 8, 2), "conv_wgrad_split_kernel<9,2,2,3,5>", 2),
        ("wgrad1", 32, 64, (1, 6, 2), "conv_wgrad_split_kernel<1,2,2,3,4>", 0),
    ]


def case_name(kind, Cin, Cout, tile, extra, hw):
    return "%s %d->%d %s%s %dx%d" % (kind, Cin, Cout, "x".join(str(t) for t in tile), "" if extra else " nopipe", hw[0], hw[1])


def inputs(kind, Cin, Cout, hw):
    """the tensors of one case, NCHW on the CPU (shared by the runs and the oracle, never modified)"""
    k = 3 if kind.endswith("3") else 1
    H, Wd = hw
    OH, OW = R.out_hw(H, Wd, k, 2)
    x, w = R.conv_inputs(701 + k, B, Cin, Cout, H, Wd, k)
    return dict(k=k, x=x, w=w, dy=R.tensor(711 + k, False, B, Cout, OH, OW), prev=R.tensor(721 + k, False, B, Cin, H, Wd), OH=OH, OW=OW)


@contextlib.contextmanager
def patched(obj, **kw):
    old = {k: getattr(obj, k) for k in kw}
    for k, v in kw.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


@contextlib.contextmanager
def launches(ops):
    """pass-through recorder of ops.call: (entry, {argument name: value}, label) of every launch"""
    rec, real = [], ops.call

    def call(name, *args, label=None, flops=0.0, nbytes=0.0):
        rec.append((name, dict(zip(header_params(name), args)), label))
        return real(name, *args, label=label, flops=flops, nbytes=nbytes)
    ops.call = call
    try:
        yield rec
    finally:
        ops.call = real


def variant_of(lib, name, a):
    if name == "spk_conv_wgrad":
        return lib.spk_wgrad_variant_of(a["ksize"], a["stride"], a["TH"], a["TW"], a["WN"], a["split"], a["flags"])
    ptrs = sum(1 << i for i, p in enumerate(("add_mask", "bn_mask", "in_mask", "in_act", "bn_act", "side_dz")) if a[p])      # SPK_PTR_*
    return lib.spk_conv_variant_of(a["MT"], a["NT"], a["split"], a["flags"], ptrs)


def G(t):
    return R.nhwc(t).cuda()


def filled(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def run_cases():
    """every case in this process -> ({array name: numpy array}, {case name: [(label, instance) of its launches]})"""
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip, ops, tiling
    lib = hip.lib()
    out, inst = {}, {}
    assert ops.SPLIT == 3 and ops.SPLIT_BWD is None, "the cases are the f16x3 launches of the training step"
    for hw in MAPS:
        H, Wd = hw
        for kind, Cin, Cout, (MT, NT), pipe, kernel, _ in conv_cases():
            c, name = inputs(kind, Cin, Cout, hw), case_name(kind, Cin, Cout, (MT, NT), pipe, hw)
            k, OH, OW = c["k"], c["OH"], c["OW"]
            with patched(ops, PIPE_CONV=pipe), patched(tiling, conv_tile=lambda *a, **kw: TILE + (MT, NT)), launches(ops) as rec:
                amax = slot()
                if kind in ("fwd3", "fwd1"):
                    y, st = ops.conv_fwd(G(c["x"]), ops.pack_conv_weight(c["w"].cuda()), Cout, k, 2, stats=True,
                                         out=filled(B, OH, OW, Cout), out_amax=amax)
                    out[name + " stats"] = st.cpu().numpy()
                else:
                    wpk_t = ops.pack_conv_weight(c["w"].cuda(), transpose=True)
                    dyg = G(c["dy"])
                    if kind == "dgrad3":
                        in_amax = ops.absmax_into(dyg, slot())
                        dyp = encode_pairs(R.nhwc(c["dy"]), sigma_of(in_amax)).cuda()
                        y = ops.conv_dgrad(dyp, wpk_t, Cin, 3, 2, hw, out=filled(B, H, Wd, Cin), in_amax=in_amax, in_presplit=True,
                                           out_amax=amax)
                    else:
                        y = ops.conv_dgrad(dyg, wpk_t, Cin, 1, 2, hw, out=G(c["prev"]), accumulate=True, out_amax=amax)
                torch.cuda.synchronize()
            out[name], out[name + " amax"] = y.cpu().numpy(), amax.cpu().numpy()
            inst[name] = [(lab, variant_of(lib, n, a)) for n, a, lab in rec if n == "spk_conv_mfma"]
            assert all(lab.startswith(kernel) for lab, _ in inst[name]) and len(inst[name]) == (4 if kind == "dgrad3" else 1), inst[name]
        for kind, Cin, Cout, wt, kernel, _ in wgrad_cases():
            c, name = inputs(kind, Cin, Cout, hw), case_name(kind, Cin, Cout, wt, True, hw)
            k, OH, OW = c["k"], c["OH"], c["OW"]
            for acc in (False, True):
                table = dict(tiling.FORCE_WGRAD_SPLIT)
                table[(OH, OW, Cin, Cout, k, 2)] = wt
                # three slabs (a slab is (Cin / 32) (Cout / 64) blocks): with four or ten regions a block walks more than one
                with patched(tiling, FORCE_WGRAD_SPLIT=table, WGRAD_TARGET_BLOCKS=3 * (Cin // 32) * (Cout // 64)), launches(ops) as rec:
                    dyg, kw = G(c["dy"]), {}
                    if kind == "wgrad3":
                        kw["dy_amax"] = ops.absmax_into(dyg, slot())
                        dyg = encode_pairs(R.nhwc(c["dy"]), sigma_of(kw["dy_amax"])).cuda()
                        kw["dy_presplit"] = True
                    dw = R.tensor(731, False, Cout, Cin, k, k).cuda() if acc else filled(Cout, Cin, k, k)
                    ops.conv_wgrad(G(c["x"]), dyg, dw, k, 2, accumulate=acc, **kw)
                    torch.cuda.synchronize()
                out[name + (" accumulate" if acc else "")] = dw.cpu().numpy()
            inst[name] = [(lab, variant_of(lib, n, a)) for n, a, lab in rec if n == "spk_conv_wgrad"]
            (args,) = [a for n, a, _ in rec if n == "spk_conv_wgrad"]
            assert inst[name][0][0].startswith(kernel) and (args["TH"], args["TW"], args["WN"]) == wt, (inst[name], wt)
            assert args["nsplit"] > 1, "more than one slab: the reduce sums"
    return out, inst


def reduce_inputs(ksize, Cin, Cout, nslab):
    g = torch.Generator().manual_seed(9000 + 7 * nslab + ksize * Cin * Cout)
    total = ksize * ksize * Cin * Cout
    # magnitudes spread over 2^-8 .. 2^8: the order of the additions shows in the low bits
    partial = torch.randn(nslab, total, generator=g) * torch.exp2(torch.randint(-8, 9, (nslab, total), generator=g).float())
    return partial, torch.randn(Cout, Cin, ksize, ksize, generator=g)


def reduce_emulation(partial, prev, ksize, Cin, Cout):
    """the four chains of wgrad_reduce_kernel in float32: s_j += slab[k] for k = j (mod 4) in ascending k, leftover slabs to s_0,
    (s0 + s1) + (s2 + s3), [tap][Cin][Cout] -> OIHW, dw_prev + s when accumulating"""
    p = partial.numpy()
    nslab, total = p.shape
    s = [np.zeros(total, np.float32) for _ in range(4)]
    k4 = nslab // 4 * 4
    for k in range(k4):
        s[k & 3] = s[k & 3] + p[k]
    for k in range(k4, nslab):
        s[0] = s[0] + p[k]
    r = ((s[0] + s[1]) + (s[2] + s[3])).reshape(ksize * ksize, Cin, Cout).transpose(2, 1, 0).reshape(Cout, Cin, ksize, ksize)
    assert r.dtype == np.float32
    return r if prev is None else prev.numpy() + r


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert os.environ.get("SPK_FL_VARIANTS", "1") != "0", "this process runs the variants; the child runs the generic instances"
    path = str(tmp_path_factory.mktemp("flag_variants") / "generic.npz")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, SPK_FL_VARIANTS="0"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert child.returncode == 0, "child with SPK_FL_VARIANTS=0: exit %d\n%s" % (child.returncode, child.stdout[-4000:])
    on = run_cases()
    d = np.load(path, allow_pickle=False)
    off = {k: d[k] for k in d.files if not k.startswith("instance:")}
    off_inst = {k[len("instance:"):]: [int(v) for v in d[k]] for k in d.files if k.startswith("instance:")}
    return on, (off, off_inst)


def all_cases():
    for hw in MAPS:
        for kind, Cin, Cout, tile, pipe, kernel, fl in conv_cases():
            yield case_name(kind, Cin, Cout, tile, pipe, hw), kind, Cin, Cout, tile, hw, fl
        for kind, Cin, Cout, wt, kernel, var in wgrad_cases():
            yield case_name(kind, Cin, Cout, wt, True, hw), kind, Cin, Cout, wt, hw, var


def test_every_case_takes_the_instance_meant(runs):
    (_, inst), (_, off_inst) = runs
    for name, kind, Cin, Cout, tile, hw, want in all_cases():
        assert [v for _, v in inst[name]] == [want] * len(inst[name]), (name, inst[name], want)
        assert off_inst[name] == [-1] * len(inst[name]), (name, off_inst[name])


def test_variants_equal_the_generic_instances_byte_for_byte(runs):
    (on, _), (off, _) = runs
    assert sorted(on) == sorted(off) and len(on) >= 2 * (len(conv_cases()) * 2 + len(wgrad_cases()) * 2)
    for name in sorted(on):
        a, b = on[name], off[name]
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s: %d of %d elements differ" % (
            name, int((a.view(np.int32) != b.view(np.int32)).sum()), a.size)


def test_variants_against_the_fp64_reference(runs):
    """the bounds of tests/test_conv_edges_gpu.py for the f16x3 mode (per element, derived in tests/conv_ref.py); the absmax slot
    holds exactly the largest stored magnitude"""
    (on, _), _ = runs
    for name, kind, Cin, Cout, tile, hw, _ in all_cases():
        c = inputs(kind, Cin, Cout, hw)
        k = c["k"]
        if kind in ("fwd3", "fwd1"):
            v, b = R.fwd(c["x"], c["w"], k, 2).finish(3)
            got = R.nchw(torch.from_numpy(on[name]))
            R.check("variant " + kind, got.double(), v, b)
            tot = torch.from_numpy(on[name + " stats"]).double().sum(0)
            s0, b0, s1, b1 = R.stats_ref(v, b, R.stats_chain(*tile))
            R.check("variant %s stats sum" % kind, tot[:, 0], s0, b0)
            R.check("variant %s stats sumsq" % kind, tot[:, 1], s1, b1)
        elif kind in ("dgrad3", "dgrad1"):
            v, b = R.dgrad(c["dy"], c["w"], k, 2, hw, 3, add=c["prev"] if kind == "dgrad1" else None)[:2]
            got = R.nchw(torch.from_numpy(on[name]))
            R.check("variant " + kind, got.double(), v, b)
        else:
            for acc in (False, True):
                prev = R.tensor(731, False, Cout, Cin, k, k) if acc else None
                v, b = R.wgrad(c["x"], c["dy"], k, 2, 3, prev=prev)[:2]
                R.check("variant " + kind, torch.from_numpy(on[name + (" accumulate" if acc else "")]).double(), v, b)
            continue
        stored = on[name][:, ::2, ::2] if kind == "dgrad1" else on[name]      # (a strided 1x1 stores the even pixels only)
        assert float(on[name + " amax"].view(np.float32)[0]) == float(np.abs(stored).max()), name


@pytest.mark.parametrize("ksize,Cin,Cout", REDUCE_SIZES)
def test_slab_reduce_equals_its_four_chains_in_float32(ksize, Cin, Cout):
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip
    got = []
    for nslab in NSLABS:
        partial, prev = reduce_inputs(ksize, Cin, Cout, nslab)
        pg = partial.cuda()
        for acc in (0, 1):
            dw = prev.cuda() if acc else filled(Cout, Cin, ksize, ksize)
            hip.call("spk_wgrad_reduce", hip.ptr(pg), hip.ptr(dw), nslab, ksize, Cin, Cout, acc, hip.stream())
            got.append((nslab, acc, dw))
    torch.cuda.synchronize()
    for nslab, acc, dw in got:
        partial, prev = reduce_inputs(ksize, Cin, Cout, nslab)
        want = reduce_emulation(partial, prev if acc else None, ksize, Cin, Cout)
        g = dw.cpu().numpy()
        assert g.tobytes() == want.tobytes(), "nslab %d accumulate %d: %d of %d weights differ" % (
            nslab, acc, int((g.view(np.int32) != want.view(np.int32)).sum()), g.size)


if __name__ == "__main__":
    arrays, instances = run_cases()
    arrays.update({"instance:" + k: np.array([v for _, v in vs], dtype=np.int64) for k, vs in instances.items()})
    np.savez(sys.argv[1], **arrays)
