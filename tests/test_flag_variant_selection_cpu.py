"""Which instance of its kernel every convolution launch of the training step runs, on a machine without a GPU: the launch record
(tests/golden/dispatch/*.json) carries the flag word and the NULL pattern of every launch, and the library answers through
spk_conv_variant_of / spk_wgrad_variant_of - the pure host functions its launchers call - with the compile-time flag variant
(csrc/conv_kernel.h FL, the weight gradients' VAR) or -1 for the generic instance that reads the word at run time.

    python tests/test_flag_variant_selection_cpu.py        # the child: exit 0 when every recorded launch maps to -1"""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from make_dispatch_golden import load  # noqa: E402  (reader of the record files; imports no library)

DISPATCH = os.path.join(ROOT, "tests", "golden", "dispatch")
HEADLINE = os.path.join(DISPATCH, "r34_t300_f16x3_b256.json")
PTRS = ("add_mask", "bn_mask", "in_mask", "in_act", "bn_act", "side_dz")        # SPK_PTR_* bits 0..5, by argument name
CONV_PIPE, CONV_M16, CONV_CK32, EPI_WMASK = 1024, 1 << 17, 1 << 23, 1 << 24
FL_ADDMASK, FL_BNMASK, FL_INMASK = 1 << 20, 1 << 21, 1 << 22

# kernels (ops label, register tile included) whose launches in the headline step must run a compile-time variant:
# the launches that ran generic before - the stride-2, 1x1 and first-block launches of the three downsample blocks ...
NEWLY_SPECIALISED = ["conv_mfma_kernel<2,1,false,3>", "conv_mfma_kernel<2,2,false,3>", "conv_mfma_kernel<3,2,false,3>",
                     "conv_mfma_kernel<1,4,false,3>", "conv_wgrad_split_kernel<9,2,2,3,5>", "conv_wgrad_split_kernel<1,2,2,3,4>"]
# ... and the ones that had their variants already
ALREADY_SPECIALISED = ["conv_mfma_kernel<1,2,false,3>", "conv_mfma_kernel<2,1,true,3>", "conv_pipe_kernel<3,2,false,false,true,true>"]
# Exceptions, by name and reason: launches of the headline step that map to -1
GENERIC_BY_DECISION = {
    # the pipelined forward sits at its 256-register bound: its variants spill - generic on purpose
    "conv_pipe_kernel<3,2,false,false,false,true>": "256-register bound: the variants spill",
    # the pipelined stride-2 forward of the last downsample block passed the register check (229 -> 218, no spill) and measured
    # 251.1 us against 251.4 us generic on the GPU: not faster, variant dropped
    "conv_pipe_kernel<1,4,false,false>": "measured on the GPU: not faster",
    # weight-gradient kernels outside conv_wgrad_split_kernel, which spk_wgrad_variant_of does not describe: the two 16x16x32
    # kernels have no generic instance at all (their VAR is always a template argument), the grouped 1x1 kernel selects its own
    "conv_wgrad_wm16_kernel": "no generic instance exists",
    "conv_wgrad_c32m16_kernel": "no generic instance exists",
    "conv_wgrad_1x1_kernel<2,2,4>": "another launcher family, unchanged",
    "conv_wgrad_1x1_kernel<2,2,2>": "another launcher family, unchanged",
}


def instances(lib, path):
    """-> [(label, flag word, pointer pattern, instance)] of every spk_conv_mfma* / spk_conv_wgrad launch of a record file (the
    streaming kernels have entries of their own and select their variants there)"""
    got = []
    for rec in load(path)["records"]:
        for ln in rec["launches"]:
            a = ln["args"]
            if ln["entry"] in ("spk_conv_mfma", "spk_conv_mfma_len"):
                ptrs = sum(1 << i for i, p in enumerate(PTRS) if a[p])
                got.append((ln["label"], a["flags"], ptrs, lib.spk_conv_variant_of(a["MT"], a["NT"], a["split"], a["flags"], ptrs)))
            elif ln["entry"] == "spk_conv_wgrad":
                got.append((ln["label"], a["flags"], 0,
                            lib.spk_wgrad_variant_of(a["ksize"], a["stride"], a["TH"], a["TW"], a["WN"], a["split"], a["flags"])))
    return got


def library():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip
    return hip.lib()


def test_every_launch_of_the_headline_step_runs_the_instance_meant():
    assert os.environ.get("SPK_FL_VARIANTS", "1") != "0"
    got = instances(library(), HEADLINE)
    seen = set()
    for label, flags, ptrs, v in got:
        seen.add(label)
        if label in GENERIC_BY_DECISION:
            assert v == -1, (label, hex(flags), v)
            continue
        assert label in NEWLY_SPECIALISED + ALREADY_SPECIALISED, "a kernel this test does not know: %s" % label
        assert v >= 0, "%s with flags 0x%x, pointers 0x%x runs the generic instance" % (label, flags, ptrs)
        if label.startswith("conv_wgrad"):
            assert v == (flags & 1) | (2 if flags & (1 << 16) else 0), (label, hex(flags), v)
        else:
            # the variant IS the launch's flag word (form bits dropped) with the mask pointers as SPK_FL_* bits
            word = flags & ~(CONV_PIPE | CONV_M16 | CONV_CK32)
            word |= (FL_ADDMASK if ptrs & 1 else 0) | (FL_BNMASK if ptrs & 2 else 0)
            word |= FL_INMASK if (ptrs & 4) and "true,3>" in label else 0
            assert v == word, (label, hex(flags), hex(ptrs), hex(v))
    assert seen == set(NEWLY_SPECIALISED + ALREADY_SPECIALISED) | set(GENERIC_BY_DECISION), sorted(seen)


def test_flag_words_no_variant_covers_stay_generic():
    lib = library()
    # the length-masked eval forward: eval-mode epilogues (EPI_AFFINE, EPI_RELU, EPI_ADD) and SPK_EPI_WMASK, whose own instance is
    # no variant (the launchers take it before they ask)
    got = instances(lib, os.path.join(DISPATCH, "r34_predict_len.json"))
    assert got and all(v == -1 for _, _, _, v in got), [g for g in got if g[3] != -1]
    assert any(flags & EPI_WMASK for _, flags, _, _ in got)
    STATS, ADD, PRE = 16, 4, 1 << 14
    assert lib.spk_conv_variant_of(2, 1, 3, STATS, 0) == STATS
    assert lib.spk_conv_variant_of(2, 1, 3, STATS | 8, 0) == -1            # with a ReLU epilogue
    assert lib.spk_conv_variant_of(2, 1, 3, STATS, 16) == -1               # an activation tensor given as the statistics' mask
    assert lib.spk_conv_variant_of(2, 1, 3, ADD, 1) == -1                  # a masked add on conv_mfma_kernel
    assert lib.spk_conv_variant_of(4, 1, 3, STATS, 0) == -1                # a register tile without variants
    assert lib.spk_conv_variant_of(2, 1, 6, STATS, 0) == -1 and lib.spk_conv_variant_of(2, 1, 0, STATS, 0) == -1      # other operand modes
    assert lib.spk_conv_variant_of(1, 2, 3, PRE, 0) == -1                  # the pair-input data gradient on (1, 2): ResNet-101 only
    assert lib.spk_conv_variant_of(1, 4, 3, STATS | CONV_PIPE, 0) == -1 and lib.spk_conv_variant_of(2, 2, 3, STATS | CONV_PIPE, 0) == -1
    # weight gradients: (ksize, stride, TH, TW, WN, split, flags); the small / large prefetch window decides with the tile
    assert lib.spk_wgrad_variant_of(3, 2, 4, 8, 2, 3, 1 << 16) == 2 and lib.spk_wgrad_variant_of(3, 2, 4, 6, 2, 3, 1 << 16) == -1
    assert lib.spk_wgrad_variant_of(3, 2, 4, 8, 2, 3, (1 << 16) | 1) == -1 and lib.spk_wgrad_variant_of(3, 2, 4, 8, 2, 6, 0) == -1
    assert lib.spk_wgrad_variant_of(1, 2, 1, 50, 2, 3, 0) == 0 and lib.spk_wgrad_variant_of(1, 2, 1, 50, 2, 3, 1 << 16) == -1


def test_resnet101_shares_most_of_the_variants():
    """ResNet-50 / 101 (Bottleneck blocks; r50_t300_f16x3 is the nearest record): the same stride-2 data gradients, shortcut
    accumulations and plain forwards; its fused-input forwards on (1, 4) / (3, 2), its weight gradients with a fused input
    BatchNorm and its (1, 2) pair-input data gradient have no variant and stay generic."""
    got = instances(library(), os.path.join(DISPATCH, "r50_t300_f16x3.json"))
    by = {}
    for label, flags, ptrs, v in got:
        by.setdefault((label, flags), set()).add(v)
    PRE, ADD, STATS = 1 << 14, 4, 16
    for label in ("conv_mfma_kernel<2,1,false,3>", "conv_mfma_kernel<2,2,false,3>", "conv_mfma_kernel<3,2,false,3>"):
        assert by[(label, PRE)] == {PRE} and by[(label, ADD)] == {ADD}, label
    assert by[("conv_mfma_kernel<3,2,false,3>", STATS)] == {STATS}
    assert by[("conv_wgrad_split_kernel<1,2,2,3,4>", 0)] == {0}
    assert by[("conv_mfma_kernel<1,4,false,3>", STATS | 1)] == {-1} and by[("conv_mfma_kernel<1,2,false,3>", PRE)] == {-1}
    assert by[("conv_wgrad_split_kernel<9,2,2,3,5>", (1 << 16) | 1)] == {-1}


def test_the_switch_makes_every_launch_generic():
    """SPK_FL_VARIANTS=0 is read once per process: a child process asks for every launch of every record"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, SPK_FL_VARIANTS="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "launches, all generic" in r.stdout


if __name__ == "__main__":
    lib = library()
    n = 0
    for path in sorted(glob.glob(os.path.join(DISPATCH, "*.json"))):
        for label, flags, ptrs, v in instances(lib, path):
            assert v == -1, (os.path.basename(path), label, hex(flags), hex(ptrs), v)
            n += 1
    assert n > 100
    print("%d launches, all generic" % n)
