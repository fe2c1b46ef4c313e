"""Thin Python wrappers over the libspkhip exports: shape checks, output allocation (torch caching
allocator owns every device buffer), tile selection, tap tables.  No arithmetic happens here."""
import collections
import ctypes
import os

import numpy as np
import torch

from . import hip, tiling
from .hip import (CONV_CK32, CONV_M16, CONV_PIPE, CONV_WS, DY_PRESPLIT, IN_PRESPLIT, SIDE_PRESPLIT, WGRAD_GROUPS, EPI_ADD, EPI_AFFINE, EPI_BNBWD, EPI_RELU,
                  EPI_STATS, EPI_WMASK, IN_AFFINE_RELU, IN_BNBWD, MASK_ACT, MASK_NONE, MASK_RAW,
                  call, ptr, stream)
from .recbatch import RecBatch

BN_EPS = 1e-5
BN_MOMENTUM = 0.1

# When set to a list, every launch appends (label, algorithmic flops, start event, end event); the events are
# recorded on the launch stream (torch's current stream), which is what bench.py's roofline pass reads.
PROFILE = None
_raw_call = call


def call(name, *args, label=None, flops=0.0, nbytes=0.0):   # noqa: F811  (instrumented wrapper around hip.call)
    """nbytes: ALGORITHMIC bytes of the launch (every tensor it must read or write, once; no halo or re-read factors)"""
    if PROFILE is None:
        return _raw_call(name, *args)
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    _raw_call(name, *args)
    e1.record()
    PROFILE.append((label or name, flops, e0, e1, nbytes))


def _iarr(v):
    return (ctypes.c_int * len(v))(*v)


class AmaxPool:
    """Slots for the absmax hand-offs of the f16x3 operand mode: one int32 (float bits, atomicMax'ed by the producing
    kernel) per gradient tensor of a step, taken in a fixed order so that a captured hipGraph sees the same addresses on
    every replay; zeroed once at the start of the step."""

    def __init__(self, device, n=4096):
        self.table = torch.zeros(n, device=device, dtype=torch.int32)
        self.next = 0

    def take_n(self, n):
        """n consecutive slots (a per-channel absmax row, spk_bn_bwd_reduce chan_amax)"""
        i = self.next
        assert i + n <= self.table.numel(), "AmaxPool exhausted"
        self.next = i + n
        return self.table[i:i + n]

    def reset(self):
        self.table.zero_()
        self.next = 0

    def take(self):
        i = self.next
        assert i < self.table.numel(), "AmaxPool exhausted"
        self.next = i + 1
        return self.table[i:i + 1]


def absmax_into(t, slot):
    """slot = max(slot, float bits of max|t|)  (spk_absmax: one pass over the tensor)"""
    call("spk_absmax", ptr(t), ptr(slot), t.numel(), stream())
    return slot


def affine_estimate(scale, shift, amax_in, est):
    """est = float bits of max_c|scale_c| * absmax + max_c|shift_c|: the bound of the values a convolution / weight gradient
    with the fused input BatchNorm+ReLU stages, given the slot with the absmax of the raw tensor"""
    call("spk_affine_estimate", ptr(scale), ptr(shift), scale.numel(), ptr(amax_in), ptr(est), stream())
    return est


def _amax_fwd_fallback(x, in_affine):
    """Operand-scale input of a forward convolution / weight-gradient X operand called without one (tests, tools)."""
    slot = absmax_into(x, torch.zeros(1, device=x.device, dtype=torch.int32))
    if in_affine is None:
        return slot
    return affine_estimate(in_affine[0], in_affine[1], slot, torch.zeros(1, device=x.device, dtype=torch.int32))


def bnbwd_estimate(coef, bn4, amax_in, raw_amax, est=None):
    """est = float bits of the rigorous bound of the BatchNorm-backward values k1 (dz - m1 - xhat m2) (spk_bnbwd_estimate):
    coef [3][C] rows of bn_bwd_coef, bn4 = [mean, invstd, ...] rows, amax_in / raw_amax = slots with absmax(incoming gradient)
    / absmax(raw tensor).  The value bn_bwd_coef(est_out=) produces without this launch."""
    if est is None:
        est = torch.zeros(1, device=coef.device, dtype=torch.int32)
    call("spk_bnbwd_estimate", ptr(coef), ptr(bn4[0]), ptr(bn4[1]), coef.shape[1], ptr(amax_in), ptr(raw_amax), ptr(est), stream())
    return est


def _amax_fallback(dy, in_bnbwd):
    """Operand-scale input of a data gradient called without one (tests, tools): absmax(dy), or for the fused
    BatchNorm-backward form the same bound bn_bwd_coef(est_out=) gives, from absmax(dy), absmax(raw) and the coefficient rows."""
    slot = torch.zeros(1, device=dy.device, dtype=torch.int32)
    absmax_into(dy, slot)
    if in_bnbwd is None:
        return slot
    raw_slot = absmax_into(in_bnbwd[0], torch.zeros(1, device=dy.device, dtype=torch.int32))
    return bnbwd_estimate(in_bnbwd[3], in_bnbwd[2], slot, raw_slot)


def f16_window_count(x, slot, counts, affine=None, pairs=False):
    """counts [4] int64 += (values, saturating, low term lost, high term subnormal) of x - or of relu(x*scale+shift) when
    affine = (scale, shift); pairs: x is an f16 pair tensor - under the operand scale of `slot` (spk_f16_window_count)."""
    C = x.shape[-1]
    call("spk_f16_window_count", ptr(x), ptr(affine[0]) if affine else None, ptr(affine[1]) if affine else None, x.numel(), C,
         ptr(slot), 1 if pairs else 0, ptr(counts), stream())
    return counts


def conv_out_hw(h, w, ksize, stride):
    pad = 1 if ksize == 3 else 0
    return (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1


# Matrix-core operand mode of the 3x3 convolutions (forward, data gradient, weight gradient).  Inputs, outputs, accumulation
# and the measured accuracy are fp32 in every mode (same test tolerances; tools/probe/split_probe.hip):
#   f32     fp32 operands on v_mfma_f32_32x32x2_f32 (157 TFLOP/s peak)
#   bf16x6  every fp32 operand split exactly into three bf16 terms, the 6 cross terms of weight >= 2^-16 on
#   bf16x9    v_mfma_f32_32x32x16_bf16 (bf16x9: all nine) - 16/6 of the fp32 matrix rate
#   f16x3   (default) operand value x 2^k as two fp16 terms (2 x 11 significand bits; k from the tensor's absmax, handed from
#           the kernel that writes a tensor to the kernels that read it), the three cross terms h1g1 + h1g2 + h2g1 on
#           v_mfma_f32_32x32x16_f16, accumulators scaled back by 2^-(ka+kb) - half the matrix instructions of bf16x6; the
#           step is power-limited on MI355X, so this is where the time goes (78 -> 59 ms per step)
# csrc/conv_kernel.h, csrc/conv_wgrad_split.hip, csrc/spk_common.h.  Packed weights carry the mode: set it before the first
# forward of a model (or mark its engine dirty).
MFMA_MODES = {"f32": 0, "bf16x6": 6, "bf16x9": 9, "f16x3": 3}
SPLIT = MFMA_MODES[os.environ.get("SPK_MFMA", "f16x3")]
# optional override for the backward kernels (data / weight gradients): None = same mode as the forward
SPLIT_BWD = MFMA_MODES[os.environ["SPK_MFMA_BWD"]] if os.environ.get("SPK_MFMA_BWD") else None


# wave-specialised (producer / consumer, persistent) convolution kernel, csrc/conv_ws_kernel.h.  SPK_CONV_WS = "0" never,
# "1" every eligible 3x3 launch, "auto" (default) only where it wins INSIDE the training step on MI355X (per-layer
# in-step times, profiles/r02_ws_instep.log): the data-gradient launches with the fused BN backward on >= 128 output
# channels in the f16x3 mode (0.576 -> 0.552 ms and 0.466 -> 0.413 ms per launch; those kernels keep the matrix pipe only
# ~25 % busy, so hiding the staging behind it pays).  Everywhere else conv_mfma_kernel is as fast or faster in-step
# (the 32/64-channel layers lose 10-20 % to the wave-specialised layout), and in the bf16x6 mode the step is power-limited
# and the two kernels tie.
WS_CONV = os.environ.get("SPK_CONV_WS", "auto")
assert WS_CONV in ("0", "1", "auto"), "SPK_CONV_WS must be 0, 1 or auto"
WS_AUTO_MIN_COUT = 128
# in-wave pipelined staging (conv_pipe_kernel): on by default for the f16x3 3x3 launches it covers; SPK_CONV_PIPE=0 disables
PIPE_CONV = os.environ.get("SPK_CONV_PIPE", "1") == "1"
# its v_mfma_f32_16x16x32_f16 form (two taps per K step; the chip holds a higher clock on that instruction shape)
PIPE_M16 = os.environ.get("SPK_PIPE_M16", "1") == "1"
# the same for the 3x3 weight gradients (conv_wgrad_pipe_kernel): opt-in.  Bit-identical, but no faster than
# conv_wgrad_split_kernel (+2..6 % on the 32/64-channel layers, -1..-12 % elsewhere, profiles/r02_wgrad_ablation.log): a tap of
# the weight gradient has three matrix instructions against ~60 VALU instructions of a staging item, so the VALU stream sets the
# pace with or without the overlap
PIPE_WGRAD = os.environ.get("SPK_WGRAD_PIPE", "0") == "1"
# ... and for the data gradients with the fused BatchNorm backward (sign-bit masks, register tiles <= 2 x 2): opt-in.  A fused
# item is ~90 VALU instructions (~450 cycles) against the 384 MFMA cycles of a 2 x 2 tap, so the staging is not hidden: per launch
# 0.75 vs 0.81 ms (64 channels) and 0.50 vs 0.54 ms (128 channels, against the wave-specialised kernel), nothing measurable per step
PIPE_BNBWD = os.environ.get("SPK_PIPE_BNBWD", "0") == "1"
GROUPED_1X1 = os.environ.get("SPK_WGRAD_1X1_GROUPS", "1") == "1"   # 1x1 weight gradients: input-channel groups as "taps"
WM16 = os.environ.get("SPK_WM16", "1") == "1"             # 3x3 grouped weight gradient with a pair-tensor dy: 16x16x32 form, dy by LDS DMA (csrc/conv_wgrad_wm16.hip)
C32M16 = os.environ.get("SPK_C32M16", "1") == "1"         # ... and its 32-channel-group layout for the first layer's weight gradients
WM_SHIFT = os.environ.get("SPK_WM_SHIFT", "1") == "1"      # 3x3 grouped weight gradient: shifted-window K loop where it applies (csrc/conv_wgrad_wm.hip, SH)
GROUPED_3X3 = os.environ.get("SPK_WGRAD_3X3_GROUPS", "1") == "1"   # 3x3 weight gradients: 2 x 2 (cin group x cout group) wave layout
GROUPED_1X1_BLOCKS = int(os.environ.get("SPK_WGRAD_1X1_BLOCKS", "512"))
# fused BatchNorm-backward data gradient at Cin = 32 (f16x3, conv_mfma_kernel): channels per staged plane.  32 = whole 128-byte
# pixels per staging pass, one chunk (csrc/conv_kernel.h, CKP); 16 = two 16-channel planes staged one after the other.  Same
# sums in the same order: bit-identical results at an equal tile (tests/test_c32_whole_pixel_gpu.py).
C32_PLANE = int(os.environ.get("SPK_C32_PLANE", "32"))
assert C32_PLANE in (16, 32), "SPK_C32_PLANE: 16 or 32"
C32_PLANE_TILES = ((2, 1), (1, 1))        # register tiles csrc/conv_split.hip instantiates with 32-channel planes
PIPE_MIN_CIN = int(os.environ.get("SPK_PIPE_MIN_CIN", "64"))    # 32 channels = two chunks: nothing to pipeline, and the second tile costs occupancy
PIPE_MAX_LDS = int(os.environ.get("SPK_PIPE_MAX_LDS", str(80 * 1024)))      # two halo tiles; <= 80 KiB keeps two blocks per CU
PIPE_TILES = ((2, 1), (3, 1), (1, 2), (2, 2), (3, 2), (1, 4))      # (MT, NT) register tiles of conv_pipe_kernel (csrc/conv_pipe.hip)
# the same idea for the 3x3 weight gradients (f16x3 mode): eight-wave blocks, one per CU (conv_wgrad_ws_kernel).  Opt-in:
# bit-identical, but 10-15 % SLOWER than conv_wgrad_split_kernel on every layer (tools/wg_abl3.sh, profiles/r02_wgrad_ablation.log:
# producers alone 0.31 ms, consumers alone 0.28 ms, together 0.49 ms - the staging is VALU-bound and a SIMD does not run one
# wave's VALU stream under another wave's MFMAs to any useful degree; two resident four-wave blocks interleave better).
WS_WGRAD = os.environ.get("SPK_WGRAD_WS", "0") == "1"
WS_WGRAD_BLOCKS = int(os.environ.get("SPK_WGRAD_WS_BLOCKS", "256"))
WS_MIN_TAPS = int(os.environ.get("SPK_WS_MIN_TAPS", "9"))
LABEL_SHAPES = os.environ.get("SPK_LABEL_SHAPES", "0") == "1"      # diagnostic: per-layer lines in bench.py's all_kernels
WS_FORCE = None        # tests / sweeps: (TH, TW, MT, NT, WC) applied to every eligible launch


def _experimental():
    """the kernel forms behind SPK_CONV_WS / SPK_PIPE_BNBWD / SPK_WGRAD_PIPE / SPK_WGRAD_WS exist only in a library built with
    SPK_EXPERIMENTAL=1 (python pytorch-kaldi-resnet_amd/build.py --experimental)"""
    return hip.has_experimental()


SPLIT_1X1 = os.environ.get("SPK_SPLIT_1X1", "1") == "1"
# channel planes a single-tap (1x1) convolution stages per barrier: the first candidate that divides the channels and fits LDS
KC_CANDIDATES = tuple(int(v) for v in os.environ.get("SPK_KC", "4,2").split(","))


def split_for(ksize, bwd=False):
    """operand mode of a convolution launch.  The bf16-term modes cover the 3x3 convolutions only (1x1 convolutions stay on
    fp32 operands there); f16x3 also runs the 1x1 convolutions (Bottleneck blocks, downsample branches).  The stem (Cin = 1)
    is a direct convolution in every mode."""
    mode = SPLIT_BWD if (bwd and SPLIT_BWD is not None) else SPLIT
    if ksize == 3:
        return mode
    return 3 if (mode == 3 and SPLIT_1X1 and ksize == 1) else 0


def pack_conv_weight(w, transpose=False, out=None):
    """OIHW nn.Conv2d weight -> MFMA fragment order (see csrc/conv_mfma.hip, csrc/conv_split.hip)."""
    Cout, Cin, KH, KW = w.shape
    split = split_for(KH, bwd=transpose)     # the transposed pack feeds the data gradient
    n = packed_numel(w, bwd=transpose)
    if out is None or out.numel() != n:
        out = torch.empty(n, device=w.device, dtype=torch.float32)
    if split:
        call("spk_pack_conv_weight_split", ptr(w), ptr(out), Cout, Cin, KH, KW, 1 if transpose else 0, split, stream(),
             label="spk_pack_conv_weight")
    else:
        call("spk_pack_conv_weight", ptr(w), ptr(out), Cout, Cin, KH, KW, 1 if transpose else 0, stream(),
             label="spk_pack_conv_weight")
    return out


def packed_numel(w, bwd=False):
    """floats of the packed form of an OIHW weight in the current operand mode (three bf16 terms = 6 bytes per weight;
    fp32 = 4 bytes; two fp16 terms = 4 bytes + a 16-byte header with the tensor's absmax)."""
    sp = split_for(w.shape[2], bwd)
    return w.numel() * 3 // 2 if sp in (6, 9) else (w.numel() + 4 if sp == 3 else w.numel())


class PackTable:
    """Device-resident job table for spk_pack_conv_weights_batched: (weight, packed buffer, transpose) triples of every
    convolution, packed by ONE launch per step.  Rebuilt by the engine whenever a buffer or the operand mode changes."""

    def __init__(self, jobs, device):
        import struct
        assert hip.lib().spk_pack_job_bytes() == 48
        blob, block0 = b"", 0
        self.key = []
        for w, wpk, transpose in jobs:
            Cout, Cin, KH, KW = w.shape
            split = split_for(KH, bwd=transpose)
            assert wpk.numel() == packed_numel(w, bwd=transpose) and w.is_contiguous()
            blob += struct.pack("<QQ8i", w.data_ptr(), wpk.data_ptr(), Cout, Cin, KH * KW, 1 if transpose else 0, split,
                                w.numel(), block0, 0)
            block0 += (w.numel() + 255) // 256
            self.key.append((w.data_ptr(), wpk.data_ptr(), transpose, split))
        self.njobs, self.blocks = len(jobs), block0
        self.has_f16 = any(k[3] == 3 for k in self.key)
        self.table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(device)
        self.launches = 0               # eager launches + launches recorded into a hipGraph
        self.launches_captured = 0

    def run(self):
        self.launches += 1
        if torch.cuda.is_current_stream_capturing():
            self.launches_captured += 1
        call("spk_pack_conv_weights_batched", ptr(self.table), self.njobs, self.blocks, 1 if self.has_f16 else 0, stream(),
             label="spk_pack_conv_weight")


STREAM_1X1 = os.environ.get("SPK_STREAM_1X1", "1") == "1"
STREAM_1X1_BLOCKS = int(os.environ.get("SPK_STREAM_1X1_BLOCKS", "512"))       # persistent blocks: two per CU
STREAM_C32 = os.environ.get("SPK_STREAM_C32", "1") == "1"
STREAM_C32_BLOCKS = int(os.environ.get("SPK_STREAM_C32_BLOCKS", "512"))
FWD_TAPS = tuple((kh - 1, kw - 1, kh * 3 + kw) for kh in range(3) for kw in range(3))

# What a forward / data-gradient launch needs that is not a pointer (_plan_conv).  stats_rows: partial-statistics rows where
# flags carry EPI_STATS (None for spk_conv1x1_stream: spk_conv1x1_stream_rows says); key: the tile-table key, and the tile,
# register tile, wave layout, kc, ips and effective IS of spk_conv_mfma / spk_conv_mfma_len (the streaming entries have none).
ConvPlan = collections.namedtuple("ConvPlan", "entry flags label nblocks stats_rows key TH TW MT NT WC kc ips IS",
                                  defaults=(None,) * 9 + (1, 1))
# ... and a weight-gradient launch (_plan_wgrad).  family: wm16 | c32m16 | wm | 1x1 | ws | pipe | split | f32
WgradPlan = collections.namedtuple("WgradPlan", "TH TW WN family cg nsplit flags label")


def _mask_form(t, n):
    """how a BatchNorm-backward operand tuple (bn_bwd: n = 3, in_bnbwd: n = 4) carries its ReLU mask: None | "sign" (one more
    element: sign-bit words) | "raw" (no activation: recomputed from the raw tensor) | "act" (an activation tensor)"""
    return None if t is None else "sign" if len(t) > n else "raw" if t[1] is None else "act"


def _plan_conv(B, IH, IW, Cin, OH, OW, OHf, OWf, Cout, taps, IS, OS, ooy, oox, split, experimental, in_affine=False,
               epi_affine=False, epi_add=False, relu=False, want_stats=False, bn_bwd=None, in_bnbwd=None, side=False,
               add_mask=False, in_presplit=False, side_presplit=False, wlen=False, out_is_x=False):
    """Which kernel form a forward / data-gradient launch takes, on which tile, under which label: integers, booleans (is the
    optional operand there) and the module switches in, a ConvPlan out - no tensor, no device, no library call.  bn_bwd /
    in_bnbwd: _mask_form.  experimental: the library has the opt-in kernel forms (_experimental())."""
    ntaps = len(taps)
    dys, dxs = [t[0] for t in taps], [t[1] for t in taps]
    want_stats = want_stats or bn_bwd is not None
    flags = ((IN_AFFINE_RELU if in_affine else 0) | (IN_PRESPLIT if in_presplit else 0) | (SIDE_PRESPLIT if side_presplit else 0)
             | (EPI_AFFINE if epi_affine else 0) | (EPI_ADD if epi_add else 0) | (EPI_RELU if relu else 0)
             | (IN_BNBWD if in_bnbwd is not None else 0) | (EPI_BNBWD if bn_bwd is not None else 0) | (EPI_WMASK if wlen else 0)
             | (EPI_STATS if want_stats else 0))
    shape = " C%d %dx%d" % (Cout, OH, OW) if LABEL_SHAPES else ""
    # what both streaming kernels ask: f16x3, the same map in and out at stride 1, training-mode epilogues, no length mask
    same_map = (not wlen and split == 3 and IS == 1 and OS == 1 and ooy == 0 and oox == 0 and (IH, IW) == (OH, OW) == (OHf, OWf)
                and in_bnbwd is None and not side and not epi_affine and not relu and not side_presplit)
    # Streaming 3x3 forward kernel of the 32-channel layer (csrc/conv3x3_c32_stream.hip): 32 -> 32 channels, the forward tap
    # order, raw output + statistics, plain or fused-BatchNorm input.  (A data gradient has mirrored taps: general kernel.)
    stream_c32 = (STREAM_C32 and same_map and Cin == 32 and Cout == 32 and want_stats and bn_bwd is None and not epi_add
                  and not in_presplit and not add_mask and tuple(taps) == FWD_TAPS and B * OH * OW * 32 < 2 ** 31 - 65536)
    if stream_c32:
        nblocks = max(1, min(STREAM_C32_BLOCKS, B * (-(-IH // 8)) * (-(-IW // 16))))
        return ConvPlan("spk_conv3x3_c32_stream", flags, "conv3x3_c32_stream_kernel" + shape, nblocks, 4 * nblocks)
    # Streaming 1x1 kernel (csrc/conv1x1_stream.hip): C -> C channels (raw output + statistics; data gradients: shortcut add with
    # or without its sign mask, BatchNorm-backward statistics with the mask as sign bits or recomputed from the raw tensor).
    # Everything else - eval-mode epilogues, strided 1x1, other widths, the fused input BatchNorm backward, an activation tensor
    # as the mask, an output that aliases the input - stays on the general kernel.
    stream_1x1 = (STREAM_1X1 and same_map and ntaps == 1 and dys[0] == 0 and dxs[0] == 0 and Cin == Cout and Cin in (32, 64, 128)
                  and not out_is_x and bn_bwd != "act" and B * OH * OW * Cin < 2 ** 31)
    if stream_1x1:
        tp = 64 * (1 if Cin >= 128 else (2 if Cin == 64 else 4))
        nblocks = max(1, min(STREAM_1X1_BLOCKS, -(-(B * IH * IW) // tp)))
        return ConvPlan("spk_conv1x1_stream", flags, "conv1x1_stream_kernel<%d>" % Cin + shape, nblocks)
    ips = 1
    if ntaps == 1 and IS > 1 and dys[0] == 0 and dxs[0] == 0:
        ips, IS = IS, 1          # strided 1x1: address the input through a strided view, stage only the pixels used
    key = (OH, OW, IS, max(dys) - min(dys) + 1, max(dxs) - min(dxs) + 1, ntaps, Cout)
    # (mode 2: the fused data gradient that may stage whole pixels - its own table key, 144 B per halo pixel)
    c32 = C32_PLANE == 32 and split == 3 and Cin == 32 and in_bnbwd is not None and ntaps == 9
    TH, TW, MT, NT = tiling.conv_tile(*key, mode=(2 if c32 else 1) if in_bnbwd is not None else 0, split=split)
    # fused BatchNorm backward with the mask as sign bits on <= 128 output channels: optionally the in-wave pipelined kernel
    pipe_fused = (PIPE_CONV and PIPE_BNBWD and split == 3 and in_bnbwd == "sign" and MT * NT <= 4 and Cout <= 128
                  and WS_FORCE is None and WS_CONV != "1" and not side_presplit)
    # Producer / consumer (wave-specialised, persistent) kernel for the bf16-split 3x3 launches (csrc/conv_ws_kernel.h) with
    # its own wave layouts and tiles; f16 pair tensors and everything else stay on conv_mfma_kernel / conv_pipe_kernel.
    ws_on = (WS_CONV == "1" or WS_FORCE is not None or (
        WS_CONV == "auto" and experimental and split == 3 and in_bnbwd is not None and Cout >= WS_AUTO_MIN_COUT and not pipe_fused))
    ws, WC = None, 1
    if split and ws_on and not side_presplit and not in_presplit and ntaps >= WS_MIN_TAPS and ips == 1:
        ws = WS_FORCE or tiling.ws_tile(*key)
    if ws is not None:
        TH, TW, MT, NT, WC = ws
        flags |= CONV_WS | ({1: 0, 2: 1, 4: 2}[WC] << 8)
    # single-tap (1x1) convolutions stage several 32-channel planes per barrier: their K loop per plane is only 4 MFMA groups
    kc = 1
    if ntaps == 1:
        halo = ((TH - 1) * IS + 1) * ((TW - 1) * IS + 1)
        kc = next((c for c in KC_CANDIDATES if Cin % (32 * c) == 0 and c * halo * tiling.LDS_PIX_BYTES <= tiling.LDS_HARD), 1)
    # in-wave pipelined kernel (csrc/conv_kernel.h, PIPE): f16x3 3x3 launches whose two halo tiles fit, with a plain input (or the
    # fused BatchNorm backward above: the ReLU mask as sign bits - not read from an activation), on a register tile
    # csrc/conv_pipe.hip instantiates; any other tile stays on conv_mfma_kernel (same LDS tile, same sums)
    halo9 = ((TH - 1) * IS + key[3]) * ((TW - 1) * IS + key[4])
    pipe = (PIPE_CONV and ws is None and split == 3 and ntaps == 9 and kc == 1 and (in_bnbwd is None or pipe_fused) and halo9 <= 576
            and (2 * halo9 + 1) * 80 <= PIPE_MAX_LDS and Cin >= PIPE_MIN_CIN and (MT, NT) in PIPE_TILES)
    # its 16x16x32 form (conv_kernel.h, M16): the (3, 2) register tile, at most eight staging items per plane
    m16 = pipe and PIPE_M16 and in_bnbwd is None and (MT, NT) == (3, 2) and halo9 <= 512 and IS == 1
    # whole-pixel staging of the 32-channel fused data gradient: on the register tiles compiled for it, on conv_mfma_kernel
    c32 = c32 and ws is None and not pipe and kc == 1 and (MT, NT) in C32_PLANE_TILES
    flags |= (CONV_PIPE if pipe else 0) | (CONV_M16 if m16 else 0) | (CONV_CK32 if c32 else 0)
    fused = "true" if in_bnbwd is not None else "false"
    if ws is not None:
        label = "conv_ws_kernel<%d,%d,%d,%s,%d>" % (MT, NT, WC, fused, split)
    elif pipe and in_bnbwd is not None:
        label = "conv_pipe_kernel<%d,%d,true,true>" % (MT, NT)
    elif pipe:
        pair = ",true" if in_presplit else (",false" if m16 else "")
        label = "conv_pipe_kernel<%d,%d,false,false%s%s>" % (MT, NT, pair, ",true" if m16 else "")
    else:
        label = "conv_mfma_kernel<%d,%d,%s,%d>" % (MT, NT, fused, split)
    if LABEL_SHAPES and c32:
        shape += " plane32"
    rows = (4 // WC) * B * (-(-OH // TH)) * (-(-OW // TW))      # one partial row per wave (per pixel group of waves)
    return ConvPlan("spk_conv_mfma_len" if wlen else "spk_conv_mfma", flags, label + shape, None, rows, key,
                    TH, TW, MT, NT, WC, kc, ips, IS)


def _conv_launch(x, wpk, out, Cout, taps, IS, OS, ooy, oox, OH, OW, in_affine, epi_affine, epi_add, relu, want_stats,
                 bn_bwd=None, in_bnbwd=None, side=None, split=0, add_mask=None, in_amax=None, out_amax=None, side_amax=None,
                 in_presplit=False, side_presplit=False, wlen=None):
    B, IH, IW, Cin = x.shape
    OHf, OWf = out.shape[1], out.shape[2]
    pa = (B, IH, IW, Cin, OH, OW, OHf, OWf, Cout, taps, IS, OS, ooy, oox, split, _experimental(), in_affine is not None,
          epi_affine is not None, epi_add is not None, relu, want_stats, _mask_form(bn_bwd, 3), _mask_form(in_bnbwd, 4),
          side is not None, add_mask is not None, in_presplit, side_presplit, wlen is not None, out is x)
    if tiling.AUTOTUNE and PROFILE is None and not torch.cuda.is_current_stream_capturing():
        p = _plan_conv(*pa)      # before the plan that counts: the autotuner fills tiling.FORCE_* (streaming forms have no key)
        if p.key is not None and p.key not in (tiling.FORCE_CONV_SPLIT if split else tiling.FORCE_CONV):
            _autotune_conv(p.key, x, wpk, out, Cout, taps, p.IS, OS, ooy, oox, OH, OW, in_affine, epi_affine, epi_add, relu, split,
                           in_amax=in_amax, in_presplit=in_presplit)
    p = _plan_conv(*pa)
    if wlen is not None:
        _check_wlen(wlen, B)
    assert not in_presplit or (split == 3 and in_affine is None and in_bnbwd is None), "f16 pair input: f16x3 mode, plain input"
    assert not side_presplit or (split == 3 and in_bnbwd is not None), "f16 pair side output: fused BatchNorm-backward data gradient in the f16x3 mode"
    assert epi_add is None or epi_add.shape == out.shape
    # sign masks (uint32 words, 32 channels each, written by bn_apply(mask=True)) replace the activated tensors where given
    in_mask = in_bnbwd[4] if (in_bnbwd is not None and len(in_bnbwd) > 4) else None
    bn_mask = bn_bwd[3] if (bn_bwd is not None and len(bn_bwd) > 3) else None
    for mk, ref in ((in_mask, x), (bn_mask, out), (add_mask, out)):
        if mk is not None:
            assert mk.dtype == torch.int32 and mk.numel() == ref.numel() // 32, "sign mask shape"
    if in_bnbwd is not None:
        assert in_affine is None and side is not None and side[0].shape == x.shape
        assert in_bnbwd[0].shape == x.shape and (in_bnbwd[1] is None or in_bnbwd[1].shape == x.shape)
    if bn_bwd is not None:
        assert bn_bwd[0].shape == out.shape and (bn_bwd[1] is None or bn_bwd[1].shape == out.shape)
    stats = None
    if p.flags & EPI_STATS:
        rows = p.stats_rows if p.stats_rows is not None else hip.lib().spk_conv1x1_stream_rows(p.nblocks, Cin)
        stats = torch.empty(rows, Cout, 2, device=x.device, dtype=torch.float32)
    in_aff = (ptr(in_affine[0]), ptr(in_affine[1])) if in_affine else (None, None)
    bn_raw, bn4 = (ptr(bn_bwd[0]), ptr(bn_bwd[2])) if bn_bwd else (None, None)
    if p.entry == "spk_conv3x3_c32_stream":
        args = (*in_aff, ptr(stats), B, IH, IW, p.flags, ptr(in_amax), ptr(out_amax), p.nblocks)
    elif p.entry == "spk_conv1x1_stream":
        args = (*in_aff, ptr(epi_add), ptr(add_mask), bn_raw, ptr(bn_mask), bn4, ptr(stats), B * IH * IW, Cin, p.flags,
                ptr(in_amax), ptr(out_amax), p.nblocks)
    else:
        args = (*in_aff, ptr(epi_affine[0]) if epi_affine else None, ptr(epi_affine[1]) if epi_affine else None, ptr(epi_add),
                ptr(in_bnbwd[0]) if in_bnbwd else None, ptr(in_bnbwd[1]) if (in_bnbwd and in_mask is None) else None,
                ptr(in_bnbwd[2]) if in_bnbwd else None, ptr(in_bnbwd[3]) if in_bnbwd else None,
                ptr(in_mask), ptr(bn_mask), ptr(add_mask), ptr(side[0]) if side else None, ptr(side[1]) if side else None,
                bn_raw, ptr(bn_bwd[1]) if (bn_bwd and bn_mask is None) else None, bn4, ptr(stats),
                B, IH, IW, Cin, OH, OW, OHf, OWf, Cout, p.IS, OS, ooy, oox, len(taps),
                _iarr([t[0] for t in taps]), _iarr([t[1] for t in taps]), _iarr([t[2] for t in taps]),
                p.TH, p.TW, p.MT, p.NT, p.kc, p.ips, p.flags, split, ptr(in_amax), ptr(out_amax), ptr(side_amax),
                *(() if wlen is None else (ptr(wlen),)))
    ips, eff_is = p.ips, p.IS      # (a strided 1x1 reads every ips-th pixel at an effective stride of 1)
    call(p.entry, ptr(x), ptr(wpk), ptr(out), *args, stream(), label=p.label,
         flops=2.0 * B * OH * OW * Cout * Cin * len(taps),
         # algorithmic bytes: the input pixels this launch reads (all of them for a stride-1 / full-tap launch), the output it
         # writes, and every fused side stream once: shortcut add, raw + side draw of the fused BatchNorm backward, raw of the
         # BatchNorm whose backward statistics are reduced, the 1-bit masks; packed weights
         nbytes=4.0 * (B * (IH // ips) * (IW // ips) * Cin * (min(1.0, len(taps) * OH * OW / max(1, (IH // ips) * (IW // ips))) if eff_is == 1 and OS > 1 else 1.0)
                       + B * OH * OW * Cout * (1 + (1 if epi_add is not None else 0) + (1 if bn_bwd is not None else 0))
                       + (2 * x.numel() if in_bnbwd is not None else 0)
                       + (x.numel() / 32 if in_mask is not None else 0) + (B * OH * OW * Cout / 32) * ((bn_mask is not None) + (add_mask is not None))
                       + wpk.numel()))
    return stats


def _check_wlen(wlen, B):
    """per-image valid widths of a length-masked launch: a device int32 vector [B]"""
    if not (wlen.is_cuda and wlen.dtype == torch.int32 and wlen.dim() == 1 and wlen.numel() == B and wlen.is_contiguous()):
        raise RuntimeError("wlen must be a contiguous int32 device tensor [%d], got %s %s %s" % (B, wlen.dtype, tuple(wlen.shape), wlen.device))


def _time_launch(fn, reps=2):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _autotune_conv(key, x, wpk, out, Cout, taps, IS, OS, ooy, oox, OH, OW, in_affine, epi_affine, epi_add, relu, split=0,
                   in_amax=None, in_presplit=False):
    """Time candidate tiles on the real operands (scratch output) and pin the fastest for this launch shape.  The operand-scale
    slot is the caller's (or computed ONCE here): no absmax pass or allocation inside a timed candidate."""
    scratch = torch.empty_like(out)
    if split == 3 and in_amax is None:
        in_amax = _amax_fwd_fallback(x, in_affine)
    add = epi_add if (epi_add is None or epi_add.data_ptr() != out.data_ptr()) else scratch
    best = None
    table = tiling.FORCE_CONV_SPLIT if split else tiling.FORCE_CONV
    for cand in tiling.conv_candidates(*key, split=split):
        table[key] = cand
        try:
            ms = _time_launch(lambda: _conv_launch(x, wpk, scratch, Cout, taps, IS, OS, ooy, oox, OH, OW, in_affine,
                                                   epi_affine, add, relu, True, split=split, in_amax=in_amax,
                                                   in_presplit=in_presplit))
        except RuntimeError:
            continue
        if best is None or ms < best[0]:
            best = (ms, cand)
    if best is None:
        del table[key]
    else:
        table[key] = best[1]


def _autotune_wgrad(key, x, dy, ksize, stride, in_affine, dy_amax=None, x_amax=None, dy_presplit=False):
    """(the operand-scale slots come from the caller: computed once, outside the timed candidates)"""
    scratch = torch.empty(dy.shape[3], x.shape[3], ksize, ksize, device=x.device, dtype=torch.float32)
    best = None
    for cand in tiling.wgrad_candidates(*key):
        tiling.FORCE_WGRAD[key] = cand
        try:
            ms = _time_launch(lambda: conv_wgrad(x, dy, scratch, ksize, stride, in_affine=in_affine, dy_amax=dy_amax,
                                                 x_amax=x_amax, dy_presplit=dy_presplit))
        except RuntimeError:
            continue
        if best is None or ms < best[0]:
            best = (ms, cand)
    if best is None:
        del tiling.FORCE_WGRAD[key]
    else:
        tiling.FORCE_WGRAD[key] = best[1]


def conv_fwd(x, wpk, Cout, ksize, stride, in_affine=None, epi_affine=None, epi_add=None, relu=False, stats=False,
             out=None, in_amax=None, out_amax=None, wlen=None):
    """Forward conv on NHWC x with packed weights. Returns (out, stats_partial or None).
    wlen: int32 device [B] valid output widths (length-masked eval forward): output columns x >= wlen[b] are stored as 0 after the
    whole epilogue and stay out of out_amax (spk_conv_mfma_len).
    f16x3 operand mode: in_amax = slot with the float bits of the absmax of the STAGED values (x itself, or the
    affine_estimate of relu(x*scale+shift) when in_affine is given); computed here with extra passes when omitted (tests)."""
    B, IH, IW, Cin = x.shape
    if split_for(ksize) == 3 and in_amax is None:
        in_amax = _amax_fwd_fallback(x, in_affine)
    OH, OW = conv_out_hw(IH, IW, ksize, stride)
    if out is None:
        out = torch.empty(B, OH, OW, Cout, device=x.device, dtype=torch.float32)
    taps = FWD_TAPS if ksize == 3 else [(0, 0, 0)]
    st = _conv_launch(x, wpk, out, Cout, taps, stride, 1, 0, 0, OH, OW, in_affine, epi_affine, epi_add, relu, stats,
                      split=split_for(ksize), in_amax=in_amax, out_amax=out_amax, wlen=wlen)
    return out, st


def conv_dgrad(dy, wpk_t, Cin, ksize, stride, in_hw, add=None, out=None, accumulate=False, bn_bwd=None, in_bnbwd=None,
               side=None, add_mask=None, in_amax=None, out_amax=None, side_amax=None, in_presplit=False, side_presplit=False):
    """Data gradient of conv_fwd: dy [B][OH][OW][Cout] -> dx [B][IH][IW][Cin].
    `add` (same shape as dx) is summed in the epilogue (only where the bits of `add_mask`, sign-mask words of the same
    shape, are set when that is given); accumulate=True adds onto the existing `out`.
    bn_bwd = (raw, act or None, bn4[4][Cin]) (stride-1 only): dx is the gradient wrt the output of that BatchNorm
    (+ReLU); the launch also returns the BatchNorm-backward partial sums -> (dx, partial).
    in_bnbwd = (raw, act or None, bn4[4][Cout], coef[3][Cout]) + side = (draw_out, dz_out or None) (stride-1 only): `dy` is
    the gradient wrt a BatchNorm(+ReLU) OUTPUT; the BatchNorm backward is applied while staging and the gradient wrt
    the raw conv output is also written to draw_out (and dy*mask to dz_out).
    f16x3 operand mode: in_amax = 1-element int32 tensor with the float bits of absmax(staged tensor) - for in_bnbwd an upper
    estimate of the BatchNorm-backward values (bn_bwd_coef(..., est_out=)) - that fixes the power-of-two operand scale; when
    omitted it is computed here with an extra pass (tests / tools; the engine always passes it).  out_amax / side_amax: slots
    the launch atomically maxes |dx| / |draw_out| into (float bits) for the kernels that consume those tensors.
    in_presplit: `dy` is an f16 pair tensor (bn_backward(pair_scale=)) scaled by the sigma of in_amax, staged by plain copy.
    side_presplit (with in_bnbwd): draw_out leaves as an f16 pair tensor scaled by the sigma of in_amax (the rigorous bound)."""
    B, OH, OW, Cout = dy.shape
    assert not in_presplit or in_amax is not None, "an f16 pair tensor comes with its scale slot"
    if split_for(ksize, True) == 3 and in_amax is None:
        in_amax = _amax_fallback(dy, in_bnbwd)
    IH, IW = in_hw
    if out is None:
        assert not accumulate
        out = torch.empty(B, IH, IW, Cin, device=dy.device, dtype=torch.float32)
    if accumulate:
        assert add is None
        add = out
    if stride == 1:
        if ksize == 3:
            taps = [(1 - kh, 1 - kw, kh * 3 + kw) for kh in range(3) for kw in range(3)]
        else:
            taps = [(0, 0, 0)]
        st = _conv_launch(dy, wpk_t, out, Cin, taps, 1, 1, 0, 0, IH, IW, None, None, add, False, False, bn_bwd, in_bnbwd,
                          side, split=split_for(ksize, True), add_mask=add_mask, in_amax=in_amax, out_amax=out_amax,
                          side_amax=side_amax, in_presplit=in_presplit, side_presplit=side_presplit)
        return (out, st) if bn_bwd is not None else out
    assert stride == 2 and bn_bwd is None and in_bnbwd is None and add_mask is None
    if ksize == 1:
        # only even input pixels receive gradient from a strided 1x1 conv
        if not accumulate:
            if add is not None:
                out.copy_(add)
            else:
                out.zero_()
        _conv_launch(dy, wpk_t, out, Cin, [(0, 0, 0)], 1, 2, 0, 0, (IH + 1) // 2, (IW + 1) // 2, None, None, out, False,
                     False, split=split_for(1, True), in_amax=in_amax, out_amax=out_amax, in_presplit=in_presplit)
        return out
    for cy in range(2):
        for cx in range(2):
            LH, LW = (IH - cy + 1) // 2, (IW - cx + 1) // 2
            if LH <= 0 or LW <= 0:
                continue
            taps = []
            for kh in range(3):
                if (cy + 1 - kh) % 2:
                    continue
                for kw in range(3):
                    if (cx + 1 - kw) % 2:
                        continue
                    taps.append(((cy + 1 - kh) // 2, (cx + 1 - kw) // 2, kh * 3 + kw))
            _conv_launch(dy, wpk_t, out, Cin, taps, 1, 2, cy, cx, LH, LW, None, None, add, False, False, split=split_for(3, True),
                         in_amax=in_amax, out_amax=out_amax, in_presplit=in_presplit)
    return out


_ws_cache = {}
_ws_retired = []


def _workspace(nbytes, device, name=None):
    """Scratch buffer per (purpose, device, launch stream): kernels on different streams never share one, and a named purpose has
    a buffer of its own (a GEMM may run between a weight gradient and its slab reduce)."""
    key = (name, str(device), torch.cuda.current_stream().cuda_stream)
    w = _ws_cache.get(key)
    if w is None or w.numel() * 4 < nbytes:
        if w is not None:
            _ws_retired.append(w)       # a captured hipGraph may still hold its address: never hand it back
        w = torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)
        _ws_cache[key] = w
    return w


def _plan_wgrad(B, Cin, OH, OW, Cout, ksize, stride, split, in_affine=False, dy_presplit=False):
    """Which weight-gradient family runs, on which tile, into how many slabs, under which label (as _plan_conv: no tensor, no
    device, no library call)."""
    TH, TW, WN = tiling.wgrad_tile(OH, OW, Cin, Cout, ksize, stride, split=split)
    f16_3x3 = split == 3 and ksize == 3
    if C32M16 and f16_3x3 and WN == 1 and dy_presplit:
        TH, TW, WN = tiling.c32m16_tile(OH, OW, Cin, Cout, ksize, stride) or (TH, TW, WN)      # the 32-channel-group 16x16x32 kernel has its own tile rule
    nreg = B * (-(-OH // TH)) * (-(-OW // TW))
    halo = ((TH - 1) * stride + ksize) * ((TW - 1) * stride + ksize)
    wv, hs = 4 // WN, 4 if halo <= 128 else 5
    nst = -(-(TH * TW) // 16)                                   # k-steps of the tile: one or two per wave group
    cg = 0
    # producer / consumer kernel (csrc/conv_wgrad_split.hip: conv_wgrad_ws_kernel): f16x3 3x3 launches whose two LDS slots fit
    if WS_WGRAD and f16_3x3 and not dy_presplit and 2 * (halo * 192 + nst * 16 * (WN * 192 + (64 if WN > 1 else 0))) <= 160 * 1024:
        family, label = "ws", "conv_wgrad_ws_kernel<%d,%d,%d,%d>" % (ksize * ksize, wv, WN, hs)
    # in-wave pipelined kernel (csrc/conv_wgrad_pipe.hip): two planar LDS slots of 64-byte rows
    elif (PIPE_WGRAD and f16_3x3 and not dy_presplit and nst % wv == 0 and nst // wv in (1, 2)
          and 2 * (2 * halo * 64 + 2 * WN * nst * 16 * 64) + 128 <= PIPE_MAX_LDS):
        family, label = "pipe", "conv_wgrad_pipe_kernel<%d,%d,%d,%d>" % (wv, WN, hs, nst // wv)
    # 3x3, f16x3: 2 input-channel groups x 2 output-channel groups of waves (csrc/conv_wgrad_wm.hip) ...
    elif (GROUPED_3X3 and f16_3x3 and WN == 2 and Cin % 64 == 0 and Cout % 64 == 0 and halo <= 112 and TH * TW <= 64
          and halo * 384 + nst * 16 * 448 <= 80 * 1024):
        # ... with a pair-tensor dy in the 16x16x32 form, X pixel pitch 416 B (csrc/conv_wgrad_wm16.hip)
        m16 = WM16 and dy_presplit and halo * 416 + 2 * -(-(TH * TW) // 32) * 32 * 256 <= 80 * 1024
        family, label, cg = ("wm16", "conv_wgrad_wm16_kernel", 2) if m16 else ("wm", "conv_wgrad_wm_kernel", 2)
    # ... and that kernel in its 32-channel-group layout (the first layer): four waves split the k-steps and fold at the end of the block
    elif (C32M16 and f16_3x3 and WN == 1 and dy_presplit and halo <= 192
          and halo * 192 + 2 * -(-(TH * TW) // 32) * 32 * 128 <= 80 * 1024):
        family, label = "c32m16", "conv_wgrad_c32m16_kernel"
    else:
        family = "split" if split else "f32"
        label = ("conv_wgrad_split_kernel<%d,%d,%d,%d,%d>" % (ksize * ksize, wv, WN, split, hs) if split
                 else "conv_wgrad_kernel<%d,%d,%d>" % (ksize * ksize, wv, WN))
    # 1x1, f16x3: conv_wgrad_1x1_kernel with 2 or 4 input-channel groups per block (csrc/conv_wgrad_1x1.hip)
    if GROUPED_1X1 and split == 3 and ksize == 1 and WN in (2, 4) and TH * TW <= 64:
        cg = 4 if Cin % 128 == 0 else (2 if Cin % 64 == 0 else 0)
        if cg and nst * 16 * (cg * 192 + WN * 192 + 64) > 80 * 1024:
            cg = 2 if cg == 4 else 0
        if cg:
            family, label = "1x1", "conv_wgrad_1x1_kernel<%d,%d,%d>" % (wv, WN, cg)
    nsplit = min(nreg, tiling.wgrad_nsplit(nreg, Cin, Cout, WN, WS_WGRAD_BLOCKS if family == "ws" else (GROUPED_1X1_BLOCKS if cg else None),
                                           cin_groups=cg or 1))
    flags = ((IN_AFFINE_RELU if in_affine else 0) | (CONV_WS if family == "ws" else 0) | (CONV_PIPE if family == "pipe" else 0)
             | (WGRAD_GROUPS | ({2: 1, 4: 2}[cg] << 12) if cg else 0) | (DY_PRESPLIT if dy_presplit else 0)
             | (hip.WGRAD_NOSHIFT if family in ("wm", "wm16") and not WM_SHIFT else 0)
             | (hip.WGRAD_M16 if family in ("wm16", "c32m16") else 0))
    return WgradPlan(TH, TW, WN, family, cg, nsplit, flags, label + (" C%d %dx%d" % (Cout, OH, OW) if LABEL_SHAPES else ""))


def conv_wgrad(x, dy, dw, ksize, stride, in_affine=None, accumulate=False, dy_amax=None, x_amax=None, dy_presplit=False):
    """dw (OIHW view, contiguous) <- weight gradient of conv(x) given dy.  f16x3 operand mode: dy_amax = slot with the float
    bits of absmax(dy) (computed here with an extra pass when omitted: tests / tools).  dy_presplit: dy is an f16 pair tensor
    scaled by the sigma of dy_amax (its scale slot), staged by plain copy."""
    B, IH, IW, Cin = x.shape
    _, OH, OW, Cout = dy.shape
    split = split_for(ksize, True)
    assert not dy_presplit or (split == 3 and dy_amax is not None), "an f16 pair tensor comes with its scale slot (f16x3 mode)"
    if split == 3 and dy_amax is None:
        dy_amax = absmax_into(dy, torch.zeros(1, device=dy.device, dtype=torch.int32))
    if split == 3 and x_amax is None:
        x_amax = _amax_fwd_fallback(x, in_affine)
    wkey = (OH, OW, Cin, Cout, ksize, stride)
    if tiling.AUTOTUNE and wkey not in tiling.FORCE_WGRAD and PROFILE is None and not torch.cuda.is_current_stream_capturing():
        tiling.FORCE_WGRAD[wkey] = tiling._wgrad_tile(*wkey)      # placeholder: stops the recursion below
        _autotune_wgrad(wkey, x, dy, ksize, stride, in_affine, dy_amax, x_amax, dy_presplit)
    p = _plan_wgrad(B, Cin, OH, OW, Cout, ksize, stride, split, in_affine is not None, dy_presplit)
    nbytes = hip.lib().spk_conv_wgrad_workspace(p.nsplit, ksize, Cin, Cout)
    ws = _workspace(nbytes, x.device)
    call("spk_conv_wgrad", ptr(x), ptr(dy), ptr(dw), ptr(ws),
         ptr(in_affine[0]) if in_affine else None, ptr(in_affine[1]) if in_affine else None,
         B, IH, IW, Cin, OH, OW, Cout, ksize, stride, p.TH, p.TW, p.WN, p.nsplit, p.flags, 1 if accumulate else 0, split,
         ptr(dy_amax) if split == 3 else None, ptr(x_amax) if split == 3 else None, stream(), label=p.label,
         flops=2.0 * B * OH * OW * Cout * Cin * ksize * ksize, nbytes=4.0 * (x.numel() + dy.numel() + nbytes / 4))
    call("spk_wgrad_reduce", ptr(ws), ptr(dw), p.nsplit, ksize, Cin, Cout, 1 if accumulate else 0, stream())
    return dw


def stem_fwd(x, w, epi_affine=None, relu=False, stats=False, amax_out=None, wlen=None):
    """x [B][F][T] -> [B][F][T][32] (+ stats partial [nblk][32][2]).
    wlen: int32 device [B] utterance lengths (<= T): frames t >= wlen[b] are read as 0 and stored as 0 (spk_stem_conv_fwd_len)."""
    B, F, T = x.shape
    out = torch.empty(B, F, T, 32, device=x.device, dtype=torch.float32)
    flags = (EPI_AFFINE if epi_affine is not None else 0) | (EPI_RELU if relu else 0) | (EPI_STATS if stats else 0)
    st = None
    if stats:
        st = torch.empty(hip.lib().spk_stem_fwd_blocks(B, F, T), 32, 2, device=x.device, dtype=torch.float32)
    args = (ptr(x), ptr(w), ptr(out), ptr(st), ptr(epi_affine[0]) if epi_affine else None,
            ptr(epi_affine[1]) if epi_affine else None, B, F, T)
    if wlen is None:
        call("spk_stem_conv_fwd", *args, flags, ptr(amax_out), stream())
    else:
        _check_wlen(wlen, B)
        call("spk_stem_conv_fwd_len", *args, flags | EPI_WMASK, ptr(amax_out), ptr(wlen), stream())
    return out, st


def stem_wgrad(x, draw, dw, accumulate=False):
    B, F, T = x.shape
    nblk = hip.lib().spk_stem_wgrad_blocks(B, F, T)
    ws = _workspace(nblk * 288 * 4, x.device)
    call("spk_stem_conv_wgrad", ptr(x), ptr(draw), ptr(dw), ptr(ws), B, F, T, 1 if accumulate else 0, stream())
    return dw


def stem_stats(x, w):
    """The statistics rows of stem_fwd(x, w, stats=True), bit for bit, without the output tensor (spk_stem_stats)."""
    B, F, T = x.shape
    st = torch.empty(hip.lib().spk_stem_fwd_blocks(B, F, T), 32, 2, device=x.device, dtype=torch.float32)
    call("spk_stem_stats", ptr(x), ptr(w), ptr(st), B, F, T, stream(), nbytes=4.0 * x.numel())
    return st


def stem_fwd_apply(x, w, scale, shift, mask=False, amax_out=None):
    """-> (raw0, a, sign words or None): stem_fwd followed by bn_apply(relu=True, mask=, amax_out=) in one launch that
    recomputes the convolution instead of reading raw0 back (spk_stem_fwd_apply); every value bit-equal to the two launches."""
    B, F, T = x.shape
    raw = torch.empty(B, F, T, 32, device=x.device, dtype=torch.float32)
    act = torch.empty_like(raw)
    mk = torch.empty(B * F * T, device=x.device, dtype=torch.int32) if mask else None
    call("spk_stem_fwd_apply", ptr(x), ptr(w), ptr(scale), ptr(shift), ptr(raw), ptr(act), ptr(mk), ptr(amax_out), B, F, T,
         stream(), nbytes=4.0 * (x.numel() + 2 * raw.numel()) + (raw.numel() / 8 if mask else 0))
    return raw, act, mk


def stem_bwd_wgrad(x, d, raw, bn4, coef, dw, accumulate=False):
    """stem_wgrad of the BatchNorm-backward apply (MASK_RAW) of d, formed in registers: d is only read and the gradient wrt raw
    is never stored (spk_stem_bwd_wgrad).  coef: the rows of bn_bwd_coef.  dw is bit-equal to the two launches."""
    B, F, T = x.shape
    nblk = hip.lib().spk_stem_wgrad_blocks(B, F, T)
    ws = _workspace(nblk * 288 * 4, x.device)
    call("spk_stem_bwd_wgrad", ptr(x), ptr(d), ptr(raw), ptr(bn4[0]), ptr(bn4[1]), ptr(bn4[2]), ptr(bn4[3]), ptr(coef), ptr(dw),
         ptr(ws), B, F, T, 1 if accumulate else 0, stream(), nbytes=4.0 * (x.numel() + 2 * raw.numel()))
    return dw


def bn_stats_partial(x2d):
    N, C = x2d.shape
    nblk = hip.lib().spk_bn_stats_blocks(N, C)
    part = torch.empty(nblk, C, 2, device=x2d.device, dtype=torch.float32)
    call("spk_bn_stats_partial", ptr(x2d), ptr(part), N, C, stream())
    return part


_ws64_cache = {}


def _ws64(device):
    """fp64 scratch of the two-stage BN finalize (spk_bn_finalize_workspace: 256 rows x C x 2 doubles; sized for C = 2048)."""
    w = _ws64_cache.get(str(device))
    if w is None:
        w = torch.zeros(256 * 2048 * 2 + 64, device=device, dtype=torch.float64)
        _ws64_cache[str(device)] = w
    return w


def bn_finalize(partial, count, gamma, beta, running_mean, running_var, nbt, out4, amax_in=None, est_out=None):
    """out4: tensor [4][C] = (mean, invstd, scale, shift).  amax_in + est_out (f16x3 mode): also the upper bound of
    |relu(raw*scale+shift)| from the slot with absmax(raw) (the affine_estimate value, without its launch)."""
    C = gamma.numel()
    call("spk_bn_finalize", ptr(partial), partial.shape[0], C, float(count), ptr(gamma), ptr(beta), ptr(running_mean),
         ptr(running_var), ptr(nbt), ptr(out4[0]), ptr(out4[1]), ptr(out4[2]), ptr(out4[3]), BN_MOMENTUM, BN_EPS,
         ptr(_ws64(partial.device)), ptr(amax_in), ptr(est_out), stream())


def bn_eval_coeffs(gamma, beta, rm, rv, out2):
    C = gamma.numel()
    call("spk_bn_eval_coeffs", ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(out2[0]), ptr(out2[1]), C, BN_EPS, stream())


def bn_apply(raw, scale, shift, res=None, res_affine=None, relu=True, out=None, mask=False, amax_out=None):
    """out = [relu](raw*scale + shift [+ res | + res*rscale + rshift]).  mask=True also returns the sign bits of `out`
    ([N][C/32] int32 words): the backward pass reads those instead of the activated tensor."""
    C = raw.shape[-1]
    N = raw.numel() // C
    if out is None:
        out = torch.empty_like(raw)
    mk = torch.empty(N * (C // 32), device=raw.device, dtype=torch.int32) if mask else None
    call("spk_bn_apply", ptr(raw), ptr(scale), ptr(shift), ptr(res),
         ptr(res_affine[0]) if res_affine else None, ptr(res_affine[1]) if res_affine else None, ptr(out), ptr(mk), N, C,
         1 if relu else 0, ptr(amax_out), stream(),
         nbytes=4.0 * raw.numel() * (2 + (1 if res is not None else 0)) + (raw.numel() / 8 if mask else 0))
    return (out, mk) if mask else out


def _bn_bwd_bytes(raw, mask_mode, passes):
    """algorithmic bytes of a BatchNorm-backward stream kernel: `passes` fp32 tensors (dy, raw, draw / dz) + the mask source"""
    n = raw.numel()
    return 4.0 * n * passes + {MASK_NONE: 0.0, MASK_RAW: 0.0, MASK_ACT: 4.0 * n}.get(mask_mode, n / 8.0)


def bn_backward(dy, raw, act, bn4, gamma, dgamma, dbeta, mask_mode, draw_out=None, dz_out=None, accumulate=False,
                partial=None, amax_out=None, pair=None, chan_amax=None):
    """Full BN backward (reduce -> finalize -> apply). bn4 = [mean, invstd, scale, shift] rows.
    `partial`: (sum dz, sum dz*xhat) rows already produced by the data-gradient epilogue (EPI_BNBWD) - skips the
    reduction pass.  Returns draw (gradient wrt the raw conv output).
    pair = (amax_in, raw_amax, est) (f16x3 mode): draw is written as an f16 PAIR tensor (include/spkhip.h) scaled by the sigma
    of `est`, the slot the finalize fills with the rigorous bound of |draw| from amax_in (absmax of dy) and raw_amax (absmax of
    raw): the data gradient and the weight gradient that consume draw stage it by plain copy with that slot as their scale.
    chan_amax ([C] int32 zeros, with pair): the reduction pass also takes the absmax of dz per CHANNEL and the bound uses it
    instead of the tensor-wide amax_in (needs partial=None: the reduction runs here)."""
    C = raw.shape[-1]
    N = raw.numel() // C
    coef = torch.empty(3, C, device=raw.device, dtype=torch.float32)
    if partial is None:
        nblk = hip.lib().spk_bn_stats_blocks(N, C)
        part = torch.empty(nblk, C, 2, device=raw.device, dtype=torch.float32)
        call("spk_bn_bwd_reduce", ptr(dy), ptr(raw), ptr(act), ptr(bn4[0]), ptr(bn4[1]), ptr(bn4[2]), ptr(bn4[3]), ptr(part),
             N, C, mask_mode, ptr(chan_amax), stream(), nbytes=_bn_bwd_bytes(raw, mask_mode, 2))
    else:
        assert chan_amax is None, "chan_amax comes out of the reduction pass: partial must be None"
        part, nblk = partial, partial.shape[0]
    call("spk_bn_bwd_finalize", ptr(part), nblk, C, float(N), ptr(gamma), ptr(bn4[1]), ptr(dgamma), ptr(dbeta), ptr(coef),
         1 if accumulate else 0, ptr(_ws64(raw.device)), ptr(pair[0]) if pair else None, ptr(pair[1]) if pair else None,
         ptr(bn4[0]) if pair else None, ptr(pair[2]) if pair else None, ptr(chan_amax) if pair else None, stream())
    if draw_out is None:
        draw_out = torch.empty_like(raw)
    call("spk_bn_bwd_apply", ptr(dy), ptr(raw), ptr(act), ptr(bn4[0]), ptr(bn4[1]), ptr(bn4[2]), ptr(bn4[3]), ptr(coef),
         ptr(draw_out), ptr(dz_out), N, C, mask_mode, ptr(amax_out), ptr(pair[2]) if pair else None, stream(),
         nbytes=_bn_bwd_bytes(raw, mask_mode, 3 + (1 if dz_out is not None else 0)))
    return draw_out


def bn_bwd_coef(partial, count, gamma, bn4, dgamma, dbeta, accumulate=False, amax_in=None, raw_amax=None, est_out=None,
                chan_amax=None):
    """BatchNorm-backward finalize only: dgamma, dbeta and the coefficient rows [gamma*invstd, mean(dz), mean(dz*xhat)].
    amax_in + raw_amax + est_out (f16x3 mode): also the RIGOROUS upper bound of the values the fused BatchNorm-backward data
    gradient will stage (spk_bnbwd_estimate), from the absmax of the incoming gradient and of the raw tensor."""
    C = gamma.numel()
    coef = torch.empty(3, C, device=gamma.device, dtype=torch.float32)
    assert est_out is None or (amax_in is not None and raw_amax is not None)
    call("spk_bn_bwd_finalize", ptr(partial), partial.shape[0], C, float(count), ptr(gamma), ptr(bn4[1]), ptr(dgamma),
         ptr(dbeta), ptr(coef), 1 if accumulate else 0, ptr(_ws64(gamma.device)), ptr(amax_in) if est_out is not None else None,
         ptr(raw_amax) if est_out is not None else None, ptr(bn4[0]) if est_out is not None else None, ptr(est_out),
         ptr(chan_amax) if est_out is not None else None, stream())
    return coef


def bn_bwd_partial(dy, raw, act, bn4, mask_mode, chan_amax=None):
    """Stand-alone reduction (sum dz, sum dz*xhat) when no data-gradient epilogue produced it.  chan_amax ([C] int32 zeros):
    also the absmax of dz per channel (float bits)."""
    C = raw.shape[-1]
    N = raw.numel() // C
    nblk = hip.lib().spk_bn_stats_blocks(N, C)
    part = torch.empty(nblk, C, 2, device=raw.device, dtype=torch.float32)
    call("spk_bn_bwd_reduce", ptr(dy), ptr(raw), ptr(act), ptr(bn4[0]), ptr(bn4[1]), ptr(bn4[2]), ptr(bn4[3]), ptr(part),
         N, C, mask_mode, ptr(chan_amax), stream(), nbytes=_bn_bwd_bytes(raw, mask_mode, 2))
    return part


# ---- squeeze-and-excitation (csrc/se.hip) -----------------------------------------------------------------------------------
def se_squeeze(x, wlen=None):
    """sums [B][C] (fp64) of an NHWC tensor over H*W; wlen (int32 device [B]): over the first wlen[b] columns only"""
    B, H, W, C = x.shape
    if wlen is not None:
        _check_wlen(wlen, B)
    part = torch.empty(B * hip.lib().spk_se_chunks(H * W) * C, device=x.device, dtype=torch.float32)
    sums = torch.empty(B, C, device=x.device, dtype=torch.float64)
    call("spk_se_squeeze", ptr(x), ptr(part), ptr(sums), B, H, W, C, ptr(wlen), stream(), nbytes=4.0 * x.numel())
    return sums


def se_excite(sums, affine, w1, w2, H, W, wlen=None):
    """(q [B][C], u [B][Cr], g [B][C]) from the squeeze sums: q = scale*sums/count + shift (affine=None: sums/count),
    u = relu(w1 q), g = sigmoid(w2 u); count = H*W, or H*wlen[b]"""
    B, C = sums.shape
    Cr = w1.shape[0]
    assert tuple(w1.shape) == (Cr, C) and tuple(w2.shape) == (C, Cr)
    q = torch.empty(B, C, device=sums.device, dtype=torch.float32)
    u = torch.empty(B, Cr, device=sums.device, dtype=torch.float32)
    g = torch.empty(B, C, device=sums.device, dtype=torch.float32)
    call("spk_se_excite", ptr(sums), ptr(affine[0]) if affine else None, ptr(affine[1]) if affine else None, ptr(w1), ptr(w2),
         ptr(q), ptr(u), ptr(g), B, C, Cr, H, W, ptr(wlen), stream())
    return q, u, g


def se_apply(raw, affine, gate, res=None, res_affine=None, relu=True, mask=False, amax_out=None, wlen=None, out=None):
    """out = [relu](gate[b][c]*(raw*scale + shift) [+ res | + res*rscale + rshift]) (affine=None: gate*raw); mask / amax_out as
    in bn_apply; wlen: columns w >= wlen[b] are stored as 0"""
    B, H, W, C = raw.shape
    if wlen is not None:
        _check_wlen(wlen, B)
    if out is None:
        out = torch.empty_like(raw)
    mk = torch.empty(B * H * W * (C // 32), device=raw.device, dtype=torch.int32) if mask else None
    call("spk_se_apply", ptr(raw), ptr(affine[0]) if affine else None, ptr(affine[1]) if affine else None, ptr(gate), ptr(res),
         ptr(res_affine[0]) if res_affine else None, ptr(res_affine[1]) if res_affine else None, ptr(out), ptr(mk), B, H, W, C,
         1 if relu else 0, ptr(amax_out), ptr(wlen), stream(),
         nbytes=4.0 * raw.numel() * (2 + (1 if res is not None else 0)) + (raw.numel() / 8 if mask else 0))
    return (out, mk) if mask else out


def se_bwd_reduce(dout, raw, act, mask_mode, chan_amax=None):
    """S [B][2][C] (fp64) = (sum_hw e, sum_hw e*raw), e = dout masked by act (MASK_ACT: the block output, MASK_BITS: its bits)"""
    B, H, W, C = raw.shape
    part = torch.empty(B * hip.lib().spk_se_chunks(H * W) * 2 * C, device=raw.device, dtype=torch.float32)
    S = torch.empty(B, 2, C, device=raw.device, dtype=torch.float64)
    call("spk_se_bwd_reduce", ptr(dout), ptr(raw), ptr(act), ptr(part), ptr(S), B, H * W, C, mask_mode, ptr(chan_amax), stream(),
         nbytes=_bn_bwd_bytes(raw, mask_mode, 2))
    return S


def se_bwd_gate(S, sums, q, u, g, w1, w2, bn4, gamma, dw1, dw2, dgamma, dbeta, HW, accumulate=False, pair=None, chan_amax=None):
    """Backward of the gate and the BatchNorm-backward finalize of dz = g*e + dq/HW from the [B][C] tables (spk_se_bwd_gate).
    -> (coef [3][C], dq [2][B][C] = (dq, dq/HW), da [B][C], du [B][Cr]).  dw1 / dw2 / dgamma / dbeta are overwritten or
    accumulated.  pair = (amax_in, raw_amax, est): est receives the rigorous bound of |draw| (f16x3 mode)."""
    B, C = q.shape
    Cr = u.shape[1]
    dev = q.device
    coef = torch.empty(3, C, device=dev, dtype=torch.float32)
    dq = torch.empty(2, B, C, device=dev, dtype=torch.float32)
    da = torch.empty(B, C, device=dev, dtype=torch.float32)
    du = torch.empty(B, Cr, device=dev, dtype=torch.float32)
    call("spk_se_bwd_gate", ptr(S), ptr(sums), ptr(q), ptr(u), ptr(g), ptr(w1), ptr(w2), ptr(bn4[0]), ptr(bn4[1]), ptr(bn4[2]),
         ptr(bn4[3]), ptr(gamma), ptr(da), ptr(du), ptr(dq), ptr(dw1), ptr(dw2), ptr(dgamma), ptr(dbeta), ptr(coef),
         1 if accumulate else 0, B, C, Cr, HW, ptr(pair[0]) if pair else None, ptr(pair[1]) if pair else None,
         ptr(chan_amax) if pair else None, ptr(pair[2]) if pair else None, stream())
    return coef, dq, da, du


def se_bwd_apply(dout, raw, act, mask_mode, g, dqs, bn4, coef, e_out=None, amax_out=None, pair_scale=None, draw_out=None):
    """draw = k1*(g*e + dqs - m1 - xhat*m2), fp32 or (pair_scale: the bound slot) an f16 pair tensor; e = dout*[out > 0] goes
    to e_out when given (dout itself is allowed)"""
    B, H, W, C = raw.shape
    if draw_out is None:
        draw_out = torch.empty_like(raw)
    call("spk_se_bwd_apply", ptr(dout), ptr(raw), ptr(act), ptr(g), ptr(dqs), ptr(bn4[0]), ptr(bn4[1]), ptr(coef), ptr(draw_out),
         ptr(e_out), B, H * W, C, mask_mode, ptr(amax_out), ptr(pair_scale), stream(),
         nbytes=_bn_bwd_bytes(raw, mask_mode, 3 + (1 if e_out is not None else 0)))
    return draw_out


def stats_pool_fwd(x, mode, wlen=None):
    """wlen: int32 device [B] valid widths: row b pools over its first wlen[b] frames only (spk_stats_pool_fwd_len)"""
    B, H, W, C = x.shape
    out = torch.empty(B, C * H * (2 if mode else 1), device=x.device, dtype=torch.float32)
    if wlen is None:
        call("spk_stats_pool_fwd", ptr(x), ptr(out), B, H, W, C, mode, stream())
    else:
        _check_wlen(wlen, B)
        call("spk_stats_pool_fwd_len", ptr(x), ptr(out), ptr(wlen), B, H, W, C, mode, stream())
    return out


def stats_pool_bwd(x, gout, mode, amax_out=None):
    """amax_out: slot the launch atomically maxes |dx| into (float bits): the operand scale of dx's f16x3 consumers"""
    B, H, W, C = x.shape
    dx = torch.empty_like(x)
    call("spk_stats_pool_bwd", ptr(x), ptr(gout), ptr(dx), B, H, W, C, mode, ptr(amax_out), stream())
    return dx


# ---- half-precision extraction (csrc/half.hip): fp16 NHWC activations, one fp16 product per MAC ------------
def h16_conv_tile():
    """(rows, columns) of the output tile of one block of spk_h16_conv_fwd"""
    return hip.lib().spk_h16_conv_tile(0), hip.lib().spk_h16_conv_tile(1)


def h16_conv_tiles_per_block():
    """(tiles per block, the number of (tile, output-channel tile) pairs of a launch from which on a block runs that many)"""
    return hip.lib().spk_h16_conv_tile(2), hip.lib().spk_h16_conv_tile(3)


def h16_packed_bytes(Cout, Cin, KH, KW):
    n = hip.lib().spk_h16_packed_bytes(Cout, Cin, KH, KW)
    if n < 0:
        hip.check(n, "spk_h16_packed_bytes")
    return n


def h16_pack_conv_weight(w, out=None):
    """OIHW fp32 -> the fp16 fragment images spk_h16_conv_fwd reads (a flat float16 tensor), rounded once to nearest even"""
    Cout, Cin, KH, KW = w.shape
    n = h16_packed_bytes(Cout, Cin, KH, KW) // 2
    if out is None or out.numel() != n:
        out = torch.empty(n, device=w.device, dtype=torch.float16)
    call("spk_h16_pack_conv_weight", ptr(w.contiguous()), ptr(out), Cout, Cin, KH, KW, stream())
    return out


def _check_h16(t, name):
    if t.dtype != torch.float16:
        raise TypeError("%s must be a float16 tensor, got %s" % (name, t.dtype))


def _check_ovf(ovf, B):
    if ovf.dtype != torch.int32 or ovf.numel() != B:
        raise ValueError("ovf must be an int32 tensor [B=%d], got %s %s" % (B, ovf.dtype, tuple(ovf.shape)))


def h16_stem_fwd(x, w, scale, shift, ovf, wlen=None):
    """x [B][F][T] fp32 -> relu(bn(conv(x))) as fp16 [B][F][T][32]; adds the not-finite stores of row b to ovf[b]"""
    B, F, T = x.shape
    _check_ovf(ovf, B)
    if wlen is not None:
        _check_wlen(wlen, B)
    out = torch.empty(B, F, T, 32, device=x.device, dtype=torch.float16)
    call("spk_h16_stem_fwd", ptr(x), ptr(w), ptr(scale), ptr(shift), ptr(out), ptr(wlen), ptr(ovf), B, F, T, stream(),
         label="h16_stem", flops=2.0 * 9 * 32 * B * F * T, nbytes=4.0 * x.numel() + 2.0 * out.numel())
    return out


def h16_conv_fwd(x, wpk, Cout, ksize, stride, scale, shift, ovf, add=None, relu=True, wlen=None):
    """x [B][IH][IW][Cin] fp16 -> [B][ceil(IH/stride)][ceil(IW/stride)][Cout] fp16 (3x3 pad 1 or 1x1):
    round16(mask(relu(acc * scale + shift + add))); adds the not-finite stores of row b to ovf[b]"""
    _check_h16(x, "x")
    B, IH, IW, Cin = x.shape
    _check_ovf(ovf, B)
    OH, OW = (IH + stride - 1) // stride, (IW + stride - 1) // stride
    out = torch.empty(B, OH, OW, Cout, device=x.device, dtype=torch.float16)
    if add is not None:
        _check_h16(add, "add")
        assert add.shape == out.shape, "the residual has the shape of the output"
    if wlen is not None:
        _check_wlen(wlen, B)
    call("spk_h16_conv_fwd", ptr(x), ptr(wpk), ptr(scale), ptr(shift), ptr(add), ptr(out), ptr(wlen), ptr(ovf), B, IH, IW, Cin,
         Cout, ksize, stride, 1 if relu else 0, stream(), label="h16_conv%dx%d_s%d_%dto%d" % (ksize, ksize, stride, Cin, Cout),
         flops=2.0 * B * OH * OW * Cout * Cin * ksize * ksize,
         nbytes=2.0 * (x.numel() + out.numel() * (2 if add is not None else 1) + Cout * Cin * ksize * ksize))
    return out


def h16_stats_pool_fwd(x, mode, wlen=None):
    """x [B][H][W][C] fp16 -> fp32 [B][C*H*(1+mode)]: stats_pool_fwd's arithmetic in fp32 on the fp16 map"""
    _check_h16(x, "x")
    B, H, W, C = x.shape
    if wlen is not None:
        _check_wlen(wlen, B)
    out = torch.empty(B, C * H * (2 if mode else 1), device=x.device, dtype=torch.float32)
    call("spk_h16_stats_pool_fwd", ptr(x), ptr(out), ptr(wlen), B, H, W, C, mode, stream(), label="h16_stats_pool",
         flops=4.0 * x.numel(), nbytes=2.0 * x.numel() + 4.0 * out.numel())
    return out


def _ptr_rows(t):
    """Device pointer of a 2-D tensor whose rows are contiguous but may be pitched (a column slice of a wider tensor): the
    callee takes stride(0) as its leading dimension."""
    assert t.is_cuda and t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1) and t.stride(0) >= t.shape[1], \
        "libspkhip takes rows of unit stride only"
    return t.data_ptr()


def gemm(A, Bm, M, N, K, sam, sak, sbk, sbn, bias=None, out=None, alpha=1.0, accumulate=False):
    """out[M][N] = alpha * sum_k A[m*sam+k*sak] * B[k*sbk+n*sbn] (+bias[n]) (+out).  `out` may be a column slice of a wider
    tensor (ldc = out.stride(0) > N)."""
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    ws = _workspace(hip.lib().spk_gemm_workspace(M, N, K), A.device, name="gemm")
    call("spk_gemm_f32", ptr(A), ptr(Bm), _ptr_rows(out), ptr(bias), M, N, K, sam, sak, sbk, sbn, out.stride(0), float(alpha),
         1 if accumulate else 0, ptr(ws), stream(), label="gemm_f32_kernel", flops=2.0 * M * N * K)
    return out


def linear_fwd(x, w, bias=None):
    """x [M][K] @ w[N][K]^T + bias."""
    M, K = x.shape
    N = w.shape[0]
    return gemm(x, w, M, N, K, K, 1, 1, K, bias=bias)


def linear_bwd(x, w, dy, dw, db=None, need_dx=True, accumulate=False):
    """Gradients of linear_fwd: dx [M][K] = dy @ w; dw [N][K] = dy^T @ x; db = colsum(dy)."""
    M, K = x.shape
    N = w.shape[0]
    dx = None
    if need_dx:
        dx = gemm(dy, w, M, K, N, N, 1, K, 1)
    gemm(dy, x, N, K, M, 1, N, K, 1, out=dw, accumulate=accumulate)
    if db is not None:
        call("spk_colsum", ptr(dy), ptr(db), M, N, 1 if accumulate else 0, stream())
    return dx


def l2norm_fwd(x):
    R, D = x.shape
    y = torch.empty_like(x)
    inv = torch.empty(R, device=x.device, dtype=torch.float32)
    call("spk_l2norm_fwd", ptr(x), ptr(y), ptr(inv), R, D, 1e-12, stream())
    return y, inv


def l2norm_bwd(y, inv, dy, out=None, accumulate=False):
    R, D = y.shape
    if out is None:
        out = torch.empty_like(y)
    call("spk_l2norm_bwd", ptr(y), ptr(inv), ptr(dy), ptr(out), R, D, 1e-12, 1 if accumulate else 0, stream())
    return out


def aam_margin_fwd(cosv, label, m, s):
    B, S = cosv.shape
    logits = torch.empty_like(cosv)
    call("spk_aam_margin_fwd", ptr(cosv), ptr(label), ptr(logits), B, S, float(m), float(s), stream())
    return logits


def aam_margin_bwd(cosv, label, dlogits, m, s):
    B, S = cosv.shape
    dcos = torch.empty_like(cosv)
    call("spk_aam_margin_bwd", ptr(cosv), ptr(label), ptr(dlogits), ptr(dcos), B, S, float(m), float(s), stream())
    return dcos


def softmax_ce(logits, label, grad_scale=None, want_rank=True):
    """-> (loss_row [B], dlogits or None, rank [B] int32 or None)."""
    B, S = logits.shape
    loss_row = torch.empty(B, device=logits.device, dtype=torch.float32)
    dl = torch.empty_like(logits) if grad_scale is not None else None
    rank = torch.empty(B, device=logits.device, dtype=torch.int32) if want_rank else None
    call("spk_softmax_ce", ptr(logits), ptr(label), ptr(loss_row), ptr(dl), ptr(rank), B, S,
         float(grad_scale if grad_scale is not None else 0.0), stream())
    return loss_row, dl, rank


def mean(v):
    out = torch.empty(1, device=v.device, dtype=torch.float32)
    call("spk_mean", ptr(v), ptr(out), v.numel(), stream())
    return out


def relu_bwd(y, dy):
    dx = torch.empty_like(dy)
    call("spk_relu_bwd", ptr(y), ptr(dy), ptr(dx), y.numel(), stream())
    return dx


def sgd_step(p, g, buf, lr, momentum, weight_decay, grad_scale, first):
    call("spk_sgd_step", ptr(p), ptr(g), ptr(buf), p.numel(), float(lr), float(momentum), float(weight_decay),
         float(grad_scale), 1 if first else 0, stream())


# ---- scoring back end ---------------------------------------------------------------------------------------------
def center_normalize(emb, mean=None, eps=1e-8):
    """rows of emb [N][D] minus mean, scaled to unit length (max(norm, eps))."""
    N, D = emb.shape
    out = torch.empty_like(emb)
    call("spk_center_normalize", ptr(emb), ptr(mean), ptr(out), N, D, float(eps), stream())
    return out


def trial_cosine(en, te, ia, ib):
    """out[t] = <en[ia[t]], te[ib[t]]>; ia / ib int32 device tensors (validated by the caller)."""
    T = ia.numel()
    out = torch.empty(T, device=en.device, dtype=torch.float32)
    assert ia.dtype == torch.int32 and ib.dtype == torch.int32 and ib.numel() == T and en.shape[1] == te.shape[1]
    call("spk_trial_cosine", ptr(en), ptr(te), ptr(ia), ptr(ib), ptr(out), T, en.shape[1], en.shape[0], te.shape[0], stream())
    return out


def topk_mean_std(scores, k):
    """mean / unbiased std of the k largest entries of every row of scores [N][M] (a column slice of a wider tensor is fine:
    ld = scores.stride(0))."""
    N, M = scores.shape
    mean = torch.empty(N, device=scores.device, dtype=torch.float32)
    std = torch.empty_like(mean)
    call("spk_topk_mean_std", _ptr_rows(scores), ptr(mean), ptr(std), N, M, int(k), scores.stride(0), stream())
    return mean, std


# ---- evaluation stage (csrc/eval.hip) -------------------------------------------------------------------------------------
def sort_tile():
    """(key, index) pairs one block of spk_sort_trials sorts in LDS"""
    return hip.lib().spk_eval_tile(0)


def sweep_block():
    """positions per block of the scan inside spk_error_sweep"""
    return hip.lib().spk_eval_tile(1)


def segment_mean(emb, rows, seg_off):
    """emb [N][D] float64, rows [N] int32 grouped by segment, seg_off [S+1] int32 -> float32 [S][D] (spk_segment_mean)."""
    N, D = emb.shape
    S = seg_off.numel() - 1
    assert emb.dtype == torch.float64 and rows.dtype == torch.int32 and seg_off.dtype == torch.int32 and rows.numel() == N
    out = torch.empty(S, D, device=emb.device, dtype=torch.float32)
    call("spk_segment_mean", ptr(emb), ptr(rows), ptr(seg_off), ptr(out), N, S, D, stream())
    return out


def trial_snorm(score, ia, ib, e_mean, e_std, t_mean, t_std):
    """adaptive S-norm of score [T] (float32 or float64) -> float64 [T]; the statistics are float64 tables indexed by ia / ib."""
    T = score.numel()
    assert score.dtype in (torch.float32, torch.float64) and ia.dtype == torch.int32 and ib.dtype == torch.int32
    assert ia.numel() == T and ib.numel() == T and all(t.dtype == torch.float64 for t in (e_mean, e_std, t_mean, t_std))
    out = torch.empty(T, device=score.device, dtype=torch.float64)
    call("spk_trial_snorm", ptr(score), 1 if score.dtype == torch.float64 else 0, ptr(ia), ptr(ib), ptr(e_mean), ptr(e_std),
         ptr(t_mean), ptr(t_std), ptr(out), T, stream())
    return out


def sort_trials(score):
    """score [T] float64 without NaN -> int32 [T] (the uint32 permutation; T < 2^31): ascending, ties in index order."""
    T = score.numel()
    assert score.dtype == torch.float64 and score.dim() == 1
    if T < 1 or T >= 1 << 31:
        raise ValueError("sort_trials: T=%d must lie in [1, 2^31)" % T)
    if bool(torch.isnan(score).any()):
        raise ValueError("sort_trials: a score is NaN")
    order = torch.empty(T, device=score.device, dtype=torch.int32)
    ws = torch.empty(hip.lib().spk_sort_trials_workspace(T), device=score.device, dtype=torch.uint8)
    call("spk_sort_trials", ptr(score), ptr(order), ptr(ws), T, stream())
    return order


def error_sweep(score, label, order, costs):
    """score [T] float64, label [T] uint8, order [T] from sort_trials, costs: P <= 8 triples (p_target, c_miss, c_fa) ->
    (out_d [1+2P] float64, out_i [3+P] int64) on the device, laid out as include/spkhip.h says."""
    T, P = score.numel(), len(costs)
    assert score.dtype == torch.float64 and label.dtype == torch.uint8 and order.dtype == torch.int32
    assert label.numel() == T and order.numel() == T and P <= 8
    cd = torch.tensor([[float(v) for v in c] for c in costs], dtype=torch.float64).reshape(P, 3).to(score.device)
    out_d = torch.empty(1 + 2 * P, device=score.device, dtype=torch.float64)
    out_i = torch.empty(3 + P, device=score.device, dtype=torch.int64)
    ws = torch.empty(hip.lib().spk_error_sweep_workspace(T, P), device=score.device, dtype=torch.uint8)
    call("spk_error_sweep", ptr(score), ptr(label), ptr(order), ptr(cd) if P else None, P, ptr(out_d), ptr(out_i), ptr(ws), T,
         stream())
    return out_d, out_i


# ---- PLDA back end (csrc/plda.hip) ---------------------------------------------------------------------------------------------
def _f64_flag(t):
    assert t.dtype in (torch.float32, torch.float64), t.dtype
    return 1 if t.dtype == torch.float64 else 0


def _f64_or_none(t, n):
    assert t is None or (t.dtype == torch.float64 and t.numel() == n and t.is_contiguous()), "a double[%d] table or None" % n
    return ptr(t)


def _rows_ld(t):
    """(device pointer, row pitch) of a 2-D float table whose rows are contiguous but may be pitched; one row has no pitch"""
    if t.shape[0] == 1:
        assert t.is_cuda and t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1), "libspkhip takes rows of unit stride only"
        return t.data_ptr(), t.shape[1]
    return _ptr_rows(t), t.stride(0)


def scatter_slab_rows(N):
    """rows per slab of spk_scatter_f64 for N rows"""
    return hip.lib().spk_scatter_slab_rows(int(N))


def scatter_f64(X, mu=None, w=None):
    """X [N][D] float32 / float64 (rows may be pitched), mu [D] and w [N] float64 or None -> C [D][D] float64 =
    sum_i w_i (x_i - mu)(x_i - mu)^T, symmetric bit for bit and the same bits on every run."""
    N, D = X.shape
    ws_bytes = hip.lib().spk_scatter_f64_workspace(N, D)
    if ws_bytes == 0:
        raise ValueError("scatter_f64: N=%d, D=%d out of range (1 <= D <= 512)" % (N, D))
    C = torch.empty(D, D, device=X.device, dtype=torch.float64)
    ws = torch.empty(ws_bytes // 8, device=X.device, dtype=torch.float64)
    call("spk_scatter_f64", _rows_ld(X)[0], _f64_flag(X), _rows_ld(X)[1], _f64_or_none(mu, D),
         _f64_or_none(w, N), ptr(C), ptr(ws), N, D, stream(), flops=2.0 * N * D * D, nbytes=float(N * D * X.element_size()))
    return C


def segment_sum_f64(X, seg_off, rows=None, mean=False):
    """X [N][D] float32 / float64, seg_off [K+1] int32, rows int32 (grouped row indices) or None (the rows themselves) ->
    (sums - with `mean` the means - [K][D] float64, counts [K] int32)"""
    N, D = X.shape
    K = seg_off.numel() - 1
    assert seg_off.dtype == torch.int32 and (rows is None or rows.dtype == torch.int32)
    out = torch.empty(K, D, device=X.device, dtype=torch.float64)
    count = torch.empty(K, device=X.device, dtype=torch.int32)
    call("spk_segment_sum_f64", _rows_ld(X)[0], _f64_flag(X), _rows_ld(X)[1], ptr(rows), ptr(seg_off), ptr(out), ptr(count),
         1 if mean else 0, K, D, stream())
    return out, count


def affine_lennorm(X, A=None, b=None, q=None, scale=False, out_dtype=torch.float32, out=None):
    """Y[i] = s_i (A x_i + b): X [N][Di] float32 / float64, A [Do][Di] float64 (None: identity), b [Do], q [Do] float64 or None;
    scale: s_i = sqrt(Do / sum_j y_j^2 q_j) (1 for a row whose sum is 0) -> Y [N][Do] of out_dtype (float32 / float64), written into
    `out` (a contiguous [N][Do] tensor, e.g. a row range of a larger table) when given."""
    N, Di = X.shape
    Do = Di if A is None else A.shape[0]
    assert A is None or (A.dtype == torch.float64 and A.shape == (Do, Di))
    assert out_dtype in (torch.float32, torch.float64)
    Y = torch.empty(N, Do, device=X.device, dtype=out_dtype) if out is None else out
    assert Y.shape == (N, Do) and Y.dtype == out_dtype and Y.is_contiguous()
    call("spk_affine_lennorm", _rows_ld(X)[0], _f64_flag(X), _rows_ld(X)[1], ptr(A), _f64_or_none(b, Do), _f64_or_none(q, Do),
         1 if scale else 0, ptr(Y), 1 if out_dtype == torch.float64 else 0, N, Di, Do, stream(),
         flops=0.0 if A is None else 2.0 * N * Di * Do)
    return Y


def plda_posterior_rows(mt, count, psi):
    """mt [K][D] float64, count [K] int32, psi [D] float64 -> (w, mt - w) float64 [K][D] (include/spkhip.h)"""
    K, D = mt.shape
    assert mt.dtype == torch.float64 and count.dtype == torch.int32 and count.numel() == K and psi.dtype == torch.float64
    w, r = torch.empty_like(mt), torch.empty_like(mt)
    call("spk_plda_posterior_rows", ptr(mt), ptr(count), ptr(psi), ptr(w), ptr(r), K, D, stream())
    return w, r


def plda_llr(en, te, ia, ib, psi, count, tab_count, tab_log):
    """en [n_en][D], te [n_te][D], psi [D] float64; ia / ib int32 [T] (validated by the caller); count int32 [n_en] or None (1);
    tab_count int32 [U], tab_log float64 [U][2] -> float32 [T]"""
    T, D = ia.numel(), en.shape[1]
    assert en.dtype == torch.float64 and te.dtype == torch.float64 and psi.dtype == torch.float64 and te.shape[1] == D
    assert ia.dtype == torch.int32 and ib.dtype == torch.int32 and ib.numel() == T and psi.numel() == D
    assert count is None or (count.dtype == torch.int32 and count.numel() == en.shape[0])
    U = tab_count.numel()
    assert tab_count.dtype == torch.int32 and tab_log.dtype == torch.float64 and tab_log.numel() == 2 * U
    out = torch.empty(T, device=en.device, dtype=torch.float32)
    call("spk_plda_llr", ptr(en), ptr(te), ptr(ia), ptr(ib), ptr(psi), ptr(count), ptr(tab_count), ptr(tab_log), U, ptr(out), T, D,
         en.shape[0], te.shape[0], stream())
    return out


# ---- windowed extraction (csrc/window.hip) ------------------------------------------------------------------
def _plan_i32(*cols):
    """host plan columns -> one contiguous int32 numpy array [len(cols)][N]; anything that is not an integer is refused"""
    out = []
    for c in cols:
        a = np.asarray(c)
        if a.dtype.kind not in "iu" or a.ndim != 1:
            raise TypeError("a window plan column must be a one-dimensional integer array")
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError("a window plan value does not fit 32 bits")
        out.append(a.astype(np.int32))
    return np.ascontiguousarray(np.stack(out))


def window_gather(src, row, start, length, Wcap, out=None):
    """src [B][F][T] float32 (device), the plan row / start / length: host integer arrays [N] -> out [N][F][Wcap]: window i is
    src[row[i], :, start[i]:start[i] + length[i]], zero past its length - bit for bit (spk_window_gather).  The plan is checked on
    the host before the launch; a bad plan raises and leaves `out` untouched."""
    B, F, T = src.shape
    plan = _plan_i32(row, start, length)
    N = plan.shape[1]
    assert src.dtype == torch.float32
    if out is None:
        out = torch.empty(N, F, int(Wcap), device=src.device, dtype=torch.float32)
    assert tuple(out.shape) == (N, F, int(Wcap)) and out.dtype == torch.float32
    if N == 0:
        return out
    pd = torch.from_numpy(plan).to(src.device)
    ip = ctypes.POINTER(ctypes.c_int)
    call("spk_window_gather", ptr(src), B, F, T, plan[0].ctypes.data_as(ip), plan[1].ctypes.data_as(ip), plan[2].ctypes.data_as(ip),
         ptr(pd), ptr(out), N, int(Wcap), stream(), nbytes=4.0 * N * F * (float(plan[2].mean()) + int(Wcap)))
    return out


def window_mean(emb, seg_off, weight):
    """emb [N][D] float32 (device), seg_off: host integer array [U + 1] (0 = seg_off[0] < ... < seg_off[U] = N), weight [N]: host
    numbers or a float32 device tensor -> float32 [U][D], out[u] = sum_r weight[r] emb[r] / sum_r weight[r] over the rows of
    segment u in order, in fp32 (spk_window_mean).  An empty segment raises."""
    N, D = emb.shape
    so = _plan_i32(seg_off)[0]
    U = so.size - 1
    assert emb.dtype == torch.float32
    if not isinstance(weight, torch.Tensor):
        weight = torch.from_numpy(np.ascontiguousarray(weight, dtype=np.float32)).to(emb.device)
    assert weight.dtype == torch.float32 and weight.numel() == N
    out = torch.empty(max(U, 0), D, device=emb.device, dtype=torch.float32)
    sd = torch.from_numpy(so).to(emb.device)
    call("spk_window_mean", ptr(emb), N, D, so.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ptr(sd), ptr(weight), ptr(out), U,
         stream(), nbytes=4.0 * (N * D + U * D))
    return out


# ---- diarization back end (csrc/diar.hip) ---------------------------------------------------------------------
def diar_tables(rec_off, Ntot):
    """host rec_off [R + 1] -> (rec_off as contiguous int64, tab int64 [3][R + 1] = rec_off, mat_off, tile_off), both on the host.
    A rec_off that does not start at 0, is not strictly increasing or does not end at Ntot raises (spk_diar_tables)."""
    ro = np.asarray(rec_off)
    if ro.dtype.kind not in "iu" or ro.ndim != 1 or ro.size < 2:
        raise TypeError("rec_off must be a one-dimensional integer array of at least two entries")
    ro = np.ascontiguousarray(ro, dtype=np.int64)
    tab = np.zeros((3, ro.size), dtype=np.int64)
    hip.call("spk_diar_tables", ro.ctypes.data, ro.size - 1, int(Ntot), tab.ctypes.data)
    return ro, tab


def _batch(rec, Ntot=None):
    """rec: a RecBatch (of Ntot rows), or host rec_off [R + 1], which the library checks first (spk_diar_tables: RuntimeError)"""
    if not isinstance(rec, RecBatch):
        diar_tables(rec, np.asarray(rec)[-1] if Ntot is None else Ntot)
    return RecBatch.of(rec, Ntot)


def score_dense_q(U, k, scale, rec=None):
    """U [N][D] float64 -> q [N] float64, q_i = scale sum_d k_d U_id^2 with k [D] (spk_score_dense_q), or with k [R][D] and rec (a
    RecBatch or host rec_off) the k of row i's recording (spk_score_dense_q_rec)"""
    N, D = U.shape
    assert U.dtype == torch.float64 and k.dtype == torch.float64 and k.is_contiguous()
    q = torch.empty(N, device=U.device, dtype=torch.float64)
    if k.dim() == 1:
        assert k.numel() == D
        call("spk_score_dense_q", ptr(U), ptr(k), float(scale), ptr(q), N, D, stream(), nbytes=8.0 * N * D)
        return q
    b = _batch(rec, N)
    assert k.numel() == b.R * D
    call("spk_score_dense_q_rec", ptr(U), b.rec_off.ctypes.data, ptr(b.table(U.device)), ptr(k), float(scale), ptr(q), N, D, b.R,
         stream(), nbytes=8.0 * N * D)
    return q


def score_dense(U, rec, q, g, K, out=None):
    """U [Ntot][D], q [Ntot] float64 (device), rec: a RecBatch or host rec_off [R + 1] -> (out float32 [sum n^2], mat_off int64
    [R + 1] on the host): recording r's n x n matrix S[i][j] = (float)(q_i + q_j + K + sum_d g_d U_id U_jd) at out[mat_off[r]:],
    symmetric bit for bit.  g [D] float64 (device), K a number: one model (spk_score_dense); g [R][D], K a float64 device tensor [R]:
    recording r's own (spk_score_dense_rec).  `out`: a float32 device tensor of >= mat_off[R] elements; a bad rec_off leaves it untouched."""
    Ntot, D = U.shape
    b = _batch(rec, Ntot)
    per_rec = torch.is_tensor(K)
    assert U.dtype == torch.float64 and q.dtype == torch.float64 and g.dtype == torch.float64 and q.numel() == Ntot
    assert (K.dtype == torch.float64 and K.numel() == b.R and g.numel() == b.R * D and g.is_contiguous()) if per_rec else g.numel() == D
    total = int(b.mat_off[-1])
    if out is None:
        out = torch.empty(total, device=U.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.numel() >= total
    call("spk_score_dense_rec" if per_rec else "spk_score_dense", ptr(U), b.rec_off.ctypes.data, ptr(b.table(U.device)), ptr(q),
         ptr(g), ptr(K) if per_rec else float(K), ptr(out), Ntot, D, b.R, stream(), flops=1.0 * total * D,
         nbytes=4.0 * total + 8.0 * Ntot * D)
    return out, b.mat_off.copy()


def ahc_threads():
    """threads of the workgroup that clusters one recording"""
    return hip.lib().spk_ahc_threads()


def ahc_max_n():
    """the largest recording (windows) spk_ahc_batch takes"""
    return hip.lib().spk_ahc_max_n()


def ahc_batch(scores, rec, min_clusters, threshold, ws_budget_bytes=1 << 31):
    """scores: float32 device tensor, the matrices of score_dense laid end to end; rec: a RecBatch or host rec_off [R + 1];
    min_clusters [R] integers; threshold [R] floats, -inf = none -> (labels int32 [Ntot], merges int32 [Ntot][2], merge_cost float64
    [Ntot], n_merges int32 [R]) on the device (spk_ahc_batch; the rule: include/spkhip.h), in launches of consecutive recordings
    whose fp64 tables fit ws_budget_bytes (RecBatch.chunks; one recording always goes)."""
    b = _batch(rec)
    R, Ntot = b.R, b.Ntot
    if int(b.n.max()) > ahc_max_n():
        raise ValueError("ahc_batch: a recording has %d windows, the cap is %d" % (int(b.n.max()), ahc_max_n()))
    assert scores.dtype == torch.float32 and scores.numel() >= int(b.mat_off[R])
    dev = scores.device
    mc = torch.from_numpy(np.ascontiguousarray(min_clusters, dtype=np.int32)).to(dev)
    th = torch.from_numpy(np.ascontiguousarray(threshold, dtype=np.float64)).to(dev)
    assert mc.numel() == R and th.numel() == R
    labels, nm = torch.empty(Ntot, device=dev, dtype=torch.int32), torch.empty(R, device=dev, dtype=torch.int32)
    merges, cost = torch.zeros(Ntot, 2, device=dev, dtype=torch.int32), torch.zeros(Ntot, device=dev, dtype=torch.float64)
    for lo, hi in b.chunks(lambda lo, hi: 8 * int(b.mat_off[hi] - b.mat_off[lo]), ws_budget_bytes):
        sb, r0, r1 = b.sub(lo, hi)
        need, m0 = int(sb.mat_off[-1]), int(b.mat_off[lo])
        ws = torch.empty(need, device=dev, dtype=torch.float64)
        call("spk_ahc_batch", scores[m0:].data_ptr(), sb.rec_off.ctypes.data, ptr(sb.table(dev)), mc[lo:hi].data_ptr(),
             th[lo:hi].data_ptr(), ptr(ws), need, labels[r0:r1].data_ptr(), merges[r0:r1].data_ptr(), cost[r0:r1].data_ptr(),
             nm[lo:hi].data_ptr(), r1 - r0, hi - lo, stream(), nbytes=12.0 * need)
    return labels, merges, cost, nm


# ---- VBx resegmentation (csrc/diar.hip) -----------------------------------------------------------------------
def vbx_threads():
    """threads of the workgroup that runs the VB-HMM of one recording"""
    return hip.lib().spk_vbx_threads()


def vbx_max_states():
    """the largest Smax spk_vbx_batch takes (one lane per state)"""
    return hip.lib().spk_vbx_max_states()


def vbx_ws_elems(rec_off, Smax, D):
    """doubles of workspace spk_vbx_batch needs for the batch; a shape it refuses raises"""
    ro = np.ascontiguousarray(np.asarray(rec_off), dtype=np.int64)
    n = hip.lib().spk_vbx_ws_elems(ro.ctypes.data, ro.size - 1, int(Smax), int(D))
    if n < 0:
        hip.check(int(n), "spk_vbx_ws_elems")
    return int(n)


def vbx_batch(X, Phi, rec, n_states, gamma, pi, Fa=0.3, Fb=17.0, loop_prob=0.99, max_iters=40, epsilon=1e-6, elbo=None,
              n_iters=None, ws_budget_bytes=1 << 31):
    """X [Ntot][D], Phi [D], gamma [Ntot][Smax], pi [R][Smax]: float64 device tensors; rec: a RecBatch or host rec_off [R + 1];
    n_states [R]: host integers.  Runs the VB-HMM of every recording (spk_vbx_batch; the rule: DESIGN.md section 6o) and updates
    gamma and pi in place -> (elbo float64 [R][max_iters], n_iters int32 [R]) on the device; recording r fills elbo[r][:n_iters[r]] and leaves the other
    slots as they were (NaN in a tensor made here).  Launches whose workspace fits ws_budget_bytes (RecBatch.chunks): the same bits."""
    Ntot, D = X.shape
    b = _batch(rec, Ntot)
    R = b.R
    ns = np.ascontiguousarray(np.asarray(n_states), dtype=np.int32)
    Smax = gamma.shape[1]
    assert X.dtype == torch.float64 and Phi.dtype == torch.float64 and gamma.dtype == torch.float64 and pi.dtype == torch.float64
    assert Phi.numel() == D and gamma.shape == (Ntot, Smax) and pi.shape == (R, Smax) and ns.shape == (R,)
    assert X.is_contiguous() and gamma.is_contiguous() and pi.is_contiguous()      # (row slices of them go to the launches)
    dev = X.device
    if elbo is None:
        elbo = torch.full((R, max(int(max_iters), 1)), float("nan"), device=dev, dtype=torch.float64)
    if n_iters is None:
        n_iters = torch.zeros(R, device=dev, dtype=torch.int32)
    assert elbo.dtype == torch.float64 and elbo.shape == (R, max(int(max_iters), 1)) and elbo.is_contiguous()
    assert n_iters.dtype == torch.int32 and n_iters.numel() == R and n_iters.is_contiguous()
    per_row, per_rec = 8 * (3 + 2 * Smax), 8 * Smax * D
    nsd = torch.from_numpy(ns).to(dev)
    for lo, hi in b.chunks(lambda lo, hi: per_row * int(b.rec_off[hi] - b.rec_off[lo]) + per_rec * (hi - lo), ws_budget_bytes):
        sb, r0, r1 = b.sub(lo, hi)
        need = vbx_ws_elems(sb.rec_off, Smax, D)
        ws = torch.empty(need, device=dev, dtype=torch.float64)
        call("spk_vbx_batch", X[r0:r1].data_ptr(), ptr(Phi), sb.rec_off.ctypes.data, ptr(sb.table(dev)), ns[lo:hi].ctypes.data,
             nsd[lo:hi].data_ptr(), gamma[r0:r1].data_ptr(), pi[lo:hi].data_ptr(), float(Fa), float(Fb), float(loop_prob),
             int(max_iters), float(epsilon), ptr(ws), need, elbo[lo:hi].data_ptr(), n_iters[lo:hi].data_ptr(), r1 - r0, D, hi - lo, Smax,
             stream(), nbytes=8.0 * need)
    return elbo, n_iters


# ---- diarization scoring (csrc/der.hip) -----------------------------------------------------------------------
def der_limits():
    """(reference speakers, hypothesis labels, hypothesis pieces) one spk_der_batch job takes"""
    l = hip.lib()
    return l.spk_der_max_ref(), l.spk_der_max_hyp(), l.spk_der_max_turns()


def der_ws_elems(pieces, Sr, Sh):
    """8-byte words of workspace of one job; a shape over the limits raises"""
    n = hip.lib().spk_der_ws_elems(int(pieces), int(Sr), int(Sh))
    if n < 0:
        hip.check(int(n), "spk_der_ws_elems")
    return int(n)


def ahc_cut_batch(merges, merge_cost, n_merges, rec, thresholds):
    """merges int32 [Ntot][2], merge_cost float64 [Ntot], n_merges int32 [R]: device tensors as ahc_batch returns them; rec: a RecBatch
    or host rec_off; thresholds [K] floats -> labels int32 [K][Ntot] on the device (spk_ahc_cut_batch)"""
    b = _batch(rec)
    dev = merges.device
    th = torch.from_numpy(np.ascontiguousarray(thresholds, dtype=np.float64)).to(dev)
    K = th.numel()
    assert merges.dtype == torch.int32 and merges.shape == (b.Ntot, 2) and merge_cost.dtype == torch.float64 and merge_cost.numel() == b.Ntot
    assert n_merges.dtype == torch.int32 and n_merges.numel() == b.R
    labels = torch.empty(K, b.Ntot, device=dev, dtype=torch.int32)
    call("spk_ahc_cut_batch", ptr(merges), ptr(merge_cost), ptr(n_merges), b.rec_off.ctypes.data, ptr(b.table(dev)), ptr(th), K,
         ptr(labels), b.Ntot, b.R, stream(), nbytes=4.0 * K * b.Ntot)
    return labels


def der_pieces(labels, wstart, wend, rec):
    """labels int32 [K][Ntot], wstart / wend int64 [Ntot] (ticks, the windows of every recording in (start, end) order): device tensors
    -> (pstart, pend) int64 [K][Ntot]: the windows with the adjacent-pair midpoint cut (spk_der_pieces)"""
    K, Ntot = labels.shape
    b = _batch(rec, Ntot)
    assert labels.dtype == torch.int32 and wstart.dtype == torch.int64 and wend.dtype == torch.int64
    assert wstart.numel() == Ntot and wend.numel() == Ntot
    ps, pe = torch.empty(K, Ntot, device=labels.device, dtype=torch.int64), torch.empty(K, Ntot, device=labels.device, dtype=torch.int64)
    call("spk_der_pieces", ptr(labels), ptr(wstart), ptr(wend), b.rec_off.ctypes.data, ptr(b.table(labels.device)), K, ptr(ps), ptr(pe),
         Ntot, b.R, stream(), nbytes=20.0 * K * Ntot)
    return ps, pe


def der_batch(rec_tab, cells, jobs, plab, pstart, pend, ws_budget_bytes=1 << 31):
    """rec_tab int64 [R][4] = (first cell, cells, Sr, 0) and cells int64 [ncells][3] = (start, end, mask): host arrays, the reference
    side of every recording; jobs int64 [J][4] = (recording, first piece, pieces, Sh): host; plab int32, pstart, pend int64 [npieces]:
    device tensors -> (out int64 [J][5] = scored, miss, fa, conf, opt; mapping int32 [J][max_ref]) on the device (spk_der_batch), in
    launches of consecutive jobs whose workspaces fit ws_budget_bytes (one job always goes).  A job over the limits raises."""
    rec_tab = np.ascontiguousarray(rec_tab, dtype=np.int64).reshape(-1, 4)
    cells = np.ascontiguousarray(cells, dtype=np.int64).reshape(-1, 3)
    jobs = np.ascontiguousarray(jobs, dtype=np.int64).reshape(-1, 4)
    J, R = jobs.shape[0], rec_tab.shape[0]
    dev = plab.device
    assert plab.dtype == torch.int32 and pstart.dtype == torch.int64 and pend.dtype == torch.int64
    assert plab.is_contiguous() and pstart.is_contiguous() and pend.is_contiguous() and pstart.numel() == plab.numel() == pend.numel()
    max_ref = hip.lib().spk_der_max_ref()
    out = torch.zeros(J, 5, device=dev, dtype=torch.int64)
    mapping = torch.full((J, max_ref), -1, device=dev, dtype=torch.int32)
    if J == 0:
        return out, mapping
    if (jobs[:, 0] < 0).any() or (jobs[:, 0] >= R).any():
        raise ValueError("der_batch: a job names a recording outside the table of %d" % R)
    need = np.array([der_ws_elems(p, rec_tab[r, 2], sh) for r, _, p, sh in jobs], dtype=np.int64)
    rt_dev = torch.from_numpy(rec_tab).to(dev)
    cells_dev = torch.from_numpy(cells).to(dev) if cells.size else torch.zeros(1, 3, device=dev, dtype=torch.int64)
    budget = max(int(ws_budget_bytes) // 8, 1)
    lo = 0
    while lo < J:
        hi, tot = lo + 1, int(need[lo])
        while hi < J and tot + int(need[hi]) <= budget:
            tot += int(need[hi])
            hi += 1
        jt = np.zeros((hi - lo, 6), dtype=np.int64)
        jt[:, :4] = jobs[lo:hi]
        jt[1:, 4] = np.cumsum(need[lo:hi])[:-1]
        jt_dev = torch.from_numpy(jt).to(dev)
        ws = torch.empty(max(tot, 1), device=dev, dtype=torch.int64)
        call("spk_der_batch", rec_tab.ctypes.data, ptr(rt_dev), ptr(cells_dev), cells.shape[0], R, jt.ctypes.data, ptr(jt_dev), hi - lo,
             ptr(plab), ptr(pstart), ptr(pend), plab.numel(), ptr(ws), max(tot, 1), out[lo:hi].data_ptr(), mapping[lo:hi].data_ptr(),
             stream(), nbytes=8.0 * tot)
        lo = hi
    return out, mapping


# ---- per-recording PCA of the dense PLDA scores (csrc/pca.hip) ------------------------------------------------
def syevj_max_dim():
    """the largest order spk_syevj_batch takes"""
    return hip.lib().spk_syevj_max_dim()


def syevj_max_sweeps():
    """the sweep bound of the Jacobi iteration"""
    return hip.lib().spk_syevj_max_sweeps()


def syevj_batch(A, orders=None):
    """A [R][ld][ld] float64 (device), symmetric (the upper triangles are read); orders: host integers [R] in [1, ld] (default ld) ->
    (w [R][ld] descending, vec [R][ld][ld] with row k the eigenvector of w[k], sweeps int32 [R], info int32 [R]) on the device
    (spk_syevj_batch); zeros at and beyond a matrix's order."""
    R, ld = A.shape[0], A.shape[1]
    assert A.dtype == torch.float64 and A.dim() == 3 and A.shape[2] == ld and A.is_contiguous()
    od = np.full(R, ld, dtype=np.int32) if orders is None else np.ascontiguousarray(np.asarray(orders), dtype=np.int32)
    assert od.shape == (R,)
    need = hip.lib().spk_syevj_ws_elems(R, ld)
    if need < 0:
        raise ValueError("syevj_batch: %s" % hip.lib().spk_last_error().decode())
    dev = A.device
    ws = torch.empty(int(need), device=dev, dtype=torch.float64)
    w = torch.empty(R, ld, device=dev, dtype=torch.float64)
    vec = torch.empty(R, ld, ld, device=dev, dtype=torch.float64)
    sweeps = torch.empty(R, device=dev, dtype=torch.int32)
    info = torch.empty(R, device=dev, dtype=torch.int32)
    odd = torch.from_numpy(od).to(dev)
    call("spk_syevj_batch", ptr(A), od.ctypes.data, ptr(odd), ptr(ws), int(need), ptr(w), ptr(vec), ptr(sweeps), ptr(info), R, ld,
         stream(), nbytes=16.0 * R * ld * ld)
    return w, vec, sweeps, info


def pca_plda_ws_elems(rec_off, L):
    """doubles of workspace spk_pca_plda_batch needs for the batch; a shape it refuses raises"""
    ro = np.ascontiguousarray(np.asarray(rec_off), dtype=np.int64)
    n = hip.lib().spk_pca_plda_ws_elems(ro.ctypes.data, ro.size - 1, int(L))
    if n < 0:
        hip.check(int(n), "spk_pca_plda_ws_elems")
    return int(n)


def pca_plda_batch(Z, rec, W, B, T, psi, mean, E, ws_budget_bytes=1 << 31):
    """Z [Ntot][L] float32 (device): the rows of plda.project; rec: a RecBatch or host rec_off [R + 1]; W, B, T [L][L], psi and mean [L]
    float64 (device) -> (dim int32 [R], s [R][L], psi_r [R][L], A_r [R][L][L], b_r [R][L], info int32 [R]) on the device: steps 1-5
    of section 6p (spk_pca_plda_batch), in launches whose workspace fits ws_budget_bytes (RecBatch.chunks): the same bits however split."""
    Ntot, L = Z.shape
    b = _batch(rec, Ntot)
    R = b.R
    if L > syevj_max_dim():
        raise ValueError("pca_plda_batch: L=%d, the hip back end takes at most %d dimensions" % (L, syevj_max_dim()))
    assert Z.dtype == torch.float32 and Z.is_contiguous()
    for t, n in ((W, L * L), (B, L * L), (T, L * L), (psi, L), (mean, L)):
        assert t.dtype == torch.float64 and t.numel() == n and t.is_contiguous()
    dev = Z.device
    dim, info = (torch.empty(R, device=dev, dtype=torch.int32) for _ in range(2))
    s, psi_r, b_r = (torch.empty(R, L, device=dev, dtype=torch.float64) for _ in range(3))
    A_r = torch.empty(R, L, L, device=dev, dtype=torch.float64)
    per = 8 * (pca_plda_ws_elems(np.array([0, 1]), L) - 1)
    for lo, hi in b.chunks(lambda lo, hi: per * (hi - lo), ws_budget_bytes, max_recs=65535):
        sb, r0, r1 = b.sub(lo, hi)
        need = pca_plda_ws_elems(sb.rec_off, L)
        ws = torch.empty(need, device=dev, dtype=torch.float64)
        call("spk_pca_plda_batch", Z[r0:r1].data_ptr(), sb.rec_off.ctypes.data, ptr(sb.table(dev)), ptr(W), ptr(B), ptr(T), ptr(psi),
             ptr(mean), float(E), ptr(ws), need, dim[lo:hi].data_ptr(), s[lo:hi].data_ptr(), psi_r[lo:hi].data_ptr(),
             A_r[lo:hi].data_ptr(), b_r[lo:hi].data_ptr(), info[lo:hi].data_ptr(), r1 - r0, L, hi - lo, stream(), nbytes=8.0 * need)
    return dim, s, psi_r, A_r, b_r, info


def pca_score_terms(psi_r):
    """psi_r [R][L] float64 (device, zero padded) -> (g [R][L], k [R][L], qn [R][L] = 1 / (psi_r + 1), K [R]) on the device: the dense
    score's terms of every recording (diarize.plda_dense_terms) and the length normalisation's weights (spk_pca_score_terms)"""
    R, L = psi_r.shape
    assert psi_r.dtype == torch.float64 and psi_r.is_contiguous()
    g, k, qn = torch.empty_like(psi_r), torch.empty_like(psi_r), torch.empty_like(psi_r)
    K = torch.empty(R, device=psi_r.device, dtype=torch.float64)
    call("spk_pca_score_terms", ptr(psi_r), ptr(g), ptr(k), ptr(qn), ptr(K), R, L, stream())
    return g, k, qn, K


def affine_lennorm_rec(Z, rec, A_r, b_r, q_r, dim, scale):
    """Z [Ntot][L] float32, A_r [R][L][L], b_r [R][L], q_r [R][L] or None (ones), dim int32 [R] (device); rec: a RecBatch or host
    rec_off [R + 1] -> U [Ntot][L] float64: recording r's rows through its own map, Do = dim[r] in the scale, zeros beyond dim[r]
    (spk_affine_lennorm_rec)"""
    Ntot, L = Z.shape
    b = _batch(rec, Ntot)
    R = b.R
    assert Z.dtype == torch.float32 and Z.is_contiguous() and dim.dtype == torch.int32 and dim.numel() == R
    assert A_r.dtype == torch.float64 and A_r.numel() == R * L * L and b_r.dtype == torch.float64 and b_r.numel() == R * L
    assert q_r is None or (q_r.dtype == torch.float64 and q_r.numel() == R * L)
    U = torch.empty(Ntot, L, device=Z.device, dtype=torch.float64)
    call("spk_affine_lennorm_rec", ptr(Z), b.rec_off.ctypes.data, ptr(b.table(Z.device)), ptr(A_r), ptr(b_r), ptr(q_r), ptr(dim),
         1 if scale else 0, ptr(U), Ntot, L, R, stream(), flops=2.0 * Ntot * L * L)
    return U


# ---- calibration and fusion of trial scores (csrc/cal.hip) ------------------------------------------------------
def cal_sizes():
    """(trials per block, pools per PAV tile, doubles of the training state, threads per block) of csrc/cal.hip"""
    l = hip.lib()
    return tuple(l.spk_cal_tile(i) for i in range(4))


def _cal_ws(name, *shape):
    n = getattr(hip.lib(), name)(*shape)
    if n < 0:
        raise ValueError("%s%r: a shape the calibration kernels refuse" % (name, tuple(shape)))
    return int(n)


def cal_apply(cols, theta):
    """cols [K][T] float64 (device), theta: host [K + 1] -> llr [T] float64 (spk_cal_apply)"""
    K, T = cols.shape
    assert cols.dtype == torch.float64 and cols.is_contiguous()
    th = np.ascontiguousarray(theta, dtype=np.float64)
    assert th.size == K + 1
    llr = torch.empty(T, device=cols.device, dtype=torch.float64)
    call("spk_cal_apply", ptr(cols), th.ctypes.data, K, ptr(llr), T, stream(), nbytes=8.0 * (K + 1) * T)
    return llr


def cal_cllr(llr, label, costs, eta):
    """llr [T] float64, label [T] uint8 (device); costs: P <= 8 triples and their Bayes thresholds eta (host) -> (out_d [2 + P],
    out_i [2 + 2 P]) on the device, laid out as include/spkcal.h says (spk_cal_cllr)"""
    T, P = llr.numel(), len(costs)
    assert llr.dtype == torch.float64 and label.dtype == torch.uint8 and label.numel() == T and len(eta) == P
    cd = np.ascontiguousarray([[float(v) for v in c] for c in costs], dtype=np.float64).reshape(P, 3)
    ed = np.ascontiguousarray(eta, dtype=np.float64).reshape(P)
    out_d = torch.empty(2 + P, device=llr.device, dtype=torch.float64)
    out_i = torch.empty(2 + 2 * P, device=llr.device, dtype=torch.int64)
    need = _cal_ws("spk_cal_cllr_ws_elems", T)
    ws = torch.empty(need, device=llr.device, dtype=torch.int64)
    call("spk_cal_cllr", ptr(llr), ptr(label), cd.ctypes.data if P else None, ed.ctypes.data if P else None, P, ptr(out_d), ptr(out_i),
         ptr(ws), need, T, stream(), nbytes=9.0 * T)
    return out_d, out_i


def cal_train(cols, label, n_tar, p_target, tau, l2, epsilon, max_iters):
    """cols [K][T] float64, label [T] uint8 (device) -> (state float64 [96], istate int64 [4]) on the device once the max_iters
    launch pairs the call enqueues have run (spk_cal_train; nothing is downloaded here)"""
    K, T = cols.shape
    assert cols.dtype == torch.float64 and cols.is_contiguous() and label.dtype == torch.uint8 and label.numel() == T
    state = torch.empty(hip.lib().spk_cal_tile(2), device=cols.device, dtype=torch.float64)
    istate = torch.empty(4, device=cols.device, dtype=torch.int64)
    need = _cal_ws("spk_cal_train_ws_elems", T, K)
    ws = torch.empty(need, device=cols.device, dtype=torch.float64)
    call("spk_cal_train", ptr(cols), ptr(label), K, T, int(n_tar), float(p_target), float(tau), float(l2), float(epsilon), int(max_iters),
         ptr(state), ptr(istate), ptr(ws), need, stream(), nbytes=(8.0 * K + 1) * T)
    return state, istate


def cal_pav(score, label, order, upto=0):
    """score [T] float64, label [T] uint8, order [T] from sort_trials (device) -> {'tie', 'pools': int64 [T][2] (the first counts[0] /
    counts[3] rows hold pools), 'counts': int64 [8], 'pool_of': int32 [T], 'min_cllr': float64 [1]} on the device (spk_cal_pav)"""
    T = score.numel()
    assert score.dtype == torch.float64 and label.dtype == torch.uint8 and order.dtype == torch.int32
    assert label.numel() == T and order.numel() == T
    dev = score.device
    r = {"tie": torch.empty(T, 2, device=dev, dtype=torch.int64), "pools": torch.empty(T, 2, device=dev, dtype=torch.int64),
         "counts": torch.zeros(8, device=dev, dtype=torch.int64), "pool_of": torch.empty(T, device=dev, dtype=torch.int32),
         "min_cllr": torch.zeros(1, device=dev, dtype=torch.float64)}
    need = _cal_ws("spk_cal_pav_ws_elems", T)
    ws = torch.empty(need, device=dev, dtype=torch.int64)
    call("spk_cal_pav", ptr(score), ptr(label), ptr(order), ptr(r["tie"]), ptr(r["pools"]), ptr(r["counts"]), ptr(r["pool_of"]),
         ptr(r["min_cllr"]), ptr(ws), need, T, int(upto), stream(), nbytes=13.0 * T)
    return r


# ---- speaker-level bootstrap of the error-rate sweep (csrc/boot.hip) -----------------------------------------------
BOOT_WS_BYTES = 128 << 20      # workspace of one chunk of replicates at most (one group of replicates always runs)


def boot_sizes(U=None):
    """(positions per workgroup, largest U, largest count, cost triples per call, replicates per workgroup at most, threads) of
    csrc/boot.hip; with U: (replicates per workgroup, entries per row of the device count table) for that many units"""
    l = hip.lib()
    if U is None:
        return tuple(l.spkb_limit(i) for i in range(6))
    return l.spkb_group(int(U)), l.spkb_pitch(int(U))


def boot_pack(score, label, order, ua, ub, eta, U):
    """score [T] float64, label [T] uint8, order [T] from sort_trials, ua / ub [T] int32 in [0, U) (device); eta: P <= 8 thresholds
    (host) -> (rec: int64 [T], one record per sorted position; q: int64 [P], the sorted scores below each threshold) (spkb_pack)"""
    T, P = score.numel(), len(eta)
    assert score.dtype == torch.float64 and label.dtype == torch.uint8 and order.dtype == torch.int32
    assert ua.dtype == torch.int32 and ub.dtype == torch.int32
    assert label.numel() == T and order.numel() == T and ua.numel() == T and ub.numel() == T
    ed = np.ascontiguousarray(eta, dtype=np.float64).reshape(P)
    rec = torch.empty(T, device=score.device, dtype=torch.int64)
    q = torch.zeros(max(P, 1), device=score.device, dtype=torch.int64)
    call("spkb_pack", ptr(score), ptr(label), ptr(order), ptr(ua), ptr(ub), ed.ctypes.data if P else None, P, ptr(rec), ptr(q), T, int(U),
         stream(), nbytes=25.0 * T)
    return rec, q[:P]


def boot_table(counts, device):
    """counts [R][U] of integers in [0, 65 535] (host) -> the device table uint16 [R][pitch] (viewed as int16) spkb_sweep reads"""
    c = np.asarray(counts)
    R, U = c.shape
    pitch = boot_sizes(U)[1]
    tab = np.zeros((R, pitch), dtype=np.uint16)
    tab[:, :U] = c
    return torch.from_numpy(tab.view(np.int16)).to(device)


def boot_sweep(rec, q, table, U, cmax, costs, act_costs, chunk=None, upto=0):
    """rec, q from boot_pack, table from boot_table, cmax: the largest count; costs: P <= 8 triples of the minimum costs, act_costs:
    len(q) triples of the actual costs -> (out_d [R][1 + P + Pa] float64, out_i [R][4 + P + 2 Pa] int64) on the device, laid out as
    include/spkboot.h says.  The replicates run in chunks of `chunk` (default: what BOOT_WS_BYTES of workspace hold, whole groups).
    upto: 1 / 2 / 3 stop every chunk after that phase (tools/boot_bench.py: the differences are the phases); the outputs are then not
    written."""
    T, R, P, Pa = rec.numel(), table.shape[0], len(costs), len(act_costs)
    assert rec.dtype == torch.int64 and table.dtype == torch.int16 and table.is_contiguous() and q.numel() == Pa
    G, pitch = boot_sizes(U)
    assert table.shape[1] == pitch, "the table of boot_table for U"
    cd = np.ascontiguousarray([[float(v) for v in c] for c in costs], dtype=np.float64).reshape(P, 3)
    ad = np.ascontiguousarray([[float(v) for v in c] for c in act_costs], dtype=np.float64).reshape(Pa, 3)
    per = hip.lib().spkb_sweep_ws_elems(T, P, Pa, 1)
    if per < 0:
        raise ValueError("spkb_sweep_ws_elems(%d, %d, %d, 1): a shape the bootstrap kernels refuse" % (T, P, Pa))
    if chunk is None:
        chunk = max(1, BOOT_WS_BYTES // (8 * per) // G) * G
    chunk = max(1, min(int(chunk), R))
    out_d = torch.empty(R, 1 + P + Pa, device=rec.device, dtype=torch.float64)
    out_i = torch.empty(R, 4 + P + 2 * Pa, device=rec.device, dtype=torch.int64)
    ws = torch.empty(per * chunk, device=rec.device, dtype=torch.int64)
    for r0 in range(0, R, chunk):
        n = min(chunk, R - r0)
        call("spkb_sweep", ptr(rec), ptr(table[r0:r0 + n]), int(U), n, int(cmax), cd.ctypes.data if P else None, P,
             ad.ctypes.data if Pa else None, ptr(q) if Pa else None, Pa, ptr(out_d[r0:r0 + n]), ptr(out_i[r0:r0 + n]), ptr(ws),
             per * chunk, T, int(upto), stream(), nbytes=2.0 * 8 * T * -(-n // G), flops=2.0 * T * n)
    return out_d, out_i
