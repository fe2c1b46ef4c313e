"""Execution engine: sequences the libspkhip kernels for the forward, backward and inference passes of
NeuralSpeakerModel.  Pure orchestration - every tensor op is a HIP kernel launch from ops.py.

Data flow of one BasicBlock in training (reference scripts/model.py:48-64), NHWC fp32:
    raw1 = conv1(x)            [stats in the conv epilogue]    -> bn1 finalize (mean/invstd/scale/shift)
    raw2 = conv2(relu(bn1(raw1)))   bn1+relu fused into conv2's input staging, never materialised
    out  = relu(bn2(raw2) + shortcut)                          one fused elementwise pass
so each block costs 7 tensor passes over HBM instead of 11.  Saved for backward: x, raw1, raw2, out (+ the
downsample's raw output).  Backward recomputes relu(bn1(raw1)) on the fly inside wgrad's input staging.

SEBasicBlock (arch "se_resnet34", scripts/model.py:67-97): the last line becomes
    sums = squeeze(raw2); q, u, g = excite(sums, bn2, W1, W2); out = relu(g * bn2(raw2) + shortcut)
- one more read of raw2.  Backward: e = dout*[out > 0] is the shortcut gradient, bn2 sees dz = g*e + dq/HW; one pass reduces
(sum e, sum e*raw2) per utterance, the gate kernels turn those [B][C] tables into dW1, dW2, dq and bn2's backward statistics,
one pass writes draw2 (csrc/se.hip).  The data-gradient fusions that assume dz = d*[out > 0] are off around that BatchNorm.

Block backward (Engine._block_bwd), the rules every block follows.  A block has at least two convolutions.  A saved training
forward always writes the sign words of every block output, so the backward always has rec["mask"] and rec["xmask"].  Gradients
wrt raw conv outputs are f16 pair tensors exactly in the f16x3 backward mode.  The BatchNorm backward of conv_i runs in one of
three forms: fused into conv_i's stride-1 data gradient (up to fuse_apply_max_c output channels), as a stand-alone pass, or -
the last BatchNorm of an SE block, always - on the SE kernels.  The shortcut gradient dz = dout*[out > 0] is stored only in
downsample blocks (the 1x1 branch reads it); an identity-shortcut block never stores it: its first convolution's data gradient
re-forms it from dout and the mask bits.  The stand-alone and SE passes read the mask of the last BatchNorm from the bits; the
fused form reduces it from the block output (MASK_ACT) and stages it from the bits.
"""
import torch

from . import ops
from .hip import MASK_ACT, MASK_BITS, MASK_NONE, MASK_RAW


class _Conv:
    def __init__(self, holder):
        self.h = holder
        self.cin, self.cout, self.k, self.stride = holder.cin, holder.cout, holder.k, holder.stride
        self.wpk = None
        self.wpk_t = None
        self.wpk_h = None       # fp16 fragment images of the half-precision extraction path (ops.h16_pack_conv_weight)

    def repack(self, need_t):
        w = self.h.weight.data
        if self.cin == 1:
            return
        self.wpk = ops.pack_conv_weight(w, False, self.wpk)
        if need_t:
            self.wpk_t = ops.pack_conv_weight(w, True, self.wpk_t)

    def pack_jobs(self, need_t):
        """(weight, packed buffer, transpose) entries for the batched pack; allocates the packed buffers on first use."""
        w = self.h.weight.data
        if self.cin == 1:
            return []
        n = ops.packed_numel(w)
        if self.wpk is None or self.wpk.numel() != n:
            self.wpk = torch.empty(n, device=w.device, dtype=torch.float32)
        jobs = [(w, self.wpk, False)]
        if need_t:
            nt = ops.packed_numel(w, bwd=True)
            if self.wpk_t is None or self.wpk_t.numel() != nt:
                self.wpk_t = torch.empty(nt, device=w.device, dtype=torch.float32)
            jobs.append((w, self.wpk_t, True))
        return jobs


class _BN:
    def __init__(self, holder):
        self.h = holder
        self.c = holder.c
        self.t4 = None      # train: [mean, invstd, scale, shift] of the forward whose backward is pending
        self.s4 = None      # the same rows for a training-mode forward WITHOUT a backward (no-grad / predict in train mode)
        self.e2 = None      # eval:  [scale, shift]

    def finalize(self, partial, count, amax_in=None, est_out=None, keep=True):
        """keep=False: the statistics go to a scratch row set, so that a no-grad training-mode forward between forward_train
        and backward does not overwrite what the pending backward reads (the running statistics still advance, as in the
        reference: any train-mode forward updates them)."""
        name = "t4" if keep else "s4"
        if getattr(self, name) is None:
            setattr(self, name, torch.empty(4, self.c, device=partial.device, dtype=torch.float32))
        t4 = getattr(self, name)
        h = self.h
        ops.bn_finalize(partial, count, h.weight.data, h.bias.data, h.running_mean, h.running_var, h.num_batches_tracked,
                        t4, amax_in=amax_in, est_out=est_out)
        return t4

    def eval_coeffs(self):
        h = self.h
        if self.e2 is None:
            self.e2 = torch.empty(2, self.c, device=h.weight.device, dtype=torch.float32)
        ops.bn_eval_coeffs(h.weight.data, h.bias.data, h.running_mean, h.running_var, self.e2)
        return self.e2


class _Block:
    def __init__(self, bp):
        self.kind = bp.kind
        self.convs = [_Conv(bp.conv1), _Conv(bp.conv2)] + ([_Conv(bp.conv3)] if bp.kind == "bottleneck" else [])
        self.bns = [_BN(bp.bn1), _BN(bp.bn2)] + ([_BN(bp.bn3)] if bp.kind == "bottleneck" else [])
        assert len(self.convs) >= 2      # Engine._block_bwd: the first conv re-forms the shortcut gradient the last one left out
        self.ds = None
        if bp.downsample is not None:
            self.ds = (_Conv(bp.downsample[0]), _BN(bp.downsample[1]))
        # SEBasicBlock: the gate's parameter holder (w1 = se.fc.0.weight [C/16][C], w2 = se.fc.2.weight [C][C/16]).  The block's
        # tail is then squeeze -> excite -> apply instead of bn_apply, and its last BatchNorm backward runs on the se_bwd kernels
        self.se = bp.se if bp.kind == "se_basic" else None


class _LogitsFn(torch.autograd.Function):
    """Bridges torch autograd to the hand-written backward: one node for the whole network.  Parameter
    gradients are written straight into the flat gradient arena (the .grad views); `anchor` only makes the
    output require grad."""

    @staticmethod
    def forward(ctx, eng, x, y, anchor):
        logits, saved = eng.forward_train(x, y)
        ctx.eng = eng
        ctx.saved = saved
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        ctx.eng.backward(ctx.saved, dlogits.contiguous())
        ctx.saved = None
        return None, None, None, None


class Engine:
    def __init__(self, model):
        self.m = model
        r = model.res
        self.stem_conv = _Conv(r.conv1)
        self.stem_bn = _BN(r.bn1)
        self.blocks = []
        self.stage_of = []             # ResNet stage (1..4) of every block
        for li in range(1, 5):
            for bp in getattr(r, "layer%d" % li):
                self.blocks.append(_Block(bp))
                self.stage_of.append(li)
        self.head_bn = _BN(model.bn1) if hasattr(model, "bn1") else None
        self.pool_mode = 1 if model.pooling == "mean+std" else 0
        self._half_dirty = True        # the fp16 weight packs of the half-precision extraction path lag the weights
        self.half_overflow = None      # int32 [B] device tensor of the last half predict: stored values that left fp16's range
        self.windows_skipped = None    # numpy int64: the utterances the last predict_windows found shorter than min_window
        self.dirty = True
        self._packed_for_bwd = False
        self._pack_tables = {}
        self._amax_pool = None
        self._amax_fwd = None          # slots of the TRAINING forward: they live on in the saved records until its backward
        self._amax_eval = None         # slots of eval-mode / no-grad forwards (never referenced by a backward)
        self._fwd_gen = 0              # generation of the training table: a backward refuses records of an older forward
        # weight gradients (compute-bound, off the critical path) run on a side stream so that they overlap the
        # HBM-bound BatchNorm-backward passes of the main dgrad chain
        self.wgrad_stream = None
        self.use_side_stream = True
        # BatchNorm-backward reductions come out of the producing data-gradient epilogue (EPI_BNBWD) where possible, and the
        # BatchNorm-backward apply runs inside the stride-1 data gradients' input staging (IN_BNBWD) - up to fuse_apply_max_c
        # output channels.  f16x3 default: the fusion only on the 32-channel layer, which is HBM-bound (the fusion saves one tensor
        # read there); from 64 channels on the BatchNorm backward runs as its own pass that writes the gradient ONCE as an f16
        # pair tensor, and the data gradient (in-wave pipelined kernel) and the weight gradient stage it by plain copy
        # (None = by operand mode: 32 in the f16x3 mode with pair tensors, no limit otherwise; SPK_FUSE_APPLY_MAXC overrides)
        import os
        self._fuse_apply_max_c = int(os.environ["SPK_FUSE_APPLY_MAXC"]) if "SPK_FUSE_APPLY_MAXC" in os.environ else None
        # the stem without two tensor passes (csrc/stem.hip): forward = statistics with no store, then one writer of raw0, a and
        # the sign bits that recomputes the convolution; backward = the BatchNorm-backward apply inside the weight gradient.
        # 0 gives the two-kernel paths back (A/B, identity tests); "fwd" / "bwd" switch one half on (per-part A/B)
        stem_fused = os.environ.get("SPK_STEM_FUSED", "1")
        self.stem_fused_fwd = stem_fused in ("1", "fwd")
        self.stem_fused_bwd = stem_fused in ("1", "bwd")
        # The blocks of the LAST stage sit between the pooling layer and the first BatchNorm backward + convolution that bound the
        # gradient's range again: sqrt'(mean) of scripts/model.py:453 is unbounded (1e8 x the rest for a row mean of 1e-20) and
        # travels down the identity shortcuts as dout.  There the BatchNorm-backward scale bound pairs every channel's own absmax
        # of dz with its own gamma*invstd (spk_bn_bwd_reduce chan_amax) - a tensor-wide absmax times the layer's largest |k1|
        # overshoots the values by the ratio of the two and pushes the whole pair tensor out of its fp16 window.  Costs the
        # stand-alone reduction pass for two more 100 MB tensors per step (their statistics no longer come from an epilogue).
        self.chan_amax = os.environ.get("SPK_CHAN_AMAX", "1") == "1"
        # diagnostics (tests / bench, never the timed path): when a [4] int64 device tensor, every tensor that an f16x3
        # matrix-core kernel stages is also run through spk_f16_window_count under the scale slot its consumer uses
        self.window_counts = None
        self.bound_log = None          # diagnostics: when a list, (Cout, k, bound slot, true-absmax slot) of every BatchNorm-backward scale

    # ---- helpers ---------------------------------------------------------------------------------------
    @property
    def dirty(self):
        """the weights changed since the fp32 packs were built (SGD step, load_state_dict, loadParameters, .cuda())"""
        return self._dirty

    @dirty.setter
    def dirty(self, v):
        self._dirty = v
        if v:
            self._half_dirty = True    # cleared only by _repack_half: the two pack sets are rebuilt independently

    @property
    def fuse_apply_max_c(self):
        if self._fuse_apply_max_c is not None:
            return self._fuse_apply_max_c
        return 32 if ops.split_for(3, True) == 3 else 1000000

    @fuse_apply_max_c.setter
    def fuse_apply_max_c(self, v):
        self._fuse_apply_max_c = v

    def _all_convs(self):
        for b in self.blocks:
            for c in b.convs:
                yield c
            if b.ds is not None:
                yield b.ds[0]

    def _repack(self, need_t):
        if not self.dirty and (self._packed_for_bwd or not need_t):
            return
        # one launch packs every convolution (forward order, plus the transposed order the backward needs); the job
        # table lives on the device and is rebuilt only when a buffer, the operand mode or need_t changes
        jobs = [j for c in self._all_convs() for j in c.pack_jobs(need_t)]
        key = [(w.data_ptr(), p.data_ptr(), t, ops.split_for(w.shape[2], t)) for w, p, t in jobs]
        tab = self._pack_tables.get(need_t)
        if tab is None or tab.key != key:
            assert not torch.cuda.is_current_stream_capturing() or tab is None, "pack table changed during graph capture"
            tab = self._pack_tables[need_t] = ops.PackTable(jobs, jobs[0][0].device)
        tab.run()
        self.dirty = False
        self._packed_for_bwd = need_t

    def _check_input(self, x):
        if not x.is_cuda:
            raise RuntimeError("pytorch_kaldi_resnet_amd runs on MI355X only: input must be a device tensor "
                               "(there is no CPU fallback)")
        if x.dim() != 3 or x.size(1) != self.m.feat_dim:
            raise RuntimeError("expected input [B, %d, T], got %s" % (self.m.feat_dim, tuple(x.shape)))
        if x.dtype != torch.float32:
            raise RuntimeError("expected float32 input")
        return x.contiguous()

    # ---- inference trunk (eval-mode BN folded into conv epilogues) -----------------------------------------
    def _fwd_pool(self, device, train=False):
        """absmax slot table of a forward pass (f16x3 operand mode), reset at its start.  The training forward has a table of
        its own: its slots (convolution inputs, raw conv outputs) live on in the saved records for the backward pass, so an
        eval-mode or no-grad forward between forward_train and backward must not touch them (it takes the other table), and
        a SECOND training forward before the backward invalidates the records (generation check in Engine.backward)."""
        if ops.split_for(3) != 3 and ops.split_for(3, True) != 3:
            return None
        name = "_amax_fwd" if train else "_amax_eval"
        if getattr(self, name) is None:
            setattr(self, name, ops.AmaxPool(device))
        pool = getattr(self, name)
        pool.reset()
        return pool

    def _count(self, x, slot, affine=None, pairs=False):
        if self.window_counts is not None and slot is not None:
            ops.f16_window_count(x, slot, self.window_counts, affine=affine, pairs=pairs)

    def trunk_eval(self, x, wl=None):
        """wl: None, or int32 device [4][B] valid widths per stage (stage_widths): the length-masked forward of a padded batch.
        Every convolution whose output another convolution or the pooling reads is masked to its stage width (the stem, and each
        block's convolutions - the last one after the residual add); the downsample branch is not: its output only meets the
        residual add, which the block's last convolution masks."""
        self._repack(False)
        pool = self._fwd_pool(x.device)
        take = (lambda: pool.take()) if pool is not None else (lambda: None)
        e = self.stem_bn.eval_coeffs()
        a_amax = take()
        a, _ = ops.stem_fwd(x, self.stem_conv.h.weight.data, epi_affine=(e[0], e[1]), relu=True, amax_out=a_amax,
                            wlen=None if wl is None else wl[0])
        stage = 0               # log2 of the trunk's stride so far: row of wl
        for b in self.blocks:
            evs = [bn.eval_coeffs() for bn in b.bns]
            if b.ds is not None:
                ed = b.ds[1].eval_coeffs()
                res, _ = ops.conv_fwd(a, b.ds[0].wpk, b.ds[0].cout, 1, b.ds[0].stride, epi_affine=(ed[0], ed[1]),
                                      in_amax=a_amax if ops.split_for(1) == 3 else None)
            else:
                res = a
            h, h_amax = a, a_amax
            n = len(b.convs)
            for i, (c, ev) in enumerate(zip(b.convs, evs)):
                last = i == n - 1
                o_amax = take()
                if c.stride == 2:
                    stage += 1
                if last and b.se is not None:
                    # z = bn2(conv2(.)) without ReLU or add, then the gate from its per-utterance channel means (over the valid
                    # columns only) and out = relu(g z + shortcut), masked to the stage width here
                    wls = None if wl is None else wl[stage]
                    z, _ = ops.conv_fwd(h, c.wpk, c.cout, c.k, c.stride, epi_affine=(ev[0], ev[1]),
                                        in_amax=h_amax if ops.split_for(c.k) == 3 else None)
                    _, gate = self._se_gate(b, z, None, wls)
                    h = ops.se_apply(z, None, gate, res=res, relu=True, amax_out=o_amax, wlen=wls)
                    h_amax = o_amax
                    continue
                h, _ = ops.conv_fwd(h, c.wpk, c.cout, c.k, c.stride, epi_affine=(ev[0], ev[1]),
                                    epi_add=res if last else None, relu=True,
                                    in_amax=h_amax if ops.split_for(c.k) == 3 else None, out_amax=o_amax,
                                    wlen=None if wl is None else wl[stage])
                h_amax = o_amax
            a, a_amax = h, h_amax
        return a

    @staticmethod
    def _se_gate(b, t, affine, wlen=None):
        """squeeze + excite of an SE block on the tensor t (raw conv output with `affine` = its BatchNorm rows, or z itself)
        -> ((sums, q, u, g) as the backward needs them, g)"""
        sums = ops.se_squeeze(t, wlen)
        q, u, g = ops.se_excite(sums, affine, b.se.w1.data, b.se.w2.data, t.shape[1], t.shape[2], wlen)
        return (sums, q, u, g), g

    def embed_eval(self, x, wl=None):
        feat = self.trunk_eval(x, wl)
        pooled = ops.stats_pool_fwd(feat, self.pool_mode, wlen=None if wl is None else wl[3])
        return ops.linear_fwd(pooled, self.m.fc1.weight.data, self.m.fc1.bias.data)

    # ---- half-precision extraction (precision="f16") ---------------------------------------------
    def _repack_half(self):
        if self.m.arch == "se_resnet34":
            raise NotImplementedError("precision='f16' does not support arch se_resnet34 yet (squeeze-and-excitation blocks in half "
                                      "precision are a follow-up): use precision='f32'")
        if not self._half_dirty:
            return
        for c in self._all_convs():
            c.wpk_h = ops.h16_pack_conv_weight(c.h.weight.data, c.wpk_h)
        self._half_dirty = False

    def trunk_eval_half(self, x, wl=None):
        """trunk_eval on fp16 activations with one fp16 product per multiply-accumulate: the stem in fp32 arithmetic stored as
        fp16, every convolution with its eval BatchNorm (fp32 scale / shift rows), residual, ReLU and length mask in an fp32
        epilogue rounded once.  The masking rule is trunk_eval's.  Resets and fills self.half_overflow."""
        self._repack_half()
        ovf = self.half_overflow = torch.zeros(x.shape[0], device=x.device, dtype=torch.int32)
        e = self.stem_bn.eval_coeffs()
        a = ops.h16_stem_fwd(x, self.stem_conv.h.weight.data, e[0], e[1], ovf, wlen=None if wl is None else wl[0])
        stage = 0
        for b in self.blocks:
            evs = [bn.eval_coeffs() for bn in b.bns]
            if b.ds is not None:
                cd, ed = b.ds[0], b.ds[1].eval_coeffs()
                res = ops.h16_conv_fwd(a, cd.wpk_h, cd.cout, 1, cd.stride, ed[0], ed[1], ovf, relu=False)
            else:
                res = a
            h, n = a, len(b.convs)
            for i, (c, ev) in enumerate(zip(b.convs, evs)):
                if c.stride == 2:
                    stage += 1
                h = ops.h16_conv_fwd(h, c.wpk_h, c.cout, c.k, c.stride, ev[0], ev[1], ovf, add=res if i == n - 1 else None,
                                     relu=True, wlen=None if wl is None else wl[stage])
            a = h
        return a

    def embed_eval_half(self, x, wl=None):
        feat = self.trunk_eval_half(x, wl)
        pooled = ops.h16_stats_pool_fwd(feat, self.pool_mode, wlen=None if wl is None else wl[3])
        return ops.linear_fwd(pooled, self.m.fc1.weight.data, self.m.fc1.bias.data)

    @staticmethod
    def stage_widths(lengths, B, T, device):
        """Validated per-utterance lengths -> int32 [4][B] on `device`: the valid widths of the stem and layer 1 (L), then of the
        three stride-2 stages, W' = ceil(W / 2) each (the output width of a 3x3 pad-1 and of a 1x1 convolution at stride 2), so the
        pooled width is ceil(L / 8).  `lengths`: a sequence of ints or an integer tensor on any device, 1 <= L[b] <= T."""
        if isinstance(lengths, torch.Tensor):
            if lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool:
                raise TypeError("lengths must be integers, got a %s tensor" % lengths.dtype)
            L = lengths.detach().to("cpu", torch.int64).reshape(-1)
            if lengths.dim() != 1:
                raise ValueError("lengths must be one-dimensional [B], got shape %s" % (tuple(lengths.shape),))
        else:
            vals = list(lengths)
            if not all(isinstance(v, int) or (hasattr(v, "__index__") and not isinstance(v, (bool, float))) for v in vals) \
                    or any(isinstance(v, bool) for v in vals):
                raise TypeError("lengths must be integers")
            L = torch.tensor([int(v) for v in vals], dtype=torch.int64)
        if L.numel() != B:
            raise ValueError("lengths has %d entries for a batch of %d utterances" % (L.numel(), B))
        if B and (int(L.min()) < 1 or int(L.max()) > T):
            raise ValueError("lengths must lie in [1, T=%d], got min %d max %d" % (T, int(L.min()), int(L.max())))
        w = [L]
        for _ in range(3):
            w.append((w[-1] + 1) // 2)
        return torch.stack(w).to(torch.int32).to(device)

    def predict(self, x, lengths=None, precision="f32"):
        """scripts/model.py:402-409.  Uses BN batch statistics when the module is in train mode, exactly like
        the reference would; decode.py always calls it under model.eval().
        lengths (eval mode only): per-utterance frame counts of a padded batch x [B, F, T] - row b is the embedding of
        x[b, :, :lengths[b]] alone, whatever the padding holds (length-masked stem, convolutions and pooling).
        precision: "f32" (the project's fp32 contract) or, eval mode only, "f16": fp16 activations and one fp16 product per
        multiply-accumulate (embed_eval_half).  A row whose activations left fp16's range has self.half_overflow[b] > 0 and
        its embedding is not to be used: predict such rows again with precision="f32"."""
        if precision not in ("f32", "f16"):
            raise ValueError("precision must be 'f32' or 'f16', got %r" % (precision,))
        x = self._check_input(x)
        with torch.no_grad():
            if precision == "f16":
                if self.m.training:
                    raise RuntimeError("predict(precision='f16') needs eval mode: the half-precision path applies the running "
                                       "BatchNorm statistics (call model.eval() first)")
                wl = None if lengths is None else self.stage_widths(lengths, x.shape[0], x.shape[2], x.device)
                return self.embed_eval_half(x, wl)
            if lengths is not None:
                if self.m.training:
                    raise RuntimeError("predict(lengths=...) needs eval mode: with BatchNorm batch statistics a padded batch has "
                                       "no per-utterance meaning (call model.eval() first)")
                return self.embed_eval(x, self.stage_widths(lengths, x.shape[0], x.shape[2], x.device))
            if self.m.training:
                emb, _ = self._embed_train(x, save=False)
                return emb
            return self.embed_eval(x)

    def predict_windows(self, x, lengths, window, period, min_window=None, average=False, precision="f32", batch_size=None,
                        segments=None):
        """Windowed extraction, eval mode only.  x [B, F, T]: a padded batch, lengths: per-utterance frame
        counts (0 <= L[b] <= T; None: T frames each).  The windows of ingest.plan_windows(lengths, window, period, min_window)
        (min_window None: 1) are gathered into padded batches of at most batch_size rows (default B; ingest.window_batches,
        spk_window_gather) and each runs through predict(xw, lengths=lw, precision=precision): a row is the embedding of its
        window run alone.
        -> (emb [N, D], utt [N], start [N], length [N]) in plan order (the last three numpy int64), or with average=True
        (emb [U', D], utt [U']): per utterance that has a window, the mean of its window embeddings weighted by window length
        (spk_window_mean).  self.windows_skipped: the utterances shorter than min_window.  After a precision="f16" call
        self.half_overflow holds the count of every WINDOW, in plan order (also with average=True).
        segments: a tuple (seg_utt, seg_start, seg_end) of speech segments, frames [seg_start[j], seg_end[j])
        of utterance seg_utt[j], sorted by utterance and disjoint within one, none ending beyond lengths[seg_utt[j]].  The plan is
        then ingest.plan_segment_windows: the window rule inside every segment.  `start` stays in utterance frames,
        self.windows_skipped lists the SEGMENTS shorter than min_window, average=True averages all windows of an utterance (a
        speech-only chunk average), and an utterance without a segment yields no row."""
        import numpy as np
        from . import ingest
        if precision not in ("f32", "f16"):
            raise ValueError("precision must be 'f32' or 'f16', got %r" % (precision,))
        if self.m.training:
            raise RuntimeError("predict_windows(...) needs eval mode: with BatchNorm batch statistics a batch of windows has no "
                               "per-window meaning (call model.eval() first)")
        x = self._check_input(x)
        B, _, T = x.shape
        if lengths is None:
            L = np.full(B, T, dtype=np.int64)
        else:
            if isinstance(lengths, torch.Tensor):
                if lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool:
                    raise TypeError("lengths must be integers, got a %s tensor" % lengths.dtype)
                lengths = lengths.detach().cpu().numpy()
            L = np.asarray(lengths)
            if L.dtype.kind not in "iu":
                raise TypeError("lengths must be integers")
            L = L.astype(np.int64)
            if L.shape != (B,):
                raise ValueError("lengths has shape %s for a batch of %d utterances" % (L.shape, B))
            if B and (int(L.min()) < 0 or int(L.max()) > T):
                raise ValueError("lengths must lie in [0, T=%d], got min %d max %d" % (T, int(L.min()), int(L.max())))
        if segments is None:
            plan = ingest.plan_windows(L, window, period, 1 if min_window is None else min_window)
        else:
            su, ss, se = (np.asarray(v, dtype=np.int64).reshape(-1) for v in segments)
            if su.size and (int(su.min()) < 0 or int(su.max()) >= B):
                raise ValueError("segments name utterance %d of a batch of %d" % (int(su.min()) if int(su.min()) < 0 else int(su.max()), B))
            if su.size == se.size and (se > L[su]).any():
                j = int(np.nonzero(se > L[su])[0][0])
                raise ValueError("segment %d ends at frame %d, beyond the %d frames of utterance %d" % (j, se[j], L[su[j]], su[j]))
            plan = ingest.plan_segment_windows(su, ss, se, window, period, 1 if min_window is None else min_window)
        self.windows_skipped = plan.skipped
        N = plan.utt.size
        D = self.m.fc1.weight.shape[0]
        half = precision == "f16"
        if half:
            self._repack_half()           # the refusals of the half path, also when there is no window to run
        if N == 0:
            self.half_overflow = torch.zeros(0, device=x.device, dtype=torch.int32) if half else self.half_overflow
            emb = torch.empty(0, D, device=x.device, dtype=torch.float32)
            return (emb, plan.utt) if average else (emb, plan.utt, plan.start, plan.length)
        batches = ingest.window_batches(plan.length, B if batch_size is None else int(batch_size))
        embs, ovfs = [], []
        with torch.no_grad():
            for idx, wcap in batches:
                xw = ops.window_gather(x, plan.utt[idx], plan.start[idx], plan.length[idx], wcap)
                embs.append(self.predict(xw, lengths=plan.length[idx].tolist(), precision=precision))
                if half:
                    ovfs.append(self.half_overflow)
            # back to plan order with the gather itself: row i of the result is row inv[i] of the concatenation, whole
            order = np.concatenate([idx for idx, _ in batches])
            inv = np.empty(N, dtype=np.int64)
            inv[order] = np.arange(N)
            zeros = np.zeros(N, dtype=np.int64)
            emb = ops.window_gather(torch.cat(embs).view(N, 1, D), inv, zeros, np.full(N, D, dtype=np.int64), D).view(N, D)
            if half:       # the counts travel as their bit patterns: the gather only moves words
                cnt = torch.cat(ovfs).view(torch.float32).view(N, 1, 1)
                self.half_overflow = ops.window_gather(cnt, inv, zeros, np.ones(N, dtype=np.int64), 1).view(N).view(torch.int32)
            if not average:
                return emb, plan.utt, plan.start, plan.length
            utts, first = np.unique(plan.utt, return_index=True)        # plan.utt ascends: the windows of an utterance are adjacent
            return ops.window_mean(emb, np.append(first, N), plan.length.astype(np.float32)), utts

    # ---- heads ----------------------------------------------------------------------------------------------
    def _head_fwd(self, emb, y, train, save):
        m = self.m
        sv = {}
        h = emb
        if m.loss in ("softmax", "AAM-v1"):
            bn = self.head_bn
            if train:
                part = ops.bn_stats_partial(emb)
                t4 = bn.finalize(part, emb.shape[0], keep=save)
                h = ops.bn_apply(emb, t4[2], t4[3], relu=True)
            else:
                e2 = bn.eval_coeffs()
                h = ops.bn_apply(emb, e2[0], e2[1], relu=True)
            sv["h"] = h
        if m.loss == "softmax":
            logits = ops.linear_fwd(h, m.last.weight.data, m.last.bias.data)
        else:
            if y is None:
                raise RuntimeError("AAM heads need labels (scripts/model.py:483: label=None fails in the reference too)")
            y = y.contiguous()
            hn, hinv = ops.l2norm_fwd(h)
            wn, winv = ops.l2norm_fwd(m.last.weight.data)
            B, S, D = h.shape[0], wn.shape[0], wn.shape[1]
            cosv = ops.gemm(hn, wn, B, S, D, D, 1, 1, D)
            logits = ops.aam_margin_fwd(cosv, y, m.m, m.s)
            if save:
                sv.update(hn=hn, hinv=hinv, wn=wn, winv=winv, cosv=cosv, y=y)
        return logits, sv

    def _head_bwd(self, emb, sv, dlogits, acc):
        m = self.m
        if m.loss == "softmax":
            dh = ops.linear_bwd(sv["h"], m.last.weight.data, dlogits, m.last.weight.grad, m.last.bias.grad, accumulate=acc)
        else:
            dcos = ops.aam_margin_bwd(sv["cosv"], sv["y"], dlogits, m.m, m.s)
            B, S = dcos.shape
            D = sv["wn"].shape[1]
            dhn = ops.gemm(dcos, sv["wn"], B, D, S, S, 1, D, 1)
            dwn = ops.gemm(dcos, sv["hn"], S, D, B, 1, S, D, 1)
            dh = ops.l2norm_bwd(sv["hn"], sv["hinv"], dhn)
            ops.l2norm_bwd(sv["wn"], sv["winv"], dwn, out=m.last.weight.grad, accumulate=acc)
        if m.loss in ("softmax", "AAM-v1"):
            bn = self.head_bn
            dh = ops.bn_backward(dh, emb, sv["h"], bn.t4, bn.h.weight.data, bn.h.weight.grad, bn.h.bias.grad, MASK_ACT,
                                 accumulate=acc)
        return dh

    # ---- training forward -----------------------------------------------------------------------------------
    def _trunk_train(self, x, save):
        saved = {"x": x, "blocks": []}
        pool = self._fwd_pool(x.device, train=save)
        if save:
            self._fwd_gen += 1                 # this forward now owns the per-engine records (BN statistics rows, scale slots)
        saved["gen"] = self._fwd_gen
        take = (lambda: pool.take()) if pool is not None else (lambda: None)
        B, F, T = x.shape
        w0 = self.stem_conv.h.weight.data
        if self.stem_fused_fwd:
            t4 = self.stem_bn.finalize(ops.stem_stats(x, w0), B * F * T, keep=save)
            a_amax = take()
            raw0, a, amask = ops.stem_fwd_apply(x, w0, t4[2], t4[3], mask=save, amax_out=a_amax)
        else:
            raw0, st = ops.stem_fwd(x, w0, stats=True)
            t4 = self.stem_bn.finalize(st, B * F * T, keep=save)
            a_amax = take()
            a = ops.bn_apply(raw0, t4[2], t4[3], relu=True, mask=save, amax_out=a_amax)
            a, amask = a if save else (a, None)
        saved["raw0"] = raw0
        for b in self.blocks:
            # in_amax[i]: slot with the absmax (or its upper estimate) of the values conv_i STAGES - the block input itself,
            # or relu(bn(raw_{i-1})) recomputed in the staging - shared by the forward conv and its weight gradient
            rec = {"x": a, "xmask": amask, "in_amax": [], "raw_amax": []}
            raws = []
            h, aff, h_amax = a, None, a_amax           # h_amax: slot describing the values the next conv stages from h
            for c, bn in zip(b.convs, b.bns):
                rec["in_amax"].append(h_amax)
                raw_amax = take()
                rec["raw_amax"].append(raw_amax)       # absmax(raw): bounds |xhat| in the BatchNorm backward's operand scale
                if ops.split_for(c.k) == 3:
                    self._count(h, h_amax, affine=aff)
                raw, st = ops.conv_fwd(h, c.wpk, c.cout, c.k, c.stride, in_affine=aff, stats=True,
                                       in_amax=h_amax if ops.split_for(c.k) == 3 else None, out_amax=raw_amax)
                # the next conv stages relu(bn(raw)): its operand-scale bound comes out of the BatchNorm finalize
                est = take()
                t4 = bn.finalize(st, raw.shape[0] * raw.shape[1] * raw.shape[2], amax_in=raw_amax, est_out=est, keep=save)
                raws.append(raw)
                h, aff, h_amax = raw, (t4[2], t4[3]), est
            out_amax = take()
            if b.se is not None:
                rec["se"], gate = self._se_gate(b, h, aff)
            res, res_affine = a, None
            if b.ds is not None:
                rawd, st = ops.conv_fwd(a, b.ds[0].wpk, b.ds[0].cout, 1, b.ds[0].stride, stats=True,
                                        in_amax=a_amax if ops.split_for(1) == 3 else None)
                td = b.ds[1].finalize(st, rawd.shape[0] * rawd.shape[1] * rawd.shape[2], keep=save)
                res, res_affine = rawd, (td[2], td[3])
                rec["rawd"] = rawd
            # a saved forward also writes the 1-bit sign words of the block output: the backward kernels read those instead of
            # the activated tensor wherever they only need [out > 0]
            if b.se is not None:
                out = ops.se_apply(h, aff, gate, res=res, res_affine=res_affine, relu=True, mask=save, amax_out=out_amax)
            else:
                out = ops.bn_apply(h, aff[0], aff[1], res=res, res_affine=res_affine, relu=True, mask=save, amax_out=out_amax)
            out, amask = out if save else (out, None)
            rec["raws"] = raws
            rec["out"] = out
            rec["mask"] = amask
            if save:
                saved["blocks"].append(rec)
            a, a_amax = out, out_amax
            res = None                  # (a forward that saves nothing frees the block input here, not a block later)
        return a, saved

    def _embed_train(self, x, save):
        self._repack(save)
        feat, saved = self._trunk_train(x, save)
        pooled = ops.stats_pool_fwd(feat, self.pool_mode)
        emb = ops.linear_fwd(pooled, self.m.fc1.weight.data, self.m.fc1.bias.data)
        saved["feat"], saved["pooled"], saved["emb"] = feat, pooled, emb
        return emb, saved

    def forward_train(self, x, y):
        emb, saved = self._embed_train(x, True)
        logits, sv = self._head_fwd(emb, y, True, True)
        saved["head"] = sv
        return logits, saved

    def forward_logits(self, x, y=None):
        x = self._check_input(x)
        m = self.m
        if m.training and torch.is_grad_enabled():
            anchor = m.fc1.bias
            return _LogitsFn.apply(self, x, y, anchor)
        with torch.no_grad():
            if m.training:
                emb, _ = self._embed_train(x, save=False)
                logits, _ = self._head_fwd(emb, y, True, False)
            else:
                emb = self.embed_eval(x)
                logits, _ = self._head_fwd(emb, y, False, False)
            return logits

    # ---- side-stream weight gradients ----------------------------------------------------------------------------
    def _wgrad(self, x, dy, dw, k, stride, in_affine=None, accumulate=False, dy_amax=None, x_amax=None, dy_presplit=False):
        if not self.use_side_stream:
            return ops.conv_wgrad(x, dy, dw, k, stride, in_affine=in_affine, accumulate=accumulate, dy_amax=dy_amax,
                                  x_amax=x_amax, dy_presplit=dy_presplit)
        if self.wgrad_stream is None:
            self.wgrad_stream = torch.cuda.Stream()
        main = torch.cuda.current_stream()
        side = self.wgrad_stream
        side.wait_stream(main)                      # dy / x are produced on the main stream
        # keep the allocator from recycling them under the side kernel - ALSO inside a graph capture: a block freed during the
        # capture goes back to the graph's private pool and is handed to the next allocation on the main branch, while the side
        # branch may replay later (measured: SPK_GRAPH_SIDE=1 without this gave a different loss on every run)
        for t in (x, dy):
            t.record_stream(side)
        with torch.cuda.stream(side):
            ops.conv_wgrad(x, dy, dw, k, stride, in_affine=in_affine, accumulate=accumulate, dy_amax=dy_amax, x_amax=x_amax,
                           dy_presplit=dy_presplit)

    def _join_wgrad(self):
        if self.use_side_stream and self.wgrad_stream is not None:
            torch.cuda.current_stream().wait_stream(self.wgrad_stream)

    # ---- backward ---------------------------------------------------------------------------------------------
    def backward(self, saved, dlogits, on_stage_done=None):
        """Hand-written backward of forward_train.  Parameter gradients go to the .grad arena views (overwritten
        when the views are fresh, accumulated otherwise).  on_stage_done(name) is called after the last weight
        gradient of each ResNet stage has been enqueued (hook for overlapping the gradient all-reduce)."""
        m = self.m
        acc = not m.attach_grads()
        if saved.get("gen") != self._fwd_gen:
            raise RuntimeError("backward of a training forward whose BatchNorm statistics rows and operand-scale slots were reused "
                               "by a later training forward (the engine keeps one set per model: run backward before the next "
                               "forward that requires grad)")
        with torch.no_grad():
            demb = self._head_bwd(saved["emb"], saved["head"], dlogits, acc)
            dpooled = ops.linear_bwd(saved["pooled"], m.fc1.weight.data, demb, m.fc1.weight.grad, m.fc1.bias.grad,
                                     accumulate=acc)
            # f16x3 operand mode of the backward kernels: every gradient tensor that feeds a matrix-core stage travels with
            # a slot holding the float bits of its absmax (atomicMax'ed by the kernel that writes it); the consumer derives
            # its power-of-two operand scale from it.  Slots are taken in a fixed order from a table zeroed once per step.
            amx = None
            if ops.split_for(3, True) == 3:
                if self._amax_pool is None:
                    self._amax_pool = ops.AmaxPool(dpooled.device)
                amx = self._amax_pool
                amx.reset()
            d_amax = amx.take() if amx else None
            d = ops.stats_pool_bwd(saved["feat"], dpooled, self.pool_mode, amax_out=d_amax)
            if on_stage_done:
                on_stage_done("head")
            stage_of = self.stage_of
            part = None      # BatchNorm-backward partial sums of `d`, when the producing dgrad epilogue made them
            for bi in range(len(self.blocks) - 1, -1, -1):
                chan = self.chan_amax and amx is not None and stage_of[bi] == stage_of[-1]
                prev = self._bn_below(saved, bi, chan)
                d, part, d_amax = self._block_bwd(self.blocks[bi], saved["blocks"][bi], d, acc, part, prev, d_amax, amx, chan)
                saved["blocks"][bi] = None
                if on_stage_done and (bi == 0 or stage_of[bi - 1] != stage_of[bi]):
                    self._join_wgrad()
                    on_stage_done("layer%d" % stage_of[bi])
            # stem: d is the gradient wrt relu(bn(raw0))
            bn = self.stem_bn
            if self.stem_fused_bwd:
                raw0 = saved["raw0"]
                if part is None:
                    part = ops.bn_bwd_partial(d, raw0, None, bn.t4, MASK_RAW)
                coef = ops.bn_bwd_coef(part, raw0.numel() // raw0.shape[-1], bn.h.weight.data, bn.t4, bn.h.weight.grad,
                                       bn.h.bias.grad, accumulate=acc)
                ops.stem_bwd_wgrad(saved["x"], d, raw0, bn.t4, coef, self.stem_conv.h.weight.grad, accumulate=acc)
            else:
                draw0 = ops.bn_backward(d, saved["raw0"], None, bn.t4, bn.h.weight.data, bn.h.weight.grad, bn.h.bias.grad,
                                        MASK_RAW, draw_out=d, accumulate=acc, partial=part)
                ops.stem_wgrad(saved["x"], draw0, self.stem_conv.h.weight.grad, accumulate=acc)
            self._join_wgrad()
            if on_stage_done:
                on_stage_done("stem")

    def _bn_below(self, saved, bi, chan):
        """The gradient block `bi` hands down is the gradient wrt the BN+ReLU output below it - the last BatchNorm of the previous
        block, or the stem's.  -> (raw, t4) of that BatchNorm when the block's last data gradient may reduce its backward
        statistics in its epilogue (EPI_BNBWD), None when they have to come from a pass of their own.  chan: block `bi` takes
        per-channel absmax rows (Engine.chan_amax: the f16x3 backward, last stage)."""
        if bi == 0:
            return saved["raw0"], self.stem_bn.t4
        below = self.blocks[bi - 1]
        if below.se is not None:
            # below an SE block the gradient wrt that BatchNorm's output is g e + dq / HW, not d [out > 0]: the epilogue
            # reduction does not apply - its statistics come from the block's own tables (se_bwd_gate)
            return None
        if chan and self.stage_of[bi - 1] == self.stage_of[bi]:
            return None                    # that BatchNorm's statistics come from its own reduction pass, with per-channel absmax
        return saved["blocks"][bi - 1]["raws"][-1], below.bns[-1].t4

    def _block_bwd(self, b, rec, dout, acc, dout_partial=None, prev=None, dout_amax=None, amx=None, chan=False):
        """Backward of one residual block.  -> (gradient wrt the block input, BN-backward partial sums of it or None,
        absmax slot of it or None).

        Walks the convs last to first.  `g` is the gradient wrt the OUTPUT of bn_i (+ReLU): dout for the last BN (mask
        = block output > 0), the data gradient of conv_{i+1} for the inner ones (mask recomputed from raw_i).  For a
        stride-1 conv_i of up to fuse_apply_max_c channels the BatchNorm backward of bn_i is applied inside the data-gradient
        kernel's input staging (IN_BNBWD): no separate apply pass; the kernel writes draw_i (for the weight gradient) and, for
        the last BN of a downsample block, dz (the shortcut gradient) as side products.  Stride-2 convs (parity-class launches),
        wider ones and the last BN of an SE block keep a separate pass.
        prev: Engine._bn_below.  amx (f16x3 backward): the step's absmax slot table; g / draw / dx each carry a slot (see
        Engine.backward).  chan: the last BatchNorm's scale bound uses the per-channel absmax of dz (Engine.chan_amax)."""
        assert not chan or dout_partial is None, "the per-channel absmax comes out of the reduction pass"
        x, raws, out = rec["x"], rec["raws"], rec["out"]
        n = len(b.convs)
        g, g_part, g_amax, dz = dout, dout_partial, dout_amax, None
        take = (lambda: amx.take()) if amx is not None else (lambda: None)
        for i in range(n - 1, -1, -1):
            c, bn, raw = b.convs[i], b.bns[i], raws[i]
            last = i == n - 1
            inp = x if i == 0 else raws[i - 1]
            in_aff = None if i == 0 else (b.bns[i - 1].t4[2], b.bns[i - 1].t4[3])
            hw = (inp.shape[1], inp.shape[2])
            # data / weight gradients with fp16 two-term operands.  Then the gradient wrt the raw conv output (draw) travels as an
            # f16 PAIR tensor - written once in the two-term form under a rigorous bound known before it is computed, staged by
            # plain copy in its data and weight gradients - and amx16 hands out the slot of that bound
            f16 = amx is not None and ops.split_for(c.k, True) == 3
            amx16 = amx if f16 else None
            raw_amax = rec["raw_amax"][i] if f16 else None
            # which form bn_i's backward takes.  An SE block's last BatchNorm is never fused: IN_BNBWD assumes dz = g [out > 0]
            se = last and b.se is not None
            fused = not se and c.stride == 1 and c.cout <= self.fuse_apply_max_c
            bits = rec["mask"] if last else None    # sign words of the block output; an inner mask is recomputed from raw_i
            # the shortcut gradient dz = dout*[out > 0] is stored for the downsample branch only.  With an identity shortcut it
            # is never stored: the first conv's data-gradient epilogue re-forms it from dout and the mask bits (dx = dgrad + dz)
            keep_dz = last and b.ds is not None
            add, add_mask = (dout, rec["mask"]) if (i == 0 and b.ds is None) else (None, None)
            ca_n = c.cout if (chan and last and f16) else 0     # channels of the per-channel absmax row of dz, 0 = none
            # what this conv's data gradient also reduces in its epilogue (stride 1 only): the backward statistics of bn_{i-1},
            # or - identity shortcut - of the BatchNorm below the block, masked by the sign bits of x
            bnb = None
            if c.stride == 1 and i > 0:
                bnb = (raws[i - 1], None, b.bns[i - 1].t4)
            elif c.stride == 1 and b.ds is None and prev is not None:
                bnb = (prev[0], x, prev[1], rec["xmask"])
            res_amax, draw_amax = take(), take()
            if fused:
                draw, draw_slot, dz_i, inb = self._bnbwd_fused(bn, raw, g, g_part, g_amax, bits, out if last else None, keep_dz,
                                                               acc, amx16, raw_amax, draw_amax, ca_n)
                res = ops.conv_dgrad(g, c.wpk_t, c.cin, c.k, 1, hw, add=add, add_mask=add_mask, bn_bwd=bnb, in_bnbwd=inb,
                                     side=(draw, dz_i), in_amax=draw_slot if f16 else None, out_amax=res_amax,
                                     side_amax=draw_amax, side_presplit=f16)
            else:
                if se:
                    draw, draw_slot, dz_i = self._bnbwd_se(b.se, rec["se"], bn, raw, g, g_amax, bits, keep_dz, acc, amx16,
                                                           raw_amax, draw_amax, ca_n)
                else:
                    draw, draw_slot, dz_i = self._bnbwd_pass(bn, raw, g, g_part, g_amax, bits, keep_dz, acc, amx16, raw_amax,
                                                             draw_amax, ca_n)
                res = ops.conv_dgrad(draw, c.wpk_t, c.cin, c.k, c.stride, hw, add=add, add_mask=add_mask, bn_bwd=bnb,
                                     in_amax=draw_slot if f16 else None, out_amax=res_amax, in_presplit=f16)
            if last:
                dz = dz_i
            self._count(draw, draw_slot, pairs=f16)
            if self.bound_log is not None and f16:
                self.bound_log.append((c.cout, c.k, draw_slot, draw_amax))
            g, g_part = res if bnb is not None else (res, None)
            g_amax = res_amax
            self._wgrad(inp, draw, c.h.weight.grad, c.k, c.stride, in_affine=in_aff, accumulate=acc,
                        dy_amax=draw_slot if f16 else None, x_amax=rec["in_amax"][i] if f16 else None, dy_presplit=f16)
        dx, part, dx_amax = g, g_part, g_amax
        if b.ds is not None:
            cd, bnd = b.ds
            f16d = amx is not None and ops.split_for(1, True) == 3
            drawd_amax = take() if f16d else None
            drawd = ops.bn_backward(dz, rec["rawd"], None, bnd.t4, bnd.h.weight.data, bnd.h.weight.grad, bnd.h.bias.grad,
                                    MASK_NONE, draw_out=dz, accumulate=acc, amax_out=drawd_amax)
            self._count(drawd, drawd_amax)
            self._wgrad(x, drawd, cd.h.weight.grad, 1, cd.stride, accumulate=acc, dy_amax=drawd_amax,
                        x_amax=rec["in_amax"][0] if f16d else None)
            # the 1x1 gradient lands on top of the 3x3 one: the same slot ends up >= the absmax of the sum's final values
            ops.conv_dgrad(drawd, cd.wpk_t, cd.cin, 1, cd.stride, (x.shape[1], x.shape[2]), out=dx, accumulate=True,
                           in_amax=drawd_amax, out_amax=dx_amax)
            part = None
        return dx, part, dx_amax

    # The three forms of one BatchNorm backward inside _block_bwd.  g / g_part / g_amax: the gradient wrt the BatchNorm's (+ReLU)
    # output, its partial sums when the producing epilogue made them, its absmax slot.  bits: sign words of the block output (the
    # last BatchNorm) or None (an inner one).  keep_dz: also store dz.  amx16: the slot table in the f16x3 mode, else None.
    # ca_n: channels of the per-channel absmax row to take, or 0.  -> (draw, the slot that scales draw for its consumers, dz).
    def _bnbwd_fused(self, bn, raw, g, g_part, g_amax, bits, act, keep_dz, acc, amx16, raw_amax, draw_amax, ca_n):
        """Fused into the data gradient of the same convolution: reduce (unless g_part came from an epilogue; the last BatchNorm
        from the block output `act`) and finalize here; the data gradient applies it while staging and writes draw and dz as
        side outputs.  -> (draw, draw_slot, dz, in_bnbwd operand of that data gradient); draw and dz are still empty."""
        ca = amx16.take_n(ca_n) if ca_n else None
        if g_part is None:
            g_part = ops.bn_bwd_partial(g, raw, act, bn.t4, MASK_RAW if bits is None else MASK_ACT, chan_amax=ca)
        est = amx16.take() if amx16 else None
        coef = ops.bn_bwd_coef(g_part, raw.numel() // raw.shape[-1], bn.h.weight.data, bn.t4, bn.h.weight.grad,
                               bn.h.bias.grad, acc, amax_in=g_amax, raw_amax=raw_amax, est_out=est, chan_amax=ca)
        draw = torch.empty_like(raw)
        dz = torch.empty_like(raw) if keep_dz else None
        inb = (raw, act, bn.t4, coef) if bits is None else (raw, act, bn.t4, coef, bits)
        return draw, (est if amx16 else draw_amax), dz, inb

    def _bnbwd_pass(self, bn, raw, g, g_part, g_amax, bits, keep_dz, acc, amx16, raw_amax, draw_amax, ca_n):
        """Stand-alone BatchNorm-backward pass (then a plain, pipelined data gradient).  An inner BatchNorm overwrites g with draw;
        the last one reads the bits instead of the block output and leaves dout alone, or (keep_dz) turns it into dz."""
        est = amx16.take() if amx16 else None
        pair = (g_amax, raw_amax, est) if amx16 else None
        ca = amx16.take_n(ca_n) if ca_n else None
        dz = g if keep_dz else None
        draw = ops.bn_backward(g, raw, bits, bn.t4, bn.h.weight.data, bn.h.weight.grad, bn.h.bias.grad,
                               MASK_RAW if bits is None else MASK_BITS, draw_out=g if bits is None else None, dz_out=dz,
                               accumulate=acc, partial=g_part, amax_out=draw_amax, pair=pair, chan_amax=ca)
        return draw, (est if amx16 else draw_amax), dz

    def _bnbwd_se(self, se, se_rec, bn, raw, g, g_amax, bits, keep_dz, acc, amx16, raw_amax, draw_amax, ca_n):
        """Last BatchNorm of an SE block (se: the gate's parameters, se_rec: what its forward saved): e = dout [out > 0] is the
        shortcut gradient; the BatchNorm sees dz = g e + dq / HW.  One pass reduces (sum e, sum e raw) per utterance, the gate
        kernels turn those tables into dW1, dW2, dq and the BatchNorm-backward statistics, one pass writes draw (and, keep_dz,
        e over dout)."""
        est = amx16.take() if amx16 else None
        pair = (g_amax, raw_amax, est) if amx16 else None
        ca = amx16.take_n(ca_n) if ca_n else None
        sums, q, u, gate = se_rec
        S = ops.se_bwd_reduce(g, raw, bits, MASK_BITS, chan_amax=ca)
        w1, w2 = se.w1, se.w2
        coef, dq, _, _ = ops.se_bwd_gate(S, sums, q, u, gate, w1.data, w2.data, bn.t4, bn.h.weight.data, w1.grad, w2.grad,
                                         bn.h.weight.grad, bn.h.bias.grad, raw.shape[1] * raw.shape[2], accumulate=acc,
                                         pair=pair, chan_amax=ca)
        e = g if keep_dz else None
        draw = ops.se_bwd_apply(g, raw, bits, MASK_BITS, gate, dq[1], bn.t4, coef, e_out=e, amax_out=draw_amax, pair_scale=est)
        return draw, (est if amx16 else draw_amax), e

    # ---- fused training step (forward + CE + backward, no autograd graph) --------------------------------------
    def loss_and_grad(self, x, y, on_stage_done=None):
        """One iteration of scripts/train_resnet.py:316-327 without the autograd shell: returns
        (loss [1] device tensor, logits, rank [B] int32 for accuracy).  Gradients land in the .grad arena."""
        x = self._check_input(x)
        y = y.contiguous()
        with torch.no_grad():
            logits, saved = self.forward_train(x, y)
            loss_row, dl, rank = ops.softmax_ce(logits, y, grad_scale=1.0 / logits.shape[0])
            loss = ops.mean(loss_row)
        self.backward(saved, dl, on_stage_done)
        return loss, logits, rank


STAGE_ORDER = ["head", "layer4", "layer3", "layer2", "layer1", "stem"]     # the order backward finishes the stages in


class GraphedTrainStep:
    """weight re-pack + forward + CE + backward of one fixed-shape batch captured as hipGraphs (torch.cuda.CUDAGraph): one
    host launch per step instead of ~450, so a busy host cannot starve the GPU.  Inputs are copied into static buffers;
    gradients land in the model's flat gradient arena exactly as in the eager path (always overwritten).
    The optimizer step stays outside the graph (its learning rate changes per epoch).

    segmented=False (one GPU): ONE graph.
    segmented=True (data parallel): the step is cut where backward finishes a ResNet stage - six graphs sharing one
    memory pool, replayed back to back.  Between two replays the host enqueues that stage's gradient all-reduce on the
    communication stream (`on_stage_done(name)`, parallel.GradAllReducer), so the RCCL kernels of stage k overlap the
    data / weight gradients of stages k-1..stem exactly as in the eager path (reference: DDP's bucketed all-reduce
    overlapped with backward, scripts/train_resnet.py:183-185,327), with 6 host launches per step instead of ~450 and
    no collective inside a captured region."""

    def __init__(self, engine, batch, frames, warmup=2, side_stream=None, segmented=False, pool=None):
        """pool: memory pool of another GraphedTrainStep of the same engine (`other.pool()`): steps for different chunk
        lengths are never replayed concurrently, so they can share one pool - the cache of per-length graphs then costs
        the activation memory of the longest length, not the sum."""
        import os
        if side_stream is None:
            side_stream = os.environ.get("SPK_GRAPH_SIDE", "0") == "1"
        m = engine.m
        dev = m.flat_parameters().device
        self.eng = engine
        # measured on MI355X / ROCm 7.2: a captured two-branch graph (weight gradients on the side stream) replays no faster than the
        # same kernels captured on one stream (round 1: ~2 % slower; round 3: 52.5-52.8 ms both ways), so the graph is recorded
        # single-stream
        side, engine.use_side_stream = engine.use_side_stream, bool(side_stream)
        self.x = torch.zeros(batch, m.feat_dim, frames, device=dev)
        self.y = torch.zeros(batch, dtype=torch.long, device=dev)
        self.shape = (batch, m.feat_dim, frames)
        # warm-up outside capture: allocates the workspaces / BN buffers the graph will reuse, picks tiles.
        # It runs real steps on a dummy batch, so the BatchNorm running statistics are snapshotted and restored.
        saved_buffers = [b.clone() for b in m.buffers()]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                for p in m.parameters():
                    p.grad = None
                engine.loss_and_grad(self.x, self.y)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        for b, sb in zip(m.buffers(), saved_buffers):
            b.copy_(sb)
        for p in m.parameters():
            p.grad = None                      # captured backward overwrites (no accumulation)
        # The optimizer rewrites the weights between replays (scripts/train_resnet.py:316-328: forward runs on what
        # optimizer.step() just wrote), so the weight re-pack MUST be a node of the graph: the warm-up steps left the
        # engine clean, mark it dirty so that the capture records the batched pack launch (its device-resident job table
        # was built during warm-up and is kept alive by self.pack_table).
        engine.dirty = True
        self.segments = []                     # [(graph, stage name reported after it or None)]
        cap = {"g": None, "ctx": None}

        def begin():
            g = torch.cuda.CUDAGraph()
            kw = {"pool": self.segments[0][0].pool()} if self.segments else ({"pool": pool} if pool is not None else {})
            # thread_local: helper threads of other libraries (the RCCL watchdog) may touch the device during capture
            ctx = torch.cuda.graph(g, capture_error_mode="thread_local", **kw)
            ctx.__enter__()
            cap["g"], cap["ctx"] = g, ctx

        def end(name):
            cap["ctx"].__exit__(None, None, None)
            self.segments.append((cap["g"], name))
            cap["g"] = cap["ctx"] = None

        def cut(name):                         # Engine.backward reports: every gradient of stage `name` is enqueued
            end(name)
            if name != STAGE_ORDER[-1]:
                begin()

        begin()
        try:
            self.loss, self.logits, self.rank = engine.loss_and_grad(self.x, self.y, cut if segmented else None)
            if cap["ctx"] is not None:
                end(None)
        except BaseException:
            if cap["ctx"] is not None:
                cap["ctx"].__exit__(None, None, None)
            raise
        self.graph = self.segments[0][0]
        assert [n for _, n in self.segments] == (STAGE_ORDER if segmented else [None])
        self.pack_table = engine._pack_tables.get(True)
        assert self.pack_table is not None and self.pack_table.launches_captured >= 1, \
            "the captured training step does not contain the conv-weight re-pack"
        engine.dirty = True                    # the capture itself executed nothing
        engine.use_side_stream = side

    def matches(self, x):
        return tuple(x.shape) == self.shape

    def pool(self):
        return self.segments[0][0].pool()

    def __call__(self, x, y, on_stage_done=None):
        self.x.copy_(x, non_blocking=True)
        self.y.copy_(y, non_blocking=True)
        for g, name in self.segments:          # segment 0 re-packs the conv weights from the parameter arena first
            g.replay()
            if name is not None and on_stage_done is not None:
                on_stage_done(name)
        self.eng.dirty, self.eng._packed_for_bwd = False, True
        self.eng.m.attach_grads()
        return self.loss, self.logits, self.rank


class GraphedStepCache:
    """Variable-length training (BASELINE configs[3]; reference scripts/datasets.py:40-43,53-57: chunk lengths drawn in
    [min, max], here ONE length per batch, identical on every rank): a GraphedTrainStep per (batch, frames), captured on
    first use, all sharing ONE memory pool - steps of different lengths are never replayed concurrently, so the cache costs
    the activation memory of the longest length it has seen, not the sum - and at most `max_graphs` of them (least recently
    used dropped first).  Host cost per step after the first visit of a length: the replay launches, < 1 ms."""

    def __init__(self, engine, segmented=False, max_graphs=64, warmup=2):
        self.eng, self.segmented, self.max_graphs, self.warmup = engine, segmented, max_graphs, warmup
        self.steps = {}            # (batch, frames) -> GraphedTrainStep, in least-recently-used order
        self._pool_owner = None    # keeps the shared pool alive even after its first graph was dropped
        self.captures = 0

    def get(self, batch, frames):
        key = (int(batch), int(frames))
        st = self.steps.pop(key, None)
        if st is None:
            pool = self._pool_owner.pool() if self._pool_owner is not None else None
            st = GraphedTrainStep(self.eng, key[0], key[1], warmup=self.warmup, segmented=self.segmented, pool=pool)
            if self._pool_owner is None:
                self._pool_owner = st
            self.captures += 1
            while len(self.steps) >= self.max_graphs:
                old = next(iter(self.steps))
                if self.steps[old] is self._pool_owner:      # never drop the owner of the pool: re-queue it
                    self.steps[old] = self.steps.pop(old)
                    if len(self.steps) == 1:
                        break
                    continue
                del self.steps[old]
        self.steps[key] = st
        return st

    def __call__(self, x, y, on_stage_done=None):
        return self.get(x.shape[0], x.shape[2])(x, y, on_stage_done)

    def __len__(self):
        return len(self.steps)
