/* libspkhip - C ABI of the MI355X (gfx950) speaker-embedding hot path.
 *
 * Drop-in boundary: the reference (ZihanLiao/pytorch-kaldi-resnet) has no native
 * layer; its seam is the torch.nn.Module protocol of NeuralSpeakerModel (scripts/model.py:334-432) as
 * driven by scripts/train_resnet.py:304-328 and scripts/decode.py:185-208.  Every torch op on that path
 * maps to one export below; the Python mirror of NeuralSpeakerModel binds them with ctypes
 * (pytorch-kaldi-resnet_amd/hip.py).  Each export cites the reference call site it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless stated otherwise
 *   - the caller owns every buffer, including workspaces; the library never allocates device memory
 *     and keeps no pointer across calls
 *   - every call is an asynchronous launch on `stream` (a hipStream_t) and never synchronises
 *   - return value: 0 = ok, < 0 = invalid argument (see spk_last_error), > 0 = hipError_t of the launch
 *   - activations are NHWC fp32: [B][H = mel bins][W = frames][C]; the network input is [B][F][T]
 *     (reference layout, scripts/datasets.py:68, scripts/model.py:247) which is NHWC with C = 1
 *   - arithmetic is fp32 throughout (MFMA v_mfma_f32_32x32x2_f32 = exact fp32 FMA chain)
 */
#ifndef SPKHIP_H
#define SPKHIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

int spk_version(void);
const char* spk_last_error(void);
/* bit 0: the library was built with SPK_EXPERIMENTAL=1 and contains the kernel forms that were measured and did not pay
 * (SPK_CONV_WS of spk_conv_mfma / spk_conv_wgrad, SPK_CONV_PIPE of spk_conv_wgrad, SPK_CONV_PIPE + SPK_IN_BNBWD of spk_conv_mfma);
 * without it those flag combinations are argument errors */
int spk_build_flags(void);

/* flags for the fused input transform / epilogue of the convolutions */
#define SPK_IN_AFFINE_RELU 1 /* input tile = max(in*in_scale[c] + in_shift[c], 0): BN+ReLU of the producer, fused */
#define SPK_EPI_AFFINE 2     /* out = acc*epi_scale[c] + epi_shift[c]   (eval-mode BN folded into the conv) */
#define SPK_EPI_ADD 4        /* out += epi_add[same index]              (residual add / gradient accumulation) */
#define SPK_EPI_RELU 8       /* out = max(out, 0) */
#define SPK_EPI_STATS 16     /* stats[4*pixel_tile + wave][c] = (sum, sumsq) of the stored values (train-mode BN) */
#define SPK_IN_BNBWD 64      /* stride-1 data gradients: the staged input is BatchNorm-backward(in) computed on the fly from
                                in, in_raw, the mask (in_act > 0, or in_raw*scale+shift > 0 when in_act is NULL), in_bn4
                                [mean,invstd,scale,shift][Cin] and in_coef [3][Cin] (spk_bn_bwd_finalize); the tile owner
                                writes that value to side_draw (for the weight gradient) and in*mask to side_dz (optional) */
#define SPK_EPI_BNBWD 32     /* with EPI_STATS, data-gradient launches: stats = (sum dz, sum dz*xhat) of the BatchNorm whose
                                output gradient this launch produces (dz = out * mask; mask = bn_act > 0, or
                                bn_raw*scale+shift > 0 when bn_act is NULL; bn4 = [mean, invstd, scale, shift][Cout]) */

/* kernel form (results are bit-identical to the plain kernel on the same tile, SPK_CONV_M16 excepted); "experimental" = needs spk_build_flags() & 1 */
#define SPK_CONV_WS 128      /* experimental: producer / consumer form of spk_conv_mfma (split != 0, 9 taps, kc = 1; flags bits 8-9 = log2 of
                                its consumer-wave channel groups) and of spk_conv_wgrad (split = 3, 3x3) */
#define SPK_CONV_PIPE 1024   /* in-wave pipelined form: spk_conv_mfma (split = 3, 9 taps, kc = 1, <= 576 halo pixels, two halo
                                tiles in LDS; plain or f16 pair input); experimental: with SPK_IN_BNBWD (in_mask given, MT*NT <= 4)
                                and for spk_conv_wgrad (split = 3, 3x3, tile of 1 or 2 k-steps of 16 pixels per wave group) */

#define SPK_CONV_M16 (1 << 17) /* with SPK_CONV_PIPE on spk_conv_mfma (plain or f16 pair input, MT = 3, NT = 2, <= 512 halo pixels,
                                Cin % 32 == 0): the same kernel on v_mfma_f32_16x16x32_f16, two taps per 32-deep K step.  Same products,
                                another summation order: equal to the other forms within fp32 accumulation error, not bit-identical */

#define SPK_WGRAD_GROUPS 2048 /* spk_conv_wgrad, split = 3: 1x1: the kernel that gives a block 1 << (flags bits 12-13) = 2 or 4
                                groups of 32 input channels (Cin % (32 * groups) == 0, WN 2 or 4, tile <= 64 pixels); 3x3: the
                                2 x 2 (input-channel group x output-channel group) wave layout (groups = 2, WN = 2) */

/* f16 pair tensors (split = 3).  A tensor with the shape and addressing of an fp32 NHWC tensor in which every aligned group of
 * four floats (16 bytes) holds [4 x fp16 high term][4 x fp16 low term] of value * sigma, sigma = the power of two that takes
 * the float whose bits the tensor's scale slot holds into [2^14, 2^15).  The slot holds a RIGOROUS upper bound of the tensor's
 * absmax, known before the producer runs (spk_bn_bwd_finalize est_out).  Producers: spk_bn_bwd_apply(pair_scale), and the side
 * output of a fused BatchNorm-backward data gradient (SPK_SIDE_PRESPLIT).  Consumers stage 16-byte groups by plain copy. */
#define SPK_WGRAD_NOSHIFT (1 << 18) /* spk_conv_wgrad + SPK_WGRAD_GROUPS, 3x3: at stride 1 with TW % 8 == 0 the kernel builds the fragments of
                                the three taps of a filter row from one 10-pixel window per lane (22 instead of 40 transposed LDS reads per
                                k-step; bit-identical results); this flag keeps the plain K loop (A/B measurements) */
#define SPK_WGRAD_M16 (1 << 19) /* spk_conv_wgrad + SPK_WGRAD_GROUPS, 3x3, with SPK_DY_PRESPLIT: conv_wgrad_wm16_kernel - the 2 x 2 wave layout on
                                v_mfma_f32_16x16x32_f16 (32 pixels per K step), dy brought into LDS by global_load_lds (no registers, no
                                staging instructions; two LDS buffers).  LDS: halo * 384 + 2 * ceil32(TH * TW) * 256 bytes.  Same products,
                                another summation order: equal to the other weight gradients within fp32 accumulation error.
                                WITHOUT SPK_WGRAD_GROUPS (3x3, WN = 1, SPK_DY_PRESPLIT): conv_wgrad_c32m16_kernel - the same kernel in its
                                layout for 32-channel groups (the first layer): a block owns 32 x 32 channels, its four waves split the
                                32-pixel k-steps of a region and fold their tiles through LDS at the end; halo <= 192 pixels, LDS: halo *
                                192 + 2 * ceil32(TH * TW) * 128 bytes (at least 36 KB); one slab per block as every other form */
#define SPK_IN_PRESPLIT (1 << 14)    /* spk_conv_mfma: `in` is an f16 pair tensor scaled by the sigma of *in_amax (plain input only) */
#define SPK_SIDE_PRESPLIT (1 << 15)  /* spk_conv_mfma + SPK_IN_BNBWD: side_draw leaves as an f16 pair tensor (scale: *in_amax) */
#define SPK_DY_PRESPLIT (1 << 16)    /* spk_conv_wgrad: `dy` is an f16 pair tensor scaled by the sigma of *dy_amax */
#define SPK_CONV_CK32 (1 << 23)      /* spk_conv_mfma + SPK_IN_BNBWD, split = 3, Cin = 32, MT = 1 or 2, NT = 1 (not CONV_PIPE / CONV_WS): the
                                        staging takes whole 128-byte pixels (one 32-channel plane of 144 B per LDS pixel instead of two
                                        16-channel planes of 80 B staged one after the other).  Bit-identical results at an equal tile */
#define SPK_EPI_WMASK (1 << 24)      /* spk_conv_mfma_len / spk_stem_conv_fwd_len only: an output pixel of image b at width (time)
                                        x >= wlen[b] is stored as 0 after the whole epilogue and does not enter out_amax / the
                                        statistics (length-masked eval forward of a padded batch).  Every other entry refuses it */

/* ---- convolutions --------------------------------------------------------------------------------- */

/* nn.Conv2d weight [Cout][Cin][KH][KW] (scripts/model.py:12-15,105-110,233-234) -> MFMA fragment order
 * [tap][K/8][N/32][64][4]; transpose = 0 for the forward conv (K = Cin), 1 for its data gradient (K = Cout). */
int spk_pack_conv_weight(const float* w, float* wpk, int Cout, int Cin, int KH, int KW, int transpose, void* stream);
/* the same weights for the split operand modes of spk_conv_mfma: split = 6 or 9: every weight as three bf16 terms whose sum
 * is the fp32 value, [tap][K/16][term][N/32][64][8 bf16] = 6 bytes per weight; split = 3: a 16-byte header (word 0 = float
 * bits of max|w|) followed by w * sigma as two fp16 terms in the same order (4 bytes per weight), sigma = the power of two
 * that puts max|w| in [2^14, 2^15) - spk_conv_mfma reads the header and derives the same sigma */
int spk_pack_conv_weight_split(const float* w, void* wpk, int Cout, int Cin, int KH, int KW, int transpose, int split,
                               void* stream);
/* every convolution of the network in one launch: `jobs` is a device array of njobs 48-byte entries
 * { const float* w; void* wpk; int Cout, Cin, KH*KW, transpose, split, total = Cout*Cin*KH*KW, block0, pad; } ordered by
 * block0 (first 256-thread block of the job; total_blocks = sum of ceil(total/256)).  spk_pack_job_bytes() = 48. */
int spk_pack_job_bytes(void);
int spk_pack_conv_weights_batched(const void* jobs, int njobs, int total_blocks, int has_f16 /* the table holds split = 3
                                  jobs: their absmax headers are refreshed first */, void* stream);

/* Implicit-GEMM convolution described by a tap table; replaces F.conv2d forward (scripts/model.py:51,56,
 * 118,122,126,58-59) and, with a transposed pack and mirrored taps, its data gradient (autograd of the same,
 * scripts/train_resnet.py:327).  Logical output pixel (oy,ox) of an OH x OW grid reads input pixel
 * (oy*IS + tap_dy[t], ox*IS + tap_dx[t]) with weight tap tap_w[t] and is stored at (oy*OS + ooy, ox*OS + oox)
 * of the physical [B][OHf][OWf][Cout] output.  TH x TW = pixel region per block (<= 128*MT pixels),
 * MT in 1..4 m-tiles per wave, NT in {1,2,4} 32-channel n-tiles per block, kc = 32-channel planes staged per barrier
 * (1 for 3x3; up to 4 for single-tap 1x1 convolutions; ntaps*kc <= 9, Cin % (32*kc) == 0).  ips = input pixel stride:
 * the taps address a logical input grid whose pixel (y,x) is physical pixel (y*ips, x*ips) - a strided 1x1 convolution
 * is run as IS = 1, ips = 2 so that only the pixels it uses are staged.
 * stats (EPI_STATS): [4*B*ceil(OH/TH)*ceil(OW/TW)][Cout][2] floats (one partial row per wave).
 * split: 0 = fp32 operands on v_mfma_f32_32x32x2_f32 (wpk from spk_pack_conv_weight); 6 or 9 = operands split exactly into
 * three bf16 terms while staged / packed (wpk from spk_pack_conv_weight_split) and the 6 most significant (or all 9) cross
 * terms multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation - inputs, outputs and measured accuracy are fp32
 * (planes are then 16 channels: Cin % (16*kc) == 0).
 * split = 3 ("f16x3", 3x3 and 1x1): operands as two fp16 terms of value * sigma, sigma a power of two (weights: from max|w| at
 * pack time; staged input: 2^(14 - exponent) of the float whose bits *in_amax holds - REQUIRED: the absmax of the staged
 * values, written by the kernel that produced the tensor, or a rigorous upper bound of it (spk_bn_finalize est_out for a fused
 * input BatchNorm+ReLU, spk_bn_bwd_finalize est_out for a fused BatchNorm backward) - so that the largest staged magnitude
 * lands in [2^14, 2^15) and nothing can saturate), three cross products on v_mfma_f32_32x32x16_f16, fp32 accumulation,
 * accumulators scaled back by 1/(sigma_in * sigma_w).  Values below bound * 2^-18 have a subnormal low term (the instruction
 * keeps fp16 subnormals: absolute error <= bound * 2^-39, relative precision falling from 22 to 11 bits at bound * 2^-28).
 * Measured accuracy = the fp32 instruction's (tools/probe/split_probe.hip).  out_amax / side_amax (optional, any split): the
 * launch atomically maxes the float bits of |stored output| / |side_draw| into them - the in_amax of the kernels that consume
 * those tensors (side_amax records the true absmax also when side_draw leaves as an f16 pair tensor).
 * flags: the SPK_* bits above. */
int spk_conv_mfma(const float* in, const float* wpk, float* out, const float* in_scale, const float* in_shift,
                  const float* epi_scale, const float* epi_shift, const float* epi_add, const float* in_raw,
                  const float* in_act, const float* in_bn4, const float* in_coef, const unsigned* in_mask /* sign bits of
                  in_act, [pixel][Cin/32] words: read instead of it */, const unsigned* bn_mask /* same for bn_act,
                  [pixel][Cout/32] */, const unsigned* add_mask /* EPI_ADD adds only where the bit is set */,
                  float* side_draw, float* side_dz,
                  const float* bn_raw, const float* bn_act, const float* bn4, float* stats, int B, int IH,
                  int IW, int Cin, int OH, int OW, int OHf, int OWf, int Cout, int IS, int OS, int ooy, int oox,
                  int ntaps, const int* tap_dy /*host*/, const int* tap_dx /*host*/, const int* tap_w /*host*/, int TH,
                  int TW, int MT, int NT, int kc, int ips, int flags, int split, const unsigned* in_amax, unsigned* out_amax,
                  unsigned* side_amax, void* stream);
/* spk_conv_mfma with a length mask (length-masked eval forward of a padded batch): same arguments plus wlen, a DEVICE int array [B]
 * of valid output widths; flags must carry SPK_EPI_WMASK.  Output pixel (y, x) of image b with x >= wlen[b] (physical output column)
 * is stored as 0 after the whole epilogue (affine, add, ReLU) and stays out of out_amax and the statistics.  Implemented by
 * conv_mfma_kernel and conv_pipe_kernel (M16 included) with a plain input; IN_BNBWD, EPI_BNBWD, IN_PRESPLIT, SIDE_PRESPLIT and
 * CONV_WS are refused, as is SPK_EPI_WMASK on spk_conv_mfma (no wlen) or on any other entry. */
int spk_conv_mfma_len(const float* in, const float* wpk, float* out, const float* in_scale, const float* in_shift,
                      const float* epi_scale, const float* epi_shift, const float* epi_add, const float* in_raw,
                      const float* in_act, const float* in_bn4, const float* in_coef, const unsigned* in_mask,
                      const unsigned* bn_mask, const unsigned* add_mask, float* side_draw, float* side_dz,
                      const float* bn_raw, const float* bn_act, const float* bn4, float* stats, int B, int IH,
                      int IW, int Cin, int OH, int OW, int OHf, int OWf, int Cout, int IS, int OS, int ooy, int oox,
                      int ntaps, const int* tap_dy /*host*/, const int* tap_dx /*host*/, const int* tap_w /*host*/, int TH,
                      int TW, int MT, int NT, int kc, int ips, int flags, int split, const unsigned* in_amax, unsigned* out_amax,
                      unsigned* side_amax, const int* wlen /*device [B]*/, void* stream);

/* Weight gradient of a 3x3 (pad 1) or 1x1 (pad 0) conv at stride 1 or 2 (autograd of nn.Conv2d).
 * x: conv input [B][IH][IW][Cin] (optionally raw + fused BN/ReLU via in_scale/in_shift and SPK_IN_AFFINE_RELU),
 * dy: gradient of the raw conv output [B][OH][OW][Cout]; dw: OIHW [Cout][Cin][k][k].
 * partial: workspace of spk_conv_wgrad_workspace(nsplit, ksize, Cin, Cout) bytes. TW must be even; the region must fit
 * the kernel's register prefetch window: halo pixels <= *max_halo_pix, TH*TW <= *max_tile_pix (spk_conv_wgrad_limits). */
int spk_conv_wgrad_limits(int WN, int* max_halo_pix /*host*/, int* max_tile_pix /*host*/);
size_t spk_conv_wgrad_workspace(int nsplit, int ksize, int Cin, int Cout);
/* Streaming 3x3 forward convolution of the 32-channel layer: 32 -> 32 channels, stride 1, padding 1, f16x3 operands - conv1 / conv2 of
 * the BasicBlocks of layer 1 (scripts/model.py:12-15,48-64).  Persistent blocks over 8 x 16-pixel tiles, the weights as matrix-core
 * fragments in LDS for the life of a block, the 10 x 18 halo staged once per tile from whole 128-byte lines one tile ahead (fused
 * BatchNorm + ReLU with SPK_IN_AFFINE_RELU), stores from the accumulator layout.  in / out: [B][H][W][32]; wpk:
 * spk_pack_conv_weight_split(split = 3, transpose = 0) of the [32][32][3][3] weights; flags: SPK_EPI_STATS [| SPK_IN_AFFINE_RELU];
 * stats: [4 * nblocks][32][2] partial rows (sum, sum of squares) for spk_bn_finalize; in_amax REQUIRED, out_amax optional;
 * nblocks: persistent blocks (<= tiles; two per CU).  Same products as spk_conv_mfma; another order of the statistics partials. */
int spk_conv3x3_c32_stream(const float* in, const float* wpk, float* out, const float* in_scale, const float* in_shift, float* stats,
                           int B, int H, int W, int flags, const unsigned* in_amax, unsigned* out_amax, int nblocks, void* stream);
/* Streaming 1x1 convolution, C -> C channels (C = 32, 64 or 128), stride 1, f16x3 operands: forward and data gradient of the 1x1
 * convolutions of the Bottleneck blocks (scripts/model.py:104-110,118-126) - a GEMM [P pixels][C] x [C][C] by persistent blocks that
 * keep the whole weight matrix in registers, stage every pixel once (whole 128-byte lines; fused BatchNorm + ReLU with
 * SPK_IN_AFFINE_RELU, plain copy of an f16 pair tensor with SPK_IN_PRESPLIT) and store from the accumulator layout.  in / out /
 * epi_add / bn_raw: [P][C]; wpk: spk_pack_conv_weight_split(split = 3) of the 1x1 weights (transpose = 1 for the data gradient);
 * flags: SPK_IN_AFFINE_RELU | SPK_IN_PRESPLIT | SPK_EPI_STATS | SPK_EPI_ADD (+ add_mask: add only where the bit is set) |
 * SPK_EPI_BNBWD (statistics of the BatchNorm-backward of bn4 = [mean, invstd, scale, shift][C] over dz = out * mask, mask = the
 * bits of bn_mask, or bn_raw * scale + shift > 0 when bn_mask is NULL).  stats: [spk_conv1x1_stream_rows(nblocks, C)][C][2]
 * partial rows for spk_bn_finalize / spk_bn_bwd_finalize.  in_amax: REQUIRED (slot of the staged values, as spk_conv_mfma);
 * out_amax: optional.  nblocks: persistent blocks (<= tiles of 64 / 128 / 256 pixels at C = 128 / 64 / 32; two per CU is the
 * measured choice).  Same arithmetic as spk_conv_mfma on these launches; another summation order of the statistics partials. */
int spk_conv1x1_stream(const float* in, const float* wpk, float* out, const float* in_scale, const float* in_shift,
                       const float* epi_add, const unsigned* add_mask, const float* bn_raw, const unsigned* bn_mask,
                       const float* bn4, float* stats, long long P, int C, int flags, const unsigned* in_amax, unsigned* out_amax,
                       int nblocks, void* stream);
int spk_conv1x1_stream_rows(int nblocks, int C);
/* spk_conv_wgrad writes nsplit partial slabs [nsplit][k*k][Cin][Cout] (nsplit <= number of pixel regions); spk_wgrad_reduce
 * sums them in a fixed order into dw (OIHW), optionally accumulating.  (`dw`/`accumulate` of spk_conv_wgrad are unused.) */
int spk_wgrad_reduce(const float* partial, float* dw, int nslab, int ksize, int Cin, int Cout, int accumulate, void* stream);
int spk_conv_wgrad(const float* x, const float* dy, float* dw, float* partial, const float* in_scale,
                   const float* in_shift, int B, int IH, int IW, int Cin, int OH, int OW, int Cout, int ksize, int stride,
                   int TH, int TW, int WN, int nsplit, int flags, int accumulate, int split /* 0, or 6 / 9 = bf16-split operands
                   (3x3 only), 3 = fp16 two-term operands (3x3 and 1x1), see spk_conv_mfma */, const unsigned* dy_amax /* split 3,
                   required: float bits of absmax(dy) or of an upper bound: fixes the dY operand scale (the scale slot of dy when
                   SPK_DY_PRESPLIT) */, const unsigned* x_amax /* split 3, required: the same for the (transformed) x operand:
                   its absmax or a bound (spk_bn_finalize est_out / spk_affine_estimate) */, void* stream);

/* Which instance of its kernel a launch takes.  The flag combinations of the training step are compiled as variants in which the
 * flag word is a template argument (the per-pass and per-item branches fold away, results bit-identical); everything else runs
 * the generic instance that reads the word from its argument block.  These are the pure host functions the launchers themselves
 * call (no GPU needed).  Return value: the variant's template argument (>= 0), or -1 = generic.  Environment SPK_FL_VARIANTS=0
 * (read once per process; default 1) makes every launch generic: A/B runs and identity tests on one build.
 * spk_conv_variant_of: MT, NT, split, flags as given to spk_conv_mfma / spk_conv_mfma_len; ptrs: which optional operands are
 * given (SPK_PTR_* bits).  spk_wgrad_variant_of: arguments as given to spk_conv_wgrad; conv_wgrad_split_kernel only (launches of
 * the other weight-gradient kernels return -1). */
#define SPK_PTR_ADD_MASK 1
#define SPK_PTR_BN_MASK 2
#define SPK_PTR_IN_MASK 4
#define SPK_PTR_IN_ACT 8
#define SPK_PTR_BN_ACT 16
#define SPK_PTR_SIDE_DZ 32
int spk_conv_variant_of(int MT, int NT, int split, int flags, int ptrs);
int spk_wgrad_variant_of(int ksize, int stride, int TH, int TW, int WN, int split, int flags);

/* Stem Conv2d(1,32,3,1,1,bias=False) (scripts/model.py:210,249): x [B][F][T] -> out [B][F][T][32];
 * stats (EPI_STATS): [spk_stem_fwd_blocks()][32][2]. */
int spk_stem_fwd_blocks(int B, int F, int T);
int spk_stem_conv_fwd(const float* x, const float* w, float* out, float* stats, const float* epi_scale,
                      const float* epi_shift, int B, int F, int T, int flags,
                      unsigned* amax_out /* optional: atomicMax of the float bits of |out| */, void* stream);
/* the same over a padded batch: image b holds len[b] <= T valid frames (len: DEVICE int array [B]; flags must carry SPK_EPI_WMASK).
 * Frames t >= len[b] of x are read as 0 whatever they hold (NaN included); outputs at t >= len[b] are stored as 0 and stay out of
 * amax_out and the statistics: each image's valid outputs equal those of a run at its own length. */
int spk_stem_conv_fwd_len(const float* x, const float* w, float* out, float* stats, const float* epi_scale,
                          const float* epi_shift, int B, int F, int T, int flags, unsigned* amax_out, const int* len /*device [B]*/,
                          void* stream);
/* its weight gradient; partial: [spk_stem_wgrad_blocks()][32*9] floats */
int spk_stem_wgrad_blocks(int B, int F, int T);
int spk_stem_conv_wgrad(const float* x, const float* draw, float* dw, float* partial, int B, int F, int T,
                        int accumulate, void* stream);
/* Training forward without reading raw0 back (the convolution is cheaper to compute twice than its output is to read once):
 * spk_stem_stats writes the rows spk_stem_conv_fwd(SPK_EPI_STATS) writes, bit for bit, and stores nothing else;
 * spk_stem_fwd_apply recomputes the convolution and writes raw_out, act_out = relu(raw*scale + shift), the sign words of act_out
 * (optional; [B*F*T] words, 32 channels each, as spk_bn_apply's mask_out) and atomicMax'es the float bits of |act_out| into
 * amax_out (optional) - every value bit-equal to spk_stem_conv_fwd followed by spk_bn_apply. */
int spk_stem_stats(const float* x, const float* w, float* stats, int B, int F, int T, void* stream);
int spk_stem_fwd_apply(const float* x, const float* w, const float* scale, const float* shift, float* raw_out, float* act_out,
                       unsigned* mask_out, unsigned* amax_out, int B, int F, int T, void* stream);
/* spk_bn_bwd_apply(MASK_RAW) of d fused into spk_stem_conv_wgrad: the gradient wrt raw is formed in registers and never stored
 * (d is only read); dw is bit-equal to the two calls.  coef: the [3][32] rows of spk_bn_bwd_finalize; partial as above. */
int spk_stem_bwd_wgrad(const float* x, const float* d, const float* raw, const float* mean, const float* invstd,
                       const float* scale, const float* shift, const float* coef, float* dw, float* partial, int B, int F, int T,
                       int accumulate, void* stream);

/* ---- batch normalisation (nn.BatchNorm2d/1d, scripts/model.py:41,44,212,235,361) ------------------- */
/* x viewed as [N][C], C a power of two in [4,1024] */
int spk_bn_stats_blocks(long long N, int C);
int spk_bn_stats_partial(const float* x, float* partial /*[blocks][C][2]*/, long long N, int C, void* stream);
/* partial -> batch mean / invstd, scale = gamma*invstd, shift = beta - mean*scale; running stats updated with
 * momentum and unbiased variance, *num_batches_tracked += 1 (pass NULLs to skip the running update) */
/* ws: fp64 workspace of spk_bn_finalize_workspace(nblk, C) bytes (0 => may be NULL); used to fold many partial
 * rows in parallel before the fixed-order final sum */
size_t spk_bn_finalize_workspace(int nblk, int C);
int spk_bn_finalize(const float* partial, int nblk, int C, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, long long* num_batches_tracked, float* mean, float* invstd,
                    float* scale, float* shift, float momentum, float eps, double* ws,
                    const unsigned* amax_in, unsigned* est_out /* optional (f16x3 hand-off): *est_out = atomicMax over channels
                    of bits(|scale_c| * A + |shift_c|), A = the float in *amax_in = absmax of the normalised tensor: an upper
                    bound of |relu(bn(raw))|, the operand scale input of the convolution that applies this BN while staging */,
                    void* stream);
/* eval mode: scale = gamma/sqrt(running_var+eps), shift = beta - running_mean*scale */
int spk_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float* scale, float* shift, int C, float eps, void* stream);
/* out = [relu](raw*scale + shift [+ res | + res*res_scale + res_shift])  (BasicBlock tail, scripts/model.py:58-62).
 * mask_out (optional, C % 32 == 0): sign bits of `out`, one uint32 per 32 channels of a pixel ([N][C/32]); the backward
 * kernels read these bits (spk_conv_mfma in_mask / bn_mask) instead of the activated tensor. */
int spk_bn_apply(const float* raw, const float* scale, const float* shift, const float* res, const float* res_scale,
                 const float* res_shift, float* out, unsigned* mask_out, long long N, int C, int relu,
                 unsigned* amax_out /* optional: atomicMax of the float bits of |out| */, void* stream);
/* backward; mask_mode 0: dz = dy, 1: dz = dy*(act > 0), 2: dz = dy*(raw*scale+shift > 0), 3: as 1 with `act` pointing at the
 * sign bits of the activated tensor ([pixel][C/32] words, spk_bn_apply mask_out) instead of the tensor */
int spk_bn_bwd_reduce(const float* dy, const float* raw, const float* act, const float* mean, const float* invstd,
                      const float* scale, const float* shift, float* partial, long long N, int C, int mask_mode,
                      unsigned* chan_amax /* optional [C], zeroed by the caller: atomicMax of the float bits of |dz| per CHANNEL
                      (non-finite values left out) - the per-channel A of spk_bn_bwd_finalize */, void* stream);
int spk_bn_bwd_finalize(const float* partial, int nblk, int C, double count, const float* gamma, const float* invstd,
                        float* dgamma, float* dbeta, float* coef /*[3][C]*/, int accumulate, double* ws,
                        const unsigned* amax_in, const unsigned* raw_amax, const float* mean, unsigned* est_out /* optional
                        (needs the three before it): the spk_bnbwd_estimate bound, per channel, by atomicMax - saves that launch */,
                        const unsigned* chan_amax /* optional [C] (spk_bn_bwd_reduce): the bound pairs every channel's own absmax
                        of dz with its own k1 instead of the tensor-wide *amax_in (which may then be NULL).  Needed where the
                        incoming gradient's range is unbounded per channel: the pooling layer's sqrt'(mean) at a tiny mean
                        (scripts/model.py:453) is huge exactly in channels whose BatchNorm gamma is tiny */,
                        void* stream);
int spk_bn_bwd_apply(const float* dy, const float* raw, const float* act, const float* mean, const float* invstd,
                     const float* scale, const float* shift, const float* coef, float* draw, float* dz_out, long long N,
                     int C, int mask_mode, unsigned* amax_out /* optional: atomicMax of the float bits of |draw| */,
                     const unsigned* pair_scale /* optional: draw is written as an f16 pair tensor (see SPK_IN_PRESPLIT) scaled
                     by the sigma of *pair_scale - the est_out slot of spk_bn_bwd_finalize */, void* stream);
/* operand-scale hand-offs of the f16x3 mode (see spk_conv_mfma): *slot = max(*slot, bits(max|x|)); and the RIGOROUS upper bound
 * max_c |k1_c| (A + |m1_c| + (R + |mean_c|) invstd_c |m2_c|) (1 + 2^-16) of the values k1 (dz - m1 - xhat m2) of a BatchNorm
 * backward - staged by a fused data gradient or written as an f16 pair tensor - from the coefficient rows coef[3][C] of
 * spk_bn_bwd_finalize, the BatchNorm's mean / invstd rows, A = the float in *amax_in (absmax of the incoming gradient, so
 * |dz| <= A) and R = the float in *raw_amax (absmax of the raw tensor, so |xhat| <= (R + |mean|) invstd) */
int spk_absmax(const float* x, unsigned* slot, long long n, void* stream);
int spk_bnbwd_estimate(const float* coef, const float* mean, const float* invstd, int C, const unsigned* amax_in,
                       const unsigned* raw_amax, unsigned* est, void* stream);
/* diagnostics of the f16x3 windows (debug / tests, never on the training path): counts[0] += values looked at, [1] += values
 * that saturate fp16 under the slot's scale (must stay 0), [2] += values whose low term is an fp16 subnormal (kept by the
 * matrix instruction: 11..22 significand bits, absolute error <= bound * 2^-39), [3] += values whose high term is subnormal.  The values are x (n floats, n % 4 == 0), or
 * max(x*scale[c]+shift[c], 0) with c = index % C when scale / shift are given, or - pairs != 0 - the stored terms of an f16
 * pair tensor. */
int spk_f16_window_count(const float* x, const float* scale, const float* shift, long long n, int C, const unsigned* slot,
                         int pairs, unsigned long long* counts /*[4], device*/, void* stream);
/* upper bound of |relu(raw * scale_c + shift_c)| from A = absmax(raw): max_c |scale_c| * A + max_c |shift_c| - the operand
 * scale input of a convolution / weight gradient that applies BatchNorm+ReLU while staging (SPK_IN_AFFINE_RELU) */
int spk_affine_estimate(const float* scale, const float* shift, int C, const unsigned* amax_in, unsigned* est, void* stream);

/* ---- squeeze-and-excitation (SELayer / SEBasicBlock, scripts/model.py:17-33,67-97; csrc/se.hip) ----------
 * Tensors are NHWC fp32 [B][H*W][C], C a power of two in [32, 1024]; the gate matrices are W1 [Cr][C] (se.fc.0.weight) and
 * W2 [C][Cr] (se.fc.2.weight), Cr <= 64, no biases.  z = scale_c raw + shift_c is the block's second BatchNorm (no ReLU).
 * Every reduction runs in a fixed order (fp32 inside a block of pixels, fp64 across blocks and utterances): no float atomics. */
/* reduction blocks per utterance: `partial` of spk_se_squeeze holds B * chunks * C floats, of spk_se_bwd_reduce twice that */
int spk_se_chunks(long long HW);
/* sums[b][c] = sum over the H*W pixels of x (AdaptiveAvgPool2d(1) before the division, :20,30); wlen (int32 [B], or NULL):
 * only the columns w < wlen[b] count */
int spk_se_squeeze(const float* x, float* partial, double* sums /*[B][C]*/, int B, int H, int W, int C, const int* wlen,
                   void* stream);
/* q = scale * sums / count + shift (scale = shift = NULL: q = sums / count), count = H * W or H * wlen[b];
 * u = relu(W1 q) [B][Cr]; g = sigmoid(W2 u) [B][C] (:21-26,31) - all three are kept for the backward pass */
int spk_se_excite(const double* sums, const float* scale, const float* shift, const float* W1, const float* W2, float* q,
                  float* u, float* g, int B, int C, int Cr, int H, int W, const int* wlen, void* stream);
/* out = [relu](g[b][c] * (raw * scale + shift) [+ res | + res * res_scale + res_shift]) (:33,94-95; scale = shift = NULL: the
 * identity affine).  mask_out / amax_out as in spk_bn_apply; wlen: pixels at width w >= wlen[b] are stored as 0 */
int spk_se_apply(const float* raw, const float* scale, const float* shift, const float* gate, const float* res,
                 const float* res_scale, const float* res_shift, float* out, unsigned* mask_out, int B, int H, int W, int C,
                 int relu, unsigned* amax_out, const int* wlen, void* stream);
/* S[b][0][c] = sum_hw e, S[b][1][c] = sum_hw e * raw with e = dout masked by `act` (mask_mode 1: the activated block output,
 * 3: its sign bits).  chan_amax ([C] zeros, or NULL): also the absmax of e per channel (float bits) */
int spk_se_bwd_reduce(const float* dout, const float* raw, const float* act, float* partial, double* S /*[B][2][C]*/, int B,
                      long long HW, int C, int mask_mode, unsigned* chan_amax, void* stream);
/* the gate's backward chain and the BatchNorm-backward finalize of dz = g e + dq / HW, from the [B][C] tables alone:
 * dg = scale S2 + shift S1, da = dg g (1 - g) [B][C], du = W2^T da [u > 0] [B][Cr], dq = W1^T du -> dq [2][B][C] = (dq, dq / HW);
 * dW1 = sum_b du (x) q, dW2 = sum_b da (x) u, dgamma, dbeta (overwritten, or added to when accumulate != 0);
 * coef [3][C] = (gamma invstd, mean dz, mean dz xhat) for spk_se_bwd_apply; est_out: atomicMax of the float bits of the bound
 * max_c |k1| (A + max_b |dq / HW| + |m1| + Xhat |m2|)(1 + 2^-16) of |draw|, A from amax_in (absmax of dout) or chan_amax,
 * Xhat = (R + |mean|) invstd with R from raw_amax - valid because 0 <= g <= 1 */
int spk_se_bwd_gate(const double* S, const double* sums, const float* q, const float* u, const float* g, const float* W1,
                    const float* W2, const float* mean, const float* invstd, const float* scale, const float* shift,
                    const float* gamma, float* da, float* du, float* dq, float* dW1, float* dW2, float* dgamma, float* dbeta,
                    float* coef, int accumulate, int B, int C, int Cr, long long HW, const unsigned* amax_in,
                    const unsigned* raw_amax, const unsigned* chan_amax, unsigned* est_out, void* stream);
/* draw = k1 (g e + dqs - m1 - xhat m2), as fp32 or (pair_scale) as an f16 pair tensor; e_out (may be dout itself, or NULL):
 * e = dout [out > 0], the shortcut gradient; amax_out: absmax of draw */
int spk_se_bwd_apply(const float* dout, const float* raw, const float* act, const float* gate, const float* dqs /*[B][C]*/,
                     const float* mean, const float* invstd, const float* coef, float* draw, float* e_out, int B, long long HW,
                     int C, int mask_mode, unsigned* amax_out, const unsigned* pair_scale, void* stream);

/* ---- statistics pooling (StatsPooling, scripts/model.py:435-457; mode 0 = 'mean', 1 = 'mean+std') -------- */
int spk_stats_pool_fwd(const float* x /*[B][H][W][C]*/, float* out /*[B][C*H*(1+mode)]*/, int B, int H, int W, int C,
                       int mode, void* stream);
/* per-image widths: row b pools over its first wlen[b] frames (DEVICE int array [B], clamped to [1, W]) with the same two-pass
 * arithmetic as spk_stats_pool_fwd at that width - 'mean+std' of one frame gives the unbiased variance 0/0 = NaN for that row */
int spk_stats_pool_fwd_len(const float* x, float* out, const int* wlen, int B, int H, int W, int C, int mode, void* stream);
int spk_stats_pool_bwd(const float* x, const float* gout, float* dx, int B, int H, int W, int C, int mode,
                       unsigned* amax_out /* optional: atomicMax of the float bits of |dx| */, void* stream);
/* Up to W = spk_stats_pool_row_cap() the two forward entries above load each row into registers once and run the same arithmetic
 * on it (bit-equal results); spk_stats_pool_row_form(0) selects the serial two-pass kernel at every width (A/B, tests), (1) gives
 * the default back.  Process-wide; returns the previous value. */
int spk_stats_pool_row_form(int on);
int spk_stats_pool_row_cap(void);

/* ---- half-precision extraction (precision="f16"; csrc/half.hip) -------------------------------------
 * Eval mode only.  Activations are NHWC fp16 tensors; a multiply-accumulate is ONE fp16 product on v_mfma_f32_16x16x32_f16 with
 * fp32 accumulation; the epilogue is fp32 and rounds once to fp16 (nearest even, subnormals kept).  A stored value outside
 * fp16's range is stored as +-inf and counted: every entry below ADDS the number of not-finite values it stored for image b to
 * ovf[b] (DEVICE int array [B], zeroed by the caller before the first launch of a forward).  Nothing is clamped.
 * wlen (may be NULL): DEVICE int array [B]; outputs of image b at width (time) x >= wlen[b] are stored as +0. */
/* bytes of a packed weight = 2 Cout Cin KH KW: 1 KB fragment images [KH*KW][Cin/32][Cout/16][lane 64][8 halfs], lane l element j =
 * w[16 m + (l & 15)][32 s + 8 (l >> 4) + j][tap] rounded to fp16.  Cin, Cout in {32, 64, 128, 256}, 1x1 or 3x3; rc < 0 otherwise */
int spk_h16_packed_bytes(int Cout, int Cin, int KH, int KW);
/* OIHW fp32 (Conv2d.weight, scripts/model.py:32-34,104-110) -> the packed fp16 form, rounded once to nearest even; a weight
 * outside fp16's range becomes +-inf (not refused) */
int spk_h16_pack_conv_weight(const float* w_oihw, void* out, int Cout, int Cin, int KH, int KW, void* stream);
/* the output tile of spk_h16_conv_fwd: rows (which = 0) and columns (which = 1); a block runs (which = 2) consecutive tiles, their
 * loads pipelined across tile boundaries, once a launch has (which = 3) or more (tile, output-channel tile) pairs, else one */
int spk_h16_conv_tile(int which);
/* stem conv1 + bn1 + ReLU in eval mode (scripts/model.py:249-251): the fp32 arithmetic of spk_stem_conv_fwd(_len) with
 * SPK_EPI_AFFINE | SPK_EPI_RELU, frames t >= wlen[b] read as 0; the result is stored as fp16 [B][F][T][32] */
int spk_h16_stem_fwd(const float* x, const float* w, const float* scale, const float* shift, void* out_f16, const int* wlen,
                     int* ovf, int B, int F, int T, void* stream);
/* conv + eval BatchNorm (+ residual) (+ ReLU) of a block (scripts/model.py:48-64,118-138): 3x3 pad 1 or 1x1 pad 0, stride 1 or 2,
 * NHWC fp16 in [B][IH][IW][Cin] -> out [B][ceil(IH/stride)][ceil(IW/stride)][Cout] fp16:
 *   v = acc * scale[c] + shift[c];  v += float(add[same address as out]) (add may be NULL);  relu: v = max(v, 0);  length mask;
 *   one rounding to fp16.  The sum over (tap, Cin) is never split across blocks. */
int spk_h16_conv_fwd(const void* in_f16, const void* wpk, const float* scale, const float* shift, const void* add_f16,
                     void* out_f16, const int* wlen, int* ovf, int B, int IH, int IW, int Cin, int Cout, int ksize, int stride,
                     int relu, void* stream);
/* StatsPooling (scripts/model.py:435-457) of an fp16 map in fp32: the formulas and the two-pass order of spk_stats_pool_fwd(_len),
 * swapped var / sqrt(mean) outputs included; wlen (may be NULL) as in spk_stats_pool_fwd_len.  out: fp32 [B][C*H*(1+mode)] */
int spk_h16_stats_pool_fwd(const void* in_f16, float* out, const int* wlen, int B, int H, int W, int C, int mode, void* stream);

/* ---- GEMM (fc1 = nn.Linear(5120,256) scripts/model.py:357; cosine F.linear :485; their gradients) ------ */
/* C[m][n] = alpha * sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn] (+ bias[n]) (+ C[m][n]).  64x64 tiles on the fp32 matrix
 * instruction, K cut into spk_gemm_splitk(M,N,K) slices whose partial tiles go through `workspace`
 * (spk_gemm_workspace(M,N,K) bytes, caller-owned) and are folded in a fixed order. */
int spk_gemm_splitk(int M, int N, int K);
size_t spk_gemm_workspace(int M, int N, int K);
int spk_gemm_f32(const float* A, const float* B, float* C, const float* bias, int M, int N, int K, long long sam,
                 long long sak, long long sbk, long long sbn, long long ldc, float alpha, int accumulate, float* workspace,
                 void* stream);
int spk_colsum(const float* dy, float* db, int M, int N, int accumulate, void* stream);

/* ---- heads ------------------------------------------------------------------------------------------- */
/* F.normalize rows (scripts/model.py:485) and its gradient */
int spk_l2norm_fwd(const float* x, float* y, float* inv_norm, int R, int D, float eps, void* stream);
int spk_l2norm_bwd(const float* y, const float* inv_norm, const float* dy, float* dx, int R, int D, float eps,
                   int accumulate, void* stream);
/* AAM margin on the label column + scale (scripts/model.py:487-499) and its gradient */
int spk_aam_margin_fwd(const float* cosv, const long long* label, float* logits, int B, int S, float m, float s,
                       void* stream);
int spk_aam_margin_bwd(const float* cosv, const long long* label, const float* dlogits, float* dcos, int B, int S,
                       float m, float s, void* stream);
/* nn.CrossEntropyLoss rows (scripts/train_resnet.py:201,317): loss_row, dlogits = (softmax-onehot)*grad_scale,
 * rank[b] = #{j: logit_j > logit_label} (scripts/accuracy.py:4-16: correct@k <=> rank < k) */
int spk_softmax_ce(const float* logits, const long long* label, float* loss_row, float* dlogits, int* rank, int B, int S,
                   float grad_scale, void* stream);
int spk_mean(const float* v, float* out, int n, void* stream);
int spk_relu_bwd(const float* y, const float* dy, float* dx, long long n, void* stream);

/* ---- optimizer (torch.optim.SGD, scripts/train_resnet.py:203-205,328) ------------------------------------ */
int spk_sgd_step(float* p, const float* g, float* buf, long long n, float lr, float momentum, float weight_decay,
                 float grad_scale, int first_step, void* stream);

/* ---- cosine scoring back end (the step after the path) ----------------- */
/* out[n] = (emb[n] - mean) / max(||emb[n] - mean||, eps): mean subtraction of scripts/cosine_score.py:52-60 followed by
 * the normalisation inside F.cosine_similarity (:62, eps 1e-8) / F.normalize (scripts/compute_topk_mean_std.py:13,16) */
int spk_center_normalize(const float* emb /*[N][D]*/, const float* mean /*[D] or NULL*/, float* out, int N, int D, float eps,
                         void* stream);
/* out[t] = <en[ia[t]], te[ib[t]]> over normalised rows: the per-trial loop of scripts/cosine_score.py:57-65 */
int spk_trial_cosine(const float* en /*[n_en][D]*/, const float* te /*[n_te][D]*/, const int* ia, const int* ib, float* out,
                     int T, int D, int n_en, int n_te, void* stream);
/* per row of scores[N][M] (row pitch ld): mean and unbiased std of the k largest entries, M <= 16384
 * (scripts/compute_topk_mean_std.py:18-21: scores.topk(300), torch.std_mean) */
int spk_topk_mean_std(const float* scores, float* mean_out, float* std_out, int N, int M, int k, long long ld, void* stream);

/* ---- evaluation stage (csrc/eval.hip): speaker-mean cohort, S-norm per trial, error-rate sweep --------
 * Everything here reproduces the reference's Python expressions bit for bit: fp64 (fp32 where numpy uses it), every operation
 * rounded on its own (no fused multiply-add), a fixed order wherever the order shows in the result. */
/* which = 0: pairs one block of spk_sort_trials sorts in LDS; 1: positions per block of spk_error_sweep's scan */
int spk_eval_tile(int which);
/* out[s][d] = mean over the rows rows[seg_off[s] .. seg_off[s + 1]) of emb, accumulated in that order as
 * acc = (float)((double)acc + emb[r][d]) and divided as acc / (float)count: numpy's float32 += float64 and /= int of
 * scripts/compute_speaker_mean.py:15-27.  rows: row indices grouped by speaker, archive order inside a speaker. */
int spk_segment_mean(const double* emb /*[N][D]*/, const int* rows /*[N]*/, const int* seg_off /*[S+1]*/, float* out /*[S][D]*/,
                     int N, int S, int D, void* stream);
/* out[t] = (s - e_mean[ia[t]]) / max(e_std[ia[t]], 1e-8) / 2 + (s - t_mean[ib[t]]) / max(t_std[ib[t]], 1e-8) / 2 in fp64 with
 * s = (double)score[t]: scripts/adaptive_snorm.py:28-35.  score: float [T] (score_f64 = 0: what spk_trial_cosine wrote) or
 * double [T] (score_f64 = 1: what a score file holds). */
int spk_trial_snorm(const void* score, int score_f64, const int* ia, const int* ib, const double* e_mean, const double* e_std,
                    const double* t_mean, const double* t_std, double* out, int T, void* stream);
/* order[T]: the permutation that sorts score[T] ascending, equal scores (-0.0 equals +0.0) in index order - Python's stable
 * sorted(enumerate(scores), key=itemgetter(1)) of scripts/compute_eer.py:40-42 and local/compute_min_dcf.py:59-61.  No NaN
 * (the caller checks).  1 <= T < 2^31; ws: spk_sort_trials_workspace(T) bytes. */
size_t spk_sort_trials_workspace(int T);
int spk_sort_trials(const double* score, unsigned* order, void* ws, int T, void* stream);
/* ComputeErrorRates + the EER of scripts/compute_eer.py:35-70,101-102 and ComputeMinDcf of local/compute_min_dcf.py:54-106 for
 * P <= 8 cost triples costs[P][3] = (p_target, c_miss, c_fa) (device memory), over label[T] (0 / 1) taken through order:
 *   out_d = eer, then (minDCF, threshold = the score at its position) per triple;
 *   out_i = position of the EER, targets, non-targets, then the position of the minimum per triple (lowest position on ties).
 * Both classes must be present (the caller checks).  ws: spk_error_sweep_workspace(T, P) bytes. */
size_t spk_error_sweep_workspace(int T, int P);
int spk_error_sweep(const double* score, const unsigned char* label, const unsigned* order, const double* costs, int P,
                    double* out_d /*[1+2P]*/, long long* out_i /*[3+P]*/, void* ws, int T, void* stream);

/* ---- feature front end (csrc/frontend.hip; DESIGN.md "Feature front end") ------------------------------------------------
 * Replaces the Kaldi binaries of stage 1 of the reference's feature_pre.sh:77-104 (compute-fbank-feats with conf/fbank.conf,
 * compute-vad with conf/vad.conf) and local/nnet3/xvector/prepare_feats_for_egs.sh:68-70 (apply-cmvn-sliding --norm-vars=false
 * --center=true --cmn-window=300 | select-voiced-frames); the fbank as restated in the reference's kaldi.py:42-188,363-527. */
/* frames per workgroup tile of spk_fbank_fwd for these sizes (0: they do not fit the LDS tile) */
int spk_fbank_tile_frames(int L, int S, int P, int F);
/* wave [B][Nmax] (int16-scale samples), nsamp[B] (device): log-mel feats [B][F][Tcap] (time innermost, 0 for t >= T[b]), raw log
 * energies log_energy [B][Tcap] (0 past T[b]) and T_out[b] = the frame count (frames >= Tcap are not computed: Tcap >= max T).
 * window [L], twiddle [P/2][2] = exp(-2 pi i k / P), mel_w / mel_lo [F] / mel_off [F+1] (filter m: weights mel_w[mel_off[m] ..
 * mel_off[m+1]) on FFT bins mel_lo[m] ..) are device tables built by the host in fp64.  P: power of two <= 1024, L <= P.
 * dither != 0 draws N(0,1) noise keyed by (seed, utt_ids[b], frame, position); energy_floor == 0: no floor. */
int spk_fbank_fwd(const float* wave, const int* nsamp, const long long* utt_ids, int B, long long Nmax, const float* window,
                  const float* twiddle, const float* mel_w, const int* mel_lo, const int* mel_off, int L, int S, int P, int F,
                  int snip_edges, float dither, float preemph, int remove_dc, float energy_floor, unsigned long long seed,
                  float* feats, float* log_energy, int* T_out, int Tcap, void* stream);
/* compute-mfcc-feats in one launch: replaces `local/make_mfcc.sh:107,126` of the reference's recipe (feature_pre.sh:92-103,
 * run.sh:74-85 with conf/mfcc.conf), the MFCC as restated in the reference's kaldi.py:550-650.
 * frames per workgroup tile for these sizes (0: the tile of C + 1 rows and the DCT copy [C][F | 1] do not fit its LDS) */
int spk_mfcc_tile_frames(int L, int S, int P, int F, int C);
/* As spk_fbank_fwd up to the log-mel values lm[0 .. F) of a frame (the same operations in the same order; the same dither draws),
 * then c[k] = sum_n dct[k][n] * lm[n] (n ascending) for k < C, c[k] *= lifter[k]; use_energy: c[0] = the raw log energy (floored
 * by log(energy_floor) when > 0); htk_compat: row k - 1 gets c[k] for k >= 1, row C - 1 gets c[0] (times sqrt 2 without
 * use_energy).  dct [C][F] and lifter [C] are device tables built by the host in fp64 (lifter: ones for cepstral_lifter 0).
 * feats [B][C][Tcap] (time innermost, 0 for t >= T[b]), log_energy [B][Tcap] (always written), T_out[b].  1 <= C <= F <= P. */
int spk_mfcc_fwd(const float* wave, const int* nsamp, const long long* utt_ids, int B, long long Nmax, const float* window,
                 const float* twiddle, const float* mel_w, const int* mel_lo, const int* mel_off, const float* dct,
                 const float* lifter, int L, int S, int P, int F, int C, int snip_edges, float dither, float preemph, int remove_dc,
                 float energy_floor, int use_energy, int htk_compat, unsigned long long seed, float* feats, float* log_energy,
                 int* T_out, int Tcap, void* stream);
/* The span form of the two launches above, for training from audio.  Replaces the feature directories that
 * stages 3 and 4 of the reference's feature_pre.sh:178-196 write (fbank of the augmented copies, then the combined set once more
 * through local/nnet3/xvector/prepare_feats_for_egs.sh:68-71) only for the training loader to crop them: the frames of a crop are
 * computed from the audio of the crop.  Row b of wave [B][Nmax] holds samples first[b] .. first[b] + nsamp[b] - 1 of an utterance
 * of total[b] samples; the launch computes frames frame0[b] .. frame0[b] + nframes[b] - 1 OF THAT UTTERANCE into columns
 * 0 .. nframes[b] - 1 (nframes clipped to the utterance's frame count; T_out[b] = the columns written, zeros up to Tcap).  The
 * snip_edges = false reflection is about 0 and total[b], the dither is keyed by the frame's index in the utterance: column j equals
 * column frame0[b] + j of the whole-utterance launch bit for bit.  A computed frame must not touch a sample outside the row after
 * reflection (the caller checks; the kernel clamps such a read into the row).  first / total: int64, frame0 / nframes: int32,
 * all device arrays of B. */
int spk_fbank_span_fwd(const float* wave, const int* nsamp, const long long* first, const long long* total, const int* frame0,
                       const int* nframes, const long long* utt_ids, int B, long long Nmax, const float* window, const float* twiddle,
                       const float* mel_w, const int* mel_lo, const int* mel_off, int L, int S, int P, int F, int snip_edges,
                       float dither, float preemph, int remove_dc, float energy_floor, unsigned long long seed, float* feats,
                       float* log_energy, int* T_out, int Tcap, void* stream);
/* the MFCC of a span (feature_pre.sh:178-196 run with local/make_mfcc.sh, prepare_feats_for_egs.sh:68-71): as above, with the
 * cepstral arguments of spk_mfcc_fwd */
int spk_mfcc_span_fwd(const float* wave, const int* nsamp, const long long* first, const long long* total, const int* frame0,
                      const int* nframes, const long long* utt_ids, int B, long long Nmax, const float* window, const float* twiddle,
                      const float* mel_w, const int* mel_lo, const int* mel_off, const float* dct, const float* lifter, int L, int S,
                      int P, int F, int C, int snip_edges, float dither, float preemph, int remove_dc, float energy_floor,
                      int use_energy, int htk_compat, unsigned long long seed, float* feats, float* log_energy, int* T_out, int Tcap,
                      void* stream);
/* 16-bit PCM as it lies in a WAV file (what the readers of compute-fbank-feats in feature_pre.sh:178-196 convert on the host):
 * out[b][s] = (float) pcm[b][s] for s < count[b], 0 up to Nmax - float32 at int16 scale, the input of the launches above */
int spk_pcm16_to_f32(const short* pcm /*[B][Nmax]*/, const int* count /*[B]*/, int B, long long Nmax, float* out /*[B][Nmax]*/,
                     void* stream);
/* out[f][j] = the N(0,1) draw spk_fbank_fwd / spk_mfcc_fwd adds (times dither) at position j of frame frame0 + f of utterance utt_id */
int spk_fbank_dither_noise(float* out /*[nframes][L]*/, long long utt_id, unsigned long long seed, int frame0, int nframes, int L,
                           void* stream);
/* compute-vad over log_energy [B][Tcap] (T[b] frames): vad[b][t] in {0, 1} (0 past T), idx[b][0 .. count[b]) = the voiced
 * frames in order, count[b].  thr = energy_threshold + mean_scale * mean(log E) (fp64); voiced iff #{t2 in the clipped context
 * window : logE > thr} >= proportion * #window */
int spk_vad_count(const float* log_energy, const int* T, int B, int Tcap, double energy_threshold, double mean_scale,
                  int frames_context, double proportion, int* vad /*[B][Tcap]*/, int* idx /*[B][Tcap]*/, int* count /*[B]*/,
                  void* stream);
/* VAD decisions -> speech segments, the step in front of windowed extraction for diarization (the role of
 * Kaldi's diarization/vad_to_segments.sh, but the rule below is this project's contract, not a port).  Row b has T[b] frames
 * (clamped to [0, Tcap]); frame t is voiced iff vad[b][t] != 0.  padding p >= 0, max_gap g >= 0, min_length m >= 1, in frames:
 *   1. runs: the maximal intervals [s_i, e_i) of voiced frames, ascending;
 *   2. padding: a_i = max(0, s_i - p), b_i = min(T, e_i + p);
 *   3. run 0 opens a segment; run i > 0 opens a new one iff a_i - b_{i-1} > g, else it joins the current one (also when the
 *      padded runs overlap).  A segment is [a of its opening run, b of its last run);
 *   4. a segment with b - a < m is dropped, the others are emitted in order.
 * nseg[b] = the number of emitted segments of row b, also when it exceeds Scap; seg[b][0 .. min(nseg[b], Scap)) = their
 * (start, end) pairs, every other word of seg is left as it was.  Integers only: the same bits on every run, wherever a row sits
 * in the batch.  Refused before any launch (rc < 0): negative B / Tcap / padding / max_gap / Scap, Tcap > 2^31 - 1025,
 * min_length < 1, and with B > 0 a NULL T or nseg, a NULL vad with Tcap > 0, a NULL seg with Scap > 0.  B == 0 returns 0 without
 * a launch. */
int spk_vad_segments(const int* vad /*[B][Tcap] device*/, const int* T /*[B] device*/, int B, int Tcap, int padding, int max_gap,
                     int min_length, int* seg /*[B][Scap][2] device: start, end*/, int Scap, int* nseg /*[B] device*/,
                     void* stream);
/* centred sliding CMN (window cmn_window, fp64 sums; 0 = none) of x [B][F][Tcap] over T[b] frames, then the frames idx[b][0 ..
 * count[b]) (idx and count NULL: all T[b] frames) compacted into out [B][F][Tout] with zero tails.  prefix: fp64 workspace of
 * B * F * (Tcap + 1) doubles (may be NULL when cmn_window == 0). */
int spk_cmn_select(const float* x, const int* T, const int* idx, const int* count, double* prefix, float* out, int B, int F,
                   int Tcap, int Tout, int cmn_window, void* stream);

/* ---- resampling (csrc/resample.hip; DESIGN.md "Feature front end", "Resampling") -------------------------------------------
 * Replaces the reference's kaldi.py: resample_waveform (Kaldi's LinearResample / ResampleWaveform, what compute-fbank-feats
 * --allow-downsample / --allow-upsample runs), and with fi = speed x rate the resampling half of
 * local/perturb_data_dir_speed.sh.  g = gcd(fi, fo), iu = fi / g, ou = fo / g. */
/* outputs per workgroup tile of spk_resample_fwd for a table of ou phases x K taps (0: table + span do not fit its LDS) */
int spk_resample_tile(int iu, int ou, int K);
/* wave_in [B][Nmax_in] (int16-scale samples), nsamp_in[B] (device) -> wave_out [B][Nmax_out], nsamp_out[b] =
 * ceil(nsamp_in[b] * ou / iu) (LinearResample::GetNumOutputSamples; Nmax_out must hold the longest row), zeros past it:
 *     wave_out[b][j] = sum_{k < K} w[j % ou][k] * wave_in[b][first[j % ou] + (j / ou) * iu + k],  0 outside [0, nsamp_in[b])
 * summed in fp32 in tap order.  first [ou] and the windowed-sinc weights are device tables built by the host in fp64; the weights
 * come as pairs of consecutive taps, phase running fastest: wq [ceil(K / 2)][ou][2], wq[m][p] = (w[p][2m], w[p][2m + 1]), with a
 * zero for the tap an odd K lacks.  Refused before any launch: fi == fo, and a table beyond the LDS budget (the message names
 * fi -> fo). */
int spk_resample_fwd(const float* wave_in, const int* nsamp_in, int B, long long Nmax_in, const int* first, const float* wq,
                     int fi, int fo, int K, float* wave_out, int* nsamp_out, long long Nmax_out, void* stream);

/* ---- augmentation (csrc/augment.hip) -------------------------------------------------------------------
 * Replaces the wav-reverberate commands of stages 2 and 3 of the reference's feature_pre.sh:109-167: the entries that
 * steps/data/reverberate_data_dir.py:345,365 (--shift-output=true --impulse-response) and steps/data/augment_data_dir.py:112
 * (--shift-output=true --additive-signals --start-times --snrs; :87-88 the --duration of a background item) write into wav.scp. */
/* longest impulse response (feature_pre.sh:128 --rir-set-parameter; reverberate_data_dir.py:345 --impulse-response) and longest
 * early part (int(0.001 fs) + int(0.05 fs) samples) a call takes */
int spk_augment_max_rir(void);
int spk_augment_max_early(void);
/* element counts of the three workspaces of spk_augment_fwd for these maxima: sizes[0] float2 spectra, sizes[1] float y,
 * sizes[2] double sums.  Rmax / Emax: longest impulse response / early part (0: no row has one), Fmax: longest filled noise,
 * nd: descriptors.  Refuses Rmax beyond spk_augment_max_rir(). */
int spk_augment_workspace(int B, long long Nmax, int Rmax, int Emax, long long Fmax, int nd, long long* sizes /*[3]*/);
/* wave [B][Nmax] (int16-scale samples), nsamp[B] (device) -> out [B][Nmax], zeros past nsamp[b], and clipped[b] += the samples
 * quantize != 0 (truncation toward zero, then [-32768, 32767]: what a 16-bit WAV pipe carries) clipped; clipped must come zeroed.
 * Row b: impulse response rir_pool[rir_off[b] .. + R), rir_row[b] = {R (0: none), peak s, early start e0, early length E}
 * (reverberate_data_dir.py:345 --impulse-response, :365 --shift-output=true: out[j] = g y[j + s]); additive signals
 * desc_ptr[b] .. desc_ptr[b + 1] in order, descriptor d = noise_pool[desc_off[d] .. + raw), desc_len[d] = {raw length, filled
 * length D (augment_data_dir.py:87-88 --duration: the signal repeated or cut to D; else D = raw), start sample
 * (augment_data_dir.py:112 --start-times)}, desc_snr[d] in dB (augment_data_dir.py:112 --snrs).  The formulas: csrc/augment.hip.
 * twiddle [1024][2] = exp(-2 pi i k / 2048), built by the host in fp64.  All sums of squares in fp64 in a fixed order. */
int spk_augment_fwd(const float* wave, const int* nsamp, int B, long long Nmax, const float* rir_pool, long long rir_pool_len,
                    const long long* rir_off, const int* rir_row, int Rmax, int Emax, const float* noise_pool,
                    long long noise_pool_len, const int* desc_ptr, const long long* desc_off, const int* desc_len,
                    const double* desc_snr, int nd, long long Fmax, const float* twiddle, float* spectra, float* y, double* work,
                    int quantize, float* out, unsigned long long* clipped, void* stream);

/* ---- Kaldi's one-byte compressed matrices (csrc/cm.hip) -------------------------------------------------
 * The 'CM ' format that Kaldi's feature scripts write by default (the reference reads it in scripts/kaldi_io.py:427-460): per
 * matrix (min, range), per column four 16-bit points (p0, p25, p75, p100), one byte per value, column-major.  All arithmetic in
 * fp32, every operation rounded on its own:  U(p) = min + (range * 1.52590218966964e-05f) * p,  P = U(p), and a code c stands for
 *   c <= 64: P0 + (P25 - P0) * c * (1/64.f);  c <= 192: P25 + (P75 - P25) * (c - 64) * (1/128.f);
 *   else P75 + (P100 - P75) * (c - 192) * (1/63.f). */
/* codes [B][F][T] (libspkio: spk_ark_read_crop_codes / _padded_codes), colhdr [B][F][4] = P (16-byte aligned), lengths [B] or
 * NULL -> out [B][F][T] fp32 (4-byte aligned), 0 for t >= lengths[b].  The bits the host readers give. */
int spk_cm_decode(const unsigned char* codes, const float* colhdr, const int* lengths, int B, int F, int T, float* out, void* stream);
/* x [B][F][Tcap], T[b] frames of row b (0 <= T[b] <= Tcap; nothing past T[b] is read) -> per row the parts of the record of its
 * [T[b]][F] matrix: minrange [B][2], hdr [B][F][4] (the 16-bit points as ints), codes [B][F][Tcap] (t < T[b] written, the rest
 * untouched).  T[b] == 0 writes nothing for b.  A row holding a non-finite value, or whose range overflows, gets minrange (NaN, NaN)
 * and nothing else.  ws: B * F * 2 floats.  Points: with s the sorted column and q = T / 4, (s[0], s[q], s[3q], s[T - 1]) for
 * T >= 5 and (s[0], s[1], s[2], s[3]) below, through Q(v) = (int)(clamp((v - min) / range, 0, 1) * 65535 + 0.499f) and kept
 * strictly increasing; found by a radix select, so T is not bounded by LDS. */
int spk_cm_compress(const float* x, const int* T, int B, int F, int Tcap, float* ws, float* minrange, int* hdr, unsigned char* codes,
                    void* stream);

/* ---- PLDA back end (csrc/plda.hip) ---------------------------------------------------------------------
 * The passes over embedding tables and the trial loop of Kaldi's ivector-compute-lda, transform-vec, ivector-normalize-length,
 * ivector-compute-plda and ivector-plda-scoring.  All sums in fp64 in a fixed order (no floating-point atomics); the two matrix
 * kernels run on v_mfma_f64_16x16x4_f64.  1 <= D, Di, Do <= 512.  The D x D factorisations stay on the host. */
/* rows per slab of spk_scatter_f64 for N rows (0: N out of range), and the bytes of its workspace (0: bad arguments) */
int spk_scatter_slab_rows(long long N);
size_t spk_scatter_f64_workspace(long long N, int D);
/* C[D][D] = sum_i w[i] (x_i - mu)(x_i - mu)^T over the rows X[N][ld] (float, or double with x_f64; ld >= D); mu double[D] or NULL
 * (zero), w double[N] or NULL (ones).  Kaldi: the total covariance and the class-mean scatter of CovarianceStats::AccStats
 * (ivector-compute-lda.cc) and the offset scatter of PldaStats::AddSamples (plda.cc).  Output tiles come from the upper triangle
 * and are mirrored (C == C^T bit for bit); rows are split into slabs of spk_scatter_slab_rows(N) whose partial sums a second pass
 * adds in slab order.  ws: spk_scatter_f64_workspace(N, D) bytes. */
int spk_scatter_f64(const void* X, int x_f64, long long ld, const double* mu, const double* w, double* C, void* ws, long long N, int D,
                    void* stream);
/* out[k][d] = sum of X[r][d] over r = rows[seg_off[k] .. seg_off[k + 1]) in list order (rows NULL: r itself), in fp64, divided by the
 * number of rows when mean != 0; count[k] (or NULL) = the number of rows.  X float or double (x_f64), row pitch ld.  Kaldi: the per-speaker sums of CovarianceStats::AccStats
 * and PldaStats::AddSamples.  (spk_segment_mean keeps the float32 accumulator of the reference's cohort script.) */
int spk_segment_sum_f64(const void* X, int x_f64, long long ld, const int* rows, const int* seg_off /*[K+1]*/, double* out /*[K][D]*/,
                        int* count /*[K]*/, int mean, int K, int D, void* stream);
/* Y[i] = s_i (A x_i + b): A double[Do][Di] (NULL: the identity, Di == Do), b double[Do] or NULL; scale = 0: s_i = 1; else
 * s_i = sqrt(Do / sum_j y_j^2 q_j) with y = A x_i + b and q double[Do] (NULL: ones), and a row whose sum is 0 keeps s_i = 1.
 * X [N][ldx] float or double (x_f64); Y [N][Do] float (rounded once from fp64) or double (y_f64).  Kaldi: transform-vec,
 * ivector-normalize-length, Plda::TransformIvector with its normalisation factor (q_j = 1 / (psi_j + 1 / n)). */
int spk_affine_lennorm(const void* X, int x_f64, long long ldx, const double* A, const double* b, const double* q, int scale, void* Y,
                       int y_f64, long long N, int Di, int Do, void* stream);
/* One EM iteration of PldaEstimator::GetStatsFromClassMeans in the basis where W = I and B = diag(psi): for class k with count[k]
 * utterances and centred mean mt[k], w_out[k][j] = count[k] psi[j] / (count[k] psi[j] + 1) * mt[k][j] and r_out = mt - w_out. */
int spk_plda_posterior_rows(const double* mt /*[K][D]*/, const int* count, const double* psi, double* w_out, double* r_out, int K,
                            int D, void* stream);
/* Plda::LogLikelihoodRatio per trial: with e = en[ia[t]], x = te[ib[t]], n = count[ia[t]] (count NULL: 1),
 * c_j = n psi_j / (n psi_j + 1), v_j = 1 + psi_j / (n psi_j + 1):
 *   out[t] = (float)(sum_j 0.5 (x_j^2 / (psi_j + 1) - (x_j - c_j e_j)^2 / v_j) + 0.5 (L1 - L0)),
 * (L0, L1) = tab_log[u] = (sum_j log v_j, sum_j log(psi_j + 1)) of the entry with tab_count[u] == n (U entries, built by the host;
 * NaN when n is not in the table).  psi_j = 0 contributes exactly 0. */
int spk_plda_llr(const double* en /*[n_en][D]*/, const double* te /*[n_te][D]*/, const int* ia, const int* ib, const double* psi,
                 const int* count /*[n_en]*/, const int* tab_count /*[U]*/, const double* tab_log /*[U][2]*/, int U, float* out,
                 int T, int D, int n_en, int n_te, void* stream);

/* ---- windowed extraction (csrc/window.hip) ---------------------------------------------------------------
 * A plan of N windows over a padded batch src [B][F][T] (fp32): window i is the frames [start[i], start[i] + len[i]) of row[i].
 * out [N][F][Wcap]: out[i][f][j] = src[row[i]][f][start[i] + j] for j < len[i] and +0 for len[i] <= j < Wcap - the slices bit for
 * bit.  row, start, len: the plan on the HOST, checked before anything is launched - row outside [0, B), start < 0, len < 1,
 * start + len > T and len > Wcap are refused (< 0, out untouched); plan_dev: the same three arrays on the device, int [3][N] (row,
 * start, len), which the kernel reads.  16-byte stores when Wcap % 4 == 0 and out is 16-byte aligned, 16-byte loads where a
 * window's start allows them, 4-byte accesses otherwise; N * F < 2^31. */
int spk_window_gather(const float* src, int B, int F, int T, const int* row /*host [N]*/, const int* start /*host [N]*/,
                      const int* len /*host [N]*/, const int* plan_dev /*device [3][N]*/, float* out, int N, int Wcap, void* stream);
/* out[u][d] = (sum_r weight[r] emb[r][d]) * (1.0f / sum_r weight[r]) over the rows r = seg_off[u] .. seg_off[u + 1] - 1 of
 * emb [N][D], in that order: acc = fmaf(weight[r], emb[r][d], acc) and tot += weight[r] in fp32, the reciprocal correctly rounded.
 * seg_off: host int [U + 1], checked before the launch (0 = seg_off[0] < ... < seg_off[U] = N: an empty segment is refused);
 * seg_off_dev: the same on the device.  One lane per (u, d), no atomics. */
int spk_window_mean(const float* emb /*[N][D]*/, int N, int D, const int* seg_off /*host [U+1]*/, const int* seg_off_dev,
                    const float* weight /*[N]*/, float* out /*[U][D]*/, int U, void* stream);

/* ---- diarization back end (csrc/diar.hip) -----------------------------------------------------------------
 * A batch of R recordings: recording r owns the rows rec_off[r] .. rec_off[r + 1] - 1 (n_r of them) of every [Ntot] table, an
 * n_r x n_r matrix at element offset mat_off[r] = sum over r' < r of n_r'^2, and T_r (T_r + 1) / 2 tiles (T_r = ceil(n_r / 16)) from
 * tile_off[r] on.  rec_off is a HOST int64 array [R + 1], checked before anything is launched: it must start at 0, be strictly
 * increasing (no empty recording) and end at Ntot, and the sum of n_r^2 must stay below 2^31; otherwise the call returns < 0 and
 * writes nothing.  The kernels read the tables from tab_dev: the device copy of what spk_diar_tables wrote. */
/* host only: tab [3][R + 1] = rec_off, mat_off, tile_off (the last entries: Ntot, sum n^2, all tiles) */
int spk_diar_tables(const long long* rec_off /*host [R+1]*/, int R, long long Ntot, long long* tab /*host [3][R+1]*/);
/* q[i] = scale * sum_d k[d] U[i][d]^2 in fp64, one wave per row: lane l adds d = l, l + 64, ... in order and the 64 partial sums
 * meet in a butterfly.  The PLDA setting of spk_score_dense: k_d = psi_d^2 / ((psi_d + 1)(2 psi_d + 1)), scale = -0.5. */
int spk_score_dense_q(const double* U /*[N][D]*/, const double* k /*[D]*/, double scale, double* q /*[N]*/, long long N, int D,
                      void* stream);
/* out[mat_off[r] + i n_r + j] = (float)(q[a] + q[b] + K + sum_d g[d] U[a][d] U[b][d]), a = rec_off[r] + i, b = rec_off[r] + j, for
 * every pair of rows of every recording: fp64 on v_mfma_f64_16x16x4_f64, one rounding to float.  16 x 16 tiles of the upper triangle,
 * every value stored at (i, j) and (j, i): out is symmetric bit for bit, and nothing outside the R matrices is written.
 * 1 <= D <= 512 (padded with zeros in registers), any n_r >= 1.  PLDA with both sides counted once (U: the projected,
 * length-normalised rows Plda::TransformIvector gives): g_d = psi_d / (2 psi_d + 1), q as above,
 * K = 0.5 sum_d (log(psi_d + 1) - log(1 + psi_d / (psi_d + 1))): Plda::LogLikelihoodRatio(u_i, 1, u_j) as spk_plda_llr states it.
 * Cosine: q = 0, K = 0, g = 1, U the unit rows. */
int spk_score_dense(const double* U /*[Ntot][D]*/, const long long* rec_off /*host [R+1]*/, const long long* tab_dev /*[3][R+1]*/,
                    const double* q /*[Ntot]*/, const double* g /*[D]*/, double K, float* out, long long Ntot, int D, int R,
                    void* stream);
/* threads of the workgroup that clusters one recording, and the largest n_r spk_ahc_batch takes (8192) */
int spk_ahc_threads(void);
int spk_ahc_max_n(void);
/* Average-linkage agglomerative clustering of every recording of the batch, one workgroup each (no workgroup waits on another).
 * S: the float matrices as spk_score_dense lays them out; only the upper triangles are read.  cost(i, j) = -(double)S[i][j]; C holds
 * summed pairwise costs, m the cluster sizes.  While more than max(min(min_clusters[r], n_r), 1) clusters are active: over the active
 * pairs i < j take the smallest c = C[i][j] / ((double)m_i (double)m_j), compared with c < best from best = +inf (a NaN or +inf never
 * wins), ties to the smallest i, then the smallest j; stop if there is none, or if c <= -threshold[r] does not hold
 * (threshold[r] = -inf: no threshold); else record (i, j, c), C[i][k] += C[j][k] for every other active k, m_i += m_j, j leaves.
 * labels[rec_off[r] + w]: 1, 2, ... numbering the final clusters by their lowest member.  merges [Ntot][2] and merge_cost [Ntot]:
 * recording r uses the slots from rec_off[r], n_merges[r] of them.  ws: ws_elems >= sum n_r^2 doubles (the kernel builds its table
 * there).  Refused on the host (< 0, nothing written): a bad rec_off, n_r > spk_ahc_max_n(), a workspace that is too small. */
int spk_ahc_batch(const float* S, const long long* rec_off /*host [R+1]*/, const long long* tab_dev /*[3][R+1]*/,
                  const int* min_clusters /*[R]*/, const double* threshold /*[R]*/, double* ws, long long ws_elems, int* labels /*[Ntot]*/,
                  int* merges /*[Ntot][2]*/, double* merge_cost /*[Ntot]*/, int* n_merges /*[R]*/, long long Ntot, int R, void* stream);

/* ---- VBx resegmentation (csrc/diar.hip) ---------------------------------------------------------------------
 * A variational-Bayes HMM over the window rows of every recording of a batch (the layout above), one workgroup per recording (no
 * workgroup waits on another), fp64 throughout.  X [Ntot][D]: rows in the space where the within-class covariance is I; Phi [D] >= 0:
 * the between-class variances.  One Smax per launch: gamma [Ntot][Smax] (in: initial responsibilities, out: the last ones), pi
 * [R][Smax] (in and out), n_states[r] in [1, Smax]: columns at or beyond n_states[r] are not read and are written as 0.  The rule
 * (rho = X sqrt(Phi), G_t = -0.5 (sum_d X_td^2 + D log 2 pi); per iteration N_s, invL_sd = 1 / (1 + Fa/Fb N_s Phi_d), alpha_sd,
 * logp_ts, forward-backward under tr_ij = loopP [i == j] + (1 - loopP) pi_j, ELBO_it = tll + 0.5 Fb sum_sd (log invL_sd - invL_sd -
 * alpha_sd^2 + 1), the pi update, and the stop after iteration it > 0 with ELBO_it - ELBO_{it-1} < epsilon; epsilon = -inf: never)
 * is stated in full in DESIGN.md section 6o.  elbo [R][max_iters]: recording r writes its first n_iters[r] slots and leaves the rest.
 * A state whose prior is below 2^-900 is taken to have prior 0: its gamma is 0.  Every sum has a fixed order and there are no
 * atomics: the same bits on every run and wherever a recording sits in a batch.
 * rec_off and n_states are given twice: HOST arrays, checked before anything is launched, and their device copies, which the kernel
 * reads.  Refused on the host (< 0, nothing written): a bad rec_off (the checks of spk_diar_tables), D outside [1, 512], Smax outside
 * [1, spk_vbx_max_states()], an n_states[r] outside [1, Smax], a recording longer than spk_ahc_max_n(), ws_elems below
 * spk_vbx_ws_elems(), Fa or Fb not positive and finite, loopP outside (0, 1), max_iters < 1, epsilon NaN or +inf. */
int spk_vbx_threads(void);     /* threads of the workgroup that runs one recording */
int spk_vbx_max_states(void);  /* 64: one lane per state */
/* host only: the doubles spk_vbx_batch needs, Ntot (3 + 2 Smax) + R Smax D; < 0 for a shape spk_vbx_batch refuses */
long long spk_vbx_ws_elems(const long long* rec_off /*host [R+1]*/, int R, int Smax, int D);
int spk_vbx_batch(const double* X /*[Ntot][D]*/, const double* Phi /*[D]*/, const long long* rec_off /*host [R+1]*/,
                  const long long* rec_off_dev /*[R+1]*/, const int* n_states /*host [R]*/, const int* n_states_dev /*[R]*/,
                  double* gamma /*[Ntot][Smax]*/, double* pi /*[R][Smax]*/, double Fa, double Fb, double loopP, int max_iters,
                  double epsilon, double* ws, long long ws_elems, double* elbo /*[R][max_iters]*/, int* n_iters /*[R]*/, long long Ntot,
                  int D, int R, int Smax, void* stream);

/* ---- per-recording PCA of the dense PLDA scores (csrc/pca.hip) ------------------------------------------------
 * spk_syevj_batch: R symmetric matrices A [R][ld][ld] of orders orders[r] in [1, ld], ld <= spk_syevj_max_dim() (256); of each the
 * upper triangle of the leading orders[r] x orders[r] part is read.  One workgroup per matrix runs a parallel-ordered cyclic
 * two-sided Jacobi iteration (round-robin pairs, m / 2 rotations per round) with __syncthreads() alone, at most
 * spk_syevj_max_sweeps() sweeps.  w [R][ld]: eigenvalues descending; vec [R][ld][ld]: row k = the unit eigenvector of w[k]; both 0 at
 * and beyond orders[r].  sweeps [R]: sweeps run, the last, rotation-free one included; info [R]: 0 converged, 1 the bound was
 * reached (a NaN in the matrix ends so, with NaN results).  The orders are given twice: a HOST array, checked, and its device copy.
 * ws: spk_syevj_ws_elems(R, ld) doubles (padded orders up to 98 iterate in LDS, up to 140 the matrix does and the eigenvector table
 * lies in ws, larger ones iterate in ws; the bits do not depend on it).
 * Refused on the host (< 0, nothing written): R or ld out of range, an order outside [1, ld], a small workspace, a null pointer. */
int spk_syevj_max_dim(void);
int spk_syevj_max_sweeps(void);
int spk_syevj_threads(void);
long long spk_syevj_ws_elems(int R, int ld);
int spk_syevj_batch(const double* A /*[R][ld][ld]*/, const int* orders /*host [R]*/, const int* orders_dev /*[R]*/, double* ws,
                    long long ws_elems, double* w /*[R][ld]*/, double* vec /*[R][ld][ld]*/, int* sweeps /*[R]*/, int* info /*[R]*/,
                    int R, int ld, void* stream);
/* Steps 1-5 of section 6p for every recording of a batch (the layout of spk_score_dense: rec_off on the host, tab_dev on the device).
 * Z [Ntot][L]: the float rows plda.project gives; W = Ti Ti^T and B = Ti diag(psi) Ti^T with Ti = T^-1 (host, once per call), T [L][L],
 * psi [L] and mean [L]: the smoothed global model; 0 < E < 1.  Per recording: the covariance C of its rows, C = P diag(s) P^T,
 * dim = min(k + 1, L, n - 1) with k the smallest k with (s_1 + ... + s_k) / tot > E, W_r = P_r W P_r^T = G G^T, T1 = G^-1,
 * T1 B_r T1^T = U diag(psi_r) U^T, A_r = U^T T1 P_r, b_r = -A_r mean.  dim [R]; s [R][L] (floored at 0, descending); psi_r [R][L];
 * A_r [R][L][L]; b_r [R][L]: rows and entries at or beyond dim[r] are 0.  A recording with n = 1 or tot <= 0 is skipped: dim = L,
 * A_r = T, b_r = -T mean, psi_r = psi.  info [R]: 0, 1 (an eigendecomposition reached its sweep bound) or 2 (a Cholesky pivot was not
 * positive); with info != 0 the recording's A_r, b_r and psi_r are 0.  The skip comes first: a skipped recording never factorises
 * W_r, so it keeps info = 0 even where W is not positive definite.  L <= 256.  ws: spk_pca_plda_ws_elems() doubles (< 0 for a
 * refused shape).  Refused on the host (< 0, nothing written): a bad rec_off, R > 65535, L outside [1, 256], E outside (0, 1) or NaN,
 * a small workspace, a null device pointer. */
long long spk_pca_plda_ws_elems(const long long* rec_off /*host [R+1]*/, int R, int L);
int spk_pca_plda_batch(const float* Z /*[Ntot][L]*/, const long long* rec_off /*host [R+1]*/, const long long* tab_dev /*[3][R+1]*/,
                       const double* W /*[L][L]*/, const double* B /*[L][L]*/, const double* T /*[L][L]*/, const double* psi /*[L]*/,
                       const double* mean /*[L]*/, double E, double* ws, long long ws_elems, int* dim /*[R]*/, double* s /*[R][L]*/,
                       double* psi_r /*[R][L]*/, double* A_r /*[R][L][L]*/, double* b_r /*[R][L]*/, int* info /*[R]*/, long long Ntot,
                       int L, int R, void* stream);
/* The score terms of every recording from its psi_r [R][L] (zero padded): g = psi / (2 psi + 1), k = psi^2 / ((psi + 1)(2 psi + 1)),
 * qn = 1 / (psi + 1) (the length normalisation's weights), all [R][L], and K [R] = 0.5 sum_d (log(psi_d + 1) - log(1 + psi_d /
 * (psi_d + 1))), one wave per recording, the sum in a fixed order.  psi = 0 gives g = k = 0, qn = 1 and adds exactly 0 to K.
 * Refused on the host (< 0): R or L (1..512) out of range, a null device pointer. */
int spk_pca_score_terms(const double* psi_r /*[R][L]*/, double* g /*[R][L]*/, double* k /*[R][L]*/, double* qn /*[R][L]*/,
                        double* K /*[R]*/, int R, int L, void* stream);
/* The per-recording forms of spk_affine_lennorm, spk_score_dense_q and spk_score_dense (the same kernel bodies): recording r's rows
 * go through A [r], b [r], q [r] (NULL: ones) with Do = dim[r] in the scale, k [r], g [r] and K [r].  Rows are L wide everywhere; the
 * zero padding beyond dim[r] contributes exactly 0. */
int spk_affine_lennorm_rec(const float* X /*[Ntot][L]*/, const long long* rec_off /*host [R+1]*/, const long long* tab_dev,
                           const double* A /*[R][L][L]*/, const double* b /*[R][L]*/, const double* q /*[R][L] or NULL*/,
                           const int* dim /*[R]*/, int scale, double* Y /*[Ntot][L]*/, long long Ntot, int L, int R, void* stream);
int spk_score_dense_q_rec(const double* U /*[Ntot][D]*/, const long long* rec_off /*host [R+1]*/, const long long* tab_dev,
                          const double* k /*[R][D]*/, double scale, double* q /*[Ntot]*/, long long Ntot, int D, int R, void* stream);
int spk_score_dense_rec(const double* U /*[Ntot][D]*/, const long long* rec_off /*host [R+1]*/, const long long* tab_dev,
                        const double* q /*[Ntot]*/, const double* g /*[R][D]*/, const double* K /*[R]*/, float* out, long long Ntot,
                        int D, int R, void* stream);

#ifdef __cplusplus
}
#endif
#endif
