// Stem convolution Conv2d(1,32,3,stride 1,pad 1,bias=False) (reference scripts/model.py:210,249) and its
// weight gradient.  Cin = 1, K = 9: this layer is HBM-bound (AI ~ 4 flop/B), so it is a direct
// convolution, not a GEMM: a thread owns (pixel, 8 output channels) with its 72 weights in registers;
// four neighbouring threads write one pixel's 32 channels = 128 contiguous bytes of the NHWC output.
// Input x is [B][F][T] fp32 (freq-major, time innermost; viewed as NCHW [B,1,F,T] by the reference).
#include "spk_common.h"

#define STEM_C 32

// the statistics contract of the stem: a thread's (sum, sumsq) of its 8 channels over its pixels in grid-stride order, then the
// xor-shuffle over the 16 pixel lanes of a wave, then the four waves in order -> stats[block][32][2].  Shared by stem_fwd_kernel
// and stem_stats_kernel: their rows are bit-equal.
static __device__ __forceinline__ void stem_stats_fold(float (&ssum)[8], float (&ssq)[8], float (&red)[4][STEM_C][2],
                                                       float* __restrict__ stats) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int off = 4; off < 64; off <<= 1) {
            ssum[c] += __shfl_xor(ssum[c], off, 64);
            ssq[c] += __shfl_xor(ssq[c], off, 64);
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
    if (lane < 4) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            red[wave][lane * 8 + c][0] = ssum[c];
            red[wave][lane * 8 + c][1] = ssq[c];
        }
    }
    __syncthreads();
    if (tid < STEM_C) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
            s0 += red[wv][tid][0];
            s1 += red[wv][tid][1];
        }
        stats[((size_t)blockIdx.x * STEM_C + tid) * 2 + 0] = s0;
        stats[((size_t)blockIdx.x * STEM_C + tid) * 2 + 1] = s1;
    }
}

// LEN (spk_stem_conv_fwd_len): image b is an utterance of len[b] <= T frames padded to T - frames t >= len[b] are read as 0 (the
// padding may hold anything, NaN included) and the outputs there are stored as 0, outside the absmax and the statistics
template <bool LEN>
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       float* __restrict__ out, float* __restrict__ stats,
                                                       const float* __restrict__ epi_scale,
                                                       const float* __restrict__ epi_shift, int B, int F, int T,
                                                       int flags, unsigned* __restrict__ amax_out, const int* __restrict__ len) {
    __shared__ float red[4][STEM_C][2];
    float mx = 0.f;
    const int tid = threadIdx.x, cg = tid & 3, pl = tid >> 2;
    float wr[9][8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) wr[t][c] = w[(cg * 8 + c) * 9 + t];
    float es[8], eh[8], ssum[8], ssq[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        es[c] = (flags & SPK_EPI_AFFINE) ? epi_scale[cg * 8 + c] : 1.f;
        eh[c] = (flags & SPK_EPI_AFFINE) ? epi_shift[cg * 8 + c] : 0.f;
        ssum[c] = 0.f;
        ssq[c] = 0.f;
    }
    const int FT = F * T;
    const long long NP = (long long)B * FT;
    for (long long p = (long long)blockIdx.x * 64 + pl; p < NP; p += (long long)gridDim.x * 64) {
        const int b = (int)(p / FT);
        const int rem = (int)(p - (long long)b * FT);
        const int f = rem / T, t0 = rem - f * T;
        const float* xb = x + (size_t)b * FT;
        const int Tb = LEN ? min(len[b], T) : T;          // frames of this utterance
        float xv[9];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int ff = f + kh - 1, tt = t0 + kw - 1;
                xv[kh * 3 + kw] = (ff >= 0 && ff < F && tt >= 0 && tt < Tb) ? xb[ff * T + tt] : 0.f;
            }
        const bool tail = LEN && t0 >= Tb;
        float o[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float v = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) v = fmaf(xv[t], wr[t][c], v);
            if (flags & SPK_EPI_AFFINE) v = v * es[c] + eh[c];
            if (flags & SPK_EPI_RELU) v = fmaxf(v, 0.f);
            if (tail) v = 0.f;
            o[c] = v;
            mx = fmaxf(mx, fabsf(v));
            ssum[c] += v;
            ssq[c] += v * v;
        }
        f32x4* dst = (f32x4*)(out + (size_t)p * STEM_C + cg * 8);
        dst[0] = (f32x4){o[0], o[1], o[2], o[3]};
        dst[1] = (f32x4){o[4], o[5], o[6], o[7]};
    }
    if (amax_out) spk_wave_amax_commit(mx, amax_out);     // absmax(out): the operand scale of its f16x3 consumers
    if (flags & SPK_EPI_STATS) stem_stats_fold(ssum, ssq, red, stats);
}

extern "C" int spk_stem_fwd_blocks(int B, int F, int T) {
    long long np = (long long)B * F * T;
    long long nb = (np + 63) / 64;
    return (int)(nb < 2048 ? nb : 2048);
}

extern "C" int spk_stem_conv_fwd(const float* x, const float* w, float* out, float* stats, const float* epi_scale,
                                 const float* epi_shift, int B, int F, int T, int flags, unsigned* amax_out, void* stream) {
    SPK_REQUIRE(x && w && out, "spk_stem_conv_fwd: null pointer");
    SPK_REQUIRE(B > 0 && F > 0 && T > 0, "spk_stem_conv_fwd: empty input");
    SPK_REQUIRE(!(flags & SPK_EPI_STATS) || stats, "spk_stem_conv_fwd: EPI_STATS needs a stats buffer");
    SPK_REQUIRE(!(flags & SPK_EPI_AFFINE) || (epi_scale && epi_shift), "spk_stem_conv_fwd: EPI_AFFINE needs scale/shift");
    SPK_REQUIRE(!(flags & SPK_EPI_WMASK), "spk_stem_conv_fwd: SPK_EPI_WMASK needs the lengths (spk_stem_conv_fwd_len)");
    hipLaunchKernelGGL(stem_fwd_kernel<false>, dim3(spk_stem_fwd_blocks(B, F, T)), dim3(256), 0, (hipStream_t)stream, x, w, out,
                       stats, epi_scale, epi_shift, B, F, T, flags, amax_out, nullptr);
    SPK_LAUNCH_CHECK("spk_stem_conv_fwd");
    return 0;
}

extern "C" int spk_stem_conv_fwd_len(const float* x, const float* w, float* out, float* stats, const float* epi_scale,
                                     const float* epi_shift, int B, int F, int T, int flags, unsigned* amax_out, const int* len,
                                     void* stream) {
    SPK_REQUIRE(x && w && out && len, "spk_stem_conv_fwd_len: null pointer");
    SPK_REQUIRE(B > 0 && F > 0 && T > 0, "spk_stem_conv_fwd_len: empty input");
    SPK_REQUIRE(flags & SPK_EPI_WMASK, "spk_stem_conv_fwd_len: flags must carry SPK_EPI_WMASK");
    SPK_REQUIRE(!(flags & SPK_EPI_STATS) || stats, "spk_stem_conv_fwd_len: EPI_STATS needs a stats buffer");
    SPK_REQUIRE(!(flags & SPK_EPI_AFFINE) || (epi_scale && epi_shift), "spk_stem_conv_fwd_len: EPI_AFFINE needs scale/shift");
    hipLaunchKernelGGL(stem_fwd_kernel<true>, dim3(spk_stem_fwd_blocks(B, F, T)), dim3(256), 0, (hipStream_t)stream, x, w, out,
                       stats, epi_scale, epi_shift, B, F, T, flags, amax_out, len);
    SPK_LAUNCH_CHECK("spk_stem_conv_fwd_len");
    return 0;
}

// ---- training forward without the raw0 read-back: statistics with no store, then one writer of raw0, a and the sign bits ----
// The convolution is 1.8 G multiply-adds over a 24.6 MB input: cheaper to compute twice than to read its 786 MB output once.

// (b, f, t) of the pixels p0, p0 + step, p0 + 2 step, ... of a grid-stride loop: one division at the start, carries afterwards
struct StemPix {
    int b, f, t, db, df, dt;
    __device__ __forceinline__ StemPix(unsigned p0, unsigned step, int F, int T) {
        const unsigned r = p0 / (unsigned)T, rs = step / (unsigned)T;
        t = (int)(p0 - r * T);
        b = (int)(r / (unsigned)F);
        f = (int)(r - (unsigned)b * F);
        dt = (int)(step - rs * T);
        db = (int)(rs / (unsigned)F);
        df = (int)(rs - (unsigned)db * F);
    }
    __device__ __forceinline__ void next(int F, int T) {
        t += dt;
        int carry = t >= T;
        t -= carry ? T : 0;
        f += df + carry;                 // f < F, df < F, carry <= 1: below 2F
        carry = f >= F;
        f -= carry ? F : 0;
        b += db + carry;
    }
};

// the nine taps of pixel (b, f, t), zero-padded; tap order kh * 3 + kw as in stem_fwd_kernel
static __device__ __forceinline__ void stem_taps(const float* __restrict__ x, int b, int f, int t, int F, int T, float (&xv)[9]) {
    const float* xc = x + ((size_t)b * F + f) * T + t;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int ff = f + kh - 1, tt = t + kw - 1;
            xv[kh * 3 + kw] = (ff >= 0 && ff < F && tt >= 0 && tt < T) ? xc[(kh - 1) * T + (kw - 1)] : 0.f;
        }
}

static __device__ __forceinline__ f32x4 stem_ld_nt(const float* p) { return __builtin_nontemporal_load((const f32x4*)p); }
static __device__ __forceinline__ void stem_st_nt(float* p, f32x4 v) { __builtin_nontemporal_store(v, (f32x4*)p); }

// stem_fwd_kernel<false> with EPI_STATS alone, minus the store: the same grid, pixel mapping, grid-stride order, multiply-add
// chain and fold, so the rows are bit-equal to the ones spk_stem_conv_fwd writes.  32-bit pixel indices (the host checks).
__global__ __launch_bounds__(256) void stem_stats_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         float* __restrict__ stats, unsigned NP, int F, int T) {
    __shared__ float red[4][STEM_C][2];
    const int tid = threadIdx.x, cg = tid & 3, pl = tid >> 2;
    float wr[9][8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) wr[t][c] = w[(cg * 8 + c) * 9 + t];
    float ssum[8], ssq[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        ssum[c] = 0.f;
        ssq[c] = 0.f;
    }
    const unsigned step = gridDim.x * 64u;
    StemPix q(blockIdx.x * 64u + pl, step, F, T);
    for (unsigned p = blockIdx.x * 64u + pl; p < NP; p += step) {
        float xv[9];
        stem_taps(x, q.b, q.f, q.t, F, T, xv);
        q.next(F, T);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float v = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) v = fmaf(xv[t], wr[t][c], v);
            ssum[c] += v;
            ssq[c] += v * v;
        }
    }
    stem_stats_fold(ssum, ssq, red, stats);
}

// One block per row (b, f) of T pixels; eight lanes hold the 32 channels of a pixel as 16-byte groups, so a wave stores 1 KB of
// contiguous raw0 and 1 KB of a per pass (the layout of bn_apply_kernel at C = 32, sign words included), non-temporal.
// raw0: the multiply-add chain of stem_fwd_kernel; a: the expression of bn_apply_kernel.  This kernel owns no sums.
__global__ __launch_bounds__(256) void stem_fwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             float* __restrict__ raw_out, float* __restrict__ act_out,
                                                             unsigned* __restrict__ mask_out, unsigned* __restrict__ amax_out,
                                                             int F, int T) {
    const int row = blockIdx.x, f = row % F;
    const int tid = threadIdx.x, c0 = (tid & 7) * 4, pl = tid >> 3;
    float wr[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) wr[t][c] = w[(c0 + c) * 9 + t];
    const f32x4 psc = *(const f32x4*)(scale + c0), psh = *(const f32x4*)(shift + c0);
    const float* xc = x + (size_t)row * T;
    const bool rok[3] = {f > 0, true, f + 1 < F};
    float mx = 0.f;
    for (int t0 = 0; t0 < T; t0 += 32) {
        const int t = t0 + pl;
        if (t >= T) continue;             // whole 8-lane groups: the lanes of a pixel stay together for the sign word
        float xv[9];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int tt = t + kw - 1;
                xv[kh * 3 + kw] = (rok[kh] && tt >= 0 && tt < T) ? xc[(kh - 1) * T + tt] : 0.f;
            }
        f32x4 rv;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 9; ++k) v = fmaf(xv[k], wr[k][c], v);
            rv[c] = v;
        }
        f32x4 v = rv * psc + psh;
        v[0] = fmaxf(v[0], 0.f);
        v[1] = fmaxf(v[1], 0.f);
        v[2] = fmaxf(v[2], 0.f);
        v[3] = fmaxf(v[3], 0.f);
        const size_t pix = (size_t)row * T + t;
        stem_st_nt(raw_out + pix * STEM_C + c0, rv);
        stem_st_nt(act_out + pix * STEM_C + c0, v);
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
        if (mask_out) {
            unsigned bits = (v[0] > 0.f ? 1u : 0u) | (v[1] > 0.f ? 2u : 0u) | (v[2] > 0.f ? 4u : 0u) | (v[3] > 0.f ? 8u : 0u);
            bits <<= 4 * (tid & 7);
            bits |= __shfl_xor(bits, 1, 64);
            bits |= __shfl_xor(bits, 2, 64);
            bits |= __shfl_xor(bits, 4, 64);
            if ((tid & 7) == 0) mask_out[pix] = bits;
        }
    }
    if (amax_out) spk_wave_amax_commit(mx, amax_out);     // absmax(a): every lane of the wave takes part
}

extern "C" int spk_stem_stats(const float* x, const float* w, float* stats, int B, int F, int T, void* stream) {
    SPK_REQUIRE(x && w && stats, "spk_stem_stats: null pointer");
    SPK_REQUIRE(B > 0 && F > 0 && T > 0, "spk_stem_stats: empty input");
    const long long np = (long long)B * F * T;
    SPK_REQUIRE(np < 2147483647LL, "spk_stem_stats: %lld pixels exceed the 32-bit pixel index of the kernel", np);
    hipLaunchKernelGGL(stem_stats_kernel, dim3(spk_stem_fwd_blocks(B, F, T)), dim3(256), 0, (hipStream_t)stream, x, w, stats,
                       (unsigned)np, F, T);
    SPK_LAUNCH_CHECK("spk_stem_stats");
    return 0;
}

extern "C" int spk_stem_fwd_apply(const float* x, const float* w, const float* scale, const float* shift, float* raw_out,
                                  float* act_out, unsigned* mask_out, unsigned* amax_out, int B, int F, int T, void* stream) {
    SPK_REQUIRE(x && w && scale && shift && raw_out && act_out, "spk_stem_fwd_apply: null pointer");
    SPK_REQUIRE(B > 0 && F > 0 && T > 0, "spk_stem_fwd_apply: empty input");
    SPK_REQUIRE((long long)B * F < 2147483647LL, "spk_stem_fwd_apply: %lld rows exceed the grid", (long long)B * F);
    hipLaunchKernelGGL(stem_fwd_apply_kernel, dim3((unsigned)(B * F)), dim3(256), 0, (hipStream_t)stream, x, w, scale, shift,
                       raw_out, act_out, mask_out, amax_out, F, T);
    SPK_LAUNCH_CHECK("spk_stem_fwd_apply");
    return 0;
}

// the weight-gradient contract of the stem: a thread's 72 sums over its pixels in grid-stride order, the xor-shuffle over the 16
// pixel lanes, the four waves pairwise -> partial[block][32*9].  Shared by stem_wgrad_kernel and stem_bwd_wgrad_kernel.
static __device__ __forceinline__ void stem_wgrad_fold(float (&acc)[9][8], float (&red)[4][STEM_C * 9], float* __restrict__ partial) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float v = acc[t][c];
#pragma unroll
            for (int off = 4; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
            if (lane < 4) red[wave][(lane * 8 + c) * 9 + t] = v;
        }
    __syncthreads();
    for (int i = tid; i < STEM_C * 9; i += 256)
        partial[(size_t)blockIdx.x * (STEM_C * 9) + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

// dW[c][tap] = sum_p x[p + tap] * draw[p][c]; per-block partials [nblk][32][9] then a fixed-order sum.
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ draw,
                                                         float* __restrict__ partial, int B, int F, int T) {
    __shared__ float red[4][STEM_C * 9];
    const int tid = threadIdx.x, cg = tid & 3, pl = tid >> 2;
    float acc[9][8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[t][c] = 0.f;
    const int FT = F * T;
    const long long NP = (long long)B * FT;
    for (long long p = (long long)blockIdx.x * 64 + pl; p < NP; p += (long long)gridDim.x * 64) {
        const int b = (int)(p / FT);
        const int rem = (int)(p - (long long)b * FT);
        const int f = rem / T, t0 = rem - f * T;
        const float* xb = x + (size_t)b * FT;
        float xv[9];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int ff = f + kh - 1, tt = t0 + kw - 1;
                xv[kh * 3 + kw] = (ff >= 0 && ff < F && tt >= 0 && tt < T) ? xb[ff * T + tt] : 0.f;
            }
        const f32x4* src = (const f32x4*)(draw + (size_t)p * STEM_C + cg * 8);
        const f32x4 d0 = src[0], d1 = src[1];
        const float d[8] = {d0[0], d0[1], d0[2], d0[3], d1[0], d1[1], d1[2], d1[3]};
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[t][c] = fmaf(xv[t], d[c], acc[t][c]);
    }
    stem_wgrad_fold(acc, red, partial);
}

// one block per weight element: 256 threads fold the per-block partials in fp64, fixed order
__global__ __launch_bounds__(256) void stem_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw,
                                                                int nblk, int accumulate) {
    __shared__ double red[256];
    const int i = blockIdx.x;
    double s = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 256) s += (double)partial[(size_t)k * (STEM_C * 9) + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) dw[i] = accumulate ? dw[i] + (float)red[0] : (float)red[0];
}

extern "C" int spk_stem_wgrad_blocks(int B, int F, int T) {
    long long np = (long long)B * F * T;
    long long nb = (np + 63) / 64;
    return (int)(nb < 1024 ? nb : 1024);
}

extern "C" int spk_stem_conv_wgrad(const float* x, const float* draw, float* dw, float* partial, int B, int F, int T,
                                   int accumulate, void* stream) {
    SPK_REQUIRE(x && draw && dw && partial, "spk_stem_conv_wgrad: null pointer");
    SPK_REQUIRE(B > 0 && F > 0 && T > 0, "spk_stem_conv_wgrad: empty input");
    const int nblk = spk_stem_wgrad_blocks(B, F, T);
    hipLaunchKernelGGL(stem_wgrad_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, x, draw, partial, B, F, T);
    SPK_LAUNCH_CHECK("spk_stem_conv_wgrad");
    hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3(STEM_C * 9), dim3(256), 0, (hipStream_t)stream, partial, dw, nblk, accumulate);
    SPK_LAUNCH_CHECK("spk_stem_wgrad_reduce");
    return 0;
}

// ---- the BatchNorm-backward apply inside the weight gradient -----------------------------------------------------------------
// draw0 has one consumer (the stem has no data gradient): formed in registers here instead of written and read back.
// stem_wgrad_kernel's mapping, block count and accumulation order; draw as bn_bwd_apply_kernel forms it for MASK_RAW (the mask
// is a select: the pooling backward hands down inf / NaN under dead rows).  The grid-stride loop is unrolled by U with the
// loads of all U iterations issued first - more bytes in flight, the order of a thread's sums unchanged.
#ifndef STEM_BWD_U
#define STEM_BWD_U 2
#endif
__global__ __launch_bounds__(256) void stem_bwd_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             const float* __restrict__ raw, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const float* __restrict__ coef,
                                                             float* __restrict__ partial, unsigned NP, int F, int T) {
    __shared__ float red[4][STEM_C * 9];
    constexpr int U = STEM_BWD_U;
    const int tid = threadIdx.x, cg = tid & 3, pl = tid >> 2, c0 = cg * 8;
    float acc[9][8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[t][c] = 0.f;
    f32x4 pmu[2], pis[2], psc[2], psh[2], pk1[2], pm1[2], pm2[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = c0 + 4 * h;
        pmu[h] = *(const f32x4*)(mean + c);
        pis[h] = *(const f32x4*)(invstd + c);
        psc[h] = *(const f32x4*)(scale + c);
        psh[h] = *(const f32x4*)(shift + c);
        pk1[h] = *(const f32x4*)(coef + c);
        pm1[h] = *(const f32x4*)(coef + STEM_C + c);
        pm2[h] = *(const f32x4*)(coef + 2 * STEM_C + c);
    }
    const unsigned step = gridDim.x * 64u;
    StemPix q(blockIdx.x * 64u + pl, step, F, T);
    for (unsigned p0 = blockIdx.x * 64u + pl; p0 < NP; p0 += step * U) {
        float xv[U][9];
        f32x4 dv[U][2], rv[U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned p = p0 + step * u;
            if (p < NP) {
                stem_taps(x, q.b, q.f, q.t, F, T, xv[u]);
                const size_t off = (size_t)p * STEM_C + c0;
                dv[u][0] = stem_ld_nt(dy + off);
                dv[u][1] = stem_ld_nt(dy + off + 4);
                rv[u][0] = stem_ld_nt(raw + off);
                rv[u][1] = stem_ld_nt(raw + off + 4);
            }
            q.next(F, T);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p0 + step * u >= NP) break;
            float o[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x4 r = rv[u][h];
                f32x4 d = dv[u][h];
                const f32x4 z = r * psc[h] + psh[h];
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = z[k] > 0.f ? d[k] : 0.f;
                const f32x4 xh = (r - pmu[h]) * pis[h];
                const f32x4 g = pk1[h] * (d - pm1[h] - xh * pm2[h]);
#pragma unroll
                for (int k = 0; k < 4; ++k) o[h * 4 + k] = g[k];
            }
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[t][c] = fmaf(xv[u][t], o[c], acc[t][c]);
        }
    }
    stem_wgrad_fold(acc, red, partial);
}

extern "C" int spk_stem_bwd_wgrad(const float* x, const float* d, const float* raw, const float* mean, const float* invstd,
                                  const float* scale, const float* shift, const float* coef, float* dw, float* partial, int B,
                                  int F, int T, int accumulate, void* stream) {
    SPK_REQUIRE(x && d && raw && mean && invstd && scale && shift && coef && dw && partial, "spk_stem_bwd_wgrad: null pointer");
    SPK_REQUIRE(B > 0 && F > 0 && T > 0, "spk_stem_bwd_wgrad: empty input");
    const long long np = (long long)B * F * T;
    SPK_REQUIRE(np < 2147483647LL / 2, "spk_stem_bwd_wgrad: %lld pixels exceed the 32-bit pixel index of the kernel", np);
    const int nblk = spk_stem_wgrad_blocks(B, F, T);
    hipLaunchKernelGGL(stem_bwd_wgrad_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, x, d, raw, mean, invstd, scale, shift,
                       coef, partial, (unsigned)np, F, T);
    SPK_LAUNCH_CHECK("spk_stem_bwd_wgrad");
    hipLaunchKernelGGL(stem_wgrad_reduce_kernel, dim3(STEM_C * 9), dim3(256), 0, (hipStream_t)stream, partial, dw, nblk, accumulate);
    SPK_LAUNCH_CHECK("spk_stem_wgrad_reduce");
    return 0;
}
