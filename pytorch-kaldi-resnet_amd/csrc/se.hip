// Squeeze-and-excitation tail of an SEBasicBlock (reference scripts/model.py:17-33, 67-97; reduction 16, no biases) on NHWC
// fp32 tensors [B][H*W][C].  With z = scale_c raw + shift_c (the block's second BatchNorm, no ReLU):
//
// Forward:   se_squeeze   sums[b][c] = sum_hw raw                    (one read of raw)
//            se_excite    q = scale sums / HW + shift, u = relu(W1 q), g = sigmoid(W2 u)      ([B][C] tables only)
//            se_apply     out = relu(g[b][c] z + shortcut)           (read raw + shortcut, write out: bn_apply with a gate)
// Backward:  e = dout [out > 0]
//            se_bwd_reduce   S1[b][c] = sum_hw e, S2[b][c] = sum_hw e raw                     (read dout + raw)
//            se_bwd_gate     dg = scale S2 + shift S1 -> da -> du -> dq, dW1, dW2, and the BatchNorm-backward statistics of
//                            dz = g e + dq / HW from the tables alone: dbeta, dgamma, coefficient rows, operand-scale bound
//            se_bwd_apply    draw = k1 (dz - m1 - xhat m2)  (+ e, the shortcut gradient, when it must be stored)
//
// Reductions are two-level and run in a fixed order: fp32 inside a block of SE_ROWS pixels, fp64 across blocks, utterances
// and the small matrix products.  No floating-point atomics (the absmax hand-offs are integer atomicMax on float bits, as in
// bn.hip).  Nothing here synchronises with the host or allocates: every launch can be captured into a graph.
#include "spk_common.h"

enum { MASK_NONE = 0, MASK_ACT = 1, MASK_RAW = 2, MASK_BITS = 3 };   // as in bn.hip; the SE kernels take MASK_ACT and MASK_BITS

#define SE_ROWS 512          // pixels of one utterance per reduction block
#define SE_MAX_CR 64         // hidden width limit of the gate kernels (C / 16 <= 64 for C <= 1024)

static bool se_c_ok(int C) { return C >= 32 && C <= 1024 && (C & (C - 1)) == 0; }

static __device__ __forceinline__ f32x4 se_ld(const float* p) { return __builtin_nontemporal_load((const f32x4*)p); }
static __device__ __forceinline__ void se_st(float* p, f32x4 v) { __builtin_nontemporal_store(v, (f32x4*)p); }

extern "C" int spk_se_chunks(long long HW) { return (int)((HW + SE_ROWS - 1) / SE_ROWS); }

// ---- per-utterance channel reductions ------------------------------------------------------------------------------------
// partial[(b * nchunk + chunk) * NV * C + v * C + c]: fp32 sums over the pixels [chunk * SE_ROWS, ...) of utterance b.
// BWD = false: NV = 1, sum of x (pixels at width >= wlen[b] left out when wlen is given)
// BWD = true:  NV = 2, (sum e, sum e * raw) with e = dy masked by the sign bits / the activated tensor
template <bool BWD>
__global__ __launch_bounds__(256) void se_reduce_kernel(const float* __restrict__ x, const float* __restrict__ raw,
                                                        const float* __restrict__ act, float* __restrict__ partial, int HW, int W,
                                                        int C, int mode, const int* __restrict__ wlen,
                                                        unsigned* __restrict__ chan_amax) {
    constexpr int NV = BWD ? 2 : 1;
    __shared__ float red[256][4 * NV];
    const int tid = threadIdx.x;
    const int qpr = C >> 2;
    const int quad = tid % qpr, prow = tid / qpr, rstep = 256 / qpr;
    const int b = blockIdx.y, nchunk = gridDim.x;
    const int p0 = blockIdx.x * SE_ROWS;
    int p1 = p0 + SE_ROWS;
    if (p1 > HW) p1 = HW;
    const size_t img = (size_t)b * HW;
    const int wl = wlen ? wlen[b] : W;
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, ss = {0.f, 0.f, 0.f, 0.f}, mx = {0.f, 0.f, 0.f, 0.f};
    for (int p = p0 + prow; p < p1; p += rstep) {
        const size_t off = (img + p) * C + quad * 4;
        if (!BWD) {
            if (wlen && (p % W) >= wl) continue;
            s += se_ld(x + off);
        } else {
            f32x4 d = se_ld(x + off);
            const f32x4 rv = se_ld(raw + off);
            if (mode == MASK_BITS) {
                const unsigned bits = ((const unsigned*)act)[(img + p) * (C >> 5) + (quad >> 3)] >> ((quad * 4) & 31);
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = ((bits >> k) & 1u) ? d[k] : 0.f;
            } else {
                const f32x4 a = *(const f32x4*)(act + off);
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = a[k] > 0.f ? d[k] : 0.f;
            }
            s += d;
            ss += d * rv;
#pragma unroll
            for (int k = 0; k < 4; ++k) mx[k] = fmaxf(mx[k], spk_finite_abs(d[k]));
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        red[tid][k] = s[k];
        if (BWD) red[tid][4 * (NV - 1) + k] = ss[k];
    }
    __syncthreads();
    if (tid < qpr) {
        float a[4 * NV];
#pragma unroll
        for (int k = 0; k < 4 * NV; ++k) a[k] = 0.f;
        for (int p = 0; p < rstep; ++p)
#pragma unroll
            for (int k = 0; k < 4 * NV; ++k) a[k] += red[p * qpr + tid][k];
        float* dst = partial + ((size_t)b * nchunk + blockIdx.x) * NV * C + tid * 4;
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[v * C + k] = a[4 * v + k];
    }
    if (BWD && chan_amax) {          // per-channel absmax of e (float bits): see bn_bwd_reduce_kernel
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) red[tid][k] = mx[k];
        __syncthreads();
        if (tid < qpr) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float m = 0.f;
                for (int p = 0; p < rstep; ++p) m = fmaxf(m, red[p * qpr + tid][k]);
                const unsigned bits = __float_as_uint(m);
                unsigned* slot = chan_amax + tid * 4 + k;
                if (bits > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, bits);
            }
        }
    }
}

// out[b * inner + i] = sum over chunks (fp64, ascending chunk order) of partial[(b * nchunk + k) * inner + i]
__global__ __launch_bounds__(256) void se_fold_kernel(const float* __restrict__ partial, double* __restrict__ out, int nchunk,
                                                      int inner, long long total) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long long b = t / inner;
    const int i = (int)(t - b * inner);
    const float* p = partial + (size_t)b * nchunk * inner + i;
    double s = 0.0;
    for (int k = 0; k < nchunk; ++k) s += (double)p[(size_t)k * inner];
    out[t] = s;
}

extern "C" int spk_se_squeeze(const float* x, float* partial, double* sums, int B, int H, int W, int C, const int* wlen,
                              void* stream) {
    SPK_REQUIRE(x && partial && sums, "spk_se_squeeze: null pointer");
    SPK_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && se_c_ok(C), "spk_se_squeeze: B=%d H=%d W=%d C=%d (C a power of two in [32,1024])", B, H, W, C);
    const long long HW = (long long)H * W;
    SPK_REQUIRE(HW * C < 2147483647LL, "spk_se_squeeze: %lld values per utterance exceed the 32-bit index of the kernel", HW * C);
    const int nchunk = spk_se_chunks(HW);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(se_reduce_kernel<false>, dim3(nchunk, B), dim3(256), 0, st, x, nullptr, nullptr, partial, (int)HW, W, C, 0,
                       wlen, nullptr);
    SPK_LAUNCH_CHECK("spk_se_squeeze");
    const long long total = (long long)B * C;
    hipLaunchKernelGGL(se_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, partial, sums, nchunk, C, total);
    SPK_LAUNCH_CHECK("spk_se_squeeze(fold)");
    return 0;
}

extern "C" int spk_se_bwd_reduce(const float* dout, const float* raw, const float* act, float* partial, double* S, int B,
                                 long long HW, int C, int mask_mode, unsigned* chan_amax, void* stream) {
    SPK_REQUIRE(dout && raw && act && partial && S, "spk_se_bwd_reduce: null pointer");
    SPK_REQUIRE(B > 0 && B <= 65535 && HW > 0 && se_c_ok(C), "spk_se_bwd_reduce: B=%d HW=%lld C=%d", B, HW, C);
    SPK_REQUIRE(HW * C < 2147483647LL, "spk_se_bwd_reduce: %lld values per utterance exceed the 32-bit index of the kernel", HW * C);
    SPK_REQUIRE(mask_mode == MASK_ACT || mask_mode == MASK_BITS, "spk_se_bwd_reduce: mask_mode=%d (MASK_ACT or MASK_BITS)", mask_mode);
    const int nchunk = spk_se_chunks(HW);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(se_reduce_kernel<true>, dim3(nchunk, B), dim3(256), 0, st, dout, raw, act, partial, (int)HW, (int)HW, C,
                       mask_mode, nullptr, chan_amax);
    SPK_LAUNCH_CHECK("spk_se_bwd_reduce");
    const long long total = (long long)B * 2 * C;
    hipLaunchKernelGGL(se_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, partial, S, nchunk, 2 * C, total);
    SPK_LAUNCH_CHECK("spk_se_bwd_reduce(fold)");
    return 0;
}

// wave-wide sum of a double in a fixed (butterfly) order: every lane ends with the same value
static __device__ __forceinline__ double se_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---- excite: one block per utterance ---------------------------------------------------------------------------------------
// q = scale * (sums / count) + shift (scale == nullptr: the identity affine - `sums` are already sums of z), count = H * W or
// H * wlen[b]; u = relu(W1 q), W1 [Cr][C]; g = sigmoid(W2 u), W2 [C][Cr].  Products accumulate in fp64.
__global__ __launch_bounds__(256) void se_excite_kernel(const double* __restrict__ sums, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const float* __restrict__ W1,
                                                        const float* __restrict__ W2, float* __restrict__ q, float* __restrict__ u,
                                                        float* __restrict__ g, int C, int Cr, int H, int W,
                                                        const int* __restrict__ wlen) {
    __shared__ float sq[1024];
    __shared__ float su[SE_MAX_CR];
    const int tid = threadIdx.x, b = blockIdx.x;
    const double cnt = (double)H * (double)(wlen ? wlen[b] : W);
    for (int c = tid; c < C; c += 256) {
        const float m = (float)(sums[(size_t)b * C + c] / cnt);
        const float v = scale ? scale[c] * m + shift[c] : m;
        sq[c] = v;
        q[(size_t)b * C + c] = v;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int j = wave; j < Cr; j += 4) {
        double acc = 0.0;
        for (int c = lane; c < C; c += 64) acc += (double)W1[(size_t)j * C + c] * (double)sq[c];
        acc = se_wave_sum(acc);
        const float uj = fmaxf((float)acc, 0.f);
        if (lane == 0) {
            su[j] = uj;
            u[(size_t)b * Cr + j] = uj;
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        double acc = 0.0;
        for (int j = 0; j < Cr; ++j) acc += (double)W2[(size_t)c * Cr + j] * (double)su[j];
        g[(size_t)b * C + c] = (float)(1.0 / (1.0 + exp(-acc)));
    }
}

extern "C" int spk_se_excite(const double* sums, const float* scale, const float* shift, const float* W1, const float* W2,
                             float* q, float* u, float* g, int B, int C, int Cr, int H, int W, const int* wlen, void* stream) {
    SPK_REQUIRE(sums && W1 && W2 && q && u && g, "spk_se_excite: null pointer");
    SPK_REQUIRE((scale == nullptr) == (shift == nullptr), "spk_se_excite: scale / shift come in pairs");
    SPK_REQUIRE(B > 0 && H > 0 && W > 0 && se_c_ok(C) && Cr >= 1 && Cr <= SE_MAX_CR, "spk_se_excite: B=%d H=%d W=%d C=%d Cr=%d", B, H, W, C, Cr);
    hipLaunchKernelGGL(se_excite_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, sums, scale, shift, W1, W2, q, u, g, C, Cr, H,
                       W, wlen);
    SPK_LAUNCH_CHECK("spk_se_excite");
    return 0;
}

// grid of the two apply kernels: blocks per utterance x utterances; about 8192 blocks in all, each thread loops over its groups
static dim3 se_apply_grid(long long nq, int B) {
    long long nb = (nq + 255) / 256;
    long long cap = 8192 / B;
    if (cap < 1) cap = 1;
    if (nb > cap) nb = cap;
    return dim3((unsigned)(nb < 1 ? 1 : nb), (unsigned)B);
}

// ---- apply: out = [relu]( g[b][c] * (raw * scale + shift) [+ res | + res * rscale + rshift] ), 0 at width >= wlen[b] ----------
// sign-mask words and the absmax hand-off as in bn_apply_kernel.  nq: 16-byte groups per utterance.
__global__ __launch_bounds__(256) void se_apply_kernel(const float* __restrict__ raw, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const float* __restrict__ gate,
                                                       const float* __restrict__ res, const float* __restrict__ rscale,
                                                       const float* __restrict__ rshift, float* __restrict__ out,
                                                       unsigned* __restrict__ mask_out, unsigned nq, int W, int C, int relu,
                                                       unsigned* __restrict__ amax_out, const int* __restrict__ wlen) {
    const int b = blockIdx.y;
    // a block covers 1024 floats and the stride is whole blocks (C <= 1024, a power of two): a thread stays on its channels
    const int c0 = (threadIdx.x * 4) & (C - 1);
    const f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 psc = scale ? *(const f32x4*)(scale + c0) : one, psh = scale ? *(const f32x4*)(shift + c0) : zero;
    const f32x4 prs = rscale ? *(const f32x4*)(rscale + c0) : one, prh = rscale ? *(const f32x4*)(rshift + c0) : zero;
    const f32x4 pg = *(const f32x4*)(gate + (size_t)b * C + c0);
    const int lgq = 29 - __builtin_clz((unsigned)C);         // log2(C / 4)
    const int wl = wlen ? wlen[b] : W;
    const size_t base = (size_t)b * nq;
    const unsigned stride = gridDim.x * 256u;
    float mx = 0.f;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < nq; i += stride) {
        const size_t gi = base + i;
        f32x4 v = pg * (se_ld(raw + gi * 4) * psc + psh);
        if (res) {
            f32x4 r = se_ld(res + gi * 4);
            if (rscale) r = r * prs + prh;
            v += r;
        }
        if (relu) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
        }
        if (wlen && (int)((i >> lgq) % (unsigned)W) >= wl) v = zero;
        se_st(out + gi * 4, v);
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
        if (mask_out) {
            // eight consecutive lanes hold the 32 channels of one word; nq is a multiple of 8, so they are active together
            unsigned bits = (v[0] > 0.f ? 1u : 0u) | (v[1] > 0.f ? 2u : 0u) | (v[2] > 0.f ? 4u : 0u) | (v[3] > 0.f ? 8u : 0u);
            bits <<= 4 * (threadIdx.x & 7);
            bits |= __shfl_xor(bits, 1, 64);
            bits |= __shfl_xor(bits, 2, 64);
            bits |= __shfl_xor(bits, 4, 64);
            if ((threadIdx.x & 7) == 0) mask_out[gi >> 3] = bits;
        }
    }
    if (amax_out) spk_wave_amax_commit(mx, amax_out);
}

extern "C" int spk_se_apply(const float* raw, const float* scale, const float* shift, const float* gate, const float* res,
                            const float* res_scale, const float* res_shift, float* out, unsigned* mask_out, int B, int H, int W,
                            int C, int relu, unsigned* amax_out, const int* wlen, void* stream) {
    SPK_REQUIRE(raw && gate && out, "spk_se_apply: null pointer");
    SPK_REQUIRE((scale == nullptr) == (shift == nullptr), "spk_se_apply: scale / shift come in pairs");
    SPK_REQUIRE((res_scale == nullptr) == (res_shift == nullptr), "spk_se_apply: residual affine must come in pairs");
    SPK_REQUIRE(!res_scale || res, "spk_se_apply: residual affine without residual");
    SPK_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && se_c_ok(C), "spk_se_apply: B=%d H=%d W=%d C=%d", B, H, W, C);
    const long long nq = (long long)H * W * C / 4;
    SPK_REQUIRE(nq < 2147483647LL / 8, "spk_se_apply: %lld values per utterance exceed the 32-bit group index of the kernel", nq * 4);
    hipLaunchKernelGGL(se_apply_kernel, se_apply_grid(nq, B), dim3(256), 0, (hipStream_t)stream, raw, scale, shift, gate, res,
                       res_scale, res_shift, out, mask_out, (unsigned)nq, W, C, relu, amax_out, wlen);
    SPK_LAUNCH_CHECK("spk_se_apply");
    return 0;
}

// ---- backward gate chain: one block per utterance ----------------------------------------------------------------------------
// dg = scale S2 + shift S1; da = dg g (1 - g) (exactly 0 where g is 0 or 1); du = W2^T da [u > 0]; dq = W1^T du.
// Writes da [B][C], du [B][Cr] and dq [2][B][C] = (dq, dq / HW - the term apply adds to every pixel).
__global__ __launch_bounds__(256) void se_gate_chain_kernel(const double* __restrict__ S, const float* __restrict__ u,
                                                            const float* __restrict__ g, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, const float* __restrict__ W1,
                                                            const float* __restrict__ W2, float* __restrict__ da,
                                                            float* __restrict__ du, float* __restrict__ dq, int B, int C, int Cr,
                                                            double hw) {
    __shared__ float sda[1024];
    __shared__ float sdu[SE_MAX_CR];
    const int tid = threadIdx.x, b = blockIdx.x;
    for (int c = tid; c < C; c += 256) {
        const double s1 = S[((size_t)b * 2 + 0) * C + c], s2 = S[((size_t)b * 2 + 1) * C + c];
        const float dg = (float)((double)scale[c] * s2 + (double)shift[c] * s1);
        const float gv = g[(size_t)b * C + c];
        const float v = dg * (gv * (1.f - gv));
        sda[c] = v;
        da[(size_t)b * C + c] = v;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int j = wave; j < Cr; j += 4) {
        double acc = 0.0;
        for (int c = lane; c < C; c += 64) acc += (double)W2[(size_t)c * Cr + j] * (double)sda[c];
        acc = se_wave_sum(acc);
        const float v = u[(size_t)b * Cr + j] > 0.f ? (float)acc : 0.f;
        if (lane == 0) {
            sdu[j] = v;
            du[(size_t)b * Cr + j] = v;
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        double acc = 0.0;
        for (int j = 0; j < Cr; ++j) acc += (double)W1[(size_t)j * C + c] * (double)sdu[j];
        dq[(size_t)b * C + c] = (float)acc;
        dq[((size_t)B + b) * C + c] = (float)(acc / hw);
    }
}

// ---- backward finalize: sums over the utterances, fp64, fixed order ----------------------------------------------------------
// blockIdx.y == 0: the BatchNorm-backward statistics of dz = g e + dq / HW from the tables,
//     sum dz       = sum_b (g S1 + dq)
//     sum dz xhat  = sum_b invstd (g (S2 - mean S1) + dq (sums / HW - mean))
//   -> dbeta, dgamma, coef[3][C] = (gamma invstd, sum dz / n, sum dz xhat / n), n = B HW, and the operand-scale bound of
//   draw = k1 (dz - m1 - xhat m2): |dz| <= A + max_b |dq / HW| because 0 <= g <= 1 (A = absmax of dout, or of e per channel).
// blockIdx.y == j + 1: dW1[j][c] = sum_b du[b][j] q[b][c], dW2[c][j] = sum_b da[b][c] u[b][j]
__device__ inline float se_bnbwd_bound(float k1, float m1, float m2, float mean, float invstd, float A, float R) {
    const float xh = (R + fabsf(mean)) * fabsf(invstd);
    return fabsf(k1) * (A + fabsf(m1) + xh * fabsf(m2)) * (1.f + 1.52587890625e-05f);
}

__global__ __launch_bounds__(256) void se_gate_finalize_kernel(const double* __restrict__ S, const double* __restrict__ sums,
                                                               const float* __restrict__ q, const float* __restrict__ u,
                                                               const float* __restrict__ g, const float* __restrict__ da,
                                                               const float* __restrict__ du, const float* __restrict__ dq,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma, float* __restrict__ dW1,
                                                               float* __restrict__ dW2, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, float* __restrict__ coef, int accumulate,
                                                               int B, int C, int Cr, double hw,
                                                               const unsigned* __restrict__ amax_in,
                                                               const unsigned* __restrict__ raw_amax,
                                                               const unsigned* __restrict__ chan_amax,
                                                               unsigned* __restrict__ est_out) {
    __shared__ double red[8][32][2];
    __shared__ float redm[8][32];
    const int tid = threadIdx.x, cl = tid & 31, row = tid >> 5;
    const int c = blockIdx.x * 32 + cl;          // C % 32 == 0: always a channel
    double s = 0.0, ss = 0.0;
    float mq = 0.f;
    if (blockIdx.y == 0) {
        const double mu = (double)mean[c], is = (double)invstd[c];
        for (int b = row; b < B; b += 8) {
            const size_t o = (size_t)b * C + c;
            const double s1 = S[((size_t)b * 2 + 0) * C + c], s2 = S[((size_t)b * 2 + 1) * C + c];
            const double gv = (double)g[o], dqv = (double)dq[o];
            s += gv * s1 + dqv;
            ss += is * (gv * (s2 - mu * s1) + dqv * (sums[o] / hw - mu));
            mq = fmaxf(mq, fabsf(dq[(size_t)B * C + o]));
        }
    } else {
        const int j = blockIdx.y - 1;
        for (int b = row; b < B; b += 8) {
            const size_t o = (size_t)b * C + c;
            s += (double)du[(size_t)b * Cr + j] * (double)q[o];
            ss += (double)da[o] * (double)u[(size_t)b * Cr + j];
        }
    }
    red[row][cl][0] = s;
    red[row][cl][1] = ss;
    redm[row][cl] = mq;
    __syncthreads();
    if (row != 0) return;
    for (int k = 1; k < 8; ++k) {
        s += red[k][cl][0];
        ss += red[k][cl][1];
        mq = fmaxf(mq, redm[k][cl]);
    }
    if (blockIdx.y == 0) {
        const double count = (double)B * hw;
        dbeta[c] = accumulate ? dbeta[c] + (float)s : (float)s;
        dgamma[c] = accumulate ? dgamma[c] + (float)ss : (float)ss;
        const float k1 = gamma[c] * invstd[c], m1 = (float)(s / count), m2 = (float)(ss / count);
        coef[c] = k1;
        coef[C + c] = m1;
        coef[2 * C + c] = m2;
        if (est_out) {
            const float A = (chan_amax ? __uint_as_float(chan_amax[c]) : __uint_as_float(*amax_in)) + mq;
            const float e = se_bnbwd_bound(k1, m1, m2, mean[c], invstd[c], A, __uint_as_float(*raw_amax));
            const unsigned bits = __float_as_uint(e);
            if (bits > __hip_atomic_load(est_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(est_out, bits);
        }
    } else {
        const int j = blockIdx.y - 1;
        float* p1 = dW1 + (size_t)j * C + c;
        float* p2 = dW2 + (size_t)c * Cr + j;
        *p1 = accumulate ? *p1 + (float)s : (float)s;
        *p2 = accumulate ? *p2 + (float)ss : (float)ss;
    }
}

extern "C" int spk_se_bwd_gate(const double* S, const double* sums, const float* q, const float* u, const float* g,
                               const float* W1, const float* W2, const float* mean, const float* invstd, const float* scale,
                               const float* shift, const float* gamma, float* da, float* du, float* dq, float* dW1, float* dW2,
                               float* dgamma, float* dbeta, float* coef, int accumulate, int B, int C, int Cr, long long HW,
                               const unsigned* amax_in, const unsigned* raw_amax, const unsigned* chan_amax, unsigned* est_out,
                               void* stream) {
    SPK_REQUIRE(S && sums && q && u && g && W1 && W2 && mean && invstd && scale && shift && gamma && da && du && dq && dW1 && dW2
                    && dgamma && dbeta && coef, "spk_se_bwd_gate: null pointer");
    SPK_REQUIRE(B > 0 && HW > 0 && se_c_ok(C) && Cr >= 1 && Cr <= SE_MAX_CR, "spk_se_bwd_gate: B=%d HW=%lld C=%d Cr=%d", B, HW, C, Cr);
    SPK_REQUIRE(!est_out || ((amax_in || chan_amax) && raw_amax), "spk_se_bwd_gate: est_out needs amax_in (or chan_amax) and raw_amax");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(se_gate_chain_kernel, dim3(B), dim3(256), 0, st, S, u, g, scale, shift, W1, W2, da, du, dq, B, C, Cr,
                       (double)HW);
    SPK_LAUNCH_CHECK("spk_se_bwd_gate(chain)");
    hipLaunchKernelGGL(se_gate_finalize_kernel, dim3(C / 32, 1 + Cr), dim3(256), 0, st, S, sums, q, u, g, da, du, dq, mean, invstd,
                       gamma, dW1, dW2, dgamma, dbeta, coef, accumulate, B, C, Cr, (double)HW, amax_in, raw_amax, chan_amax,
                       est_out);
    SPK_LAUNCH_CHECK("spk_se_bwd_gate");
    return 0;
}

// ---- backward apply: e = dout [out > 0]; dz = g e + dq / HW; draw = k1 (dz - m1 - xhat m2) ---------------------------------
// draw as fp32, or as an f16 pair tensor under the bound in pair_scale; e (the shortcut gradient) only when e_out is given
// (it may alias dout: every thread reads its group before it writes it).
__global__ __launch_bounds__(256) void se_bwd_apply_kernel(const float* dout, const float* __restrict__ raw,
                                                           const float* __restrict__ act, const float* __restrict__ gate,
                                                           const float* __restrict__ dqs, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ coef,
                                                           float* __restrict__ draw, float* e_out, unsigned nq, int C, int mode,
                                                           unsigned* __restrict__ amax_out,
                                                           const unsigned* __restrict__ pair_scale) {
    const int b = blockIdx.y;
    const int c0 = (threadIdx.x * 4) & (C - 1);
    const f32x4 pmu = *(const f32x4*)(mean + c0), pis = *(const f32x4*)(invstd + c0), pk1 = *(const f32x4*)(coef + c0);
    const f32x4 pm1 = *(const f32x4*)(coef + C + c0), pm2 = *(const f32x4*)(coef + 2 * C + c0);
    const f32x4 pg = *(const f32x4*)(gate + (size_t)b * C + c0), pdq = *(const f32x4*)(dqs + (size_t)b * C + c0);
    const float sig = pair_scale ? spk_sigma_from_amax_bits(*pair_scale) : 1.f;
    const size_t base = (size_t)b * nq;
    const unsigned stride = gridDim.x * 256u;
    float mx = 0.f;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < nq; i += stride) {
        const size_t gi = base + i, off = gi * 4;
        const f32x4 rv = se_ld(raw + off);
        f32x4 d = se_ld(dout + off);
        if (mode == MASK_BITS) {
            const unsigned bits = ((const unsigned*)act)[gi >> 3] >> (c0 & 31);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = ((bits >> k) & 1u) ? d[k] : 0.f;
        } else {
            const f32x4 a = *(const f32x4*)(act + off);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = a[k] > 0.f ? d[k] : 0.f;
        }
        const f32x4 dz = pg * d + pdq;
        const f32x4 xh = (rv - pmu) * pis;
        const f32x4 o = pk1 * (dz - pm1 - xh * pm2);
        if (e_out) se_st(e_out + off, d);
        if (pair_scale) {
            uint2 t0, t1;
            split2h(o, sig, t0, t1);
            se_st(draw + off, spk_pair_pack(t0, t1));
        } else
            se_st(draw + off, o);
        mx = fmaxf(fmaxf(mx, fmaxf(fabsf(o[0]), fabsf(o[1]))), fmaxf(fabsf(o[2]), fabsf(o[3])));
    }
    if (amax_out) spk_wave_amax_commit(mx, amax_out);
}

extern "C" int spk_se_bwd_apply(const float* dout, const float* raw, const float* act, const float* gate, const float* dqs,
                                const float* mean, const float* invstd, const float* coef, float* draw, float* e_out, int B,
                                long long HW, int C, int mask_mode, unsigned* amax_out, const unsigned* pair_scale, void* stream) {
    SPK_REQUIRE(dout && raw && act && gate && dqs && mean && invstd && coef && draw, "spk_se_bwd_apply: null pointer");
    SPK_REQUIRE(B > 0 && B <= 65535 && HW > 0 && se_c_ok(C), "spk_se_bwd_apply: B=%d HW=%lld C=%d", B, HW, C);
    SPK_REQUIRE(mask_mode == MASK_ACT || mask_mode == MASK_BITS, "spk_se_bwd_apply: mask_mode=%d (MASK_ACT or MASK_BITS)", mask_mode);
    const long long nq = HW * C / 4;
    SPK_REQUIRE(nq < 2147483647LL / 8, "spk_se_bwd_apply: %lld values per utterance exceed the 32-bit group index of the kernel", nq * 4);
    hipLaunchKernelGGL(se_bwd_apply_kernel, se_apply_grid(nq, B), dim3(256), 0, (hipStream_t)stream, dout, raw, act, gate, dqs, mean,
                       invstd, coef, draw, e_out, (unsigned)nq, C, mask_mode, amax_out, pair_scale);
    SPK_LAUNCH_CHECK("spk_se_bwd_apply");
    return 0;
}
