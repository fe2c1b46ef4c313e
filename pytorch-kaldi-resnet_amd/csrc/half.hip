// Half-precision extraction (precision="f16"): fp16 activations in HBM, ONE fp16 product per
// multiply-accumulate on v_mfma_f32_16x16x32_f16 with fp32 accumulation, fp32 epilogue, one rounding to fp16 (nearest even,
// subnormals kept).  Eval mode only: BatchNorm is the fp32 (scale, shift) row pair of spk_bn_eval_coeffs, never folded into the
// weights.  A stored value that does not fit fp16 is stored as the conversion gives it (+-inf) and counted per utterance in
// ovf[b]; nothing is clamped.  The kernels ADD to ovf: the caller zeroes it before the first launch of a forward.
//
// Convolution as a GEMM with the OUTPUT CHANNELS on the accumulator's row index and the pixels on its column:
//   D[cout][pixel] = sum_k W[cout][k] * X[k][pixel],   k = (tap, cin), one k-step = 32 consecutive channels of one tap.
// Lane l of v_mfma_f32_16x16x32_f16 holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15], j = 0..7, and
// D[row 4 (l >> 4) + r][col l & 15] in register r: the B fragment of a lane is 8 consecutive channels of ONE pixel (a 16-byte LDS
// read of NHWC fp16, no transpose) and its four results are four consecutive channels of one pixel (one 8-byte store).
//
// Packed weights (spk_h16_pack_conv_weight): fragment images of 1 KB in the order [tap][Cin / 32][Cout / 16][lane 64][8 halfs],
//   lane l, element j  =  w[cout = 16 m + (l & 15)][cin = 32 s + 8 (l >> 4) + j][tap]      (spk_h16_packed_bytes = 2 Cout Cin KH KW)
// so a block copies the images of its channel tile into LDS with 16-byte moves and a wave reads a fragment lane-linearly.
//
// One block = 256 threads = H16_TH x H16_TW output pixels x 16 MREP output channels (MREP = 4, or 2 at Cout = 32) of one image;
// wave w owns output rows 2 w and 2 w + 1 (four 16-pixel column tiles) and all the block's channels: MREP x 4 accumulator tiles.
// Per pass (a 32-channel slice of Cin; at 3x3 stride 2 also one tap row) the block stages the halo of the slice and the weight
// images of the pass in LDS (through registers, loaded one pass ahead), then every wave runs taps x MREP x 4 matrix instructions
// on 16-byte LDS reads.  The halo lies in
// four 8-channel planes of 16 bytes per pixel: a fragment read covers 16 consecutive pixels of each plane, which the four lane
// groups of ds_read_b128 take without a bank conflict (plane size a multiple of 256 B); at 3x3 stride 2 the columns are stored
// even ones first so that the 16 pixels of a read are consecutive again.  LDS stays below 64 KB per block (two blocks per CU).
#include "spk_common.h"

#define H16_TH 8
#define H16_TW 32
#define H16_TPB 4            // tiles per block ...
#define H16_TPB_MIN 8192     // ... from this many (tile, channel tile) pairs on: 2048 blocks, eight per CU

typedef _Float16 h16;

extern "C" int spk_stem_fwd_blocks(int B, int F, int T);      // stem.hip: the stem's grid

template <int KS, int ST, int MREP>
struct H16Geo {
    static constexpr bool ROWPASS = KS == 3 && ST == 2;                      // one pass per tap row
    static constexpr int HR = (KS == 3 && ST == 1) ? H16_TH + 2 : H16_TH;     // halo rows in LDS
    static constexpr int HC = KS == 1 ? H16_TW : (ST == 1 ? H16_TW + 2 : 2 * H16_TW + 2);   // halo columns (stride 2: 33 even + 33 odd)
    static constexpr int NPIX = HR * HC;
    static constexpr int NPIXR = (NPIX + 15) & ~15;
    static constexpr int PLANE = NPIXR * 16;                                 // bytes of one 8-channel plane
    static constexpr int TAPS = KS == 1 ? 1 : (ROWPASS ? 3 : 9);              // taps of one pass
    static constexpr int NPASS = ROWPASS ? 3 : 1;                             // passes per Cin slice
    static constexpr int WOFF = 4 * PLANE;
    static constexpr int LDS = WOFF + TAPS * MREP * 1024;
    static_assert(PLANE % 256 == 0, "plane size keeps the four planes on the same banks");
    static_assert(LDS <= 65536, "static LDS");
};

// adds the per-lane counts of not-finite stored values to ovf[b]: one atomic per wave and utterance, nothing when the wave stored
// only finite values (every healthy wave).  Every lane of the wave must call it.
static __device__ __forceinline__ void h16_ovf_commit(int cnt, int b, int* __restrict__ ovf) {
    unsigned long long m = __builtin_amdgcn_ballot_w64(cnt > 0);
    while (m) {
        const int src = (int)__builtin_ctzll(m);
        const int bb = __shfl(b, src, 64);
        int c = b == bb ? cnt : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
        if ((int)(threadIdx.x & 63) == src) atomicAdd(ovf + bb, c);
        if (b == bb) cnt = 0;
        m = __builtin_amdgcn_ballot_w64(cnt > 0);
    }
}

static __device__ __forceinline__ int h16_not_finite(h16 v) {
    return (__builtin_bit_cast(unsigned short, v) & 0x7c00u) == 0x7c00u;
}

// ---- weight pack: OIHW fp32 -> fp16 fragment images (round to nearest even; a value outside fp16's range becomes +-inf) ------------
__global__ __launch_bounds__(256) void h16_pack_kernel(const float* __restrict__ w, h16* __restrict__ out, int Cout, int Cin,
                                                       int taps) {
    const long long total = (long long)Cout * Cin * taps;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx & 7), l = (int)((idx >> 3) & 63);
    long long r = idx >> 9;
    const int mt = Cout / 16, ncs = Cin / 32;
    const int m = (int)(r % mt);
    r /= mt;
    const int s = (int)(r % ncs);
    const int t = (int)(r / ncs);
    const int co = 16 * m + (l & 15), ci = 32 * s + 8 * (l >> 4) + j;
    out[idx] = (h16)w[((size_t)co * Cin + ci) * taps + t];
}

// ---- stem: the arithmetic of stem_fwd_kernel (stem.hip) with eval BatchNorm + ReLU, stored as fp16 ------------------------------
__global__ __launch_bounds__(256) void h16_stem_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ scale, const float* __restrict__ shift,
                                                       h16* __restrict__ out, const int* __restrict__ len, int* __restrict__ ovf,
                                                       int B, int F, int T) {
    const int tid = threadIdx.x, cg = tid & 3, pl = tid >> 2;
    float wr[9][8], es[8], eh[8];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 8; ++c) wr[t][c] = w[(cg * 8 + c) * 9 + t];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        es[c] = scale[cg * 8 + c];
        eh[c] = shift[cg * 8 + c];
    }
    const int FT = F * T;
    const long long NP = (long long)B * FT;
    // the loop bound is the same for every thread of the block, so that whole waves reach h16_ovf_commit
    for (long long base = (long long)blockIdx.x * 64; base < NP; base += (long long)gridDim.x * 64) {
        const long long p = base + pl;
        const bool live = p < NP;
        const int b = live ? (int)(p / FT) : 0;
        int bad = 0;
        if (live) {
            const int rem = (int)(p - (long long)b * FT);
            const int f = rem / T, t0 = rem - f * T;
            const float* xb = x + (size_t)b * FT;
            const int Tb = len ? min(len[b], T) : T;
            float xv[9];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int ff = f + kh - 1, tt = t0 + kw - 1;
                    xv[kh * 3 + kw] = (ff >= 0 && ff < F && tt >= 0 && tt < Tb) ? xb[ff * T + tt] : 0.f;
                }
            const bool tail = t0 >= Tb;
            f16x8 o;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                float v = 0.f;
#pragma unroll
                for (int t = 0; t < 9; ++t) v = fmaf(xv[t], wr[t][c], v);
                v = fmaxf(v * es[c] + eh[c], 0.f);
                if (tail) v = 0.f;
                o[c] = (h16)v;
                bad += h16_not_finite(o[c]);
            }
            *(f16x8*)(out + (size_t)p * 32 + cg * 8) = o;
        }
        h16_ovf_commit(bad, b, ovf);
    }
}

// ---- the convolution -----------------------------------------------------------------------------------------------------------
// A block owns `tpb` consecutive tiles (linear index over image, tile row, tile column) of one output-channel tile.  Its passes -
// (tile, Cin slice, tap row) - are software-pipelined through registers: the global loads of pass p + 1 are issued before the
// matrix instructions of pass p and written to LDS after them, across tile boundaries too, so that the load latency hides behind
// the compute of the block itself.  With one pass per tile (Cin = 32, not 3x3 stride 2) the weight images are the same for every
// tile: they are staged once.
struct H16Tile {
    int b, oy0, ox0;
};
static __device__ __forceinline__ H16Tile h16_tile(unsigned t, int tiles_x, int tiles_y) {
    H16Tile r;
    const unsigned row = t / (unsigned)tiles_x;
    r.ox0 = (int)(t - row * (unsigned)tiles_x) * H16_TW;
    r.b = (int)(row / (unsigned)tiles_y);
    r.oy0 = (int)(row - (unsigned)r.b * (unsigned)tiles_y) * H16_TH;
    return r;
}

template <int KS, int ST, int MREP>
__global__ __launch_bounds__(256, 2) void h16_conv_kernel(const h16* __restrict__ in, const h16* __restrict__ wpk,
                                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                                          const h16* __restrict__ add, h16* __restrict__ out,
                                                          const int* __restrict__ wlen, int* __restrict__ ovf, int IH, int IW, int OH,
                                                          int OW, int Cin, int Cout, int tiles_x, int tiles_y, unsigned tiles,
                                                          int tpb, int relu) {
    using G = H16Geo<KS, ST, MREP>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[G::LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, x16 = lane & 15, q = lane >> 4;
    const int nzc = Cout / (16 * MREP);
    const int zc = (int)(blockIdx.x % (unsigned)nzc);
    const unsigned t0 = blockIdx.x / (unsigned)nzc * (unsigned)tpb;          // first tile of the block
    const int ntile = (int)min((unsigned)tpb, tiles - t0);
    const int ncs = Cin >> 5, mtiles = Cout >> 4;
    const size_t img = (size_t)IH * IW * Cin;

    f32x4 acc[MREP][4];
#pragma unroll
    for (int m = 0; m < MREP; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    constexpr int HL = (G::NPIXR / 16 + 3) / 4;                  // 16-byte halo pieces per thread and pass
    constexpr int WL = (G::TAPS * MREP * 64 + 255) / 256;        // 16-byte weight pieces per thread and pass
    // (named registers, not arrays: an array that lives across the pass loop ends up in scratch memory)
    uint4 h0, h1, h2, h3, h4, h5, h6, h7, h8, w0, w1, w2, w3, w4, w5, w6, w7, w8;
    static_assert(HL <= 9 && WL <= 9, "staging registers");
    const int npass = ncs * G::NPASS;                            // passes per tile
    const int total = ntile * npass;
    const bool wfix = npass == 1;                                // the weight images do not change from pass to pass
    const auto halo_put = [=](int u, uint4 v) {
        const int pix = (wave + 4 * u) * 16 + x16;
        if (pix < G::NPIXR) *(uint4*)(lds + q * G::PLANE + pix * 16) = v;
    };
    const auto weight_put = [=](int u, uint4 v) {
        const int i = tid + 256 * u;
        if (i < G::TAPS * MREP * 64) *(uint4*)(lds + G::WOFF + i * 16) = v;
    };
    // halo: a wave instruction takes 16 pixels x 64 bytes of the slice, in the order it will write and read them
    const auto halo_get = [=](int u, int cs, int tp, H16Tile t) {
        const int iy_base = KS == 1 ? t.oy0 * ST : (G::ROWPASS ? t.oy0 * 2 - 1 + tp : t.oy0 - 1);
        const int ix_base = KS == 1 ? t.ox0 * ST : t.ox0 * ST - 1;
        const int pix = (wave + 4 * u) * 16 + x16;
        const int hy = pix / G::HC, hc = pix - hy * G::HC;
        int iy, ix;
        if (KS == 1) {
            iy = iy_base + hy * ST;
            ix = ix_base + hc * ST;
        } else if (G::ROWPASS) {
            iy = iy_base + hy * 2;
            ix = ix_base + (hc < 33 ? 2 * hc : 2 * (hc - 33) + 1);
        } else {
            iy = iy_base + hy;
            ix = ix_base + hc;
        }
        uint4 v = (uint4){0u, 0u, 0u, 0u};
        if (pix < G::NPIX && iy >= 0 && iy < IH && ix >= 0 && ix < IW)
            v = *(const uint4*)(in + (size_t)t.b * img + ((size_t)iy * IW + ix) * Cin + cs * 32 + q * 8);
        return v;
    };
    // weight images of the pass: TAPS runs of MREP KB
    const auto weight_get = [=](int u, int cs, int tp) {
        const int i = tid + 256 * u;
        uint4 v = (uint4){0u, 0u, 0u, 0u};
        if (i < G::TAPS * MREP * 64) {
            const int tl = i / (MREP * 64), r = i - tl * (MREP * 64);
            const int t = G::ROWPASS ? tp * 3 + tl : tl;
            v = *(const uint4*)(wpk + (((size_t)t * ncs + cs) * mtiles + (size_t)zc * MREP) * 512 + (size_t)r * 8);
        }
        return v;
    };
#define H16_EACH(OP) OP(0) OP(1) OP(2) OP(3) OP(4) OP(5) OP(6) OP(7) OP(8)
#define H16_PUT_H(u) \
    if constexpr (u < HL) halo_put(u, h##u);
#define H16_PUT_W(u) \
    if constexpr (u < WL) weight_put(u, w##u);
#define H16_GET_H(u) \
    if constexpr (u < HL) h##u = halo_get(u, cs, tp, ft);
#define H16_GET_W(u) \
    if constexpr (u < WL) w##u = weight_get(u, cs, tp);
    int cs = 0, tp = 0, fi = 0;              // the pass being fetched: slice, tap row, tile of the block
    H16Tile ft = h16_tile(t0, tiles_x, tiles_y);
    int ci = 0, left = npass;                // the pass being computed: tile of the block, passes left in it
    H16Tile ct = ft;
#pragma unroll 1
    for (int p = -1; p < total; ++p) {
        if (p >= 0) {
            __syncthreads();                 // the reads of the previous pass are done
            H16_EACH(H16_PUT_H)
            if (!wfix || p == 0) {
                H16_EACH(H16_PUT_W)
            }
            __syncthreads();
        }
        if (p + 1 < total) {
            H16_EACH(H16_GET_H)
            if (!wfix || p < 0) {
                H16_EACH(H16_GET_W)
            }
            if (++tp == G::NPASS) {
                tp = 0;
                if (++cs == ncs) {
                    cs = 0;
                    ft = h16_tile(t0 + (unsigned)min(++fi, ntile - 1), tiles_x, tiles_y);
                }
            }
        }
        if (p < 0) continue;
#pragma unroll
        for (int tl = 0; tl < G::TAPS; ++tl) {
            const int ky = KS == 1 ? 0 : (G::ROWPASS ? 0 : tl / 3), kx = KS == 1 ? 0 : tl % 3;
            f16x8 a[MREP];
#pragma unroll
            for (int m = 0; m < MREP; ++m) a[m] = *(const f16x8*)(lds + G::WOFF + (tl * MREP + m) * 1024 + lane * 16);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int row = wave * 2 + (n >> 1), col = (n & 1) * 16 + x16;
                const int pix = G::ROWPASS ? row * G::HC + (kx & 1) * 33 + col + (kx >> 1) : (row + ky) * G::HC + col + kx;
                const f16x8 bf = *(const f16x8*)(lds + q * G::PLANE + pix * 16);
#pragma unroll
                for (int m = 0; m < MREP; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[m], bf, acc[m][n], 0, 0, 0);
            }
        }
        if (--left > 0) continue;
        // the tile is complete.  Epilogue in fp32: affine, residual, ReLU, length mask, ONE rounding to fp16
        const int b = ct.b;
        const int wl = wlen ? wlen[b] : OW;
        int bad = 0;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int oy = ct.oy0 + wave * 2 + (n >> 1), ox = ct.ox0 + (n & 1) * 16 + x16;
            if (oy < OH && ox < OW) {
                const size_t pix = ((size_t)b * OH + oy) * OW + ox;
#pragma unroll
                for (int m = 0; m < MREP; ++m) {
                    const int c = (zc * MREP + m) * 16 + q * 4;
                    const f32x4 sc = *(const f32x4*)(scale + c), sh = *(const f32x4*)(shift + c);
                    f32x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaf(acc[m][n][r], sc[r], sh[r]);
                    if (add) {
                        const f16x4 ad = *(const f16x4*)(add + pix * Cout + c);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] += (float)ad[r];
                    }
                    if (relu) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                    }
                    if (ox >= wl) v = (f32x4){0.f, 0.f, 0.f, 0.f};
                    const f16x4 o = __builtin_convertvector(v, f16x4);      // v_cvt_f16_f32: nearest even, subnormals kept
#pragma unroll
                    for (int r = 0; r < 4; ++r) bad += h16_not_finite(o[r]);
                    *(f16x4*)(out + pix * Cout + c) = o;
                }
            }
        }
        h16_ovf_commit(bad, b, ovf);
#pragma unroll
        for (int m = 0; m < MREP; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
        left = npass;
        ct = h16_tile(t0 + (unsigned)min(++ci, ntile - 1), tiles_x, tiles_y);
    }
#undef H16_GET_W
#undef H16_GET_H
#undef H16_PUT_W
#undef H16_PUT_H
#undef H16_EACH
}

// ---- statistics pooling: the formulas and the order of stats_pool_fwd_kernel (pool.hip) on fp16 input, fp32 arithmetic ----------
__global__ __launch_bounds__(256) void h16_stats_pool_kernel(const h16* __restrict__ x, float* __restrict__ out, int B, int H,
                                                             int Wp, int C, int mode, const int* __restrict__ wlen) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)B * H * C;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long bh = idx / C;
    const int h = (int)(bh % H);
    const int b = (int)(bh / H);
    const h16* p = x + (size_t)bh * Wp * C + c;
    const int W = wlen ? max(1, min(wlen[b], Wp)) : Wp;
    float s = 0.f;
    for (int w = 0; w < W; ++w) s += (float)p[(size_t)w * C];
    const float mean = s / (float)W;
    if (mode == 0) {
        out[(size_t)b * C * H + (size_t)c * H + h] = mean;
        return;
    }
    float m2 = 0.f;
    for (int w = 0; w < W; ++w) {
        const float d = (float)p[(size_t)w * C] - mean;
        m2 = fmaf(d, d, m2);
    }
    float* o = out + (size_t)b * C * 2 * H + (size_t)c * 2 * H;
    o[h] = m2 / (float)(W - 1);
    o[H + h] = sqrtf(mean);
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------
static bool h16_chan_ok(int c) { return c == 32 || c == 64 || c == 128 || c == 256; }

extern "C" int spk_h16_conv_tile(int which) {
    return which == 0 ? H16_TH : which == 1 ? H16_TW : which == 2 ? H16_TPB : H16_TPB_MIN;
}

extern "C" int spk_h16_packed_bytes(int Cout, int Cin, int KH, int KW) {
    SPK_REQUIRE(h16_chan_ok(Cout) && h16_chan_ok(Cin), "spk_h16_packed_bytes: Cin=%d Cout=%d (32, 64, 128 or 256)", Cin, Cout);
    SPK_REQUIRE((KH == 1 && KW == 1) || (KH == 3 && KW == 3), "spk_h16_packed_bytes: kernel %dx%d (1x1 or 3x3)", KH, KW);
    return 2 * Cout * Cin * KH * KW;
}

extern "C" int spk_h16_pack_conv_weight(const float* w, void* out, int Cout, int Cin, int KH, int KW, void* stream) {
    SPK_REQUIRE(h16_chan_ok(Cout) && h16_chan_ok(Cin), "spk_h16_pack_conv_weight: Cin=%d Cout=%d (32, 64, 128 or 256)", Cin, Cout);
    SPK_REQUIRE((KH == 1 && KW == 1) || (KH == 3 && KW == 3), "spk_h16_pack_conv_weight: kernel %dx%d (1x1 or 3x3)", KH, KW);
    SPK_REQUIRE(w && out, "spk_h16_pack_conv_weight: null pointer");
    const long long total = (long long)Cout * Cin * KH * KW;
    hipLaunchKernelGGL(h16_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (h16*)out, Cout,
                       Cin, KH * KW);
    SPK_LAUNCH_CHECK("spk_h16_pack_conv_weight");
    return 0;
}

extern "C" int spk_h16_stem_fwd(const float* x, const float* w, const float* scale, const float* shift, void* out,
                                const int* wlen, int* ovf, int B, int F, int T, void* stream) {
    SPK_REQUIRE(B > 0 && F > 0 && T > 0, "spk_h16_stem_fwd: empty input");
    SPK_REQUIRE(x && w && scale && shift && out && ovf, "spk_h16_stem_fwd: null pointer");
    hipLaunchKernelGGL(h16_stem_kernel, dim3(spk_stem_fwd_blocks(B, F, T)), dim3(256), 0, (hipStream_t)stream, x, w, scale, shift,
                       (h16*)out, wlen, ovf, B, F, T);
    SPK_LAUNCH_CHECK("spk_h16_stem_fwd");
    return 0;
}

template <int KS, int ST, int MREP>
static void h16_conv_launch(unsigned grid, hipStream_t s, const h16* in, const h16* wpk, const float* scale, const float* shift,
                            const h16* add, h16* out, const int* wlen, int* ovf, int IH, int IW, int OH, int OW, int Cin, int Cout,
                            int tx, int ty, unsigned tiles, int tpb, int relu) {
    hipLaunchKernelGGL((h16_conv_kernel<KS, ST, MREP>), dim3(grid), dim3(256), 0, s, in, wpk, scale, shift, add, out, wlen, ovf, IH,
                       IW, OH, OW, Cin, Cout, tx, ty, tiles, tpb, relu);
}

extern "C" int spk_h16_conv_fwd(const void* in, const void* wpk, const float* scale, const float* shift, const void* add, void* out,
                                const int* wlen, int* ovf, int B, int IH, int IW, int Cin, int Cout, int ksize, int stride,
                                int relu, void* stream) {
    SPK_REQUIRE(h16_chan_ok(Cin) && h16_chan_ok(Cout), "spk_h16_conv_fwd: Cin=%d Cout=%d (32, 64, 128 or 256)", Cin, Cout);
    SPK_REQUIRE(ksize == 1 || ksize == 3, "spk_h16_conv_fwd: ksize=%d (1 or 3)", ksize);
    SPK_REQUIRE(stride == 1 || stride == 2, "spk_h16_conv_fwd: stride=%d (1 or 2)", stride);
    SPK_REQUIRE(B > 0 && IH > 0 && IW > 0, "spk_h16_conv_fwd: empty input");
    SPK_REQUIRE(in && wpk && scale && shift && out && ovf, "spk_h16_conv_fwd: null pointer");
    // pad 1 at 3x3, pad 0 at 1x1: the output size of both is ceil(I / stride)
    const int OH = (IH + stride - 1) / stride, OW = (IW + stride - 1) / stride;
    const int tx = spk_ceil_div(OW, H16_TW), ty = spk_ceil_div(OH, H16_TH);
    const int mrep = Cout == 32 ? 2 : 4;
    const int nzc = Cout / (16 * mrep);
    const long long tiles = (long long)B * tx * ty;
    SPK_REQUIRE(tiles * nzc <= 0x7fffffffLL, "spk_h16_conv_fwd: %lld tiles exceed the grid", tiles * nzc);
    // tiles per block: enough blocks to fill the chip several times over come first, then the longer pipeline
    const int tpb = tiles * nzc >= H16_TPB_MIN ? H16_TPB : 1;
    const long long blocks = (tiles + tpb - 1) / tpb * nzc;
    SPK_REQUIRE((long long)B * IH * IW * Cin <= (1LL << 40), "spk_h16_conv_fwd: input too large");
    const hipStream_t s = (hipStream_t)stream;
#define H16_GO(KS, ST, MR)                                                                                                       \
    h16_conv_launch<KS, ST, MR>((unsigned)blocks, s, (const h16*)in, (const h16*)wpk, scale, shift, (const h16*)add, (h16*)out, wlen, \
                                ovf, IH, IW, OH, OW, Cin, Cout, tx, ty, (unsigned)tiles, tpb, relu)
    if (ksize == 3 && stride == 1) {
        if (mrep == 2) H16_GO(3, 1, 2); else H16_GO(3, 1, 4);
    } else if (ksize == 3) {
        if (mrep == 2) H16_GO(3, 2, 2); else H16_GO(3, 2, 4);
    } else if (stride == 1) {
        if (mrep == 2) H16_GO(1, 1, 2); else H16_GO(1, 1, 4);
    } else {
        if (mrep == 2) H16_GO(1, 2, 2); else H16_GO(1, 2, 4);
    }
#undef H16_GO
    SPK_LAUNCH_CHECK("spk_h16_conv_fwd");
    return 0;
}

extern "C" int spk_h16_stats_pool_fwd(const void* x, float* out, const int* wlen, int B, int H, int W, int C, int mode,
                                      void* stream) {
    SPK_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, "spk_h16_stats_pool_fwd: empty input");
    SPK_REQUIRE(mode == 0 || mode == 1, "spk_h16_stats_pool_fwd: mode=%d", mode);
    SPK_REQUIRE(x && out, "spk_h16_stats_pool_fwd: null pointer");
    const long long total = (long long)B * H * C;
    hipLaunchKernelGGL(h16_stats_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const h16*)x, out, B, H, W, C, mode, wlen);
    SPK_LAUNCH_CHECK("spk_h16_stats_pool_fwd");
    return 0;
}
