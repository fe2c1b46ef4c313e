// Kaldi's one-byte compressed matrix ('CM ') on the device: the decode that turns a batch of codes as they lie in the archive into
// the fp32 [B][F][T] input of the model, and the compression that writes such records from a batch of features.
// Format and contract: DESIGN.md section 6g (Kaldi's compressed-matrix.h; the reference reads the format in
// scripts/kaldi_io.py:427-460 and its prepare_feats_for_egs.sh writes it by default).
//
// A record holds (min, range) of the whole matrix, per column (= mel bin) four 16-bit points p0 <= p25 <= p75 <= p100 of the
// column's distribution, and one byte per value, column-major - the frames of one bin are contiguous, which is the time-innermost
// layout of a batch row.  With U(u) = min + (range * (1 / 65535.f)) * u and P = U(p):
//     value(c) = c <= 64 ? P0 + (P25 - P0) * c * (1/64.f) : c <= 192 ? P25 + (P75 - P25) * (c - 64) * (1/128.f)
//                                                                      : P75 + (P100 - P75) * (c - 192) * (1/63.f)
// All arithmetic here is fp32 with every operation rounded on its own (never contracted into an FMA), in
// exactly this order: the decode returns the bits of the host readers (libspkio, kaldi_io.read_mat), and the compression the bytes
// of tests/cm_ref.py.
//
// spk_cm_decode: a streaming kernel, 1 byte in and 4 out per value.  The batch is taken as one flat run of B*F*T codes; a lane
// takes 16 consecutive codes starting at a 16-byte boundary of the code buffer (one 16-byte load) and stores them as four 16-byte
// stores when their place in `out` is 16-byte aligned too, as 16 4-byte stores otherwise (an output that starts 4 bytes off, an odd
// T against a shifted code buffer).  The codes before the first boundary and after the last whole 16 go to one lane each, byte by
// byte.  A run of 16 may cross rows (T is arbitrary: 203, 1): the lane follows (row, t) and reloads the row's four P values when
// the row changes; a run that lies in one row (nearly all of them at T = 300) takes straight-line code.  Measured: DESIGN.md 6g.
//
// spk_cm_compress: two launches over one workgroup per (b, f) row of x [B][F][Tcap], T[b] frames each.
//   1. cm_row_minmax: the row's min and max -> workspace (the matrix's come first, the 16-bit points are relative to them).
//   2. cm_compress_rows: every workgroup folds its matrix's F row results into (min, range); finds the order statistics s[T/4] and
//      s[3(T/4)] of its row with a radix select - 4 passes of 8 bits over the order-preserving integer image of the floats, a
//      256-bin LDS histogram per rank, the row re-read (from L2) in each pass, so no T is too long for LDS; builds the four points,
//      and encodes the row, four codes per 4-byte store where the row's alignment allows.
// Nothing past T[b] is read; a row with T[b] = 0 writes nothing.  A non-finite value (or a range that overflows) makes the
// matrix's (min, range) NaN and leaves its headers and codes unwritten: the caller reports it.
#include "spk_common.h"

namespace {

constexpr int CM_THREADS = 256;
constexpr float CM_INV65535 = 1.52590218966964e-05f;

// ---- the format's arithmetic, one rounding per operation: nothing below this line may be contracted into an FMA (the compiler's
// default for device code is to contract), and fp32 division is the correctly rounded one ----
#pragma clang fp contract(off)
__device__ __forceinline__ float cm_add(float a, float b) { return a + b; }
__device__ __forceinline__ float cm_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float cm_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float cm_div(float a, float b) { return __fdiv_rn(a, b); }

__device__ __forceinline__ float cm_u(float vmin, float scale, int u) { return cm_add(vmin, cm_mul(scale, (float)u)); }

__device__ __forceinline__ float cm_value(float4 P, unsigned c) {
    float base, d, k, s;
    if (c <= 64u) { base = P.x; d = cm_sub(P.y, P.x); k = (float)c; s = 1 / 64.f; }
    else if (c <= 192u) { base = P.y; d = cm_sub(P.z, P.y); k = (float)(c - 64u); s = 1 / 128.f; }
    else { base = P.z; d = cm_sub(P.w, P.z); k = (float)(c - 192u); s = 1 / 63.f; }
    return cm_add(base, cm_mul(cm_mul(d, k), s));
}

// clamp to [0, hi] first (NaN -> 0: a zero-width segment divides 0 by 0), then truncate
__device__ __forceinline__ unsigned cm_clamp_trunc(float f, float hi) {
    f = f >= 0.f ? (f <= hi ? f : hi) : 0.f;
    return (unsigned)(int)f;
}

__device__ __forceinline__ unsigned cm_code(float4 P, float v) {
    if (v < P.y) return cm_clamp_trunc(cm_add(cm_mul(cm_div(cm_sub(v, P.x), cm_sub(P.y, P.x)), 64.f), 0.5f), 64.f);
    if (v < P.z)
        return 64u + cm_clamp_trunc(cm_add(cm_mul(cm_div(cm_sub(v, P.y), cm_sub(P.z, P.y)), 128.f), 0.5f), 128.f);
    return 192u + cm_clamp_trunc(cm_add(cm_mul(cm_div(cm_sub(v, P.z), cm_sub(P.w, P.z)), 63.f), 0.5f), 63.f);
}

// Q(v) = (int)(clamp((v - min) / range, 0, 1) * 65535 + 0.499f)
__device__ __forceinline__ int cm_q(float v, float vmin, float vrange) {
    float f = cm_div(cm_sub(v, vmin), vrange);
    f = f >= 0.f ? (f <= 1.f ? f : 1.f) : 0.f;
    return (int)cm_add(cm_mul(f, 65535.f), 0.499f);
}

// ---- decode ----
struct CmDecodeArgs {
    const unsigned char* codes;   // [B][F][T]
    const float4* colhdr;         // [B * F] (P0, P25, P75, P100)
    const int* lengths;           // [B] or NULL
    float* out;                   // [B][F][T]
    long long N;                  // B * F * T
    long long head;               // codes before the first 16-byte boundary of the code buffer (chunk 0)
    long long nchunk;             // chunk 0, the whole 16s, the tail
    long long nrow;               // B * F
    int F, T;
};

// n codes from flat index i0 on; c16: their bytes when FULL (n == 16)
template <bool FULL>
__device__ __forceinline__ void cm_decode_run(const CmDecodeArgs& a, long long i0, int n, uint4 c16) {
    // (row, t) of the first code; 32-bit division whenever the batch allows it (the 64-bit one is a long instruction sequence)
    long long r;
    if (a.N < (1ll << 31)) r = (long long)((unsigned)i0 / (unsigned)a.T);
    else r = i0 / a.T;
    int t = (int)(i0 - r * a.T);
    float4 P = a.colhdr[r];
    int len = a.lengths ? min(max(a.lengths[(unsigned)r / (unsigned)a.F], 0), a.T) : a.T;      // nrow < 2^31
    float v[16];
    const unsigned w[4] = {c16.x, c16.y, c16.z, c16.w};
    if (FULL && t + 16 <= a.T) {          // the whole run lies in one row (15 of 16 runs and more from T = 256 on): straight-line code
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = t + j < len ? cm_value(P, (w[j >> 2] >> (8 * (j & 3))) & 255u) : 0.f;
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (!FULL && j >= n) break;
            const unsigned c = FULL ? (w[j >> 2] >> (8 * (j & 3))) & 255u : (unsigned)a.codes[i0 + j];
            v[j] = t < len ? cm_value(P, c) : 0.f;
            if (++t == a.T) {         // next row (T may be shorter than the run)
                t = 0;
                ++r;
                if (r < a.nrow) {
                    P = a.colhdr[r];
                    if (a.lengths) len = min(max(a.lengths[(unsigned)r / (unsigned)a.F], 0), a.T);
                }
            }
        }
    }
    float* o = a.out + i0;
    if (FULL && (((size_t)o) & 15) == 0) {
#pragma unroll
        for (int j = 0; j < 16; j += 4) *(float4*)(o + j) = make_float4(v[j], v[j + 1], v[j + 2], v[j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (!FULL && j >= n) break;
            o[j] = v[j];
        }
    }
}

__global__ __launch_bounds__(CM_THREADS) void cm_decode_kernel(CmDecodeArgs a) {
    const long long k = (long long)blockIdx.x * CM_THREADS + threadIdx.x;
    if (k >= a.nchunk) return;
    if (k == 0) {
        if (a.head > 0) cm_decode_run<false>(a, 0, (int)a.head, make_uint4(0, 0, 0, 0));
        return;
    }
    const long long i0 = a.head + 16 * (k - 1);
    const long long left = a.N - i0;          // > 0 by the chunk count
    if (left >= 16) cm_decode_run<true>(a, i0, 16, *(const uint4*)(a.codes + i0));
    else cm_decode_run<false>(a, i0, (int)left, make_uint4(0, 0, 0, 0));
}

// ---- compress ----
// order-preserving image of a float: a < b (as floats) => key(a) < key(b); -0 sorts below +0, which Q maps to the same point
__device__ __forceinline__ unsigned cm_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cm_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// min and max over the workgroup (all threads get them); `bad` or-ed
__device__ __forceinline__ void cm_block_minmax(float& mn, float& mx, int& bad, float* red /*[3 * waves]*/) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off, 64));
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        bad |= __shfl_xor(bad, off, 64);
    }
    constexpr int W = CM_THREADS / 64;
    const int wave = threadIdx.x >> 6;
    __syncthreads();              // red may still be read from a previous use
    if ((threadIdx.x & 63) == 0) {
        red[wave] = mn;
        red[W + wave] = mx;
        red[2 * W + wave] = bad ? 1.f : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < W; ++i) {
        mn = fminf(mn, red[i]);
        mx = fmaxf(mx, red[W + i]);
        bad |= red[2 * W + i] != 0.f;
    }
}

// ws[(b * F + f) * 2] = (min, max) of x[b][f][0 .. T[b]); (NaN, NaN) when a value is not finite; untouched when T[b] == 0
__global__ __launch_bounds__(CM_THREADS) void cm_row_minmax(const float* x, const int* T, int F, int Tcap, float* ws) {
    __shared__ float red[3 * CM_THREADS / 64];
    const int f = blockIdx.x, b = blockIdx.y;
    const int Tb = min(max(T[b], 0), Tcap);
    if (Tb == 0) return;
    const float* row = x + ((size_t)b * F + f) * Tcap;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int bad = 0;
    for (int t = threadIdx.x; t < Tb; t += CM_THREADS) {
        const float v = row[t];
        bad |= !(fabsf(v) < __builtin_inff());
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    cm_block_minmax(mn, mx, bad, red);
    if (threadIdx.x == 0) {
        const float nan = __builtin_nanf("");
        ws[((size_t)b * F + f) * 2] = bad ? nan : mn;
        ws[((size_t)b * F + f) * 2 + 1] = bad ? nan : mx;
    }
}

__global__ __launch_bounds__(CM_THREADS) void cm_compress_rows(const float* x, const int* T, int F, int Tcap, const float* ws,
                                                               float* minrange, int* hdr, unsigned char* codes, int vec) {
    __shared__ float red[3 * CM_THREADS / 64];
    __shared__ unsigned hist[2][256];
    __shared__ unsigned sel_prefix[2], sel_rank[2];
    __shared__ float4 Psh;
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int Tb = min(max(T[b], 0), Tcap);
    if (Tb == 0) return;
    // (min, range) of the matrix from its F row results
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int bad = 0;
    for (int g = tid; g < F; g += CM_THREADS) {
        const float a = ws[((size_t)b * F + g) * 2], c = ws[((size_t)b * F + g) * 2 + 1];
        bad |= (a != a) || (c != c);
        mn = fminf(mn, a);
        mx = fmaxf(mx, c);
    }
    cm_block_minmax(mn, mx, bad, red);
    if (mn == 0.f) mn = 0.f;      // a minimum of zero is stored as +0 whatever the signs of the zeros in the matrix and their order
    const float vmin = mn;
    if (mx == mn) mx = cm_add(mn, cm_add(1.f, fabsf(mn)));
    const float vrange = cm_sub(mx, vmin);
    if (bad || !(vrange < __builtin_inff())) {       // block-uniform
        if (f == 0 && tid == 0) minrange[2 * b] = minrange[2 * b + 1] = __builtin_nanf("");
        return;
    }
    if (f == 0 && tid == 0) {
        minrange[2 * b] = vmin;
        minrange[2 * b + 1] = vrange;
    }
    const size_t rb = ((size_t)b * F + f) * Tcap;
    const float* row = x + rb;
    // the order statistics: s[0] and (Tb >= 4) s[Tb - 1] are the row's min and max, known from the first launch
    const float s0 = ws[((size_t)b * F + f) * 2], smax = ws[((size_t)b * F + f) * 2 + 1];
    float s25 = 0.f, s75 = 0.f, s100 = 0.f;          // s[r25], s[r75], s[r100] where the rank exists
    if (Tb >= 5) {
        if (tid < 2) {
            sel_prefix[tid] = 0u;
            sel_rank[tid] = (unsigned)(tid == 0 ? Tb / 4 : 3 * (Tb / 4));
        }
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const unsigned mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
            for (int i = tid; i < 512; i += CM_THREADS) (&hist[0][0])[i] = 0u;
            __syncthreads();
            const unsigned pre0 = sel_prefix[0], pre1 = sel_prefix[1];
            for (int t = tid; t < Tb; t += CM_THREADS) {
                const unsigned k = cm_key(row[t]);
                const unsigned bin = (k >> shift) & 255u;
                if ((k & mask) == pre0) atomicAdd(&hist[0][bin], 1u);
                if ((k & mask) == pre1) atomicAdd(&hist[1][bin], 1u);
            }
            __syncthreads();
            if (tid == 0 || tid == 64) {              // one lane per rank, in different waves
                const int r = tid >> 6;
                unsigned want = sel_rank[r], cum = 0u;
                int d = 0;
                for (; d < 255; ++d) {
                    const unsigned h = hist[r][d];
                    if (cum + h > want) break;
                    cum += h;
                }
                sel_rank[r] = want - cum;
                sel_prefix[r] |= (unsigned)d << shift;
            }
            __syncthreads();
        }
        s25 = cm_unkey(sel_prefix[0]);
        s75 = cm_unkey(sel_prefix[1]);
        s100 = smax;
    } else if (tid == 0) {         // 1 .. 4 values: sorted in registers by one lane
        float s[4];
        for (int i = 0; i < Tb; ++i) {
            const float v = row[i];
            int j = i;
            for (; j > 0 && s[j - 1] > v; --j) s[j] = s[j - 1];
            s[j] = v;
        }
        if (Tb > 1) s25 = s[1];
        if (Tb > 2) s75 = s[2];
        if (Tb > 3) s100 = s[3];
    }
    if (tid == 0) {
        const bool many = Tb >= 5;
        const int p0 = min(cm_q(s0, vmin, vrange), 65532);
        const int p25 = (many || Tb > 1) ? min(max(cm_q(s25, vmin, vrange), p0 + 1), 65533) : p0 + 1;
        const int p75 = (many || Tb > 2) ? min(max(cm_q(s75, vmin, vrange), p25 + 1), 65534) : p25 + 1;
        const int p100 = (many || Tb > 3) ? max(cm_q(s100, vmin, vrange), p75 + 1) : p75 + 1;
        int* h = hdr + ((size_t)b * F + f) * 4;
        h[0] = p0;
        h[1] = p25;
        h[2] = p75;
        h[3] = p100;
        const float scale = cm_mul(vrange, CM_INV65535);
        Psh = make_float4(cm_u(vmin, scale, p0), cm_u(vmin, scale, p25), cm_u(vmin, scale, p75), cm_u(vmin, scale, p100));
    }
    __syncthreads();
    const float4 P = Psh;
    unsigned char* crow = codes + rb;
    // four codes per store from the first t whose place (rb + t) is a multiple of 4: with the bases aligned (vec) that is a 16-byte
    // aligned float4 of x and a 4-byte aligned word of codes
    const int head = vec ? min((int)((4 - (rb & 3)) & 3), Tb) : Tb;
    const int quads = (Tb - head) / 4;
    for (int t = tid; t < head; t += CM_THREADS) crow[t] = (unsigned char)cm_code(P, row[t]);
    for (int g = tid; g < quads; g += CM_THREADS) {
        const int t = head + 4 * g;
        const float4 v = *(const float4*)(row + t);
        *(unsigned*)(crow + t) = cm_code(P, v.x) | (cm_code(P, v.y) << 8) | (cm_code(P, v.z) << 16) | (cm_code(P, v.w) << 24);
    }
    for (int t = head + 4 * quads + tid; t < Tb; t += CM_THREADS) crow[t] = (unsigned char)cm_code(P, row[t]);
}

}  // namespace

// ---- exports (include/spkhip.h) ----
extern "C" int spk_cm_decode(const unsigned char* codes, const float* colhdr, const int* lengths, int B, int F, int T, float* out,
                             void* stream) {
    SPK_REQUIRE(codes && colhdr && out, "spk_cm_decode: null pointer");
    SPK_REQUIRE(B > 0 && F > 0 && T > 0 && (long long)B * F < (1ll << 31), "spk_cm_decode: B=%d F=%d T=%d", B, F, T);
    SPK_REQUIRE(((size_t)colhdr & 15) == 0 && ((size_t)out & 3) == 0, "spk_cm_decode: colhdr must be 16-byte and out 4-byte aligned");
    CmDecodeArgs a;
    a.codes = codes; a.colhdr = (const float4*)colhdr; a.lengths = lengths; a.out = out; a.F = F; a.T = T;
    a.nrow = (long long)B * F;
    a.N = a.nrow * T;
    const long long head = (long long)((16 - ((size_t)codes & 15)) & 15);
    a.head = head < a.N ? head : a.N;
    a.nchunk = 1 + (a.N - a.head + 15) / 16;
    const long long blocks = (a.nchunk + CM_THREADS - 1) / CM_THREADS;
    SPK_REQUIRE(blocks < (1ll << 31), "spk_cm_decode: %lld values exceed the grid", a.N);
    hipLaunchKernelGGL(cm_decode_kernel, dim3((unsigned)blocks), dim3(CM_THREADS), 0, (hipStream_t)stream, a);
    SPK_LAUNCH_CHECK("spk_cm_decode");
    return 0;
}

extern "C" int spk_cm_compress(const float* x, const int* T, int B, int F, int Tcap, float* ws, float* minrange, int* hdr,
                               unsigned char* codes, void* stream) {
    SPK_REQUIRE(x && T && ws && minrange && hdr && codes, "spk_cm_compress: null pointer");
    SPK_REQUIRE(B > 0 && B <= 65535 && F > 0 && Tcap > 0, "spk_cm_compress: B=%d (<= 65535) F=%d Tcap=%d", B, F, Tcap);
    const int vec = (((size_t)x & 15) == 0 && ((size_t)codes & 3) == 0) ? 1 : 0;
    const dim3 grid((unsigned)F, (unsigned)B);
    hipLaunchKernelGGL(cm_row_minmax, grid, dim3(CM_THREADS), 0, (hipStream_t)stream, x, T, F, Tcap, ws);
    SPK_LAUNCH_CHECK("spk_cm_compress");
    hipLaunchKernelGGL(cm_compress_rows, grid, dim3(CM_THREADS), 0, (hipStream_t)stream, x, T, F, Tcap, (const float*)ws, minrange,
                       hdr, codes, vec);
    SPK_LAUNCH_CHECK("spk_cm_compress");
    return 0;
}
