// PLDA back end on the device: the passes over [N][D] embedding tables and the trial loop of Kaldi's
// ivector-compute-lda, transform-vec, ivector-normalize-length, ivector-compute-plda and ivector-plda-scoring.
//   spk_scatter_f64       - C = sum_i w_i (x_i - mu)(x_i - mu)^T in fp64 on v_mfma_f64_16x16x4_f64: upper-triangle tiles, row slabs
//                           whose partial sums a second pass adds in slab order and mirrors (no atomics: two runs give the same bits)
//   spk_segment_sum_f64   - per-class fp64 row sums (or means) and counts: the class means of both trainers
//   spk_affine_lennorm    - Y = s_i (A x_i + b), s_i = 1 or sqrt(Do / sum_j y_j^2 q_j), on the same fp64 matrix tile
//   spk_plda_posterior_rows - the two row tables of one EM iteration in the basis where W = I and B = diag(psi)
//   spk_plda_llr          - the log-likelihood ratio of every trial (one wave per trial, fp64 sums in a fixed lane order)
// The D x D factorisations stay on the host.  Fragment map of the fp64 matrix instruction (it differs from every fp32 shape): lane l
// holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; register r of the result is D[i = (l >> 4) + 4 r][j = l & 15].
// Operands are read straight from global memory in that map (16 consecutive columns per lane group): there is no LDS staging and
// no barrier in the two matrix kernels, the instruction itself (64 cycles per issue) is the bound.
#pragma clang fp contract(off)
#include "spk_common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));
#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

#define PLDA_MAX_D 512
#define SC_TILE 64              // output tile of one block: 2 x 2 waves of 32 x 32 (2 x 2 instruction tiles each)
#define SC_MIN_SLAB 1024        // rows of a slab: at least this many, at most SC_MAX_SLABS slabs
#define SC_MAX_SLABS 128

static long long scatter_slab_rows(long long N) {
    long long r = (N + SC_MAX_SLABS - 1) / SC_MAX_SLABS;
    if (r < SC_MIN_SLAB) r = SC_MIN_SLAB;
    return (r + 3) & ~3ll;
}

extern "C" int spk_scatter_slab_rows(long long N) { return N > 0 && N < (1ll << 37) ? (int)scatter_slab_rows(N) : 0; }

extern "C" size_t spk_scatter_f64_workspace(long long N, int D) {
    if (N < 1 || D < 1 || D > PLDA_MAX_D) return 0;
    const long long R = scatter_slab_rows(N);
    return (size_t)((N + R - 1) / R) * D * D * sizeof(double);
}

// grid (upper-triangle tile pairs, slabs).  ws [slabs][D][D]: only elements (a, b) with a <= b are ever read back.
template <typename T>
__global__ __launch_bounds__(256) void scatter_kernel(const T* __restrict__ X, long long ld, const double* __restrict__ mu,
                                                      const double* __restrict__ w, double* __restrict__ ws, long long N, int D,
                                                      long long slab_rows, int ntile) {
    int p = blockIdx.x, ti = 0;
    while (p >= ntile - ti) {
        p -= ntile - ti;
        ++ti;
    }
    const int tj = ti + p;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    if (ti == tj && wm > wn) return;                          // lower triangle of a diagonal tile (wave-uniform)
    const int a0 = ti * SC_TILE + wm * 32, b0 = tj * SC_TILE + wn * 32;
    if (a0 >= D || b0 >= D) return;
    int ca[2], cb[2];
    double ma[2], mb[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        ca[m] = a0 + 16 * m + c;
        cb[m] = b0 + 16 * m + c;
        ma[m] = (mu && ca[m] < D) ? mu[ca[m]] : 0.0;
        mb[m] = (mu && cb[m] < D) ? mu[cb[m]] : 0.0;
    }
    f64x4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = (f64x4){0.0, 0.0, 0.0, 0.0};
    const long long lo = (long long)blockIdx.y * slab_rows;
    const long long hi = lo + slab_rows < N ? lo + slab_rows : N;
#pragma unroll 4
    for (long long i0 = lo; i0 < hi; i0 += 4) {
        const long long row = i0 + g;
        const bool vr = row < hi;
        const T* xr = X + (size_t)(vr ? row : lo) * ld;
        const double wi = (vr && w) ? w[row] : 1.0;
        double a[2], b[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            a[m] = (vr && ca[m] < D) ? ((double)xr[ca[m]] - ma[m]) * wi : 0.0;
            b[m] = (vr && cb[m] < D) ? (double)xr[cb[m]] - mb[m] : 0.0;
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[m][n] = MFMA_F64(a[m], b[n], acc[m][n]);
    }
    double* out = ws + (size_t)blockIdx.y * D * D;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ra = a0 + 16 * m + g + 4 * r, cc = b0 + 16 * n + c;
                if (ra < D && cc < D) out[(size_t)ra * D + cc] = acc[m][n][r];
            }
}

// C[a][b] = sum over slabs, in slab order, of the partial at (min(a, b), max(a, b)): symmetric bit for bit
__global__ __launch_bounds__(256) void scatter_reduce_kernel(const double* __restrict__ ws, double* __restrict__ C, int D, int slabs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= D * D) return;
    const int a = i / D, b = i - a * D;
    const int r = a < b ? a : b, c = a < b ? b : a;
    double s = 0.0;
    for (int k = 0; k < slabs; ++k) s += ws[(size_t)k * D * D + (size_t)r * D + c];
    C[i] = s;
}

extern "C" int spk_scatter_f64(const void* X, int x_f64, long long ld, const double* mu, const double* w, double* C, void* ws,
                               long long N, int D, void* stream) {
    SPK_REQUIRE(X && C && ws && N >= 1 && N < (1ll << 37), "spk_scatter_f64: bad arguments");
    SPK_REQUIRE(D >= 1 && D <= PLDA_MAX_D && ld >= D, "spk_scatter_f64: D=%d must lie in [1, %d] and ld=%lld >= D", D, PLDA_MAX_D, ld);
    const long long R = scatter_slab_rows(N);
    const int slabs = (int)((N + R - 1) / R), ntile = spk_ceil_div(D, SC_TILE);
    const dim3 grid(ntile * (ntile + 1) / 2, slabs);
    if (x_f64)
        hipLaunchKernelGGL(scatter_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, (const double*)X, ld, mu, w, (double*)ws,
                           N, D, R, ntile);
    else
        hipLaunchKernelGGL(scatter_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)X, ld, mu, w, (double*)ws, N,
                           D, R, ntile);
    SPK_LAUNCH_CHECK("spk_scatter_f64");
    hipLaunchKernelGGL(scatter_reduce_kernel, dim3(spk_ceil_div(D * D, 256)), dim3(256), 0, (hipStream_t)stream, (const double*)ws, C,
                       D, slabs);
    SPK_LAUNCH_CHECK("spk_scatter_f64 (reduce)");
    return 0;
}

// ---- class sums -------------------------------------------------------------------------------------------------------------
// One thread per (class, dimension), rows in list order; neighbouring threads read neighbouring dimensions of one row.
template <typename T>
__global__ __launch_bounds__(256) void segment_sum_kernel(const T* __restrict__ X, long long ld, const int* __restrict__ rows,
                                                          const int* __restrict__ seg_off, double* __restrict__ out,
                                                          int* __restrict__ count, int mean, int K, int D) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)K * D) return;
    const int k = (int)(i / D), d = (int)(i - (long long)k * D);
    const int lo = seg_off[k], hi = seg_off[k + 1];
    double acc = 0.0;
    for (int r = lo; r < hi; ++r) acc += (double)X[(size_t)(rows ? rows[r] : r) * ld + d];
    out[i] = (mean && hi > lo) ? acc / (double)(hi - lo) : acc;
    if (d == 0 && count) count[k] = hi - lo;
}

extern "C" int spk_segment_sum_f64(const void* X, int x_f64, long long ld, const int* rows, const int* seg_off, double* out,
                                   int* count, int mean, int K, int D, void* stream) {
    SPK_REQUIRE(X && seg_off && out && K >= 1 && D >= 1 && ld >= D, "spk_segment_sum_f64: bad arguments");
    const long long n = (long long)K * D;
    SPK_REQUIRE((n + 255) / 256 < (1ll << 31), "spk_segment_sum_f64: K * D = %lld is too large", n);
    const dim3 grid((unsigned)((n + 255) / 256));
    if (x_f64)
        hipLaunchKernelGGL(segment_sum_kernel<double>, grid, dim3(256), 0, (hipStream_t)stream, (const double*)X, ld, rows, seg_off,
                           out, count, mean, K, D);
    else
        hipLaunchKernelGGL(segment_sum_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)X, ld, rows, seg_off, out,
                           count, mean, K, D);
    SPK_LAUNCH_CHECK("spk_segment_sum_f64");
    return 0;
}

// ---- affine map + length normalisation --------------------------------------------------------------------------------------
// One block per 32 rows; its four waves share the output columns (instruction tile t of 16 columns belongs to wave t & 3), so a
// block owns whole rows and the row sums need one exchange through LDS.  The sum over k may run in any order, so step s of lane
// group g takes k = k0 + 4 g + s: every lane reads four consecutive values of its row of X and of A.  A == NULL: the identity.
// REC (spk_affine_lennorm_rec): block (x, r) takes rows 32 x .. of recording r, whose A, b and q lie at r Do Di
// and r Do, and whose Do in the scale is dim[r]; the arithmetic is the same.
template <typename TI, typename TO, int NT, bool REC = false>
__global__ __launch_bounds__(256) void affine_kernel(const TI* __restrict__ X, long long ldx, const double* __restrict__ A,
                                                     const double* __restrict__ b, const double* __restrict__ q, TO* __restrict__ Y,
                                                     long long N, int Di, int Do, int scale, const long long* __restrict__ rec_off = nullptr,
                                                     const int* __restrict__ dim = nullptr) {
    __shared__ double part[4][32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    long long row0 = (long long)blockIdx.x * 32;
    int Ds = Do;
    if (REC) {
        const int r = blockIdx.y;
        row0 += rec_off[r];
        N = rec_off[r + 1];
        if (row0 >= N) return;                                 // block-uniform
        A += (size_t)r * Do * Di;
        b += (size_t)r * Do;
        if (q) q += (size_t)r * Do;
        Ds = dim[r];
    }
    f64x4 acc[2][NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int j = 16 * (wave + 4 * n) + c;
        const double bj = (b && j < Do) ? b[j] : 0.0;
        acc[0][n] = (f64x4){bj, bj, bj, bj};
        acc[1][n] = acc[0][n];
    }
    if (A) {
        for (int k0 = 0; k0 < Di; k0 += 16) {
            double xa[2][4];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const long long row = row0 + 16 * m + c;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int k = k0 + 4 * g + s;
                    xa[m][s] = (row < N && k < Di) ? (double)X[(size_t)row * ldx + k] : 0.0;
                }
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int j0 = 16 * (wave + 4 * n);
                if (j0 < Do) {                                 // wave-uniform
                    const int j = j0 + c;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const int k = k0 + 4 * g + s;
                        const double bf = (j < Do && k < Di) ? A[(size_t)j * Di + k] : 0.0;
                        acc[0][n] = MFMA_F64(xa[0][s], bf, acc[0][n]);
                        acc[1][n] = MFMA_F64(xa[1][s], bf, acc[1][n]);
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long row = row0 + 16 * m + g + 4 * r;
                    const int j = 16 * (wave + 4 * n) + c;
                    if (row < N && j < Do) acc[m][n][r] += (double)X[(size_t)row * ldx + j];
                }
    }
    if (scale) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double s = 0.0;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int j = 16 * (wave + 4 * n) + c;
                    const double qj = j < Do ? (q ? q[j] : 1.0) : 0.0;
                    s += acc[m][n][r] * acc[m][n][r] * qj;
                }
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, 64);
                if (c == 0) part[wave][16 * m + g + 4 * r] = s;
            }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = 16 * m + g + 4 * r;
                const double tot = ((part[0][rr] + part[1][rr]) + part[2][rr]) + part[3][rr];
                const double f = tot > 0.0 ? sqrt((double)Ds / tot) : 1.0;
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[m][n][r] *= f;
            }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long row = row0 + 16 * m + g + 4 * r;
                const int j = 16 * (wave + 4 * n) + c;
                if (row < N && j < Do) Y[(size_t)row * Do + j] = (TO)acc[m][n][r];
            }
}

template <typename TI, typename TO>
static void affine_launch(const void* X, long long ldx, const double* A, const double* b, const double* q, void* Y, long long N,
                          int Di, int Do, int scale, hipStream_t st) {
    const dim3 grid((unsigned)((N + 31) / 32));
    const int need = spk_ceil_div(spk_ceil_div(Do, 16), 4);
#define AFF(NT) hipLaunchKernelGGL((affine_kernel<TI, TO, NT>), grid, dim3(256), 0, st, (const TI*)X, ldx, A, b, q, (TO*)Y, N, Di, Do, scale)
    if (need <= 1) AFF(1);
    else if (need <= 2) AFF(2);
    else if (need <= 4) AFF(4);
    else AFF(8);
#undef AFF
}

extern "C" int spk_affine_lennorm(const void* X, int x_f64, long long ldx, const double* A, const double* b, const double* q,
                                  int scale, void* Y, int y_f64, long long N, int Di, int Do, void* stream) {
    SPK_REQUIRE(X && Y && N >= 1 && N < (1ll << 36), "spk_affine_lennorm: bad arguments");
    SPK_REQUIRE(Di >= 1 && Di <= PLDA_MAX_D && Do >= 1 && Do <= PLDA_MAX_D && ldx >= Di,
                "spk_affine_lennorm: Di=%d and Do=%d must lie in [1, %d] and ldx=%lld >= Di", Di, Do, PLDA_MAX_D, ldx);
    SPK_REQUIRE(A || Di == Do, "spk_affine_lennorm: A = NULL is the identity and needs Di == Do (%d, %d)", Di, Do);
    hipStream_t st = (hipStream_t)stream;
    if (x_f64 && y_f64) affine_launch<double, double>(X, ldx, A, b, q, Y, N, Di, Do, scale, st);
    else if (x_f64) affine_launch<double, float>(X, ldx, A, b, q, Y, N, Di, Do, scale, st);
    else if (y_f64) affine_launch<float, double>(X, ldx, A, b, q, Y, N, Di, Do, scale, st);
    else affine_launch<float, float>(X, ldx, A, b, q, Y, N, Di, Do, scale, st);
    SPK_LAUNCH_CHECK("spk_affine_lennorm");
    return 0;
}

// The per-recording form: X [Ntot][L] float rows, A [R][L][L], b [R][L], q [R][L] or NULL, dim [R]; rows and entries of A and b at or
// beyond dim[r] are 0, so Y [Ntot][L] is 0 there.
extern "C" int spk_affine_lennorm_rec(const float* X, const long long* rec_off, const long long* tab_dev, const double* A,
                                      const double* b, const double* q, const int* dim, int scale, double* Y, long long Ntot, int L,
                                      int R, void* stream) {
    SPK_REQUIRE(L >= 1 && L <= 256, "spk_affine_lennorm_rec: L=%d must lie in [1, 256]", L);
    const int rc = spk_diar_check("spk_affine_lennorm_rec", rec_off, R, Ntot, nullptr);
    if (rc) return rc;
    SPK_REQUIRE(R <= 65535, "spk_affine_lennorm_rec: R=%d must stay below 65536", R);
    long long nmax = 0;
    for (int r = 0; r < R; ++r) nmax = rec_off[r + 1] - rec_off[r] > nmax ? rec_off[r + 1] - rec_off[r] : nmax;
    SPK_REQUIRE(X && tab_dev && A && b && dim && Y, "spk_affine_lennorm_rec: null device pointer");
    const dim3 grid((unsigned)((nmax + 31) / 32), (unsigned)R);
    const int need = spk_ceil_div(spk_ceil_div(L, 16), 4);
#define AFF(NT)                                                                                                                     \
    hipLaunchKernelGGL((affine_kernel<float, double, NT, true>), grid, dim3(256), 0, (hipStream_t)stream, X, (long long)L, A, b, q, Y, \
                       Ntot, L, L, scale, tab_dev, dim)
    if (need <= 1) AFF(1);
    else if (need <= 2) AFF(2);
    else AFF(4);
#undef AFF
    SPK_LAUNCH_CHECK("spk_affine_lennorm_rec");
    return 0;
}

// ---- one EM iteration's row tables --------------------------------------------------------------------------------------------
// In the basis where W = I and B = diag(psi) the posterior of class k (n utterances, centred mean m) has the diagonal covariance
// psi / (n psi + 1) and the mean w = n psi / (n psi + 1) * m: w_out = w, r_out = m - w.
__global__ __launch_bounds__(256) void posterior_rows_kernel(const double* __restrict__ mt, const int* __restrict__ count,
                                                             const double* __restrict__ psi, double* __restrict__ w_out,
                                                             double* __restrict__ r_out, int K, int D) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)K * D) return;
    const int k = (int)(i / D), j = (int)(i - (long long)k * D);
    const double np = (double)count[k] * psi[j];
    const double w = np / (np + 1.0) * mt[i];
    w_out[i] = w;
    r_out[i] = mt[i] - w;
}

extern "C" int spk_plda_posterior_rows(const double* mt, const int* count, const double* psi, double* w_out, double* r_out, int K,
                                       int D, void* stream) {
    SPK_REQUIRE(mt && count && psi && w_out && r_out && K >= 1 && D >= 1, "spk_plda_posterior_rows: bad arguments");
    const long long n = (long long)K * D;
    SPK_REQUIRE((n + 255) / 256 < (1ll << 31), "spk_plda_posterior_rows: K * D = %lld is too large", n);
    hipLaunchKernelGGL(posterior_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mt, count, psi,
                       w_out, r_out, K, D);
    SPK_LAUNCH_CHECK("spk_plda_posterior_rows");
    return 0;
}

// ---- trial scores -------------------------------------------------------------------------------------------------------------
// One wave per trial; lane l takes j = l, l + 64, ... and the 64 partial sums meet in a butterfly: a fixed order.  Per dimension the
// two quadratic terms are subtracted before they are summed, so psi_j = 0 (c = 0, v = 1) contributes exactly 0.
__global__ __launch_bounds__(256) void plda_llr_kernel(const double* __restrict__ en, const double* __restrict__ te,
                                                       const int* __restrict__ ia, const int* __restrict__ ib,
                                                       const double* __restrict__ psi, const int* __restrict__ count,
                                                       const int* __restrict__ tab_count, const double* __restrict__ tab_log, int U,
                                                       float* __restrict__ out, int T, int D) {
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    const double* e = en + (size_t)ia[t] * D;
    const double* x = te + (size_t)ib[t] * D;
    const int n = count ? count[ia[t]] : 1;
    const double dn = (double)n;
    double s = 0.0;
    for (int j = lane; j < D; j += 64) {
        const double p = psi[j], den = dn * p + 1.0;
        const double c = dn * p / den, v = 1.0 + p / den;
        const double d = x[j] - c * e[j];
        s += 0.5 * (x[j] * x[j] / (p + 1.0) - d * d / v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
        double lg = __builtin_nan("");
        for (int u = 0; u < U; ++u)
            if (tab_count[u] == n) {
                lg = 0.5 * (tab_log[2 * u + 1] - tab_log[2 * u]);
                break;
            }
        out[t] = (float)(s + lg);
    }
}

extern "C" int spk_plda_llr(const double* en, const double* te, const int* ia, const int* ib, const double* psi, const int* count,
                            const int* tab_count, const double* tab_log, int U, float* out, int T, int D, int n_en, int n_te,
                            void* stream) {
    SPK_REQUIRE(en && te && ia && ib && psi && tab_count && tab_log && out && T >= 1 && D >= 1 && U >= 1 && n_en >= 1 && n_te >= 1,
                "spk_plda_llr: bad arguments");
    (void)n_en; (void)n_te;   // index ranges are validated by the caller that built the index arrays (host side)
    hipLaunchKernelGGL(plda_llr_kernel, dim3((unsigned)(((long long)T + 3) / 4)), dim3(256), 0, (hipStream_t)stream, en, te, ia, ib,
                       psi, count, tab_count, tab_log, U, out, T, D);
    SPK_LAUNCH_CHECK("spk_plda_llr");
    return 0;
}
