// Per-recording PCA of ivector-plda-scoring-dense (--target-energy) on the device.
//   spk_syevj_batch    - batched symmetric eigensolver: one workgroup per matrix runs a parallel-ordered cyclic two-sided Jacobi
//                        iteration to convergence with __syncthreads() alone; nothing waits on another workgroup
//   spk_pca_plda_batch - steps 1-5 of section 6p for every recording of a batch: covariance and every matrix product on
//                        v_mfma_f64_16x16x4_f64 tiled over (recording, tile); the two eigendecompositions, the Cholesky factorisation
//                        and the triangular inverse one workgroup per recording (the device code of spk_syevj_batch)
// The per-recording forms of the row kernels (spk_affine_lennorm_rec, spk_score_dense_q_rec, spk_score_dense_rec) live beside the
// kernels whose bodies they share (csrc/plda.hip, csrc/diar.hip).
// All arithmetic is fp64, every sum runs in a fixed order, there are no floating-point atomics: the same bits on every run, wherever
// a recording sits in its batch.  Fragment map of the fp64 matrix instruction: see csrc/plda.hip.
#pragma clang fp contract(off)
#include "spk_common.h"

#include <vector>

typedef double f64x4 __attribute__((ext_vector_type(4)));
#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

#define EIG_THREADS 256
#define EIG_WAVES (EIG_THREADS / 64)
#define EIG_MAX_DIM 256
#define EIG_MAX_SWEEPS 30
#define EIG_LDS_DOUBLES (140 * 140)   // LDS of one workgroup, 153 KB of the CU's 160: padded orders up to 98 keep the matrix and the
                                     // eigenvector table there, orders up to 140 the matrix alone (the table in the workspace)
#define EIG_EPS 0x1p-53

// ---- the Jacobi iteration ----------------------------------------------------------------------------------------------------------
// A [me][me] symmetric and VT [me][me], me even (an odd order is padded with a zero row and column, whose pairs never rotate); each in
// LDS or in global memory (eig_place) - the arithmetic is the same.  A round holds me / 2 disjoint pairs (p, q) in round-robin order: index
// me - 1 stays, the others move round a ring, so me - 1 rounds - a sweep - meet every pair once.  A round computes the rotation of
// every pair from (a_pp, a_qq, a_pq), then, after one barrier, applies A <- J^T A J block by block: the 2 x 2 block (pair k, pair l),
// k <= l, takes the row rotation of k and the column rotation of l and is stored twice, so A stays symmetric bit for bit; the block
// (k, k) is set to diag(a_pp - t a_pq, a_qq + t a_pq).  VT rows p and q take the same rotation (VT row i = eigenvector i at the end).
// A pair is left alone when |a_pq| <= 2^-53 sqrt(|a_pp| |a_qq|) or |a_pq| <= 2^-53 max_i |a_ii| / me (the maximum taken at the
// sweep's start); a sweep in which no pair rotated ends the iteration.  A NaN fails both tests, so it rotates until the sweep bound.
struct EigShared {
    double c[EIG_MAX_DIM / 2], s[EIG_MAX_DIM / 2], t[EIG_MAX_DIM / 2];
    short p[EIG_MAX_DIM / 2], q[EIG_MAX_DIM / 2], rot[EIG_MAX_DIM / 2];
    double red[EIG_WAVES];
    int perm[EIG_MAX_DIM];
};

static __device__ __forceinline__ double eig_nanmax(double m, double v) { return (v > m || v != v) ? v : m; }   // a NaN sticks

// -> sweeps run (the clean last one included); *info = 0 converged, 1 the sweep bound was reached.  Block-uniform.
static __device__ int eig_jacobi(double* A, double* VT, int me, EigShared& sh, int* info) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = me >> 1, n1 = me - 1;
    for (int idx = tid; idx < me * me; idx += EIG_THREADS) VT[idx] = (idx / me == idx % me) ? 1.0 : 0.0;
    __syncthreads();
    int sweep = 0;
    *info = 1;
    while (sweep < EIG_MAX_SWEEPS) {
        double dm = 0.0;
        for (int i = tid; i < me; i += EIG_THREADS) dm = eig_nanmax(dm, fabs(A[(size_t)i * me + i]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dm = eig_nanmax(dm, __shfl_xor(dm, off, 64));
        if (lane == 0) sh.red[wave] = dm;
        __syncthreads();
        dm = eig_nanmax(eig_nanmax(eig_nanmax(sh.red[0], sh.red[1]), sh.red[2]), sh.red[3]);
        const double thr = dm * (EIG_EPS / (double)me);
        int rotated = 0;
        for (int r = 0; r < n1; ++r) {
            if (tid < h) {
                int a, b;
                if (tid == 0) {
                    a = n1;
                    b = r;
                } else {
                    a = (r + tid) % n1;
                    b = (r + n1 - tid) % n1;
                }
                const int p = a < b ? a : b, q = a < b ? b : a;
                const double app = A[(size_t)p * me + p], aqq = A[(size_t)q * me + q], apq = A[(size_t)p * me + q];
                const double mag = fabs(apq);
                const bool skip = apq == 0.0 || mag <= EIG_EPS * (sqrt(fabs(app)) * sqrt(fabs(aqq))) || mag <= thr;
                double c = 1.0, s = 0.0, t = 0.0;
                if (!skip) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta != theta) t = theta;
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                    rotated = 1;
                }
                sh.c[tid] = c;
                sh.s[tid] = s;
                sh.t[tid] = t;
                sh.p[tid] = (short)p;
                sh.q[tid] = (short)q;
                sh.rot[tid] = skip ? 0 : 1;
            }
            __syncthreads();
            // the blocks (k, l), k <= l: rows k and h - 1 - k of the triangle together hold h + 1 of them
            const int items = ((h + 1) >> 1) * (h + 1);
            for (int it = tid; it < items; it += EIG_THREADS) {
                const int kk = it / (h + 1), j = it - kk * (h + 1);
                int k, l;
                if (j < h - kk) {
                    k = kk;
                    l = kk + j;
                } else {
                    k = h - 1 - kk;
                    l = k + (j - (h - kk));
                    if (k == kk) continue;
                }
                const int rk = sh.rot[k], rl = sh.rot[l];
                if (!(rk | rl)) continue;
                const int p1 = sh.p[k], q1 = sh.q[k];
                if (k == l) {
                    const double apq = A[(size_t)p1 * me + q1], t = sh.t[k];
                    A[(size_t)p1 * me + p1] = A[(size_t)p1 * me + p1] - t * apq;
                    A[(size_t)q1 * me + q1] = A[(size_t)q1 * me + q1] + t * apq;
                    A[(size_t)p1 * me + q1] = 0.0;
                    A[(size_t)q1 * me + p1] = 0.0;
                    continue;
                }
                const int p2 = sh.p[l], q2 = sh.q[l];
                const double c1 = sh.c[k], s1 = sh.s[k], c2 = sh.c[l], s2 = sh.s[l];
                const double b00 = A[(size_t)p1 * me + p2], b01 = A[(size_t)p1 * me + q2];
                const double b10 = A[(size_t)q1 * me + p2], b11 = A[(size_t)q1 * me + q2];
                const double r00 = c1 * b00 - s1 * b10, r01 = c1 * b01 - s1 * b11;
                const double r10 = s1 * b00 + c1 * b10, r11 = s1 * b01 + c1 * b11;
                const double o00 = c2 * r00 - s2 * r01, o01 = s2 * r00 + c2 * r01;
                const double o10 = c2 * r10 - s2 * r11, o11 = s2 * r10 + c2 * r11;
                A[(size_t)p1 * me + p2] = o00;
                A[(size_t)p2 * me + p1] = o00;
                A[(size_t)p1 * me + q2] = o01;
                A[(size_t)q2 * me + p1] = o01;
                A[(size_t)q1 * me + p2] = o10;
                A[(size_t)p2 * me + q1] = o10;
                A[(size_t)q1 * me + q2] = o11;
                A[(size_t)q2 * me + q1] = o11;
            }
            for (int it = tid; it < h * me; it += EIG_THREADS) {
                const int l = it / me, i = it - l * me;
                if (!sh.rot[l]) continue;
                const double c = sh.c[l], s = sh.s[l];
                double* vp = VT + (size_t)sh.p[l] * me + i;
                double* vq = VT + (size_t)sh.q[l] * me + i;
                const double a = *vp, b = *vq;
                *vp = c * a - s * b;
                *vq = s * a + c * b;
            }
            __syncthreads();
        }
        ++sweep;
        if (!__syncthreads_or(rotated)) {
            *info = 0;
            break;
        }
    }
    return sweep;
}

// where the two tables of padded order me lie: both in LDS, the matrix alone, or both in the workspace at `ws` (2 me^2 doubles)
static __device__ __forceinline__ void eig_place(double* lds, double* ws, int me, double*& A, double*& VT) {
    const int mm = me * me;
    A = mm <= EIG_LDS_DOUBLES ? lds : ws;
    VT = 2 * mm <= EIG_LDS_DOUBLES ? lds + mm : ws + mm;
}

// the symmetric matrix of order m at `in` (row pitch ld; the upper triangle is read and mirrored) -> A [me][me], zero padded
static __device__ void eig_load(const double* __restrict__ in, int ld, int m, double* A, int me) {
    for (int idx = threadIdx.x; idx < me * me; idx += EIG_THREADS) {
        const int i = idx / me, j = idx - i * me;
        const int a = i < j ? i : j, b = i < j ? j : i;
        A[idx] = b < m ? in[(size_t)a * ld + b] : 0.0;
    }
    __syncthreads();
}

// eigenvalues descending (ties by index, a NaN last; with `floor0` values below 0 become 0) -> w [ldw] (0 at and beyond m), the
// eigenvectors as rows in the same order -> vec [ldw][ldv] (0 outside m x m)
static __device__ void eig_store(const double* A, const double* VT, int m, int me, EigShared& sh, bool floor0, double* __restrict__ w,
                                 double* __restrict__ vec, int ldw, int ldv) {
    const int tid = threadIdx.x;
    for (int i = tid; i < m; i += EIG_THREADS) {
        const double wi = A[(size_t)i * me + i];
        int rank = 0;
        for (int j = 0; j < m; ++j) {
            const double wj = A[(size_t)j * me + j];
            const bool before = wj > wi || (wi != wi && wj == wj) || ((wj == wi || (wi != wi && wj != wj)) && j < i);
            rank += before ? 1 : 0;
        }
        sh.perm[rank] = i;
    }
    __syncthreads();
    for (int k = tid; k < ldw; k += EIG_THREADS) {
        double v = 0.0;
        if (k < m) {
            v = A[(size_t)sh.perm[k] * me + sh.perm[k]];
            if (floor0 && v < 0.0) v = 0.0;
        }
        w[k] = v;
    }
    for (int idx = tid; idx < ldw * ldv; idx += EIG_THREADS) {
        const int k = idx / ldv, j = idx - k * ldv;
        vec[idx] = (k < m && j < m) ? VT[(size_t)sh.perm[k] * me + j] : 0.0;
    }
    __syncthreads();
}

__global__ __launch_bounds__(EIG_THREADS) void syevj_kernel(const double* __restrict__ in, int ld, const int* __restrict__ orders,
                                                            double* __restrict__ ws, double* __restrict__ w, double* __restrict__ vec,
                                                            int* __restrict__ sweeps, int* __restrict__ info) {
    __shared__ double lds[EIG_LDS_DOUBLES];
    __shared__ EigShared sh;
    const int r = blockIdx.x, m = orders[r], me = m + (m & 1), ldp = ld + (ld & 1);
    double *A, *VT;
    eig_place(lds, ws + (size_t)r * 2 * ldp * ldp, me, A, VT);
    eig_load(in + (size_t)r * ld * ld, ld, m, A, me);
    int inf;
    const int sw = eig_jacobi(A, VT, me, sh, &inf);
    eig_store(A, VT, m, me, sh, false, w + (size_t)r * ld, vec + (size_t)r * ld * ld, ld, ld);
    if (threadIdx.x == 0) {
        sweeps[r] = sw;
        info[r] = inf;
    }
}

extern "C" int spk_syevj_max_dim(void) { return EIG_MAX_DIM; }
extern "C" int spk_syevj_max_sweeps(void) { return EIG_MAX_SWEEPS; }
extern "C" int spk_syevj_threads(void) { return EIG_THREADS; }

extern "C" long long spk_syevj_ws_elems(int R, int ld) {
    SPK_REQUIRE(R >= 1 && R < (1 << 20), "spk_syevj_ws_elems: R=%d must lie in [1, 2^20)", R);
    SPK_REQUIRE(ld >= 1 && ld <= EIG_MAX_DIM, "spk_syevj_ws_elems: ld=%d must lie in [1, %d]", ld, EIG_MAX_DIM);
    const long long ldp = ld + (ld & 1);
    return (long long)R * 2 * ldp * ldp;
}

extern "C" int spk_syevj_batch(const double* A, const int* orders, const int* orders_dev, double* ws, long long ws_elems, double* w,
                               double* vec, int* sweeps, int* info, int R, int ld, void* stream) {
    SPK_REQUIRE(R >= 1 && R < (1 << 20), "spk_syevj_batch: R=%d must lie in [1, 2^20)", R);
    SPK_REQUIRE(ld >= 1 && ld <= EIG_MAX_DIM, "spk_syevj_batch: ld=%d must lie in [1, %d]", ld, EIG_MAX_DIM);
    SPK_REQUIRE(orders, "spk_syevj_batch: orders is missing");
    for (int r = 0; r < R; ++r)
        SPK_REQUIRE(orders[r] >= 1 && orders[r] <= ld, "spk_syevj_batch: orders[%d]=%d must lie in [1, ld=%d]", r, orders[r], ld);
    const long long ldp = ld + (ld & 1), need = (long long)R * 2 * ldp * ldp;
    SPK_REQUIRE(ws_elems >= need, "spk_syevj_batch: the workspace holds %lld doubles, the batch needs %lld", ws_elems, need);
    SPK_REQUIRE(A && orders_dev && ws && w && vec && sweeps && info, "spk_syevj_batch: null device pointer");
    hipLaunchKernelGGL(syevj_kernel, dim3((unsigned)R), dim3(EIG_THREADS), 0, (hipStream_t)stream, A, ld, orders_dev, ws, w, vec, sweeps,
                       info);
    SPK_LAUNCH_CHECK("spk_syevj_batch");
    return 0;
}

// ---- the PCA of one batch -----------------------------------------------------------------------------------------------------------
// Workspace of recording r, PCA_BUFS buffers of Lp^2 doubles (Lp = L rounded up to even) and mu [L], from ws + r * per:
//   0 C, later M = T1 B_r T1^T   1, 2 the Jacobi iteration's A and VT (where they do not fit in LDS)   3 P (eigenvectors of C as rows)   4 X (products in
//   flight)   5 W_r, then its Cholesky factor G   6 B_r   7 T1 = G^-1   8 U (eigenvectors of M as rows)
// After the R blocks: skip [R] ints.  Matrices in the workspace have row pitch L.
#define PCA_BUFS 9

static long long pca_per(int L) {
    const long long Lp = L + (L & 1);
    return PCA_BUFS * Lp * Lp + L;
}

// mu[r][d] = (1 / n) sum_i z_id, the rows in order
__global__ __launch_bounds__(256) void pca_mean_kernel(const float* __restrict__ Z, const long long* __restrict__ rec_off,
                                                       double* __restrict__ ws, long long per, long long mu_at, int L, int R) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)R * L) return;
    const int r = (int)(idx / L), d = (int)(idx - (long long)r * L);
    const long long lo = rec_off[r], hi = rec_off[r + 1];
    double s = 0.0;
    for (long long i = lo; i < hi; ++i) s += (double)Z[(size_t)i * L + d];
    ws[(size_t)r * per + mu_at + d] = s / (double)(hi - lo);
}

// C = (1 / n) sum_i z_i z_i^T - mu mu^T: one wave per 16 x 16 tile (ti <= tj) of one recording, four rows per instruction, in order
__global__ __launch_bounds__(256) void pca_cov_kernel(const float* __restrict__ Z, const long long* __restrict__ rec_off,
                                                      double* __restrict__ ws, long long per, long long mu_at, int L, int T) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), r = blockIdx.y;
    if (tile >= T * T) return;                                    // wave-uniform
    const int ti = tile / T, tj = tile - ti * T;
    if (ti > tj) return;
    const long long lo = rec_off[r], hi = rec_off[r + 1];
    const int ca = ti * 16 + c, cb = tj * 16 + c;
    f64x4 acc = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (long long i0 = lo; i0 < hi; i0 += 4) {
        const long long row = i0 + g;
        const bool vr = row < hi;
        const double a = (vr && ca < L) ? (double)Z[(size_t)row * L + ca] : 0.0;
        const double b = (vr && cb < L) ? (double)Z[(size_t)row * L + cb] : 0.0;
        acc = MFMA_F64(a, b, acc);
    }
    double* C = ws + (size_t)r * per;
    const double* mu = C + mu_at;
    const double n = (double)(hi - lo);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int i = ti * 16 + g + 4 * rr, j = tj * 16 + c;
        if (i < L && j < L) C[(size_t)i * L + j] = acc[rr] / n - mu[i] * mu[j];
    }
}

// out_r [M][N] = A_r [M][K] op(B_r), op(B) = B [K][N] or, with tb, the transpose of B [N][K]; M, N, K are dim[r] where their selector
// is 1 and L where it is 0.  One wave per 16 x 16 tile, k in order.  A recording that is skipped or in error is left alone.
__global__ __launch_bounds__(256) void pca_gemm_kernel(const double* __restrict__ A, long long sa, const double* __restrict__ B,
                                                       long long sb, int tb, double* __restrict__ O, long long so,
                                                       const int* __restrict__ dim, const int* __restrict__ skip,
                                                       const int* __restrict__ info, int selM, int selN, int selK, int L, int T) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), r = blockIdx.y;
    if (tile >= T * T || skip[r] || info[r]) return;              // wave-uniform
    const int d = dim[r], M = selM ? d : L, N = selN ? d : L, K = selK ? d : L;
    const int ti = tile / T, tj = tile - ti * T;
    if (ti * 16 >= M || tj * 16 >= N) return;
    const double* Ar = A + (size_t)r * sa;
    const double* Br = B + (size_t)r * sb;
    const int ia = ti * 16 + c, jb = tj * 16 + c;
    f64x4 acc = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + g;
        const bool vk = k < K;
        const double a = (vk && ia < M) ? Ar[(size_t)ia * L + k] : 0.0;
        const double b = (vk && jb < N) ? (tb ? Br[(size_t)jb * L + k] : Br[(size_t)k * L + jb]) : 0.0;
        acc = MFMA_F64(a, b, acc);
    }
    double* Or = O + (size_t)r * so;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int i = ti * 16 + g + 4 * rr, j = tj * 16 + c;
        if (i < M && j < N) Or[(size_t)i * L + j] = acc[rr];
    }
}

// steps 2 and 3: C = P diag(s) P^T, the retained dimension, the skips
__global__ __launch_bounds__(EIG_THREADS) void pca_eig1_kernel(const long long* __restrict__ rec_off, double* __restrict__ ws,
                                                               long long per, double E, int* __restrict__ dim, double* __restrict__ s,
                                                               int* __restrict__ skip, int* __restrict__ info, int L) {
    __shared__ double lds[EIG_LDS_DOUBLES];
    __shared__ EigShared sh;
    const int r = blockIdx.x, me = L + (L & 1);
    const long long n = rec_off[r + 1] - rec_off[r];
    double* base = ws + (size_t)r * per;
    double *A, *VT;
    eig_place(lds, base + (size_t)me * me, me, A, VT);
    eig_load(base, L, L, A, me);
    int inf;
    eig_jacobi(A, VT, me, sh, &inf);
    double* sr = s + (size_t)r * L;
    eig_store(A, VT, L, me, sh, true, sr, base + 3 * (size_t)me * me, L, L);
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int k = 0; k < L; ++k) tot += sr[k];
        int d = L, sk = 1;
        if (inf == 0 && n > 1 && tot > 0.0) {
            double cum = 0.0;
            int k = 0;
            while (k < L) {
                cum += sr[k];
                ++k;
                if (cum / tot > E) break;
            }
            d = k + 1;
            d = d > L ? L : d;
            d = d > n - 1 ? (int)(n - 1) : d;
            sk = 0;
        }
        dim[r] = d;
        skip[r] = sk;
        info[r] = inf;
    }
}

// step 5, first half: W_r = G G^T in place (lower triangle, left-looking: column j after the columns before it, every sum in the
// order of k), then T1 = G^-1 by forward substitution, one column per thread.  A pivot that is not positive: info = 2.
__global__ __launch_bounds__(EIG_THREADS) void pca_chol_kernel(double* __restrict__ ws, long long per, const int* __restrict__ dim,
                                                               const int* __restrict__ skip, int* __restrict__ info, int L) {
    __shared__ double col[EIG_MAX_DIM];
    const int r = blockIdx.x, tid = threadIdx.x, me = L + (L & 1);
    if (skip[r] || info[r]) return;                               // block-uniform
    const int m = dim[r];
    double* G = ws + (size_t)r * per + 5 * (size_t)me * me;
    double* T1 = ws + (size_t)r * per + 7 * (size_t)me * me;
    for (int j = 0; j < m; ++j) {
        for (int i = j + tid; i < m; i += EIG_THREADS) {
            double v = G[(size_t)i * L + j];
            for (int k = 0; k < j; ++k) v -= G[(size_t)i * L + k] * G[(size_t)j * L + k];
            col[i] = v;
        }
        __syncthreads();
        const double piv = col[j];
        if (!(piv > 0.0)) {                                       // block-uniform (a NaN lands here too)
            if (tid == 0) info[r] = 2;
            return;
        }
        const double d = sqrt(piv);
        for (int i = j + tid; i < m; i += EIG_THREADS) G[(size_t)i * L + j] = i == j ? d : col[i] / d;
        __syncthreads();
    }
    for (int j = tid; j < m; j += EIG_THREADS) {
        for (int i = 0; i < j; ++i) T1[(size_t)i * L + j] = 0.0;
        for (int i = j; i < m; ++i) {
            double v = i == j ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) v -= G[(size_t)i * L + k] * T1[(size_t)k * L + j];
            T1[(size_t)i * L + j] = v / G[(size_t)i * L + i];
        }
    }
}

// step 5, second half: M = U diag(psi_r) U^T
__global__ __launch_bounds__(EIG_THREADS) void pca_eig2_kernel(double* __restrict__ ws, long long per, const int* __restrict__ dim,
                                                               const int* __restrict__ skip, int* __restrict__ info,
                                                               double* __restrict__ psi_r, int L) {
    __shared__ double lds[EIG_LDS_DOUBLES];
    __shared__ EigShared sh;
    const int r = blockIdx.x, mL = L + (L & 1);
    if (skip[r] || info[r]) return;                               // block-uniform
    const int m = dim[r], me = m + (m & 1);
    double* base = ws + (size_t)r * per;
    double *A, *VT;
    eig_place(lds, base + (size_t)mL * mL, me, A, VT);
    eig_load(base, L, m, A, me);
    int inf;
    eig_jacobi(A, VT, me, sh, &inf);
    eig_store(A, VT, m, me, sh, true, psi_r + (size_t)r * L, base + 8 * (size_t)mL * mL, L, L);
    if (threadIdx.x == 0 && inf) info[r] = inf;
}

// what is left: b_r = -A_r m (k in order), zeros at and beyond dim; a skipped recording gets the global model, one in error zeros
__global__ __launch_bounds__(256) void pca_final_kernel(const double* __restrict__ Tg, const double* __restrict__ psig,
                                                        const double* __restrict__ mean, const int* __restrict__ dim,
                                                        const int* __restrict__ skip, const int* __restrict__ info,
                                                        double* __restrict__ psi_r, double* __restrict__ A_r, double* __restrict__ b_r,
                                                        int L) {
    const int r = blockIdx.x, tid = threadIdx.x;
    double* Ar = A_r + (size_t)r * L * L;
    const bool sk = skip[r] && !info[r];
    const int d = info[r] ? 0 : dim[r];
    if (sk) {
        for (int idx = tid; idx < L * L; idx += 256) Ar[idx] = Tg[idx];
        for (int k = tid; k < L; k += 256) psi_r[(size_t)r * L + k] = psig[k];
    } else {
        for (int idx = d * L + tid; idx < L * L; idx += 256) Ar[idx] = 0.0;
        if (info[r])
            for (int k = tid; k < L; k += 256) psi_r[(size_t)r * L + k] = 0.0;
    }
    __syncthreads();
    for (int i = tid; i < L; i += 256) {
        double v = 0.0;
        if (i < d)
            for (int k = 0; k < L; ++k) v += Ar[(size_t)i * L + k] * mean[k];
        b_r[(size_t)r * L + i] = i < d ? -v : 0.0;
    }
}

// step 7's terms of every recording from its psi_r (diarize.plda_dense_terms) and the weights of step 6: one wave per recording; lane l
// adds the summands of K at d = l, l + 64, ... in order and the 64 partial sums meet in a butterfly
__global__ __launch_bounds__(64) void pca_terms_kernel(const double* __restrict__ psi_r, double* __restrict__ g, double* __restrict__ k,
                                                       double* __restrict__ qn, double* __restrict__ K, int L) {
    const int r = blockIdx.x, lane = threadIdx.x;
    double s = 0.0;
    for (int d = lane; d < L; d += 64) {
        const size_t i = (size_t)r * L + d;
        const double p = psi_r[i];
        g[i] = p / (2.0 * p + 1.0);
        k[i] = p * p / ((p + 1.0) * (2.0 * p + 1.0));
        qn[i] = 1.0 / (p + 1.0);
        s += log(p + 1.0) - log(1.0 + p / (p + 1.0));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) K[r] = 0.5 * s;
}

extern "C" int spk_pca_score_terms(const double* psi_r, double* g, double* k, double* qn, double* K, int R, int L, void* stream) {
    SPK_REQUIRE(R >= 1 && R < (1 << 20), "spk_pca_score_terms: R=%d must lie in [1, 2^20)", R);
    SPK_REQUIRE(L >= 1 && L <= 512, "spk_pca_score_terms: L=%d must lie in [1, 512]", L);
    SPK_REQUIRE(psi_r && g && k && qn && K, "spk_pca_score_terms: null device pointer");
    hipLaunchKernelGGL(pca_terms_kernel, dim3((unsigned)R), dim3(64), 0, (hipStream_t)stream, psi_r, g, k, qn, K, L);
    SPK_LAUNCH_CHECK("spk_pca_score_terms");
    return 0;
}

static int pca_shape(const char* who, const long long* rec_off, int R, long long Ntot, int L) {
    const int rc = spk_diar_check(who, rec_off, R, Ntot, nullptr);
    if (rc) return rc;
    SPK_REQUIRE(R <= 65535, "%s: R=%d must stay below 65536", who, R);
    SPK_REQUIRE(L >= 1 && L <= EIG_MAX_DIM, "%s: L=%d must lie in [1, %d]", who, L, EIG_MAX_DIM);
    return 0;
}

extern "C" long long spk_pca_plda_ws_elems(const long long* rec_off, int R, int L) {
    SPK_REQUIRE(rec_off && R >= 1, "spk_pca_plda_ws_elems: bad arguments (R=%d)", R);
    const int rc = pca_shape("spk_pca_plda_ws_elems", rec_off, R, rec_off[R], L);
    if (rc) return rc;
    return (long long)R * pca_per(L) + (R + 1) / 2;
}

extern "C" int spk_pca_plda_batch(const float* Z, const long long* rec_off, const long long* tab_dev, const double* W, const double* B,
                                  const double* T, const double* psi, const double* mean, double E, double* ws, long long ws_elems,
                                  int* dim, double* s, double* psi_r, double* A_r, double* b_r, int* info, long long Ntot, int L, int R,
                                  void* stream) {
    const int rc = pca_shape("spk_pca_plda_batch", rec_off, R, Ntot, L);
    if (rc) return rc;
    SPK_REQUIRE(E > 0.0 && E < 1.0, "spk_pca_plda_batch: E=%g must lie strictly between 0 and 1", E);
    const long long per = pca_per(L), need = (long long)R * per + (R + 1) / 2;
    SPK_REQUIRE(ws_elems >= need, "spk_pca_plda_batch: the workspace holds %lld doubles, the batch needs %lld", ws_elems, need);
    SPK_REQUIRE(Z && tab_dev && W && B && T && psi && mean && ws && dim && s && psi_r && A_r && b_r && info,
                "spk_pca_plda_batch: null device pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long LL = (long long)(L + (L & 1)) * (L + (L & 1)), mu_at = PCA_BUFS * LL;
    const int Tn = spk_ceil_div(L, 16);
    const dim3 tiles((unsigned)spk_ceil_div(Tn * Tn, 4), (unsigned)R);
    int* skip = (int*)(ws + (size_t)R * per);
    double *bC = ws, *bP = ws + 3 * LL, *bX = ws + 4 * LL, *bW = ws + 5 * LL, *bB = ws + 6 * LL, *bT1 = ws + 7 * LL, *bU = ws + 8 * LL;
    hipLaunchKernelGGL(pca_mean_kernel, dim3((unsigned)(((long long)R * L + 255) / 256)), dim3(256), 0, st, Z, tab_dev, ws, per, mu_at, L,
                       R);
    SPK_LAUNCH_CHECK("spk_pca_plda_batch (mean)");
    hipLaunchKernelGGL(pca_cov_kernel, tiles, dim3(256), 0, st, Z, tab_dev, ws, per, mu_at, L, Tn);
    SPK_LAUNCH_CHECK("spk_pca_plda_batch (covariance)");
    hipLaunchKernelGGL(pca_eig1_kernel, dim3((unsigned)R), dim3(EIG_THREADS), 0, st, tab_dev, ws, per, E, dim, s, skip, info, L);
    SPK_LAUNCH_CHECK("spk_pca_plda_batch (first eigendecomposition)");
#define PCA_GEMM(Ap, Bp, sbv, tbv, Op, sov, sm, sn, sk)                                                                             \
    do {                                                                                                                            \
        hipLaunchKernelGGL(pca_gemm_kernel, tiles, dim3(256), 0, st, (const double*)(Ap), per, (const double*)(Bp), (long long)(sbv), \
                           tbv, Op, (long long)(sov), (const int*)dim, (const int*)skip, (const int*)info, sm, sn, sk, L, Tn);      \
        SPK_LAUNCH_CHECK("spk_pca_plda_batch (product)");                                                                           \
    } while (0)
    PCA_GEMM(bP, W, 0, 0, bX, per, 1, 0, 0);                      // X = P_r W
    PCA_GEMM(bX, bP, per, 1, bW, per, 1, 1, 0);                   // W_r = X P_r^T
    PCA_GEMM(bP, B, 0, 0, bX, per, 1, 0, 0);                      // X = P_r B
    PCA_GEMM(bX, bP, per, 1, bB, per, 1, 1, 0);                   // B_r = X P_r^T
    hipLaunchKernelGGL(pca_chol_kernel, dim3((unsigned)R), dim3(EIG_THREADS), 0, st, ws, per, (const int*)dim, (const int*)skip, info, L);
    SPK_LAUNCH_CHECK("spk_pca_plda_batch (Cholesky)");
    PCA_GEMM(bT1, bB, per, 0, bX, per, 1, 1, 1);                  // X = T1 B_r
    PCA_GEMM(bX, bT1, per, 1, bC, per, 1, 1, 1);                  // M = X T1^T
    hipLaunchKernelGGL(pca_eig2_kernel, dim3((unsigned)R), dim3(EIG_THREADS), 0, st, ws, per, (const int*)dim, (const int*)skip, info,
                       psi_r, L);
    SPK_LAUNCH_CHECK("spk_pca_plda_batch (second eigendecomposition)");
    PCA_GEMM(bT1, bP, per, 0, bX, per, 1, 0, 1);                  // X = T1 P_r
    PCA_GEMM(bU, bX, per, 0, A_r, (long long)L * L, 1, 0, 1);     // A_r = U^T X (U's eigenvectors are its rows here)
#undef PCA_GEMM
    hipLaunchKernelGGL(pca_final_kernel, dim3((unsigned)R), dim3(256), 0, st, T, psi, mean, (const int*)dim, (const int*)skip,
                       (const int*)info, psi_r, A_r, b_r, L);
    SPK_LAUNCH_CHECK("spk_pca_plda_batch (final)");
    return 0;
}
