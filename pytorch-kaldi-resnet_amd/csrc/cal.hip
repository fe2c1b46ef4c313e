// Calibration of trial scores on the device (include/spkcal.h): what follows the error-rate sweep of eval.hip.
//   spk_cal_apply - llr = ((w0 s0 + w1 s1) + ...) + b over K score columns
//   spk_cal_cllr  - the two softplus sums of Cllr, N_tar, N_non and miss / fa / actDCF at P Bayes thresholds, one pass
//   spk_cal_train - prior-weighted logistic regression by a damped Newton state machine that lives on the device
//   spk_cal_pav   - minCllr: tie pools, pool-adjacent-violators in int64 (tiles, then the concatenation), per-trial pool index
// Every fp64 operation is rounded on its own, as in eval.hip - apply, the counts and the actDCF doubles are the host's bit for bit:
#pragma clang fp contract(off)
#include "spk_common.h"

#define CAL_THREADS 256
#define CAL_ITEMS 4
#define CAL_BLOCK (CAL_THREADS * CAL_ITEMS)       // trials per block of apply / cllr / evaluate / the tie-pool scan
#define CAL_MAX_K 8
#define CAL_MAX_D (CAL_MAX_K + 1)
#define CAL_MAX_NV (1 + CAL_MAX_D + CAL_MAX_D * (CAL_MAX_D + 1) / 2)       // f, g, H at K = 8: 55
#define CAL_MAX_COSTS 8
#define PAV_TILE 1024                             // pools one workgroup runs the rule on in LDS: 16 KiB
#define PAV_THREADS 64
#define CAL_STATE_ELEMS 96
// state: theta [9], theta_acc [9], d [9], f_acc, f_last, lambda2, g [9] at 30, H [45] (lower triangle, row-major) at 40
#define ST_THETA 0
#define ST_ACC 9
#define ST_D 18
#define ST_FACC 27
#define ST_FLAST 28
#define ST_LAMBDA2 29
#define ST_G 30
#define ST_H 40
// istate: status (0 running, 1 converged, 2 not_converged, 3 singular), evaluations, Newton steps taken, halvings

extern "C" int spk_cal_max_k(void) { return CAL_MAX_K; }
extern "C" int spk_cal_tile(int which) { return which == 0 ? CAL_BLOCK : which == 1 ? PAV_TILE : which == 2 ? CAL_STATE_ELEMS : CAL_THREADS; }

static int cal_blocks(int T) { return (int)(((long long)T + CAL_BLOCK - 1) / CAL_BLOCK); }
static int pav_tiles(int T) { return (int)(((long long)T + PAV_TILE - 1) / PAV_TILE); }

struct CalTheta {
    double v[CAL_MAX_D];
};
struct CalCosts {
    double p[CAL_MAX_COSTS], c_miss[CAL_MAX_COSTS], c_fa[CAL_MAX_COSTS], eta[CAL_MAX_COSTS];
};

// sum over the block in a fixed order: halving tree in LDS; every thread gets the result
template <typename V>
static __device__ __forceinline__ V block_sum(V v, V* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = CAL_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    const V r = sh[0];
    __syncthreads();
    return r;
}

// ---- apply ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CAL_THREADS) void cal_apply_kernel(const double* __restrict__ cols, CalTheta th, int K,
                                                                double* __restrict__ llr, int T) {
    const long long i = (long long)blockIdx.x * CAL_THREADS + threadIdx.x;
    if (i >= T) return;
    double z = th.v[0] * cols[i];
    for (int k = 1; k < K; ++k) z = z + th.v[k] * cols[(size_t)k * T + i];
    llr[i] = z + th.v[K];
}

extern "C" int spk_cal_apply(const double* cols, const double* theta, int K, double* llr, int T, void* stream) {
    SPK_REQUIRE(cols && theta && llr, "spk_cal_apply: null pointer");
    SPK_REQUIRE(K >= 1 && K <= CAL_MAX_K, "spk_cal_apply: K=%d systems, must lie in [1, %d]", K, CAL_MAX_K);
    SPK_REQUIRE(T >= 1, "spk_cal_apply: T=%d must lie in [1, 2^31)", T);
    CalTheta th;
    for (int k = 0; k < CAL_MAX_D; ++k) th.v[k] = k <= K ? theta[k] : 0.0;
    hipLaunchKernelGGL(cal_apply_kernel, dim3((unsigned)(((long long)T + CAL_THREADS - 1) / CAL_THREADS)), dim3(CAL_THREADS), 0,
                       (hipStream_t)stream, cols, th, K, llr, T);
    SPK_LAUNCH_CHECK("spk_cal_apply");
    return 0;
}

// ---- Cllr and actDCF --------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ double softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// per block: pd [2][nb] = softplus sums over targets / non-targets, pi [1 + 2 * 8][nb] = targets, miss [8], fa [8]
__global__ __launch_bounds__(CAL_THREADS) void cal_cllr_kernel(const double* __restrict__ llr, const unsigned char* __restrict__ label,
                                                               CalCosts cs, int P, double* __restrict__ pd,
                                                               long long* __restrict__ pi, int T, int nb) {
    __shared__ double shd[CAL_THREADS];
    __shared__ int shi[CAL_THREADS];
    double st = 0.0, sn = 0.0;
    int nt = 0, miss[CAL_MAX_COSTS], fa[CAL_MAX_COSTS];
#pragma unroll
    for (int m = 0; m < CAL_MAX_COSTS; ++m) miss[m] = fa[m] = 0;
    for (int it = 0; it < CAL_ITEMS; ++it) {
        const long long i = (long long)blockIdx.x * CAL_BLOCK + it * CAL_THREADS + threadIdx.x;
        if (i >= T) break;
        const double l = llr[i];
        const bool tar = label[i] != 0;
        if (tar) st += softplus(-l);
        else sn += softplus(l);
        nt += tar;
#pragma unroll
        for (int m = 0; m < CAL_MAX_COSTS; ++m) {
            if (m < P) {
                const bool accept = l >= cs.eta[m];
                miss[m] += tar && !accept;
                fa[m] += !tar && accept;
            }
        }
    }
    st = block_sum(st, shd);
    sn = block_sum(sn, shd);
    nt = block_sum(nt, shi);
    if (threadIdx.x == 0) {
        pd[blockIdx.x] = st;
        pd[nb + blockIdx.x] = sn;
        pi[blockIdx.x] = nt;
    }
#pragma unroll
    for (int m = 0; m < CAL_MAX_COSTS; ++m) {
        if (m < P) {
            const int a = block_sum(miss[m], shi), b = block_sum(fa[m], shi);
            if (threadIdx.x == 0) {
                pi[(size_t)(1 + m) * nb + blockIdx.x] = a;
                pi[(size_t)(1 + CAL_MAX_COSTS + m) * nb + blockIdx.x] = b;
            }
        }
    }
}

// out_d: the two sums, then actDCF per triple; out_i: N_tar, N_non, then miss [P], fa [P]
__global__ __launch_bounds__(CAL_THREADS) void cal_cllr_final_kernel(const double* __restrict__ pd, const long long* __restrict__ pi,
                                                                     CalCosts cs, int P, double* __restrict__ out_d,
                                                                     long long* __restrict__ out_i, int T, int nb) {
    __shared__ double shd[CAL_THREADS];
    __shared__ long long shl[CAL_THREADS];
    for (int v = 0; v < 2; ++v) {
        double a = 0.0;
        for (int b = threadIdx.x; b < nb; b += CAL_THREADS) a += pd[(size_t)v * nb + b];
        a = block_sum(a, shd);
        if (threadIdx.x == 0) out_d[v] = a;
    }
    long long a = 0;
    for (int b = threadIdx.x; b < nb; b += CAL_THREADS) a += pi[b];
    const long long n_tar = block_sum(a, shl), n_non = (long long)T - n_tar;
    if (threadIdx.x == 0) {
        out_i[0] = n_tar;
        out_i[1] = n_non;
    }
    for (int m = 0; m < P; ++m) {
        long long x = 0, y = 0;
        for (int b = threadIdx.x; b < nb; b += CAL_THREADS) {
            x += pi[(size_t)(1 + m) * nb + b];
            y += pi[(size_t)(1 + CAL_MAX_COSTS + m) * nb + b];
        }
        const long long miss = block_sum(x, shl), fa = block_sum(y, shl);
        if (threadIdx.x == 0) {
            out_i[2 + m] = miss;
            out_i[2 + P + m] = fa;
            const double fnr = (double)miss / (double)n_tar, fpr = (double)fa / (double)n_non;
            const double p = cs.p[m], c_miss = cs.c_miss[m], c_fa = cs.c_fa[m];
            out_d[2 + m] = (c_miss * fnr * p + c_fa * fpr * (1.0 - p)) / fmin(c_miss * p, c_fa * (1.0 - p));
        }
    }
}

extern "C" long long spk_cal_cllr_ws_elems(int T) {
    if (T < 1) return -1;
    return (long long)cal_blocks(T) * (2 + 1 + 2 * CAL_MAX_COSTS);
}

extern "C" int spk_cal_cllr(const double* llr, const unsigned char* label, const double* costs, const double* eta, int P, double* out_d,
                            long long* out_i, void* ws, long long ws_elems, int T, void* stream) {
    SPK_REQUIRE(llr && label && out_d && out_i && ws, "spk_cal_cllr: null pointer");
    SPK_REQUIRE(T >= 2, "spk_cal_cllr: T=%d must lie in [2, 2^31)", T);
    SPK_REQUIRE(P >= 0 && P <= CAL_MAX_COSTS && (P == 0 || (costs && eta)), "spk_cal_cllr: P=%d cost triples, at most %d", P,
                CAL_MAX_COSTS);
    SPK_REQUIRE(ws_elems >= spk_cal_cllr_ws_elems(T), "spk_cal_cllr: workspace of %lld words, %lld needed", ws_elems,
                spk_cal_cllr_ws_elems(T));
    CalCosts cs;
    for (int m = 0; m < CAL_MAX_COSTS; ++m) {
        cs.p[m] = m < P ? costs[3 * m] : 0.0;
        cs.c_miss[m] = m < P ? costs[3 * m + 1] : 0.0;
        cs.c_fa[m] = m < P ? costs[3 * m + 2] : 0.0;
        cs.eta[m] = m < P ? eta[m] : 0.0;
    }
    const int nb = cal_blocks(T);
    double* pd = (double*)ws;
    long long* pi = (long long*)ws + 2 * (size_t)nb;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cal_cllr_kernel, dim3(nb), dim3(CAL_THREADS), 0, st, llr, label, cs, P, pd, pi, T, nb);
    hipLaunchKernelGGL(cal_cllr_final_kernel, dim3(1), dim3(CAL_THREADS), 0, st, pd, pi, cs, P, out_d, out_i, T, nb);
    SPK_LAUNCH_CHECK("spk_cal_cllr");
    return 0;
}

// ---- training ---------------------------------------------------------------------------------------------------------------------
__global__ void cal_train_init_kernel(double* state, long long* istate) {
    const int i = threadIdx.x;
    if (i < CAL_STATE_ELEMS) state[i] = i == ST_FACC ? __builtin_inf() : 0.0;
    if (i < 4) istate[i] = 0;
}

// One pass over the trials at the theta of the state: per-block partial sums of f, g (K + 1) and the lower triangle of H, every
// term weighted by its class (p / N_tar or (1 - p) / N_non).  partial [NV][nb].  A wave adds its 64 lanes by a fixed shuffle
// tree, the four waves meet in LDS and are added in wave order: the same bits on every run.
template <int K>
__global__ __launch_bounds__(CAL_THREADS) void cal_eval_kernel(const double* __restrict__ cols, const unsigned char* __restrict__ label,
                                                               const double* __restrict__ state, const long long* __restrict__ istate,
                                                               double* __restrict__ partial, double cp, double cn, double tau, int T,
                                                               int nb) {
    if (istate[0] != 0) return;                                // (uniform: the machine has stopped)
    constexpr int D = K + 1, NV = 1 + D + D * (D + 1) / 2;
    __shared__ double sh[CAL_THREADS / 64][NV];
    double th[D], acc[NV];
#pragma unroll
    for (int k = 0; k < D; ++k) th[k] = state[ST_THETA + k];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    for (int it = 0; it < CAL_ITEMS; ++it) {
        const long long i = (long long)blockIdx.x * CAL_BLOCK + it * CAL_THREADS + threadIdx.x;
        if (i >= T) break;
        double s[D];
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] = cols[(size_t)k * T + i];
        s[K] = 1.0;
        double z = th[0] * s[0];
#pragma unroll
        for (int k = 1; k < K; ++k) z = z + th[k] * s[k];
        z = z + th[K];
        const double x = z + tau;
        const bool tar = label[i] != 0;
        const double y = tar ? -x : x;                         // the term is softplus(y)
        const double e = exp(-fabs(y));
        const double den = 1.0 + e;
        const double sig = (y >= 0.0 ? 1.0 : e) / den;         // softplus'(y)
        const double c = tar ? cp : cn;
        acc[0] += c * (fmax(y, 0.0) + log1p(e));
        const double cd = c * (tar ? -sig : sig), ch = c * (e / (den * den));
        int idx = 1 + D;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            acc[1 + j] += cd * s[j];
            const double chj = ch * s[j];
#pragma unroll
            for (int k = 0; k <= j; ++k) acc[idx++] += chj * s[k];
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double a = acc[v];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a += __shfl_down(a, off, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][v] = a;
    }
    __syncthreads();
    if ((int)threadIdx.x < NV) {
        double a = sh[0][threadIdx.x];
        for (int w = 1; w < CAL_THREADS / 64; ++w) a += sh[w][threadIdx.x];
        partial[(size_t)threadIdx.x * nb + blockIdx.x] = a;
    }
}

// One workgroup: the partial sums of every block, then - one lane - the L2 term, the Cholesky factor and the four transitions.
__global__ __launch_bounds__(CAL_THREADS) void cal_step_kernel(double* state, long long* istate, const double* __restrict__ partial,
                                                               int K, int nb, double l2, double epsilon, int last) {
    if (istate[0] != 0) return;
    __shared__ double shd[CAL_THREADS];
    __shared__ double tot[CAL_MAX_NV], L[CAL_MAX_D * (CAL_MAX_D + 1) / 2], xs[CAL_MAX_D];
    const int D = K + 1, NV = 1 + D + D * (D + 1) / 2;
    for (int v = 0; v < NV; ++v) {
        double a = 0.0;
        for (int b = threadIdx.x; b < nb; b += CAL_THREADS) a += partial[(size_t)v * nb + b];
        a = block_sum(a, shd);
        if (threadIdx.x == 0) tot[v] = a;
    }
    if (threadIdx.x != 0) return;
    double* theta = state + ST_THETA;
    double* tacc = state + ST_ACC;
    double* d = state + ST_D;
    double ww = 0.0;
    for (int k = 0; k < K; ++k) ww = ww + theta[k] * theta[k];
    const double f = tot[0] + 0.5 * l2 * ww;
    istate[1] += 1;
    state[ST_FLAST] = f;
    long long status = 0;
    if (!(f <= state[ST_FACC])) {                              // 1: not a descent (or not a number): half the step
        for (int j = 0; j < D; ++j) {
            d[j] = 0.5 * d[j];
            theta[j] = tacc[j] + d[j];
        }
        istate[3] += 1;
    } else {                                                   // 2: accept
        state[ST_FACC] = f;
        for (int j = 0; j < D; ++j) {
            tacc[j] = theta[j];
            tot[1 + j] = tot[1 + j] + (j < K ? l2 * theta[j] : 0.0);
            state[ST_G + j] = tot[1 + j];
        }
        for (int j = 0; j < D; ++j) {
            const int jj = 1 + D + j * (j + 1) / 2 + j;
            if (j < K) tot[jj] = tot[jj] + l2;
        }
        for (int v = 0; v < D * (D + 1) / 2; ++v) state[ST_H + v] = tot[1 + D + v];
        const double* g = tot + 1;
        const double* H = tot + 1 + D;
        for (int j = 0; j < D && status == 0; ++j) {
            for (int k = 0; k <= j; ++k) {
                double s = H[j * (j + 1) / 2 + k];
                for (int m = 0; m < k; ++m) s = s - L[j * (j + 1) / 2 + m] * L[k * (k + 1) / 2 + m];
                if (k == j) {
                    if (!(s > 0.0)) {
                        status = 3;
                        break;
                    }
                    L[j * (j + 1) / 2 + j] = sqrt(s);
                } else {
                    L[j * (j + 1) / 2 + k] = s / L[k * (k + 1) / 2 + k];
                }
            }
        }
        if (status == 0) {                                     // 3: x = H^-1 g, d = -x, lambda2 = g . x
            for (int j = 0; j < D; ++j) {
                double s = g[j];
                for (int m = 0; m < j; ++m) s = s - L[j * (j + 1) / 2 + m] * xs[m];
                xs[j] = s / L[j * (j + 1) / 2 + j];
            }
            for (int j = D - 1; j >= 0; --j) {
                double s = xs[j];
                for (int m = j + 1; m < D; ++m) s = s - L[m * (m + 1) / 2 + j] * xs[m];
                xs[j] = s / L[j * (j + 1) / 2 + j];
            }
            double lambda2 = 0.0;
            for (int j = 0; j < D; ++j) lambda2 = lambda2 + g[j] * xs[j];
            state[ST_LAMBDA2] = lambda2;
            if (lambda2 <= epsilon) {
                status = 1;
            } else {                                           // 4: the Newton step
                for (int j = 0; j < D; ++j) {
                    d[j] = -xs[j];
                    theta[j] = theta[j] + d[j];
                }
                istate[2] += 1;
            }
        }
    }
    if (status == 0 && last) status = 2;
    istate[0] = status;
}

extern "C" long long spk_cal_train_ws_elems(int T, int K) {
    if (T < 1 || K < 1 || K > CAL_MAX_K) return -1;
    return (long long)cal_blocks(T) * (1 + (K + 1) + (K + 1) * (K + 2) / 2);
}

template <int K>
static void launch_eval(hipStream_t st, int nb, const double* cols, const unsigned char* label, const double* state,
                        const long long* istate, double* partial, double cp, double cn, double tau, int T) {
    hipLaunchKernelGGL(cal_eval_kernel<K>, dim3(nb), dim3(CAL_THREADS), 0, st, cols, label, state, istate, partial, cp, cn, tau, T, nb);
}

extern "C" int spk_cal_train(const double* cols, const unsigned char* label, int K, int T, long long n_tar, double p_target, double tau,
                             double l2, double epsilon, int max_iters, double* state, long long* istate, double* ws,
                             long long ws_elems, void* stream) {
    SPK_REQUIRE(cols && label && state && istate && ws, "spk_cal_train: null pointer");
    SPK_REQUIRE(K >= 1 && K <= CAL_MAX_K, "spk_cal_train: K=%d systems, must lie in [1, %d]", K, CAL_MAX_K);
    SPK_REQUIRE(T >= 2, "spk_cal_train: T=%d must lie in [2, 2^31)", T);
    SPK_REQUIRE(n_tar >= 1 && n_tar < T, "spk_cal_train: %lld targets among %d trials: both classes are needed", n_tar, T);
    SPK_REQUIRE(p_target > 0.0 && p_target < 1.0 && l2 >= 0.0 && epsilon >= 0.0 && tau == tau,
                "spk_cal_train: p_target in (0, 1), l2 >= 0 and epsilon >= 0 are needed");
    SPK_REQUIRE(max_iters >= 1 && max_iters <= 10000, "spk_cal_train: max_iters=%d must lie in [1, 10000]", max_iters);
    SPK_REQUIRE(ws_elems >= spk_cal_train_ws_elems(T, K), "spk_cal_train: workspace of %lld words, %lld needed", ws_elems,
                spk_cal_train_ws_elems(T, K));
    const int nb = cal_blocks(T);
    const double cp = p_target / (double)n_tar, cn = (1.0 - p_target) / (double)(T - n_tar);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cal_train_init_kernel, dim3(1), dim3(128), 0, st, state, istate);
    for (int it = 0; it < max_iters; ++it) {
        switch (K) {
            case 1: launch_eval<1>(st, nb, cols, label, state, istate, ws, cp, cn, tau, T); break;
            case 2: launch_eval<2>(st, nb, cols, label, state, istate, ws, cp, cn, tau, T); break;
            case 3: launch_eval<3>(st, nb, cols, label, state, istate, ws, cp, cn, tau, T); break;
            case 4: launch_eval<4>(st, nb, cols, label, state, istate, ws, cp, cn, tau, T); break;
            case 5: launch_eval<5>(st, nb, cols, label, state, istate, ws, cp, cn, tau, T); break;
            case 6: launch_eval<6>(st, nb, cols, label, state, istate, ws, cp, cn, tau, T); break;
            case 7: launch_eval<7>(st, nb, cols, label, state, istate, ws, cp, cn, tau, T); break;
            default: launch_eval<8>(st, nb, cols, label, state, istate, ws, cp, cn, tau, T); break;
        }
        hipLaunchKernelGGL(cal_step_kernel, dim3(1), dim3(CAL_THREADS), 0, st, state, istate, ws, K, nb, l2, epsilon,
                           it == max_iters - 1 ? 1 : 0);
    }
    SPK_LAUNCH_CHECK("spk_cal_train");
    return 0;
}

// ---- minCllr: pool-adjacent-violators in integers -------------------------------------------------------------------------------
// Sorted position i opens a tie pool when its score differs from that of position i - 1 (-0.0 == +0.0; no NaN).  flag / label
// counts per block, their exclusive scans, then every opening position writes (start, targets before it) of its pool.
static __device__ __forceinline__ void pav_items(const double* __restrict__ score, const unsigned char* __restrict__ label,
                                                 const unsigned* __restrict__ order, long long base, int T, int* flag, int* lab) {
    for (int k = 0; k < CAL_ITEMS; ++k) {
        const long long i = base + k;
        flag[k] = lab[k] = 0;
        if (i < T) {
            const unsigned o = order[i];
            lab[k] = label[o] != 0;
            flag[k] = i == 0 || score[o] != score[order[i - 1]];
        }
    }
}

__global__ __launch_bounds__(CAL_THREADS) void pav_count_kernel(const double* __restrict__ score, const unsigned char* __restrict__ label,
                                                                const unsigned* __restrict__ order, long long* __restrict__ blk_f,
                                                                long long* __restrict__ blk_l, int T) {
    __shared__ int sh[CAL_THREADS];
    int flag[CAL_ITEMS], lab[CAL_ITEMS], nf = 0, nl = 0;
    pav_items(score, label, order, (long long)blockIdx.x * CAL_BLOCK + (long long)threadIdx.x * CAL_ITEMS, T, flag, lab);
    for (int k = 0; k < CAL_ITEMS; ++k) {
        nf += flag[k];
        nl += lab[k];
    }
    nf = block_sum(nf, sh);
    nl = block_sum(nl, sh);
    if (threadIdx.x == 0) {
        blk_f[blockIdx.x] = nf;
        blk_l[blockIdx.x] = nl;
    }
}

// in place, one workgroup: a[b] -> the sum of a[0 .. b); a[n] = the total, also written to *total when given
__global__ __launch_bounds__(CAL_THREADS) void cal_scan_kernel(long long* a, int n, long long* total) {
    __shared__ long long sh[CAL_THREADS];
    long long carry = 0;
    for (int lo = 0; lo < n; lo += CAL_THREADS) {
        const int b = lo + threadIdx.x;
        const long long mine = b < n ? a[b] : 0;
        sh[threadIdx.x] = mine;
        __syncthreads();
        for (int off = 1; off < CAL_THREADS; off <<= 1) {
            const long long add = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (b < n) a[b] = carry + sh[threadIdx.x] - mine;
        carry += sh[CAL_THREADS - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a[n] = carry;
        if (total) *total = carry;
    }
}

// inclusive scan of one int per thread over the block
static __device__ __forceinline__ int block_scan(int v, int* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < CAL_THREADS; off <<= 1) {
        const int add = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    const int r = sh[threadIdx.x];
    __syncthreads();
    return r;
}

// starts [P0 + 1][2] = (first sorted position, targets before it), the last row (T, N_tar)
__global__ __launch_bounds__(CAL_THREADS) void pav_starts_kernel(const double* __restrict__ score, const unsigned char* __restrict__ label,
                                                                 const unsigned* __restrict__ order, const long long* __restrict__ blk_f,
                                                                 const long long* __restrict__ blk_l, long long* __restrict__ starts,
                                                                 int T, int nb) {
    __shared__ int sh[CAL_THREADS];
    const long long base = (long long)blockIdx.x * CAL_BLOCK + (long long)threadIdx.x * CAL_ITEMS;
    int flag[CAL_ITEMS], lab[CAL_ITEMS], nf = 0, nl = 0;
    pav_items(score, label, order, base, T, flag, lab);
    for (int k = 0; k < CAL_ITEMS; ++k) {
        nf += flag[k];
        nl += lab[k];
    }
    long long p = blk_f[blockIdx.x] + block_scan(nf, sh) - nf;          // pools opened before this thread's first position
    long long ct = blk_l[blockIdx.x] + block_scan(nl, sh) - nl;         // targets before it
    for (int k = 0; k < CAL_ITEMS; ++k) {
        if (base + k >= T) break;
        if (flag[k]) {
            starts[2 * p] = base + k;
            starts[2 * p + 1] = ct;
            ++p;
        }
        ct += lab[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const long long P0 = blk_f[nb];
        starts[2 * P0] = T;
        starts[2 * P0 + 1] = blk_l[nb];
    }
}

// tie [P0][2] = (targets, trials) of every tie pool
__global__ __launch_bounds__(CAL_THREADS) void pav_ties_kernel(const long long* __restrict__ starts, const long long* __restrict__ count,
                                                               long long* __restrict__ tie) {
    const long long p = (long long)blockIdx.x * CAL_THREADS + threadIdx.x;
    if (p >= *count) return;
    tie[2 * p] = starts[2 * p + 3] - starts[2 * p + 1];
    tie[2 * p + 1] = starts[2 * p + 2] - starts[2 * p];
}

// The rule on one tile of the list `in` [*count][2]: one lane, the stack in LDS in place (it never passes the read position).
// out [tile * PAV_TILE ...][2] and tile_cnt [tile] = what is left of the tile.
__global__ __launch_bounds__(PAV_THREADS) void pav_tile_kernel(const long long* __restrict__ in, const long long* __restrict__ count,
                                                               long long* __restrict__ out, long long* __restrict__ tile_cnt) {
    __shared__ long long st[PAV_TILE], sn[PAV_TILE];
    const long long lo = (long long)blockIdx.x * PAV_TILE, left = *count - lo;
    const int m = left < 0 ? 0 : left > PAV_TILE ? PAV_TILE : (int)left;
    if (m == 0) {
        if (threadIdx.x == 0) tile_cnt[blockIdx.x] = 0;
        return;
    }
    for (int i = threadIdx.x; i < m; i += PAV_THREADS) {
        st[i] = in[2 * (lo + i)];
        sn[i] = in[2 * (lo + i) + 1];
    }
    __syncthreads();
    __shared__ int left_over;
    if (threadIdx.x == 0) {
        int sp = 0;
        for (int i = 0; i < m; ++i) {
            long long t = st[i], n = sn[i];
            while (sp > 0 && st[sp - 1] * n >= t * sn[sp - 1]) {       // at most i pops in all: sp <= i
                --sp;
                t += st[sp];
                n += sn[sp];
            }
            st[sp] = t;
            sn[sp] = n;
            ++sp;
        }
        left_over = sp;
        tile_cnt[blockIdx.x] = sp;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < left_over; i += PAV_THREADS) {
        out[2 * (lo + i)] = st[i];
        out[2 * (lo + i) + 1] = sn[i];
    }
}

// tile_off: the exclusive scan of tile_cnt; one workgroup per tile copies its rows to their place in the concatenation
__global__ __launch_bounds__(PAV_THREADS) void pav_compact_kernel(const long long* __restrict__ src, const long long* __restrict__ tile_off,
                                                                  long long* __restrict__ dst) {
    const long long at = tile_off[blockIdx.x];
    const int m = (int)(tile_off[blockIdx.x + 1] - at);
    const long long lo = (long long)blockIdx.x * PAV_TILE;
    for (int i = threadIdx.x; i < m; i += PAV_THREADS) {
        dst[2 * (at + i)] = src[2 * (lo + i)];
        dst[2 * (at + i) + 1] = src[2 * (lo + i) + 1];
    }
}

// The rule over the whole concatenation, one workgroup: the list is staged through LDS a tile at a time, one lane runs the stack,
// which lives in `pools` (the top in registers).  *P = the pools left.
__global__ __launch_bounds__(CAL_THREADS) void pav_final_kernel(const long long* __restrict__ in, const long long* __restrict__ count,
                                                                long long* pools, long long* __restrict__ P, int max_chunks) {
    __shared__ long long st[PAV_TILE], sn[PAV_TILE];
    const long long M = *count;
    long long sp = 0, ct = 0, cn = 0;
    bool top = false;
    for (int c = 0; c < max_chunks; ++c) {
        const long long lo = (long long)c * PAV_TILE;
        if (lo >= M) break;                                    // (uniform)
        const int m = M - lo > PAV_TILE ? PAV_TILE : (int)(M - lo);
        for (int i = threadIdx.x; i < m; i += CAL_THREADS) {
            st[i] = in[2 * (lo + i)];
            sn[i] = in[2 * (lo + i) + 1];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 0; i < m; ++i) {
                long long t = st[i], n = sn[i];
                while (top && ct * n >= t * cn) {              // every pop removes a pool for good: at most M in all
                    t += ct;
                    n += cn;
                    if (sp > 0) {
                        --sp;
                        ct = pools[2 * sp];
                        cn = pools[2 * sp + 1];
                    } else {
                        top = false;
                    }
                }
                if (top) {
                    pools[2 * sp] = ct;
                    pools[2 * sp + 1] = cn;
                    ++sp;
                }
                ct = t;
                cn = n;
                top = true;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (top) {
            pools[2 * sp] = ct;
            pools[2 * sp + 1] = cn;
            ++sp;
        }
        *P = sp;
    }
}

// cum [P + 1]: the first sorted position of every final pool (exclusive scan of n), and minCllr: each thread adds the terms of a
// run of consecutive pools in pool order, the runs are added by the fixed tree
__global__ __launch_bounds__(CAL_THREADS) void pav_finish_kernel(const long long* __restrict__ pools, const long long* __restrict__ Pp,
                                                                 const long long* __restrict__ n_tar_p, long long* __restrict__ cum,
                                                                 double* __restrict__ out_d, int T, int max_chunks) {
    __shared__ long long sh[CAL_THREADS];
    __shared__ double shd[CAL_THREADS];
    const long long P = *Pp, n_tar = *n_tar_p, n_non = (long long)T - n_tar;
    long long carry = 0;
    for (int c = 0; c < max_chunks; ++c) {
        const long long lo = (long long)c * CAL_THREADS;
        if (lo >= P) break;
        const long long b = lo + threadIdx.x;
        const long long mine = b < P ? pools[2 * b + 1] : 0;
        sh[threadIdx.x] = mine;
        __syncthreads();
        for (int off = 1; off < CAL_THREADS; off <<= 1) {
            const long long add = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (b < P) cum[b] = carry + sh[threadIdx.x] - mine;
        carry += sh[CAL_THREADS - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) cum[P] = carry;
    const long long run = (P + CAL_THREADS - 1) / CAL_THREADS;
    const double d_tar = (double)n_tar, d_non = (double)n_non;
    double a = 0.0, b = 0.0;
    for (int c = 0; c < max_chunks; ++c) {                     // (run <= max_chunks)
        const long long q = (long long)threadIdx.x * run + c;
        if (c >= run || q >= P) break;
        const long long t = pools[2 * q], n = pools[2 * q + 1];
        if (t > 0 && t < n) {
            const double dt = (double)t, dn = (double)(n - t);
            a += dt * log1p((dn / dt) * (d_tar / d_non));
            b += dn * log1p((dt / dn) * (d_non / d_tar));
        }
    }
    a = block_sum(a, shd);
    b = block_sum(b, shd);
    if (threadIdx.x == 0) out_d[0] = ((1.0 / d_tar) * a + (1.0 / d_non) * b) / (2.0 * 0.69314718055994530942);
}

// pool_of [trial] = the final pool that holds its sorted position: the last q with cum[q] <= i
__global__ __launch_bounds__(CAL_THREADS) void pav_index_kernel(const unsigned* __restrict__ order, const long long* __restrict__ cum,
                                                                const long long* __restrict__ Pp, int* __restrict__ pool_of, int T) {
    const long long i = (long long)blockIdx.x * CAL_THREADS + threadIdx.x;
    if (i >= T) return;
    long long lo = 0, hi = *Pp;                                // cum[lo] <= i < cum[hi]
    for (int step = 0; step < 32 && hi - lo > 1; ++step) {
        const long long mid = (lo + hi) >> 1;
        if (cum[mid] <= i) lo = mid;
        else hi = mid;
    }
    pool_of[order[i]] = (int)lo;
}

extern "C" long long spk_cal_pav_ws_elems(int T) {
    if (T < 1) return -1;
    return 4 * ((long long)T + 1) + 2 * ((long long)cal_blocks(T) + 1) + (long long)pav_tiles(T) + 1;
}

extern "C" int spk_cal_pav(const double* score, const unsigned char* label, const unsigned* order, long long* tie, long long* pools,
                           long long* counts, int* pool_of, double* out_d, long long* ws, long long ws_elems, int T, int upto,
                           void* stream) {
    SPK_REQUIRE(score && label && order && tie && pools && counts && pool_of && out_d && ws, "spk_cal_pav: null pointer");
    SPK_REQUIRE(T >= 2, "spk_cal_pav: T=%d must lie in [2, 2^31)", T);
    SPK_REQUIRE(ws_elems >= spk_cal_pav_ws_elems(T), "spk_cal_pav: workspace of %lld words, %lld needed", ws_elems,
                spk_cal_pav_ws_elems(T));
    const int nb = cal_blocks(T), nt = pav_tiles(T);
    long long* buf_a = ws;                                     // [T + 1][2]
    long long* buf_b = buf_a + 2 * ((size_t)T + 1);            // [T + 1][2]
    long long* blk_f = buf_b + 2 * ((size_t)T + 1);            // [nb + 1]
    long long* blk_l = blk_f + nb + 1;                         // [nb + 1]
    long long* tile_cnt = blk_l + nb + 1;                      // [nt + 1]
    hipStream_t st = (hipStream_t)stream;
    // counts: tie pools, pools after the tiles, after the tiles of their concatenation, final pools, targets
    hipLaunchKernelGGL(pav_count_kernel, dim3(nb), dim3(CAL_THREADS), 0, st, score, label, order, blk_f, blk_l, T);
    hipLaunchKernelGGL(cal_scan_kernel, dim3(1), dim3(CAL_THREADS), 0, st, blk_f, nb, counts + 0);
    hipLaunchKernelGGL(cal_scan_kernel, dim3(1), dim3(CAL_THREADS), 0, st, blk_l, nb, counts + 4);
    hipLaunchKernelGGL(pav_starts_kernel, dim3(nb), dim3(CAL_THREADS), 0, st, score, label, order, blk_f, blk_l, buf_a, T, nb);
    hipLaunchKernelGGL(pav_ties_kernel, dim3((unsigned)(((long long)T + CAL_THREADS - 1) / CAL_THREADS)), dim3(CAL_THREADS), 0, st, buf_a,
                       counts + 0, tie);
    if (upto != 1) {
        const long long* in = tie;
        for (int level = 0; level < 2; ++level) {
            hipLaunchKernelGGL(pav_tile_kernel, dim3(nt), dim3(PAV_THREADS), 0, st, in, counts + level, buf_a, tile_cnt);
            hipLaunchKernelGGL(cal_scan_kernel, dim3(1), dim3(CAL_THREADS), 0, st, tile_cnt, nt, counts + level + 1);
            hipLaunchKernelGGL(pav_compact_kernel, dim3(nt), dim3(PAV_THREADS), 0, st, buf_a, tile_cnt, buf_b);
            in = buf_b;
        }
    }
    if (upto != 1 && upto != 2) {
        hipLaunchKernelGGL(pav_final_kernel, dim3(1), dim3(CAL_THREADS), 0, st, buf_b, counts + 2, pools, counts + 3, nt);
        hipLaunchKernelGGL(pav_finish_kernel, dim3(1), dim3(CAL_THREADS), 0, st, pools, counts + 3, counts + 4, buf_a, out_d, T,
                           (int)(((long long)T + CAL_THREADS - 1) / CAL_THREADS));
        hipLaunchKernelGGL(pav_index_kernel, dim3((unsigned)(((long long)T + CAL_THREADS - 1) / CAL_THREADS)), dim3(CAL_THREADS), 0, st,
                           order, buf_a, counts + 3, pool_of, T);
    }
    SPK_LAUNCH_CHECK("spk_cal_pav");
    return 0;
}
