// Diarization back end on the device (DESIGN.md sections 6n and 6o): what Kaldi's callhome_diarization recipe runs behind the sliding-window
// extraction - ivector-plda-scoring-dense (its per-recording PCA: csrc/pca.hip, section 6p) and agglomerative-cluster.
//   spk_diar_tables   - host only: checks rec_off and derives the three offset tables both kernels read
//   spk_score_dense_q - q_i = scale * sum_d k_d U_id^2 per row (one wave per row, fp64, a fixed lane order)
//   spk_score_dense   - S[i][j] = (float)(q_i + q_j + K + sum_d g_d U_id U_jd) for every pair of rows of one recording, all
//                       recordings of a batch in one launch, on v_mfma_f64_16x16x4_f64: one wave per 16 x 16 tile of the upper
//                       triangle, mirrored, so S == S^T bit for bit
//   spk_ahc_batch     - average-linkage agglomerative clustering, one workgroup per recording running its whole merge loop with
//                       __syncthreads() alone: nothing waits on another workgroup
//   spk_vbx_batch     - VBx resegmentation (section 6o): a variational-Bayes HMM over the window rows, one workgroup per recording
//                       running every iteration, its forward-backward pass in scaled form on one wave
// Fragment map of the fp64 matrix instruction: see csrc/plda.hip.  No floating-point atomics anywhere: the same bits on every run.
#pragma clang fp contract(off)
#include "spk_common.h"

#include <vector>

typedef double f64x4 __attribute__((ext_vector_type(4)));
#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

#define DIAR_MAX_D 512
#define AHC_THREADS 256
#define AHC_WAVES (AHC_THREADS / 64)
#define AHC_MAX_N 8192          // sizes and cached columns are 16-bit in LDS: 2 * 2 * 8192 bytes, and a rescan list of the same size
#define AHC_NONE 0xffffu

// ---- offset tables --------------------------------------------------------------------------------------------------------------
// tab [3][R + 1]: rec_off (rows), mat_off (elements of the n x n matrices laid end to end) and tile_off (16 x 16 tiles of the upper
// triangles).  rec_off must start at 0, be strictly increasing and end at Ntot; sum n^2 must stay below 2^31.
int spk_diar_check(const char* who, const long long* rec_off, int R, long long Ntot, long long* tab) {
    SPK_REQUIRE(rec_off && R >= 1 && Ntot >= 1, "%s: bad arguments (R=%d, Ntot=%lld)", who, R, Ntot);
    SPK_REQUIRE(rec_off[0] == 0 && rec_off[R] == Ntot, "%s: rec_off must run from 0 to Ntot=%lld, got %lld .. %lld", who, Ntot,
                rec_off[0], rec_off[R]);
    long long mat = 0, tile = 0;
    for (int r = 0; r < R; ++r) {
        const long long n = rec_off[r + 1] - rec_off[r];
        SPK_REQUIRE(n >= 1, "%s: recording %d is empty or rec_off decreases (rec_off %lld, %lld)", who, r, rec_off[r], rec_off[r + 1]);
        SPK_REQUIRE(n < (1ll << 16) && mat + n * n < (1ll << 31), "%s: the sum of n^2 reaches 2^31 at recording %d (n=%lld)", who, r, n);
        if (tab) {
            tab[r] = rec_off[r];
            tab[(R + 1) + r] = mat;
            tab[2 * (R + 1) + r] = tile;
        }
        const long long t = (n + 15) / 16;
        mat += n * n;
        tile += t * (t + 1) / 2;
    }
    if (tab) {
        tab[R] = Ntot;
        tab[(R + 1) + R] = mat;
        tab[2 * (R + 1) + R] = tile;
    }
    return 0;
}

extern "C" int spk_diar_tables(const long long* rec_off, int R, long long Ntot, long long* tab) {
    SPK_REQUIRE(tab, "spk_diar_tables: tab is missing");
    return spk_diar_check("spk_diar_tables", rec_off, R, Ntot, tab);
}

// ---- q ----------------------------------------------------------------------------------------------------------------------------
// REC (the per-recording forms of section 6p): k [R][D], row i takes the k of its recording (rec_off = the first row of tab)
template <bool REC>
__global__ __launch_bounds__(256) void dense_q_kernel(const double* __restrict__ U, const double* __restrict__ k, double scale,
                                                      double* __restrict__ q, long long N, int D, const long long* __restrict__ rec_off,
                                                      int R) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    if (REC) {
        int lo = 0, hi = R;                                       // the last r with rec_off[r] <= i
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (rec_off[mid] <= i) lo = mid;
            else hi = mid;
        }
        k += (size_t)lo * D;
    }
    const double* u = U + (size_t)i * D;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) s += k[d] * u[d] * u[d];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) q[i] = scale * s;
}

extern "C" int spk_score_dense_q(const double* U, const double* k, double scale, double* q, long long N, int D, void* stream) {
    SPK_REQUIRE(U && k && q && N >= 1 && N < (1ll << 32) && D >= 1, "spk_score_dense_q: bad arguments");
    hipLaunchKernelGGL(dense_q_kernel<false>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, U, k, scale, q, N, D,
                       (const long long*)nullptr, 0);
    SPK_LAUNCH_CHECK("spk_score_dense_q");
    return 0;
}

extern "C" int spk_score_dense_q_rec(const double* U, const long long* rec_off, const long long* tab_dev, const double* k, double scale,
                                     double* q, long long Ntot, int D, int R, void* stream) {
    SPK_REQUIRE(D >= 1 && D <= DIAR_MAX_D, "spk_score_dense_q_rec: D=%d must lie in [1, %d]", D, DIAR_MAX_D);
    const int rc = spk_diar_check("spk_score_dense_q_rec", rec_off, R, Ntot, nullptr);
    if (rc) return rc;
    SPK_REQUIRE(U && tab_dev && k && q, "spk_score_dense_q_rec: null device pointer");
    hipLaunchKernelGGL(dense_q_kernel<true>, dim3((unsigned)((Ntot + 3) / 4)), dim3(256), 0, (hipStream_t)stream, U, k, scale, q, Ntot,
                       D, tab_dev, R);
    SPK_LAUNCH_CHECK("spk_score_dense_q_rec");
    return 0;
}

// ---- dense scores -----------------------------------------------------------------------------------------------------------------
// One wave per tile.  The sum over d may run in any order, so step s of lane group gq takes d = d0 + 4 gq + s: a lane reads four
// consecutive values of its row.  D is padded to a multiple of 16 with zeros in registers.  A tile on the diagonal computes
// (g u_i) u_j and (g u_j) u_i, whose roundings differ: only its entries with i <= j are kept, and every entry is stored twice.
// REC: g [R][D] and Kr [R], the terms of the tile's recording.
template <bool REC>
__global__ __launch_bounds__(256) void score_dense_kernel(const double* __restrict__ U, const long long* __restrict__ tab,
                                                          const double* __restrict__ q, const double* __restrict__ g, double K,
                                                          const double* __restrict__ Kr, float* __restrict__ out, int D, int R,
                                                          long long ntiles) {
    const int lane = threadIdx.x & 63, c = lane & 15, gq = lane >> 4;
    const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntiles) return;                                   // wave-uniform
    const long long* rec_off = tab;
    const long long* mat_off = tab + (R + 1);
    const long long* tile_off = tab + 2 * (R + 1);
    int lo = 0, hi = R;                                           // the last r with tile_off[r] <= tile
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_off[mid] <= tile) lo = mid;
        else hi = mid;
    }
    const int r = lo;
    if (REC) {
        g += (size_t)r * D;
        K = Kr[r];
    }
    const long long row0 = rec_off[r];
    const int n = (int)(rec_off[r + 1] - row0), T = (n + 15) >> 4;
    int p = (int)(tile - tile_off[r]), ti = 0;
    while (p >= T - ti) {
        p -= T - ti;
        ++ti;
    }
    const int tj = ti + p;
    const int ia = ti * 16 + c, jb = tj * 16 + c;                 // the row this lane feeds to A and to B
    const bool va = ia < n, vb = jb < n;
    const double* ua = U + (size_t)(row0 + (va ? ia : 0)) * D;
    const double* ub = U + (size_t)(row0 + (vb ? jb : 0)) * D;
    f64x4 acc = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int d0 = 0; d0 < D; d0 += 16) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int d = d0 + 4 * gq + s;
            const bool vd = d < D;
            const double a = (va && vd) ? g[d] * ua[d] : 0.0;
            const double b = (vb && vd) ? ub[d] : 0.0;
            acc = MFMA_F64(a, b, acc);
        }
    }
    float* S = out + mat_off[r];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int i = ti * 16 + gq + 4 * rr, j = tj * 16 + c;
        if (i < n && j < n && (ti != tj || i <= j)) {
            const float v = (float)(((acc[rr] + q[row0 + i]) + q[row0 + j]) + K);
            S[(size_t)i * n + j] = v;
            S[(size_t)j * n + i] = v;
        }
    }
}

// the host side of both entries: K is read where !REC, Kr where REC
template <bool REC>
static int score_dense_launch(const char* who, const double* U, const long long* rec_off, const long long* tab_dev, const double* q,
                              const double* g, double K, const double* Kr, float* out, long long Ntot, int D, int R, void* stream) {
    SPK_REQUIRE(D >= 1 && D <= DIAR_MAX_D, "%s: D=%d must lie in [1, %d]", who, D, DIAR_MAX_D);
    std::vector<long long> tab;
    if (R >= 1) tab.resize(3 * ((size_t)R + 1));
    const int rc = spk_diar_check(who, rec_off, R, Ntot, tab.data());
    if (rc) return rc;
    SPK_REQUIRE(U && tab_dev && q && g && (!REC || Kr) && out, "%s: null device pointer", who);
    const long long ntiles = tab[2 * (R + 1) + R];
    hipLaunchKernelGGL(score_dense_kernel<REC>, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, U, tab_dev, q, g,
                       K, Kr, out, D, R, ntiles);
    SPK_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int spk_score_dense(const double* U, const long long* rec_off, const long long* tab_dev, const double* q, const double* g,
                               double K, float* out, long long Ntot, int D, int R, void* stream) {
    return score_dense_launch<false>("spk_score_dense", U, rec_off, tab_dev, q, g, K, nullptr, out, Ntot, D, R, stream);
}

extern "C" int spk_score_dense_rec(const double* U, const long long* rec_off, const long long* tab_dev, const double* q, const double* g,
                                   const double* K, float* out, long long Ntot, int D, int R, void* stream) {
    return score_dense_launch<true>("spk_score_dense_rec", U, rec_off, tab_dev, q, g, 0.0, K, out, Ntot, D, R, stream);
}

// ---- clustering -------------------------------------------------------------------------------------------------------------------
// The table of summed costs of recording r lies at ws + mat_off[r], n x n doubles.  The rule holds it symmetric; the kernel keeps the
// entry of a pair (a, b), a < b, once, at [a][b], so the lower triangle is free: row n - 1 of it (n - 1 slots) holds the cached
// minimum of every row, val[a] = min over active b > a of C[a][b] / (m_a m_b), next to its column in LDS.  A merge (i, j) changes
// row i, column i and kills j, so the rows to look at again are a < j: row i is scanned afresh, a row whose cached column was i
// or j too, and any other row a < i compares its one new entry at column i with what it holds.  Rows past j keep their minimum.
// Lexicographic order (cost, row, column) everywhere, so the pair found is the one a serial scan with `c < best` finds.
struct AhcCand {
    double c;
    int i;
};

static __device__ __forceinline__ bool ahc_better(double c2, int i2, double c1, int i1) { return c2 < c1 || (c2 == c1 && i2 < i1); }

static __device__ __forceinline__ AhcCand ahc_wave_min(AhcCand v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double c2 = __shfl_xor(v.c, off, 64);
        const int i2 = __shfl_xor(v.i, off, 64);
        if (ahc_better(c2, i2, v.c, v.i)) {
            v.c = c2;
            v.i = i2;
        }
    }
    return v;
}

// the minimum of row a over the active columns b > a (one wave; every lane returns it)
static __device__ __forceinline__ AhcCand ahc_scan_row(const double* __restrict__ C, const unsigned short* msz, int n, int a, int lane) {
    AhcCand v = {__builtin_inf(), 0x7fffffff};
    const double ma = (double)msz[a];
    const double* row = C + (size_t)a * n;
    for (int b = a + 1 + lane; b < n; b += 64) {
        const unsigned mb = msz[b];
        if (mb) {
            const double c = row[b] / (ma * (double)mb);
            if (c < v.c) {                                        // b grows inside a lane: the first of equal costs stays
                v.c = c;
                v.i = b;
            }
        }
    }
    return ahc_wave_min(v);
}

__global__ __launch_bounds__(AHC_THREADS) void ahc_kernel(const float* __restrict__ S, const long long* __restrict__ tab,
                                                          const int* __restrict__ min_clusters, const double* __restrict__ threshold,
                                                          double* __restrict__ ws, int* __restrict__ labels, int* __restrict__ merges,
                                                          double* __restrict__ merge_cost, int* __restrict__ n_merges, int R) {
    __shared__ unsigned short msz[AHC_MAX_N];                     // cluster sizes, 0 = not active
    __shared__ unsigned short col[AHC_MAX_N];                     // the column of the cached row minimum, AHC_NONE = the row has none
    __shared__ unsigned short todo[AHC_MAX_N];                    // rows to scan again after a merge
    __shared__ double red_c[AHC_WAVES];
    __shared__ int red_i[AHC_WAVES];
    __shared__ int ntodo;
    __shared__ int pick_i, pick_j, go;
    __shared__ double pick_c;

    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = tab[r];
    const int n = (int)(tab[r + 1] - row0);
    const long long moff = tab[(R + 1) + r];
    const float* Sr = S + moff;
    double* C = ws + moff;
    double* val = C + (size_t)(n - 1) * n;                        // [n - 1], in the unused lower triangle
    int* lab = labels + row0;
    int target = min_clusters[r];
    target = target > n ? n : target;
    target = target < 1 ? 1 : target;
    const double thr = threshold[r];                              // -inf: none (c <= +inf holds for every cost that can win)

    for (int a = tid; a < n; a += AHC_THREADS) {
        msz[a] = 1;
        lab[a] = a;
    }
    for (int a = 0; a < n - 1; ++a)                               // the upper triangle, rows read along their length
        for (int b = a + 1 + tid; b < n; b += AHC_THREADS) C[(size_t)a * n + b] = -(double)Sr[(size_t)a * n + b];
    __syncthreads();
    for (int a = wave; a < n - 1; a += AHC_WAVES) {
        const AhcCand v = ahc_scan_row(C, msz, n, a, lane);
        if (lane == 0) {
            val[a] = v.c;
            col[a] = v.i == 0x7fffffff ? AHC_NONE : (unsigned short)v.i;
        }
    }
    __syncthreads();

    int nactive = n, steps = 0;
    while (nactive > target) {
        // the smallest cached minimum over the active rows, ties to the smallest row
        AhcCand v = {__builtin_inf(), 0x7fffffff};
        for (int a = tid; a < n - 1; a += AHC_THREADS)
            if (msz[a] && col[a] != AHC_NONE) {
                const double c = val[a];
                if (c < v.c) {
                    v.c = c;
                    v.i = a;
                }
            }
        v = ahc_wave_min(v);
        if (lane == 0) {
            red_c[wave] = v.c;
            red_i[wave] = v.i;
        }
        __syncthreads();
        if (tid == 0) {
            AhcCand b = {red_c[0], red_i[0]};
            for (int w = 1; w < AHC_WAVES; ++w)
                if (ahc_better(red_c[w], red_i[w], b.c, b.i)) {
                    b.c = red_c[w];
                    b.i = red_i[w];
                }
            const bool found = b.i != 0x7fffffff;
            const bool ok = found && (b.c <= -thr);
            go = ok ? 1 : 0;
            if (ok) {
                pick_i = b.i;
                pick_j = col[b.i];
                pick_c = b.c;
                merges[2 * (row0 + steps)] = b.i;
                merges[2 * (row0 + steps) + 1] = col[b.i];
                merge_cost[row0 + steps] = b.c;
            }
            ntodo = 0;
        }
        __syncthreads();
        if (!go) break;                                           // block-uniform
        const int i = pick_i, j = pick_j;
        // C[i][k] += C[j][k] for every other active k; labels of j's members move to i
        for (int k = tid; k < n; k += AHC_THREADS) {
            if (lab[k] == j) lab[k] = i;
            if (k == i || k == j || !msz[k]) continue;
            double* eik = k < i ? C + (size_t)k * n + i : C + (size_t)i * n + k;
            const double* ejk = k < j ? C + (size_t)k * n + j : C + (size_t)j * n + k;
            *eik = *eik + *ejk;
        }
        __syncthreads();
        if (tid == 0) {
            msz[i] = (unsigned short)(msz[i] + msz[j]);
            msz[j] = 0;
        }
        __syncthreads();
        // rows a < j: the cheap update, or onto the list of rows to scan again
        const double mi = (double)msz[i];
        for (int a = tid; a < j && a < n - 1; a += AHC_THREADS) {
            if (!msz[a]) continue;
            const unsigned ca = col[a];
            if (a == i || ca == (unsigned)i || ca == (unsigned)j) {
                todo[atomicAdd(&ntodo, 1)] = (unsigned short)a;  // (an integer counter in LDS: the list's order does not matter)
            } else if (a < i) {
                const double c = C[(size_t)a * n + i] / ((double)msz[a] * mi);
                if (ca == AHC_NONE ? c < __builtin_inf() : (c < val[a] || (c == val[a] && (unsigned)i < ca))) {
                    val[a] = c;
                    col[a] = (unsigned short)i;
                }
            }
        }
        __syncthreads();
        const int nt = ntodo;
        for (int t = wave; t < nt; t += AHC_WAVES) {
            const int a = todo[t];
            const AhcCand w = ahc_scan_row(C, msz, n, a, lane);
            if (lane == 0) {
                val[a] = w.c;
                col[a] = w.i == 0x7fffffff ? AHC_NONE : (unsigned short)w.i;
            }
        }
        --nactive;
        ++steps;
        __syncthreads();
    }
    __syncthreads();
    // labels 1, 2, ... by lowest member: a cluster is named by its lowest member all along, so rank the active rows
    if (tid == 0) {
        int rank = 0;
        for (int a = 0; a < n; ++a) col[a] = msz[a] ? (unsigned short)(++rank) : (unsigned short)0;
        n_merges[r] = steps;
    }
    __syncthreads();
    for (int a = tid; a < n; a += AHC_THREADS) lab[a] = col[lab[a]];
}

extern "C" int spk_ahc_threads(void) { return AHC_THREADS; }
extern "C" int spk_ahc_max_n(void) { return AHC_MAX_N; }

extern "C" int spk_ahc_batch(const float* S, const long long* rec_off, const long long* tab_dev, const int* min_clusters,
                             const double* threshold, double* ws, long long ws_elems, int* labels, int* merges, double* merge_cost,
                             int* n_merges, long long Ntot, int R, void* stream) {
    std::vector<long long> tab;
    if (R >= 1) tab.resize(3 * ((size_t)R + 1));
    const int rc = spk_diar_check("spk_ahc_batch", rec_off, R, Ntot, tab.data());
    if (rc) return rc;
    for (int r = 0; r < R; ++r)
        SPK_REQUIRE(rec_off[r + 1] - rec_off[r] <= AHC_MAX_N, "spk_ahc_batch: recording %d has %lld windows, the cap is %d", r,
                    rec_off[r + 1] - rec_off[r], AHC_MAX_N);
    SPK_REQUIRE(ws_elems >= tab[(R + 1) + R], "spk_ahc_batch: the workspace holds %lld doubles, the batch needs %lld", ws_elems,
                tab[(R + 1) + R]);
    SPK_REQUIRE(S && tab_dev && min_clusters && threshold && ws && labels && merges && merge_cost && n_merges,
                "spk_ahc_batch: null device pointer");
    hipLaunchKernelGGL(ahc_kernel, dim3((unsigned)R), dim3(AHC_THREADS), 0, (hipStream_t)stream, S, tab_dev, min_clusters, threshold, ws,
                       labels, merges, merge_cost, n_merges, R);
    SPK_LAUNCH_CHECK("spk_ahc_batch");
    return 0;
}

// ---- VBx resegmentation --------------------------------------------------------------------------------------
// A variational-Bayes HMM over the window rows of one recording: states are speakers, tr_ij = loopP [i == j] + (1 - loopP) pi_j.  One
// workgroup per recording runs every iteration with __syncthreads() alone; every loop is bounded by max_iters, T, S or D.
// Workspace of recording r, from ws + rec_off[r] (3 + 2 Smax) + r Smax D:  G [T], M [T], C [T], P [T][S], A [T][S], alpha [S][D].
// The forward-backward pass is the scaled form of the contract's O(S) recursion: with M_t = max over the live states of logp_ts and
// p_ts = exp(logp_ts - M_t) (formed by the whole workgroup, so the chain holds no exp and no log),
//   u_ts = p_ts (loopP a_{t-1,s} + (1 - loopP) pi_s)   (u_0s = p_0s pi_s),   c_t = sum_s u_ts,   a_ts = u_ts / c_t
//   x_ts = p_ts b_ts / c_t,   b_{t-1,s} = loopP x_ts + (1 - loopP) sum_j pi_j x_tj   (b_{T-1} = 1)
// so that a_ts = e^{lfw_ts} / sum_i e^{lfw_ti}, gamma_ts = a_ts b_ts, tll = sum_t (M_t + log c_t) and step 7's summand is pi_s x_ts.
// A state is live while pi_s >= 2^-900; below that its prior is taken as 0 (p = 0, gamma = 0: what the contract gives for pi_s = 0).
// With live priors b stays below 1 + loopP / ((1 - loopP) pi_s) <= 2^954, so nothing overflows and 0 * inf cannot arise.
#define VBX_THREADS 256
#define VBX_WAVES (VBX_THREADS / 64)
#define VBX_MAX_S 64            // one lane per state
#define VBX_PF 8                // chain steps whose operands are loaded ahead
#define VBX_PI_FLOOR 0x1p-900
#define VBX_LOG_2PI 1.8378770664093454836

// v of the lane that the DPP control names (a move inside a row of 16 lanes: no LDS crossbar, a few cycles)
template <int CTRL>
static __device__ __forceinline__ double vbx_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// the sum over the lanes 0 .. W - 1 (W a power of two), the same bits in each of them; lanes at or past S hold 0.  Partners at
// distance 1 and 2 by quad permutes, the other half of 8 and of 16 lanes by the two row mirrors, 32 and 64 lanes through the
// crossbar; both partners of a pair add the same two numbers, so every lane ends with the same bits.
static __device__ __forceinline__ double vbx_sum(double v, int W) {
    if (W >= 2) v += vbx_dpp<0xB1>(v);                              // quad_perm [1, 0, 3, 2]
    if (W >= 4) v += vbx_dpp<0x4E>(v);                              // quad_perm [2, 3, 0, 1]
    if (W >= 8) v += vbx_dpp<0x141>(v);                             // row_half_mirror
    if (W >= 16) v += vbx_dpp<0x140>(v);                            // row_mirror
    if (W >= 32) v += __shfl_xor(v, 16, 64);
    if (W >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}

__global__ __launch_bounds__(VBX_THREADS) void vbx_kernel(const double* __restrict__ X, const double* __restrict__ Phi,
                                                          const long long* __restrict__ rec_off, const int* __restrict__ n_states,
                                                          double* __restrict__ gamma, double* __restrict__ pi, double Fa, double Fb,
                                                          double loopP, int max_iters, double epsilon, double* __restrict__ ws,
                                                          double* __restrict__ elbo, int* __restrict__ n_iters, int D, int Smax) {
    __shared__ double sq[DIAR_MAX_D], phi[DIAR_MAX_D];
    __shared__ double npart[VBX_WAVES][VBX_MAX_S];
    __shared__ double cS[VBX_MAX_S], eS[VBX_MAX_S], piS[VBX_MAX_S];
    __shared__ double red[VBX_WAVES];

    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = rec_off[r];
    const int T = (int)(rec_off[r + 1] - row0), S = n_states[r];
    int W = 1;
    while (W < S) W <<= 1;
    const double* Xr = X + (size_t)row0 * D;
    double* gam = gamma + (size_t)row0 * Smax;
    double* G = ws + (size_t)row0 * (3 + 2 * Smax) + (size_t)r * Smax * D;
    double* M = G + T;
    double* C = M + T;
    double* P = C + T;
    double* A = P + (size_t)T * S;
    double* AL = A + (size_t)T * S;
    const double FaFb = Fa / Fb, omlp = 1.0 - loopP;

    for (int d = tid; d < D; d += VBX_THREADS) {
        phi[d] = Phi[d];
        sq[d] = sqrt(Phi[d]);
    }
    if (tid < VBX_MAX_S) {
        const double p0 = tid < S ? pi[(size_t)r * Smax + tid] : 0.0;
        piS[tid] = p0 >= VBX_PI_FLOOR ? p0 : 0.0;
    }
    for (int t = wave; t < T; t += VBX_WAVES) {
        double s = 0.0;
        for (int d = lane; d < D; d += 64) s += Xr[(size_t)t * D + d] * Xr[(size_t)t * D + d];
        s = vbx_sum(s, 64);
        if (lane == 0) G[t] = -0.5 * (s + (double)D * VBX_LOG_2PI);
    }
    __syncthreads();

    double prev = 0.0;
    int done = 0;
    for (int it = 0; it < max_iters; ++it) {
        // 1: N_s, wave w over the windows t = w, w + 4, ...; the four partial sums meet in a fixed order where they are used
        {
            double a = 0.0;
            if (lane < S)
#pragma unroll 8
                for (int t = wave; t < T; t += VBX_WAVES) a += gam[(size_t)t * Smax + lane];
            npart[wave][lane] = a;
        }
        __syncthreads();
        // 2, 3: alpha_sd, one (s, d) per thread, the sum over t in order
        for (int idx = tid; idx < S * D; idx += VBX_THREADS) {
            const int s = idx / D, d = idx - s * D;
            double acc = 0.0;
#pragma unroll 8
            for (int t = 0; t < T; ++t) acc += gam[(size_t)t * Smax + s] * (Xr[(size_t)t * D + d] * sq[d]);
            const double Ns = ((npart[0][s] + npart[1][s]) + npart[2][s]) + npart[3][s];
            const double invL = 1.0 / (1.0 + FaFb * Ns * phi[d]);
            AL[idx] = FaFb * invL * acc;
        }
        __syncthreads();
        // the two sums over d of every state: one wave per state, lane l takes d = l, l + 64, ...
        for (int s = wave; s < S; s += VBX_WAVES) {
            const double Ns = ((npart[0][s] + npart[1][s]) + npart[2][s]) + npart[3][s];
            double c = 0.0, e = 0.0;
            for (int d = lane; d < D; d += 64) {
                const double invL = 1.0 / (1.0 + FaFb * Ns * phi[d]), a = AL[s * D + d];
                c += (invL + a * a) * phi[d];
                e += ((log(invL) - invL) - a * a) + 1.0;
            }
            c = vbx_sum(c, 64);
            e = vbx_sum(e, 64);
            if (lane == 0) {
                cS[s] = -0.5 * c;
                eS[s] = e;
            }
        }
        __syncthreads();
        // 4: logp_ts, one (t, s) per thread
        for (int idx = tid; idx < T * S; idx += VBX_THREADS) {
            const int t = idx / S, s = idx - t * S;
            double dot = 0.0;
#pragma unroll 8
            for (int d = 0; d < D; ++d) dot += (Xr[(size_t)t * D + d] * sq[d]) * AL[s * D + d];
            P[idx] = Fa * ((dot + cS[s]) + G[t]);
        }
        __syncthreads();
        // M_t and p_ts, one window per thread
        for (int t = tid; t < T; t += VBX_THREADS) {
            double m = -__builtin_inf();
            for (int s = 0; s < S; ++s)
                if (piS[s] > 0.0) m = fmax(m, P[(size_t)t * S + s]);
            M[t] = m;
            for (int s = 0; s < S; ++s) P[(size_t)t * S + s] = piS[s] > 0.0 ? exp(P[(size_t)t * S + s] - m) : 0.0;
        }
        __syncthreads();
        // 5, 7: the two chains on one wave, lane s holding state s; the operands of VBX_PF steps are loaded a block ahead
        if (wave == 0) {
            const bool live = lane < S;
            const double pis = piS[lane], q = omlp * pis;
            double ahat = 0.0, buf[VBX_PF];
#pragma unroll
            for (int k = 0; k < VBX_PF; ++k) buf[k] = (live && k < T) ? P[(size_t)k * S + lane] : 0.0;
            for (int t0 = 0; t0 < T; t0 += VBX_PF) {
                double cur[VBX_PF];
#pragma unroll
                for (int k = 0; k < VBX_PF; ++k) {
                    cur[k] = buf[k];
                    const int tn = t0 + VBX_PF + k;
                    buf[k] = (live && tn < T) ? P[(size_t)tn * S + lane] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < VBX_PF; ++k) {
                    const int t = t0 + k;
                    if (t < T) {                                     // wave-uniform
                        const double u = t == 0 ? cur[k] * pis : cur[k] * (loopP * ahat + q);
                        const double c = vbx_sum(u, W);
                        ahat = live ? u / c : 0.0;
                        if (live) A[(size_t)t * S + lane] = ahat;
                        if (lane == 0) C[t] = c;
                    }
                }
            }
            double bhat = 1.0, acc = 0.0, g = ahat;                 // gamma_{T-1} = a_{T-1}
            if (live) gam[(size_t)(T - 1) * Smax + lane] = g;
            // step j = 0, 1, ... handles t = T - 1 - j >= 1: it needs p_t, c_t and a_{t-1}
            double bp[VBX_PF], bc[VBX_PF], ba[VBX_PF];
#pragma unroll
            for (int k = 0; k < VBX_PF; ++k) {
                const int t = T - 1 - k;
                const bool v = t >= 1;
                bp[k] = (live && v) ? P[(size_t)t * S + lane] : 0.0;
                bc[k] = v ? C[t] : 1.0;
                ba[k] = (live && v) ? A[(size_t)(t - 1) * S + lane] : 0.0;
            }
            for (int j0 = 0; j0 < T - 1; j0 += VBX_PF) {
                double cp[VBX_PF], cc[VBX_PF], ca[VBX_PF];
#pragma unroll
                for (int k = 0; k < VBX_PF; ++k) {
                    cp[k] = bp[k];
                    cc[k] = bc[k];
                    ca[k] = ba[k];
                    const int t = T - 1 - (j0 + VBX_PF + k);
                    const bool v = t >= 1;
                    bp[k] = (live && v) ? P[(size_t)t * S + lane] : 0.0;
                    bc[k] = v ? C[t] : 1.0;
                    ba[k] = (live && v) ? A[(size_t)(t - 1) * S + lane] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < VBX_PF; ++k) {
                    const int t = T - 1 - (j0 + k);
                    if (t >= 1) {                                    // wave-uniform
                        const double x = (cp[k] * bhat) / cc[k], y = pis * x;
                        acc += y;
                        bhat = loopP * x + omlp * vbx_sum(y, W);
                        g = ca[k] * bhat;
                        if (live) gam[(size_t)(t - 1) * Smax + lane] = g;
                    }
                }
            }
            double pn = live ? g + omlp * acc : 0.0;                // g = gamma_0 here (T = 1: acc = 0)
            pn = pn / vbx_sum(pn, W);
            piS[lane] = (live && pn >= VBX_PI_FLOOR) ? pn : 0.0;
        }
        __syncthreads();
        // 6, 8: tll = sum_t (M_t + log c_t) and the ELBO, the same bits in every thread
        {
            double s = 0.0;
            for (int t = tid; t < T; t += VBX_THREADS) s += M[t] + log(C[t]);
            s = vbx_sum(s, 64);
            if (lane == 0) red[wave] = s;
        }
        __syncthreads();
        double e = 0.0;
        for (int s = 0; s < S; ++s) e += eS[s];
        const double el = (((red[0] + red[1]) + red[2]) + red[3]) + 0.5 * Fb * e;
        if (tid == 0) elbo[(size_t)r * max_iters + it] = el;
        done = it + 1;
        if (it > 0 && el - prev < epsilon) break;                   // block-uniform
        prev = el;
    }
    // (the last barrier of the loop stands between the last writes of piS and gamma and these reads)
    for (int s = tid; s < Smax; s += VBX_THREADS) pi[(size_t)r * Smax + s] = s < S ? piS[s] : 0.0;
    if (S < Smax)
        for (int idx = tid; idx < T * (Smax - S); idx += VBX_THREADS) {
            const int t = idx / (Smax - S);
            gam[(size_t)t * Smax + S + (idx - t * (Smax - S))] = 0.0;
        }
    if (tid == 0) n_iters[r] = done;
}

extern "C" int spk_vbx_threads(void) { return VBX_THREADS; }
extern "C" int spk_vbx_max_states(void) { return VBX_MAX_S; }

// what both host entry points check: rec_off (as spk_diar_tables does), D, Smax and the length of every recording
static int vbx_shape(const char* who, const long long* rec_off, int R, long long Ntot, int Smax, int D) {
    const int rc = spk_diar_check(who, rec_off, R, Ntot, nullptr);
    if (rc) return rc;
    SPK_REQUIRE(D >= 1 && D <= DIAR_MAX_D, "%s: D=%d must lie in [1, %d]", who, D, DIAR_MAX_D);
    SPK_REQUIRE(Smax >= 1 && Smax <= VBX_MAX_S, "%s: Smax=%d must lie in [1, %d]", who, Smax, VBX_MAX_S);
    for (int r = 0; r < R; ++r)
        SPK_REQUIRE(rec_off[r + 1] - rec_off[r] <= AHC_MAX_N, "%s: recording %d has %lld windows, the cap is %d", who, r,
                    rec_off[r + 1] - rec_off[r], AHC_MAX_N);
    return 0;
}

extern "C" long long spk_vbx_ws_elems(const long long* rec_off, int R, int Smax, int D) {
    SPK_REQUIRE(rec_off && R >= 1, "spk_vbx_ws_elems: bad arguments (R=%d)", R);
    const int rc = vbx_shape("spk_vbx_ws_elems", rec_off, R, rec_off[R], Smax, D);
    if (rc) return rc;
    return rec_off[R] * (3 + 2 * (long long)Smax) + (long long)R * Smax * D;
}

extern "C" int spk_vbx_batch(const double* X, const double* Phi, const long long* rec_off, const long long* rec_off_dev,
                             const int* n_states, const int* n_states_dev, double* gamma, double* pi, double Fa, double Fb,
                             double loopP, int max_iters, double epsilon, double* ws, long long ws_elems, double* elbo, int* n_iters,
                             long long Ntot, int D, int R, int Smax, void* stream) {
    const int rc = vbx_shape("spk_vbx_batch", rec_off, R, Ntot, Smax, D);
    if (rc) return rc;
    SPK_REQUIRE(n_states, "spk_vbx_batch: n_states is missing");
    for (int r = 0; r < R; ++r)
        SPK_REQUIRE(n_states[r] >= 1 && n_states[r] <= Smax, "spk_vbx_batch: n_states[%d]=%d must lie in [1, Smax=%d]", r, n_states[r],
                    Smax);
    SPK_REQUIRE(Fa > 0.0 && Fa < __builtin_inf() && Fb > 0.0 && Fb < __builtin_inf(), "spk_vbx_batch: Fa=%g and Fb=%g must be positive and finite",
                Fa, Fb);
    SPK_REQUIRE(loopP > 0.0 && loopP < 1.0, "spk_vbx_batch: loopP=%g must lie strictly between 0 and 1", loopP);
    SPK_REQUIRE(max_iters >= 1, "spk_vbx_batch: max_iters=%d must be at least 1", max_iters);
    SPK_REQUIRE(epsilon < __builtin_inf(), "spk_vbx_batch: epsilon=%g must be a number below +inf (-inf: never stop early)", epsilon);
    const long long need = Ntot * (3 + 2 * (long long)Smax) + (long long)R * Smax * D;
    SPK_REQUIRE(ws_elems >= need, "spk_vbx_batch: the workspace holds %lld doubles, the batch needs %lld", ws_elems, need);
    SPK_REQUIRE(X && Phi && rec_off_dev && n_states_dev && gamma && pi && ws && elbo && n_iters, "spk_vbx_batch: null device pointer");
    hipLaunchKernelGGL(vbx_kernel, dim3((unsigned)R), dim3(VBX_THREADS), 0, (hipStream_t)stream, X, Phi, rec_off_dev, n_states_dev, gamma,
                       pi, Fa, Fb, loopP, max_iters, epsilon, ws, elbo, n_iters, D, Smax);
    SPK_LAUNCH_CHECK("spk_vbx_batch");
    return 0;
}
