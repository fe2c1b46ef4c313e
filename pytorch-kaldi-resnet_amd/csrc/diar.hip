// Diarization back end on the device: what Kaldi's callhome_diarization recipe runs behind the sliding-window
// extraction - ivector-plda-scoring-dense (without its per-recording PCA) and agglomerative-cluster.
//   spk_diar_tables   - host only: checks rec_off and derives the three offset tables both kernels read
//   spk_score_dense_q - q_i = scale * sum_d k_d U_id^2 per row (one wave per row, fp64, a fixed lane order)
//   spk_score_dense   - S[i][j] = (float)(q_i + q_j + K + sum_d g_d U_id U_jd) for every pair of rows of one recording, all
//                       recordings of a batch in one launch, on v_mfma_f64_16x16x4_f64: one wave per 16 x 16 tile of the upper
//                       triangle, mirrored, so S == S^T bit for bit
//   spk_ahc_batch     - average-linkage agglomerative clustering, one workgroup per recording running its whole merge loop with
//                       __syncthreads() alone: nothing waits on another workgroup
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
static int diar_tables(const char* who, const long long* rec_off, int R, long long Ntot, long long* tab) {
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
    return diar_tables("spk_diar_tables", rec_off, R, Ntot, tab);
}

// ---- q ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dense_q_kernel(const double* __restrict__ U, const double* __restrict__ k, double scale,
                                                      double* __restrict__ q, long long N, int D) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;
    const double* u = U + (size_t)i * D;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) s += k[d] * u[d] * u[d];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) q[i] = scale * s;
}

extern "C" int spk_score_dense_q(const double* U, const double* k, double scale, double* q, long long N, int D, void* stream) {
    SPK_REQUIRE(U && k && q && N >= 1 && N < (1ll << 32) && D >= 1, "spk_score_dense_q: bad arguments");
    hipLaunchKernelGGL(dense_q_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, U, k, scale, q, N, D);
    SPK_LAUNCH_CHECK("spk_score_dense_q");
    return 0;
}

// ---- dense scores -----------------------------------------------------------------------------------------------------------------
// One wave per tile.  The sum over d may run in any order, so step s of lane group gq takes d = d0 + 4 gq + s: a lane reads four
// consecutive values of its row.  D is padded to a multiple of 16 with zeros in registers.  A tile on the diagonal computes
// (g u_i) u_j and (g u_j) u_i, whose roundings differ: only its entries with i <= j are kept, and every entry is stored twice.
__global__ __launch_bounds__(256) void score_dense_kernel(const double* __restrict__ U, const long long* __restrict__ tab,
                                                          const double* __restrict__ q, const double* __restrict__ g, double K,
                                                          float* __restrict__ out, int D, int R, long long ntiles) {
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

extern "C" int spk_score_dense(const double* U, const long long* rec_off, const long long* tab_dev, const double* q, const double* g,
                               double K, float* out, long long Ntot, int D, int R, void* stream) {
    SPK_REQUIRE(D >= 1 && D <= DIAR_MAX_D, "spk_score_dense: D=%d must lie in [1, %d]", D, DIAR_MAX_D);
    std::vector<long long> tab;
    if (R >= 1) tab.resize(3 * ((size_t)R + 1));
    const int rc = diar_tables("spk_score_dense", rec_off, R, Ntot, tab.data());
    if (rc) return rc;
    SPK_REQUIRE(U && tab_dev && q && g && out, "spk_score_dense: null device pointer");
    const long long ntiles = tab[2 * (R + 1) + R];
    hipLaunchKernelGGL(score_dense_kernel, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, U, tab_dev, q, g, K,
                       out, D, R, ntiles);
    SPK_LAUNCH_CHECK("spk_score_dense");
    return 0;
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
    const int rc = diar_tables("spk_ahc_batch", rec_off, R, Ntot, tab.data());
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
