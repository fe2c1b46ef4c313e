// Evaluation stage on the device: what follows the cosine scores (score.hip) in the reference's run_aam_v2.sh:139-181 / test.sh.
//   spk_segment_mean - per-speaker mean of the training embeddings, the S-norm cohort (scripts/compute_speaker_mean.py:15-27)
//   spk_trial_snorm  - adaptive S-norm of every trial score (scripts/adaptive_snorm.py:28-35)
//   spk_sort_trials  - the permutation that sorts the trial scores, ties in index order (Python's stable sorted(...) at
//                      scripts/compute_eer.py:40-42 and local/compute_min_dcf.py:59-61)
//   spk_error_sweep  - miss / false-alarm rates at every threshold, the EER and the minimum detection costs
//                      (ComputeErrorRates, compute_eer.py:101-102, ComputeMinDcf: local/compute_min_dcf.py:54-106)
// Nothing here is approximate: every value is the one the reference's Python expression gives, bit for bit.  So every fp64
// operation is rounded on its own - no contraction to fused multiply-add anywhere in this file:
#pragma clang fp contract(off)
#include "spk_common.h"

#define EVAL_THREADS 256
#define SORT_TILE 4096          // (key, index) pairs one block sorts in LDS: 4096 * 12 bytes = 48 KiB
#define SCAN_ITEMS 4            // consecutive positions per thread of the sweep
#define SCAN_BLOCK (EVAL_THREADS * SCAN_ITEMS)
#define SWEEP_MAX_COSTS 8

extern "C" int spk_eval_tile(int which) { return which == 0 ? SORT_TILE : SCAN_BLOCK; }

// ---- speaker means --------------------------------------------------------------------------------------------------------
// One thread per (speaker, dimension); the rows of a speaker are walked in archive order, because the rounding order IS the
// contract: numpy's `float32_array += float64_vector` adds in fp64 and rounds the sum to fp32 after every utterance, and
// `float32_array /= int` divides in fp32.  Neighbouring threads read neighbouring dimensions of the same row (coalesced).
__global__ __launch_bounds__(EVAL_THREADS) void segment_mean_kernel(const double* __restrict__ emb, const int* __restrict__ rows,
                                                                    const int* __restrict__ seg_off, float* __restrict__ out,
                                                                    int S, int D) {
    const long long i = (long long)blockIdx.x * EVAL_THREADS + threadIdx.x;
    if (i >= (long long)S * D) return;
    const int s = (int)(i / D), d = (int)(i - (long long)s * D);
    const int lo = seg_off[s], hi = seg_off[s + 1];
    float acc = 0.f;
    for (int r = lo; r < hi; ++r) acc = (float)((double)acc + emb[(size_t)rows[r] * D + d]);
    out[i] = acc / (float)(hi - lo);
}

extern "C" int spk_segment_mean(const double* emb, const int* rows, const int* seg_off, float* out, int N, int S, int D,
                                void* stream) {
    SPK_REQUIRE(emb && rows && seg_off && out && N > 0 && S > 0 && S <= N && D > 0, "spk_segment_mean: bad arguments");
    const long long n = (long long)S * D;
    SPK_REQUIRE((n + EVAL_THREADS - 1) / EVAL_THREADS < (1ll << 31), "spk_segment_mean: S * D = %lld is too large", n);
    hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)((n + EVAL_THREADS - 1) / EVAL_THREADS)), dim3(EVAL_THREADS), 0,
                       (hipStream_t)stream, emb, rows, seg_off, out, S, D);
    SPK_LAUNCH_CHECK("spk_segment_mean");
    return 0;
}

// ---- adaptive S-norm ------------------------------------------------------------------------------------------------------
template <typename ST>
__global__ __launch_bounds__(EVAL_THREADS) void trial_snorm_kernel(const ST* __restrict__ score, const int* __restrict__ ia,
                                                                   const int* __restrict__ ib, const double* __restrict__ e_mean,
                                                                   const double* __restrict__ e_std,
                                                                   const double* __restrict__ t_mean,
                                                                   const double* __restrict__ t_std, double* __restrict__ out,
                                                                   int T) {
    const long long t = (long long)blockIdx.x * EVAL_THREADS + threadIdx.x;
    if (t >= T) return;
    const double s = (double)score[t];
    const int a = ia[t], b = ib[t];
    out[t] = (s - e_mean[a]) / fmax(e_std[a], 1e-8) / 2 + (s - t_mean[b]) / fmax(t_std[b], 1e-8) / 2;
}

extern "C" int spk_trial_snorm(const void* score, int score_f64, const int* ia, const int* ib, const double* e_mean,
                               const double* e_std, const double* t_mean, const double* t_std, double* out, int T, void* stream) {
    SPK_REQUIRE(score && ia && ib && e_mean && e_std && t_mean && t_std && out && T > 0, "spk_trial_snorm: bad arguments");
    const dim3 grid((unsigned)(((long long)T + EVAL_THREADS - 1) / EVAL_THREADS));
    if (score_f64)
        hipLaunchKernelGGL(trial_snorm_kernel<double>, grid, dim3(EVAL_THREADS), 0, (hipStream_t)stream, (const double*)score, ia,
                           ib, e_mean, e_std, t_mean, t_std, out, T);
    else
        hipLaunchKernelGGL(trial_snorm_kernel<float>, grid, dim3(EVAL_THREADS), 0, (hipStream_t)stream, (const float*)score, ia, ib,
                           e_mean, e_std, t_mean, t_std, out, T);
    SPK_LAUNCH_CHECK("spk_trial_snorm");
    return 0;
}

// ---- sort -----------------------------------------------------------------------------------------------------------------
// Bitonic network over P = max(SORT_TILE, 2^ceil(log2 T)) composite keys (image of the score, trial index).  The image is the
// usual order-preserving one (sign bit flipped for positive values, all bits for negative ones) with -0.0 keyed as +0.0, as
// Python compares them equal; the index makes every key unique, so the network needs no stability.  Padding is (all ones,
// position >= T): above every real key, +inf included.  Compare-exchange steps whose partner lies inside a tile run in LDS,
// one launch for all of them; the wider ones are one launch each over HBM.
static __device__ __forceinline__ unsigned long long score_image(double s) {
    if (s == 0.0) s = 0.0;                                   // -0.0 -> +0.0
    const unsigned long long u = (unsigned long long)__double_as_longlong(s);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

static __device__ __forceinline__ bool pair_less(unsigned long long ka, unsigned ia, unsigned long long kb, unsigned ib) {
    return ka < kb || (ka == kb && ia < ib);
}

// strides `from` ... 1 of the level `size` on the tile in LDS; `up`: this compare-exchange sorts ascending
static __device__ __forceinline__ void tile_steps(unsigned long long* sk, unsigned* si, unsigned long long gbase,
                                                  unsigned long long size, int from) {
    for (int stride = from; stride > 0; stride >>= 1) {
        for (int i = threadIdx.x; i < SORT_TILE / 2; i += EVAL_THREADS) {
            const int lo = 2 * i - (i & (stride - 1));       // index with the `stride` bit cleared
            const int hi = lo + stride;
            const bool up = ((gbase + lo) & size) == 0;
            const unsigned long long ka = sk[lo], kb = sk[hi];
            const unsigned xa = si[lo], xb = si[hi];
            if (pair_less(kb, xb, ka, xa) == up) {
                sk[lo] = kb; sk[hi] = ka;
                si[lo] = xb; si[hi] = xa;
            }
        }
        __syncthreads();
    }
}

static __device__ __forceinline__ void tile_store(const unsigned long long* sk, const unsigned* si, unsigned long long gbase,
                                                  unsigned long long* key, unsigned* idx, unsigned* order, int T) {
    for (int i = threadIdx.x; i < SORT_TILE; i += EVAL_THREADS) {
        if (order) {                                          // last launch: only the permutation leaves
            if (gbase + i < (unsigned long long)T) order[gbase + i] = si[i];
        } else {
            key[gbase + i] = sk[i];
            idx[gbase + i] = si[i];
        }
    }
}

// keys from the scores, then every level up to SORT_TILE
__global__ __launch_bounds__(EVAL_THREADS) void sort_tile_kernel(const double* __restrict__ score, unsigned long long* key,
                                                                 unsigned* idx, unsigned* order, int T) {
    __shared__ unsigned long long sk[SORT_TILE];
    __shared__ unsigned si[SORT_TILE];
    const unsigned long long gbase = (unsigned long long)blockIdx.x * SORT_TILE;
    for (int i = threadIdx.x; i < SORT_TILE; i += EVAL_THREADS) {
        const unsigned long long g = gbase + i;
        sk[i] = g < (unsigned long long)T ? score_image(score[g]) : ~0ull;
        si[i] = (unsigned)g;
    }
    __syncthreads();
    for (int size = 2; size <= SORT_TILE; size <<= 1) tile_steps(sk, si, gbase, (unsigned long long)size, size >> 1);
    tile_store(sk, si, gbase, key, idx, order, T);
}

// one compare-exchange step of level `size` with stride >= SORT_TILE, over HBM; one thread per pair
__global__ __launch_bounds__(EVAL_THREADS) void sort_global_kernel(unsigned long long* key, unsigned* idx, unsigned long long size,
                                                                   unsigned long long stride, unsigned long long npairs) {
    const unsigned long long i = (unsigned long long)blockIdx.x * EVAL_THREADS + threadIdx.x;
    if (i >= npairs) return;
    const unsigned long long lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
    const bool up = (lo & size) == 0;
    const unsigned long long ka = key[lo], kb = key[hi];
    const unsigned xa = idx[lo], xb = idx[hi];
    if (pair_less(kb, xb, ka, xa) == up) {
        key[lo] = kb; key[hi] = ka;
        idx[lo] = xb; idx[hi] = xa;
    }
}

// the strides SORT_TILE / 2 ... 1 of level `size` (> SORT_TILE)
__global__ __launch_bounds__(EVAL_THREADS) void sort_merge_kernel(unsigned long long* key, unsigned* idx, unsigned* order,
                                                                  unsigned long long size, int T) {
    __shared__ unsigned long long sk[SORT_TILE];
    __shared__ unsigned si[SORT_TILE];
    const unsigned long long gbase = (unsigned long long)blockIdx.x * SORT_TILE;
    for (int i = threadIdx.x; i < SORT_TILE; i += EVAL_THREADS) {
        sk[i] = key[gbase + i];
        si[i] = idx[gbase + i];
    }
    __syncthreads();
    tile_steps(sk, si, gbase, size, SORT_TILE / 2);
    tile_store(sk, si, gbase, key, idx, order, T);
}

static unsigned long long sort_padded(int T) {
    unsigned long long P = SORT_TILE;
    while (P < (unsigned long long)T) P <<= 1;
    return P;
}

extern "C" size_t spk_sort_trials_workspace(int T) { return T < 1 ? 0 : (size_t)sort_padded(T) * 12; }

extern "C" int spk_sort_trials(const double* score, unsigned* order, void* ws, int T, void* stream) {
    SPK_REQUIRE(score && order && ws, "spk_sort_trials: bad arguments");
    SPK_REQUIRE(T >= 1, "spk_sort_trials: T=%d must lie in [1, 2^31)", T);     // (an int is below 2^31)
    const unsigned long long P = sort_padded(T);
    unsigned long long* key = (unsigned long long*)ws;
    unsigned* idx = (unsigned*)(key + P);
    const unsigned tiles = (unsigned)(P / SORT_TILE);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sort_tile_kernel, dim3(tiles), dim3(EVAL_THREADS), 0, st, score, key, idx, P == SORT_TILE ? order : nullptr, T);
    for (unsigned long long size = 2ull * SORT_TILE; size <= P; size <<= 1) {
        for (unsigned long long stride = size >> 1; stride >= SORT_TILE; stride >>= 1)
            hipLaunchKernelGGL(sort_global_kernel, dim3((unsigned)(P / 2 / EVAL_THREADS)), dim3(EVAL_THREADS), 0, st, key, idx, size,
                               stride, P / 2);
        hipLaunchKernelGGL(sort_merge_kernel, dim3(tiles), dim3(EVAL_THREADS), 0, st, key, idx, size == P ? order : nullptr, size, T);
    }
    SPK_LAUNCH_CHECK("spk_sort_trials");
    return 0;
}

// ---- error-rate sweep -----------------------------------------------------------------------------------------------------
// Position i of the sorted list is the threshold "reject everything up to and including i".  With ct / cn the inclusive counts
// of targets / non-targets up to i (exact integers: a multi-block scan in 64 bits),
//   fnr = ct / (double)n_tar,  fpr = 1 - cn / (double)n_non,  c = c_miss * fnr * p + c_fa * fpr * (1 - p)   (left to right)
// and the answers are argmins with the lowest position winning ties (np.nanargmin; the strict `<` of ComputeMinDcf).
// Three passes: targets per block; their exclusive scan (one block); rates and per-block argmins; then one block picks the
// winners and writes the report.  Metric 0 is |fnr - fpr|, metric 1 + k the cost of triple k.
struct Best {
    double val;
    long long pos, ct;
};

static __device__ __forceinline__ bool best_before(const Best& b, const Best& a) {     // b replaces a
    return b.val < a.val || (b.val == a.val && b.pos < a.pos);                           // (a NaN never wins: nanargmin)
}

static __device__ __forceinline__ Best block_best(Best v, Best* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = EVAL_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off && best_before(sh[threadIdx.x + off], sh[threadIdx.x])) sh[threadIdx.x] = sh[threadIdx.x + off];
        __syncthreads();
    }
    const Best r = sh[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(EVAL_THREADS) void sweep_count_kernel(const unsigned char* __restrict__ label,
                                                                   const unsigned* __restrict__ order,
                                                                   long long* __restrict__ block_tar, int T) {
    __shared__ int sh[EVAL_THREADS];
    const long long base = (long long)blockIdx.x * SCAN_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
    int n = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < T) n += label[order[base + k]] != 0;
    sh[threadIdx.x] = n;
    __syncthreads();
    for (int off = EVAL_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_tar[blockIdx.x] = sh[0];
}

// in place: block_tar[b] -> targets before block b; block_tar[nb] = all targets
__global__ __launch_bounds__(EVAL_THREADS) void sweep_offsets_kernel(long long* block_tar, int nb) {
    __shared__ long long sh[EVAL_THREADS];
    long long carry = 0;
    for (int lo = 0; lo < nb; lo += EVAL_THREADS) {
        const int b = lo + threadIdx.x;
        const long long mine = b < nb ? block_tar[b] : 0;
        sh[threadIdx.x] = mine;
        __syncthreads();
        for (int off = 1; off < EVAL_THREADS; off <<= 1) {
            const long long add = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (b < nb) block_tar[b] = carry + sh[threadIdx.x] - mine;
        carry += sh[EVAL_THREADS - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_tar[nb] = carry;
}

__global__ __launch_bounds__(EVAL_THREADS) void sweep_rates_kernel(const unsigned char* __restrict__ label,
                                                                   const unsigned* __restrict__ order,
                                                                   const long long* __restrict__ block_tar,
                                                                   const double* __restrict__ costs, int P,
                                                                   Best* __restrict__ partial, int T, int nb) {
    __shared__ int sh[EVAL_THREADS];
    __shared__ Best shb[EVAL_THREADS];
    const long long base = (long long)blockIdx.x * SCAN_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
    int lab[SCAN_ITEMS], n = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        lab[k] = base + k < T ? (label[order[base + k]] != 0) : 0;
        n += lab[k];
    }
    sh[threadIdx.x] = n;
    __syncthreads();
    for (int off = 1; off < EVAL_THREADS; off <<= 1) {
        const int add = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    const long long n_tar = block_tar[nb], n_non = (long long)T - n_tar;
    const double d_tar = (double)n_tar, d_non = (double)n_non;
    long long ct = block_tar[blockIdx.x] + sh[threadIdx.x] - n;      // targets before this thread's first position
    Best best[1 + SWEEP_MAX_COSTS];
#pragma unroll
    for (int m = 0; m < 1 + SWEEP_MAX_COSTS; ++m) best[m] = Best{__builtin_inf(), 0x7fffffffffffffffll, 0};
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const long long pos = base + k;
        if (pos >= T) break;
        ct += lab[k];
        const long long cn = pos + 1 - ct;
        const double fnr = (double)ct / d_tar;
        const double fpr = 1.0 - (double)cn / d_non;
        const double gap = fabs(fnr - fpr);
        if (gap < best[0].val) best[0] = Best{gap, pos, ct};
#pragma unroll
        for (int m = 0; m < SWEEP_MAX_COSTS; ++m) {
            if (m < P) {
                const double p = costs[3 * m], c_miss = costs[3 * m + 1], c_fa = costs[3 * m + 2];
                const double c = c_miss * fnr * p + c_fa * fpr * (1.0 - p);
                if (c < best[1 + m].val) best[1 + m] = Best{c, pos, ct};
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 1 + SWEEP_MAX_COSTS; ++m) {
        if (m <= P) {
            const Best r = block_best(best[m], shb);
            if (threadIdx.x == 0) partial[(size_t)m * nb + blockIdx.x] = r;
        }
    }
}

// out_d: eer, then (minDCF, threshold) per triple; out_i: eer position, n_tar, n_non, then the position per triple
__global__ __launch_bounds__(EVAL_THREADS) void sweep_final_kernel(const double* __restrict__ score,
                                                                   const unsigned* __restrict__ order,
                                                                   const long long* __restrict__ block_tar,
                                                                   const double* __restrict__ costs, int P,
                                                                   const Best* __restrict__ partial, double* __restrict__ out_d,
                                                                   long long* __restrict__ out_i, int T, int nb) {
    __shared__ Best shb[EVAL_THREADS];
    const long long n_tar = block_tar[nb], n_non = (long long)T - n_tar;
    for (int m = 0; m <= P; ++m) {
        Best v = Best{__builtin_inf(), 0x7fffffffffffffffll, 0};
        for (int b = threadIdx.x; b < nb; b += EVAL_THREADS) {
            const Best o = partial[(size_t)m * nb + b];
            if (best_before(o, v)) v = o;
        }
        const Best r = block_best(v, shb);
        if (threadIdx.x != 0) continue;
        const long long pos = r.pos < T ? r.pos : 0;          // (nothing comparable: every rate is NaN; the host rejects that)
        if (m == 0) {
            const double fnr = (double)r.ct / (double)n_tar;
            const double fpr = 1.0 - (double)(pos + 1 - r.ct) / (double)n_non;
            out_d[0] = fmax(fpr, fnr);
            out_i[0] = pos;
            out_i[1] = n_tar;
            out_i[2] = n_non;
        } else {
            const double p = costs[3 * (m - 1)], c_miss = costs[3 * (m - 1) + 1], c_fa = costs[3 * (m - 1) + 2];
            out_d[2 * m - 1] = r.val / fmin(c_miss * p, c_fa * (1.0 - p));
            out_d[2 * m] = score[order[pos]];
            out_i[2 + m] = pos;
        }
    }
}

static int sweep_blocks(int T) { return (int)(((long long)T + SCAN_BLOCK - 1) / SCAN_BLOCK); }

extern "C" size_t spk_error_sweep_workspace(int T, int P) {
    if (T < 1 || P < 0 || P > SWEEP_MAX_COSTS) return 0;
    const size_t nb = (size_t)sweep_blocks(T);
    return (nb + 1) * sizeof(long long) + (size_t)(1 + P) * nb * sizeof(Best);
}

extern "C" int spk_error_sweep(const double* score, const unsigned char* label, const unsigned* order, const double* costs, int P,
                               double* out_d, long long* out_i, void* ws, int T, void* stream) {
    SPK_REQUIRE(score && label && order && out_d && out_i && ws && T >= 1, "spk_error_sweep: bad arguments");
    SPK_REQUIRE(P >= 0 && P <= SWEEP_MAX_COSTS && (P == 0 || costs), "spk_error_sweep: P=%d cost triples, at most %d", P,
                SWEEP_MAX_COSTS);
    const int nb = sweep_blocks(T);
    long long* block_tar = (long long*)ws;
    Best* partial = (Best*)(block_tar + nb + 1);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sweep_count_kernel, dim3(nb), dim3(EVAL_THREADS), 0, st, label, order, block_tar, T);
    hipLaunchKernelGGL(sweep_offsets_kernel, dim3(1), dim3(EVAL_THREADS), 0, st, block_tar, nb);
    hipLaunchKernelGGL(sweep_rates_kernel, dim3(nb), dim3(EVAL_THREADS), 0, st, label, order, block_tar, costs, P, partial, T, nb);
    hipLaunchKernelGGL(sweep_final_kernel, dim3(1), dim3(EVAL_THREADS), 0, st, score, order, block_tar, costs, P, partial, out_d,
                       out_i, T, nb);
    SPK_LAUNCH_CHECK("spk_error_sweep");
    return 0;
}
