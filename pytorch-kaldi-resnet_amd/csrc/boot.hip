// Speaker-level bootstrap of the error-rate sweep on the device (include/spkboot.h): R weighted replicates of
// the sweep of eval.hip over one sorted trial list.
//   spkb_pack  - once per system: one 8-byte record (both unit ids, label) per sorted position, and the number of scores below each
//                Bayes threshold
//   spkb_sweep - a chunk of replicates: weighted target / non-target sums per (replicate, tile); their exclusive scan over the tiles;
//                rates, per-tile argmins and the counts at the actDCF positions; one workgroup per replicate writes the report
// A replicate is a row of counts c[U]; trial (a, b) weighs c[a] c[b], or c[a] when a = b.  Every count is an exact int64, every rate
// the host's double: true fp64 divisions, every operation rounded on its own, no atomics - the same bits wherever a replicate sits.
#pragma clang fp contract(off)
#include "spk_common.h"

#define BOOT_THREADS 256
#define BOOT_WAVES (BOOT_THREADS / 64)
#define BOOT_ITEMS 4                               // consecutive positions per thread
#define BOOT_TILE (BOOT_THREADS * BOOT_ITEMS)      // positions per workgroup
#define BOOT_MAX_COSTS 8
#define BOOT_MAX_G 16                              // replicates per workgroup at most
#define BOOT_ROWS_BYTES 65536                      // LDS for the count rows of a group of more than one replicate: two workgroups per CU
#define BOOT_MAX_U 65535
#define BOOT_MAX_COUNT 65535

extern "C" int spkb_limit(int which) {
    return which == 0 ? BOOT_TILE : which == 1 ? BOOT_MAX_U : which == 2 ? BOOT_MAX_COUNT : which == 3 ? BOOT_MAX_COSTS
         : which == 4 ? BOOT_MAX_G : which == 5 ? BOOT_THREADS : -1;
}
// entries per row of the device count table: rows start on 16 bytes
extern "C" int spkb_pitch(int U) { return U < 1 || U > BOOT_MAX_U ? -1 : (U + 7) & ~7; }
// replicates per workgroup: as many rows as fit BOOT_ROWS_BYTES, at least one (a row of 65 535 units takes 128 KiB), at most BOOT_MAX_G
extern "C" int spkb_group(int U) {
    if (U < 1 || U > BOOT_MAX_U) return -1;
    const int g = BOOT_ROWS_BYTES / (2 * spkb_pitch(U));
    return g < 1 ? 1 : g > BOOT_MAX_G ? BOOT_MAX_G : g;
}

static int boot_tiles(int T) { return (int)(((long long)T + BOOT_TILE - 1) / BOOT_TILE); }

struct BootCosts {
    double p[BOOT_MAX_COSTS], c_miss[BOOT_MAX_COSTS], c_fa[BOOT_MAX_COSTS];
};
struct BootEta {
    double v[BOOT_MAX_COSTS];
};
struct BootBest {
    double val;
    long long pos, ct, cn;
};
#define BOOT_NO_POS 0x7fffffffffffffffll

// ---- records ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BOOT_THREADS) void boot_pack_kernel(const unsigned char* __restrict__ label, const unsigned* __restrict__ order,
                                                                 const int* __restrict__ ua, const int* __restrict__ ub,
                                                                 uint2* __restrict__ rec, int T, int U) {
    const long long i = (long long)blockIdx.x * BOOT_THREADS + threadIdx.x;
    if (i >= T) return;
    const unsigned o = order[i];
    const unsigned a = min((unsigned)ua[o], (unsigned)(U - 1)), b = min((unsigned)ub[o], (unsigned)(U - 1));   // (the host checked the range)
    rec[i] = make_uint2(a | (b << 16), label[o] != 0);
}

// q[m] = the number of sorted scores below eta[m]: one thread per threshold bisects the sorted list
__global__ void boot_below_kernel(const double* __restrict__ score, const unsigned* __restrict__ order, BootEta eta, int P,
                                  long long* __restrict__ q, int T) {
    const int m = threadIdx.x;
    if (m >= P) return;
    long long lo = 0, hi = T;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (score[order[mid]] < eta.v[m]) lo = mid + 1;
        else hi = mid;
    }
    q[m] = lo;
}

extern "C" int spkb_pack(const double* score, const unsigned char* label, const unsigned* order, const int* ua, const int* ub,
                         const double* eta, int P, void* rec, long long* q, int T, int U, void* stream) {
    SPK_REQUIRE(score && label && order && ua && ub && rec, "spkb_pack: null pointer");
    SPK_REQUIRE(T >= 2, "spkb_pack: T=%d must lie in [2, 2^31)", T);
    SPK_REQUIRE(U >= 1 && U <= BOOT_MAX_U, "spkb_pack: U=%d units, must lie in [1, %d]", U, BOOT_MAX_U);
    SPK_REQUIRE(P >= 0 && P <= BOOT_MAX_COSTS && (P == 0 || (eta && q)), "spkb_pack: P=%d thresholds, at most %d", P, BOOT_MAX_COSTS);
    BootEta e;
    for (int m = 0; m < BOOT_MAX_COSTS; ++m) e.v[m] = m < P ? eta[m] : 0.0;
    for (int m = 0; m < P; ++m) SPK_REQUIRE(e.v[m] == e.v[m], "spkb_pack: threshold %d is NaN", m);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(boot_pack_kernel, dim3((unsigned)(((long long)T + BOOT_THREADS - 1) / BOOT_THREADS)), dim3(BOOT_THREADS), 0, st,
                       label, order, ua, ub, (uint2*)rec, T, U);
    if (P) hipLaunchKernelGGL(boot_below_kernel, dim3(1), dim3(64), 0, st, score, order, e, P, q, T);
    SPK_LAUNCH_CHECK("spkb_pack");
    return 0;
}

// ---- the sweep ------------------------------------------------------------------------------------------------------------------------
// the count rows of this workgroup's replicates, global -> LDS, 16 bytes at a time (the rows are consecutive and pitched to 16 bytes)
static __device__ __forceinline__ void boot_stage(const unsigned short* __restrict__ counts, int pitch, int rows, unsigned short* lds) {
    const uint4* src = (const uint4*)counts;
    uint4* dst = (uint4*)lds;
    const int n = rows * (pitch >> 3);
    for (int i = threadIdx.x; i < n; i += BOOT_THREADS) dst[i] = src[i];
    __syncthreads();
}

static __device__ __forceinline__ unsigned boot_weight(const unsigned short* row, unsigned ab) {
    const unsigned a = ab & 0xffffu, b = ab >> 16;
    const unsigned ca = row[a], cb = row[b];
    return a == b ? ca : ca * cb;                       // (65 535^2 < 2^32)
}

// this thread's records: `ok` positions lie inside the list
static __device__ __forceinline__ void boot_load(const uint2* __restrict__ rec, long long base, int T, unsigned* ab, bool* tar, bool* ok) {
#pragma unroll
    for (int k = 0; k < BOOT_ITEMS; ++k) {
        ok[k] = base + k < T;
        const uint2 r = ok[k] ? rec[base + k] : make_uint2(0u, 0u);
        ab[k] = r.x;
        tar[k] = r.y != 0;
    }
}

static __device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// tile_sum [Rc][2][nb + 1]: weighted targets / non-targets of (replicate, tile)
__global__ __launch_bounds__(BOOT_THREADS) void boot_count_kernel(const uint2* __restrict__ rec, const unsigned short* __restrict__ counts,
                                                                  int pitch, int G, int Rc, long long* __restrict__ tile_sum, int T,
                                                                  int nb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char boot_lds[];
    __shared__ long long shw[BOOT_MAX_G][BOOT_WAVES][2];
    unsigned short* rows = (unsigned short*)boot_lds;
    const int r0 = blockIdx.y * G, ng = min(G, Rc - r0);
    boot_stage(counts + (size_t)r0 * pitch, pitch, ng, rows);
    unsigned ab[BOOT_ITEMS];
    bool tar[BOOT_ITEMS], ok[BOOT_ITEMS];
    boot_load(rec, (long long)blockIdx.x * BOOT_TILE + (long long)threadIdx.x * BOOT_ITEMS, T, ab, tar, ok);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int g = 0; g < ng; ++g) {
        const unsigned short* row = rows + (size_t)g * pitch;
        long long t = 0, n = 0;
#pragma unroll
        for (int k = 0; k < BOOT_ITEMS; ++k) {
            const long long w = ok[k] ? (long long)boot_weight(row, ab[k]) : 0;
            t += tar[k] ? w : 0;
            n += tar[k] ? 0 : w;
        }
        t = wave_sum(t);
        n = wave_sum(n);
        if (lane == 0) {
            shw[g][wave][0] = t;
            shw[g][wave][1] = n;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * ng) {
        const int g = threadIdx.x >> 1, v = threadIdx.x & 1;
        long long s = 0;
        for (int w = 0; w < BOOT_WAVES; ++w) s += shw[g][w][v];
        tile_sum[((size_t)(r0 + g) * 2 + v) * (nb + 1) + blockIdx.x] = s;
    }
}

// in place, one workgroup per replicate: tile_sum[r][v][b] -> the sum before tile b; [nb] = the total
__global__ __launch_bounds__(BOOT_THREADS) void boot_offsets_kernel(long long* tile_sum, int nb) {
    __shared__ long long sh[BOOT_THREADS];
    for (int v = 0; v < 2; ++v) {
        long long* col = tile_sum + ((size_t)blockIdx.x * 2 + v) * (nb + 1);
        long long carry = 0;
        for (int lo = 0; lo < nb; lo += BOOT_THREADS) {
            const int b = lo + threadIdx.x;
            const long long mine = b < nb ? col[b] : 0;
            sh[threadIdx.x] = mine;
            __syncthreads();
            for (int off = 1; off < BOOT_THREADS; off <<= 1) {
                const long long add = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
                __syncthreads();
                sh[threadIdx.x] += add;
                __syncthreads();
            }
            if (b < nb) col[b] = carry + sh[threadIdx.x] - mine;
            carry += sh[BOOT_THREADS - 1];
            __syncthreads();
        }
        if (threadIdx.x == 0) col[nb] = carry;
    }
}

static __device__ __forceinline__ bool boot_before(double bv, long long bp, double av, long long ap) {     // b replaces a
    return bv < av || (bv == av && bp < ap);
}

// partial [Rc][1 + P][nb]: the best of metric m (0: |fnr - fpr|, 1 + k: the cost of triple k) inside the tile; act [Rc][Pa][2]: ct, cn
// at position q - 1.  A replicate without targets or without non-targets is skipped: the last kernel flags it.
__global__ __launch_bounds__(BOOT_THREADS) void boot_rates_kernel(const uint2* __restrict__ rec, const unsigned short* __restrict__ counts,
                                                                  int pitch, int G, int Rc, const long long* __restrict__ tile_sum,
                                                                  BootCosts cs, int P, const long long* __restrict__ q, int Pa,
                                                                  BootBest* __restrict__ partial, long long* __restrict__ act, int T,
                                                                  int nb) {
    extern __shared__ __attribute__((aligned(16))) unsigned char boot_lds[];
    __shared__ long long shw[BOOT_WAVES][2];
    __shared__ BootBest shb[1 + BOOT_MAX_COSTS][BOOT_WAVES];
    __shared__ double shc[4][BOOT_MAX_COSTS];                     // p, c_miss, c_fa, 1 - p of every triple
    if (threadIdx.x < BOOT_MAX_COSTS) {
        shc[0][threadIdx.x] = cs.p[threadIdx.x];
        shc[1][threadIdx.x] = cs.c_miss[threadIdx.x];
        shc[2][threadIdx.x] = cs.c_fa[threadIdx.x];
        shc[3][threadIdx.x] = 1.0 - cs.p[threadIdx.x];
    }
    unsigned short* rows = (unsigned short*)boot_lds;
    const int r0 = blockIdx.y * G, ng = min(G, Rc - r0);
    boot_stage(counts + (size_t)r0 * pitch, pitch, ng, rows);
    const long long base = (long long)blockIdx.x * BOOT_TILE + (long long)threadIdx.x * BOOT_ITEMS;
    unsigned ab[BOOT_ITEMS];
    bool tar[BOOT_ITEMS], ok[BOOT_ITEMS];
    boot_load(rec, base, T, ab, tar, ok);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int g = 0; g < ng; ++g) {
        const int r = r0 + g;
        const long long* sum_t = tile_sum + ((size_t)r * 2 + 0) * (nb + 1);
        const long long* sum_n = tile_sum + ((size_t)r * 2 + 1) * (nb + 1);
        const long long n_tar = sum_t[nb], n_non = sum_n[nb];
        if (n_tar == 0 || n_non == 0) continue;                  // (the same for every thread of the workgroup)
        const unsigned short* row = rows + (size_t)g * pitch;
        long long w[BOOT_ITEMS], t = 0, n = 0;
#pragma unroll
        for (int k = 0; k < BOOT_ITEMS; ++k) {
            w[k] = ok[k] ? (long long)boot_weight(row, ab[k]) : 0;
            t += tar[k] ? w[k] : 0;
            n += tar[k] ? 0 : w[k];
        }
        // inclusive scan inside the wave, then the waves before this one
        long long it = t, in = n;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long a = __shfl_up(it, off, 64), b = __shfl_up(in, off, 64);
            if (lane >= off) {
                it += a;
                in += b;
            }
        }
        if (lane == 63) {
            shw[wave][0] = it;
            shw[wave][1] = in;
        }
        __syncthreads();
        long long ct = sum_t[blockIdx.x] + it - t, cn = sum_n[blockIdx.x] + in - n;      // before this thread's first position
        for (int v = 0; v < wave; ++v) {
            ct += shw[v][0];
            cn += shw[v][1];
        }
        const double d_tar = (double)n_tar, d_non = (double)n_non;
        double bval[1 + BOOT_MAX_COSTS];                          // metric m: value and position; the counts only for metric 0,
        long long bpos[1 + BOOT_MAX_COSTS], bct = 0, bcn = 0;     // whose rates the last kernel recomputes
#pragma unroll
        for (int m = 0; m < 1 + BOOT_MAX_COSTS; ++m) {
            bval[m] = __builtin_inf();
            bpos[m] = BOOT_NO_POS;
        }
#pragma unroll
        for (int k = 0; k < BOOT_ITEMS; ++k) {
            const long long pos = base + k;
            if (ok[k]) {
                ct += tar[k] ? w[k] : 0;
                cn += tar[k] ? 0 : w[k];
                const double fnr = (double)ct / d_tar;
                const double fpr = 1.0 - (double)cn / d_non;
                const double gap = fabs(fnr - fpr);
                if (gap < bval[0]) {
                    bval[0] = gap;
                    bpos[0] = pos;
                    bct = ct;
                    bcn = cn;
                }
#pragma unroll
                for (int m = 0; m < BOOT_MAX_COSTS; ++m) {
                    if (m < P) {
                        const double c = shc[1][m] * fnr * shc[0][m] + shc[2][m] * fpr * shc[3][m];
                        if (c < bval[1 + m]) {
                            bval[1 + m] = c;
                            bpos[1 + m] = pos;
                        }
                    }
                    if (m < Pa && pos == q[m] - 1) {
                        act[((size_t)r * Pa + m) * 2 + 0] = ct;
                        act[((size_t)r * Pa + m) * 2 + 1] = cn;
                    }
                }
            }
        }
        // the wave's winner of every metric: (value, position) through the lanes, then the lane that holds it hands it over
#pragma unroll
        for (int m = 0; m < 1 + BOOT_MAX_COSTS; ++m) {
            if (m <= P) {
                double bv = bval[m];
                long long bp = bpos[m];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const double ov = __shfl_xor(bv, off, 64);
                    const long long op = __shfl_xor(bp, off, 64);
                    if (boot_before(ov, op, bv, bp)) {
                        bv = ov;
                        bp = op;
                    }
                }
                if (bp == BOOT_NO_POS ? lane == 0 : bpos[m] == bp) shb[m][wave] = BootBest{bv, bp, m == 0 ? bct : 0, m == 0 ? bcn : 0};
            }
        }
        __syncthreads();
        if ((int)threadIdx.x <= P) {
            int win = 0;
            double bv = shb[threadIdx.x][0].val;
            long long bp = shb[threadIdx.x][0].pos;
#pragma unroll
            for (int v = 1; v < BOOT_WAVES; ++v) {
                const double ov = shb[threadIdx.x][v].val;
                const long long op = shb[threadIdx.x][v].pos;
                if (boot_before(ov, op, bv, bp)) {
                    bv = ov;
                    bp = op;
                    win = v;
                }
            }
            BootBest* dst = partial + ((size_t)r * (1 + P) + threadIdx.x) * nb + blockIdx.x;
            dst->val = bv;
            dst->pos = bp;
            dst->ct = shb[threadIdx.x][win].ct;
            dst->cn = shb[threadIdx.x][win].cn;
        }
        // (the next replicate writes shw after every thread has read it, and shb only behind its own barrier)
    }
}

static __device__ __forceinline__ BootBest boot_block_best(BootBest v, BootBest* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = BOOT_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const BootBest o = sh[threadIdx.x + off], a = sh[threadIdx.x];
            if (boot_before(o.val, o.pos, a.val, a.pos)) sh[threadIdx.x] = o;
        }
        __syncthreads();
    }
    const BootBest r = sh[0];
    __syncthreads();
    return r;
}

// one workgroup per replicate.  out_d [Rc][1 + P + Pa] = eer, minDCF [P], actDCF [Pa]; out_i [Rc][4 + P + 2 Pa] = flag, n_tar, n_non,
// eer position, position [P], miss [Pa], fa [Pa].  A flagged replicate has NaN for every double and -1 for every position and count
// behind n_non.
__global__ __launch_bounds__(BOOT_THREADS) void boot_final_kernel(const long long* __restrict__ tile_sum, BootCosts cs, int P, BootCosts as,
                                                                  const long long* __restrict__ q, int Pa,
                                                                  const BootBest* __restrict__ partial, const long long* __restrict__ act,
                                                                  double* __restrict__ out_d, long long* __restrict__ out_i, int T, int nb) {
    __shared__ BootBest shb[BOOT_THREADS];
    const int r = blockIdx.x;
    const long long n_tar = tile_sum[((size_t)r * 2 + 0) * (nb + 1) + nb], n_non = tile_sum[((size_t)r * 2 + 1) * (nb + 1) + nb];
    double* od = out_d + (size_t)r * (1 + P + Pa);
    long long* oi = out_i + (size_t)r * (4 + P + 2 * Pa);
    if (n_tar == 0 || n_non == 0) {
        if (threadIdx.x == 0) {
            oi[0] = 1;
            oi[1] = n_tar;
            oi[2] = n_non;
            for (int k = 3; k < 4 + P + 2 * Pa; ++k) oi[k] = -1;
            for (int k = 0; k < 1 + P + Pa; ++k) od[k] = __longlong_as_double(0x7ff8000000000000ll);
        }
        return;
    }
    const double d_tar = (double)n_tar, d_non = (double)n_non;
    for (int m = 0; m <= P; ++m) {
        BootBest v = BootBest{__builtin_inf(), BOOT_NO_POS, 0, 0};
        for (int b = threadIdx.x; b < nb; b += BOOT_THREADS) {
            const BootBest o = partial[((size_t)r * (1 + P) + m) * nb + b];
            if (boot_before(o.val, o.pos, v.val, v.pos)) v = o;
        }
        const BootBest w = boot_block_best(v, shb);
        if (threadIdx.x != 0) continue;
        if (m == 0) {
            const double fnr = (double)w.ct / d_tar;
            const double fpr = 1.0 - (double)w.cn / d_non;
            od[0] = fmax(fpr, fnr);
            oi[0] = 0;
            oi[1] = n_tar;
            oi[2] = n_non;
            oi[3] = w.pos;
        } else {
            od[m] = w.val / fmin(cs.c_miss[m - 1] * cs.p[m - 1], cs.c_fa[m - 1] * (1.0 - cs.p[m - 1]));
            oi[3 + m] = w.pos;
        }
    }
    if ((int)threadIdx.x < Pa) {
        const int m = threadIdx.x;
        const bool none = q[m] == 0;
        const long long miss = none ? 0 : act[((size_t)r * Pa + m) * 2 + 0];
        const long long fa = n_non - (none ? 0 : act[((size_t)r * Pa + m) * 2 + 1]);
        const double fnr = (double)miss / d_tar, fpr = (double)fa / d_non;
        od[1 + P + m] = (as.c_miss[m] * fnr * as.p[m] + as.c_fa[m] * fpr * (1.0 - as.p[m])) / fmin(as.c_miss[m] * as.p[m], as.c_fa[m] * (1.0 - as.p[m]));
        oi[4 + P + m] = miss;
        oi[4 + P + Pa + m] = fa;
    }
}

// 8-byte words of workspace for a chunk of Rc replicates: tile sums, per-tile bests (4 words each), counts at the actDCF positions
extern "C" long long spkb_sweep_ws_elems(int T, int P, int Pa, int Rc) {
    if (T < 2 || P < 0 || P > BOOT_MAX_COSTS || Pa < 0 || Pa > BOOT_MAX_COSTS || Rc < 1) return -1;
    const long long nb = boot_tiles(T);
    return (long long)Rc * (2 * (nb + 1) + 4 * (1 + P) * nb + 2 * Pa);
}

static bool boot_fill(BootCosts& cs, const double* costs, int P) {
    for (int m = 0; m < BOOT_MAX_COSTS; ++m) {
        cs.p[m] = m < P ? costs[3 * m] : 0.0;
        cs.c_miss[m] = m < P ? costs[3 * m + 1] : 0.0;
        cs.c_fa[m] = m < P ? costs[3 * m + 2] : 0.0;
        if (m < P && !(cs.p[m] > 0.0 && cs.p[m] < 1.0 && cs.c_miss[m] > 0.0 && cs.c_fa[m] > 0.0)) return false;
    }
    return true;
}

extern "C" int spkb_sweep(const void* rec, const unsigned short* counts, int U, int Rc, int cmax, const double* costs, int P,
                          const double* act_costs, const long long* q, int Pa, double* out_d, long long* out_i, long long* ws,
                          long long ws_elems, int T, int upto, void* stream) {
    SPK_REQUIRE(rec && counts && out_d && out_i && ws, "spkb_sweep: null pointer");
    SPK_REQUIRE(T >= 2, "spkb_sweep: T=%d must lie in [2, 2^31)", T);
    SPK_REQUIRE(U >= 1 && U <= BOOT_MAX_U, "spkb_sweep: U=%d units, must lie in [1, %d]", U, BOOT_MAX_U);
    SPK_REQUIRE(P >= 0 && P <= BOOT_MAX_COSTS && (P == 0 || costs), "spkb_sweep: P=%d cost triples, at most %d", P, BOOT_MAX_COSTS);
    SPK_REQUIRE(Pa >= 0 && Pa <= BOOT_MAX_COSTS && (Pa == 0 || (act_costs && q)), "spkb_sweep: Pa=%d actDCF triples, at most %d", Pa,
                BOOT_MAX_COSTS);
    SPK_REQUIRE(cmax >= 0 && cmax <= BOOT_MAX_COUNT, "spkb_sweep: a count of %d, at most %d", cmax, BOOT_MAX_COUNT);
    SPK_REQUIRE((long long)cmax * cmax * T < (1ll << 53),                 // (below 2^32 * 2^31: no overflow)
                "spkb_sweep: max(counts)^2 * T = %d^2 * %d reaches 2^53: the weighted counts would not be exact in a double", cmax, T);
    const int G = spkb_group(U), pitch = spkb_pitch(U);
    SPK_REQUIRE(Rc >= 1 && (Rc + G - 1) / G <= 65535, "spkb_sweep: Rc=%d replicates in one call, must lie in [1, %d]", Rc, 65535 * G);
    SPK_REQUIRE(((uintptr_t)counts & 15) == 0 && ((uintptr_t)rec & 7) == 0, "spkb_sweep: counts must start on 16 bytes, rec on 8");
    SPK_REQUIRE(ws_elems >= spkb_sweep_ws_elems(T, P, Pa, Rc), "spkb_sweep: workspace of %lld words, %lld needed", ws_elems,
                spkb_sweep_ws_elems(T, P, Pa, Rc));
    BootCosts cs, as;
    SPK_REQUIRE(boot_fill(cs, costs, P) && boot_fill(as, act_costs, Pa),
                "spkb_sweep: a cost triple needs 0 < p_target < 1, c_miss > 0 and c_fa > 0");
    const int nb = boot_tiles(T), groups = (Rc + G - 1) / G;
    long long* tile_sum = ws;
    BootBest* partial = (BootBest*)(tile_sum + (size_t)Rc * 2 * (nb + 1));
    long long* act = (long long*)(partial + (size_t)Rc * (1 + P) * nb);
    const size_t lds = (size_t)G * pitch * 2;
    hipStream_t st = (hipStream_t)stream;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)boot_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)boot_rates_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            spk_set_error("spkb_sweep: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e));
            return (int)e;
        }
    }
    hipLaunchKernelGGL(boot_count_kernel, dim3(nb, groups), dim3(BOOT_THREADS), lds, st, (const uint2*)rec, counts, pitch, G, Rc, tile_sum,
                       T, nb);
    if (upto != 1) hipLaunchKernelGGL(boot_offsets_kernel, dim3(Rc), dim3(BOOT_THREADS), 0, st, tile_sum, nb);
    if (upto != 1 && upto != 2)
        hipLaunchKernelGGL(boot_rates_kernel, dim3(nb, groups), dim3(BOOT_THREADS), lds, st, (const uint2*)rec, counts, pitch, G, Rc, tile_sum, cs,
                           P, q, Pa, partial, act, T, nb);
    if (upto < 1 || upto > 3)
        hipLaunchKernelGGL(boot_final_kernel, dim3(Rc), dim3(BOOT_THREADS), 0, st, tile_sum, cs, P, as, q, Pa, partial, act, out_d, out_i, T,
                           nb);
    SPK_LAUNCH_CHECK("spkb_sweep");
    return 0;
}
