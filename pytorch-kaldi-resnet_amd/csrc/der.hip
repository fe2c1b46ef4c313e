// Diarization scoring on the device: cut one merge list at K thresholds, turn every cut into hypothesis pieces
// and score every (recording, hypothesis) job against the reference - the diarization error rate in exact int64 tick arithmetic.
//   spk_ahc_cut_batch - labels [K][Ntot] of the K prefixes of every recording's merge list, one workgroup per (recording, threshold)
//   spk_der_pieces    - the windows of every cut with make_rttm's adjacent-pair midpoint cut, in ticks
//   spk_der_batch     - (scored, miss, fa, conf, opt) and the speaker mapping of every job, one workgroup per job: per-label disjoint
//                       pieces, the counts over the elementary intervals of the scored set, the co-occurrence matrix C with integer
//                       atomics (LDS while it fits, a workspace tile beyond) and the assignment by shortest augmenting paths
// Integers only, __syncthreads() only, no workgroup waits on another, every loop is bounded by a count known at launch.  Integer
// adds commute: the bits do not depend on scheduling, on the position of a job in a batch or on where C lies.
#include "spk_common.h"

#include <vector>

#define CUT_THREADS 256
#define CUT_MAX_N 8192          // = spk_ahc_max_n(): parents are 16-bit in LDS
#define DER_THREADS 256
#define DER_WAVES (DER_THREADS / 64)
#define DER_MAX_REF 64          // one bit per reference speaker in a cell's mask
#define DER_MAX_HYP 1024
#define DER_MAX_TURNS 8192
#define DER_LDS_C 4096          // entries of C held in LDS; a larger Sr x Sh matrix lies in the job's workspace tile
#define DER_INF 0x1fffffffffffffffll

extern "C" int spk_ahc_max_n(void);

typedef long long i64;
typedef unsigned long long u64;

// ---- cutting the merge list ---------------------------------------------------------------------------------------------------------
// The merge sequence does not depend on the threshold, so the labels at threshold t are those of the longest prefix of merges whose
// costs all satisfy c <= -t.  A merge (i, j) has i < j and j leaves: parent[j] = i, and a window's cluster is the end of its chain of
// parents - the cluster's lowest member, by which spk_ahc_batch numbers the labels too.  A merge that is not 0 <= i < j < n ends the
// prefix (a guard: spk_ahc_batch never writes one).
__global__ __launch_bounds__(CUT_THREADS) void ahc_cut_kernel(const int* __restrict__ merges, const double* __restrict__ merge_cost,
                                                              const int* __restrict__ n_merges, const i64* __restrict__ rec_off,
                                                              const double* __restrict__ thresholds, int* __restrict__ labels,
                                                              i64 Ntot) {
    __shared__ unsigned short parent[CUT_MAX_N];
    __shared__ unsigned short rnk[CUT_MAX_N];
    __shared__ int cnt[CUT_THREADS];
    __shared__ int plen;

    const int r = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const i64 row0 = rec_off[r];
    const int n = (int)(rec_off[r + 1] - row0);
    int nm = n_merges[r];
    nm = nm < 0 ? 0 : (nm > n - 1 ? n - 1 : nm);
    const double lim = -thresholds[k];
    const int* mer = merges + 2 * row0;
    const double* cost = merge_cost + row0;
    int* lab = labels + (size_t)k * Ntot + row0;

    if (tid == 0) plen = nm;
    for (int a = tid; a < n; a += CUT_THREADS) parent[a] = (unsigned short)a;
    __syncthreads();
    for (int s = tid; s < nm; s += CUT_THREADS) {
        const int i = mer[2 * s], j = mer[2 * s + 1];
        if (!(cost[s] <= lim) || !(i >= 0 && i < j && j < n)) atomicMin(&plen, s);
    }
    __syncthreads();
    const int L = plen;
    for (int s = tid; s < L; s += CUT_THREADS) parent[mer[2 * s + 1]] = (unsigned short)mer[2 * s];   // (every j leaves once)
    __syncthreads();
    // rank of the roots: thread t counts the roots of its slice, thread 0 adds the counts up
    const int per = (n + CUT_THREADS - 1) / CUT_THREADS, a0 = tid * per, a1 = a0 + per < n ? a0 + per : n;
    int c = 0;
    for (int a = a0; a < a1; ++a) c += parent[a] == a;
    cnt[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < CUT_THREADS; ++t) {
            const int v = cnt[t];
            cnt[t] = run;
            run += v;
        }
    }
    __syncthreads();
    c = cnt[tid];
    for (int a = a0; a < a1; ++a) rnk[a] = parent[a] == a ? (unsigned short)(++c) : (unsigned short)0;
    __syncthreads();
    for (int a = tid; a < n; a += CUT_THREADS) {
        int x = a;
        for (int step = 0; step < n && parent[x] != x; ++step) x = parent[x];       // (parents decrease: at most n - 1 steps)
        lab[a] = rnk[x];
    }
}

extern "C" int spk_ahc_cut_batch(const int* merges, const double* merge_cost, const int* n_merges, const long long* rec_off,
                                 const long long* rec_off_dev, const double* thresholds, int K, int* labels, long long Ntot, int R,
                                 void* stream) {
    SPK_REQUIRE(rec_off && R >= 1 && R <= 65535 && Ntot >= 1 && K >= 1 && K <= 65535, "spk_ahc_cut_batch: bad arguments (R=%d, K=%d, Ntot=%lld)",
                R, K, Ntot);
    SPK_REQUIRE(rec_off[0] == 0 && rec_off[R] == Ntot, "spk_ahc_cut_batch: rec_off must run from 0 to Ntot=%lld, got %lld .. %lld", Ntot,
                rec_off[0], rec_off[R]);
    for (int r = 0; r < R; ++r) {
        const long long n = rec_off[r + 1] - rec_off[r];
        SPK_REQUIRE(n >= 1, "spk_ahc_cut_batch: recording %d is empty or rec_off decreases", r);
        SPK_REQUIRE(n <= spk_ahc_max_n() && n <= CUT_MAX_N, "spk_ahc_cut_batch: recording %d has %lld windows, the cap is %d", r, n,
                    CUT_MAX_N);
    }
    SPK_REQUIRE(merges && merge_cost && n_merges && rec_off_dev && thresholds && labels, "spk_ahc_cut_batch: null device pointer");
    hipLaunchKernelGGL(ahc_cut_kernel, dim3((unsigned)R, (unsigned)K), dim3(CUT_THREADS), 0, (hipStream_t)stream, merges, merge_cost,
                       n_merges, rec_off_dev, thresholds, labels, (i64)Ntot);
    SPK_LAUNCH_CHECK("spk_ahc_cut_batch");
    return 0;
}

// ---- the hypothesis of a cut --------------------------------------------------------------------------------------------------------
// The windows of a recording in (start, end) order, in ticks.  An adjacent pair with different labels that overlaps is cut at
// (a + b) / 2 rounded down, a the later window's start and b the earlier one's end (both as given: the cuts of a window's two sides
// do not meet).  Pieces of one label are not merged: "active" counts a speaker once.
__global__ __launch_bounds__(256) void der_pieces_kernel(const int* __restrict__ labels, const i64* __restrict__ wstart,
                                                         const i64* __restrict__ wend, const i64* __restrict__ rec_off, int R, i64 Ntot,
                                                         i64* __restrict__ pstart, i64* __restrict__ pend) {
    const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
    if (w >= Ntot) return;
    int lo = 0, hi = R;                                           // the last r with rec_off[r] <= w
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rec_off[mid] <= w) lo = mid;
        else hi = mid;
    }
    const int* lab = labels + (size_t)blockIdx.y * Ntot;
    const size_t o = (size_t)blockIdx.y * Ntot + w;
    i64 s = wstart[w], e = wend[w];
    const int l = lab[w];
    if (w > rec_off[lo] && lab[w - 1] != l && wstart[w] < wend[w - 1]) s = (wstart[w] + wend[w - 1]) >> 1;
    if (w + 1 < rec_off[lo + 1] && lab[w + 1] != l && wstart[w + 1] < wend[w]) e = (wstart[w + 1] + wend[w]) >> 1;
    pstart[o] = s;
    pend[o] = e;
}

extern "C" int spk_der_pieces(const int* labels, const long long* wstart, const long long* wend, const long long* rec_off,
                              const long long* rec_off_dev, int K, long long* pstart, long long* pend, long long Ntot, int R,
                              void* stream) {
    SPK_REQUIRE(rec_off && R >= 1 && Ntot >= 1 && Ntot < (1ll << 31) && K >= 1 && K <= 65535, "spk_der_pieces: bad arguments (R=%d, K=%d, Ntot=%lld)",
                R, K, Ntot);
    SPK_REQUIRE(rec_off[0] == 0 && rec_off[R] == Ntot, "spk_der_pieces: rec_off must run from 0 to Ntot=%lld", Ntot);
    for (int r = 0; r < R; ++r) SPK_REQUIRE(rec_off[r + 1] > rec_off[r], "spk_der_pieces: recording %d is empty or rec_off decreases", r);
    SPK_REQUIRE(labels && wstart && wend && rec_off_dev && pstart && pend, "spk_der_pieces: null device pointer");
    hipLaunchKernelGGL(der_pieces_kernel, dim3((unsigned)((Ntot + 255) / 256), (unsigned)K), dim3(256), 0, (hipStream_t)stream, labels,
                       wstart, wend, rec_off_dev, R, (i64)Ntot, pstart, pend);
    SPK_LAUNCH_CHECK("spk_der_pieces");
    return 0;
}

// ---- scoring ----------------------------------------------------------------------------------------------------------------------
// What the host prepares per recording, from the reference alone: the scored set S cut into cells - sorted disjoint intervals
// [start, end) of S on which the set of active reference speakers is constant, with that set as a 64-bit mask (cells with no
// speaker included: false alarms count there).  rec_tab [R][4] = (first cell, cells, Sr, 0); cells [ncells][3] = (start, end, mask).
// A job: job_tab [J][6] = (recording, first piece, pieces, Sh, workspace offset in 8-byte words, 0); its pieces are (label in
// 1 .. Sh, start, end) in any order; a label outside 1 .. Sh or an empty piece is ignored.
// Workspace of a job: cs [P] (a piece's start after the pieces of its label were made disjoint), ord [P] (the pieces by start, 32-bit,
// P rounded up to even), and Sr Sh entries of C where that exceeds DER_LDS_C.
struct DerBest {
    i64 v;
    int j;
};

__global__ __launch_bounds__(DER_THREADS) void der_kernel(const i64* __restrict__ rec_tab, const i64* __restrict__ cells,
                                                          const i64* __restrict__ job_tab, const int* __restrict__ plab,
                                                          const i64* __restrict__ pstart, const i64* __restrict__ pend,
                                                          i64* __restrict__ ws, i64* __restrict__ out, int* __restrict__ mapping) {
    __shared__ u64 Clds[DER_LDS_C];
    __shared__ i64 hv[DER_MAX_HYP + 1];                           // running end per label, then the column potentials
    __shared__ i64 minv[DER_MAX_HYP + 1];
    __shared__ int hp[DER_MAX_HYP + 1], way[DER_MAX_HYP + 1];
    __shared__ unsigned char used[DER_MAX_HYP + 1];
    __shared__ i64 hu[DER_MAX_REF + 1];
    __shared__ u64 acc[3];                                        // scored, miss, sum of Nh over S
    __shared__ i64 red_v[DER_WAVES];
    __shared__ int red_j[DER_WAVES];
    __shared__ int cur_j0, cur_done;

    const int job = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const i64* jt = job_tab + (size_t)job * 6;
    const int r = (int)jt[0], P = (int)jt[2], Sh = (int)jt[3];
    const i64 p0 = jt[1];
    const i64* rt = rec_tab + (size_t)r * 4;
    const i64* cell = cells + rt[0] * 3;
    const int nc = (int)rt[1], Sr = (int)rt[2];
    const int* lab = plab + p0;
    const i64* ps = pstart + p0;
    const i64* pe = pend + p0;
    i64* cs = ws + jt[4];
    int* ord = (int*)(cs + P);
    const int Peven = (P + 1) & ~1;
    const bool inlds = (i64)Sr * Sh <= DER_LDS_C;
    u64* C = inlds ? Clds : (u64*)(cs + P + Peven / 2);
    const int nC = Sr * Sh;

    for (int x = tid; x < nC; x += DER_THREADS) C[x] = 0;
    for (int l = tid; l <= Sh; l += DER_THREADS) hv[l] = -DER_INF;
    if (tid < 3) acc[tid] = 0;
    // 1: the pieces by start (rank by counting: ties to the lower index)
    for (int p = tid; p < P; p += DER_THREADS) {
        const i64 s = ps[p];
        int rank = 0;
        for (int q = 0; q < P; ++q) {
            const i64 t = ps[q];
            rank += (t < s) || (t == s && q < p);
        }
        ord[rank] = p;
    }
    __syncthreads();
    // 2: per label, in order of start, a piece starts where the earlier pieces of its label end (thread t owns the labels = t mod 256)
    for (int k = 0; k < P; ++k) {
        const int p = ord[k], l = lab[p];
        if (l >= 1 && l <= Sh && (l & (DER_THREADS - 1)) == tid) {
            const i64 e = pe[p], run = hv[l];
            i64 s = ps[p];
            s = s > run ? s : run;
            cs[p] = s < e ? s : e;                                // (an empty piece: start = end)
            if (e > run) hv[l] = e;
        } else if (!(l >= 1 && l <= Sh) && (k & (DER_THREADS - 1)) == tid) {
            cs[p] = pe[p];                                        // ignored: empty
        }
    }
    __syncthreads();
    // 3: the elementary intervals.  Keys: the nc cell starts, then every piece's start and end.  A key b inside a cell, the first of
    // its value, opens the interval [b, next key or the cell's end): there Nh = #starts <= b - #ends <= b and Nr = the cell's.
    {
        u64 a_sc = 0, a_miss = 0, a_nh = 0;
        const int nkeys = nc + 2 * P;
        for (int key = tid; key < nkeys; key += DER_THREADS) {
            i64 b;
            int c;
            bool first = true;
            if (key < nc) {
                c = key;
                b = cell[3 * c];
                const int nr = __popcll((u64)cell[3 * c + 2]);
                a_sc += (u64)(cell[3 * c + 1] - b) * (u64)nr;
            } else {
                const int q = key - nc;
                b = q < P ? cs[q] : pe[q - P];
                if (q < P ? !(b < pe[q]) : !(cs[q - P] < b)) continue;   // an empty piece has no keys
                int lo = -1, hi = nc;                              // the last cell with start <= b
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (cell[3 * mid] <= b) lo = mid;
                    else hi = mid;
                }
                c = lo;
                if (c < 0 || !(b < cell[3 * c + 1]) || b == cell[3 * c]) continue;
            }
            i64 nxt = cell[3 * c + 1];
            int ns = 0, ne = 0;
            for (int q = 0; q < P; ++q) {
                const i64 s = cs[q], e = pe[q];
                if (!(s < e)) continue;
                ns += s <= b;
                ne += e <= b;
                if (s > b && s < nxt) nxt = s;
                if (e > b && e < nxt) nxt = e;
                if (key >= nc && ((s == b && q < key - nc) || (e == b && q + P < key - nc))) first = false;
            }
            if (!first) continue;
            const int nh = ns - ne, nr = __popcll((u64)cell[3 * c + 2]);
            const u64 len = (u64)(nxt - b);
            a_nh += len * (u64)nh;
            if (nr > nh) a_miss += len * (u64)(nr - nh);
        }
        atomicAdd(&acc[0], a_sc);
        atomicAdd(&acc[1], a_miss);
        atomicAdd(&acc[2], a_nh);
    }
    // 4: C[i][j] += |piece of label j, cell with speaker i|
    for (int p = tid; p < P; p += DER_THREADS) {
        const i64 s = cs[p], e = pe[p];
        const int l = lab[p];
        if (!(s < e) || !(l >= 1 && l <= Sh)) continue;
        int lo = -1, hi = nc;                                      // the last cell with start <= s
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (cell[3 * mid] <= s) lo = mid;
            else hi = mid;
        }
        for (int c = lo < 0 ? 0 : lo; c < nc; ++c) {
            const i64 c0 = cell[3 * c], c1 = cell[3 * c + 1];
            if (c0 >= e) break;
            const i64 a = s > c0 ? s : c0, b = e < c1 ? e : c1;
            if (b <= a) continue;
            u64 m = (u64)cell[3 * c + 2];
            while (m) {
                const int i = __ffsll((long long)m) - 1;
                m &= m - 1;
                if (i < Sr) atomicAdd(&C[(size_t)i * Sh + (l - 1)], (u64)(b - a));
            }
        }
    }
    __syncthreads();
    // 5: the assignment: rows = the smaller side (n <= 64), columns = the larger (m), cost = -C, shortest augmenting paths with
    // potentials, at most n augmentations of at most n + 1 steps
    const bool tr = Sr > Sh;                                       // rows are the hypothesis labels
    const int n = tr ? Sh : Sr, m = tr ? Sr : Sh;
#define DER_COST(i, j) (-(i64)(tr ? C[(size_t)((j) - 1) * Sh + ((i) - 1)] : C[(size_t)((i) - 1) * Sh + ((j) - 1)]))
    for (int j = tid; j <= m; j += DER_THREADS) {
        hv[j] = 0;
        hp[j] = 0;
    }
    for (int i = tid; i <= n; i += DER_THREADS) hu[i] = 0;
    __syncthreads();
    for (int i = 1; i <= n; ++i) {
        for (int j = tid; j <= m; j += DER_THREADS) {
            minv[j] = DER_INF;
            used[j] = 0;
            way[j] = 0;
        }
        if (tid == 0) {
            hp[0] = i;
            cur_j0 = 0;
            cur_done = 0;
        }
        __syncthreads();
        for (int step = 0; step <= n; ++step) {
            if (cur_done) break;                                   // block-uniform (read after a barrier)
            const int j0 = cur_j0, i0 = hp[j0];
            DerBest best = {DER_INF, 0x7fffffff};
            const i64 ui = hu[i0];
            for (int j = 1 + tid; j <= m; j += DER_THREADS) {
                if (used[j] || j == j0) continue;
                const i64 cur = DER_COST(i0, j) - ui - hv[j];
                i64 mv = minv[j];
                if (cur < mv) {
                    minv[j] = mv = cur;
                    way[j] = j0;
                }
                if (mv < best.v) {                                 // j grows inside a thread: the first of equal values stays
                    best.v = mv;
                    best.j = j;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const i64 v2 = __shfl_xor(best.v, off, 64);
                const int j2 = __shfl_xor(best.j, off, 64);
                if (v2 < best.v || (v2 == best.v && j2 < best.j)) {
                    best.v = v2;
                    best.j = j2;
                }
            }
            if (lane == 0) {
                red_v[wave] = best.v;
                red_j[wave] = best.j;
            }
            __syncthreads();
            DerBest b = {red_v[0], red_j[0]};
            for (int w = 1; w < DER_WAVES; ++w)
                if (red_v[w] < b.v || (red_v[w] == b.v && red_j[w] < b.j)) {
                    b.v = red_v[w];
                    b.j = red_j[w];
                }
            const i64 delta = b.v;
            const int j1 = b.j <= m ? b.j : 0;                     // (n <= m: an unused column always exists; 0 ends the path)
            for (int j = tid; j <= m && b.j <= m; j += DER_THREADS) {
                if (used[j] || j == j0) {
                    hu[hp[j]] += delta;                            // (the rows of the used columns are distinct)
                    hv[j] -= delta;
                } else {
                    minv[j] -= delta;
                }
            }
            __syncthreads();
            if (tid == 0) {
                used[j0] = 1;
                cur_j0 = j1;
                if (j1 == 0 || hp[j1] == 0) cur_done = 1;
            }
            __syncthreads();
        }
        if (tid == 0) {
            int j0 = cur_j0;
            for (int step = 0; step <= n && j0 != 0; ++step) {
                const int j1 = way[j0];
                hp[j0] = hp[j1];
                j0 = j1;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        int* mp = mapping + (size_t)job * DER_MAX_REF;
        for (int i = 0; i < DER_MAX_REF; ++i) mp[i] = -1;
        u64 opt = 0;
        for (int j = 1; j <= m; ++j) {
            const int i = hp[j];
            if (i == 0) continue;
            const u64 v = (u64)(-DER_COST(i, j));
            if (v == 0) continue;
            opt += v;
            if (tr) mp[j - 1] = i;                                 // reference speaker j - 1 -> label i
            else mp[i - 1] = j;
        }
        const u64 scored = acc[0], miss = acc[1], nh = acc[2];
        i64* o = out + (size_t)job * 5;
        o[0] = (i64)scored;
        o[1] = (i64)miss;
        o[2] = (i64)(nh + miss - scored);                          // fa = sum max(0, Nh - Nr) = sum Nh - sum Nr + miss
        o[3] = (i64)(scored - miss - opt);                         // conf = sum min(Nr, Nh) - opt, min(Nr, Nh) = Nr - max(0, Nr - Nh)
        o[4] = (i64)opt;
    }
#undef DER_COST
}

extern "C" int spk_der_max_ref(void) { return DER_MAX_REF; }
extern "C" int spk_der_max_hyp(void) { return DER_MAX_HYP; }
extern "C" int spk_der_max_turns(void) { return DER_MAX_TURNS; }

// the 8-byte words of workspace one job needs
static long long der_job_words(long long P, long long Sr, long long Sh) {
    return P + ((P + 1) & ~1ll) / 2 + (Sr * Sh > DER_LDS_C ? Sr * Sh : 0);
}

extern "C" long long spk_der_ws_elems(int pieces, int Sr, int Sh) {
    SPK_REQUIRE(pieces >= 0 && pieces <= DER_MAX_TURNS && Sr >= 0 && Sr <= DER_MAX_REF && Sh >= 0 && Sh <= DER_MAX_HYP,
                "spk_der_ws_elems: pieces=%d, Sr=%d, Sh=%d exceed the limits (%d, %d, %d)", pieces, Sr, Sh, DER_MAX_TURNS, DER_MAX_REF,
                DER_MAX_HYP);
    return der_job_words(pieces, Sr, Sh);
}

extern "C" int spk_der_batch(const long long* rec_tab, const long long* rec_tab_dev, const long long* cells, long long ncells, int R,
                             const long long* job_tab, const long long* job_tab_dev, int J, const int* plab, const long long* pstart,
                             const long long* pend, long long npieces, long long* ws, long long ws_elems, long long* out, int* mapping,
                             void* stream) {
    SPK_REQUIRE(rec_tab && job_tab && R >= 1 && J >= 1 && J < (1 << 30) && ncells >= 0 && npieces >= 0 && ws_elems >= 0,
                "spk_der_batch: bad arguments (R=%d, J=%d)", R, J);
    for (int r = 0; r < R; ++r) {
        const long long* t = rec_tab + 4 * (size_t)r;
        SPK_REQUIRE(t[0] >= 0 && t[1] >= 0 && t[1] < (1ll << 30) && t[0] + t[1] <= ncells, "spk_der_batch: the cells of recording %d (%lld + %lld) leave the table of %lld",
                    r, t[0], t[1], ncells);
        SPK_REQUIRE(t[2] >= 0 && t[2] <= DER_MAX_REF, "spk_der_batch: recording %d has %lld reference speakers, the cap is %d", r, t[2],
                    DER_MAX_REF);
    }
    for (int j = 0; j < J; ++j) {
        const long long* t = job_tab + 6 * (size_t)j;
        SPK_REQUIRE(t[0] >= 0 && t[0] < R, "spk_der_batch: job %d names recording %lld of %d", j, t[0], R);
        SPK_REQUIRE(t[2] >= 0 && t[2] <= DER_MAX_TURNS, "spk_der_batch: job %d has %lld pieces, the cap is %d", j, t[2], DER_MAX_TURNS);
        SPK_REQUIRE(t[1] >= 0 && t[1] + t[2] <= npieces, "spk_der_batch: the pieces of job %d (%lld + %lld) leave the table of %lld", j, t[1],
                    t[2], npieces);
        SPK_REQUIRE(t[3] >= 0 && t[3] <= DER_MAX_HYP, "spk_der_batch: job %d has %lld hypothesis labels, the cap is %d", j, t[3], DER_MAX_HYP);
        SPK_REQUIRE(t[4] >= 0 && t[4] + der_job_words(t[2], rec_tab[4 * (size_t)t[0] + 2], t[3]) <= ws_elems,
                    "spk_der_batch: the workspace of job %d (from %lld, %lld words) leaves the %lld words given", j, t[4],
                    der_job_words(t[2], rec_tab[4 * (size_t)t[0] + 2], t[3]), ws_elems);
    }
    SPK_REQUIRE(rec_tab_dev && job_tab_dev && (cells || !ncells) && (npieces == 0 || (plab && pstart && pend)) && ws && out && mapping,
                "spk_der_batch: null device pointer");
    hipLaunchKernelGGL(der_kernel, dim3((unsigned)J), dim3(DER_THREADS), 0, (hipStream_t)stream, rec_tab_dev, cells, job_tab_dev, plab,
                       pstart, pend, ws, out, mapping);
    SPK_LAUNCH_CHECK("spk_der_batch");
    return 0;
}
