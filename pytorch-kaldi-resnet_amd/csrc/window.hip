// Windowed extraction: the two device steps around the length-masked predict.
//
// spk_window_gather: window i of a plan is the frames [start[i], start[i] + len[i]) of utterance row[i] of a padded batch
// src [B][F][T]; it becomes row i of out [N][F][Wcap], zero past its length - the padded batch predict(x, lengths=) takes.  The
// output is the slices bit for bit (plain moves, no arithmetic).  A lane owns four consecutive frames j0 .. j0 + 3 of one (i, f)
// row: one 16-byte store when out and Wcap allow it (Wcap % 4 == 0 and out 16-byte aligned - always, behind ingest.window_batches),
// four 4-byte stores otherwise; one 16-byte load when the four frames lie inside the window and their address is 16-byte aligned
// (start[i] + row offset a multiple of 4), four guarded 4-byte loads otherwise, so a window that starts anywhere is read without a
// misaligned vector access.  The grid is one-dimensional over N * F * ceil(Wcap / 4) lanes: N * F may exceed 65 535.
// The plan is made on the host (ingest.plan_windows), so it is validated there, before anything is launched; the kernel reads the
// device copy of the same three arrays.
//
// spk_window_mean: the length-weighted mean of the window embeddings of every utterance, one lane per (utterance, dimension), the
// rows of a segment taken in order with one fused multiply-add each: no atomics, the same bits on every run.
#include "spk_common.h"

namespace {

constexpr int WIN_THREADS = 256;

struct WinGatherArgs {
    const float* src;      // [B][F][T]
    const int* plan;       // device [3][N]: row, start, len
    float* out;            // [N][F][Wcap]
    long long total;       // N * F * quads
    int N, F, T, Wcap, quads, vec_out;
};

__global__ __launch_bounds__(WIN_THREADS) void window_gather_kernel(WinGatherArgs a) {
    const long long g = (long long)blockIdx.x * WIN_THREADS + threadIdx.x;
    if (g >= a.total) return;
    long long r;            // output row i * F + f
    int q;
    if (a.total < (1ll << 31)) {
        r = (long long)((unsigned)g / (unsigned)a.quads);
        q = (int)((unsigned)g - (unsigned)r * (unsigned)a.quads);
    } else {
        r = g / a.quads;
        q = (int)(g - r * a.quads);
    }
    const int i = (int)(r / a.F), f = (int)(r - (long long)i * a.F);      // N * F < 2^31 (host)
    const int row = a.plan[i], start = a.plan[a.N + i], len = a.plan[2 * a.N + i];
    const int j0 = 4 * q;
    const float* s = a.src + ((size_t)row * a.F + f) * a.T + start + j0;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (j0 + 4 <= len && (((size_t)s) & 15) == 0) {
        const float4 t = *(const float4*)s;
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + k < len) v[k] = s[k];
    }
    float* o = a.out + (size_t)r * a.Wcap + j0;
    if (a.vec_out) {
        *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + k < a.Wcap) o[k] = v[k];
    }
}

__global__ __launch_bounds__(WIN_THREADS) void window_mean_kernel(const float* __restrict__ emb, const int* __restrict__ seg_off,
                                                                  const float* __restrict__ weight, float* __restrict__ out,
                                                                  long long total, int D) {
    const long long g = (long long)blockIdx.x * WIN_THREADS + threadIdx.x;
    if (g >= total) return;
    const int u = (int)(g / D), d = (int)(g - (long long)u * D);
    const int r0 = seg_off[u], r1 = seg_off[u + 1];
    float acc = 0.f, tot = 0.f;
    for (int r = r0; r < r1; ++r) {
        const float w = weight[r];
        acc = fmaf(w, emb[(size_t)r * D + d], acc);
        tot += w;
    }
    out[g] = acc * __fdiv_rn(1.0f, tot);
}

}  // namespace

// ---- exports (include/spkhip.h) ----
extern "C" int spk_window_gather(const float* src, int B, int F, int T, const int* row, const int* start, const int* len,
                                 const int* plan_dev, float* out, int N, int Wcap, void* stream) {
    SPK_REQUIRE(B > 0 && F > 0 && T > 0 && N > 0 && Wcap > 0, "spk_window_gather: B=%d F=%d T=%d N=%d Wcap=%d", B, F, T, N, Wcap);
    SPK_REQUIRE(row && start && len, "spk_window_gather: the host plan (row, start, len) is missing");
    SPK_REQUIRE((long long)N * F < (1ll << 31) && (long long)B * F < (1ll << 31), "spk_window_gather: N * F or B * F exceeds 2^31");
    for (int i = 0; i < N; ++i) {
        SPK_REQUIRE(row[i] >= 0 && row[i] < B, "spk_window_gather: window %d: row %d outside [0, B=%d)", i, row[i], B);
        SPK_REQUIRE(start[i] >= 0, "spk_window_gather: window %d: start %d < 0", i, start[i]);
        SPK_REQUIRE(len[i] >= 1, "spk_window_gather: window %d: len %d < 1", i, len[i]);
        SPK_REQUIRE((long long)start[i] + len[i] <= T, "spk_window_gather: window %d: start %d + len %d > T=%d", i, start[i], len[i], T);
        SPK_REQUIRE(len[i] <= Wcap, "spk_window_gather: window %d: len %d > Wcap=%d", i, len[i], Wcap);
    }
    SPK_REQUIRE(src && plan_dev && out, "spk_window_gather: null device pointer");
    SPK_REQUIRE(((size_t)src & 3) == 0 && ((size_t)out & 3) == 0, "spk_window_gather: src and out must be 4-byte aligned");
    WinGatherArgs a;
    a.src = src; a.plan = plan_dev; a.out = out; a.N = N; a.F = F; a.T = T; a.Wcap = Wcap;
    a.quads = (Wcap + 3) / 4;
    a.vec_out = (Wcap % 4 == 0 && ((size_t)out & 15) == 0) ? 1 : 0;
    a.total = (long long)N * F * a.quads;
    const long long blocks = (a.total + WIN_THREADS - 1) / WIN_THREADS;
    SPK_REQUIRE(blocks < (1ll << 31), "spk_window_gather: %lld output values exceed the grid", a.total * 4);
    hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)blocks), dim3(WIN_THREADS), 0, (hipStream_t)stream, a);
    SPK_LAUNCH_CHECK("spk_window_gather");
    return 0;
}

extern "C" int spk_window_mean(const float* emb, int N, int D, const int* seg_off, const int* seg_off_dev, const float* weight,
                               float* out, int U, void* stream) {
    SPK_REQUIRE(N > 0 && D > 0 && U > 0 && U <= N, "spk_window_mean: N=%d D=%d U=%d", N, D, U);
    SPK_REQUIRE(seg_off, "spk_window_mean: the host seg_off is missing");
    SPK_REQUIRE(seg_off[0] == 0 && seg_off[U] == N, "spk_window_mean: seg_off must run from 0 to N=%d, got %d .. %d", N, seg_off[0],
                seg_off[U]);
    for (int u = 0; u < U; ++u)
        SPK_REQUIRE(seg_off[u + 1] > seg_off[u], "spk_window_mean: segment %d is empty (seg_off %d, %d)", u, seg_off[u], seg_off[u + 1]);
    SPK_REQUIRE(emb && seg_off_dev && weight && out, "spk_window_mean: null device pointer");
    const long long total = (long long)U * D;
    const long long blocks = (total + WIN_THREADS - 1) / WIN_THREADS;
    SPK_REQUIRE(blocks < (1ll << 31), "spk_window_mean: U * D = %lld is too large", total);
    hipLaunchKernelGGL(window_mean_kernel, dim3((unsigned)blocks), dim3(WIN_THREADS), 0, (hipStream_t)stream, emb, seg_off_dev, weight,
                       out, total, D);
    SPK_LAUNCH_CHECK("spk_window_mean");
    return 0;
}
