// Sample-rate conversion of a padded batch of waveforms: Kaldi's LinearResample / ResampleWaveform (reference: kaldi.py
// resample_waveform: Hann-windowed sinc, cutoff 0.99 x 0.5 x min(rate), 6 zero crossings, one filter per output phase).
// Semantics: DESIGN.md section "Feature front end", "Resampling".
//
// With g = gcd(fi, fo), iu = fi / g, ou = fo / g, output j of a row has phase p = j % ou and unit u = j / ou:
//     y[j] = sum_{k < K} w[p][k] * x[first[p] + u * iu + k],      x = 0 outside [0, n)
// The host builds first [ou] and w [ou][K] in fp64 and passes them rounded to fp32, w as pairs of consecutive taps with the phase
// running fastest: wq [ceil(K / 2)][ou][2] (an odd K is padded with a zero tap).
//
// spk_resample_fwd: one workgroup of 256 threads per (row, run of RS_NT tiles of TO consecutive outputs).  The whole table sits in
// LDS for the life of the workgroup; per tile the input span the TO outputs share (about TO * iu / ou + K samples; neighbouring
// outputs overlap in all but iu / ou of them) is staged with 16-byte loads from a 16-byte aligned start, zero outside [0, n).
// Each thread then sums the taps of its TO / 256 outputs (256 apart, side by side: independent chains) and the wave stores 256
// contiguous bytes per output.
// The tap loop is two 8-byte LDS reads and one packed FMA per pair of taps: the weight pairs of the lanes of a wave (consecutive
// outputs, consecutive phases) lie in consecutive banks, and the span is kept twice, once as it is and once shifted by one sample,
// so that a window starting at an odd sample is a run of aligned pairs as well.  The taps 0, 2, 4, .. and 1, 3, 5, .. of an output
// are summed in two fp32 chains (the halves of the packed FMA), each in index order, and added at the end: a fixed order whatever
// the alignment.  The zero tap of an odd K adds w = 0 times a finite sample: an output depends on its row's samples only, never
// on the batch, the row index, the padding or the tile it falls in, bit for bit.  What bounds the kernel: DESIGN.md, same section.
//
// spkw_resample_span_fwd (include/spkwav.h): the same body on a span.  Row b holds samples [ifirst, ifirst + icount) of an utterance
// of itotal samples and gets outputs [ofirst, ofirst + ocount) of that utterance's resampling: column i is output j = ofirst + i,
// phase, unit and window start are those of j in the utterance, and only the staging moves the window into the row (- ifirst).  The
// values read and the order of the sums are the whole form's, so the columns equal the whole-utterance launch bit for bit, whatever
// the row-relative alignment of the window.  A staged sample is loaded only if the row holds it: one inside the utterance but
// outside the row counts as 0, like one outside the utterance, and nothing at or past icount is read.  blockIdx.y indexes an optional
// device list of rows, so the rows of one rate of a mixed batch take one launch; the other rows are not touched.
#include "spk_common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_LDS_LIMIT = 64 * 1024;       // table + the two copies of the span of one workgroup
constexpr int RS_MAX_TILE = 1024;             // outputs per tile (a multiple of RS_THREADS)
constexpr int RS_NT = 8;                      // at most this many tiles per workgroup: the table load is shared by them

struct ResampleArgs {
    const float* wave_in;      // [B][Nmax_in]
    const int* nsamp_in;       // [B]                                                            (whole form)
    const int* first;          // [ou]
    const float2* wq;          // [K2][ou] pairs of taps (2m, 2m + 1)
    float* wave_out;           // [B][Nmax_out]
    int* nsamp_out;            // [B]                                                            (whole form)
    long long Nmax_in, Nmax_out;
    int iu, ou, K2, TO, NT, span, tab4, vec;    // K2 = ceil(K / 2); span: floats of one copy of the staged input (multiple of 4);
                                                // tab4: floats before the first copy
};

// the span form: row b holds samples [ifirst, ifirst + icount) of an utterance of itotal samples and gets outputs
// [ofirst, ofirst + ocount) of that utterance's resampled signal; rows: the rows this launch works on (NULL: all B of them).
// Derived, so that the kernel arguments of the whole form keep their layout.
struct ResampleSpanArgs : ResampleArgs {
    const long long *ifirst, *itotal, *ofirst;    // [B]
    const int *icount, *ocount;                   // [B]
    const int* rows;                              // [gridDim.y] or NULL
    int B;
};

// samples of the span per tile: f(j) = first[j % ou] + (j / ou) * iu = ceil(j * iu / ou - c) grows by at most
// ceil((TO - 1) * iu / ou) (+ 1 for the fp64 rounding of the host table) over TO outputs; + 2 K2 taps, + 3 for the aligned start,
// + 1 for the shifted copy (it ends one sample early); rounded up to whole float4
inline long long rs_span(int TO, int iu, int ou, int K) {
    const long long d = ((long long)(TO - 1) * iu + ou - 1) / ou + 1 + 2 * ((K + 1) / 2) + 3 + 1;
    return (d + 3) / 4 * 4;
}
inline long long rs_table(int ou, int K) { return ((long long)ou * 2 * ((K + 1) / 2) + ou + 3) / 4 * 4; }
inline long long rs_lds_floats(int TO, int iu, int ou, int K) { return rs_table(ou, K) + 2 * rs_span(TO, iu, ou, K); }

typedef float rs_f2 __attribute__((ext_vector_type(2)));

// NPT = TO / 256 outputs per thread and tile, summed side by side (independent chains hide the LDS latency of each other).
// One body for both forms.  The row holds samples [f, f + c) of an utterance of n samples and gets its outputs [o, o + n_out);
// the whole form is f = o = 0, c = n, n_out = every output of the utterance: with SPAN = false the offsets fold away and the kernel
// is the one it was, instruction for instruction.  A sample of
// the utterance that the row does not hold reads as 0, like one outside the utterance: nothing outside [x, x + c) is loaded.
template <int NPT, bool SPAN, class A>
__device__ __forceinline__ void resample_body(const A& a) {
    extern __shared__ float4 rs_lds4[];
    float2* wq = (float2*)rs_lds4;                     // [K2][ou]
    int* first = (int*)(wq + (size_t)a.K2 * a.ou);     // [ou]
    float4* span4 = rs_lds4 + (a.tab4 >> 2);           // [span / 4]: the staged input, 16-byte aligned (tab4 is a multiple of 4)
    float* spano = (float*)(span4 + (a.span >> 2));    // [span]: the same shifted by one sample, spano[i] = span[i + 1]
    int b = blockIdx.y;
    const int tid = threadIdx.x;
    // every index below fits 32 bits (the host checks Nmax_in, Nmax_out, itotal < 2^30 and iu * ou < 2^31): no 64-bit division
    // on the device
    const int Nout = (int)a.Nmax_out;
    // n: samples of the utterance; f, o: the row's first sample and first output in it; [0, vhi): the row's samples that exist
    int n, f = 0, o = 0, vhi, want = Nout;
    if constexpr (SPAN) {
        if (a.rows) b = a.rows[blockIdx.y];
        if (b < 0 || b >= a.B) return;                // a row list is device data: a bad entry is skipped, not followed
        n = (int)min(max(a.itotal[b], 0ll), (1ll << 30) - 1);
        f = (int)min(max(a.ifirst[b], 0ll), (long long)n);
        o = (int)min(max(a.ofirst[b], 0ll), (1ll << 30) - 1);
        vhi = min(min(max(a.icount[b], 0), (int)a.Nmax_in), n - f);
        want = min(max(a.ocount[b], 0), Nout);
    } else {
        n = min(max(a.nsamp_in[b], 0), (int)a.Nmax_in);
        vhi = n;
    }
    // LinearResample::GetNumOutputSamples: the outputs j with j / fo < n / fi, i.e. ceil(n * ou / iu), split at whole units
    const unsigned nq = (unsigned)n / (unsigned)a.iu, nr = (unsigned)n - nq * (unsigned)a.iu;
    const long long n_out_ll = (long long)nq * a.ou + (nr * (unsigned)a.ou + (unsigned)a.iu - 1u) / (unsigned)a.iu;
    // the outputs of this row that exist: its first n_out columns
    const int n_out = SPAN ? (int)min(max(n_out_ll - o, 0ll), (long long)want) : (int)min(n_out_ll, (long long)Nout);
    if constexpr (!SPAN) {
        if (blockIdx.x == 0 && tid == 0) a.nsamp_out[b] = n_out;
    }
    const float* x = a.wave_in + (size_t)b * a.Nmax_in;
    float* y = a.wave_out + (size_t)b * a.Nmax_out;
    const int amod = (int)(((long long)b * a.Nmax_in) & 3);        // the row's first sample, modulo 16 bytes
    const long long jb_ll = (long long)blockIdx.x * a.NT * a.TO;   // < Nmax_out + NT * TO
    if (jb_ll >= Nout) return;
    const int jb = (int)jb_ll;
    if (jb < n_out) {         // block-uniform: a workgroup entirely past the row's end stores zeros only
        for (int i = tid; i < a.K2 * a.ou; i += RS_THREADS) wq[i] = a.wq[i];
        for (int i = tid; i < a.ou; i += RS_THREADS) first[i] = a.first[i];
    }
    for (int t = 0; t < a.NT; ++t) {
        const int j0 = jb + t * a.TO;                 // < 2^30 + NT * TO
        if (j0 >= Nout) break;
        if (j0 >= n_out) {    // block-uniform
            for (int i = tid; i < NPT * RS_THREADS && j0 + i < Nout; i += RS_THREADS) y[j0 + i] = 0.f;
            continue;
        }
        __syncthreads();      // the table is in LDS; the previous tile's reads of the span are done
        // column j0 is output o + j0 of the utterance (< 2^31: o < 2^30, j0 < n_out <= 2^30)
        const unsigned u0 = (unsigned)(o + j0) / (unsigned)a.ou, p0 = (unsigned)(o + j0) - u0 * (unsigned)a.ou;
        // first input sample of that output, counted from the row's first sample (may be negative)
        const int lo = first[p0] + (int)u0 * a.iu - f;
        // row-relative start of the span: the element whose ABSOLUTE index in wave_in is the multiple of 4 at or below lo's
        const int s0 = lo - ((lo + amod) & 3);
        // four quads per thread at a time: the 16-byte loads of the quads that lie inside the row are all issued before the first
        // of them is waited for; a quad that straddles an end of the row (or an unaligned base) is gathered by element
        for (int q0 = tid; q0 < a.span / 4; q0 += 4 * RS_THREADS) {
            float4 v[4];
            bool in[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int s = s0 + 4 * (q0 + e * RS_THREADS);
                in[e] = a.vec && q0 + e * RS_THREADS < a.span / 4 && s >= 0 && s + 4 <= vhi;
                if (in[e]) v[e] = *(const float4*)(x + s);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int q = q0 + e * RS_THREADS;
                if (q >= a.span / 4) break;
                const int s = s0 + 4 * q;
                if (!in[e]) {
                    v[e].x = (s >= 0 && s < vhi) ? x[s] : 0.f;
                    v[e].y = (s + 1 >= 0 && s + 1 < vhi) ? x[s + 1] : 0.f;
                    v[e].z = (s + 2 >= 0 && s + 2 < vhi) ? x[s + 2] : 0.f;
                    v[e].w = (s + 3 >= 0 && s + 3 < vhi) ? x[s + 3] : 0.f;
                }
                span4[q] = v[e];
                if (q > 0) spano[4 * q - 1] = v[e].x;
                *(float2*)(spano + 4 * q) = make_float2(v[e].y, v[e].z);
                spano[4 * q + 2] = v[e].w;
            }
        }
        __syncthreads();
        // windows and weights as pair indices into the LDS block: the loop below adds a scalar to them, nothing else
        const rs_f2* lds2 = (const rs_f2*)rs_lds4;
        int xi[NPT], wi[NPT];
        rs_f2 acc[NPT];
#pragma unroll
        for (int c = 0; c < NPT; ++c) {       // an output past n_out reads a valid window too; its sum is dropped below
            const unsigned i = (unsigned)(tid + c * RS_THREADS);
            const unsigned du = (p0 + i) / (unsigned)a.ou;                        // units past u0
            const int p = (int)(p0 + i - du * (unsigned)a.ou);
            int r = first[p] + (int)(u0 + du) * a.iu - f - s0;
            // a table that is what the host builds keeps r in [0, span - 2 K2 - 1]; anything else stays inside the span
            r = min(max(r, 0), a.span - 2 * a.K2 - 1);
            // an odd start reads the shifted copy: its pair r >> 1 is (span[r], span[r + 1])
            xi[c] = ((a.tab4 + ((r & 1) ? a.span : 0)) >> 1) + (r >> 1);
            wi[c] = p;
            acc[c] = rs_f2{0.f, 0.f};
        }
        int wo = 0;
#pragma unroll 2
        for (int m = 0; m < a.K2; ++m, wo += a.ou) {
#pragma unroll
            for (int c = 0; c < NPT; ++c) acc[c] = __builtin_elementwise_fma(lds2[wi[c] + wo], lds2[xi[c] + m], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < NPT; ++c) {
            const int j = j0 + tid + c * RS_THREADS;
            if (j < Nout) y[j] = j < n_out ? acc[c].x + acc[c].y : 0.f;
        }
    }
}

template <int NPT>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(ResampleArgs a) { resample_body<NPT, false>(a); }

template <int NPT>
__global__ __launch_bounds__(RS_THREADS) void resample_span_kernel(ResampleSpanArgs a) { resample_body<NPT, true>(a); }

// rows of a batch that pass through unchanged beside resampled ones: out[b][i] = in[b][i] for i < count[b], 0 up to Nmax_out
__global__ __launch_bounds__(RS_THREADS) void copy_rows_kernel(const float* in, const int* count, const int* rows, int B, long long Nmax_in,
                                                               long long Nmax_out, float* out) {
    const int b = rows ? rows[blockIdx.y] : blockIdx.y;
    if (b < 0 || b >= B) return;
    const long long c = min((long long)max(count[b], 0), min(Nmax_in, Nmax_out));
    const float* x = in + (size_t)b * Nmax_in;
    float* y = out + (size_t)b * Nmax_out;
    for (long long i = (long long)blockIdx.x * RS_THREADS + threadIdx.x; i < Nmax_out; i += (long long)gridDim.x * RS_THREADS)
        y[i] = i < c ? x[i] : 0.f;
}

int rs_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

}  // namespace

// ---- exports (include/spkhip.h) ----
extern "C" int spk_resample_tile(int iu, int ou, int K) {
    if (iu < 1 || ou < 1 || K < 1) return 0;
    for (int TO = RS_MAX_TILE; TO >= RS_THREADS; TO >>= 1)
        if (rs_lds_floats(TO, iu, ou, K) * 4 <= RS_LDS_LIMIT) return TO;
    return 0;
}

// what the two forms share: the checks of the rates and sizes, the tile, the LDS layout and the grid (`gy` rows); < 0: refused
static int rs_setup(const char* who, ResampleArgs& a, int gy, int B, long long Nmax_in, long long Nmax_out, int fi, int fo, int K,
                    dim3& grid, int& lds) {
    SPK_REQUIRE(fi > 0 && fo > 0 && fi != fo && fi < (1 << 24) && fo < (1 << 24),
                "%s: rates %d -> %d Hz (positive, different, below 2^24)", who, fi, fo);
    SPK_REQUIRE(B > 0 && B <= 65535 && Nmax_in > 0 && Nmax_out > 0 && Nmax_in < (1ll << 30) && Nmax_out < (1ll << 30) && K > 0,
                "%s: B=%d Nmax_in=%lld Nmax_out=%lld (< 2^30) K=%d", who, B, Nmax_in, Nmax_out, K);
    const int g = rs_gcd(fi, fo), iu = fi / g, ou = fo / g;
    SPK_REQUIRE((long long)iu * ou < (1ll << 31), "%s: %d -> %d Hz: %d x %d samples per unit exceed 32-bit indexing", who, fi, fo, iu,
                ou);
    const int TO = spk_resample_tile(iu, ou, K);
    SPK_REQUIRE(TO > 0, "%s: %d -> %d Hz needs a filter table of %d phases x %d taps (%lld bytes), which does not fit "
                "the %d bytes of LDS the kernel is built for", who, fi, fo, ou, K, rs_table(ou, K) * 4, RS_LDS_LIMIT);
    a.Nmax_in = Nmax_in; a.Nmax_out = Nmax_out; a.iu = iu; a.ou = ou; a.K2 = (K + 1) / 2; a.TO = TO;
    a.span = (int)rs_span(TO, iu, ou, K);
    a.tab4 = (int)rs_table(ou, K);
    a.vec = ((size_t)a.wave_in & 15) == 0 ? 1 : 0;     // 16-byte loads need an aligned base; otherwise element loads
    // tiles per workgroup: enough outputs to pay for loading the table once, as few as that allows (short rows keep the grid wide)
    const long long tiles = (Nmax_out + TO - 1) / TO;
    long long nt = (2ll * ou * K + TO - 1) / TO;
    nt = nt < 1 ? 1 : (nt > RS_NT ? RS_NT : nt);
    a.NT = (int)(nt > tiles ? tiles : nt);
    const long long gx = (tiles + a.NT - 1) / a.NT;
    SPK_REQUIRE(gx < (1ll << 31), "%s: Nmax_out=%lld exceeds the grid", who, Nmax_out);
    lds = (a.tab4 + 2 * a.span) * 4;
    grid = dim3((unsigned)gx, (unsigned)gy);
    return 0;
}

extern "C" int spk_resample_fwd(const float* wave_in, const int* nsamp_in, int B, long long Nmax_in, const int* first,
                                const float* wq, int fi, int fo, int K, float* wave_out, int* nsamp_out, long long Nmax_out,
                                void* stream) {
    SPK_REQUIRE(wave_in && nsamp_in && first && wq && wave_out && nsamp_out, "spk_resample_fwd: null pointer");
    ResampleArgs a = {};
    a.wave_in = wave_in; a.nsamp_in = nsamp_in; a.first = first; a.wq = (const float2*)wq; a.wave_out = wave_out; a.nsamp_out = nsamp_out;
    dim3 grid;
    int lds;
    if (const int rc = rs_setup("spk_resample_fwd", a, B, B, Nmax_in, Nmax_out, fi, fo, K, grid, lds)) return rc;
    if (a.TO == 4 * RS_THREADS) hipLaunchKernelGGL(resample_kernel<4>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a);
    else if (a.TO == 2 * RS_THREADS) hipLaunchKernelGGL(resample_kernel<2>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(resample_kernel<1>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a);
    SPK_LAUNCH_CHECK("spk_resample_fwd");
    return 0;
}

// ---- exports (include/spkwav.h) ----
extern "C" int spkw_resample_span_fwd(const float* wave_in, const long long* ifirst, const int* icount, const long long* itotal,
                                      const long long* ofirst, const int* ocount, const int* rows, int R, int B, long long Nmax_in,
                                      const int* first, const float* wq, int fi, int fo, int K, float* wave_out, long long Nmax_out,
                                      void* stream) {
    SPK_REQUIRE(wave_in && ifirst && icount && itotal && ofirst && ocount && first && wq && wave_out,
                "spkw_resample_span_fwd: null pointer");
    SPK_REQUIRE(rows ? (R > 0 && R <= B) : R == B, "spkw_resample_span_fwd: R=%d rows of B=%d (R == B without a row list)", R, B);
    ResampleSpanArgs a = {};
    a.B = B;
    a.wave_in = wave_in; a.first = first; a.wq = (const float2*)wq; a.wave_out = wave_out;
    a.ifirst = ifirst; a.icount = icount; a.itotal = itotal; a.ofirst = ofirst; a.ocount = ocount; a.rows = rows;
    dim3 grid;
    int lds;
    if (const int rc = rs_setup("spkw_resample_span_fwd", a, R, B, Nmax_in, Nmax_out, fi, fo, K, grid, lds)) return rc;
    if (a.TO == 4 * RS_THREADS) hipLaunchKernelGGL(resample_span_kernel<4>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a);
    else if (a.TO == 2 * RS_THREADS) hipLaunchKernelGGL(resample_span_kernel<2>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(resample_span_kernel<1>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a);
    SPK_LAUNCH_CHECK("spkw_resample_span_fwd");
    return 0;
}

extern "C" int spkw_copy_rows_fwd(const float* wave_in, const int* count, const int* rows, int R, int B, long long Nmax_in,
                                  float* wave_out, long long Nmax_out, void* stream) {
    SPK_REQUIRE(wave_in && count && wave_out, "spkw_copy_rows_fwd: null pointer");
    SPK_REQUIRE(B > 0 && B <= 65535 && (rows ? (R > 0 && R <= B) : R == B) && Nmax_in > 0 && Nmax_out > 0 && Nmax_in < (1ll << 30) &&
                Nmax_out < (1ll << 30), "spkw_copy_rows_fwd: R=%d rows of B=%d, Nmax_in=%lld Nmax_out=%lld (< 2^30)", R, B, Nmax_in,
                Nmax_out);
    const long long gx = (Nmax_out + 4 * RS_THREADS - 1) / (4 * RS_THREADS);
    hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)gx, (unsigned)R), dim3(RS_THREADS), 0, (hipStream_t)stream, wave_in, count,
                       rows, B, Nmax_in, Nmax_out, wave_out);
    SPK_LAUNCH_CHECK("spkw_copy_rows_fwd");
    return 0;
}
