// Reverberation and additive noise of a padded batch of waveforms: the signal contract of Kaldi's wav-reverberate as the recipe
// calls it (reference: feature_pre.sh:109-167; steps/data/reverberate_data_dir.py:345,365 emits --impulse-response and
// --shift-output=true, steps/data/augment_data_dir.py:87-88,112 emits --additive-signals / --start-times / --snrs and the
// --duration of a background item).  Semantics and the stated assumptions: DESIGN.md section 6f.
//
// Per row b with speech x[0..N), an optional impulse response h[0..R) (peak s, early part h[e0 .. e0 + E)) and descriptors
// d = (pool offset, raw length, filled length D, start sample o, SNR in dB):
//     p_before = sum x^2 / N
//     y = x * h (full linear convolution, M = N + R - 1 samples), p_sig = mean square of x * h_early     (R > 0)
//     y = x, M = N, p_sig = p_before, s = 0                                                           (R == 0)
//     y[i] += a_d n_d[(i - o_d) mod raw_d]  for 0 <= i - o_d < D_d, i < M;   a_d = sqrt(10^(-snr_d / 10) p_sig / q_d),
//                                                                            q_d = sum_{t < D_d} n_d[t mod raw_d]^2 / D_d
//     out[j] = g y[j + s], j < N;   g = sqrt(p_before / (sum y^2 / M));   optionally trunc + clip to int16, clipped samples counted
//
// The convolution is the hot path and runs in the frequency domain, uniformly partitioned overlap-save: blocks of P = 1024
// samples, FFTs of L = 2048 points (radix-2, in LDS, one workgroup of 256 threads per FFT, twiddles built by the host in fp64).
//   aug_spectra_kernel  the spectra (bins 0 .. P, the rest follows from the inputs being real) of the windows
//                       x[(m - 1) P .. (m + 1) P) of the speech, of the partitions h[p P .. (p + 1) P) of the impulse response
//                       and of the partitions of its early part, each zero padded to L.
//   aug_conv_kernel     output block m: Y[k] = sum_p X_{m-p}[k] H_p[k] in ascending p, one thread per bin; the Hermitian half
//                       is mirrored into LDS, one inverse FFT, the last P points are y[m P .. (m + 1) P).  The early part goes
//                       the same way; its block is squared and summed instead of stored.
//   aug_sumsq_kernel    partial sums of x^2 per row and of the filled noise per descriptor.
//   aug_scale_kernel    p_before, p_sig and the scale a_d of every descriptor (one wave per row).
//   aug_mix_kernel      adds the scaled noises to y in descriptor order, partial sums of y^2.
//   aug_gain_kernel     g per row.     aug_out_kernel   the shifted, scaled, optionally quantised output and the clipped counts.
// Every sum of squares is accumulated in fp64 over chunks of 4096 samples counted from the row's (or the noise's) own first
// sample: within a chunk each thread sums its samples in index order, the threads are combined by a butterfly and the chunks are
// added in index order.  The scalars p, a_d and g stay fp64 and each sample operation rounds once to fp32.  The clipped count is
// an integer, added with integer atomics.  Nothing depends on the order in which workgroups run, and nothing a row reads lies
// past its own counts: its output is the same, bit for bit, whatever the batch, the row index, the padding and the other rows.
#include "spk_common.h"

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_P = 1024;                 // samples per block and taps per partition
constexpr int AUG_L = 2 * AUG_P;            // FFT size
constexpr int AUG_LOGL = 11;
constexpr int AUG_BINS = AUG_P + 1;         // stored bins of a spectrum
constexpr int AUG_CHUNK = 4096;             // samples per partial sum
constexpr int AUG_MAX_RIR = 32768;
constexpr int AUG_MAX_EARLY = 4 * AUG_P;

struct AugDims {
    int B, nd;
    long long Nmax, Mmax;        // Mmax >= max N + R - 1
    int nwx, np, nep;            // slots of a row: speech windows, impulse-response partitions, early partitions
    int nb;                      // output blocks of a row (ceil(Mmax / P))
    int ncp, nca;                // chunks: of the power sums (rows and descriptors), of y
};

inline long long aug_cdiv(long long a, long long b) { return (a + b - 1) / b; }

inline AugDims aug_dims(int B, long long Nmax, int Rmax, int Emax, long long Fmax, int nd) {
    AugDims d;
    d.B = B; d.nd = nd; d.Nmax = Nmax;
    d.Mmax = Nmax + (Rmax > 0 ? Rmax - 1 : 0);
    d.nwx = Rmax > 0 ? (int)aug_cdiv(Nmax, AUG_P) + 1 : 0;
    d.np = (int)aug_cdiv(Rmax, AUG_P);
    d.nep = (int)aug_cdiv(Emax, AUG_P);
    d.nb = (int)aug_cdiv(d.Mmax, AUG_P);
    d.ncp = (int)aug_cdiv(Nmax > Fmax ? Nmax : Fmax, AUG_CHUNK);
    d.nca = (int)aug_cdiv(d.Mmax, AUG_CHUNK);
    return d;
}
inline long long aug_spectra_elems(const AugDims& d) { return (long long)d.B * (d.nwx + d.np + d.nep) * AUG_BINS; }
// fp64 workspace: [B + nd][ncp] power partials, [B][nb] early partials, [B][nca] y partials, [B] p_before, [B] p_sig, [B] g, [nd] a
inline long long aug_off_sig(const AugDims& d) { return (long long)(d.B + d.nd) * d.ncp; }
inline long long aug_off_after(const AugDims& d) { return aug_off_sig(d) + (long long)d.B * d.nb; }
inline long long aug_off_pb(const AugDims& d) { return aug_off_after(d) + (long long)d.B * d.nca; }
inline long long aug_f64_elems(const AugDims& d) { return aug_off_pb(d) + 3ll * d.B + d.nd; }

struct AugArgs {
    const float* wave;           // [B][Nmax]
    const int* nsamp;            // [B]
    const float* rir_pool;
    const long long* rir_off;    // [B]
    const int* rir_row;          // [B][4]: R (0: none), peak s, early start e0, early length E
    const float* noise_pool;
    const int* desc_ptr;         // [B + 1]
    const long long* desc_off;   // [nd]
    const int* desc_len;         // [nd][3]: raw length, filled length, start sample
    const double* desc_snr;      // [nd] dB
    const float2* twiddle;       // [L / 2] exp(-2 pi i k / L)
    float2* spectra;             // [B][nwx + np + nep][BINS]
    float* y;                    // [B][Mmax]
    double* part_pow;            // [B + nd][ncp]
    double* part_sig;            // [B][nb]
    double* part_after;          // [B][nca]
    double* p_before;            // [B]
    double* p_sig;               // [B]
    double* gain;                // [B]
    double* scale;               // [nd]
    float* out;                  // [B][Nmax]
    unsigned long long* clipped; // [B]
    long long pool_len, noise_len;
    int Rmax, Emax, quantize;
    AugDims d;
};

struct AugRow {
    int N, R, s, e0, E;
    const float* h;
};

// the row's counts, clamped to what the launch was sized for (a table that is what the host builds is never clamped)
__device__ inline AugRow aug_row(const AugArgs& a, int b) {
    AugRow r;
    r.N = (int)min((long long)max(a.nsamp[b], 0), a.d.Nmax);
    r.R = min(max(a.rir_row[4 * b], 0), a.Rmax);
    long long off = a.rir_off[b];
    if (off < 0 || off + r.R > a.pool_len) r.R = 0;
    r.h = a.rir_pool + (r.R > 0 ? off : 0);
    r.s = r.R > 0 ? min(max(a.rir_row[4 * b + 1], 0), r.R - 1) : 0;
    r.e0 = r.R > 0 ? min(max(a.rir_row[4 * b + 2], 0), r.R - 1) : 0;
    r.E = r.R > 0 ? min(min(max(a.rir_row[4 * b + 3], 1), a.Emax), r.R - r.e0) : 0;
    return r;
}

// in-place radix-2 FFT of L points in LDS (decimation in time: the input is stored bit-reversed), all 256 threads
__device__ inline void aug_fft(float2* z, const float2* tw, int tid) {
    for (int st = 0; st < AUG_LOGL; ++st) {
        const int half = 1 << st;
#pragma unroll
        for (int c = 0; c < AUG_L / 2 / AUG_THREADS; ++c) {
            const int k = tid + c * AUG_THREADS;
            const int pos = k & (half - 1);
            const int i0 = ((k >> st) << (st + 1)) + pos, i1 = i0 + half;
            const float2 w = tw[pos << (AUG_LOGL - 1 - st)];
            const float2 u = z[i0], v = z[i1];
            const float2 bv = make_float2(v.x * w.x - v.y * w.y, v.x * w.y + v.y * w.x);
            z[i0] = make_float2(u.x + bv.x, u.y + bv.y);
            z[i1] = make_float2(u.x - bv.x, u.y - bv.y);
        }
        __syncthreads();
    }
}

__device__ inline int aug_brev(int n) { return (int)(__brev((unsigned)n) >> (32 - AUG_LOGL)); }

// sum over the workgroup in a fixed order: butterfly within a wave, then the four waves in index order
__device__ inline double aug_block_sum(double v, double* red, int tid) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// sum of n partials in a fixed order by one wave: lane l takes l, l + 64, .., then a butterfly
__device__ inline double aug_wave_total(const double* p, int n, int lane) {
    double v = 0.0;
    for (int i = lane; i < n; i += 64) v += p[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(AUG_THREADS) void aug_spectra_kernel(AugArgs a) {
    __shared__ float2 z[AUG_L];
    __shared__ float2 tw[AUG_L / 2];
    const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
    const AugRow r = aug_row(a, b);
    if (r.R == 0) return;                                  // block-uniform, as every return below
    const int nwx = (r.N + AUG_P - 1) / AUG_P + 1;
    const float* src;
    int lo, hi, base;                                      // value n of the FFT input is src[base + n] for lo <= base + n < hi
    int nlim;                                              // .. and n < nlim
    if (j < a.d.nwx) {
        if (j >= nwx) return;
        src = a.wave + (size_t)b * a.d.Nmax; base = (j - 1) * AUG_P; lo = 0; hi = r.N; nlim = AUG_L;
    } else if (j < a.d.nwx + a.d.np) {
        const int p = j - a.d.nwx;
        if (p * AUG_P >= r.R) return;
        src = r.h; base = p * AUG_P; lo = 0; hi = r.R; nlim = AUG_P;
    } else {
        const int p = j - a.d.nwx - a.d.np;
        if (p * AUG_P >= r.E) return;
        src = r.h + r.e0; base = p * AUG_P; lo = 0; hi = r.E; nlim = AUG_P;
    }
    for (int k = tid; k < AUG_L / 2; k += AUG_THREADS) tw[k] = a.twiddle[k];
    for (int n = tid; n < AUG_L; n += AUG_THREADS) {
        const int i = base + n;
        const float v = (n < nlim && i >= lo && i < hi) ? src[i] : 0.f;
        z[aug_brev(n)] = make_float2(v, 0.f);
    }
    __syncthreads();
    aug_fft(z, tw, tid);
    float2* dst = a.spectra + ((size_t)b * (a.d.nwx + a.d.np + a.d.nep) + j) * AUG_BINS;
    for (int k = tid; k < AUG_BINS; k += AUG_THREADS) dst[k] = z[k];
}

// sum_p X_{m-p}[k] H_p[k] over the partitions p in [p_lo, p_hi], ascending, mirrored into z (bit-reversed, conjugated: the forward
// FFT of the conjugate spectrum is the conjugate of the inverse FFT, and only the real part is kept)
__device__ inline void aug_mac(const float2* X, const float2* H, int m, int p_lo, int p_hi, float2* z, int tid) {
    float2 acc[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) acc[c] = make_float2(0.f, 0.f);
    for (int p = p_lo; p <= p_hi; ++p) {
        const float2* xs = X + (size_t)(m - p) * AUG_BINS;
        const float2* hs = H + (size_t)p * AUG_BINS;
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const int k = tid + c * AUG_THREADS;
            if (k < AUG_BINS) {
                const float2 x = xs[k], h = hs[k];
                acc[c].x = fmaf(x.x, h.x, acc[c].x);
                acc[c].x = fmaf(-x.y, h.y, acc[c].x);
                acc[c].y = fmaf(x.x, h.y, acc[c].y);
                acc[c].y = fmaf(x.y, h.x, acc[c].y);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const int k = tid + c * AUG_THREADS;
        if (k < AUG_BINS) {
            z[aug_brev(k)] = make_float2(acc[c].x, -acc[c].y);
            if (k > 0 && k < AUG_P) z[aug_brev(AUG_L - k)] = acc[c];
        }
    }
}

__global__ __launch_bounds__(AUG_THREADS) void aug_conv_kernel(AugArgs a) {
    __shared__ float2 z[AUG_L];
    __shared__ float2 tw[AUG_L / 2];
    __shared__ double red[4];
    const int b = blockIdx.y, m = blockIdx.x, tid = threadIdx.x;
    const AugRow r = aug_row(a, b);
    if (r.R == 0) return;
    const int M = r.N + r.R - 1;
    if (m * AUG_P >= M) return;
    const int nwx = (r.N + AUG_P - 1) / AUG_P + 1;
    const int np = (r.R + AUG_P - 1) / AUG_P, nep = (r.E + AUG_P - 1) / AUG_P;
    const float2* X = a.spectra + (size_t)b * (a.d.nwx + a.d.np + a.d.nep) * AUG_BINS;
    const float2* H = X + (size_t)a.d.nwx * AUG_BINS;
    const float2* He = H + (size_t)a.d.np * AUG_BINS;
    for (int k = tid; k < AUG_L / 2; k += AUG_THREADS) tw[k] = a.twiddle[k];
    const int p_lo = max(0, m - (nwx - 1));
    aug_mac(X, H, m, p_lo, min(np - 1, m), z, tid);
    __syncthreads();
    aug_fft(z, tw, tid);
    float* y = a.y + (size_t)b * a.d.Mmax;
    for (int i = tid; i < AUG_P; i += AUG_THREADS)
        if (m * AUG_P + i < M) y[m * AUG_P + i] = z[AUG_P + i].x * (1.f / AUG_L);
    // the early part: x * h_early has N + E - 1 samples; only their squares are needed
    const int Me = r.N + r.E - 1;
    if (m * AUG_P >= Me) return;
    __syncthreads();
    aug_mac(X, He, m, p_lo, min(nep - 1, m), z, tid);
    __syncthreads();
    aug_fft(z, tw, tid);
    double s = 0.0;
    for (int i = tid; i < AUG_P; i += AUG_THREADS)
        if (m * AUG_P + i < Me) {
            const double v = (double)(z[AUG_P + i].x * (1.f / AUG_L));
            s = fma(v, v, s);
        }
    s = aug_block_sum(s, red, tid);
    if (tid == 0) a.part_sig[(size_t)b * a.d.nb + m] = s;
}

// job < B: sum of x^2 of row `job`; job >= B: sum of the filled noise of descriptor job - B; chunk blockIdx.x
__global__ __launch_bounds__(AUG_THREADS) void aug_sumsq_kernel(AugArgs a) {
    __shared__ double red[4];
    const int job = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const float* src;
    int len, raw;
    if (job < a.d.B) {
        src = a.wave + (size_t)job * a.d.Nmax;
        len = raw = (int)min((long long)max(a.nsamp[job], 0), a.d.Nmax);
    } else {
        const int d = job - a.d.B;
        const long long off = a.desc_off[d];
        raw = a.desc_len[3 * d];
        len = a.desc_len[3 * d + 1];
        if (raw < 1 || off < 0 || off + raw > a.noise_len) return;
        src = a.noise_pool + off;
    }
    const long long i0 = (long long)c * AUG_CHUNK;
    if (i0 >= len) return;
    double s = 0.0;
    for (int k = tid; k < AUG_CHUNK && i0 + k < len; k += AUG_THREADS) {
        const long long i = i0 + k;
        const double v = (double)src[i < raw ? i : i % raw];
        s = fma(v, v, s);
    }
    s = aug_block_sum(s, red, tid);
    if (tid == 0) a.part_pow[(size_t)job * a.d.ncp + c] = s;
}

// one wave per row: p_before, p_sig and the scale of each of the row's descriptors
__global__ __launch_bounds__(64) void aug_scale_kernel(AugArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const AugRow r = aug_row(a, b);
    const double pb = r.N > 0 ? aug_wave_total(a.part_pow + (size_t)b * a.d.ncp, (r.N + AUG_CHUNK - 1) / AUG_CHUNK, lane) / (double)r.N : 0.0;
    double ps = pb;
    if (r.R > 0) {
        const int Me = r.N + r.E - 1;
        ps = aug_wave_total(a.part_sig + (size_t)b * a.d.nb, (Me + AUG_P - 1) / AUG_P, lane) / (double)Me;
    }
    if (lane == 0) {
        a.p_before[b] = pb;
        a.p_sig[b] = ps;
    }
    for (int d = a.desc_ptr[b]; d < a.desc_ptr[b + 1]; ++d) {
        const int fill = a.desc_len[3 * d + 1];
        const int nc = min((fill + AUG_CHUNK - 1) / AUG_CHUNK, a.d.ncp);
        const double q = aug_wave_total(a.part_pow + (size_t)(a.d.B + d) * a.d.ncp, nc, lane) / (double)fill;
        if (lane == 0) a.scale[d] = sqrt(pow(10.0, -a.desc_snr[d] / 10.0) * ps / q);
    }
}

__global__ __launch_bounds__(AUG_THREADS) void aug_mix_kernel(AugArgs a) {
    __shared__ double red[4];
    const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
    const AugRow r = aug_row(a, b);
    const int M = r.R > 0 ? r.N + r.R - 1 : r.N;
    const int i0 = c * AUG_CHUNK;
    if (i0 >= M) return;
    float* y = a.y + (size_t)b * a.d.Mmax;
    const float* x = a.wave + (size_t)b * a.d.Nmax;
    const int d0 = a.desc_ptr[b], d1 = a.desc_ptr[b + 1];
    double s = 0.0;
    for (int k = tid; k < AUG_CHUNK && i0 + k < M; k += AUG_THREADS) {
        const int i = i0 + k;
        float v = r.R > 0 ? y[i] : x[i];
        for (int d = d0; d < d1; ++d) {
            const int raw = a.desc_len[3 * d], fill = a.desc_len[3 * d + 1];
            const int t = i - a.desc_len[3 * d + 2];
            const long long off = a.desc_off[d];
            if (t >= 0 && t < fill && raw >= 1 && off >= 0 && off + raw <= a.noise_len) {
                const float nv = a.noise_pool[off + (t < raw ? t : t % raw)];
                v = (float)fma(a.scale[d], (double)nv, (double)v);
            }
        }
        y[i] = v;
        s = fma((double)v, (double)v, s);
    }
    s = aug_block_sum(s, red, tid);
    if (tid == 0) a.part_after[(size_t)b * a.d.nca + c] = s;
}

__global__ __launch_bounds__(64) void aug_gain_kernel(AugArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const AugRow r = aug_row(a, b);
    const int M = r.R > 0 ? r.N + r.R - 1 : r.N;
    const double tot = aug_wave_total(a.part_after + (size_t)b * a.d.nca, (M + AUG_CHUNK - 1) / AUG_CHUNK, lane);
    if (lane != 0) return;
    const bool plain = r.R == 0 && a.desc_ptr[b + 1] == a.desc_ptr[b];
    // an untouched row is returned as it came; a silent result (p_after == 0) stays silent
    a.gain[b] = (plain || !(tot > 0.0)) ? 1.0 : sqrt(a.p_before[b] / (tot / (double)M));
}

__global__ __launch_bounds__(AUG_THREADS) void aug_out_kernel(AugArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const AugRow r = aug_row(a, b);
    const float* y = a.y + (size_t)b * a.d.Mmax;
    float* o = a.out + (size_t)b * a.d.Nmax;
    const double g = a.gain[b];
    const long long j0 = (long long)blockIdx.x * AUG_CHUNK;
    int nclip = 0;
    for (int k = tid; k < AUG_CHUNK && j0 + k < a.d.Nmax; k += AUG_THREADS) {
        const long long j = j0 + k;
        float v = 0.f;
        if (j < r.N) {
            v = (float)(g * (double)y[j + r.s]);
            if (a.quantize) {
                v = truncf(v);
                if (v > 32767.f) { v = 32767.f; ++nclip; }
                else if (v < -32768.f) { v = -32768.f; ++nclip; }
            }
        }
        o[j] = v;
    }
    if (!a.quantize) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nclip += __shfl_xor(nclip, off, 64);
    if ((tid & 63) == 0 && nclip > 0) atomicAdd(a.clipped + b, (unsigned long long)nclip);      // integers: any order, same sum
}

}  // namespace

// ---- exports (include/spkhip.h) ----
extern "C" int spk_augment_max_rir() { return AUG_MAX_RIR; }
extern "C" int spk_augment_max_early() { return AUG_MAX_EARLY; }

extern "C" int spk_augment_workspace(int B, long long Nmax, int Rmax, int Emax, long long Fmax, int nd, long long* sizes) {
    SPK_REQUIRE(sizes, "spk_augment_workspace: null pointer");
    SPK_REQUIRE(B > 0 && B <= 65535 && Nmax > 0 && Nmax < (1ll << 30) && Rmax >= 0 && Rmax <= AUG_MAX_RIR && Emax >= 0 &&
                Emax <= AUG_MAX_EARLY && Emax <= Rmax && Fmax >= 0 && Fmax < (1ll << 30) && nd >= 0,
                "spk_augment_workspace: B=%d Nmax=%lld Rmax=%d (<= %d) Emax=%d (<= %d) Fmax=%lld nd=%d", B, Nmax, Rmax, AUG_MAX_RIR,
                Emax, AUG_MAX_EARLY, Fmax, nd);
    const AugDims d = aug_dims(B, Nmax, Rmax, Emax, Fmax, nd);
    sizes[0] = aug_spectra_elems(d);        // float2
    sizes[1] = (long long)B * d.Mmax;       // float
    sizes[2] = aug_f64_elems(d);            // double
    return 0;
}

extern "C" int spk_augment_fwd(const float* wave, const int* nsamp, int B, long long Nmax, const float* rir_pool, long long rir_pool_len,
                               const long long* rir_off, const int* rir_row, int Rmax, int Emax, const float* noise_pool,
                               long long noise_pool_len, const int* desc_ptr, const long long* desc_off, const int* desc_len,
                               const double* desc_snr, int nd, long long Fmax, const float* twiddle, float* spectra, float* y,
                               double* work, int quantize, float* out, unsigned long long* clipped, void* stream) {
    long long sizes[3];
    if (spk_augment_workspace(B, Nmax, Rmax, Emax, Fmax, nd, sizes) != 0) return -1;
    SPK_REQUIRE(wave && nsamp && rir_off && rir_row && desc_ptr && y && work && out && clipped, "spk_augment_fwd: null pointer");
    SPK_REQUIRE(Rmax == 0 || (rir_pool && twiddle && spectra && rir_pool_len > 0 && Emax > 0),
                "spk_augment_fwd: impulse responses need their pool, the twiddles and the spectrum workspace");
    SPK_REQUIRE(nd == 0 || (noise_pool && desc_off && desc_len && desc_snr && noise_pool_len > 0),
                "spk_augment_fwd: %d descriptors need the noise pool and the descriptor tables", nd);
    const AugDims d = aug_dims(B, Nmax, Rmax, Emax, Fmax, nd);
    SPK_REQUIRE(d.Mmax < (1ll << 30) && (long long)B + nd <= 65535, "spk_augment_fwd: Mmax=%lld (< 2^30), B + descriptors = %lld (<= 65535)",
                d.Mmax, (long long)B + nd);
    AugArgs a;
    a.wave = wave; a.nsamp = nsamp; a.rir_pool = rir_pool; a.rir_off = rir_off; a.rir_row = rir_row; a.noise_pool = noise_pool;
    a.desc_ptr = desc_ptr; a.desc_off = desc_off; a.desc_len = desc_len; a.desc_snr = desc_snr; a.twiddle = (const float2*)twiddle;
    a.spectra = (float2*)spectra; a.y = y;
    a.part_pow = work; a.part_sig = work + aug_off_sig(d); a.part_after = work + aug_off_after(d);
    a.p_before = work + aug_off_pb(d); a.p_sig = a.p_before + B; a.gain = a.p_sig + B; a.scale = a.gain + B;
    a.out = out; a.clipped = clipped; a.pool_len = rir_pool_len; a.noise_len = noise_pool_len;
    a.Rmax = Rmax; a.Emax = Emax; a.quantize = quantize ? 1 : 0; a.d = d;
    hipStream_t st = (hipStream_t)stream;
    if (Rmax > 0) {
        hipLaunchKernelGGL(aug_spectra_kernel, dim3((unsigned)(d.nwx + d.np + d.nep), (unsigned)B), dim3(AUG_THREADS), 0, st, a);
        SPK_LAUNCH_CHECK("spk_augment_fwd");
        hipLaunchKernelGGL(aug_conv_kernel, dim3((unsigned)d.nb, (unsigned)B), dim3(AUG_THREADS), 0, st, a);
        SPK_LAUNCH_CHECK("spk_augment_fwd");
    }
    hipLaunchKernelGGL(aug_sumsq_kernel, dim3((unsigned)d.ncp, (unsigned)(B + nd)), dim3(AUG_THREADS), 0, st, a);
    SPK_LAUNCH_CHECK("spk_augment_fwd");
    hipLaunchKernelGGL(aug_scale_kernel, dim3((unsigned)B), dim3(64), 0, st, a);
    SPK_LAUNCH_CHECK("spk_augment_fwd");
    hipLaunchKernelGGL(aug_mix_kernel, dim3((unsigned)d.nca, (unsigned)B), dim3(AUG_THREADS), 0, st, a);
    SPK_LAUNCH_CHECK("spk_augment_fwd");
    hipLaunchKernelGGL(aug_gain_kernel, dim3((unsigned)B), dim3(64), 0, st, a);
    SPK_LAUNCH_CHECK("spk_augment_fwd");
    hipLaunchKernelGGL(aug_out_kernel, dim3((unsigned)aug_cdiv(Nmax, AUG_CHUNK), (unsigned)B), dim3(AUG_THREADS), 0, st, a);
    SPK_LAUNCH_CHECK("spk_augment_fwd");
    return 0;
}
