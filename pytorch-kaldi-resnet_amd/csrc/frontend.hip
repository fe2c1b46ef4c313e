// Kaldi-compatible feature front end (compute-fbank-feats, compute-vad, apply-cmvn-sliding --norm-vars=false --center=true,
// select-voiced-frames; reference: feature_pre.sh:77-104 and local/nnet3/xvector/prepare_feats_for_egs.sh:68-70, the fbank as
// restated in kaldi.py:42-188,363-527).  Semantics: DESIGN.md section "Feature front end".
//
// spk_fbank_fwd: one workgroup of 4 waves per (utterance, tile of FT consecutive frames).  The tile's waveform span is staged
// once in LDS (frames overlap by L - S samples; the reflection of snip_edges=false is applied on load).  Each wave takes one frame
// per round: dither, explicit fp32 DC removal, raw log energy, pre-emphasis, window, zero pad to P, a complex radix-2 FFT of
// M = P/2 points of the even/odd samples plus the real-split post-pass, power, sparse mel sum, log.  The log-mel values of the
// tile are transposed through LDS and stored as runs of FT frames per mel row ([B][F][Tcap], time innermost).
// The host builds the window, the twiddles exp(-2 pi i k / P) and the mel weights in fp64 and passes them rounded to fp32.
//
// spk_mfcc_fwd (compute-mfcc-feats; reference: local/make_mfcc.sh:107,126 and kaldi.py:550-650): the same
// kernel template, instantiated with the cepstral epilogue.  The frame pipeline up to the log-mel values is the fbank's, operation
// for operation; a wave then keeps its F log-mels in its own FFT buffer (free once the real split has been read), and lane k sums
// row k of the DCT (staged once per workgroup in LDS, row stride odd) over them in ascending order, applies the lifter, and the
// energy / HTK order rules pick the output row.  The tile has C + 1 rows: the cepstra, then the log energies.
//
// spk_fbank_span_fwd / spk_mfcc_span_fwd (training from audio; they replace the feature directories of the
// reference's feature_pre.sh:178-196 and prepare_feats_for_egs.sh:68-71): the same template again, for rows that hold a span of
// samples of an utterance; a frame is computed from its position in the utterance, so column j is bit for bit column frame0 + j of
// the whole-utterance launch.  spk_pcm16_to_f32 converts the 16-bit samples as read from the file.
//
// Host side: the four exports put their parameters into one FeCall and go through fe_launch<MFCC, SPAN>, which holds every
// argument check, the tile lookup, the kernel arguments and the launch once; what only some forms need sits under `if constexpr`.
#include <type_traits>

#include "spk_common.h"

namespace {

constexpr int FE_THREADS = 256;   // 4 waves, one frame each per round
constexpr int FE_WAVES = 4;
constexpr float FE_FLT_EPS = 1.1920928955078125e-07f;
constexpr float FE_LOG_EPS = -15.942385152878742f;     // log(FLT_EPSILON), correctly rounded (logf may be 1 ulp off)

__device__ inline float fe_log_floor_eps(float v) { return v > FE_FLT_EPS ? logf(v) : FE_LOG_EPS; }

// counter-based N(0,1) draw keyed by (seed, utt_id, frame, position): splitmix64 finaliser + Box-Muller
__host__ __device__ inline unsigned long long fe_mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
__device__ inline unsigned long long fe_utt_key(unsigned long long seed, long long utt_id) {
    return fe_mix64(seed * 0x9e3779b97f4a7c15ULL ^ fe_mix64((unsigned long long)utt_id + 0x632be59bd9b4e019ULL));
}
__device__ inline float fe_gauss(unsigned long long key, int t, int j) {
    const unsigned long long ctr = ((unsigned long long)(unsigned)t << 20) | (unsigned)j;     // j < P <= 1024
    const unsigned long long h = fe_mix64(key + ctr * 0xd1b54a32d192ed03ULL);
    const float u1 = (float)((unsigned)(h >> 40) + 1u) * 0x1p-24f;                           // (0, 1]
    const float u2 = (float)((unsigned)(h >> 8) & 0xffffffu) * 0x1p-24f;                      // [0, 1)
    return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// the frame buffers fb / z belong to one wave: its lanes exchange data through LDS with a wave-local barrier (LDS operations of a
// wave complete in order; the fences keep the compiler from moving LDS accesses across it), not a workgroup barrier
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ inline int fe_frames(long long N, int L, int S, int snip) {
    if (snip) return N < L ? 0 : (int)(1 + (N - L) / S);
    return (int)((N + S / 2) / S);
}

struct FbankArgs {
    const float* wave;
    const int* nsamp;
    const long long* utt_ids;
    long long Nmax;
    const float* window;      // [L]
    const float* twiddle;     // [M][2] exp(-2 pi i k / P)
    const float* mel_w;       // concatenated weights of the filters
    const int* mel_lo;        // [F] first FFT bin of filter m
    const int* mel_off;       // [F + 1] offsets into mel_w (filter m covers bins mel_lo[m] .. + mel_off[m+1]-mel_off[m])
    int L, S, P, logM, F, snip, FT, span;
    float dither, preemph, log_floor;   // log_floor: -inf when energy_floor == 0
    int remove_dc;
    unsigned long long seed;
    float* feats;     // [B][F][Tcap]
    float* loge;      // [B][Tcap]
    int* T_out;       // [B]
    int Tcap;
    // cepstral epilogue (the MFCC instantiation only)
    const float* dct;         // [C][F] DCT-II rows, row 0 = sqrt(1 / F)
    const float* lifter;      // [C] 1 + Q / 2 sin(pi k / Q) (ones for Q == 0)
    int C, Fp, use_energy, htk;     // Fp: row stride of the DCT copy in LDS (odd)
};

// the span form (spk_fbank_span_fwd, spk_mfcc_span_fwd): row b of `wave` holds samples [first[b], first[b] + nsamp[b]) of an
// utterance of total[b] samples, and the launch computes frames frame0[b] .. frame0[b] + nframes[b] - 1 of THAT utterance.  The
// fields of FbankArgs keep their place, so the kernel arguments of the whole-utterance kernels are what they were, and fe_launch
// fills them by the same lines for all four kernels
struct SpanArgs : FbankArgs {
    const long long* first;   // [B] sample of the utterance that row b starts with
    const long long* total;   // [B] samples of the utterance
    const int* frame0;        // [B] first frame computed (column 0 of the output)
    const int* nframes;       // [B] frames computed (clipped to the utterance's frame count)
};

// one tile of one utterance.  MFCC = false: the log-mel tile (fbank_kernel); true: its DCT, liftered (mfcc_kernel).  R output
// rows of a.feats.  SPAN: A is SpanArgs, the tile's frames are frames f0 + t of the utterance (reflection about 0 and total[b],
// dither keyed by the absolute frame) and column t of the output is frame f0 + t; per frame the same operations in the same order
template <bool MFCC, bool SPAN = false, class A = FbankArgs>
__device__ __forceinline__ void frontend_tile(const A& a) {
    extern __shared__ float fe_lds[];
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * a.FT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    long long N, first = 0, navail = 0;     // N: samples of the utterance; the row holds [first, first + navail) of them
    int T, f0 = 0;                          // T: frames this row computes, f0: the frame of the utterance that column 0 is
    if constexpr (SPAN) {
        N = a.total[b];
        first = a.first[b];
        navail = min((long long)a.nsamp[b], a.Nmax);
        f0 = a.frame0[b];
        const int Tu = N > 0 ? fe_frames(N, a.L, a.S, a.snip) : 0;
        T = (navail > 0 && f0 >= 0) ? max(min(a.nframes[b], Tu - f0), 0) : 0;
    } else {
        N = min((long long)a.nsamp[b], a.Nmax);
        T = N > 0 ? fe_frames(N, a.L, a.S, a.snip) : 0;
    }
    if (blockIdx.x == 0 && tid == 0) a.T_out[b] = T;
    const int R = MFCC ? a.C : a.F;
    float* frow = a.feats + (size_t)b * R * a.Tcap;
    const int nt = min(a.FT, a.Tcap - t0);
    if (t0 >= T) {        // tile entirely past the utterance: zeros only (block-uniform)
        for (int i = tid; i < R * nt; i += FE_THREADS) frow[(size_t)(i / nt) * a.Tcap + t0 + i % nt] = 0.f;
        for (int i = tid; i < nt; i += FE_THREADS) a.loge[(size_t)b * a.Tcap + t0 + i] = 0.f;
        return;
    }
    const int M = a.P >> 1;
    // LDS: the float2 FFT buffers first (8-byte aligned whatever the span length), then the per-wave frame buffers, the span
    float2* zbuf = (float2*)fe_lds;                         // [4][M]   FFT
    float* fbuf = (float*)(zbuf + FE_WAVES * M);            // [4][P]   frame samples, then power spectrum
    float* span = fbuf + FE_WAVES * a.P;                    // [span]
    float* otile = span + a.span;                           // [R + 1][FT]: feature rows, then the log energies
    float* dct = otile + (R + 1) * a.FT;                    // [C][Fp] (MFCC only)
    const float* wv = a.wave + (size_t)b * a.Nmax;
    const long long s0 = ((long long)t0 + f0) * a.S - (a.snip ? 0 : (a.L / 2 - a.S / 2));
    for (int i = tid; i < a.span; i += FE_THREADS) {
        long long s = s0 + i;
        if (s < 0) s = -s - 1;                      // reflected once (snip_edges = false)
        if (s >= N) s = 2 * N - 1 - s;
        if constexpr (SPAN) {                       // the utterance's sample s lies at s - first of the row; a sample outside the
            s -= first;                             // row is only reached for frames the host wrapper refuses: stay in bounds
            s = s < 0 ? 0 : (s >= navail ? navail - 1 : s);
        } else {
            s = s < 0 ? 0 : (s >= N ? N - 1 : s);   // only reached for N < L, which the API refuses: stay in bounds
        }
        span[i] = wv[s];
    }
    if constexpr (MFCC)
        for (int i = tid; i < a.C * a.F; i += FE_THREADS) dct[(i / a.F) * a.Fp + i % a.F] = a.dct[i];
    const unsigned long long key = a.dither != 0.f ? fe_utt_key(a.seed, a.utt_ids[b]) : 0ull;
    float* fb = fbuf + w * a.P;
    float2* z = zbuf + w * M;
    __syncthreads();
    for (int r = 0; r < a.FT; r += FE_WAVES) {
        const int tl = r + w;                       // frame within the tile
        const int t = t0 + tl;
        if (t >= T) break;                          // wave-uniform: frames past the utterance are not computed (stored as 0)
        const float* x0 = span + tl * a.S;
        // 1-2. dither, frame mean (explicit fp32 subtraction: DESIGN.md "Feature front end")
        float sum = 0.f;
        for (int j = lane; j < a.L; j += 64) {
            float v = x0[j];
            if (a.dither != 0.f) v = fmaf(a.dither, fe_gauss(key, t + f0, j), v);      // keyed by the frame of the utterance
            fb[j] = v;
            sum += v;
        }
        const float mean = a.remove_dc ? wave_sum(sum) / (float)a.L : 0.f;
        // 3. raw log energy
        float e = 0.f;
        for (int j = lane; j < a.L; j += 64) {
            const float v = fb[j] - mean;
            fb[j] = v;
            e = fmaf(v, v, e);
        }
        e = wave_sum(e);
        wave_lds_sync();
        // 4-6. pre-emphasis, window, zero pad; z[n] = y[2n] + i y[2n+1], stored bit-reversed for the in-place radix-2 FFT
        for (int n = lane; n < M; n += 64) {
            float y[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int j = 2 * n + q;
                y[q] = 0.f;
                if (j < a.L) y[q] = (fb[j] - a.preemph * fb[j > 0 ? j - 1 : 0]) * a.window[j];
            }
            const int br = (int)(__brev((unsigned)n) >> (32 - a.logM));
            z[br] = make_float2(y[0], y[1]);
        }
        wave_lds_sync();
        // 7. FFT of M points (decimation in time), then the real split: X[k] = E[k] + W_P^k O[k]
        for (int st = 0; st < a.logM; ++st) {
            const int half = 1 << st;
            for (int k = lane; k < (M >> 1); k += 64) {
                const int pos = k & (half - 1);
                const int i0 = ((k >> st) << (st + 1)) + pos, i1 = i0 + half;
                const float2 tw = ((const float2*)a.twiddle)[pos << (a.logM - st)];
                const float2 u = z[i0], v = z[i1];
                const float2 bv = make_float2(v.x * tw.x - v.y * tw.y, v.x * tw.y + v.y * tw.x);
                z[i0] = make_float2(u.x + bv.x, u.y + bv.y);
                z[i1] = make_float2(u.x - bv.x, u.y - bv.y);
            }
            wave_lds_sync();
        }
        for (int k = lane; k < M; k += 64) {
            const float2 zk = z[k], zc = z[(M - k) & (M - 1)];
            const float er = 0.5f * (zk.x + zc.x), ei = 0.5f * (zk.y - zc.y);     // (Z[k] + conj Z[M-k]) / 2
            const float orr = 0.5f * (zk.y + zc.y), oi = -0.5f * (zk.x - zc.x);   // (Z[k] - conj Z[M-k]) / 2i
            const float2 tw = ((const float2*)a.twiddle)[k];
            const float xr = er + (orr * tw.x - oi * tw.y), xi = ei + (orr * tw.y + oi * tw.x);
            fb[k] = xr * xr + xi * xi;
        }
        wave_lds_sync();
        // mel filterbank (sparse: each filter's bin range), log
        for (int m = lane; m < a.F; m += 64) {
            const int lo = a.mel_lo[m], o0 = a.mel_off[m], cnt = a.mel_off[m + 1] - o0;
            float s = 0.f;
            for (int q = 0; q < cnt; ++q) s = fmaf(a.mel_w[o0 + q], fb[lo + q], s);
            if constexpr (MFCC) ((float*)z)[m] = fe_log_floor_eps(s);      // z is free since the real split (F <= P floats)
            else otile[m * a.FT + tl] = fe_log_floor_eps(s);
        }
        const float le = fmaxf(fe_log_floor_eps(e), a.log_floor);
        if (lane == 0) otile[R * a.FT + tl] = le;
        wave_lds_sync();
        if constexpr (MFCC) {
            // cepstra: c[k] = sum_n D[k][n] lm[n] (n ascending), times the lifter; C0 replaced by the energy; HTK order: C0 last
            const float* lm = (const float*)z;
            for (int k = lane; k < a.C; k += 64) {
                const float* d = dct + k * a.Fp;
                float c = 0.f;
                int n = 0;
                for (; n + 8 <= a.F; n += 8) {      // eight LDS reads of each operand in flight, summed in the same order
                    float dv[8], lv[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        dv[q] = d[n + q];
                        lv[q] = lm[n + q];
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q) c = fmaf(dv[q], lv[q], c);
                }
                for (; n < a.F; ++n) c = fmaf(d[n], lm[n], c);
                c *= a.lifter[k];
                int row = k;
                if (k == 0 && a.use_energy) c = le;
                if (a.htk) {
                    row = k > 0 ? k - 1 : a.C - 1;
                    if (k == 0 && !a.use_energy) c *= 1.41421356237309505f;
                }
                otile[row * a.FT + tl] = c;
            }
            wave_lds_sync();        // the next round overwrites z
        }
    }
    __syncthreads();                                // the otile columns of every wave are complete
    // transposed store: each feature row gets a run of nt consecutive frames; zeros past T
    for (int i = tid; i < (R + 1) * nt; i += FE_THREADS) {
        const int m = i / nt, tl = i - m * nt, t = t0 + tl;
        const float v = t < T ? otile[m * a.FT + tl] : 0.f;
        if (m < R) frow[(size_t)m * a.Tcap + t] = v;
        else a.loge[(size_t)b * a.Tcap + t] = v;
    }
}

__global__ __launch_bounds__(FE_THREADS) void fbank_kernel(FbankArgs a) { frontend_tile<false>(a); }
__global__ __launch_bounds__(FE_THREADS) void mfcc_kernel(FbankArgs a) { frontend_tile<true>(a); }
__global__ __launch_bounds__(FE_THREADS) void fbank_span_kernel(SpanArgs a) { frontend_tile<false, true>(a); }
__global__ __launch_bounds__(FE_THREADS) void mfcc_span_kernel(SpanArgs a) { frontend_tile<true, true>(a); }

// 16-bit PCM as it lies in a WAV file -> float32 at int16 scale: out[b][s] = in[b][s] for s < count[b], 0 up to Nmax.  A thread
// converts 8 samples (one 16-byte load, two 16-byte stores) when the row pitch and the bases allow, else one at a time
__global__ __launch_bounds__(256) void pcm16_to_f32_kernel(const short* __restrict__ in, const int* __restrict__ count, long long Nmax,
                                                           float* __restrict__ out, int vec) {
    const int b = blockIdx.y;
    const long long n = min(max((long long)count[b], 0ll), Nmax);
    const short* src = in + (size_t)b * Nmax;
    float* dst = out + (size_t)b * Nmax;
    const long long s = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (s >= Nmax) return;
    if (vec && s + 8 <= n) {                        // vec: Nmax % 8 == 0 and both bases 16-byte aligned, so every row is
        const int4 q = *(const int4*)(src + s);
        const int v[4] = {q.x, q.y, q.z, q.w};
        float f[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = (float)(short)(v[i] & 0xffff);
            f[2 * i + 1] = (float)(short)(v[i] >> 16);
        }
        *(float4*)(dst + s) = make_float4(f[0], f[1], f[2], f[3]);
        *(float4*)(dst + s + 4) = make_float4(f[4], f[5], f[6], f[7]);
        return;
    }
    const long long e = min(s + 8, Nmax);
    for (long long i = s; i < e; ++i) dst[i] = i < n ? (float)src[i] : 0.f;
}

// the noise fbank_kernel adds (before scaling by dither) to frames frame0 .. frame0 + nframes - 1 of utterance utt_id
__global__ __launch_bounds__(256) void dither_noise_kernel(float* out, long long utt_id, unsigned long long seed, int frame0,
                                                           int nframes, int L) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)nframes * L) return;
    const int f = (int)(i / L), j = (int)(i % L);
    out[i] = fe_gauss(fe_utt_key(seed, utt_id), frame0 + f, j);
}

// compute-vad: one wave per utterance.  Mean log energy in fp64, decisions over the clipped context window, and the compaction
// list of voiced frames (ballot + prefix popcount, in frame order)
__global__ __launch_bounds__(64) void vad_kernel(const float* __restrict__ loge, const int* __restrict__ Tv, int Tcap, double thr0,
                                                 double mean_scale, int ctx, double prop, int* __restrict__ vad,
                                                 int* __restrict__ idx, int* __restrict__ count) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int T = min(max(Tv[b], 0), Tcap);
    const float* e = loge + (size_t)b * Tcap;
    double s = 0.0;
    for (int t = lane; t < T; t += 64) s += (double)e[t];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    const double thr = thr0 + (T > 0 ? mean_scale * (s / (double)T) : 0.0);
    int carry = 0;
    for (int t0 = 0; t0 < Tcap; t0 += 64) {
        const int t = t0 + lane;
        bool v = false;
        if (t < T) {
            int num = 0, den = 0;
            for (int t2 = max(t - ctx, 0); t2 <= min(t + ctx, T - 1); ++t2) {
                ++den;
                num += (double)e[t2] > thr;
            }
            v = (double)num >= (double)den * prop;
        }
        if (t < Tcap) vad[(size_t)b * Tcap + t] = v ? 1 : 0;
        const unsigned long long mask = __ballot(v);
        const int pos = carry + __popcll(mask & ((1ull << lane) - 1ull));
        if (v) idx[(size_t)b * Tcap + pos] = t;
        carry += __popcll(mask);
    }
    if (lane == 0) count[b] = carry;
}

// VAD decisions -> speech segments (the rule is in include/spkhip.h): one wave per row, one pass over the
// frames.  Per 64-frame chunk the wave takes the ballot of the voiced frames; run starts (v[t] && !v[t-1]) and run ends
// (!v[t] && v[t-1], the exclusive end of the run) are bits of two masks made from it and the last bit of the chunk before.  Every
// decision is local to a run start: the run end before it is the highest end bit below the lane (or the carry of earlier chunks),
// so the lane knows whether its run opens a segment; the start that opened the segment it closes is the highest opener bit below
// the lane (or the carry), so it knows the closed segment's extent and whether min_length keeps it; the output index is the
// count of kept segments so far plus a prefix popcount.  Starts and ends are frame numbers, so nothing but masks crosses lanes.
// The last segment is closed at T by lane 0.  A round is SEG_CHUNKS chunks: the loads of the next round are issued before the
// chunks of this one are looked at.
constexpr int SEG_CHUNKS = 8;

__device__ inline int seg_top(unsigned long long m) { return 63 - __clzll((long long)m); }     // highest set bit, m != 0

__global__ __launch_bounds__(64) void vad_segments_kernel(const int* __restrict__ vad, const int* __restrict__ Tv, int Tcap, int pad,
                                                          int gap, int minlen, int* __restrict__ seg, int Scap,
                                                          int* __restrict__ nseg) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int T = min(max(Tv[b], 0), Tcap);
    const int* v = vad + (size_t)b * Tcap;
    int* out = seg + (size_t)b * Scap * 2;
    const unsigned long long below = (1ull << lane) - 1ull;
    int last_end = -1;      // exclusive end of the last run that ended in an earlier chunk (-1: none yet)
    int open_t = -1;        // first frame of the run that opened the current segment (-1: no run yet)
    int nout = 0;           // segments kept so far
    unsigned long long pv = 0;      // v[t0 - 1]
    int w[SEG_CHUNKS], wn[SEG_CHUNKS];
#pragma unroll
    for (int u = 0; u < SEG_CHUNKS; ++u) {
        const int t = u * 64 + lane;
        wn[u] = t < T ? v[t] : 0;
    }
    for (int tb = 0; tb < T; tb += 64 * SEG_CHUNKS) {
#pragma unroll
        for (int u = 0; u < SEG_CHUNKS; ++u) {      // the next round's loads fly while this round's chunks are looked at
            w[u] = wn[u];
            const int t = tb + (SEG_CHUNKS + u) * 64 + lane;
            wn[u] = t < T ? v[t] : 0;
        }
#pragma unroll
        for (int u = 0; u < SEG_CHUNKS; ++u) {
            const int t0 = tb + u * 64;
            if (t0 < T) {       // wave-uniform
                const unsigned long long vm = __ballot(w[u] != 0);
                const unsigned long long prev = (vm << 1) | pv;
                const unsigned long long sm = vm & ~prev, em = ~vm & prev;
                const int t = t0 + lane;
                const unsigned long long eb = em & below;
                const int e_prev = eb ? t0 + seg_top(eb) : last_end;
                const bool first = e_prev < 0;                                       // run 0: nothing ended before it
                const int a = max(t - pad, 0);
                const int b_prev = (int)min((long long)e_prev + pad, (long long)T);  // unused for run 0
                const bool opener = ((sm >> lane) & 1ull) && (first || a - b_prev > gap);
                const unsigned long long om = __ballot(opener);
                const unsigned long long ob = om & below;
                const int a_open = max((ob ? t0 + seg_top(ob) : open_t) - pad, 0);
                const bool keep = opener && !first && b_prev - a_open >= minlen;
                const unsigned long long km = __ballot(keep);
                if (keep) {
                    const int i = nout + __popcll(km & below);
                    if (i < Scap) {
                        out[2 * (size_t)i] = a_open;
                        out[2 * (size_t)i + 1] = b_prev;
                    }
                }
                nout += __popcll(km);
                if (em) last_end = t0 + seg_top(em);
                if (om) open_t = t0 + seg_top(om);
                pv = vm >> 63;
            }
        }
    }
    if (lane == 0) {
        if (open_t >= 0) {      // the segment that is open at T; a run that reaches T (a multiple of 64) ends there
            const int a_open = max(open_t - pad, 0);
            const int b_last = (int)min((long long)(pv ? T : last_end) + pad, (long long)T);
            if (b_last - a_open >= minlen) {
                if (nout < Scap) {
                    out[2 * (size_t)nout] = a_open;
                    out[2 * (size_t)nout + 1] = b_last;
                }
                ++nout;
            }
        }
        nseg[b] = nout;
    }
}

// fp64 prefix sums of every (b, m) row over its T[b] frames: pre[row][0] = 0, pre[row][t + 1] = sum x[0..t]; one wave per row
__global__ __launch_bounds__(256) void cmn_prefix_kernel(const float* __restrict__ x, const int* __restrict__ Tv, int B, int F,
                                                         int Tcap, double* __restrict__ pre) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B * F) return;
    const int T = min(max(Tv[row / F], 0), Tcap);
    const float* xr = x + (size_t)row * Tcap;
    double* pr = pre + (size_t)row * (Tcap + 1);
    if (lane == 0) pr[0] = 0.0;
    double carry = 0.0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        double v = t < T ? (double)xr[t] : 0.0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double u = __shfl_up(v, off, 64);
            if (lane >= off) v += u;
        }
        if (t < T) pr[t + 1] = carry + v;
        carry += __shfl(v, 63, 64);
    }
}

// out[b][m][j] = x[b][m][t] - mean of the centred sliding window around t (W > 0; W == 0: no CMN), t = idx[b][j] (the j-th voiced
// frame; idx NULL: t = j), for j < count[b] (count NULL: T[b]); zero for count[b] <= j < Tout
__global__ __launch_bounds__(256) void cmn_select_kernel(const float* __restrict__ x, const int* __restrict__ Tv,
                                                         const int* __restrict__ idx, const int* __restrict__ count,
                                                         const double* __restrict__ pre, float* __restrict__ out, int F, int Tcap,
                                                         int Tout, int W, int nj) {
    const int row = blockIdx.x / nj;       // b * F + m
    const int j = (blockIdx.x - row * nj) * 256 + threadIdx.x;
    const int b = row / F;
    if (j >= Tout) return;
    const int T = min(max(Tv[b], 0), Tcap);
    const int n = count ? min(count[b], T) : T;
    float v = 0.f;
    if (j < n) {
        const int t = idx ? idx[(size_t)b * Tcap + j] : j;
        const float xv = x[(size_t)row * Tcap + t];
        if (W > 0) {
            int start = t - W / 2, end = start + W;
            if (start < 0) {
                end -= start;
                start = 0;
            }
            if (end > T) {
                start -= end - T;
                end = T;
                start = max(start, 0);
            }
            const double* pr = pre + (size_t)row * (Tcap + 1);
            const double mean = (pr[end] - pr[start]) / (double)(end - start);
            v = (float)((double)xv - mean);
        } else {
            v = xv;
        }
    }
    out[(size_t)row * Tout + j] = v;
}

int fe_lds_bytes(int FT, int L, int S, int P, int F) {
    const int span = (FT - 1) * S + L;
    return (FE_WAVES * P /* z */ + FE_WAVES * P /* fb */ + span + (F + 1) * FT) * 4;
}

// the MFCC tile: C + 1 output rows, and the DCT copy [C][F | 1] behind them (in long long: C * F of a refused call may be large)
long long fe_mfcc_lds_bytes(int FT, int L, int S, int P, int F, int C) {
    return (long long)fe_lds_bytes(FT, L, S, P, C) + (long long)C * (F | 1) * 4;
}

constexpr int FE_LDS_LIMIT = 64 * 1024;

// frames per workgroup tile: the largest of 32, 16, 8, 4 whose tile fits the LDS (0: none does)
template <bool MFCC>
int fe_tile_frames(int L, int S, int P, int F, int C) {
    for (int FT = 32; FT >= FE_WAVES; FT >>= 1)
        if ((MFCC ? fe_mfcc_lds_bytes(FT, L, S, P, F, C) : (long long)fe_lds_bytes(FT, L, S, P, F)) <= FE_LDS_LIMIT) return FT;
    return 0;
}

// everything a front-end call is given, in the order of the parameters of spk_mfcc_span_fwd (include/spkhip.h).  first, total,
// frame0 and nframes are null for the whole-utterance forms; dct, lifter, C, use_energy and htk_compat are empty for fbank
struct FeCall {
    const float* wave; const int* nsamp; const long long *first, *total; const int *frame0, *nframes; const long long* utt_ids;
    int B; long long Nmax;
    const float *window, *twiddle, *mel_w; const int *mel_lo, *mel_off; const float *dct, *lifter;
    int L, S, P, F, C, snip_edges; float dither, preemph; int remove_dc; float energy_floor; int use_energy, htk_compat;
    unsigned long long seed; float *feats, *log_energy; int* T_out; int Tcap; void* stream;
};

// the one host path of the four exports: every check (`name`: the export that was called, for the messages), the tile, the kernel
// arguments, the launch.  Grid (ceil(Tcap / FT), B), FE_THREADS threads, the tile's LDS bytes
template <bool MFCC, bool SPAN>
int fe_launch(const char* name, const FeCall& c) {
    SPK_REQUIRE(c.wave && c.nsamp && c.window && c.twiddle && c.mel_w && c.mel_lo && c.mel_off && c.feats && c.log_energy && c.T_out,
                "%s: null pointer", name);
    if constexpr (SPAN) SPK_REQUIRE(c.first && c.total && c.frame0 && c.nframes, "%s: null pointer", name);
    if constexpr (MFCC) SPK_REQUIRE(c.dct && c.lifter, "%s: null pointer", name);
    SPK_REQUIRE(c.dither == 0.f || c.utt_ids, "%s: dither != 0 needs utt_ids", name);
    SPK_REQUIRE(c.B > 0 && c.B <= 65535 && c.Nmax > 0 && c.Tcap > 0, "%s: B=%d Nmax=%lld Tcap=%d", name, c.B, c.Nmax, c.Tcap);
    SPK_REQUIRE(c.P >= 4 && c.P <= 1024 && (c.P & (c.P - 1)) == 0, "%s: padded window P=%d must be a power of two in [4, 1024]", name, c.P);
    SPK_REQUIRE(c.L >= 2 && c.L <= c.P && c.S >= 1, "%s: frame length L=%d (<= P=%d), shift S=%d", name, c.L, c.P, c.S);
    if constexpr (MFCC) {
        SPK_REQUIRE(c.F >= 1 && c.F <= c.P, "%s: num_mel_bins F=%d (the log-mels of a frame reuse its FFT buffer of P=%d floats)", name,
                    c.F, c.P);
        SPK_REQUIRE(c.C >= 1 && c.C <= c.F, "%s: num_ceps C=%d must be in [1, num_mel_bins F=%d]", name, c.C, c.F);
    } else {
        SPK_REQUIRE(c.F >= 1 && c.F <= 1024, "%s: num_mel_bins F=%d", name, c.F);
    }
    SPK_REQUIRE(c.dither >= 0.f && c.preemph >= 0.f && c.preemph <= 1.f && c.energy_floor >= 0.f, "%s: dither=%g preemph=%g energy_floor=%g",
                name, c.dither, c.preemph, c.energy_floor);
    const int FT = fe_tile_frames<MFCC>(c.L, c.S, c.P, c.F, c.C);
    if constexpr (MFCC) SPK_REQUIRE(FT > 0, "%s: L=%d S=%d P=%d F=%d C=%d do not fit the LDS tile", name, c.L, c.S, c.P, c.F, c.C);
    else SPK_REQUIRE(FT > 0, "%s: L=%d S=%d P=%d F=%d do not fit the LDS tile", name, c.L, c.S, c.P, c.F);
    typename std::conditional<SPAN, SpanArgs, FbankArgs>::type a;
    a.wave = c.wave; a.nsamp = c.nsamp; a.utt_ids = c.utt_ids; a.Nmax = c.Nmax;
    a.window = c.window; a.twiddle = c.twiddle; a.mel_w = c.mel_w; a.mel_lo = c.mel_lo; a.mel_off = c.mel_off;
    a.L = c.L; a.S = c.S; a.P = c.P; a.F = c.F; a.snip = c.snip_edges ? 1 : 0; a.FT = FT; a.span = (FT - 1) * c.S + c.L;
    int lg = 0;
    while ((1 << lg) < c.P / 2) ++lg;
    a.logM = lg;
    a.dither = c.dither; a.preemph = c.preemph; a.remove_dc = c.remove_dc ? 1 : 0;
    a.log_floor = c.energy_floor > 0.f ? logf(c.energy_floor) : -__builtin_inff();
    a.seed = c.seed; a.feats = c.feats; a.loge = c.log_energy; a.T_out = c.T_out; a.Tcap = c.Tcap;
    if constexpr (MFCC) {
        a.dct = c.dct; a.lifter = c.lifter; a.C = c.C; a.Fp = c.F | 1; a.use_energy = c.use_energy ? 1 : 0; a.htk = c.htk_compat ? 1 : 0;
    } else {
        a.dct = nullptr; a.lifter = nullptr; a.C = 0; a.Fp = 0; a.use_energy = 0; a.htk = 0;
    }
    if constexpr (SPAN) {
        a.first = c.first; a.total = c.total; a.frame0 = c.frame0; a.nframes = c.nframes;
    }
    const int lds = MFCC ? (int)fe_mfcc_lds_bytes(FT, c.L, c.S, c.P, c.F, c.C) : fe_lds_bytes(FT, c.L, c.S, c.P, c.F);
    const dim3 grid((unsigned)spk_ceil_div(c.Tcap, FT), (unsigned)c.B);
    if constexpr (SPAN) hipLaunchKernelGGL(MFCC ? mfcc_span_kernel : fbank_span_kernel, grid, dim3(FE_THREADS), lds, (hipStream_t)c.stream, a);
    else hipLaunchKernelGGL(MFCC ? mfcc_kernel : fbank_kernel, grid, dim3(FE_THREADS), lds, (hipStream_t)c.stream, a);
    SPK_LAUNCH_CHECK(name);
    return 0;
}

}  // namespace

// ---- exports (include/spkhip.h) ----
extern "C" int spk_fbank_tile_frames(int L, int S, int P, int F) { return fe_tile_frames<false>(L, S, P, F, 0); }

extern "C" int spk_mfcc_tile_frames(int L, int S, int P, int F, int C) { return fe_tile_frames<true>(L, S, P, F, C); }

extern "C" int spk_fbank_fwd(const float* wave, const int* nsamp, const long long* utt_ids, int B, long long Nmax,
                             const float* window, const float* twiddle, const float* mel_w, const int* mel_lo, const int* mel_off,
                             int L, int S, int P, int F, int snip_edges, float dither, float preemph, int remove_dc,
                             float energy_floor, unsigned long long seed, float* feats, float* log_energy, int* T_out, int Tcap,
                             void* stream) {
    const FeCall c = {wave, nsamp, nullptr, nullptr, nullptr, nullptr, utt_ids, B, Nmax, window, twiddle, mel_w, mel_lo, mel_off,
                      nullptr, nullptr, L, S, P, F, 0, snip_edges, dither, preemph, remove_dc, energy_floor, 0, 0, seed, feats,
                      log_energy, T_out, Tcap, stream};
    return fe_launch<false, false>("spk_fbank_fwd", c);
}

extern "C" int spk_mfcc_fwd(const float* wave, const int* nsamp, const long long* utt_ids, int B, long long Nmax,
                            const float* window, const float* twiddle, const float* mel_w, const int* mel_lo, const int* mel_off,
                            const float* dct, const float* lifter, int L, int S, int P, int F, int C, int snip_edges, float dither,
                            float preemph, int remove_dc, float energy_floor, int use_energy, int htk_compat,
                            unsigned long long seed, float* feats, float* log_energy, int* T_out, int Tcap, void* stream) {
    const FeCall c = {wave, nsamp, nullptr, nullptr, nullptr, nullptr, utt_ids, B, Nmax, window, twiddle, mel_w, mel_lo, mel_off,
                      dct, lifter, L, S, P, F, C, snip_edges, dither, preemph, remove_dc, energy_floor, use_energy, htk_compat, seed,
                      feats, log_energy, T_out, Tcap, stream};
    return fe_launch<true, false>("spk_mfcc_fwd", c);
}

extern "C" int spk_fbank_span_fwd(const float* wave, const int* nsamp, const long long* first, const long long* total, const int* frame0,
                                  const int* nframes, const long long* utt_ids, int B, long long Nmax, const float* window,
                                  const float* twiddle, const float* mel_w, const int* mel_lo, const int* mel_off, int L, int S, int P,
                                  int F, int snip_edges, float dither, float preemph, int remove_dc, float energy_floor,
                                  unsigned long long seed, float* feats, float* log_energy, int* T_out, int Tcap, void* stream) {
    const FeCall c = {wave, nsamp, first, total, frame0, nframes, utt_ids, B, Nmax, window, twiddle, mel_w, mel_lo, mel_off,
                      nullptr, nullptr, L, S, P, F, 0, snip_edges, dither, preemph, remove_dc, energy_floor, 0, 0, seed, feats,
                      log_energy, T_out, Tcap, stream};
    return fe_launch<false, true>("spk_fbank_span_fwd", c);
}

extern "C" int spk_mfcc_span_fwd(const float* wave, const int* nsamp, const long long* first, const long long* total, const int* frame0,
                                 const int* nframes, const long long* utt_ids, int B, long long Nmax, const float* window,
                                 const float* twiddle, const float* mel_w, const int* mel_lo, const int* mel_off, const float* dct,
                                 const float* lifter, int L, int S, int P, int F, int C, int snip_edges, float dither, float preemph,
                                 int remove_dc, float energy_floor, int use_energy, int htk_compat, unsigned long long seed,
                                 float* feats, float* log_energy, int* T_out, int Tcap, void* stream) {
    const FeCall c = {wave, nsamp, first, total, frame0, nframes, utt_ids, B, Nmax, window, twiddle, mel_w, mel_lo, mel_off,
                      dct, lifter, L, S, P, F, C, snip_edges, dither, preemph, remove_dc, energy_floor, use_energy, htk_compat, seed,
                      feats, log_energy, T_out, Tcap, stream};
    return fe_launch<true, true>("spk_mfcc_span_fwd", c);
}

extern "C" int spk_pcm16_to_f32(const short* pcm, const int* count, int B, long long Nmax, float* out, void* stream) {
    SPK_REQUIRE(pcm && count && out, "spk_pcm16_to_f32: null pointer");
    SPK_REQUIRE(B > 0 && B <= 65535 && Nmax > 0 && Nmax < (1ll << 31), "spk_pcm16_to_f32: B=%d Nmax=%lld", B, Nmax);
    const int vec = (Nmax % 8 == 0) && ((size_t)pcm % 16 == 0) && ((size_t)out % 16 == 0);
    hipLaunchKernelGGL(pcm16_to_f32_kernel, dim3((unsigned)((Nmax + 2047) / 2048), (unsigned)B), dim3(256), 0, (hipStream_t)stream, pcm,
                       count, Nmax, out, vec);
    SPK_LAUNCH_CHECK("spk_pcm16_to_f32");
    return 0;
}

extern "C" int spk_fbank_dither_noise(float* out, long long utt_id, unsigned long long seed, int frame0, int nframes, int L,
                                      void* stream) {
    SPK_REQUIRE(out, "spk_fbank_dither_noise: null pointer");
    SPK_REQUIRE(frame0 >= 0 && nframes > 0 && L >= 1 && L <= 1024, "spk_fbank_dither_noise: frame0=%d nframes=%d L=%d", frame0,
                nframes, L);
    const long long n = (long long)nframes * L;
    hipLaunchKernelGGL(dither_noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, utt_id, seed,
                       frame0, nframes, L);
    SPK_LAUNCH_CHECK("spk_fbank_dither_noise");
    return 0;
}

extern "C" int spk_vad_count(const float* log_energy, const int* T, int B, int Tcap, double energy_threshold, double mean_scale,
                             int frames_context, double proportion, int* vad, int* idx, int* count, void* stream) {
    SPK_REQUIRE(log_energy && T && vad && idx && count, "spk_vad_count: null pointer");
    SPK_REQUIRE(B > 0 && Tcap > 0, "spk_vad_count: B=%d Tcap=%d", B, Tcap);
    SPK_REQUIRE(frames_context >= 0 && mean_scale >= 0.0, "spk_vad_count: frames_context=%d mean_scale=%g", frames_context, mean_scale);
    hipLaunchKernelGGL(vad_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, log_energy, T, Tcap, energy_threshold,
                       mean_scale, frames_context, proportion, vad, idx, count);
    SPK_LAUNCH_CHECK("spk_vad_count");
    return 0;
}

extern "C" int spk_vad_segments(const int* vad, const int* T, int B, int Tcap, int padding, int max_gap, int min_length, int* seg,
                                int Scap, int* nseg, void* stream) {
    // Tcap: the frame index of a lane past the last round's prefetch must stay an int
    SPK_REQUIRE(B >= 0 && Tcap >= 0 && Tcap <= 0x7fffffff - 2 * 64 * SEG_CHUNKS && Scap >= 0, "spk_vad_segments: B=%d Tcap=%d Scap=%d", B,
                Tcap, Scap);
    SPK_REQUIRE(padding >= 0 && max_gap >= 0 && min_length >= 1, "spk_vad_segments: padding=%d max_gap=%d (>= 0) min_length=%d (>= 1)",
                padding, max_gap, min_length);
    if (B == 0) return 0;
    SPK_REQUIRE(T && nseg && (vad || Tcap == 0) && (seg || Scap == 0), "spk_vad_segments: null pointer");
    hipLaunchKernelGGL(vad_segments_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, vad, T, Tcap, padding, max_gap,
                       min_length, seg, Scap, nseg);
    SPK_LAUNCH_CHECK("spk_vad_segments");
    return 0;
}

extern "C" int spk_cmn_select(const float* x, const int* T, const int* idx, const int* count, double* prefix, float* out, int B,
                              int F, int Tcap, int Tout, int cmn_window, void* stream) {
    SPK_REQUIRE(x && T && out, "spk_cmn_select: null pointer");
    SPK_REQUIRE(cmn_window == 0 || prefix, "spk_cmn_select: cmn_window > 0 needs the prefix workspace");
    SPK_REQUIRE((idx == nullptr) == (count == nullptr), "spk_cmn_select: idx and count go together");
    SPK_REQUIRE(B > 0 && F > 0 && Tcap > 0 && Tout > 0 && cmn_window >= 0, "spk_cmn_select: B=%d F=%d Tcap=%d Tout=%d W=%d", B, F,
                Tcap, Tout, cmn_window);
    SPK_REQUIRE((long long)B * F * spk_ceil_div(Tout, 256) < (1ll << 31), "spk_cmn_select: B=%d F=%d Tout=%d exceed the grid", B, F, Tout);
    SPK_REQUIRE(Tout <= Tcap, "spk_cmn_select: Tout=%d > Tcap=%d", Tout, Tcap);
    if (cmn_window > 0) {
        hipLaunchKernelGGL(cmn_prefix_kernel, dim3((unsigned)spk_ceil_div(B * F, 4)), dim3(256), 0, (hipStream_t)stream, x, T, B, F,
                           Tcap, prefix);
        SPK_LAUNCH_CHECK("spk_cmn_select");
    }
    const int nj = spk_ceil_div(Tout, 256);
    hipLaunchKernelGGL(cmn_select_kernel, dim3((unsigned)(B * F * nj)), dim3(256), 0, (hipStream_t)stream, x, T, idx, count, prefix,
                       out, F, Tcap, Tout, cmn_window, nj);
    SPK_LAUNCH_CHECK("spk_cmn_select");
    return 0;
}
