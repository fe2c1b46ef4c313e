// WAV ingest for the feature front end (host only): the wav.scp entries that the reference's feature_pre.sh:77-104 hands to
// compute-fbank-feats, read without Kaldi.  PCM 16-bit mono RIFF/WAVE (also through WAVE_FORMAT_EXTENSIBLE); chunks other than
// 'fmt ' and 'data' are skipped.  Samples stay at int16 scale (Kaldi does not normalise them).
// Returns 0 on success, < 0 on error (message, naming the file, via spk_io_last_error).
#include <fcntl.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

extern "C" void spk_io_set_error(const char* msg);

static void wav_err(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    spk_io_set_error(buf);
}

static uint32_t rd32(const unsigned char* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
static uint16_t rd16(const unsigned char* p) { return (uint16_t)(p[0] | (p[1] << 8)); }

static bool pread_full(int fd, void* dst, size_t n, int64_t off) {
    char* d = (char*)dst;
    while (n) {
        const ssize_t r = pread(fd, d, n, (off_t)off);
        if (r <= 0) return false;
        d += r;
        n -= (size_t)r;
        off += r;
    }
    return true;
}

// one file: sample rate, sample count, byte offset of the first sample
static int probe_one(const char* path, int expect_rate, int32_t* rate, int64_t* nsamp, int64_t* data_off) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        wav_err("%s: cannot open", path);
        return -2;
    }
    struct stat st;
    fstat(fd, &st);
    const int64_t fsize = st.st_size;
    unsigned char h[12];
    int rc = 0;
    if (!pread_full(fd, h, 12, 0) || memcmp(h, "RIFF", 4) != 0 || memcmp(h + 8, "WAVE", 4) != 0) {
        wav_err("%s: not a RIFF/WAVE file", path);
        close(fd);
        return -3;
    }
    int64_t off = 12;
    bool have_fmt = false;
    int channels = 0, bits = 0;
    uint32_t sr = 0;
    for (;;) {
        unsigned char c[8];
        if (off + 8 > fsize || !pread_full(fd, c, 8, off)) {
            wav_err("%s: no data chunk", path);
            rc = -3;
            break;
        }
        const uint32_t sz = rd32(c + 4);
        if (memcmp(c, "fmt ", 4) == 0) {
            unsigned char f[40] = {0};
            if (sz < 16 || !pread_full(fd, f, sz < 40 ? sz : 40, off + 8)) {
                wav_err("%s: short fmt chunk", path);
                rc = -3;
                break;
            }
            int tag = rd16(f);
            channels = rd16(f + 2);
            sr = rd32(f + 4);
            bits = rd16(f + 14);
            if (tag == 0xFFFE) {             // WAVE_FORMAT_EXTENSIBLE: the sub-format GUID starts with the format tag
                if (sz < 40) {
                    wav_err("%s: short WAVE_FORMAT_EXTENSIBLE fmt chunk", path);
                    rc = -3;
                    break;
                }
                tag = rd16(f + 24);
            }
            if (tag != 1) {
                wav_err("%s: format tag %d is not PCM (only 16-bit PCM mono is supported)", path, tag);
                rc = -4;
                break;
            }
            if (channels != 1) {
                wav_err("%s: %d channels (only mono is supported)", path, channels);
                rc = -4;
                break;
            }
            if (bits != 16) {
                wav_err("%s: %d-bit samples (only 16-bit PCM is supported)", path, bits);
                rc = -4;
                break;
            }
            if (expect_rate > 0 && (int64_t)sr != expect_rate) {
                wav_err("%s: sample rate %u differs from sample_frequency %d", path, sr, expect_rate);
                rc = -5;
                break;
            }
            have_fmt = true;
        } else if (memcmp(c, "data", 4) == 0) {
            if (!have_fmt) {
                wav_err("%s: data chunk before fmt chunk", path);
                rc = -3;
                break;
            }
            int64_t bytes = sz;
            if (bytes > fsize - (off + 8)) bytes = fsize - (off + 8);     // streamed files: size field 0xFFFFFFFF or truncated
            *rate = (int32_t)sr;
            *nsamp = bytes / 2;
            *data_off = off + 8;
            break;
        }
        off += 8 + (int64_t)sz + (sz & 1);        // chunks are padded to even sizes
    }
    close(fd);
    return rc;
}

extern "C" int spk_wav_probe(int n, const char* const* paths, int expect_rate, int32_t* rate, int64_t* nsamp, int64_t* data_off) {
    if (n < 0 || (n > 0 && (!paths || !rate || !nsamp || !data_off))) {
        wav_err("spk_wav_probe: bad arguments");
        return -1;
    }
    for (int i = 0; i < n; ++i) {
        const int rc = probe_one(paths[i], expect_rate, rate + i, nsamp + i, data_off + i);
        if (rc) return rc;
    }
    return 0;
}

// out[b][s] = int16 sample s of file b (as float) for s < nsamp[b], 0 for nsamp[b] <= s < Nmax; pread on nthreads threads
extern "C" int spk_wav_read_padded(int B, const char* const* paths, const int64_t* data_off, const int64_t* nsamp, int64_t Nmax,
                                   float* out, int nthreads) {
    if (B <= 0 || Nmax <= 0 || !paths || !data_off || !nsamp || !out) {
        wav_err("spk_wav_read_padded: bad arguments");
        return -1;
    }
    for (int b = 0; b < B; ++b) {
        if (nsamp[b] < 0 || nsamp[b] > Nmax) {
            wav_err("spk_wav_read_padded: %s has %lld samples, outside [0, Nmax=%lld]", paths[b], (long long)nsamp[b],
                    (long long)Nmax);
            return -7;
        }
    }
    if (nthreads < 1) nthreads = 1;
    if (nthreads > B) nthreads = B;
    std::atomic<int> next(0), fail(0);
    auto work = [&]() {
        std::vector<int16_t> tmp;
        for (;;) {
            const int b = next.fetch_add(1);
            if (b >= B || fail.load()) break;
            const int fd = open(paths[b], O_RDONLY);
            if (fd < 0) {
                wav_err("%s: cannot open", paths[b]);
                fail.store(1);
                break;
            }
            const int64_t n = nsamp[b];
            tmp.resize((size_t)n);
            const bool ok = pread_full(fd, tmp.data(), (size_t)n * 2, data_off[b]);
            close(fd);
            if (!ok) {
                wav_err("%s: short read of %lld samples", paths[b], (long long)n);
                fail.store(1);
                break;
            }
            float* dst = out + (size_t)b * Nmax;
            for (int64_t s = 0; s < n; ++s) dst[s] = (float)tmp[(size_t)s];     // little-endian host
            if (n < Nmax) memset(dst + n, 0, (size_t)(Nmax - n) * sizeof(float));
        }
    };
    std::vector<std::thread> pool;
    for (int i = 1; i < nthreads; ++i) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    return fail.load() ? -8 : 0;
}

// out[b][s] = sample first[b] + s of file b, as it lies in the file (int16), for s < count[b]; 0 for count[b] <= s < Nmax.  Only the
// span is read (pread on nthreads threads): the reader of training from audio, where a batch needs a few seconds of each file
extern "C" int spk_wav_read_span(int B, const char* const* paths, const int64_t* data_off, const int64_t* nsamp, const int64_t* first,
                                 const int64_t* count, int64_t Nmax, int16_t* out, int nthreads) {
    if (B <= 0 || Nmax <= 0 || !paths || !data_off || !nsamp || !first || !count || !out) {
        wav_err("spk_wav_read_span: bad arguments");
        return -1;
    }
    for (int b = 0; b < B; ++b) {
        if (first[b] < 0 || count[b] < 0 || first[b] > nsamp[b] || count[b] > nsamp[b] - first[b]) {
            wav_err("spk_wav_read_span: %s: span of %lld samples from sample %lld lies outside the file's %lld samples", paths[b],
                    (long long)count[b], (long long)first[b], (long long)nsamp[b]);
            return -7;
        }
        if (count[b] > Nmax) {
            wav_err("spk_wav_read_span: %s: span of %lld samples is longer than the row of Nmax=%lld", paths[b], (long long)count[b],
                    (long long)Nmax);
            return -7;
        }
    }
    if (nthreads < 1) nthreads = 1;
    if (nthreads > B) nthreads = B;
    std::atomic<int> next(0), fail(0);
    auto work = [&]() {
        for (;;) {
            const int b = next.fetch_add(1);
            if (b >= B || fail.load()) break;
            const int fd = open(paths[b], O_RDONLY);
            if (fd < 0) {
                wav_err("%s: cannot open", paths[b]);
                fail.store(1);
                break;
            }
            const int64_t n = count[b];
            int16_t* dst = out + (size_t)b * Nmax;
            const bool ok = n == 0 || pread_full(fd, dst, (size_t)n * 2, data_off[b] + 2 * first[b]);     // little-endian host
            close(fd);
            if (!ok) {
                wav_err("%s: short read of %lld samples from sample %lld", paths[b], (long long)n, (long long)first[b]);
                fail.store(1);
                break;
            }
            if (n < Nmax) memset(dst + n, 0, (size_t)(Nmax - n) * sizeof(int16_t));
        }
    };
    std::vector<std::thread> pool;
    for (int i = 1; i < nthreads; ++i) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    return fail.load() ? -8 : 0;
}
