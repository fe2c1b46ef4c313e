// libspkio - native batch ingest for Kaldi 'FM ' and 'CM ' (one-byte compressed) matrices (the step before the hot path).
//
// Reference behaviour being replaced (scripts/datasets.py:59-72 + scripts/kaldi_io.py:41-71,376-410): per sample,
// open the ark, seek to the scp offset, read the WHOLE utterance, crop seq_len frames at a random start, transpose to
// [F, T].  Here a batch is read by a small thread pool with pread(): only the cropped rows are read, and they are
// transposed straight into the caller's (pinned) [B][F][T] staging buffer, so the DataLoader worker processes, the
// full-utterance read and the collate copy disappear.
//
// C ABI, host pointers only:
//   spk_ark_probe      - parse the matrix headers at (path, offset): rows / cols / payload offset (done once per scp)
//   spk_ark_read_crop  - fill out[b][f][t] = M_b[start_b + t][f] for t < T, all b in the batch
//   spk_ark_probe_kinds / spk_ark_read_*_kinds / spk_ark_read_*_codes - the same with 'CM ' entries: decoded here to the bits
//                        kaldi_io.read_mat gives, or handed on as codes + column headers for the GPU decode (csrc/cm.hip)
// Returns 0 on success, < 0 on error (message via spk_io_last_error).
#include <fcntl.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

static thread_local char g_err[512] = "";
static std::mutex g_err_mu;
static char g_err_shared[512] = "";

static void set_err(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lk(g_err_mu);
    memcpy(g_err_shared, g_err, sizeof(g_err));
}

extern "C" const char* spk_io_last_error(void) { return g_err_shared; }
extern "C" void spk_io_set_error(const char* msg) { set_err("%s", msg); }      // for the other translation units of libspkio

// file-descriptor cache: arks are few and large, reopen per sample is what the reference pays
static std::mutex g_fd_mu;
static std::map<std::string, int> g_fds;

static int get_fd(const char* path) {
    std::lock_guard<std::mutex> lk(g_fd_mu);
    auto it = g_fds.find(path);
    if (it != g_fds.end()) return it->second;
    int fd = open(path, O_RDONLY);
    if (fd >= 0) g_fds[path] = fd;
    return fd;
}

extern "C" void spk_ark_close_all(void) {
    std::lock_guard<std::mutex> lk(g_fd_mu);
    for (auto& kv : g_fds) close(kv.second);
    g_fds.clear();
}

static bool pread_all(int fd, void* buf, size_t n, int64_t off) {
    char* p = (char*)buf;
    while (n) {
        ssize_t r = pread(fd, p, n, off);
        if (r <= 0) return false;
        p += r;
        off += r;
        n -= (size_t)r;
    }
    return true;
}

// header at `off`: "\0B" then the type token.
//   "FM " \x04 int32 rows \x04 int32 cols (15 bytes), then rows*cols float32 row-major
//   "CM " float32 min, float32 range, int32 rows, int32 cols (21 bytes), then cols x 4 uint16 column headers, then cols*rows uint8
//         codes COLUMN-major: all frames of bin 0 first - the [F][T] layout of a batch row
// data_off: FM the first float, CM the first column header.
enum { KIND_FM = 0, KIND_CM = 1 };
constexpr int FM_HEAD = 15, CM_HEAD = 21;

static int parse_header(int fd, int64_t off, int32_t* rows, int32_t* cols, int64_t* data_off, int32_t* kind, const char* path) {
    unsigned char h[CM_HEAD];
    if (!pread_all(fd, h, FM_HEAD, off)) {
        set_err("%s:%lld: short read in matrix header", path, (long long)off);
        return -2;
    }
    if (h[0] != 0 || h[1] != 'B') {
        set_err("%s:%lld: not a binary Kaldi object (text arks are not supported by the native reader)", path, (long long)off);
        return -3;
    }
    if (memcmp(h + 2, "CM ", 3) == 0) {
        if (!kind) {
            set_err("%s:%lld: matrix type 'CM ' needs the probe that reports kinds (spk_ark_probe_kinds); this one describes "
                    "float32 'FM ' entries only", path, (long long)off);
            return -4;
        }
        if (!pread_all(fd, h + FM_HEAD, CM_HEAD - FM_HEAD, off + FM_HEAD)) {
            set_err("%s:%lld: short read in compressed matrix header", path, (long long)off);
            return -2;
        }
        memcpy(rows, h + 13, 4);
        memcpy(cols, h + 17, 4);
        *data_off = off + CM_HEAD;
        *kind = KIND_CM;
        if (*rows < 0 || *cols <= 0) {
            set_err("%s:%lld: bad matrix shape %d x %d", path, (long long)off, *rows, *cols);
            return -6;
        }
        struct stat st;
        const int64_t need = *data_off + (int64_t)*cols * 8 + (int64_t)*cols * *rows;
        if (fstat(fd, &st) != 0 || st.st_size < need) {
            set_err("%s:%lld: truncated compressed matrix: %d x %d needs the file to reach byte %lld", path, (long long)off, *rows,
                    *cols, (long long)need);
            return -9;
        }
        return 0;
    }
    if (memcmp(h + 2, "FM ", 3) != 0) {
        set_err("%s:%lld: matrix type '%c%c%c' unsupported (float32 'FM ' and one-byte compressed 'CM ' only; 'CM2' / 'CM3' / 'DM ' "
                "are not read natively)", path, (long long)off, h[2], h[3], h[4]);
        return -4;
    }
    if (h[5] != 4 || h[10] != 4) {
        set_err("%s:%lld: bad int32 size markers in matrix header", path, (long long)off);
        return -5;
    }
    memcpy(rows, h + 6, 4);
    memcpy(cols, h + 11, 4);
    *data_off = off + FM_HEAD;
    if (kind) *kind = KIND_FM;
    if (*rows < 0 || *cols <= 0) {
        set_err("%s:%lld: bad matrix shape %d x %d", path, (long long)off, *rows, *cols);
        return -6;
    }
    return 0;
}

extern "C" int spk_ark_probe_kinds(int n, const char* const* paths, const int64_t* offsets, int32_t* rows, int32_t* cols,
                                   int64_t* data_offsets, int32_t* kinds) {
    for (int i = 0; i < n; ++i) {
        int fd = get_fd(paths[i]);
        if (fd < 0) {
            set_err("cannot open %s", paths[i]);
            return -1;
        }
        int rc = parse_header(fd, offsets[i], &rows[i], &cols[i], &data_offsets[i], kinds ? &kinds[i] : nullptr, paths[i]);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int spk_ark_probe(int n, const char* const* paths, const int64_t* offsets, int32_t* rows, int32_t* cols,
                             int64_t* data_offsets) {
    return spk_ark_probe_kinds(n, paths, offsets, rows, cols, data_offsets, nullptr);
}

// kind of the record whose payload starts at data_off, for the callers that pass no kinds: the bytes in front of the payload
static int kind_at(int fd, int64_t data_off, const char* path) {
    unsigned char h[CM_HEAD];
    const bool cm = data_off >= CM_HEAD && pread_all(fd, h, 5, data_off - CM_HEAD) && memcmp(h, "\0BCM ", 5) == 0;
    const bool fm = data_off >= FM_HEAD && pread_all(fd, h, 11, data_off - FM_HEAD) && memcmp(h, "\0BFM \x04", 6) == 0 && h[10] == 4;
    if (cm == fm) {
        set_err("%s:%lld: no 'FM ' or 'CM ' matrix header in front of this payload offset", path, (long long)data_off);
        return -1;
    }
    return cm ? KIND_CM : KIND_FM;
}

// U(u) of DESIGN.md section 6g: every operation rounded to float32 on its own (this file is built with -ffp-contract=off)
static inline float cm_u(float vmin, float scale, uint16_t u) { return vmin + scale * (float)u; }
static inline float cm_value(const float* P, uint8_t c) {
    if (c <= 64) return P[0] + (P[1] - P[0]) * (float)c * (1 / 64.f);
    if (c <= 192) return P[1] + (P[2] - P[1]) * (float)(c - 64) * (1 / 128.f);
    return P[2] + (P[3] - P[2]) * (float)(c - 192) * (1 / 63.f);
}

// frames [start, start + n) of the CM record at data_off: codes[f * stride + t] (t < n) and P[f][4] = U of the column headers.
// One read of the span the F strips cover when that is no more than the bytes the same crop of an 'FM ' record reads
// (rows <= 4 n), F strip reads otherwise.  span: scratch of the worker.
static bool cm_fetch(int fd, const char* path, int64_t data_off, int rows, int F, int start, int n, uint8_t* codes, size_t stride,
                     float* P, std::vector<uint8_t>& span) {
    std::vector<unsigned char> head(16 + (size_t)F * 8);
    if (!pread_all(fd, head.data(), head.size(), data_off - 16)) {
        set_err("%s:%lld: short read of the compressed matrix headers", path, (long long)(data_off - CM_HEAD));
        return false;
    }
    float vmin, vrange;
    int32_t r, c;
    memcpy(&vmin, head.data(), 4);
    memcpy(&vrange, head.data() + 4, 4);
    memcpy(&r, head.data() + 8, 4);
    memcpy(&c, head.data() + 12, 4);
    if (r != rows || c != F) {
        set_err("%s:%lld: compressed matrix is %d x %d, the table says %d x %d", path, (long long)(data_off - CM_HEAD), r, c, rows, F);
        return false;
    }
    const float scale = vrange * 1.52590218966964e-05f;
    for (int i = 0; i < F * 4; ++i) {
        uint16_t u;
        memcpy(&u, head.data() + 16 + (size_t)i * 2, 2);
        P[i] = cm_u(vmin, scale, u);
    }
    if (n <= 0) return true;
    const int64_t payload = data_off + (int64_t)F * 8;
    if ((int64_t)rows <= 4 * (int64_t)n) {
        const size_t len = (size_t)(F - 1) * rows + n;
        span.resize(len);
        if (!pread_all(fd, span.data(), len, payload + start)) {
            set_err("%s:%lld: short read of %d frames at frame %d of a compressed matrix", path, (long long)(data_off - CM_HEAD), n, start);
            return false;
        }
        for (int f = 0; f < F; ++f) memcpy(codes + (size_t)f * stride, span.data() + (size_t)f * rows, n);
    } else {
        for (int f = 0; f < F; ++f)
            if (!pread_all(fd, codes + (size_t)f * stride, n, payload + (int64_t)f * rows + start)) {
                set_err("%s:%lld: short read of %d frames at frame %d of a compressed matrix", path, (long long)(data_off - CM_HEAD), n,
                        start);
                return false;
            }
    }
    return true;
}

// blocked transpose [n][F] -> [F][stride]: 16x16 tiles keep both the reads and the writes inside a few cache lines
static void transpose_frames(const float* src, int n, int F, float* dst, size_t stride) {
    constexpr int TB = 16;
    for (int t0 = 0; t0 < n; t0 += TB) {
        const int t1 = t0 + TB < n ? t0 + TB : n;
        for (int f0 = 0; f0 < F; f0 += TB) {
            const int f1 = f0 + TB < F ? f0 + TB : F;
            for (int f = f0; f < f1; ++f) {
                float* d = dst + (size_t)f * stride;
                const float* sp = src + f;
                for (int t = t0; t < t1; ++t) d[t] = sp[(size_t)t * F];
            }
        }
    }
}

// the one reader behind the four entry points.  starts == NULL: whole utterances, zero past rows[b] (padded); else crops of T
// frames.  out != NULL: float32 [B][F][T], 'FM ' rows transposed, 'CM ' rows decoded here; else codes [B][F][T] + colhdr [B][F][4]
// ('CM ' rows only).  kinds == NULL: looked up in front of each payload.
static int read_batch(const char* who, int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows,
                      const int32_t* starts, const int32_t* kinds, int F, int T, float* out, uint8_t* codes, float* colhdr,
                      int nthreads) {
    if (B <= 0 || F <= 0 || T <= 0 || (!out && !(codes && colhdr))) {
        set_err("%s: bad arguments", who);
        return -1;
    }
    for (int b = 0; b < B; ++b) {
        if (starts) {
            if (starts[b] < 0 || starts[b] + T > rows[b]) {   // the reference asserts len(full_mat) >= seq_len (datasets.py:65)
                set_err("%s: crop [%d, %d) outside utterance %d of %d frames", who, starts[b], starts[b] + T, b, rows[b]);
                return -7;
            }
        } else if (rows[b] < 1 || rows[b] > T) {
            set_err("%s: utterance %d has %d frames, outside [1, T=%d]", who, b, rows[b], T);
            return -7;
        }
    }
    if (nthreads < 1) nthreads = 1;
    if (nthreads > B) nthreads = B;
    std::atomic<int> next(0), fail(0);
    auto work = [&]() {
        std::vector<float> tmp;
        std::vector<uint8_t> ctmp, span;
        std::vector<float> P((size_t)F * 4);
        for (;;) {
            const int b = next.fetch_add(1);
            if (b >= B || fail.load()) break;
            int fd = get_fd(paths[b]);
            if (fd < 0) {
                set_err("cannot open %s", paths[b]);
                fail.store(1);
                break;
            }
            const int kind = kinds ? kinds[b] : kind_at(fd, data_offsets[b], paths[b]);
            if (kind != KIND_FM && kind != KIND_CM) {
                if (kinds) set_err("%s: entry %d has kind %d (0 'FM ', 1 'CM ')", who, b, kind);
                fail.store(1);
                break;
            }
            const int start = starts ? starts[b] : 0, n = starts ? T : rows[b];
            if (!out) {
                if (kind != KIND_CM) {
                    set_err("%s: %s:%lld is a float32 'FM ' matrix: it has no codes", who, paths[b], (long long)(data_offsets[b] - FM_HEAD));
                    fail.store(1);
                    break;
                }
                uint8_t* dst = codes + (size_t)b * F * T;
                if (!cm_fetch(fd, paths[b], data_offsets[b], rows[b], F, start, n, dst, T, colhdr + (size_t)b * F * 4, span)) {
                    fail.store(1);
                    break;
                }
                if (n < T)
                    for (int f = 0; f < F; ++f) memset(dst + (size_t)f * T + n, 0, (size_t)(T - n));
                continue;
            }
            float* dst = out + (size_t)b * F * T;     // [F][T], time innermost (reference datasets.py:68 `.T`)
            if (kind == KIND_FM) {
                tmp.resize((size_t)n * F);
                const int64_t off = data_offsets[b] + (int64_t)start * F * (int64_t)sizeof(float);
                if (!pread_all(fd, tmp.data(), tmp.size() * sizeof(float), off)) {
                    set_err("%s: short read of %d frames at frame %d", paths[b], n, start);
                    fail.store(1);
                    break;
                }
                transpose_frames(tmp.data(), n, F, dst, T);
            } else {
                ctmp.resize((size_t)n * F);
                if (!cm_fetch(fd, paths[b], data_offsets[b], rows[b], F, start, n, ctmp.data(), n, P.data(), span)) {
                    fail.store(1);
                    break;
                }
                for (int f = 0; f < F; ++f) {
                    const float* p = P.data() + (size_t)f * 4;
                    const uint8_t* c = ctmp.data() + (size_t)f * n;
                    float* d = dst + (size_t)f * T;
                    for (int t = 0; t < n; ++t) d[t] = cm_value(p, c[t]);
                }
            }
            if (n < T)
                for (int f = 0; f < F; ++f) memset(dst + (size_t)f * T + n, 0, (size_t)(T - n) * sizeof(float));
        }
    };
    std::vector<std::thread> pool;
    for (int i = 1; i < nthreads; ++i) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    return fail.load() ? -8 : 0;
}

extern "C" int spk_ark_read_crop(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows,
                                 const int32_t* starts, int F, int T, float* out, int nthreads) {
    if (!starts || !out) {
        set_err("spk_ark_read_crop: bad arguments");
        return -1;
    }
    return read_batch("spk_ark_read_crop", B, paths, data_offsets, rows, starts, nullptr, F, T, out, nullptr, nullptr, nthreads);
}

// whole utterances of up to T frames into [B][F][T], the frames past rows[b] zero-filled (a length-sorted padded batch for the
// length-masked predict; the lengths go to the model separately)
extern "C" int spk_ark_read_padded(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows, int F, int T,
                                   float* out, int nthreads) {
    if (!out) {
        set_err("spk_ark_read_padded: bad arguments");
        return -1;
    }
    return read_batch("spk_ark_read_padded", B, paths, data_offsets, rows, nullptr, nullptr, F, T, out, nullptr, nullptr, nthreads);
}

// the same two with the kinds the probe reported (no look in front of the payload), 'FM ' and 'CM ' entries mixed freely
extern "C" int spk_ark_read_crop_kinds(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows,
                                       const int32_t* starts, const int32_t* kinds, int F, int T, float* out, int nthreads) {
    if (!starts || !out || !kinds) {
        set_err("spk_ark_read_crop_kinds: bad arguments");
        return -1;
    }
    return read_batch("spk_ark_read_crop_kinds", B, paths, data_offsets, rows, starts, kinds, F, T, out, nullptr, nullptr, nthreads);
}

extern "C" int spk_ark_read_padded_kinds(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows,
                                         const int32_t* kinds, int F, int T, float* out, int nthreads) {
    if (!out || !kinds) {
        set_err("spk_ark_read_padded_kinds: bad arguments");
        return -1;
    }
    return read_batch("spk_ark_read_padded_kinds", B, paths, data_offsets, rows, nullptr, kinds, F, T, out, nullptr, nullptr, nthreads);
}

// 'CM ' entries as stored: codes[b][f][t] = the code of frame starts[b] + t, bin f, and colhdr[b][f][4] = U(p0, p25, p75, p100):
// the inputs of spk_cm_decode (libspkhip).  A quarter of the bytes of the float readers and no arithmetic but the F x 4 headers.
extern "C" int spk_ark_read_crop_codes(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows,
                                       const int32_t* starts, int F, int T, uint8_t* codes, float* colhdr, int nthreads) {
    if (!starts || !codes || !colhdr) {
        set_err("spk_ark_read_crop_codes: bad arguments");
        return -1;
    }
    std::vector<int32_t> kinds((size_t)(B > 0 ? B : 0), KIND_CM);
    return read_batch("spk_ark_read_crop_codes", B, paths, data_offsets, rows, starts, kinds.data(), F, T, nullptr, codes, colhdr, nthreads);
}

// whole utterances: codes zero for rows[b] <= t < T
extern "C" int spk_ark_read_padded_codes(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows, int F,
                                         int T, uint8_t* codes, float* colhdr, int nthreads) {
    if (!codes || !colhdr) {
        set_err("spk_ark_read_padded_codes: bad arguments");
        return -1;
    }
    std::vector<int32_t> kinds((size_t)(B > 0 ? B : 0), KIND_CM);
    return read_batch("spk_ark_read_padded_codes", B, paths, data_offsets, rows, nullptr, kinds.data(), F, T, nullptr, codes, colhdr,
                      nthreads);
}

extern "C" int spk_io_version(void) { return 100; }
