/* libspkio - native batch ingest of Kaldi float32 and one-byte compressed matrices (host-side C ABI, no device code).
 * Replaces, for fixed-length training batches, the per-sample path of the reference:
 *   kaldi_io.read_mat (scripts/kaldi_io.py:376-410, open_or_fd :41-71) -> random crop + transpose
 *   (scripts/datasets.py:59-72) -> default collate.
 * All pointers are HOST pointers; `out` should be pinned memory so the H2D copy can be asynchronous. */
#ifndef SPKIO_H
#define SPKIO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int spk_io_version(void);
const char* spk_io_last_error(void);
/* parse n matrix headers at (paths[i], offsets[i]) (the scp's "path:offset"): rows, cols, payload offset */
int spk_ark_probe(int n, const char* const* paths, const int64_t* offsets, int32_t* rows, int32_t* cols,
                  int64_t* data_offsets);
/* out[b][f][t] = M_b[starts[b] + t][f], t < T; reads only the cropped frames with pread() on `nthreads` threads */
int spk_ark_read_crop(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows,
                      const int32_t* starts, int F, int T, float* out, int nthreads);
/* whole utterances, padded: out[b][f][t] = M_b[t][f] for t < rows[b], 0 for rows[b] <= t < T (1 <= rows[b] <= T) - the input of a
 * length-masked predict over a length-sorted batch */
int spk_ark_read_padded(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows, int F, int T,
                        float* out, int nthreads);
/* Kaldi's one-byte compressed matrices ('CM ') next to float32 'FM '.  kinds[i]: 0 'FM ', 1 'CM ';
 * data_offsets[i] of a 'CM ' entry is the byte of its first column header; its header sizes are checked against the file length.
 * 'CM2' / 'CM3' / 'DM ' stay refused.  spk_ark_probe above refuses 'CM ' (it cannot say which kind an entry is). */
int spk_ark_probe_kinds(int n, const char* const* paths, const int64_t* offsets, int32_t* rows, int32_t* cols,
                        int64_t* data_offsets, int32_t* kinds);
/* spk_ark_read_crop / spk_ark_read_padded with the probed kinds; 'FM ' and 'CM ' entries may be mixed.  A 'CM ' entry is decoded
 * on the host in float32, every operation rounded on its own: the bits of kaldi_io.read_mat.  (The two functions above take the
 * same entries and find the kind in front of each payload.) */
int spk_ark_read_crop_kinds(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows,
                            const int32_t* starts, const int32_t* kinds, int F, int T, float* out, int nthreads);
int spk_ark_read_padded_kinds(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows,
                              const int32_t* kinds, int F, int T, float* out, int nthreads);
/* 'CM ' entries as stored, the input of the GPU decode in libspkhip: codes[b][f][t] = the code of frame starts[b] + t, bin f (padded form:
 * frame t, 0 for rows[b] <= t < T), colhdr[b][f][4] = the float32 values of the column header (p0, p25, p75, p100):
 * min + (range * 1.52590218966964e-05f) * p. */
int spk_ark_read_crop_codes(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows,
                            const int32_t* starts, int F, int T, uint8_t* codes, float* colhdr, int nthreads);
int spk_ark_read_padded_codes(int B, const char* const* paths, const int64_t* data_offsets, const int32_t* rows, int F, int T,
                              uint8_t* codes, float* colhdr, int nthreads);
void spk_ark_close_all(void);
/* text-ark embedding writer: out <- "key [ v0 v1 ... ]\n" per row of v[n][D], each value printed exactly as numpy's
 * str(np.float32) does - the line format of the reference's scripts/decode.py:199-206.  Returns the bytes written
 * (-1 if cap < spk_text_vectors_bound). */
int64_t spk_text_vectors_bound(int n, int D, const char* const* keys);
int64_t spk_format_text_vectors(int n, int D, const float* v, const char* const* keys, char* out, int64_t cap,
                                int nthreads);
/* vector-ark reader for the scoring back end (reference: kaldi_io.read_vec_flt_ark as used by scripts/compute_mean.py:9-33 and
 * scripts/cosine_score.py:52-60): the whole ark - text 'key [ v0 ... ]' lines as scripts/decode.py:206 writes them, or binary FV / DV
 * records - into one malloc'ed [n][D] float64 matrix (text values parsed as doubles, as numpy does) and a buffer of n NUL-terminated
 * keys; parsed on `nthreads` threads.  Free both with spk_vec_ark_free.  0 on success. */
int spk_vec_ark_load(const char* path, int nthreads, int64_t* n, int32_t* D, double** data, char** keys, int64_t* keys_bytes);
void spk_vec_ark_free(double* data, char* keys);
void spk_io_set_error(const char* msg);
/* WAV ingest for the feature front end (csrc_io/wav_reader.cpp; the wav.scp files that the reference's feature_pre.sh:77-104 gives
 * to compute-fbank-feats): RIFF/WAVE, PCM 16-bit mono (also as WAVE_FORMAT_EXTENSIBLE), chunks other than 'fmt ' / 'data' skipped.
 * Probe: per file the sample rate, the sample count and the byte offset of the samples; other widths, channel counts, formats and
 * (expect_rate > 0) sample rates are refused with an error naming the file. */
int spk_wav_probe(int n, const char* const* paths, int expect_rate, int32_t* rate, int64_t* nsamp, int64_t* data_offsets);
/* out[b][s] = sample s of file b at int16 scale for s < nsamp[b], 0 up to Nmax; pread() on `nthreads` threads */
int spk_wav_read_padded(int B, const char* const* paths, const int64_t* data_offsets, const int64_t* nsamp, int64_t Nmax, float* out,
                        int nthreads);
/* the reader of training from audio (ingest.WavTrainLoader; replaces the feature directories that stages 3 and 4 of the reference's
 * feature_pre.sh:170-197 write only to be cropped): out[b][s] = sample first[b] + s of file b as it lies in the file (int16) for
 * s < count[b], 0 up to Nmax.  Only the span is read, pread() on `nthreads` threads.  first < 0, first + count > nsamp and
 * count > Nmax are refused with an error naming the file. */
int spk_wav_read_span(int B, const char* const* paths, const int64_t* data_offsets, const int64_t* nsamp, const int64_t* first,
                      const int64_t* count, int64_t Nmax, int16_t* out, int nthreads);
#ifdef __cplusplus
}
#endif
#endif
