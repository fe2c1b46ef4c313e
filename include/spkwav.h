/* libspkhip - training from audio with speed perturbation (csrc/resample.hip; DESIGN.md sections 6e "Resampling" and 6k): the fourth
 * header of the library.  These entries are built into libspkhip.so with the kernels of include/spkhip.h and follow its conventions -
 * device pointers, `stream` a hipStream_t or NULL, 0 on success, < 0 with spk_last_error() set where a call is refused on the host
 * before anything is launched - but they are declared here, named spkw_*, bound by their own table (hip._WAV_SIGS,
 * hip.wav_symbols()) and counted apart from the exports of spkhip.h, spkder.h and spkcal.h. */
#ifndef SPKWAV_H
#define SPKWAV_H
#ifdef __cplusplus
extern "C" {
#endif
/* The span form of spk_resample_fwd (same tables first [ou], wq [ceil(K / 2)][ou][2], same rates and limits, same tile for the same
 * (fi, fo, K)).  Row b of wave_in [B][Nmax_in] holds samples [ifirst[b], ifirst[b] + icount[b]) of an utterance of itotal[b] samples;
 * with y_b what spk_resample_fwd writes for that whole utterance,
 *     wave_out[b][i] = y_b[ofirst[b] + i]   for i < ocount[b] (0 where y_b has no such output),   0 from ocount[b] up to Nmax_out
 * bit for bit: the taps of an output are summed in the order of the whole form whatever the alignment of its window in the row.
 * x = 0 outside [0, itotal[b]).  A sample inside the utterance that the row does not hold is NOT read - it counts as 0, and whatever
 * lies at or past icount[b] in the row is ignored - so a caller that asks for outputs its rows do not cover gets wrong values for
 * those outputs and no foreign memory is touched; features.check_resample_spans refuses such rows on the host.
 * ifirst, itotal, ofirst: int64 [B]; icount, ocount: int32 [B] (clamped to [0, Nmax_in], [0, Nmax_out]); itotal[b] < 2^30.
 * rows: NULL (then R == B: every row) or int32 [R], 1 <= R <= B: the rows this launch works on - the others are not touched, so a
 * batch that mixes rates takes one launch per rate into one wave_out; an entry outside [0, B) is skipped.
 * Nothing is read back; nothing synchronises. */
int spkw_resample_span_fwd(const float* wave_in, const long long* ifirst, const int* icount, const long long* itotal,
                           const long long* ofirst, const int* ocount, const int* rows, int R, int B, long long Nmax_in,
                           const int* first, const float* wq, int fi, int fo, int K, float* wave_out, long long Nmax_out,
                           void* stream);
/* The rows of such a batch that are not resampled: wave_out[b][i] = wave_in[b][i] for i < count[b] (clamped to [0, min(Nmax_in,
 * Nmax_out)]), 0 up to Nmax_out, for the rows of the list (rows, R, B as above). */
int spkw_copy_rows_fwd(const float* wave_in, const int* count, const int* rows, int R, int B, long long Nmax_in, float* wave_out,
                       long long Nmax_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
