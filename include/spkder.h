/* libspkhip - diarization scoring (csrc/der.hip): the second header of the library.  These entries are built into
 * libspkhip.so with the kernels of include/spkhip.h and follow its conventions - device pointers unless marked HOST, `stream` a
 * hipStream_t or NULL, 0 on success, < 0 with spk_last_error() set where a call is refused on the host before anything is launched -
 * but they are declared here, bound by their own table (hip._DER_SIGS, hip.der_symbols()) and counted apart from spkhip.h's exports. */
#ifndef SPKDER_H
#define SPKDER_H
#ifdef __cplusplus
extern "C" {
#endif
/* All times are int64 ticks; everything is integer arithmetic, so a correct implementation has one answer.
 * spk_ahc_cut_batch: the labels of K cuts of the merge lists spk_ahc_batch wrote (merges, merge_cost, n_merges: the same layout), one
 * workgroup per (recording, threshold).  Cut k of recording r applies the longest prefix of its merges whose costs all satisfy
 * c <= -thresholds[k] (the stopping rule of spk_ahc_batch) and numbers the clusters 1, 2, ... by lowest member window:
 * labels [K][Ntot] equals what spk_ahc_batch gives at that threshold.  n_r <= spk_ahc_max_n().  rec_off is given twice: the HOST
 * array, checked, and its device copy.  Refused on the host (< 0, nothing written): a bad rec_off, a recording over the cap, K or R
 * outside [1, 65535], a null pointer. */
int spk_ahc_cut_batch(const int* merges /*[Ntot][2]*/, const double* merge_cost /*[Ntot]*/, const int* n_merges /*[R]*/,
                      const long long* rec_off /*host [R+1]*/, const long long* rec_off_dev /*[R+1]*/,
                      const double* thresholds /*[K]*/, int K, int* labels /*[K][Ntot]*/, long long Ntot, int R, void* stream);
/* The hypothesis of every cut: window w of a recording (the windows in (start, end) order, wstart / wend in ticks) with make_rttm's
 * adjacent-pair cut: where the neighbour's label differs and the two overlap, the shared side moves to (a + b) >> 1, a the later
 * start and b the earlier end.  pstart, pend [K][Ntot]. */
int spk_der_pieces(const int* labels /*[K][Ntot]*/, const long long* wstart /*[Ntot]*/, const long long* wend /*[Ntot]*/,
                   const long long* rec_off /*host [R+1]*/, const long long* rec_off_dev /*[R+1]*/, int K, long long* pstart,
                   long long* pend, long long Ntot, int R, void* stream);
/* the limits of one spk_der_batch job: reference speakers (64), hypothesis labels (1024), hypothesis pieces (8192) */
int spk_der_max_ref(void);
int spk_der_max_hyp(void);
int spk_der_max_turns(void);
/* host only: the 8-byte words of workspace one job needs (its pieces' disjoint starts, their order by start, and C where Sr Sh
 * exceeds what LDS holds: 4096 entries); < 0 over a limit */
long long spk_der_ws_elems(int pieces, int Sr, int Sh);
/* Scores J jobs, one workgroup each (no workgroup waits on another; every loop has a bound known at launch).  The reference side is
 * prepared on the host, once per recording: rec_tab [R][4] = (first cell, cells, Sr, 0) and cells [ncells][3] = (start, end, mask):
 * the scored set S (UEM or reference extent, minus collars, minus overlap where asked) as sorted disjoint intervals on each of which
 * the set of active reference speakers is constant, bit i of mask = speaker i.  job_tab [J][6] = (recording, first piece, pieces, Sh,
 * workspace offset in 8-byte words, 0): the job's hypothesis is plab / pstart / pend [first piece .. + pieces), labels in 1 .. Sh, in
 * any order and overlapping freely (a piece with another label or with end <= start is ignored); the workspaces of two jobs must not
 * overlap.  out [J][5] = scored, miss, fa, conf, opt as section 6r defines them; mapping [J][spk_der_max_ref()]: the label assigned to
 * reference speaker i, or -1 (pairs that share no tick are not reported): an optimum of the assignment, solved in the workgroup on
 * exact int64 values.  rec_tab and job_tab are given twice: HOST arrays, checked, and their device copies.  Refused on the host (< 0,
 * nothing written): a table entry outside its array, Sr, Sh or pieces over the limits, a workspace that is too small, a null pointer. */
int spk_der_batch(const long long* rec_tab /*host [R][4]*/, const long long* rec_tab_dev, const long long* cells /*[ncells][3]*/,
                  long long ncells, int R, const long long* job_tab /*host [J][6]*/, const long long* job_tab_dev, int J,
                  const int* plab, const long long* pstart, const long long* pend, long long npieces, long long* ws,
                  long long ws_elems, long long* out /*[J][5]*/, int* mapping /*[J][64]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif
