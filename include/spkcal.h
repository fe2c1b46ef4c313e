/* libspkhip - calibration and fusion of trial scores (csrc/cal.hip): the third header of the library.  These
 * entries are built into libspkhip.so with the kernels of include/spkhip.h and follow its conventions - device pointers unless marked
 * HOST, `stream` a hipStream_t or NULL, 0 on success, < 0 with spk_last_error() set where a call is refused on the host before
 * anything is launched - but they are declared here, bound by their own table (hip._CAL_SIGS, hip.cal_symbols()) and counted apart
 * from spkhip.h's and spkder.h's exports. */
#ifndef SPKCAL_H
#define SPKCAL_H
#ifdef __cplusplus
extern "C" {
#endif
/* Everything is fp64 with every operation rounded on its own, or int64.  T trials, 2 <= T < 2^31; K systems, 1 <= K <= spk_cal_max_k()
 * = 8; cols [K][T]: column k holds system k's score of every trial; label [T]: non-zero = target.  No value may be NaN or infinite:
 * the caller checks that. */
int spk_cal_max_k(void);
/* sizes: 0 = trials per block of apply / cllr / the evaluation pass / the tie-pool scan, 1 = pools per tile of spk_cal_pav, 2 = the
 * doubles of the training state, 3 = threads per block */
int spk_cal_tile(int which);
/* llr [T] = ((theta[0] cols[0] + theta[1] cols[1]) + ...) + theta[K], left to right.  theta: HOST [K + 1], weights then bias.  T >= 1. */
int spk_cal_apply(const double* cols, const double* theta /*host [K+1]*/, int K, double* llr, int T, void* stream);
/* host only: the 8-byte words of workspace of the call of that name; < 0 for a shape it refuses */
long long spk_cal_cllr_ws_elems(int T);
long long spk_cal_train_ws_elems(int T, int K);
long long spk_cal_pav_ws_elems(int T);
/* One pass over llr [T].  costs: HOST [P][3] = (p_target, c_miss, c_fa), eta: HOST [P], the Bayes threshold of each triple as the
 * caller computed it; P <= 8.  out_d [2 + P] = sum over targets of softplus(-llr), sum over non-targets of softplus(llr), then actDCF
 * per triple = (c_miss (miss / N_tar) p + c_fa (fa / N_non) (1 - p)) / min(c_miss p, c_fa (1 - p)); out_i [2 + 2 P] = N_tar, N_non,
 * miss [P] = #{targets: llr < eta}, fa [P] = #{non-targets: llr >= eta}.  The sums are per-block trees added in block order. */
int spk_cal_cllr(const double* llr, const unsigned char* label, const double* costs /*host [P][3]*/, const double* eta /*host [P]*/,
                 int P, double* out_d, long long* out_i, void* ws, long long ws_elems, int T, void* stream);
/* Prior-weighted logistic regression from theta = 0 by the damped Newton state machine of section 6s: max_iters pairs of launches
 * (one pass over the trials: f, g, H at theta as per-block partial sums; one workgroup: their sum in block order, Cholesky, the four
 * transitions) are put on the stream and the call returns; once the machine has stopped the remaining launches return at once.
 * n_tar: the targets among label; tau = logit(p_target) as the caller computed it.  state [spk_cal_tile(2)] doubles: theta [9] at 0,
 * the last accepted theta [9] at 9 (the result), the step [9] at 18, its objective at 27, the last objective at 28, lambda2 at 29,
 * g [9] at 30, the lower triangle of H [45] at 40; istate [4] = status (0 running, 1 converged, 2 not_converged, 3 singular),
 * evaluations used, Newton steps, halvings. */
int spk_cal_train(const double* cols, const unsigned char* label, int K, int T, long long n_tar, double p_target, double tau, double l2,
                  double epsilon, int max_iters, double* state, long long* istate, double* ws, long long ws_elems, void* stream);
/* minCllr by pool-adjacent-violators in int64.  order [T]: what spk_sort_trials gives for score.  tie [T][2]: the pools of equal
 * scores as (targets, trials), counts[0] of them; pools [T][2]: the final pools, counts[3] of them, t / n strictly increasing;
 * pool_of [T]: each trial's final pool; out_d [1] = minCllr; counts [8] = tie pools, pools left by the rule inside tiles, pools left
 * by a second round of tiles over their concatenation, final pools, N_tar.  upto: 1 = stop after the tie pools, 2 = after the tiles,
 * anything else = all of it. */
int spk_cal_pav(const double* score, const unsigned char* label, const unsigned* order, long long* tie, long long* pools,
                long long* counts, int* pool_of, double* out_d, long long* ws, long long ws_elems, int T, int upto, void* stream);

#ifdef __cplusplus
}
#endif
#endif
