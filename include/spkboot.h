/* libspkhip - speaker-level bootstrap of the error-rate sweep (csrc/boot.hip): the fifth header of the library.
 * These entries are built into libspkhip.so and follow the conventions of include/spkhip.h - device pointers unless marked HOST,
 * `stream` a hipStream_t or NULL, 0 on success, < 0 with spk_last_error() set where a call is refused on the host before anything is
 * launched - but they are declared here, named spkb_*, bound by their own table (hip._BOOT_SIGS, hip.boot_symbols()) and counted apart
 * from the other four headers' exports. */
#ifndef SPKBOOT_H
#define SPKBOOT_H
#ifdef __cplusplus
extern "C" {
#endif
/* T trials, 2 <= T < 2^31, sorted by spk_sort_trials; U units, 1 <= U <= 65 535, both sides of a trial in one unit space; a replicate
 * is a row of counts c [U] <= 65 535 and trial (a, b) weighs c[a] c[b], or c[a] when a = b.  Counts are int64, rates and costs fp64
 * with every operation rounded on its own. */
/* host only: 0 = positions per workgroup (the tile), 1 = largest U, 2 = largest count, 3 = cost triples per call (each of P and Pa),
 * 4 = replicates per workgroup at most, 5 = threads per workgroup; < 0 otherwise */
int spkb_limit(int which);
/* host only: entries per row of the device count table, (U + 7) & ~7 (rows start on 16 bytes; the padding is never read as a unit) */
int spkb_pitch(int U);
/* host only: replicates a workgroup sweeps with its records held in registers - the rows that fit 64 KiB of LDS, 1 ... 16 */
int spkb_group(int U);
/* Once per system.  rec [T]: 8 bytes per sorted position, ua | ub << 16 and the label; q [P] = the number of sorted scores below
 * eta [P] (HOST; the Bayes thresholds as the caller computed them), P <= 8.  label [T] non-zero = target, order [T] from
 * spk_sort_trials over score [T], ua / ub [T] in [0, U): the caller checks the range. */
int spkb_pack(const double* score, const unsigned char* label, const unsigned* order, const int* ua, const int* ub,
              const double* eta /*host [P]*/, int P, void* rec, long long* q, int T, int U, void* stream);
/* host only: the 8-byte words of workspace of spkb_sweep for a chunk of Rc replicates; < 0 for a shape it refuses */
long long spkb_sweep_ws_elems(int T, int P, int Pa, int Rc);
/* A chunk of Rc replicates.  counts [Rc][spkb_pitch(U)] uint16, on 16 bytes; cmax: a bound of every count the caller vouches for,
 * cmax^2 T < 2^53.  costs: HOST [P][3] = (p_target, c_miss, c_fa) of the minimum costs, act_costs: HOST [Pa][3] of the actual costs
 * with q [Pa] from spkb_pack.  Per replicate: out_d [Rc][1 + P + Pa] = EER, minDCF [P], actDCF [Pa]; out_i [Rc][4 + P + 2 Pa] = flag,
 * N_tar, N_non, EER position, minDCF position [P], miss [Pa], fa [Pa].  flag 1 = no target or no non-target weight: every double is
 * NaN, every position and count after N_non is -1.  The lowest position wins every tie.  upto: 1 = stop after the sums per (replicate,
 * tile), 2 = after their scan, 3 = after the rates (measurement: the outputs are then not written), anything else = all of it. */
int spkb_sweep(const void* rec, const unsigned short* counts, int U, int Rc, int cmax, const double* costs /*host [P][3]*/, int P,
               const double* act_costs /*host [Pa][3]*/, const long long* q, int Pa, double* out_d, long long* out_i, long long* ws,
               long long ws_elems, int T, int upto, void* stream);

#ifdef __cplusplus
}
#endif
#endif
