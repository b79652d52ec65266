/*
 * bild_amd_visits.h -- the C ABI of libbild_amd.so beyond bild_amd.h: exact visit counts under a dwell-time prior.
 * The conventions of bild_amd.h hold (return codes, bild_last_error, row-major arrays, logs).
 */
#ifndef BILD_AMD_VISITS_H
#define BILD_AMD_VISITS_H

#include "bild_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- visits to a set of states under a dwell-time prior ----
 * GenericGaussianModel only, at most 4 states.  The exact posterior distribution of the number N of
 * visits to the set G (bit s of target: state s belongs to G), jointly with the last state, under the dwell-time prior of
 * bild_gauss_dwell_evidence (same tables, same NaN flag).  A visit is a maximal run of consecutive frames with theta_t in G:
 * a run that begins at frame 0 counts, a run that the end of the trajectory cuts off counts, and a jump between two states
 * of G continues the visit, so 0 <= N <= (T + 1) / 2.  That block's forward recursion resolved by the number n of visits
 * that have begun, with g_s = 1 for s in G and 0 otherwise:
 *   A(b, s, n)     = [n = g_s] (log_init[s] + omega_s(0, b) + F[s][b])
 *                    (+) log sum_{c = 1 .. b - 1} exp(alpha(c, s, n) + omega_s(c, b) + W[s][c - 1][b])
 *   alpha(c, s, n) = log sum_r exp(A(c, r, n - [r not in G and s in G]) + log_jump[r][s])                       (1 <= c < T)
 * A segment keeps n; a jump into G from outside adds one.  One launch per end frame b, alpha kept for every c:
 * S T_longest (min(n_max, (T_longest + 1) / 2) + 1) doubles per trajectory of a chunk beside the forward tables (8 MB at
 * T = 1000, 2 states and the complete n_max).  Rows n > n_max are neither kept nor fed: what enters G from row n_max is
 * dropped.  Per trajectory of T frames:
 *   logev, n_nan_windows   as bild_gauss_dwell_evidence gives them, bit for bit: the same forward kernel on the same tables
 *   log_visits     (n_max + 1) x S: entry [n][s] = A(T, s, n) - logev = log P(N = n, theta_{T-1} = s | x); -inf where the
 *                  probability is 0, and -inf for n > (T + 1) / 2
 *   log_tail       log P(N > n_max | x), formed on the host as log(max(0, 1 - sum exp(log_visits))), the sum over n ascending
 *                  and s ascending inside: a difference from 1; -inf exactly when n_max >= (T + 1) / 2
 * Every entry is normalised by logev of the ordinary forward pass, not by their sum: sum exp(log_visits) = 1 at a complete
 * n_max holds up to rounding and is a check, not a construction.  A NaN window enters no sum.  flags = 0
 * (BILD_DWELL_NAN_PROPAGATE): a trajectory with n_nan_windows > 0 has NaN in logev, log_visits and log_tail; the other
 * trajectories are untouched.  BILD_DWELL_NAN_OMIT: the skipped windows weigh 0.  A trajectory without a profile of positive
 * weight has logev -inf and NaN in log_visits and log_tail.  The switch frames c of an entry are summed by eight waves, wave q
 * taking c = c0 + q, c0 + q + 8, .. in ascending order from the first c0 that can reach the entry's tile of 63 values of n,
 * the waves merged in wave order: no atomics, fixed summation orders that depend on the trajectory alone, so results are
 * bit-identical across calls, the order of the set, a trajectory alone or in a batch, n_max (the rows kept) and scratch_bytes
 * (chunks of whole trajectories; 0: at most 1 GiB and a third of the free device memory).  Refused before any device work:
 * what bild_gauss_dwell_occupancy refuses -- a target that is empty, names a state the model does not have or holds every
 * state, so a model of one state is always refused -- and a negative n_max (BILD_ERR_INVALID).  Plain launches on the set's
 * stream.  Synchronous. */
typedef struct bild_dwell_visits_out {
    double *logev;                          /* n_traj */
    int64_t *n_nan_windows;                 /* n_traj */
    double *log_visits;                     /* n_traj x (n_max + 1) x S */
    double *log_tail;                       /* n_traj */
} bild_dwell_visits_out;                    /* every pointer may be NULL: not written */

int bild_gauss_dwell_visits(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                            const double *log_jump, const double *log_dwell, const double *log_surv, int T_max, int n_max,
                            unsigned target, unsigned flags, int64_t scratch_bytes, bild_dwell_visits_out *out);

#ifdef __cplusplus
}
#endif
#endif /* BILD_AMD_VISITS_H */
