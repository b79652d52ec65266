/*
 * bild_amd_windows.h -- the C ABI of libbild_amd.so beyond bild_amd.h: exact window support under a dwell-time prior.
 * The conventions of bild_amd.h hold (return codes, bild_last_error, row-major arrays, logs).
 */
#ifndef BILD_AMD_WINDOWS_H
#define BILD_AMD_WINDOWS_H

#include "bild_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- window support under a dwell-time prior ----
 * GenericGaussianModel only, at most 4 states.  For every query (u, v, G) on a trajectory of T frames,
 * 0 <= u < v <= T, G a set of states (bit s of the target: state s belongs to G), the exact posterior probability that every
 * frame of [u, v) is in G, under the dwell-time prior of bild_gauss_dwell_evidence (same tables, same NaN flag).  With that
 * block's alpha, gamma and omega, head(0, s) = log_init[s] and head(a, s) = alpha(a, s), w(0, b, s) = F[s][b] and
 * w(a, b, s) = W[s][a - 1][b], seg(a, b, s) = omega_s(a, b) + w(a, b, s):
 *   C(b, s)     = log[ sum_{a = 0 .. u} exp(head(a, s) + seg(a, b, s)) + sum_{c = u + 1 .. b - 1} exp(kappa(c, s) + seg(c, b, s)) ]
 *                                                                                                       (u < b < v, s in G)
 *   kappa(c, s) = log sum_{s' in G} exp(C(c, s') + log_jump[s'][s])                                     (u < c < v, s in G)
 *   num         = log sum_{s in G} sum_{b = v .. T} [ sum_{a <= u} exp(head(a, s) + seg(a, b, s) + gamma(b, s))
 *                                                     + sum_{u < c < v} exp(kappa(c, s) + seg(c, b, s) + gamma(b, s)) ]
 *   log_all     = num - logev
 * The forward recursion restricted to the states of G over the window, started from the unconstrained alpha at the window's
 * left edge and closed with the backward tables at its right edge.  The complement, P(some frame of [u, v) is in G), is
 * 1 - exp(log_all) of the complement of G.  The queries: win_traj[i] the trajectory of query i, NOT DECREASING in i;
 * win_u[i], win_v[i] its window; win_target[i] its bit mask.  A trajectory may have any number of queries, none included.
 *   logev, n_nan_windows   per trajectory, as bild_gauss_dwell_evidence gives them, bit for bit: the same forward kernel on
 *                          the same tables
 *   log_all                per query; -inf where the probability is 0
 * Normalised by logev of the full forward pass.  A NaN window enters no sum.  flags = 0 (BILD_DWELL_NAN_PROPAGATE): the
 * queries of a trajectory with n_nan_windows > 0 (of the full pass) are NaN, as is its logev; the other trajectories are
 * untouched.  BILD_DWELL_NAN_OMIT: the skipped windows weigh 0.  A trajectory without a profile of positive weight has logev
 * -inf and NaN in its queries.  One workgroup of eight wavefronts per query, one launch per chunk: the chain C in tiles of 64
 * end frames (the wavefronts stride the start frames left of a tile and are merged in wavefront order; the tile's triangle by
 * one wavefront), then num with the wavefronts striding the start frame and the lanes the end frame, states ascending, merged
 * by butterflies and in wavefront order: no atomics, fixed summation orders that depend on the trajectory and the query
 * alone, so results are bit-identical across calls, the order of the set and of the queries, a trajectory alone or in a
 * batch, and scratch_bytes (chunks of whole trajectories with the forward and backward tables and S (v - u - 1) doubles a
 * query; 0: at most 1 GiB and a third of the free device memory).  Refused before any device work (BILD_ERR_INVALID): what
 * bild_gauss_dwell_first_contact refuses, n_win < 0, a NULL array with n_win > 0, a win_traj outside the set or smaller than
 * its predecessor, a window outside 0 <= u < v <= T of its trajectory, and a target that is empty, names a state the model
 * does not have or holds every state: a model of one state has no valid query.  Plain launches on the set's stream.
 * Synchronous. */
typedef struct bild_dwell_windows_out {
    double *logev;                          /* n_traj */
    double *log_all;                        /* n_win */
    int64_t *n_nan_windows;                 /* n_traj */
} bild_dwell_windows_out;                   /* every pointer may be NULL: not written */

int bild_gauss_dwell_windows(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                             const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                             int64_t scratch_bytes, int64_t n_win, const int32_t *win_traj, const int32_t *win_u,
                             const int32_t *win_v, const uint32_t *win_target, unsigned flags, bild_dwell_windows_out *out);

#ifdef __cplusplus
}
#endif
#endif /* BILD_AMD_WINDOWS_H */
