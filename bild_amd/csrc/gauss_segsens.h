// Gradient of the exact evidence of GenericGaussianModel with respect to model parameters (gauss_segsens.cpp: host side
// and C ABI; gauss_segsens.hip: kernels).  Private to the library.
//
// By Fisher's identity the gradient of log sum_k pi_k ev_k is the posterior mean of the gradient of the log-likelihood.
// The posterior weight of "a segment starts at a in state s and has not ended by frame t" is
//     Omega(s, a, t) = sum_k k_post[k] sum_{b > t} Q_k(a, b, s) / total_k
// (Q_k: gauss_segdp.hip, the marginals), and a window's term is minus the sum of tau_j over its counted entries, so
//     grad_p = - sum_{s, a, j} Omega(s, a, t_j) dtau_{a, j, p}
// with t_j the frame of entry j of the tau row of window start a - 1 (gauss.hip).  Omega is stored per trajectory and
// state in W's triangular layout: row a >= 1 at gauss_wrow(T, a - 1), entry t at + (t + 1 - a) (the place of W[a - 1][t + 1]);
// behind the S triangles of w_per_state(Tm) doubles lie S first-segment rows (a = 0) of ld = Tm + 1 doubles, entry t at t.
#pragma once
#include <stdint.h>

#include "gauss.h"
#include "gauss_segdp.h"

namespace bild {

struct SegsensWeights {
    const double *coef;     // per (trajectory, k): k_post[k] / sum_s Z_k(T, s) exp(M_k(T, s) - top_k); 0: k is skipped
    const double *top;      // per (trajectory, k): top_k, the scale of Q_k (segdp_top)
    double *omega;          // per trajectory om_slot doubles
    int64_t om_slot;        // S * (w_per_state(Tm) + ld)
    int64_t om_tri;         // w_per_state(Tm)
};

// a weighted tangent job: gauss.h's job (its set, rank, entries, output row, factor slot) and where its weights lie
struct SegsensJob {
    GaussSensJob j;
    int64_t om;             // first == 0: the (trajectory, state) triangle; first == 1: its first-segment row
    int T;                  // the trajectory's frames (row offsets of the triangle)
    int a_lo, a_hi;         // segment starts a whose window start a - 1 uses this tau row: their weights are added, ascending
    int first;              // the first interval
    int pad;
};

int launch_segsens_weight(const SegdpParams &p, const SegsensWeights &w, void *stream);
int launch_segsens_solve(const GaussSensSet *sets, const SegsensJob *jobs, int njobs, int P, int nmax, const double *omega,
                         double *out, void *stream);
int launch_segsens_factor(const GaussSensSet *sets, const SegsensJob *jobs, int njobs, int P, const double *omega, double *base,
                          double *out, void *stream);

} // namespace bild
