// Gradient of the exact evidence under a dwell-time prior with respect to model parameters (gauss_dwellsens.cpp: host side and
// C ABI; gauss_dwellsens.hip: the weight kernel).  Private to the library.
//
// With the tables of gauss_dwell.h the posterior weight of a segment [a, b) in state s is
//     Q(a, b, s) = exp(alpha(a, s) + omega_s(a, b) + W[s][a - 1][b] + gamma(b, s) - logev)
// (a = 0: log_init[s] in place of alpha and F in place of W), and
//     Omega(s, a, t) = sum_{b > t} Q(a, b, s)
// is the posterior probability that a segment in state s starts at a and has not ended by frame t.  Omega is written in
// the layout gauss_segsens.h describes, so that the weighted tangent jobs of section 20 (gauss_segtangent.h) read it as
// they read the table of the segment recursion.
#pragma once
#include <stdint.h>

#include "gauss_dwell.h"

namespace bild {

struct DwellsensWeights {
    double *omega;          // per trajectory om_slot doubles
    int64_t om_slot;        // S * (w_per_state(Tm) + ld)
    int64_t om_tri;         // w_per_state(Tm)
};

// needs p.alpha, p.gamma, p.fin and the prior tables: behind launch_dwell_forward and launch_dwell_backward
int launch_dwellsens_weight(const DwellParams &p, const DwellsensWeights &w, void *stream);

} // namespace bild
