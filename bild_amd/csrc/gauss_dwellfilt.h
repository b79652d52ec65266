// Exact online filtering under a dwell-time prior (gauss_dwellfilt.cpp: host side and C ABI; gauss_dwellfilt.hip: the kernel;
// DESIGN.md section 25).  Private to the library.
//
// With the tables of gauss_dwell.h, for the prefix ends b = 1 .. T (frame t = b - 1):
//     G(b, s) = log( init_s e^log_surv[s][b] e^F[s][b] + sum_{c = 1}^{b - 1} e^(alpha(c, s) + log_surv[s][b - c] + W[s][c - 1][b]) )
//     E(b)    = log sum_s e^G(b, s)
// E(b) is the evidence of x[:b]: the forward sum at end frame b with the last segment censored.  alpha is complete behind the
// forward pass, so no term waits for another.  A window's table entry depends on the data inside the window alone, so the
// tables of the whole trajectory serve every prefix.
#pragma once
#include <stdint.h>

#include "gauss_dwell.h"

namespace bild {

struct DwellFilter {
    double *prefix;         // per trajectory Tm: E(t + 1)
    double *filt;           // per trajectory [s][Tm]: G(t + 1, s) - E(t + 1)
    double *run_mean;       // per trajectory Tm: sum_s sum_c (b - c) term / e^E(b)
    int32_t *n_surv;        // per trajectory Tm: nG(t + 1), the NaN windows [c, b) with a reachable start and a finite log_surv weight
    int32_t *n_dwell;       // per trajectory Tm: nA(t + 1), the same with the log_dwell weight
    double *log_run;        // per trajectory [s][Tm][R]: the single term with c = b - r, minus E(b), at [r - 1]; null: not asked for
    int R;                  // run lengths kept (0 without log_run)
};

// bytes of one trajectory in the tables above (needs no device)
inline int64_t dwell_filter_bytes(int S, int Tm, int R) { return (int64_t)Tm * ((2 + S) * 8 + 2 * 4) + (int64_t)S * Tm * R * 8; }

// needs p.alpha, p.alphaArg and the prior tables: behind launch_dwell_forward
int launch_dwell_filter(const DwellParams &p, const DwellFilter &o, void *stream);

} // namespace bild
