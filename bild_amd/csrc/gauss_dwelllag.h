// Exact fixed-lag smoothing under a dwell-time prior (gauss_dwelllag.cpp: host side and C ABI; gauss_dwelllag.hip: the kernels;
// DESIGN.md section 26).  Private to the library.
//
// A cut u = 1 .. T is the truncated trajectory x[:u]; a window's table entry depends on the data inside the window alone, so the
// tables of the whole trajectory serve every cut.  With the tables of gauss_dwell.h, head(0, s) = log_init[s], w(0, b, s) =
// F[s][b], head(a, s) = alpha(a, s), w(a, b, s) = W[s][a - 1][b] (a >= 1), omega_u(a, b, s) = log_dwell[s][b - a] for b < u and
// log_surv[s][u - a] for b = u:
//     gamma_u(u, s) = 0,  beta_u(a, s) = log sum_{a < b <= u} e^(omega_u(a, b, s) + W[s][a - 1][b] + gamma_u(b, s)),
//     gamma_u(a, s) = log sum_s'' e^(log_jump[s][s''] + beta_u(a, s''))
//     J_u(t, s)     = log sum_{a <= t < b <= u} e^(head(a, s) + omega_u(a, b, s) + w(a, b, s) + gamma_u(b, s))
//     E(u)          = log sum_s e^J_u(u - 1, s)
// and the answer at frame t and lag l is J_u(t, s) - E(u) with u = min(t + l + 1, T).  The starts a of every sum are split at the
// left edge of the window of `lag` + 1 frames behind the end frame:
//     Hbase(b, s) = log sum_{a <= b - 1 - lag} e^(head(a, s) + log_dwell[s][b - a] + w(a, b, s)),  Kbase(b, s) with log_surv
// which depend on no cut, and the starts b - lag <= a <= t, which a cut's wave adds frame by frame.
#pragma once
#include <stdint.h>

#include "gauss_dwell.h"

namespace bild {

constexpr int kDwellLagMax = 63;    // lag + 1 frames of a window are the lanes of one wavefront (BILD_DWELL_LAG_MAX of the C ABI)
constexpr int kDwellLagCuts = 4;    // cuts (waves) of one workgroup of the window kernel

struct DwellLag {
    double *Hbase, *Kbase;  // per trajectory [s][ld]: end frame b at [b], b = 1 .. T
    double *lagged;         // per trajectory [s][Tm][lag + 1]
    int lag;
};

// bytes of one trajectory in the tables above (needs no device)
inline int64_t dwell_lag_bytes(int S, int Tm, int lag) { return (int64_t)S * (2 * (Tm + 1) + (int64_t)Tm * (lag + 1)) * 8; }

// need p.alpha, p.alphaArg and the prior tables: behind launch_dwell_forward; the windows need the bases
int launch_dwell_lag_bases(const DwellParams &p, const DwellLag &o, void *stream);
int launch_dwell_lag_windows(const DwellParams &p, const DwellLag &o, void *stream);

} // namespace bild
