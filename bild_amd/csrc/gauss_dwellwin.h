// Exact window support under a dwell-time prior (gauss_dwellwin.cpp: host side and C ABI; gauss_dwellwin.hip: the kernel;
// include/bild_amd_windows.h).  Private to the library.
//
// With the tables and omega of gauss_dwell.h, head(0, s) = log_init[s] and head(a, s) = alpha(a, s), w(0, b, s) = F[s][b] and
// w(a, b, s) = W[s][a - 1][b], seg(a, b, s) = omega_s(a, b) + w(a, b, s).  A query is (u, v, G), 0 <= u < v <= T, G a bit mask
// of states: the log weight of the profiles whose frames u .. v - 1 are all in G,
//     C(b, s)     = log[ sum_{a = 0 .. u} exp(head(a, s) + seg(a, b, s)) + sum_{c = u + 1 .. b - 1} exp(kappa(c, s) + seg(c, b, s)) ]
//                                                                                                          u < b < v, s in G
//     kappa(c, s) = log sum_{s' in G} exp(C(c, s') + log_jump[s'][s])                                      u < c < v, s in G
//     num         = log sum_{s in G} sum_{b = v .. T} [ sum_{a <= u} exp(head(a, s) + seg(a, b, s) + gamma(b, s))
//                                                       + sum_{u < c < v} exp(kappa(c, s) + seg(c, b, s) + gamma(b, s)) ]
// alpha is the ordinary forward pass's and gamma the backward pass's (kDwellForward | kDwellBackward).  num is not normalised
// on the device: the host subtracts the log evidence of the full forward pass.  A NaN table entry enters no sum.
#pragma once
#include <stdint.h>

#include "gauss_dwell.h"

namespace bild {

constexpr int kDwellWinWaves = 8;       // waves of a workgroup: one query each workgroup

struct DwellWinQuery {
    int32_t traj;           // the trajectory's slot in the chunk
    int32_t u, v;           // the window [u, v)
    uint32_t target;        // bit s: state s belongs to G
    int64_t kappa;          // the query's row in DwellWindows::kappa: kappa(c, s) at [s * (v - u - 1) + (c - u - 1)]
};

struct DwellWindows {
    const DwellWinQuery *queries;   // the chunk's queries
    double *kappa;                  // the chunk's scratch rows
    double *num;                    // per query of the chunk
    int n;                          // queries of the chunk (> 0)
};

// needs p.alpha (launch_dwell_forward) and p.gamma (launch_dwell_backward)
int launch_dwell_windows(const DwellParams &p, const DwellWindows &o, void *stream);

} // namespace bild
