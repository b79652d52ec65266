// Expected segment-length counts under a dwell-time prior (gauss_dwelllen.cpp: host side and C ABI; gauss_dwelllen.hip: the
// kernels).  Private to the library.
//
// With the tables of gauss_dwell.h and the segment weight of gauss_dwellsens.h,
//     Q(a, b, s) = exp(alpha(a, s) + omega_s(a, b) + W[s][a - 1][b] + gamma(b, s) - logev)      (a = 0: log_init[s] and F),
// the derivatives of logev with respect to the prior's length tables are sums of Q along the diagonals b - a = l:
//     D[s][l] = sum_{a = 0}^{T - l - 1} Q(a, a + l, s)     completed segments of length l      (d logev / d log_dwell[s][l])
//     C[s][l] = Q(T - l, T, s)                             the last segment, censored at l     (d logev / d log_surv[s][l])
//     I[s]    = sum_{b = 1}^{T} Q(0, b, s)                 P(theta_0 = s)
// The start frames a are cut into blocks of kDwellLenBlock; a block's share of D is summed over ascending a, the shares are
// added in block order: every order depends on the trajectory alone.
#pragma once
#include <stdint.h>

#include "gauss_dwell.h"

namespace bild {

constexpr int kDwellLenBlock = 64;      // start frames of one block: a multiple of kDwellTile, aligned to the trajectory.  A wave's
                                        // chain of dependent-latency steps is this long: short blocks, many waves

struct DwellLengths {
    double *part;           // per (trajectory, s, block, l): the block's share of D[s][l], Tm entries a block, length l at [l - 1]
    double *dwell, *cens;   // per trajectory [s][ld]: D and C, length l at [l - 1]; written for l = 1 .. T
    double *init;           // per trajectory S
    int nblk;               // blocks of the longest trajectory
};

// needs p.alpha, p.gamma, p.fin and the prior tables: behind launch_dwell_forward and launch_dwell_backward
int launch_dwell_lengths(const DwellParams &p, const DwellLengths &o, void *stream);

} // namespace bild
