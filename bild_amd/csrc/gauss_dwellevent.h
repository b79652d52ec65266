// Exact switch counts and first-contact times under a dwell-time prior (gauss_dwellevent.cpp: host side and C ABI;
// gauss_dwellevent.hip: the kernels).  Private to the library.
//
// With the tables and omega of gauss_dwell.h, the forward recursion resolved by the number n of switches:
//     A_0(b, s) = log_init[s] + omega_s(0, b) + F[s][b]
//     A_n(b, s) = log sum_{c = n .. b - 1} exp(alpha_{n-1}(c, s) + omega_s(c, b) + W[s][c - 1][b])       (n >= 1, n < b <= T)
//     alpha_n(c, s) = log sum_s' exp(A_n(c, s') + log_jump[s'][s])                                        (1 <= c < T)
// A_n(T, s) is the log weight of the profiles of n switches that end in s.  Level n reads level n - 1 alone, so a level is
// one launch without a sequential chain, and only alpha_{n-1} and alpha_n are kept: two rows of S (Tm + 1) entries that
// the levels use in turn, and the column A_n(T, .) of every level.
//
// First contact with a set G of states (a bit mask): Ax is the table A of the ordinary forward pass under the prior with
// log_init[s] = log_jump[.][s] = -inf for s in G (DwellCall's second prior block), beta and gamma those of the full prior:
//     first(0) = log sum_{s in G} exp(log_init[s] + h(s)),   h(s) = log sum_{b = 1 .. T} exp(omega_s(0, b) + F[s][b] + gamma(b, s))
//     first(t) = log sum_{s' not in G} sum_{s in G} exp(Ax(t, s') + log_jump[s'][s] + beta(t, s))        (1 <= t < T)
//     never    = log sum_{s' not in G} exp(Ax(T, s'))
// None of them is normalised on the device: the host subtracts the log evidence of the full forward pass.
#pragma once
#include <stdint.h>

#include "gauss_dwell.h"

namespace bild {

constexpr int kDwellEventWaves = 8;     // waves of a workgroup of the level kernel: they stride the switch frame c

struct DwellLevels {
    double *lev;            // per trajectory 2 x [s][ld]: alpha_n at row n & 1
    double *last;           // per trajectory (k_max + 1) x S: A_n(T, s); level n of a trajectory with T <= n is not written
    int k_max;
};

struct DwellContact {
    const double *Ax;       // the table A of the forward pass on the second prior block, per trajectory [s][ld]
    double *first;          // per trajectory ld entries: first(t) at [t], t < T, and never at [Tm]
    unsigned target;        // bit s: state s belongs to G
};

// level n = 0 .. k_max of the chunk's trajectories; needs the prior tables of p alone
int launch_dwell_level(const DwellParams &p, const DwellLevels &o, int n, void *stream);
// needs p.beta and p.gamma (launch_dwell_backward) and o.Ax (launch_dwell_forward on the second block)
int launch_dwell_contact(const DwellParams &p, const DwellContact &o, void *stream);

} // namespace bild
