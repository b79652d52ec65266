// Exact posterior of the number of frames in a set of states under a dwell-time prior (gauss_dwellocc.cpp: host side and C
// ABI; gauss_dwellocc.hip: the kernel).  Private to the library.
//
// With the tables and omega of gauss_dwell.h, G a non-empty proper subset of the states (a bit mask) and g_s = 1 for s in G
// and 0 otherwise, the forward recursion resolved by the number n of the b frames of a partial profile that are in G:
//     A(b, s, n) = [n = g_s b] (log_init[s] + omega_s(0, b) + F[s][b])
//                  (+) log sum_{c = 1 .. b - 1} exp(alpha(c, s, n - g_s (b - c)) + omega_s(c, b) + W[s][c - 1][b])
//     alpha(c, s, n) = log sum_s' exp(A(c, s', n) + log_jump[s'][s])                                   (1 <= c < T, 0 <= n <= c)
// A segment outside G keeps n, a segment inside G adds its length; alpha(c, ., n) is empty outside 0 <= n <= c.  A(T, s, n) is
// the log weight of the profiles with n frames in G that end in s.  End frame b reads alpha of every earlier c at an index
// that shifts with the segment length, so alpha is kept for every c and the end frames are one launch each; A itself never
// goes to memory.  Not normalised on the device: the host subtracts the log evidence of the ordinary forward pass.
#pragma once
#include <stdint.h>

#include "gauss_dwell.h"

namespace bild {

constexpr int kDwellOccWaves = 8;       // waves of a workgroup of the kernel: they stride the switch frame c

struct DwellOccupancy {
    double *alpha;          // per trajectory [c][s][n], c < Tm, n < ld: alpha(c, s, n), written for 1 <= c < T and n <= c alone
    double *last;           // per trajectory [n][s], n < ld: A(T, s, n), written for n <= T alone
    int64_t stride;         // entries of alpha per trajectory: S * Tm * ld
    unsigned target;        // bit s: state s belongs to G
};

// bytes of one trajectory in the call's own tables
constexpr int64_t dwell_occupancy_bytes(int S, int Tm) { return ((int64_t)S * Tm * (Tm + 1) + (int64_t)S * (Tm + 1)) * 8; }

// end frame b = 1 .. Tm of the chunk's trajectories, in ascending order on one stream; a trajectory with T < b has no work.
// Needs the prior tables of p alone
int launch_dwell_occupancy(const DwellParams &p, const DwellOccupancy &o, int b, void *stream);

} // namespace bild
