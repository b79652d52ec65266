// Exact posterior of the number of visits to a set of states under a dwell-time prior (gauss_dwellvis.cpp: host side and C
// ABI; gauss_dwellvis.hip: the kernel).  Private to the library.
//
// With the tables and omega of gauss_dwell.h, G a non-empty proper subset of the states (a bit mask) and g_s = 1 for s in G
// and 0 otherwise, a visit is a maximal run of frames in G, and the forward recursion is resolved by the number n of visits
// that have begun before the end frame b of a partial profile:
//     A(b, s, n) = [n = g_s] (log_init[s] + omega_s(0, b) + F[s][b])
//                  (+) log sum_{c = 1 .. b - 1} exp(alpha(c, s, n) + omega_s(c, b) + W[s][c - 1][b])
//     alpha(c, s, n) = log sum_r exp(A(c, r, n - [r not in G and s in G]) + log_jump[r][s])                    (1 <= c < T)
// A segment keeps n; a jump into G from outside adds one.  A(b, ., n) is empty for n > ceil(b / 2) and alpha(b, s, n) for
// n > ceil(b / 2) + g_s.  A(T, s, n) is the log weight of the profiles with n visits that end in s.  Rows n > n_top are
// neither kept nor fed.  End frame b reads alpha of every earlier c, so alpha is kept for every c and the end frames are one
// launch each; A itself never goes to memory.  Not normalised on the device: the host subtracts the log evidence of the
// ordinary forward pass.
#pragma once
#include <stdint.h>

#include "gauss_dwell.h"

namespace bild {

constexpr int kDwellVisWaves = 8;  // waves of a workgroup of the kernel: they stride the switch frame c
constexpr int kDwellVisTile = 63;       // rows n that a workgroup owns: lane 0 carries the row below them for the jump mix

// the rows that end frame b computes and writes: n = 0 .. dwell_visits_cap(b, n_top), one more than A(b, ., .) can fill
constexpr int dwell_visits_cap(int b, int n_top) { return (b + 1) / 2 + 1 < n_top ? (b + 1) / 2 + 1 : n_top; }

struct DwellVisits {
    double *alpha;          // per trajectory [c][s][n], c < Tm, n < ldn: alpha(c, s, n), written for 1 <= c < T and n <= cap(c) alone
    double *last;           // per trajectory [n][s], n < ldn: A(T, s, n), written for n <= cap(T) alone
    int64_t stride;         // entries of alpha per trajectory: S * Tm * ldn
    int ldn;                // n_top + 1
    int n_top;              // the last row kept: min(n_max, (Tm + 1) / 2)
    unsigned target;        // bit s: state s belongs to G
};

// bytes of one trajectory in the call's own tables
constexpr int64_t dwell_visits_bytes(int S, int Tm, int n_top) { return ((int64_t)S * Tm * (n_top + 1) + (int64_t)S * (n_top + 1)) * 8; }

// end frame b = 1 .. Tm of the chunk's trajectories, in ascending order on one stream; a trajectory with T < b has no work.
// Needs the prior tables of p alone
int launch_dwell_visits(const DwellParams &p, const DwellVisits &o, int b, void *stream);

} // namespace bild
