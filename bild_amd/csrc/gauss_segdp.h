// Exact evidence of every k by a segment recursion over GenericGaussianModel's tables (gauss_segdp.cpp: host side and C
// ABI; gauss_segdp.hip: kernels).  Private to the library.
//
// Every table of the recursion is stored per trajectory as [level][state][frame], frame 0 .. Tm (ld = Tm + 1 entries, Tm the
// longest trajectory of the call), one slot of K * S * ld entries per trajectory of the chunk.  A sum over partial profiles
// is kept as a pair (M, Z): M is the largest log-likelihood among them, from the (max, +) pass, and Z = sum exp(logL - M),
// so every exponent is non-positive and Z >= 1 where M is finite.  Empty or all-weight-0 sums have Z = 0.
//
// Forward, level j = switches so far:
//   A_j(b, s)      partial profiles on [0, b) with j switches whose last segment is in state s and ends at b
//   alpha_j(c, s)  the same up to frame c, with the j-th switch at c into state s: the sum of A_{j-1}(c, s') over the
//                  allowed s' (segdp_mix_kernel); A_j(b, s) = sum_c alpha_j(c, s) exp W[s][c - 1][b] (segdp_level_kernel)
// Backward, level m = switches still to come:
//   gamma_m(b, s)  completions of a profile whose segment in state s ends at b; gamma_0 = [b == T]
//   beta_m(a, s)   completions that start with a segment [a, .) in state s: sum_b exp W[s][a - 1][b] gamma_m(b, s)
//                  (segdp_blevel_kernel); gamma_{m+1}(b, s) = sum of beta_m(b, s'') over the allowed s'' (segdp_bmix_kernel)
#pragma once
#include <stdint.h>

#include <vector>

#include "gauss.h"

namespace bild {

constexpr int kSegdpMaxK = 64;      // k_max of one call
constexpr int kSegdpThreads = 256;
constexpr int kSegdpSlices = 16;    // splits of the switch range of one level: one wave each, 1024 lanes a workgroup
constexpr int kSegdpTile = 64;      // end frames of one workgroup of a level / frames of one wave of the marginals

// a forward table: (M, Z), R = the Z-weighted mean log-likelihood of the partial profiles, the number of partial profiles
// that use no NaN window (ok) and of those that do (bad), and the back-pointer of M
struct SegdpFwd {
    double *M, *Z, *R, *ok, *bad;
    int32_t *arg;       // A: the switch frame c of the maximum; alpha: the preceding state s'; -1: none
};

struct SegdpBwd {
    double *M, *Z;
};

struct SegdpParams {
    const GaussTraj *trajs;     // the chunk's trajectories (device)
    const uint8_t *tr;          // transitions, S x S
    SegdpFwd A, alpha;
    SegdpBwd beta, gamma;       // null without marginals
    double *row_tot;            // marginals: per (k, s, tile of frames, a) the sum of a row's terms inside the tile
    double *cover;              // marginals: per (k, s, t) the terms of segments that cover t and end inside t's tile
    double *post;               // marginals: per (k, s, t) all terms of segments that cover t (unnormalised, scaled by top_k)
    int32_t *map_seg_start, *map_seg_state;     // per trajectory K x K
    double *fin;                // per (trajectory, k, s): M, Z, R, ok, bad of A_k(T, s)
    int64_t slot;               // K * S * ld: entries of one trajectory in every table
    int n_traj, S, K, Tm, ld, ntile;
};

int launch_segdp_init(const SegdpParams &p, bool backward, void *stream);
int launch_segdp_mix(const SegdpParams &p, int j, void *stream);        // alpha_j from A_{j-1}
int launch_segdp_level(const SegdpParams &p, int j, void *stream);      // A_j from alpha_j
int launch_segdp_blevel(const SegdpParams &p, int m, void *stream);     // beta_m from gamma_m
int launch_segdp_bmix(const SegdpParams &p, int m, void *stream);       // gamma_m from beta_{m-1}
int launch_segdp_backtrack(const SegdpParams &p, void *stream);
int launch_segdp_cover(const SegdpParams &p, void *stream);
int launch_segdp_carry(const SegdpParams &p, void *stream);

// ---- the host side that the calls on the recursion share (gauss_segdp.cpp; evidence, draws, sensitivities) ----
struct CallFrame;

// transitions: not NULL, entries 0 or 1 (exact.cpp as well).  A BILD_* code.
int segdp_check_transitions(int S, const uint8_t *transitions);
// What every call on the recursion refuses, in this order: k_max outside 0 .. kSegdpMaxK, flags other than BILD_SEGDP_NAN_OMIT,
// the transitions, a negative scratch_bytes, T_max shorter than a trajectory.  A BILD_* code.
int segdp_check_call(int S, int k_max, unsigned flags, const uint8_t *transitions, int64_t scratch_bytes, int n_traj, const int *T,
                     int T_max);

// C(n, k) from exact integer steps (each division is exact), carried in a 64-bit mantissa once it no longer fits 128 bits
long double binom_ld(int n, int k);
// valid traces of k switches for every k < K: the sum of the entries of transitions^k
std::vector<long double> trace_counts(int S, const uint8_t *tr, int K);
int alloc_fwd(CallFrame &call, SegdpFwd *t, size_t n);

// The profiles of one (trajectory, k) from the S x 5 block `fin` of the last column of the forward table; n_all = all
// profiles of that k, omit = BILD_SEGDP_NAN_OMIT.  logev = top + log(z) - log(count); z = 0 where logev is -inf or NaN.
struct SegdpEvidence {
    double logev, kl, count, bad, top, z, map_logl;     // map_logl: NaN where no profile has one
    bool any, usable;                                   // any profile at all; logev is a number
};
SegdpEvidence segdp_evidence(const double *fin, int S, long double n_all, bool omit);

// the launches of one chunk: init, then mix and level per j, then the back-pointer walk / init, then blevel and bmix per level
int segdp_run_forward(const SegdpParams &p, int k_max, void *stream);
int segdp_run_backward(const SegdpParams &p, int k_max, void *stream);

} // namespace bild
