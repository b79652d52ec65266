// Exact inference under a dwell-time (explicit-duration, semi-Markov) prior over GenericGaussianModel's tables
// (gauss_dwell.cpp: host side and C ABI; gauss_dwell.hip: kernels).  Private to the library.
//
// Every table is stored per trajectory as [state][frame], frame 0 .. Tm (ld = Tm + 1 entries, Tm the longest trajectory of
// the call), one slot of S * ld entries per trajectory of the chunk, and holds logs.  With omega_s(a, b) = log_dwell[s][b - a]
// for b < T and log_surv[s][T - a] for b = T:
//   A(b, s)      log sum over the partial profiles on [0, b) whose last segment is in state s and ends at b (b = T: whole
//                profiles, the last segment censored); AV the same in (max, +), Aarg the start c of that last segment
//   alpha(c, s)  log sum_s' exp(A(c, s') + log_jump[s'][s]); alphaV in (max, +), alphaArg the s' of the maximum (-1: no
//                partial profile of finite prior weight without a NaN window jumps into s at c)
//   beta(a, s)   log sum_{b > a} exp(omega_s(a, b) + W[s][a - 1][b] + gamma(b, s))
//   gamma(b, s)  log sum_s'' exp(log_jump[s][s''] + beta(b, s'')) for b < T, 0 for b = T
#pragma once
#include <stdint.h>

#include "gauss.h"

namespace bild {

constexpr int kDwellMaxS = 4;       // states: the sequential passes keep every state of a frame in registers
constexpr int kDwellWaves = 8;      // waves of a workgroup of the forward and backward passes: one trajectory each
constexpr int kDwellTile = 64;      // frames of one tile: a lane each
constexpr int kDwellThreads = 256;  // the statistics kernels: a wave per tile

struct DwellParams {
    const GaussTraj *trajs;         // the chunk's trajectories (device)
    const double *log_init;         // S
    const double *log_jump;         // S x S
    const double *log_dwell;        // S x L, length l at [l - 1]
    const double *log_surv;         // S x L
    double *A, *AV, *alpha, *alphaV;
    int32_t *Aarg, *alphaArg;
    double *beta, *gamma;           // null without marginals
    double *row_tot;                // per (s, tile, a): the sum of a row's segment weights that end inside the tile
    double *cover;                  // per (s, t): the weights of the segments that cover t and end inside t's tile
    double *post;                   // per (s, t): the weights of all segments that cover t
    double *stay_part;              // per (s, tile): sum of weight x (length - 1) over the segments that end inside the tile
    double *fin;                    // per trajectory: log evidence, log joint of the MAP profile (NaN: none)
    long long *n_nan;               // per trajectory: NaN windows skipped
    uint8_t *map_states;            // per trajectory Tm bytes
    double *jumps, *stay;           // per trajectory S x S and S
    int64_t slot;                   // S * ld
    int n_traj, S, L, Tm, ld, ntile;
};

// What every call on a dwell-time prior refuses about the prior and the set's lengths (gauss_dwell.cpp; host only): more than
// kDwellMaxS states, L < 1 or shorter than a trajectory, a NaN or +inf table entry, a finite diagonal of log_jump, log_init
// that is -inf everywhere, a negative scratch_bytes, T_max shorter than a trajectory.  A BILD_* code.
int dwell_check_call(int S, int L, const double *log_init, const double *log_jump, const double *log_dwell, const double *log_surv,
                     int n_traj, const int *T, int T_max, int64_t scratch_bytes);

// The four prior tables in one device block: packed, allocated through the frame and uploaded by a synchronous copy.  The
// device pointers in *prior.  A BILD_* code.
struct CallFrame;
struct DwellPrior {
    const double *log_init, *log_jump, *log_dwell, *log_surv;
};
int dwell_upload_prior(CallFrame &call, int S, int L, const double *log_init, const double *log_jump, const double *log_dwell,
                       const double *log_surv, DwellPrior *prior);

int launch_dwell_forward(const DwellParams &p, void *stream);
int launch_dwell_backward(const DwellParams &p, void *stream);
int launch_dwell_cover(const DwellParams &p, void *stream);
int launch_dwell_carry(const DwellParams &p, void *stream);
int launch_dwell_counts(const DwellParams &p, void *stream);

} // namespace bild
