// Exact posterior draws of profiles under a dwell-time prior, from the backward tables of the dwell-time recursion
// (gauss_dwelldraw.cpp: host side and C ABI; gauss_dwelldraw.hip: kernels).  Private to the library.
//
// beta and gamma are the tables of gauss_dwell.h, built by its backward kernel.  A draw walks its profile from the left:
// (s_0, t_1) against log_init[s] + omega_s(0, b) + F[s][b] + gamma(b, s), then per switch the state s_i against
// log_jump[s_{i-1}][q] + beta(t_i, q) and the segment's end t_{i+1} against omega_{s_i}(t_i, b) + W[s_i][t_i - 1][b] +
// gamma(b, s_i), until a pick returns b = T.  Every pick is an inverse-CDF pick of one uniform over a list in a fixed order;
// one wavefront owns one draw.
#pragma once
#include <stdint.h>

#include "gauss_dwell.h"

namespace bild {

constexpr int kDwelldrawThreads = 256;  // four draws a workgroup

struct DwelldrawParams {
    const GaussTraj *trajs;         // the chunk's trajectories (device)
    const double *log_init;         // S
    const double *log_jump;         // S x S
    const double *log_dwell;        // S x L, length l at [l - 1]
    const double *log_surv;         // S x L
    const double *beta, *gamma;     // the chunk's backward tables: [state][frame], a slot per trajectory
    double *head;                   // per trajectory of the chunk: scale M and total Z of the list of the first pick
    const int32_t *order;           // the chunk's draws: their index r in the call
    const int32_t *slot_of;         // ... and their trajectory's place in the chunk
    const int64_t *stream;          // per r: the index of its Philox stream; null: r
    const double *uniforms;         // per r a row of U; null: the Philox stream of `seed`
    uint8_t *states;                // per r a row of T_max bytes, or null
    int32_t *n_switches, *n_uniforms;   // per r
    double *logl, *log_prior;       // per r
    double *uniforms_out;           // per r a row of U (zeroed by the host), or null
    uint64_t seed;
    int64_t slot;                   // S * ld: entries of one trajectory in beta and in gamma
    int n_traj, n_draws, S, L, ld, U, T_max;
};

int launch_dwelldraw_head(const DwelldrawParams &p, void *stream);
int launch_dwelldraw(const DwelldrawParams &p, const DwelldrawParams *d_p, void *stream);     // d_p: p in device memory

} // namespace bild
