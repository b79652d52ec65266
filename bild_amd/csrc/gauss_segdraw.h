// Exact posterior draws of profiles from the backward tables of the segment recursion (gauss_segdraw.cpp: host side and C
// ABI; gauss_segdraw.hip: kernels).  Private to the library.
//
// The tables beta_m and gamma_m are those of gauss_segdp.h, built by its kernels.  A draw of k switches walks its profile
// from the left: (s_0, t_1) against exp F[s][b] gamma_k(b, s), then per switch i the state s_i against beta_{k-i}(t_i, q) and
// the segment's end t_{i+1} against exp W[s_i][t_i - 1][b] gamma_{k-i}(b, s_i).  Every pick is an inverse-CDF pick of one
// uniform over a list in a fixed order; one wavefront owns one draw.
#pragma once
#include <stdint.h>

#include "gauss_segdp.h"

namespace bild {

constexpr int kSegdrawThreads = 256;    // four draws a workgroup

struct SegdrawParams {
    const GaussTraj *trajs;     // the chunk's trajectories (device)
    const uint8_t *tr;          // transitions, S x S
    SegdpBwd beta, gamma;       // the chunk's backward tables, levels 0 .. K - 1
    double *head;               // per (trajectory of the chunk, k): M and Z of the list of the first pick
    const int32_t *order;       // the chunk's draws: their index r in the call
    const int32_t *slot_of;     // ... and their trajectory's place in the chunk
    const int32_t *draw_k;      // per r
    const double *uniforms;     // per r a row of U; null: Philox stream r of `seed`
    int32_t *seg_start, *seg_state;     // per r a row of K
    double *logl;               // per r
    double *uniforms_out;       // per r a row of U (zeroed by the host), or null
    uint64_t seed;
    int64_t slot;               // K * S * ld: entries of one trajectory in every table
    int n_traj, n_draws, S, K, ld, U;
};

int launch_segdraw_head(const SegdrawParams &p, void *stream);
int launch_segdraw(const SegdrawParams &p, const SegdrawParams *d_p, void *stream);   // d_p: p in device memory

} // namespace bild
