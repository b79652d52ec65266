// Kalman filter and smoother of candidate profiles (bild_kalman_segments, bild_kalman_mixture: kalman.cpp; kernels:
// kalman.hip).  Private to the library.
#pragma once
#include <cstdint>

#include "common.h"

struct bild_model;
struct bild_trajset;

namespace bild {

constexpr int kKalMaxModes = 32;  // effective modes (BILD_Q_NEFF) of the modal chain one task carries, one lane per mode
constexpr int kKalMaxStates = 255;
constexpr int kKalOutputs = 8;    // terms, pred_mean, pred_var, filt_mean, filt_var, smooth_mean, smooth_var, innov
constexpr int kKalBlock = 64;     // mixture: candidates per reduction block (fixed: the result does not depend on chunking)

// lanes of one task: the smallest of 8, 16, 32 that holds the effective modes
inline int kalman_lanes(int n) { return n <= 8 ? 8 : n <= 16 ? 16 : 32; }
// doubles of one frame's record between the two passes:
//   [C- w (L) | S, observed, filtered y-variance, e (kDMax), filtered y-mean (kDMax), state]
inline int kalman_rec(int L) { return L + 4 + 2 * kDMax; }

struct KalParams {
    const TrajDesc *trajs;
    const int32_t *seg_start, *seg_state, *traj_id; // the chunk's candidates (traj_id may be null: trajectory 0)
    int32_t K1;
    int64_t n;         // candidates of the chunk
    int32_t dstar_max; // tasks = n * dstar_max; task (r, e) runs covariance chain e of candidate r
    int32_t S, d, Tout;
    // per state, zero-padded to L modes: lam, sig, wq (S x L), C0 (S x L x L), M0, G (S x L x d), Q (S x L x L)
    const double *lam, *sig, *wq, *C0, *M0, *G, *Q;
    double *rec;              // per-frame records of the forward pass
    const int64_t *rec_off;   // per task: its first record double
    double *out[kKalOutputs]; // (n, Tout, d) each, null: not wanted
};
int launch_kalman(const KalParams &p, int L, void *stream);
// the arguments and the envelope of a call (kalman.cpp), checked before any device work; also what
// bild_logl_sensitivities accepts (sens.cpp)
int kalman_check_args(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *seg_start,
                      const int32_t *seg_state, const int32_t *traj_id, int64_t scratch_bytes);

struct MixParams {
    const double *mean, *var; // the chunk's smoothed outputs, (n, Tout, d)
    const double *ref;        // reference tracks, (n_ref, Tout, d)
    const int32_t *ref_row;   // trajectory -> its row of `ref`
    const double *w;          // per candidate of the chunk: weight (relative to the trajectory's largest)
    const int32_t *blk_start; // nblk + 1 chunk-local candidate offsets of the chunk's blocks
    const int32_t *blk_traj;  // trajectory of each block
    const int32_t *blk_T;     // frames of that trajectory
    int32_t nblk, Tout, d;
    double *part;             // nblk x Tout x d x 3: sums of w (m - ref), w v, w (m - ref)^2 over the block
    const int32_t *run_b0;    // nrun + 1: the chunk's blocks in runs of one trajectory each
    int32_t nrun;
    double *acc;              // n_traj x Tout x d x 3, accumulated over the chunks in block order
};
int launch_kalman_mix(const MixParams &p, void *stream);

} // namespace bild
