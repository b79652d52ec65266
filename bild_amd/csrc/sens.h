// Forward sensitivities of the Kalman-filter log-likelihood (bild_logl_sensitivities: sens.cpp; kernel: sens.hip).
// Private to the library.
#pragma once
#include <cstdint>

#include "common.h"

namespace bild {

constexpr int kSensMaxP = 4;                                             // parameters (tangents) of one call
constexpr int kSensStride = 1 + kSensMaxP + kSensMaxP * (kSensMaxP + 1) / 2; // doubles of one task's sums
constexpr int kSensMaxP32 = 0; // at L = 32 lanes (17..32 effective modes) the kernel runs without tangents only: with
                               // one it spills

struct SensParams {
    const TrajDesc *trajs;
    const int32_t *seg_start, *seg_state, *traj_id; // the chunk's candidates (traj_id may be null: trajectory 0)
    int32_t K1;
    int64_t n;         // candidates of the chunk
    int32_t dstar_max; // tasks = n * dstar_max; task (r, e) runs covariance chain e of candidate r
    int32_t S, d;
    // per state, zero-padded to L modes: lam, sig, wq (S x L), C0 (S x L x L), M0, G (S x L x d), Q (S x L x L)
    const double *lam, *sig, *wq, *C0, *M0, *G, *Q;
    // per parameter p, the same in the modal basis of each state: dlam, dsig (P x S x L), dC0 (P x S x L x L),
    // dM0, dG (P x S x L x d)
    const double *dlam, *dsig, *dC0, *dM0, *dG;
    int32_t has_dG;
    const double *ds2; // per (trajectory, chain): kSensMaxP derivatives of the chain's variance s2
    double *out;       // per task: logL, P gradient entries, P (P + 1) / 2 Fisher entries (upper triangle, row-major);
                       // stride kSensStride
};
int launch_sens(const SensParams &p, int L, int P, void *stream);

} // namespace bild
