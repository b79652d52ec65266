// Per-frame moments and posterior tracks of GenericGaussianModel profiles (bild_gauss_kalman_segments,
// bild_gauss_kalman_mixture: gauss_kalman.cpp; kernels: gauss_kalman.hip).  Private to the library.
#pragma once
#include <stdint.h>

#include "gauss.h"
#include "kalman.h"

namespace bild {

// one (trajectory, dimension, state) that a window uses
struct GaussKalSet {
    const int32_t *vidx;    // valid frames of the dimension, ascending
    const int32_t *midx;    // missing frames of the dimension, ascending
    const int32_t *rank;    // T + 1: valid frames before frame t
    const double *xv;       // values at the valid frames
    const double *msd;      // the state's MSD at lags 0 .. Tmax
    double msd_inf, mean;
    const double *fac;      // the shared factor of (state, dimension) (gap-free jobs), column-major
    int fac_ld, order;
};

// one window as a job: entries j < n of the data vector (valid frames from rank `rank` on) and nmiss missing frames
// (the dimension's missing frames from index `miss` on)
struct GaussKalJob {
    int set;
    int rank;
    int n;
    int centred;        // ss_order 0: the first value is centred as well (the first interval)
    int miss, nmiss;
    int64_t fac;        // factor jobs: the scratch slot ((n + nmiss + 1) x n doubles, leading dimension n + nmiss + 1)
    int64_t rec;        // the job's record: (L_jj, z_j) per entry, then (mean, var) per missing frame
};

// one (candidate, interval, dimension): frames [t0, t1) from its window's job, then [t1, t2) NaN (behind the trajectory)
struct GaussKalRef {
    int64_t cand;       // candidate of the call
    int64_t rec;        // record of the job; -1: no job (no entry, no missing frame)
    int set, k;
    int t0, t1, t2;
    int rank, n, skip;  // as the job's; skip: first counted entry
    int miss;           // the job's first missing frame (index among the dimension's)
    int nan;            // a later ss_order-0 window without a valid frame: NaN everywhere
};

struct GaussKalScatter {
    const GaussKalSet *sets;
    const GaussKalRef *refs;
    const double *rec;
    double *out[kKalOutputs];   // chunk-local (n, Tout, d) each; filt_* unused, null: not wanted
    int64_t c0;                 // first candidate of the chunk
    int nrefs, Tout, d;
};

int launch_gauss_kal_factor(const GaussKalSet *sets, const GaussKalJob *jobs, int njobs, double *scratch, double *rec, void *stream);
int launch_gauss_kal_solve(const GaussKalSet *sets, const GaussKalJob *jobs, int njobs, int nmax, double *rec, void *stream);
int launch_gauss_kal_scatter(const GaussKalScatter &p, void *stream);

} // namespace bild
