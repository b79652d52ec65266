// The weighted tangent jobs of an evidence gradient ("the jobs"), shared by the calls that have a table
// of segment weights Omega in gauss_segsens.h's layout: bild_gauss_segment_sensitivities (gauss_segsens.cpp) and
// bild_gauss_dwell_sensitivities (gauss_dwellsens.cpp).  Host only; private to the library.
//
// A call declares one SegTangent BEFORE its CallFrame (asynchronous copies read its vectors, so they must outlive the frame's
// wait) and then, in this order:
//   stage()    host work only: the valid frames of every (trajectory, dimension) and the jobs of every trajectory, in the
//              order their sums are added: state, dimension, the first interval, starts ascending
//   upload()   the model and derivative tables, the data and the sets to the device; the shared Toeplitz tangent factor of
//              every (state, dimension), once per call; waits for the stream
//   reserve()  the job and output rows of the widest chunk
//   run()      per chunk of whole trajectories, behind the launch that fills Omega: the job upload, the gap-free starts to
//              segsens_solve_kernel<P>, the starts behind a missing frame to segsens_factor_kernel<P> in budgeted chunks,
//              longest first, and the host sums, a trajectory's jobs in the staged order.  Waits for the stream.
#pragma once
#include <vector>

#include "gauss_call.h"
#include "gauss_segsens.h"

namespace bild {

struct SegTangent {
    struct HostJob {
        SegsensJob job;
        int state;
        bool gap_free;
    };

    void stage(const bild_gauss_model *m, int n_traj, const int *T, const double *x, int P, const bild_gauss_derivs *dm);
    int upload(CallFrame &call);
    int reserve(CallFrame &call, int chunk);
    // skip[i] != 0: trajectory j0 + i launches no job and is NaN in every output.  omega: the chunk's table, om_slot doubles
    // a trajectory, S triangles of om_tri doubles and then S first-segment rows of ld doubles.  Outputs may be null.
    int run(CallFrame &call, int j0, int nc, const char *skip, const double *omega, int64_t om_slot, int64_t om_tri, int ld,
            double *exp_logl, double *grad, double *fisher);

private:
    size_t vbase(int j, int k) const { return (size_t)(toff[j] * d + (int64_t)k * T[j]); }

    const bild_gauss_model *m = nullptr;
    const bild_gauss_derivs *dm = nullptr;
    const int *T = nullptr;
    int n_traj = 0, S = 0, d = 0, L1 = 0, P = 0, nmax_shared = 0;
    std::vector<int64_t> toff, shared_off;
    std::vector<int32_t> vidx, nvalid, iota;
    std::vector<double> xv, dmsd, h_out;
    std::vector<std::vector<HostJob>> jobs_of;
    std::vector<int> shared_n;
    std::vector<GaussSensSet> sets;
    std::vector<GaussSensJob> shared_jobs;
    std::vector<SegsensJob> all, flat;
    std::vector<int> solve_ix, fact_ix;
    GaussSensSet *d_sets = nullptr;
    SegsensJob *d_jobs = nullptr;
    double *d_out = nullptr, *d_scratch = nullptr;
    int64_t scratch_cap = 0;
    size_t max_jobs = 0;
};

} // namespace bild
