// What gauss.cpp (host) and gauss.hip (kernels) share: GenericGaussianModel's table layout, the kernels' parameter
// blocks and their launchers.  Private to the library.
#pragma once
#include <stdint.h>

namespace bild {

constexpr int kGaussMaxT = 2048;        // longest trajectory a set accepts (the solve kernel keeps one vector in LDS)

// Table W of a (trajectory, state): entry (a, b), 0 <= a < b <= T, at gauss_wrow(T, a) + (b - a - 1); T (T + 1) / 2 doubles
// (constexpr: host and device code both use it)
constexpr int64_t gauss_wrow(int T, int a) { return (int64_t)a * T - (int64_t)a * (a - 1) / 2; }
constexpr int64_t gauss_w_per_state(int T) { return (int64_t)T * (T + 1) / 2; }

// one window start of one (state, dimension)
struct GaussJob {
    int rank;       // index of the start's first valid frame among the dimension's valid frames
    int n;          // length of its vector: valid frames from there on (ss_order 0) or their increments (ss_order 1)
    int tau_row;    // row of tau to write; -1: the shared factor (no data row, written to GaussJobSet::factor)
    int centred;    // ss_order 0: the first value is centred as well (the first interval)
    int factor_out; // write the factor to GaussJobSet::factor instead of the job's scratch slot
};

// the (trajectory, dimension, state) a batch of jobs belongs to
struct GaussJobSet {
    const int32_t *vidx;    // valid frames of the dimension, ascending (V)
    const double *xv;       // their values (V)
    const double *msd;      // the state's MSD at integer lags 0 .. T-1
    double msd_inf, mean;
    int order;
    double *tau;            // rows of tau_ld doubles: (state, rank) -> row state * (V + 1) + rank; row V: the first interval
    int64_t tau_ld;
    double *factor;         // the shared factor (column-major, leading dimension = its order)
};

struct GaussAccum {
    const int32_t *vidx;
    const int32_t *rank_of; // T: number of valid frames before frame a
    const double *tau;
    int64_t tau_ld;
    const int32_t *order;   // per state, this dimension
    double *W, *F;          // the trajectory's tables: S x w_per_state, S x (T + 1)
    int64_t w_per_state;
    int S, T, V, dim;
};

struct GaussTraj {
    const double *W, *F;
    int64_t w_per_state;
    int T;
};

struct GaussWalk {
    const GaussTraj *trajs;
    const int32_t *seg_start, *seg_state;   // segment rows, or
    const double *ss;                       // (s, theta) rows
    const int64_t *thetas;
    const int32_t *traj_id;                 // may be null
    int32_t *status;                        // {refused?, a refused row}
    double *out;
    int64_t n;
    int K1, S;
};

int launch_gauss_factor(const GaussJobSet &p, const GaussJob *d_jobs, int njobs, double *scratch, int64_t slot_doubles, void *stream);
int launch_gauss_solve(const GaussJobSet &p, const GaussJob *d_jobs, int njobs, int ld0, void *stream);
int launch_gauss_accumulate(const GaussAccum &p, void *stream);
int launch_gauss_walk(const GaussWalk &p, bool st, void *stream);

} // namespace bild
