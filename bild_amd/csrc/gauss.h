// What gauss.cpp, gauss_sim.cpp (host) and gauss.hip (kernels) share: the model handle, GenericGaussianModel's table
// layout, the kernels' parameter blocks and their launchers.  Private to the library.
#pragma once
#include <stdint.h>

#include <mutex>
#include <vector>

struct bild_gauss_model {
    int S = 0, d = 0, L = 0;            // L: the largest lag of the MSD tables
    std::vector<int32_t> order;         // S x d
    std::vector<double> mean, msd_inf;  // S x d
    std::vector<double> msd;            // S x d x (L + 1)
    // the generator's Toeplitz factors (gauss_sim.cpp): device memory from the first bild_gauss_simulate on, grown with
    // the longest trajectory; freed by bild_gauss_model_destroy.  A model that never simulates holds host memory only.
    mutable std::mutex sim_mu;
    mutable double *factors = nullptr;
    mutable int factor_T = 0;                   // frames the factors cover (0: none yet)
    mutable std::vector<int64_t> factor_off;    // S x d: offset of the factor of (state, dimension)
    mutable std::vector<int> factor_n;          // S x d: its order (= leading dimension): factor_T, or factor_T - 1 (ss_order 1)
    mutable std::vector<int> factor_ok;         // S x d: leading pivots that are finite and positive
};

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

// The generator (gauss_sim.cpp; kernels in gauss.hip).  Column: one (trajectory, interval, dimension) against the leading
// len x len block of its (state, dimension) factor: y_r = sum_{j <= r} L_rj zvec_j, zvec_j = z[z + j] for j >= skip0 and
// 0 below; y_r (r >= skip0) goes to out row `row + r`.
struct GaussSimCol {
    int64_t z;          // zvec_j = Z[z + j] (j >= skip0)
    int64_t row;        // output row (of d values) of entry 0: the frame frame0 of the trajectory
    int len, skip0;     // rows of the factor used; skip0 = 1: a later ss_order-0 interval (entry 0 is the conditioning slot)
    int frame0, traj;   // device mode: the normal of entry j is that of (trajectory traj of the call, frame frame0 + j)
    int k, pad;
};

// up to kGaussSimTN columns of one (state, dimension), longest first
struct GaussSimBlock {
    const double *L;    // the factor (column-major, leading dimension ld)
    int ld, k, c0, nc, nmax;
};

struct GaussSimTask {
    int block, r0;      // row tile [r0, r0 + kGaussSimTM)
};

constexpr int kGaussSimTM = 64, kGaussSimTN = 32;

struct GaussSimProduct {
    const GaussSimCol *cols;
    const GaussSimBlock *blocks;
    const GaussSimTask *tasks;
    double *z;          // the normals of the chunk (device mode: written by gauss_sim_normals_kernel)
    double *out;
    int ntasks, ncols, d;
    uint64_t seed;
};

// the sequential pass: one workgroup per (trajectory, group of kGaussSimDG dimensions)
constexpr int kGaussSimDG = 8;

struct GaussSimAssemble {
    const int64_t *frame_off;   // first output row of each trajectory
    const int64_t *iv_off;      // per trajectory: its first interval in iv (n + 1 entries)
    const int32_t *iv;          // intervals (t0, t1, state), runs of equal state
    const int32_t *order;       // S x d
    const double *mean;         // S x d
    const double *const *L;     // S x d: the factors (column 0 is the conditioning column)
    const uint8_t *missing;     // per output row
    double *out;
    int n, d;
};

// The sensitivities (gauss_sens.cpp; kernels in gauss_sens.hip).  One set per (trajectory,
// dimension, state) that a window uses, and one per (state, dimension, parameter) of a shared factor.
constexpr int kGaussSensMaxP = 4;
constexpr int kGaussSensStride = 16;    // doubles per job output: sum tau, sum dtau_p (4), Fisher upper triangle (10), pad

struct GaussSensSet {
    const int32_t *vidx;        // valid frames of the dimension, ascending
    const double *xv;           // their values
    const double *msd;          // the state's MSD at lags 0 .. Tmax
    const double *dmsd;         // its derivatives: P rows of dmsd_ld doubles
    int64_t dmsd_ld;
    double msd_inf, mean;
    double dmsd_inf[kGaussSensMaxP], dmean[kGaussSensMaxP];
    const double *fac;          // the shared factor of (state, dimension) (gap-free jobs; layout: gauss_sens_solve_kernel)
    int fac_ld, order;
};

struct GaussSensJob {
    int set;
    int rank;           // rank of the window's first valid frame among the dimension's valid frames
    int n;              // entries the job runs: up to the window's last counted entry
    int skip;           // first counted entry (1: a later ss_order-0 interval, whose entry 0 is the conditioning value)
    int centred;        // ss_order 0: the first value is centred as well (the first interval)
    int out;            // output row (kGaussSensStride doubles); -1: a shared factor (no data row, no output)
    int64_t fac;        // the job's factor at base + fac: (rows x n) elements of 1 + P doubles (L, dL_p), leading dimension rows
};

int launch_gauss_sens_factor(const GaussSensSet *sets, const GaussSensJob *jobs, int njobs, int P, double *base, double *out,
                             void *stream);
int launch_gauss_sens_solve(const GaussSensSet *sets, const GaussSensJob *jobs, int njobs, int P, int nmax, double *out,
                            void *stream);

int launch_gauss_factor_sets(const GaussJobSet *d_sets, const GaussJob *d_jobs, int nsets, void *stream);
int launch_gauss_sim_normals(const GaussSimProduct &p, void *stream);
int launch_gauss_sim_product(const GaussSimProduct &p, void *stream);
int launch_gauss_sim_assemble(const GaussSimAssemble &p, void *stream);

int launch_gauss_factor(const GaussJobSet &p, const GaussJob *d_jobs, int njobs, double *scratch, int64_t slot_doubles, void *stream);
int launch_gauss_solve(const GaussJobSet &p, const GaussJob *d_jobs, int njobs, int ld0, void *stream);
int launch_gauss_accumulate(const GaussAccum &p, void *stream);
int launch_gauss_walk(const GaussWalk &p, bool st, void *stream);

} // namespace bild
