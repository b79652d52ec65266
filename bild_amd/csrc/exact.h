// Exact evidence by enumeration (exact.cpp: host side and C ABI; exact.hip: kernels).  Private to
// the library.
//
// The profiles of one trajectory are numbered trace-major: local index L = trace * C(T - 1, k) + combination rank, traces
// in CFC.full_sample order, combinations in itertools.combinations order.  They are reduced in blocks of kExactBlock
// consecutive local indices (a block never spans two trajectories; block q of a trajectory starts at q * kExactBlock), and
// a chunk of the call is a run of whole blocks.  The per-trajectory results are a left fold over that trajectory's blocks
// in index order, so they depend neither on the chunking nor on the other trajectories of the set.
#pragma once
#include <stdint.h>

namespace bild {

constexpr int kExactMaxK = 15;          // K1 <= 16
constexpr int kExactBlock = 4096;       // profiles per reduction block (one workgroup)
constexpr int kExactThreads = 256;
constexpr int kExactMargMax = 8192;     // S x T doubles of one block's marginal accumulators in LDS (64 KiB)

struct ExactBlock {
    int64_t local0;     // first profile of the block (local index in its trajectory)
    int64_t row0;       // its row in the chunk
    int32_t traj, n;    // trajectory, profiles in the block (<= kExactBlock)
};

// enumeration: one lane per profile of the chunk
struct ExactEnum {
    const ExactBlock *blocks;
    const uint64_t *binom;  // C(a, m) at a * (k + 1) + m, 0 <= a < A, 0 <= m <= k, saturated at 2^64 - 1
    const int32_t *traces;  // n_traces x (k + 1), full_sample order
    const int64_t *ncomb;   // per trajectory: C(T - 1, k)
    const int32_t *T;       // per trajectory
    int32_t *seg_start, *seg_state, *traj_id;   // chunk rows: n x (k + 1), n
    int nblocks, k, A;
};

// what one block leaves for the fold
struct ExactPart {
    double m;           // largest non-NaN logL of the block (-inf: none finite)
    double s, sl;       // sum exp(l - m), sum l exp(l - m) (terms of weight 0 skipped)
    double map_l;       // logL of the block's MAP profile
    int64_t map_idx;    // its local index (-1: every logL of the block is NaN)
    int64_t n_nan;
};

struct ExactReduce {
    const ExactBlock *blocks;
    const double *logl;                     // chunk rows
    const int32_t *seg_start, *seg_state;   // chunk rows, n x K1
    const int32_t *T;                       // per trajectory
    ExactPart *part;                        // per block
    double *marg;                           // per block S x Tm (null: no marginals)
    int nblocks, K1, S, Tm;
};

// per-trajectory accumulator across chunks
struct ExactAcc {
    double M, s, sl, map_l;
    int64_t map_idx, n_nan;
};

// one run of consecutive blocks of one trajectory in the chunk
struct ExactRun {
    int32_t traj, b0, nb, pad;
};

struct ExactFold {
    const ExactRun *runs;
    const ExactPart *part;
    const double *marg;     // per block S x Tm, or null
    const int32_t *T;
    ExactAcc *acc;          // per trajectory
    double *acc_marg;       // per trajectory S x Tm, or null
    int nruns, S, Tm;
};

int launch_exact_enumerate(const ExactEnum &p, void *stream);
int launch_exact_reduce(const ExactReduce &p, void *stream);
int launch_exact_fold(const ExactFold &p, void *stream);
// dynamic LDS of the reduction kernel
size_t exact_reduce_lds(int K1, int S, int Tmax, bool marginals);

} // namespace bild
