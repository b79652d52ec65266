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

#include <vector>

#include "gauss.h"

struct bild_gauss_trajset;

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

// ---- the host side that the calls on the recursion share (gauss_dwell.cpp; evidence, sensitivities, lengths, filter, draws) ----
struct CallFrame;

// The per-trajectory tables of the recursion: the member of DwellParams (its element size is the table's), the set it
// belongs to and its entries per trajectory (S states, Tm frames, slot = S * (Tm + 1), ntile tiles).  What a trajectory
// costs (dwell_table_bytes) and what a call allocates (DwellCall::open) both come from this list and from nowhere else.
enum : unsigned {
    kDwellForward = 1u,     // what launch_dwell_forward writes
    kDwellBackward = 2u,    // beta and gamma
    kDwellJumps = 4u,       // launch_dwell_counts' jump half (stay_part null)
    kDwellCover = 8u,       // launch_dwell_cover and _carry, and the stay half of the counts
    kDwellStats = kDwellCover | kDwellJumps,
};
#define BILD_DWELL_TABLES(X)                            \
    X(A, kDwellForward, slot)                           \
    X(AV, kDwellForward, slot)                          \
    X(alpha, kDwellForward, slot)                       \
    X(alphaV, kDwellForward, slot)                      \
    X(Aarg, kDwellForward, slot)                        \
    X(alphaArg, kDwellForward, slot)                    \
    X(fin, kDwellForward, 2)                            \
    X(n_nan, kDwellForward, 1)                          \
    X(map_states, kDwellForward, Tm)                    \
    X(beta, kDwellBackward, slot)                       \
    X(gamma, kDwellBackward, slot)                      \
    X(jumps, kDwellJumps, (int64_t)S * S)               \
    X(cover, kDwellCover, slot)                         \
    X(post, kDwellCover, slot)                          \
    X(row_tot, kDwellCover, (int64_t)S * ntile * Tm)    \
    X(stay_part, kDwellCover, (int64_t)S * ntile)       \
    X(stay, kDwellCover, S)
constexpr int dwell_ntile(int Tm) { return (Tm + kDwellTile - 1) / kDwellTile; }

// bytes of one trajectory in the tables of `sets` (needs no device)
inline int64_t dwell_table_bytes(unsigned sets, int S, int Tm)
{
    const DwellParams p{};
    const int ntile = dwell_ntile(Tm);
    const int64_t slot = (int64_t)S * (Tm + 1);
    int64_t bytes = 0;
#define X(name, set, entries) \
    if (sets & (set)) bytes += (int64_t)(entries) * (int64_t)sizeof(*p.name);
    BILD_DWELL_TABLES(X)
#undef X
    return bytes;
}

// Section 21's NaN rule on what the forward pass leaves of a trajectory (fin: its pair; n_nan: its skipped NaN windows; omit:
// BILD_DWELL_NAN_OMIT): bad = the evidence is NaN, usable = it is a finite number, and every statistic with it.
struct DwellVerdict {
    bool bad, usable;
    double logev;
};
DwellVerdict dwell_nan_rule(const double *fin, long long n_nan, bool omit);

// One call on the recursion.  Declared BEFORE the call's CallFrame: asynchronous copies write its vectors, so they must
// outlive the frame's wait.  In this order:
//   check()      what a call refuses before it touches the device: out, flags, dwell_check_call.  Fills n_traj, T, S, L, omit
//                and Tm (the set's longest, at least 1).  Where n_traj is 0, a call returns BILD_OK behind it.
//   over()       (the draws) the chunks run over n of the set's trajectories, the longest of Tm frames
//   second()     (the first-contact times) a second prior block: another log_init and log_jump over the same log_dwell and
//                log_surv.  open() then uploads it too and gives it forward tables of its own in p2 (a trajectory costs the
//                forward tables twice), and run() ends with the forward pass on it.  The two arrays outlive open()
//   open()       the frame on the set's stream, the chunks (a trajectory costs the tables of `sets` and the call's own
//                `own_bytes`), the prior's upload, the tables and p
//   run()        per chunk: the forward pass (kDwellForward) and the backward pass (kDwellBackward) of nc trajectories
//   read_back()  fin and n_nan of the chunk, and the wait for the stream; verdict(i) is dwell_nan_rule on trajectory i
struct DwellCall {
    int n_traj = 0, n = 0, S = 0, L = 0, Tm = 1, chunk = 0;
    const int *T = nullptr;
    bool omit = false;
    DwellParams p{}, p2{};          // p2: p with the second block's log_init, log_jump and forward tables (second() only)
    std::vector<double> fin;
    std::vector<long long> n_nan;

    int check(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init, const double *log_jump,
              const double *log_dwell, const double *log_surv, int T_max, unsigned flags, int64_t scratch_bytes, const void *out);
    void over(int n_used, int Tm_used) { n = n_used, Tm = Tm_used; }
    void second(const double *log_init2, const double *log_jump2) { prior2[0] = log_init2, prior2[1] = log_jump2; }
    int open(CallFrame &call, const bild_gauss_model *m, const bild_gauss_trajset *ts, unsigned sets, int64_t own_bytes);
    int run(CallFrame &call, const GaussTraj *trajs, int nc);
    int read_back(CallFrame &call, int nc);
    DwellVerdict verdict(int i) const { return dwell_nan_rule(fin.data() + 2 * i, n_nan[i], omit); }

private:
    const double *prior[4] = {}, *prior2[2] = {};
    int64_t scratch_bytes = 0;
    unsigned sets = 0;
};

int launch_dwell_forward(const DwellParams &p, void *stream);
int launch_dwell_backward(const DwellParams &p, void *stream);
int launch_dwell_cover(const DwellParams &p, void *stream);
int launch_dwell_carry(const DwellParams &p, void *stream);
int launch_dwell_counts(const DwellParams &p, void *stream);

} // namespace bild
