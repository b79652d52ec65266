// Exact evidence of every k by a segment recursion over GenericGaussianModel's tables (gauss_segdp.cpp: host side and C
// ABI; gauss_segdp.hip: kernels).  Private to the library.
//
// Every table of the recursion is stored per trajectory as [level][state][frame], frame 0 .. Tm (ld = Tm + 1 entries, Tm the
// longest trajectory of the call), one slot of K * S * ld entries per trajectory of the chunk.  A sum over partial profiles
// is kept as a pair (M, Z): M is the largest log-likelihood among them, from the (max, +) pass, and Z = sum exp(logL - M),
// so every exponent is non-positive and Z >= 1 where M is finite.  Empty or all-weight-0 sums have Z = 0.
//
// Forward, level j = switches so far:
//   A_j(b, s)      partial profiles on [0, b) with j switches whose last segment is in state s and ends at b
//   alpha_j(c, s)  the same up to frame c, with the j-th switch at c into state s: the sum of A_{j-1}(c, s') over the
//                  allowed s' (segdp_mix_kernel); A_j(b, s) = sum_c alpha_j(c, s) exp W[s][c - 1][b] (segdp_level_kernel)
// Backward, level m = switches still to come:
//   gamma_m(b, s)  completions of a profile whose segment in state s ends at b; gamma_0 = [b == T]
//   beta_m(a, s)   completions that start with a segment [a, .) in state s: sum_b exp W[s][a - 1][b] gamma_m(b, s)
//                  (segdp_blevel_kernel); gamma_{m+1}(b, s) = sum of beta_m(b, s'') over the allowed s'' (segdp_bmix_kernel)
#pragma once
#include <stdint.h>

#include <vector>

#include "gauss.h"

struct bild_gauss_trajset;

namespace bild {

constexpr int kSegdpMaxK = 64;      // k_max of one call
constexpr int kSegdpThreads = 256;
constexpr int kSegdpSlices = 16;    // splits of the switch range of one level: one wave each, 1024 lanes a workgroup
constexpr int kSegdpTile = 64;      // end frames of one workgroup of a level / frames of one wave of the marginals

// a forward table: (M, Z), R = the Z-weighted mean log-likelihood of the partial profiles, the number of partial profiles
// that use no NaN window (ok) and of those that do (bad), and the back-pointer of M
struct SegdpFwd {
    double *M, *Z, *R, *ok, *bad;
    int32_t *arg;       // A: the switch frame c of the maximum; alpha: the preceding state s'; -1: none
};

struct SegdpBwd {
    double *M, *Z;
};

struct SegdpParams {
    const GaussTraj *trajs;     // the chunk's trajectories (device)
    const uint8_t *tr;          // transitions, S x S
    SegdpFwd A, alpha;
    SegdpBwd beta, gamma;       // null without marginals
    double *row_tot;            // marginals: per (k, s, tile of frames, a) the sum of a row's terms inside the tile
    double *cover;              // marginals: per (k, s, t) the terms of segments that cover t and end inside t's tile
    double *post;               // marginals: per (k, s, t) all terms of segments that cover t (unnormalised, scaled by top_k)
    int32_t *map_seg_start, *map_seg_state;     // per trajectory K x K
    double *fin;                // per (trajectory, k, s): M, Z, R, ok, bad of A_k(T, s)
    int64_t slot;               // K * S * ld: entries of one trajectory in every table
    int n_traj, S, K, Tm, ld, ntile;
};

int launch_segdp_init(const SegdpParams &p, bool backward, void *stream);
int launch_segdp_mix(const SegdpParams &p, int j, void *stream);        // alpha_j from A_{j-1}
int launch_segdp_level(const SegdpParams &p, int j, void *stream);      // A_j from alpha_j
int launch_segdp_blevel(const SegdpParams &p, int m, void *stream);     // beta_m from gamma_m
int launch_segdp_bmix(const SegdpParams &p, int m, void *stream);       // gamma_m from beta_{m-1}
int launch_segdp_backtrack(const SegdpParams &p, void *stream);
int launch_segdp_cover(const SegdpParams &p, void *stream);
int launch_segdp_carry(const SegdpParams &p, void *stream);

// ---- the host side that the calls on the recursion share (gauss_segdp.cpp; evidence, draws, sensitivities) ----
struct CallFrame;

// transitions: not NULL, entries 0 or 1 (exact.cpp as well).  A BILD_* code.
int segdp_check_transitions(int S, const uint8_t *transitions);

// C(n, k) from exact integer steps (each division is exact), carried in a 64-bit mantissa once it no longer fits 128 bits
long double binom_ld(int n, int k);
// valid traces of k switches for every k < K: the sum of the entries of transitions^k
std::vector<long double> trace_counts(int S, const uint8_t *tr, int K);

// The per-trajectory tables of the recursion: the member of SegdpParams (its element size is the table's), the set it
// belongs to and its entries per trajectory (S states, K levels, Tm frames, slot = K * S * (Tm + 1), ntile tiles).  What a
// trajectory costs (segdp_table_bytes) and what a call allocates (SegdpCall::open) both come from this list and from nowhere else.
enum : unsigned {
    kSegdpForward = 1u,     // A and alpha, the MAP arrays and fin: what segdp_run_forward writes
    kSegdpBackward = 2u,    // beta and gamma
    kSegdpCover = 4u,       // launch_segdp_cover and _carry
};
#define BILD_SEGDP_FWD(X, t) /* a SegdpFwd */                                                                   \
    X(t.M, kSegdpForward, slot) X(t.Z, kSegdpForward, slot) X(t.R, kSegdpForward, slot) X(t.ok, kSegdpForward, slot) \
    X(t.bad, kSegdpForward, slot) X(t.arg, kSegdpForward, slot)
#define BILD_SEGDP_TABLES(X)                                                                \
    BILD_SEGDP_FWD(X, A)                                                                    \
    BILD_SEGDP_FWD(X, alpha)                                                                \
    X(map_seg_start, kSegdpForward, (int64_t)K * K)                                         \
    X(map_seg_state, kSegdpForward, (int64_t)K * K)                                         \
    X(fin, kSegdpForward, (int64_t)K * S * 5)                                               \
    X(beta.M, kSegdpBackward, slot) X(beta.Z, kSegdpBackward, slot)                         \
    X(gamma.M, kSegdpBackward, slot) X(gamma.Z, kSegdpBackward, slot)                       \
    X(cover, kSegdpCover, slot)                                                             \
    X(post, kSegdpCover, slot)                                                              \
    X(row_tot, kSegdpCover, (int64_t)K * S * ntile * Tm)

constexpr int segdp_ntile(int Tm) { return (Tm + kSegdpTile - 1) / kSegdpTile; }

// bytes of one trajectory in the tables of `sets` (needs no device)
inline int64_t segdp_table_bytes(unsigned sets, int S, int K, int Tm)
{
    const SegdpParams p{};
    const int ntile = segdp_ntile(Tm);
    const int64_t slot = (int64_t)K * S * (Tm + 1);
    int64_t bytes = 0;
#define X(member, set, entries) \
    if (sets & (set)) bytes += (int64_t)(entries) * (int64_t)sizeof(*p.member);
    BILD_SEGDP_TABLES(X)
#undef X
    return bytes;
}

// The profiles of one (trajectory, k) from the S x 5 block `fin` of the last column of the forward table; n_all = all
// profiles of that k, omit = BILD_SEGDP_NAN_OMIT.  logev = top + log(z) - log(count); z = 0 where logev is -inf or NaN.
struct SegdpEvidence {
    double logev, kl, count, bad, top, z, map_logl;     // map_logl: NaN where no profile has one
    bool any, usable;                                   // any profile at all; logev is a number
};
SegdpEvidence segdp_evidence(const double *fin, int S, long double n_all, bool omit);

// the launches of one chunk: init, then mix and level per j, then the back-pointer walk / init, then blevel and bmix per level
int segdp_run_forward(const SegdpParams &p, int k_max, void *stream);
int segdp_run_backward(const SegdpParams &p, int k_max, void *stream);

// One call on the recursion, shaped as DwellCall (gauss_dwell.h) and, like it, declared BEFORE the call's CallFrame.
//   check()      what a call refuses before it touches the device: out, segdp_check_call.  Fills n_traj, T, S, K, k_max, omit
//                and Tm (the set's longest, at least 1).  Where n_traj is 0, a call returns BILD_OK behind it.
//   over()       (the draws) the chunks run over n of the set's trajectories, the longest of Tm frames
//   open()       the frame on the set's stream, the chunks (a trajectory costs the tables of `sets` and the call's own
//                `own_bytes`), the transitions' upload, the tables, p and the trace counts
//   run()        per chunk: segdp_run_forward (kSegdpForward) and segdp_run_backward (kSegdpBackward) of nc trajectories
//   read_back()  fin of the chunk, and the wait for the stream
//   each_k()     f(k, the SegdpEvidence of k) for every k of trajectory i of the chunk, which has Tj frames
struct SegdpCall {
    int n_traj = 0, n = 0, S = 0, K = 0, k_max = 0, Tm = 1, chunk = 0;
    const int *T = nullptr;
    bool omit = false;
    SegdpParams p{};
    std::vector<double> fin;
    std::vector<long double> ntraces;

    int check(const bild_gauss_model *m, const bild_gauss_trajset *ts, int k_max, const uint8_t *transitions, int T_max, unsigned flags,
              int64_t scratch_bytes, const void *out);
    void over(int n_used, int Tm_used) { n = n_used, Tm = Tm_used; }
    int open(CallFrame &call, const bild_gauss_model *m, const bild_gauss_trajset *ts, unsigned sets, int64_t own_bytes);
    int run(CallFrame &call, const GaussTraj *trajs, int nc);
    int read_back(CallFrame &call, int nc);
    template <class F> void each_k(int i, int Tj, F f) const
    {
        for (int k = 0; k < K; ++k)
            f(k, segdp_evidence(fin.data() + ((size_t)i * K + k) * S * 5, S, binom_ld(Tj - 1, k) * ntraces[k], omit));
    }

private:
    const uint8_t *transitions = nullptr;
    int64_t scratch_bytes = 0;
    unsigned sets = 0;
};

} // namespace bild
