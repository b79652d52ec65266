/*
 * bild_amd -- C ABI of the MI355X (gfx950) Rouse Kalman-filter log-likelihood.
 *
 * This is the drop-in boundary for the one hot path of BILD
 * (OpenTrajectoryAnalysis/bild): everything the reference does per candidate looping
 * profile inside
 *
 *     bild/src/MSRouse_logL.pyx:95-256   MSRouse_logL(model, profile, traj)        (native)
 *     bild/src/MSRouse_logL_py.py:54-121 MSRouse_logL(model, profile, traj)        (fallback)
 *
 * batched over the samples of one AMIS step, i.e. the loop of
 *
 *     bild/amis.py:717-739               FixedkSampler.logL(ss, thetas) -> (N,) float64
 *
 * Plain C: opaque handles, raw pointers and sizes.  No torch / numpy / HIP types appear
 * in any signature (a HIP stream is passed as void*).  All matrices are row-major
 * float64.  Every function returns a bild_status; bild_last_error() gives the message of
 * the calling thread's most recent failure.  There is NO CPU fallback: evaluation
 * functions fail with BILD_ERR_NO_DEVICE when no gfx950 device is usable.
 *
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md.
 */
#ifndef BILD_AMD_H
#define BILD_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: round 4 -- bild_config_string / bild_config_reload, the inference driver (bild_run_*), the direct exchange
 *    (bild_exchange_*); negative cumulative positions of an (s, theta) row are refused on every path.
 * 1: rounds 1-3 (the version constant was not bumped while entry points were added). */
#define BILD_AMD_ABI_VERSION 2

typedef enum bild_status {
    BILD_OK              = 0,
    BILD_ERR_INVALID     = 1, /* bad argument: NULL, shape, range, non-finite model       */
    BILD_ERR_HIP         = 2, /* HIP runtime call failed                                  */
    BILD_ERR_NO_DEVICE   = 3, /* no usable GPU                                            */
    BILD_ERR_UNSUPPORTED = 4, /* model outside the compiled kernel envelope (N, d, S)     */
    BILD_ERR_NOMEM       = 5
} bild_status;

/* evaluation path, low 4 bits of `flags` of the bild_logl_* calls */
#define BILD_PATH_AUTO  0u /* modal when the model admits it (symmetric B), else dense    */
#define BILD_PATH_DENSE 1u /* canonical recursion  C <- B C B + Sig  every frame
                              (pyx:220-241)                                               */
#define BILD_PATH_MODAL 2u /* same recursion carried in each state's eigenbasis of B      */

/* bild_logl_segments_device only: check the device-resident descriptors with a small kernel first (traj_id range,
 * first start 0, non-decreasing starts, states < S) and refuse the batch with BILD_ERR_INVALID instead of letting a bad
 * index drive an out-of-range access.  The verdict has to be read back, so with this flag the call WAITS for the stream
 * once before launching.  Without it the device entry trusts its input (the host-buffer entries always validate). */
#define BILD_VALIDATE_DEVICE 0x10u

/* Do not start candidates from the prefix table (see "prefix table" below): every task runs from frame 0.  Results are
 * bit-identical either way; the flag exists for A/B measurements and tests.  (Environment BILD_NO_PREFIX=1: never build one.) */
#define BILD_NO_PREFIX 0x20u

/* With a prefix table: do not take the table's sums where a candidate's filter has converged onto the switch-free one
 * (see "prefix table" below); every frame behind the first switch is run.  Bit-identical to BILD_NO_PREFIX.
 * (Environment BILD_NO_JUMP=1: the same for every call.) */
#define BILD_NO_JUMP 0x40u

/* Split launches.  With all tables of a trajectory set in place a batch is launched as two kernels: a table walk with
 * one LANE per task (csrc/walk.hip), which finishes every task that needs no Kalman frame -- 96 % of the headline batch --
 * and appends the others to work lists ordered by expected work, and the frame loop (csrc/kernels.hip) over the listed
 * tasks only.  The walk adds the same numbers in the same order as the frame-loop kernel would: results are bit-identical
 * to the single launch, which this flag (or BILD_NO_SPLIT=1 in the environment) restores for A/B measurements and tests.
 * Lists of up to 16 segments per candidate are split; longer ones always take the single launch. */
#define BILD_NO_SPLIT 0x80u

/* Do not start chains of close switches from the transient state table (see "prefix table" below: the state a transient
 * has reached when the next switch comes is a record of that table): every chain runs from its first switch.  Results are
 * bit-identical either way.  (Environment BILD_NO_STATES=1: never build the table.  The table holds a record for every gap
 * a chain can start with -- up to the set's longest converged transient, measured when the transient table is built -- and
 * costs ~100 MB per 1000 frames of a 2-state trajectory: it is built for sets that need at most 4 GB of it, 64 GB for sets
 * declared for >= 1e8 evaluations with bild_trajset_expect, BILD_STATES_MAX_BYTES=<n> otherwise; at most a third of the free
 * memory in any case.  The same budget, after the first level's share, holds the PAIR state table -- the states the builders
 * of the pair table leave behind their second switch, from which a chain of three and more close switches starts at its third
 * switch: ~2 GB per 1000 frames of a 2-state trajectory, built whole or not at all; BILD_NO_PAIR_STATES=1,
 * BILD_PAIR_STATES_STRIDE=<n>.  The flag and BILD_NO_STATES switch both levels off.) */
#define BILD_NO_STATES 0x100u

/* Do not leave a transient on the first-order tail (csrc/tail.hip: once the covariance of a candidate's filter has converged
 * onto the switch-free filter's, the effect of the remaining deviation of the means on all later frames is a dot product with
 * a vector kept beside the prefix table): every transient runs until its means have converged too, as until round 3.  The
 * results differ by ~1e-12 (second-order terms of a deviation below 2^-20).  (Environment BILD_NO_TAIL=1: never build the vectors.) */
#define BILD_NO_TAIL 0x200u

/* Do not end a chain of close switches on a first-order tail THROUGH its next switch (csrc/tail.hip, "switch tails": behind the
 * third switch of a chain, a look that finds the covariance converged but the next switch too close for the ordinary tail takes
 * the dot product with a vector whose adjoint runs through that switch and the transient behind it, kept in a table of
 * T x S (S - 1) x d* x J x 240 bytes -- ~36 MB per 1000 frames of a 2-state trajectory, from the byte budget of the state tables
 * after both of their levels, built whole or not at all).  With the flag, results are those of a set without the table, bit for
 * bit; without it they differ by ~1e-11, the class of BILD_NO_TAIL.  (Environment BILD_NO_SWITCH_TAIL=1: never build the table.
 * BILD_NO_TAIL, flag or environment, switches both kinds of tail off.) */
#define BILD_NO_SWITCH_TAIL 0x400u

/* bild_model_create flags */
#define BILD_MODEL_NO_REDUCE 1u /* keep all N modes: skip the invariant-subspace reduction */

typedef struct bild_model   bild_model;
typedef struct bild_trajset bild_trajset;

int         bild_abi_version(void);
const char *bild_last_error(void);
void        bild_set_last_error(const char *msg); /* for the library's own translation units */

/* The experiment switches of the library are environment variables (BILD_NO_SPLIT, BILD_NO_STATES, BILD_PAIRS_MAX_TASKS ...:
 * csrc/config.h lists them all).  They are read ONCE, at the first use of the library in a process.
 * bild_config_string(): the switches that are set, as "NAME=value NAME=value" ("" when the defaults are in force) -- what
 * a bug report should carry.  bild_config_reload(): read the environment again (tests and tools that flip a switch inside
 * one process; must not run concurrently with evaluations; tables a trajectory set has built already stay as they are). */
const char *bild_config_string(void);
int         bild_config_reload(void);

/* Number of visible GPUs (0 without a device; never fails on a CPU-only host). */
int bild_device_count(int *count);

/* ------------------------------------------------------------------ model ----------
 * Replaces the per-call model setup of the reference kernel
 * (bild/src/MSRouse_logL.pyx:150-166): measurement vector w, and for each of the S
 * states the propagator (B, G, Sig) and steady state (M0, C0) that the reference pulls
 * out of rouse.Model (._dynamics['B'|'G'|'Sig'], .steady_state()).
 *
 *   N  monomers, d spatial dimensions (1..8), S states
 *   B, Sig, C0 : S x N x N     G, M0 : S x N x d     w : N
 *
 * Envelope: d <= 8 (a task carries up to three mean vectors; more dimensions with one localization error repeat
 * the covariance recursion: d = 4..6 costs two tasks per sample, d = 7..8 three), S <= 255, and at most 128 modes left by the (exact) invariant-subspace
 * reduction -- N <= 256 monomers for the default end-to-end measurement, N <= 128 for an
 * arbitrary w; above 32 modes only the modal path exists.  Outside: BILD_ERR_UNSUPPORTED.
 *
 * Host analysis only (eigenbases for the modal path, packing); no GPU is needed to
 * create a model.  Device copies are made lazily on the device that is current when an
 * evaluation first uses the model.  The caller keeps ownership of all inputs.
 */
int bild_model_create(int N, int d, int S,
                      const double *B, const double *G, const double *Sig,
                      const double *M0, const double *C0, const double *w,
                      unsigned flags, bild_model **out);
int bild_model_destroy(bild_model *m);

/* integer properties of a model */
#define BILD_Q_N            0
#define BILD_Q_D            1
#define BILD_Q_S            2
#define BILD_Q_MODAL_OK     3 /* 1 if the modal path is available                         */
#define BILD_Q_NP           4 /* padded row count the kernels run with                    */
#define BILD_Q_NEFF         5 /* modes kept after invariant-subspace reduction            */
#define BILD_Q_HAS_G        6 /* 1 if any G entry is non-zero                             */
#define BILD_Q_LAST_GEOMETRY 7 /* id of the vector-kernel geometry (BILD_GEOMETRIES) whose
                                  frame loop ran the last evaluating launch on this model;
                                  -1: another kernel family, a split launch whose table
                                  walk finished the batch (no frame loop), or none yet      */
int bild_model_query(const bild_model *m, int what, int64_t *value);

/* Host-analysis export (for tests that run without a GPU).  `what`:
 *   BILD_X_LAMBDA : n       eigenvalues of B[s] in the modal basis
 *   BILD_X_SIGMA  : n       diagonal of Q^T Sig[s] Q
 *   BILD_X_Q      : Nr x n  modal basis of state s (columns), in reduced coordinates
 *   BILD_X_WQ     : n       Q^T w
 *   BILD_X_R      : n x n   basis change  Q[s2]^T Q[s]   (state s -> s2)
 *   BILD_X_C0Q    : n x n   Q^T C0[s] Q
 *   BILD_X_V      : N x Nr  reduction basis (identity when no reduction applied)
 * n = Nr = BILD_Q_NEFF.  `buf` must hold the stated number of doubles. */
#define BILD_X_LAMBDA 0
#define BILD_X_SIGMA  1
#define BILD_X_Q      2
#define BILD_X_WQ     3
#define BILD_X_R      4
#define BILD_X_C0Q    5
#define BILD_X_V      6
int bild_model_export(const bild_model *m, int what, int s, int s2, double *buf, int64_t buf_len);

/* ------------------------------------------------------------- trajectories --------
 * Replaces the per-call trajectory setup (pyx:144-147, 174-178): the (T, d) data with
 * NaN marking missing frames (a frame is missing iff any coordinate is NaN), and the
 * per-dimension localization error from which the reference derives
 * s2 = unique(err)^2 and Cind (np.unique, sorted).
 *
 *   n_traj trajectories, lengths T[j] >= 1
 *   x        : sum(T) x d, trajectories concatenated in order
 *   loc_err  : n_traj x d, standard deviations (> 0 is not required, >= 0 is)
 *
 * Needs a GPU: the data are uploaded once and stay resident for all AMIS steps.
 */
int bild_trajset_create(const bild_model *m, int n_traj, const int32_t *T,
                        const double *x, const double *loc_err, bild_trajset **out);
/* (The device memory of a set's tables -- blocks of 128 KiB and more -- is not returned to the driver but kept, in size classes, for the
 * tables of the next set: up to BILD_TABLE_CACHE_BYTES, default 4 GB per process; 0 turns that off.  No evaluation on the set may be in
 * flight when it is destroyed.) */
int bild_trajset_destroy(bild_trajset *ts);
/* Optional, before the first evaluation on the set: how many evaluations the caller expects to run on it in total.  The
 * tables of a set (see "prefix table" below) are built at its first evaluation and cost about 1.5 ms per trajectory of
 * 1000 frames; they pay from a few hundred evaluations on (prefix + transient tables: >= 300) resp. a few thousand (pair
 * and state tables: >= 3000).  Without a declaration everything is built -- right for an AMIS run, wasteful for a
 * handful of single evaluations per trajectory.  Which tables exist depends on the set and on this declaration alone,
 * never on the call history: results stay reproducible (and agree between declarations to rounding, like between sets). */
int bild_trajset_expect(bild_trajset *ts, int64_t evaluations);

/* ---------------------------------------------------------------- evaluation -------
 * One call = one AMIS batch (bild/amis.py:717-739): n independent evaluations
 * logL(profile_r, traj[traj_id[r]]) -> out[r].
 *
 * Profiles come run-length encoded, K1 segments per sample:
 *   segment i of sample r is in state seg_state[r*K1+i] and starts at frame
 *   seg_start[r*K1+i]; seg_start[r*K1+0] must be 0, later starts >= 1 and non-decreasing (segment 0 owns
 *   frame 0: it selects the steady state the filter starts from and is never empty).
 *   Empty later segments (equal starts, or a start >= T) are legal and skipped -- this is what
 *   FixedkSampler.st2profile (bild/amis.py:685-693) produces for
 *   seg_start[1:] = floor(cumsum(s)[:-1]*(T-1)) + 1, seg_state = theta.
 *   state[0] selects the steady state the filter starts from, state[t] the propagator
 *   into frame t (bild/util.py:15-23).
 *   traj_id may be NULL (all samples refer to trajectory 0).
 *
 * All-missing trajectory -> 0.0 (semantics of MSRouse_logL_py.py:90-94).  NaN/Inf in a
 * result is passed through, never trapped.
 *
 * REPRODUCIBILITY CONTRACT (differs from the reference, whose MSRouse_logL is a pure function of its three arguments):
 *   - on ONE trajectory set a result is a pure function of (candidate, trajectory): bit-identical whatever the batch it
 *     is part of, the order of the batch, the entry point (host buffers, device buffers, (s, theta) rows or segment
 *     lists), the stream, the launch geometry, what was evaluated before, and with or without the split launch / the
 *     transient state table (BILD_NO_SPLIT, BILD_NO_STATES);
 *   - the same (candidate, trajectory) pair on two DIFFERENT trajectory sets (the trajectory alone / among hundreds of
 *     others) may take its sums from different tables -- which of them are built depends on the size of the set -- and
 *     agrees to rounding, |delta| ~ 1e-11 at |logL| ~ 3e4, not to the bit;
 *   - BILD_NO_JUMP (or BILD_NO_PREFIX) gives the frame-by-frame result, which IS a pure function of its inputs on any
 *     set; the default differs from it by ~1e-11 (bound and measurements: DESIGN.md section 2, tests/test_gpu_adversarial.py).
 * Against the reference's Cython kernel every path agrees to |delta| < 1e-8 (observed 1e-10; the reference's two own
 * kernels differ by 2.6e-10 among themselves).
 */

/* host buffers in, host buffer out; synchronous */
int bild_logl_segments(const bild_model *m, const bild_trajset *ts, int64_t n, int K1,
                       const int32_t *seg_start, const int32_t *seg_state,
                       const int32_t *traj_id, unsigned flags, double *out);

/* The sampler's own parametrisation, i.e. the arguments of FixedkSampler.logL(ss, thetas) (bild/amis.py:717-739)
 * as they are: ss (n x K1 float64, rows on the simplex), thetas (n x K1 int64).  The switch frames are computed here
 * exactly as FixedkSampler.st2profile does (bild/amis.py:685-688: sequential cumsum, times (T-1), floor, +1; T is the
 * length of the sample's trajectory), written straight into pinned staging memory and shipped with one copy.
 * A row is refused (BILD_ERR_INVALID) when one of its cumulative positions cumsum(s)[i] * (T-1) is negative, non-finite,
 * >= 2^31 or smaller than the one before it -- i.e. whenever it is not a point on the simplex in a way that would change
 * the profile (the reference does not check: np.floor of a negative position gives switch index 0 and a profile whose
 * first interval is empty).  Host buffers, synchronous. */
int bild_logl_st(const bild_model *m, const bild_trajset *ts, int64_t n, int K1,
                 const double *ss, const int64_t *thetas, const int32_t *traj_id,
                 unsigned flags, double *out);

/* Same input, but the n results stay in HBM: d_out (device, n doubles) is written asynchronously on `hip_stream`
 * (a hipStream_t, NULL = default stream), nothing is copied back and nothing is waited for.  This is what a
 * multi-GPU AMIS step uses: the shard's results go straight into the all-gather (dist.ShardedModel). */
int bild_logl_st_to_device(const bild_model *m, const bild_trajset *ts, int64_t n, int K1,
                           const double *ss, const int64_t *thetas, const int32_t *traj_id,
                           unsigned flags, void *hip_stream, double *d_out);

/* bild_logl_st_to_device waits for nothing, so it cannot refuse a row that is not a point on the simplex (negative or
 * non-finite interval lengths): such a row gets NaN as its result and the model remembers it.  This call waits for the
 * model's pending to_device calls, returns BILD_ERR_INVALID if any row was refused since the last query (*bad_row: one
 * of them, else -1; may be NULL) and forgets the verdict.  bild_logl_st itself reports such rows directly. */
int bild_logl_st_status(const bild_model *m, int64_t *bad_row);

/* The conversion alone (host only, no GPU): FixedkSampler.st2profile's switch frames (bild/amis.py:685-693) as
 * run-length segments.  Sample r belongs to a trajectory of T[r * T_stride] frames (T_stride 0: one length for all).
 * seg_start / seg_state: n x K1 int32 out. */
int bild_segments_from_st(int64_t n, int K1, int n_states, const int32_t *T, int64_t T_stride,
                          const double *ss, const int64_t *thetas,
                          int32_t *seg_start, int32_t *seg_state);

/* expanded profiles (MSRouse_logL semantics, pyx:95-98): states is n rows of length
 * ld >= max T, row r holds T[traj_id[r]] valid entries.  Run-length encoded on the host,
 * then as above. */
int bild_logl_profiles(const bild_model *m, const bild_trajset *ts, int64_t n, int64_t ld,
                       const int32_t *states, const int32_t *traj_id, unsigned flags,
                       double *out);

/* device buffers in, device buffer out; asynchronous on `hip_stream` (a hipStream_t, or
 * NULL for the default stream).  This is the entry point timed by bench.py: nothing
 * crosses PCIe.  d_out must hold n doubles.  Re-entrant: concurrent launches of one model on
 * different streams share no scratch (partial results of d* > 1 live in a per-call, stream-ordered
 * allocation).  The descriptors are NOT validated unless BILD_VALIDATE_DEVICE is set in `flags`. */
int bild_logl_segments_device(const bild_model *m, const bild_trajset *ts, int64_t n, int K1,
                              const int32_t *d_seg_start, const int32_t *d_seg_state,
                              const int32_t *d_traj_id, unsigned flags, void *hip_stream,
                              double *d_out);

/* The sampler's own (s, theta) rows, RESIDENT IN HBM: d_ss (n x K1 float64), d_thetas (n x K1 uint8), d_traj_id (n int32
 * or NULL).  Everything FixedkSampler.logL does for a batch happens on the device, asynchronously on `hip_stream`: switch
 * frames as st2profile computes them (bild/amis.py:685-688), cleaning, the table walk, the frame loop for the chains of
 * close switches, results to d_out (n doubles).  K1 <= 16.  Rows that are no points on the simplex (negative / non-finite
 * interval lengths, a state >= S) get NaN; d_status (2 ints in device-visible memory, zeroed by the caller, or NULL)
 * then holds {1, such a row}.  This is the entry bench.py times as `value`: candidates in HBM as the sampler produced
 * them, nothing converted, ordered or scheduled beforehand. */
int bild_logl_st_device(const bild_model *m, const bild_trajset *ts, int64_t n, int K1,
                        const double *d_ss, const uint8_t *d_thetas, const int32_t *d_traj_id,
                        unsigned flags, void *hip_stream, double *d_out, int32_t *d_status);

/* ------------------------------------------------- prefix table and launch order -------
 * Until its first switch a candidate's filter state depends only on (trajectory, localization-error chain, initial
 * state, frame) -- not on the candidate.  At the first evaluation of a trajectory set on the modal path (chains of up to
 * 32 modes) the library therefore runs the recursion once per (trajectory, chain, state) WITHOUT switches, keeps the state
 * after every frame in HBM (T x S x d* records of ~1 KB; skipped when it would take more than a quarter of the free
 * memory), and every candidate starts from the record in front of its first switch.  Same kernel, same arithmetic:
 * results are bit-identical to running every candidate from frame 0 (BILD_NO_PREFIX).  One-time cost per trajectory
 * set: one launch of about the duration of a single candidate, reported by bild_prefix_info.
 *
 * Behind a switch a Kalman filter forgets its starting point at a geometric rate: after a few tens of frames the
 * candidate's state [C | M] agrees with the table's record of the same frame and state to rounding.  The kernel checks
 * exactly that (whole state, first 24 frames behind the switch and then after as many frames as the measured deviation
 * still needs at the usual rate of decay; relative tolerance 2^-43 per column) and,
 * once it holds, takes the table's sums up to the candidate's next switch and continues from the record in front of
 * it: equal state + same propagator + same data = same future.  Nothing is assumed about stationarity; a candidate
 * that does not converge runs every frame.  This changes results by ~1e-12 (differences of running sums, tolerance of
 * the comparison); BILD_NO_JUMP switches it off.  A result never depends on the other candidates of the batch.
 *
 * Transient tables.  A transient that starts on the switch-free filter of the old state depends on (trajectory, chain,
 * old state, new state, frame) only.  Right behind the prefix table the library lets the kernel evaluate one candidate
 * per such switch and keeps how many frames the transient took to converge and what it added to the log-likelihood
 * beyond the new state's own sums (16 bytes per entry).  A candidate whose next switch is at least that many frames
 * away takes the entry and runs nothing.  Second level, the pair table: two switches closer together than the first
 * one's transient, keyed by (old, middle, new state, frame, gap <= 64) -- built for trajectory sets where the build (a
 * launch of T x gaps x S(S-1)^2 short tasks per trajectory) needs at most 40 M tasks; chains of three and more close
 * switches are run frame by frame from the table's state in front of them.  All tables are built at the FIRST evaluation
 * on a trajectory set and never later, and whether they are built depends on the set alone: results are reproducible
 * bit for bit for a given trajectory set whatever was evaluated before, in whatever batches and order.  The same candidate
 * evaluated on two different sets (one trajectory alone / among hundreds) may take its sums from different tables and
 * agrees to ~1e-11.  BILD_NO_TRANSIENTS=1 / BILD_NO_PAIRS=1 (environment) switch a level off for experiments;
 * BILD_PAIRS_MAX_TASKS=<n> replaces the 40 M budget (sets of many trajectories that will see hundreds of batches).
 *
 * Candidates then differ in length, so the order in which they are dealt to wavefronts matters for speed (never for
 * results).  The host-buffer entry points schedule internally (batches larger than the chip holds at once: on the device,
 * behind the upload; BILD_NO_SCHEDULE=1 switches every scheduling off).  For device-resident candidates the caller may obtain
 * the launch order once (bild_schedule_segments, host arrays) and pass it, device-resident, to
 * bild_logl_segments_device_ordered: order[slot] = index of the sample evaluated in slot `slot`; a permutation of
 * 0..n-1 (checked only with BILD_VALIDATE_DEVICE).  NULL = the order of the arrays. */
int bild_schedule_segments(const bild_model *m, const bild_trajset *ts, int64_t n, int K1,
                           const int32_t *seg_start, const int32_t *seg_state,
                           const int32_t *traj_id /* may be NULL */,
                           unsigned flags, int32_t *order /* out, n */);
int bild_logl_segments_device_ordered(const bild_model *m, const bild_trajset *ts, int64_t n, int K1,
                                      const int32_t *d_seg_start, const int32_t *d_seg_state,
                                      const int32_t *d_traj_id, const int32_t *d_order,
                                      unsigned flags, void *hip_stream, double *d_out);
/* frames (task x frame pairs) of a batch, and how many of them the launch really runs when candidates start from the
 * prefix table in the given launch order (host arrays; order may be NULL): the executed-operation count of a launch is
 * bild_flop_count's `executed` times frames_run / frames_total */
int bild_frames_executed(const bild_model *m, const bild_trajset *ts, int64_t n, int K1,
                         const int32_t *seg_start, const int32_t *traj_id, const int32_t *order,
                         unsigned flags, double *frames_total, double *frames_run);
/* frames the tasks of all launches of this model ran themselves since the last call (counted on the device while
 * bild_kernel_timing is enabled; the rest came out of the prefix table); resets the counter; synchronises the device */
int bild_frames_run_read(const bild_model *m, int64_t *frames);
/* diagnostics: while d_buffer (device, one int32 per task = sample x localization-error chain) is set, every launch of
 * the vector kernels records how many frames each task ran itself; NULL switches it off */
int bild_debug_frames_per_task(int32_t *d_buffer);
/* size of the tables (prefix, transient, pair) in bytes (0: none built) and the device time their construction took */
int bild_prefix_info(const bild_trajset *ts, int64_t *bytes, double *build_ms);

/* ---------------------------------------------------------- several GPUs ------------
 * One process per GPU.  The evaluations of a batch are independent, so ranks evaluate disjoint shards with no
 * communication inside the likelihood; the ONE exchange of an AMIS step is an all-gather of the shards' results
 * (every rank forms the importance weights from the full vector, bild/amis.py:843-845).  These calls put that
 * collective behind the C ABI, on RCCL over xGMI, so that a multi-GPU host program needs nothing but this library:
 *
 *   rank 0:      bild_comm_unique_id(id)            -> 128 bytes, to be handed to every rank by ANY channel the host
 *                                                      program has (file, socket, MPI, torch.distributed store ...)
 *   every rank:  bild_comm_create(id, world, rank)  on the device that is current (one per rank)
 *   per step:    bild_logl_st_to_device(... stream, d_local)   results of the rank's shard stay in HBM
 *                bild_comm_allgather(comm, d_local, d_all, n_per_rank, stream)   same stream: ordered behind the kernel
 *                one device-to-host copy of d_all
 *
 * Shards must be padded to a common length n_per_rank.  RCCL is located at run time (an RCCL already loaded into the
 * process is used; else librccl.so.1; bild_comm_library(path) or BILD_AMD_RCCL name another one); without one the
 * calls fail with BILD_ERR_UNSUPPORTED.  bild_amd/dist.py (LibraryComm, ShardedModel) is the Python binding. */
#define BILD_COMM_ID_BYTES 128
typedef struct bild_comm bild_comm;
int bild_comm_library(const char *path);
int bild_comm_unique_id(char *id, int id_len);
int bild_comm_create(const char *id, int world, int rank, bild_comm **out);
int bild_comm_allgather(bild_comm *c, const double *d_send, double *d_recv, int64_t n_per_rank, void *hip_stream);
int bild_comm_destroy(bild_comm *c);
/* device buffers for a host program that brings no GPU framework of its own (shard and gathered vector above);
 * bild_device_to_host copies on `hip_stream` and waits for it */
int bild_device_alloc(int64_t bytes, void **out);
int bild_device_free(void *ptr);
int bild_device_to_host(void *dst, const void *d_src, int64_t bytes, void *hip_stream);

/* The direct exchange: the same all-gather as ONE kernel per rank that stores the rank's shard straight into every
 * peer's receive block (mapped through an IPC handle; over xGMI between GPUs) and waits for the peers' shards there --
 * for the 10-256 KB a rank contributes per AMIS step a ring collective is latency-bound (7 dependent hops on 8 GPUs), a
 * one-shot peer write is one hop.  Replaces nothing in the reference (bild/amis.py:732-733 declines to
 * parallelise); the vector it assembles is the one bild/amis.py:843-845 consumes.
 *
 *   every rank:  bild_exchange_create(world, rank, slot_doubles, &x)      on its current device; slot_doubles >= longest shard
 *                bild_exchange_handle(x, handle)                          64 bytes, to be handed to every rank by any channel
 *                bild_exchange_connect(x, handles)                        all ranks' handles in rank order (world x 64 bytes)
 *   per step:    bild_logl_st_to_device(... stream, d_local)
 *                bild_exchange_allgather(x, d_local, n, stream, d_all)    same stream; d_all: world x n doubles on the device
 *                (consume d_all on that stream, or copy it to the host: bild_device_to_host)
 *                bild_exchange_status(x, &peer)                           after the stream has been waited for: a peer that
 *                                                                         did not deliver within the timeout (5 s) is an error
 * Every rank must call bild_exchange_allgather the same number of times with the same n.  world <= 16.  The waits are
 * bounded: a rank whose peer never arrives gets BILD_ERR_HIP from bild_exchange_status instead of a hung GPU.
 * bild_exchange_set_step (tests: rehearse the wrap of the 32-bit step counter; the same call on every rank, with no
 * exchange in flight) and bild_exchange_set_timeout are for tests and tools. */
#define BILD_EXCHANGE_HANDLE_BYTES 64
typedef struct bild_exchange bild_exchange;
int bild_exchange_create(int world, int rank, int64_t slot_doubles, bild_exchange **out);
int bild_exchange_handle(const bild_exchange *x, char *handle);
int bild_exchange_connect(bild_exchange *x, const char *handles);
int bild_exchange_allgather(bild_exchange *x, const double *d_send, int64_t n, void *hip_stream, double *d_recv);
int bild_exchange_status(bild_exchange *x, int *peer);
int bild_exchange_set_step(bild_exchange *x, uint32_t step);
int bild_exchange_set_timeout(bild_exchange *x, double seconds);
int bild_exchange_destroy(bild_exchange *x);

/* canonical floating-point operations of one batch,
 *   F = (T-1)(4 N^3 d* + 2 N^2 d) + Tv((4 N^2 + 3 N) d* + 4 N d)      
 * summed over samples, and the operations the selected path actually executes. */
int bild_flop_count(const bild_model *m, const bild_trajset *ts, int64_t n,
                    const int32_t *traj_id /* host, may be NULL */, unsigned flags,
                    double *canonical, double *executed);

/* name and accumulated device time (ms, HIP events on the launch stream) of the kernel the
 * most recent evaluations ran; resets the accumulator.  Used by bench.py for the roofline
 * figure.  Timing is off unless enabled. */
/* enable = 0: off; 1: every launch is bracketed by events; p > 1: every p-th launch (the events themselves cost a few
 * microseconds per launch: sampling keeps them out of most steps of a timed region) */
int bild_kernel_timing(int enable);
int bild_kernel_timing_read(double *total_ms, int64_t *launches, char *name, int name_len);
/* the same for the table-walk kernel that precedes the frame loop in a split launch (see "split launches" above) */
int bild_kernel_timing_read_walk(double *total_ms, int64_t *launches);

/* ------------------------------------------------ host-side AMIS bookkeeping -------
 * SURVEY section 8, row f-1.  Plain host code (no GPU): everything reference
 * bild/amis.py FixedkSampler.step (amis.py:805-906) does once the likelihood of the new
 * batch is known -- mixture denominators of all samples drawn so far, weights, refit of
 * the Dirichlet (amis.py:110-151) and CFC (amis.py:284-399) proposals, brakes
 * (amis.py:856-874), evidence / standard error / KL (amis.py:876-903) -- in one pass over
 * the pooled samples.  Random numbers are drawn by the caller (NumPy stream, reference
 * order).  bild_amd/amis.py holds the same bookkeeping in NumPy as the specification.
 *
 *   k1 = k + 1 intervals, n states, transitions[from*n + to] != 0 where allowed
 *   a0 (k1), logp0 (n x k1, [state][slot]): the initial proposal
 */
typedef struct bild_amis bild_amis;
int bild_amis_create(int k1, int n, const uint8_t *transitions, double concentration_brake,
                     double polarization_brake, double logprior, const double *a0,
                     const double *logp0, bild_amis **out);
int bild_amis_destroy(bild_amis *m);
const char *bild_amis_error(const bild_amis *m);
int64_t bild_amis_pool_size(const bild_amis *m);
int64_t bild_amis_num_proposals(const bild_amis *m);
/* proposal `which` (negative: from the end); either output may be NULL */
int bild_amis_params(const bild_amis *m, int64_t which, double *a, double *logp);
/* pooled per-sample arrays: 0 logLs, 1 log mixture denominators, 2 log density under the
 * current proposal, 3 log weights */
int bild_amis_pool(const bild_amis *m, int what, double *out);
/* rebuild a freshly created sampler from saved state: Q_extra further proposals (a: Q_extra x k1,
 * logp: Q_extra x n x k1) and P pooled samples with their per-sample arrays */
int bild_amis_restore(bild_amis *m, int64_t Q_extra, const double *a, const double *logp, int64_t P,
                      const double *ss, const int64_t *thetas, const double *logLs,
                      const double *logd, const double *cur, const double *logw);
/* traces from the current proposal (amis.py:223-256); u: k1 blocks of N uniform numbers */
int bild_amis_sample_traces(const bild_amis *m, int64_t N, const double *u, int64_t *thetas);
/* one iteration: ss (N x k1), thetas (N x k1), logLs (N) -> evidence[3] = (logev, dlogev, KL);
 * a CFC fit that does not converge returns BILD_ERR_INVALID with
 * bild_amis_error() == "Iteration did not converge" (the reference raises RuntimeError) */
int bild_amis_step(bild_amis *m, int64_t N, const double *ss, const int64_t *thetas,
                   const double *logLs, double *evidence);
/* The fused step (pooled samples on the device, see bild_amis_use_device below; K1 = k + 1 <= 16): the new samples go up
 * ONCE, as the (s, theta) rows the likelihood kernels read, straight into the pool; their log-likelihood on `ts` (one
 * trajectory) is computed there (as bild_logl_st would) and written into the pool; the passes over the pool follow on the
 * same stream.  Nothing but a few hundred partial sums comes down; the host's copy of the pool (bild_amis_pool) catches up
 * when it is asked for.  Same results as bild_logl_st followed by bild_amis_step. */
int bild_amis_step_fused(bild_amis *m, const bild_model *model, const bild_trajset *ts, int64_t N,
                         const double *ss, const int64_t *thetas, unsigned flags, double *evidence);
/* The same with the N samples DRAWN on the device from the current proposal -- a counter-based generator (Philox-4x32-10)
 * keyed by `seed`, one stream per (k + 1, index of the sample in the pool): counter (pool index low, pool index high, k + 1,
 * block), the pool index of sample r of the step being the pool size before the step + r, so a sample is a pure function of
 * (seed, k + 1, pool index, the proposal); uniforms two per block, words (2, 3) before words (0, 1); gamma variates by
 * Marsaglia-Tsang, each normal the cosine of a Box-Muller pair of two uniforms, traces slot by slot from the CFC weights
 * (tests/philox_oracle.py: amis_draw states the whole draw).  Opt-in: not the reference's NumPy random stream
 * (bild/amis.py:831-832), the same sampler in distribution.
 * Nothing goes up but the proposal's parameters.  bild_amis_pool_samples brings the pooled samples to the host. */
int bild_amis_step_device_rng(bild_amis *m, const bild_model *model, const bild_trajset *ts, int64_t N,
                              uint64_t seed, unsigned flags, double *evidence);
int bild_amis_pool_samples(const bild_amis *m, double *ss /* P x k1 */, int64_t *thetas /* P x k1 */);
/* keep the pooled samples in HBM and run the passes of bild_amis_step over them on the GPU (enable != 0), or return
 * to the host implementation (0).  Same arithmetic per sample (csrc/amis_math.h); sums are formed per block in a fixed
 * order, so results are reproducible and agree with the host's to rounding.  For batches of thousands of samples per
 * step; BILD_ERR_UNSUPPORTED when n_states * (k + 1) > 64, BILD_ERR_NO_DEVICE without a GPU. */
int bild_amis_use_device(bild_amis *m, int enable);

/* Histograms behind the choice of the next k in the adaptive-k loop (reference
 * bild/choicesampler.py:115-210): rvs (samplesize x kmax) common random sample, mu (kmax)
 * evidence estimates (NaN = ignored), dmu (kmax) natural step sizes, omit (kmax) flags or
 * NULL.  Outputs (any may be NULL): n0[kmax], dn[kmax][kmax], n_omit[kmax]. */
int bild_choice_counts(int64_t samplesize, int kmax, const double *rvs, const double *mu,
                       const double *dmu, double dE, const uint8_t *omit,
                       int64_t *n0, int64_t *dn, int64_t *n_omit);

/* ------------------------------------------------ the inference driver ------------
 * the adaptive-k loops of bild.core.sample (bild/core.py:138-227) for MANY trajectories
 * as one native state machine, advanced one ROUND at a time.  A round is one iteration of that loop for every trajectory
 * that is still running: at most one AMIS step (bild/amis.py:805-906) per trajectory, the exhaustive enumerations of the
 * samplers it opens (bild/amis.py:741-803), the choice sampler that picks the next k (bild/choicesampler.py:83-210) and
 * the stop rules -- with ONE likelihood call for all candidate rows of the round, and the per-trajectory bookkeeping on a
 * pool of host threads (BILD_HOST_THREADS, default min(8, cores)).
 *
 * Random numbers are NOT drawn by the library: bild_run_plan says how many the round needs, the caller draws them in
 * bulk from whatever stream it keeps (bild_amd.core.sample_many: three vectorised NumPy calls per round) --
 *     gammas    counts[0] standard gamma variates with the shape parameters *gamma_shapes  (np.random.standard_gamma)
 *     uniforms  counts[1] numbers in [0, 1)                                                  (np.random.random_sample)
 *     normals   counts[2] standard normal numbers                                            (np.random.standard_normal)
 * and per trajectory they are consumed in the reference's order: the gamma variates of the Dirichlet draw (normalised
 * exactly as np.random.dirichlet does: sequential sum, one reciprocal), the uniforms of the state traces (k + 1 blocks
 * of N, bild_amis_sample_traces), the samplesize x kmax normals of the choice sampler.  A run of ONE trajectory therefore
 * walks through the random numbers bild.core.sample would and reproduces it bit for bit.
 *
 * Per-k constants that do not depend on the trajectory are the caller's to provide, for k = 0 .. n_k - 1 (n_k >= k_max + 1):
 *     logp0     the CFC weights of the uniform distribution over traces (CFC.logp_uniform, amis.py:455-476),
 *               concatenated: n_states x (k + 1) doubles for each k
 *     logprior  log k! - log N_total(k)                                  (amis.py:654-659)
 *     n_total   N_total(k), the number of valid traces                   (amis.py:478-497)
 *     n_traces / traces   for every k that may be enumerated: all valid traces (CFC.full_sample, amis.py:499-536),
 *               n_traces[k] x (k + 1) int32, concatenated over k; n_traces[k] = 0: none given
 */
typedef struct bild_run bild_run;
typedef struct bild_run_settings {
    int32_t init_runs;            /* AMIS steps a freshly opened sampler takes at once (core.py:24: 20)   */
    int32_t k_lookahead;          /* core.py:26: 2                                                          */
    int32_t k_max;                /* core.py:27: 20                                                         */
    int32_t reserved;
    double  certainty_in_k;       /* stop when max p(k) reaches it (core.py:25: 0.99)                      */
    double  dE;                   /* evidence margin (core.py:23: 0)                                        */
    int64_t N;                    /* candidates per AMIS step (amis.py:624: 100)                            */
    double  concentration_brake;  /* amis.py:625: 1e-2                                                      */
    double  polarization_brake;   /* amis.py:626: 1e-3                                                      */
    int64_t max_fev;              /* amis.py:627: 20000                                                     */
    int64_t max_fcomplete;        /* amis.py:628: 1000                                                      */
    int64_t choice_samplesize;    /* choicesampler.py:83: 10000                                             */
} bild_run_settings;
int bild_run_create(int n_traj, const int32_t *T, int n_states, const uint8_t *transitions,
                    const bild_run_settings *settings, int n_k, const double *logp0, const double *logprior,
                    const double *n_total, const int64_t *n_traces, const int32_t *traces, bild_run **out);
int bild_run_destroy(bild_run *r);
const char *bild_run_error(const bild_run *r);
/* counts[8]: gammas, uniforms, normals, candidate rows of the round, trajectories still running, AMIS steps in the round,
 * trajectories that have failed so far (bild_run_traj_info), reserved.
 * counts[3] == 0 and counts[4] == 0: the run is over (no stage / finish for this plan). */
int bild_run_plan(bild_run *r, int64_t *counts, const double **gamma_shapes);
/* the whole round on the GPU: rows from the random numbers, bild_logl_st over them (traj_id = index of the trajectory in
 * the set `ts`, which must hold the run's trajectories in order), bookkeeping */
int bild_run_round(bild_run *r, const bild_model *m, const bild_trajset *ts, unsigned flags,
                   const double *gammas, const double *uniforms, const double *normals);
/* the same in three steps for a caller that evaluates the rows itself (CPU tests, models that are not this library's):
 * stage, look at the rows (ss: n x K1 float64, thetas: n x K1 int64, traj_id: n; rows shorter than K1 are padded with
 * empty intervals in their last state), finish with their log-likelihoods */
int bild_run_stage(bild_run *r, const double *gammas, const double *uniforms);
int bild_run_rows(const bild_run *r, int64_t *n, int *K1, const double **ss, const int64_t **thetas,
                  const int32_t **traj_id);
int bild_run_finish(bild_run *r, const double *logLs, const double *normals);
/* results.  traj_info: info[5] = state (0 running, 1 done, 2 failed), kind of failure (1: "Iteration did not converge",
 * a RuntimeError in the reference; 2: ValueError; 3: other), samplers, log rows, widest pk / KLD row.
 * traj_log: k, flags (bit 0: pk given, 1: KLD given, 2: I_la given; bits 8-15 / 16-23: entries of the pk / KLD row), I_la,
 * pk and KLD (rows x width, NaN-padded).
 * sampler_info: info[5] = kind (0: k >= T, 1: enumerated, 2: AMIS), exhausted, AMIS steps, evidences, enumerated rows.
 * sampler_data: evidences (x 3); for an enumerated sampler its rows.  take_core: ownership of an AMIS sampler's native
 * bookkeeping passes to the caller (bild_amis_destroy).  totals[3]: rounds, likelihood evaluations, host threads. */
int bild_run_traj_info(const bild_run *r, int j, int64_t *info, const char **message);
int bild_run_traj_log(const bild_run *r, int j, int32_t *k, int32_t *flags, double *i_la, double *pk, double *kld);
int bild_run_sampler_info(const bild_run *r, int j, int k, int64_t *info);
int bild_run_sampler_data(const bild_run *r, int j, int k, double *evidences, double *ss, int64_t *thetas,
                          double *logLs);
int bild_run_take_core(bild_run *r, int j, int k, bild_amis **out);
int bild_run_totals(const bild_run *r, int64_t *totals);

/* Weighted state occupancy per frame over a set of profiles (reference bild/amis.py:945-972):
 * post[s*T + t] = sum of w[p] over the profiles p that are in state s at frame t.  Profiles as
 * in bild_logl_segments (P x k1).  Sums of non-negative terms only. */
int bild_interval_marginals(int64_t P, int k1, int n, int64_t T, const int32_t *seg_start,
                            const int32_t *seg_state, const double *w, double *post);

/* ---------------------------------------------------------------- GenericGaussianModel -------
 * The reference's model-agnostic Gaussian model (bild/models.py:536-728): every state n and dimension k is a Gaussian
 * process given by its MSD, its mean m and its steady-state order (0: the positions are stationary, 1: the increments
 * are).  The likelihood of a profile is a sum over its intervals of the Gaussian log-density of the interval's window:
 * [0, t1) for the first interval, [t0 - 1, t1) for the others, valid frames only, per dimension; ss_order 0 conditions a
 * later interval on the first valid value of its window (taken raw, as the reference does), ss_order 1 uses the
 * increments between consecutive valid frames, minus m.  A later ss_order-0 interval whose window has no valid frame in
 * some dimension (the reference raises IndexError) makes that candidate's result NaN.  Derivation, covariance rule and
 * costs: DESIGN.md, "GenericGaussianModel".
 *
 * A trajectory set builds, for every trajectory and state, the term of every window [a, b) (T (T + 1) / 2 doubles) and
 * of every first interval (T + 1), summed over the dimensions in index order; an evaluation is k + 1 reads of those.
 * Results are a pure function of (candidate, trajectory set): bit-identical whatever the batch, its order and the entry
 * point. */
typedef struct bild_gauss_model bild_gauss_model;
typedef struct bild_gauss_trajset bild_gauss_trajset;

/* S states, d dimensions; per (state, dimension) i = s*d + k: ss_order[i] in {0, 1}, mean[i], the MSD at the integer
 * lags 0 .. Tmax (msd[i*(Tmax+1) + lag]) and its limit msd_inf[i] (read for ss_order 0 only).  Host memory only: needs
 * no GPU. */
int bild_gauss_model_create(int S, int d, int Tmax, const int32_t *ss_order, const double *mean, const double *msd,
                            const double *msd_inf, bild_gauss_model **out);
int bild_gauss_model_destroy(bild_gauss_model *m);

/* n_traj trajectories of T[j] frames each (1 <= T[j] <= 2048, T[j] - 1 <= Tmax), x: their T[j] x d values one after the
 * other, row-major, NaN = missing.  Uploads them and builds the tables before it returns (BILD_ERR_UNSUPPORTED beyond
 * 2048 frames).  The model must outlive the set. */
int bild_gauss_trajset_create(const bild_gauss_model *m, int n_traj, const int32_t *T, const double *x,
                              bild_gauss_trajset **out);
int bild_gauss_trajset_destroy(bild_gauss_trajset *ts);
/* device bytes of the set's tables, and the wall time of their build in ms; either pointer may be NULL */
int bild_gauss_trajset_info(const bild_gauss_trajset *ts, int64_t *table_bytes, double *build_ms);

/* Evaluation, host buffers in and out, synchronous.  Segments as for bild_logl_segments (first start 0, later starts
 * >= 1 and non-decreasing, states < S; empty segments and boundaries between equal states are dropped, so the intervals
 * are the runs of equal state); traj_id may be NULL (all rows on trajectory 0). */
int bild_gauss_logl_segments(const bild_gauss_model *m, const bild_gauss_trajset *ts, int64_t n, int K1,
                             const int32_t *seg_start, const int32_t *seg_state, const int32_t *traj_id, double *out);
/* the sampler's (s, theta) rows as bild_logl_st takes them; the switch frames are computed on the device with the same
 * operations as FixedkSampler.st2profile.  A row that is no point on the simplex or names a state >= S gets NaN and the
 * call returns BILD_ERR_INVALID (the other rows' results are written all the same). */
int bild_gauss_logl_st(const bild_gauss_model *m, const bild_gauss_trajset *ts, int64_t n, int K1, const double *ss,
                       const int64_t *thetas, const int32_t *traj_id, double *out);

/* n trajectories of the model (GenericGaussianModel.trajectories_from_loopingprofiles), the batched form of the loop of
 * GenericGaussianModel.trajectory_from_loopingprofile.  Trajectory i has 1 <= T[i] <= 2048 frames, at most the model's
 * Tmax + 1 (else BILD_ERR_UNSUPPORTED), and the profile given by its segments (n x K1, as bild_gauss_logl_segments takes
 * them; starts >= T[i] pad); its intervals are the runs of equal state.  missing (sum T bytes, may be NULL) marks frames to
 * return as NaN (every dimension).  out receives the sum T x d values, trajectory after trajectory, row-major.
 *
 * Per (state, dimension) one lower Cholesky factor of the Toeplitz covariance of the longest window serves every
 * interval.  The model keeps these factors in device memory from its first call on and rebuilds
 * them when a longer trajectory arrives (the first call, and each growth, pays the factorisations); results do not
 * depend on that history.  Calls on one model are serialised.  A factor whose leading block of the size a column needs
 * has a pivot that is not finite and positive: BILD_ERR_INVALID, naming the state, the dimension and the size.
 *
 * normals != NULL (replay): per trajectory, one after the other, the normals in the order the loop draws them:
 * interval after interval, and within an interval dimension after dimension, for dimension k of the interval [t0, t1)
 * in state s
 *   first interval (t0 = 0):  t1 normals if ss_order[s][k] = 0, t1 - 1 if it is 1;
 *   later intervals:          t1 - t0 normals;
 * so sum_k (T[i] - ss_order[first state][k]) per trajectory.  They are uploaded in chunks of whole trajectories within
 * scratch_bytes, or, when that is 0, within min(1 GiB, a third of the free device memory); a trajectory that alone
 * exceeds the budget: BILD_ERR_UNSUPPORTED (in device mode as well, where the chunks are drawn on the device).
 * normals == NULL (device mode): the normal of (index i of the trajectory in the call, frame t, dimension k) -- the one
 * the loop would draw for frame t (for frame t + 1 ... : entry j of a first ss_order-1 interval belongs to frame j + 1,
 * every other entry j of interval [t0, t1) to frame t0 + j) -- is one of the Box-Muller pair of the Philox-4x32-10 block
 * with key = seed and counter (i, t / 2, k, 1), the cosine for even t, the sine for odd t (gauss.hip).  So trajectory i
 * does not depend on the other trajectories of the call.  Synchronous. */
int bild_gauss_simulate(const bild_gauss_model *m, int n, const int32_t *T, int K1, const int32_t *seg_start,
                        const int32_t *seg_state, const uint8_t *missing, const double *normals, uint64_t seed,
                        int64_t scratch_bytes, double *out);

/* ---------------------------------------------------------------- Rouse trajectory generator -------
 * n trajectories of the multi-state Rouse model (MultiStateRouse.trajectories_from_loopingprofiles), computed in each
 * state's modal coordinates: per state s an orthonormal eigenbasis V[s] (N x N, row = monomer, column = mode) with
 * B = V diag(b) V^T, Sig = V diag(sqrt_sig^2) V^T, C0 = V diag(sqrt_cinf^2) V^T, and VtG[s] = V^T G, VtM0[s] = V^T M0
 * (N x d); w (N) is the measurement vector.  Derivation: DESIGN.md section 11.
 *
 * Trajectory i has T[i] >= 1 frames and the profile given by its segments (n x K1, as bild_logl_segments takes them: first
 * start 0, later starts >= 1 and non-decreasing, states < S; starts >= T[i] pad).  Frame 0 is drawn from the steady state
 * of its state, frame t >= 1 propagates with the state in force at t.  missing (sum T bytes, may be NULL) marks frames to
 * return as NaN; loc_err (n x d) scales the localization noise.  out receives the sum T x d values, trajectory after
 * trajectory, row-major.
 *
 * normals != NULL (replay): per trajectory, one after the other, T N d normals of the dynamics (frame, mode, dimension;
 * frame 0 the steady state) and then T d of the localization noise -- the order in which
 * MultiStateRouse.trajectory_from_loopingprofile draws them.  They are uploaded in chunks of whole trajectories within
 * scratch_bytes, or, when that is 0, within min(1 GiB, a third of the free device memory); a trajectory that alone
 * exceeds the budget: BILD_ERR_UNSUPPORTED.  normals == NULL (device mode): the normals are a pure function of (seed,
 * index i of the trajectory in the call, frame, mode, dimension), those of the localization noise of (seed, i, frame,
 * dimension) -- Philox-4x32-10, one Box-Muller pair per two frames (sim.hip) --, so trajectory i does not depend on the
 * other trajectories of the call.  Synchronous.  BILD_ERR_UNSUPPORTED when N > 256 or d > 8. */
int bild_rouse_simulate(int S, int N, int d, const double *V, const double *b, const double *sqrt_sig,
                        const double *sqrt_cinf, const double *VtG, const double *VtM0, const double *w, int n,
                        const int32_t *T, int K1, const int32_t *seg_start, const int32_t *seg_state,
                        const uint8_t *missing, const double *loc_err, const double *normals, uint64_t seed,
                        int64_t scratch_bytes, double *out);

/* ---------------------------------------------------------------- Kalman filter and smoother ---------
 * Per-frame moments of candidate profiles on a trajectory set (MultiStateRouse.kalman): the filter of the likelihood
 * entries (same conventions: frame 0 starts from the steady state of state[0], frame t >= 1 is predicted with the state of
 * frame t, a frame with a NaN coordinate is predicted but not updated, one covariance per distinct localization error) and
 * the modified Bryson-Frazier smoother behind it, which inverts no predicted covariance.  Profiles as for
 * bild_logl_segments (n x K1, traj_id may be NULL).  Each output is n x T_max x d, frame-major per candidate; NaN behind
 * a candidate's own T; a NULL pointer is not computed.  For frame t, dimension k, y = w.x the noise-free measurement:
 *   terms                 -(e^2 / S + log S + log 2 pi) / 2 on observed frames, 0.0 on missing ones (summed: the logL)
 *   pred_mean, pred_var   mean and variance of the observation x_t given the frames before t (at t = 0 the steady state)
 *   filt_mean, filt_var   mean and variance of y_t given the frames up to t
 *   smooth_mean, smooth_var   the same given all frames
 *   innov                 standardized innovation (x_t - pred_mean) / sqrt(pred_var) on observed frames, NaN on missing
 * Envelope: the modal path, <= 32 effective modes (BILD_Q_NEFF), d <= 8, S <= 255, else BILD_ERR_UNSUPPORTED before any
 * device work.  A candidate's outputs are a pure function of (model, trajectory, profile): bit-identical whatever the
 * batch, its order, the chunking and the other trajectories of the set.  The call runs in chunks of whole candidates
 * whose workspace (records of the forward pass, about (L + 10) doubles per frame and chain, L = 8, 16 or 32 the modes
 * rounded up, and the outputs) fits scratch_bytes; 0: at most 1 GiB and a third of the free device memory.  The tables
 * of the set are neither built nor read.  Synchronous. */
typedef struct bild_kalman_out {
    double *terms, *pred_mean, *pred_var, *filt_mean, *filt_var, *smooth_mean, *smooth_var, *innov;
    int32_t T_max; /* frames per candidate in the outputs: >= T of every candidate's trajectory */
} bild_kalman_out;
int bild_kalman_segments(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *seg_start,
                         const int32_t *seg_state, const int32_t *traj_id, const bild_kalman_out *out, int64_t scratch_bytes);
/* The posterior mixture of the smoothed y over the candidates of each trajectory of the set, weights exp(log_weights)
 * normalised within the trajectory: mean = sum w m / W, var = sum w v / W + sum w (m - mean)^2 / W (law of total
 * variance), accumulated around the smoothed mean of the trajectory's highest-weight candidate (the first of them).
 * mean, var: n_traj x Tmax x d, Tmax the set's longest trajectory; NaN behind a trajectory's T and for a trajectory
 * without candidates or with all log-weights -inf.  NaN or +inf log-weights: BILD_ERR_INVALID.  The sums run in fixed
 * blocks of 64 of a trajectory's candidates in index order, so the result does not depend on the chunking; per-candidate
 * outputs stay on the device and only a chunk of them exists at a time. */
int bild_kalman_mixture(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *seg_start,
                        const int32_t *seg_state, const int32_t *traj_id, const double *log_weights, double *mean, double *var,
                        int64_t scratch_bytes);

/* ---------------------------------------------------------------- log-likelihood sensitivities ------
 * The log-likelihood of candidate profiles (the filter of bild_logl_segments, run as bild_kalman_segments runs it) with
 * its gradient and the innovations form of its Fisher information with respect to P <= 4 parameters theta_p, by forward
 * sensitivities of the filter in the modal basis of each state.  The caller gives the derivatives of the model arrays:
 * each member of bild_model_derivs is P x (the shape of the array of bild_model_create: S x N x N for dB, dSig, dC0,
 * S x N x d for dG, dM0), row-major, NULL = zero; ds2 is P x n_traj x d, the derivative of the variance of dimension k of
 * trajectory j (the square of its localization error), NULL = zero.  Per candidate r (traj_id may be NULL):
 *   logl[r]                  sum over frames and dimensions of the terms of bild_kalman_segments (equal to bild_logl_segments
 *                            to rounding, not bit for bit)
 *   grad[r * P + p]          d logl / d theta_p
 *   fisher[(r * P + p) * P + q]   sum over observed frames and dimensions of dS_p dS_q / (2 S^2) + de_p de_q / S, S the
 *                            innovation variance and e the innovation: positive semi-definite, and its expectation over
 *                            the data is the Fisher information
 * NULL outputs are not computed.  The derivatives are projected into the model's reduced coordinates and each state's modal
 * basis once per call; BILD_ERR_UNSUPPORTED, with the residual in the message and before any device work, when one leaves
 * the reduced subspace, when a dB or dSig is not diagonal in a state's modal basis (relative residual above 1e-9: the
 * parameter moves the eigenvectors -- bond strengths, loop positions, N, the measurement), or when two dimensions of one
 * covariance chain (equal localization errors) have different ds2.  Envelope: that of bild_kalman_segments, 0 <= P <= 4,
 * and P = 0 for models of 17 to 32 effective modes.  A candidate's results are a pure function of (model, trajectory,
 * profile, derivatives): bit-identical whatever the batch, its order, the chunking and the other trajectories of the set.
 * The call runs in chunks of whole candidates within scratch_bytes (0: at most 1 GiB and a third of the free device
 * memory); the tables of the set are neither built nor read.  Synchronous. */
typedef struct bild_model_derivs {
    const double *dB, *dG, *dSig, *dM0, *dC0;
} bild_model_derivs;
int bild_logl_sensitivities(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *seg_start,
                            const int32_t *seg_state, const int32_t *traj_id, int P, const bild_model_derivs *dm,
                            const double *ds2, double *logl, double *grad, double *fisher, int64_t scratch_bytes);

/* ---------------------------------------------------------------- GenericGaussianModel sensitivities --
 * The log-likelihood of candidate profiles under a GenericGaussianModel (the value of bild_gauss_logl_segments, to
 * rounding) with its gradient and the innovations form of its Fisher information with respect to P <= 4 parameters
 * theta_p, by forward tangents of the Cholesky factorisation of every window.  The caller gives the
 * derivatives of the model arrays of bild_gauss_model_create, each P x (that array's shape), row-major, NULL = zero: dmsd
 * P x S x d x (Tmax + 1), dmsd_inf and dmean P x S x d.  The trajectories are given directly, as bild_gauss_simulate takes
 * them (n_traj, T, x: sum T x d, NaN = missing): no interval tables are built.  Segments and traj_id (may be NULL) as for
 * bild_gauss_logl_segments.  Per candidate r:
 *   logl[r]                       the log-likelihood (bild_gauss_logl_segments to rounding, not bit for bit)
 *   grad[r * P + p]               d logl / d theta_p
 *   fisher[(r * P + p) * P + q]   sum over the counted entries of every window of dS_p dS_q / (2 S^2) + de_p de_q / S, S the
 *                                 innovation variance and e the innovation: symmetric, positive semi-definite, with the
 *                                 Fisher information as its expectation
 * NULL outputs are not written.  A candidate that bild_gauss_logl_segments gives NaN (a later ss_order-0 interval without a
 * valid frame) gets NaN in all of its outputs; the others are untouched.  A candidate's outputs are a pure function of
 * (model, derivatives, its trajectory, its profile): bit-identical whatever the batch, its order, duplicates, the chunking,
 * and (logl) whatever P and whether fisher is NULL.  Windows are de-duplicated across the call; the factorisations of
 * windows with a missing frame run in chunks within scratch_bytes (0: at most 1 GiB and a third of the free device memory).
 * Before any device work: BILD_ERR_UNSUPPORTED for P > 4 and for a trajectory of more than 2048 frames, BILD_ERR_INVALID
 * for a derivative that is not finite, a trajectory longer than the MSD tables (T - 1 > Tmax) and a bad segment row or
 * traj_id.  Synchronous. */
typedef struct bild_gauss_derivs {
    const double *dmsd, *dmsd_inf, *dmean;
} bild_gauss_derivs;
int bild_gauss_logl_sensitivities(const bild_gauss_model *m, int n_traj, const int32_t *T, const double *x, int64_t n, int K1,
                                  const int32_t *seg_start, const int32_t *seg_state, const int32_t *traj_id, int P,
                                  const bild_gauss_derivs *dm, double *logl, double *grad, double *fisher,
                                  int64_t scratch_bytes);

/* ---------------------------------------------------------------- GenericGaussianModel moments --------
 * Per-frame moments of candidate profiles under a GenericGaussianModel (GenericGaussianModel.kalman; DESIGN.md section
 * 16), from the Cholesky factorisation of every window of the likelihood.  Trajectories, segments and traj_id as for
 * bild_gauss_logl_sensitivities; outputs as for bild_kalman_segments (n x T_max x d each, NULL = not computed, NaN behind
 * a candidate's own T), each frame t of dimension k taken from the window of the interval that contains t.  With the
 * window's data vector y (entry j at its valid frame v_j, ss_order 0, or at v_{j+1}, the increment v_j -> v_{j+1},
 * ss_order 1), L L^T its covariance and z = L^-1 y:
 *   terms                 -(log L_jj + z_j^2 / 2 + log(2 pi) / 2) at the frame of an entry the likelihood counts, 0.0
 *                         elsewhere (summed: bild_gauss_logl_segments to rounding)
 *   pred_mean, pred_var   the observed coordinate given the earlier entries of its window, at counted frames (else NaN)
 *   innov                 z_j at counted frames (else NaN)
 *   smooth_mean, smooth_var   the observed coordinate given every valid frame of its window: the data and 0 at a valid
 *                         frame; the Gaussian conditional at a missing one (NaN for an ss_order-1 frame before the
 *                         window's first valid frame).  The MSDs include the localization noise, so these are moments of
 *                         the observed coordinate, not of a noise-free one.
 * filt_mean and filt_var must be NULL (the model has no filter): BILD_ERR_INVALID.  A later ss_order-0 window without a
 * valid frame (bild_gauss_logl_segments: NaN) gives NaN over its frames and dimension in every output.  A candidate's
 * outputs are a pure function of (model, its trajectory, its profile): bit-identical whatever the batch, its order,
 * duplicates and the chunking.  Windows are de-duplicated across the call; the factorisations of windows with a missing
 * frame, and the outputs, run in chunks within scratch_bytes (0: at most 1 GiB and a third of the free device memory).
 * Before any device work: the refusals of bild_gauss_logl_sensitivities, T_max shorter than a candidate's trajectory and
 * a negative scratch_bytes.  Synchronous. */
int bild_gauss_kalman_segments(const bild_gauss_model *m, int n_traj, const int32_t *T, const double *x, int64_t n, int K1,
                               const int32_t *seg_start, const int32_t *seg_state, const int32_t *traj_id,
                               const bild_kalman_out *out, int64_t scratch_bytes);
/* The posterior mixture of the smoothed coordinate over the candidates of each trajectory, weights exp(log_weights)
 * normalised within the trajectory, as bild_kalman_mixture forms it: mean = sum w m / W, var = sum w v / W +
 * sum w (m - mean)^2 / W, accumulated around the smoothed track of the trajectory's highest-weight candidate (the first of
 * them) in fixed blocks of 64 candidates in index order, weight 0 skipped; so the result does not depend on the chunking,
 * and at a valid frame the mean is the data and the variance 0.  mean, var: n_traj x T_max x d, T_max the longest
 * trajectory; NaN behind a trajectory's T and for a trajectory without candidates or with all log-weights -inf.  NaN or
 * +inf log-weights: BILD_ERR_INVALID, before any device work. */
int bild_gauss_kalman_mixture(const bild_gauss_model *m, int n_traj, const int32_t *T, const double *x, int64_t n, int K1,
                              const int32_t *seg_start, const int32_t *seg_state, const int32_t *traj_id,
                              const double *log_weights, double *mean, double *var, int64_t scratch_bytes);

/* ---------------------------------------------------------------- exact evidence by enumeration --------
 * For a fixed number k of switches, every profile of a trajectory of T frames: a switch combination c_1 < ... < c_k from
 * {1, ..., T - 1} (a segment starting at each c_i) and a valid trace, k + 1 states whose consecutive pairs transitions
 * (S x S, row-major, 0 / 1) allows.  Traces are the outer index in FixedkSampler's CFC.full_sample order, combinations
 * the inner one in itertools.combinations order: the order in which FixedkSampler.fix_exhaustive pools them.  Under the
 * uniform prior over these profiles, per trajectory:
 *   logev      log mean exp(logL): top = the largest logL, log(mean exp(logL - top)) + top
 *   kl         mean(logL exp(logL - top)) / mean(exp(logL - top)) - logev (KL of the posterior from the prior)
 *   map_*      the profile of largest logL, the first in the order above among equal maxima, as segments (k + 1 each),
 *              and its logL -- the value the likelihood call gives for it
 *   n_nan      candidates whose logL is NaN (GenericGaussianModel: DESIGN.md section 10).  With any of them logev, kl and
 *              the marginals are NaN, as on the host; the MAP is taken among the others.
 *   log_post   (NULL: not computed) the normalised log marginal posterior of the state at each frame, S x T_max per
 *              trajectory, NaN behind its T: log(sum of exp(logL - top) over the profiles in state s at frame t) minus the
 *              log of that sum over s -- sums of non-negative terms only.
 * A candidate with logL = -inf weighs 0 and adds 0 to kl's numerator (the host's formula gives NaN there).  A trajectory
 * with T - 1 < k has no profiles: logev -inf, kl NaN, map segments -1, map_logl NaN, log_post NaN; the others are computed
 * as usual.  Results are bit-identical across calls, the order of the set's trajectories, a trajectory alone or in a
 * batch, and scratch_bytes (the work is reduced in blocks of 4096 consecutive profiles of one trajectory and folded in
 * block order) -- given bit-identical log-likelihoods: MultiStateRouse gives those on one set (see "REPRODUCIBILITY
 * CONTRACT" above; the same trajectory on another set agrees to rounding).
 * Refused before any device work: k outside 0 .. 15 (BILD_ERR_UNSUPPORTED), a transitions entry other than 0 / 1, T_max
 * shorter than a trajectory of the set, a negative scratch_bytes (BILD_ERR_INVALID); more profiles in all than
 * max_profiles, 2^53 or more for one trajectory, more than 2^26 valid traces, and with log_post S x T above 8192 for a
 * trajectory (the LDS accumulators of a block) (BILD_ERR_UNSUPPORTED, the count in the message).  Chunks of whole blocks
 * run within scratch_bytes (0: at most 1 GiB and a third of the free device memory; at least one block).  Synchronous. */

/* host only, no device: C(T - 1, k) x (valid traces of k switches), as a double (exact below 2^53); T >= 1 */
int bild_exact_count(int T, int k, int S, const uint8_t *transitions, double *n_profiles);

typedef struct bild_exact_out {
    double *logev, *kl, *map_logl;          /* n_traj each */
    int32_t *map_seg_start, *map_seg_state; /* n_traj x (k + 1) */
    int64_t *n_nan;                         /* n_traj */
    double *log_post;                       /* n_traj x S x T_max, NULL = marginals not computed */
} bild_exact_out;                           /* every pointer may be NULL: not written */

/* MultiStateRouse: the profiles are evaluated by bild_logl_segments_device on the model's stream (evaluation path: the
 * low 4 bits of flags).  A set that has not been evaluated on yet and whose declaration (bild_trajset_expect) is below the
 * call's count -- or that has none and sees 1e8 profiles or more -- is declared for the count. */
int bild_exact_evidence(const bild_model *m, const bild_trajset *ts, int k, const uint8_t *transitions, double max_profiles,
                        int64_t scratch_bytes, int T_max, unsigned flags, bild_exact_out *out);
/* GenericGaussianModel: the walk of bild_gauss_logl_segments over the rows in HBM */
int bild_gauss_exact_evidence(const bild_gauss_model *m, const bild_gauss_trajset *ts, int k, const uint8_t *transitions,
                              double max_profiles, int64_t scratch_bytes, int T_max, bild_exact_out *out);

/* ---------------------------------------------------------------- exact evidence of every k by a segment recursion ----
 * GenericGaussianModel only.  The log-likelihood of a profile is a sum of per-segment table
 * entries, F[n_0][t1_0] + sum_i W[n_i][t0_i - 1][t1_i], so the sums over all profiles of k switches -- the profiles and the
 * uniform prior of "exact evidence by enumeration" above -- follow from a semi-Markov forward recursion over segments, for
 * every k = 0 .. k_max in one call and in O(k_max S T^2) terms.  With K = k_max + 1, per trajectory and k:
 *   logev        log mean exp(logL) over the profiles of k switches (-inf: no profile)
 *   kl           posterior mean of logL minus logev (NaN without profiles)
 *   map_logl     the largest logL, and map_seg_start / map_seg_state a profile that attains it: k + 1 segments, the rest
 *                of the row of K entries padded with empty segments at T in state 0 (-1 everywhere: no profile).
 *                Among equal maxima the smallest final state wins, then, from the last switch to the first, the
 *                smallest switch frame and then the smallest preceding state: a rule on the trajectory's own tables.
 *   n_profiles   profiles the mean is taken over; n_omitted: profiles left out of it (both as doubles, exact below 2^53)
 *   log_post     (NULL: not computed) normalised log marginal posterior of the state per frame, K x S x T_max per
 *                trajectory, NaN behind its T; sums of non-negative terms only.
 * A profile that uses a NaN window ("Deviation") is never a MAP candidate.  flags = 0
 * (BILD_SEGDP_NAN_PROPAGATE): logev, kl and log_post of a k with such a profile are NaN, n_profiles counts every profile
 * and n_omitted is 0.  BILD_SEGDP_NAN_OMIT: such profiles are left out of the sums and of n_profiles, and counted in
 * n_omitted.  A term of weight -inf weighs 0 and adds 0 to kl.  A k without a profile (T - 1 < k, or no valid trace) does
 * not affect the others.  No floating-point atomics: every reduction has a fixed order that depends on the trajectory
 * alone, so results are bit-identical across calls, the order of the set, a trajectory alone or in a batch, and
 * scratch_bytes (chunks of whole trajectories; 0: at most 1 GiB and a third of the free device memory; at least one
 * trajectory).  Refused before any device work: k_max outside 0 .. 64 (BILD_ERR_UNSUPPORTED), unknown flags, a transitions
 * entry other than 0 / 1, T_max shorter than a trajectory of the set, a negative scratch_bytes (BILD_ERR_INVALID).
 * Plain launches on the set's stream.  Synchronous. */
#define BILD_SEGDP_NAN_PROPAGATE 0u
#define BILD_SEGDP_NAN_OMIT 1u

typedef struct bild_segdp_out {
    double *logev, *kl, *map_logl;          /* n_traj x K each */
    double *n_profiles, *n_omitted;         /* n_traj x K */
    int32_t *map_seg_start, *map_seg_state; /* n_traj x K x K */
    double *log_post;                       /* n_traj x K x S x T_max, NULL = marginals not computed */
} bild_segdp_out;                           /* every pointer may be NULL: not written */

int bild_gauss_segment_evidence(const bild_gauss_model *m, const bild_gauss_trajset *ts, int k_max, const uint8_t *transitions,
                                int T_max, unsigned flags, int64_t scratch_bytes, bild_segdp_out *out);

/* ---------------------------------------------------------------- exact posterior draws of profiles ----
 * GenericGaussianModel only.  Independent draws from the exact posterior over the profiles of k
 * switches (the profiles and the uniform prior of the segment recursion above), by sampling a profile segment by segment
 * from the left against the backward tables of that recursion.  Draw r belongs to trajectory draw_traj[r] of the set and
 * has draw_k[r] switches (0 .. k_max); it consumes a row of U = max(1, 2 k_max) uniforms in [0, 1):
 *   u[0]       (s_0, t_1) jointly, the list ordered by state, then by the end frame b = 1 .. T, weights
 *              exp F[s][b] gamma_k(b, s) (gamma_m(b, s): the sum over the completions, m switches to come, of a profile
 *              whose segment in state s ends at b)
 *   u[2i - 1]  s_i among the q with transitions[s_{i-1}, q], ascending, weights beta_{k-i}(t_i, q) (beta_m(a, s) =
 *              sum_{b > a} exp W[s][a - 1][b] gamma_m(b, s)), for i = 1 .. k
 *   u[2i]      t_{i+1} among b = t_i + 1 .. T, ascending, weights exp W[s_i][t_i - 1][b] gamma_{k-i}(b, s_i), for i < k; the
 *              last segment ends at T and takes no uniform.
 * A pick returns the first entry of positive weight whose inclusive running weight exceeds u times the list's total, and the
 * last entry of positive weight where rounding carries that product past the end; an entry of weight 0 -- a NaN window
 * ("Deviation") or a term of -inf -- is never returned, so a NaN profile is never drawn.  A pick with
 * one candidate still consumes its uniform.  With K = k_max + 1, per draw:
 *   seg_start, seg_state  draw_k[r] + 1 segments, the rest of the row of K entries padded with empty segments at T in
 *                         state 0; -1 everywhere: the trajectory has no profile of positive weight with that many switches
 *   logl                  F[s_0][t_1] + sum_i W[s_i][t_i - 1][t_{i+1}], added from the left as bild_gauss_logl_segments adds
 *                         it; NaN for a -1 row
 *   uniforms_out          (may be NULL) the uniforms the draw consumed, in the layout of `uniforms`; 0 where none was
 * Replay: `uniforms` (n_draws x U) is given and `seed` ignored.  Device: uniforms == NULL; the uniforms of draw r are the
 * Philox-4x32-10 stream (key: seed; counter: r) taken in the order above, so a draw is a pure function of (seed, r, its
 * trajectory's tables, its k, transitions).  Results do not depend on the other draws, on the set's other trajectories or
 * their order, or on scratch_bytes (chunks of whole trajectories as in bild_gauss_segment_evidence; trajectories that no draw
 * names are skipped).  Refused before any device work: what bild_gauss_segment_evidence refuses, n_draws < 0, a draw_traj
 * or draw_k out of range, a uniform outside [0, 1) or NaN (BILD_ERR_INVALID).  n_draws = 0 returns at once.  Plain
 * launches on the set's stream, no atomics.  Synchronous. */
typedef struct bild_segdraw_out {
    int32_t *seg_start, *seg_state;         /* n_draws x K */
    double *logl;                           /* n_draws */
    double *uniforms_out;                   /* n_draws x U, or NULL */
} bild_segdraw_out;

int bild_gauss_segment_draw(const bild_gauss_model *m, const bild_gauss_trajset *ts, int k_max, const uint8_t *transitions,
                            int T_max, int64_t scratch_bytes, int64_t n_draws, const int32_t *draw_traj, const int32_t *draw_k,
                            const double *uniforms, uint64_t seed, bild_segdraw_out *out);

/* ---------------------------------------------------------------- evidence sensitivities ----
 * GenericGaussianModel only.  The gradient of the exact evidence of the segment recursion above with
 * respect to P <= 4 model parameters, for trajectories whose profile is not known.  With ev_k = exp(logev_k) of
 * bild_gauss_segment_evidence (same k_max, transitions and NaN flag; the same numbers, bit for bit) and a prior over k,
 * pi_k proportional to exp(log_k_prior[k]) (a row of K = k_max + 1 per trajectory, finite or -inf; NULL: uniform), per
 * trajectory:
 *   logev          K values, as bild_gauss_segment_evidence gives them
 *   log_marginal   log sum_k pi_k ev_k, pi normalised over k = 0 .. k_max
 *   k_post         K values: pi_k ev_k / sum pi ev
 *   grad           P values: d log_marginal / d theta_p.  By Fisher's identity it is the posterior mean of the gradient of the
 *                  log-likelihood: with Omega(s, a, t) the posterior probability (k mixed by k_post) that a segment in
 *                  state s starts at a and has not ended by frame t, grad_p = - sum Omega(s, a, t_j) dtau_p over the
 *                  entries j of the window that starts at a - 1 (the first window for a = 0), tau and dtau those of
 *                  bild_gauss_logl_sensitivities.
 *   exp_logl       - sum Omega tau: the posterior mean of the log-likelihood (one k: kl + logev of that k)
 *   fisher         P x P: sum Omega (2 a_p a_q + g_p g_q), the innovations form
 *                  of bild_gauss_logl_sensitivities, posterior-weighted.  This is the posterior mean of the complete-data
 *                  information: a scoring matrix for a fit.  It is NOT the information of the marginal likelihood, which
 *                  is smaller by the posterior covariance of the score; standard errors need the latter.
 * The trajectories' data are given as bild_gauss_simulate returns them (x: sum T x d in the set's order, NaN = missing);
 * they must be the data the set was built from.  Derivatives as for bild_gauss_logl_sensitivities.  A k of prior weight 0
 * is skipped, NaN or not.  flags = 0: a trajectory with a k of positive prior weight whose logev is NaN has NaN in
 * log_marginal, k_post, grad, exp_logl and fisher; the other trajectories are untouched.  A trajectory without a profile
 * of positive weight under the prior has log_marginal -inf and NaN in the rest.  NULL outputs are not written.  No
 * atomics, fixed summation orders that depend on the trajectory alone: results are bit-identical across calls, the order
 * of the set, a trajectory alone or in a batch, and scratch_bytes (chunks of whole trajectories, and of factorisations
 * of windows with a missing frame; 0: at most 1 GiB and a third of the free device memory).  tau sums do not depend on P.
 * Refused before any device work: what bild_gauss_segment_evidence and bild_gauss_logl_sensitivities refuse, a NaN or
 * +inf log_k_prior entry, a log_k_prior row that is -inf everywhere (BILD_ERR_INVALID).  Plain launches on the set's
 * stream.  Synchronous. */
typedef struct bild_segsens_out {
    double *logev;                          /* n_traj x K */
    double *log_marginal;                   /* n_traj */
    double *k_post;                         /* n_traj x K */
    double *grad;                           /* n_traj x P */
    double *exp_logl;                       /* n_traj */
    double *fisher;                         /* n_traj x P x P */
} bild_segsens_out;                         /* every pointer may be NULL: not written */

int bild_gauss_segment_sensitivities(const bild_gauss_model *m, const bild_gauss_trajset *ts, const double *x, int k_max,
                                     const uint8_t *transitions, unsigned flags, const double *log_k_prior, int P,
                                     const bild_gauss_derivs *dm, int64_t scratch_bytes, bild_segsens_out *out);

/* ---------------------------------------------------------------- exact inference under a dwell-time prior ----
 * GenericGaussianModel only, at most 4 states.  The profiles and the per-segment log-likelihood of
 * the segment recursion above, under an explicit-duration (semi-Markov) prior in place of the uniform prior per k: a profile
 * of segments [t_i, t_{i+1}) in states s_i, i = 0 .. k, t_0 = 0, t_{k+1} = T, lengths l_i = t_{i+1} - t_i >= 1, has
 *   log prior = log_init[s_0] + sum_{i<k} (log_dwell[s_i][l_i] + log_jump[s_i][s_{i+1}]) + log_surv[s_k][l_k]
 * (the last segment is right-censored; one segment over the whole trajectory gets log_init + log_surv[.][T]).  log_dwell and
 * log_surv are S x L, the entry of length l = 1 .. L at column l - 1, and serve every trajectory of the set; the ordinary
 * Markov chain is the geometric case.  Entries are finite or -inf.  There is one evidence per trajectory and no k:
 *   logev          log sum over all profiles of exp(log prior + logL)
 *   map_logjoint   the largest log prior + logL, and map_states a profile that attains it as T_max bytes of expanded states
 *                  (255 behind T, and everywhere without a profile of finite prior weight; map_logjoint is then NaN).  Among
 *                  equal maxima the smallest final state wins, then, from the last switch back, the smallest switch frame
 *                  and then the smallest preceding state.
 *   n_nan_windows  windows [a, b) in state s that were skipped because their table entry is NaN (DESIGN.md section 10,
 *                  "Deviation"), counted where the prior weight of the segment is finite and a partial profile of finite
 *                  prior weight without a NaN window reaches the start a in state s
 *   log_post       S x T_max: log P(theta_t = s | data), NaN behind T; sums of non-negative terms only, not renormalised
 *   exp_jumps      S x S: posterior expected number of jumps s' -> s
 *   exp_stay       S: posterior expected number of frames stayed, sum over the segments in s of (length - 1)
 * so that exp_jumps and exp_stay are the derivatives of logev with respect to log_jump and to the log of a Markov chain's
 * P_ss.  log_post == NULL skips the backward and the statistics passes; exp_jumps and exp_stay are then not written.
 * A NaN window never enters a maximum or a sum.  flags = 0 (BILD_DWELL_NAN_PROPAGATE): a trajectory with n_nan_windows > 0
 * has NaN in logev, log_post, exp_jumps and exp_stay; its MAP profile is taken among the other profiles.
 * BILD_DWELL_NAN_OMIT: the profiles that use such a window weigh 0, so logev is the evidence under the prior restricted to
 * the remaining profiles (not renormalised).  The device does the same work in both modes.  A trajectory without a profile of
 * positive weight has logev -inf and NaN in log_post, exp_jumps and exp_stay.  No atomics, fixed summation orders that depend
 * on the trajectory alone: results are bit-identical across calls, the order of the set, a trajectory alone or in a batch, and
 * scratch_bytes (chunks of whole trajectories; 0: at most 1 GiB and a third of the free device memory; at least one
 * trajectory).  Refused before any device work: more than 4 states (BILD_ERR_UNSUPPORTED), L shorter than a trajectory of the
 * set, a NaN or +inf table entry, a finite diagonal entry of log_jump (a self-jump would split what the likelihood treats as
 * one segment), log_init that is -inf everywhere, unknown flags, a negative scratch_bytes, T_max shorter than a trajectory of
 * the set (BILD_ERR_INVALID).  Plain launches on the set's stream.  Synchronous. */
#define BILD_DWELL_NAN_PROPAGATE 0u
#define BILD_DWELL_NAN_OMIT 1u

typedef struct bild_dwell_out {
    double *logev, *map_logjoint;           /* n_traj each */
    uint8_t *map_states;                    /* n_traj x T_max */
    int64_t *n_nan_windows;                 /* n_traj */
    double *log_post;                       /* n_traj x S x T_max, NULL = forward pass only */
    double *exp_jumps;                      /* n_traj x S x S */
    double *exp_stay;                       /* n_traj x S */
} bild_dwell_out;                           /* every pointer may be NULL: not written */

int bild_gauss_dwell_evidence(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                              const double *log_jump, const double *log_dwell, const double *log_surv, int T_max, unsigned flags,
                              int64_t scratch_bytes, bild_dwell_out *out);

/* ---------------------------------------------------------------- exact posterior draws under a dwell-time prior ----
 * GenericGaussianModel only, at most 4 states.  Independent draws from the exact posterior over the
 * profiles of every number of switches under the dwell-time prior of the block above (same tables, same refusals), by
 * sampling a profile segment by segment from the left against the backward tables of that recursion: beta(a, s) =
 * log sum_{b > a} exp(omega_s(a, b) + W[s][a - 1][b] + gamma(b, s)), gamma(b, s) = log sum_q exp(log_jump[s][q] + beta(b, q))
 * for b < T and 0 for b = T, with omega_s(a, b) = log_dwell[s][b - a] for b < T and log_surv[s][T - a] for b = T.  There is
 * no k and no k_max.  Draw r belongs to trajectory draw_traj[r] of the set and consumes uniforms u[0], u[1], .. in [0, 1):
 *   u[0]       (s_0, t_1) jointly, the list ordered by state, then by the end frame b = 1 .. T, log weights
 *              log_init[s] + omega_s(0, b) + F[s][b] + gamma(b, s); t_1 = T ends the draw with 0 switches
 *   u[2i - 1]  s_i among q = 0 .. S - 1, ascending, log weights log_jump[s_{i-1}][q] + beta(t_i, q); the list's total is
 *              gamma(t_i, s_{i-1})
 *   u[2i]      t_{i+1} among b = t_i + 1 .. T, ascending, log weights omega_{s_i}(t_i, b) + W[s_i][t_i - 1][b] + gamma(b, s_i);
 *              the list's total is beta(t_i, s_i).  The draw ends when a pick returns b = T,
 * for i = 1, 2, ..: a draw of k switches consumes exactly 1 + 2k uniforms (at most 2T - 1).  A pick returns the first entry
 * of positive weight whose inclusive running weight exceeds u times the list's total, and the last entry of positive
 * weight where rounding carries that product past the end; an entry of weight 0 -- a NaN window (DESIGN.md section 10,
 * "Deviation"), a prior term of -inf, gamma = -inf behind an absorbing state -- is never returned, so a NaN profile is never
 * drawn.  A pick with one candidate still consumes its uniform.  Per draw:
 *   states        T_max bytes: the expanded profile, 255 behind T (the layout of bild_dwell_out.map_states)
 *   n_switches    k
 *   logl          F[s_0][t_1] + sum_i W[s_i][t_i - 1][t_{i+1}], added from the left onto 0.0 as bild_gauss_logl_segments adds it
 *   log_prior     log_init[s_0], then per completed segment + log_dwell, + log_jump, at last + log_surv, in that order
 *   n_uniforms    the uniforms consumed
 *   uniforms_out  the first U uniforms consumed, 0 where none was
 * A trajectory without a profile of positive weight gives a row of 255, n_switches -1, NaN in logl and log_prior and
 * n_uniforms 0.  Device mode, uniforms == NULL: draw r takes its uniforms on demand, without limit, from the
 * Philox-4x32-10 stream (key: seed; counter: draw_stream[r], or r where draw_stream is NULL) in the order above, so a draw
 * is a pure function of (seed, its stream index, its trajectory's tables, the prior).  Replay, uniforms given (n_draws x
 * U): seed is ignored; a draw that needs more than U uniforms is not completed and gets the 255 row, n_switches -1, NaN
 * and n_uniforms -1 (U = 2 T_max - 1 always suffices).  U may be 0 in device mode: nothing is kept.  Results do not depend on
 * the other draws, on the set's other trajectories or their order, or on scratch_bytes (chunks of whole trajectories as in
 * bild_gauss_dwell_evidence, 16 S (T + 1) bytes each for beta and gamma, T the longest trajectory a draw names; trajectories
 * that no draw names are skipped; the forward tables are not built).  Refused before any device work: what
 * bild_gauss_dwell_evidence refuses, n_draws < 0, a draw_traj out of range, U < 0, a replay with U < 1, a uniform outside
 * [0, 1) or NaN (BILD_ERR_INVALID).  n_draws = 0 returns at once.  Plain launches on the set's stream, no atomics.
 * Synchronous. */
typedef struct bild_dwelldraw_out {
    uint8_t *states;                        /* n_draws x T_max */
    int32_t *n_switches;                    /* n_draws */
    double *logl, *log_prior;               /* n_draws each */
    int32_t *n_uniforms;                    /* n_draws */
    double *uniforms_out;                   /* n_draws x U */
} bild_dwelldraw_out;                       /* every pointer may be NULL: not written */

int bild_gauss_dwell_draw(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                          const double *log_jump, const double *log_dwell, const double *log_surv, int T_max, int64_t scratch_bytes,
                          int64_t n_draws, const int32_t *draw_traj, const int64_t *draw_stream, int U, const double *uniforms,
                          uint64_t seed, bild_dwelldraw_out *out);

/* ---------------------------------------------------------------- evidence sensitivities under a dwell-time prior ----
 * GenericGaussianModel only, at most 4 states.  The gradient of logev of bild_gauss_dwell_evidence (same
 * tables, same NaN flag; the same number, bit for bit: the same forward kernel) with respect to P <= 4 model parameters, for
 * trajectories whose profile is not known.  The prior does not depend on the parameters, so by Fisher's identity the
 * gradient is the posterior mean of the gradient of the log-likelihood.  With the tables of the block before the last,
 *   Q(a, b, s) = exp(alpha(a, s) + omega_s(a, b) + W[s][a - 1][b] + gamma(b, s) - logev)      (a = 0: log_init[s] and F)
 * the posterior probability of the segment [a, b) in state s, alpha(a, s) = log sum_s' exp(A(a, s') + log_jump[s'][s]), and
 *   Omega(s, a, t) = sum_{b > t} Q(a, b, s)
 * the posterior probability that a segment in state s starts at a and has not ended by frame t.  Per trajectory:
 *   logev          as bild_gauss_dwell_evidence gives it
 *   n_nan_windows  as bild_gauss_dwell_evidence gives it
 *   grad           P values: d logev / d theta_p = - sum Omega(s, a, t_j) dtau_p over the entries j of the window that starts
 *                  at a - 1 (the first window for a = 0), tau and dtau those of bild_gauss_logl_sensitivities
 *   exp_logl       - sum Omega tau: the posterior mean of the log-likelihood
 *   fisher         P x P: sum Omega (2 a_p a_q + g_p g_q), the innovations form of bild_gauss_logl_sensitivities,
 *                  posterior-weighted.  This is the posterior mean of the complete-data information: a scoring matrix for a
 *                  fit.  It is NOT the information of the marginal likelihood, which is smaller by the posterior covariance
 *                  of the score; standard errors need the latter.
 * x and the derivatives as for bild_gauss_segment_sensitivities.  flags = 0 (BILD_DWELL_NAN_PROPAGATE): a trajectory with
 * n_nan_windows > 0 has NaN in logev, grad, exp_logl and fisher; the other trajectories are untouched.
 * BILD_DWELL_NAN_OMIT: the skipped windows weigh 0.  A trajectory without a profile of positive weight has logev -inf and
 * NaN in grad, exp_logl and fisher.  NULL outputs are not written.  No atomics, fixed summation orders that depend on the
 * trajectory alone: results are bit-identical across calls, the order of the set, a trajectory alone or in a batch, and
 * scratch_bytes (chunks of whole trajectories, and of factorisations of windows with a missing frame; 0: at most 1 GiB
 * and a third of the free device memory).  tau sums do not depend on P.  Refused before any device work: what
 * bild_gauss_dwell_evidence refuses (there is no T_max here) and what bild_gauss_logl_sensitivities refuses.  Plain
 * launches on the set's stream.  Synchronous. */
typedef struct bild_dwellsens_out {
    double *logev;                          /* n_traj */
    int64_t *n_nan_windows;                 /* n_traj */
    double *grad;                           /* n_traj x P */
    double *exp_logl;                       /* n_traj */
    double *fisher;                         /* n_traj x P x P */
} bild_dwellsens_out;                       /* every pointer may be NULL: not written */

int bild_gauss_dwell_sensitivities(const bild_gauss_model *m, const bild_gauss_trajset *ts, const double *x, int L,
                                   const double *log_init, const double *log_jump, const double *log_dwell,
                                   const double *log_surv, unsigned flags, int P, const bild_gauss_derivs *dm,
                                   int64_t scratch_bytes, bild_dwellsens_out *out);

/* ---------------------------------------------------------------- expected segment lengths under a dwell-time prior ----
 * GenericGaussianModel only, at most 4 states.  The derivatives of logev of bild_gauss_dwell_evidence
 * (same tables, same NaN flag, same refusals) with respect to the prior's own logs: expected counts, the E-step of a fit of
 * the whole dwell-time prior.  With Q(a, b, s) the posterior probability of the segment [a, b) in state s (the block above),
 * per trajectory of T frames:
 *   logev, n_nan_windows, exp_jumps   as bild_gauss_dwell_evidence gives them, bit for bit: the same kernels on the same tables
 *   exp_init       S: I[s] = sum_{b = 1 .. T} Q(0, b, s) = P(theta_0 = s | data)                 (d logev / d log_init[s])
 *   exp_dwell      S x T_max, length l at column l - 1: D[s][l] = sum_{a = 0 .. T - l - 1} Q(a, a + l, s), the expected number
 *                  of completed segments in state s of l frames, l = 1 .. T - 1                  (d logev / d log_dwell[s][l])
 *   exp_cens       S x T_max, length l at column l - 1: C[s][l] = Q(T - l, T, s), the probability that the last, right-censored
 *                  segment is in state s and has l frames, l = 1 .. T                             (d logev / d log_surv[s][l])
 * Columns behind the trajectory's T are 0, and so is exp_dwell at l = T.  Every exponent is clamped at 0, as in the block
 * above; a NaN window, a start that no profile reaches and a tail of weight 0 add nothing.  Sums of non-negative terms:
 * sum_l D[s][l] = sum_s' exp_jumps[s][s'], sum_{s, l} C = 1, sum_l (l - 1) (D + C)[s][l] = exp_stay[s] and
 * sum_{s, l} l (D + C)[s][l] = T up to rounding.  flags = 0 (BILD_DWELL_NAN_PROPAGATE): a trajectory with n_nan_windows > 0
 * has NaN in logev and in every count (columns l <= T).  BILD_DWELL_NAN_OMIT: the skipped windows weigh 0.  A trajectory without
 * a profile of positive weight has logev -inf and NaN in every count.  The start frames a are summed in blocks of 64 frames
 * of the trajectory, ascending inside a block, the blocks in order: no atomics, fixed summation orders that depend on the
 * trajectory alone, so results are bit-identical across calls, the order of the set, a trajectory alone or in a batch, and
 * scratch_bytes (chunks of whole trajectories; 0: at most 1 GiB and a third of the free device memory).  The marginals and
 * the MAP profile of bild_gauss_dwell_evidence are not computed.  Plain launches on the set's stream.  Synchronous. */
typedef struct bild_dwell_lengths_out {
    double *logev;                          /* n_traj */
    int64_t *n_nan_windows;                 /* n_traj */
    double *exp_jumps;                      /* n_traj x S x S */
    double *exp_init;                       /* n_traj x S */
    double *exp_dwell, *exp_cens;           /* n_traj x S x T_max each */
} bild_dwell_lengths_out;                   /* every pointer may be NULL: not written */

int bild_gauss_dwell_lengths(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                             const double *log_jump, const double *log_dwell, const double *log_surv, int T_max, unsigned flags,
                             int64_t scratch_bytes, bild_dwell_lengths_out *out);

/* ---------------------------------------------------------------- exact online filtering under a dwell-time prior ----
 * GenericGaussianModel only, at most 4 states.  The causal answers under the dwell-time prior of
 * bild_gauss_dwell_evidence (same tables, same NaN flag): what that call says about the truncated trajectory x[:t + 1], for
 * every frame t of every trajectory, from one forward pass.  With that block's alpha, for the prefix ends b = t + 1 = 1 .. T:
 *   G(b, s) = log( e^(log_init[s] + log_surv[s][b] + F[s][b]) + sum_{c = 1 .. b - 1} e^(alpha(c, s) + log_surv[s][b - c] + W[s][c - 1][b]) )
 *   E(b)    = log sum_s e^G(b, s)
 * the forward sum at end frame b with the last segment censored.  A window's table entry depends on the data inside the
 * window alone, so the tables of the whole trajectory serve every prefix.  Per trajectory of T frames:
 *   logev          the evidence of the whole trajectory as bild_gauss_dwell_evidence gives it, bit for bit: the same kernel
 *   prefix_logev   T_max: E(t + 1), the evidence of x[:t + 1] under the same tables
 *   log_filtered   S x T_max: G(t + 1, s) - E(t + 1) = log P(theta_t = s | x_0 .. x_t)
 *   run_mean       T_max: the expected length so far of the segment that contains frame t given x_0 .. x_t,
 *                  sum_s sum_c (b - c) term / e^E(b), c = 0 for the first segment: a sum of non-negative terms
 *   log_run        S x T_max x run_max: entry [s][t][r - 1] = log P(theta_t = s, the current segment has lasted r frames |
 *                  x_0 .. x_t), the single term with c = b - r minus E(b), for r = 1 .. min(run_max, b); -inf where that term
 *                  weighs 0 and -inf behind min(run_max, b).  A subtraction of logs: no exp
 *   n_nan_windows  T_max: what bild_gauss_dwell_evidence reports as n_nan_windows of x[:t + 1]; 0 behind T
 * Every other entry behind a trajectory's T is NaN.  prefix_logev[t] - prefix_logev[t - 1] is log p(x_t | x_0 .. x_{t-1}) only
 * where the tables are consistent under truncation: log_surv[s][l] = log sum_{l' >= l} exp(log_dwell[s][l']) and normalised
 * jumps; otherwise it is a difference of two evidences and no more.
 * NaN windows: the kernel counts per end frame b the skipped windows [c, b) whose start is reachable (alphaArg >= 0; c = 0:
 * log_init finite) under their log_surv weight, nG(b), and under their log_dwell weight, nA(b);
 * n_nan_windows[t] = nG(t + 1) + sum_{e <= t} nA(e).  flags = 0 (BILD_DWELL_NAN_PROPAGATE): every output at a frame t with
 * n_nan_windows[t] > 0 is NaN, earlier frames are untouched; logev follows bild_gauss_dwell_evidence.  BILD_DWELL_NAN_OMIT:
 * the skipped windows weigh 0.  A prefix without a profile of positive weight has prefix_logev -inf and NaN in log_filtered,
 * run_mean and the whole row of log_run at that frame.  The switches c are summed by eight waves, wave q taking c = 1 + q,
 * 9 + q, .. in ascending order, the waves merged in wave order: no atomics, fixed summation orders that depend on the
 * trajectory alone, so results are bit-identical across calls, the order of the set, a trajectory alone or in a batch,
 * scratch_bytes (chunks of whole trajectories; 0: at most 1 GiB and a third of the free device memory) and whether log_run is
 * asked for.  Refused before any device work: what bild_gauss_dwell_evidence refuses, run_max < 0, and log_run given with
 * run_max = 0 (BILD_ERR_INVALID).  log_run == NULL: run_max is not used.  Plain launches on the set's stream.  Synchronous. */
typedef struct bild_dwell_filter_out {
    double *logev;                          /* n_traj */
    double *prefix_logev;                   /* n_traj x T_max */
    double *log_filtered;                   /* n_traj x S x T_max */
    double *run_mean;                       /* n_traj x T_max */
    double *log_run;                        /* n_traj x S x T_max x run_max */
    int64_t *n_nan_windows;                 /* n_traj x T_max */
} bild_dwell_filter_out;                    /* every pointer may be NULL: not written */

int bild_gauss_dwell_filter(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                            const double *log_jump, const double *log_dwell, const double *log_surv, int T_max, int run_max,
                            unsigned flags, int64_t scratch_bytes, bild_dwell_filter_out *out);

/* ---------------------------------------------------------------- exact fixed-lag smoothing under a dwell-time prior ----
 * GenericGaussianModel only, at most 4 states.  Between the filter above and the smoothed marginals of
 * bild_gauss_dwell_evidence (same tables, same NaN flag): log P(theta_t = s | x_0 .. x_{t + l}) for every frame t and every
 * l = 0 .. lag, what bild_gauss_dwell_evidence says about frame t of the truncated trajectory x[:u], u = min(t + l + 1, T).  With
 * that block's alpha, head(0, s) = log_init[s], w(0, b, s) = F[s][b], head(a, s) = alpha(a, s), w(a, b, s) = W[s][a - 1][b] for
 * a >= 1, and omega_u(a, b, s) = log_dwell[s][b - a] for b < u, log_surv[s][u - a] for b = u:
 *   gamma_u(u, s) = 0,  beta_u(a, s) = log sum_{a < b <= u} e^(omega_u(a, b, s) + W[s][a - 1][b] + gamma_u(b, s)),
 *   gamma_u(a, s) = log sum_s'' e^(log_jump[s][s''] + beta_u(a, s''))
 *   J_u(t, s)     = log sum_{a <= t < b <= u} e^(head(a, s) + omega_u(a, b, s) + w(a, b, s) + gamma_u(b, s))
 *   E(u)          = log sum_s e^J_u(u - 1, s)        (the filter's E(u))
 * A window's table entry depends on the data inside the window alone, so the tables of the whole trajectory serve every cut u.
 * Per trajectory of T frames:
 *   logev          the evidence of the whole trajectory as bild_gauss_dwell_evidence gives it, bit for bit: the same kernel
 *   log_lagged     S x T_max x (lag + 1): entry [s][t][l] = J_u(t, s) - E(u).  Column 0 is the filtered marginal; where
 *                  t + l + 1 >= T the cut is the whole trajectory and the entry is the smoothed marginal, so the last columns of
 *                  the last frames repeat; with lag >= T - 1 column lag is the smoothed marginal at every frame.  -inf where
 *                  the probability is 0
 *   n_nan_windows  T_max: what bild_gauss_dwell_evidence reports as n_nan_windows of x[:t + 1], as bild_gauss_dwell_filter
 *                  gives it; 0 behind T
 * log_lagged behind a trajectory's T is NaN.  A NaN window enters no sum.  flags = 0 (BILD_DWELL_NAN_PROPAGATE): entry
 * [.][t][l] is NaN exactly where n_nan_windows[u - 1] > 0 for its cut u; logev follows bild_gauss_dwell_evidence.
 * BILD_DWELL_NAN_OMIT: the skipped windows weigh 0.  A cut without a profile of positive weight (E(u) = -inf) has NaN in all its
 * entries.  The starts a of every sum are split at the left edge of the window: the starts a <= b - 1 - lag of an end frame b
 * are summed once for all cuts, by eight waves (wave q: a = 1 + q, 9 + q, .. ascending, wave 0 the first segment before them)
 * merged in wave order; the starts inside the window ascending, and the ends b of a cut by butterflies over one wavefront.  No
 * atomics, fixed summation orders that depend on the trajectory and on lag alone, so results are bit-identical across calls,
 * the order of the set, a trajectory alone or in a batch and scratch_bytes (chunks of whole trajectories; 0: at most 1 GiB and
 * a third of the free device memory); a different lag moves the split, and a column then agrees with the same column under
 * another lag to rounding only.  The terms number O(S T^2) + O(S T lag^2).  Refused before any device work: what
 * bild_gauss_dwell_evidence refuses, lag < 0 (BILD_ERR_INVALID) and lag > BILD_DWELL_LAG_MAX = 63 (BILD_ERR_UNSUPPORTED: a window
 * of lag + 1 frames is one wavefront).  Plain launches on the set's stream.  Synchronous. */
#define BILD_DWELL_LAG_MAX 63
typedef struct bild_dwell_lag_out {
    double *logev;                          /* n_traj: bild_gauss_dwell_evidence's number, bit for bit */
    double *log_lagged;                     /* n_traj x S x T_max x (lag + 1) */
    int64_t *n_nan_windows;                 /* n_traj x T_max */
} bild_dwell_lag_out;                       /* every pointer may be NULL: not written */

int bild_gauss_dwell_lag(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                         const double *log_jump, const double *log_dwell, const double *log_surv, int T_max, int lag,
                         unsigned flags, int64_t scratch_bytes, bild_dwell_lag_out *out);

/* ---------------------------------------------------------------- switch counts under a dwell-time prior ----
 * GenericGaussianModel only, at most 4 states.  The exact posterior distribution of the number K of
 * switches of the profile, jointly with its last state, under the dwell-time prior of bild_gauss_dwell_evidence (same tables,
 * same NaN flag): that block's forward recursion resolved by the number of switches.  For n = 0 .. k_max:
 *   A_0(b, s)     = log_init[s] + omega_s(0, b) + F[s][b]
 *   A_n(b, s)     = log sum_{c = n .. b - 1} exp(alpha_{n-1}(c, s) + omega_s(c, b) + W[s][c - 1][b])        (n >= 1, n < b <= T)
 *   alpha_n(c, s) = log sum_s' exp(A_n(c, s') + log_jump[s'][s])                                         (1 <= c < T)
 * Level n reads level n - 1 alone: one launch per level, two rows of alpha in memory, O(S T) per trajectory beside the
 * output column.  Per trajectory of T frames:
 *   logev, n_nan_windows   as bild_gauss_dwell_evidence gives them, bit for bit: the same forward kernel on the same tables
 *   log_count      (k_max + 1) x S: entry [n][s] = A_n(T, s) - logev = log P(K = n, theta_{T-1} = s | x); -inf where the
 *                  probability is 0, and -inf for n > T - 1
 *   log_tail       log(max(0, 1 - sum_{n, s} exp(log_count[n][s]))), the sum over n ascending and s ascending inside: the
 *                  probability of more than k_max switches.  A DIFFERENCE from 1: accurate to an absolute 1e-15 or so of the
 *                  probability, not relatively, and 0 (-inf) or a few 1e-16 where the true tail is below that.  -inf exactly
 *                  when k_max >= T - 1
 * A NaN window enters no sum.  flags = 0 (BILD_DWELL_NAN_PROPAGATE): a trajectory with n_nan_windows > 0 has NaN in logev,
 * log_count and log_tail; the other trajectories are untouched.  BILD_DWELL_NAN_OMIT: the skipped windows weigh 0.  A
 * trajectory without a profile of positive weight has logev -inf and NaN in log_count and log_tail.  sum_n exp(log_count)
 * is 1 at k_max >= T - 1 up to rounding only: logev is the forward pass's number, not the sum of the levels.  The switches c
 * of a level are summed by eight waves, wave q taking c = n + q, n + q + 8, .. in ascending order, the waves merged in wave
 * order: no atomics, fixed summation orders that depend on the trajectory alone, so results are bit-identical across calls,
 * the order of the set, a trajectory alone or in a batch, scratch_bytes (chunks of whole trajectories; 0: at most 1 GiB and a
 * third of the free device memory), and k_max: the levels n <= k_max of a call are those of every call with a larger k_max.
 * Refused before any device work: what bild_gauss_dwell_evidence refuses, k_max < 0 and k_max > max(T_max, 1) - 1
 * (BILD_ERR_INVALID).  Plain launches on the set's stream.  Synchronous. */
typedef struct bild_dwell_switch_counts_out {
    double *logev;                          /* n_traj */
    int64_t *n_nan_windows;                 /* n_traj */
    double *log_count;                      /* n_traj x (k_max + 1) x S */
    double *log_tail;                       /* n_traj */
} bild_dwell_switch_counts_out;             /* every pointer may be NULL: not written */

int bild_gauss_dwell_switch_counts(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                   const double *log_jump, const double *log_dwell, const double *log_surv, int T_max, int k_max,
                                   unsigned flags, int64_t scratch_bytes, bild_dwell_switch_counts_out *out);

/* ---------------------------------------------------------------- first-contact times under a dwell-time prior ----
 * GenericGaussianModel only, at most 4 states.  The exact posterior distribution of the first frame at
 * which the profile is in a state of the set G (bit s of target: state s belongs to G), and the probability that it never
 * is, under the dwell-time prior of bild_gauss_dwell_evidence (same tables, same NaN flag).  With Ax the table A of that
 * block's forward pass under the prior with log_init[s] = -inf and log_jump[.][s] = -inf for s in G (the profiles that avoid G;
 * the same forward kernel on a second prior block) and beta, gamma of the full prior:
 *   h(s)     = log sum_{b = 1 .. T} exp(omega_s(0, b) + F[s][b] + gamma(b, s))
 *   first(0) = log sum_{s in G} exp(log_init[s] + h(s)) - logev
 *   first(t) = log sum_{s' not in G} sum_{s in G} exp(Ax(t, s') + log_jump[s'][s] + beta(t, s)) - logev        (1 <= t < T)
 *   never    = log sum_{s' not in G} exp(Ax(T, s')) - logev
 * Per trajectory of T frames:
 *   logev, n_nan_windows   as bild_gauss_dwell_evidence gives them, bit for bit: the same forward kernel on the same tables
 *   log_first      T_max: first(t), -inf where the probability is 0; NaN behind T
 *   log_never      never
 * Every term is normalised by logev of the full forward pass, not by their sum: sum_t exp(log_first[t]) + exp(log_never) = 1
 * holds up to rounding and is a check, not a construction.  A NaN window enters no sum.  flags = 0
 * (BILD_DWELL_NAN_PROPAGATE): a trajectory with n_nan_windows > 0 (of the full pass) has NaN in logev, log_first and
 * log_never; the other trajectories are untouched.  BILD_DWELL_NAN_OMIT: the skipped windows weigh 0.  A trajectory without a
 * profile of positive weight has logev -inf and NaN in log_first and log_never.  h(s) is summed by one wavefront, lane l
 * taking b = 1 + l, 65 + l, .. ascending, merged by butterflies; first(t) over s' ascending and s ascending inside: no
 * atomics, fixed summation orders that depend on the trajectory alone, so results are bit-identical across calls, the order
 * of the set, a trajectory alone or in a batch, and scratch_bytes (chunks of whole trajectories, which hold the forward tables
 * twice; 0: at most 1 GiB and a third of the free device memory).  Refused before any device work: what
 * bild_gauss_dwell_evidence refuses, and a target that is empty, names a state the model does not have or holds every state
 * (BILD_ERR_INVALID): a model of one state is always refused.  Plain launches on the set's stream.  Synchronous. */
typedef struct bild_dwell_first_contact_out {
    double *logev;                          /* n_traj */
    int64_t *n_nan_windows;                 /* n_traj */
    double *log_first;                      /* n_traj x T_max */
    double *log_never;                      /* n_traj */
} bild_dwell_first_contact_out;             /* every pointer may be NULL: not written */

int bild_gauss_dwell_first_contact(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                   const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                                   unsigned target, unsigned flags, int64_t scratch_bytes, bild_dwell_first_contact_out *out);

/* ---------------------------------------------------------------- looped time under a dwell-time prior ----
 * GenericGaussianModel only, at most 4 states.  The exact posterior distribution of the number N of
 * frames t with theta_t in the set G (bit s of target: state s belongs to G), jointly with the last state, under the
 * dwell-time prior of bild_gauss_dwell_evidence (same tables, same NaN flag).  Every frame counts, observed or missing.  That
 * block's forward recursion resolved by n, with g_s = 1 for s in G and 0 otherwise:
 *   A(b, s, n)     = [n = g_s b] (log_init[s] + omega_s(0, b) + F[s][b])
 *                    (+) log sum_{c = 1 .. b - 1} exp(alpha(c, s, n - g_s (b - c)) + omega_s(c, b) + W[s][c - 1][b])
 *   alpha(c, s, n) = log sum_s' exp(A(c, s', n) + log_jump[s'][s])                                  (1 <= c < T, 0 <= n <= c)
 * A segment outside G keeps n, a segment inside G adds its length; alpha(c, ., n) is empty outside 0 <= n <= c.  The shifted
 * index couples every n of every earlier c: one launch per end frame b, alpha kept for every c, S T_longest (T_longest + 1)
 * doubles per trajectory of a chunk beside the forward tables (16 MB at T = 1000 and 2 states).  Per trajectory of T frames:
 *   logev, n_nan_windows   as bild_gauss_dwell_evidence gives them, bit for bit: the same forward kernel on the same tables
 *   log_occ        (T_max + 1) x S: entry [n][s] = A(T, s, n) - logev = log P(N = n, theta_{T-1} = s | x); -inf where the
 *                  probability is 0, and -inf for n > T
 * Every entry is normalised by logev of the ordinary forward pass, not by their sum: sum exp(log_occ) = 1 holds up to rounding
 * and is a check, not a construction.  A NaN window enters no sum.  flags = 0 (BILD_DWELL_NAN_PROPAGATE): a trajectory with
 * n_nan_windows > 0 has NaN in logev and log_occ; the other trajectories are untouched.  BILD_DWELL_NAN_OMIT: the skipped
 * windows weigh 0.  A trajectory without a profile of positive weight has logev -inf and NaN in log_occ.  The switch frames c
 * of an entry are summed by eight waves, wave q taking c = c0 + q, c0 + q + 8, .. in ascending order from the first c0 that can
 * reach the entry's tile of 64 values of n, the waves merged in wave order: no atomics, fixed summation orders that depend on
 * the trajectory alone, so results are bit-identical across calls, the order of the set, a trajectory alone or in a batch, and
 * scratch_bytes (chunks of whole trajectories; 0: at most 1 GiB and a third of the free device memory).  Refused before any
 * device work: what bild_gauss_dwell_evidence refuses, and a target that is empty, names a state the model does not have or
 * holds every state (BILD_ERR_INVALID): a model of one state is always refused.  Plain launches on the set's stream.
 * Synchronous. */
typedef struct bild_dwell_occupancy_out {
    double *logev;                          /* n_traj */
    int64_t *n_nan_windows;                 /* n_traj */
    double *log_occ;                        /* n_traj x (T_max + 1) x S */
} bild_dwell_occupancy_out;                 /* every pointer may be NULL: not written */

int bild_gauss_dwell_occupancy(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                               const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                               unsigned target, unsigned flags, int64_t scratch_bytes, bild_dwell_occupancy_out *out);

#ifdef __cplusplus
}
#endif
#endif /* BILD_AMD_H */
