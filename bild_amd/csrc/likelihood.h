// What the units of the likelihood library share (model.cpp, tables.cpp, launch.cpp, api.cpp): the objects behind the
// C ABI's model and trajectory-set handles, error reporting, and the entry points between the units.  Private: the units
// all work in namespace bild, and so does this header.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bild_amd.h"
#include "common.h"
#include "config.h"
#include "host_linalg.h"

using namespace bild;
using la::Mat;

namespace bild {

// errors: sets the message bild_last_error returns (printf format) and returns `code`
int fail(int code, const char *fmt, ...);

#define HIP_TRY(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? BILD_ERR_NO_DEVICE \
                                                                              : BILD_ERR_HIP,      \
                        "%s failed: %s", #call, hipGetErrorString(e_));                            \
    } while (0)

// return on a code that is not BILD_OK
#define BILD_TRY(x)                     \
    do {                                \
        int rc_ = (x);                  \
        if (rc_ != BILD_OK) return rc_; \
    } while (0)

// A buffer that grows by a quarter beyond what is asked: device memory, or (Pinned) page-locked host staging -- copies to
// and from that are true asynchronous DMA transfers
template <bool Pinned> struct GrowBuf {
    void *ptr = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return BILD_OK;
        release();
        size_t want = bytes + bytes / 4 + (Pinned ? 4096 : 256);
        hipError_t e = Pinned ? hipHostMalloc(&ptr, want, hipHostMallocDefault) : hipMalloc(&ptr, want);
        if (e != hipSuccess) {
            ptr = nullptr;
            return fail(BILD_ERR_NOMEM, "%s(%zu) failed: %s", Pinned ? "hipHostMalloc" : "hipMalloc", want, hipGetErrorString(e));
        }
        cap = want;
        return BILD_OK;
    }
    void release()
    {
        if (ptr) (void)(Pinned ? hipHostFree(ptr) : hipFree(ptr));
        ptr = nullptr;
        cap = 0;
    }
};
using DeviceBuf = GrowBuf<false>;
using PinnedBuf = GrowBuf<true>;

} // namespace bild

// ---- the objects behind the handles ------------------------------------------------------
struct bild_model {
    int N = 0, d = 0, S = 0;
    unsigned flags = 0;
    // inputs as given
    Mat B, G, Sig, M0, C0, w;
    // invariant-subspace reduction: V is N x n (columns orthonormal); r* are the projected arrays
    int n = 0;
    Mat V;
    Mat rB, rG, rSig, rM0, rC0, rw;
    bool has_G = false;
    // modal analysis (in reduced coordinates)
    bool modal_ok = false;
    std::string modal_why;
    Mat lam, sigd, Q, wq, R, C0q, M0q, Gq; // S*n, S*n, S*n*n, S*n, S*S*n*n, S*n*n, S*n*d, S*n*d
    // packed for the kernels
    int NP = 0; // padded row count of the modal packing; the launch geometry is chosen per batch (geometry_for)
    int NPm[2] = {0, 0}; // padded row count per path (kDense, kModal): the dense packing is rounded up to whole 4x4 tiles
                         // where the matrix-pipe kernel applies (dense_mfma.hip)
    bool wide = false; // NP > kMidMaxNP: LDS-resident kernel (wide.hip), modal path only
    bool mid = false;  // kMaxNP < NP <= kMidMaxNP: tile-register kernel (modal_mfma.hip), modal path only
    bool symmetric = true; // B, Sig, C0 symmetric (what the reference's dsymv calls assume)
    bool tab_factored = false; // modal table of the vector kernels holds Q[s], Q[s]^T instead of all pairs R[s2][s]
    Mat blob_states[2], blob_tab[2];
    // device residency
    mutable std::mutex mu;      // device residency and workspace growth
    mutable std::mutex call_mu; // host-buffer evaluations share one workspace: one at a time per model
    mutable int device = -1;
    mutable double *d_states[2] = {nullptr, nullptr};
    mutable double *d_tab[2] = {nullptr, nullptr};
    // host-buffer entry points (one call at a time per model, call_mu): ONE packed device buffer
    // [seg_start | seg_state | traj_id] filled by one copy out of pinned staging, results back through
    // pinned staging, all on the model's own stream
    mutable DeviceBuf ws_in, ws_out, ws_sched; // ws_sched: workspace of the device-side launch order (schedule.hip)
    mutable PinnedBuf h_in, h_out;
    mutable hipStream_t stream = nullptr;
    mutable unsigned long long *d_frames = nullptr; // frames the tasks ran themselves, summed while kernel timing is on
    mutable hipEvent_t h_in_event = nullptr; // behind the last kernel of a call that left its results on the device (nobody waited)
    mutable bool h_in_busy = false;
    // work lists of split launches (walk.hip): [two sets of kWorkBuckets counters, padded to 128 bytes] [kWorkBuckets lists].
    // Launches alternate between the two sets, and the walk kernel of a launch zeroes the OTHER set -- last touched by the
    // launch before, which has finished -- for the launch after: no launch of its own is needed to zero sixteen integers.
    // The block serves every launch on the stream that used it first (launches on one stream run one after another);
    // launches on other streams get a stream-ordered allocation of their own.
    // Two such blocks: the first for the model's own stream (host-buffer calls), the second for the first other stream that
    // launches on the model (a caller's stream: bench.py, dist.ShardedModel); launches on further streams allocate.
    struct WorkSlot {
        DeviceBuf ws_work;
        DeviceBuf ws_lists; // same rule: segment lists the walk kernel writes for the frame loop ((s, theta) input resident in HBM)
        hipStream_t stream = nullptr;
        bool taken = false;
        int work_set = 0;
        // held from the flip of `work_set` until BOTH kernels of the launch are enqueued: two threads launching on one
        // (model, stream) must enqueue in the order in which they flipped, or a walk would count into a set the frame loop of
        // the launch in front of it still reads
        std::mutex launch_mu;
    };
    mutable WorkSlot slots[2];
    // the block of stream `st`, or null (caller holds `mu`)
    WorkSlot *slot_for(hipStream_t st) const
    {
        if (st == stream && stream != nullptr) {
            slots[0].stream = st;
            slots[0].taken = true;
            return &slots[0];
        }
        if (!slots[1].taken) {
            slots[1].stream = st;
            slots[1].taken = true;
        }
        return slots[1].stream == st ? &slots[1] : nullptr;
    }
    mutable PinnedBuf h_status; // (s, theta) rows refused on the device by calls nobody waited for: sticky until bild_logl_st_status
    // id of the vector geometry whose frame loop the last evaluating launch ran (BILD_Q_LAST_GEOMETRY); -1: another kernel family,
    // or a split launch whose table walk finished the batch.  Table builders leave it alone.
    mutable std::atomic<int> last_geom{-1};
};

struct bild_trajset {
    const bild_model *model = nullptr;
    int n_traj = 0;
    int d = 0;
    std::vector<TrajDesc> descs; // host copy; .x are device pointers
    int dstar_max = 1;
    int means_max = 1; // most dimensions any covariance chain carries
    int Tmax = 0;
    bool all_valid = true;
    int device = -1;
    double *d_x = nullptr; // all trajectories, each followed by kPadRows padding rows, then kZeroPad zeros
    double *d_zeros = nullptr;
    TrajDesc *d_descs = nullptr;
    // prefix table of the vector kernels' modal path (common.h: prefix_record_doubles), built at the first evaluation
    // that can use it: 0 not tried yet, 1 built, -1 not available for this set (too large, or the build failed)
    mutable std::mutex prefix_mu;
    mutable std::atomic<int> prefix_state{0};
    mutable double *d_prefix = nullptr;
    mutable double *d_tail_g = nullptr;   // first-order tails (tail.hip): kDMax x NP doubles per prefix record
    mutable double *d_prefix_L = nullptr; // running log-likelihood of every record, densely (walk.hip reads nothing else)
    mutable int64_t prefix_records = 0;
    mutable double prefix_build_ms = 0.0;
    // transient table (common.h: TransEntry), built right behind the prefix table: 0 not tried, 1 built, -1 none
    mutable std::atomic<int> trans_state{0};
    mutable TransEntry *d_trans = nullptr;
    mutable int64_t trans_entries = 0;
    mutable double trans_build_ms = 0.0;
    mutable std::atomic<int> trans2_state{0}; // pair table (two switches as one transient): 0 not tried, 1 built, -1 not available
    mutable TransEntry *d_trans2 = nullptr;
    mutable int64_t trans2_entries = 0;
    mutable double trans2_build_ms = 0.0;
    mutable int gap_max = 0;              // gaps 1 .. gap_max - 1 are in the pair table
    // the caller's declaration of how many evaluations the set will see (bild_trajset_expect; < 0: none given): which tables
    // are worth their build -- a property of the set and of that declaration, never of the call history
    mutable std::atomic<int64_t> expected_evals{-1};
    mutable double *d_strans = nullptr;   // transient state table (common.h), filled by the launch that builds the transient table
    mutable int64_t strans_records = 0;   // records of the state table as built: strans_entries * sgap
    mutable int64_t strans_entries = 0;   // (trajectory, chain, old state, new state, frame) combinations
    mutable int sgap = kStateGap;         // gaps 1 .. sgap - 1 behind a switch are covered (sized when the table is built) ...
    mutable int sstride = kStateStride, snq = 0; // ... by snq records per entry, one for every sstride-th gap
    mutable double *d_pstrans = nullptr;  // pair state table (common.h), filled by the launch that builds the pair table
    mutable int64_t pstrans_records = 0;  // records of the pair state table as built: prefix_records (S - 1)^2 (gap_max - 1) pnq
    mutable int pgap = 0, pstride = kPairStateStride, pnq = 0; // gaps 1 .. pgap - 1 behind the second switch, every pstride-th
    // switch tails (tail.hip; KParams::stail), built behind the pair table: 0 not tried, 1 built, -1 none
    mutable std::atomic<int> stail_state{0};
    mutable double *d_stail = nullptr;
    mutable int stail_J = 0;
    mutable int64_t stail_bytes = 0;
    mutable double stail_build_ms = 0.0;
    mutable int trans_m_max = 0;          // longest converged transient of the single table
    mutable int two_switch_covered = 0;  // every candidate of <= 2 switches comes out of the tables (checked on the device when the pair table is built)
    mutable int trans_m_typ = 48;         // typical frames-to-convergence of the table's entries (90th percentile): the scheduler's yardstick
};

namespace bild {

// ---- model.cpp -----------------------------------------------------------------------
// device copies of the model's tables, its stream and counters, made on first use
int ensure_device(const bild_model &m);
// the path (kDense / kModal) the flags ask for
int pick_mode(const bild_model &m, unsigned flags, int *mode);
// the launch parameters that depend on the model, the set and the path alone
int fill_params(const bild_model &m, const bild_trajset &ts, int mode, KParams &p);
// LDS of one workgroup of the vector kernels: the model's tables and the product images of its groups
size_t lds_bytes(const bild_model &m, const Geometry &geom, int mode);

// ---- tables.cpp ----------------------------------------------------------------------
// The tables of a trajectory set, each tried once (at the first evaluation that can use it) and synchronous.  A table that
// cannot be built is an optimisation not made: these return BILD_OK whatever happens.
int ensure_prefix(const bild_model &m, const bild_trajset &ts, hipStream_t st);
int ensure_transients(const bild_model &m, const bild_trajset &ts, hipStream_t st);
int ensure_pairs(const bild_model &m, const bild_trajset &ts, hipStream_t st);
int ensure_switch_tails(const bild_model &m, const bild_trajset &ts, hipStream_t st);

// ---- launch.cpp ----------------------------------------------------------------------
// What a launch may be given beyond the segment lists (all device-visible, all optional)
struct LaunchIn {
    // the sampler's own (s, theta) instead of segment lists (bild/amis.py:717-739): the walk kernel converts them on
    // the device and writes the lists the frame loop needs into d_seg_start / d_seg_state of the call (then WRITABLE)
    const double *d_ss = nullptr;
    const int8_t *d_thetas = nullptr;
    int32_t *status = nullptr;   // [0] != 0: a row was not a point on the simplex, [1]: such a row
    // set by ensure_transients / ensure_pairs alone: this launch FILLS a table (kFillTransients: ts.d_trans and ts.d_strans,
    // kFillPairs: ts.d_trans2 and ts.d_pstrans) instead of reading it -- an argument of this internal call, so that no ABI caller can ask for it
    enum Fill { kFillNone, kFillTransients, kFillPairs } fill = kFillNone;
};
int launch_batch(const bild_model &m, const bild_trajset &ts, int64_t n, int K1, const int32_t *d_seg_start,
                 const int32_t *d_seg_state, const int32_t *d_traj_id, const int32_t *d_order, unsigned flags,
                 hipStream_t st, double *d_out, const LaunchIn &in = LaunchIn());
// split launches (table walk + frame loop over the work lists) are possible for this many segments per candidate
constexpr int kSplitMaxK1 = kSegLds;
bool schedule(const bild_model &m, const bild_trajset &ts, int64_t n, int K1, const int32_t *seg_start, const int32_t *seg_state,
              const int32_t *traj_id, unsigned flags, int32_t *order, bool inside_a_call);
int device_order(const bild_model &m, const bild_trajset &ts, int64_t n, int K1, const int32_t *d_start, const int32_t *d_tid,
                 unsigned flags, hipStream_t st, const int32_t **d_order);

} // namespace bild
