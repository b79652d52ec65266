// C ABI of bild_amd (include/bild_amd.h): argument checks, the host-buffer calls (staging through pinned memory) and the
// device-buffer calls of the likelihood.  The model, the tables of a trajectory set and the launches are model.cpp,
// tables.cpp and launch.cpp.
#include <climits>
#include <emmintrin.h>
#include <cstdarg>
#include <chrono>

#include "internal.h"
#include "likelihood.h"

static thread_local std::string g_err; // bild_last_error

int bild::fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {

// Host buffers in, host buffer out.  `fill(h_start, h_state)` writes the n x K1 run-length segments straight into
// pinned staging memory (and validates them: these indices drive device addressing); then ONE host-to-device copy of
// the packed block [seg_start | seg_state | traj_id], the launch, one device-to-host copy of the results, one
// synchronisation -- all on the model's own stream.
// BILD_TRACE_STAGED=1: print where a host-buffer call spends its time (microseconds), every 64th call
struct StageClock {
    bool on;
    std::chrono::steady_clock::time_point t0;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    StageClock() : on(config().trace_staged), t0(std::chrono::steady_clock::now()) {}
    void lap(int i)
    {
        if (!on) return;
        auto t1 = std::chrono::steady_clock::now();
        acc[i] += std::chrono::duration<double, std::micro>(t1 - t0).count();
        t0 = t1;
    }
};

// Device block of a host-buffer call (ws_in), filled by ONE copy out of the pinned block of the same layout:
//   [ header: reserved, zero ]                                                               kStagedHeader bytes
//   [ payload: segment lists (seg_start | seg_state), or (s, theta) rows (ss float64 | thetas uint8, padded to 8 bytes) ]
//   [ traj_id (n int32), when given ] [ launch order (n int32), when the host scheduled ]
// and behind what is copied, device only:
//   [ (s, theta) input: the segment lists the walk kernel writes for the frame loop: seg_start | seg_state ]
constexpr size_t kStagedHeader = 128;

template <typename Fill>
int run_staged(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *traj_id, unsigned flags,
               double *out, double *d_out_user, hipStream_t st_user, bool st_payload, Fill &&fill)
{
    int rc;
    if (traj_id)
        for (int64_t r = 0; r < n; ++r)
            if (traj_id[r] < 0 || traj_id[r] >= ts->n_traj)
                return fail(BILD_ERR_INVALID, "traj_id[%lld]=%d out of range", (long long)r, traj_id[r]);
    std::lock_guard<std::mutex> call_lock(m->call_mu);
    const size_t nseg = (size_t)n * K1;
    const size_t payload = st_payload ? nseg * sizeof(double) + ((nseg + 7) & ~(size_t)7) : 2 * nseg * sizeof(int32_t);
    const size_t copy_cap = kStagedHeader + payload + 2 * (size_t)n * sizeof(int32_t); // room for traj_id and the launch order
    const size_t lists = st_payload ? 2 * nseg * sizeof(int32_t) : 0;
    // A previous call that left its results on the device (bild_logl_st_to_device: nothing waited for) may still be
    // running: its kernels read the device block and the work lists, its copy reads the pinned block.  The event was
    // recorded behind its last kernel.
    if (m->h_in_busy) HIP_TRY(hipEventSynchronize(m->h_in_event));
    m->h_in_busy = false;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        if ((rc = m->h_in.reserve(copy_cap))) return rc;
        if ((rc = m->ws_in.reserve(copy_cap + lists))) return rc;
        if ((rc = m->h_out.reserve((size_t)n * sizeof(double) + 64))) return rc; // (+ the status word of (s, theta) input)
        if (!d_out_user && (rc = m->ws_out.reserve((size_t)n * sizeof(double)))) return rc;
    }
    StageClock clk;
    char *h_base = (char *)m->h_in.ptr, *d_base = (char *)m->ws_in.ptr;
    std::memset(h_base, 0, kStagedHeader);
    int32_t *h_tid = (int32_t *)(h_base + kStagedHeader + payload);
    int32_t *h_order = h_tid + (traj_id ? n : 0);
    if ((rc = fill(h_base + kStagedHeader))) return rc;
    if (traj_id) std::memcpy(h_tid, traj_id, (size_t)n * sizeof(int32_t));
    clk.lap(0);
    // the host scheduler serves launches that will NOT be split (no tables, BILD_NO_JUMP, ...): see schedule()
    const bool ordered = !st_payload && schedule(*m, *ts, n, K1, (const int32_t *)(h_base + kStagedHeader),
                                                 (const int32_t *)(h_base + kStagedHeader) + nseg, traj_id, flags, h_order, true);
    clk.lap(1);
    const size_t in_bytes = kStagedHeader + payload + ((traj_id ? (size_t)n : 0) + (ordered ? (size_t)n : 0)) * sizeof(int32_t);
    int32_t *d_tid = traj_id ? (int32_t *)(d_base + kStagedHeader + payload) : nullptr;
    const int32_t *d_order = ordered ? (int32_t *)(d_base + kStagedHeader + payload) + (traj_id ? n : 0) : nullptr;
    int32_t *d_start, *d_state;
    LaunchIn in;
    // the status word lives in pinned host memory the device writes to directly: the host reads it after its synchronisation
    int32_t *h_status = (int32_t *)((char *)m->h_out.ptr + (size_t)n * sizeof(double));
    // Batches of up to 50 000 rows on one trajectory: the walk kernel reads the (s, theta) rows straight out of the pinned
    // block over PCIe (450 KB for the 10k batch) -- no host-to-device copy to enqueue and wait for: 136 -> 130 us per call.
    // BILD_IN_VIA_COPY=1: always through a copy in HBM.
    const bool in_copy = config().in_via_copy;
    const bool direct_in = !in_copy && st_payload && !traj_id && n <= 50000;
    if (st_payload) {
        d_start = (int32_t *)(d_base + copy_cap);
        d_state = d_start + nseg;
        const char *in_base = direct_in ? h_base : d_base;
        in.d_ss = (const double *)(in_base + kStagedHeader);
        in.d_thetas = (const int8_t *)(in_base + kStagedHeader + nseg * sizeof(double));
        if (d_out_user) { // nobody waits: the verdict stays with the model until bild_logl_st_status asks
            if (!m->h_status.ptr) {
                std::lock_guard<std::mutex> lk(m->mu);
                if ((rc = m->h_status.reserve(64))) return rc;
                std::memset(m->h_status.ptr, 0, 64);
            }
            h_status = (int32_t *)m->h_status.ptr;
        } else {
            h_status[0] = h_status[1] = 0;
        }
        in.status = h_status;
    } else {
        d_start = (int32_t *)(d_base + kStagedHeader);
        d_state = d_start + nseg;
    }
    // Results of a host-buffer call: the kernels write them straight into the pinned block (80 KB of posted writes over
    // PCIe for the 10k batch) -- no device-to-host copy to launch and wait for.  BILD_OUT_VIA_COPY=1: through HBM and a copy.
    const bool out_via_copy = config().out_via_copy;
    double *d_out = d_out_user ? d_out_user : (out_via_copy ? (double *)m->ws_out.ptr : (double *)m->h_out.ptr);
    hipStream_t st = d_out_user ? st_user : m->stream;
    if (!direct_in) HIP_TRY(hipMemcpyAsync(d_base, h_base, in_bytes, hipMemcpyHostToDevice, st));
    if (!ordered && !st_payload) {
        const int32_t *on_device = nullptr;
        if (device_order(*m, *ts, n, K1, d_start, d_tid, flags, st, &on_device) == 0) d_order = on_device;
    }
    rc = launch_batch(*m, *ts, n, K1, d_start, d_state, d_tid, d_order, flags, st, d_out, in);
    if (rc) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    if (d_out_user) {
        // results stay in HBM, ordered on the caller's stream; the event covers everything this call reads
        HIP_TRY(hipEventRecord(m->h_in_event, st));
        m->h_in_busy = true;
        return BILD_OK;
    }
    clk.lap(2);
    if (out_via_copy) HIP_TRY(hipMemcpyAsync(m->h_out.ptr, d_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    clk.lap(3);
    if (st_payload && h_status[0] != 0)
        return fail(BILD_ERR_INVALID, "interval lengths of sample %d are not non-negative finite numbers (of a point on the simplex)", h_status[1]);
    std::memcpy(out, m->h_out.ptr, (size_t)n * sizeof(double));
    clk.lap(4);
    if (clk.on) {
        static int calls = 0;
        if ((calls++ & 63) == 0)
            fprintf(stderr, "[bild staged n=%lld] fill %.1f  schedule %.1f  enqueue(H2D+launch) %.1f  wait(kernel+D2H) %.1f  copy out %.1f us\n",
                    (long long)n, clk.acc[0], clk.acc[1], clk.acc[2], clk.acc[3], clk.acc[4]);
    }
    return BILD_OK;
}

} // namespace

void *bild::internal_model_stream(const bild_model *m)
{
    if (!m || ensure_device(*m) != BILD_OK) return nullptr;
    return (void *)m->stream;
}

// (s, theta) rows that are resident in HBM already (internal.h): the fused AMIS step (amis_host.cpp) keeps its pooled samples
// there and hands the newest batch over where it lies
int bild::internal_logl_st_resident(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const double *d_ss,
                                    const uint8_t *d_thetas, unsigned flags, double *d_out, int32_t *status, void **stream)
{
    if (!m || !ts || ts->model != m || n < 1 || K1 < 1 || K1 > kSplitMaxK1 || !d_ss || !d_thetas || !d_out || !status)
        return fail(BILD_ERR_INVALID, "internal_logl_st_resident: bad arguments");
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != ts->device) return fail(BILD_ERR_INVALID, "trajectory set lives on device %d, current device is %d", ts->device, dev);
    std::lock_guard<std::mutex> call_lock(m->call_mu);
    if (m->h_in_busy) HIP_TRY(hipEventSynchronize(m->h_in_event));
    m->h_in_busy = false;
    const size_t nseg = (size_t)n * K1;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        if (int rc = m->ws_in.reserve(2 * nseg * sizeof(int32_t))) return rc;
    }
    int32_t *d_start = (int32_t *)m->ws_in.ptr, *d_state = d_start + nseg; // the lists the walk kernel writes for the frame loop
    LaunchIn in;
    in.d_ss = d_ss;
    in.d_thetas = (const int8_t *)d_thetas;
    in.status = status;
    if (stream) *stream = (void *)m->stream;
    int rc = launch_batch(*m, *ts, n, K1, d_start, d_state, nullptr, nullptr, flags, m->stream, d_out, in);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(m->h_in_event, m->stream)); // (the next host-buffer call must not reuse the lists before this one is through)
    m->h_in_busy = true;
    return BILD_OK;
}

// ------------------------------------------------------------------------------------
// exported
// ------------------------------------------------------------------------------------
extern "C" {

int bild_abi_version(void) { return BILD_AMD_ABI_VERSION; }

const char *bild_last_error(void) { return g_err.c_str(); }

void bild_set_last_error(const char *msg) { g_err = msg ? msg : ""; }

int bild_device_count(int *count)
{
    if (!count) return fail(BILD_ERR_INVALID, "count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *count = (e == hipSuccess) ? c : 0;
    return BILD_OK;
}

static int check_eval_args(const bild_model *m, const bild_trajset *ts, int64_t n, int K1)
{
    if (!m || !ts) return fail(BILD_ERR_INVALID, "NULL handle");
    if (ts->model != m) return fail(BILD_ERR_INVALID, "trajectory set belongs to a different model");
    if (n < 0) return fail(BILD_ERR_INVALID, "negative batch size");
    if (K1 < 1) return fail(BILD_ERR_INVALID, "need at least one segment per sample");
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != ts->device) return fail(BILD_ERR_INVALID, "trajectory set lives on device %d, current device is %d", ts->device, dev);
    return BILD_OK;
}

int bild_logl_segments_device_ordered(const bild_model *m, const bild_trajset *ts, int64_t n, int K1,
                                      const int32_t *d_seg_start, const int32_t *d_seg_state, const int32_t *d_traj_id,
                                      const int32_t *d_order, unsigned flags, void *hip_stream, double *d_out)
{
    int rc = check_eval_args(m, ts, n, K1);
    if (rc) return rc;
    if (n == 0) return BILD_OK;
    if (!d_seg_start || !d_seg_state || !d_out) return fail(BILD_ERR_INVALID, "NULL device buffer");
    hipStream_t st = (hipStream_t)hip_stream;
    if (flags & BILD_VALIDATE_DEVICE) {
        // checked on the device, verdict read back BEFORE anything is launched: this variant of the call waits
        int *d_err = nullptr;
        int h_err[2] = {0, 0};
        const size_t err_bytes = (2 + (d_order ? (size_t)n : 0)) * sizeof(int);
        HIP_TRY(hipMallocAsync((void **)&d_err, err_bytes, st));
        HIP_TRY(hipMemsetAsync(d_err, 0, err_bytes, st));
        int lrc = launch_validate(d_seg_start, d_seg_state, d_traj_id, d_order, n, K1, m->S, ts->n_traj, d_err, (void *)st);
        hipError_t ce = lrc == 0 ? hipMemcpyAsync(h_err, d_err, sizeof h_err, hipMemcpyDeviceToHost, st) : (hipError_t)lrc;
        (void)hipFreeAsync(d_err, st);
        if (ce != hipSuccess) return fail(BILD_ERR_HIP, "descriptor check failed to run: %s", hipGetErrorString(ce));
        HIP_TRY(hipStreamSynchronize(st));
        static const char *const what[] = {"", "traj_id out of range", "first segment does not start at frame 0",
                                           "segment starts are decreasing", "state out of range",
                                           "launch order is not a permutation of the samples"};
        if (h_err[0] != 0)
            return fail(BILD_ERR_INVALID, "device descriptors rejected: %s (e.g. sample %d)", what[h_err[0] & 7], h_err[1]);
    }
    return launch_batch(*m, *ts, n, K1, d_seg_start, d_seg_state, d_traj_id, d_order, flags, st, d_out);
}

int bild_logl_st_device(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const double *d_ss, const uint8_t *d_thetas,
                        const int32_t *d_traj_id, unsigned flags, void *hip_stream, double *d_out, int32_t *d_status)
{
    int rc = check_eval_args(m, ts, n, K1);
    if (rc) return rc;
    if (n == 0) return BILD_OK;
    if (!d_ss || !d_thetas || !d_out) return fail(BILD_ERR_INVALID, "NULL device buffer");
    if (K1 > kSplitMaxK1) return fail(BILD_ERR_UNSUPPORTED, "(s, theta) rows resident in HBM: at most %d segments per candidate (got %d)", kSplitMaxK1, K1);
    LaunchIn in;
    in.d_ss = d_ss;
    in.d_thetas = (const int8_t *)d_thetas;
    // the verdict on the rows: the caller's word, or a scratch word of the model nobody reads (rows that are no points on
    // the simplex still get NaN)
    if (d_status) {
        in.status = d_status;
    } else {
        std::lock_guard<std::mutex> lk(m->mu);
        if (!m->h_status.ptr) {
            if ((rc = m->h_status.reserve(64))) return rc;
            std::memset(m->h_status.ptr, 0, 64);
        }
        in.status = (int32_t *)m->h_status.ptr + 8;
    }
    return launch_batch(*m, *ts, n, K1, nullptr, nullptr, d_traj_id, nullptr, flags, (hipStream_t)hip_stream, d_out, in);
}

int bild_logl_segments_device(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *d_seg_start,
                              const int32_t *d_seg_state, const int32_t *d_traj_id, unsigned flags, void *hip_stream,
                              double *d_out)
{
    return bild_logl_segments_device_ordered(m, ts, n, K1, d_seg_start, d_seg_state, d_traj_id, nullptr, flags, hip_stream, d_out);
}

int bild_schedule_segments(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *seg_start,
                           const int32_t *seg_state, const int32_t *traj_id, unsigned flags, int32_t *order)
{
    if (!m || !ts || !order) return fail(BILD_ERR_INVALID, "NULL argument");
    if (ts->model != m) return fail(BILD_ERR_INVALID, "trajectory set belongs to a different model");
    if (n < 0 || K1 < 1) return fail(BILD_ERR_INVALID, "bad sizes");
    if (n > 0 && !seg_start) return fail(BILD_ERR_INVALID, "NULL buffer");
    if (traj_id)
        for (int64_t r = 0; r < n; ++r)
            if (traj_id[r] < 0 || traj_id[r] >= ts->n_traj) return fail(BILD_ERR_INVALID, "traj_id out of range");
    // the same checks as bild_logl_segments: the estimate of a candidate's work indexes arrays with these numbers
    for (int64_t r = 0; r < n; ++r) {
        const int32_t *a = seg_start + r * K1;
        if (a[0] != 0) return fail(BILD_ERR_INVALID, "seg_start[%lld][0] must be 0", (long long)r);
        for (int i = 1; i < K1; ++i)
            if (a[i] < a[i - 1] || a[i] < 1)
                return fail(BILD_ERR_INVALID, "segment starts of sample %lld are decreasing (or a later segment starts at frame 0)", (long long)r);
        if (seg_state)
            for (int i = 0; i < K1; ++i)
                if (seg_state[r * K1 + i] < 0 || seg_state[r * K1 + i] >= m->S)
                    return fail(BILD_ERR_INVALID, "state %d out of range at sample %lld", seg_state[r * K1 + i], (long long)r);
    }
    if (!schedule(*m, *ts, n, K1, seg_start, seg_state, traj_id, flags, order, false))
        for (int64_t r = 0; r < n; ++r) order[r] = (int32_t)r;
    return BILD_OK;
}

int bild_frames_executed(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *seg_start,
                         const int32_t *traj_id, const int32_t *order, unsigned flags, double *frames_total, double *frames_run)
{
    if (!m || !ts || !frames_total || !frames_run || (n > 0 && !seg_start)) return fail(BILD_ERR_INVALID, "NULL argument");
    int mode;
    int rc = pick_mode(*m, flags, &mode);
    if (rc) return rc;
    const bool prefix = ts->prefix_state == 1 && mode == kModal && !m->wide && !m->mid && !(flags & BILD_NO_PREFIX);
    Geometry geom{};
    int tpw = 1;
    if (prefix && geometry_for(m->NPm[mode], mode, n * ts->dstar_max, ts->means_max, &geom)) tpw = geom.tasks_per_wave();
    double total = 0.0, run = 0.0;
    const int ds = ts->dstar_max;
    // tasks are (slot, chain) pairs, tpw consecutive tasks share a wave and start at the earliest first switch among them
    const int64_t ntasks = n * ds;
    for (int64_t w0 = 0; w0 < ntasks; w0 += tpw) {
        int tw = INT_MAX;
        for (int64_t t = w0; t < std::min(ntasks, w0 + tpw); ++t) {
            const int64_t r = order ? order[t / ds] : t / ds;
            const TrajDesc &td = ts->descs[traj_id ? traj_id[r] : 0];
            if ((int)(t % ds) >= td.dstar) continue;
            int t0 = K1 > 1 ? seg_start[r * K1 + 1] : td.T;
            t0 = t0 < 1 ? 1 : (t0 > td.T ? td.T : t0);
            tw = std::min(tw, t0);
        }
        for (int64_t t = w0; t < std::min(ntasks, w0 + tpw); ++t) {
            const int64_t r = order ? order[t / ds] : t / ds;
            const TrajDesc &td = ts->descs[traj_id ? traj_id[r] : 0];
            if ((int)(t % ds) >= td.dstar) continue;
            total += td.T;
            run += prefix ? td.T - tw : td.T;
        }
    }
    *frames_total = total;
    *frames_run = run;
    return BILD_OK;
}

int bild_frames_run_read(const bild_model *m, int64_t *frames)
{
    if (!m || !frames) return fail(BILD_ERR_INVALID, "NULL argument");
    *frames = 0;
    if (!m->d_frames) return BILD_OK;
    unsigned long long v[kFrameCounters];
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(v, m->d_frames, sizeof v, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(m->d_frames, 0, sizeof v));
    unsigned long long tot = 0;
    for (unsigned long long w : v) tot += w;
    *frames = (int64_t)tot;
    return BILD_OK;
}

int bild_logl_segments(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *seg_start,
                       const int32_t *seg_state, const int32_t *traj_id, unsigned flags, double *out)
{
    int rc = check_eval_args(m, ts, n, K1);
    if (rc) return rc;
    if (n == 0) return BILD_OK;
    if (!seg_start || !seg_state || !out) return fail(BILD_ERR_INVALID, "NULL buffer");
    const int S = m->S;
    return run_staged(m, ts, n, K1, traj_id, flags, out, nullptr, nullptr, false, [&](char *payload) -> int {
        int32_t *h_start = (int32_t *)payload, *h_state = h_start + (size_t)n * K1;
        for (int64_t r = 0; r < n; ++r) {
            const int32_t *a = seg_start + r * K1, *b = seg_state + r * K1;
            if (a[0] != 0) return fail(BILD_ERR_INVALID, "seg_start[%lld][0] must be 0", (long long)r);
            for (int i = 0; i < K1; ++i) {
                if (b[i] < 0 || b[i] >= S) return fail(BILD_ERR_INVALID, "state %d out of range at sample %lld", b[i], (long long)r);
                if (i > 0 && (a[i] < a[i - 1] || a[i] < 1))
                    return fail(BILD_ERR_INVALID, "segment starts of sample %lld are decreasing (or a later segment starts at frame 0)", (long long)r);
                h_start[r * K1 + i] = a[i];
                h_state[r * K1 + i] = b[i];
            }
        }
        return BILD_OK;
    });
}

// The (s, theta) parametrisation of the sampler itself.  Switch frames as reference bild/amis.py:685-688 computes
// them, in the same floating-point operations:  np.cumsum(s)[:-1] is a sequential sum, times (T - 1) is one
// multiplication, floor, + 1.  No contraction of the multiply into the add: x86-64 baseline code has no fused
// instruction, and the pragma keeps it that way on any other target (file scope: it covers the lambda below).
#pragma clang fp contract(off)
static int st_row(const double *s, const int64_t *th, int K1, int S, double Tm1, int64_t r, int32_t *a, int32_t *b)
{
    a[0] = 0;
    double acc = 0.0;
    int32_t prev = 0;
    bool ok = true;
    for (int i = 0; i < K1; ++i) {
        ok &= (uint64_t)th[i] < (uint64_t)S;
        b[i] = (int32_t)th[i];
        if (i + 1 < K1) {
            acc = acc + s[i];
            const double pos = acc * Tm1;
            // floor(pos) for 0 <= pos < 2^31 is the truncating conversion (one SSE2 instruction, no libm call).  The
            // intrinsic is defined for every input: NaN and out-of-range values give INT64_MIN, which the unsigned range
            // test below rejects.  A position in (-1, 0) would truncate to 0 where np.floor gives -1 (the reference then
            // builds a profile whose FIRST interval is empty, amis.py:685-693): refused, like every negative position.
            const int64_t fl = _mm_cvttsd_si64(_mm_set_sd(pos));
            ok &= (uint64_t)fl < 2147483646ull;
            ok &= !(pos < 0.0);
            const int32_t idx = (int32_t)fl + 1;
            ok &= idx >= prev;
            prev = idx;
            a[i + 1] = idx;
        }
    }
    if (ok) return BILD_OK;
    for (int i = 0; i < K1; ++i)
        if (th[i] < 0 || th[i] >= S)
            return fail(BILD_ERR_INVALID, "state %lld out of range at sample %lld", (long long)th[i], (long long)r);
    return fail(BILD_ERR_INVALID, "interval lengths of sample %lld are not non-negative finite numbers (of a point on the simplex)", (long long)r);
}

int bild_segments_from_st(int64_t n, int K1, int n_states, const int32_t *T, int64_t T_stride, const double *ss,
                          const int64_t *thetas, int32_t *seg_start, int32_t *seg_state)
{
    if (n < 0 || K1 < 1 || n_states < 1) return fail(BILD_ERR_INVALID, "bad sizes");
    if (n == 0) return BILD_OK;
    if (!T || !ss || !thetas || !seg_start || !seg_state) return fail(BILD_ERR_INVALID, "NULL buffer");
    for (int64_t r = 0; r < n; ++r) {
        const int32_t Tr = T[r * T_stride];
        if (Tr < 1) return fail(BILD_ERR_INVALID, "trajectory length %d < 1", Tr);
        int rc = st_row(ss + r * K1, thetas + r * K1, K1, n_states, (double)(Tr - 1), r, seg_start + r * K1, seg_state + r * K1);
        if (rc) return rc;
    }
    return BILD_OK;
}

static int logl_st_impl(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const double *ss, const int64_t *thetas,
                        const int32_t *traj_id, unsigned flags, double *out, double *d_out, void *hip_stream)
{
    int rc = check_eval_args(m, ts, n, K1);
    if (rc) return rc;
    if (n == 0) return BILD_OK;
    if (!ss || !thetas || (!out && !d_out)) return fail(BILD_ERR_INVALID, "NULL buffer");
    const int S = m->S;
    // The rows go up as they are -- float64 interval lengths, states narrowed to one byte -- and the walk kernel turns
    // them into switch frames on the device (walk.hip; same operations as st_row below, bit for bit).  Lists of more
    // segments than that kernel holds in registers are converted here.
    const bool host_convert = config().st_on_host;
    if (K1 <= kSplitMaxK1 && !host_convert)
        return run_staged(m, ts, n, K1, traj_id, flags, out, d_out, (hipStream_t)hip_stream, true, [&](char *payload) -> int {
            const size_t nseg = (size_t)n * K1;
            std::memcpy(payload, ss, nseg * sizeof(double));
            uint8_t *th8 = (uint8_t *)(payload + nseg * sizeof(double));
            uint64_t bad = 0;
            for (size_t i = 0; i < nseg; ++i) {
                bad |= (uint64_t)((uint64_t)thetas[i] >= (uint64_t)S);
                th8[i] = (uint8_t)thetas[i];
            }
            if (bad)
                for (size_t i = 0; i < nseg; ++i)
                    if (thetas[i] < 0 || thetas[i] >= S)
                        return fail(BILD_ERR_INVALID, "state %lld out of range at sample %lld", (long long)thetas[i], (long long)(i / K1));
            return BILD_OK;
        });
    return run_staged(m, ts, n, K1, traj_id, flags, out, d_out, (hipStream_t)hip_stream, false, [&](char *payload) -> int {
        int32_t *h_start = (int32_t *)payload, *h_state = h_start + (size_t)n * K1;
        for (int64_t r = 0; r < n; ++r) {
            const double Tm1 = (double)(ts->descs[traj_id ? traj_id[r] : 0].T - 1);
            int rc2 = st_row(ss + r * K1, thetas + r * K1, K1, S, Tm1, r, h_start + r * K1, h_state + r * K1);
            if (rc2) return rc2;
        }
        return BILD_OK;
    });
}

int bild_logl_st(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const double *ss, const int64_t *thetas,
                 const int32_t *traj_id, unsigned flags, double *out)
{
    if (!out) return fail(BILD_ERR_INVALID, "NULL buffer");
    return logl_st_impl(m, ts, n, K1, ss, thetas, traj_id, flags, out, nullptr, nullptr);
}

int bild_logl_st_to_device(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const double *ss,
                           const int64_t *thetas, const int32_t *traj_id, unsigned flags, void *hip_stream, double *d_out)
{
    if (!d_out) return fail(BILD_ERR_INVALID, "NULL device buffer");
    return logl_st_impl(m, ts, n, K1, ss, thetas, traj_id, flags, nullptr, d_out, hip_stream);
}

int bild_logl_profiles(const bild_model *m, const bild_trajset *ts, int64_t n, int64_t ld, const int32_t *states,
                       const int32_t *traj_id, unsigned flags, double *out)
{
    if (!m || !ts) return fail(BILD_ERR_INVALID, "NULL handle");
    if (n < 0) return fail(BILD_ERR_INVALID, "negative batch size");
    if (n == 0) return BILD_OK;
    if (!states || !out) return fail(BILD_ERR_INVALID, "NULL buffer");
    // run-length encode
    std::vector<int> nseg((size_t)n);
    int K1 = 1;
    for (int64_t r = 0; r < n; ++r) {
        const int tj = traj_id ? traj_id[r] : 0;
        if (tj < 0 || tj >= ts->n_traj) return fail(BILD_ERR_INVALID, "traj_id[%lld]=%d out of range", (long long)r, tj);
        const int T = ts->descs[tj].T;
        if (ld < T) return fail(BILD_ERR_INVALID, "profile row stride %lld shorter than trajectory length %d", (long long)ld, T);
        int c = 1;
        for (int t = 1; t < T; ++t) c += states[r * ld + t] != states[r * ld + t - 1];
        nseg[r] = c;
        K1 = std::max(K1, c);
    }
    std::vector<int32_t> seg_start((size_t)n * K1), seg_state((size_t)n * K1);
    for (int64_t r = 0; r < n; ++r) {
        const int tj = traj_id ? traj_id[r] : 0;
        const int T = ts->descs[tj].T;
        int c = 0;
        seg_start[r * K1] = 0;
        seg_state[r * K1] = states[r * ld];
        for (int t = 1; t < T; ++t)
            if (states[r * ld + t] != states[r * ld + t - 1]) {
                ++c;
                seg_start[r * K1 + c] = t;
                seg_state[r * K1 + c] = states[r * ld + t];
            }
        for (int i = c + 1; i < K1; ++i) {
            seg_start[r * K1 + i] = INT_MAX;
            seg_state[r * K1 + i] = seg_state[r * K1 + c];
        }
    }
    return bild_logl_segments(m, ts, n, K1, seg_start.data(), seg_state.data(), traj_id, flags, out);
}

int bild_flop_count(const bild_model *m, const bild_trajset *ts, int64_t n, const int32_t *traj_id, unsigned flags,
                    double *canonical, double *executed)
{
    if (!m || !ts || !canonical || !executed) return fail(BILD_ERR_INVALID, "NULL argument");
    int mode;
    int rc = pick_mode(*m, flags, &mode);
    if (rc) return rc;
    const double N = m->N, d = m->d, nr = m->n;
    double can = 0.0, exe = 0.0;
    for (int64_t r = 0; r < n; ++r) {
        const int tj = traj_id ? traj_id[r] : 0;
        if (tj < 0 || tj >= ts->n_traj) return fail(BILD_ERR_INVALID, "traj_id out of range");
        const TrajDesc &td = ts->descs[tj];
        const double T = td.T, Tv = td.nvalid, ds = td.dstar, du = td.nuniq;
        can += (T - 1) * (4 * N * N * N * du + 2 * N * N * d) + Tv * ((4 * N * N + 3 * N) * du + 4 * N * d);
        if (mode == kDense)
            exe += (T - 1) * (4 * nr * nr * nr * ds + 2 * nr * nr * d) + Tv * ((4 * nr * nr + 3 * nr) * ds + 4 * nr * d);
        else // elementwise predict (2 mul / entry) + update; basis changes at state switches not counted
            exe += (T - 1) * (2 * nr * nr * ds + nr * ds + 2 * nr * d) + Tv * ((4 * nr * nr + 3 * nr) * ds + 4 * nr * d);
    }
    *canonical = can;
    *executed = exe;
    return BILD_OK;
}

int bild_logl_st_status(const bild_model *m, int64_t *bad_row)
{
    if (!m) return fail(BILD_ERR_INVALID, "NULL handle");
    std::lock_guard<std::mutex> call_lock(m->call_mu);
    if (m->h_in_busy) HIP_TRY(hipEventSynchronize(m->h_in_event));
    m->h_in_busy = false;
    if (bad_row) *bad_row = -1;
    if (!m->h_status.ptr) return BILD_OK;
    int32_t *h = (int32_t *)m->h_status.ptr;
    if (h[0] == 0) return BILD_OK;
    const int row = h[1];
    h[0] = h[1] = 0;
    if (bad_row) *bad_row = row;
    return fail(BILD_ERR_INVALID, "interval lengths of sample %d are not non-negative finite numbers (of a point on the simplex)", row);
}

} // extern "C"
