// The Rouse trajectory generator: the C ABI bild_rouse_simulate (include/bild_amd.h), its checks, the staging of the
// per-state modal arrays and of the trajectories, and the chunked upload of host-drawn normals.  Kernel: sim.hip.
#include "sim.h"
#include "sim_host.h"

namespace {

using namespace bild;

bool all_finite(const double *a, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

// frames per LDS chunk: even, at most 64, the chunk's rows within 16 KiB (at least 2 frames)
int sim_chunk(int N, int dpb)
{
    const int c = (int)(16384 / (((size_t)N * dpb + 1) * sizeof(double)));
    return std::max(2, std::min(64, c) & ~1);
}

} // namespace

extern "C" int bild_rouse_simulate(int S, int N, int d, const double *V, const double *b, const double *sqrt_sig,
                                   const double *sqrt_cinf, const double *VtG, const double *VtM0, const double *w, int n,
                                   const int32_t *T, int K1, const int32_t *seg_start, const int32_t *seg_state,
                                   const uint8_t *missing, const double *loc_err, const double *normals, uint64_t seed,
                                   int64_t scratch_bytes, double *out)
{
    if (S < 1 || N < 1 || d < 1) return fail(BILD_ERR_INVALID, "S = %d, N = %d, d = %d must be positive", S, N, d);
    if (n < 0 || K1 < 1) return fail(BILD_ERR_INVALID, "n = %d, K1 = %d", n, K1);
    if (scratch_bytes < 0) return fail(BILD_ERR_INVALID, "scratch_bytes = %lld is negative", (long long)scratch_bytes);
    if (!V || !b || !sqrt_sig || !sqrt_cinf || !VtG || !VtM0 || !w) return fail(BILD_ERR_INVALID, "NULL model array");
    if (n > 0 && (!T || !seg_start || !seg_state || !loc_err || !out)) return fail(BILD_ERR_INVALID, "NULL trajectory array");
    if (N > kSimMaxN) return fail(BILD_ERR_UNSUPPORTED, "N = %d: the generator supports at most %d modes", N, kSimMaxN);
    if (d > 8) return fail(BILD_ERR_UNSUPPORTED, "d = %d: the generator supports at most 8 dimensions", d);
    const size_t SN = (size_t)S * N, SNN = SN * N, SND = SN * d;
    if (!all_finite(V, SNN) || !all_finite(b, SN) || !all_finite(sqrt_sig, SN) || !all_finite(sqrt_cinf, SN) ||
        !all_finite(VtG, SND) || !all_finite(VtM0, SND) || !all_finite(w, N))
        return fail(BILD_ERR_INVALID, "a model array has a non-finite entry");
    if (n == 0) return BILD_OK;

    // trajectories: lengths, segments, localization errors
    std::vector<int64_t> frame_off(n + 1, 0), z_off(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        if (T[i] < 1) return fail(BILD_ERR_INVALID, "trajectory %d has %d frames", i, T[i]);
        frame_off[i + 1] = frame_off[i] + T[i];
        z_off[i + 1] = z_off[i] + (int64_t)T[i] * (N + 1) * d;
        const int32_t *a = seg_start + (size_t)i * K1, *s = seg_state + (size_t)i * K1;
        if (a[0] != 0) return fail(BILD_ERR_INVALID, "trajectory %d: the first segment must start at 0", i);
        for (int q = 0; q < K1; ++q) {
            if (s[q] < 0 || s[q] >= S) return fail(BILD_ERR_INVALID, "trajectory %d: state %d out of range (%d states)", i, s[q], S);
            if (q > 0 && (a[q] < 1 || a[q] < a[q - 1]))
                return fail(BILD_ERR_INVALID, "trajectory %d: segment starts must be >= 1 and non-decreasing", i);
        }
        for (int k = 0; k < d; ++k)
            if (!std::isfinite(loc_err[(size_t)i * d + k])) return fail(BILD_ERR_INVALID, "trajectory %d: localization error is not finite", i);
    }
    const int64_t rows = frame_off[n];

    int dev = 0;
    if (hipGetDeviceCount(&dev) != hipSuccess || dev < 1) return fail(BILD_ERR_NO_DEVICE, "no usable GPU");
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    // replay scratch: at most 1 GiB and a third of the free memory (or the caller's budget), whole trajectories per chunk
    const int64_t scratch = sim_scratch_bytes(scratch_bytes, free_b);
    const int64_t scratch_doubles = std::min<int64_t>(scratch / 8, z_off[n]);
    if (normals)
        for (int i = 0; i < n; ++i)
            if (z_off[i + 1] - z_off[i] > scratch_doubles)
                return fail(BILD_ERR_UNSUPPORTED, "trajectory %d needs %lld bytes of normals; the upload budget is %lld", i,
                            (long long)(z_off[i + 1] - z_off[i]) * 8, (long long)scratch);

    // per state: V, V^T, the modal vectors, u = V^T w
    std::vector<double> Vt(SNN), u(SN, 0.0);
    for (int s = 0; s < S; ++s) {
        const double *Vs = V + (size_t)s * N * N;
        for (int m = 0; m < N; ++m)
            for (int j = 0; j < N; ++j) {
                Vt[(size_t)s * N * N + (size_t)j * N + m] = Vs[(size_t)m * N + j];
                u[(size_t)s * N + j] += Vs[(size_t)m * N + j] * w[m];
            }
    }

    SimBufs bufs;
    HIP_TRY(hipStreamCreateWithFlags(&bufs.stream, hipStreamNonBlocking));
    SimParams p{};
    BILD_TRY(bufs.put(&p.V, V, SNN));
    BILD_TRY(bufs.put(&p.Vt, Vt.data(), SNN));
    BILD_TRY(bufs.put(&p.b, b, SN));
    BILD_TRY(bufs.put(&p.ssig, sqrt_sig, SN));
    BILD_TRY(bufs.put(&p.scinf, sqrt_cinf, SN));
    BILD_TRY(bufs.put(&p.g, VtG, SND));
    BILD_TRY(bufs.put(&p.m0, VtM0, SND));
    BILD_TRY(bufs.put(&p.u, u.data(), SN));
    BILD_TRY(bufs.put(&p.T, T, n));
    BILD_TRY(bufs.put(&p.frame_off, frame_off.data(), n));
    BILD_TRY(bufs.put(&p.seg_start, seg_start, (size_t)n * K1));
    BILD_TRY(bufs.put(&p.seg_state, seg_state, (size_t)n * K1));
    uint8_t *d_missing;
    BILD_TRY(bufs.put(&d_missing, missing, rows));
    if (!missing) HIP_TRY(hipMemsetAsync(d_missing, 0, rows, bufs.stream));
    p.missing = d_missing;
    BILD_TRY(bufs.put(&p.err, loc_err, (size_t)n * d));
    BILD_TRY(bufs.put(&p.out, nullptr, rows * d));
    p.K1 = K1;
    p.S = S;
    p.N = N;
    p.d = d;
    p.dpb = std::min(d, kSimMaxLanes / N);
    p.chunk = sim_chunk(N, p.dpb);
    p.seed = seed;

    // the launches keep their trajectory arrays at the launch's first trajectory
    auto launch = [&](SimParams q, int first, int count) {
        q.T += first;
        q.frame_off += first;
        q.seg_start += (size_t)first * K1;
        q.seg_state += (size_t)first * K1;
        q.err += (size_t)first * d;
        if (q.z_off) q.z_off += first;
        q.first = first;
        q.n = count;
        if (launch_rouse_simulate(q, bufs.stream)) return fail(BILD_ERR_HIP, "launch of the simulation kernel failed");
        return (int)BILD_OK;
    };
    if (!normals) {
        BILD_TRY(launch(p, 0, n));
    } else {
        double *d_z;
        BILD_TRY(bufs.put(&d_z, nullptr, (size_t)scratch_doubles));
        BILD_TRY(bufs.put(&p.z_off, z_off.data(), n));
        p.z = d_z;
        for (int first = 0; first < n;) {
            const int last = sim_chunk_end(z_off, first, n, scratch_doubles);
            // (pageable source: the copy is staged, and the next chunk's copy waits for this chunk's kernel on the stream)
            HIP_TRY(hipMemcpyAsync(d_z, normals + z_off[first], (size_t)(z_off[last] - z_off[first]) * 8, hipMemcpyHostToDevice,
                                   bufs.stream));
            p.z_first = z_off[first];
            BILD_TRY(launch(p, first, last - first));
            first = last;
        }
    }
    HIP_TRY(hipMemcpyAsync(out, p.out, (size_t)rows * d * 8, hipMemcpyDeviceToHost, bufs.stream));
    HIP_TRY(hipStreamSynchronize(bufs.stream));
    return BILD_OK;
}
