// Exact evidence of every k by a segment recursion (include/bild_amd.h, "exact evidence of every k"):
// SegdpCall is the host side of the recursion that bild_gauss_segment_evidence here, gauss_segsens.cpp and
// gauss_segdraw.cpp share (gauss_segdp.h): the refusals, the frame on the set's stream, the chunks of whole trajectories, the
// transitions' upload, the tables, the kernels' parameters, the launches level after level, and the host's formulas on the
// last column of the forward table, k by k.  Kernels: gauss_segdp.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "gauss_call.h"
#include "gauss_segdp.h"

namespace bild {

int segdp_check_transitions(int S, const uint8_t *transitions)
{
    if (!transitions) return fail(BILD_ERR_INVALID, "transitions is NULL");
    for (int i = 0; i < S * S; ++i)
        if (transitions[i] > 1) return fail(BILD_ERR_INVALID, "transitions[%d] = %d; must be 0 or 1", i, transitions[i]);
    return BILD_OK;
}

// What every call on the recursion refuses, in this order: k_max outside 0 .. kSegdpMaxK, flags other than BILD_SEGDP_NAN_OMIT,
// the transitions, a negative scratch_bytes, T_max shorter than a trajectory.  A BILD_* code.
static int segdp_check_call(int S, int k_max, unsigned flags, const uint8_t *transitions, int64_t scratch_bytes, int n_traj,
                            const int *T, int T_max)
{
    if (k_max < 0 || k_max > kSegdpMaxK)
        return fail(BILD_ERR_UNSUPPORTED, "k_max = %d: the segment recursion supports 0 <= k_max <= %d", k_max, kSegdpMaxK);
    if (flags & ~BILD_SEGDP_NAN_OMIT) return fail(BILD_ERR_INVALID, "flags = %u: unknown bits", flags);
    BILD_TRY(segdp_check_transitions(S, transitions));
    if (scratch_bytes < 0) return fail(BILD_ERR_INVALID, "scratch_bytes = %lld is negative", (long long)scratch_bytes);
    for (int j = 0; j < n_traj; ++j)
        if (T[j] > T_max) return fail(BILD_ERR_INVALID, "trajectory %d has %d frames, more than T_max = %d", j, T[j], T_max);
    return BILD_OK;
}

long double binom_ld(int n, int k)
{
    if (k < 0 || n < k) return 0.0L;
    unsigned __int128 c = 1;
    for (int i = 0; i < k; ++i) {
        const unsigned __int128 f = (unsigned __int128)(n - i);
        if (c >> 100) {
            long double d = (long double)c;
            for (int i2 = i; i2 < k; ++i2) d = d * (long double)(n - i2) / (long double)(i2 + 1);
            return d;
        }
        c = c * f / (unsigned __int128)(i + 1);
    }
    return (long double)c;
}

std::vector<long double> trace_counts(int S, const uint8_t *tr, int K)
{
    std::vector<long double> out(K), v(S, 1.0L), w(S);
    for (int k = 0; k < K; ++k) {
        long double n = 0.0L;
        for (long double x : v) n += x;
        out[k] = n;
        for (int a = 0; a < S; ++a) {
            long double acc = 0.0L;
            for (int b = 0; b < S; ++b)
                if (tr[a * S + b]) acc += v[b];
            w[a] = acc;
        }
        v.swap(w);
    }
    return out;
}

SegdpEvidence segdp_evidence(const double *f, int S, long double n_all, bool omit)
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
    double ok = 0.0, bad = 0.0, top = ninf, map_l = nan;
    bool have_map = false;
    for (int s = 0; s < S; ++s) {
        ok += f[s * 5 + 3];
        bad += f[s * 5 + 4];
        if (f[s * 5 + 1] > 0.0) top = std::max(top, f[s * 5]);
        if (f[s * 5 + 3] > 0.0 && (!have_map || f[s * 5] > map_l)) {
            map_l = f[s * 5];
            have_map = true;
        }
    }
    const bool any = n_all > 0.0L;
    const double count = !any ? 0.0 : omit ? ok : (double)n_all;
    const double log_count = omit ? std::log(ok) : (double)logl(n_all);
    SegdpEvidence e{ninf, nan, count, bad, top, 0.0, any && have_map ? map_l : nan, any, false};
    if (any && !omit && bad > 0.0) e.logev = nan;
    else if (any && count > 0.0 && top != ninf) {
        double z = 0.0, u = 0.0;
        for (int s = 0; s < S; ++s) {
            if (!(f[s * 5 + 1] > 0.0)) continue;
            const double w = f[s * 5 + 1] * std::exp(f[s * 5] - top);
            z += w;
            if (w > 0.0) u += w * f[s * 5 + 2];
        }
        e.logev = top + std::log(z) - log_count;
        e.kl = u / z - e.logev;
        e.z = z;
        e.usable = true;
    }
    return e;
}

int segdp_run_forward(const SegdpParams &p, int k_max, void *st)
{
    if (launch_segdp_init(p, false, st)) return fail(BILD_ERR_HIP, "launch of the segment recursion's first level failed");
    for (int j = 1; j <= k_max; ++j)
        if (launch_segdp_mix(p, j, st) || launch_segdp_level(p, j, st))
            return fail(BILD_ERR_HIP, "launch of level %d of the segment recursion failed", j);
    if (launch_segdp_backtrack(p, st)) return fail(BILD_ERR_HIP, "launch of the back-pointer walk failed");
    return BILD_OK;
}

int segdp_run_backward(const SegdpParams &p, int k_max, void *st)
{
    if (launch_segdp_init(p, true, st)) return fail(BILD_ERR_HIP, "launch of the backward recursion's first level failed");
    for (int lv = 0; lv < k_max; ++lv)
        if (launch_segdp_blevel(p, lv, st) || launch_segdp_bmix(p, lv + 1, st))
            return fail(BILD_ERR_HIP, "launch of level %d of the backward recursion failed", lv);
    return BILD_OK;
}

int SegdpCall::check(const bild_gauss_model *m, const bild_gauss_trajset *ts, int k_max_, const uint8_t *tr, int T_max, unsigned flags,
                     int64_t scratch, const void *out)
{
    BILD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    S = m->S;
    BILD_TRY(segdp_check_call(S, k_max_, flags, tr, scratch, n_traj, T, T_max));
    for (int j = 0; j < n_traj; ++j) Tm = std::max(Tm, T[j]);
    n = n_traj;
    k_max = k_max_;
    K = k_max + 1;
    omit = (flags & BILD_SEGDP_NAN_OMIT) != 0;
    transitions = tr;
    scratch_bytes = scratch;
    return BILD_OK;
}

int SegdpCall::open(CallFrame &call, const bild_gauss_model *m, const bild_gauss_trajset *ts, unsigned sets_, int64_t own_bytes)
{
    sets = sets_;
    BILD_TRY(call.open(m, ts));
    BILD_TRY(call.chunk_of(segdp_table_bytes(sets, S, K, Tm) + own_bytes, scratch_bytes, n, &chunk));

    uint8_t *d_tr = nullptr;
    BILD_TRY(call.alloc(&d_tr, (size_t)S * S));
    HIP_TRY(hipMemcpy(d_tr, transitions, (size_t)S * S, hipMemcpyHostToDevice));    // (synchronous: caller memory)
    const int ld = Tm + 1, ntile = segdp_ntile(Tm);
    const int64_t slot = (int64_t)K * S * ld;
#define X(member, set, entries) \
    if (sets & (set)) BILD_TRY(call.alloc(&p.member, (size_t)chunk * (size_t)(entries)));
    BILD_SEGDP_TABLES(X)
#undef X
    p.tr = d_tr;
    p.slot = slot;
    p.S = S;
    p.K = K;
    p.Tm = Tm;
    p.ld = ld;
    p.ntile = ntile;
    if (sets & kSegdpForward) {
        fin.resize((size_t)chunk * K * S * 5);
        ntraces = trace_counts(S, transitions, K);
    }
    return BILD_OK;
}

int SegdpCall::run(CallFrame &call, const GaussTraj *trajs, int nc)
{
    p.trajs = trajs;
    p.n_traj = nc;
    if (sets & kSegdpForward) BILD_TRY(segdp_run_forward(p, k_max, call.st));
    if (sets & kSegdpBackward) BILD_TRY(segdp_run_backward(p, k_max, call.st));
    return BILD_OK;
}

int SegdpCall::read_back(CallFrame &call, int nc)
{
    HIP_TRY(hipMemcpyAsync(fin.data(), p.fin, (size_t)nc * K * S * 5 * 8, hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    return BILD_OK;
}

} // namespace bild

extern "C" int bild_gauss_segment_evidence(const bild_gauss_model *m, const bild_gauss_trajset *ts, int k_max, const uint8_t *transitions,
                                           int T_max, unsigned flags, int64_t scratch_bytes, bild_segdp_out *out)
{
    SegdpCall rec;      // (before the frame, with the host copies below: asynchronous copies write them)
    std::vector<double> post;
    std::vector<int32_t> seg_a, seg_v;
    BILD_TRY(rec.check(m, ts, k_max, transitions, T_max, flags, scratch_bytes, out));
    if (rec.n_traj == 0) return BILD_OK;
    const bool marg = out->log_post != nullptr;
    const int S = rec.S, K = rec.K;

    CallFrame call;
    BILD_TRY(rec.open(call, m, ts, marg ? kSegdpForward | kSegdpBackward | kSegdpCover : kSegdpForward, 0));
    hipStream_t st = call.st;
    const SegdpParams &p = rec.p;
    const int chunk = rec.chunk, ld = p.ld;
    const int64_t slot = p.slot;

    post.resize(marg ? (size_t)chunk * slot : 0);
    seg_a.resize((size_t)chunk * K * K);
    seg_v.resize((size_t)chunk * K * K);
    const double nan = std::numeric_limits<double>::quiet_NaN();

    for (int j0 = 0; j0 < rec.n_traj; j0 += chunk) {
        const int nc = std::min(chunk, rec.n_traj - j0);
        BILD_TRY(rec.run(call, call.d_trajs + j0, nc));
        if (marg) {
            if (launch_segdp_cover(p, st) || launch_segdp_carry(p, st)) return fail(BILD_ERR_HIP, "launch of the marginal kernels failed");
            HIP_TRY(hipMemcpyAsync(post.data(), p.post, (size_t)nc * slot * 8, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipMemcpyAsync(seg_a.data(), p.map_seg_start, (size_t)nc * K * K * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(seg_v.data(), p.map_seg_state, (size_t)nc * K * K * 4, hipMemcpyDeviceToHost, st));
        BILD_TRY(rec.read_back(call, nc));

        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = rec.T[jt];
            rec.each_k(i, Tj, [&](int k, const SegdpEvidence &e) {
                const size_t o = (size_t)jt * K + k;
                if (out->logev) out->logev[o] = e.logev;
                if (out->kl) out->kl[o] = e.kl;
                if (out->map_logl) out->map_logl[o] = e.map_logl;
                if (out->n_profiles) out->n_profiles[o] = e.count;
                if (out->n_omitted) out->n_omitted[o] = e.any && rec.omit ? e.bad : 0.0;
                if (out->map_seg_start) std::copy_n(seg_a.data() + ((size_t)i * K + k) * K, K, out->map_seg_start + o * K);
                if (out->map_seg_state) std::copy_n(seg_v.data() + ((size_t)i * K + k) * K, K, out->map_seg_state + o * K);
                if (!marg) return;
                double *lp = out->log_post + o * S * T_max;
                const double *ps = post.data() + (size_t)i * slot + (size_t)k * S * ld;
                for (int t = 0; t < T_max; ++t) {
                    const bool in = e.usable && t < Tj;
                    double tot = 0.0;
                    if (in)
                        for (int s = 0; s < S; ++s) tot += ps[(size_t)s * ld + t];
                    for (int s = 0; s < S; ++s) lp[(size_t)s * T_max + t] = in ? std::log(ps[(size_t)s * ld + t]) - std::log(tot) : nan;
                }
            });
        }
    }
    return BILD_OK;
}
