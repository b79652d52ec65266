// The first-order tail of a transient (round 4).
//
// Behind a switch a candidate's filter converges onto the switch-free filter of its new state (common.h: prefix table).  The
// COVARIANCE forgets twice as fast as the means (its deviation is quadratic in what the means' is linear in): for the
// default Rouse model C agrees with the table's to 2^-43 after 16-20 frames, the means after 36-46 -- and until round 4 a
// candidate ran all of them.  Once C has converged, K_t and S_t of the candidate ARE the table's, and a mean deviation
// delta at frame t0 evolves linearly, delta_t = (I - K_t w^T) Lambda delta_{t-1} (Lambda delta_{t-1} over a missing frame), and
// shifts every later innovation by -w^T Lambda delta_{t-1}.  What that does to the log-likelihood of the frames behind t0 is,
// per dimension,
//     sum_t [ e_t (w^T Lambda delta_{t-1}) / S_t  -  (w^T Lambda delta_{t-1})^2 / (2 S_t) ]  =  g_{t0} . delta_{t0}  +  O(delta^2),
// with a vector g_{t0} that depends on the TABLE's filter alone (e_t: its innovations):
//     g_{t-1} = [frame t observed] (e_t / S_t) Lambda w  +  A_t^T g_t,     A_t^T g = Lambda (g - w (K_t . g))  resp.  Lambda g,     g_{T-1} = 0.
// The recursion is run once per (trajectory, chain, state), right behind the prefix table, and leaves g for every record
// (kDMax x NP doubles, beside the table: KParams::tail_g) -- in two kernels: what it needs of the table's filter at every frame
// (gain, innovations) is recomputed for all frames in parallel, the pass that is sequential in t then moves one double per
// lane and frame (3.1 ms per T = 1000 trajectory in one kernel that did both -> 0.8 ms in two -> see tail_scan_kernel).  The frame loop then leaves a transient as
// soon as its covariance has converged and its means are within 2^-20 of the table's (delta^2 terms ~ 1e-11 at the bound, 1e-12 in the runs), adds
// g . delta, and takes the table's sums for the rest of the segment -- if the next switch is far enough away for the means
// to have converged by then (kernels.hip: compare_with_table).  NumPy experiment behind it (default model, N = 20 / 32): jump
// after 17-21 / 75 frames instead of 36-46 / 89-111, remaining log-likelihood reproduced to 2-4e-13.
//
// g needs no more than a few digits (it multiplies a delta of 1e-7): the filter quantities are recomputed here from the
// records in plain arithmetic, not in the bit-exact order of the frame loop.
#include <hip/hip_runtime.h>

#include "common.h"

namespace bild {
namespace {

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Phase 1, parallel over frames: one wavefront per (task, frame t) recomputes what the table's filter did AT frame t from the
// record of frame t - 1 -- gain K_t (NP doubles) and, per dimension, e_t / S_t -- into a scratch array of NP + 4 doubles per
// record: [K (NP) | e_0/S, e_1/S, e_2/S | observed].  (task = (trajectory j, chain e, state s); lane i < NP owns row i)
__global__ void __launch_bounds__(64) tail_gain_kernel(const TrajDesc *__restrict__ trajs, int n_traj, int S, int NP, int d, int dstar_max,
                                                       const double *__restrict__ states, const double *__restrict__ prefix,
                                                       const int64_t *__restrict__ first, double *__restrict__ gain)
{
    // blocks are numbered trajectory by trajectory: first[j] = number of (chain, state, frame) blocks in front of trajectory j
    const int64_t b = blockIdx.x;
    int j = 0;
    for (int hi = n_traj; hi - j > 1;) { // first[j] <= b < first[j + 1]
        const int mid = (j + hi) / 2;
        if (first[mid] <= b) j = mid;
        else hi = mid;
    }
    const TrajDesc &td = trajs[j];
    const int T = td.T;
    int64_t q = b - first[j]; // (e * S + s) * T + t
    const int t = (int)(q % T);
    q /= T;
    const int s = (int)(q % S), e = (int)(q / S);
    if (e >= td.dstar || t < 1) return;
    const int lane = threadIdx.x, nd = td.ndims[e];
    const bool row = lane < NP;
    const int i = row ? lane : 0;
    const int REC = prefix_record_doubles(NP);
    const double *sb = states + (size_t)s * StateBlock::size(NP);
    const double lam = row ? sb[StateBlock::lam(NP) + i] : 0.0, wi = row ? sb[StateBlock::wq(NP) + i] : 0.0,
                 sig = row ? sb[StateBlock::sig(NP) + i] : 0.0;
    const int64_t rec0 = td.prefix_rec0 + ((int64_t)e * S + s) * T;
    const double *rec = prefix + (rec0 + (t - 1)) * REC; // state after frame t - 1
    const double *x = td.x + (size_t)t * d;
    double *out = gain + (rec0 + t) * (NP + 4);
    const bool observed = !isnan(x[0]);
    if (!observed) {
        if (lane < NP + 4) out[lane] = 0.0;
        return;
    }
    // predicted covariance times w:  (C- w)_i = lam_i sum_c lam_c w_c C_ic + sig_i w_i   (row i of C = column i, symmetric)
    double cw = 0.0;
    if (row) {
        for (int c = 0; c < NP; ++c) cw = fma(sb[StateBlock::lam(NP) + c] * sb[StateBlock::wq(NP) + c], rec[(size_t)i * NP + c], cw);
        cw = fma(lam, cw, sig * wi);
    }
    double part[1 + kDMax];
    part[0] = row ? wi * cw : 0.0;
    for (int m = 0; m < kDMax; ++m) part[1 + m] = (row && m < nd) ? wi * lam * rec[(size_t)(NP + m) * NP + i] : 0.0; // (no external force: the host checks has_G)
    for (int v = 0; v < 1 + kDMax; ++v) part[v] = wave_sum(part[v]);
    const double Sv = td.s2[e] + part[0];
    if (row) out[i] = cw / Sv;
    if (lane < kDMax) out[NP + lane] = lane < nd ? (x[td.dims[e][lane]] - part[1 + lane]) / Sv : 0.0;
    if (lane == kDMax) out[NP + kDMax] = 1.0;
}

// Phase 2, sequential over frames:  g_{t-1} = (e_t / S_t) Lambda w + Lambda (g_t - w (K_t . g_t))  backwards (Lambda g_t over a missing frame).
// The three dimensions of a task sit side by side in one wavefront -- rows of W = 16 lanes (W = 32 above 16 modes: two wavefronts
// per task), lane i of a row owns mode i of its dimension --, so that K_t . g_t is ONE butterfly over a row for all of them, in
// DPP moves (no LDS round trips: four ds_bpermute steps per dimension were 0.79 us of every frame, 0.8 ms of a T = 1000
// trajectory's first evaluation); what a frame needs from memory -- one double per lane and two scalars -- is asked for
// kTailChunk frames ahead.
constexpr int kTailChunk = 16;

template <int CTRL>
__device__ __forceinline__ double dpp_move(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// sum over the 16 lanes of a DPP row, the same in every lane of the row
__device__ __forceinline__ double row_sum16(double v)
{
    v += dpp_move<0xB1>(v);  // quad_perm [1, 0, 3, 2]
    v += dpp_move<0x4E>(v);  // quad_perm [2, 3, 0, 1]
    v += dpp_move<0x141>(v); // row_half_mirror
    v += dpp_move<0x140>(v); // row_mirror
    return v;
}

template <int W>
__global__ void __launch_bounds__(64) tail_scan_kernel(const TrajDesc *__restrict__ trajs, int n_traj, int S, int NP, int dstar_max,
                                                       const double *__restrict__ states, const double *__restrict__ gain,
                                                       double *__restrict__ tail_g)
{
    constexpr int kDimsPerWave = 64 / W, kParts = (kDMax + kDimsPerWave - 1) / kDimsPerWave;
    const int task = blockIdx.x / kParts, part = blockIdx.x % kParts; // task = (j * dstar_max + e) * S + s
    const int s = task % S, e = (task / S) % dstar_max, j = task / (S * dstar_max);
    if (j >= n_traj) return;
    const TrajDesc &td = trajs[j];
    if (e >= td.dstar) return;
    const int lane = threadIdx.x, T = td.T;
    const int m = part * kDimsPerWave + lane / W, il = lane % W;
    const bool row = il < NP && m < kDMax;
    const int i = il < NP ? il : 0, mm = m < kDMax ? m : 0;
    const double *sb = states + (size_t)s * StateBlock::size(NP);
    const double lam = row ? sb[StateBlock::lam(NP) + i] : 0.0, wi = row ? sb[StateBlock::wq(NP) + i] : 0.0;
    const int64_t rec0 = td.prefix_rec0 + ((int64_t)e * S + s) * T;
    const int Wd = NP + 4;
    double g = 0.0;
    if (row) tail_g[((rec0 + (T - 1)) * kDMax + m) * NP + i] = 0.0; // g_{T-1} = 0
    if (T < 2) return;
    // frames T - 1 ... 1 in chunks of kTailChunk; the chunk after this one is on its way while this one is worked on
    double Kb[kTailChunk], cb[kTailChunk], ob[kTailChunk];
    auto ask = [&](int t_hi, double *K, double *c, double *o) {
#pragma unroll
        for (int u = 0; u < kTailChunk; ++u) {
            const int t = t_hi - u > 1 ? t_hi - u : 1;
            const double *r = gain + (rec0 + t) * Wd;
            K[u] = r[i];
            c[u] = r[NP + mm];
            o[u] = r[NP + kDMax];
        }
    };
    ask(T - 1, Kb, cb, ob);
    for (int t_hi = T - 1; t_hi >= 1; t_hi -= kTailChunk) {
        double Kn[kTailChunk], cn[kTailChunk], on[kTailChunk];
        ask(t_hi - kTailChunk, Kn, cn, on);
#pragma unroll
        for (int u = 0; u < kTailChunk; ++u) {
            const int t = t_hi - u;
            if (t >= 1) {
                if (ob[u] != 0.0) {
                    double kg = row ? Kb[u] * g : 0.0;
                    kg = row_sum16(kg);
                    if constexpr (W == 32) kg += __shfl_xor(kg, 16, 64);
                    g = lam * (g - wi * kg) + cb[u] * lam * wi;
                } else {
                    g *= lam;
                }
                if (row) tail_g[((rec0 + (t - 1)) * kDMax + m) * NP + i] = g;
            }
        }
#pragma unroll
        for (int u = 0; u < kTailChunk; ++u) {
            Kb[u] = Kn[u];
            cb[u] = cn[u];
            ob[u] = on[u];
        }
    }
}

// ---- switch tails -----------------------------------------------------------------------------------------------------------
// The vector g above is the adjoint of the switch-free filter: a look may take it only if no further switch disturbs the frames it
// speaks for, and the chains that end a launch -- four and more close switches -- are refused for exactly that.  The adjoint can be
// taken along the path such a candidate really has in front of it: state s up to frame t2 - 1, the switch s -> sn at t2, the
// transient from a synchronised start (m frames: the transient table's entry), then the switch-free filter of sn.  That path
// depends on (trajectory, chain, s -> sn, t2) alone.  One wavefront per such switch:
//   forward   the transient once more, in plain arithmetic, from the prefix record of (s, t2 - 1) through the basis change R: its
//             gains K'_u and e'_u / S'_u for u = t2 ... t2 + m - 1 (kept in LDS);
//   backward  h = tail_g of (sn, t2 + m - 1) -- where the builder of the entry found the transient synchronised --, the recursion of
//             phase 2 above through the transient's frames, G_0 = R^T h across the switch (from sn's basis into s's), and J - 1 more
//             steps along the switch-free filter of s (its gains: phase 1's scratch), G_j at frame t2 - j.
// G_j (kDMax x NP, laid out as tail_g) is read by a look at frame t = t2 - j, which compares the state after frame t - 1:
// logl_body.h, compare_with_table.  Entries without a converged transient inside the trajectory (m <= 0, t2 + m >= T) or with one
// longer than kSwitchTailMaxM stay zero and are never read (the look asks for room behind the transient, and for m <= the cap).
// lane i < NP owns row i of C (LDS, stride NP + 1) and entry i of every vector.
__global__ void __launch_bounds__(64) switch_tail_kernel(const TrajDesc *__restrict__ trajs, int n_traj, int S, int NP, int d, int dstar_max,
                                                         const double *__restrict__ states, const double *__restrict__ tab, int tab_factored,
                                                         const double *__restrict__ prefix, const double *__restrict__ tail_g,
                                                         const TransEntry *__restrict__ trans, const int64_t *__restrict__ first,
                                                         const double *__restrict__ gain, int J, double *__restrict__ stail)
{
    extern __shared__ __align__(16) double sm[];
    // entries are numbered as the transient state table's: first[j] * (S - 1) = TrajDesc::strans0
    const int64_t b = blockIdx.x;
    int j = 0;
    for (int hi = n_traj; hi - j > 1;) {
        const int mid = (j + hi) / 2;
        if (first[mid] * (S - 1) <= b) j = mid;
        else hi = mid;
    }
    const TrajDesc &td = trajs[j];
    const int T = td.T;
    int64_t q = b - first[j] * (S - 1); // ((e * S + s) * (S - 1) + sn') * T + t2
    const int t2 = (int)(q % T);
    q /= T;
    const int sni = (int)(q % (S - 1));
    q /= (S - 1);
    const int s = (int)(q % S), e = (int)(q / S);
    const int sn = sni + (sni >= s ? 1 : 0);
    if (e >= td.dstar || t2 < 1) return;
    const int m = trans[td.trans0 + (((int64_t)e * S + s) * S + sn) * T + t2].m;
    if (m <= 0 || m > kSwitchTailMaxM || t2 + m >= T) return;
    const int lane = threadIdx.x, nd = td.ndims[e];
    const bool row = lane < NP;
    const int i = row ? lane : 0;
    const int LD = NP + 1, REC = prefix_record_doubles(NP), MS = table_stride(NP);
    double *const Cs = sm;                      // NP x LD
    double *const Ys = Cs + NP * LD;            // NP x LD: the other side of a product
    double *const vs = Ys + NP * LD;            // kDMax x NP: vectors on their way through a matrix; NP: C w of a frame
    double *const Ks = vs + kDMax * NP;         // kSwitchTailMaxM x NP: the transient's gains
    double *const cs = Ks + kSwitchTailMaxM * NP; // kSwitchTailMaxM x (kDMax + 1): e / S per dimension | observed
    const double *sb0 = states + (size_t)s * StateBlock::size(NP), *sb1 = states + (size_t)sn * StateBlock::size(NP);
    const int64_t rec_s = td.prefix_rec0 + ((int64_t)e * S + s) * T, rec_n = td.prefix_rec0 + ((int64_t)e * S + sn) * T;

    // the state in front of the switch: the record of (s, t2 - 1)
    const double *rec = prefix + (rec_s + (t2 - 1)) * REC;
    double M[kDMax];
    if (row)
        for (int c = 0; c < NP; ++c) Cs[i * LD + c] = rec[(size_t)c * NP + i];
    for (int v = 0; v < kDMax; ++v) M[v] = (row && v < nd) ? rec[(size_t)(NP + v) * NP + i] : 0.0;
    __syncthreads();
    // the basis change A <- X A, C <- C X^T, X = R[sn][s] (or Q[s], then Q[sn]^T)
    const int steps = tab_factored ? 2 : 1;
    for (int stp = 0; stp < steps; ++stp) {
        const double *X = tab + (size_t)(tab_factored ? (stp == 0 ? s : S + sn) : sn * S + s) * MS;
        for (int v = 0; v < kDMax; ++v)
            if (row) vs[v * NP + i] = M[v];
        if (row) // Y = X C
            for (int c = 0; c < NP; ++c) {
                double a = 0.0;
                for (int k = 0; k < NP; ++k) a = fma(X[i * NP + k], Cs[k * LD + c], a);
                Ys[i * LD + c] = a;
            }
        __syncthreads();
        for (int v = 0; v < kDMax; ++v) {
            double a = 0.0;
            if (row)
                for (int k = 0; k < NP; ++k) a = fma(X[i * NP + k], vs[v * NP + k], a);
            M[v] = a;
        }
        if (row) // C = Y X^T (row i of Y is this lane's own)
            for (int c = 0; c < NP; ++c) {
                double a = 0.0;
                for (int k = 0; k < NP; ++k) a = fma(Ys[i * LD + k], X[c * NP + k], a);
                Cs[i * LD + c] = a;
            }
        __syncthreads();
    }
    // forward through the transient
    const double lam1 = row ? sb1[StateBlock::lam(NP) + i] : 0.0, w1 = row ? sb1[StateBlock::wq(NP) + i] : 0.0,
                 sig1 = row ? sb1[StateBlock::sig(NP) + i] : 0.0;
    for (int u = 0; u < m; ++u) {
        const double *x = td.x + (size_t)(t2 + u) * d;
        const bool observed = !isnan(x[0]);
        double cw = 0.0;
        if (row) {
            for (int c = 0; c < NP; ++c) {
                double v = lam1 * sb1[StateBlock::lam(NP) + c] * Cs[i * LD + c];
                if (c == i) v += sig1;
                Cs[i * LD + c] = v;
                cw = fma(v, sb1[StateBlock::wq(NP) + c], cw);
            }
        }
        for (int v = 0; v < kDMax; ++v) M[v] *= lam1;
        if (lane < kDMax + 1) cs[u * (kDMax + 1) + lane] = 0.0;
        if (row) Ks[u * NP + i] = 0.0;
        if (!observed) continue; // (uniform: one frame, one wavefront)
        const double Sv = td.s2[e] + wave_sum(row ? w1 * cw : 0.0);
        const double K = cw / Sv;
        if (row) vs[i] = cw;
        __syncthreads();
        double ev[kDMax];
        for (int v = 0; v < kDMax; ++v) {
            const double pred = wave_sum(row ? w1 * M[v] : 0.0);
            ev[v] = v < nd ? x[td.dims[e][v]] - pred : 0.0;
            M[v] += K * ev[v];
        }
        if (row) {
            for (int c = 0; c < NP; ++c) Cs[i * LD + c] -= K * vs[c];
            Ks[u * NP + i] = K;
        }
        if (lane < kDMax) cs[u * (kDMax + 1) + lane] = ev[lane] / Sv;
        if (lane == kDMax) cs[u * (kDMax + 1) + kDMax] = 1.0;
        __syncthreads();
    }
    __syncthreads();
    // backward: from where the transient is synchronised, through its frames ...
    double g[kDMax];
    for (int v = 0; v < kDMax; ++v) g[v] = row ? tail_g[((rec_n + (t2 + m - 1)) * kDMax + v) * NP + i] : 0.0;
    for (int u = m - 1; u >= 0; --u) {
        const bool observed = cs[u * (kDMax + 1) + kDMax] != 0.0;
        const double K = row ? Ks[u * NP + i] : 0.0;
        for (int v = 0; v < kDMax; ++v) {
            if (observed) {
                const double kg = wave_sum(K * g[v]);
                g[v] = lam1 * (g[v] - w1 * kg) + cs[u * (kDMax + 1) + v] * lam1 * w1;
            } else {
                g[v] *= lam1;
            }
        }
    }
    // ... across the switch, G_0 = X^T h for the factors of the basis change in reverse order ...
    for (int stp = steps - 1; stp >= 0; --stp) {
        const double *X = tab + (size_t)(tab_factored ? (stp == 0 ? s : S + sn) : sn * S + s) * MS;
        __syncthreads();
        for (int v = 0; v < kDMax; ++v)
            if (row) vs[v * NP + i] = g[v];
        __syncthreads();
        for (int v = 0; v < kDMax; ++v) {
            double a = 0.0;
            if (row)
                for (int k = 0; k < NP; ++k) a = fma(X[k * NP + i], vs[v * NP + k], a);
            g[v] = a;
        }
    }
    double *out = stail + (size_t)b * J * kDMax * NP;
    for (int v = 0; v < kDMax; ++v)
        if (row) out[v * NP + i] = g[v];
    // ... and along the switch-free filter of s, frames t2 - 1, t2 - 2, ... (what a frame needs from memory is asked for a chunk ahead)
    const double lam0 = row ? sb0[StateBlock::lam(NP) + i] : 0.0, w0 = row ? sb0[StateBlock::wq(NP) + i] : 0.0;
    const int Wd = NP + 4;
    constexpr int kChunk = 8;
    for (int j0 = 1; j0 < J; j0 += kChunk) {
        double Kb[kChunk], cb[kChunk][kDMax], ob[kChunk];
#pragma unroll
        for (int u = 0; u < kChunk; ++u) {
            const int t = t2 - (j0 + u) >= 1 ? t2 - (j0 + u) : 1;
            const double *r = gain + (rec_s + t) * Wd;
            Kb[u] = r[i];
#pragma unroll
            for (int v = 0; v < kDMax; ++v) cb[u][v] = r[NP + v];
            ob[u] = r[NP + kDMax];
        }
#pragma unroll
        for (int u = 0; u < kChunk; ++u) {
            const int jj = j0 + u;
            if (jj >= J || t2 - jj < 1) break;
#pragma unroll
            for (int v = 0; v < kDMax; ++v) {
                if (ob[u] != 0.0) {
                    const double kg = wave_sum(row ? Kb[u] * g[v] : 0.0);
                    g[v] = lam0 * (g[v] - w0 * kg) + cb[u][v] * lam0 * w0;
                } else {
                    g[v] *= lam0;
                }
                if (row) out[((size_t)jj * kDMax + v) * NP + i] = g[v];
            }
        }
    }
}

} // namespace

int launch_switch_tail(const TrajDesc *d_trajs, int n_traj, int S, int NP, int d, int dstar_max, const double *d_states, const double *d_tab,
                       int tab_factored, const double *d_prefix, const double *d_tail_g, const TransEntry *d_trans, const int64_t *d_first,
                       int64_t total, int J, double *d_gain, double *d_stail, void *stream)
{
    const int64_t blocks = total * (S - 1);
    if (blocks <= 0 || blocks >= ((int64_t)1 << 31) || J < 1 || NP > kMaxNP) return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = (size_t)(2 * NP * (NP + 1) + kDMax * NP + kSwitchTailMaxM * (NP + kDMax + 1)) * sizeof(double);
    hipLaunchKernelGGL(tail_gain_kernel, dim3((unsigned)total), dim3(64), 0, st, d_trajs, n_traj, S, NP, d, dstar_max, d_states, d_prefix, d_first, d_gain);
    hipLaunchKernelGGL(switch_tail_kernel, dim3((unsigned)blocks), dim3(64), lds, st, d_trajs, n_traj, S, NP, d, dstar_max, d_states, d_tab,
                       tab_factored, d_prefix, d_tail_g, d_trans, d_first, d_gain, J, d_stail);
    return (int)hipGetLastError();
}

// tail_g: prefix_records x kDMax x NP doubles; gain: scratch of prefix_records x (NP + 4) doubles; first: n_traj + 1 prefix sums of
// dstar_max * S * T_j (device), total = first[n_traj]
int launch_tail(const TrajDesc *d_trajs, int n_traj, int S, int NP, int d, int dstar_max, const double *d_states, const double *d_prefix,
                const int64_t *d_first, int64_t total, double *d_gain, double *d_tail_g, void *stream)
{
    const int64_t tasks = (int64_t)n_traj * dstar_max * S;
    if (tasks <= 0 || total <= 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tail_gain_kernel, dim3((unsigned)total), dim3(64), 0, st, d_trajs, n_traj, S, NP, d, dstar_max, d_states, d_prefix, d_first, d_gain);
    if (NP <= 16)
        hipLaunchKernelGGL(tail_scan_kernel<16>, dim3((unsigned)tasks), dim3(64), 0, st, d_trajs, n_traj, S, NP, dstar_max, d_states, d_gain, d_tail_g);
    else // (two dimensions per wavefront: two wavefronts per task)
        hipLaunchKernelGGL(tail_scan_kernel<32>, dim3((unsigned)(2 * tasks)), dim3(64), 0, st, d_trajs, n_traj, S, NP, dstar_max, d_states, d_gain, d_tail_g);
    return (int)hipGetLastError();
}

} // namespace bild
