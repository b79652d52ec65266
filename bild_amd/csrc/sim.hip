// The Rouse trajectory generator (bild_rouse_simulate, sim.cpp): MultiStateRouse.trajectories_from_loopingprofiles.
//
// Every state s has one orthonormal eigenbasis V_s with B = V diag(b) V^T, LSig = V diag(sqrt sig), LC0 = V diag(sqrt cinf)
// (rouse.Model.update_dynamics), so in the modal coordinates x' = V_s^T x of the state in force the CPU step
// conf <- B conf + G + LSig xi is N independent scalar recurrences on the same normals xi:
//     x'_j <- b_j x'_j + (V^T G)_j + sqrt(sig_j) xi_j,        steady state  x'_j = (V^T M0)_j + sqrt(cinf_j) xi_j,
// the measurement is y = (V^T w) . x', and a switch is one basis change x' <- V_new^T (V_old x').  DESIGN.md section 11.
//
// Layout: one workgroup per (trajectory, group of dimensions), one lane per (mode j, dimension k), lane = j * dpb + kk --
// so the replay normals of a frame (mode-major, dimension-minor as NumPy draws them) are read contiguously.  The
// per-lane constants of the state in force live in registers and are reloaded at a switch; V is read through L2 at a
// switch only.  Every lane writes u_j x'_j for a chunk of frames into LDS; after the chunk one transposed pass sums each
// (frame, dimension) over the modes in mode order, adds the localization noise and writes the rows coalesced.  Results
// depend on (N, d) and the inputs only, not on the batch or the launch.
//
// Device mode: the normal of (trajectory index i in the call, frame t, mode j, dimension k) is one of the Box-Muller pair
// of the Philox-4x32-10 block with key = seed, counter = (i, t / 2, 16 j + k, 0) -- frame t even takes the cosine, t odd
// the sine; the localization noise of (i, t, k) likewise from counter (i, t / 2, 2^31 + k, 0).
#include <hip/hip_runtime.h>

#include "philox.h"
#include "sim.h"

namespace bild {

namespace {

// lanes of a workgroup (a multiple of 64) and its dynamic LDS: the chunk's rows, then x' and V_old x' of a basis change
int sim_block_threads(int N, int dpb) { return (N * dpb + 63) / 64 * 64; }

size_t sim_lds_bytes(int N, int dpb, int chunk)
{
    const size_t L = (size_t)N * dpb;
    return ((size_t)chunk * (L + 1) + 2 * L) * sizeof(double);
}

constexpr uint32_t kNoiseStream = 0x80000000u;

__global__ void __launch_bounds__(kSimMaxLanes) rouse_sim_kernel(SimParams p)
{
    extern __shared__ double lds[];
    const int N = p.N, d = p.d, dpb = p.dpb, C = p.chunk;
    const int L = N * dpb, stride = L + 1;
    double *buf = lds;                              // C rows of `stride`: u_j x'_j of every lane
    double *xs = lds + (size_t)C * stride;          // basis change: x' and V_old x'
    double *zs = xs + L;

    const int i = blockIdx.x;
    const int k0 = blockIdx.y * dpb, dd = min(dpb, d - k0);
    const int l = threadIdx.x, j = l / dpb, kk = l - j * dpb, k = k0 + kk;
    const bool active = l < L && kk < dd;
    const uint32_t gi = (uint32_t)(p.first + i);
    const int T = p.T[i];
    const int64_t row0 = p.frame_off[i];
    const int32_t *seg_start = p.seg_start + (size_t)i * p.K1, *seg_state = p.seg_state + (size_t)i * p.K1;
    const double *z = p.z ? p.z + (p.z_off[i] - p.z_first) : nullptr;
    const size_t zrow = (size_t)N * d;

    int cur = seg_state[0], si = 0;
    double b = 0, sg = 0, g = 0, u = 0;
    auto load = [&](int s) {
        if (!active) return;
        b = p.b[(size_t)s * N + j];
        sg = p.ssig[(size_t)s * N + j];
        g = p.g[((size_t)s * N + j) * d + k];
        u = p.u[(size_t)s * N + j];
    };
    load(cur);

    double x = 0, xi_next = 0;
    for (int t0 = 0; t0 < T; t0 += C) {
        const int nf = min(C, T - t0);
        for (int f = 0; f < nf; ++f) {
            const int t = t0 + f;
            if (t > 0) {        // the segment in force (uniform over the workgroup)
                while (si + 1 < p.K1 && seg_start[si + 1] <= t) ++si;
                const int s = seg_state[si];
                if (s != cur) { // x' <- V_s^T (V_cur x')
                    if (active) xs[l] = x;
                    __syncthreads();
                    if (active) {
                        const double *Vt = p.Vt + (size_t)cur * N * N;
                        double acc = 0;
                        for (int m = 0; m < N; ++m) acc = fma(Vt[(size_t)m * N + j], xs[m * dpb + kk], acc);
                        zs[l] = acc;
                    }
                    __syncthreads();
                    if (active) {
                        const double *V = p.V + (size_t)s * N * N;
                        double acc = 0;
                        for (int m = 0; m < N; ++m) acc = fma(V[(size_t)m * N + j], zs[m * dpb + kk], acc);
                        x = acc;
                    }
                    cur = s;
                    load(cur);
                }
            }
            if (active) {
                double xi;
                if (z) {
                    xi = z[(size_t)t * zrow + (size_t)j * d + k];
                } else if ((t & 1) == 0) {
                    uint32_t r[4];
                    philox4x32_10(gi, (uint32_t)(t >> 1), (uint32_t)(16 * j + k), 0u, (uint32_t)p.seed, (uint32_t)(p.seed >> 32), r);
                    philox_normal_pair(r, &xi, &xi_next);
                } else {
                    xi = xi_next;
                }
                if (t == 0) x = p.m0[((size_t)cur * N + j) * d + k] + p.scinf[(size_t)cur * N + j] * xi;
                else x = b * x + g + sg * xi;
                buf[f * stride + l] = u * x;
            }
        }
        __syncthreads();
        // rows: two frames of one dimension per task (the two values of a localization-noise pair)
        for (int task = l; task < (C / 2) * dd; task += blockDim.x) {
            const int q = task / dd, kq = task - q * dd, f0 = 2 * q, kd = k0 + kq;
            if (f0 >= nf) continue;
            const int t = t0 + f0;
            double e0, e1;
            if (z) {
                const double *zn = z + (size_t)T * zrow;
                e0 = zn[(size_t)t * d + kd];
                e1 = f0 + 1 < nf ? zn[(size_t)(t + 1) * d + kd] : 0.0;
            } else {
                uint32_t r[4];
                philox4x32_10(gi, (uint32_t)(t >> 1), kNoiseStream + (uint32_t)kd, 0u, (uint32_t)p.seed, (uint32_t)(p.seed >> 32), r);
                philox_normal_pair(r, &e0, &e1);
            }
            const double err = p.err[(size_t)i * d + kd];
            for (int e = 0; e < 2 && f0 + e < nf; ++e) {
                const double *row = buf + (f0 + e) * stride + kq;
                double y = 0;
                for (int m = 0; m < N; ++m) y += row[m * dpb];
                const int64_t r = row0 + t + e;
                p.out[r * d + kd] = p.missing[r] ? __builtin_nan("") : y + err * (e ? e1 : e0);
            }
        }
        __syncthreads();
    }
}

} // namespace

int launch_rouse_simulate(const SimParams &p, void *stream)
{
    if (p.n <= 0) return 0;
    const dim3 grid((unsigned)p.n, (unsigned)((p.d + p.dpb - 1) / p.dpb));
    hipLaunchKernelGGL(rouse_sim_kernel, grid, dim3(sim_block_threads(p.N, p.dpb)), sim_lds_bytes(p.N, p.dpb, p.chunk),
                       (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

} // namespace bild
