// Counter-based Philox-4x32-10 (Salmon et al., SC'11), shared by the five device-side draws: the AMIS samples
// (amis_device.hip: draw_kernel), the Rouse trajectories (sim.hip), the GenericGaussianModel trajectories (gauss.hip:
// gauss_sim_normals_kernel), the exact profile draws (gauss_segdraw.hip) and the dwell-time profile draws
// (gauss_dwelldraw.hip).  Their counter layouts are part of the C ABI's contract (include/bild_amd.h) and are held to a
// host statement of this file, tests/philox_oracle.py, by tests/test_gpu_device_streams.py.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bild {

// one block: 4 x 32 random bits, a pure function of the counter (c0..c3) and the key (k0, k1)
__device__ inline void philox4x32_10(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * x0, p1 = (uint64_t)0xCD9E8D57u * x2;
        const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y1 = (uint32_t)p1, y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1, y3 = (uint32_t)p0;
        x0 = y0;
        x1 = y1;
        x2 = y2;
        x3 = y3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = x0;
    out[1] = x1;
    out[2] = x2;
    out[3] = x3;
}

// uniform in [0, 1) with 53 random bits from two words
__device__ inline double philox_uniform(uint32_t hi, uint32_t lo)
{
    const uint64_t bits = ((uint64_t)hi << 32) | lo;
    return (double)(bits >> 11) * 0x1p-53;
}

// both normals of one Box-Muller pair from one block
__device__ inline void philox_normal_pair(const uint32_t out[4], double *n0, double *n1)
{
    const double u1 = 1.0 - philox_uniform(out[0], out[1]), u2 = philox_uniform(out[2], out[3]); // u1 in (0, 1]
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    *n0 = r * c;
    *n1 = r * s;
}

// A stream of one (seed, stream, sample): the block counter is the fourth word.  Uniforms are taken two per block, the
// second word pair first; normal() is one Box-Muller value per two uniforms (the draws of amis_device.hip).
struct Philox {
    uint32_t c[4], k[2];
    uint32_t out[4];
    int have;
    __device__ Philox(uint64_t seed, uint64_t stream, uint64_t sample)
    {
        c[0] = (uint32_t)sample;
        c[1] = (uint32_t)(sample >> 32);
        c[2] = (uint32_t)stream;
        c[3] = 0; // block counter of this stream
        k[0] = (uint32_t)seed;
        k[1] = (uint32_t)(seed >> 32);
        have = 0;
    }
    __device__ void block()
    {
        philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1], out);
        ++c[3];
        have = 2;
    }
    // uniform in [0, 1) with 53 random bits
    __device__ double uniform()
    {
        if (!have) block();
        --have;
        return philox_uniform(out[2 * have], out[2 * have + 1]);
    }
    __device__ double normal() // Box-Muller, one of the pair
    {
        const double u1 = 1.0 - uniform(), u2 = uniform(); // u1 in (0, 1]
        return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
    }
    __device__ double gamma(double a)
    {
        if (!(a > 0)) return 0.0;
        double boost = 1.0;
        if (a < 1.0) { // gamma(a) = gamma(a + 1) U^(1/a)
            boost = pow(1.0 - uniform(), 1.0 / a);
            a += 1.0;
        }
        const double d = a - 1.0 / 3.0, cc = 1.0 / sqrt(9.0 * d);
        for (int it = 0; it < 64; ++it) { // (acceptance > 95 % per trial)
            const double x = normal(), t = 1.0 + cc * x;
            if (t <= 0) continue;
            const double v = t * t * t, u = 1.0 - uniform();
            if (u < 1.0 - 0.0331 * (x * x) * (x * x) || log(u) < 0.5 * x * x + d * (1.0 - v + log(v))) return boost * d * v;
        }
        return boost * d;
    }
};

} // namespace bild
