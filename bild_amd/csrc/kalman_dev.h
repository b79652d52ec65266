// Device helpers of the modal Kalman kernels (kalman.hip: filter and smoother, sens.hip: forward sensitivities).  One task
// = (candidate, covariance chain) on L lanes of one wavefront; lane i owns row i of a symmetric L x L matrix.  Private to
// the library.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace bild {
namespace {

constexpr double kLog2Pi = 1.8378770664093453;

// Order LDS traffic between lanes of ONE wavefront: DS instructions of a wave execute in issue order, so only the
// compiler has to be kept from reordering.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum over the L lanes of a task; every lane gets the same bits (each butterfly stage adds the same two numbers)
template <int L> __device__ __forceinline__ double task_sum(double v)
{
#pragma unroll
    for (int off = L / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double pick(const double (&a)[kDMax], int k)
{
    return k == 0 ? a[0] : k == 1 ? a[1] : a[2];
}

// X <- A X A^T for a symmetric X (lane i holds row i), A = Q (tr false) or Q^T (tr true) of one state (L x L, row-major):
// first Z = A X, then A Z^T = A X A^T.  buf: the task's L x (L + 1) LDS block.
template <int L> __device__ void conj_sym(double (&X)[L], const double *__restrict__ Q, bool tr, double *buf, int i)
{
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        wave_lds_fence();
#pragma unroll
        for (int c = 0; c < L; ++c) buf[i * (L + 1) + c] = X[c];
        wave_lds_fence();
        double acc[L];
#pragma unroll
        for (int c = 0; c < L; ++c) acc[c] = 0.0;
        for (int a = 0; a < L; ++a) {
            const double ai = tr ? Q[a * L + i] : Q[i * L + a];
#pragma unroll
            for (int c = 0; c < L; ++c) acc[c] = fma(ai, pass == 0 ? buf[a * (L + 1) + c] : buf[c * (L + 1) + a], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < L; ++c) X[c] = acc[c];
    }
}

// v <- A v for kDMax columns (lane i holds row i)
template <int L> __device__ void apply_vec(double (&v)[kDMax], const double *__restrict__ Q, bool tr, double *buf, int i)
{
    wave_lds_fence();
#pragma unroll
    for (int k = 0; k < kDMax; ++k) buf[i * (L + 1) + k] = v[k];
    wave_lds_fence();
    double acc[kDMax] = {0.0, 0.0, 0.0};
    for (int a = 0; a < L; ++a) {
        const double ai = tr ? Q[a * L + i] : Q[i * L + a];
#pragma unroll
        for (int k = 0; k < kDMax; ++k) acc[k] = fma(ai, buf[a * (L + 1) + k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < kDMax; ++k) v[k] = acc[k];
}

} // namespace
} // namespace bild
