// What the kernels of the exact-inference calls share (gauss_segdp.hip, gauss_segdraw.hip, gauss_segsens.hip, gauss_dwell.hip,
// gauss_dwelldraw.hip, gauss_dwellsens.hip, gauss_dwellfilt.hip): the two constants, the reductions and scans across the 64 lanes of a
// wavefront, the running sums of exponentials of the dwell-time recursion, the step of an inverse-CDF pick, the carry of the
// marginals and the uniforms of a draw.  Every function does its operations in one fixed
// order, so a kernel that calls it sums as the others do.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bild {

__device__ __forceinline__ double neg_inf() { return __longlong_as_double(0xfff0000000000000ll); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// butterflies over the wave, partners 32 lanes apart first: every lane gets the result
template <class X> __device__ __forceinline__ X wave_sum(X v)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double wave_max(double v)    // no NaN among them
{
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// inclusive scan: lane l gets the terms of the lanes <= l
__device__ __forceinline__ double wave_scan_up(double v, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const double dn = __shfl_up(v, off, 64);
        if (lane >= off) v += dn;
    }
    return v;
}

// suffix sum: lane l gets the terms of the lanes >= l
__device__ __forceinline__ double wave_scan_down(double v, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const double up = __shfl_down(v, off, 64);
        if (lane + off < 64) v += up;
    }
    return v;
}

// ---- sums of exponentials kept as (m, z): the sum is z exp(m) (gauss_dwell.hip, gauss_dwellfilt.hip) ----
// (m, z) += exp(t): z counts in units of exp(m)
__device__ __forceinline__ void lse_add(double &m, double &z, double t)
{
    if (!(t > neg_inf())) return;
    if (t > m) {
        z = z * exp(m - t) + 1.0;
        m = t;
    } else {
        z += exp(t - m);
    }
}

// (m, z) of two sums; the same bits whichever side is called first
__device__ __forceinline__ void lse_merge(double &m, double &z, double m2, double z2)
{
    const double top = fmax(z > 0.0 ? m : neg_inf(), z2 > 0.0 ? m2 : neg_inf());
    if (!(top > neg_inf())) {
        m = neg_inf(), z = 0.0;
        return;
    }
    const double u = z > 0.0 ? z * exp(m - top) : 0.0, v = z2 > 0.0 ? z2 * exp(m2 - top) : 0.0;
    m = top;
    z = u + v;
}

__device__ __forceinline__ double lse_value(double m, double z) { return z > 0.0 ? m + log(z) : neg_inf(); }

// lse_add with a second sum on the same scale: r counts len * exp(t) in units of exp(m) and is rescaled together with z
__device__ __forceinline__ void lse_add_len(double &m, double &z, double &r, double t, double len)
{
    if (!(t > neg_inf())) return;
    if (t > m) {
        const double e = exp(m - t);
        z = z * e + 1.0;
        r = r * e + len;
        m = t;
    } else {
        const double e = exp(t - m);
        z += e;
        r += len * e;
    }
}

// The wave's inverse-CDF pick among the entries b = lo .. hi of a list (lo >= 1), walked in blocks of 64 ascending b, lane = b;
// weight(b) is the entry's weight, >= 0.  The first b of positive weight whose running total, continued from `base`, exceeds
// `target`; 0 if the list ends before, and then `base` and `last` (the last b of positive weight) are carried on.
template <class Weight>
__device__ __forceinline__ int wave_pick(int lo, int hi, double target, int lane, double &base, int &last, Weight weight)
{
    for (int b0 = lo; b0 <= hi; b0 += 64) {
        const int b = b0 + lane;
        const double e = b <= hi ? weight(b) : 0.0;
        double c = wave_scan_up(e, lane);
        c += base;
        const unsigned long long pos = __ballot(e > 0.0), hit = __ballot(e > 0.0 && c > target);
        if (hit) return __builtin_amdgcn_readfirstlane(b0 + __ffsll((long long)hit) - 1);
        if (pos) last = b0 + 63 - __clzll((long long)pos);
        base = __shfl(c, 63, 64);
    }
    return 0;
}

// The carry of the marginals, one wave per tile of 64 frames t of one table row: post(t) = cover(t) + the sum over the rows
// a <= t of the totals of the tiles to the right of t's.  row_tot holds per (tile, a) the total of row a inside the tile, Tm
// entries a tile; cover and post are the row's frames.
__device__ __forceinline__ void wave_carry(const double *__restrict__ row_tot, const double *__restrict__ cover, double *__restrict__ post,
                                           int T, int Tm, int tile, bool live, int lane)
{
    const int t = tile * 64 + lane;
    const int ntile = (T + 63) / 64;
    double carry = 0.0;
    for (int blk = 0; live && blk <= tile; ++blk) {
        const int a = blk * 64 + lane;
        double v = 0.0;
        if (a < T)
            for (int r = tile + 1; r < ntile; ++r) v += row_tot[(int64_t)r * Tm + a];
        // rows left of the tile count for all of its frames; row a of the tile itself counts for the frames t >= a
        if (blk < tile) v = wave_sum(v);
        else v = wave_scan_up(v, lane);
        carry += v;
    }
    if (t < T) post[t] = cover[t] + carry;
}

// after a launch: 0, or 1 if it was refused
inline int launched() { return hipGetLastError() == hipSuccess ? 0 : 1; }

} // namespace bild
