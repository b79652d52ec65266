// Device helpers of one frame of the vector likelihood kernels (logl_body.h): the wave-local LDS fence, the cross-lane sums and
// broadcasts of the block / row / row-pair layouts, the task's one logarithm, and the matrix-times-columns products of a basis
// change.  They hold no state of a task: everything comes in and goes out through arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "common.h"

namespace bild {
namespace {

constexpr double kLog2Pi = 1.8378770664093453;
constexpr double kLn2 = 0.69314718055994531;

// Order LDS traffic between lanes of ONE wavefront: DS instructions of a wave execute in
// issue order, so only the compiler has to be kept from reordering.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sum of one value per lane over the 16 lanes {4b + c + 16k : c, k < 4} that share lane bits 2-3
// ("block" b of v_mfma_f64_4x4x4_4b: operands are laid out as lane = row-or-column + 4*block + 16*k,
// measured with tools/probe/mfma_blocksum.hip), plus `add`; every lane of the block gets the result.
// First product: rows of A summed over k against B = 1; second: the four row sums summed again.
// Two issue slots on the matrix pipe instead of a chain of NP FMAs on the vector pipe.
__device__ __forceinline__ double block_sum16(double v, double add)
{
    const double rows = __builtin_amdgcn_mfma_f64_4x4x4f64(v, 1.0, 0.0, 0, 0, 0);
    return __builtin_amdgcn_mfma_f64_4x4x4f64(rows, 1.0, add, 0, 0, 0);
}

// ROW layout: a task occupies one 16-lane row of the wavefront and lane j of the row owns column j of [C | M].
// gfx950 lets a double-precision VOP2 instruction read its first operand through DPP with the row_newbcast
// controls (lane I of the row broadcast to all 16 lanes), so "acc += x[lane I] * w" is ONE instruction and the
// all-gather of C w through LDS (a write, a wave barrier, NP/2 reads and their latency) disappears from the
// frame loop.  hipcc does not fold a v_mov_b64_dpp into the FMA and does not pad the hazards of an asm
// statement: a DPP source needs two wait states after the VALU instruction that wrote it (dpp_ready).
template <int I>
__device__ __forceinline__ void fmac_bcast(double &acc, double x, double w)
{
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(w), "n"(I));
}
// orders every later reader of x behind two wait states after its producer
__device__ __forceinline__ void dpp_ready(double &x) { asm volatile("s_nop 1" : "+v"(x)); }

// Row PAIR (the two-row frame of the listed loop): rows 2p and 2p + 1 of the wavefront run one task.  v_permlane16_swap exchanges
// the odd rows of its first operand with the even rows of its second; with x as both operands the first result holds the even
// row's x in both rows, the second the odd row's.
__device__ __forceinline__ void pair_swap(double x, double &even, double &odd)
{
    const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
    const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    even = __hiloint2double((int)h[0], (int)l[0]);
    odd = __hiloint2double((int)h[1], (int)l[1]);
}
// the odd rows take x of lane + 1 of their row, the even rows keep their own (DPP row_shl:1, written in the odd rows only)
__device__ __forceinline__ double odd_rows_shift(double x)
{
    const int lo = __double2loint(x), hi = __double2hiint(x);
    const int l = __builtin_amdgcn_update_dpp(lo, lo, 0x101, 0xA, 0xF, false);
    const int h = __builtin_amdgcn_update_dpp(hi, hi, 0x101, 0xA, 0xF, false);
    return __hiloint2double(h, l);
}

template <int NP, int I = 0>
struct RowOps {
    // sa += sum over even i of x[lane i] w[i], sb likewise over odd i (the order of the packed layouts)
    static __device__ __forceinline__ void dot(double &sa, double &sb, double x, const double (&w)[NP])
    {
        fmac_bcast<I>(sa, x, w[I]);
        fmac_bcast<I + 1>(sb, x, w[I + 1]);
        RowOps<NP, I + 2>::dot(sa, sb, x, w);
    }
    // col[i] += x[lane i] * c
    static __device__ __forceinline__ void rank1(double (&col)[NP], double x, double c)
    {
        fmac_bcast<I>(col[I], x, c);
        fmac_bcast<I + 1>(col[I + 1], x, c);
        RowOps<NP, I + 2>::rank1(col, x, c);
    }
};
template <int NP>
struct RowOps<NP, NP> {
    static __device__ __forceinline__ void dot(double &, double &, double, const double (&)[NP]) {}
    static __device__ __forceinline__ void rank1(double (&)[NP], double, double) {}
};
// the same for a row of a PAIR, which holds entries 2k + (row odd) as its entry k: x is the row's (C w) as shifted by
// odd_rows_shift, so that lane 2k of the row holds entry 2k + (row odd) in both rows
template <int NP, int K = 0>
struct PairOps {
    // s += sum over the row's entries i of x[i] w[i], i ascending (sa of RowOps::dot in the even row, sb in the odd one)
    static __device__ __forceinline__ void dot(double &s, double x, const double (&w)[NP])
    {
        fmac_bcast<2 * K>(s, x, w[K]);
        PairOps<NP, K + 1>::dot(s, x, w);
    }
    static __device__ __forceinline__ void rank1(double (&col)[NP / 2], double x, double c)
    {
        fmac_bcast<2 * K>(col[K], x, c);
        PairOps<NP, K + 1>::rank1(col, x, c);
    }
};
template <int NP>
struct PairOps<NP, NP / 2> {
    static __device__ __forceinline__ void dot(double &, double, const double (&)[NP]) {}
    static __device__ __forceinline__ void rank1(double (&)[NP / 2], double, double) {}
};

// log() is needed once per task; out of line, so that its polynomial constants are not hoisted
// out of the task loop into registers the frame loop then has to spill around.
__device__ __attribute__((noinline)) double log_once(double x) { return log(x); }

// The log-likelihood of a piece from its sums: tot = sum over the dimensions of sum_t e_t^2 / S_t, the product of the S_t as P x 2^E, nv
// observed frames, nd dimensions (reference bild/src/MSRouse_logL.pyx:250-254 summed over frames).  One place for the arithmetic of
// the task loop (piece_value) and of the pass that fills the running log-likelihoods of the prefix table (prefix_L_kernel).
__device__ __forceinline__ double piece_from_sums(double tot, double P, int E, int nv, int nd)
{
    const double logS = log_once(P) + (double)E * kLn2;
    tot += (double)nd * (logS + (double)nv * kLog2Pi);
    return -0.5 * tot;
}

template <int NP, int CPL>
struct Cols {
    double v[CPL][NP];
};

// Tg[c][i] = sum_k X[i][k] * in[q][k]  for the own columns c = cidx[q]: the product X * A is
// streamed column-major into the group's LDS image Tg (NC columns of NP doubles), two rows at
// a time, so no second register image of A is needed.  X is row-major in LDS (dense propagator
// or modal basis change); one X operand pair feeds 2*CPL FMAs.
template <int NP, int CPL, bool ROOMY = false, typename XPtr>
__device__ __forceinline__ void matvec_to_lds(XPtr X, const Cols<NP, CPL> &in, double *__restrict__ Tg,
                                              const int (&cidx)[CPL], const bool (&store)[CPL])
{
    // rows per trip: two give each X operand pair 2*CPL independent FMAs; with a single column per
    // lane one row at a time keeps the operand registers of this (rare) path out of the budget of
    // the frame loop -- unless the geometry has registers to spare (ROOMY: two waves per SIMD, the frame loop over the
    // work lists, where a basis change is 2.6 us = nine frames of a chain): then two rows per trip, two trips in flight
    if constexpr (ROOMY && CPL == 1) {
        // Hand-scheduled (round 4).  Left to itself the compiler reads the five 16-byte pieces of a matrix row, WAITS for all
        // of them, runs the row's ten FMAs, and only then asks for the next row: ten LDS latencies per product, 2.2 us per
        // basis change -- ten frames' worth, paid two or three times by every chain that ends a launch.  Here the two rows of
        // trip i + 1 are asked for BEFORE the FMAs of trip i (two register sets, 40 VGPRs: the frame loop's L / sgd / wq are
        // dead across a basis change), and scheduling barriers keep the order: the product is then bound by its hundred FMAs.
        // Every accumulator sees its terms in the order of the loop below (k ascending, even and odd k apart): bit-identical.
        constexpr int H = NP / 2;
        double2 cur[2][H], nxt[2][H];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k2 = 0; k2 < H; ++k2) cur[r][k2] = *reinterpret_cast<const double2 *>(X + r * NP + 2 * k2);
#pragma unroll
        for (int i = 0; i < NP; i += 2) {
            if (i + 2 < NP) {
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int k2 = 0; k2 < H; ++k2) nxt[r][k2] = *reinterpret_cast<const double2 *>(X + (i + 2 + r) * NP + 2 * k2);
            }
            __builtin_amdgcn_sched_barrier(0);
            double a[2] = {0.0, 0.0}, a2[2] = {0.0, 0.0};
#pragma unroll
            for (int k2 = 0; k2 < H; ++k2)
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    a[r] = fma(cur[r][k2].x, in.v[0][2 * k2], a[r]);
                    a2[r] = fma(cur[r][k2].y, in.v[0][2 * k2 + 1], a2[r]);
                }
            a[0] += a2[0];
            a[1] += a2[1];
            if (store[0]) *reinterpret_cast<double2 *>(Tg + cidx[0] * NP + i) = make_double2(a[0], a[1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k2 = 0; k2 < H; ++k2) cur[r][k2] = nxt[r][k2];
        }
        return;
    }
    constexpr int R = (CPL == 1 && !ROOMY) ? 1 : 2;
    constexpr int kTrips = ROOMY ? NP / 2 : 1; // (ROOMY: the whole product unrolled, so that the LDS reads of the matrix run ahead of the FMAs)
#pragma unroll kTrips
    for (int i = 0; i < NP; i += R) {
        double a[R][CPL], a2[R][CPL]; // even / odd k: two dependent chains per output instead of one
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < CPL; ++q) a[r][q] = a2[r][q] = 0.0;
#pragma unroll
        for (int k = 0; k < NP; k += 2) {
            double2 x[R];
#pragma unroll
            for (int r = 0; r < R; ++r) x[r] = *reinterpret_cast<const double2 *>(X + (i + r) * NP + k);
#pragma unroll
            for (int q = 0; q < CPL; ++q)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    a[r][q] = fma(x[r].x, in.v[q][k], a[r][q]);
                    a2[r][q] = fma(x[r].y, in.v[q][k + 1], a2[r][q]);
                }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < CPL; ++q) a[r][q] += a2[r][q];
#pragma unroll
        for (int q = 0; q < CPL; ++q)
            if (store[q]) {
                if (R == 2)
                    *reinterpret_cast<double2 *>(Tg + cidx[q] * NP + i) = make_double2(a[0][q], a[R - 1][q]);
                else
                    Tg[cidx[q] * NP + i] = a[0][q];
            }
    }
}

// The same product for a row of a PAIR: out[k] = sum_m X[2k + odd][m] * in[m], the outputs this row keeps (X points at row `odd` of the
// matrix).  One matrix row per trip, the row of trip k + 1 asked for in front of the FMAs of trip k (two register sets of NP doubles),
// every output formed as above -- one accumulator over even m, one over odd m, m ascending, then their sum: the same bits.  STORE: the
// outputs of the lanes with `store` also go to Tg[2k] (Tg points at entry `odd` of the lane's column in the pair's image).
template <int NP, bool STORE, typename XPtr>
__device__ __forceinline__ void matvec_pair(XPtr X, const double (&in)[NP], double (&out)[NP / 2], double *__restrict__ Tg, bool store)
{
    static_assert(NP % 2 == 0, "a row of a pair holds every second entry");
    constexpr int H = NP / 2;
    double2 cur[H], nxt[H];
#pragma unroll
    for (int k2 = 0; k2 < H; ++k2) cur[k2] = *reinterpret_cast<const double2 *>(X + 2 * k2);
#pragma unroll
    for (int k = 0; k < H; ++k) {
        if (k + 1 < H) {
#pragma unroll
            for (int k2 = 0; k2 < H; ++k2) nxt[k2] = *reinterpret_cast<const double2 *>(X + 2 * (k + 1) * NP + 2 * k2);
        }
        __builtin_amdgcn_sched_barrier(0);
        double a = 0.0, a2 = 0.0;
#pragma unroll
        for (int k2 = 0; k2 < H; ++k2) {
            a = fma(cur[k2].x, in[2 * k2], a);
            a2 = fma(cur[k2].y, in[2 * k2 + 1], a2);
        }
        out[k] = a + a2;
        if constexpr (STORE) {
            if (store) Tg[2 * k] = out[k];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k2 = 0; k2 < H; ++k2) cur[k2] = nxt[k2];
    }
}

} // namespace
} // namespace bild
