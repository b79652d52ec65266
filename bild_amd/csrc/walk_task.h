// The table walk of one task (walk.hip: walk_kernel; kernels.hip: logl_one_kernel, the walk and the listed frame loop in one
// launch): one copy of the code for both paths.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>

#include "chain_work.h"
#include "common.h"

namespace bild {

// K1 = segments per candidate, a compile-time constant: every loop over the list unrolls without a trip-count test in
// between, so that the loads of the list go out back to back (with the test, each pair of loads was waited for before
// the next was issued: K1 memory round trips instead of one).
// returns the work-list bucket of a task that goes on to the frame loop, -1 for a task that is done
// `hand` (the one-launch path, kernels.hip: logl_one_kernel) sees what a task that goes on to the frame loop has worked out:
// its list, which entries are switches, the plan of the frame loop per entry (the same expressions as kernels.hip: the walk plan),
// the running sum in front of the first switch and the expected frames; walk.hip passes a hook that does nothing.
template <int KMAX, bool ST, typename Hand>
__device__ __forceinline__ int walk_task(const WalkParams &p, const int64_t task, Hand &&hand)
{
    constexpr int K1 = KMAX;
    const int64_t r = task / p.dstar_max;
    const int e = (int)(task - r * p.dstar_max);
    const int S = p.S;
    const int tj = p.traj_id ? p.traj_id[r] : 0;
    const TrajDesc *__restrict__ td = p.trajs + tj;
    const int T = td->T;

    // ---- the segment list -----------------------------------------------------------------------------------------
    int a[KMAX], b[KMAX];
    bool ok = true;
    if constexpr (ST) {
        const double *__restrict__ s = p.ss + r * K1;
        const uint8_t *__restrict__ th = reinterpret_cast<const uint8_t *>(p.thetas) + r * K1;
        const double Tm1 = (double)(T - 1);
        double acc = 0.0;
        int prev = 0;
#pragma unroll
        for (int i = 0; i < KMAX; ++i) {
            a[i] = INT_MAX;
            b[i] = 0;
        }
#pragma unroll
        for (int i = 0; i < KMAX; ++i) {
            if (i < K1) {
                const int st = th[i];
                ok = ok && st < S;
                b[i] = st;
                if (i == 0) a[0] = 0;
                if (i + 1 < K1) {
                    acc = __dadd_rn(acc, s[i]);            // np.cumsum: sequential
                    const double pos = __dmul_rn(acc, Tm1); // one multiplication, not fused with the sum
                    // floor for 0 <= pos < 2^31 is the truncating conversion; as on the host (api.cpp: st_row) a negative
                    // position -- where truncation and np.floor differ -- and NaN are refused
                    const bool in_range = pos >= 0.0 && pos < 2147483646.0;
                    const int idx = in_range ? (int)pos + 1 : INT_MAX;
                    ok = ok && in_range && idx >= prev;
                    prev = idx;
                    if (i + 1 < KMAX) a[i + 1] = idx;
                }
            }
        }
        if (!ok) {
            // not a point on the simplex (or a state out of range): nothing of this row drives an address
            if (atomicCAS(p.status, 0, 1) == 0) p.status[1] = (int)(r < INT_MAX ? r : INT_MAX);
            if (!p.convert_all) {
                p.out[task] = __longlong_as_double(0x7ff8000000000000ll);
            } else if (e == 0) {
                // every list goes on to the frame loop: the refused row gets one without a switch (nothing of the row drives an
                // address there either), marked by a negative first start -- a start no kernel reads, segment 0 owns frame 0 --,
                // and its result is replaced by NaN behind the frame loop (mark_refused_rows_kernel)
#pragma unroll
                for (int i = 0; i < KMAX; ++i)
                    if (i < K1) {
                        p.seg_out_start[r * K1 + i] = i == 0 ? -1 : INT_MAX;
                        p.seg_out_state[r * K1 + i] = 0;
                    }
            }
            return -1;
        }
    } else {
        const int32_t *__restrict__ sst = p.seg_start + r * K1;
        const int32_t *__restrict__ ssv = p.seg_state + r * K1;
#pragma unroll
        for (int i = 0; i < KMAX; ++i) {
            a[i] = INT_MAX;
            b[i] = 0;
            if (i < K1) {
                a[i] = sst[i];
                b[i] = ssv[i];
            }
        }
    }
    // (every chain of a candidate that goes on to the frame loop writes the candidate's list: the same values)
    auto write_list = [&]() {
        if constexpr (ST) {
#pragma unroll
            for (int i = 0; i < KMAX; ++i)
                if (i < K1) {
                    p.seg_out_start[r * K1 + i] = a[i];
                    p.seg_out_state[r * K1 + i] = b[i];
                }
        }
    };
    if (p.convert_all) {
        if (e == 0) write_list();
        return -1;
    }
    if (e >= td->dstar) {
        p.out[task] = 0.0;
        return -1;
    }

    // ---- cleaned list, without moving anything: which entries are switches, and what lies behind each ---------------
    // (the cleaning rule of kernels.hip: an entry at or beyond the trajectory's end ends the list; an empty segment and
    // a segment in the state of its predecessor are no switches)
    unsigned keep = 1u;   // bit i: entry i is a real switch (bit 0: the initial segment)
    int sprev[KMAX];      // state in front of entry i
    {
        int prev = b[0];
        bool dead = false;
#pragma unroll
        for (int i = 1; i < KMAX; ++i) {
            sprev[i] = prev;
            if (i < K1) {
                const int end = (i + 1 < K1 && i + 1 < KMAX) ? a[i + 1] : INT_MAX;
                dead = dead || a[i] >= T;
                if (!dead && end > a[i] && b[i] != prev) {
                    keep |= 1u << i;
                    prev = b[i];
                }
            }
        }
    }
    int n2[KMAX], sm[KMAX], n4[KMAX]; // behind switch i: start and state of the next switch, start of the one after
    int first = T;                    // first switch, or T
    {
        int nxt_t = INT_MAX, nxt_s = 0, nxt2_t = INT_MAX;
#pragma unroll
        for (int i = KMAX - 1; i >= 1; --i) {
            n2[i] = nxt_t;
            sm[i] = nxt_s;
            n4[i] = nxt2_t;
            if (keep & (1u << i)) {
                nxt2_t = nxt_t;
                nxt_t = a[i];
                nxt_s = b[i];
            }
        }
        if (nxt_t < T) first = nxt_t;
    }

    // ---- everything the walk may need, for all switches at once ------------------------------------------------------
    // Loads of a group of switches are issued together, unconditionally and without a branch in between (a switch that
    // is none reads entry 0 of the tables): one memory round trip per group instead of one per switch.
    const int64_t rec_e = td->prefix_rec0 + (int64_t)e * S * T; // records of chain e: + state * T + frame
    const int64_t tr_e = td->trans0 + (int64_t)e * S * S * T;   // entries of chain e: + (s * S + sn) * T + frame
    const double *__restrict__ Lc = p.Lc + rec_e;
    const TransEntry *__restrict__ tr1 = p.trans + tr_e;
    const bool pairs = p.trans2 != nullptr && !(p.debug & 1);
    const TransEntry *__restrict__ tr2 = pairs ? p.trans2 : p.trans; // (no pair table: the loads still need an address)
    const int64_t tr2_e = pairs ? (td->trans0 * S + (int64_t)e * S * S * S * T) * p.gap_max : 0;
    double v1[KMAX], v2[KMAX];
    int m1[KMAX], m2[KMAX];
    double extra = Lc[(int64_t)b[0] * T + (first - 1)];
    constexpr int kGroup = 5;
    if (p.debug & 4) {
        p.out[task] = extra;
        return -1;
    }
#pragma unroll
    for (int g0 = 1; g0 < KMAX; g0 += kGroup) {
        TransEntry en[kGroup], e2[kGroup];
        double la[kGroup], lb[kGroup], l2[kGroup], l4[kGroup];
        bool pair_ok[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            const int i = g0 + j;
            if (i < KMAX) {
                const bool kp = (keep >> i) & 1u;
                const int ti = kp ? a[i] : 1, s0 = kp ? sprev[i] : 0, s1 = kp ? b[i] : 0;
                const int t3 = (kp && n2[i] < T) ? n2[i] : T;
                pair_ok[j] = kp && pairs && n2[i] < T && n2[i] - ti < p.gap_max;
                const int smj = pair_ok[j] ? sm[i] : 0;
                const int t4 = (pair_ok[j] && n4[i] < T) ? n4[i] : T;
                const int64_t i2 = pair_ok[j] ? tr2_e + ((((int64_t)s0 * S + s1) * S + smj) * T + ti) * p.gap_max + (n2[i] - ti) : 0;
                en[j] = tr1[((int64_t)s0 * S + s1) * T + ti];
                la[j] = Lc[(int64_t)s1 * T + (ti - 1)];
                lb[j] = Lc[(int64_t)s1 * T + (t3 - 1)];
                e2[j] = tr2[i2];
                l2[j] = Lc[(int64_t)smj * T + (ti - 1)];
                l4[j] = Lc[(int64_t)smj * T + (t4 - 1)];
            }
        }
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
            const int i = g0 + j;
            if (i < KMAX) {
                const bool kp = (keep >> i) & 1u;
                v1[i] = en[j].c + (lb[j] - la[j]);
                m1[i] = kp ? en[j].m : 0;
                v2[i] = e2[j].c + (l4[j] - l2[j]);
                m2[i] = pair_ok[j] ? e2[j].m : 0;
            }
        }
    }

    // ---- the walk (kernels.hip: land) ---------------------------------------------------------------------------------
    const double extra0 = extra;
    bool heavy = false, skip = false;
#pragma unroll
    for (int i = 1; i < KMAX; ++i) {
        if (!(keep & (1u << i)) || heavy) continue;
        if (skip) { // second switch of a pair that came out of the pair table
            skip = false;
            continue;
        }
        const int t3 = n2[i] < T ? n2[i] : T;
        const int t4 = n4[i] < T ? n4[i] : T;
        if (m1[i] > 0 && a[i] + m1[i] <= t3) {
            extra += v1[i];
        } else if (m2[i] > 0 && a[i] + m2[i] <= t4) {
            extra += v2[i];
            skip = true;
        } else {
            heavy = true;
        }
    }
    if (!heavy) {
        p.out[task] = extra;
        if (p.frames_task) p.frames_task[task] = 0;
        if (p.tasks_done) {
            const unsigned long long done = __ballot(1);
            if ((threadIdx.x & 63) == (unsigned)__ffsll((long long)done) - 1)
                atomicAdd(p.tasks_done, (unsigned long long)__popcll(done));
        }
        return -1;
    }

    // ---- a chain the tables do not cover: hand the task to the frame loop, in the bucket of its expected work ----------
    // (chain_work.h, over the entries of the `keep` mask)
    ChainWork cw{p.m_typ, p.trans2 != nullptr};
#pragma unroll
    for (int i = 1; i < KMAX; ++i) {
        if (!(keep & (1u << i))) continue;
        cw.add(a[i], (n2[i] < T ? n2[i] : T) - a[i]);
    }
    const int w = cw.finish(T);
    if (p.no_lists) { // (cannot happen: the host checked the tables entry by entry -- a visible NaN rather than a stale result if it did)
        p.out[task] = __longlong_as_double(0x7ff8000000000000ll);
        return -1;
    }
    int bucket = w / kWorkBucketFrames;
    bucket = bucket < 0 ? 0 : (bucket >= kWorkBuckets ? kWorkBuckets - 1 : bucket);
    write_list();
    hand(a, b, keep, v1, v2, m1, m2, extra0, w);
    return bucket;
}

} // namespace bild
