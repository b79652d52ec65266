// Host pieces of the GenericGaussianModel calls that take trajectories directly (gauss_sens.cpp, gauss_kalman.cpp): the
// checks of a call before any device work and the intervals of a candidate.  Private to the library.
#pragma once
#include <algorithm>
#include <cmath>

#include "gauss.h"
#include "likelihood.h"

namespace bild {

// the model, the trajectories (1 <= T <= 2048, T - 1 <= Tmax), the derivative arrays (P of them), the segment rows and
// traj_id
inline int gauss_check_args(const bild_gauss_model *m, int n_traj, const int32_t *T, const double *x, int64_t n, int K1, const int32_t *seg_start,
               const int32_t *seg_state, const int32_t *traj_id, int P, const bild_gauss_derivs *dm)
{
    if (!m) return fail(BILD_ERR_INVALID, "NULL model");
    if (n_traj < 1 || !T || !x) return fail(BILD_ERR_INVALID, "need at least one trajectory (n_traj = %d, T and x non-NULL)", n_traj);
    if (n < 0 || K1 < 1) return fail(BILD_ERR_INVALID, "n = %lld, K1 = %d", (long long)n, K1);
    if (P < 0) return fail(BILD_ERR_INVALID, "P = %d is negative", P);
    if (P > kGaussSensMaxP) return fail(BILD_ERR_UNSUPPORTED, "at most %d parameters per call; P = %d", kGaussSensMaxP, P);
    for (int j = 0; j < n_traj; ++j) {
        if (T[j] < 1) return fail(BILD_ERR_INVALID, "trajectory %d has %d frames", j, T[j]);
        if (T[j] > kGaussMaxT)
            return fail(BILD_ERR_UNSUPPORTED, "trajectory %d has %d frames; GenericGaussianModel supports at most %d", j, T[j], kGaussMaxT);
        if (T[j] - 1 > m->L)
            return fail(BILD_ERR_INVALID, "trajectory %d has %d frames but the MSD tables end at lag %d", j, T[j], m->L);
    }
    if (dm && P > 0) {
        const size_t sd = (size_t)m->S * m->d, L1 = (size_t)m->L + 1;
        const struct {
            const double *a;
            size_t count;
            const char *name;
        } arrs[] = {{dm->dmsd, (size_t)P * sd * L1, "dmsd"}, {dm->dmsd_inf, (size_t)P * sd, "dmsd_inf"}, {dm->dmean, (size_t)P * sd, "dmean"}};
        for (const auto &a : arrs)
            if (a.a)
                for (size_t i = 0; i < a.count; ++i)
                    if (!std::isfinite(a.a[i])) return fail(BILD_ERR_INVALID, "%s[%zu] is not finite", a.name, i);
    }
    if (n == 0) return BILD_OK;
    if (!seg_start || !seg_state) return fail(BILD_ERR_INVALID, "NULL segment arrays");
    for (int64_t r = 0; r < n; ++r) {
        if (traj_id && (traj_id[r] < 0 || traj_id[r] >= n_traj))
            return fail(BILD_ERR_INVALID, "traj_id[%lld] = %d out of range (%d trajectories)", (long long)r, traj_id[r], n_traj);
        const int32_t *a = seg_start + r * K1, *b = seg_state + r * K1;
        if (a[0] != 0) return fail(BILD_ERR_INVALID, "sample %lld: the first segment must start at 0", (long long)r);
        for (int i = 0; i < K1; ++i) {
            if (b[i] < 0 || b[i] >= m->S) return fail(BILD_ERR_INVALID, "sample %lld: state %d out of range", (long long)r, b[i]);
            if (i > 0 && (a[i] < 1 || a[i] < a[i - 1]))
                return fail(BILD_ERR_INVALID, "sample %lld: segment starts must be >= 1 and non-decreasing", (long long)r);
        }
    }
    return BILD_OK;
}

// the intervals of candidate r as gauss_walk_kernel cleans them: (window start a, end b, state, first?)
template <class F> void for_each_interval(const int32_t *st, const int32_t *sv, int K1, int T, F &&f)
{
    int t0 = 0, cur = sv[0];
    bool first = true;
    for (int i = 0; i < K1; ++i) {
        const int s = std::min(st[i], T);
        const int e = i + 1 < K1 ? std::min(st[i + 1], T) : T;
        if (e <= s || sv[i] == cur) continue;
        f(first ? 0 : t0 - 1, s, cur, first);
        first = false;
        t0 = s;
        cur = sv[i];
    }
    f(first ? 0 : t0 - 1, T, cur, first);
}

} // namespace bild
