// What sim.cpp (host) and sim.hip (kernel) share: the parameter block of the Rouse trajectory generator and its
// launcher.  Private to the library.
#pragma once
#include <stdint.h>

namespace bild {

constexpr int kSimMaxN = 256;       // modes per state
constexpr int kSimMaxLanes = 1024;  // modes x dimensions of one workgroup (dimensions beyond that go to further workgroups)

struct SimParams {
    // per state, in the state's eigenbasis V (N x N, orthonormal columns = modes)
    const double *V;        // S x N x N, V[s][m][j]: monomer m, mode j
    const double *Vt;       // S x N x N, its transpose per state
    const double *b;        // S x N    one-frame decay per mode
    const double *ssig;     // S x N    sqrt of the per-frame noise variance
    const double *scinf;    // S x N    sqrt of the steady-state variance
    const double *g;        // S x N x d  V^T G
    const double *m0;       // S x N x d  V^T M0
    const double *u;        // S x N    V^T w
    // per trajectory (this launch's range: trajectories first .. first + n - 1 of the call)
    const int32_t *T;
    const int64_t *frame_off;   // first output row of each trajectory (rows of d values)
    const int32_t *seg_start, *seg_state;   // n x K1, as bild_logl_segments takes them
    const uint8_t *missing;     // per output row: 1 = missing frame (NaN)
    const double *err;          // n x d localization error
    // replay mode: host-drawn normals, per trajectory T N d (dynamics: frame, mode, dimension) then T d (localization)
    const double *z;            // null: device mode
    const int64_t *z_off;       // per trajectory, offset of its normals among all of the call's
    int64_t z_first;            // offset of the normal at z[0]
    uint64_t seed;              // device mode
    int64_t first;              // index in the call of this launch's first trajectory (the device streams are keyed by it)
    double *out;                // rows of d values
    int n, K1, S, N, d;
    int dpb;                    // dimensions per workgroup
    int chunk;                  // frames per LDS chunk (even)
};

int launch_rouse_simulate(const SimParams &p, void *stream);

} // namespace bild
