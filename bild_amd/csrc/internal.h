// Entry points between the translation units of the library (not part of the C ABI).
#pragma once
#include <stdint.h>

#include <mutex>

struct bild_model;
struct bild_trajset;
struct bild_gauss_model;
struct bild_gauss_trajset;

namespace bild {

struct GaussTraj;

// One batch of the sampler's own (s, theta) rows that are ALREADY in HBM (ss: n x K1 float64, thetas: n x K1 uint8), on the
// model's own stream, results to d_out (device, n doubles); nothing is waited for.  `status` (2 ints, device-visible,
// zeroed by the caller) reports rows that are no points on the simplex.  Serialised per model like the host-buffer calls;
// the model's stream is returned in *stream (a hipStream_t).  K1 <= 16.
int internal_logl_st_resident(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const double *d_ss, const uint8_t *d_thetas,
                              unsigned flags, double *d_out, int32_t *status, void **stream);

// the model's own stream (a hipStream_t): device copies of the model are made on first use; null on failure
void *internal_model_stream(const bild_model *m);

// GenericGaussianModel (gauss.cpp): the number of trajectories of a set and their frames (valid while the set lives)
int internal_gauss_set_lengths(const bild_gauss_model *m, const bild_gauss_trajset *ts, int *n_traj, const int **T);
// the walk (gauss_walk_kernel<false>) over segment rows that are ALREADY in HBM, results to d_out (device, n doubles), on
// `stream` (a hipStream_t); nothing is waited for.  The set's tables are complete when it is created: any stream may read them.
int internal_gauss_walk_resident(const bild_gauss_model *m, const bild_gauss_trajset *ts, int64_t n, int K1, const int32_t *d_seg_start,
                                 const int32_t *d_seg_state, const int32_t *d_traj_id, double *d_out, void *stream);

// the device descriptors (one GaussTraj per trajectory) and the stream of a set (a hipStream_t), and the lock that serialises
// the calls that use that stream
int internal_gauss_set_device(const bild_gauss_model *m, const bild_gauss_trajset *ts, const GaussTraj **d_trajs, void **stream,
                              std::mutex **mu);

} // namespace bild
