// Host-only build for the sanitizers (make asan): the kernel launchers of the .hip files, which this build does not
// contain.  The sanitizer run happens on a machine without a GPU, where no evaluation gets as far as a launch
// (bild_trajset_create fails with BILD_ERR_NO_DEVICE first); the geometry tables are host code and are duplicated here
// only as far as packing needs them (padded_rows), with the same values as kernels.hip.
#include "common.h"
#include "amis_math.h"
#include "internal.h"
#include "kalman.h"
#include "sens.h"

namespace bild {
int padded_rows(int n)
{
    static const int rows[] = {4, 8, 10, 12, 16, 20, 24, 28, 32};
    for (int r : rows)
        if (r >= n) return r;
    return 0;
}
bool geometry_for(int, int, int64_t, int, Geometry *, bool, bool) { return false; }
const char *kernel_name(const Geometry &, int) { return "none"; }
int launch_logl(const Geometry &, int, const KParams &, int, size_t, void *, void *, void *) { return 1; }
int launch_logl_one(const Geometry &, const KParams &, const WalkParams &, int, size_t, void *, void *, void *) { return 1; }
int launch_reduce_partials(const double *, double *, int64_t, int, void *) { return 1; }
int launch_prefix_L(const TrajDesc *, int, int, int, int, int, double *, double *, void *) { return 1; }
int launch_validate(const int32_t *, const int32_t *, const int32_t *, const int32_t *, int64_t, int, int, int, int *, void *) { return 1; }
bool builder_geometry(int, Geometry *) { return false; }
bool listed_geometry(const Geometry &, Geometry *) { return false; }
bool dense_mfma_supported(int NP) { return NP % 4 == 0 && NP >= 4 && NP <= 24; }
int launch_logl_dense_mfma(int, const KParams &, void *) { return 1; }
bool modal_mfma_supported(int NP) { return NP == 36 || NP == 40; }
int launch_logl_modal_mfma(int, const KParams &, void *) { return 1; }
size_t wide_lds_bytes(int) { return 0; }
int launch_pair_tasks(const int64_t *, int, const TrajDesc *, int, int, int64_t, int32_t *, int32_t *, int32_t *, void *) { return 1; }
int launch_two_switch_cover(const TrajDesc *, const int64_t *, int64_t, int, int, const TransEntry *, const TransEntry *, int, int *, void *) { return 1; }
size_t device_schedule_bytes(int64_t) { return 0; }
int device_schedule(const int32_t *, const int32_t *, const TrajDesc *, int, int64_t, int, int, int, int, int64_t, void *, size_t, const int32_t **, void *) { return 1; }
int launch_logl_wide(int, const KParams &, int, void *) { return 1; }
int launch_walk(const WalkParams &, void *, void *, void *) { return 1; }
int launch_kalman(const KalParams &, int, void *) { return 1; }
int launch_kalman_mix(const MixParams &, void *) { return 1; }
int launch_sens(const SensParams &, int, int, void *) { return 1; }
int launch_tail(const TrajDesc *, int, int, int, int, int, const double *, const double *, const int64_t *, int64_t, double *, double *, void *) { return 1; }
int launch_switch_tail(const TrajDesc *, int, int, int, int, int, const double *, const double *, int, const double *, const double *, const TransEntry *, const int64_t *, int64_t, int, double *, double *, void *) { return 1; }
int launch_mark_refused_rows(const int32_t *, int, int64_t, double *, void *) { return 1; }
int amis_dev_pass_a_rows(int64_t, int64_t) { return 0; }
int amis_dev_draw(int, int, int64_t, uint64_t, uint64_t, const double *, const double *, const uint8_t *, double *, uint8_t *, void *) { return 1; }
int amis_dev_pass_a(const AmisView &, int64_t, int64_t, int64_t, double, double *, double *, double *, double *, double *, int *, void *, const uint8_t *, uint8_t *, int32_t *, int32_t *, int32_t *, double *) { return 1; }
int amis_dev_pass_b(const AmisView &, int64_t, double, int, const double *, double *, double *, int, void *) { return 1; }
int amis_dev_pass_c(const AmisView &, int64_t, const double *, double, const double *, const double *, double *, int, void *) { return 1; }
} // namespace bild
#include "gauss.h"
namespace bild {
int launch_gauss_factor(const GaussJobSet &, const GaussJob *, int, double *, int64_t, void *) { return 1; }
int launch_gauss_solve(const GaussJobSet &, const GaussJob *, int, int, void *) { return 1; }
int launch_gauss_accumulate(const GaussAccum &, void *) { return 1; }
int launch_gauss_walk(const GaussWalk &, bool, void *) { return 1; }
int launch_gauss_factor_sets(const GaussJobSet *, const GaussJob *, int, void *) { return 1; }
int launch_gauss_sim_normals(const GaussSimProduct &, void *) { return 1; }
int launch_gauss_sim_product(const GaussSimProduct &, void *) { return 1; }
int launch_gauss_sim_assemble(const GaussSimAssemble &, void *) { return 1; }
int launch_gauss_sens_factor(const GaussSensSet *, const GaussSensJob *, int, int, double *, double *, void *) { return 1; }
int launch_gauss_sens_solve(const GaussSensSet *, const GaussSensJob *, int, int, int, double *, void *) { return 1; }
} // namespace bild
#include "gauss_kalman.h"
namespace bild {
int launch_gauss_kal_factor(const GaussKalSet *, const GaussKalJob *, int, double *, double *, void *) { return 1; }
int launch_gauss_kal_solve(const GaussKalSet *, const GaussKalJob *, int, int, double *, void *) { return 1; }
int launch_gauss_kal_scatter(const GaussKalScatter &, void *) { return 1; }
} // namespace bild
#include "exchange.h"
namespace bild {
int launch_exchange(const ExParams &, void *) { return 1; }
} // namespace bild
#include "sim.h"
namespace bild {
int launch_rouse_simulate(const SimParams &, void *) { return 1; }
} // namespace bild
#include "exact.h"
namespace bild {
int launch_exact_enumerate(const ExactEnum &, void *) { return 1; }
int launch_exact_reduce(const ExactReduce &, void *) { return 1; }
int launch_exact_fold(const ExactFold &, void *) { return 1; }
size_t exact_reduce_lds(int, int, int, bool) { return 0; }
} // namespace bild
#include "gauss_segdp.h"
namespace bild {
int launch_segdp_init(const SegdpParams &, bool, void *) { return 1; }
int launch_segdp_mix(const SegdpParams &, int, void *) { return 1; }
int launch_segdp_level(const SegdpParams &, int, void *) { return 1; }
int launch_segdp_blevel(const SegdpParams &, int, void *) { return 1; }
int launch_segdp_bmix(const SegdpParams &, int, void *) { return 1; }
int launch_segdp_backtrack(const SegdpParams &, void *) { return 1; }
int launch_segdp_cover(const SegdpParams &, void *) { return 1; }
int launch_segdp_carry(const SegdpParams &, void *) { return 1; }
} // namespace bild
#include "gauss_segdraw.h"
namespace bild {
int launch_segdraw_head(const SegdrawParams &, void *) { return 1; }
int launch_segdraw(const SegdrawParams &, const SegdrawParams *, void *) { return 1; }
} // namespace bild
#include "gauss_segsens.h"
namespace bild {
int launch_segsens_weight(const SegdpParams &, const SegsensWeights &, void *) { return 1; }
int launch_segsens_solve(const GaussSensSet *, const SegsensJob *, int, int, int, const double *, double *, void *) { return 1; }
int launch_segsens_factor(const GaussSensSet *, const SegsensJob *, int, int, const double *, double *, double *, void *) { return 1; }
} // namespace bild
#include "gauss_dwell.h"
namespace bild {
int launch_dwell_forward(const DwellParams &, void *) { return 1; }
int launch_dwell_backward(const DwellParams &, void *) { return 1; }
int launch_dwell_cover(const DwellParams &, void *) { return 1; }
int launch_dwell_carry(const DwellParams &, void *) { return 1; }
int launch_dwell_counts(const DwellParams &, void *) { return 1; }
} // namespace bild
#include "gauss_dwellsens.h"
namespace bild {
int launch_dwellsens_weight(const DwellParams &, const DwellsensWeights &, void *) { return 1; }
}
#include "gauss_dwelllen.h"
namespace bild {
int launch_dwell_lengths(const DwellParams &, const DwellLengths &, void *) { return 1; }
}
#include "gauss_dwellfilt.h"
namespace bild {
int launch_dwell_filter(const DwellParams &, const DwellFilter &, void *) { return 1; }
}
#include "gauss_dwelllag.h"
namespace bild {
int launch_dwell_lag_bases(const DwellParams &, const DwellLag &, void *) { return 1; }
int launch_dwell_lag_windows(const DwellParams &, const DwellLag &, void *) { return 1; }
}
#include "gauss_dwellevent.h"
namespace bild {
int launch_dwell_level(const DwellParams &, const DwellLevels &, int, void *) { return 1; }
int launch_dwell_contact(const DwellParams &, const DwellContact &, void *) { return 1; }
}
#include "gauss_dwellocc.h"
namespace bild {
int launch_dwell_occupancy(const DwellParams &, const DwellOccupancy &, int, void *) { return 1; }
}
#include "gauss_dwellwin.h"
namespace bild {
int launch_dwell_windows(const DwellParams &, const DwellWindows &, void *) { return 1; }
}
#include "gauss_dwellvis.h"
namespace bild {
int launch_dwell_visits(const DwellParams &, const DwellVisits &, int, void *) { return 1; }
}
#include "gauss_dwelldraw.h"
namespace bild {
int launch_dwelldraw_head(const DwelldrawParams &, void *) { return 1; }
int launch_dwelldraw(const DwelldrawParams &, const DwelldrawParams *, void *) { return 1; }
} // namespace bild
