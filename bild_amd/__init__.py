"""
bild_amd -- MI355X-native Rouse Kalman-filter likelihood for BILD
(Bayesian Inference of Looping Dynamics).

One hot path, behind the reference's own interfaces:

* `models.MultiStateRouse.logL(profile, traj)`      (reference bild/models.py:265-278)
* `amis.FixedkSampler.logL(ss, thetas)`             (reference bild/amis.py:717-739)

both evaluated by hand-written HIP kernels for gfx950 through the C ABI declared in
``include/bild_amd.h`` (``bild_amd/libbild_amd.so``).  There is no CPU fallback.
"""
from . import rouse, profiles, util, trajectory, models, gauss, amis, choicesampler, core, postproc, exact  # noqa: F401
from .core import sample, sample_many, SamplingResults, posterior_distances  # noqa: F401
from .models import MultiStateModel, MultiStateRouse, FactorizedModel, KalmanResult, FitResult  # noqa: F401
from .gauss import GenericGaussianModel  # noqa: F401
from .exact import exact_evidence, ExactResult, exact_sample, ExactSamplingResults, exact_draw, ExactDraws  # noqa: F401
from .exact import exact_sensitivities, EvidenceSensitivities  # noqa: F401
from .exact import DwellPrior, exact_dwell, ExactDwellResults, fit_markov_prior, MarkovPriorFit  # noqa: F401
from .exact import exact_dwell_draw, ExactDwellDraws  # noqa: F401
from .exact import exact_dwell_sensitivities, DwellSensitivities  # noqa: F401
from .exact import exact_dwell_lengths, DwellLengthCounts, fit_dwell_prior, DwellPriorFit  # noqa: F401
from .exact import exact_dwell_filter, DwellFilterResults  # noqa: F401
from .exact import exact_dwell_lag, DwellLagResults  # noqa: F401
from .exact import exact_dwell_switch_counts, DwellSwitchCounts, exact_dwell_first_contact, DwellFirstContact  # noqa: F401
from .exact import exact_dwell_occupancy, DwellOccupancy, pooled_occupancy  # noqa: F401
from .exact import exact_dwell_windows, DwellWindowSupport, DwellMapSupport  # noqa: F401
from .exact import exact_dwell_visits, DwellVisits, pooled_visits  # noqa: F401
from .amis import FixedkSampler, Dirichlet, CFC  # noqa: F401
from .profiles import Loopingprofile  # noqa: F401
from .trajectory import Trajectory  # noqa: F401

__version__ = '0.1.0'
