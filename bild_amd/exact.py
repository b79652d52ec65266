"""
Exact evidence for a fixed number of switches by enumerating every profile on the GPU (bild_exact_evidence,
bild_gauss_exact_evidence).

For k switches the profiles of a trajectory of T frames are every switch combination c_1 < ... < c_k from {1, ..., T - 1}
with every valid trace of k + 1 states, in the order `FixedkSampler.fix_exhaustive` pools them: traces outer
(`CFC.full_sample` order), combinations inner (`itertools.combinations` order).  Under the uniform prior over them this
gives what `fix_exhaustive`, `MAP_profile` and `log_marginal_posterior` give, without the host's `max_fcomplete` cap: at
T = 1000 and two states there are ~2e3 profiles at k = 1, ~1e6 at k = 2 and ~3.3e8 at k = 3.
"""
import numpy as np

from . import _lib
from .profiles import Loopingprofile, states_from_segments

MAX_K = 15


class ExactResult:
    """
    The exact answer for one trajectory and one k.

    k, n_profiles : the number of switches and of profiles enumerated (C(T - 1, k) x valid traces)
    logev : log of the mean likelihood under the uniform prior (-inf without profiles; NaN if a logL is NaN)
    KL : Kullback-Leibler divergence of the posterior from the prior (NaN without profiles or with a NaN logL; a profile with
        logL = -inf weighs 0 and adds 0, where the host's formula gives NaN)
    n_nan : profiles whose logL is NaN
    map_profile, map_logL : the profile of largest logL (the first in enumeration order among equal maxima, the NaN profiles
        left out) as a `Loopingprofile`, and its logL; None and NaN without one
    log_marginal_posterior : (S, T) normalised log posterior marginals of the state per frame, or None when not asked for
    """

    __slots__ = ('k', 'n_profiles', 'logev', 'KL', 'n_nan', 'map_profile', 'map_logL', 'log_marginal_posterior')

    def __init__(self, **kw):
        for name in self.__slots__:
            setattr(self, name, kw[name])

    def __repr__(self):
        return (f"ExactResult(k={self.k}, n_profiles={self.n_profiles}, logev={self.logev!r}, KL={self.KL!r}, "
                f"n_nan={self.n_nan}, map_logL={self.map_logL!r})")


def profile_count(T, k, transitions):
    """ number of profiles of k switches on a trajectory of T frames: C(T - 1, k) x valid traces (host only) """
    return _lib.exact_count(T, k, transitions)


def exact_evidence(trajs, model, k, marginals=True, max_profiles=2 ** 32, scratch_bytes=0):
    """
    Exact evidence, KL, MAP profile and (optionally) posterior marginals of ``trajs`` at ``k`` switches.

    trajs : a trajectory or a list of them (as `model.trajset` takes them); a list gives a list of results
    model : a `MultiStateRouse` or a `GenericGaussianModel` (anything else: TypeError)
    k : number of switches, 0 <= k <= 15
    marginals : compute `log_marginal_posterior` (needs S x T <= 8192 per trajectory: the LDS accumulators of a block)
    max_profiles : refuse (ValueError, with the count) when all trajectories together have more profiles than this
    scratch_bytes : device workspace of one chunk (0: at most 1 GiB and a third of the free memory)

    The count and every refusal run before the trajectories are uploaded, so they need no GPU.
    Returns an `ExactResult` or a list of them.
    """
    from .gauss import GenericGaussianModel
    from .models import MultiStateRouse
    if not isinstance(model, (MultiStateRouse, GenericGaussianModel)):
        raise TypeError(f"exact evidence needs a MultiStateRouse or GenericGaussianModel, not {type(model).__name__}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k <= MAX_K:
        raise ValueError(f"k = {k!r}: exact enumeration supports integers 0 <= k <= {MAX_K}")
    k = int(k)
    S = model.nStates
    transitions = np.asarray(model.transitions, dtype=bool)
    if transitions.shape != (S, S):
        raise ValueError(f"model.transitions has shape {transitions.shape}; ({S}, {S}) expected")
    single = not isinstance(trajs, (list, tuple))
    items = [trajs] if single else list(trajs)
    if not items:
        return []
    Ts = [len(t) for t in items]
    counts = [int(profile_count(T, k, transitions)) for T in Ts]
    total = sum(counts)
    if total > max_profiles:
        raise ValueError(f"{total} profiles at k = {k} on {len(items)} trajector{'y' if len(items) == 1 else 'ies'} "
                         f"exceed max_profiles = {max_profiles}")
    if marginals:
        for T, c in zip(Ts, counts):
            if c and S * T > 8192:
                raise ValueError(f"marginals of {S} states x {T} frames exceed the 8192 values of a block's accumulators; "
                                 f"call with marginals=False")

    arg = items[0] if single else items
    if isinstance(model, GenericGaussianModel):
        ts = model.trajset(arg)
        res = _lib.exact_evidence(model.handle(), ts, k, transitions, marginals, max_profiles, scratch_bytes, gauss=True)
    else:
        # a set declared for the count: the large tables of the likelihood are built (bild_trajset_expect)
        ts = model.trajset(arg, expect=total if total >= 10 ** 8 else None)
        res = _lib.exact_evidence(model.handle(), ts, k, transitions, marginals, max_profiles, scratch_bytes,
                                  path=model.path)

    out = []
    for j, (T, c) in enumerate(zip(Ts, counts)):
        seg_start, seg_state = res['map_seg_start'][j:j + 1], res['map_seg_state'][j:j + 1]
        profile = None
        if seg_start[0, 0] >= 0:
            profile = Loopingprofile(states_from_segments(seg_start, seg_state, T)[0])
        post = None if res['log_post'] is None else res['log_post'][j, :, :T].copy()
        out.append(ExactResult(k=k, n_profiles=c, logev=float(res['logev'][j]), KL=float(res['kl'][j]),
                               n_nan=int(res['n_nan'][j]), map_profile=profile, map_logL=float(res['map_logl'][j]),
                               log_marginal_posterior=post))
    return out[0] if single else out

