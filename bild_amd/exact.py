"""
Exact evidence for a fixed number of switches by enumerating every profile on the GPU (bild_exact_evidence,
bild_gauss_exact_evidence).

For k switches the profiles of a trajectory of T frames are every switch combination c_1 < ... < c_k from {1, ..., T - 1}
with every valid trace of k + 1 states, in the order `FixedkSampler.fix_exhaustive` pools them: traces outer
(`CFC.full_sample` order), combinations inner (`itertools.combinations` order).  Under the uniform prior over them this
gives what `fix_exhaustive`, `MAP_profile` and `log_marginal_posterior` give, without the host's `max_fcomplete` cap: at
T = 1000 and two states there are ~2e3 profiles at k = 1, ~1e6 at k = 2 and ~3.3e8 at k = 3.

`exact_sample` (bild_gauss_segment_evidence) does not enumerate: GenericGaussianModel's log-likelihood
is a sum of per-segment table entries, so the sums over all profiles of k switches follow from a recursion over segments,
for every k up to k_max in one call.

`exact_draw` (bild_gauss_segment_draw) draws profiles from that exact posterior, segment by segment
against the recursion's backward tables: independent draws, without weights or burn-in.

`exact_dwell` (bild_gauss_dwell_evidence) replaces the uniform prior per k by a dwell-time prior
(`DwellPrior`): one evidence per trajectory over the profiles of every k, MAP profile, marginals and expected jump / stay
counts; `fit_markov_prior` fits a Markov prior's switching rates to a data set by EM on those counts.

`exact_dwell_draw` (bild_gauss_dwell_draw) draws profiles from the exact posterior under that prior,
segment by segment against the backward tables of the dwell-time recursion.

`exact_dwell_sensitivities` (bild_gauss_dwell_sensitivities) is the gradient of `exact_dwell`'s evidence
with respect to model parameters; `GenericGaussianModel.fit_dwell` fits a model, and a Markov prior with it, on that gradient.

`exact_dwell_lengths` (bild_gauss_dwell_lengths) is the gradient of that evidence with respect to the
prior's own length tables: the expected number of segments of every length; `fit_dwell_prior` fits the dwell-time distributions
themselves by EM on those counts, in the discrete-hazard parametrisation of `DwellPrior.from_hazard`.

`exact_dwell_filter` (bild_gauss_dwell_filter) gives the causal answers under that prior: per frame the
state probabilities, the run-length posterior and the evidence of the data so far, and from the latter the one-step predictive
log-likelihoods.

`exact_dwell_lag` (bild_gauss_dwell_lag) fills the range between the filter and the smoothed marginals:
per frame the state probabilities given the data up to `lag` frames later, for every lag up to `lag` at once.

`exact_dwell_switch_counts` and `exact_dwell_first_contact` (bild_gauss_dwell_switch_counts, bild_gauss_dwell_first_contact;
DESIGN.md section 27) are the exact posteriors of two functionals of the whole profile: the number of switches, and the first
frame in a set of states together with the probability that there is none.

`exact_dwell_occupancy` (bild_gauss_dwell_occupancy) is the exact posterior of a third: the number of
frames spent in a set of states, the looped fraction of the trajectory; `pooled_occupancy` is that of a whole data set.

`exact_dwell_windows` (bild_gauss_dwell_windows) is the exact posterior probability that every frame of a
window is in a set of states, for any number of windows a trajectory; `ExactDwellResults.map_support` asks it about the MAP
profile: how well the posterior supports each called segment and the placement of each called switch.

`exact_dwell_visits` (bild_gauss_dwell_visits) is the exact posterior of the number of visits to a set of
states: contact episodes, maximal runs of frames in the set, for any number of states; `pooled_visits` is that of a data set.
"""
import math
import warnings

import numpy as np
from scipy.special import logsumexp

from . import _lib
from .profiles import Loopingprofile, segments_from_states, states_from_segments

MAX_K = 15


class _Record:
    """ the base of the result classes: the attributes are the class's ``__slots__``, each given by keyword (KeyError without one) """

    __slots__ = ()

    def __init__(self, **kw):
        for name in self.__slots__:
            setattr(self, name, kw[name])


class ExactResult(_Record):
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



# ---------------------------------------------------------------- every k at once: the segment recursion (section 18)

MAX_K_SEGMENT = 64


def segment_profile_count(T, k, transitions):
    """ profiles of k switches on T frames as an exact integer: C(T - 1, k) x `CFC.N_total(k)` """
    from .amis import CFC
    return math.comb(T - 1, k) * int(CFC(transitions).N_total(k)) if 0 <= k <= T - 1 else 0


class ExactSamplingResults:
    """
    The exact counterpart of `SamplingResults` for one trajectory of a `GenericGaussianModel`: evidence, KL, MAP profile and
    state marginals of every k = 0 ... k_max under the uniform prior over the profiles of k switches.

    traj, model, dE : as given to `exact_sample`
    k : 0 ... k_max
    evidence : log-evidence per k (-inf: no profile of k switches; NaN under nan='propagate' where a profile of k switches
        uses a NaN window); evidence_se : zeros, the evidence is exact
    KL : Kullback-Leibler divergence of the posterior from the prior per k
    n_profiles : profiles the evidence averages over, a list of Python integers (exact; the device's count of the profiles
        left under nan='omit' is exact below 2^53); n_omitted : profiles left out (nan='omit' only)
    map_logL : the largest log-likelihood per k (NaN without a profile)
    nan : the NaN mode the results were made with ('propagate' or 'omit')
    """

    def __init__(self, traj, model, dE, evidence, KL, map_logL, n_profiles, n_omitted, map_seg_start, map_seg_state, log_post,
                 nan='propagate'):
        self.traj = traj
        self.model = model
        self.dE = dE
        self.nan = nan
        self.evidence = np.asarray(evidence, dtype=np.float64)
        self.k = np.arange(len(self.evidence))
        self.evidence_se = np.zeros(len(self.evidence))
        self.KL = np.asarray(KL, dtype=np.float64)
        self.map_logL = np.asarray(map_logL, dtype=np.float64)
        self.n_profiles = list(n_profiles)
        self.n_omitted = list(n_omitted)
        self._seg_start = np.asarray(map_seg_start, dtype=np.int32)
        self._seg_state = np.asarray(map_seg_state, dtype=np.int32)
        self._log_post = log_post

    def __repr__(self):
        return f"ExactSamplingResults(T={len(self.traj)}, k_max={len(self.k) - 1}, evidence={self.evidence!r})"

    def map_profile(self, k):
        """ a profile of k switches of largest log-likelihood as a `Loopingprofile` (None without one) """
        if self._seg_start[k, 0] < 0:
            return None
        return Loopingprofile(states_from_segments(self._seg_start[k:k + 1, :k + 1], self._seg_state[k:k + 1, :k + 1],
                                                   len(self.traj))[0])

    def best_k(self, dE=None):
        """ smallest k whose evidence is within dE of the maximum, as `SamplingResults.best_k`; NaN evidences are ignored """
        if dE is None:
            dE = self.dE
        ev = self.evidence
        bad = np.isnan(ev)
        if np.all(bad):
            raise ValueError("every evidence is NaN (profiles with a NaN window at every k): use nan='omit'")
        if np.any(bad):
            warnings.warn(f"evidence is NaN for k = {self.k[bad].tolist()}; these k are ignored (nan='omit' leaves the NaN "
                          f"profiles out instead)", RuntimeWarning, stacklevel=2)
        ev = np.where(bad, -np.inf, ev)
        return int(np.min(self.k[ev >= np.max(ev) - dE]))

    def best_profile(self, dE=None):
        """ MAP profile at `best_k` """
        return self.map_profile(self.best_k(dE))

    def log_marginal_posterior_k(self, k):
        """
        (S, T) log posterior state marginals of the profiles of k switches.  The device sums them in linear scale against
        the level's `map_logL`: values above -600 carry all their digits, those between -600 and -700 lose them towards
        -700, and a marginal below about -700 may be reported as -inf ("Range").
        """
        if self._log_post is None:
            raise ValueError("the marginals were not computed: call exact_sample with marginals=True")
        return self._log_post[k]

    def log_marginal_posterior(self, dE=None):
        """
        (S, T) log posterior state marginals at `best_k`; ``dE='average'`` averages over k weighted by evidence, with
        `SamplingResults.log_marginal_posterior`'s formula (k with NaN evidence are left out with `best_k`'s warning)
        """
        if isinstance(dE, str) and dE == 'average':
            if self._log_post is None:
                raise ValueError("the marginals were not computed: call exact_sample with marginals=True")
            if np.any(np.isnan(self.evidence)):
                self.best_k(0)      # the warning, or the error when nothing is left
            with np.errstate(under='ignore'):
                logpost = logsumexp([self._log_post[k] + logev for k, logev in zip(self.k, self.evidence) if logev > -np.inf],
                                    axis=0)
                return logpost - logsumexp(logpost, axis=0)
        return self.log_marginal_posterior_k(self.best_k(dE))

    def draw(self, n, k=None, dE=None, seed=0, uniforms=None):
        """ n profiles drawn from the exact posterior as `ExactDraws`: `exact_draw` of these results """
        return exact_draw(self, n, k=k, dE=dE, seed=seed, uniforms=uniforms)

    def posterior_distance(self, n=1000, dE=None, seed=0):
        """
        (mean, var), each (T, d): the smoothed track averaged over n profiles drawn from the exact posterior at `best_k(dE)`,
        or with ``dE='average'`` over k by evidence, in one `model.kalman_mixture` call with equal weights -- the counterpart
        of `SamplingResults.posterior_distance`, whose weighted samples the exact draws replace.
        """
        if isinstance(dE, str) and dE == 'average':
            draws = exact_draw(self, n, k='average', seed=seed)
        else:
            draws = exact_draw(self, n, k=None, dE=dE, seed=seed)
        mean, var = self.model.kalman_mixture((draws.seg_start, draws.seg_state), [self.traj], np.zeros(len(draws.k)))
        return mean[0], var[0]


def _check_exact_sample(trajs, model, k_max, nan):
    """ every refusal of `exact_sample`; returns (single, items, transitions) """
    from .gauss import GenericGaussianModel
    if not isinstance(model, GenericGaussianModel):
        raise TypeError(f"exact_sample needs a GenericGaussianModel, whose log-likelihood is a sum of segment terms, not "
                        f"{type(model).__name__}")
    if isinstance(k_max, bool) or not isinstance(k_max, (int, np.integer)) or not 0 <= k_max <= MAX_K_SEGMENT:
        raise ValueError(f"k_max = {k_max!r}: the segment recursion supports integers 0 <= k_max <= {MAX_K_SEGMENT}")
    if nan not in ('propagate', 'omit'):
        raise ValueError(f"nan = {nan!r}: 'propagate' or 'omit'")
    S = model.msd.shape[0]      # (nStates is read off transitions)
    transitions = np.asarray(model.transitions, dtype=bool)
    if transitions.shape != (S, S):
        raise ValueError(f"model.transitions has shape {transitions.shape}; ({S}, {S}) expected")
    single = not isinstance(trajs, (list, tuple))
    items = [trajs] if single else list(trajs)
    for t in items:
        if len(t) > model.max_T:
            raise ValueError(f"trajectory of {len(t)} frames: GenericGaussianModel evaluates at most {model.max_T} frames")
    return single, items, transitions


def results_from_arrays(traj, model, dE, transitions, res, j=0, nan='propagate'):
    """ `ExactSamplingResults` of trajectory j from arrays shaped as `_lib.gauss_segment_evidence` returns them """
    T = len(traj)
    K = res['logev'].shape[1]
    n_omitted = [int(x) for x in res['n_omitted'][j]]
    n_profiles = [segment_profile_count(T, k, transitions) - n_omitted[k] for k in range(K)]
    post = None if res['log_post'] is None else res['log_post'][j, :, :, :T].copy()
    return ExactSamplingResults(traj, model, dE, res['logev'][j].copy(), res['kl'][j].copy(), res['map_logl'][j].copy(), n_profiles,
                                n_omitted, res['map_seg_start'][j].copy(), res['map_seg_state'][j].copy(), post, nan=nan)


def exact_sample(trajs, model, dE=0, k_max=20, marginals=True, nan='propagate', scratch_bytes=0):
    """
    Everything `sample` produces for a `GenericGaussianModel` -- evidence per k, best k, MAP profile, state marginals --
    exactly and for every k = 0 ... k_max at once, by a recursion over segments on the GPU (no sampler, no `evidence_se`,
    no `max_fcomplete`).

    trajs : a trajectory or a list of them; a list gives a list of results from ONE device call
    model : a `GenericGaussianModel` (anything else: TypeError -- the log-likelihood must be a sum of segment terms)
    dE : the default of `best_k` and the methods built on it
    k_max : largest number of switches, 0 <= k_max <= 64; k beyond T - 1 carry evidence -inf
    marginals : compute the state marginals of every k
    nan : 'propagate' -- a k with a profile that uses a NaN window (a later ss_order-0 segment without a valid frame) has NaN
        evidence, KL and marginals; 'omit' -- such profiles are left out of the sums and of the count (`n_omitted`)
    scratch_bytes : device workspace of one chunk of whole trajectories (0: at most 1 GiB and a third of the free memory)

    MAP ties (every switch frame inside a gap gives the same log-likelihood) are broken on the trajectory's own tables: the
    smallest final state, then from the last switch backwards the smallest switch frame and the smallest preceding state.
    The log marginals are exact down to about -600; a state marginal below about e^-700 at a frame underflows and is
    reported as -inf, not as its finite value (`ExactSamplingResults.log_marginal_posterior_k`).
    Every refusal is raised before the trajectories are uploaded.  Returns `ExactSamplingResults` or a list of them.
    """
    single, items, transitions = _check_exact_sample(trajs, model, k_max, nan)
    if not items:
        return []
    ts = model.trajset(items[0] if single else items)
    res = _lib.gauss_segment_evidence(model.handle(), ts, int(k_max), transitions, marginals=marginals, omit=nan == 'omit',
                                      scratch_bytes=scratch_bytes)
    out = [results_from_arrays(t, model, dE, transitions, res, j, nan=nan) for j, t in enumerate(items)]
    return out[0] if single else out


# ---------------------------------------------------------------- profiles drawn from the exact posterior (section 19)

class ExactDraws:
    """
    Profiles of one trajectory drawn independently from the exact posterior (`exact_draw`).

    k : (n,) switches of each draw; `n_switches` is the same array
    seg_start, seg_state : (n, k_max + 1) int32 run-length rows, k + 1 segments each, padded with empty segments at T in
        state 0 (the layout of `model.logL_segments` and `model.kalman_mixture`)
    logL : (n,) log-likelihood of each drawn profile, from the same tables
    uniforms : (n, max(1, 2 k_max)) the uniforms each draw consumed (0 where none was): given back as ``uniforms=`` with the
        same k they reproduce the draws
    """

    def __init__(self, T, k, seg_start, seg_state, logL, uniforms):
        self.T = int(T)
        self.k = np.asarray(k, dtype=np.int64)
        self.seg_start = np.asarray(seg_start, dtype=np.int32)
        self.seg_state = np.asarray(seg_state, dtype=np.int32)
        self.logL = np.asarray(logL, dtype=np.float64)
        self.uniforms = np.asarray(uniforms, dtype=np.float64)

    def __len__(self):
        return len(self.k)

    def __repr__(self):
        return f"ExactDraws(n={len(self.k)}, T={self.T}, k={np.unique(self.k).tolist()})"

    @property
    def n_switches(self):
        return self.k

    def states(self):
        """ (n, T) int array: the state of every frame of every draw """
        if len(self.k) == 0:
            return np.zeros((0, self.T), dtype=int)
        if np.any(self.seg_start[:, 0] < 0):
            raise ValueError("a draw has no profile (no profile of positive weight with that many switches)")
        return states_from_segments(self.seg_start, self.seg_state, self.T)

    def profiles(self):
        """ the draws as a list of `Loopingprofile` """
        return [Loopingprofile(row) for row in self.states()]


def _draw_k(r, n, k, dE, rng):
    """ the (n,) switches of the draws of one result, every refusal included """
    K = len(r.k)
    ev = r.evidence
    if k is None:
        ks = np.full(n, r.best_k(dE), dtype=np.int64)
    elif isinstance(k, str):
        if k != 'average':
            raise ValueError(f"k = {k!r}: None, an integer, an integer array of length n, or 'average'")
        if np.any(np.isnan(ev)):
            r.best_k(0)     # the warning, or the error when nothing is left
        use = np.flatnonzero(np.isfinite(ev))
        if len(use) == 0:
            raise ValueError("no k has finite evidence")
        with np.errstate(under='ignore'):
            w = np.exp(ev[use] - np.max(ev[use]))
        ks = use[rng.choice(len(use), size=n, p=w / np.sum(w))].astype(np.int64)
    else:
        a = np.asarray(k)
        if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"k = {k!r}: None, an integer, an integer array of length n, or 'average'")
        if a.ndim == 0:
            ks = np.full(n, int(a), dtype=np.int64)
        elif a.shape == (n,):
            ks = a.astype(np.int64)
        else:
            raise ValueError(f"k has shape {a.shape}; an integer or ({n},) expected")
    for kk in np.unique(ks):
        if not 0 <= kk < K:
            raise ValueError(f"k = {int(kk)}: the results hold k = 0 ... {K - 1}")
        if np.isnan(ev[kk]):
            raise ValueError(f"the evidence of k = {int(kk)} is NaN (a profile of {int(kk)} switches uses a NaN window): make the "
                             f"results with nan='omit', which leaves such profiles out")
        if ev[kk] == -np.inf:
            raise ValueError(f"the evidence of k = {int(kk)} is -inf: no profile of {int(kk)} switches to draw")
    return ks


def exact_draw(results, n, k=None, dE=None, seed=0, uniforms=None, scratch_bytes=0):
    """
    n profiles per trajectory, drawn independently from the exact posterior over the profiles of k switches, by sampling
    segment after segment against the backward tables of the segment recursion on the GPU: no
    burn-in, no weights, no sampler error.

    results : an `ExactSamplingResults` or a list of them over one model and one k_max; a list is served by ONE device call on
        one trajectory set and gives a list of `ExactDraws`
    n : draws per result
    k : None -- `best_k(dE)` of each result; an int -- that k for every draw; an int array of length n -- each draw's own k
        (replay uses this form; for a list of results also (len(results), n): each result's own); 'average' -- each draw's k is picked on the host with probability proportional to
        exp(evidence_k) over the k of finite evidence, from ``np.random.default_rng(seed)`` (k with NaN evidence are left out
        with `best_k`'s warning)
    seed : of the device's uniforms (draw i of result j is stream j n + i), and of the host's choice of k under 'average'
    uniforms : replay -- (n, max(1, 2 k_max)) uniforms in [0, 1), for a list of results (len(results), n, max(1, 2 k_max)):
        `ExactDraws.uniforms` of an earlier call; ``seed`` is then not used by the device
    scratch_bytes : device workspace of one chunk of whole trajectories (0: at most 1 GiB and a third of the free memory)

    A k outside 0 ... k_max, or one whose evidence is -inf or NaN, raises ValueError; profiles that use a NaN window are never
    drawn, so results made with nan='omit' give draws from the posterior without them.  Every refusal is raised before any
    device work.  Returns an `ExactDraws` or a list of them.
    """
    single = isinstance(results, ExactSamplingResults)
    items = [results] if single else list(results)
    if any(not isinstance(r, ExactSamplingResults) for r in items):
        raise TypeError("exact_draw needs ExactSamplingResults (from exact_sample) or a list of them")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError(f"n = {n!r}: a non-negative integer")
    n = int(n)
    if not items:
        return []
    model = items[0].model
    K = len(items[0].k)
    if any(r.model is not model for r in items):
        raise ValueError("exact_draw needs results over one model")
    if any(len(r.k) != K for r in items):
        raise ValueError("exact_draw needs results of one k_max")
    k_max, U = K - 1, max(1, 2 * (K - 1))
    transitions = np.asarray(model.transitions, dtype=bool)
    rng = np.random.default_rng(seed)
    per_result = not single and not isinstance(k, str) and k is not None and np.ndim(k) == 2
    if per_result and np.shape(k) != (len(items), n):
        raise ValueError(f"k has shape {np.shape(k)}; an integer, ({n},) or ({len(items)}, {n}) expected")
    ks = [_draw_k(r, n, np.asarray(k)[j] if per_result else k, dE, rng) for j, r in enumerate(items)]
    if uniforms is not None:
        uniforms = np.asarray(uniforms, dtype=np.float64)
        want = (n, U) if single else (len(items), n, U)
        if uniforms.shape != want:
            raise ValueError(f"uniforms has shape {uniforms.shape}; {want} expected")
        if not np.all((uniforms >= 0) & (uniforms < 1)):
            raise ValueError("uniforms must lie in [0, 1) (NaN or a value outside given)")
        uniforms = uniforms.reshape(len(items) * n, U)
    if n == 0:
        out = [ExactDraws(len(r.traj), ks[j], np.zeros((0, K), dtype=np.int32), np.zeros((0, K), dtype=np.int32), np.zeros(0),
                          np.zeros((0, U))) for j, r in enumerate(items)]
        return out[0] if single else out
    ts = model.trajset(items[0].traj if single else [r.traj for r in items])
    res = _lib.gauss_segment_draw(model.handle(), ts, k_max, transitions, np.repeat(np.arange(len(items)), n), np.concatenate(ks),
                                  uniforms=uniforms, seed=seed, scratch_bytes=scratch_bytes)
    out = [ExactDraws(len(r.traj), ks[j], res['seg_start'][j * n:(j + 1) * n], res['seg_state'][j * n:(j + 1) * n],
                      res['logl'][j * n:(j + 1) * n], res['uniforms'][j * n:(j + 1) * n]) for j, r in enumerate(items)]
    return out[0] if single else out


# ---------------------------------------------------------------- gradient of the exact evidence (section 20)

class EvidenceSensitivities(_Record):
    """
    `exact_sensitivities` of n trajectories, K = k_max + 1 and P parameters:

    log_marginal : (n,) log sum_k pi_k ev_k, pi the normalised prior over k
    k_posterior : (n, K) pi_k ev_k / sum pi ev
    logev : (n, K) the log evidence of every k, the numbers `exact_sample` gives
    grad : (n, P) the gradient of ``log_marginal`` with respect to the parameters
    expected_logL : (n,) the posterior mean of the log-likelihood
    fisher : (n, P, P) or None; the posterior mean of the complete-data information (innovations form).  A scoring matrix:
        the information of the marginal likelihood is smaller, so it does not give standard errors.

    A trajectory whose evidence is NaN at a k of positive prior weight (``nan='propagate'``) is NaN in all but ``logev``.
    """

    __slots__ = ('log_marginal', 'k_posterior', 'logev', 'grad', 'expected_logL', 'fisher')

    def __repr__(self):
        return f"EvidenceSensitivities(n={len(self.log_marginal)}, K={self.logev.shape[1]}, P={self.grad.shape[1]})"


def _log_k_prior(k_prior, n, K):
    """ `exact_sensitivities`' k_prior -> None or (n, K) log weights, checked """
    if k_prior is None:
        return None
    if isinstance(k_prior, (int, np.integer)) and not isinstance(k_prior, bool):
        if not 0 <= k_prior < K:
            raise ValueError(f"k_prior = {k_prior}: a single k must lie in 0 ... {K - 1}")
        w = np.zeros(K)
        w[int(k_prior)] = 1.0
    else:
        w = np.asarray(k_prior, dtype=np.float64)
    if w.shape not in ((K,), (n, K)):
        raise ValueError(f"k_prior has shape {w.shape}; None, an integer, ({K},) or ({n}, {K}) expected")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("k_prior must be finite and non-negative")
    w = np.broadcast_to(w, (n, K))
    if np.any(w.sum(axis=1) <= 0):
        raise ValueError("k_prior is zero everywhere for a trajectory")
    with np.errstate(divide='ignore'):
        return np.ascontiguousarray(np.log(w))


def exact_sensitivities(trajs, model, dmsd=None, dmsd_inf=None, dmean=None, k_max=20, k_prior=None, nan='propagate', fisher=True,
                        scratch_bytes=0):
    """
    The gradient of the exact evidence of `exact_sample` with respect to P <= 4 model parameters, for trajectories whose
    looping profile is not known (bild_gauss_segment_sensitivities).  By Fisher's identity it is the
    posterior mean over all profiles of the gradient of the log-likelihood; the posterior weights of the segments come from
    the segment recursion, the gradients from forward tangents of every window's Cholesky factor.  No sampler, no noise.

    trajs : a trajectory or a list of them (one device call)
    model : a `GenericGaussianModel` (anything else: TypeError)
    dmsd, dmsd_inf, dmean : the derivatives of the model's tables, as `GenericGaussianModel.logL_sensitivities` takes them
    k_max : largest number of switches, 0 <= k_max <= 64
    k_prior : the prior over k.  None: uniform on 0 ... k_max; an integer: that k alone; (K,) or (n_traj, K) non-negative
        weights (normalised here).  A k of weight 0 is skipped.
    nan : as for `exact_sample`.  Under 'propagate' a trajectory with a NaN evidence at a k of positive weight is NaN.
    fisher : return the posterior-weighted Fisher matrix
    scratch_bytes : device workspace of one chunk (0: the library's rule)

    Every refusal is raised before the trajectories are uploaded.  Returns `EvidenceSensitivities`.
    """
    single, items, transitions = _check_exact_sample(trajs, model, k_max, nan)
    P, given = model._derivative_arrays(dmsd, dmsd_inf, dmean)
    K = int(k_max) + 1
    prior = _log_k_prior(k_prior, len(items), K)
    if not items:
        return EvidenceSensitivities(log_marginal=np.zeros(0), k_posterior=np.zeros((0, K)), logev=np.zeros((0, K)),
                                     grad=np.zeros((0, P)), expected_logL=np.zeros(0), fisher=np.zeros((0, P, P)) if fisher else None)
    arrs = model._direct_arrays(items)
    ts = model.trajset(items[0] if single else items)
    res = _lib.gauss_segment_sensitivities(model.handle(), ts, arrs, int(k_max), transitions, log_k_prior=prior, P=P,
                                           omit=nan == 'omit', fisher=fisher, scratch_bytes=scratch_bytes, **given)
    return EvidenceSensitivities(log_marginal=res['log_marginal'], k_posterior=res['k_post'], logev=res['logev'], grad=res['grad'],
                                 expected_logL=res['exp_logl'], fisher=res['fisher'])


# ---------------------------------------------------------------- a dwell-time prior in place of the choice of k (section 21)

MAX_S_DWELL = 4


class DwellPrior:
    """
    An explicit-duration (semi-Markov) prior over looping profiles.  A profile of segments of lengths l_0 ... l_k in states
    s_0 ... s_k has

        log prior = log_init[s_0] + sum_{i<k} (log_dwell[s_i][l_i] + log_jump[s_i][s_{i+1}]) + log_surv[s_k][l_k]

    (the last segment is right-censored; a single segment over the whole trajectory gets log_init + log_surv[.][T]).

    log_init : (S,)
    log_jump : (S, S), the diagonal -inf: a self-jump would split what the likelihood treats as one segment
    log_dwell, log_surv : (S, L); column l - 1 is the entry of length l = 1 ... L, so the tables serve trajectories of up to L
        frames, of every length

    Entries are finite or -inf; `log_init` must not be -inf everywhere.  Anything else raises ValueError.  The tables need
    not be normalised.  `DwellPrior.markov` gives the geometric tables of an ordinary Markov chain.
    """

    def __init__(self, log_init, log_jump, log_dwell, log_surv):
        self.log_init = np.array(log_init, dtype=np.float64)
        self.log_jump = np.array(log_jump, dtype=np.float64)
        self.log_dwell = np.array(log_dwell, dtype=np.float64)
        self.log_surv = np.array(log_surv, dtype=np.float64)
        if self.log_init.ndim != 1 or len(self.log_init) < 1:
            raise ValueError(f"log_init has shape {self.log_init.shape}; (S,) expected")
        S = len(self.log_init)
        if self.log_jump.shape != (S, S):
            raise ValueError(f"log_jump has shape {self.log_jump.shape}; ({S}, {S}) expected")
        if self.log_dwell.ndim != 2 or self.log_dwell.shape[0] != S or self.log_dwell.shape[1] < 1:
            raise ValueError(f"log_dwell has shape {self.log_dwell.shape}; ({S}, L) with L >= 1 expected")
        if self.log_surv.shape != self.log_dwell.shape:
            raise ValueError(f"log_surv has shape {self.log_surv.shape}; that of log_dwell, {self.log_dwell.shape}, expected")
        for name in ('log_init', 'log_jump', 'log_dwell', 'log_surv'):
            a = getattr(self, name)
            if np.any(np.isnan(a)) or np.any(a == np.inf):
                raise ValueError(f"{name} has a NaN or +inf entry; entries must be finite or -inf")
        if np.any(np.diag(self.log_jump) != -np.inf):
            raise ValueError("the diagonal of log_jump must be -inf: a self-jump would split one segment into two")
        if np.all(self.log_init == -np.inf):
            raise ValueError("log_init is -inf everywhere")

    @property
    def nStates(self):
        return len(self.log_init)

    @property
    def L(self):
        """ the longest trajectory the tables serve """
        return self.log_dwell.shape[1]

    def tables(self):
        """ (log_init, log_jump, log_dwell, log_surv): the order in which the `_lib.gauss_dwell_*` calls take them """
        return self.log_init, self.log_jump, self.log_dwell, self.log_surv

    def __repr__(self):
        return f"DwellPrior(S={self.nStates}, L={self.L})"

    @classmethod
    def markov(cls, P, init=None, n=2048):
        """
        The prior of a Markov chain with row-stochastic transition matrix P (S, S) and initial distribution init (uniform where
        None), with tables for trajectories of up to n frames:

            log_dwell[s][l] = (l - 1) log P_ss + log(1 - P_ss),  log_surv[s][l] = (l - 1) log P_ss,
            log_jump[s][s'] = log(P_ss' / (1 - P_ss))

        An absorbing state (P_ss = 1) never jumps: its log_jump row and log_dwell are -inf.
        """
        P = np.asarray(P, dtype=np.float64)
        if P.ndim != 2 or P.shape[0] != P.shape[1]:
            raise ValueError(f"P has shape {P.shape}; a square matrix expected")
        S = len(P)
        if not np.all(np.isfinite(P)) or np.any(P < 0) or np.any(np.abs(P.sum(axis=1) - 1) > 1e-9):
            raise ValueError("P must be row-stochastic: finite, non-negative, rows summing to 1")
        init = np.full(S, 1.0 / S) if init is None else np.asarray(init, dtype=np.float64)
        if init.shape != (S,) or not np.all(np.isfinite(init)) or np.any(init < 0) or abs(init.sum() - 1) > 1e-9:
            raise ValueError(f"init must be a distribution over the {S} states")
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"n = {n!r}: a positive integer")
        stay = np.diag(P).copy()
        off = P - np.diag(stay)
        leave = off.sum(axis=1)     # 1 - P_ss from the entries themselves: exact for small switching probabilities
        lm1 = np.arange(n, dtype=np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            log_stay, log_leave = np.log(stay), np.log(leave)
            surv = np.where(lm1[None, :] > 0, lm1[None, :] * log_stay[:, None], 0.0)      # (0 x -inf = 0: a segment of one frame)
            log_jump = np.where(off > 0, np.log(off) - log_leave[:, None], -np.inf)
            log_init = np.log(init)
        return cls(log_init, log_jump, surv + log_leave[:, None], surv)

    @classmethod
    def from_hazard(cls, hazard, jump, init=None):
        """
        The prior whose dwell times have the discrete hazard h_s(l) = P(a segment in s ends after l frames | it reached l):

            log_surv[s][l] = sum_{m < l} log(1 - h_s(m))   (0 at l = 1),   log_dwell[s][l] = log_surv[s][l] + log h_s(l)

        hazard : (S, L), entries in [0, 1]; column l - 1 is length l.  A hazard of 1 at l admits no longer segment.
        jump : (S, S) with a zero diagonal; row s is the distribution of the state that follows s, or all zero for a state
            that never leaves, whose hazard must then be 0 everywhere
        init : (S,) distribution of the first state, uniform where None

        A constant hazard 1 - P_ss with jump P_ss' / (1 - P_ss) gives `DwellPrior.markov`'s tables.  The prior is normalised
        over the profiles of every T <= L.  Anything else raises ValueError.
        """
        hazard = np.array(hazard, dtype=np.float64)
        jump = np.array(jump, dtype=np.float64)
        if hazard.ndim != 2 or hazard.shape[1] < 1:
            raise ValueError(f"hazard has shape {hazard.shape}; (S, L) with L >= 1 expected")
        S = hazard.shape[0]
        if not np.all(np.isfinite(hazard)) or np.any(hazard < 0) or np.any(hazard > 1):
            raise ValueError("hazard must have finite entries in [0, 1]")
        if jump.shape != (S, S):
            raise ValueError(f"jump has shape {jump.shape}; ({S}, {S}) expected")
        if not np.all(np.isfinite(jump)) or np.any(jump < 0) or np.any(np.diag(jump) != 0):
            raise ValueError("jump must be finite and non-negative with a zero diagonal")
        rows = jump.sum(axis=1)
        never = np.all(jump == 0, axis=1)
        if np.any(~never & (np.abs(rows - 1) > 1e-9)):
            raise ValueError("every row of jump must sum to 1 or be all zero")
        if np.any(hazard[never] > 0):
            raise ValueError("a state whose row of jump is all zero never leaves: its hazard must be 0")
        init = np.full(S, 1.0 / S) if init is None else np.asarray(init, dtype=np.float64)
        if init.shape != (S,) or not np.all(np.isfinite(init)) or np.any(init < 0) or abs(init.sum() - 1) > 1e-9:
            raise ValueError(f"init must be a distribution over the {S} states")
        with np.errstate(divide='ignore'):
            # (the running sum in extended precision: the rounding of L additions stays below that of one)
            stay = np.log1p(-hazard).astype(np.longdouble)
            surv = np.concatenate([np.zeros((S, 1)), np.cumsum(stay, axis=1)[:, :-1].astype(np.float64)], axis=1)
            return cls(np.log(init), np.where(jump > 0, np.log(jump), -np.inf), surv + np.log(hazard), surv)

    def log_prob(self, profile):
        """ log prior of an expanded profile (a `Loopingprofile` or an integer array); host only """
        states = np.asarray(profile[:], dtype=int)
        T = len(states)
        if T < 1 or T > self.L:
            raise ValueError(f"profile of {T} frames: the tables serve 1 ... {self.L}")
        if np.any(states < 0) or np.any(states >= self.nStates):
            raise ValueError(f"profile has a state outside 0 ... {self.nStates - 1}")
        cuts = np.concatenate(([0], np.flatnonzero(np.diff(states)) + 1, [T]))
        total = self.log_init[states[0]]
        for i in range(len(cuts) - 1):
            s, length = states[cuts[i]], cuts[i + 1] - cuts[i]
            if i + 2 < len(cuts):
                total = total + self.log_dwell[s, length - 1] + self.log_jump[s, states[cuts[i + 1]]]
            else:
                total = total + self.log_surv[s, length - 1]
        return float(total)


class ExactDwellResults(_Record):
    """
    `exact_dwell` of one trajectory.

    traj, model, prior, nan : as given
    log_evidence : log sum over all profiles of prior x likelihood (NaN under nan='propagate' with `n_nan_windows` > 0)
    map_profile : the profile of largest prior x likelihood as a `Loopingprofile` (None without a profile of finite prior weight
        that uses no NaN window); map_log_joint : its log prior + log-likelihood (NaN without one)
    log_marginal_posterior : (S, T) log P(theta_t = s | data), or None when not asked for
    expected_jumps : (S, S) posterior expected number of jumps s -> s'; expected_stay : (S,) posterior expected number of frames
        stayed in s (sum of length - 1 over its segments): the derivatives of `log_evidence` with respect to `log_jump` and to
        a Markov chain's log P_ss.  None without marginals.
    n_nan_windows : windows skipped because their table entry is NaN, among those of finite prior weight with a reachable start
    """

    __slots__ = ('traj', 'model', 'prior', 'nan', 'log_evidence', 'map_profile', 'map_log_joint', 'log_marginal_posterior',
                 'expected_jumps', 'expected_stay', 'n_nan_windows')

    def __repr__(self):
        return (f"ExactDwellResults(T={len(self.traj)}, log_evidence={self.log_evidence!r}, map_log_joint={self.map_log_joint!r}, "
                f"n_nan_windows={self.n_nan_windows})")

    def draw(self, n, seed=0, uniforms=None, keep_uniforms=0):
        """ n profiles drawn from the exact posterior under the prior as `ExactDwellDraws`: `exact_dwell_draw` of these results """
        return exact_dwell_draw(self, n, seed=seed, uniforms=uniforms, keep_uniforms=keep_uniforms)

    def posterior_distance(self, n=1000, seed=0):
        """
        (mean, var), each (T, d): the smoothed track averaged over n profiles drawn from the exact posterior under the prior,
        in one `model.kalman_mixture` call with equal weights -- the counterpart of `ExactSamplingResults.posterior_distance`
        """
        draws = exact_dwell_draw(self, n, seed=seed)
        mean, var = self.model.kalman_mixture(draws.segments(), [self.traj], np.zeros(len(draws)))
        return mean[0], var[0]

    def map_support(self, radii=(0, 2, 5), scratch_bytes=0):
        """
        How well the exact posterior supports the MAP profile, as `DwellMapSupport`, from ONE `exact_dwell_windows` call: per
        called segment the probability that every frame of it is in its state and that none is, and per called switch frame c
        and radius r of ``radii`` (non-negative integers) the probability of at least one switch at the frames c - r ... c + r.
        ValueError without a MAP profile, for a model of one state, and for a radius that is not a non-negative integer.
        """
        S = self.model.msd.shape[0]
        if self.map_profile is None:
            raise ValueError("the results have no MAP profile to support")
        if S < 2:
            raise ValueError("a model of one state has no other profile: nothing to support")
        radii = tuple(radii)
        if any(isinstance(r, bool) or not isinstance(r, (int, np.integer)) or r < 0 for r in radii):
            raise ValueError(f"radii = {radii!r}: non-negative integers")
        states = np.asarray(self.map_profile[:], dtype=int)
        T = len(states)
        starts = np.concatenate(([0], np.flatnonzero(np.diff(states) != 0) + 1))
        ends = np.append(starts[1:], T)
        seg_state = states[starts]
        windows = []
        for a, b, s in zip(starts, ends, seg_state):
            windows.append((int(a), int(b), (int(s),)))
            windows.append((int(a), int(b), tuple(r for r in range(S) if r != s)))
        for c in starts[1:]:
            for r in radii:
                windows.extend((max(int(c) - int(r) - 1, 0), min(int(c) + int(r) + 1, T), (s,)) for s in range(S))
        res = exact_dwell_windows(self.traj, self.model, self.prior, windows, nan=self.nan, scratch_bytes=scratch_bytes)
        n_seg = len(starts)
        same = np.exp(res.log_all[2 * n_seg:]).reshape(n_seg - 1, len(radii), S)
        return DwellMapSupport(traj=self.traj, model=self.model, prior=self.prior, nan=self.nan, radii=radii, seg_start=starts, seg_end=ends,
                               seg_state=seg_state, log_whole=res.log_all[0:2 * n_seg:2].copy(), log_absent=res.log_all[1:2 * n_seg:2].copy(),
                               switch_frames=starts[1:].copy(), p_switch_within=1.0 - same.sum(axis=2), n_queries=len(windows),
                               log_evidence=res.log_evidence, n_nan_windows=res.n_nan_windows)


def _check_exact_dwell(trajs, model, prior, nan):
    """ every refusal of `exact_dwell`; returns (single, items) """
    from .gauss import GenericGaussianModel
    if not isinstance(model, GenericGaussianModel):
        raise TypeError(f"exact_dwell needs a GenericGaussianModel, whose log-likelihood is a sum of segment terms, not "
                        f"{type(model).__name__}")
    if not isinstance(prior, DwellPrior):
        raise TypeError(f"prior must be a DwellPrior, not {type(prior).__name__}")
    if nan not in ('propagate', 'omit'):
        raise ValueError(f"nan = {nan!r}: 'propagate' or 'omit'")
    S = model.msd.shape[0]
    if prior.nStates != S:
        raise ValueError(f"the prior has {prior.nStates} states, the model {S}")
    if S > MAX_S_DWELL:
        raise ValueError(f"the model has {S} states: the dwell-time recursion supports at most {MAX_S_DWELL}")
    single = not isinstance(trajs, (list, tuple))
    items = [trajs] if single else list(trajs)
    for t in items:
        if len(t) > model.max_T:
            raise ValueError(f"trajectory of {len(t)} frames: GenericGaussianModel evaluates at most {model.max_T} frames")
        if len(t) > prior.L:
            raise ValueError(f"trajectory of {len(t)} frames: the prior's tables serve at most {prior.L}")
    return single, items


def _dwell_per_trajectory(call, cls, single, items, model, prior, nan, fields, *scalars, **options):
    """
    What the `exact_dwell*` entry points share behind their refusals, (single, items) as `_check_exact_dwell` returns them.
    Without items the answer is [] and nothing is uploaded; else ONE trajectory set of them and ONE ``call`` -- a
    `_lib.gauss_dwell_*` -- on it with the prior's tables, the entry point's own ``scalars`` and ``options``.  Trajectory j
    becomes a ``cls`` of traj, model, prior, nan, log_evidence and the entry point's own ``fields(res, j, T)``; a single
    trajectory gives its result, a list a list.
    """
    if not items:
        return []
    ts = model.trajset(items[0] if single else items)
    res = call(model.handle(), ts, *prior.tables(), *scalars, omit=nan == 'omit', **options)
    out = [cls(traj=t, model=model, prior=prior, nan=nan, log_evidence=float(res['logev'][j]), **fields(res, j, len(t)))
           for j, t in enumerate(items)]
    return out[0] if single else out


def exact_dwell(trajs, model, prior, marginals=True, nan='propagate', scratch_bytes=0):
    """
    Exact inference for a `GenericGaussianModel` under a dwell-time prior (`DwellPrior`) in place of "uniform over the profiles
    of one k, k chosen by evidence": one evidence per trajectory over the profiles of every number of switches, the MAP
    profile, the state marginals, and the expected jump and stay counts, by one forward and one backward recursion over
    segments on the GPU (bild_gauss_dwell_evidence).

    trajs : a trajectory or a list of them; a list gives a list of results from ONE device call
    model : a `GenericGaussianModel` with at most 4 states (anything else: TypeError).  The prior's `log_jump` decides which
        jumps exist; `model.transitions` is not consulted.
    prior : a `DwellPrior` over the model's states whose tables cover the longest trajectory
    marginals : compute `log_marginal_posterior`, `expected_jumps` and `expected_stay` (the backward pass)
    nan : 'propagate' -- a trajectory with `n_nan_windows` > 0 (a later ss_order-0 segment without a valid frame that the prior
        allows and a profile reaches) has NaN evidence, marginals and counts; its MAP profile is still taken among the
        profiles that use no such window.  'omit' -- the profiles that use such a window weigh 0: the evidence is then that of
        the prior RESTRICTED to the remaining profiles, not renormalised over them.
    scratch_bytes : device workspace of one chunk of whole trajectories (0: at most 1 GiB and a third of the free memory)

    MAP ties are broken as in `exact_sample`: the smallest final state, then from the last switch backwards the smallest
    switch frame and the smallest preceding state.  Every refusal is raised before the trajectories are uploaded.  Returns
    `ExactDwellResults` or a list of them.
    """
    single, items = _check_exact_dwell(trajs, model, prior, nan)

    def fields(res, j, T):
        states = res['map_states'][j, :T]
        marg = res['log_post'] is not None
        return dict(map_profile=None if T == 0 or states[0] == 255 else Loopingprofile(states.astype(int)),
                    map_log_joint=float(res['map_logjoint'][j]), log_marginal_posterior=res['log_post'][j, :, :T].copy() if marg else None,
                    expected_jumps=res['exp_jumps'][j].copy() if marg else None, expected_stay=res['exp_stay'][j].copy() if marg else None,
                    n_nan_windows=int(res['n_nan_windows'][j]))
    return _dwell_per_trajectory(_lib.gauss_dwell_evidence, ExactDwellResults, single, items, model, prior, nan, fields,
                                 marginals=marginals, scratch_bytes=scratch_bytes)


# ---------------------------------------------------------------- online filtering under the dwell-time prior (section 25)

class DwellFilterResults(_Record):
    """
    `exact_dwell_filter` of one trajectory of T frames: at frame t, what `exact_dwell` says about the truncation x[:t + 1].

    traj, model, prior, nan : as given
    log_evidence : the evidence of the whole trajectory, `exact_dwell`'s number bit for bit
    prefix_log_evidence : (T,) the evidence of x[:t + 1] under the same prior tables
    log_predictive : (T,) `prefix_log_evidence[t] - prefix_log_evidence[t - 1]`, the first entry `prefix_log_evidence[0]`.
        This is log p(x_t | x_0 ... x_{t-1}) ONLY for a prior whose tables are consistent under truncation:
        `log_surv[s][l]` = log sum_{l' >= l} exp(`log_dwell[s][l']`) with normalised jumps, as `DwellPrior.markov` and
        `DwellPrior.from_hazard` build them; the terms then add up to `log_evidence` frame by frame.  For other tables it is
        only a difference of two evidences.
    log_filtered : (S, T) log P(theta_t = s | x_0 ... x_t)
    run_length_mean : (T,) the expected number of frames that the segment containing frame t has lasted, given x_0 ... x_t
    log_run_length : (S, T, run_max) log P(theta_t = s, the current segment has lasted r frames | x_0 ... x_t) at [s, t, r - 1],
        -inf for r > t + 1; None without `run_max`
    n_nan_windows : (T,) `exact_dwell`'s `n_nan_windows` of x[:t + 1]

    Under nan='propagate' every array is NaN at the frames with `n_nan_windows[t]` > 0 and untouched before; a frame whose
    prefix has no profile of positive weight has `prefix_log_evidence` -inf and NaN elsewhere.
    """

    __slots__ = ('traj', 'model', 'prior', 'nan', 'log_evidence', 'prefix_log_evidence', 'log_predictive', 'log_filtered',
                 'run_length_mean', 'log_run_length', 'n_nan_windows')

    def __repr__(self):
        return f"DwellFilterResults(T={len(self.traj)}, log_evidence={self.log_evidence!r})"


def exact_dwell_filter(trajs, model, prior, run_max=0, nan='propagate', scratch_bytes=0):
    """
    Exact online (causal) inference for a `GenericGaussianModel` under a dwell-time prior: for every frame t the state
    probabilities, the distribution of how long the current segment has lasted (the Bayesian online change-point quantity) and
    the evidence given the data up to t alone, from the forward pass of `exact_dwell` and one more kernel without a
    sequential chain (bild_gauss_dwell_filter).

    trajs, model, prior, nan, scratch_bytes : as for `exact_dwell`; a list gives a list of results from ONE device call
    run_max : run lengths r = 1 ... run_max kept in `log_run_length` (0: not computed; S x T x run_max doubles a trajectory)

    Every refusal of `exact_dwell`, and a negative `run_max`, is raised before the trajectories are uploaded.  Returns
    `DwellFilterResults` or a list of them.
    """
    single, items = _check_exact_dwell(trajs, model, prior, nan)
    if int(run_max) != run_max or run_max < 0:
        raise ValueError(f"run_max = {run_max!r}: an integer >= 0")

    def fields(res, j, T):
        prefix = res['prefix_logev'][j, :T].copy()
        with np.errstate(invalid='ignore'):
            predictive = np.diff(prefix, prepend=0.0)
        return dict(prefix_log_evidence=prefix, log_predictive=predictive, log_filtered=res['log_filtered'][j, :, :T].copy(),
                    run_length_mean=res['run_mean'][j, :T].copy(),
                    log_run_length=None if res['log_run'] is None else res['log_run'][j, :, :T].copy(),
                    n_nan_windows=res['n_nan_windows'][j, :T].copy())
    return _dwell_per_trajectory(_lib.gauss_dwell_filter, DwellFilterResults, single, items, model, prior, nan, fields,
                                 run_max=int(run_max), scratch_bytes=scratch_bytes)


# ---------------------------------------------------------------- fixed-lag smoothing under the dwell-time prior (section 26)

MAX_DWELL_LAG = _lib.DWELL_LAG_MAX


class DwellLagResults(_Record):
    """
    `exact_dwell_lag` of one trajectory of T frames: at frame t and lag l, what `exact_dwell` says about frame t of the
    truncation x[:t + l + 1].

    traj, model, prior, nan, lag : as given
    log_evidence : the evidence of the whole trajectory, `exact_dwell`'s number bit for bit
    log_lagged : (S, T, lag + 1) log P(theta_t = s | x_0 ... x_{t + l}) at [s, t, l].  Column 0 is `exact_dwell_filter`'s
        `log_filtered`.  Where t + l + 1 >= T the data end and the entry is `exact_dwell`'s smoothed marginal: the last columns
        of the last frames repeat, and with lag >= T - 1 column `lag` is the smoothed marginal at every frame.
    n_nan_windows : (T,) `exact_dwell`'s `n_nan_windows` of x[:t + 1]

    Under nan='propagate' entry [:, t, l] is NaN where the truncation it speaks of, x[:min(t + l + 1, T)], has
    `n_nan_windows` > 0; a truncation without a profile of positive weight has NaN in all its entries.
    """

    __slots__ = ('traj', 'model', 'prior', 'nan', 'lag', 'log_evidence', 'log_lagged', 'n_nan_windows')

    def __repr__(self):
        return f"DwellLagResults(T={len(self.traj)}, lag={self.lag}, log_evidence={self.log_evidence!r})"

    def fixed_lag(self, lag):
        """ (S, T) log P(theta_t = s | x_0 ... x_{t + lag}): column `lag` of `log_lagged` """
        if int(lag) != lag or not 0 <= lag <= self.lag:
            raise ValueError(f"lag = {lag!r}: an integer in 0 ... {self.lag}")
        return self.log_lagged[:, :, int(lag)]

    def settling_lag(self, tol=1e-3):
        """
        (T,) int64: per frame the smallest l from which every later computed column stays within `tol` (in probability, the
        maximum over the states) of column `lag`; `lag` where only that column does, -1 at a frame with a NaN entry.  The
        columns l > T - 1 - t are not computed from more data: they repeat column T - 1 - t.  NumPy on the host.
        """
        return settling_lag(self.log_lagged, tol)


def settling_lag(log_lagged, tol=1e-3):
    """ `DwellLagResults.settling_lag` of an (S, T, lag + 1) array """
    log_lagged = np.asarray(log_lagged, dtype=np.float64)
    S, T, n = log_lagged.shape
    p = np.exp(log_lagged)
    off = np.max(np.abs(p - p[:, :, -1:]), axis=0) > tol        # (T, lag + 1); NaN compares False
    # the last column that is off, -1 where none is: the answer is the column behind it
    last_off = np.where(off.any(axis=1), n - 1 - np.argmax(off[:, ::-1], axis=1), -1)
    out = (last_off + 1).astype(np.int64)
    out[np.isnan(p).any(axis=(0, 2))] = -1
    return out


def exact_dwell_lag(trajs, model, prior, lag, nan='propagate', scratch_bytes=0):
    """
    Exact fixed-lag smoothing for a `GenericGaussianModel` under a dwell-time prior: for every frame t the state probabilities
    given the data up to frame t + l, for every l = 0 ... `lag` at once -- the filter of `exact_dwell_filter` at l = 0, the
    smoothed marginals of `exact_dwell` once the data end, and the whole curve in between: what a delayed online decision
    gains, and how much data behind a frame its smoothed answer needs.  From the forward pass of `exact_dwell`, two sums of the
    size of the filter's on tables that are built once, and one short backward chain per truncation
    (bild_gauss_dwell_lag).

    trajs, model, prior, nan, scratch_bytes : as for `exact_dwell`; a list gives a list of results from ONE device call
    lag : the largest lag, an integer in 0 ... 63 (a window of lag + 1 frames is one wavefront); S x T x (lag + 1) doubles a
        trajectory

    Every refusal of `exact_dwell`, and a `lag` that is no integer, negative or above 63, is raised before the trajectories are
    uploaded.  Returns `DwellLagResults` or a list of them.
    """
    single, items = _check_exact_dwell(trajs, model, prior, nan)
    if isinstance(lag, (bool, np.bool_)) or int(lag) != lag or lag < 0:
        raise ValueError(f"lag = {lag!r}: an integer >= 0")
    if lag > MAX_DWELL_LAG:
        raise ValueError(f"lag = {lag}: at most {MAX_DWELL_LAG}")
    fields = lambda res, j, T: dict(lag=int(lag), log_lagged=res['log_lagged'][j, :, :T].copy(),
                                    n_nan_windows=res['n_nan_windows'][j, :T].copy())
    return _dwell_per_trajectory(_lib.gauss_dwell_lag, DwellLagResults, single, items, model, prior, nan, fields, int(lag),
                                 scratch_bytes=scratch_bytes)


# ---------------------------------------------------------------- profiles drawn under the dwell-time prior (section 22)

class ExactDwellDraws:
    """
    Profiles of one trajectory drawn independently from the exact posterior under a dwell-time prior (`exact_dwell_draw`).

    T : frames of the trajectory
    n_switches : (n,) switches of each draw
    logL, log_prior : (n,) log-likelihood and log prior of each drawn profile, from the tables the draw was made on
    n_uniforms : (n,) uniforms each draw consumed, 1 + 2 `n_switches`
    uniforms : (n, U) the first U uniforms each draw consumed (0 where none was), U = ``keep_uniforms`` or the width of the
        replayed rows; None when neither was given.  Given back as ``uniforms=`` they reproduce the draws.
    """

    def __init__(self, T, states, n_switches, logL, log_prior, n_uniforms, uniforms):
        self.T = int(T)
        self._states = np.asarray(states, dtype=np.uint8)
        self.n_switches = np.asarray(n_switches, dtype=np.int64)
        self.logL = np.asarray(logL, dtype=np.float64)
        self.log_prior = np.asarray(log_prior, dtype=np.float64)
        self.n_uniforms = np.asarray(n_uniforms, dtype=np.int64)
        self.uniforms = None if uniforms is None else np.asarray(uniforms, dtype=np.float64)

    def __len__(self):
        return len(self.n_switches)

    def __repr__(self):
        return f"ExactDwellDraws(n={len(self)}, T={self.T}, n_switches={np.unique(self.n_switches).tolist()})"

    def states(self):
        """ (n, T) int array: the state of every frame of every draw """
        return self._states[:, :self.T].astype(int)

    def profiles(self):
        """ the draws as a list of `Loopingprofile` """
        return [Loopingprofile(row) for row in self.states()]

    def segments(self):
        """ (seg_start, seg_state), each (n, max switches + 1) int32: run-length rows padded with empty segments at T """
        if len(self) == 0:
            return np.zeros((0, 1), dtype=np.int32), np.zeros((0, 1), dtype=np.int32)
        return segments_from_states(self.states())

    def dwell_lengths(self, state, completed=True):
        """
        the lengths of the drawn segments in ``state``, concatenated over the draws; ``completed`` leaves out each draw's
        last segment, which the end of the trajectory censors (host only)
        """
        st = self._states[:, :self.T]
        n, T = st.shape
        if n == 0 or T == 0:
            return np.zeros(0, dtype=np.int64)
        first = np.ones((n, T), dtype=bool)
        first[:, 1:] = st[:, 1:] != st[:, :-1]
        rows, starts = np.nonzero(first)
        last = np.append(rows[1:] != rows[:-1], True)       # the segment is its draw's last
        ends = np.where(last, T, np.append(starts[1:], T))
        use = st[rows, starts] == state
        if completed:
            use &= ~last
        return (ends - starts)[use].astype(np.int64)

    def first_contact(self, target):
        """
        (n,) int array: the first frame of each draw whose state is ``target`` or, for a collection, one of its states; -1 where
        the draw never is (host only).  The histogram counterpart of `exact_dwell_first_contact`.
        """
        wanted = [target] if isinstance(target, (int, np.integer)) else list(target)
        hit = np.isin(self._states[:, :self.T], np.asarray(wanted, dtype=np.int64))
        return np.where(hit.any(axis=1), hit.argmax(axis=1), -1).astype(np.int64)

    def occupancy(self, target):
        """
        (n,) int array: the number of frames of each draw whose state is ``target`` or, for a collection, one of its states
        (host only).  The histogram counterpart of `exact_dwell_occupancy`.
        """
        wanted = [target] if isinstance(target, (int, np.integer)) else list(target)
        return np.isin(self._states[:, :self.T], np.asarray(wanted, dtype=np.int64)).sum(axis=1).astype(np.int64)

    def visits(self, target):
        """
        (n,) int array: the number of visits of each draw to ``target`` or, for a collection, to the set of its states: the
        maximal runs of consecutive frames in the set, a run at frame 0 and a run that reaches frame T - 1 included (host only).
        The histogram counterpart of `exact_dwell_visits`.
        """
        wanted = [target] if isinstance(target, (int, np.integer)) else list(target)
        hit = np.isin(self._states[:, :self.T], np.asarray(wanted, dtype=np.int64))
        if hit.shape[1] == 0:
            return np.zeros(len(hit), dtype=np.int64)
        return (hit[:, 0].astype(np.int64) + (hit[:, 1:] & ~hit[:, :-1]).sum(axis=1)).astype(np.int64)

    def all_in(self, u, v, target):
        """
        the fraction of the draws with every frame of [u, v), 0 <= u < v <= T, in ``target`` or, for a collection, in one of its
        states (host only; NaN without draws).  The counting counterpart of `exact_dwell_windows`, with the standard error
        sqrt(p (1 - p) / n) of a count.
        """
        if not 0 <= u < v <= self.T:
            raise ValueError(f"window [{u}, {v}): 0 <= u < v <= T = {self.T} expected")
        wanted = [target] if isinstance(target, (int, np.integer)) else list(target)
        if len(self) == 0:
            return float('nan')
        return float(np.isin(self._states[:, u:v], np.asarray(wanted, dtype=np.int64)).all(axis=1).mean())


def exact_dwell_draw(results, n, seed=0, uniforms=None, keep_uniforms=0, scratch_bytes=0):
    """
    n profiles per trajectory, drawn independently from the exact posterior under the dwell-time prior of `exact_dwell`, by
    sampling segment after segment against the backward tables of the dwell-time recursion on the GPU (DESIGN.md section
    22): no burn-in, no weights, no k and no k_max.

    results : an `ExactDwellResults` or a list of them over one model and one prior; a list is served by ONE device call on
        one trajectory set and gives a list of `ExactDwellDraws`
    n : draws per result
    seed : of the device's uniforms; draw i of result j is stream j n + i
    uniforms : replay -- (n, U) uniforms in [0, 1), for a list of results (len(results), n, U), U >= 1: rows of
        `ExactDwellDraws.uniforms` of an earlier call; ``seed`` is then not used.  A draw of k switches consumes 1 + 2k of
        its row; a row that is too short raises ValueError (U = 2T - 1 always suffices).
    keep_uniforms : device mode -- return the first ``keep_uniforms`` uniforms each draw consumed
    scratch_bytes : device workspace of one chunk of whole trajectories (0: at most 1 GiB and a third of the free memory)

    Profiles that use a NaN window are never drawn: results made with nan='omit' give draws from the posterior without
    them; results made with nan='propagate' that have `n_nan_windows` > 0, and results whose `log_evidence` is -inf, raise
    ValueError.  Every refusal but the short replay row is raised before any upload.  Returns an `ExactDwellDraws` or a
    list of them.
    """
    single = isinstance(results, ExactDwellResults)
    if not single and not isinstance(results, (list, tuple)):
        raise TypeError(f"exact_dwell_draw needs ExactDwellResults (from exact_dwell) or a list of them, not {type(results).__name__}")
    items = [results] if single else list(results)
    if any(not isinstance(r, ExactDwellResults) for r in items):
        raise TypeError("exact_dwell_draw needs ExactDwellResults (from exact_dwell) or a list of them")
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError(f"n = {n!r}: a non-negative integer")
    if isinstance(keep_uniforms, bool) or not isinstance(keep_uniforms, (int, np.integer)) or keep_uniforms < 0:
        raise ValueError(f"keep_uniforms = {keep_uniforms!r}: a non-negative integer")
    n = int(n)
    if not items:
        return []
    model, prior = items[0].model, items[0].prior
    if any(r.model is not model for r in items):
        raise ValueError("exact_dwell_draw needs results over one model")
    if any(r.prior is not prior for r in items):
        raise ValueError("exact_dwell_draw needs results under one prior")
    for j, r in enumerate(items):
        if r.nan == 'propagate' and r.n_nan_windows > 0:
            raise ValueError(f"result {j} was made with nan='propagate' and has {r.n_nan_windows} NaN windows: make the results "
                             f"with nan='omit', which leaves the profiles that use them out")
        if r.log_evidence == -np.inf:
            raise ValueError(f"the log evidence of result {j} is -inf: no profile of positive weight to draw")
    U = int(keep_uniforms)
    if uniforms is not None:
        uniforms = np.asarray(uniforms, dtype=np.float64)
        if uniforms.ndim != (2 if single else 3) or uniforms.shape[:-1] != ((n,) if single else (len(items), n)) or uniforms.shape[-1] < 1:
            want = f"({n}, U)" if single else f"({len(items)}, {n}, U)"
            raise ValueError(f"uniforms has shape {uniforms.shape}; {want} with U >= 1 expected")
        if not np.all((uniforms >= 0) & (uniforms < 1)):
            raise ValueError("uniforms must lie in [0, 1) (NaN or a value outside given)")
        U = uniforms.shape[-1]
        uniforms = uniforms.reshape(len(items) * n, U)
    if n == 0:
        out = [ExactDwellDraws(len(r.traj), np.zeros((0, len(r.traj)), dtype=np.uint8), np.zeros(0), np.zeros(0), np.zeros(0),
                               np.zeros(0), np.zeros((0, U)) if U else None) for r in items]
        return out[0] if single else out
    ts = model.trajset(items[0].traj if single else [r.traj for r in items])
    res = _lib.gauss_dwell_draw(model.handle(), ts, *prior.tables(), np.repeat(np.arange(len(items)), n), uniforms=uniforms,
                                keep_uniforms=U, seed=seed, scratch_bytes=scratch_bytes)
    short = np.flatnonzero(res['n_uniforms'] < 0)
    if len(short):
        j, i = divmod(int(short[0]), n)
        T = len(items[j].traj)
        raise ValueError(f"draw {i}" + ("" if single else f" of result {j}") + f" needs more than the {U} uniforms of its row: "
                         f"rows of 2T - 1 = {2 * T - 1} uniforms always suffice")
    out = []
    for j, r in enumerate(items):
        rows = slice(j * n, (j + 1) * n)
        out.append(ExactDwellDraws(len(r.traj), res['states'][rows], res['n_switches'][rows], res['logl'][rows], res['log_prior'][rows],
                                   res['n_uniforms'][rows], None if res['uniforms'] is None else res['uniforms'][rows]))
    return out[0] if single else out


class MarkovPriorFit(_Record):
    """
    `fit_markov_prior`'s result: P (S, S) and init (S,), the total log evidence of the data set at every iteration's
    parameters (`log_evidence`, one entry per device call; the last belongs to the parameters one M-step before P),
    n_iter and converged.  `prior(n)` is `DwellPrior.markov(P, init, n)`.
    """

    __slots__ = ('P', 'init', 'log_evidence', 'n_iter', 'converged')

    def __repr__(self):
        return f"MarkovPriorFit(n_iter={self.n_iter}, converged={self.converged}, P={self.P!r})"

    def prior(self, n=2048):
        return DwellPrior.markov(self.P, self.init, n=n)


class EvidenceNotFinite(ValueError):
    """ `fit_markov_prior`: the total log evidence of the data set is NaN or -inf; ``total`` holds it """

    def __init__(self, total):
        self.total = float(total)
        super().__init__(f"the total log evidence is {total}: " + ("a trajectory has NaN windows, use nan='omit'"
                                                                   if np.isnan(total) else "a trajectory has no profile of positive weight"))


def _fit_model(name, model):
    """ the first refusal of `fit_markov_prior` and `fit_dwell_prior` (``name`` in the messages): TypeError unless a GenericGaussianModel """
    from .gauss import GenericGaussianModel
    if not isinstance(model, GenericGaussianModel):
        raise TypeError(f"{name} needs a GenericGaussianModel, whose log-likelihood is a sum of segment terms, not "
                        f"{type(model).__name__}")


def _fit_trajs(name, trajs):
    """ the trajectories of `fit_markov_prior` and `fit_dwell_prior`, at least one (ValueError) -> (single, items, n), n the frames of the longest """
    single = not isinstance(trajs, (list, tuple))
    items = [trajs] if single else list(trajs)
    if not items:
        raise ValueError(f"{name} needs at least one trajectory")
    return single, items, max(len(t) for t in items)


def _markov_start(model, start):
    """ `fit_markov_prior`'s start -> (allowed (S, S) off-diagonal transitions, P (S, S), init (S,)), checked """
    S = model.msd.shape[0]
    allowed = np.asarray(model.transitions, dtype=bool).copy()
    if allowed.shape != (S, S):
        raise ValueError(f"model.transitions has shape {allowed.shape}; ({S}, {S}) expected")
    np.fill_diagonal(allowed, False)
    init = None
    if start is None:
        n_out = allowed.sum(axis=1)
        P = np.where(allowed, 0.1 / np.maximum(n_out, 1)[:, None], 0.0)
        P[np.arange(S), np.arange(S)] = 1.0 - P.sum(axis=1)
    else:
        if isinstance(start, tuple):
            start, init = start
        P = np.array(start, dtype=np.float64)
        if P.shape != (S, S):
            raise ValueError(f"start has shape {P.shape}; ({S}, {S}) expected")
        if np.any((P > 0) & ~allowed & ~np.eye(S, dtype=bool)):
            raise ValueError("start has a positive entry that model.transitions forbids")
    init = np.full(S, 1.0 / S) if init is None else np.array(init, dtype=np.float64)
    return allowed, P, init


def fit_markov_prior(trajs, model, start=None, tol=1e-8, max_iter=200, nan='propagate'):
    """
    Maximum-likelihood switching rates of a data set: EM over the transition matrix P and the initial distribution of a Markov
    prior on the looping profiles, the model held fixed.  The trajectory set with its tables is built once; every iteration
    is one `exact_dwell` device call on it, whose expected counts are the E-step:

        P_ss' proportional to sum exp_jumps[s][s'],  P_ss proportional to sum exp_stay[s],  init_s = mean P(theta_0 = s)

    trajs : a list of trajectories (or one)
    model : a `GenericGaussianModel`; transitions that `model.transitions` forbids stay 0
    start : None -- P_ss = 0.9, the rest spread evenly over the allowed transitions, uniform init; a matrix P; or (P, init)
    tol : stop when an M-step moves no entry of P by more than this
    max_iter : at most this many device calls
    nan : as for `exact_dwell`; a NaN total evidence ('propagate' with NaN windows) raises ValueError

    The total log evidence never decreases.  A state that the posterior never visits keeps its row.  Returns `MarkovPriorFit`.
    """
    _fit_model('fit_markov_prior', model)
    S = model.msd.shape[0]
    allowed, P, init = _markov_start(model, start)
    if not (tol > 0) or isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"tol = {tol!r} must be positive and max_iter = {max_iter!r} a positive integer")
    single, items, n = _fit_trajs('fit_markov_prior', trajs)
    _check_exact_dwell(items, model, DwellPrior.markov(P, init, n=n), nan)

    ts = model.trajset(items[0] if single else items)       # built once: the iterations change the prior, not the tables
    history, converged = [], False
    for _ in range(int(max_iter)):
        prior = DwellPrior.markov(P, init, n=n)
        res = _lib.gauss_dwell_evidence(model.handle(), ts, *prior.tables(), marginals=True, omit=nan == 'omit')
        total = float(np.sum(res['logev']))
        if not np.isfinite(total):
            raise EvidenceNotFinite(total)
        history.append(total)
        jumps, stay = res['exp_jumps'].sum(axis=0), res['exp_stay'].sum(axis=0)
        jumps = np.where(allowed, jumps, 0.0)
        denom = stay + jumps.sum(axis=1)
        new = P.copy()
        for s in range(S):
            if denom[s] > 0:
                new[s] = jumps[s] / denom[s]
                new[s, s] = stay[s] / denom[s]
        first = np.array([np.exp(res['log_post'][j, :, 0]) for j in range(len(items))]).mean(axis=0)
        step = float(np.max(np.abs(new - P)))
        P, init = new, first / first.sum()
        if step < tol:
            converged = True
            break
    return MarkovPriorFit(P=P, init=init, log_evidence=np.array(history), n_iter=len(history), converged=converged)


# ---------------------------------------------------------------- gradient of the evidence under the dwell-time prior (section 23)

class DwellSensitivities(_Record):
    """
    `exact_dwell_sensitivities` of n trajectories and P parameters:

    log_evidence : (n,) the log evidence under the prior, the numbers `exact_dwell` gives
    n_nan_windows : (n,) int64, as `exact_dwell` counts them
    grad : (n, P) the gradient of ``log_evidence`` with respect to the parameters
    expected_logL : (n,) the posterior mean of the log-likelihood
    fisher : (n, P, P) or None; the posterior mean of the complete-data information (innovations form).  A scoring matrix:
        the information of the marginal likelihood is smaller, so it does not give standard errors.

    A trajectory with NaN windows under ``nan='propagate'`` is NaN in all but ``n_nan_windows``; a trajectory without a profile
    of positive weight has ``log_evidence`` -inf and NaN in ``grad``, ``expected_logL`` and ``fisher``.
    """

    __slots__ = ('log_evidence', 'n_nan_windows', 'grad', 'expected_logL', 'fisher')

    def __repr__(self):
        return f"DwellSensitivities(n={len(self.log_evidence)}, P={self.grad.shape[1]})"


def exact_dwell_sensitivities(trajs, model, prior, dmsd=None, dmsd_inf=None, dmean=None, nan='propagate', fisher=True, scratch_bytes=0):
    """
    The gradient of the exact evidence of `exact_dwell` with respect to P <= 4 model parameters, for trajectories whose looping
    profile is not known (bild_gauss_dwell_sensitivities).  The prior does not depend on the model's
    parameters, so by Fisher's identity the gradient is the posterior mean over all profiles of the gradient of the
    log-likelihood; the posterior weights of the segments come from the forward and backward tables of the dwell-time
    recursion, the gradients from forward tangents of every window's Cholesky factor.  No sampler, no noise, no k_max.

    trajs : a trajectory or a list of them (one device call)
    model : a `GenericGaussianModel` with at most 4 states (anything else: TypeError)
    prior : a `DwellPrior` over the model's states whose tables cover the longest trajectory
    dmsd, dmsd_inf, dmean : the derivatives of the model's tables, as `GenericGaussianModel.logL_sensitivities` takes them
    nan : as for `exact_dwell`.  Under 'propagate' a trajectory with NaN windows is NaN; under 'omit' those windows weigh 0.
    fisher : return the posterior-weighted Fisher matrix.  It is the posterior mean of the complete-data information, a
        scoring matrix for a fit; it is NOT the information of the marginal likelihood, which is smaller by the posterior
        covariance of the score, so it does not give standard errors.
    scratch_bytes : device workspace of one chunk (0: the library's rule)

    Every refusal is raised before the trajectories are uploaded.  Returns `DwellSensitivities`.
    """
    single, items = _check_exact_dwell(trajs, model, prior, nan)
    P, given = model._derivative_arrays(dmsd, dmsd_inf, dmean)
    if not items:
        return DwellSensitivities(log_evidence=np.zeros(0), n_nan_windows=np.zeros(0, dtype=np.int64), grad=np.zeros((0, P)),
                                  expected_logL=np.zeros(0), fisher=np.zeros((0, P, P)) if fisher else None)
    arrs = model._direct_arrays(items)
    ts = model.trajset(items[0] if single else items)
    res = _lib.gauss_dwell_sensitivities(model.handle(), ts, arrs, *prior.tables(), P=P, omit=nan == 'omit', fisher=fisher,
                                         scratch_bytes=scratch_bytes, **given)
    return DwellSensitivities(log_evidence=res['logev'], n_nan_windows=res['n_nan_windows'], grad=res['grad'],
                              expected_logL=res['exp_logl'], fisher=res['fisher'])


# ---------------------------------------------------------------- expected segment lengths and a fit of the dwell-time prior (section 24)

class DwellLengthCounts(_Record):
    """
    `exact_dwell_lengths` of one trajectory of T frames: the derivatives of `log_evidence` with respect to the prior's logs,
    which are posterior expected counts.

    traj, model, prior, nan : as given
    log_evidence, n_nan_windows, expected_jumps (S, S) : `exact_dwell`'s numbers, bit for bit
    expected_init : (S,) P(theta_0 = s | data)
    expected_dwell : (S, T); column l - 1 is the expected number of completed segments in state s of l frames (0 at l = T)
    expected_censored : (S, T); column l - 1 is the probability that the last, right-censored segment is in s with l frames

    Under nan='propagate' a trajectory with `n_nan_windows` > 0 is NaN in all but `n_nan_windows`; a trajectory without a
    profile of positive weight has `log_evidence` -inf and NaN counts.
    """

    __slots__ = ('traj', 'model', 'prior', 'nan', 'log_evidence', 'n_nan_windows', 'expected_jumps', 'expected_init',
                 'expected_dwell', 'expected_censored')

    def __repr__(self):
        return f"DwellLengthCounts(T={len(self.traj)}, log_evidence={self.log_evidence!r}, n_nan_windows={self.n_nan_windows})"

    def lifetime_pmf(self, state):
        """
        (T,) `expected_dwell[state]` over its sum: the exact posterior mean of the histogram of the completed lifetimes of
        `state`, column l - 1 for l frames.  NaN when the sum is 0 (no completed segment has positive weight).
        """
        row = self.expected_dwell[state]
        total = row.sum()
        return row / total if total > 0 else np.full(len(row), np.nan)


def exact_dwell_lengths(trajs, model, prior, nan='propagate', scratch_bytes=0):
    """
    The exact posterior expected segment-length counts of a `GenericGaussianModel` under a dwell-time prior: how many completed
    segments of each length every state has, and where the last, censored one stands (bild_gauss_dwell_lengths; DESIGN.md
    section 24).  They are the derivatives of `exact_dwell`'s evidence with respect to `prior.log_dwell` and
    `prior.log_surv`, and the E-step of `fit_dwell_prior`.  No draws, no histogram noise.

    trajs, model, prior, nan, scratch_bytes : as for `exact_dwell`; a list gives a list of results from ONE device call

    Every refusal is `exact_dwell`'s and is raised before the trajectories are uploaded.  Returns `DwellLengthCounts` or a list
    of them.
    """
    single, items = _check_exact_dwell(trajs, model, prior, nan)
    fields = lambda res, j, T: dict(n_nan_windows=int(res['n_nan_windows'][j]), expected_jumps=res['exp_jumps'][j].copy(),
                                    expected_init=res['exp_init'][j].copy(), expected_dwell=res['exp_dwell'][j, :, :T].copy(),
                                    expected_censored=res['exp_cens'][j, :, :T].copy())
    return _dwell_per_trajectory(_lib.gauss_dwell_lengths, DwellLengthCounts, single, items, model, prior, nan, fields,
                                 scratch_bytes=scratch_bytes)


# ---------------------------------------------------------------- switch counts and first-contact times (section 27)

class DwellSwitchCounts(_Record):
    """
    `exact_dwell_switch_counts` of one trajectory of T frames: the exact posterior of the number K of switches.

    traj, model, prior, nan : as given
    log_evidence, n_nan_windows : `exact_dwell`'s numbers, bit for bit
    log_count : (k_max + 1, S) log P(K = n, theta_{T-1} = s | data) at [n, s]; -inf where the probability is 0 and for n > T - 1
    log_tail : log P(K > k_max | data), computed as log(max(0, 1 - sum exp `log_count`)): a difference from 1, accurate to about
        1e-15 of the probability and no better; -inf exactly when k_max >= T - 1

    Under nan='propagate' a trajectory with `n_nan_windows` > 0 is NaN in all but `n_nan_windows`; a trajectory without a
    profile of positive weight has `log_evidence` -inf and NaN elsewhere.
    """

    __slots__ = ('traj', 'model', 'prior', 'nan', 'log_evidence', 'n_nan_windows', 'log_count', 'log_tail')

    def __repr__(self):
        return (f"DwellSwitchCounts(T={len(self.traj)}, k_max={len(self.log_count) - 1}, log_evidence={self.log_evidence!r}, "
                f"n_nan_windows={self.n_nan_windows})")

    def pmf(self):
        """ (k_max + 1,) P(K = n | data): the states summed in ascending order.  It sums to 1 - exp(`log_tail`). """
        return np.exp(self.log_count).sum(axis=1)

    def mean(self):
        """ sum_n n P(K = n | data): the posterior mean of K when k_max is complete (k_max >= T - 1), a lower bound otherwise """
        return float(np.arange(len(self.log_count)) @ self.pmf())

    def segment_count_pmf(self, state):
        """
        ((k_max + 2) // 2 + 1,) the probability that `state` has j segments, at [j], among the profiles of at most k_max switches (it
        sums to 1 - exp(`log_tail`)).  Two states only, where the states alternate: a profile of K switches that ends in q has
        ceil((K + 1) / 2) segments in q and floor((K + 1) / 2) in the other state.  With three states or more the number of
        segments of one state is not a function of K and the last state (it needs a recursion of its own inside every level):
        NotImplementedError, histogram `exact_dwell_draw`'s profiles instead.
        """
        S = self.log_count.shape[1]
        if S != 2:
            raise NotImplementedError(f"segment_count_pmf is derived for two states, where the states alternate; the model has {S}: "
                                      f"count the segments of the profiles of exact_dwell_draw instead")
        if state not in (0, 1):
            raise ValueError(f"state = {state!r}: 0 or 1")
        weight = np.exp(self.log_count)
        out = np.zeros((len(weight) + 1) // 2 + 1)
        for n in range(len(weight)):
            for q in range(2):
                out[(n + 2) // 2 if q == state else (n + 1) // 2] += weight[n, q]
        return out


def exact_dwell_switch_counts(trajs, model, prior, k_max=None, nan='propagate', scratch_bytes=0):
    """
    The exact posterior distribution of the number of switches of a `GenericGaussianModel` profile under a dwell-time prior,
    jointly with the last state: the forward recursion of `exact_dwell` resolved by the number of switches, one device
    launch per level (bild_gauss_dwell_switch_counts).  No draws, no histogram noise in the tail.

    trajs, model, prior, nan, scratch_bytes : as for `exact_dwell`; a list gives a list of results from ONE device call
    k_max : the levels 0 ... k_max are computed; None: T - 1 of the longest trajectory, the complete distribution.  At most that.

    Every refusal is `exact_dwell`'s, or a `k_max` that is negative or beyond the longest trajectory's T - 1, and is raised
    before the trajectories are uploaded.  Returns `DwellSwitchCounts` or a list of them.
    """
    single, items = _check_exact_dwell(trajs, model, prior, nan)
    top = max([len(t) for t in items] + [1]) - 1
    if k_max is None:
        k_max = top
    if isinstance(k_max, bool) or not isinstance(k_max, (int, np.integer)) or k_max < 0 or k_max > top:
        raise ValueError(f"k_max = {k_max!r}: an integer from 0 to {top}, the longest trajectory's T - 1, or None for that")
    fields = lambda res, j, T: dict(n_nan_windows=int(res['n_nan_windows'][j]), log_count=res['log_count'][j].copy(),
                                    log_tail=float(res['log_tail'][j]))
    return _dwell_per_trajectory(_lib.gauss_dwell_switch_counts, DwellSwitchCounts, single, items, model, prior, nan, fields, int(k_max),
                                 scratch_bytes=scratch_bytes)


class DwellFirstContact(_Record):
    """
    `exact_dwell_first_contact` of one trajectory of T frames: the exact posterior of the first frame in a target set of states.

    traj, model, prior, nan : as given
    target : the states of the set, a sorted tuple
    log_evidence, n_nan_windows : `exact_dwell`'s numbers, bit for bit
    log_first : (T,) log P(the first frame in the set is t | data); -inf where the probability is 0
    log_never : log P(no frame is in the set | data), the censoring term of a pooled first-passage analysis

    Each is normalised by `log_evidence`, not by their sum: that they add up to 1 holds to rounding.  Under nan='propagate' a
    trajectory with `n_nan_windows` > 0 is NaN in all but `n_nan_windows`; a trajectory without a profile of positive weight
    has `log_evidence` -inf and NaN elsewhere.
    """

    __slots__ = ('traj', 'model', 'prior', 'nan', 'target', 'log_evidence', 'n_nan_windows', 'log_first', 'log_never')

    def __repr__(self):
        return (f"DwellFirstContact(T={len(self.traj)}, target={self.target}, log_evidence={self.log_evidence!r}, "
                f"log_never={self.log_never!r})")

    def cdf(self):
        """ (T,) P(the set has been entered by frame t | data), the running sum of exp `log_first`; 1 - cdf()[-1] is the never share """
        return np.cumsum(np.exp(self.log_first))


def _target_states(target, S):
    """ `exact_dwell_first_contact`'s target as a sorted tuple of states: a non-empty proper subset of 0 ... S - 1 """
    try:
        states = list(target)
    except TypeError:       # one state
        states = [target]
    if any(isinstance(s, bool) or not isinstance(s, (int, np.integer)) for s in states):
        raise ValueError(f"target = {target!r}: a state or a collection of states")
    states = sorted(set(int(s) for s in states))
    if not states:
        raise ValueError("target is empty: no state to reach")
    if states[0] < 0 or states[-1] >= S:
        raise ValueError(f"target = {target!r}: the model's states are 0 ... {S - 1}")
    if len(states) == S:
        raise ValueError(f"target = {target!r} holds every state: the first frame is always in it")
    return tuple(states)


def exact_dwell_first_contact(trajs, model, prior, target, nan='propagate', scratch_bytes=0):
    """
    The exact posterior distribution of the first frame at which a `GenericGaussianModel` profile is in one of the states
    `target` under a dwell-time prior, and the probability that it never is: a forward pass over the profiles that avoid the
    set, combined with the backward tables of `exact_dwell` (bild_gauss_dwell_first_contact).  No
    draws, no histogram noise in the early frames.

    trajs, model, prior, nan, scratch_bytes : as for `exact_dwell`; a list gives a list of results from ONE device call
    target : a state or a collection of states, a non-empty proper subset of the model's (so a model of one state is refused)

    Every refusal is `exact_dwell`'s or the target's (ValueError) and is raised before the trajectories are uploaded.
    Returns `DwellFirstContact` or a list of them.
    """
    single, items = _check_exact_dwell(trajs, model, prior, nan)
    states = _target_states(target, model.msd.shape[0])
    fields = lambda res, j, T: dict(target=states, n_nan_windows=int(res['n_nan_windows'][j]), log_first=res['log_first'][j, :T].copy(),
                                    log_never=float(res['log_never'][j]))
    return _dwell_per_trajectory(_lib.gauss_dwell_first_contact, DwellFirstContact, single, items, model, prior, nan, fields,
                                 sum(1 << s for s in states), scratch_bytes=scratch_bytes)


# ---------------------------------------------------------------- looped time (section 28)

class DwellOccupancy(_Record):
    """
    `exact_dwell_occupancy` of one trajectory of T frames: the exact posterior of the number N of frames in a target set of
    states.  Every frame counts, observed or missing.

    traj, model, prior, nan : as given
    target : the states of the set, a sorted tuple
    log_evidence, n_nan_windows : `exact_dwell`'s numbers, bit for bit
    log_occupancy : (T + 1, S) log P(N = n, theta_{T-1} = s | data) at [n, s]; -inf where the probability is 0

    Normalised by `log_evidence`, not by its sum: that it adds up to 1 holds to rounding.  Under nan='propagate' a trajectory
    with `n_nan_windows` > 0 is NaN in all but `n_nan_windows`; a trajectory without a profile of positive weight has
    `log_evidence` -inf and NaN elsewhere.
    """

    __slots__ = ('traj', 'model', 'prior', 'nan', 'target', 'log_evidence', 'n_nan_windows', 'log_occupancy')

    def __repr__(self):
        return (f"DwellOccupancy(T={len(self.log_occupancy) - 1}, target={self.target}, log_evidence={self.log_evidence!r}, "
                f"n_nan_windows={self.n_nan_windows})")

    def pmf(self):
        """ (T + 1,) P(N = n | data): the last states summed in ascending order """
        return np.exp(self.log_occupancy).sum(axis=1)

    def cdf(self):
        """ (T + 1,) P(N <= n | data), the running sum of `pmf` """
        return np.cumsum(self.pmf())

    def mean(self):
        """ the posterior mean of N, in frames: the sum of `exact_dwell`'s marginals over the set """
        return float(np.arange(len(self.log_occupancy)) @ self.pmf())

    def var(self):
        """ the posterior variance of N, in frames squared, about `mean` """
        pmf, n = self.pmf(), np.arange(len(self.log_occupancy))
        return float((n - n @ pmf) ** 2 @ pmf)

    def interval(self, level=0.95):
        """
        the central interval (lo, hi) in frames: lo the smallest n whose cdf reaches (1 - level) / 2, hi the smallest whose cdf
        reaches 1 - (1 - level) / 2 (T where rounding keeps the cdf below it)
        """
        if not 0 < level < 1:
            raise ValueError(f"level = {level!r}: a probability strictly between 0 and 1")
        cdf = self.cdf()
        if np.any(np.isnan(cdf)):
            raise ValueError("the result is NaN: no interval")
        tail = (1 - level) / 2
        lo, hi = (min(int(np.searchsorted(cdf, q, side='left')), len(cdf) - 1) for q in (tail, 1 - tail))
        return lo, hi

    def fraction(self):
        """ (T + 1,) the grid n / T that `pmf` lives on: the looped fraction of the trajectory """
        T = len(self.log_occupancy) - 1
        return np.arange(T + 1) / max(T, 1)


def exact_dwell_occupancy(trajs, model, prior, target, nan='propagate', scratch_bytes=0):
    """
    The exact posterior distribution of the number of frames that a `GenericGaussianModel` profile spends in the states
    `target` under a dwell-time prior, jointly with the last state: the forward recursion of `exact_dwell` resolved by that
    number, one device launch per end frame (bild_gauss_dwell_occupancy).  No draws, no histogram noise
    in the tails that a credible interval is read from.

    trajs, model, prior, nan, scratch_bytes : as for `exact_dwell`; a list gives a list of results from ONE device call.  A
        trajectory of a chunk costs S T (T + 1) doubles of the longest T beside `exact_dwell`'s forward tables
    target : a state or a collection of states, a non-empty proper subset of the model's (so a model of one state is refused)

    Every refusal is `exact_dwell`'s or the target's (ValueError) and is raised before the trajectories are uploaded.
    Returns `DwellOccupancy` or a list of them.
    """
    single, items = _check_exact_dwell(trajs, model, prior, nan)
    states = _target_states(target, model.msd.shape[0])
    fields = lambda res, j, T: dict(target=states, n_nan_windows=int(res['n_nan_windows'][j]),
                                    log_occupancy=res['log_occ'][j, :T + 1].copy())
    return _dwell_per_trajectory(_lib.gauss_dwell_occupancy, DwellOccupancy, single, items, model, prior, nan, fields,
                                 sum(1 << s for s in states), scratch_bytes=scratch_bytes)


def pooled_occupancy(results):
    """
    (sum_j T_j + 1,) the pmf of the total number of frames in the target set over several trajectories' `DwellOccupancy`: given
    model and prior their posteriors are independent, so it is the convolution of their pmfs, in linear space and in the order
    of the list (host only).  Refused (ValueError): an empty list, differing targets, a result that is NaN.
    """
    results = list(results)
    if not results:
        raise ValueError("no result to pool")
    if any(r.target != results[0].target for r in results):
        raise ValueError(f"the results have differing targets: {sorted(set(r.target for r in results))}")
    total = np.ones(1)
    for j, r in enumerate(results):
        pmf = r.pmf()
        if np.any(np.isnan(pmf)):
            raise ValueError(f"result {j} is NaN (n_nan_windows = {r.n_nan_windows}, log_evidence = {r.log_evidence!r})")
        total = np.convolve(total, pmf)
    return total


# ---------------------------------------------------------------- visits to a set of states (section 30)

class DwellVisits(_Record):
    """
    `exact_dwell_visits` of one trajectory of T frames: the exact posterior of the number N of visits to a target set of states,
    a visit being a maximal run of consecutive frames in the set.  A run at frame 0 counts, a run cut off by the end of the
    trajectory counts, and a jump between two states of the set continues the visit: 0 <= N <= (T + 1) // 2.

    traj, model, prior, nan : as given
    target : the states of the set, a sorted tuple
    log_evidence, n_nan_windows : `exact_dwell`'s numbers, bit for bit
    log_visits : (n_max + 1, S) log P(N = n, theta_{T-1} = s | data) at [n, s], n_max at most (T + 1) // 2; -inf where the
        probability is 0
    log_tail : log P(N > n_max | data), computed as log(max(0, 1 - sum exp `log_visits`)): a difference from 1, accurate to about
        1e-15 of the probability and no better; -inf exactly when n_max >= (T + 1) // 2

    Normalised by `log_evidence`, not by its sum: that it adds up to 1 holds to rounding.  Under nan='propagate' a trajectory
    with `n_nan_windows` > 0 is NaN in all but `n_nan_windows`; a trajectory without a profile of positive weight has
    `log_evidence` -inf and NaN elsewhere.
    """

    __slots__ = ('traj', 'model', 'prior', 'nan', 'target', 'log_evidence', 'n_nan_windows', 'log_visits', 'log_tail')

    def __repr__(self):
        return (f"DwellVisits(T={len(self.traj)}, n_max={len(self.log_visits) - 1}, target={self.target}, "
                f"log_evidence={self.log_evidence!r}, n_nan_windows={self.n_nan_windows})")

    def pmf(self):
        """ (n_max + 1,) P(N = n | data): the last states summed in ascending order.  It sums to 1 - exp(`log_tail`). """
        return np.exp(self.log_visits).sum(axis=1)

    def cdf(self):
        """ (n_max + 1,) P(N <= n | data), the running sum of `pmf` """
        return np.cumsum(self.pmf())

    def mean(self):
        """ sum_n n P(N = n | data): the posterior mean of N when `log_tail` is -inf, a lower bound otherwise """
        return float(np.arange(len(self.log_visits)) @ self.pmf())

    def var(self):
        """ the posterior variance of N about `mean`, over the rows of the table (the whole of it when `log_tail` is -inf) """
        pmf, n = self.pmf(), np.arange(len(self.log_visits))
        return float((n - n @ pmf) ** 2 @ pmf)

    def interval(self, level=0.95):
        """
        the central interval (lo, hi) in visits: lo the smallest n whose cdf reaches (1 - level) / 2, hi the smallest whose cdf
        reaches 1 - (1 - level) / 2 (n_max where rounding keeps the cdf below it).  ValueError where `log_tail` leaves more
        than (1 - level) / 2 outside the table: hi is then beyond n_max.
        """
        if not 0 < level < 1:
            raise ValueError(f"level = {level!r}: a probability strictly between 0 and 1")
        cdf = self.cdf()
        if np.any(np.isnan(cdf)) or np.isnan(self.log_tail):
            raise ValueError("the result is NaN: no interval")
        tail = (1 - level) / 2
        if math.exp(self.log_tail) > tail:
            raise ValueError(f"P(N > n_max = {len(cdf) - 1}) = {math.exp(self.log_tail):.3g} exceeds (1 - level) / 2 = {tail:.3g}: "
                             f"the upper end lies beyond the table, raise n_max")
        lo, hi = (min(int(np.searchsorted(cdf, q, side='left')), len(cdf) - 1) for q in (tail, 1 - tail))
        return lo, hi


def exact_dwell_visits(trajs, model, prior, target, n_max=None, nan='propagate', scratch_bytes=0):
    """
    The exact posterior distribution of the number of visits of a `GenericGaussianModel` profile to the states `target` under a
    dwell-time prior, jointly with the last state: the number of contact episodes, maximal runs of consecutive frames in the
    set, for any number of states.  With one state as the target it is the number of that state's segments.  The forward
    recursion of `exact_dwell` resolved by the number of visits begun, one device launch per end frame
    (bild_gauss_dwell_visits).  No draws, no histogram noise in P(N = 0) and in the tail.

    trajs, model, prior, nan, scratch_bytes : as for `exact_dwell`; a list gives a list of results from ONE device call.  A
        trajectory of a chunk costs S T (n_max + 1) doubles of the longest T beside `exact_dwell`'s forward tables
    target : a state or a collection of states, a non-empty proper subset of the model's (so a model of one state is refused)
    n_max : the rows 0 ... n_max are computed; None: (T + 1) // 2 of the longest trajectory, the complete distribution.  Each
        result holds the rows up to its own (T + 1) // 2 at most.

    Every refusal is `exact_dwell`'s, the target's or a `n_max` that is no non-negative integer (ValueError) and is raised
    before the trajectories are uploaded.  Returns `DwellVisits` or a list of them.
    """
    single, items = _check_exact_dwell(trajs, model, prior, nan)
    states = _target_states(target, model.msd.shape[0])
    if n_max is None:
        n_max = (max([len(t) for t in items] + [0]) + 1) // 2
    if isinstance(n_max, bool) or not isinstance(n_max, (int, np.integer)) or n_max < 0:
        raise ValueError(f"n_max = {n_max!r}: a non-negative integer, or None for the complete distribution")
    fields = lambda res, j, T: dict(target=states, n_nan_windows=int(res['n_nan_windows'][j]),
                                    log_visits=res['log_visits'][j, :min(int(n_max), (T + 1) // 2) + 1].copy(),
                                    log_tail=float(res['log_tail'][j]))
    return _dwell_per_trajectory(_lib.gauss_dwell_visits, DwellVisits, single, items, model, prior, nan, fields,
                                 sum(1 << s for s in states), int(n_max), scratch_bytes=scratch_bytes)


def pooled_visits(results):
    """
    (sum_j n_max_j + 1,) the pmf of the total number of visits to the target set over several trajectories' `DwellVisits`:
    given model and prior their posteriors are independent, so it is the convolution of their pmfs, in linear space and in the
    order of the list (host only).  Refused (ValueError): an empty list, differing targets, a result that is NaN, a result
    whose `log_tail` is not -inf (its table is cut: the total would miss mass at every count).
    """
    results = list(results)
    if not results:
        raise ValueError("no result to pool")
    if any(r.target != results[0].target for r in results):
        raise ValueError(f"the results have differing targets: {sorted(set(r.target for r in results))}")
    total = np.ones(1)
    for j, r in enumerate(results):
        pmf = r.pmf()
        if np.any(np.isnan(pmf)) or np.isnan(r.log_tail):
            raise ValueError(f"result {j} is NaN (n_nan_windows = {r.n_nan_windows}, log_evidence = {r.log_evidence!r})")
        if r.log_tail != -np.inf:
            raise ValueError(f"result {j} is cut at n_max = {len(pmf) - 1} (log_tail = {r.log_tail!r}): pool complete distributions")
        total = np.convolve(total, pmf)
    return total


# ---------------------------------------------------------------- windows and called segments (section 29)

class DwellWindowSupport(_Record):
    """
    `exact_dwell_windows` of one trajectory of T frames: for each of its n windows the exact posterior probability that every
    frame of the window is in the window's set of states.

    traj, model, prior, nan : as given
    windows : (n, 2) int array, the windows [u, v); targets : their sets of states, a tuple of sorted tuples
    log_evidence, n_nan_windows : `exact_dwell`'s numbers, bit for bit
    log_all : (n,) log P(theta_t in the set for every u <= t < v | data); -inf where the probability is 0

    Normalised by `log_evidence`.  Under nan='propagate' a trajectory with `n_nan_windows` > 0 is NaN in all but
    `n_nan_windows`; a trajectory without a profile of positive weight has `log_evidence` -inf and NaN in `log_all`.
    """

    __slots__ = ('traj', 'model', 'prior', 'nan', 'windows', 'targets', 'log_evidence', 'n_nan_windows', 'log_all')

    def __repr__(self):
        return f"DwellWindowSupport(T={len(self.traj)}, windows={len(self.log_all)}, log_evidence={self.log_evidence!r})"

    def p_all(self):
        """ (n,) P(every frame of the window is in its set | data) """
        return np.exp(self.log_all)

    def p_not_all(self):
        """
        (n,) P(some frame of the window is outside its set | data) = -expm1(`log_all`).  Its absolute error is that of
        `log_all`, so its relative error grows as it nears 0: a window that the posterior supports at 1 - 1e-12 has few
        correct digits here.
        """
        return -np.expm1(self.log_all)


def _window_queries(windows, S, T, where):
    """ one trajectory's windows (u, v, target) -> ((n, 2) int array, tuple of sorted state tuples); ValueError on a bad one """
    try:
        rows = [tuple(w) for w in windows]
    except TypeError:
        raise ValueError(f"the windows{where}: a sequence of (u, v, target)") from None
    uv, targets = np.zeros((len(rows), 2), dtype=np.int64), []
    for i, w in enumerate(rows):
        if len(w) != 3:
            raise ValueError(f"window {i}{where} = {w!r}: (u, v, target) expected")
        u, v, target = w
        if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in (u, v)) or not 0 <= u < v <= T:
            raise ValueError(f"window {i}{where} = [{u!r}, {v!r}): integers with 0 <= u < v <= T = {T} expected")
        uv[i] = u, v
        targets.append(_target_states(target, S))
    return uv, tuple(targets)


def exact_dwell_windows(trajs, model, prior, windows, nan='propagate', scratch_bytes=0):
    """
    The exact posterior probability, under a dwell-time prior, that a `GenericGaussianModel` profile is in the states `target`
    at EVERY frame of a window [u, v), for any number of windows a trajectory: "is this called loop really there?".  The
    forward recursion of `exact_dwell` restricted to the target over the window, started from the unconstrained forward
    tables at its left edge and closed with the backward tables at its right edge; the windows of a call run in parallel on the
    GPU (bild_gauss_dwell_windows).  The per-frame marginals cannot give this number: they lose the
    correlation between frames.  The probability that SOME frame of the window is in a set is `p_not_all` of its complement.

    trajs, model, prior, nan, scratch_bytes : as for `exact_dwell`; a list gives a list of results from ONE device call
    windows : a sequence of (u, v, target), 0 <= u < v <= T, for one trajectory; for a list of trajectories a list of such
        sequences, one a trajectory (an empty one: that trajectory still gets its evidence).  A target is a state or a
        collection of states, a non-empty proper subset of the model's (so a model of one state has no valid window).

    Every refusal is `exact_dwell`'s, the target's, a window outside its trajectory or a list of the wrong length (ValueError)
    and is raised before the trajectories are uploaded.  Returns `DwellWindowSupport` or a list of them.
    """
    single, items = _check_exact_dwell(trajs, model, prior, nan)
    S = model.msd.shape[0]
    try:
        per_traj = [windows] if single else list(windows)
    except TypeError:
        raise ValueError("windows: a list of sequences of (u, v, target), one a trajectory") from None
    if len(per_traj) != len(items):
        raise ValueError(f"{len(per_traj)} sequences of windows for {len(items)} trajectories")
    parsed = [_window_queries(w, S, len(t), '' if single else f" of trajectory {j}") for j, (w, t) in enumerate(zip(per_traj, items))]
    counts = np.array([len(uv) for uv, _ in parsed], dtype=np.int64)
    first = np.concatenate(([0], np.cumsum(counts)))
    uv = np.concatenate([uv for uv, _ in parsed] + [np.zeros((0, 2), dtype=np.int64)])
    masks = np.array([sum(1 << s for s in g) for _, targets in parsed for g in targets], dtype=np.uint32)

    def fields(res, j, T):
        return dict(windows=parsed[j][0], targets=parsed[j][1], n_nan_windows=int(res['n_nan_windows'][j]),
                    log_all=res['log_all'][first[j]:first[j + 1]].copy())
    return _dwell_per_trajectory(_lib.gauss_dwell_windows, DwellWindowSupport, single, items, model, prior, nan, fields,
                                 np.repeat(np.arange(len(items)), counts), uv[:, 0], uv[:, 1], masks, scratch_bytes=scratch_bytes)


class DwellMapSupport(_Record):
    """
    `ExactDwellResults.map_support`: the exact posterior's support of the MAP profile of one trajectory of T frames, the
    confidence column of a called profile.

    traj, model, prior, nan : those of the results; log_evidence, n_nan_windows : `exact_dwell`'s numbers
    seg_start, seg_end, seg_state : (n_seg,) the called segments [start, end) and their states
    log_whole : (n_seg,) log P(every frame of the segment is in its state | data)
    log_absent : (n_seg,) log P(no frame of the segment is in its state | data)
    radii : as given; switch_frames : (n_seg - 1,) the called switch frames c (the first frame of the new state)
    p_switch_within : (n_seg - 1, len(radii)) P(at least one switch at the frames c - r ... c + r | data), the range clamped to
        the trajectory: 1 - sum_s P(the frames max(c - r - 1, 0) ... min(c + r, T - 1) are all in s)
    n_queries : the windows of the one device call
    """

    __slots__ = ('traj', 'model', 'prior', 'nan', 'radii', 'seg_start', 'seg_end', 'seg_state', 'log_whole', 'log_absent',
                 'switch_frames', 'p_switch_within', 'n_queries', 'log_evidence', 'n_nan_windows')

    def __repr__(self):
        return f"DwellMapSupport(T={len(self.traj)}, segments={len(self.seg_start)}, radii={self.radii}, n_queries={self.n_queries})"

    def p_whole(self):
        """ (n_seg,) P(every frame of the segment is in its state | data) """
        return np.exp(self.log_whole)

    def p_present(self):
        """ (n_seg,) P(some frame of the segment is in its state | data) = -expm1(`log_absent`) """
        return -np.expm1(self.log_absent)


def _hazard_edges(edges, n):
    """ `fit_dwell_prior`'s edges, checked; None: the powers of two below n (1 alone for n <= 2) """
    if edges is None:
        edges = [1]
        while 2 * edges[-1] < n:
            edges.append(2 * edges[-1])
    edges = np.asarray(edges)
    if edges.ndim != 1 or len(edges) < 1 or not np.issubdtype(edges.dtype, np.integer) or edges[0] != 1 or np.any(np.diff(edges) <= 0):
        raise ValueError(f"edges = {edges!r}: a strictly increasing integer array that starts at 1")
    return edges.astype(np.int64)


def _hazard_bins(edges, n):
    """ (n,) the bin of every length 1 ... n: bin j covers [edges[j], edges[j + 1]), the last one is open """
    return np.searchsorted(edges, np.arange(1, n + 1), side='right') - 1


def hazard_m_step(dwell, cens, jumps, first, edges, hazard, jump, init, allowed=None, min_risk=1e-6):
    """
    The exact M-step of a dwell-time prior with a piecewise-constant hazard, on expected counts summed over the data set
    (host only; `fit_dwell_prior` calls it once per iteration):

        h[s][bin] = sum_bin D / sum_bin (D + R),   R_l = sum_{m > l} (D_m + C_m)

    -- the Kaplan-Meier estimator on expected counts: D_l segments end at l, R_l are still running behind l --,
    jump[s] proportional to jumps[s] over the allowed s', init proportional to first.

    dwell, cens : (S, n) D and C, column l - 1 for length l;  jumps : (S, S);  first : (S,)
    edges : (n_bins,) the first length of every bin, strictly increasing from 1
    hazard (S, n_bins), jump (S, S), init (S,) : the current values, which an entry without mass keeps: a bin whose
        sum (D + R) is below `min_risk`, a row of jumps or a `first` that sums to 0
    allowed : (S, S) bool, the jumps that exist (None: every off-diagonal one)

    Returns (hazard, jump, init, supported): new arrays and the (S, n_bins) bool of the bins that had `min_risk` at risk.
    """
    dwell, cens = np.asarray(dwell, dtype=np.float64), np.asarray(cens, dtype=np.float64)
    hazard, jump, init = np.array(hazard, dtype=np.float64), np.array(jump, dtype=np.float64), np.array(init, dtype=np.float64)
    S, n = dwell.shape
    n_bins = len(edges)
    both = dwell + cens
    running = np.concatenate([np.cumsum(both[:, ::-1], axis=1)[:, ::-1][:, 1:], np.zeros((S, 1))], axis=1)      # R_l
    bins = _hazard_bins(edges, n)
    ended, risk = np.zeros((S, n_bins)), np.zeros((S, n_bins))
    for j in range(n_bins):
        ended[:, j] = dwell[:, bins == j].sum(axis=1)
        risk[:, j] = ended[:, j] + running[:, bins == j].sum(axis=1)
    supported = risk >= min_risk
    hazard[supported] = np.minimum(ended[supported] / risk[supported], 1.0)
    off = ~np.eye(S, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool) & ~np.eye(S, dtype=bool)
    jumps = np.where(off, np.asarray(jumps, dtype=np.float64), 0.0)
    mass = jumps.sum(axis=1)
    jump[mass > 0] = jumps[mass > 0] / mass[mass > 0, None]
    first = np.asarray(first, dtype=np.float64)
    if first.sum() > 0:
        init = first / first.sum()
    return hazard, jump, init, supported


class DwellPriorFit(_Record):
    """
    `fit_dwell_prior`'s result.

    edges : (n_bins,) the first length of every bin of the piecewise-constant hazard; the last bin is open
    hazard : (S, n_bins) P(a segment in s ends after l frames | it reached l), l in the bin
    jump : (S, S) the distribution of the state that follows s; init : (S,)
    log_evidence : the total log evidence of the data set at every iteration's parameters, one entry per device call; the last
        belongs to these parameters where the fit converged, and to the parameters one M-step before these where it did not
    n_iter, converged
    expected_dwell, expected_censored : (S, n) the data-set sums of the last E-step (`DwellLengthCounts`), n the longest trajectory
    supported : (S, n_bins) bool; False where the last E-step had less than `min_risk` segments at risk in the bin, which
        therefore kept its value: the data say nothing about it
    prior(n=None) : the `DwellPrior` with tables for n frames (None: the longest trajectory of the fit)

    No standard errors: the counts are posterior expectations, not observations, and the information of the marginal
    likelihood is not computed.
    """

    __slots__ = ('edges', 'hazard', 'jump', 'init', 'log_evidence', 'n_iter', 'converged', 'expected_dwell', 'expected_censored',
                 'supported')

    def __repr__(self):
        return f"DwellPriorFit(n_iter={self.n_iter}, converged={self.converged}, edges={self.edges.tolist()}, hazard={self.hazard!r})"

    def prior(self, n=None):
        n = self.expected_dwell.shape[1] if n is None else n
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"n = {n!r}: a positive integer")
        return DwellPrior.from_hazard(self.hazard[:, _hazard_bins(self.edges, int(n))], self.jump, self.init)


def _hazard_start(model, start, n_bins):
    """ `fit_dwell_prior`'s start -> (allowed (S, S), hazard (S, n_bins), jump (S, S), init (S,)), checked """
    S = model.msd.shape[0]
    allowed = np.asarray(model.transitions, dtype=bool).copy()
    if allowed.shape != (S, S):
        raise ValueError(f"model.transitions has shape {allowed.shape}; ({S}, {S}) expected")
    np.fill_diagonal(allowed, False)
    leaves = allowed.any(axis=1)
    even = np.where(allowed, 1.0 / np.maximum(allowed.sum(axis=1), 1)[:, None], 0.0)
    if start is None:
        hazard, jump, init = np.where(leaves[:, None], np.full((S, n_bins), 0.1), 0.0), even, np.full(S, 1.0 / S)
    elif isinstance(start, MarkovPriorFit):
        P = np.asarray(start.P, dtype=np.float64)
        if P.shape != (S, S):
            raise ValueError(f"start.P has shape {P.shape}; ({S}, {S}) expected")
        off = P - np.diag(np.diag(P))
        leave = off.sum(axis=1)
        hazard = np.repeat(leave[:, None], n_bins, axis=1)
        jump = np.where(leave[:, None] > 0, off / np.where(leave > 0, leave, 1.0)[:, None], 0.0)
        init = np.array(start.init, dtype=np.float64)
    elif isinstance(start, tuple) and len(start) == 3:
        hazard, jump, init = (np.array(a, dtype=np.float64) for a in start)
    else:
        raise ValueError("start must be None, a MarkovPriorFit or a (hazard_per_bin, jump, init) tuple")
    if hazard.shape != (S, n_bins):
        raise ValueError(f"the start's hazard has shape {hazard.shape}; ({S}, {n_bins}) expected")
    if jump.shape != (S, S) or init.shape != (S,):
        raise ValueError(f"the start's jump and init have shapes {jump.shape} and {init.shape}; ({S}, {S}) and ({S},) expected")
    if np.any((jump > 0) & ~allowed):
        raise ValueError("start has a positive jump that model.transitions forbids")
    return allowed, hazard, jump, init


def fit_dwell_prior(trajs, model, edges=None, start=None, tol=1e-8, max_iter=500, min_risk=1e-6, nan='propagate'):
    """
    Maximum-likelihood dwell-time distributions of a data set: EM over a whole `DwellPrior` in the discrete-hazard
    parametrisation (`DwellPrior.from_hazard`), the model held fixed.  The hazard of every state is piecewise constant on bins
    of lengths; the E-step is one `exact_dwell_lengths` device call on a trajectory set that is built once, the M-step is exact
    and in closed form (`hazard_m_step`: Kaplan-Meier on the expected counts).  `fit_markov_prior` is the case of one bin.

    trajs : a list of trajectories (or one)
    model : a `GenericGaussianModel` (anything else: TypeError); transitions that `model.transitions` forbids stay 0
    edges : the first length of every bin, a strictly increasing integer array that starts at 1.  Bin j covers the lengths
        [edges[j], edges[j + 1]), the last bin is open up to the longest trajectory n; the states share the bins.  None: the
        doubling edges 1, 2, 4, ... below n.  [1]: the Markov family.
    start : None -- hazard 0.1 everywhere, jumps spread evenly over the allowed transitions, uniform init; a `MarkovPriorFit`;
        or a (hazard per bin (S, n_bins), jump (S, S), init (S,)) tuple
    tol : stop when an M-step moves no bin hazard, jump entry or init entry by more than this
    max_iter : at most this many device calls
    min_risk : a bin with fewer expected segments at risk than this keeps its value (see `DwellPriorFit.supported`), and so
        does a jump row without mass: a partial M-step, so the total log evidence never decreases
    nan : as for `exact_dwell`; a total evidence that is not finite raises `EvidenceNotFinite`

    A fit that converges returns the parameters of its last E-step, which the M-step would have moved by no more than `tol`:
    `log_evidence[-1]`, `expected_dwell` and `expected_censored` are then those of `prior()`.  A fit that stops at `max_iter`
    returns the last M-step's parameters, one step ahead of `log_evidence[-1]`, as `fit_markov_prior` does.

    EM on a hidden semi-Markov model may stop at a local optimum.  No standard errors are reported: the expected counts are
    not observations, and the information of the marginal likelihood is not computed.  Returns `DwellPriorFit`.
    """
    _fit_model('fit_dwell_prior', model)
    single, items, n = _fit_trajs('fit_dwell_prior', trajs)
    edges = _hazard_edges(edges, n)
    allowed, hazard, jump, init = _hazard_start(model, start, len(edges))
    if not (tol > 0) or isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1 or not (min_risk > 0):
        raise ValueError(f"tol = {tol!r} and min_risk = {min_risk!r} must be positive and max_iter = {max_iter!r} a positive integer")
    bins = _hazard_bins(edges, n)
    _check_exact_dwell(items, model, DwellPrior.from_hazard(hazard[:, bins], jump, init), nan)

    ts = model.trajset(items[0] if single else items)       # built once: the iterations change the prior, not the tables
    history, converged = [], False
    for _ in range(int(max_iter)):
        prior = DwellPrior.from_hazard(hazard[:, bins], jump, init)
        res = _lib.gauss_dwell_lengths(model.handle(), ts, *prior.tables(), omit=nan == 'omit')
        total = float(np.sum(res['logev']))
        if not np.isfinite(total):
            raise EvidenceNotFinite(total)
        history.append(total)
        dwell, cens = res['exp_dwell'].sum(axis=0), res['exp_cens'].sum(axis=0)
        new_hazard, new_jump, new_init, supported = hazard_m_step(dwell, cens, res['exp_jumps'].sum(axis=0), res['exp_init'].sum(axis=0),
                                                                  edges, hazard, jump, init, allowed=allowed, min_risk=min_risk)
        step = max(float(np.max(np.abs(new_hazard - hazard))), float(np.max(np.abs(new_jump - jump))), float(np.max(np.abs(new_init - init))))
        if step <= tol:     # (the step is not taken: the evidence and the counts stay those of the parameters returned)
            converged = True
            break
        hazard, jump, init = new_hazard, new_jump, new_init
    return DwellPriorFit(edges=edges, hazard=hazard, jump=jump, init=init, log_evidence=np.array(history), n_iter=len(history),
                         converged=converged, expected_dwell=dwell, expected_censored=cens, supported=supported)
