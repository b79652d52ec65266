"""
`GenericGaussianModel`: the reference's model-agnostic Gaussian model (bild/models.py:536-728), with its likelihood
evaluated on the GPU from per-trajectory interval tables (include/bild_amd.h, "GenericGaussianModel").

Every pure state is a Gaussian process given by its MSD, its mean and its steady-state order, per dimension; a profile's
likelihood is the product over its intervals of the Gaussian densities of the interval's frames, conditioned on the last
frame before the interval (ss_order 0) or built from the increments (ss_order 1).  The covariance rule that turns an MSD
into a covariance (the reference's ``bayesmsd.gp.msd2C_fun``) is `covariance` below.
"""
from collections import OrderedDict

import numpy as np

from . import _lib
from .models import (KalmanResult, MultiStateModel, MultiStateRouse, _REPLAY_GROUP_BYTES, _draw_normals, _fisher_scoring,
                     _fit_profiles, _log_chain_rule, _missing_frames, _missing_is_none, _ragged_segments)
from .profiles import segments_from_states
from .trajectory import Trajectory

MAX_T = 2048    # longest trajectory the GPU tables accept (gauss.h: kGaussMaxT)


def covariance(msd, msd_inf, ti, ss_order):
    """
    Covariance of a process observed at the integer times ``ti`` (ascending), from its MSD at integer lags (``msd[lag]``):

    * ss_order 0, the positions:  ``C_ij = (msd_inf - msd(|ti_i - ti_j|)) / 2``;
    * ss_order 1, the increments between consecutive times:
      ``K_ij = (msd(ti_{i+1} - ti_j) + msd(ti_i - ti_{j+1}) - msd(ti_{i+1} - ti_{j+1}) - msd(ti_i - ti_j)) / 2``, lags taken
      in absolute value.

    This is the rule of ``bayesmsd.gp.msd2C_fun`` as its documentation defines it.
    """
    msd = np.asarray(msd, dtype=np.float64)
    ti = np.asarray(ti, dtype=np.int64)
    if ss_order == 0:
        return 0.5 * (msd_inf - msd[np.abs(ti[:, None] - ti[None, :])])
    if ss_order == 1:
        a, b = ti[:-1], ti[1:]
        lag = lambda x, y: msd[np.abs(x[:, None] - y[None, :])]
        return 0.5 * (lag(b, a) + lag(a, b) - lag(b, b) - lag(a, a))
    raise ValueError(f"ss_order should be in {{0, 1}}; was {ss_order}")


def _tabulate(fun, ss_order, n_lags):
    """ a callable MSD at the lags 0 .. n_lags - 1 and (ss_order 0) at infinity """
    lags = np.arange(n_lags, dtype=np.float64)
    with np.errstate(all='ignore'):
        try:
            vals = np.asarray(fun(lags), dtype=np.float64)
        except Exception:
            vals = None
        if vals is None or vals.shape != lags.shape:
            vals = np.array([float(fun(t)) for t in lags])
        inf = float(fun(np.inf)) if ss_order == 0 else 0.0
    return vals, inf


class GenericGaussianModel(MultiStateModel):
    """
    Pure states are Gaussian processes; correlations between them are minimal (reference bild/models.py:536-728).

    The model needs no physics: only the MSD of each pure state, for example from control experiments.  Within an
    interval the trajectory follows its state's process; across a switch only continuity is kept: an ss_order-0 state
    conditions on the last valid point before the interval, an ss_order-1 state starts its increments there.

    Parameters
    ----------
    state_spec : (nStates, d, 3) nested sequence of ``(msd, m, ss_order)``
        ``msd`` is a callable MSD function (evaluated once, on an array of the lags 0 .. 2047 and, for ss_order 0, at
        ``np.inf``) or an array of its values: the lags 0, 1, ... and, for ss_order 0, msd(inf) as the last entry.  ``m``
        is the mean (of the positions for ss_order 0, of the increments for ss_order 1), ``ss_order`` is 0 or 1.

    Notes
    -----
    * The likelihood runs on the GPU: a trajectory set builds one table of every window's term per state (see
      include/bild_amd.h), after which an evaluation is k + 1 lookups.  Trajectories are limited to 2048 frames, and to
      the lags the MSD arrays cover.
    * Where the reference conditions a later ss_order-0 interval on a window without any valid frame it raises
      IndexError; here that candidate's logL is NaN, so that a batch does not fail as a whole.
    * The reference's ``MSD_function_powerlaw`` and ``MSD_function_twoLocusRouse`` helpers are not provided: they build
      on ``bayesmsd.deco.imaging``, which is not available to this package.  Any callable or array of MSD values works.
    * ``initial_loopingprofile`` raises NotImplementedError, as in the reference.
    """

    def __init__(self, state_spec):
        spec = [[tuple(entry) for entry in state] for state in state_spec]
        if len(spec) == 0 or any(len(state) != len(spec[0]) for state in spec) or len(spec[0]) == 0 \
                or any(len(entry) != 3 for state in spec for entry in state):
            raise ValueError("state_spec must have shape (nStates, d, 3): (msd, m, ss_order) per state and dimension")
        S, d = len(spec), len(spec[0])
        order = np.zeros((S, d), dtype=np.int32)
        mean = np.zeros((S, d))
        tables, infs = [], np.zeros((S, d))
        for n in range(S):
            row = []
            for k in range(d):
                msd, m, o = spec[n][k]
                if o not in (0, 1):
                    raise ValueError(f"ss_order should be in {{0, 1}}; was {o} (state {n}, dimension {k})")
                order[n, k] = int(o)
                mean[n, k] = float(m)
                if not np.isfinite(mean[n, k]):
                    raise ValueError(f"the mean of state {n}, dimension {k} is not finite")
                if callable(msd):
                    vals, inf = _tabulate(msd, o, MAX_T)
                else:
                    a = np.asarray(msd, dtype=np.float64)
                    if a.ndim != 1 or len(a) < (2 if o == 0 else 1):
                        raise ValueError(f"the MSD array of state {n}, dimension {k} must be 1-d: the lags 0, 1, ..."
                                         + (" and msd(inf) last" if o == 0 else ""))
                    vals, inf = (a[:-1], float(a[-1])) if o == 0 else (a, 0.0)
                if not np.all(np.isfinite(vals)) or not np.isfinite(inf):
                    raise ValueError(f"the MSD of state {n}, dimension {k} is not finite at every lag" +
                                     (" and at infinity" if o == 0 else ""))
                row.append(vals)
                infs[n, k] = inf
            tables.append(row)
        n_lags = min(len(v) for row in tables for v in row)
        self.state_spec = spec
        self.msd = np.array([[v[:n_lags] for v in row] for row in tables])     # (S, d, n_lags)
        self.msd_inf = infs
        self.mean = mean
        self.ss_order = order
        self.init_transitions(S)
        self._handle = None
        self._trajsets = OrderedDict()

    # ------------------------------------------------------------------ interface
    @property
    def d(self):
        return self.msd.shape[1]

    @property
    def max_T(self):
        """ the longest trajectory the model can evaluate: its MSD lags, at most 2048 frames """
        return min(MAX_T, self.msd.shape[2])

    def initial_loopingprofile(self, traj):
        raise NotImplementedError

    def __getstate__(self):
        state = dict(self.__dict__)
        state['_handle'] = None
        state['_trajsets'] = OrderedDict()
        return state

    def invalidate(self):
        """ call after changing the MSD tables, means or orders in place """
        self._handle = None
        self._trajsets.clear()

    def handle(self):
        if self._handle is None:
            self._handle = _lib.GaussModelHandle(self.ss_order, self.mean, self.msd, self.msd_inf)
        return self._handle

    def _get_noise(self, traj):
        return np.zeros(0)      # no localization error: it is part of the MSDs

    _fingerprints = MultiStateRouse._fingerprints

    def trajset(self, trajs):
        """
        Device-resident trajectories with their interval tables, built at the first use of a trajectory (or list of
        them) and cached like `MultiStateRouse.trajset`: keyed by the identity of the trajectory objects and guarded by
        their address, shape and content.  Raises before any device work for trajectories beyond `max_T` frames.
        """
        single = not isinstance(trajs, (list, tuple))
        items = (trajs,) if single else tuple(trajs)
        prints, arrs = self._fingerprints(items)
        for a in arrs:
            if a.ndim != 2 or a.shape[1] != self.d:
                raise ValueError(f"trajectory shape {a.shape} does not match the model's d = {self.d}")
            if len(a) > self.max_T:
                raise ValueError(f"trajectory of {len(a)} frames: GenericGaussianModel evaluates at most {self.max_T} "
                                 f"(the GPU tables take up to {MAX_T} frames, the MSD tables cover {self.msd.shape[2]} lags)")
        key = tuple(id(t) if p[0] is not None else p for t, p in zip(items, prints))
        hit = self._trajsets.get(key)
        if hit is not None:
            ts, kept, old_prints = hit
            if all(a is b or p[0] is None for a, b, p in zip(kept, items, prints)) and old_prints == prints:
                self._trajsets.move_to_end(key)
                return ts
        ts = _lib.GaussTrajSetHandle(self.handle(), arrs)
        self._trajsets[key] = (ts, items, prints)
        while len(self._trajsets) > 8:
            self._trajsets.popitem(last=False)
        return ts

    # ------------------------------------------------------------------ likelihood
    def logL(self, profile, traj):
        """ log p(traj | profile, model) (reference bild/models.py:608-663) """
        states = np.asarray(profile[:])
        assert len(states) == len(traj)
        return float(self.logL_batch(states[None, :], traj)[0])

    def logL_batch(self, profiles, traj):
        """ many expanded profiles on one trajectory: (n, T) int array or list of Loopingprofile -> (n,) """
        if not isinstance(profiles, np.ndarray):
            profiles = np.stack([np.asarray(p[:]) for p in profiles])
        seg_start, seg_state = segments_from_states(profiles)
        return _lib.gauss_logl_segments(self.handle(), self.trajset(traj), seg_start, seg_state)

    def logL_st_batch(self, ss, thetas, traj):
        """ one AMIS batch in the sampler's (s, theta) parametrisation (reference FixedkSampler.logL) """
        return _lib.gauss_logl_st(self.handle(), self.trajset(traj), ss, thetas)

    def logL_st(self, s, theta, traj):
        return float(self.logL_st_batch(np.asarray(s)[None, :], np.asarray(theta)[None, :], traj)[0])

    def logL_segments(self, seg_start, seg_state, trajs, traj_id=None):
        """ general batch: run-length encoded profiles over a set of trajectories """
        return _lib.gauss_logl_segments(self.handle(), self.trajset(trajs), seg_start, seg_state, traj_id)

    # ------------------------------------------------------------------ parameter sensitivities and fit
    _kalman_args = MultiStateRouse._kalman_args

    def logL_sensitivities(self, profiles, trajs, dmsd=None, dmsd_inf=None, dmean=None, traj_id=None, fisher=True,
                           scratch_bytes=0):
        """
        Log-likelihood of candidate profiles with its gradient and Fisher information with respect to P <= 4 parameters
        (bild_gauss_logl_sensitivities: forward tangents of every window's Cholesky factor).

        profiles, trajs, traj_id : as for `MultiStateRouse.logL_sensitivities`: expanded profiles of one trajectory, or
            ``(seg_start, seg_state)`` over a list of trajectories with ``traj_id``
        dmsd : (P, S, d, n_lags) derivatives of the MSD tables (n_lags = ``self.msd.shape[2]``), dmsd_inf and dmean :
            (P, S, d) those of msd(inf) and of the means; None = zero.  The arrays given must agree on P.
        fisher : return the Fisher information (innovations form: sum over the counted entries of every window of
            dS_p dS_q / (2 S^2) + de_p de_q / S); its computation costs nothing extra, and logL does not depend on it
        scratch_bytes : budget of the per-window factorisations of windows with a missing frame (0: the library's rule)

        Returns (logL (n,), grad (n, P), fisher (n, P, P) or None); NaN rows where `logL_segments` gives NaN.
        """
        items, seg_start, seg_state, tid = self._kalman_args(profiles, trajs, traj_id)
        P, given = self._derivative_arrays(dmsd, dmsd_inf, dmean)
        arrs = self._direct_arrays(items)
        return _lib.gauss_logl_sensitivities(self.handle(), arrs, seg_start, seg_state, tid, P=P, fisher=fisher,
                                             scratch_bytes=scratch_bytes, **given)

    def _derivative_arrays(self, dmsd, dmsd_inf, dmean):
        """ the derivative arrays of a sensitivities call, checked on the host: -> (P, dict of the arrays given) """
        S, d, n_lags = self.msd.shape
        given = {}
        for name, a, tail in (('dmsd', dmsd, (S, d, n_lags)), ('dmsd_inf', dmsd_inf, (S, d)), ('dmean', dmean, (S, d))):
            if a is None:
                continue
            a = np.asarray(a, dtype=np.float64)
            if a.ndim != len(tail) + 1 or a.shape[1:] != tail:
                raise ValueError(f"{name} has shape {a.shape}, expected (P,) + {tail}")
            given[name] = a
        lens = {len(a) for a in given.values()}
        if len(lens) > 1:
            raise ValueError(f"derivative arrays disagree on the number of parameters: {sorted(lens)}")
        P = lens.pop() if lens else 0
        if P > 4:
            raise _lib.BildAmdError(_lib.ERR_UNSUPPORTED, f"at most 4 parameters per call; {P} given")
        for name, a in given.items():
            if not np.all(np.isfinite(a)):
                raise ValueError(f"{name} is not finite everywhere")
        if 'dmsd' in given:     # the library's tables end at lag Tmax = n_lags - 1, as the model handle's do
            given['dmsd'] = given['dmsd'][..., :n_lags]
        return P, given

    def _direct_arrays(self, items):
        """ the (T, d) arrays of trajectories that a call takes directly (no trajectory set), checked on the host """
        _, arrs = self._fingerprints(items)
        for a in arrs:
            if a.ndim != 2 or a.shape[1] != self.d:
                raise ValueError(f"trajectory shape {a.shape} does not match the model's d = {self.d}")
            if len(a) > self.max_T:
                raise ValueError(f"trajectory of {len(a)} frames: GenericGaussianModel evaluates at most {self.max_T} "
                                 f"(the GPU takes up to {MAX_T} frames, the MSD tables cover {self.msd.shape[2]} lags)")
        return arrs

    # ------------------------------------------------------------------ per-frame moments
    def kalman(self, profiles, trajs, traj_id=None, outputs=('smooth',), scratch_bytes=0):
        """
        Per-frame moments of candidate profiles (bild_gauss_kalman_segments), from the Cholesky
        factor of every window of the likelihood.  Each frame is taken from the window of the interval that contains it.

        profiles, trajs, traj_id : as for `MultiStateRouse.kalman`
        outputs : subset of 'terms', 'pred', 'smooth', 'innov' ('filt' is not offered: the model has no filter)
        scratch_bytes : budget of the window factorisations and of one chunk of outputs (0: the library's rule)

        Returns a `KalmanResult` with arrays (n, T_max, d), NaN behind a trajectory's own length:

        * ``terms``: the log-likelihood term of each entry the likelihood counts, at its frame (the frame of the value,
          ss_order 0, or the end of the increment, ss_order 1), 0.0 elsewhere; summed, `logL_segments` to rounding;
        * ``pred_mean``, ``pred_var``: the observed coordinate given the earlier entries of its window, at counted frames;
        * ``innov``: the standardised innovation there (NaN elsewhere, as ``pred_*``);
        * ``smooth_mean``, ``smooth_var``: the coordinate given every valid frame of its window -- the data and 0 at a
          valid frame, the Gaussian conditional at a missing one (NaN for an ss_order-1 frame before the window's first
          valid frame).  The MSDs contain the localization noise and the model does not split it off, so these are
          moments of the *observed* coordinate, not of a noise-free one as `MultiStateRouse.kalman` gives.

        A candidate that `logL_segments` gives NaN (a later ss_order-0 interval without a valid frame) is NaN over that
        interval and dimension.  Argument errors are raised before any device work.
        """
        outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
        for o in outputs:
            if o == 'filt':
                raise ValueError("GenericGaussianModel has no filtered moments ('filt'); choose from 'terms', 'pred', "
                                 "'smooth', 'innov'")
            if o not in KalmanResult.GROUPS:
                raise ValueError(f"unknown output {o!r}; choose from {sorted(KalmanResult.GROUPS)}")
        items, seg_start, seg_state, tid = self._kalman_args(profiles, trajs, traj_id)
        arrs = self._direct_arrays(items)
        names = [name for o in outputs for name in KalmanResult.GROUPS[o]]
        res = _lib.gauss_kalman_segments(self.handle(), arrs, seg_start, seg_state, tid, outputs=names,
                                         scratch_bytes=scratch_bytes)
        return KalmanResult(res)

    def kalman_mixture(self, profiles, trajs, log_weights, traj_id=None, scratch_bytes=0):
        """
        Posterior mixture of the smoothed coordinate over weighted candidates (bild_gauss_kalman_mixture): per trajectory
        of ``trajs``, the candidates on it weighted by exp(log_weights), normalised within the trajectory (law of total
        variance).  Arguments as for `kalman`.  -> (mean, var), each (n_traj, T_max, d); NaN for a trajectory without
        candidates of finite weight.  At a valid frame the mean is the data and the variance 0.
        """
        items, seg_start, seg_state, tid = self._kalman_args(profiles, trajs, traj_id)
        log_weights = np.asarray(log_weights, dtype=np.float64).reshape(-1)
        if log_weights.shape != (len(seg_start),):
            raise ValueError(f"{len(log_weights)} log-weights for {len(seg_start)} candidates")
        if np.any(np.isnan(log_weights)) or np.any(log_weights == np.inf):
            raise ValueError("log-weights must be finite or -inf (NaN or +inf given)")
        arrs = self._direct_arrays(items)
        return _lib.gauss_kalman_mixture(self.handle(), arrs, seg_start, seg_state, log_weights, tid,
                                         scratch_bytes=scratch_bytes)

    def _tables(self):
        """ the tabulated arrays a fit differentiates: msd (S, d, n_lags), msd_inf and mean (S, d) """
        return self.msd, self.msd_inf, self.mean

    @classmethod
    def fit(cls, trajs, profiles, family, start, derivatives=None, tol=1e-8, max_iter=50):
        """
        Maximum-likelihood fit of positive parameters theta on trajectories whose looping profiles are known, by Fisher
        scoring in log theta with Levenberg damping (the stopping rule of `MultiStateRouse.fit`).

        trajs : list of trajectories
        profiles : one per trajectory (a `Loopingprofile`, a 1-d integer array, or ``(seg_start, seg_state)`` of shape
            (n_traj, K1) for all of them), or a single state index: a constant profile
        family : ``family(**theta)`` returns a ``state_spec``; every spec of the family must give MSD tables of one length
        start : dict of starting values (at most 4 parameters, positive and finite)
        derivatives : optional ``derivatives(**theta)`` -> (dmsd, dmsd_inf, dmean) with respect to theta, shaped as
            `logL_sensitivities` takes them (None entries = zero).  Without it, central differences in log theta of the
            tabulated msd, msd(inf) and means of the family's models (step 1e-5); the device part stays exact.
        tol, max_iter : the fit stops when the Newton decrement g^T F^-1 g / 2 falls below ``tol``, or after ``max_iter``
            device calls

        Returns a `FitResult`: the fitted model, params, standard errors (inverse Fisher information at the optimum, by
        the delta method from log theta), their covariance, logL, n_iter (device calls), converged and the history.
        """
        start = dict(start)
        params = tuple(start)
        if not params:
            raise ValueError("nothing to fit: start is empty")
        if len(params) > 4:
            raise ValueError("at most 4 parameters")
        theta = np.array([float(start[p]) for p in params])
        if np.any(~np.isfinite(theta)) or np.any(theta <= 0):
            raise ValueError(f"parameters must be positive and finite: {start}")
        if tol <= 0 or max_iter < 1:
            raise ValueError("need tol > 0 and max_iter >= 1")
        items = list(trajs) if isinstance(trajs, (list, tuple)) else [trajs]
        if not items:
            raise ValueError("need at least one trajectory")
        probe = cls(family(**dict(zip(params, theta))))
        seg = _fit_profiles(profiles, [len(t) for t in items], probe.nStates)
        tid = np.arange(len(items), dtype=np.int32)

        def evaluate(th):
            kw = dict(zip(params, th))
            model = cls(family(**kw))
            if derivatives is not None:
                dmsd, dmsd_inf, dmean = derivatives(**kw)
            else:
                dmsd, dmsd_inf, dmean = _log_differences(cls, family, params, th)
            logl, g, F = model.logL_sensitivities(seg, items, dmsd=dmsd, dmsd_inf=dmsd_inf, dmean=dmean, traj_id=tid)
            g, F = _log_chain_rule(g, F, np.broadcast_to(th, g.shape))
            return model, float(logl.sum()), g.sum(axis=0), F.sum(axis=0)

        return _fisher_scoring(evaluate, theta, params, tol, max_iter)

    @classmethod
    def fit_marginal(cls, trajs, family, start, derivatives=None, k_max=20, k_prior=None, nan='propagate', tol=1e-8, max_iter=50):
        """
        Maximum-likelihood fit of positive parameters theta on trajectories whose looping profiles are NOT known: the
        objective is the sum over the trajectories of the exact log marginal likelihood log sum_k pi_k p(traj | theta, k)
        (`bild_amd.exact_sensitivities`), every profile of up to ``k_max`` switches summed over.

        trajs, family, start, derivatives, tol, max_iter : as for `fit`
        k_max, k_prior, nan : as for `bild_amd.exact_sensitivities`

        Each evaluation builds the model of the trial theta, its trajectory set, and makes one `exact_sensitivities` call.
        The steps are Fisher scoring in log theta with the posterior mean of the complete-data information as the
        matrix (`fit`'s stopping rule and damping); that matrix overstates the information of the marginal likelihood,
        so the standard errors come from the observed information instead: central differences in log theta (step 1e-4)
        of the exact gradient at the optimum, symmetrised -- 2 P further evaluations, counted in ``n_iter``.  ``cov`` and
        ``se`` follow from its pseudo-inverse by the delta method; ``logL`` holds the total log marginal.
        """
        from .exact import exact_sensitivities, _check_exact_sample, _log_k_prior
        start = dict(start)
        params = tuple(start)
        if not params:
            raise ValueError("nothing to fit: start is empty")
        if len(params) > 4:
            raise ValueError("at most 4 parameters")
        theta = np.array([float(start[p]) for p in params])
        if np.any(~np.isfinite(theta)) or np.any(theta <= 0):
            raise ValueError(f"parameters must be positive and finite: {start}")
        if tol <= 0 or max_iter < 1:
            raise ValueError("need tol > 0 and max_iter >= 1")
        items = list(trajs) if isinstance(trajs, (list, tuple)) else [trajs]
        if not items:
            raise ValueError("need at least one trajectory")
        probe = cls(family(**dict(zip(params, theta))))
        _check_exact_sample(items, probe, k_max, nan)
        _log_k_prior(k_prior, len(items), int(k_max) + 1)

        def evaluate(th):
            kw = dict(zip(params, th))
            model = cls(family(**kw))
            if derivatives is not None:
                dmsd, dmsd_inf, dmean = derivatives(**kw)
            else:
                dmsd, dmsd_inf, dmean = _log_differences(cls, family, params, th)
            r = exact_sensitivities(items, model, dmsd=dmsd, dmsd_inf=dmsd_inf, dmean=dmean, k_max=k_max, k_prior=k_prior, nan=nan)
            g, F = _log_chain_rule(r.grad, r.fisher, np.broadcast_to(th, r.grad.shape))
            return model, float(r.log_marginal.sum()), g.sum(axis=0), F.sum(axis=0)

        first = evaluate(theta)
        if np.isnan(first[1]):
            hint = " (a trajectory has a NaN evidence: a later ss_order-0 segment without a valid frame; try nan='omit')" \
                if nan == 'propagate' else ""
            raise ValueError(f"the log marginal likelihood is NaN at the start{hint}")
        calls = [first]

        def cached(th):     # the start is evaluated once
            return calls.pop() if calls else evaluate(th)

        res = _fisher_scoring(cached, theta, params, tol, max_iter)
        th = np.array([res.params[p] for p in params])
        P, h = len(params), _MARGINAL_INFO_STEP
        H = np.zeros((P, P))
        for p in range(P):
            e = np.zeros(P)
            e[p] = h
            H[:, p] = -(evaluate(th * np.exp(e))[2] - evaluate(th * np.exp(-e))[2]) / (2 * h)
        H = 0.5 * (H + H.T)
        cov = np.linalg.pinv(H) * np.outer(th, th)
        res.cov = cov
        res.se = dict(zip(params, np.sqrt(np.maximum(np.diag(cov), 0.))))
        res.n_iter += 2 * P
        return res

    @classmethod
    def fit_dwell(cls, trajs, family, start, prior=None, markov_start=None, derivatives=None, nan='propagate', tol=1e-8, max_iter=50,
                  prior_tol=1e-10, prior_max_iter=200):
        """
        Maximum-likelihood fit of positive parameters theta on trajectories whose looping profiles are NOT known, under a
        dwell-time prior on the profiles: `fit_marginal`'s contract with `bild_amd.exact_dwell`'s evidence (one per
        trajectory, no k and no k_max) in place of the k-uniform marginal.  The gradient is exact
        (`bild_amd.exact_dwell_sensitivities`).

        trajs, family, start, derivatives, tol, max_iter : as for `fit`
        prior : a `DwellPrior` -- held fixed: an evaluation is the model of the trial theta, its trajectory set and one
            `exact_dwell_sensitivities` call.  None -- a Markov prior is fitted along with the model by the profile
            likelihood: an evaluation builds the model and its trajectory set, runs `bild_amd.fit_markov_prior` on that set
            (one build per evaluation: the inner EM and the gradient call share the cached set), warm-started from the
            (P, init) of the last accepted evaluation, and makes one `exact_dwell_sensitivities` call at the fitted prior.
            The objective is the total log evidence at (theta, P^(theta)), the full maximum-likelihood fit of the hidden
            semi-Markov model on exact evidence.
        markov_start : ``prior=None`` only: the start of the first inner fit, as `fit_markov_prior` takes it (None, P or
            (P, init))
        nan : as for `exact_dwell`
        prior_tol, prior_max_iter : ``tol`` and ``max_iter`` of the inner `fit_markov_prior`

        With ``prior=None`` the theta-gradient of the profile likelihood is taken as the partial gradient at P^(theta), by the
        envelope theorem.  That rests on the inner EM having converged: at an EM fixed point the derivative of the evidence
        with respect to P vanishes, short of it a term of the size of the last EM step times dP^/dtheta is left out.  This is
        why ``prior_tol`` is deliberately tighter than ``tol``.

        The steps are Fisher scoring in log theta with the posterior mean of the complete-data information as the matrix;
        the standard errors come, as in `fit_marginal`, from the observed information: central differences in log theta
        (step 1e-4) of the exact gradient at the optimum, symmetrised -- 2 P further evaluations, each of which re-profiles P,
        counted in ``n_iter``.  With ``prior=None`` they are therefore those of the profile likelihood.  No standard errors are
        given for P.  ``logL`` holds the total log evidence; ``prior_fit`` the `MarkovPriorFit` of the accepted evaluation
        (None under a fixed prior).  A NaN or -inf objective at the start raises ValueError; at a trial theta it rejects the step,
        with either kind of prior (the inner fit's `EvidenceNotFinite` is taken as that objective).
        """
        from .exact import DwellPrior, EvidenceNotFinite, exact_dwell_sensitivities, fit_markov_prior, _check_exact_dwell, _markov_start
        start = dict(start)
        params = tuple(start)
        if not params:
            raise ValueError("nothing to fit: start is empty")
        if len(params) > 4:
            raise ValueError("at most 4 parameters")
        theta = np.array([float(start[p]) for p in params])
        if np.any(~np.isfinite(theta)) or np.any(theta <= 0):
            raise ValueError(f"parameters must be positive and finite: {start}")
        if tol <= 0 or max_iter < 1:
            raise ValueError("need tol > 0 and max_iter >= 1")
        if not (prior_tol > 0) or isinstance(prior_max_iter, bool) or not isinstance(prior_max_iter, (int, np.integer)) or prior_max_iter < 1:
            raise ValueError(f"prior_tol = {prior_tol!r} must be positive and prior_max_iter = {prior_max_iter!r} a positive integer")
        items = list(trajs) if isinstance(trajs, (list, tuple)) else [trajs]
        if not items:
            raise ValueError("need at least one trajectory")
        if prior is not None and not isinstance(prior, DwellPrior):
            raise TypeError(f"prior must be a DwellPrior or None, not {type(prior).__name__}")
        if prior is not None and markov_start is not None:
            raise ValueError("markov_start starts the fit of a Markov prior: it needs prior=None")
        probe = cls(family(**dict(zip(params, theta))))
        n_frames = max(len(t) for t in items)
        if prior is None:
            _, P0, init0 = _markov_start(probe, markov_start)
            _check_exact_dwell(items, probe, DwellPrior.markov(P0, init0, n=n_frames), nan)
        else:
            _check_exact_dwell(items, probe, prior, nan)
        state = {'warm': markov_start, 'best': -np.inf, 'fit': None, 'frozen': False}

        def evaluate(th):
            kw = dict(zip(params, th))
            model = cls(family(**kw))
            if derivatives is not None:
                dmsd, dmsd_inf, dmean = derivatives(**kw)
            else:
                dmsd, dmsd_inf, dmean = _log_differences(cls, family, params, th)
            model._derivative_arrays(dmsd, dmsd_inf, dmean)     # (refused before the set is built)
            pf, pr = None, prior
            if prior is None:
                try:
                    pf = fit_markov_prior(items, model, start=state['warm'], tol=prior_tol, max_iter=int(prior_max_iter), nan=nan)
                except EvidenceNotFinite as e:
                    # the objective is e.total here: NaN at the start raises below; a trial theta is rejected as a step and damped,
                    # as under a fixed prior
                    P = len(th)
                    return model, e.total, np.zeros(P), np.zeros((P, P))
                pr = pf.prior(n_frames)
            r = exact_dwell_sensitivities(items, model, pr, dmsd=dmsd, dmsd_inf=dmsd_inf, dmean=dmean, nan=nan)
            g, F = _log_chain_rule(r.grad, r.fisher, np.broadcast_to(th, r.grad.shape))
            total = float(r.log_evidence.sum())
            # `_fisher_scoring`'s acceptance rule (noted there as well): the start, then every evaluation whose objective is
            # finite and strictly larger than every one before
            if not state['frozen'] and np.isfinite(total) and total > state['best']:
                state['best'], state['fit'] = total, pf
                if pf is not None:
                    state['warm'] = (pf.P, pf.init)
            return model, total, g.sum(axis=0), F.sum(axis=0)

        first = evaluate(theta)
        if np.isnan(first[1]):
            hint = " (a trajectory has NaN windows: a later ss_order-0 segment without a valid frame; try nan='omit')" \
                if nan == 'propagate' else ""
            raise ValueError(f"the log evidence is NaN at the start{hint}")
        if first[1] == -np.inf:
            raise ValueError("the log evidence is -inf at the start: a trajectory has no profile of positive weight")
        calls = [first]

        def cached(th):     # the start is evaluated once
            return calls.pop() if calls else evaluate(th)

        res = _fisher_scoring(cached, theta, params, tol, max_iter)
        state['frozen'] = True
        res.prior_fit = state['fit']
        th = np.array([res.params[p] for p in params])
        P, h = len(params), _MARGINAL_INFO_STEP
        H = np.zeros((P, P))
        for p in range(P):
            e = np.zeros(P)
            e[p] = h
            H[:, p] = -(evaluate(th * np.exp(e))[2] - evaluate(th * np.exp(-e))[2]) / (2 * h)
        H = 0.5 * (H + H.T)
        cov = np.linalg.pinv(H) * np.outer(th, th)
        res.cov = cov
        res.se = dict(zip(params, np.sqrt(np.maximum(np.diag(cov), 0.))))
        res.n_iter += 2 * P
        return res

    # ------------------------------------------------------------------ generative model
    def trajectory_from_loopingprofile(self, profile, missing_frames=None, rng=None):
        """
        Sample a trajectory (reference bild/models.py:665-728): interval by interval, each dimension from its state's
        process, conditioned on the previous interval's last point (ss_order 0) or continuing from it (ss_order 1).

        missing_frames : None, a fraction in (0, 1), a number of frames, or an array of frame indices
        rng : numpy Generator (default: a fresh one)
        """
        rng = np.random.default_rng() if rng is None else rng
        T = len(profile)
        if T > self.msd.shape[2]:
            raise ValueError(f"profile of {T} frames: the MSD tables cover {self.msd.shape[2]} lags")
        if missing_frames is None or (np.isscalar(missing_frames) and missing_frames == 0):
            missing = np.array([], dtype=int)
        elif np.isscalar(missing_frames):
            if 0 < missing_frames < 1:
                missing = np.nonzero(rng.random(T) < missing_frames)[0]
            else:
                missing = rng.choice(T, size=int(missing_frames), replace=False).astype(int)
        else:
            missing = np.asarray(missing_frames, dtype=int)

        ivs = profile.intervals()
        ivs[-1] = (ivs[-1][0], T, ivs[-1][2])
        snippets = []
        for i, (t0, t1, n) in enumerate(ivs):
            t_start = 0 if i == 0 else t0 - 1
            snippets.append([])
            for k in range(self.d):
                ti = np.arange(t_start, t1)
                m, o = self.mean[n, k], self.ss_order[n, k]
                C = covariance(self.msd[n, k], self.msd_inf[n, k], ti, o)
                cont = o == 0 and i > 0
                if cont:
                    mu = (snippets[i - 1][k][-1] - m) * C[1:, 0] / C[0, 0]
                    C = (C - C[:, [0]] * C[[0], :] / C[0, 0])[1:, 1:]
                x = (np.linalg.cholesky(C) @ rng.standard_normal(len(C)) if len(C) else np.zeros(0)) + m
                if cont:
                    x = x + mu
                if o == 0:
                    snippets[i].append(x)
                elif i == 0:
                    snippets[i].append(np.insert(np.cumsum(x), 0, 0))
                else:
                    snippets[i].append(snippets[i - 1][k][-1] + np.cumsum(x))
        data = np.concatenate([np.array(snip).T for snip in snippets])
        data[missing] = np.nan
        return Trajectory(data, loopingprofile=profile)

    def trajectories_from_loopingprofiles(self, profiles, missing_frames=None, rng=None, seed=None):
        """
        Many trajectories at once, generated on the GPU: one Cholesky factor per (state, dimension)
        serves every interval, so a trajectory costs one triangular product per interval and dimension.

        profiles : sequence of `Loopingprofile` or 1-d integer arrays (lengths may differ), or an (n, T) integer array;
            at most `max_T` frames each
        missing_frames : one of `trajectory_from_loopingprofile`'s forms (None, a fraction, a count, an index array -- as
            a NumPy array), applied to every trajectory, or a list / tuple with one such entry per trajectory
        rng : numpy Generator -- replay mode: the host draws exactly the numbers that
            ``[self.trajectory_from_loopingprofile(p, missing_frames, rng=rng) for p in profiles]`` draws, in the same
            order, and leaves ``rng`` where that loop would; the results equal the loop's to rounding.
        seed : int in [0, 2**64) -- device mode (also when neither ``rng`` nor ``seed`` is given, with a fresh seed): the
            normals come from a counter-based generator on the device; trajectory ``i`` is a pure function of
            (seed, i, its profile, its missing frames), and its missing frames are drawn from
            ``np.random.default_rng([seed, i])``.

        The model keeps its factors on the device after the first call (and rebuilds them, once, for a longer
        trajectory).  A covariance that is not positive definite raises numpy.linalg.LinAlgError, as the loop does.

        Returns
        -------
        list of `Trajectory`, one per profile and in order
        """
        if rng is not None and seed is not None:
            raise ValueError("give either rng (replay mode) or seed (device mode), not both")
        items = list(profiles)
        states = [np.asarray(p[:]) for p in items]
        S = self.nStates
        for i, st in enumerate(states):
            if st.ndim != 1 or len(st) < 1 or not np.issubdtype(st.dtype, np.integer):
                raise ValueError(f"profile {i} is not a non-empty 1-d integer array")
            if st.min() < 0 or st.max() >= S:
                raise ValueError(f"profile {i} has a state outside 0 .. {S - 1}")
            if len(st) > self.max_T:
                raise ValueError(f"profile {i} has {len(st)} frames: GenericGaussianModel generates at most {self.max_T} "
                                 f"(the GPU takes up to {MAX_T} frames, the MSD tables cover {self.msd.shape[2]} lags)")
        n = len(states)
        if isinstance(missing_frames, (list, tuple)):
            if len(missing_frames) != n:
                raise ValueError(f"missing_frames has {len(missing_frames)} entries for {n} profiles")
            specs = list(missing_frames)
        else:
            specs = [missing_frames] * n
        if seed is not None:
            seed = int(seed)
            if not 0 <= seed < 2 ** 64:
                raise ValueError("seed must be an integer in [0, 2**64)")
        if n == 0:
            return []

        T = np.array([len(st) for st in states], dtype=np.int64)
        seg_start, seg_state = _ragged_segments(states, T)
        d = self.d
        offs = np.concatenate([[0], np.cumsum(T)])

        if rng is None:     # device mode
            mask = np.zeros(int(offs[-1]), dtype=bool)
            if seed is None:
                seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
            for i, spec in enumerate(specs):
                if not _missing_is_none(spec):
                    drawn = np.isscalar(spec)
                    mask[offs[i]:offs[i + 1]][_missing_frames(spec, int(T[i]), np.random.default_rng([seed, i]) if drawn else None)] = True
            data = _lib.gauss_simulate(self.handle(), T, seg_start, seg_state, mask, seed=seed)
        else:               # replay mode: host groups of at most _REPLAY_GROUP_BYTES of normals
            per = normals_per_trajectory(self.ss_order, seg_state[:, 0], T)
            data = np.empty((int(offs[-1]), d))
            i0 = 0
            while i0 < n:
                i1 = i0 + 1
                while i1 < n and per[i0:i1 + 1].sum() * 8 <= _REPLAY_GROUP_BYTES:
                    i1 += 1
                mask, z = _draw_normals(specs[i0:i1], T[i0:i1], per[i0:i1], rng)
                data[offs[i0]:offs[i1]] = _lib.gauss_simulate(self.handle(), T[i0:i1], seg_start[i0:i1], seg_state[i0:i1], mask,
                                                              normals=z)
                i0 = i1
        return [Trajectory(data[offs[i]:offs[i + 1]], loopingprofile=items[i]) for i in range(n)]


_LOG_STEP = 1e-5
_MARGINAL_INFO_STEP = 1e-4      # fit_marginal: step in log theta of the observed information's central differences


def _log_differences(cls, family, params, theta, h=_LOG_STEP):
    """
    d(msd, msd_inf, mean) / d theta of the family's tabulated arrays by central differences in log theta (step h):
    -> dmsd (P, S, d, n_lags), dmsd_inf, dmean (P, S, d)
    """
    out = None
    for p in range(len(params)):
        tabs = []
        for sgn in (1.0, -1.0):
            th = np.array(theta, dtype=np.float64)
            th[p] *= np.exp(sgn * h)
            tabs.append(cls(family(**dict(zip(params, th))))._tables())
        if out is None:
            out = [np.zeros((len(params),) + t.shape) for t in tabs[0]]
        for o, hi, lo in zip(out, tabs[0], tabs[1]):
            if hi.shape != o.shape[1:]:
                raise ValueError("the family's models differ in the shape of their tables")
            o[p] = (hi - lo) / (2 * h * theta[p])
    return tuple(out)


def normals_per_trajectory(ss_order, first_state, T):
    """
    How many normals `GenericGaussianModel.trajectory_from_loopingprofile` draws for a trajectory of T frames whose first
    state is ``first_state``: per dimension T, one fewer where that state has ss_order 1 (its first frame is 0).
    Vectorised over trajectories.
    """
    ss_order = np.asarray(ss_order)
    return np.asarray(T, dtype=np.int64) * ss_order.shape[1] - ss_order[np.asarray(first_state)].sum(axis=1)
