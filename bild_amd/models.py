"""
Inference models: the interface (`MultiStateModel`) and the GPU-backed multi-state Rouse
model (`MultiStateRouse`).

Counterpart of reference bild/models.py:24-370 for the one hot path this package
accelerates.  `MultiStateRouse` keeps the reference's constructor, attributes
(``models``, ``measurement``, ``localization_error``, ``transitions``, ``nStates``, ``d``)
and ``logL(profile, traj) -> float`` contract, so it can be handed to
``bild.amis.FixedkSampler`` / ``bild.core.sample`` / ``bild.postproc`` unchanged; in
addition it offers batched entry points that evaluate a whole AMIS step in one launch.

The likelihood itself runs on the GPU through the C ABI in include/bild_amd.h; there is no
CPU implementation in this package.
"""
import abc
from collections import OrderedDict

import numpy as np

from . import _lib
from . import rouse
from .profiles import Loopingprofile, segments_from_states
from .trajectory import Trajectory, as_array


class MultiStateModel(metaclass=abc.ABCMeta):
    """
    Interface used by the samplers (reference bild/models.py:24-160).

    Attributes
    ----------
    transitions : (n, n) bool -- ``transitions[i, j]``: is the switch i -> j allowed
    """

    def init_transitions(self, n):
        self.transitions = ~np.eye(n, dtype=bool)

    @property
    def nStates(self):
        return self.transitions.shape[0]

    @property
    def d(self):
        raise NotImplementedError  # pragma: no cover

    def initial_loopingprofile(self, traj):
        return Loopingprofile(np.random.choice(self.nStates, size=len(traj)))

    @abc.abstractmethod
    def logL(self, loopingprofile, traj):
        raise NotImplementedError  # pragma: no cover


class MultiStateRouse(MultiStateModel):
    """
    Multi-state Rouse model with a Kalman-filter likelihood evaluated on the GPU.

    Parameters are those of reference bild/models.py:222-228:

    N : int -- number of monomers
    D, k : float -- Rouse parameters
    d : int -- spatial dimension (1..8)
    looppositions : tuple -- per state ``None`` (no extra bond), ``(i, j[, rel_strength])`` or a
        list of such
    measurement : "end2end" or (N,) array
    localization_error : float, (d,) array or None (then ``traj.localization_error`` is used)

    Extra keyword:
    path : 'auto' | 'modal' | 'dense' -- kernel path (see include/bild_amd.h)
    """

    def __init__(self, N, D, k, d=3,
                 looppositions=(None, (0, -1)),
                 measurement="end2end",
                 localization_error=None,
                 path='auto',
                 ):
        self._d = d
        # what with_parameters needs to rebuild the model (looppositions are not stored otherwise)
        self._ctor = dict(N=N, D=D, k=k, d=d, looppositions=tuple(looppositions), measurement=measurement, path=path)

        if str(measurement) == "end2end":
            measurement = np.zeros(N)
            measurement[0] = -1
            measurement[-1] = 1
        measurement = np.asarray(measurement, dtype=np.float64)
        assert len(measurement) == N
        self.measurement = measurement

        if localization_error is not None and np.isscalar(localization_error):
            localization_error = localization_error * np.ones(d)
        self.localization_error = localization_error

        self.models = []
        for loop in looppositions:
            if loop is not None and np.isscalar(loop[0]):
                loop = [loop]
            self.models.append(rouse.Model(N, D, k, d, add_bonds=loop))

        self.init_transitions(len(self.models))

        self.path = path
        self._handle = None
        self._trajsets = OrderedDict()  # small LRU of device-resident trajectory sets

    # ------------------------------------------------------------------ interface
    @property
    def d(self):
        return self._d

    def _get_noise(self, traj):
        # precedence model > trajectory > error: reference bild/models.py:255-263
        if self.localization_error is not None:
            return np.asarray(self.localization_error)
        elif getattr(traj, 'localization_error', None) is not None:
            return np.asarray(traj.localization_error)
        else:
            raise ValueError("No localization error specified (use MultiStateModel.localization_error "
                             "or Trajectory.localization_error)")

    # ------------------------------------------------------------------ device state
    @classmethod
    def from_arrays(cls, B, G, Sig, M0, C0, measurement, localization_error=None, path='auto'):
        """
        Build directly from per-state arrays (e.g. taken from an installed ``rouse``:
        ``m._dynamics['B'|'G'|'Sig']`` and ``m.steady_state()``), bypassing this package's
        own Rouse matrix builder.
        """
        self = cls.__new__(cls)
        G = np.asarray(G, dtype=np.float64)
        S, N, d = G.shape
        self._d = d
        self.measurement = np.asarray(measurement, dtype=np.float64)
        if localization_error is not None and np.isscalar(localization_error):
            localization_error = localization_error * np.ones(d)
        self.localization_error = localization_error
        self.models = None
        self._arrays = dict(B=B, G=G, Sig=Sig, M0=M0, C0=C0)
        self.init_transitions(S)
        self.path = path
        self._handle = None
        self._trajsets = OrderedDict()
        return self

    @classmethod
    def from_reference(cls, ref_model, path='auto'):
        """
        Build from a reference ``bild.models.MultiStateRouse`` (or anything with its attribute surface:
        ``models[i]._dynamics['B'|'G'|'Sig']``, ``.check_dynamics()``, ``.steady_state()``, ``measurement``,
        ``localization_error``; reference bild/src/MSRouse_logL.pyx:150-160): the matrices of the installed
        ``rouse`` package are used as they are, bypassing this package's own Rouse builder.
        """
        for mod in ref_model.models:
            mod.check_dynamics()
        steady = [mod.steady_state() for mod in ref_model.models]
        return cls.from_arrays(B=np.array([mod._dynamics['B'] for mod in ref_model.models]),
                               G=np.array([mod._dynamics['G'] for mod in ref_model.models]),
                               Sig=np.array([mod._dynamics['Sig'] for mod in ref_model.models]),
                               M0=np.array([st[0] for st in steady]), C0=np.array([st[1] for st in steady]),
                               measurement=ref_model.measurement,
                               localization_error=getattr(ref_model, 'localization_error', None), path=path)

    def __getstate__(self):
        # device handles are not state: they are recreated on first use after unpickling / copying
        state = dict(self.__dict__)
        state['_handle'] = None
        state['_trajsets'] = OrderedDict()
        return state

    def arrays(self):
        """ stacked (B, G, Sig, M0, C0) over states, as the kernel consumes them (pyx:152-163) """
        if self.models is None:
            return self._arrays
        return rouse.stack_dynamics(self.models)

    def handle(self):
        if self._handle is None:
            a = self.arrays()
            self._handle = _lib.ModelHandle(a['B'], a['G'], a['Sig'], a['M0'], a['C0'], self.measurement)
        return self._handle

    def invalidate(self):
        """ call after changing ``models`` / ``measurement`` in place """
        self._handle = None
        self._trajsets.clear()

    def trajset(self, trajs, expect=None):
        """
        Device-resident set of trajectories (uploaded once, reused across AMIS steps).

        trajs : a trajectory or a list of trajectories
        expect : optional, the number of evaluations the set will see in total (`bild_trajset_expect`): a few single
            evaluations per trajectory are cheaper without the set's tables.  The declaration decides which tables the set
            builds (none below 300 evaluations, prefix + transient tables below 3000, all of them above or when nothing is
            declared -- the transient state table up to 4 GB, up to 64 GB from 1e8 evaluations on) and is therefore part of
            the cache key: a set declared for ten evaluations is never handed to an AMIS
            run (which asks without a declaration), and the other way round.

        The cache is keyed by the IDENTITY of the trajectory objects, and an entry is trusted while the address and shape
        of each trajectory's data, the localization errors in force and a content guard (the sum of the bit patterns of
        all values; a strided subsample of 65 536 of them for longer data) are unchanged: a lookup costs microseconds.
        In-place edits (masking frames with NaN, rescaling, refilling a preallocated array, changing single values)
        therefore lead to a fresh upload and fresh tables; only for data of more than 65 536 values can an edit between
        the guard's sample points go unnoticed -- call `invalidate()` after editing such data in place.  Trajectory-likes
        whose ``t[:]`` builds a new array on every access are keyed by a hash of their contents instead, so that they are
        not uploaded again on every call.
        """
        single = not isinstance(trajs, (list, tuple))
        items = (trajs,) if single else tuple(trajs)
        prints, arrs = self._fingerprints(items)
        if expect is not None and expect < 0:
            raise ValueError("expect must be a non-negative number of evaluations")
        # (tables.cpp: kExpectPrefix, kExpectPairs, and the budget of the transient state table: 64 instead of 4 GB from 1e8 on)
        table_class = 2 if expect is None else (3 if expect >= 10 ** 8 else 2 if expect >= 3000 else 1 if expect >= 300 else 0)
        key = (table_class,) + tuple(id(t) if p[0] is not None else p for t, p in zip(items, prints))
        hit = self._trajsets.get(key)
        if hit is not None:
            ts, kept, old_prints = hit
            if all(a is b or p[0] is None for a, b, p in zip(kept, items, prints)) and old_prints == prints:
                self._trajsets.move_to_end(key)
                return ts
        noises = [np.frombuffer(p[2], dtype=np.float64) for p in prints]
        ts = _lib.TrajSetHandle(self.handle(), arrs, np.stack(noises))
        if expect is not None:
            ts.expect(expect)
        self._trajsets[key] = (ts, items, prints)   # `items` keeps the objects (and their ids) alive
        while len(self._trajsets) > 8:
            self._trajsets.popitem(last=False)
        return ts

    def _fingerprints(self, items):
        """ per trajectory: (data address or None, shape, noise bytes, content guard); and the data arrays themselves """
        out, arrs = [], []
        for t in items:
            view = t[:]
            a = view if (type(view) is np.ndarray and view.dtype == np.float64 and view.ndim == 2 and view.flags.c_contiguous) \
                else as_array(t)
            arrs.append(a)
            noise = np.ascontiguousarray(self._get_noise(t), dtype=np.float64).tobytes()
            addr = _lib.aptr(view) if isinstance(view, np.ndarray) else None
            # `t[:]` of an ndarray or of this package's Trajectory is a view of one buffer; anything else is asked twice
            stable = addr is not None and (type(t) in (np.ndarray, Trajectory) or
                                           (isinstance(t[:], np.ndarray) and t[:].__array_interface__['data'][0] == addr))
            if stable:
                # the guard: the sum of the bit patterns -- every value takes part (NaNs included, which an ordinary sum would
                # drown in); beyond 65 536 values a strided subsample of that many
                bits = a.reshape(-1).view(np.uint64)
                if bits.size > 65536:
                    bits = bits[::bits.size // 65536 + 1]
                out.append((addr, a.shape, noise, int(np.add.reduce(bits))))
            else:   # no stable buffer to identify the data by: the contents are the key
                out.append((None, a.shape, noise, hash(a.tobytes())))
        return out, arrs

    # ------------------------------------------------------------------ likelihood
    def logL(self, profile, traj):
        """
        log p(traj | profile, model), reference bild/models.py:265-278 -> MSRouse_logL.

        Returns
        -------
        float
        """
        states = np.asarray(profile[:])
        assert len(states) == len(traj)
        return float(_lib.logl_profiles(self.handle(), self.trajset(traj), states[None, :], path=self.path)[0])

    def logL_batch(self, profiles, traj):
        """ many expanded profiles on one trajectory: (n, T) int array or list of Loopingprofile -> (n,) """
        if not isinstance(profiles, np.ndarray):
            profiles = np.stack([np.asarray(p[:]) for p in profiles])
        seg_start, seg_state = segments_from_states(profiles)
        return _lib.logl_segments(self.handle(), self.trajset(traj), seg_start, seg_state, path=self.path)

    def logL_st_batch(self, ss, thetas, traj):
        """
        One AMIS batch in (s, theta) parametrisation: what reference
        ``FixedkSampler.logL(ss, thetas)`` (bild/amis.py:717-739) computes with a Python loop.
        """
        return _lib.logl_st(self.handle(), self.trajset(traj), ss, thetas, path=self.path)

    def logL_st_batch_to_device(self, ss, thetas, traj, d_out, stream=0):
        """
        Same batch, results left in HBM at the raw device pointer ``d_out`` (float64[len(thetas)]), asynchronous on
        the HIP stream ``stream``: what `dist.ShardedModel` feeds into the all-gather of a multi-GPU AMIS step.
        """
        _lib.logl_st_to_device(self.handle(), self.trajset(traj), ss, thetas, d_out, stream=stream, path=self.path)

    def check_st_rows(self):
        """
        `logL_st_batch_to_device` waits for nothing and cannot refuse a row that is no point on the simplex (it gets NaN):
        this waits for the pending calls and raises if one of their rows was refused (bild_logl_st_status)
        """
        _lib.logl_st_status(self.handle())

    def logL_st(self, s, theta, traj):
        """ the per-sample hook the reference sampler prefers when present (bild/amis.py:734-736) """
        return float(self.logL_st_batch(np.asarray(s)[None, :], np.asarray(theta)[None, :], traj)[0])

    def logL_segments(self, seg_start, seg_state, trajs, traj_id=None):
        """ general batch: run-length encoded profiles over a set of trajectories """
        return _lib.logl_segments(self.handle(), self.trajset(trajs), seg_start, seg_state, traj_id, path=self.path)

    # ------------------------------------------------------------------ filter and smoother
    def kalman(self, profiles, trajs, traj_id=None, outputs=('smooth',), scratch_bytes=0):
        """
        Per-frame moments of the Kalman filter and smoother of candidate profiles (bild_kalman_segments), for the
        noise-free measured distance y_t = w.x_t of each dimension.

        profiles : (n, T) int array or list of Loopingprofile, on the one trajectory ``trajs``; or ``(seg_start,
            seg_state)``, each (n, K1), run-length encoded as `logL_segments` takes them, on the list ``trajs`` with
            ``traj_id`` (n,) (None: all on the first)
        outputs : subset of 'terms', 'pred', 'filt', 'smooth', 'innov'
        scratch_bytes : device workspace of one chunk of the call (0: at most 1 GiB and a third of the free memory)

        Returns a `KalmanResult`: the requested arrays, each (n, T_max, d), NaN behind a trajectory's own length; the
        others are None.  The trajectory set is the one `trajset` gives (an AMIS run's set is reused); its likelihood
        tables are neither built nor read.  Argument and envelope errors are raised before any set is created.
        """
        outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
        for o in outputs:
            if o not in KalmanResult.GROUPS:
                raise ValueError(f"unknown output {o!r}; choose from {sorted(KalmanResult.GROUPS)}")
        items, seg_start, seg_state, tid = self._kalman_args(profiles, trajs, traj_id)
        self._kalman_envelope()
        names = [name for o in outputs for name in KalmanResult.GROUPS[o]]
        ts = self.trajset(items if len(items) > 1 or isinstance(trajs, (list, tuple)) else items[0])
        res = _lib.kalman_segments(self.handle(), ts, seg_start, seg_state, tid, outputs=names, scratch_bytes=scratch_bytes)
        return KalmanResult(res)

    def kalman_mixture(self, profiles, trajs, log_weights, traj_id=None, scratch_bytes=0):
        """
        Posterior mixture of the smoothed y over weighted candidates (bild_kalman_mixture): per trajectory of ``trajs``,
        the candidates on it weighted by exp(log_weights), normalised within the trajectory.  Arguments as for `kalman`.
        -> (mean, var), each (n_traj, T_max, d); NaN for a trajectory without candidates of finite weight.
        """
        items, seg_start, seg_state, tid = self._kalman_args(profiles, trajs, traj_id)
        log_weights = np.asarray(log_weights, dtype=np.float64).reshape(-1)
        if log_weights.shape != (len(seg_start),):
            raise ValueError(f"{len(log_weights)} log-weights for {len(seg_start)} candidates")
        if np.any(np.isnan(log_weights)) or np.any(log_weights == np.inf):
            raise ValueError("log-weights must be finite or -inf (NaN or +inf given)")
        self._kalman_envelope()
        ts = self.trajset(items if len(items) > 1 or isinstance(trajs, (list, tuple)) else items[0])
        return _lib.kalman_mixture(self.handle(), ts, seg_start, seg_state, log_weights, tid, scratch_bytes=scratch_bytes)

    def _kalman_args(self, profiles, trajs, traj_id):
        """ -> (trajectories, seg_start, seg_state, traj_id or None), checked on the host """
        items = list(trajs) if isinstance(trajs, (list, tuple)) else [trajs]
        if not items:
            raise ValueError("need at least one trajectory")
        lengths = [len(t) for t in items]
        if isinstance(profiles, tuple) and len(profiles) == 2 and not isinstance(profiles[0], Loopingprofile):
            seg_start = np.ascontiguousarray(profiles[0], dtype=np.int32)
            seg_state = np.ascontiguousarray(profiles[1], dtype=np.int32)
            if seg_start.ndim != 2 or seg_start.shape != seg_state.shape or seg_start.shape[1] < 1:
                raise ValueError(f"seg_start {seg_start.shape} and seg_state {seg_state.shape} must both be (n, K1)")
            n = len(seg_start)
            if traj_id is not None:
                traj_id = np.ascontiguousarray(traj_id, dtype=np.int32).reshape(-1)
                if traj_id.shape != (n,):
                    raise ValueError(f"traj_id has {traj_id.size} entries for {n} candidates")
                if n and (traj_id.min() < 0 or traj_id.max() >= len(items)):
                    raise ValueError(f"traj_id out of range for {len(items)} trajectories")
            if n and (np.any(seg_start[:, 0] != 0) or np.any(np.diff(seg_start, axis=1) < 0) or np.any(seg_start[:, 1:] < 1)):
                raise ValueError("segment starts must begin at 0 and be non-decreasing (later starts >= 1)")
            if n and (seg_state.min() < 0 or seg_state.max() >= self.nStates):
                raise ValueError(f"states out of range ({self.nStates} states)")
            return items, seg_start, seg_state, traj_id
        if traj_id is not None:
            raise ValueError("traj_id goes with (seg_start, seg_state) profiles")
        if len(items) != 1:
            raise ValueError("expanded profiles refer to one trajectory")
        states = profiles if isinstance(profiles, np.ndarray) else np.stack([np.asarray(p[:]) for p in profiles])
        states = np.atleast_2d(np.asarray(states))
        if states.ndim != 2 or states.shape[1] != lengths[0]:
            raise ValueError(f"profiles of shape {states.shape} do not match a trajectory of {lengths[0]} frames")
        if states.size and (states.min() < 0 or states.max() >= self.nStates):
            raise ValueError(f"states out of range ({self.nStates} states)")
        seg_start, seg_state = segments_from_states(states.astype(np.int32))
        return items, seg_start, seg_state, None

    def _kalman_envelope(self):
        """ the smoother's envelope (csrc/kalman.cpp), checked on the model handle alone: no device work """
        h = self.handle()
        why = None
        if not h.query(_lib.Q_MODAL_OK):
            why = "the smoother needs the modal path, which this model lacks (B, Sig or C0 not symmetric, or no common eigenbasis)"
        elif h.query(_lib.Q_NEFF) > 32:
            why = f"the smoother supports at most 32 effective modes; this model has {h.query(_lib.Q_NEFF)}"
        elif h.query(_lib.Q_D) > 8:
            why = f"the smoother supports at most 8 dimensions; d = {h.query(_lib.Q_D)}"
        elif h.query(_lib.Q_S) > 255:
            why = f"the smoother supports at most 255 states; S = {h.query(_lib.Q_S)}"
        if why is not None:
            raise _lib.BildAmdError(_lib.ERR_UNSUPPORTED, why)

    # ------------------------------------------------------------------ parameter sensitivities and fit
    PARAMS = ('D', 'k', 'localization_error')

    def logL_sensitivities(self, profiles, trajs, params=('D', 'k', 'localization_error'), traj_id=None, log=True, fisher=True,
                           scratch_bytes=0, derivatives=None):
        """
        Log-likelihood of candidate profiles with its gradient and Fisher information with respect to model parameters
        (bild_logl_sensitivities: forward sensitivities of the filter).

        profiles, trajs, traj_id : as for `kalman`
        params : names out of 'D', 'k', 'localization_error' (at most 4).  'localization_error' is one sigma shared by all
            dimensions: the model's own when it has one, else each trajectory's (which must then be equal across its
            dimensions).  Models built with `from_arrays` / `from_reference` have no D or k: pass ``derivatives`` instead.
        log : differentiate with respect to log theta (the gradient times theta, the Fisher entries times theta_p theta_q)
        fisher : compute the Fisher information (innovations form: sum over observed frames and dimensions of
            dS_p dS_q / (2 S^2) + de_p de_q / S)
        derivatives : raw derivatives instead of ``params`` -- a dict with any of dB, dSig, dC0 (P, S, N, N), dG, dM0
            (P, S, N, d) and ds2 (P, n_traj, d: the derivative of the variance of each dimension of each trajectory); then
            ``log`` must be False

        Returns (logL (n,), grad (n, P), fisher (n, P, P) or None).
        """
        items, seg_start, seg_state, tid = self._kalman_args(profiles, trajs, traj_id)
        if derivatives is not None:
            if log:
                raise ValueError("raw derivatives are derivatives with respect to theta: pass log=False with them")
            derivs = {k: v for k, v in derivatives.items() if k != 'ds2'}
            ds2 = derivatives.get('ds2')
            lens = {len(np.asarray(v)) for v in derivatives.values() if v is not None}
            if len(lens) > 1:
                raise ValueError(f"derivative arrays disagree on the number of parameters: {sorted(lens)}")
            P = lens.pop() if lens else 0
            theta = None
        else:
            params = self._check_params(params)
            P = len(params)
            derivs, ds2, theta = self._derivatives(params, items)
        if P > 4:
            raise _lib.BildAmdError(_lib.ERR_UNSUPPORTED, f"at most 4 parameters per call; {P} given")
        self._kalman_envelope()
        if P > 0 and self.handle().query(_lib.Q_NEFF) > 16:
            raise _lib.BildAmdError(_lib.ERR_UNSUPPORTED, f"models of 17 to 32 effective modes (this one has "
                                    f"{self.handle().query(_lib.Q_NEFF)}) support no parameters; {P} given")
        ts = self.trajset(items if len(items) > 1 or isinstance(trajs, (list, tuple)) else items[0])
        logl, grad, F = _lib.logl_sensitivities(self.handle(), ts, seg_start, seg_state, tid, derivs=derivs, ds2=ds2, P=P,
                                                fisher=fisher, scratch_bytes=scratch_bytes)
        if log and P:
            th = theta[np.zeros(len(logl), dtype=int) if tid is None else tid]     # (n, P): theta of each candidate
            grad, F = _log_chain_rule(grad, F, th)
        return logl, grad, F

    def _check_params(self, params):
        params = (params,) if isinstance(params, str) else tuple(params)
        for p in params:
            if p not in self.PARAMS:
                raise ValueError(f"unknown parameter {p!r}; choose from {self.PARAMS}")
        if len(set(params)) != len(params):
            raise ValueError(f"parameters repeat: {params}")
        if self.models is None and any(p in ('D', 'k') for p in params):
            raise ValueError("this model was built from arrays (from_arrays / from_reference): it has no D or k; "
                             "pass derivatives= with the raw derivative arrays instead")
        return params

    def _sigma(self, items):
        """ the one localization error per trajectory that 'localization_error' differentiates (n_traj,) """
        sig = []
        for t in items:
            err = np.asarray(self._get_noise(t), dtype=np.float64).reshape(-1)
            if err.size != 1 and np.any(err != err[0]):
                raise ValueError(f"'localization_error' is one sigma shared by all dimensions; this trajectory has {err}")
            sig.append(float(err[0]))
        return np.array(sig)

    def _derivatives(self, params, items):
        """ -> (raw derivative arrays, ds2 (P, n_traj, d) or None, theta (n_traj, P)) """
        S, N, d = self.nStates, len(self.measurement), self.d
        derivs = {k: np.zeros((len(params), S, N, N if k in ('dB', 'dSig', 'dC0') else d)) for k in _lib.DERIV_NAMES}
        ds2 = None
        theta = np.zeros((len(items), len(params)))
        for p, name in enumerate(params):
            if name == 'localization_error':
                sig = self._sigma(items)
                ds2 = np.zeros((len(params), len(items), d)) if ds2 is None else ds2
                ds2[p] = 2. * sig[:, None]
                theta[:, p] = sig
                continue
            for s, m in enumerate(self.models):
                for k, v in m.dynamics_derivatives(name).items():
                    derivs[k][p, s] = v
            theta[:, p] = self._ctor[name]
        return derivs, ds2, theta

    def with_parameters(self, D=None, k=None, localization_error=None):
        """ a new model with the same bonds, measurement, d and path, and the parameters given replaced """
        if self.models is None:
            raise ValueError("this model was built from arrays (from_arrays / from_reference): it has no D or k to replace")
        c = dict(self._ctor)
        if D is not None:
            c['D'] = float(D)
        if k is not None:
            c['k'] = float(k)
        err = self.localization_error if localization_error is None else localization_error
        out = MultiStateRouse(c['N'], c['D'], c['k'], d=c['d'], looppositions=c['looppositions'], measurement=self.measurement,
                              localization_error=err, path=c['path'])
        out.transitions = self.transitions.copy()
        return out

    def fit(self, trajs, profiles, params=('D', 'k', 'localization_error'), start=None, tol=1e-8, max_iter=50):
        """
        Maximum-likelihood fit of the parameters ``params`` (out of 'D', 'k', 'localization_error') on trajectories whose
        looping profiles are known, by Fisher scoring in log theta with Levenberg damping.

        trajs : list of trajectories
        profiles : one per trajectory (a `Loopingprofile`, a 1-d integer array, or ``(seg_start, seg_state)`` of shape
            (n_traj, K1) for all of them), or a single state index: a constant profile
        start : dict of starting values (default: this model's)
        tol, max_iter : the fit stops when the Newton decrement g^T F^-1 g / 2 falls below ``tol``, or after ``max_iter``
            device calls

        Every iteration is one `logL_sensitivities` call over all trajectories; a step is accepted only if the total
        logL rises, else the damping grows.  A call builds the model at the trial parameters on the host and uploads the
        trajectories again (a new model has a new trajectory set): for N = 20 that is well under a millisecond of model
        analysis per call, and the upload is one copy of the data.  Parameters not listed stay as they are.  Fitting
        'localization_error' sets the model-level localization error, which takes precedence over the trajectories' own
        (reference bild/models.py:255-263); without it the noise in force stays what it was.

        Returns a `FitResult`: the fitted model, params, standard errors (inverse Fisher information at the optimum, by
        the delta method from log theta), their covariance, logL, n_iter, converged and the history.
        """
        params = self._check_params(params)
        if not params:
            raise ValueError("nothing to fit: params is empty")
        if len(params) > 4:
            raise ValueError("at most 4 parameters")
        if self.models is None:
            raise ValueError("this model was built from arrays (from_arrays / from_reference): it cannot be refitted")
        items = list(trajs) if isinstance(trajs, (list, tuple)) else [trajs]
        if not items:
            raise ValueError("need at least one trajectory")
        seg = _fit_profiles(profiles, [len(t) for t in items], self.nStates)
        if tol <= 0 or max_iter < 1:
            raise ValueError("need tol > 0 and max_iter >= 1")
        cur = self._current_params(items, params)
        start = {} if start is None else dict(start)
        for kname in start:
            if kname not in params:
                raise ValueError(f"start value for {kname!r}, which is not fitted")
        theta = np.array([float(start.get(p, cur[p])) for p in params])
        if np.any(~np.isfinite(theta)) or np.any(theta <= 0):
            raise ValueError(f"parameters must be positive and finite: {dict(zip(params, theta))}")
        tid = np.arange(len(items), dtype=np.int32)

        def evaluate(th):
            model = self._model_at(params, th)
            logl, g, F = model.logL_sensitivities(seg, items, params=params, traj_id=tid, log=True)
            return model, float(logl.sum()), g.sum(axis=0), F.sum(axis=0)

        return _fisher_scoring(evaluate, theta, params, tol, max_iter)

    def _current_params(self, items, params):
        out = {'D': self._ctor['D'], 'k': self._ctor['k']}
        if 'localization_error' in params:
            out['localization_error'] = float(self._sigma(items)[0])
        return out

    def _model_at(self, params, theta):
        kw = {p: float(v) for p, v in zip(params, theta)}
        return self.with_parameters(**kw)

    # ------------------------------------------------------------------ generative model
    def initial_loopingprofile(self, traj):
        """ initial guess: the per-frame best state of the factorized model (reference bild/models.py:280-293) """
        return self.toFactorized().initial_loopingprofile(traj)

    def toFactorized(self):
        """
        The `FactorizedModel` that draws every frame from the steady-state distance distribution of its
        state (reference bild/models.py:352-370): Maxwell with scale^2 = w.C0.w + mean squared localization
        error per dimension.  CPU only, cheap; not a substitute for `logL`.
        """
        from scipy import stats
        err = self.localization_error
        noise2_per_d = np.sum(np.asarray(err) ** 2) / self.d if err is not None else 0
        w = self.measurement
        return FactorizedModel([stats.maxwell(scale=np.sqrt(w @ C0 @ w + noise2_per_d)) for C0 in self.arrays()['C0']],
                               d=self.d)

    def trajectory_from_loopingprofile(self, profile, localization_error=None, missing_frames=None, rng=None):
        """
        Sample a trajectory from the model (reference bild/models.py:295-350): steady-state
        conformation of ``profile[0]``, propagate with ``profile[t]``, measure, blank the
        missing frames, then add localization noise.
        """
        rng = np.random.default_rng() if rng is None else rng
        localization_error = _localization_error(self, localization_error)
        T = len(profile)
        missing = _missing_frames(missing_frames, T, rng)

        data = np.full((T, self.d), np.nan)
        conf = self.models[profile[0]].conf_ss(rng)
        data[0] = self.measurement @ conf
        for i in range(1, T):
            conf = self.models[profile[i]].evolve(conf, rng)
            data[i] = self.measurement @ conf
        data[missing, :] = np.nan
        data += localization_error[None, :] * rng.standard_normal(data.shape)
        return Trajectory(data, localization_error=localization_error, loopingprofile=profile)

    def trajectories_from_loopingprofiles(self, profiles, localization_error=None, missing_frames=None, rng=None, seed=None):
        """
        Many trajectories at once, generated on the GPU in each state's modal coordinates.

        profiles : sequence of `Loopingprofile` or 1-d integer arrays (lengths may differ), or an (n, T) integer array
        localization_error : as for `trajectory_from_loopingprofile`
        missing_frames : one of that method's forms (None, a fraction, a count, an index array -- as a NumPy array),
            applied to every trajectory, or a list / tuple with one such entry per trajectory
        rng : numpy Generator -- replay mode: the host draws exactly the numbers that
            ``[self.trajectory_from_loopingprofile(p, localization_error, missing_frames, rng=rng) for p in profiles]``
            draws, in the same order, and leaves ``rng`` where that loop would; the results equal the loop's to rounding.
        seed : int in [0, 2**64) -- device mode (also when neither ``rng`` nor ``seed`` is given, with a fresh seed): the
            normals come from a counter-based generator on the device; trajectory ``i`` is a pure function of
            (seed, i, its profile, its missing frames), and its missing frames are drawn from
            ``np.random.default_rng([seed, i])``.

        Returns
        -------
        list of `Trajectory`, one per profile and in order
        """
        if rng is not None and seed is not None:
            raise ValueError("give either rng (replay mode) or seed (device mode), not both")
        if self.models is None:
            raise ValueError("this model was built from arrays (from_arrays / from_reference): it has no per-state eigenbasis, "
                             "so it cannot generate trajectories (trajectory_from_loopingprofile cannot either)")
        items = list(profiles)
        states = [np.asarray(p[:]) for p in items]
        S = self.nStates
        for i, st in enumerate(states):
            if st.ndim != 1 or len(st) < 1 or not np.issubdtype(st.dtype, np.integer):
                raise ValueError(f"profile {i} is not a non-empty 1-d integer array")
            if st.min() < 0 or st.max() >= S:
                raise ValueError(f"profile {i} has a state outside 0 .. {S - 1}")
        err = _localization_error(self, localization_error)
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

        arrs = self._modal_arrays()
        T = np.array([len(st) for st in states], dtype=np.int64)
        seg_start, seg_state = _ragged_segments(states, T)
        errs = np.tile(err, (n, 1))
        N, d = self.measurement.shape[0], self.d
        offs = np.concatenate([[0], np.cumsum(T)])

        if rng is None:     # device mode
            mask = np.zeros(int(offs[-1]), dtype=bool)
            if seed is None:
                seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0])
            for i, spec in enumerate(specs):
                if not _missing_is_none(spec):
                    drawn = np.isscalar(spec)
                    mask[offs[i]:offs[i + 1]][_missing_frames(spec, int(T[i]), np.random.default_rng([seed, i]) if drawn else None)] = True
            data = _lib.rouse_simulate(*arrs, self.measurement, T, seg_start, seg_state, mask, errs, seed=seed)
        else:               # replay mode: host groups of at most _REPLAY_GROUP_BYTES of normals
            per = T * (N + 1) * d
            data = np.empty((int(offs[-1]), d))
            i0 = 0
            while i0 < n:
                i1 = i0 + 1
                while i1 < n and per[i0:i1 + 1].sum() * 8 <= _REPLAY_GROUP_BYTES:
                    i1 += 1
                mask, z = _replay_draws(specs[i0:i1], T[i0:i1], N, d, rng)
                data[offs[i0]:offs[i1]] = _lib.rouse_simulate(*arrs, self.measurement, T[i0:i1], seg_start[i0:i1],
                                                              seg_state[i0:i1], mask, errs[i0:i1], normals=z)
                i0 = i1
        return [Trajectory(data[offs[i]:offs[i + 1]], localization_error=err.copy(), loopingprofile=items[i]) for i in range(n)]

    def _modal_arrays(self):
        """ per state, stacked: V, b, sqrt(sig), sqrt(cinf), V^T G, V^T M0 -- what bild_rouse_simulate takes """
        out = [[] for _ in range(6)]
        for m in self.models:
            V, b, sig, cinf = m.modal_dynamics()
            for lst, a in zip(out, (V, b, np.sqrt(np.maximum(sig, 0.)), np.sqrt(np.maximum(cinf, 0.)),
                                    V.T @ m._dynamics['G'], V.T @ m._dynamics['M0'])):
                lst.append(a)
        return [np.ascontiguousarray(np.stack(lst), dtype=np.float64) for lst in out]


class KalmanResult:
    """
    Per-frame moments of `MultiStateRouse.kalman` and `GenericGaussianModel.kalman` (which offers no ``filt_*``; its
    ``smooth_*`` are moments of the observed coordinate), each (n, T_max, d) float64 or None when not requested:
    ``terms`` (log-likelihood of each observation, 0.0 on missing frames), ``pred_mean`` / ``pred_var`` (the observation
    given the frames before), ``filt_mean`` / ``filt_var`` and ``smooth_mean`` / ``smooth_var`` (the noise-free y = w.x
    given the frames up to t / all frames), ``innov`` (standardised one-step-ahead innovations, NaN on missing frames).
    """
    GROUPS = {'terms': ('terms',), 'pred': ('pred_mean', 'pred_var'), 'filt': ('filt_mean', 'filt_var'),
              'smooth': ('smooth_mean', 'smooth_var'), 'innov': ('innov',)}

    def __init__(self, arrays):
        for name in _lib.KALMAN_OUTPUTS:
            setattr(self, name, arrays.get(name))

    def __repr__(self):
        have = [n for n in _lib.KALMAN_OUTPUTS if getattr(self, n) is not None]
        return f"KalmanResult({', '.join(have)})"


class FitResult:
    """
    `MultiStateRouse.fit`, `GenericGaussianModel.fit`: ``model`` (at the fitted parameters), ``params`` and ``se`` (dicts by name), ``cov`` (P x P, in
    the order of ``names``), ``logL`` (total at the optimum), ``n_iter`` (device calls), ``converged``, ``history``
    (accepted (params, logL) in order, the start first); ``prior_fit``: the `MarkovPriorFit` of the accepted evaluation where
    `GenericGaussianModel.fit_dwell` fitted a Markov prior along with the model, None for every other fit
    """

    def __init__(self, model, params, se, cov, logL, n_iter, converged, history, names, prior_fit=None):
        self.model, self.params, self.se, self.cov, self.logL = model, params, se, cov, logL
        self.n_iter, self.converged, self.history, self.names = n_iter, converged, history, tuple(names)
        self.prior_fit = prior_fit

    def __repr__(self):
        ps = ', '.join(f"{k}={v:.6g}+-{self.se[k]:.2g}" for k, v in self.params.items())
        return f"FitResult({ps}, logL={self.logL:.6f}, n_iter={self.n_iter}, converged={self.converged})"


def _log_chain_rule(grad, fisher, theta):
    """ derivatives with respect to theta -> with respect to log theta: grad * theta, fisher * theta_p theta_q (per row) """
    grad = grad * theta
    if fisher is not None:
        fisher = fisher * theta[:, :, None] * theta[:, None, :]
    return grad, fisher


def _newton_decrement(g, F):
    """ g^T F^-1 g / 2 (pseudo-inverse: a singular F is no error here) """
    return 0.5 * float(g @ np.linalg.pinv(F) @ g)


def _damped_step(g, F, mu):
    """ the Levenberg-damped Fisher-scoring step (F + mu diag(F)) delta = g """
    A = F + mu * np.diag(np.diag(F))
    return np.linalg.lstsq(A, g, rcond=None)[0]


def _fisher_scoring(evaluate, theta, params, tol, max_iter):
    """
    Fisher scoring in log theta with Levenberg damping, shared by the fits: ``evaluate(theta)`` -> (model, total logL,
    gradient and Fisher information with respect to log theta).  Stops when the Newton decrement falls below ``tol``, after
    ``max_iter`` evaluations, or when the damping exceeds 1e12; a step is accepted only if the logL rises.  -> `FitResult`
    with standard errors from the inverse Fisher information by the delta method.

    The acceptance rule -- the start, then a trial whose logL is finite and strictly larger than the current one -- is mirrored
    by `GenericGaussianModel.fit_dwell`'s ``evaluate``, which has to know which evaluation was accepted (its warm start and
    `FitResult.prior_fit`): change the two together.
    """
    model, L, g, F = evaluate(theta)
    history = [(dict(zip(params, theta)), L)]
    mu, n_iter, converged = 0.0, 1, False
    while True:
        dec = _newton_decrement(g, F)
        if dec < tol:
            converged = True
            break
        if n_iter >= max_iter:
            break
        step = _damped_step(g, F, mu)
        trial = theta * np.exp(step)
        tm, tL, tg, tF = evaluate(trial)
        n_iter += 1
        if np.isfinite(tL) and tL > L:
            theta, model, L, g, F = trial, tm, tL, tg, tF
            history.append((dict(zip(params, theta)), L))
            mu = 0.0 if mu <= 1e-3 else mu / 10.
        else:
            mu = 1e-3 if mu == 0.0 else mu * 10.
            if mu > 1e12:
                break
    cov_log = np.linalg.pinv(F)
    cov = cov_log * np.outer(theta, theta)
    se = np.sqrt(np.maximum(np.diag(cov), 0.))
    return FitResult(model=model, params=dict(zip(params, theta)), se=dict(zip(params, se)), cov=cov, logL=L,
                     n_iter=n_iter, converged=converged, history=history, names=params)


def _fit_profiles(profiles, lengths, n_states):
    """ `fit`'s profiles -> (seg_start, seg_state), one row per trajectory """
    n = len(lengths)
    if isinstance(profiles, (int, np.integer)):
        if not 0 <= profiles < n_states:
            raise ValueError(f"state {profiles} out of range ({n_states} states)")
        return (np.zeros((n, 1), dtype=np.int32), np.full((n, 1), int(profiles), dtype=np.int32))
    if isinstance(profiles, tuple) and len(profiles) == 2 and not isinstance(profiles[0], Loopingprofile) \
            and np.ndim(profiles[0]) == 2:
        seg_start = np.ascontiguousarray(profiles[0], dtype=np.int32)
        seg_state = np.ascontiguousarray(profiles[1], dtype=np.int32)
        if seg_start.shape != seg_state.shape or len(seg_start) != n:
            raise ValueError(f"(seg_start, seg_state) of shapes {seg_start.shape}, {seg_state.shape} for {n} trajectories")
        return seg_start, seg_state
    items = list(profiles)
    if len(items) != n:
        raise ValueError(f"{len(items)} profiles for {n} trajectories")
    states = [np.asarray(p[:]) for p in items]
    for i, (st, T) in enumerate(zip(states, lengths)):
        if st.ndim != 1 or len(st) != T or not np.issubdtype(st.dtype, np.integer):
            raise ValueError(f"profile {i} is not an integer array of the trajectory's {T} frames")
        if st.min() < 0 or st.max() >= n_states:
            raise ValueError(f"profile {i} has a state outside 0 .. {n_states - 1}")
    return _ragged_segments(states, np.array(lengths, dtype=np.int64))


# replay mode: host memory of the normals handed to the library in one call
_REPLAY_GROUP_BYTES = 256 << 20


def _localization_error(model, localization_error):
    """ the localization error a generator call uses (MultiStateRouse.trajectory_from_loopingprofile's rules) -> (d,) """
    if localization_error is None:
        if model.localization_error is None:
            raise ValueError("Need to specify either localization_error or model.localization_error")
        localization_error = model.localization_error
    if np.isscalar(localization_error):
        localization_error = model.d * [localization_error]
    localization_error = np.asarray(localization_error, dtype=np.float64)
    if localization_error.shape != (model.d,):
        raise ValueError("Did not understand localization_error")
    return localization_error


def _missing_is_none(spec):
    return spec is None or (np.isscalar(spec) and spec == 0)


def _missing_frames(spec, T, rng):
    """ the missing frames of one trajectory, drawn from ``rng`` as trajectory_from_loopingprofile draws them """
    if _missing_is_none(spec):
        return np.array([], dtype=int)
    if np.isscalar(spec):
        if 0 < spec < 1:
            return np.nonzero(rng.random(T) < spec)[0]
        return rng.choice(T, size=int(spec), replace=False).astype(int)
    return np.asarray(spec, dtype=int)


def _replay_draws(specs, T, N, d, rng):
    """
    What the loop of trajectory_from_loopingprofile draws from ``rng`` for trajectories of lengths T, in its order: per
    trajectory the missing frames, N d normals of the steady state, (T - 1) N d of the steps, T d of the localization
    noise.  -> (missing mask (sum T,) bool, normals (sum T (N + 1) d,)), as bild_rouse_simulate takes them
    """
    T = np.asarray(T, dtype=np.int64)
    return _draw_normals(specs, T, T * (N + 1) * d, rng)


def _draw_normals(specs, T, per, rng):
    """
    Per trajectory of length T[i]: its missing frames drawn from ``rng`` as the loops draw them, then one
    ``standard_normal`` fill of per[i] normals.  -> (missing mask (sum T,) bool, normals (sum per,)) in that order
    """
    T, per = np.asarray(T, dtype=np.int64), np.asarray(per, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(T)])
    mask = np.zeros(int(offs[-1]), dtype=bool)
    z = np.empty(int(per.sum()))
    zo = 0
    for i, spec in enumerate(specs):
        mask[offs[i]:offs[i + 1]][_missing_frames(spec, int(T[i]), rng)] = True
        rng.standard_normal(out=z[zo:zo + per[i]])
        zo += per[i]
    return mask, z


def _ragged_segments(states, T):
    """ profiles of lengths T -> run-length segments (n, K1) int32, padded with empty segments at T[i] """
    n = len(states)
    flat = np.concatenate(states)
    offs = np.concatenate([[0], np.cumsum(T)])
    change = np.ones(len(flat), dtype=bool)
    change[1:] = flat[1:] != flat[:-1]
    change[offs[:-1]] = True
    idx = np.flatnonzero(change)
    owner = np.searchsorted(offs, idx, side='right') - 1
    nseg = np.bincount(owner, minlength=n)
    K1 = int(nseg.max())
    rank = np.arange(len(idx)) - np.repeat(np.cumsum(nseg) - nseg, nseg)
    seg_start = np.repeat(np.asarray(T, dtype=np.int32)[:, None], K1, axis=1)
    seg_state = np.zeros((n, K1), dtype=np.int32)
    seg_start[owner, rank] = idx - offs[owner]
    seg_state[owner, rank] = flat[idx]
    return seg_start, seg_state


class FactorizedModel(MultiStateModel):
    """
    Time-scale-separated stand-in likelihood: every frame is drawn independently from the
    distance distribution of its state (reference bild/models.py:372-534).  Cheap, CPU only;
    the reference's own tests use it as the likelihood double for everything above the kernel,
    and so do this package's sampler tests.

    distributions : objects with ``logpdf(r)`` (e.g. ``scipy.stats.maxwell(scale=...)``)
    """

    def __init__(self, distributions, d=3):
        self.distributions = distributions
        self._d = d
        self._tables = {}
        self.init_transitions(len(distributions))

    @property
    def d(self):
        return self._d

    def clear_memo(self):
        self._tables = {}

    def _table(self, traj):
        key = id(traj)
        hit = self._tables.get(key)
        if hit is None or hit[0] is not traj:
            arr = as_array(traj)
            r = np.sqrt(np.sum(arr ** 2, axis=1))
            with np.errstate(divide='ignore', invalid='ignore'):
                table = np.array([dist.logpdf(r) for dist in self.distributions])  # (n, T), NaN on missing frames
            hit = (traj, table)
            self._tables[key] = hit
        return hit[1]

    def initial_loopingprofile(self, traj):
        """ per-frame maximum-likelihood state, missing frames filled from the next valid one """
        table = self._table(traj)
        valid = np.nonzero(~np.any(np.isnan(as_array(traj)), axis=1))[0]
        best = np.argmax(table[:, valid], axis=0)
        states = np.zeros(len(traj), dtype=int)
        states[:valid[0] + 1] = best[0]
        last = valid[0]
        for t, s in zip(valid[1:], best[1:]):
            states[last + 1:t + 1] = s
            last = t
        states[last + 1:] = best[-1]
        return Loopingprofile(states)

    def logL(self, profile, traj):
        table = self._table(traj)
        states = np.asarray(profile[:], dtype=int)
        return float(np.nansum(table[states, np.arange(len(states))]))

    def trajectory_from_loopingprofile(self, profile, localization_error=0., missing_frames=None):
        """
        Generative model (reference bild/models.py:487-534): a distance from the state's distribution and a
        uniformly random direction per frame.  The localization error is part of the distributions already: it is
        only recorded on the trajectory, not added.
        """
        if np.isscalar(localization_error):
            localization_error = self.d * [localization_error]
        localization_error = np.asarray(localization_error, dtype=np.float64)
        if localization_error.shape != (self.d,):
            raise ValueError("Did not understand localization_error")
        T = len(profile)
        if missing_frames is None or (np.isscalar(missing_frames) and missing_frames == 0):
            missing = np.array([], dtype=int)
        elif np.isscalar(missing_frames):
            if 0 < missing_frames < 1:
                missing = np.nonzero(np.random.rand(T) < missing_frames)[0]
            else:
                missing = np.random.choice(T, size=missing_frames, replace=False).astype(int)
        else:
            missing = np.asarray(missing_frames, dtype=int)
        magnitudes = np.array([self.distributions[state].rvs() for state in profile[:]])
        data = np.random.normal(size=(len(magnitudes), self.d))
        data *= np.expand_dims(magnitudes / np.linalg.norm(data, axis=1), 1)
        data[missing, :] = np.nan
        return Trajectory(data, localization_error=localization_error, loopingprofile=profile)

    def logL_batch(self, profiles, traj):
        table = self._table(traj)
        if not isinstance(profiles, np.ndarray):
            profiles = np.stack([np.asarray(p[:]) for p in profiles])
        return np.nansum(table[profiles, np.arange(profiles.shape[1])[None, :]], axis=1)
