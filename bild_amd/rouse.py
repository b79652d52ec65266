"""
Rouse-chain dynamics: the per-state matrices the Kalman-filter likelihood consumes.

The reference obtains these from the un-vendored third-party package ``rouse``
(``rouse.Model(N, D, k, d, add_bonds=loop)``, reference bild/models.py:246) and reads
``_dynamics['B'|'G'|'Sig']`` and ``steady_state()`` from it
(bild/src/MSRouse_logL.pyx:152-160). ``rouse`` is not available to this build, so this
module restates the standard discrete-time Rouse / Ornstein-Uhlenbeck physics from first
principles; it exposes the same duck-typed surface the reference kernels touch
(``check_dynamics``, ``_dynamics``, ``steady_state``, ``propagate_M``, ``propagate_C``,
``conf_ss``, ``evolve``), so a `Model` here can be handed to the reference's
``MSRouse_logL`` unchanged.  Parity with an installed ``rouse`` is *unpinned* (SURVEY.md
section 8c, "Level M"); the kernel-level parity contract is on identical array inputs.

Physics (one spatial dimension; all d dimensions are independent and identical):

    dx = -k A x dt + F dt + sqrt(2 D) dW

with ``A`` the connectivity (graph-Laplacian) matrix of the chain plus extra bonds.  With
the symmetric eigendecomposition ``k A = V diag(a) V^T`` the exact one-frame (dt = 1)
propagator is

    B   = V diag(exp(-a))                V^T
    Sig = V diag(D (1 - exp(-2a)) / a)   V^T      (a -> 0:  2 D)
    G   = V diag((1 - exp(-a)) / a)      V^T F    (a -> 0:  F)

and the steady state is ``M0 = (kA)^+ F``, ``C0 = D (kA)^+`` on the internal modes.  The
free centre-of-mass mode (a = 0) has no steady state; **convention of this build**: it is
pinned (variance 0, mean 0), i.e. the Moore-Penrose pseudo-inverse is used.  For any
measurement vector with ``sum(w) == 0`` (the reference default, end-to-end) the likelihood
does not depend on that choice, because the uniform vector is a common null vector of
every state's Laplacian.
"""
import numpy as np

# relative threshold under which an eigenvalue of k*A counts as a zero (free) mode
_ZERO_MODE_RTOL = 1e-12


class Model:
    """
    One Rouse model (one looping state).

    Parameters mirror ``rouse.Model(N, D, k, d, add_bonds=...)`` as called at reference
    bild/models.py:246.

    Parameters
    ----------
    N : int
        number of monomers
    D, k : float
        monomer diffusion constant and backbone spring constant
    d : int
        spatial dimension
    add_bonds : list of (i, j[, rel_strength]) or None
        extra harmonic bonds of strength ``rel_strength * k`` between monomers ``i`` and
        ``j`` (negative indices count from the end, as in reference bild/models.py:223).
    """

    def __init__(self, N, D=1., k=1., d=3, add_bonds=None):
        self.N = int(N)
        self.D = float(D)
        self.k = float(k)
        self.d = int(d)

        A = 2. * np.eye(self.N) - np.eye(self.N, k=1) - np.eye(self.N, k=-1)
        A[0, 0] = A[-1, -1] = 1.
        if self.N == 1:
            A[:] = 0.
        self.A = A
        self.F = np.zeros((self.N, self.d))

        if add_bonds is not None:
            for bond in add_bonds:
                self.add_bond(*bond)

        self._dynamics = {'needs_updating': True}

    def add_bond(self, i, j, rel_strength=1.):
        i = int(i) % self.N
        j = int(j) % self.N
        if i != j:
            self.A[i, i] += rel_strength
            self.A[j, j] += rel_strength
            self.A[i, j] -= rel_strength
            self.A[j, i] -= rel_strength
        self._dynamics = {'needs_updating': True}

    # ------------------------------------------------------------------ dynamics
    def update_dynamics(self):
        a, V = np.linalg.eigh(self.k * self.A)
        scale = max(np.max(np.abs(a)), 1e-300)
        if np.any(a < -_ZERO_MODE_RTOL * scale * self.N):
            raise ValueError("connectivity matrix has a negative mode: dynamics are unstable")
        zero = np.abs(a) <= _ZERO_MODE_RTOL * scale * self.N
        a_safe = np.where(zero, 1., a)

        b = np.where(zero, 1., np.exp(-a_safe))
        g = np.where(zero, 1., -np.expm1(-a_safe) / a_safe)
        sig = np.where(zero, 2. * self.D, -self.D * np.expm1(-2. * a_safe) / a_safe)
        cinf = np.where(zero, 0., self.D / a_safe)
        minf = np.where(zero, 0., 1. / a_safe)

        def sym(diag):
            X = (V * diag) @ V.T
            return 0.5 * (X + X.T)

        # the eigenbasis itself, for the modal generator (modal_dynamics); kept out of _dynamics, which callers read by key
        self._modal = (V, b, sig, cinf)
        self._dynamics = {
            'needs_updating': False,
            'N': self.N, 'D': self.D, 'k': self.k, 'd': self.d,
            'B': np.ascontiguousarray(sym(b)),
            'G': np.ascontiguousarray(sym(g) @ self.F),
            'Sig': np.ascontiguousarray(sym(sig)),
            'M0': np.ascontiguousarray(sym(minf) @ self.F),
            'C0': np.ascontiguousarray(sym(cinf)),
            # square root of Sig / C0 for sampling
            'LSig': V * np.sqrt(np.maximum(sig, 0.)),
            'LC0': V * np.sqrt(np.maximum(cinf, 0.)),
        }

    def dynamics_derivatives(self, param):
        """
        Derivatives of the dynamics with respect to ``param`` ('D' or 'k'): a dict with dB, dG, dSig (N, N) and dM0 (N, d),
        dC0 (N, N), in the layout of ``_dynamics`` and ``steady_state()``.  With a = k alpha per mode (alpha an eigenvalue
        of A) the eigenvectors do not depend on D or k, so every derivative is diagonal in the same basis:

            b = exp(-a)             db/dk = -alpha b                                        db/dD = 0
            sig = -D expm1(-2a)/a   dsig/dk = (D/k) (2 exp(-2a) + expm1(-2a)/a)              dsig/dD = sig/D
            cinf = D/a              dcinf/dk = -cinf/k                                       dcinf/dD = 1/a
            g = -expm1(-a)/a        dg/dk = (a/k) (exp(-a) (1 + a) - 1)/a^2                   dg/dD = 0
            minf = 1/a              dminf/dk = -minf/k                                       dminf/dD = 0

        and the pinned zero mode (sig = 2D, cinf = 0, b = g = 1, minf = 0) has dsig/dD = 2 and nothing else.  The brackets
        that cancel for small a are summed as series there.
        """
        if param not in ('D', 'k'):
            raise ValueError(f"unknown parameter {param!r}; choose 'D' or 'k'")
        a, V = np.linalg.eigh(self.k * self.A)
        scale = max(np.max(np.abs(a)), 1e-300)
        zero = np.abs(a) <= _ZERO_MODE_RTOL * scale * self.N
        a = np.where(zero, 1., a)
        if param == 'D':
            db = np.zeros_like(a)
            dsig = np.where(zero, 2., -np.expm1(-2. * a) / a)
            dcinf = np.where(zero, 0., 1. / a)
            dg = np.zeros_like(a)
            dminf = np.zeros_like(a)
        else:
            k, D = self.k, self.D
            db = np.where(zero, 0., -(a / k) * np.exp(-a))
            # 2 exp(-u) + 2 expm1(-u)/u at u = 2a; and h(a) = exp(-a) (1 + a) - 1
            dsig = np.where(zero, 0., (D / k) * _two_exp_plus(2. * a))
            dcinf = np.where(zero, 0., -(D / a) / k)
            dg = np.where(zero, 0., _h_over_a(a) / k)
            dminf = np.where(zero, 0., -(1. / a) / k)

        def sym(diag):
            X = (V * diag) @ V.T
            return np.ascontiguousarray(0.5 * (X + X.T))

        return {'dB': sym(db), 'dG': np.ascontiguousarray(sym(dg) @ self.F), 'dSig': sym(dsig),
                'dM0': np.ascontiguousarray(sym(dminf) @ self.F), 'dC0': sym(dcinf)}

    def check_dynamics(self, run_if_necessary=True):
        if self._dynamics['needs_updating']:
            if not run_if_necessary:
                raise RuntimeError("Model changed since last call to update_dynamics()")
            self.update_dynamics()

    def modal_dynamics(self):
        """
        -> (V (N, N), b (N,), sig (N,), cinf (N,)): the orthonormal eigenbasis (columns = modes) in which the dynamics are
        diagonal, ``B = V diag(b) V^T``, ``LSig = V diag(sqrt(sig))``, ``LC0 = V diag(sqrt(cinf))``
        """
        self.check_dynamics()
        if getattr(self, '_modal', None) is None:     # a model pickled before the basis was kept
            self.update_dynamics()
        return tuple(a.copy() for a in self._modal)

    def steady_state(self):
        """ -> (M (N, d), C (N, N)) ; reference call sites pyx:160, models.py:366 """
        self.check_dynamics()
        return self._dynamics['M0'].copy(), self._dynamics['C0'].copy()

    # reference call sites: bild/src/MSRouse_logL_py.py:109-110
    def propagate_M(self, M, check_dynamics=True):
        if check_dynamics:
            self.check_dynamics()
        return self._dynamics['B'] @ M + self._dynamics['G']

    def propagate_C(self, C, check_dynamics=True):
        if check_dynamics:
            self.check_dynamics()
        B = self._dynamics['B']
        return B @ C @ B + self._dynamics['Sig']

    # reference call sites: bild/models.py:332,337 (generative model)
    def conf_ss(self, rng=None):
        self.check_dynamics()
        rng = np.random.default_rng() if rng is None else rng
        return self._dynamics['M0'] + self._dynamics['LC0'] @ rng.standard_normal((self.N, self.d))

    def evolve(self, conf, rng=None):
        self.check_dynamics()
        rng = np.random.default_rng() if rng is None else rng
        return (self._dynamics['B'] @ conf + self._dynamics['G']
                + self._dynamics['LSig'] @ rng.standard_normal((self.N, self.d)))


def _two_exp_plus(u):
    """ 2 exp(-u) + 2 expm1(-u)/u = (2/u) (exp(-u) (1 + u) - 1), without the cancellation at small u """
    u = np.asarray(u, dtype=np.float64)
    out = np.empty_like(u)
    small = u < 0.5
    us = np.where(small, u, 1.)
    out[~small] = 2. * np.exp(-u[~small]) + 2. * np.expm1(-u[~small]) / u[~small]
    out[small] = 2. * _h_series(us[small]) / us[small]
    return out


def _h_over_a(a):
    """ a (exp(-a) (1 + a) - 1) / a^2 = (exp(-a) (1 + a) - 1) / a, without the cancellation at small a """
    a = np.asarray(a, dtype=np.float64)
    out = np.empty_like(a)
    small = a < 0.5
    out[~small] = (np.exp(-a[~small]) * (1. + a[~small]) - 1.) / a[~small]
    out[small] = _h_series(a[small]) / a[small]
    return out


def _h_series(u):
    """ exp(-u) (1 + u) - 1 = sum_{m >= 2} (-1)^m (1 - m) u^m / m!  for u < 0.5 (terms to m = 24: below 1e-17 relative) """
    total = np.zeros_like(u)
    term = np.ones_like(u)     # u^m / m!
    for m in range(1, 25):
        term = term * u / m
        if m >= 2:
            total = total + (-1) ** m * (1 - m) * term
    return total


def stack_dynamics(models):
    """
    Stack the per-state arrays the likelihood path consumes
    (reference bild/src/MSRouse_logL.pyx:152-160).

    Returns
    -------
    dict with B (S,N,N), G (S,N,d), Sig (S,N,N), M0 (S,N,d), C0 (S,N,N), all C-contiguous f64
    """
    for m in models:
        m.check_dynamics()
    out = {}
    for key in ('B', 'G', 'Sig', 'M0', 'C0'):
        out[key] = np.ascontiguousarray(np.stack([m._dynamics[key] for m in models]), dtype=np.float64)
    return out
