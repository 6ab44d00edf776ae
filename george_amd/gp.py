"""The ``GP`` facade: owns kernel / mean / white-noise models and a solver class.

Same public surface and semantics as the reference's ``src/george/gp.py``
(``GP`` :22-635) -- ``compute, recompute, log_likelihood, grad_log_likelihood,
nll, grad_nll, predict, apply_inverse, sample, sample_conditional, get_matrix``
plus the deprecated ``lnlikelihood`` aliases -- so user code ports by changing
the import.  Differences are behind the API:

* the default solver is the HIP :class:`george_amd.BasicSolver`;
* ``predict`` and ``grad_log_likelihood`` use the solver's fused device-resident
  entry points when it has them -- ``BasicSolver`` (``gh_chol_predict`` /
  ``gh_chol_grad``) and ``HODLRSolver`` (``gh_hodlr_predict`` / ``gh_hodlr_grad``,
  column strips on the factor) both do: the N x M cross-covariance, K^-1 and the
  (N, N, P) gradient tensor of gp.py:532-541 / :436-466 never reach the host;
  any other duck-typed solver (the multi-device HODLR split among them) takes the
  generic NumPy path below, formula for formula as the reference.
"""
import contextlib
import warnings

import numpy as np

from . import kernels
from .modeling import ModelSet, ConstantModel
from .solvers import TrivialSolver, BasicSolver
from .utils import multivariate_gaussian_samples, pivoted_cholesky

__all__ = ["GP"]

TINY = 1.25e-12          # default white-noise variance (gp.py:19)


def _as_model(obj):
    try:
        return ConstantModel(float(obj))
    except TypeError:
        return obj


def _is_number(obj):
    try:
        float(obj)
    except TypeError:
        return False
    return True


class GP(ModelSet):

    def __init__(self, kernel=None, fit_kernel=True, mean=None, fit_mean=None,
                 white_noise=None, fit_white_noise=None, solver=None, **kwargs):
        self._computed = False
        self._alpha = None
        self._y = None
        super(GP, self).__init__([
            ("mean", ConstantModel(0.0) if mean is None else _as_model(mean)),
            ("white_noise", ConstantModel(np.log(TINY)) if white_noise is None else _as_model(white_noise)),
            ("kernel", kernels.EmptyKernel() if kernel is None else kernel),
        ])
        # a plain number for mean / white_noise is held fixed unless asked otherwise (gp.py:96-122)
        if _is_number(mean) and fit_mean is None:
            fit_mean = False
        if _is_number(white_noise) and fit_white_noise is None:
            fit_white_noise = False
        if not fit_kernel:
            self.models["kernel"].freeze_all_parameters()
        if mean is None or (fit_mean is not None and not fit_mean):
            self.models["mean"].freeze_all_parameters()
        if white_noise is None or (fit_white_noise is not None and not fit_white_noise):
            self.models["white_noise"].freeze_all_parameters()

        if solver is None:
            empty = kernel is None or kernel.kernel_type == kernels.EmptyKernel.kernel_type
            solver = TrivialSolver if empty else BasicSolver
        self.solver_type = solver
        self.solver_kwargs = kwargs
        self.solver = None

    # -- sub-model helpers ----------------------------------------------------
    @property
    def mean(self):
        return self.models["mean"]

    @property
    def white_noise(self):
        return self.models["white_noise"]

    @staticmethod
    def _model_arg(x):
        return x[:, 0] if (x.ndim == 2 and x.shape[1] == 1) else x

    def _call_mean(self, x):
        mu = self.mean.get_value(self._model_arg(x)).flatten()
        if not np.all(np.isfinite(mu)):
            raise ValueError("mean function returned NaN or Inf for parameters:\n{0}".format(
                self.mean.get_parameter_dict(include_frozen=True)))
        return mu

    def _call_mean_gradient(self, x):
        g = self.mean.get_gradient(self._model_arg(x))
        if np.any(np.isnan(g)) or np.any(np.isinf(g)):
            raise ValueError("mean gradient function returned NaN or Inf for parameters:\n{0}".format(
                self.mean.get_parameter_dict(include_frozen=True)))
        return g

    def _call_white_noise(self, x):
        return self.white_noise.get_value(self._model_arg(x)).flatten()

    def _call_white_noise_gradient(self, x):
        return self.white_noise.get_gradient(self._model_arg(x))

    # -- state ------------------------------------------------------------------
    @property
    def computed(self):
        return (self._computed and self.solver.computed
                and (self.kernel is None or not self.kernel.dirty))

    @computed.setter
    def computed(self, v):
        self._computed = v
        if v and self.kernel is not None:
            self.kernel.dirty = False

    def _offers(self, name, on_type=False):
        """Does the solver (``on_type``: the solver class, before an instance is made) define the optional call ``name``?
        An optional capability is a callable attribute; a class that does not define it takes the generic branch."""
        return callable(getattr(self.solver_type if on_type else self.solver, name, None))

    def parse_samples(self, t):
        t = np.atleast_1d(t)
        if t.ndim == 1:
            t = np.atleast_2d(t).T
        if t.ndim != 2 or (self.kernel is not None and t.shape[1] != self.kernel.ndim):
            raise ValueError("Dimension mismatch")
        return t

    def _check_dimensions(self, y, check_dim=True):
        y = np.atleast_1d(y)
        if check_dim and y.ndim > 1:
            raise ValueError("The predicted dimension must be 1-D")
        if len(y) != self._x.shape[0]:
            raise ValueError("Dimension mismatch")
        return y

    def _residual(self, y):
        return np.ascontiguousarray(self._check_dimensions(y) - self._call_mean(self._x), dtype=np.float64)

    def _residual_quiet(self, y, quiet):
        """Residual for the likelihood entry points: a wrongly shaped ``y`` ALWAYS raises; only a failing
        mean function is silenced by ``quiet`` (gp.py:383-392).  Returns None when silenced."""
        yv = self._check_dimensions(y)
        try:
            mu = self._call_mean(self._x)
        except ValueError:
            if quiet:
                return None
            raise
        return np.ascontiguousarray(yv - mu, dtype=np.float64)

    def _recomputed_residual(self, y, quiet):
        """:meth:`recompute`, then :meth:`_residual_quiet`: the residual on a computed model, or None where ``quiet`` silenced
        a matrix that does not factor or a failing mean function."""
        if not self.recompute(quiet=quiet):
            return None
        return self._residual_quiet(y, quiet)

    def _compute_alpha(self, y, cache):
        if not cache:
            return self.solver.apply_inverse(self._residual(y), in_place=True).flatten()
        if self._alpha is None or not np.array_equiv(y, self._y):
            self._y = y
            self._alpha = self.solver.apply_inverse(self._residual(y), in_place=True).flatten()
        return self._alpha

    # -- the hot path -------------------------------------------------------------
    def compute(self, x, yerr=0.0, **kwargs):
        """Build and factorise K(x, x) + diag(yerr^2 + exp(white_noise))  (gp.py:303-337)."""
        self._obj_cache = None           # a gradient cached by the fused objective belongs to the OLD (x, yerr)
        self._x = np.ascontiguousarray(self.parse_samples(x), dtype=np.float64)
        # scalar yerr broadcasts over the points, anything else must have one entry per point
        if np.ndim(yerr) == 0 or (np.size(yerr) == 1 and len(self._x) != 1):
            sig = np.full(len(self._x), float(np.reshape(yerr, ())))
        else:
            sig = self._check_dimensions(yerr)
        self._yerr2 = np.ascontiguousarray(sig ** 2, dtype=np.float64)
        self._factorize(**kwargs)

    def _factorize(self, **kwargs):
        """A fresh solver computed on the recorded ``_x`` / ``_yerr2``."""
        self.solver = self.solver_type(self.kernel, **(self.solver_kwargs))
        sigma = np.sqrt(self._yerr2 + np.exp(self._call_white_noise(self._x)))
        self.solver.compute(self._x, sigma, **kwargs)

        self._const = -0.5 * (len(self._x) * np.log(2 * np.pi) + self.solver.log_determinant)
        self.computed = True
        self._alpha = None

    # -- sequential use: the data set gains or loses trailing points ---------------
    # (no reference counterpart: gp.py:303-337 always rebuilds)
    def _refactorize_or_restore(self, x, yerr2, **kwargs):
        """``compute`` on already parsed inputs; whatever it raises leaves the GP as it was."""
        keep = (self._x, self._yerr2, self.solver, self._computed, getattr(self, "_const", None), self._alpha,
                getattr(self, "_obj_cache", None))
        self._obj_cache = None
        self._x, self._yerr2 = x, yerr2
        try:
            self._factorize(**kwargs)
        except Exception:
            self._x, self._yerr2, self.solver, self._computed, self._const, self._alpha, self._obj_cache = keep
            raise

    def append(self, x, yerr=0.0, **kwargs):
        """Add the points ``x`` (error bars ``yerr``, a scalar or one per new point) behind the ones of the last ``compute``.
        With a computed GP and a solver that offers ``append`` (the HIP :class:`BasicSolver`) the factor is extended in
        place -- one pass over it and a small Schur block instead of a factorisation; white noise is evaluated at the new
        points only.  Otherwise (not computed yet, parameters changed since, any other solver) the concatenated inputs are
        computed afresh.  ``y`` of later calls has the new length.  On ``LinAlgError`` the GP is unchanged."""
        xn = np.ascontiguousarray(self.parse_samples(x), dtype=np.float64)
        m = len(xn)
        if np.ndim(yerr) == 0 or (np.size(yerr) == 1 and m != 1):
            sig = np.full(m, float(np.reshape(yerr, ())))
        else:
            sig = np.atleast_1d(np.asarray(yerr, dtype=np.float64))
            if sig.ndim > 1 or len(sig) != m:
                raise ValueError("Dimension mismatch")
        if not (hasattr(self, "_x") and hasattr(self, "_yerr2")):
            return self.compute(xn, sig, **kwargs)
        if xn.shape[1] != self._x.shape[1]:
            raise ValueError("Dimension mismatch")
        if m == 0:
            return
        x_all = np.ascontiguousarray(np.concatenate([self._x, xn]))
        yerr2_all = np.ascontiguousarray(np.concatenate([self._yerr2, sig ** 2]))
        if not (self.computed and self._offers("append") and getattr(self.solver, "appendable", True)):
            return self._refactorize_or_restore(x_all, yerr2_all, **kwargs)
        sigma_new = np.sqrt(sig ** 2 + np.exp(self._call_white_noise(xn)))
        self.solver.append(xn, sigma_new)                # (raises with the solver as it was)
        self._obj_cache = None
        self._x, self._yerr2 = x_all, yerr2_all
        self._const = -0.5 * (len(self._x) * np.log(2 * np.pi) + self.solver.log_determinant)
        self._alpha = None

    def truncate(self, n, **kwargs):
        """Keep the first ``n`` points of the last ``compute`` / ``append`` (``0 < n <= len(x)``): undoes a tentative
        ``append``.  Data movement on the device with the HIP :class:`BasicSolver`, a fresh ``compute`` otherwise."""
        if not (hasattr(self, "_x") and hasattr(self, "_yerr2")):
            raise RuntimeError("You need to compute the model first")
        n = int(n)
        if not 0 < n <= len(self._x):
            raise ValueError("truncate: n must be in 1 .. {0}".format(len(self._x)))
        if n == len(self._x):
            return
        x_cut, yerr2_cut = np.ascontiguousarray(self._x[:n]), np.ascontiguousarray(self._yerr2[:n])
        if not (self.computed and self._offers("truncate")):
            return self._refactorize_or_restore(x_cut, yerr2_cut, **kwargs)
        self.solver.truncate(n)
        self._obj_cache = None
        self._x, self._yerr2 = x_cut, yerr2_cut
        self._const = -0.5 * (len(self._x) * np.log(2 * np.pi) + self.solver.log_determinant)
        self._alpha = None

    def remove(self, indices, **kwargs):
        """Take points out of the data set of the last ``compute`` / ``append``, anywhere in it.  ``indices`` means what it
        means to ``np.delete(np.arange(n), indices)``: integers (negative ones count from the end), a slice or a boolean
        mask -- ``gp.remove(slice(0, m))`` is a sliding window.  With a computed GP and a solver that offers ``remove`` (the HIP
        :class:`BasicSolver`) the factor is updated on the device (a rank-m Cholesky update, no kernel evaluations);
        otherwise (parameters changed since, any other solver, a solver that cannot) the kept inputs are computed afresh.
        Removing nothing does nothing; removing every point is a ``ValueError``; an index out of range an ``IndexError``.
        ``y`` of later calls has the new length.  On any exception the GP is unchanged."""
        if not (hasattr(self, "_x") and hasattr(self, "_yerr2")):
            raise RuntimeError("You need to compute the model first")
        n = len(self._x)
        if isinstance(indices, slice):
            rem = np.arange(n, dtype=np.int64)[indices]
        else:
            idx = np.asarray(indices)
            if idx.dtype == bool:
                if idx.shape != (n,):
                    raise IndexError("remove: a boolean mask must have one entry per point ({0})".format(n))
                rem = np.flatnonzero(idx)
            else:
                idx = np.atleast_1d(idx)
                if idx.size == 0:
                    rem = np.empty(0, dtype=np.int64)
                elif idx.ndim != 1 or idx.dtype.kind not in "iu":
                    raise IndexError("remove: indices must be integers, a slice or a boolean mask")
                else:
                    idx = idx.astype(np.int64)
                    if idx.min() < -n or idx.max() >= n:
                        raise IndexError("remove: index out of range for {0} points".format(n))
                    rem = np.where(idx < 0, idx + n, idx)
        rem = np.unique(rem).astype(np.int64)
        if len(rem) == 0:
            return
        if len(rem) == n:
            raise ValueError("remove: every point would be removed")
        keep = np.ones(n, dtype=bool)
        keep[rem] = False
        x_keep, yerr2_keep = np.ascontiguousarray(self._x[keep]), np.ascontiguousarray(self._yerr2[keep])
        if self.computed and self._offers("remove"):
            try:
                self.solver.remove(rem)                   # (raises with the solver as it was)
            except RuntimeError:
                return self._refactorize_or_restore(x_keep, yerr2_keep, **kwargs)
            self._obj_cache = None
            self._x, self._yerr2 = x_keep, yerr2_keep
            self._const = -0.5 * (len(self._x) * np.log(2 * np.pi) + self.solver.log_determinant)
            self._alpha = None
            return
        return self._refactorize_or_restore(x_keep, yerr2_keep, **kwargs)

    def recompute(self, quiet=False, **kwargs):
        if not self.computed:
            if not (hasattr(self, "_x") and hasattr(self, "_yerr2")):
                raise RuntimeError("You need to compute the model first")
            try:
                self.compute(self._x, np.sqrt(self._yerr2), **kwargs)
            except (ValueError, np.linalg.LinAlgError):
                if quiet:
                    return False
                raise
        return True

    def log_likelihood(self, y, quiet=False):
        """-1/2 r^T K^-1 r - 1/2 log|K| - N/2 log 2 pi   (gp.py:369-397)."""
        r = self._recomputed_residual(y, quiet)
        if r is None:
            return -np.inf
        ll = self._const - 0.5 * self.solver.dot_solve(r)
        return ll if np.isfinite(ll) else -np.inf

    def grad_log_likelihood(self, y, quiet=False):
        """Gradient wrt the unfrozen parameters, ordered mean | white_noise | kernel (gp.py:406-468)."""
        r = self._recomputed_residual(y, quiet)
        if r is None:
            return np.zeros(len(self), dtype=np.float64)

        n_wn, n_k = len(self.white_noise), len(self.kernel)
        fused = self._offers("grad")
        kgrad = diagA = None
        if fused and (n_wn or n_k):
            # alpha, diag(A) and 1/2 sum A_ij dK_ij/dtheta in one device-resident call
            which = self.kernel.unfrozen_mask.astype(np.uint32)
            kg_full, alpha, diagA = self.solver.grad(r, which)
            kgrad = kg_full[self.kernel.unfrozen_mask]
        else:
            alpha = self.solver.apply_inverse(r, in_place=True).flatten()
            if n_wn or n_k:
                A = np.einsum("i,j", alpha, alpha) - self.solver.get_inverse()
                diagA = np.diag(A)
                if n_k:
                    kgrad = 0.5 * np.einsum("ijk,ij", self.kernel.get_gradient(self._x), A)
        return self._assemble_grad(alpha, diagA, kgrad, quiet)

    def _assemble_grad(self, alpha, diagA, kgrad, quiet, diag_weight=0.5):
        """mean | white_noise | kernel blocks of the gradient from alpha, diag(alpha alpha^T - K^-1) and
        the kernel block (gp.py:443-466).  The cross-validation gradients have the same layout from ``v`` and ``diag(B)``
        (:meth:`_loo_parts`) with ``diag_weight=1.0``."""
        n_wn, n_k = len(self.white_noise), len(self.kernel)
        grad = np.empty(len(self))
        at = 0
        n_m = len(self.mean)
        if n_m:
            try:
                mg = self._call_mean_gradient(self._x)
            except ValueError:
                if quiet:
                    return np.zeros(len(self), dtype=np.float64)
                raise
            grad[at:at + n_m] = np.dot(mg, alpha)
            at += n_m
        if n_wn:
            wn = self._call_white_noise(self._x)
            wng = self._call_white_noise_gradient(self._x)
            grad[at:at + n_wn] = diag_weight * np.sum((np.exp(wn) * diagA)[None, :] * wng, axis=1)
            at += n_wn
        if n_k:
            grad[at:at + n_k] = kgrad
        return grad

    # -- the optimiser objective (gp.py:470-480; docs/tutorials/hyper.rst:131-152) ----------------
    # ``minimize(gp.nll, p0, jac=gp.grad_nll, args=(y,))`` asks for the value and then the gradient at
    # every iterate.  With a solver that offers ``objective`` (the HIP BasicSolver) each iterate is ONE
    # fused device call -- build, factor, one forward solve shared by r^T K^-1 r and alpha, K^-1,
    # gradient reduction, one synchronisation -- instead of compute + dot_solve + grad with the matrix
    # factored twice (the reference marks the model dirty again when grad_nll re-sets the same vector):
    # once a gradient has been asked for, ``nll`` computes it eagerly and ``grad_nll`` at the same
    # (vector, y) returns it.  ``nll_and_grad`` is the explicit one-call form (``jac=True``).
    def set_parameter_vector(self, vector, include_frozen=False):
        if self._computed and self.solver is not None and not self.kernel.dirty:
            v = np.asarray(vector, dtype=np.float64)
            cur = self.get_parameter_vector(include_frozen=include_frozen)
            if v.shape == cur.shape and np.array_equal(v, cur):
                return                                  # same point: keep the factorisation
        super(GP, self).set_parameter_vector(vector, include_frozen=include_frozen)

    def _fused_capable(self):
        return (self._offers("objective", on_type=True)
                and hasattr(self, "_x") and hasattr(self, "_yerr2"))

    def _objective(self, y, want_grad, quiet):
        """(log-likelihood, gradient | None) at the current parameters through the solver's fused entry
        point; (-inf, zeros) where the reference's quiet mode returns them."""
        bad = (-np.inf, np.zeros(len(self)) if want_grad else None)
        r = self._residual_quiet(y, quiet)
        if r is None:
            return bad
        n_wn, n_k = len(self.white_noise), len(self.kernel)
        need_A = want_grad and (n_wn or n_k)
        self.solver = self.solver_type(self.kernel, **(self.solver_kwargs))
        sigma = np.sqrt(self._yerr2 + np.exp(self._call_white_noise(self._x)))
        which = self.kernel.unfrozen_mask.astype(np.uint32)
        try:
            if need_A:
                logdet, quad, kg_full, alpha, diagA = self.solver.objective(self._x, sigma, r, which, want_grad=True)
            else:
                logdet, quad, kg_full, alpha, diagA = self.solver.objective(self._x, sigma, r, which, want_grad=False)
        except (ValueError, np.linalg.LinAlgError):
            if quiet:
                return bad
            raise
        self._const = -0.5 * (len(self._x) * np.log(2 * np.pi) + logdet)
        self.computed = True
        self._alpha = None
        ll = self._const - 0.5 * quad
        ll = ll if np.isfinite(ll) else -np.inf
        if not want_grad:
            return ll, None
        if not need_A:                                   # only mean parameters vary: alpha is all that is needed
            alpha = self.solver.apply_inverse(r).flatten()
            return ll, self._assemble_grad(alpha, None, None, quiet)
        kgrad = kg_full[self.kernel.unfrozen_mask] if n_k else None
        return ll, self._assemble_grad(alpha, diagA, kgrad, quiet)

    def nll_and_grad(self, vector, y, quiet=True):
        """``(nll(vector, y), grad_nll(vector, y))`` from one fused device call."""
        self.set_parameter_vector(vector)
        if not np.isfinite(self.log_prior()):
            return np.inf, np.zeros(len(vector))
        if self.computed or not self._fused_capable():
            return -self.log_likelihood(y, quiet=quiet), -self.grad_log_likelihood(y, quiet=quiet)
        ll, g = self._objective(y, True, quiet)
        self._obj_cache = (np.array(vector, dtype=np.float64), np.array(y, dtype=np.float64), g)
        return -ll, -g

    # -- the inducing inputs of a sparse solver as parameters (no reference counterpart) ------------
    # With ``InducingSolver(variational=True)`` the objective is Titsias' lower bound of the exact log-likelihood
    # (``log_determinant`` carries its trace term), so maximising it over the hyper-parameters and the inducing inputs jointly
    # does not over-fit; under DTC and FITC the same calls work, and over-fit.
    def _need_inducing(self):
        if not self._offers("grad_inducing", on_type=True):
            raise NotImplementedError("{0} has no inducing inputs to differentiate (no grad_inducing)".format(self.solver_type.__name__))

    @property
    def inducing_inputs(self):
        """The (m, ndim) inducing inputs the solver used in its last ``compute``."""
        self._need_inducing()
        self.recompute()
        return np.array(self.solver.u)

    def grad_log_likelihood_inducing(self, y, quiet=False):
        """The gradient of :meth:`log_likelihood` with respect to the inducing inputs, (m, ndim).  The relative jitter follows
        ``mean_j k(u_j, u_j)``, which the gradient treats as a constant: exact for stationary kernels only."""
        self._need_inducing()
        r = self._recomputed_residual(y, quiet)
        if r is None:
            return np.zeros(np.shape(self.solver.u), dtype=np.float64)
        return self.solver.grad_inducing(r)[3]

    def nll_and_grad_inducing(self, vector, y, quiet=True):
        """``(-F, -dF)`` at ``vector`` = the parameter vector followed by ``u.ravel()``, for
        ``scipy.optimize.minimize(gp.nll_and_grad_inducing, v0, jac=True, args=(y,))``: sets the parameters, puts ``u`` into
        ``solver_kwargs["inducing"]``, and makes one ``compute``, one ``dot_solve`` and one ``grad_inducing``.  The model must
        have been computed once (the data are the recorded ones).  ``quiet`` as in :meth:`nll_and_grad`.  The relative jitter
        follows ``mean_j k(u_j, u_j)``, constant in ``u`` for stationary kernels only: for others the gradient is that of the
        objective at a fixed absolute jitter."""
        self._need_inducing()
        if not (hasattr(self, "_x") and hasattr(self, "_yerr2")):
            raise RuntimeError("You need to compute the model first")
        vector = np.asarray(vector, dtype=np.float64)
        npar, ndim = len(self), self._x.shape[1]
        if vector.ndim != 1 or len(vector) <= npar or (len(vector) - npar) % ndim:
            raise ValueError("vector is the parameter vector followed by u.ravel()")
        bad = (np.inf, np.zeros(len(vector)))
        self.set_parameter_vector(vector[:npar])
        if not np.isfinite(self.log_prior()):
            return bad
        self.solver_kwargs["inducing"] = np.array(vector[npar:].reshape(-1, ndim))
        self._obj_cache = None
        self._computed = False
        try:
            self._factorize()
        except (ValueError, np.linalg.LinAlgError):
            if quiet:
                return bad
            raise
        r = self._residual_quiet(y, quiet)
        if r is None:
            return bad
        ll = self._const - 0.5 * self.solver.dot_solve(r)
        kg_full, alpha, diagA, ugrad = self.solver.grad_inducing(r, self.kernel.unfrozen_mask.astype(np.uint32))
        kgrad = kg_full[self.kernel.unfrozen_mask] if len(self.kernel) else None
        g = np.concatenate([self._assemble_grad(alpha, diagA, kgrad, quiet), ugrad.ravel()])
        return (-ll, -g) if np.isfinite(ll) else bad

    def _cached_grad(self, vector, y):
        c = getattr(self, "_obj_cache", None)
        if c is None or not self.computed:
            return None
        v, yy = np.asarray(vector, dtype=np.float64), np.asarray(y, dtype=np.float64)
        if v.shape == c[0].shape and yy.shape == c[1].shape and np.array_equal(v, c[0]) and np.array_equal(yy, c[1]):
            return c[2]
        return None

    def nll(self, vector, y, quiet=True):
        self.set_parameter_vector(vector)
        if not np.isfinite(self.log_prior()):
            return np.inf
        if self.computed or not self._fused_capable():
            return -self.log_likelihood(y, quiet=quiet)
        # eager gradient only while the caller keeps asking for it: two value-only evaluations in a
        # row (a gradient-free optimiser, MCMC) switch it off again
        self._nll_since_grad = getattr(self, "_nll_since_grad", 0) + 1
        if self._nll_since_grad > 2:
            self._grad_seen = False
        want_grad = getattr(self, "_grad_seen", False)
        ll, g = self._objective(y, want_grad, quiet)
        self._obj_cache = (np.array(vector, dtype=np.float64), np.array(y, dtype=np.float64), g) if want_grad else None
        return -ll

    def grad_nll(self, vector, y, quiet=True):
        self._grad_seen = True
        self._nll_since_grad = 0
        self.set_parameter_vector(vector)
        if not np.isfinite(self.log_prior()):
            return np.zeros(len(vector))
        g = self._cached_grad(vector, y)
        if g is not None:
            return -g
        if self.computed or not self._fused_capable():
            return -self.grad_log_likelihood(y, quiet=quiet)
        ll, g = self._objective(y, True, quiet)
        self._obj_cache = (np.array(vector, dtype=np.float64), np.array(y, dtype=np.float64), g)
        return -g

    # -- leave-one-out cross-validation (no reference counterpart; GPML section 5.4.2) ---------------
    # With alpha = K^-1 r and c_i = (K^-1)_ii the prediction of y_i from all OTHER points is mu_i = y_i - alpha_i / c_i with
    # variance 1 / c_i, and L = sum_i log p(y_i | y_-i) = sum_i 1/2 log c_i - 1/2 alpha_i^2 / c_i - 1/2 log 2 pi.  Its gradient
    # is sum_ij B_ij dK_ij/dtheta with B = 1/2 (v alpha^T + alpha v^T) - K^-1 diag(w) K^-1, u = alpha / c, v = K^-1 u,
    # w = 1/2 (1 + alpha^2 / c) / c: one N^3 product for any number of parameters.  A solver that offers
    # ``loo`` (the HIP BasicSolver) keeps all of it on the device; one that offers ``loo_blocks`` instead (VecchiaSolver) sums
    # one closed form per block -- the leave-one-out of ITS density, with Q in the place of K^-1 and nothing N x N; one that
    # offers ``loo_lowrank`` (InducingSolver) does the same for the DTC / FITC density from C^-1 = D - R^T R in strips, with the
    # gradient through dC, not dK; any other one with ``apply_inverse`` and ``get_inverse`` takes the NumPy branch, formula
    # for formula (its kernel gradient is exact only where the solver inverts K(x, x) + diag itself).
    def _loo_parts(self, r, want_grad):
        """``(L, resid, var, lpd, kgrad | None, v | None, diagB | None)`` for the residual ``r`` on the computed solver;
        ``kgrad`` over the unfrozen kernel parameters."""
        n_k = len(self.kernel)
        device = next((name for name in ("loo", "loo_blocks", "loo_lowrank") if self._offers(name)), None)
        if device is not None:
            which = self.kernel.unfrozen_mask.astype(np.uint32) if want_grad else None
            L, resid, var, lpd, kg_full, v, diagB = getattr(self.solver, device)(r, which)
            kgrad = kg_full[self.kernel.unfrozen_mask] if (want_grad and n_k) else None
            return L, resid, var, lpd, kgrad, v, diagB
        # (vectorised, not _lgo_parts' loop over N one-point groups: that costs N Python iterations and other low bits)
        alpha = np.asarray(self.solver.apply_inverse(np.array(r, dtype=np.float64))).flatten()
        Kinv = np.asarray(self.solver.get_inverse())
        c = np.array(np.diag(Kinv), dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            resid = alpha / c
            var = 1.0 / c
            lpd = 0.5 * np.log(c) - 0.5 * alpha * resid - 0.5 * np.log(2 * np.pi)
            L = float(np.sum(lpd))
            if not want_grad:
                return L, resid, var, lpd, None, None, None
            w = 0.5 * (1.0 + alpha * resid) / c
            v = np.asarray(self.solver.apply_inverse(np.array(resid, dtype=np.float64))).flatten()
            B = 0.5 * (np.einsum("i,j", v, alpha) + np.einsum("i,j", alpha, v)) - np.dot(Kinv * w[None, :], Kinv)
        kgrad = np.einsum("ijk,ij", self.kernel.get_gradient(self._x), B) if n_k else None
        return L, resid, var, lpd, kgrad, v, np.array(np.diag(B))

    def _neg_cv(self, L, kgrad, v, diagB, quiet):
        """What ``loo_nll_and_grad`` and ``lgo_nll_and_grad`` return for the value ``L`` and the parts of its gradient."""
        if not np.isfinite(L):
            return np.inf, np.zeros(len(self))
        return -L, -self._assemble_grad(v, diagB, kgrad, quiet, diag_weight=1.0)

    def loo_predict(self, y, return_var=True):
        """Leave-one-out predictions: ``mu[i]`` (and ``var[i]``) of ``y[i]`` from all other points, mean model included, without
        N refits.  ``(y - mu) / sqrt(var)`` are the standardised leave-one-out residuals."""
        self.recompute()
        y = self._check_dimensions(y)
        _, resid, var, _, _, _, _ = self._loo_parts(self._residual(y), False)
        mu = np.asarray(y, dtype=np.float64) - resid
        return (mu, var) if return_var else mu

    def loo_log_likelihood(self, y, quiet=False, pointwise=False):
        """The log pseudo-likelihood ``sum_i log p(y_i | y_-i)`` (GPML eq. 5.11), or its N terms with ``pointwise=True``."""
        bad = np.full(len(np.atleast_1d(y)), -np.inf) if pointwise else -np.inf
        r = self._recomputed_residual(y, quiet)
        if r is None:
            return bad
        L, _, _, lpd, _, _, _ = self._loo_parts(r, False)
        if not np.isfinite(L):
            return bad
        return lpd if pointwise else L

    def grad_loo_log_likelihood(self, y, quiet=False):
        """Gradient of :meth:`loo_log_likelihood` wrt the unfrozen parameters, ordered mean | white_noise | kernel."""
        r = self._recomputed_residual(y, quiet)
        if r is None:
            return np.zeros(len(self), dtype=np.float64)
        _, _, _, _, kgrad, v, diagB = self._loo_parts(r, True)
        return self._assemble_grad(v, diagB, kgrad, quiet, diag_weight=1.0)

    def loo_nll_and_grad(self, vector, y, quiet=True):
        """``(-loo_log_likelihood, -grad_loo_log_likelihood)`` at ``vector`` for ``scipy.optimize.minimize(..., jac=True)``:
        one fused device call per iterate (build, factor, leave-one-out value and gradient) with a solver that offers
        ``loo_objective``; ``(inf, zeros)`` outside the prior."""
        self.set_parameter_vector(vector)
        if not np.isfinite(self.log_prior()):
            return np.inf, np.zeros(len(vector))
        bad = (np.inf, np.zeros(len(self)))
        fused = (self._offers("loo_objective", on_type=True)
                 and hasattr(self, "_x") and hasattr(self, "_yerr2"))
        if self.computed or not fused:
            r = self._recomputed_residual(y, quiet)
            if r is None:
                return bad
            L, _, _, _, kgrad, v, diagB = self._loo_parts(r, True)
        else:
            r = self._residual_quiet(y, quiet)
            if r is None:
                return bad
            self._obj_cache = None
            self.solver = self.solver_type(self.kernel, **(self.solver_kwargs))
            sigma = np.sqrt(self._yerr2 + np.exp(self._call_white_noise(self._x)))
            which = self.kernel.unfrozen_mask.astype(np.uint32)
            try:
                logdet, L, _, _, kg_full, v, diagB = self.solver.loo_objective(self._x, sigma, r, which, want_grad=True)
            except (ValueError, np.linalg.LinAlgError):
                if quiet:
                    return bad
                raise
            self._const = -0.5 * (len(self._x) * np.log(2 * np.pi) + logdet)
            self.computed = True
            self._alpha = None
            kgrad = kg_full[self.kernel.unfrozen_mask] if len(self.kernel) else None
        return self._neg_cv(L, kgrad, v, diagB, quiet)

    # -- leave-group-out cross-validation (no reference counterpart) -------------------------------
    # The groups I_1 .. I_G partition the points; with C = K^-1, alpha = C r and C_gg the block of C on group g the joint
    # prediction of the group from all OTHER groups has residual u_g = C_gg^-1 alpha_g and covariance C_gg^-1, and
    # L = sum_g 1/2 log|C_gg| - 1/2 alpha_g^T u_g - m_g/2 log 2 pi.  Its gradient is sum_ij B_ij dK_ij/dtheta with
    # B = 1/2 (v alpha^T + alpha v^T) - C W C, v = C u, W = blockdiag_g 1/2 (C_gg^-1 + u_g u_g^T): leave-one-out is the case of
    # one-point groups.  A solver that offers ``lgo`` (the HIP BasicSolver) keeps all of it on the
    # device for groups of up to ``LGO_MAX_GROUP`` points; any other one, or a larger group, takes the NumPy branch on
    # ``apply_inverse`` and ``get_inverse``, formula for formula.
    def _lgo_groups(self, groups):
        """``(order, start)`` of a ``groups`` argument: an (n,) integer array of labels -- any integers, groups numbered by
        sorted unique label -- or a positive int b, windows of b consecutive points.  ``order`` lists the points sorted by
        group (within a group as they appear in the data), ``start`` the G + 1 offsets of the groups in it."""
        if not hasattr(self, "_x"):
            raise RuntimeError("You need to compute the model first")
        n = len(self._x)
        if isinstance(groups, (int, np.integer)) and not isinstance(groups, (bool, np.bool_)):
            if groups < 1:
                raise ValueError("a window must have at least one point")
            labels = np.arange(n) // int(groups)
        else:
            labels = np.asarray(groups)
            if labels.dtype.kind not in "iu":
                raise ValueError("groups must be an int or an array of integer labels")
            if labels.shape != (n,):
                raise ValueError("groups must have one label per point: shape ({0},)".format(n))
        order = np.argsort(labels, kind="stable").astype(np.int64)
        _, counts = np.unique(labels, return_counts=True)
        start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return order, start

    def _lgo_parts(self, r, order, start, want_grad, want_cov=False):
        """``(L, resid, var, lpd, cov_blocks | None, kgrad | None, v | None, diagB | None)`` for the residual ``r`` on the
        computed solver; ``kgrad`` over the unfrozen kernel parameters."""
        n_k = len(self.kernel)
        G = len(start) - 1
        device = self._offers("lgo")
        if device and np.max(np.diff(start)) <= getattr(self.solver, "LGO_MAX_GROUP", 0):
            which = self.kernel.unfrozen_mask.astype(np.uint32) if want_grad else None
            L, resid, var, lpd, cov, kg_full, v, diagB = self.solver.lgo(r, order, start, which, want_cov)
            kgrad = kg_full[self.kernel.unfrozen_mask] if (want_grad and n_k) else None
            return L, resid, var, lpd, cov, kgrad, v, diagB
        alpha = np.asarray(self.solver.apply_inverse(np.array(r, dtype=np.float64))).flatten()
        Kinv = np.asarray(self.solver.get_inverse())
        n = len(alpha)
        resid, var, lpd = np.empty(n), np.empty(n), np.empty(G)
        covs = []
        with np.errstate(divide="ignore", invalid="ignore"):
            for g in range(G):
                I = order[start[g]:start[g + 1]]
                Cgg = Kinv[np.ix_(I, I)]
                try:
                    R = np.linalg.cholesky(0.5 * (Cgg + Cgg.T))
                    Ri = np.linalg.inv(R)
                except np.linalg.LinAlgError:               # (not positive definite, or not finite: the terms come out NaN)
                    R = Ri = np.full(Cgg.shape, np.nan)
                cov = np.dot(Ri.T, Ri)
                resid[I] = np.dot(cov, alpha[I])
                var[I] = np.diag(cov)
                lpd[g] = np.sum(np.log(np.diag(R))) - 0.5 * np.dot(alpha[I], resid[I]) - 0.5 * len(I) * np.log(2 * np.pi)
                covs.append(cov)
            L = float(np.sum(lpd))
            if not want_grad:
                return L, resid, var, lpd, (covs if want_cov else None), None, None, None
            v = np.asarray(self.solver.apply_inverse(np.array(resid, dtype=np.float64))).flatten()
            M = np.zeros((n, n))
            for g in range(G):
                I = order[start[g]:start[g + 1]]
                W = 0.5 * (covs[g] + np.einsum("i,j", resid[I], resid[I]))
                M += np.dot(np.dot(Kinv[:, I], W), Kinv[I, :])
            B = 0.5 * (np.einsum("i,j", v, alpha) + np.einsum("i,j", alpha, v)) - M
        kgrad = np.einsum("ijk,ij", self.kernel.get_gradient(self._x), B) if n_k else None
        return L, resid, var, lpd, (covs if want_cov else None), kgrad, v, np.array(np.diag(B))

    def lgo_predict(self, y, groups, return_var=True, return_cov=False):
        """Leave-group-out predictions: ``mu[i]`` (and ``var[i]``) of ``y[i]`` from all points OUTSIDE its group, mean model
        and white noise included, without G refits.  ``groups``: an (n,) integer array of labels or a positive int b (windows
        of b consecutive points).  With ``return_cov`` also the list of the G joint predictive covariances, groups in the
        order of their sorted labels, rows in the order the group's points appear in the data."""
        order, start = self._lgo_groups(groups)
        self.recompute()
        y = self._check_dimensions(y)
        _, resid, var, _, cov, _, _, _ = self._lgo_parts(self._residual(y), order, start, False, return_cov)
        out = (np.asarray(y, dtype=np.float64) - resid,)
        if return_var:
            out += (var,)
        if return_cov:
            out += (cov,)
        return out if len(out) > 1 else out[0]

    def lgo_log_likelihood(self, y, groups, quiet=False, pointwise=False):
        """The leave-group-out log pseudo-likelihood ``sum_g log p(y_g | y_-g)``, or its G terms with ``pointwise=True``."""
        order, start = self._lgo_groups(groups)
        bad = np.full(len(start) - 1, -np.inf) if pointwise else -np.inf
        r = self._recomputed_residual(y, quiet)
        if r is None:
            return bad
        L, _, _, lpd, _, _, _, _ = self._lgo_parts(r, order, start, False)
        if not np.isfinite(L):
            return bad
        return lpd if pointwise else L

    def grad_lgo_log_likelihood(self, y, groups, quiet=False):
        """Gradient of :meth:`lgo_log_likelihood` wrt the unfrozen parameters, ordered mean | white_noise | kernel."""
        order, start = self._lgo_groups(groups)
        r = self._recomputed_residual(y, quiet)
        if r is None:
            return np.zeros(len(self), dtype=np.float64)
        _, _, _, _, _, kgrad, v, diagB = self._lgo_parts(r, order, start, True)
        return self._assemble_grad(v, diagB, kgrad, quiet, diag_weight=1.0)

    def lgo_nll_and_grad(self, vector, y, groups, quiet=True):
        """``(-lgo_log_likelihood, -grad_lgo_log_likelihood)`` at ``vector`` for ``scipy.optimize.minimize(..., jac=True)``:
        ``set_parameter_vector``, ``recompute`` and one leave-group-out call per iterate; ``(inf, zeros)`` outside the prior or
        on a matrix that is not positive definite."""
        order, start = self._lgo_groups(groups)
        self.set_parameter_vector(vector)
        if not np.isfinite(self.log_prior()):
            return np.inf, np.zeros(len(vector))
        bad = (np.inf, np.zeros(len(self)))
        r = self._recomputed_residual(y, quiet)
        if r is None:
            return bad
        try:
            L, _, _, _, _, kgrad, v, diagB = self._lgo_parts(r, order, start, True)
        except np.linalg.LinAlgError:
            if quiet:
                return bad
            raise
        return self._neg_cv(L, kgrad, v, diagB, quiet)

    # -- expected information of the hyper-parameters ---------------------------------------------
    # (no reference counterpart.)  For the Gaussian likelihood the expected (Fisher) information is
    #   F_ab = 1/2 tr(K^-1 dK/dtheta_a K^-1 dK/dtheta_b)      white-noise and kernel parameters
    #   F_mn = (d mean / d m)^T K^-1 (d mean / d n)           mean parameters; their cross block with the others is exactly 0
    # It needs no y and is positive semidefinite by construction.  A solver that offers ``fisher`` (the HIP BasicSolver) computes the
    # white-noise and kernel block on the device, keeping the derivative matrices and every N^3 product there; one that offers
    # ``fisher_blocks`` instead (VecchiaSolver) sums one closed form per block -- the information of ITS likelihood, with Q in
    # the place of K^-1 in the mean block, and no N x N array anywhere.  Any other solver with ``get_inverse`` takes the NumPy branch, formula for formula.
    def fisher_information(self):
        """The expected (Fisher) information of the unfrozen parameters at their current values, ``(len(gp), len(gp))``,
        ordered mean | white_noise | kernel like :meth:`grad_log_likelihood`.  It does not depend on ``y``.  Its inverse is
        :meth:`parameter_covariance`; small eigenvalues are directions the data cannot separate.  With ``VecchiaSolver`` it is
        the information of the Vecchia likelihood (the dense one when every predecessor is a neighbour), at about the cost of one
        ``nll_and_grad`` for any N.  For a kernel with a general
        (full-matrix) metric the parameter derivatives are the reference's, not the derivatives of the value (DESIGN.md
        section 9, "Known discrepancy"), and the information inherits that; isotropic and axis-aligned metrics are right."""
        self.recompute()
        n_m, n_wn, n_k = len(self.mean), len(self.white_noise), len(self.kernel)
        F = np.zeros((len(self), len(self)))
        if n_m:
            mg = np.ascontiguousarray(np.atleast_2d(self._call_mean_gradient(self._x)), dtype=np.float64)
            Fm = np.dot(mg, np.asarray(self.solver.apply_inverse(np.array(mg.T, dtype=np.float64, order="C"))))
            F[:n_m, :n_m] = 0.5 * (Fm + Fm.T)
        if not (n_wn or n_k):
            return F
        rows = None
        if n_wn:
            wn = self._call_white_noise(self._x)
            wng = np.atleast_2d(self._call_white_noise_gradient(self._x))
            rows = np.ascontiguousarray(np.exp(wn)[None, :] * wng, dtype=np.float64)
        device = next((name for name in ("fisher", "fisher_blocks") if self._offers(name)), None)
        if device is not None:
            mask = self.kernel.unfrozen_mask
            full = getattr(self.solver, device)(mask.astype(np.uint32), rows)
            keep = np.concatenate([np.arange(n_wn), n_wn + np.flatnonzero(mask)]).astype(int)
            F[n_m:, n_m:] = full[np.ix_(keep, keep)]
            return F
        Kinv = np.asarray(self.solver.get_inverse())
        M = [Kinv * rows[p][None, :] for p in range(n_wn)]
        if n_k:
            G = self.kernel.get_gradient(self._x)
            M += [np.dot(Kinv, G[:, :, p]) for p in range(n_k)]
        M = np.stack(M)
        Fk = 0.5 * np.einsum("aij,bji->ab", M, M)
        F[n_m:, n_m:] = 0.5 * (Fk + Fk.T)
        return F

    def parameter_covariance(self):
        """The inverse of :meth:`fisher_information`: the Cramer-Rao bound on the covariance of any unbiased estimate of the
        unfrozen parameters, evaluated AT THE CURRENT parameters -- the asymptotic covariance of a maximum-likelihood fit
        when they are its optimum.  It is not a posterior: no prior enters and nothing is integrated over.  Computed by a
        Cholesky factor of the information scaled to unit diagonal; ``numpy.linalg.LinAlgError`` when it is singular -- a
        parameter the data cannot identify: a zero diagonal entry, or a pivot of the scaled matrix at or below
        ``len(gp) * eps**0.75``, which is below the accuracy the information itself is computed with."""
        F = self.fisher_information()
        if not len(F):
            return F
        d = np.sqrt(np.diag(F))
        if not np.all(np.isfinite(F)) or np.any(d <= 0.0):
            raise np.linalg.LinAlgError("the information matrix is singular: a parameter with no information")
        L = np.linalg.cholesky(F / np.outer(d, d))
        if np.min(np.diag(L)) ** 2 <= len(F) * np.finfo(np.float64).eps ** 0.75:
            raise np.linalg.LinAlgError("the information matrix is singular to working precision")
        Li = np.linalg.solve(L, np.eye(len(F)))
        C = np.dot(Li.T, Li) / np.outer(d, d)
        return 0.5 * (C + C.T)

    # -- ensembles (emcee ``vectorize=True``) ------------------------------------------------------
    def log_likelihood_batch(self, vectors, y, quiet=True):
        """``log_likelihood(y, quiet)`` at each row of ``vectors`` (shape ``(B, len(gp))``, ``get_parameter_vector()``
        order), as an array of shape ``(B,)``.  Uses the ``x`` and ``yerr`` of the last ``compute``.  With the HIP
        :class:`BasicSolver` and ``N <= BasicSolver.BATCH_MAX_N`` the B members are factorised together, every launch of
        one factorisation carrying all of them (gh_chol_objective_batch); otherwise -- larger N, other solvers -- the rows
        go through ``set_parameter_vector`` + ``log_likelihood`` one by one, with the same results.  A failed member is
        ``-inf`` with ``quiet=True``; with ``quiet=False`` the first one raises ``np.linalg.LinAlgError`` naming it.  The
        GP's parameter vector, ``computed`` flag and factorisation are what they were before the call."""
        vectors, y = self._batch_args(vectors, y)
        if len(vectors) == 0:
            return np.empty(0)
        if self._batch_on_device():
            return self._log_likelihood_batch_device(vectors, y, quiet)
        return self._log_likelihood_batch_loop(vectors, y, quiet)

    def _batch_args(self, vectors, y):
        """The checked ``(vectors (B, len(gp)), y)`` of every batched method."""
        if not (hasattr(self, "_x") and hasattr(self, "_yerr2")):
            raise RuntimeError("you must call 'compute' first")
        vectors = np.asarray(vectors, dtype=np.float64)
        if vectors.ndim != 2 or vectors.shape[1] != len(self):
            raise ValueError("vectors must have shape (B, {0})".format(len(self)))
        return vectors, np.asarray(self._check_dimensions(y), dtype=np.float64)

    def _batch_on_device(self, member_bytes=None):
        """Do the batched methods take the device path: the HIP BasicSolver itself, ``N <= BATCH_MAX_N`` and, where the
        caller gives one member's device bytes, those within ``BATCH_MAX_BYTES``?"""
        return (self.solver_type is BasicSolver and len(self._x) <= BasicSolver.BATCH_MAX_N
                and (member_bytes is None or member_bytes <= BasicSolver.BATCH_MAX_BYTES))

    def _each_member(self, members, fn, catch, vectors=None, quiet=False):
        """The per-member loop: under :meth:`_state_kept`, for each b of ``members``, ``set_parameter_vector(vectors[b])``
        (when ``vectors`` is given) and ``fn(b)``.  An exception of ``catch`` is raised again, as its own type, with the
        member named in front of its message or, ``quiet``, skipped."""
        with self._state_kept():
            for b in members:
                if vectors is not None:
                    self.set_parameter_vector(vectors[b])
                try:
                    fn(b)
                except catch as e:
                    if not quiet:
                        raise type(e)("member {0}: {1}".format(b, e))

    @staticmethod
    def _raise_not_positive_definite(info, names=None):
        """Raises ``LinAlgError`` for the first member whose ``info`` is set (named ``names[b]`` when given)."""
        bad = np.flatnonzero(info != 0)
        if len(bad):
            b = int(bad[0])
            raise np.linalg.LinAlgError("member {0}: {1}-th leading minor of the array is not positive definite".format(
                b if names is None else int(names[b]), int(info[b])))

    def _batch_blocks(self, vectors):
        """{model name: its FULL parameter rows (B, full size)} for rows in ``get_parameter_vector()`` order."""
        blocks, at = {}, 0
        for name in ("mean", "white_noise", "kernel"):
            m = self.models[name]
            full = np.tile(m.get_parameter_vector(include_frozen=True), (len(vectors), 1))
            k = int(m.unfrozen_mask.sum())
            full[:, m.unfrozen_mask] = vectors[:, at:at + k]
            blocks[name] = full
            at += k
        return blocks

    def _batch_values(self, name, rows, arg):
        """(B, len(arg)): model ``name``'s ``get_value(arg)`` at each of its full parameter rows.  A ConstantModel is mapped
        column-wise; any other model is set row by row and restored."""
        m = self.models[name]
        B = len(rows)
        if type(m) is ConstantModel:
            return rows[:, :1] + np.zeros((B, len(arg)))              # ConstantModel.get_value, row by row
        out = np.empty((B, len(arg)))
        for b, v in enumerate(self._per_member(m, rows, lambda: m.get_value(arg))):
            out[b] = v.flatten()
        return out

    def _batch_gradients(self, name, rows, arg):
        """[model ``name``'s ``get_gradient(arg)`` at row b for b in range(B)].  A ConstantModel's gradient does not depend on
        its value: it is evaluated once."""
        m = self.models[name]
        if type(m) is ConstantModel:
            return [m.get_gradient(arg)] * len(rows)
        return self._per_member(m, rows, lambda: m.get_gradient(arg))

    @staticmethod
    def _per_member(m, rows, fn):
        saved, was_dirty = m.get_parameter_vector(include_frozen=True), m.dirty
        out = []
        try:
            for row in rows:
                m.set_parameter_vector(row, include_frozen=True)
                out.append(fn())
        finally:
            m.set_parameter_vector(saved, include_frozen=True)
            m.dirty = was_dirty
        return out

    def _batch_inputs(self, vectors, y, quiet, t=None):
        """Per-member (full kernel parameter rows (B, kernel.full_size), sigma (B, N), r (B, N), ok (B,)) for rows in
        ``get_parameter_vector()`` order: exactly what ``set_parameter_vector(v)`` followed by ``compute`` / ``_residual``
        forms, without touching the GP's state.  Constant mean and white-noise models are mapped column-wise; any other
        model goes through its own ``set_parameter_vector`` / ``get_value`` per member (and is restored).  With test
        points ``t`` ((M, ndim), parsed) the tuple has a fifth entry, the mean model at ``t`` (B, M), and ``ok`` also
        requires that one to be finite."""
        B, n = len(vectors), len(self._x)
        blocks = self._batch_blocks(vectors)

        def values(name, arg):
            return self._batch_values(name, blocks[name], arg)

        def check(mu, where):
            ok = np.all(np.isfinite(mu), axis=1)                       # (_call_mean raises where this is False)
            if not quiet and not ok.all():
                b = int(np.argmin(ok))
                raise ValueError("member {0}: mean function returned NaN or Inf{1} for parameters:\n{2}".format(
                    b, where, blocks["mean"][b]))
            return ok

        mu = values("mean", self._model_arg(self._x))
        ok = check(mu, "")
        with np.errstate(invalid="ignore", over="ignore"):
            sigma = np.sqrt(self._yerr2[None, :] + np.exp(values("white_noise", self._model_arg(self._x))))
        r = np.ascontiguousarray(y[None, :] - mu)
        if t is None:
            return blocks["kernel"], sigma, r, ok
        mu_t = values("mean", self._model_arg(t))
        ok = ok & check(mu_t, " at the test points")
        return blocks["kernel"], sigma, r, ok, mu_t

    def _log_likelihood_batch_device(self, vectors, y, quiet):
        kp, sigma, r, ok = self._batch_inputs(vectors, y, quiet)
        solver = BasicSolver(self.kernel, **(self.solver_kwargs))      # (its own pooled handle: self.solver is untouched)
        logdet, quad, info = solver.objective_batch(kp, self._x, sigma, r)
        if not quiet:
            self._raise_not_positive_definite(info)
        with np.errstate(invalid="ignore"):
            const = -0.5 * (len(self._x) * np.log(2 * np.pi) + logdet)
            ll = const - 0.5 * quad
        ll[~(ok & (info == 0) & np.isfinite(ll))] = -np.inf
        return ll

    @contextlib.contextmanager
    def _state_kept(self):
        """Restores, on exit, what a per-member loop of ``set_parameter_vector`` + ``compute`` changes: the parameter
        vector, the models' dirty flags, the solver and its factor, the ``computed`` flag, the alpha cache and the
        objective cache."""
        saved = dict(vector=self.get_parameter_vector(include_frozen=True), solver=self.solver,
                     computed=self._computed, dirty=[m.dirty for m in self.models.values()],
                     const=getattr(self, "_const", None), alpha=self._alpha, y=self._y,
                     obj_cache=getattr(self, "_obj_cache", None))
        try:
            yield
        finally:
            ModelSet.set_parameter_vector(self, saved["vector"], include_frozen=True)
            for m, d in zip(self.models.values(), saved["dirty"]):
                m.dirty = d
            self.solver, self._computed = saved["solver"], saved["computed"]
            self._const, self._alpha, self._y = saved["const"], saved["alpha"], saved["y"]
            self._obj_cache = saved["obj_cache"]

    def _log_likelihood_batch_loop(self, vectors, y, quiet):
        out = np.empty(len(vectors))

        def one(b):
            out[b] = self.log_likelihood(y, quiet=quiet)

        self._each_member(range(len(vectors)), one, np.linalg.LinAlgError, vectors)
        return out

    def predict_batch(self, vectors, y, t, return_cov=True, return_var=False, quiet=False):
        """``predict(y, t, return_cov, return_var)`` at each row of ``vectors`` (shape ``(B, len(gp))``,
        ``get_parameter_vector()`` order), stacked: ``mu`` (B, M), and ``var`` (B, M) or ``cov`` (B, M, M) as ``predict``
        returns them (``return_var`` wins).  Row b includes member b's mean model at ``t``.  Uses the ``x`` and ``yerr``
        of the last ``compute``.  With the HIP :class:`BasicSolver`, ``N <= BasicSolver.BATCH_MAX_N`` and one member's
        device buffers within ``BasicSolver.BATCH_MAX_BYTES`` the B members are factorised and predicted together
        (gh_chol_predict_batch); otherwise the rows go through ``set_parameter_vector`` + ``predict`` one by one, with the
        same results.  A member whose matrix is not positive definite, or whose mean model is not finite at ``x`` or
        ``t``, raises (``np.linalg.LinAlgError`` / ``ValueError`` naming it) unless ``quiet``, which gives it NaN rows.
        The GP's parameter vector, ``computed`` flag, factorisation and caches are what they were before the call."""
        vectors, y = self._batch_args(vectors, y)
        xs = np.ascontiguousarray(self.parse_samples(t), dtype=np.float64)
        want_var = bool(return_var)
        want_cov = bool(return_cov) and not want_var
        if self._batch_on_device(BasicSolver.predict_batch_bytes(len(self._x), len(xs), want_var, want_cov)):
            mu, var, cov = self._predict_batch_device(vectors, y, xs, want_var, want_cov, quiet)
        else:
            mu, var, cov = self._predict_batch_loop(vectors, y, xs, want_var, want_cov, quiet)
        if want_var:
            return mu, var
        if want_cov:
            return mu, cov
        return mu

    def _predict_batch_device(self, vectors, y, xs, want_var, want_cov, quiet):
        B, m = len(vectors), len(xs)
        if B == 0:
            return np.empty((0, m)), np.empty((0, m)) if want_var else None, np.empty((0, m, m)) if want_cov else None
        kp, sigma, r, ok, mean_t = self._batch_inputs(vectors, y, quiet, t=xs)
        solver = BasicSolver(self.kernel, **(self.solver_kwargs))      # (its own pooled handle: self.solver is untouched)
        mu, var, cov, info = solver.predict_batch(kp, self._x, sigma, r, xs, return_var=want_var, return_cov=want_cov)
        if not quiet:
            self._raise_not_positive_definite(info)
        mu += mean_t
        failed = ~(ok & (info == 0))
        for a in (mu, var, cov):
            if a is not None:
                a[failed] = np.nan
        return mu, var, cov

    def _predict_batch_loop(self, vectors, y, xs, want_var, want_cov, quiet):
        B, m = len(vectors), len(xs)
        mu = np.full((B, m), np.nan)
        var = np.full((B, m), np.nan) if want_var else None
        cov = np.full((B, m, m), np.nan) if want_cov else None

        def one(b):
            out = self.predict(y, xs, return_cov=want_cov, return_var=want_var)
            if want_var:
                mu[b], var[b] = out
            elif want_cov:
                mu[b], cov[b] = out
            else:
                mu[b] = out

        self._each_member(range(B), one, ValueError, vectors, quiet)   # (np.linalg.LinAlgError is a ValueError)
        return mu, var, cov

    def sample_conditional_batch(self, vectors, y, t, size=1, quiet=False, factor="svd"):
        """``sample_conditional(y, t, size)`` at each row of ``vectors``: ``predict_batch(..., return_cov=True)`` and then,
        for b = 0, 1, ... in order, ``multivariate_gaussian_samples(cov_b, size, mean=mu_b)`` -- the random stream is
        consumed as the loop of ``set_parameter_vector`` + ``sample_conditional`` consumes it.  The draws are made on the
        host (SVD, as the reference).  Returns (B, M) for ``size == 1``, else (B, size, M).  A member that failed under
        ``quiet=True`` has NaN draws and consumes no random numbers.

        ``factor="cholesky"``: the covariances are factored by the pivoted Cholesky of :meth:`sample_conditional` -- with the
        HIP :class:`BasicSolver`, under ``predict_batch``'s routing rule (``N <= BATCH_MAX_N``, one member's device bytes
        within ``BATCH_MAX_BYTES``), all B members in one device call (gh_chol_sample_conditional_batch), the covariances
        never leaving the device.  The random-number rule differs from the SVD path's: ONE call
        ``np.random.standard_normal((B, size, M))`` is made before anything else, member b uses block b, and a failed
        member's numbers are drawn and discarded (its rows are NaN under ``quiet=True``)."""
        self._check_factor(factor)
        if factor == "cholesky":
            return self._sample_conditional_batch_cholesky(vectors, y, t, size, quiet)
        mu, cov = self.predict_batch(vectors, y, t, return_cov=True, quiet=quiet)
        B, m = mu.shape
        out = np.full((B, m) if size == 1 else (B, size, m), np.nan)
        for b in range(B):
            if np.all(np.isfinite(mu[b])):
                out[b] = multivariate_gaussian_samples(cov[b], size, mean=mu[b])
        return out

    def _sample_conditional_batch_cholesky(self, vectors, y, t, size, quiet):
        vectors, y = self._batch_args(vectors, y)
        xs = np.ascontiguousarray(self.parse_samples(t), dtype=np.float64)
        B, m = len(vectors), len(xs)
        z = np.random.standard_normal((B, size, m))
        if B == 0:
            return np.empty((0, m) if size == 1 else (0, size, m))
        if self._batch_on_device(BasicSolver.sample_batch_bytes(len(self._x), m, size)):
            kp, sigma, r, ok, mean_t = self._batch_inputs(vectors, y, quiet, t=xs)
            solver = BasicSolver(self.kernel, **(self.solver_kwargs))  # (its own pooled handle: self.solver is untouched)
            out, _, _, info = solver.sample_conditional_batch(kp, self._x, sigma, r, xs, z)
            if not quiet:
                self._raise_not_positive_definite(info)
            out += mean_t[:, None, :]
            out[~(ok & (info == 0))] = np.nan
        else:
            out = np.full((B, size, m), np.nan)

            def one(b):
                out[b] = self._sample_conditional_cholesky(y, xs, z[b])

            self._each_member(range(B), one, ValueError, vectors, quiet)   # (np.linalg.LinAlgError is a ValueError)
        return out[:, 0] if size == 1 else out

    @staticmethod
    def _check_factor(factor):
        if factor not in ("svd", "cholesky"):
            raise ValueError("factor must be 'svd' or 'cholesky', not {0!r}".format(factor))

    @staticmethod
    def _cholesky_draws(mu, cov, z, tol=None):
        """``mu + z[:, :rank] @ L[:, :rank].T`` with ``L`` the pivoted Cholesky factor of ``cov``: the host form of what the
        device does (the same formula: the same ``z`` gives the same draws up to rounding whenever the pivots agree)."""
        L, _, rank = pivoted_cholesky(cov, tol)
        if rank < 0:
            return np.full(z.shape, np.nan)
        return mu + np.dot(z[:, :rank], L[:, :rank].T)

    def _sample_conditional_cholesky(self, y, xs, z):
        """(size, M) draws of ``sample_conditional(factor="cholesky")`` for the normals ``z``, mean model included."""
        self.recompute()
        if self._offers("sample_conditional"):
            out, _, _ = self.solver.sample_conditional(self.kernel, self._residual(y), xs, z)
            return out + self._call_mean(xs)
        mu, cov = self.predict(y, xs, return_cov=True)
        return self._cholesky_draws(mu, cov, z)

    # -- many gradients at once (multi-start fits, per-iteration re-fits, gradient-based ensembles) -----------------------
    def grad_log_likelihood_batch(self, vectors, y, quiet=True):
        """``grad_log_likelihood(y, quiet)`` at each row of ``vectors`` (shape ``(B, len(gp))``, ``get_parameter_vector()``
        order), as an array of shape ``(B, len(gp))`` ordered mean | white_noise | kernel.  Uses the ``x`` and ``yerr`` of
        the last ``compute``.  With the HIP :class:`BasicSolver`, ``N <= BasicSolver.BATCH_MAX_N`` and one member's device
        buffers within ``BasicSolver.BATCH_MAX_BYTES`` the B members are factorised, inverted and reduced together
        (gh_chol_objective_grad_batch); otherwise the rows go through ``set_parameter_vector`` + ``grad_log_likelihood``
        one by one, with the same results.  A member whose matrix is not positive definite, or whose mean is not finite,
        has a zero gradient with ``quiet=True``; with ``quiet=False`` the first one raises (``np.linalg.LinAlgError`` /
        ``ValueError`` naming it).  The GP's parameter vector, ``computed`` flag, factorisation and caches are what they
        were before the call."""
        vectors, y = self._batch_args(vectors, y)
        if len(vectors) == 0:
            return np.empty((0, len(self)))
        if self._grad_batch_on_device():
            return self._grad_batch_device(vectors, y, quiet)[1]
        out = np.empty((len(vectors), len(self)))

        def one(b):
            out[b] = self.grad_log_likelihood(y, quiet=quiet)

        self._each_member(range(len(vectors)), one, ValueError, vectors)   # (np.linalg.LinAlgError is a ValueError)
        return out

    def nll_and_grad_batch(self, vectors, y, quiet=True):
        """``nll_and_grad(v, y, quiet)`` at each row ``v`` of ``vectors``: ``(nll (B,), grad (B, len(gp)))``.  A row
        outside the prior gives ``(inf, 0)`` and is not evaluated; a failed member gives ``(inf, 0)`` with ``quiet=True``.
        Routing, errors and the GP's state as :meth:`grad_log_likelihood_batch`."""
        vectors, y = self._batch_args(vectors, y)
        B = len(vectors)
        nll, grad = np.full(B, np.inf), np.zeros((B, len(self)))
        if B == 0:
            return nll, grad
        idx = np.flatnonzero(self._batch_in_prior(vectors))
        if not len(idx):
            return nll, grad
        if self._grad_batch_on_device():
            ll, g = self._grad_batch_device(vectors[idx], y, quiet, index=idx)
            nll[idx], grad[idx] = -ll, -g
            return nll, grad

        def one(b):
            nll[b], grad[b] = self.nll_and_grad(vectors[b], y, quiet=quiet)

        self._each_member(idx, one, ValueError)
        return nll, grad

    def _grad_batch_on_device(self):
        return self._batch_on_device(BasicSolver.grad_batch_bytes(len(self._x)))

    def _batch_in_prior(self, vectors):
        """(B,) bool: is ``log_prior()`` finite at each row (evaluated on the GP's own models, then restored)?"""
        inside = np.empty(len(vectors), dtype=bool)
        with self._state_kept():
            for b, v in enumerate(vectors):
                ModelSet.set_parameter_vector(self, v)
                inside[b] = np.isfinite(self.log_prior())
        return inside

    def _grad_batch_device(self, vectors, y, quiet, index=None):
        """(log-likelihood (B,), gradient (B, len(gp))) of every row from one batched device call; failed members are
        (-inf, 0) or, with ``quiet=False``, the first one in row order raises (named by ``index[b]`` when given)."""
        kp, sigma, r, ok = self._batch_inputs(vectors, y, True)
        solver = BasicSolver(self.kernel, **(self.solver_kwargs))      # (its own pooled handle: self.solver is untouched)
        which = self.kernel.unfrozen_mask.astype(np.uint32)
        logdet, quad, kg, alpha, diagA, info = solver.objective_grad_batch(kp, self._x, sigma, r, which)
        with np.errstate(invalid="ignore", over="ignore"):
            grad, ok_g = self._assemble_grad_batch(vectors, alpha, diagA, kg)
            ll = -0.5 * (len(self._x) * np.log(2 * np.pi) + logdet) - 0.5 * quad
        bad = ~ok | (info != 0) | ~ok_g
        if not quiet and bad.any():
            b = int(np.argmax(bad))
            name = b if index is None else int(index[b])
            if not ok[b]:
                raise ValueError("member {0}: mean function returned NaN or Inf for parameters:\n{1}".format(
                    name, self._batch_blocks(vectors[b:b + 1])["mean"][0]))
            if info[b] != 0:                                       # (b is then the first member whose info is set)
                self._raise_not_positive_definite(info, index)
            raise ValueError("member {0}: mean gradient function returned NaN or Inf for parameters:\n{1}".format(
                name, self._batch_blocks(vectors[b:b + 1])["mean"][0]))
        ll[bad | ~np.isfinite(ll)] = -np.inf
        grad[bad] = 0.0
        return ll, grad

    def _assemble_grad_batch(self, vectors, alpha, diagA, kgrad):
        """Row b is ``set_parameter_vector(vectors[b])`` + ``_assemble_grad(alpha[b], diagA[b], kgrad[b][kernel mask])``,
        bit for bit, without touching the GP's state: the gradient counterpart of :meth:`_batch_inputs`.  ``alpha``,
        ``diagA``: (B, N); ``kgrad``: (B, kernel.full_size).  Returns ``(grad (B, len(gp)), ok (B,))``; ``ok[b]`` is False
        (and the row zero) where the mean gradient is not finite, where ``_assemble_grad`` raises or, quiet, returns zeros."""
        B = len(vectors)
        blocks = self._batch_blocks(vectors)
        arg = self._model_arg(self._x)
        n_m, n_wn, n_k = len(self.mean), len(self.white_noise), len(self.kernel)
        grad = np.empty((B, len(self)))
        ok = np.ones(B, dtype=bool)
        at = 0
        if n_m:
            for b, mg in enumerate(self._batch_gradients("mean", blocks["mean"], arg)):
                if np.any(np.isnan(mg)) or np.any(np.isinf(mg)):
                    ok[b] = False
                else:
                    grad[b, at:at + n_m] = np.dot(mg, alpha[b])
            at += n_m
        if n_wn:
            wn = self._batch_values("white_noise", blocks["white_noise"], arg)
            for b, wng in enumerate(self._batch_gradients("white_noise", blocks["white_noise"], arg)):
                grad[b, at:at + n_wn] = 0.5 * np.sum((np.exp(wn[b]) * diagA[b])[None, :] * wng, axis=1)
            at += n_wn
        if n_k:
            grad[:, at:at + n_k] = np.asarray(kgrad)[:, self.kernel.unfrozen_mask]
        grad[~ok] = 0.0
        return grad, ok

    def predict(self, y, t, return_cov=True, return_var=False, cache=True, kernel=None):
        """Conditional mean and (co)variance at ``t``  (gp.py:482-545)."""
        self.recompute()
        xs = np.ascontiguousarray(self.parse_samples(t), dtype=np.float64)
        if kernel is None:
            kernel = self.kernel

        if self._offers("predict"):
            if cache:
                self._compute_alpha(y, True)       # keep the reference's alpha-cache semantics (gp.py:260-275)
            want_var = bool(return_var)
            want_cov = bool(return_cov) and not want_var
            mu, var, cov = self.solver.predict(kernel, self._residual(y), xs,
                                               return_var=want_var, return_cov=want_cov)
            mu = mu + self._call_mean(xs)
            if want_var:
                return mu, var
            if want_cov:
                return mu, cov
            return mu

        alpha = self._compute_alpha(y, cache)
        Kxs = kernel.get_value(xs, self._x)
        mu = np.dot(Kxs, alpha) + self._call_mean(xs)
        if not (return_var or return_cov):
            return mu
        KinvKxs = self.solver.apply_inverse(Kxs.T)
        if return_var:
            var = kernel.get_value(xs, diag=True)
            var -= np.sum(Kxs.T * KinvKxs, axis=0)
            return mu, var
        cov = kernel.get_value(xs)
        cov -= np.dot(Kxs, KinvKxs)
        return mu, cov

    # -- derivatives of the prediction with respect to the test points (no reference counterpart: gp.py stops at predict) --
    # With alpha = K^-1 r, w_c = K^-1 K(x, t_c), G_cid = d k(t_c, x_i) / d t_cd and D_cd the x1- plus x2-gradient of k at (t_c, t_c):
    #     dmu_cd = sum_i G_cid alpha_i + d mean / d t_cd,        dvar_cd = D_cd - 2 sum_i G_cid w_ic.
    # A solver that offers ``predict_gradient`` (the HIP BasicSolver) does it in one device call and never stores G; any other
    # one takes the NumPy branch on ``apply_inverse``, formula for formula, in blocks of test points that keep the host
    # tensor G under PREDICT_GRADIENT_BLOCK_ELEMENTS doubles.
    PREDICT_GRADIENT_BLOCK_ELEMENTS = 1 << 24            # 128 MB of G per block

    def _mean_gradient_at(self, xs, mean_gradient):
        """d mean / d t at ``xs``, (M, ndim): the caller's ``mean_gradient``, or exactly 0 for a ConstantModel mean."""
        if mean_gradient is None:
            if isinstance(self.mean, ConstantModel):
                return None
            raise ValueError("the mean model {0} has no derivative with respect to its input: pass mean_gradient=, a "
                             "callable t -> (M, ndim)".format(type(self.mean).__name__))
        g = np.asarray(mean_gradient(self._model_arg(xs)), dtype=np.float64)
        if g.ndim == 1 and xs.shape[1] == 1:
            g = g[:, None]
        if g.shape != xs.shape:
            raise ValueError("mean_gradient must return an array of shape (M, ndim) = {0}".format(xs.shape))
        return g

    def _predict_gradient_generic(self, kernel, alpha, xs, want_var, want_value):
        """the NumPy branch: (mu | None, var | None, dmu, dvar | None) without the mean model"""
        x = self._x
        m, n, nd = len(xs), len(x), xs.shape[1]
        step = max(1, int(self.PREDICT_GRADIENT_BLOCK_ELEMENTS // max(1, max(n, 1) * nd)))
        if want_var:                                     # D needs the (B, B, ndim) gradients of a block against itself
            step = max(1, min(step, int(np.sqrt(self.PREDICT_GRADIENT_BLOCK_ELEMENTS / nd))))
        mu = np.empty(m) if want_value else None
        var = np.empty(m) if (want_value and want_var) else None
        dmu = np.empty((m, nd))
        dvar = np.empty((m, nd)) if want_var else None
        for c0 in range(0, m, step):
            tb = np.ascontiguousarray(xs[c0:c0 + step])
            sl = slice(c0, c0 + len(tb))
            G = np.asarray(kernel.get_x1_gradient(tb, x))                     # (B, N, ndim)
            dmu[sl] = np.einsum("cid,i->cd", G, alpha)
            Kxs = kernel.get_value(tb, x) if (want_value or want_var) else None
            if want_value:
                mu[sl] = np.dot(Kxs, alpha)
            if want_var:
                Wb = np.asarray(self.solver.apply_inverse(np.ascontiguousarray(Kxs.T)))      # (N, B)
                idx = np.arange(len(tb))
                D = (np.asarray(kernel.get_x1_gradient(tb, tb))[idx, idx] + np.asarray(kernel.get_x2_gradient(tb, tb))[idx, idx])
                dvar[sl] = D - 2.0 * np.einsum("cid,ic->cd", G, Wb)
                if want_value:
                    var[sl] = kernel.get_value(tb, diag=True) - np.sum(Kxs.T * Wb, axis=0)
        return mu, var, dmu, dvar

    def predict_gradient(self, y, t, return_var=False, return_value=False, cache=True, kernel=None, mean_gradient=None):
        """Derivatives of :meth:`predict` with respect to the test points ``t``: ``dmu`` (M, ndim); ``(dmu, dvar)`` with
        ``return_var``; ``(mu, dmu)`` with ``return_value``; ``(mu, var, dmu, dvar)`` with both -- values and derivatives of
        one evaluation, the shape ``scipy.optimize.minimize(..., jac=True)`` asks for.

        ``mean_gradient``: a callable ``t -> (M, ndim)``, the derivative of the mean model with respect to its input (the
        modelling protocol has none).  With ``None`` a constant mean contributes exactly 0 and any other mean model raises
        ``ValueError``.  The mean model's value at ``t`` is added to ``mu`` as in :meth:`predict`."""
        self.recompute()
        xs = np.ascontiguousarray(self.parse_samples(t), dtype=np.float64)
        if kernel is None:
            kernel = self.kernel
        want_var, want_value = bool(return_var), bool(return_value)
        mg = self._mean_gradient_at(xs, mean_gradient)

        if self._offers("predict_gradient"):
            if cache:
                self._compute_alpha(y, True)       # the alpha-cache semantics of predict
            mu, var, dmu, dvar = self.solver.predict_gradient(kernel, self._residual(y), xs, return_var=want_var,
                                                              return_value=want_value)
        else:
            alpha = self._compute_alpha(y, cache)
            mu, var, dmu, dvar = self._predict_gradient_generic(kernel, alpha, xs, want_var, want_value)
        if mg is not None:
            dmu = dmu + mg
        if want_value:
            mu = mu + self._call_mean(xs)
            return (mu, var, dmu, dvar) if want_var else (mu, dmu)
        return (dmu, dvar) if want_var else dmu

    def apply_inverse(self, y):
        """K^-1 (y - mean) for a vector or an (n, K) matrix  (gp.py:277-301)."""
        self.recompute(quiet=False)
        r = np.array(y, dtype=np.float64, order="F")
        r = self._check_dimensions(r, check_dim=False)
        r -= self._call_mean(self._x)[(slice(None),) + (np.newaxis,) * (r.ndim - 1)]
        b = self.solver.apply_inverse(r, in_place=True)
        return b.flatten() if r.ndim == 1 else b

    # -- sampling -------------------------------------------------------------------
    def sample_conditional(self, y, t, size=1, factor="svd"):
        """Draws from the predictive distribution at ``t`` given ``y``: (M,) for ``size == 1``, else (size, M).

        ``factor="svd"`` (the default) is the reference's path, draw for draw: ``predict`` and
        ``multivariate_gaussian_samples`` (an SVD of the M x M covariance on the host).  ``factor="cholesky"`` factors the
        covariance by a diagonally pivoted Cholesky with rank truncation (a predictive covariance is numerically
        semidefinite: a plain Cholesky fails on it) and returns ``mu + z[:, :rank] @ L[:, :rank].T``.  Its random-number
        rule differs from the SVD path's: ONE call ``z = np.random.standard_normal((size, M))`` is made before the factor.
        A solver that offers ``sample_conditional`` (the HIP :class:`BasicSolver`) does all of it on the device -- the
        covariance never reaches the host; the mean model at ``t`` is added on the host, as in ``predict``.  Any other solver
        goes through ``predict(..., return_cov=True)`` and :func:`george_amd.utils.pivoted_cholesky` with the same formula."""
        self._check_factor(factor)
        if factor == "svd":
            mu, cov = self.predict(y, t)
            return multivariate_gaussian_samples(cov, size, mean=mu)
        xs = np.ascontiguousarray(self.parse_samples(t), dtype=np.float64)
        z = np.random.standard_normal((size, len(xs)))
        out = self._sample_conditional_cholesky(y, xs, z)
        return out[0] if size == 1 else out

    def sample(self, t=None, size=1, factor="svd"):
        """Draws from the prior: at the computed points (``t=None``: ``apply_sqrt`` of the solver, whatever ``factor``) or
        at ``t``, where ``factor`` chooses as in :meth:`sample_conditional` -- ``"svd"``: ``get_matrix`` + ``TINY`` on the
        diagonal + ``multivariate_gaussian_samples``, the reference's path; ``"cholesky"``: ONE call
        ``z = np.random.standard_normal((size, M))``, then ``mean(t) + z @ L.T`` with ``L`` the pivoted Cholesky factor of
        ``K(t, t) + TINY I``, built and factored on the device (gh_kernel_sample) when the GP's solver is a device solver
        (one that offers ``sample_conditional``), else on the host."""
        self._check_factor(factor)
        if t is None:
            self.recompute()
            n = self._x.shape[0]
            out = self.solver.apply_sqrt(np.random.randn(size, n))
            out += self._call_mean(self._x)
            return out[0] if size == 1 else out
        x = self.parse_samples(t)
        if factor == "cholesky":
            x = np.ascontiguousarray(x, dtype=np.float64)
            z = np.random.standard_normal((size, len(x)))
            if self._offers("sample_conditional", on_type=True):
                out, _ = self.kernel.kernel.sample(x, z, jitter=TINY)
            else:
                cov = self.get_matrix(x)
                cov[np.diag_indices_from(cov)] += TINY
                out = self._cholesky_draws(0.0, cov, z)
            out = out + self._call_mean(x)
            return out[0] if size == 1 else out
        cov = self.get_matrix(x)
        cov[np.diag_indices_from(cov)] += TINY
        return multivariate_gaussian_samples(cov, size, mean=self._call_mean(x))

    def get_matrix(self, x1, x2=None):
        x1 = self.parse_samples(x1)
        if x2 is None:
            return self.kernel.get_value(x1)
        return self.kernel.get_value(x1, self.parse_samples(x2))

    # -- aliases ----------------------------------------------------------------------
    def lnlikelihood(self, y, quiet=False):
        warnings.warn("'lnlikelihood' is deprecated. Use 'log_likelihood'", DeprecationWarning)
        return self.log_likelihood(y, quiet=quiet)

    def grad_lnlikelihood(self, y, quiet=False):
        warnings.warn("'grad_lnlikelihood' is deprecated. Use 'grad_log_likelihood'", DeprecationWarning)
        return self.grad_log_likelihood(y, quiet=quiet)

    def get_value(self, *args, **kwargs):
        return self.log_likelihood(*args, **kwargs)

    def get_gradient(self, *args, **kwargs):
        return self.grad_log_likelihood(*args, **kwargs)
