"""GP -- the reference's user-facing class for the dense hot path, MI355X-native.

Mirrors ``gpyreg.GP`` (reference gaussian_process.py:24) for everything on the path
this package accelerates: construction from the three plugin objects, ``update``
(full-recompute loop :870-884), ``predict`` (:1663-1816), ``log_likelihood`` /
``log_posterior`` (:1468-1518), the name-mangled ``_GP__compute_nlZ`` (:1520) the
reference's tests call, hyperparameter get/set and dict conversion (:516-689),
``clean`` (:886-905) and the ``Posterior`` record (:2568-2586).

All O(N^2) / O(N^3) arithmetic runs in libgpcore.so (HIP, gfx950): hyperparameter
vectors are evaluated in BATCHES (``nll_batch``) -- one launch sequence covers all
samples -- and posteriors stay resident in HBM; ``Posterior.alpha/.sW/.L`` are
materialised as NumPy arrays lazily on first access.  There is no NumPy/SciPy
fallback for the core: without the HIP library or a GPU these methods raise.
"""

from __future__ import annotations

import math
import threading
from textwrap import indent

import numpy as np
import scipy.optimize
from numpy.linalg import LinAlgError  # scipy.linalg.LinAlgError is this class

from . import _lib
from . import _remove as _rm
from . import priors as _pr
from . import sharding as _sh
from .f_min_fill import f_min_fill
from .slice_sample import SliceSampler


class Posterior:
    """The reference's posterior record (gaussian_process.py:2568-2586).

    ``alpha``  = (K + sn2_mult*Sigma)^-1 (y - m)            shape (N, 1)
    ``sW``     = 1/sqrt(min(sn2) * sn2_mult)                 shape (N, 1)
    ``L``      = upper Cholesky factor of (K + mult*Sigma)/sl when ``L_chol`` (a
                 Fortran-ordered array like SciPy's), else -(K + mult*Sigma)^-1
    Fields backed by device memory are fetched on first access and then cached;
    assigning to them (as ``GP.clean`` does) detaches them from the device copy.
    """

    def __init__(self, hyp, alpha, sW, L, sn2_mult, Lchol, _handle=None, _index=None, _owner=None):
        self.hyp = hyp
        self._alpha, self._sW, self._L = alpha, sW, L
        self.sn2_mult = sn2_mult
        self.L_chol = Lchol
        self._handle, self._index = _handle, _index
        self._owner = _owner  # a copied / unpickled GP whose device posteriors are rebuilt at first use (GP._restore)
        self._have = {"alpha": alpha is not None, "sW": sW is not None, "L": L is not None}

    def _fetch(self, what):
        if not self._have[what] and self._handle is None and self._owner is not None:
            self._owner._restore()
        if self._have[what] or self._handle is None:
            return
        a, w, Lm = self._handle.fetch(
            self._index, alpha=(what == "alpha"), sW=(what == "sW"), L=(what == "L")
        )
        if what == "alpha":
            self._alpha = a.reshape(-1, 1)
        elif what == "sW":
            self._sW = w.reshape(-1, 1)
        else:
            self._L = Lm.T if self.L_chol else Lm  # lower factor^T = SciPy's upper U
        self._have[what] = True

    @property
    def alpha(self):
        self._fetch("alpha")
        return self._alpha

    @alpha.setter
    def alpha(self, v):
        self._alpha, self._have["alpha"] = v, True

    @property
    def sW(self):
        self._fetch("sW")
        return self._sW

    @sW.setter
    def sW(self, v):
        self._sW, self._have["sW"] = v, True

    @property
    def L(self):
        self._fetch("L")
        return self._L

    @L.setter
    def L(self, v):
        self._L, self._have["L"] = v, True

    def _detach(self):
        self._handle = None

    def __getstate__(self):
        # a record copied or pickled BY ITSELF becomes the reference's plain record: its fields are brought to the host
        for what in ("alpha", "sW", "L"):
            self._fetch(what)
        d = self.__dict__.copy()
        d["_handle"] = d["_index"] = d["_owner"] = None
        return d


def _on_device(method):
    """The device copy of (X, y) belongs to the context, not to the GP: uploading this GP's data and the call that
    uses it must not be separated by another thread's GP on the same device.  Held for the whole method (re-entrant)."""
    import functools

    @functools.wraps(method)
    def held(self, *a, **k):
        with _lib.context(self.device).lock:
            return method(self, *a, **k)

    return held


def _mix_samples(means, variances):
    """Moments of the equal-weight mixture of per-sample Gaussians, column = sample: (mean (M,1), variance (M,1) |
    None, between-sample variance).  One sample: returned as it is (between = 0)."""
    S = means.shape[1]
    if S == 1:
        return means, variances, 0
    centre = np.reshape(np.sum(means, 1), (-1, 1)) / S
    between = np.sum((means - centre) ** 2, 1) / (S - 1)
    total = None if variances is None else np.reshape(np.sum(variances, 1) / S + between, (-1, 1))
    return centre, total, between


def _cv_folds(folds, N):
    """``cv_predict``'s reading of ``folds``: None (leave-one-out) stays None, an int F becomes F contiguous blocks
    (``np.array_split``), a sequence of index collections becomes a list of sorted int64 arrays, validated."""
    if folds is None:
        return None
    if isinstance(folds, (int, np.integer)) and not isinstance(folds, (bool, np.bool_)):
        F = int(folds)
        if F < 2 or F > N:
            raise ValueError(f"cv_predict: an integer folds must lie in [2, N = {N}], got {F}")
        return list(np.array_split(np.arange(N, dtype=np.int64), F))
    try:
        seq = list(folds)
    except TypeError:
        raise ValueError(f"cv_predict: folds must be None, an int or a sequence of index arrays, got {folds!r}") from None
    if not seq:
        raise ValueError("cv_predict: folds is an empty sequence")
    owner = np.full(N, -1, dtype=np.int64)
    out = []
    for f, idx in enumerate(seq):
        a = np.asarray(idx)
        if a.size == 0:
            raise ValueError(f"cv_predict: fold {f} is empty")
        if a.dtype.kind not in "iu":
            raise ValueError(f"cv_predict: fold {f} must hold integer indices, got dtype {a.dtype}")
        a = np.sort(a.ravel().astype(np.int64))
        if a[0] < 0 or a[-1] >= N:
            bad = a[0] if a[0] < 0 else a[-1]
            raise ValueError(f"cv_predict: fold {f} has index {bad} out of range [0, {N})")
        if np.any(a[1:] == a[:-1]):
            raise ValueError(f"cv_predict: fold {f} repeats index {a[1:][a[1:] == a[:-1]][0]}")
        if a.size >= N:
            raise ValueError(f"cv_predict: fold {f} holds all {N} points: nothing is left to predict from")
        clash = owner[a] >= 0
        if clash.any():
            raise ValueError(f"cv_predict: fold {f} overlaps fold {owner[a][clash][0]} at index {a[clash][0]}")
        owner[a] = f
        out.append(a)
    return out


def _mix_sample_grads(means, dmeans, dvariances):
    """Gradients of ``_mix_samples``' mixture moments.  means (M, S); dmeans, dvariances (M, D, S), the per-sample
    gradients with respect to the D inputs of each row: (dmean (M, D), dvariance (M, D)).  The spread term is
    d/dx sum_s (mu_s - mu)^2 / (S - 1) = 2 sum_s (mu_s - mu) dmu_s / (S - 1) (sum_s (mu_s - mu) = 0)."""
    S = means.shape[1]
    if S == 1:
        return dmeans[:, :, 0], dvariances[:, :, 0]
    centre = np.sum(means, 1, keepdims=True) / S
    dmu = np.sum(dmeans, 2) / S
    ds2 = np.sum(dvariances, 2) / S + 2 * np.einsum("ms,mds->md", means - centre, dmeans) / (S - 1)
    return dmu, ds2


def _quad_measures(mu, sigma, D):
    """``quad``'s reading of the Gaussian measures: a scalar fills a row of D, sigma broadcasts to mu's shape."""
    mu = np.tile(mu, (1, D)) if np.size(mu) == 1 else np.atleast_2d(np.asarray(mu, dtype=float))
    sigma = np.tile(sigma, (1, D)) if np.size(sigma) == 1 else np.atleast_2d(np.asarray(sigma, dtype=float))
    sigma = np.broadcast_to(sigma, mu.shape).astype(float)
    return mu, sigma


def _quad_gamma(mu, sigma, ell, ln_sf2):
    """Gamma (M, M), the prior covariance between the integrals against the measures: sf2 prod_l ell_l / sqrt(t_jkl)
    exp(-1/2 sum_l (mu_jl - mu_kl)^2 / t_jkl), t_jkl = ell_l^2 + sigma_jl^2 + sigma_kl^2 (its diagonal: quad's nf_kk)."""
    t = ell**2 + sigma[:, None, :]**2 + sigma[None, :, :]**2
    d = mu[:, None, :] - mu[None, :, :]
    return np.exp(ln_sf2 + np.sum(np.log(ell)) - 0.5 * np.sum(np.log(t), 2) - 0.5 * np.sum(d**2 / t, 2))


def _mean_grad_x(mean, hyp, X, who="predict_grad"):
    """d m(x) / dx (M, D) of a stock mean function under the mean hyperparameters ``hyp``; exact types only (a
    subclass may compute anything): other mean objects raise NotImplementedError (``who``: the method named there)."""
    from .mean_functions import ConstantMean, NegativeQuadratic, ZeroMean

    if type(mean) in (ZeroMean, ConstantMean):
        return np.zeros(X.shape)
    if type(mean) is NegativeQuadratic:
        D = X.shape[1]
        return -(X - hyp[1:1 + D]) / np.exp(2 * hyp[1 + D:1 + 2 * D])
    raise NotImplementedError(f"{who}: the mean function {mean!r} ({type(mean).__name__}) is user-defined; its "
                              "gradient with respect to x_star is unknown")


def _mean_hyp(hyp, counts):
    """The mean function's hyperparameters in a sample's vector (or in the rows of a batch); counts = GP._counts()."""
    cov_N, noise_N, mean_N = counts
    return hyp[..., cov_N + noise_N:cov_N + noise_N + mean_N]


def _sn2_mult(post):
    """A posterior record's noise multiplier; 1 for a record that never had one (no data, or cleaned)."""
    return 1 if post.sn2_mult is None else post.sn2_mult


class PosteriorPaths:
    """``GP.sample_paths``' result: ``n_paths`` sampled posterior FUNCTIONS per hyperparameter sample, evaluable --
    with their gradient -- at any points, any number of times (``_paths`` has the formulas).  ``paths(x_star)`` returns
    f (M, n_paths, S), ``paths(x_star, compute_grad=True)`` (f, df) with df (M, D, n_paths, S), entry [j, l] the
    derivative with respect to x_star[j, l]; ``f[:, r, s]`` is the same function in every call.  The object owns device
    copies of what evaluation needs: it describes the posterior as it was when ``sample_paths`` ran and stays valid after
    the GP is updated.  ``close()`` frees the device memory (garbage collection does too).  It cannot be pickled or
    copied: the handle cannot be recreated once the posterior has moved on."""

    def __init__(self, n_paths, n_features, seed, D, kid, degree, mean, hyps, counts, handle=None, host=None,
                 post_range=None, group=None):
        self.n_paths, self.n_features, self.seed = n_paths, n_features, seed
        self._D, self._kid, self._degree, self._mean, self._hyps, self._counts = D, kid, degree, mean, hyps, counts
        self._handle, self._host, self._range, self._group = handle, host, post_range, group
        self._closed = False

    def __call__(self, x_star, compute_grad: bool = False):
        from . import _paths

        if self._closed:
            raise ValueError("PosteriorPaths has been closed")
        x_star = np.atleast_2d(np.asarray(x_star, dtype=float))
        if x_star.ndim != 2 or x_star.shape[1] != self._D:
            raise ValueError(f"x_star must be (M, {self._D}), got {x_star.shape}")
        M, D, R = x_star.shape[0], self._D, self.n_paths
        cov_N = self._counts[0]
        S = len(self._hyps)
        h_mean = [_mean_hyp(h, self._counts) for h in self._hyps]
        dm = [_mean_grad_x(self._mean, h, x_star) for h in h_mean] if compute_grad else None
        if self._host is not None:  # a GP without data: prior paths (v = 0) on the host
            f = np.empty((M, R, S))
            df = np.empty((M, D, R, S)) if compute_grad else None
            for s, (theta, b, wt) in enumerate(self._host):
                out = _paths.evaluate(self._kid, self._degree, self._hyps[s][:cov_N], None, None, theta, b, wt, x_star,
                                      compute_grad)
                if compute_grad:
                    f[:, :, s], df[:, :, :, s] = out
                else:
                    f[:, :, s] = out
        else:
            if self._handle is None:  # (a rank that holds no sample of the set)
                f, df = np.zeros((M, R, 0)), np.zeros((M, D, R, 0))
            elif compute_grad:
                f, df = self._handle.eval(x_star, True)
            else:
                f, df = self._handle.eval(x_star, False), None
            if self._range is not None:  # each rank has its block of samples: one all-gather of the stacked rows
                k = f.shape[2]
                rows = f.reshape(M * R, k)
                if compute_grad:
                    rows = np.concatenate([rows, df.reshape(M * D * R, k)], axis=0)
                full, _ = _sh.gather_rows(self._range[2], rows.shape[0], lambda a, b: (rows.T, np.zeros(b - a, bool)),
                                          self._group, _sh.fingerprint(x_star, bool(compute_grad), self.seed))
                rows = full.T.copy()
                f = rows[:M * R].reshape(M, R, -1)
                if compute_grad:
                    df = rows[M * R:].reshape(M, D, R, -1)
        for s in range(S):
            f[:, :, s] += np.reshape(self._mean.compute(h_mean[s], x_star), (-1, 1))
            if compute_grad:
                df[:, :, :, s] += dm[s][:, :, None]
        return (f, df) if compute_grad else f

    def close(self):
        """Free the device copies; the object cannot be called afterwards."""
        self._closed = True
        if self._handle is not None:
            self._handle.free()
            self._handle = None

    def __reduce_ex__(self, protocol):
        raise TypeError("PosteriorPaths cannot be pickled or copied: it owns device memory that describes the posterior "
                        "at the time sample_paths ran and cannot be recreated; call sample_paths again")


# GP.fit's options with the reference's defaults (gaussian_process.py:991-1006; "burn": thin * n_samples when unset)
_FIT_DEFAULTS = {"opts_N": 3, "init_N": 2**10, "init_method": "sobol", "thin": 5, "df_base": 7, "widths": None,
                 "tol_opt": 1e-5, "tol_opt_mcmc": 1e-3, "sampler": "slicesample", "n_samples": 10, "burn": None,
                 "lower_bounds": "current", "upper_bounds": "current"}

_DTYPES = {"f64": _lib.F64, "fp64": _lib.F64, "float64": _lib.F64,
           "f32": _lib.F32, "fp32": _lib.F32, "float32": _lib.F32}


class GradientConditionedPosterior:
    """``GP.condition_on_gradients``' result: for every hyperparameter sample of the GP, the posterior given its data
    (X, y, s2) AND the gradient observations (X_g, dy, s2_grad) (``_gradobs`` has the formulas).  The object owns the
    device factors of the joint system of order n = N + Ng D and a copy of the points: it describes the GP as it was
    when it was made and stays valid after the GP changes.  ``nlZ`` (S,) is the joint negative log marginal likelihood
    (the number ``GP.nll_batch_grad_obs`` returns for the same hyperparameters), ``sn2_mult`` (S,) and ``L_chol`` (S,)
    the jitter multiplier and the branch of each sample's joint factorization, ``alpha`` a list of (values (N,),
    gradients (Ng, D)) pairs in the user's order.  ``predict`` gives the mean and variance, ``gradient_posterior`` the
    joint posterior of the gradient (and the value), ``predict_grad`` the gradients of ``predict``'s two moments.
    ``close()`` (or leaving a ``with`` block, or garbage collection) frees the device memory."""

    def __init__(self, handle, mean, noise, counts, hyps, dims, nlZ, sn2_mult, L_chol):
        self._handle, self._mean, self._noise, self._counts, self._hyps = handle, mean, noise, counts, hyps
        self._N, self._Ng, self.D = dims
        self.nlZ, self.sn2_mult, self.L_chol = nlZ, sn2_mult, L_chol
        self._alpha = None

    def _live(self):
        if self._handle is None:
            raise ValueError("this GradientConditionedPosterior has been closed")
        return self._handle

    @property
    def alpha(self):
        from . import _gradobs

        if self._alpha is None:
            h = self._live()
            self._alpha = [_gradobs.from_joint(h.fetch(s, sW=False, L=False)[0], self._N, self._Ng, self.D)
                           for s in range(len(self._hyps))]
        return self._alpha

    def predict(self, x_star, add_noise: bool = False, s2_star=None, separate_samples: bool = False):
        """Posterior mean and variance at ``x_star`` (M, D) with ``GP.predict``'s conventions: (mu, s2), each (M, S)
        with ``separate_samples``, else the (M, 1) moments of the equal-weight mixture over the samples (divisor
        S - 1 for the spread of the means).  The variance is clamped at 0; ``add_noise`` adds the noise function's
        value (with ``s2_star``) times the joint factorization's multiplier."""
        x_star = np.atleast_2d(np.asarray(x_star, dtype=float))
        if x_star.ndim != 2 or x_star.shape[1] != self.D or x_star.shape[0] < 1:
            raise ValueError(f"x_star must be (M, {self.D}), got {x_star.shape}")
        if not np.all(np.isfinite(x_star)):
            raise ValueError("x_star must be finite")
        cov_N, noise_N, _ = self._counts
        fmu, fs2 = self._live().predict_gobs(x_star)
        S = len(self._hyps)
        mu, s2 = np.empty(fmu.shape), np.empty(fs2.shape)
        for s, hyp in enumerate(self._hyps):
            mu[:, s] = np.reshape(self._mean.compute(_mean_hyp(hyp, self._counts), x_star), (-1,)) + fmu[:, s]
            s2[:, s] = np.maximum(fs2[:, s], 0)
            if add_noise:
                sn2 = self._noise.compute(hyp[cov_N:cov_N + noise_N], x_star, None, s2_star) * self.sn2_mult[s]
                s2[:, s] += np.reshape(np.broadcast_to(sn2, (x_star.shape[0], 1)), (-1,))
        if not separate_samples and S >= 1:
            mu, s2, _ = _mix_samples(mu, s2)
        return mu, s2

    def _queries(self, x_star):
        x_star = np.atleast_2d(np.asarray(x_star, dtype=float))
        if x_star.ndim != 2 or x_star.shape[1] != self.D or x_star.shape[0] < 1:
            raise ValueError(f"x_star must be (M, {self.D}), got {x_star.shape}")
        if not np.all(np.isfinite(x_star)):
            raise ValueError("x_star must be finite")
        return x_star

    def _joint_rows(self, x_star, diag, who):
        """(mean (M, D + 1, S), C (M, D + 1[, D + 1], S)) of (f, grad f) per sample: one gpc_grad_post_gobs call plus the
        mean function's value and x-gradient (stock means only)."""
        handle = self._live()
        M, P, S = x_star.shape[0], self.D + 1, len(self._hyps)
        mean = np.empty((M, P, S))
        for s, h in enumerate(self._hyps):
            hm = _mean_hyp(h, self._counts)
            mean[:, 1:, s] = _mean_grad_x(self._mean, hm, x_star, who)
            mean[:, 0, s] = np.reshape(self._mean.compute(hm, x_star), (-1,))
        fmu, dfmu, C = handle.grad_post_gobs(x_star, diag)
        mean[:, 0, :] += fmu
        mean[:, 1:, :] += dfmu
        return mean, C

    def gradient_posterior(self, x_star, cov: str = "full", with_value: bool = False,
                           separate_samples: bool = False):
        """The posterior distribution of the gradient of the latent function at ``x_star`` given the values AND the
        gradient observations: (dmu, dcov), with ``GP.gradient_posterior``'s contract.

        dmu (M, D) is the posterior mean of grad f (the stock mean functions' gradient included); dcov (M, D, D) its
        posterior covariance, entry [j, l, k] = Cov(df/dx_l, df/dx_k) at x_star[j], or with ``cov="diag"`` the
        variances (M, D) alone (cheaper: no Gram matrix is formed).  With ``with_value`` f itself is prepended as slot
        0: shapes (M, D + 1) and (M, D + 1, D + 1) (or (M, D + 1)), slot 0 holding ``predict``'s latent mean and variance
        before its clamp and [j, 0, 1 + l] = Cov(f, df/dx_l) = half of ``predict_grad``'s variance gradient.  Nothing is
        clamped or projected: each per-sample matrix is returned as computed (symmetric to the bit; its smallest
        eigenvalue may be a rounding error below 0 where the posterior is nearly certain -- at a gradient point
        observed without noise, for one).  With ``separate_samples`` a trailing axis S holds the hyperparameter
        samples; otherwise the moments of their equal-weight mixture are returned: the mean of the means, and the mean
        of the covariances plus the between-sample covariance of the mean vectors (divisor S - 1; one sample is
        returned as it is).

        The operand of the joint system, the solves and the per-query Gram matrices run on the device
        (gpc_grad_post_gobs; ``_gradobs`` has the formulas).  Stock mean functions only (NotImplementedError
        otherwise).  Not sharded: the calling rank computes every sample."""
        from . import _gradpost as _gpm

        if cov not in ("full", "diag"):
            raise ValueError(f"gradient_posterior: cov must be 'full' or 'diag', got {cov!r}")
        diag = cov == "diag"
        self._live()
        x_star = self._queries(x_star)
        mean, C = self._joint_rows(x_star, diag, "gradient_posterior")
        if not with_value:
            mean = mean[:, 1:]
            C = C[:, 1:] if diag else C[:, 1:, 1:]
        if separate_samples:
            return mean, C
        return _gpm.mix_diag(mean, C) if diag else _gpm.mix(mean, C)

    def predict_grad(self, x_star, add_noise: bool = False, s2_star=None, separate_samples: bool = False):
        """``predict``'s mean and variance at ``x_star`` and their gradients with respect to ``x_star``:
        (mu, s2, dmu, ds2), with ``GP.predict_grad``'s conventions.  mu and s2 are what ``predict`` returns for the same
        arguments (within rounding); dmu and ds2 are (M, D), or (M, D, S) with ``separate_samples``, entry [j, l] the
        derivative with respect to x_star[j, l].  All four come from ONE gpc_grad_post_gobs call: mu and s2 are slot 0
        of the joint posterior of (f, grad f), dmu its gradient slots and ds2_l = 2 Cov(f, df/dx_l).  The variance is
        clamped at 0 and its gradient is 0 where the clamp holds; ``add_noise`` adds the noise function's value (with
        ``s2_star``) times the joint factorization's multiplier, as ``predict`` does, and leaves ds2 unchanged (stock
        ``GaussianNoise`` only: the noise must not depend on x_star).  Stock mean functions only.  Not sharded."""
        from .noise_functions import GaussianNoise

        self._live()
        x_star = self._queries(x_star)
        if add_noise and type(self._noise) is not GaussianNoise:
            raise NotImplementedError(f"predict_grad: the noise function {self._noise!r} is user-defined; add_noise "
                                      "needs noise that does not depend on x_star")
        cov_N, noise_N, _ = self._counts
        mean, C = self._joint_rows(x_star, False, "predict_grad")
        mu, dmu = mean[:, 0, :], mean[:, 1:, :]
        fs2 = C[:, 0, 0, :]
        # the clamp of predict, s2 = max(s2, 0): no variance gradient where it holds s2 at 0
        ds2 = np.where((fs2 <= 0)[:, None, :], 0.0, 2 * C[:, 0, 1:, :])
        s2 = np.maximum(fs2, 0)
        if add_noise:
            for s, hyp in enumerate(self._hyps):
                sn2 = self._noise.compute(hyp[cov_N:cov_N + noise_N], x_star, None, s2_star) * self.sn2_mult[s]
                s2[:, s] += np.reshape(np.broadcast_to(sn2, (x_star.shape[0], 1)), (-1,))
        if not separate_samples:
            dmu, ds2 = _mix_sample_grads(mu, dmu, ds2)
            mu, s2, _ = _mix_samples(mu, s2)
        return mu, s2, dmu, ds2

    def close(self):
        if self._handle is not None:
            self._handle.free()
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class GP:
    """A single Gaussian process (reference gaussian_process.py:24-62).

    Parameters are the reference's (``D``, ``covariance``, ``mean``, ``noise``) plus
    build-only keywords: ``device`` (HIP device index, default LOCAL_RANK or 0),
    ``dtype`` ("f64" default, or "f32" for the factorization arithmetic) and
    ``reference_quirks`` (default False): where the reference's own code is wrong -- three places,
    all found by diffing against its printed output -- return ITS numbers instead of the corrected ones:
    the quadrature variance with user-provided noise rescaled by exp(2 hyp[cov_N]) sn2_mult although
    the factor was scaled by min(sn2) sn2_mult (gaussian_process.py:1921-1922, :1953-1958); quadrature
    with an isotropic kernel in D > 1 reading the two hyperparameters as ARD length scales
    (:1898-1903); ``update`` with one new point AND new hyperparameters appending under the old
    samples and dropping the new ones (:736-746).  Also settable as an attribute afterwards.
    """

    def __init__(self, D: int, covariance: object, mean: object, noise: object,
                 device: int | None = None, dtype: str = "f64", reference_quirks: bool = False):
        """``gpyreg.GP(D, covariance, mean, noise)`` (reference gaussian_process.py:43-62) plus ``device``, ``dtype``
        and ``reference_quirks``.

        DEFAULT DEVIATIONS FROM THE REFERENCE -- a drop-in that differs by default has to say so here.  With
        ``reference_quirks=False`` (the default) three results are NOT the reference's numbers, because the reference's
        own code is wrong there (each found by diffing against its printed output, each reproduced exactly with
        ``reference_quirks=True``):

        1. ``quad(compute_var=True)`` with user-provided noise ``s2``: the reference rescales by
           ``exp(2 hyp[cov_N]) * sn2_mult`` although the factor was scaled by ``min(sn2) * sn2_mult``
           (gaussian_process.py:1921-1922 against :1953-1958); the default here uses the factor's own scale.
        2. ``quad`` with an isotropic squared-exponential kernel in D > 1: the reference reads the two hyperparameters
           as ARD length scales of the first two dimensions (:1898-1903); the default uses one length scale for all.
        3. ``update(X_new=one point, y_new, hyp=new samples)``: the reference appends under the OLD samples and drops
           the new ones (:736-746); the default recomputes with the new ones.

        Everything else -- nlZ, gradients, posteriors, predictions, lpd, fits under a fixed seed -- is held to the
        reference's values by the golden fixtures under tests/golden/."""
        self.D = D
        self._quirks = bool(reference_quirks)
        self.covariance = covariance
        self.mean = mean
        self.noise = noise
        self._token = None
        self._post_handle = None
        self._rebuild = False
        self._X = self._y = self._s2 = None
        self.posteriors = None
        self.no_prior = None  # set_bounds must not touch the priors before set_priors ran
        self.normalization_constants = None
        self.temporary_data = {}
        self.device = device
        if dtype not in _DTYPES:
            raise ValueError("dtype must be 'f64' or 'f32'")
        self.dtype = dtype
        # Multi-GPU: when a torch.distributed process group with more than one rank is initialised
        # (one process per GPU, torchrun), every batched entry point shards the hyperparameter samples
        # over the ranks and all-gathers the per-sample results (the reference's loops over samples:
        # f_min_fill.py:174-176, gaussian_process.py:876-879, :1727).  Every rank must call with the
        # same arguments.  ``shard = False`` keeps this GP rank-local (replicas).
        self.shard = True
        self.process_group = None
        self._post_range = None  # (lo, hi, S): the block of posterior samples resident on this rank
        # Any object with the reference's covariance protocol is accepted (the reference calls
        # whatever it was given: gaussian_process.py:2388-2390; AbstractKernel,
        # covariance_functions.py:9-20).  The built-in kernels are evaluated on the device; any
        # other object's own compute() supplies K and dK, and the factorization, solves and the
        # gradient contraction still run on the device (gpc_nll_batch_K and friends).
        self._builtin = getattr(covariance, "_gpc_kernel_id", None) is not None
        self.set_bounds()
        self.set_priors()

    @property
    def reference_quirks(self):
        return self.__dict__.get("_quirks", False)

    @reference_quirks.setter
    def reference_quirks(self, v):
        self._quirks = bool(v)

    # ------------------------------------------------------------------ plumbing
    # X, y and s2 are plain public attributes in the reference and its tests assign them directly
    # (testing/test_gaussian_process.py:1139).  Here the device holds a copy of X and y, so assigning
    # any of them marks that copy stale (re-uploaded on next use).  Mutating the arrays IN PLACE
    # cannot be seen: call ``invalidate()`` afterwards.
    @property
    def X(self):
        return self._X

    @X.setter
    def X(self, v):
        self._X, self._token = v, None

    @property
    def y(self):
        return self._y

    @y.setter
    def y(self, v):
        self._y, self._token = v, None

    @property
    def s2(self):
        return self._s2

    @s2.setter
    def s2(self, v):
        self._s2 = v

    def invalidate(self):
        """Declare the device copy of X, y stale (after an in-place edit of ``gp.X`` / ``gp.y``)."""
        self._token = None

    def _counts(self):
        cov_N = self.covariance.hyperparameter_count(self.D)
        mean_N = self.mean.hyperparameter_count(self.D)
        noise_N = self.noise.hyperparameter_count()
        return cov_N, noise_N, mean_N

    def _ctx(self):
        ctx = _lib.context(self.device)
        if self.X is None or self.y is None:
            raise ValueError("GP has no training data")
        if ctx.data_token is not self._token or self._token is None:
            self._token = object()
            ctx.set_data(self.X, self.y, self._token)
        return ctx

    def _const_mean(self):
        """The mean is the stock ZeroMean or ConstantMean (exact types: a subclass may compute anything)."""
        from .mean_functions import ConstantMean, ZeroMean

        return type(self.mean) in (ZeroMean, ConstantMean)

    def _noise_values(self, hyp: np.ndarray, grad: bool, counts=None):
        """The noise part of ``_plugin_values``: sn2, dsn2 | None, per-point flag."""
        from .noise_functions import GaussianNoise

        cov_N, noise_N, _ = counts or self._counts()
        S = hyp.shape[0]
        h_noise = hyp[:, cov_N:cov_N + noise_N]
        dsn2 = None
        if type(self.noise) is GaussianNoise:
            sn2 = self.noise.values(h_noise, self.X, self.y, self.s2, grad)
            if grad:
                sn2, dsn2 = sn2
            vec = self.noise.per_point(self.y, self.s2)
        else:
            sn2_rows, dsn2_rows, vec = [], [], False
            for s in range(S):
                r = self.noise.compute(h_noise[s], self.X, self.y, self.s2, compute_grad=grad)
                if grad:
                    r, d = r
                    dsn2_rows.append(np.asarray(d, dtype=float))
                vec = not np.isscalar(r)
                sn2_rows.append(np.ravel(r) if vec else np.array([float(r)]))
            sn2 = np.stack(sn2_rows)
            dsn2 = np.stack(dsn2_rows) if dsn2_rows else None
        if dsn2 is not None and not vec:
            dsn2 = dsn2[:, :1, :]  # a single noise value: the core reads ONE gradient row per sample (:2491-2498)
        return sn2, (dsn2 if (grad and noise_N > 0) else None), vec

    def _plugin_values(self, hyp: np.ndarray, grad: bool):
        """Evaluate the O(N*D) boundary plugins for every sample
        (gaussian_process.py:2371-2400): m (S,N), sn2 (S,N|1), dm (S,N,mean_N), dsn2 (S,N|1,noise_N).

        The stock plugins evaluate all rows in one NumPy pass (their ``values``; the design stage of
        ``fit`` hands over 1024 hyperparameter vectors at once).  Exact types only: a subclass or any other
        object with the reference's protocol is called once per sample through its own ``compute``."""
        from .mean_functions import ConstantMean, NegativeQuadratic, ZeroMean

        counts = self._counts()
        mean_N = counts[2]
        S, N = hyp.shape[0], self.X.shape[0]
        h_mean = _mean_hyp(hyp, counts)
        dm = None
        if type(self.mean) in (ZeroMean, ConstantMean, NegativeQuadratic):
            m = self.mean.values(h_mean, self.X, grad)
            if grad:
                m, dm = m
        else:
            m, dm_rows = np.empty((S, N)), []
            for s in range(S):
                r = self.mean.compute(h_mean[s], self.X, compute_grad=grad)
                if grad:
                    r, d = r
                    if mean_N > 0:
                        dm_rows.append(np.asarray(d, dtype=float).reshape(N, mean_N))
                m[s] = np.reshape(r, (-1,))
            dm = np.stack(dm_rows) if dm_rows else None
        sn2, dsn2, vec = self._noise_values(hyp, grad)
        return {"m": m, "sn2": sn2, "vec": vec,
                "dm": dm if (grad and mean_N > 0) else None,
                "dsn2": dsn2}

    def _kid(self):
        return self.covariance._gpc_kernel_id, self.covariance._gpc_degree

    def _user_cov(self, hyp_cov, grad):
        """K (S,N,N) [and the per-sample dK (N,N,cov_N) arrays] from a user-defined covariance
        object's own ``compute`` (the reference's call at gaussian_process.py:2388-2390)."""
        Ks, dKs = [], []
        for h in hyp_cov:
            if grad:
                K, dK = self.covariance.compute(h, self.X, compute_grad=True)
                dKs.append(np.asarray(dK, dtype=float))
            else:
                K = self.covariance.compute(h, self.X)
            Ks.append(np.asarray(K, dtype=float))
        return np.stack(Ks), dKs

    # ------------------------------------------------------------------ core (batched)
    def nll_batch(self, hyp: np.ndarray, compute_grad: bool = False):
        """Negative log marginal likelihood (and gradient) for MANY hyperparameter
        vectors at once: ``hyp`` (S, hyp_N) -> nlZ (S,), dnlZ (S, hyp_N) | None.

        Equivalent to S calls of the reference's ``__core_computation(hyp, 1, grad)``
        (gaussian_process.py:2357-2512); raises ``LinAlgError`` if any sample is
        still not positive definite after the 10 jitter escalations.  Under an initialised
        process group (and S > 1) the rows are sharded over the ranks and all-gathered: every
        rank returns -- or raises -- the same thing.
        """
        hyp = np.atleast_2d(np.asarray(hyp, dtype=float))
        cov_N, noise_N, mean_N = self._counts()
        hyp_N = cov_N + noise_N + mean_N
        if hyp.shape[1] != hyp_N:
            raise ValueError("Input hyperparameter array is the wrong shape!")
        S = hyp.shape[0]
        C = 1 + (hyp_N if compute_grad else 0)

        counts = (cov_N, noise_N, mean_N)  # (once per call: three plugin calls each, on the path of every evaluation)

        def local(lo, hi):
            nlz, dnlz, info = self._nll_batch_local(hyp[lo:hi], compute_grad, counts)
            rows = nlz[:, None] if not compute_grad else np.concatenate([nlz[:, None], dnlz], axis=1)
            return rows, info != 0

        if self.shard and S > 1 and _sh.active_group(self.process_group) is not None:
            full, bad = _sh.gather_rows(S, C, local, self.process_group, _sh.fingerprint(hyp))
        else:
            full, bad = local(0, S)
        if np.any(bad):
            raise LinAlgError("Singular matrix for L Cholesky decomposition")
        return full[:, 0].copy(), (full[:, 1:].copy() if compute_grad else None)

    @_on_device
    def _nll_batch_local(self, hyp, compute_grad, counts=None):
        """This rank's evaluation of the rows of ``hyp``: nlZ, dnlZ | None, info (no exception for a
        failed sample: the caller decides, after the exchange when sharded)."""
        cov_N, noise_N, mean_N = counts = counts or self._counts()
        ctx = self._ctx()
        if self._builtin and self._const_mean():
            # the stock zero / constant mean: one value per sample crosses the boundary (gpc_nll_batch_cm), not an
            # (S, N) array of copies of it and an (S, N, 1) array of ones -- same results, to the bit
            sn2, dsn2, vec = self._noise_values(hyp, compute_grad, counts)
            kid, deg = self._kid()
            m0 = hyp[:, cov_N + noise_N] if mean_N == 1 else None
            nlz, dnlz, mult, lchol, info = ctx.nll_batch_cm(
                kid, deg, _DTYPES[self.dtype], hyp[:, :cov_N], m0, sn2, vec, compute_grad, dsn2)
            return nlz, dnlz, info
        pv = self._plugin_values(hyp, compute_grad)
        if self._builtin:
            kid, deg = self._kid()
            nlz, dnlz, mult, lchol, info = ctx.nll_batch(
                kid, deg, _DTYPES[self.dtype], hyp[:, :cov_N], pv["m"], pv["sn2"], pv["vec"],
                compute_grad, pv["dm"], pv["dsn2"])
        else:
            K, dK = self._user_cov(hyp[:, :cov_N], compute_grad)
            nlz, dnlz, mult, lchol, info = ctx.nll_batch_K(
                _DTYPES[self.dtype], K, (lambda s, p: dK[s][:, :, p]) if compute_grad else None, cov_N,
                pv["m"], pv["sn2"], pv["vec"], compute_grad, pv["dm"], pv["dsn2"])
        return nlz, dnlz, info

    def __compute_nlZ(self, hyp, compute_grad, compute_prior):
        """Reference gaussian_process.py:1520-1538 (single hyperparameter vector)."""
        hyp = np.asarray(hyp, dtype=float)
        nlz, dnlz = self.nll_batch(hyp[None, :], compute_grad)
        nlZ = float(nlz[0])
        dnlZ = dnlz[0] if compute_grad else None
        if compute_prior:
            if compute_grad:
                P, dP = self.__compute_log_priors(hyp, True)
                nlZ -= P
                dnlZ -= dP
            else:
                nlZ -= self.__compute_log_priors(hyp, False)
        if compute_grad:
            return nlZ, dnlZ
        return nlZ

    def __gp_obj_fun(self, hyp, compute_grad, swap_sign):
        """Reference :1540-1559: nlZ minus log prior (when priors are set), optional sign swap."""
        r = self.__compute_nlZ(hyp, compute_grad, self.no_prior is not True)
        if compute_grad:
            nlZ, dnlZ = r
            return (-nlZ, -dnlZ) if swap_sign else (nlZ, dnlZ)
        return -r if swap_sign else r

    def _obj_batch(self, hyp, compute_grad=False):
        """Batched ``__gp_obj_fun(hyp, compute_grad, False)`` over the rows of ``hyp``."""
        hyp = np.atleast_2d(np.asarray(hyp, dtype=float))
        nlz, dnlz = self.nll_batch(hyp, compute_grad)
        nlz = nlz.copy()
        if self.no_prior is not True and hyp.shape[0] > 8:
            # every row's prior in one vectorised pass (bit-identical to the row loop: priors.log_priors_rows)
            P, dP = _pr.log_priors_rows(hyp, self.hyper_priors, self.lower_bounds, self.upper_bounds,
                                        self.normalization_constants, compute_grad)
            nlz -= P
            if compute_grad:
                dnlz -= dP
        elif self.no_prior is not True:
            for s in range(hyp.shape[0]):
                if compute_grad:
                    P, dP = self.__compute_log_priors(hyp[s], True)
                    nlz[s] -= P
                    dnlz[s] -= dP
                else:
                    nlz[s] -= self.__compute_log_priors(hyp[s], False)
        return (nlz, dnlz) if compute_grad else nlz

    def _neg_obj_rows(self, hyp):
        """One device batch for the rows of ``hyp``; returns row -> ``__gp_obj_fun(hyp[row], False, True)``, the log
        prior of a row being evaluated when (and only if) the row is asked for."""
        hyp = np.atleast_2d(np.asarray(hyp, dtype=float))
        nlz, _ = self.nll_batch(hyp, False)

        def value(k):
            v = float(nlz[k])
            if self.no_prior is not True:
                v -= self.__compute_log_priors(hyp[k], False)
            return -v

        return value

    # ------------------------------------------------------------------ bounds and priors
    def _hyp_N(self):
        return sum(self._counts())

    def set_bounds(self, bounds: dict = None):
        """Reference :147-210.  ``None`` entries (or ``bounds=None``) mean "not set" (NaN);
        ``fit`` replaces those by the recommended bounds."""
        lower = np.full((self._hyp_N(),), np.nan)
        upper = np.full((self._hyp_N(),), np.nan)
        i = 0
        for name, cnt in self._hyper_info():
            vals = None
            if bounds is not None:
                if name not in bounds:
                    raise ValueError("Missing hyperparameter " + name)
                vals = bounds[name]
            if vals is not None:
                lower[i:i + cnt], upper[i:i + cnt] = vals
            i += cnt
        self.lower_bounds, self.upper_bounds = lower, upper
        if self.no_prior is not None:
            self.__recompute_normalization_constants()

    def bounds_to_dict(self, lower_bounds: np.ndarray, upper_bounds: np.ndarray):
        """Reference :224-258."""
        out, i = {}, 0
        for name, cnt in self._hyper_info():
            out[name] = (lower_bounds[i:i + cnt], upper_bounds[i:i + cnt])
            i += cnt
        return out

    def get_bounds(self):
        return self.bounds_to_dict(self.lower_bounds, self.upper_bounds)

    def get_recommended_bounds(self, lower_bounds=None, upper_bounds=None):
        """Reference :260-359: NaN entries are filled from the plugins' ``get_bounds_info``."""
        if self.X is None or self.y is None:
            raise ValueError("GP does not have X or y set!")

        def resolve(v, current):
            if isinstance(v, (list, tuple, np.ndarray)):
                return np.array(v, dtype=float).copy()
            if v == "current":
                return current.copy()
            if v is None or v == "recommended":
                return np.full_like(current, np.nan)
            raise ValueError("`lower_bounds` should be 'recommended'/`None`, 'current', or an array.")

        lb = resolve(lower_bounds, self.lower_bounds)
        ub = resolve(upper_bounds, self.upper_bounds)
        info = [self.covariance.get_bounds_info(self.X, self.y),
                self.noise.get_bounds_info(self.X, self.y),
                self.mean.get_bounds_info(self.X, self.y)]
        rec_lb = np.concatenate([d["LB"] for d in info])
        rec_ub = np.concatenate([d["UB"] for d in info])
        lb = np.where(np.isnan(lb), rec_lb, lb)
        ub = np.where(np.isnan(ub), rec_ub, ub)
        ub = np.maximum(lb, ub)
        return self.bounds_to_dict(lb, ub)

    def set_priors(self, priors: dict = None):
        """Reference :418-514.  ``priors[name] = (type, params)`` with type one of
        'gaussian' (mu, sigma), 'student_t' (mu, sigma, df), 'smoothbox' (a, b, sigma),
        'smoothbox_student_t' (a, b, sigma, df); ``None`` = no prior."""
        hp = _pr.empty_priors(self._hyp_N())
        any_prior = False
        i = 0
        for name, cnt in self._hyper_info():
            vals = None
            if priors is not None:
                if name not in priors:
                    raise ValueError("Missing hyperparameter " + name)
                vals = priors[name]
            if vals is not None:
                any_prior = True
                kind, params = vals
                sl = slice(i, i + cnt)
                if kind == "gaussian":
                    hp["mu"][sl], hp["sigma"][sl] = params
                    hp["df"][sl] = 0
                elif kind == "student_t":
                    hp["mu"][sl], hp["sigma"][sl], hp["df"][sl] = params
                elif kind == "smoothbox":
                    hp["a"][sl], hp["b"][sl], hp["sigma"][sl] = params
                    hp["df"][sl] = 0
                elif kind == "smoothbox_student_t":
                    hp["a"][sl], hp["b"][sl], hp["sigma"][sl], hp["df"][sl] = params
                else:
                    raise ValueError("Unknown hyperprior type " + kind)
            i += cnt
        self.hyper_priors = hp
        self.no_prior = not any_prior
        self.__recompute_normalization_constants()

    def get_priors(self):
        """Reference :361-416."""
        hp = self.hyper_priors
        out, i = {}, 0
        for name, cnt in self._hyper_info():
            sl = slice(i, i + cnt)
            mu, sigma, df, a, b = (hp[k][sl] for k in ("mu", "sigma", "df", "a", "b"))
            val = None
            if np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(np.isfinite(sigma)):
                if np.all((df == 0) | (df == np.inf)):
                    val = ("smoothbox", (a.copy(), b.copy(), sigma.copy()))
                elif np.all(df > 0):
                    val = ("smoothbox_student_t", (a.copy(), b.copy(), sigma.copy(), df.copy()))
            elif np.all(np.isfinite(mu)) and np.all(np.isfinite(sigma)):
                if np.all((df == 0) | (df == np.inf)):
                    val = ("gaussian", (mu.copy(), sigma.copy()))
                elif np.all(df > 0):
                    val = ("student_t", (mu.copy(), sigma.copy(), df.copy()))
            out[name] = val
            i += cnt
        return out

    def __recompute_normalization_constants(self):
        self.normalization_constants = _pr.normalization_constants(
            self.hyper_priors, self.lower_bounds, self.upper_bounds)

    def __compute_log_priors(self, hyp: np.ndarray, compute_grad: bool):
        return _pr.log_priors(hyp, self.hyper_priors, self.lower_bounds, self.upper_bounds,
                              self.normalization_constants, compute_grad)

    # ------------------------------------------------------------------ fit
    def fit(self, X=None, y=None, s2=None, hyp0=None, options: dict = None):
        """Train the hyperparameters (reference :910-1232): space-filling design ->
        multi-start L-BFGS-B -> slice sampling -> posteriors.

        Same options and defaults as the reference.  What changes is how the core is
        called: the design (``init_N`` = 1024 evaluations by default) is ONE device batch,
        the ``opts_N`` optimisers advance in lock-step with their NLL+gradient requests
        batched per iteration (each trajectory is unchanged: it only sees its own values),
        the slice-sampling chain stays sequential, and the final posteriors are one batch.
        """
        o = dict(_FIT_DEFAULTS, **(options or {}))  # the reference's option names and defaults (:991-1006)
        opts_N, init_N, init_method, thin, s_N = o["opts_N"], o["init_N"], o["init_method"], o["thin"], o["n_samples"]
        df_base, widths, sampler_name = o["df_base"], o["widths"], o["sampler"]
        tol_opt, tol_opt_mcmc = o["tol_opt"], o["tol_opt_mcmc"]
        lower_bounds, upper_bounds = o["lower_bounds"], o["upper_bounds"]
        burn_in = o["burn"] if "burn" in (options or {}) else thin * s_N
        options = o

        for name, value in zip(("X", "y", "s2"), self._convert_shapes(X, y, s2)):
            if value is not None:  # data given to fit replace what the GP holds (:1011-1017)
                setattr(self, name, value)
        cov_N, noise_N, _ = self._counts()

        info = [self.covariance.get_bounds_info(self.X, self.y),
                self.noise.get_bounds_info(self.X, self.y),
                self.mean.get_bounds_info(self.X, self.y)]
        self.hyper_priors["df"][np.isnan(self.hyper_priors["df"])] = df_base

        current = (isinstance(lower_bounds, str) and lower_bounds == "current"
                   and isinstance(upper_bounds, str) and upper_bounds == "current")
        if current and (np.any(np.isnan(self.lower_bounds)) or np.any(np.isnan(self.upper_bounds))):
            self.set_bounds(self.get_recommended_bounds(self.lower_bounds, self.upper_bounds))
        else:
            self.set_bounds(self.get_recommended_bounds(lower_bounds, upper_bounds))
        LB, UB = self.lower_bounds, self.upper_bounds
        PLB = np.concatenate([d["PLB"] for d in info])
        PUB = np.concatenate([d["PUB"] for d in info])
        PLB = np.minimum(np.maximum(PLB, LB), UB)
        PUB = np.maximum(np.minimum(PUB, UB), LB)

        if hyp0 is None:
            if self.posteriors is not None:
                hyp0 = self.get_hyperparameters(as_array=True)
            else:
                hyp0 = np.reshape(np.minimum(np.maximum((PLB + PUB) / 2, LB), UB), (1, -1))
        elif isinstance(hyp0, dict):
            hyp0 = self.hyperparameters_from_dict(hyp0)
        hyp0 = np.atleast_2d(hyp0)

        tol = tol_opt_mcmc if (s_N > 0 and sampler_name != "laplace") else tol_opt

        # 1. objective on the space-filling design: one batch (reference :1096-1130)
        if init_N > 0:
            X0, y0 = f_min_fill(lambda Xd: self._obj_batch(Xd, False), hyp0, LB, UB, PLB, PUB,
                                self.hyper_priors, init_N, init_method)
            hyp = X0[0:np.maximum(opts_N, 1), :]
            if noise_N > 0 and 1 < opts_N < init_N:  # a good low-noise start for run #2
                xx, noise_y = X0[opts_N:, :], y0[opts_N:]
                order = np.argsort(xx[:, cov_N])
                xx, noise_y = xx[order, :], noise_y[order]
                idx_best = np.argmin(noise_y[0:math.ceil(0.2 * np.size(noise_y))])
                hyp[1, :] = xx[idx_best, :]
            widths_default = np.std(X0, axis=0, ddof=1) if init_N > 1 else np.zeros(shape=PLB.shape)
        else:
            nll = np.asarray(self._obj_batch(hyp0, False))
            hyp = hyp0[np.argsort(nll), :]
            widths_default = PUB - PLB

        idx0 = widths_default == 0
        if np.any(idx0):
            if np.shape(hyp)[0] > 1:
                widths_default[idx0] = np.std(hyp, axis=0, ddof=1)[idx0]
                idx0 = widths_default == 0
            if np.any(idx0):
                widths_default[idx0] = np.minimum(1, UB[idx0] - LB[idx0])

        # starts go strictly inside the box: one ulp off every finite bound of a free coordinate (:1152-1163)
        free = LB != UB
        inner_lo = np.where(free & np.isfinite(LB), np.nextafter(LB, np.inf), LB)
        inner_hi = np.where(free & np.isfinite(UB), np.nextafter(UB, -np.inf), UB)
        hyp = np.minimum(inner_hi[None, :], np.maximum(inner_lo[None, :], hyp))

        # 2. multi-start L-BFGS-B, starts in lock-step (reference :1177-1187)
        nll = np.full((np.maximum(opts_N, 1),), np.inf)
        opts_N = int(np.minimum(opts_N, hyp.shape[0]))
        opt_results = self._minimize_lockstep(hyp[:opts_N], LB, UB, tol)
        for i, res in enumerate(opt_results):
            hyp[i, :] = res.x
            nll[i] = res.fun
        if opts_N > 0:
            optimize_result = opt_results[int(np.argmin(nll))]
            hyp_start = hyp[int(np.argmin(nll)), :].copy()
        else:
            optimize_result = None
            hyp_start = hyp[0, :].copy()

        if s_N == 0:
            hyp_start = np.reshape(hyp_start, (1, -1))
            self.update(hyp=hyp_start)
            return hyp_start, optimize_result, None

        # 3. slice sampling from the best optimum: a sequential chain (reference :1205-1225)
        if sampler_name != "slicesample":
            raise ValueError("Unknown sampler!")
        widths = widths_default if widths is None else np.minimum(widths, widths_default)
        # (the shrinkage proposals of a coordinate are evaluated several at a time, see slice_sample.py; the chain is
        # the sequential sampler's.  Measured: 8 per batch up to N = 1000, 6 beyond -- tools/fit_time.py)
        slicer = SliceSampler(lambda h: self.__gp_obj_fun(h, False, True), hyp_start, widths, LB, UB,
                              {"display": "off", "diagnostics": False,
                               "log_f_batch": self._neg_obj_rows,
                               "speculate": int(options.get("slice_speculate", 8 if self.X.shape[0] <= 1024 else 6))})
        sampling_result = slicer.sample(s_N * thin, burn=burn_in)
        hyp = sampling_result["samples"][thin - 1::thin, :]

        # 4. posteriors for the retained samples: one batch (reference :1231)
        self.update(hyp=hyp)
        return hyp, optimize_result, sampling_result

    def _minimize_lockstep(self, starts, LB, UB, tol):
        """Run one ``scipy.optimize.minimize`` (L-BFGS-B) per start, each in its own thread;
        their objective calls meet at a rendezvous that evaluates all pending requests as ONE
        ``_obj_batch`` call.  Every optimiser sees exactly the values it would see alone."""
        n = starts.shape[0]
        if n == 0:
            return []
        bounds = list(zip(LB, UB))
        if n == 1:
            f = lambda h: self.__gp_obj_fun(h, True, False)
            return [scipy.optimize.minimize(fun=f, x0=starts[0], jac=True, bounds=bounds, tol=tol)]

        cv = threading.Condition()
        state = {"active": n, "pending": {}, "results": {}, "error": None, "gen": 0}

        def flush():  # caller holds cv
            ids = sorted(state["pending"])
            xs = np.stack([state["pending"][i] for i in ids])
            state["pending"].clear()
            try:
                vals, grads = self._obj_batch(xs, True)
                for k, i in enumerate(ids):
                    state["results"][i] = (float(vals[k]), grads[k].copy())
            except Exception as e:  # noqa: BLE001 - re-raised in every waiting optimiser
                state["error"] = e
            state["gen"] += 1
            cv.notify_all()

        def objective(i, x):
            with cv:
                if state["error"] is not None:
                    raise state["error"]
                state["pending"][i] = np.array(x, dtype=float)
                if len(state["pending"]) == state["active"]:
                    flush()
                else:
                    gen = state["gen"]
                    while state["gen"] == gen:
                        cv.wait()
                if state["error"] is not None:
                    raise state["error"]
                return state["results"].pop(i)

        out, errs = [None] * n, [None] * n

        def worker(i):
            try:
                out[i] = scipy.optimize.minimize(fun=lambda x: objective(i, x), x0=starts[i], jac=True,
                                                 bounds=bounds, tol=tol)
            except Exception as e:  # noqa: BLE001
                errs[i] = e
            finally:
                with cv:
                    state["active"] -= 1
                    if state["active"] > 0 and len(state["pending"]) == state["active"]:
                        flush()

        threads = [threading.Thread(target=worker, args=(i,)) for i in range(n)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for e in errs:
            if e is not None:
                raise e
        return out

    def log_likelihood(self, hyp: object, compute_grad: bool = False):
        """(Positive) log marginal likelihood (reference :1468-1488).  With
        ``compute_grad`` the reference negates a tuple (a TypeError); here the pair
        (lZ, dlZ) is returned."""
        if isinstance(hyp, dict):
            hyp = self.hyperparameters_from_dict(hyp)[0]
        r = self.__compute_nlZ(np.asarray(hyp, dtype=float).ravel(), compute_grad, False)
        if compute_grad:
            return -r[0], -r[1]
        return -r

    def log_posterior(self, hyp: object, compute_grad: bool = False):
        """Log marginal likelihood plus log prior (reference :1490-1518)."""
        if isinstance(hyp, dict):
            hyp = self.hyperparameters_from_dict(hyp)[0]
        r = self.__compute_nlZ(np.asarray(hyp, dtype=float).ravel(), compute_grad, True)
        if compute_grad:
            return -r[0], -r[1]
        return -r

    # ------------------------------------------------------------------ curvature of the objective
    def _nll_hess_check(self, who):
        """The refusals of the marginal-likelihood Hessian that need no device."""
        from . import _nllhess as _nh
        from .mean_functions import ConstantMean, NegativeQuadratic, ZeroMean
        from .noise_functions import GaussianNoise

        if not self._builtin:
            raise NotImplementedError(f"{who}: the covariance function {self.covariance!r} is user-defined; its second "
                                      "derivatives with respect to the hyperparameters are unknown")
        if self.dtype != "f64":
            raise NotImplementedError(f"{who}: the Hessian is computed in fp64 only; this GP's dtype is {self.dtype!r}")
        _nh.check_kind(*self._kid(), who=who)
        if type(self.noise) is not GaussianNoise:
            raise NotImplementedError(f"{who}: the noise function {self.noise!r} ({type(self.noise).__name__}) is "
                                      "user-defined; its second derivatives with respect to the hyperparameters are unknown")
        if type(self.mean) not in (ZeroMean, ConstantMean, NegativeQuadratic):
            raise NotImplementedError(f"{who}: the mean function {self.mean!r} ({type(self.mean).__name__}) is "
                                      "user-defined; its second derivatives with respect to the hyperparameters are unknown")

    def nll_hess_batch(self, hyp=None):
        """Negative log marginal likelihood, its gradient and its HESSIAN with respect to the hyperparameters for many
        hyperparameter vectors: ``hyp`` (S, hyp_N) -> nlZ (S,), dnlZ (S, hyp_N), H (S, hyp_N, hyp_N), ordered
        [cov | noise | mean] as ``nll_batch``'s gradient.  Every H[s] is symmetric to the bit.

        ``hyp=None`` uses the resident posteriors (appended points included); otherwise temporary posteriors are built
        for ``hyp`` and freed.  The closed form (``_nllhess``) runs on the device (gpc_nll_hess) at each sample's own
        jitter multiplier, held fixed; the second derivatives of the noise and mean functions are added here.  dnlZ
        comes from the same sums and equals ``nll_batch``'s to rounding.

        Built-in covariance functions, the stock ``GaussianNoise`` and the stock mean functions in float64 only
        (NotImplementedError otherwise, naming the reason); the Matern kernel of degree 1 has no second derivative.
        Under a process group the call is NOT sharded: it runs on the calling rank alone, whatever the others do, and
        exchanges nothing (resident posteriors that are sharded are rebuilt locally as temporaries)."""
        self._nll_hess_check("nll_hess_batch")
        return self._nll_hess_local(hyp)

    @_on_device
    def _nll_hess_local(self, hyp):
        """``nll_hess_batch`` after its refusals: this rank's device call and the plugin terms."""
        from . import _nllhess as _nh

        cov_N, noise_N, mean_N = counts = self._counts()
        resident = hyp is None
        if resident:
            self._require_posteriors()
            hyp = np.stack([p.hyp for p in self.posteriors])
            resident = self._post_range is None and self._post_handle is not None
        hyp = np.atleast_2d(np.asarray(hyp, dtype=float))
        if hyp.shape[1] != cov_N + noise_N + mean_N:
            raise ValueError("Input hyperparameter array is the wrong shape!")
        S = hyp.shape[0]
        ctx = self._ctx()
        pv = self._plugin_values(hyp, True)
        kid, deg = self._kid()
        if resident:
            handle = self._post_handle
            mult = np.array([float(_sn2_mult(p)) for p in self.posteriors])
        else:
            handle, mult, _, info = ctx.posterior_batch(kid, deg, _DTYPES[self.dtype], hyp[:, :cov_N], pv["m"], pv["sn2"],
                                                        pv["vec"])
            if np.any(info != 0):
                handle.free()
                raise LinAlgError("Singular matrix for L Cholesky decomposition")
        try:
            H, g, alpha, diagq = handle.nll_hess(cov_N, pv["dm"], pv["dsn2"])
        finally:
            if not resident:
                handle.free()
        for s in range(S):
            if noise_N:
                d2 = _nh.noise_d2(self.noise, hyp[s, cov_N:cov_N + noise_N], self.X, self.y, self.s2)
                H[s, cov_N:cov_N + noise_N, cov_N:cov_N + noise_N] += 0.5 * mult[s] * np.einsum(
                    "a,anm->nm", diagq[s], np.broadcast_to(d2, (diagq.shape[1],) + d2.shape[1:]))
            if mean_N:
                d2 = _nh.mean_d2(self.mean, _mean_hyp(hyp[s], counts), self.X)
                H[s, cov_N + noise_N:, cov_N + noise_N:] -= np.einsum("a,akl->kl", alpha[s], d2)
        nlz, _, info = self._nll_batch_local(hyp, False, counts)
        if np.any(info != 0):
            raise LinAlgError("Singular matrix for L Cholesky decomposition")
        return nlz, g, H

    def log_posterior_hess(self, hyp):
        """Value, gradient and Hessian of ``log_posterior`` at ONE hyperparameter vector (array or dict), the prior
        terms included (the four prior families are products over the dimensions: a diagonal), in ``log_posterior``'s
        sign convention.  A fixed dimension (lower bound = upper bound) carries NaN, as in the gradient."""
        from . import _nllhess as _nh

        if isinstance(hyp, dict):
            hyp = self.hyperparameters_from_dict(hyp)[0]
        hyp = np.asarray(hyp, dtype=float).ravel()
        nlz, g, H = self.nll_hess_batch(hyp[None, :])
        val, grad, hess = -float(nlz[0]), -g[0], -H[0]
        if self.no_prior is not True:
            lp, dlp = self.__compute_log_priors(hyp, True)
            d2 = _nh.prior_d2(hyp, self.hyper_priors, self.lower_bounds, self.upper_bounds)
            val, grad = val + lp, grad + dlp
            hess[np.diag_indices_from(hess)] += d2
        return val, grad, hess

    def laplace_approximation(self, hyp=None, free=None):
        """The Laplace approximation of the hyperparameter posterior at ``hyp`` (default: the first resident sample,
        e.g. the MAP that ``fit`` left): a dict with

            mean          ``hyp``
            hess          the Hessian of the NEGATIVE log posterior over the free coordinates
            cov           its inverse, or None
            is_pd         whether ``hess`` is positive definite (a Cholesky factorization succeeds)
            log_evidence  log p(y) ~ log posterior(hyp) + k/2 log 2 pi - 1/2 log det hess, k free coordinates; None
                          when ``hess`` is not positive definite
            free          the indices of the free coordinates

        ``free``: indices (or a boolean mask) of the coordinates the Gaussian lives on; by default all that are not
        fixed by the bounds.  ``hyp`` is taken as it is -- the caller vouches that it is a mode.  Nothing is repaired:
        when the Hessian is not positive definite (a ridge, a saddle, a point that is no mode), ``cov`` is None and
        ``is_pd`` False."""
        if hyp is None:
            self._require_posteriors()
            hyp = self.posteriors[0].hyp
        if isinstance(hyp, dict):
            hyp = self.hyperparameters_from_dict(hyp)[0]
        hyp = np.asarray(hyp, dtype=float).ravel().copy()
        val, _, hess = self.log_posterior_hess(hyp)
        if free is None:
            lb, ub = self.lower_bounds, self.upper_bounds
            fixed = np.zeros(hyp.size, bool) if lb is None or ub is None else np.asarray(lb) == np.asarray(ub)
            free = np.flatnonzero(~fixed)
        else:
            free = np.asarray(free)
            free = np.flatnonzero(free) if free.dtype == bool else free.astype(int)
        A = -hess[np.ix_(free, free)]
        out = dict(mean=hyp, hess=A, cov=None, is_pd=False, log_evidence=None, free=free)
        if free.size and np.all(np.isfinite(A)):
            try:
                L = np.linalg.cholesky(A)
            except LinAlgError:
                return out
            Li = np.linalg.solve(L, np.eye(free.size))
            out.update(cov=Li.T @ Li, is_pd=True,
                       log_evidence=val + 0.5 * free.size * np.log(2 * np.pi) - np.sum(np.log(np.diag(L))))
        return out

    # ------------------------------------------------------------------ cross-validation objective
    def _cv_grad_check(self, who, loss="lpd", weights=None):
        """The refusals of the cross-validation objective that need no device.  Returns ``weights`` as a float64
        vector (None stays None)."""
        from . import _cvgrad as _cg
        from .mean_functions import ConstantMean, NegativeQuadratic, ZeroMean
        from .noise_functions import GaussianNoise

        if not self._builtin:
            raise NotImplementedError(f"{who}: the covariance function {self.covariance!r} is user-defined; its "
                                      "derivatives with respect to the hyperparameters are not available on the device")
        if self.dtype != "f64":
            raise NotImplementedError(f"{who}: the cross-validation objective is computed in fp64 only; this GP's dtype "
                                      f"is {self.dtype!r}")
        _cg.check_kind(*self._kid(), who=who)
        if type(self.noise) is not GaussianNoise:
            raise NotImplementedError(f"{who}: the noise function {self.noise!r} ({type(self.noise).__name__}) is "
                                      "user-defined; only the stock GaussianNoise is served")
        if type(self.mean) not in (ZeroMean, ConstantMean, NegativeQuadratic):
            raise NotImplementedError(f"{who}: the mean function {self.mean!r} ({type(self.mean).__name__}) is "
                                      "user-defined; only the stock mean functions are served")
        _cg.check_loss(loss, who)
        return _cg.check_weights(weights, None if self.X is None else self.X.shape[0], who)

    def cv_nll_batch(self, hyp=None, compute_grad: bool = True, loss: str = "lpd", weights=None):
        """The leave-one-out cross-validation objective and its gradient with respect to the hyperparameters for many
        hyperparameter vectors: ``hyp`` (S, hyp_N) -> L (S,), dL (S, hyp_N) | None, ordered [cov | noise | mean] as
        ``nll_batch``'s gradient.

        ``loss="lpd"``: L is the NEGATIVE leave-one-out log predictive density (Rasmussen & Williams 5.4.2; the negated
        sum of ``cv_predict(return_lpd=True)``'s single-point folds); ``loss="mse"``: the sum of squared leave-one-out
        residuals.  ``weights`` (N,), finite and >= 0, weighs the points (default 1).

        ``hyp=None`` uses the resident posteriors (appended points included); otherwise temporary posteriors are built
        for ``hyp`` and freed (LinAlgError when a factorization fails).  The closed form (``_cvgrad``) runs on the
        device (gpc_cv_grad) at each sample's own jitter multiplier, held fixed: all derivatives collapse onto one
        weight matrix, so value and gradient cost one N^3 product and one contraction pass whatever hyp_N is.  Without
        ``compute_grad`` the value comes from the leave-one-out pass of ``cv_predict`` (gpc_cv) and no product is
        launched; the two values agree to rounding, not to the bit.

        Built-in covariance functions, the stock ``GaussianNoise`` and the stock mean functions in float64 only
        (NotImplementedError otherwise, naming the reason); the Matern kernel of degree 1 is refused.  Under a process
        group the call is NOT sharded: it runs on the calling rank alone, whatever the others do, and exchanges nothing
        (resident posteriors that are sharded are rebuilt locally as temporaries)."""
        weights = self._cv_grad_check("cv_nll_batch", loss, weights)
        return self._cv_nll_local(hyp, compute_grad, loss, weights)

    @_on_device
    def _cv_nll_local(self, hyp, compute_grad, loss, weights):
        """``cv_nll_batch`` after its refusals: this rank's device call and the plugin columns."""
        from . import _cvgrad as _cg

        cov_N, noise_N, mean_N = self._counts()
        resident = hyp is None
        if resident:
            self._require_posteriors()
            hyp = np.stack([p.hyp for p in self.posteriors])
            resident = self._post_range is None and self._post_handle is not None
        hyp = np.atleast_2d(np.asarray(hyp, dtype=float))
        if hyp.shape[1] != cov_N + noise_N + mean_N:
            raise ValueError("Input hyperparameter array is the wrong shape!")
        S = hyp.shape[0]
        ctx = self._ctx()
        pv = self._plugin_values(hyp, bool(compute_grad))
        kid, deg = self._kid()
        if resident:
            handle = self._post_handle
            mult = np.array([float(_sn2_mult(p)) for p in self.posteriors])
        else:
            handle, mult, _, info = ctx.posterior_batch(kid, deg, _DTYPES[self.dtype], hyp[:, :cov_N], pv["m"], pv["sn2"],
                                                        pv["vec"])
            if np.any(info != 0):
                handle.free()
                raise LinAlgError("Singular matrix for L Cholesky decomposition")
        try:
            if not compute_grad:
                dmu, s2, _, _, info = handle.cv(None)  # (N, S): alpha / q and 1 / q
                if np.any(info != 0):
                    raise LinAlgError("cv_nll_batch: a leave-one-out variance is not positive in floating point")
                return _cg.loo_value((dmu / s2).T, (1 / s2).T, loss, weights), None
            gsum, diagG, beta, alpha, q, _ = handle.cv_grad(cov_N, loss, weights)
        finally:
            if not resident:
                handle.free()
        L = _cg.loo_value(alpha, q, loss, weights)
        dL = np.empty((S, hyp.shape[1]))
        for s in range(S):
            dL[s] = _cg.assemble(gsum[s], diagG[s], beta[s], mult[s], None if pv["dsn2"] is None else pv["dsn2"][s],
                                 None if pv["dm"] is None else pv["dm"][s])
        return L, dL

    def log_pseudo_likelihood(self, hyp, compute_grad: bool = False):
        """The leave-one-out log pseudo-likelihood (Rasmussen & Williams 5.4.2), the sum over the points of the log
        density of y_i under its leave-one-out prediction, at ONE hyperparameter vector (array or dict), in
        ``log_likelihood``'s sign convention: -L of ``cv_nll_batch(loss="lpd")``.  With ``compute_grad`` the pair
        (lpl, dlpl); negated, an objective for ``scipy.optimize``."""
        if isinstance(hyp, dict):
            hyp = self.hyperparameters_from_dict(hyp)[0]
        L, dL = self.cv_nll_batch(np.asarray(hyp, dtype=float).ravel()[None, :], compute_grad)
        if compute_grad:
            return -float(L[0]), -dL[0]
        return -float(L[0])

    # ------------------------------------------------------------------ hyperparameters
    def get_hyperparameters(self, as_array: bool = False):
        """Reference :516-552."""
        if self.posteriors is None:
            cov_N, noise_N, mean_N = self._counts()
            hyp = np.full((1, cov_N + mean_N + noise_N), np.nan)
        else:
            hyp = np.zeros((np.size(self.posteriors), np.size(self.posteriors[0].hyp)))
            for i in range(np.size(self.posteriors)):
                hyp[i, :] = self.posteriors[i].hyp.copy()
        if as_array:
            return hyp
        return self.hyperparameters_to_dict(hyp)

    def set_hyperparameters(self, hyp_new: object, compute_posterior: bool = True):
        """Reference :554-593."""
        if isinstance(hyp_new, np.ndarray):
            cov_N, noise_N, mean_N = self._counts()
            if hyp_new.ndim == 1:
                hyp_new = np.reshape(hyp_new, (1, -1))
            if hyp_new.shape[1] != cov_N + mean_N + noise_N:
                raise ValueError("Input hyperparameter array is the wrong shape!")
            self.update(hyp=hyp_new, compute_posterior=compute_posterior)
        else:
            self.update(hyp=self.hyperparameters_from_dict(hyp_new),
                        compute_posterior=compute_posterior)

    def _hyper_info(self):
        return (self.covariance.hyperparameter_info(self.D)
                + self.noise.hyperparameter_info()
                + self.mean.hyperparameter_info(self.D))

    def hyperparameters_to_dict(self, hyp_arr: np.ndarray):
        """Reference :595-647: order is [covariance | noise | mean]."""
        cov_N, noise_N, mean_N = self._counts()
        if hyp_arr.ndim == 1:
            hyp_arr = np.reshape(hyp_arr, (1, -1))
        if hyp_arr.shape[1] != cov_N + mean_N + noise_N:
            raise ValueError("Input hyperparameter array is the wrong shape!")
        out = []
        for r in range(hyp_arr.shape[0]):
            row = hyp_arr[r, :].copy()
            d, i = {}, 0
            for name, cnt in self._hyper_info():
                d[name] = row[i:i + cnt]
                i += cnt
            out.append(d)
        return out

    def hyperparameters_from_dict(self, hyp_dict_list):
        """Reference :649-689."""
        if isinstance(hyp_dict_list, dict):
            hyp_dict_list = [hyp_dict_list]
        cov_N, noise_N, mean_N = self._counts()
        arr = np.zeros((len(hyp_dict_list), cov_N + mean_N + noise_N))
        for r, d in enumerate(hyp_dict_list):
            j = 0
            for name, cnt in self._hyper_info():
                arr[r, j:j + cnt] = d[name]
                j += cnt
        return arr

    # ------------------------------------------------------------------ data / posterior
    def update(self, X_new=None, y_new=None, s2_new=None, hyp=None, compute_posterior: bool = True,
               block_append: bool = False):
        """Add data and/or replace hyperparameters, then rebuild every posterior
        (reference :691-884).  A single new observation (no ``s2``, no new ``hyp``, existing
        posteriors with scalar noise) takes the reference's rank-one path (:750-844) on the
        device in O(N^2): high-noise posteriors get a new last row of the factor, of its inverse
        and of alpha; low-noise posteriors the rank-one update of -inv (:819-827).  A posterior
        whose append is numerically unstable (``sqrt_arg <= 0``, :789-798) is recomputed alone,
        like the reference's ``full_updates``.  Anything else is the full recompute loop (:870-884).

        ``block_append=True`` asks for the same fast path for k >= 2 new observations in one call (the reference has
        none: it recomputes).  Where the rank-one path's other conditions hold -- resident posteriors, ``y_new``
        given, no ``s2``, no new ``hyp``, scalar noise, ``compute_posterior`` -- all k rows are appended to every
        resident posterior in one device call in O(S N^2 k) (``gpc_post_append_block``: the rank-one algebra with a
        k x k Schur block, factorized without jitter); a sample whose block is not positive definite is recomputed
        alone, the others keep their appended rows, and the posterior handle stays the same object.  Where they do
        not hold the call is the full recompute, silently; k = 1 is the rank-one path, same bits.  The result
        agrees with the full recompute to rounding (1e-8 relative in fp64), not to the bit, which is why it is a
        keyword and not the default.  Measured on an MI355X (``profiles/block_append_cfg3.json``, wall time): at
        N = 4096, S = 16 the block append is 3.0x / 2.5x faster than the full recompute at k = 5 / 128 and the two are
        level at k = 512 (k / N = 1/8); at N = 400, S = 8 it is about 2x faster for k = 5 .. 64 and the full recompute overtakes
        it from k = 128 on (k / N about 1/3, where the storage also has to grow by a tile).  Against k one-point
        updates it wins from k = 5 on; at k = 2 on the large problem two one-point updates are 1.3x faster."""
        X_new, y_new, s2_new = self._convert_shapes(X_new, y_new, s2_new)
        if X_new is not None:
            X_new = X_new.copy()
        if y_new is not None:
            y_new = y_new.copy()
        if s2_new is not None:
            s2_new = s2_new.copy()
        if hyp is not None:
            hyp = np.atleast_2d(np.asarray(hyp, dtype=float)).copy()
        if (hyp is not None and self.reference_quirks and X_new is not None and y_new is not None
                and compute_posterior and self.X is not None and self.y is not None and X_new.shape[0] == 1
                and y_new.shape[0] == 1 and s2_new is None and self.s2 is None and self.posteriors is not None):
            # the reference's rank-one test (:738-746) never looks at ``hyp``: the point is appended under the OLD
            # samples and the new hyperparameters are silently dropped
            hyp = None

        if X_new is not None and hyp is None:
            self._restore()  # (a copied GP: the rank-one path below extends RESIDENT posteriors)
        # the append path: one new row (the reference's rank-one path) or, under ``block_append``, k >= 2 rows at once
        append = (X_new is not None and y_new is not None and compute_posterior
                  and self.X is not None and self.y is not None
                  and (X_new.shape[0] == 1 or (block_append and X_new.shape[0] >= 2))
                  and y_new.shape[0] == X_new.shape[0] and s2_new is None and hyp is None
                  and self.s2 is None and self.posteriors is not None
                  and (self._post_handle is not None or self._post_range is not None))
        append_args = None
        if append:
            cov_N, noise_N, mean_N = self._counts()
            local_posts, first = self._local_posteriors()
            # per-point noise: the append formulas do not apply.  Decided on a record EVERY rank holds (a rank of a
            # sharded set may have no local posterior), so that all ranks take the same path
            if not np.isscalar(self.noise.compute(self.posteriors[0].hyp[cov_N:cov_N + noise_N], X_new, y_new, 0)):
                append, local_posts = False, []
            append_args = self._append_args(local_posts, X_new, y_new)

        if X_new is not None:
            self.X = X_new if self.X is None else np.concatenate((self.X, X_new))
        if y_new is not None:
            self.y = y_new if self.y is None else np.concatenate((self.y, y_new))
        if s2_new is not None:
            self.s2 = s2_new if self.s2 is None else np.concatenate((self.s2, s2_new))

        if append:
            self._append_points(local_posts, append_args, X_new, y_new)
            return

        if hyp is None:
            hyp = self.get_hyperparameters(as_array=True)
        s_N = hyp.shape[0]
        self._drop_handle()
        self.posteriors = np.empty((s_N,), dtype=Posterior)
        if compute_posterior and self.X is not None and self.y is not None:
            self._compute_posteriors(hyp)
        else:
            for i in range(s_N):
                self.posteriors[i] = Posterior(hyp[i, :], None, None, None, None, None)

    def _append_args(self, local_posts, X_new, y_new):
        """What the device's append entry points take for this rank's posteriors, evaluated on the data BEFORE the new
        rows are stored: (m_star, sn2_star, y_new), led by the cross covariances (Ks, kss | Kss) when the covariance is
        a user-defined object -- it supplies its own, like the reference's rank-one path does whatever the object is
        (gaussian_process.py:771-772).  One new row: scalars per sample (``append`` / ``append_K``); k rows: k-vectors
        and, for an object, Ks (S, n, k) and Kss (S, k, k) (``append_block`` / ``append_block_K``)."""
        cov_N, noise_N, _ = counts = self._counts()
        k = X_new.shape[0]
        one = k == 1
        m_star, sn2_star, Ks, kss = [], [], [], []
        for p in local_posts:
            h = p.hyp
            sn2_star.append(float(self.noise.compute(h[cov_N:cov_N + noise_N], X_new, y_new, 0)))
            m_new = np.ravel(self.mean.compute(_mean_hyp(h, counts), X_new))
            m_star.append(float(m_new[0]) if one else np.array(m_new, dtype=float))
            if not self._builtin:
                cross = np.asarray(self.covariance.compute(h[0:cov_N], self.X, X_new), dtype=float)
                Ks.append(np.ravel(cross) if one else cross.reshape(self.X.shape[0], k))
                if one:
                    kss.append(float(np.ravel(self.covariance.compute(h[0:cov_N], X_new, compute_diag=True))[0]))
                else:
                    kss.append(np.asarray(self.covariance.compute(h[0:cov_N], X_new), dtype=float).reshape(k, k))
        args = (m_star, sn2_star, float(y_new[0, 0]) if one else np.ravel(y_new).astype(float))
        if not self._builtin and local_posts:
            args = (np.stack(Ks), np.array(kss) if one else np.stack(kss)) + args
        return args

    @_on_device
    def _append_points(self, local_posts, append_args, X_new, y_new):
        """The append path (one new row: rank-one; k >= 2 rows under ``block_append``: one block append) on this
        rank's posteriors (all of them unless the set is sharded): append on the device,
        recompute alone the ones whose append is unstable (``sqrt_arg <= 0``, :789-798, :866-869), then -- under a
        process group -- exchange (sn2_mult, L_chol, failed) so that every rank updates its records or raises alike."""
        cov_N, _, _ = self._counts()
        S = self.posteriors.size

        def local(lo, hi):
            if not local_posts:
                return np.zeros((0, 2)), np.zeros(0, bool)
            self._ctx()  # uploads the extended X, y
            h = self._post_handle
            if X_new.shape[0] == 1:
                ok = h.append(*append_args) if self._builtin else h.append_K(*append_args)
            else:
                ok = h.append_block(*append_args) if self._builtin else h.append_block_K(*append_args)
            rows = np.array([[float(p.sn2_mult), float(p.L_chol)] for p in local_posts])
            bad = np.zeros(len(local_posts), bool)
            redo = np.flatnonzero(~ok)
            if redo.size:  # unstable for these posteriors only: full update of exactly those
                hyp_r = np.stack([local_posts[i].hyp for i in redo])
                pv = self._plugin_values(hyp_r, False)
                K = None if self._builtin else self._user_cov(hyp_r[:, :cov_N], False)[0]
                mult, lchol, info = h.recompute(redo, hyp_r[:, :cov_N], pv["m"], pv["sn2"], pv["vec"], K=K)
                rows[redo, 0], rows[redo, 1] = mult, lchol
                bad[redo] = info != 0
            return rows, bad

        if self._post_range is not None:
            full, bad = _sh.gather_rows(S, 2, local, self.process_group, _sh.fingerprint(X_new, y_new))
        else:
            full, bad = local(0, S)
        if np.any(bad):
            raise LinAlgError("Singular matrix for L Cholesky decomposition")
        for i, p in enumerate(self.posteriors):
            m = full[i, 0]
            p.sn2_mult = int(m) if m < 2**62 else m
            p.L_chol = bool(full[i, 1])
            p._alpha = p._sW = p._L = None  # cached host copies are stale; refetched lazily
            p._have = {"alpha": False, "sW": False, "L": False}

    def remove_points(self, idx, recompute: bool = False):
        """Drop training rows: ``idx`` is an integer array (negative values count from the end) or a boolean mask over
        the rows of ``X``; the rows leave ``X``, ``y`` and ``s2`` and every posterior is brought to the reduced data.

        With resident posteriors, scalar noise, no ``s2`` and no process group the rows are taken out of every
        resident posterior on the device in O(S N^2 k) (``gpc_post_remove``, the inverse of the block append: a blocked
        orthogonal sweep over the factor and its inverse for high-noise samples, from the 64-column panel that holds
        the first removed row on, and a rank-k correction of -inv for low-noise ones; no covariance is evaluated, so a
        user-defined covariance object takes the same path).  A sample whose k x k block is not positive definite is
        recomputed alone, and the posterior handle stays the same object.  The result agrees with the recompute to
        rounding (1e-8 relative in fp64), not to the bit.  Anything else -- and ``recompute=True`` -- is the full
        recompute on the reduced data, silently, as ``update``'s fallbacks are; so is a removal that would sweep more
        than one panel or that leaves at most 128 rows, because the device path as it stands LOSES to the recompute
        there.  Measured on an MI355X (``profiles/remove_points_cfg3.json``, wall time, device path / recompute): taking
        back the LAST rows (what a kriging-believer batch does with its fantasy observations) costs 2.4 / 14.2 ms at
        N = 4096, S = 16 for k = 1 .. 64 and 0.42 / 0.74 ms at N = 400, S = 8 (k = 5); dropping the FIRST rows would cost
        19.1 / 14.5 ms (k <= 16) to 78.0 / 13.4 ms (k = 128), and at N = 100 even the last rows cost 0.33 / 0.18 ms: both
        are therefore recomputed."""
        if self.X is None or self.y is None:
            raise ValueError("GP has no training data")
        idx = _rm.check_indices(idx, self.X.shape[0])
        keep = np.setdiff1d(np.arange(self.X.shape[0]), idx)
        self._restore()  # (a copied GP: the fast path shrinks RESIDENT posteriors)
        fast = (not recompute and self.s2 is None and self.posteriors is not None and self._post_handle is not None
                and self._post_range is None and _sh.active_group(self.process_group) is None)
        if fast:
            cov_N, noise_N, _ = self._counts()
            h0 = self.posteriors[0].hyp
            fast = bool(np.isscalar(self.noise.compute(h0[cov_N:cov_N + noise_N], self.X[keep], self.y[keep], 0)))
        fast = fast and self._remove_pays(idx)
        had_posteriors = self.posteriors is not None and any(p is not None and p.L_chol is not None for p in self.posteriors)
        self.X, self.y = self.X[keep].copy(), self.y[keep].copy()
        if self.s2 is not None:
            self.s2 = self.s2[keep].copy()
        if fast:
            self._remove_resident(idx)
            return
        if self.posteriors is None:
            return
        hyp = self.get_hyperparameters(as_array=True)
        s_N = hyp.shape[0]
        self._drop_handle()
        self.posteriors = np.empty((s_N,), dtype=Posterior)
        if had_posteriors:
            self._compute_posteriors(hyp)
        else:  # (records without posteriors, as update(compute_posterior=False) leaves them)
            for i in range(s_N):
                self.posteriors[i] = Posterior(hyp[i, :], None, None, None, None, None)

    def _remove_pays(self, idx):
        """Is this removal inside the limits within which the device path was measured to beat the full recompute
        (remove.h: a sweep of at most RM_SWEEP_MAX_PANELS panels, more than RM_MIN_KEPT_ROWS rows kept)?"""
        ctx = _lib.context(self.device)
        N = self.X.shape[0]
        return (N - idx.size > ctx.get_option("remove_min_rows")
                and _rm.swept_panels(N, idx) <= ctx.get_option("remove_max_panels"))

    @_on_device
    def _remove_resident(self, idx):
        """The fast path of ``remove_points`` (X, y hold the kept rows already): shrink on the device, recompute alone
        the samples it left stale, refresh the records the way ``_append_points`` does."""
        counts = self._counts()
        cov_N = counts[0]
        posts = list(self.posteriors)
        hyp = np.stack([p.hyp for p in posts])
        ym = np.ravel(self.y)[None, :] - np.reshape(self._plugin_values(hyp, False)["m"], (len(posts), -1))
        self._ctx()  # uploads the reduced X, y
        h = self._post_handle
        ok = h.remove(idx, ym)
        redo = np.flatnonzero(~ok)
        if redo.size:  # stale for these posteriors only: full update of exactly those
            pv = self._plugin_values(hyp[redo], False)
            K = None if self._builtin else self._user_cov(hyp[redo, :cov_N], False)[0]
            mult, lchol, info = h.recompute(redo, hyp[redo, :cov_N], pv["m"], pv["sn2"], pv["vec"], K=K)
            if np.any(info != 0):
                raise LinAlgError("Singular matrix for L Cholesky decomposition")
            for j, i in enumerate(redo):
                posts[i].sn2_mult = int(mult[j]) if mult[j] < 2**62 else mult[j]
                posts[i].L_chol = bool(lchol[j])
        for p in posts:
            p._alpha = p._sW = p._L = None  # cached host copies are stale; refetched lazily
            p._have = {"alpha": False, "sW": False, "L": False}

    @_on_device
    def _compute_posteriors(self, hyp, shard=None):
        """S x ``__core_computation(hyp, 0, 0)`` (reference :876-879) in one batch.  ``shard``: the caller's decision
        (``None``: this GP's ``shard`` attribute) -- an argument, so that a rank-local rebuild never flips an attribute
        other threads of the process read on their way into a collective.  Under a process
        group the samples are block-partitioned: this rank factors and keeps ONLY its block
        (``_post_range``); ``sn2_mult`` / ``L_chol`` of every sample are exchanged, the factors never are.
        ``Posterior.alpha/.sW/.L`` of a sample that lives on another rank read as ``None``."""
        cov_N, _, _ = self._counts()
        S = hyp.shape[0]
        made = {}

        def local(lo, hi):
            ctx = self._ctx()
            pv = self._plugin_values(hyp[lo:hi], False)
            if self._builtin:
                kid, deg = self._kid()
                handle, mult, lchol, info = ctx.posterior_batch(
                    kid, deg, _DTYPES[self.dtype], hyp[lo:hi, :cov_N], pv["m"], pv["sn2"], pv["vec"])
            else:
                K, _ = self._user_cov(hyp[lo:hi, :cov_N], False)
                handle, mult, lchol, info = ctx.posterior_batch_K(
                    _DTYPES[self.dtype], K, pv["m"], pv["sn2"], pv["vec"])
            made["handle"], made["lo"], made["hi"] = handle, lo, hi
            return np.stack([mult, lchol.astype(float)], axis=1), info != 0

        sharded = (self.shard if shard is None else shard) and S > 1 and _sh.active_group(self.process_group) is not None
        try:
            if sharded:
                full, bad = _sh.gather_rows(S, 2, local, self.process_group, _sh.fingerprint(hyp))
            else:
                full, bad = local(0, S)
        except Exception:
            if "handle" in made:
                made["handle"].free()
            raise
        if np.any(bad):
            if "handle" in made:
                made["handle"].free()
            raise LinAlgError("Singular matrix for L Cholesky decomposition")
        handle = made.get("handle")
        if sharded:  # (a rank with no sample of the set made no handle: its block is empty, at its place in the order)
            lo, hi = _sh.shard_bounds(S, *_sh.active_group(self.process_group))
        else:
            lo, hi = 0, S
        self._post_handle = handle
        self._post_range = (lo, hi, S) if sharded else None
        self._rebuild = False
        for i in range(S):
            m = full[i, 0]
            mine = handle is not None and lo <= i < hi
            self.posteriors[i] = Posterior(
                hyp[i, :], None, None, None, int(m) if m < 2**62 else m, bool(full[i, 1]),
                _handle=handle if mine else None, _index=(i - lo) if mine else None)

    def _local_posteriors(self):
        """The posterior records whose factors are resident on this rank (all of them unless sharded)."""
        if self._post_range is None:
            return list(self.posteriors), 0
        lo, hi, _ = self._post_range
        return list(self.posteriors[lo:hi]), lo

    def _gather_samples(self, local_cols, *args):
        """(R, S_local) per-sample columns of this rank -> (R, S) on every rank (no-op unless sharded).
        ``args``: the caller's arguments every rank must have passed identically (checked in the exchange)."""
        if self._post_range is None:
            return local_cols
        lo, hi, S = self._post_range
        R = local_cols.shape[0]
        full, _ = _sh.gather_rows(S, R, lambda a, b: (local_cols.T, np.zeros(b - a, bool)), self.process_group,
                                  _sh.fingerprint(*args))
        return full.T.copy()

    def _require_posteriors(self):
        """Every posterior consumer's first step: rebuild a copied GP's device posteriors, refuse a cleaned GP."""
        self._restore()
        if self._post_handle is None and self._post_range is None:
            raise ValueError("posteriors have been cleaned; call update() first")

    def _device_rows(self, call, layout, *key):
        """The per-sample row protocol of every posterior consumer: {name: array, all S samples on the last axis}.

        ``layout``: the ordered (name, shape) pairs of what the consumer computes per sample, shape without the
        sample axis -- (), (M,), (M, D), (M, D, D) ...; an output that a flag switches off is simply not listed.
        ``call(handle, local_posts, lo)`` runs only on a rank that holds samples and returns the arrays in the
        layout's order, sample axis last, for this rank's samples (global indices lo, lo + 1, ...); per-sample
        fix-ups of the local block belong inside it.  A rank without a sample contributes shape + (0,) zeros.
        Unsharded, what ``call`` returned is handed on as it is.  Sharded, the fields are stacked to (R, k) rows,
        exchanged in ONE all-gather and split again by the layout; ``key`` holds the arguments every rank must have
        passed identically (``ShardError`` otherwise)."""
        self._require_posteriors()
        self._ctx()
        local_posts, lo = self._local_posteriors()
        names = [n for n, _ in layout]
        if local_posts:
            fields = call(self._post_handle, local_posts, lo)
        else:
            fields = [np.zeros(tuple(shape) + (0,)) for _, shape in layout]
        if len(fields) != len(layout):
            raise ValueError(f"_device_rows: the call returned {len(fields)} arrays for the {len(layout)} of {names}")
        if self._post_range is None:
            return dict(zip(names, fields))
        k = len(local_posts)
        heights = [math.prod(shape) for _, shape in layout]
        rows = np.concatenate([np.reshape(f, (h, k)) for f, h in zip(fields, heights)], axis=0)
        rows = self._gather_samples(rows, *key)
        S, ends = rows.shape[1], np.cumsum(heights)
        return {n: rows[e - h:e].reshape(tuple(shape) + (S,)) for (n, shape), h, e in zip(layout, heights, ends)}

    def _noise_star(self, post, x_star, y_star, s2_star):
        """A sample's predictive noise at ``x_star``: the noise function's value times the record's multiplier."""
        cov_N, noise_N, _ = self._counts()
        return self.noise.compute(post.hyp[cov_N:cov_N + noise_N], x_star, y_star, s2_star) * _sn2_mult(post)

    def _drop_handle(self):
        self._rebuild = False
        if self._post_handle is not None:
            if self.posteriors is not None:
                for p in self.posteriors:
                    if p is not None:
                        p._detach()
            self._post_handle.free()
            self._post_handle = None
        self._post_range = None

    def clean(self):
        """Drop the auxiliary structures (reference :886-905); ``update`` rebuilds them."""
        self.temporary_data = {}
        if self.posteriors is not None:
            for p in self.posteriors:
                p.alpha = None
                p.sW = None
                p.L = None
                p.sn2_mult = None
                p.L_chol = None
        self._drop_handle()

    # ------------------------------------------------------------------ copies
    # The reference's GP is plain Python: its users copy.deepcopy() and pickle it (PyVBMC keeps copies of its GPs and
    # stores them with its results).  Here the posteriors live in HBM behind a handle that cannot be copied by value,
    # but they are a deterministic function of (X, y, s2, hyp): everything host-side travels with the copy, the device
    # posteriors are rebuilt on the copy's device when it first needs them (``_restore``; a set that grew by rank-one
    # appends is rebuilt by full factorizations, equal to rounding).  Fields already materialised on the host
    # (``Posterior.alpha/.sW/.L``) travel as they are, so a stored GP can be inspected on a machine without a GPU.
    def __getstate__(self):
        d = self.__dict__.copy()
        live = self._post_handle is not None or self._post_range is not None or d.get("_rebuild", False)
        d["_post_handle"] = None
        d["_post_range"] = None
        d["_token"] = None
        d["process_group"] = None  # a process group does not travel: the copy uses the default group
        if self.posteriors is not None:
            d["posteriors"] = [
                None if p is None else dict(hyp=p.hyp, sn2_mult=p.sn2_mult, L_chol=p.L_chol,
                                            alpha=p._alpha if p._have["alpha"] else None,
                                            sW=p._sW if p._have["sW"] else None, L=p._L if p._have["L"] else None)
                for p in self.posteriors]
        d["_rebuild"] = bool(live and self.posteriors is not None)
        # a set that was sharded over a process group is rebuilt collectively (every rank holds a copy and touches it);
        # anything else is rebuilt on the rank that touches it, with no collective: a stored GP opened by ONE rank of
        # a group must not wait in an all-gather for peers that never come
        d["_rebuild_sharded"] = self._post_range is not None or bool(
            self.__dict__.get("_rebuild") and self.__dict__.get("_rebuild_sharded"))  # (a copy of a copy not yet restored)
        return d

    def __setstate__(self, d):
        posts = d.pop("posteriors", None)
        self.__dict__.update(d)
        self.posteriors = None
        if posts is not None:
            self.posteriors = np.empty(len(posts), dtype=object)
            for i, t in enumerate(posts):
                if t is not None:
                    self.posteriors[i] = Posterior(t["hyp"], t["alpha"], t["sW"], t["L"], t["sn2_mult"], t["L_chol"],
                                                   _owner=self if self._rebuild else None)

    def __deepcopy__(self, memo):
        import copy

        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__setstate__(copy.deepcopy(self.__getstate__(), memo))
        new.process_group = self.process_group  # same process: same group
        return new

    def _restore(self):
        """Rebuild the device posteriors of a copied / unpickled GP from its hyperparameter samples.  The Posterior
        records handed out before keep their identity (and whatever they had materialised)."""
        if not self.__dict__.get("_rebuild", False):
            return
        self._rebuild = False
        old = self.posteriors
        self.posteriors = np.empty(old.size, dtype=object)
        # (rank-local unless the set was sharded; passed down, never toggled on the object: ADVICE r4)
        self._compute_posteriors(np.stack([p.hyp for p in old]),
                                 shard=self.shard and self.__dict__.get("_rebuild_sharded", False))
        for i, p in enumerate(old):
            q = self.posteriors[i]
            p._handle, p._index, p._owner = q._handle, q._index, None
            p.sn2_mult, p.L_chol = q.sn2_mult, q.L_chol
            self.posteriors[i] = p

    # ------------------------------------------------------------------ predict
    @_on_device
    def predict(self, x_star, y_star=None, s2_star=None, add_noise: bool = False,
                separate_samples: bool = False, return_lpd: bool = False):
        """Posterior mean and variance at ``x_star`` (reference :1663-1816).  The K*
        products and solves for all hyperparameter samples run in one device batch."""
        x_star, y_star, s2_star = self._convert_shapes(x_star, y_star, s2_star)
        s_N = self.posteriors.size
        N_star, D = x_star.shape
        cov_N, _, _ = counts = self._counts()
        if return_lpd and y_star is None:
            raise ValueError("Cannot calculate log predictive density without y_star.")

        mu = np.zeros((N_star, s_N))
        s2 = np.zeros((N_star, s_N))
        if self.y is not None:
            def call(handle, local_posts, lo):
                if self._builtin:
                    return handle.predict(x_star)
                # user-defined kernel: its own cross covariances, the solves on the device
                Ks = np.stack([self.covariance.compute(p.hyp[0:cov_N], self.X, x_star) for p in local_posts])
                kss = np.stack([self.covariance.compute(p.hyp[0:cov_N], x_star, compute_diag=True)[:, 0]
                                for p in local_posts], axis=1)
                fmu, fq, _ = handle.predict_K(Ks)
                return fmu, kss + fq

            fmu, fs2 = self._device_rows(call, [("fmu", (N_star,)), ("fs2", (N_star,))], x_star).values()
        y_s2 = np.zeros((N_star, s_N)) if (return_lpd or add_noise) else None
        lpd = np.zeros((N_star, s_N)) if (return_lpd and separate_samples) else None

        for s in range(s_N):
            hyp = self.posteriors[s].hyp
            m_star = np.reshape(self.mean.compute(_mean_hyp(hyp, counts), x_star), (-1,))
            if self.y is not None:
                mu[:, s] = m_star + fmu[:, s]
                s2[:, s] = fs2[:, s]
            else:
                mu[:, s] = m_star
                s2[:, s] = self.covariance.compute(hyp[0:cov_N], x_star, compute_diag=True)[:, 0]
            s2[:, s] = np.maximum(s2[:, s], 0)  # :1770
            if return_lpd or add_noise:
                y_s2[:, s:s + 1] = s2[:, s:s + 1] + self._noise_star(self.posteriors[s], x_star, y_star, s2_star)
            if return_lpd and separate_samples:
                lpd[:, s:s + 1] = -0.5 * (y_star - mu[:, s:s + 1]) ** 2 / y_s2[:, s:s + 1] \
                    - 0.5 * np.log(2 * np.pi * y_s2[:, s:s + 1])

        if add_noise:
            s2 = y_s2
        if not separate_samples:
            # the mixture over hyperparameter samples (:1789-1811): mean of the means; mean of the variances plus the
            # spread of the means; the density of y_star under that ONE Gaussian, with the noisy variance
            mu, s2, between = _mix_samples(mu, s2)
            if return_lpd:
                noisy = s2 if add_noise else np.reshape(np.sum(y_s2, 1) / s_N + between, (-1, 1))
                lpd = -0.5 * (y_star - mu) ** 2 / noisy - 0.5 * np.log(2 * np.pi * noisy)
        if return_lpd:
            return mu, s2, lpd
        return mu, s2

    # ------------------------------------------------------------------ cross-validation
    @_on_device
    def cv_predict(self, folds=None, add_noise: bool = False, separate_samples: bool = False,
                   return_lpd: bool = False):
        """Leave-fold-out predictions of the training targets from the resident posteriors, the hyperparameters held
        fixed (Rasmussen & Williams 5.4.2): what ``update`` on the data without a fold followed by ``predict`` at the
        fold returns, without refitting anything (gpc_cv; no covariance is evaluated, so user-defined kernels and
        posteriors grown by appends are served alike).

        ``folds``: None = leave-one-out; an int F >= 2 = ``np.array_split(np.arange(N), F)``, contiguous blocks in the
        order of the data (shuffle the data beforehand if a shuffle is wanted); otherwise a sequence of index arrays,
        pairwise disjoint, which need not cover all points.

        Returns ``(mu, s2)``, (N, 1) or with ``separate_samples`` (N, S), with ``predict``'s conventions: the latent
        variance clamped at 0, the noisy one with ``add_noise``, the equal-weight mixture over hyperparameter samples.
        Points in no fold are NaN.  With ``return_lpd`` also ``lpd`` (per point: the density of y_i under the noisy
        predictive marginal, mixed as ``predict`` mixes it) and ``lpd_fold`` ((F, S), or (F, 1) = the log-mean-exp
        over samples): the joint log density of each fold given the rest."""
        import warnings

        if self.y is None:
            raise ValueError("cv_predict: the GP has no training data")
        N = self.X.shape[0]
        fl = _cv_folds(folds, N)
        F = N if fl is None else len(fl)
        s_N = self.posteriors.size
        key = np.zeros(0) if fl is None else np.concatenate([np.r_[-1, f] for f in fl]).astype(float)
        dmu, s2n, quad, logdet, info = self._device_rows(
            lambda handle, local_posts, lo: [np.asarray(a, dtype=float) for a in handle.cv(fl)],
            [("dmu", (N,)), ("s2n", (N,)), ("quad", (F,)), ("logdet", (F,)), ("info", (F,))], key).values()
        bad = np.argwhere(info != 0)
        if bad.size:
            f, s = bad[0]
            warnings.warn(f"cv_predict: the held-out block of fold {f} for hyperparameter sample {s} is not positive "
                          f"definite in floating point ({bad.shape[0]} fold/sample pairs in all); its values are NaN",
                          RuntimeWarning, stacklevel=2)
        hyp = np.stack([p.hyp for p in self.posteriors])
        sn2, _, _ = self._noise_values(hyp, False)
        mult = np.array([float(_sn2_mult(p)) for p in self.posteriors])
        noise = (np.broadcast_to(np.asarray(sn2, dtype=float).reshape(s_N, -1), (s_N, N)) * mult[:, None]).T
        y = np.reshape(self.y, (-1, 1))
        mu = y - dmu
        y_s2 = s2n
        s2 = y_s2 if add_noise else np.maximum(s2n - noise, 0)
        lpd = lpd_fold = None
        if return_lpd:
            k = np.ones((F, 1)) if fl is None else np.array([[f.size] for f in fl], dtype=float)
            lpd_fold = -0.5 * quad - 0.5 * logdet - 0.5 * k * np.log(2 * np.pi)
            if separate_samples:
                lpd = -0.5 * (y - mu) ** 2 / y_s2 - 0.5 * np.log(2 * np.pi * y_s2)
        if not separate_samples:
            mu, s2, between = _mix_samples(mu, s2)
            if return_lpd:
                noisy = s2 if add_noise else np.reshape(np.sum(y_s2, 1) / s_N + between, (-1, 1))
                lpd = -0.5 * (y - mu) ** 2 / noisy - 0.5 * np.log(2 * np.pi * noisy)
                top = np.max(lpd_fold, axis=1, keepdims=True)
                lpd_fold = top + np.log(np.mean(np.exp(lpd_fold - top), axis=1, keepdims=True))
        if return_lpd:
            return mu, s2, lpd, lpd_fold
        return mu, s2

    @_on_device
    def predict_grad(self, x_star, y_star=None, s2_star=None, add_noise: bool = False,
                     separate_samples: bool = False):
        """``predict``'s mean and variance at ``x_star`` and their gradients with respect to ``x_star``:
        (mu, s2, dmu, ds2).  mu and s2 are what ``predict`` returns for the same arguments (within rounding: the
        device sums the variance in another order); dmu and ds2 are (M, D), or (M, D, S) with ``separate_samples``,
        entry [j, l] the derivative with respect to x_star[j, l].  The covariance part runs on the device
        (gpc_predict_grad), the mean function's part on the host.  Where the clamp s2 = max(s2, 0) is active the
        variance gradient is 0; the noise does not depend on x_star, so ``add_noise`` leaves it unchanged.  Built-in
        (stationary) covariance functions and the stock mean and noise functions only: other objects raise
        NotImplementedError."""
        from .noise_functions import GaussianNoise

        x_star, y_star, s2_star = self._convert_shapes(x_star, y_star, s2_star)
        if not self._builtin:
            raise NotImplementedError(f"predict_grad: the covariance function {self.covariance!r} is user-defined; it "
                                      "has no derivative with respect to x_star")
        if add_noise and type(self.noise) is not GaussianNoise:
            raise NotImplementedError(f"predict_grad: the noise function {self.noise!r} is user-defined; add_noise "
                                      "needs noise that does not depend on x_star")
        s_N = self.posteriors.size
        N_star, D = x_star.shape
        cov_N, _, _ = counts = self._counts()
        hyps = [self.posteriors[s].hyp for s in range(s_N)]
        dm = np.stack([_mean_grad_x(self.mean, _mean_hyp(h, counts), x_star) for h in hyps], axis=2)

        mu = np.zeros((N_star, s_N))
        s2 = np.zeros((N_star, s_N))
        dmu, ds2 = dm, np.zeros((N_star, D, s_N))
        if self.y is not None:
            fmu, fs2, dfmu, dfs2 = self._device_rows(
                lambda handle, local_posts, lo: handle.predict_grad(x_star),
                [("fmu", (N_star,)), ("fs2", (N_star,)), ("dfmu", (N_star, D)), ("dfs2", (N_star, D))], x_star).values()
            dmu = dm + dfmu
            ds2 = dfs2
        y_s2 = np.zeros((N_star, s_N)) if add_noise else None
        for s in range(s_N):
            hyp = hyps[s]
            m_star = np.reshape(self.mean.compute(_mean_hyp(hyp, counts), x_star), (-1,))
            if self.y is not None:
                mu[:, s] = m_star + fmu[:, s]
                s2[:, s] = fs2[:, s]
            else:  # no data: the prior, whose variance is constant for stationary kernels
                mu[:, s] = m_star
                s2[:, s] = self.covariance.compute(hyp[0:cov_N], x_star, compute_diag=True)[:, 0]
            s2[:, s] = np.maximum(s2[:, s], 0)
            if add_noise:
                y_s2[:, s:s + 1] = s2[:, s:s + 1] + self._noise_star(self.posteriors[s], x_star, y_star, s2_star)

        # the clamp of predict, s2 = max(s2, 0): no variance gradient where it holds s2 at 0 (s2 <= 0 before it; at
        # s2 = 0 exactly the one-sided derivatives differ, and 0 is the one that keeps the floor)
        ds2 = np.where((s2 <= 0)[:, None, :], 0.0, ds2)
        if add_noise:
            s2 = y_s2
        if not separate_samples:
            dmu, ds2 = _mix_sample_grads(mu, dmu, ds2)
            mu, s2, _ = _mix_samples(mu, s2)
        return mu, s2, dmu, ds2

    @_on_device
    def gradient_posterior(self, x_star, cov: str = "full", with_value: bool = False,
                           separate_samples: bool = False):
        """The posterior distribution of the gradient of the latent function at ``x_star``: (dmu, dcov).

        dmu (M, D) is the posterior mean of grad f (``predict_grad``'s dmu, the stock mean functions' gradient
        included); dcov (M, D, D) its posterior covariance, entry [j, l, k] = Cov(df/dx_l, df/dx_k) at x_star[j], or
        with ``cov="diag"`` the variances (M, D) alone (cheaper: no Gram matrix is formed).  With ``with_value`` f
        itself is prepended as slot 0: shapes (M, D + 1) and (M, D + 1, D + 1) (or (M, D + 1)), slot 0 holding
        ``predict``'s latent mean and variance and [j, 0, 1 + l] = Cov(f, df/dx_l) = half of ``predict_grad``'s variance
        gradient before its clamp.  Nothing is clamped or projected: a joint covariance must stay consistent, so each
        per-sample matrix is returned as computed (symmetric to the bit; in floating point its smallest eigenvalue
        may be a rounding error below 0 where the posterior is nearly certain).  With ``separate_samples`` a trailing
        axis S holds the hyperparameter samples; otherwise the moments of their equal-weight mixture are returned: the
        mean of the means, and the mean of the covariances plus the between-sample covariance of the mean vectors
        (divisor S - 1, ``predict``'s convention; one sample is returned as it is).  E[(df/dx_l)^2] = dmu_l^2 + dcov_ll.

        With data the operand, the solves and the per-query Gram matrices run on the device (gpc_grad_post); a GP
        without data returns the prior (the mean function's gradient and the diagonal prior block) from the host.
        Built-in covariance functions and stock mean functions only (NotImplementedError otherwise); the Matern kernel
        of degree 1 has no mean-square derivative and is refused.  Under sharding each rank computes its samples and
        the results are gathered: the same values as one process."""
        from . import _gradpost as _gpm

        if cov not in ("full", "diag"):
            raise ValueError(f"gradient_posterior: cov must be 'full' or 'diag', got {cov!r}")
        diag = cov == "diag"
        x_star, _, _ = self._convert_shapes(x_star, None, None)
        if not self._builtin:
            raise NotImplementedError(f"gradient_posterior: the covariance function {self.covariance!r} is "
                                      "user-defined; it has no derivative with respect to x_star")
        kid, degree = self._kid()
        _gpm.check_kind(kid, degree)
        s_N = self.posteriors.size
        M, D = x_star.shape
        P = D + 1
        cov_N, _, _ = counts = self._counts()
        hyps = [self.posteriors[s].hyp for s in range(s_N)]
        mean = np.empty((M, P, s_N))
        for s, h in enumerate(hyps):
            hm = _mean_hyp(h, counts)
            mean[:, 1:, s] = _mean_grad_x(self.mean, hm, x_star, "gradient_posterior")
            mean[:, 0, s] = np.reshape(self.mean.compute(hm, x_star), (-1,))
        if self.y is None:  # no data: the prior
            Hd = np.stack([_gpm.prior_block(kid, degree, h[:cov_N], D) for h in hyps], axis=1)  # (P, S)
            C = np.broadcast_to(Hd[None], (M, P, s_N)).copy()
            if not diag:
                C = np.einsum("mas,ab->mabs", C, np.eye(P))
        else:
            fmu, dfmu, C = self._device_rows(
                lambda handle, local_posts, lo: handle.grad_post(x_star, diag),
                [("fmu", (M,)), ("dfmu", (M, D)), ("cov", (M, P) if diag else (M, P, P))],
                x_star, np.array([float(diag)])).values()
            mean[:, 0, :] += fmu
            mean[:, 1:, :] += dfmu
        if not with_value:
            mean = mean[:, 1:]
            C = C[:, 1:] if diag else C[:, 1:, 1:]
        if separate_samples:
            return mean, C
        return _gpm.mix_diag(mean, C) if diag else _gpm.mix(mean, C)

    @_on_device
    def predict_hess(self, x_star, compute_var: bool = True, separate_samples: bool = False):
        """``predict_grad``'s (mu, s2, dmu, ds2) at ``x_star`` and the Hessians of the predictive mean and variance
        with respect to ``x_star``: (mu, s2, dmu, ds2, Hmu, Hs2), shapes (M,), (M,), (M, D), (M, D), (M, D, D),
        (M, D, D); ``separate_samples`` adds a trailing axis S.  Entry [j, a, b] is the second derivative with respect
        to x_star[j, a] and x_star[j, b]; every matrix is symmetric to the bit.  With ``compute_var=False`` the three
        variance entries are None and no product with the factors is launched (the mean Hessian is one pass over the
        pairs).

        mu, s2, dmu, ds2 follow ``predict_grad``'s conventions (no noise): the stock mean functions, the clamp
        s2 = max(s2, 0), a zero variance gradient where the clamp holds -- and there Hs2 is 0 as well.  Without
        ``separate_samples`` the moments of the equal-weight mixture are differentiated (``predict``'s convention,
        spread with divisor S - 1): Hmu is the mean of the per-sample Hessians, Hs2 the mean of theirs plus
        2 / (S - 1) sum_s [(dmu_s - dmu)(dmu_s - dmu)^T + (mu_s - mu)(Hmu_s - Hmu)].

        With data everything but the mean function runs on the device (gpc_predict_hess); a GP without data returns
        the prior: the mean function's Hessian and Hs2 = 0.  Built-in covariance functions and stock mean functions
        only (NotImplementedError otherwise); the Matern kernel of degree 1 has no second derivative and is refused.
        Under sharding each rank computes its samples and the results are gathered: the same values as one process."""
        from . import _hess as _hm

        x_star, _, _ = self._convert_shapes(x_star, None, None)
        if not self._builtin:
            raise NotImplementedError(f"predict_hess: the covariance function {self.covariance!r} is user-defined; it "
                                      "has no derivative with respect to x_star")
        kid, degree = self._kid()
        _hm.check_kind(kid, degree)
        var = bool(compute_var)
        s_N = self.posteriors.size
        M, D = x_star.shape
        cov_N, _, _ = counts = self._counts()
        hyps = [self.posteriors[s].hyp for s in range(s_N)]
        h_mean = [_mean_hyp(h, counts) for h in hyps]
        dmu = np.stack([_mean_grad_x(self.mean, hm, x_star, "predict_hess") for hm in h_mean], axis=2)
        Hmu = np.stack([_hm.mean_hess(self.mean, hm, x_star) for hm in h_mean], axis=3)
        mu = np.stack([np.reshape(self.mean.compute(hm, x_star), (-1,)) for hm in h_mean], axis=1)
        s2 = ds2 = Hs2 = None
        if self.y is None:  # no data: the prior, whose variance is constant for stationary kernels
            if var:
                s2 = np.stack([self.covariance.compute(h[0:cov_N], x_star, compute_diag=True)[:, 0] for h in hyps], axis=1)
                ds2, Hs2 = np.zeros((M, D, s_N)), np.zeros((M, D, D, s_N))
        else:
            def call(handle, local_posts, lo):
                fmu, fs2, dfmu, dfs2, hmu, hs2 = handle.predict_hess(x_star, var)
                return [fmu, dfmu, hmu] + ([fs2, dfs2, hs2] if var else [])

            layout = [("fmu", (M,)), ("dfmu", (M, D)), ("hmu", (M, D, D))]
            if var:
                layout += [("fs2", (M,)), ("dfs2", (M, D)), ("hs2", (M, D, D))]
            r = self._device_rows(call, layout, x_star, np.array([float(var)]))
            mu, dmu, Hmu = mu + r["fmu"], dmu + r["dfmu"], Hmu + r["hmu"]
            if var:
                s2, ds2, Hs2 = r["fs2"], r["dfs2"], r["hs2"]
        if var:
            # the clamp of predict, s2 = max(s2, 0): neither gradient nor curvature where it holds s2 at 0
            held = s2 <= 0
            s2 = np.maximum(s2, 0)
            ds2 = np.where(held[:, None, :], 0.0, ds2)
            Hs2 = np.where(held[:, None, None, :], 0.0, Hs2)
        if separate_samples:
            return mu, s2, dmu, ds2, Hmu, Hs2
        Hmu_m, Hs2_m = _hm.mix(mu, dmu, Hmu, Hs2)
        if var:
            dmu_m, ds2_m = _mix_sample_grads(mu, dmu, ds2)
        else:
            dmu_m, ds2_m = np.sum(dmu, 2) / s_N, None
        mu_m, s2_m, _ = _mix_samples(mu, s2)
        return np.reshape(mu_m, (-1,)), None if s2_m is None else np.reshape(s2_m, (-1,)), dmu_m, ds2_m, Hmu_m, Hs2_m

    def _hyp_grad_check(self, who):
        """The refusals of the hyperparameter gradients of predictions that need no device."""
        from . import _hypgrad as _hg
        from .mean_functions import ConstantMean, NegativeQuadratic, ZeroMean
        from .noise_functions import GaussianNoise

        if not self._builtin:
            raise NotImplementedError(f"{who}: the covariance function {self.covariance!r} is user-defined; its "
                                      "derivatives with respect to the hyperparameters are not on the device")
        if self.dtype != "f64":
            raise NotImplementedError(f"{who}: the hyperparameter gradients are computed in fp64 only; this GP's dtype is "
                                      f"{self.dtype!r}")
        _hg.check_kind(*self._kid(), who=who)
        if type(self.noise) is not GaussianNoise:
            raise NotImplementedError(f"{who}: the noise function {self.noise!r} ({type(self.noise).__name__}) is "
                                      "user-defined; its derivatives at x_star are unknown")
        if type(self.mean) not in (ZeroMean, ConstantMean, NegativeQuadratic):
            raise NotImplementedError(f"{who}: the mean function {self.mean!r} ({type(self.mean).__name__}) is "
                                      "user-defined; its derivatives at x_star are unknown")

    def predict_hyp_grad(self, x_star, compute_var: bool = True, add_noise: bool = False, s2_star=None):
        """The prediction at ``x_star`` under every resident hyperparameter sample and its derivatives with respect to
        that sample's own hyperparameters: (mu, s2, dmu, ds2), mu and s2 (M, S), dmu and ds2 (M, hyp_N, S), entry
        [j, p, s] the derivative of sample s's prediction at x_star[j] with respect to its hyperparameter p, ordered
        [cov | noise | mean] on the scales ``nll_batch`` differentiates on.  Always per sample: every sample has its
        own theta, so no mixture is formed.  With ``compute_var=False`` s2 and ds2 are None and no product with the
        factors is launched; mu and dmu carry the same bits.

        The derivatives hold each sample's jitter multiplier fixed, as ``nll_hess_batch`` does.  The mean function and
        d m(x_star) / d theta_mean are added here; with ``add_noise`` so are mult sn2(x_star) (``s2_star``: the
        provided noise at x_star) and its derivatives in the noise columns.  ``predict_grad``'s conventions: the clamp
        s2 = max(s2, 0) on the latent variance, and a zero variance gradient where it holds.

        Everything but the plugins runs on the device (gpc_predict_hyp_grad; ``_hypgrad`` has the closed form).
        Built-in covariance functions, the stock ``GaussianNoise`` and the stock mean functions in float64 only
        (NotImplementedError otherwise, naming the reason); the Matern kernel of degree 1 is refused.  Under sharding
        each rank computes its samples and the results are gathered: the same values as one process."""
        self._hyp_grad_check("predict_hyp_grad")
        return self._predict_hyp_grad_local(x_star, compute_var, add_noise, s2_star)

    @_on_device
    def _predict_hyp_grad_local(self, x_star, compute_var, add_noise, s2_star):
        """``predict_hyp_grad`` after its refusals: the device call and the plugin terms."""
        x_star, _, s2_star = self._convert_shapes(x_star, None, s2_star)
        if self.y is None:
            raise ValueError("predict_hyp_grad: the GP holds no data; the prior's derivatives are the plugins' own")
        var = bool(compute_var)
        if add_noise and not var:
            raise ValueError("predict_hyp_grad: add_noise needs compute_var")
        self._require_posteriors()
        s_N = self.posteriors.size
        M = x_star.shape[0]
        cov_N, noise_N, mean_N = counts = self._counts()
        P = cov_N + noise_N + mean_N
        hyp = np.stack([p.hyp for p in self.posteriors])
        pv = self._plugin_values(hyp, True)

        def call(handle, local_posts, lo):
            sl = slice(lo, lo + len(local_posts))
            fmu, fs2, dfmu, dfs2 = handle.predict_hyp_grad(
                x_star, cov_N, pv["sn2"][sl], None if pv["dsn2"] is None else pv["dsn2"][sl],
                None if pv["dm"] is None else pv["dm"][sl], var)
            return [fmu, dfmu] + ([fs2, dfs2] if var else [])

        layout = [("fmu", (M,)), ("dfmu", (M, P))] + ([("fs2", (M,)), ("dfs2", (M, P))] if var else [])
        r = self._device_rows(call, layout, x_star, np.array([float(var)]))
        mu, dmu = r["fmu"].copy(), r["dfmu"].copy()
        h_mean = _mean_hyp(hyp, counts)
        m_star = self.mean.values(h_mean, x_star, mean_N > 0)
        if mean_N > 0:
            m_star, dm_star = m_star
            dmu[:, cov_N + noise_N:, :] += np.transpose(dm_star, (1, 2, 0))
        mu += np.transpose(m_star)
        if not var:
            return mu, None, dmu, None
        s2, ds2 = r["fs2"], r["dfs2"]
        # the clamp of predict, s2 = max(s2, 0): no gradient where it holds s2 at 0
        held = s2 <= 0
        s2 = np.maximum(s2, 0)
        ds2 = np.where(held[:, None, :], 0.0, ds2)
        if add_noise:
            mult = np.array([float(_sn2_mult(p)) for p in self.posteriors])
            ns, dns = self.noise.values(hyp[:, cov_N:cov_N + noise_N], x_star, None, s2_star, True)
            s2 = s2 + np.transpose(np.broadcast_to(ns, (s_N, M)) * mult[:, None])
            if noise_N:
                dns = np.broadcast_to(dns, (s_N, M, noise_N)) * mult[:, None, None]
                ds2[:, cov_N:cov_N + noise_N, :] += np.transpose(dns, (1, 2, 0))
        return mu, s2, dmu, ds2

    def predict_laplace(self, x_star, laplace=None, add_noise: bool = False):
        """The prediction at the first resident hyperparameter sample theta-hat (e.g. the MAP that ``fit`` left) with the
        hyperparameter uncertainty of a Laplace approximation carried into it: a dict with

            mu, s2     the prediction at theta-hat (M,), ``predict_hyp_grad``'s
            var_mu     g_mu^T Sigma g_mu, g_mu = d mu / d theta restricted to ``laplace["free"]``
            var_s2     g_s2^T Sigma g_s2, the same for the variance
            s2_total   s2 + var_mu

        ``laplace``: what ``laplace_approximation`` returned (default: ``self.laplace_approximation()``); its ``cov``
        is Sigma, on the coordinates ``free``.  This is the FIRST-ORDER delta method: Var_theta[mu*] ~ g^T Sigma g, the
        variance of the linearisation of mu*(theta) about theta-hat under N(theta-hat, Sigma).  ``var_s2`` is returned
        so that callers can assemble a marginal-GP variance of their choice; no paper's constants are built in.  When
        ``laplace["cov"]`` is None (``is_pd`` False: the Hessian at theta-hat is not positive definite) a ValueError
        is raised; nothing is repaired."""
        from . import _hypgrad as _hg

        if laplace is None:
            laplace = self.laplace_approximation()
        if laplace["cov"] is None:
            raise ValueError("predict_laplace: the Laplace approximation has no covariance (is_pd is False: the Hessian "
                             "of the negative log posterior is not positive definite at this point)")
        mu, s2, dmu, ds2 = self.predict_hyp_grad(x_star, True, add_noise)
        var_mu = _hg.delta_variance(dmu[:, :, 0], laplace["cov"], laplace["free"])
        var_s2 = _hg.delta_variance(ds2[:, :, 0], laplace["cov"], laplace["free"])
        return dict(mu=mu[:, 0], s2=s2[:, 0], var_mu=var_mu, var_s2=var_s2, s2_total=s2[:, 0] + var_mu)

    @_on_device
    def predict_full(self, x_star, y_star=None, s2_star=None, add_noise: bool = False):
        """Posterior mean and FULL covariance per hyperparameter sample (reference :1561-1661):
        mu (M, S), cov (M, M, S).  K**, Ks, V = L^-T Ks and K** - V^T V are device products."""
        x_star, y_star, s2_star = self._convert_shapes(x_star, y_star, s2_star)
        s_N = self.posteriors.size
        N_star, _ = x_star.shape
        cov_N, _, _ = counts = self._counts()
        mu = np.zeros((N_star, s_N))
        cov = np.zeros((s_N, N_star, N_star))
        if self.y is not None:
            def call(handle, local_posts, lo):
                if self._builtin:
                    fmu, fcov = handle.predict_full(x_star)
                else:
                    Ks = np.stack([self.covariance.compute(p.hyp[0:cov_N], self.X, x_star) for p in local_posts])
                    Kss = np.stack([self.covariance.compute(p.hyp[0:cov_N], x_star) for p in local_posts])
                    fmu, _, fcov = handle.predict_K(Ks, Kss, want_var=False)
                return fmu, fcov.transpose(1, 2, 0)  # (the device's covariances are sample-first)

            fmu, fcov = self._device_rows(call, [("fmu", (N_star,)), ("fcov", (N_star, N_star))], x_star).values()
        for s in range(s_N):
            hyp = self.posteriors[s].hyp
            m_star = np.reshape(self.mean.compute(_mean_hyp(hyp, counts), x_star), (-1,))
            if self.y is None:  # no data: the prior
                mu[:, s] = m_star
                C = self.covariance.compute(hyp[0:cov_N], x_star)
            else:
                mu[:, s] = m_star + fmu[:, s]
                C = fcov[:, :, s]
            C = (C + C.T) / 2  # :1647
            cov[s, :, :] = C
            if add_noise:  # :1659, verbatim semantics
                cov[s, :, :] += np.dot(np.eye(N_star), self._noise_star(self.posteriors[s], x_star, y_star, s2_star))
        return mu, cov.transpose(1, 2, 0)

    def predict_cov(self, x_a, x_b):
        """Posterior covariance of the latent function between the rows of ``x_a`` and the rows of ``x_b``, per
        hyperparameter sample: cov (Ma, Mb, S),

            cov[:, :, s] = k_s(x_a, x_b) - k_s(x_a, X) (K_s + Sigma_s)^-1 k_s(X, x_b),

        the [A, B] block of ``predict_full(np.vstack([x_a, x_b]))[1][:, :, s]`` to rounding, without building the rest
        of that matrix.  No noise term (the two sets are different points) and no symmetrisation (the block is not
        square).  With data the products run on the device (gpc_predict_cov); a GP without data returns the prior
        k_s(x_a, x_b) from the covariance object, on the host.  Built-in covariance functions only.  Under sharding
        each rank computes its samples and the results are gathered: the same values as one process."""
        if not self._builtin:
            raise NotImplementedError(f"predict_cov: the covariance function {self.covariance!r} is user-defined; the "
                                      "cross covariance runs on the built-in covariance functions only")
        x_a, _, _ = self._convert_shapes(x_a, None, None)
        x_b, _, _ = self._convert_shapes(x_b, None, None)
        if self.y is None:  # no data: the prior
            cov_N = self._counts()[0]
            return np.stack([self.covariance.compute(p.hyp[0:cov_N], x_a, x_b) for p in self.posteriors], axis=2)
        return self._cov_on_device(x_a, x_b, None)[0]

    def lookahead_variance(self, x_cand, x_ref, weights=None, y_cand=None, s2_cand=None,
                           separate_samples: bool = False):
        """How much ONE more observation at each candidate would reduce the weighted posterior variance at the
        reference points: reduction (Mc, S) with ``separate_samples``, else (Mc, 1),

            reduction[c, s] = sum_r w_rs C_s(x_ref_r, x_cand_c)^2 / den_cs,
            den_cs          = max(fs2_s(x_cand_c), 0) + sn2_s(x_cand_c) * sn2_mult_s,

        C_s ``predict_cov``'s covariance, fs2 ``predict``'s variance of the candidate before its clamp and sn2 the noise
        function's value at the candidate (``y_cand``, ``s2_cand`` as ``predict``'s ``y_star``, ``s2_star``), exactly
        as ``predict(add_noise=True)`` forms it; 0 where den_cs <= 0.  This is s2_s(x_ref_r) - s2_s(x_ref_r | x_c)
        summed with the weights, the core of integrated-variance designs.  ``weights``: None for 1 / M_ref (the mean
        reduction over the reference points), (M_ref,) shared by the samples, or (M_ref, S) per sample; they must be
        finite.  Without ``separate_samples`` the result is the plain mean over the samples: the expected reduction of
        the AVERAGE WITHIN-SAMPLE variance -- the between-sample spread of the means, which ``predict``'s mixture
        variance also holds, does not enter.  The value is reported as computed: it is not clamped against
        sum_r w_r s2_r (the Cauchy-Schwarz bound holds in exact arithmetic).  With data the covariance never leaves
        the device: its weighted squares are summed there (gpc_predict_cov) and Mc x S numbers come back.  A GP
        without data applies the same formula to the prior, on the host.  Built-in covariance functions only; sharded
        like ``predict_cov``."""
        if not self._builtin:
            raise NotImplementedError(f"lookahead_variance: the covariance function {self.covariance!r} is user-defined; "
                                      "the cross covariance runs on the built-in covariance functions only")
        x_cand, y_cand, s2_cand = self._convert_shapes(x_cand, y_cand, s2_cand)
        x_ref, _, _ = self._convert_shapes(x_ref, None, None)
        s_N = self.posteriors.size
        Mc, Mr = x_cand.shape[0], x_ref.shape[0]
        cov_N = self._counts()[0]
        w = self._lookahead_weights("lookahead_variance", weights, Mr)
        if self.y is None:  # no data: the prior
            wsq = np.empty((Mc, s_N))
            fs2 = np.empty((Mc, s_N))
            for s in range(s_N):
                hyp = self.posteriors[s].hyp
                C = self.covariance.compute(hyp[0:cov_N], x_ref, x_cand)
                ws = w[:, s] if w.ndim == 2 else w
                wsq[:, s] = np.sum(ws[:, None] * C * C, axis=0)
                fs2[:, s] = self.covariance.compute(hyp[0:cov_N], x_cand, compute_diag=True)[:, 0]
        else:
            _, wsq, fs2 = self._cov_on_device(x_ref, x_cand, w)
        den = np.maximum(fs2, 0) + self._lookahead_noise(x_cand, y_cand, s2_cand)
        red = np.where(den > 0, wsq / np.where(den > 0, den, 1.0), 0.0)
        if not separate_samples:
            red = np.reshape(np.sum(red, 1) / s_N, (-1, 1))
        return red

    def _lookahead_weights(self, who, weights, Mr):
        """The reference points' weights of ``lookahead_variance`` / ``lookahead_batch``: None -> 1 / Mr each, else
        (Mr,) or (Mr, S), finite."""
        s_N = self.posteriors.size
        if weights is None:
            return np.full(Mr, 1.0 / Mr)
        w = np.asarray(weights, dtype=float)
        if w.shape not in ((Mr,), (Mr, s_N)):
            raise ValueError(f"{who}: weights must be ({Mr},) or ({Mr}, {s_N}), got {w.shape}")
        if not np.all(np.isfinite(w)):
            raise ValueError(f"{who}: weights must be finite")
        return w

    def _lookahead_noise(self, x_cand, y_cand, s2_cand, mult=None):
        """The noise part of the look-ahead denominators: (Mc, S), sn2_s(x_c) * sn2_mult_s as ``predict(add_noise=True)``
        forms it (``mult``: multipliers to use instead of the records')."""
        nz = np.empty((x_cand.shape[0], self.posteriors.size))
        for s, post in enumerate(self.posteriors):
            if mult is None:
                nz[:, s:s + 1] = self._noise_star(post, x_cand, y_cand, s2_cand)
            else:
                cov_N, noise_N, _ = self._counts()
                nz[:, s:s + 1] = self.noise.compute(post.hyp[cov_N:cov_N + noise_N], x_cand, y_cand, s2_cand) * mult[s]
        return nz

    def lookahead_batch(self, x_cand, x_ref, q, weights=None, y_cand=None, s2_cand=None,
                        separate_samples: bool = False):
        """Greedy batch design by the weighted integrated variance: the q candidates that ``lookahead_variance``,
        argmax and ``update`` with a fantasy target would pick one after the other -- without the loop, and without
        touching this GP.  Returns ``(idx, gain)``: idx (q,) the selection order; gain (q, S) with
        ``separate_samples``, else (q, 1), the chosen candidate's reduction at the step it was chosen (its cumulative
        sum is the total expected reduction).

        The posterior covariance after conditioning does not depend on the observed value, so per sample s, from
        C_s = ``predict_cov([x_ref; x_cand], x_cand)``, v_s = ``predict``'s unclamped variance of the candidates and
        n_s = sn2_s(x_c) * sn2_mult_s (``y_cand``, ``s2_cand`` as ``lookahead_variance``'s), step t is

            den_s(c)  = max(v_s(c), 0) + n_s(c)
            gain_s(c) = sum_r w_rs C_s(r, c)^2 / den_s(c)            (0 where den_s(c) <= 0)
            c_t       = argmax_c (1/S) sum_s gain_s(c) over the candidates not yet chosen, lowest index on a tie
            l_s(a)    = C_s(a, c_t) / sqrt(den_s(c_t));  C_s(a, b) -= l_s(a) l_s(Mr + b);  v_s(b) -= l_s(Mr + b)^2

        (``_lookahead_batch`` restates it).  A candidate is chosen at most once; step 0's gains are
        ``lookahead_variance``'s.  ``weights`` as ``lookahead_variance``'s; ``1 <= q <= Mc`` (``ValueError``).  With
        data the whole loop runs on the device (gpc_lookahead_batch) in fp64, also for fp32 posteriors, and q indices
        and q x S gains come back; a GP without data runs the same recurrence on the prior, on the host.  Built-in
        covariance functions only.  Under a process group the call is NOT sharded (the selection needs every sample at
        every step): it runs on the calling rank alone and exchanges nothing; resident posteriors that are sharded are
        rebuilt locally as temporaries."""
        from . import _lookahead_batch as _lb

        if not self._builtin:
            raise NotImplementedError(f"lookahead_batch: the covariance function {self.covariance!r} is user-defined; "
                                      "the cross covariance runs on the built-in covariance functions only")
        x_cand, y_cand, s2_cand = self._convert_shapes(x_cand, y_cand, s2_cand)
        x_ref, _, _ = self._convert_shapes(x_ref, None, None)
        s_N = self.posteriors.size
        Mc, Mr = x_cand.shape[0], x_ref.shape[0]
        if isinstance(q, bool) or int(q) != q or not 1 <= int(q) <= Mc:
            raise ValueError(f"lookahead_batch: q must be an integer in [1, {Mc}] (the number of candidates), got {q!r}")
        q = int(q)
        w = self._lookahead_weights("lookahead_batch", weights, Mr)
        if self.y is None:  # no data: the prior
            cov_N = self._counts()[0]
            x_all = np.vstack([x_ref, x_cand])
            C0 = np.stack([self.covariance.compute(p.hyp[0:cov_N], x_all, x_cand) for p in self.posteriors])
            v0 = np.stack([self.covariance.compute(p.hyp[0:cov_N], x_cand, compute_diag=True)[:, 0]
                           for p in self.posteriors], axis=1)
            w2 = w if w.ndim == 2 else np.repeat(w[:, None], s_N, axis=1)
            idx, gain = _lb.greedy_batch(C0, v0, self._lookahead_noise(x_cand, y_cand, s2_cand), w2, q)
        else:
            idx, gain = self._lookahead_batch_local(x_cand, x_ref, q, w, y_cand, s2_cand)
        if not separate_samples:
            gain = np.reshape(np.sum(gain, 1) / s_N, (-1, 1))
        return idx, gain

    @_on_device
    def _lookahead_batch_local(self, x_cand, x_ref, q, w, y_cand, s2_cand):
        """``lookahead_batch`` after its refusals: this rank's device call, on the resident posteriors or (sharded)
        on temporaries built for all samples."""
        self._require_posteriors()
        ctx = self._ctx()
        if self._post_range is None and self._post_handle is not None:
            return self._post_handle.lookahead_batch(x_ref, x_cand, q, w, self._lookahead_noise(x_cand, y_cand, s2_cand))
        cov_N = self._counts()[0]
        hyp = np.stack([p.hyp for p in self.posteriors])
        pv = self._plugin_values(hyp, False)
        kid, deg = self._kid()
        handle, mult, _, info = ctx.posterior_batch(kid, deg, _DTYPES[self.dtype], hyp[:, :cov_N], pv["m"], pv["sn2"],
                                                    pv["vec"])
        try:
            if np.any(info != 0):
                raise LinAlgError("Singular matrix for L Cholesky decomposition")
            return handle.lookahead_batch(x_ref, x_cand, q, w, self._lookahead_noise(x_cand, y_cand, s2_cand, mult))
        finally:
            handle.free()

    @_on_device
    def _cov_on_device(self, x_a, x_b, weights):
        """The device part of ``predict_cov`` (weights None: (cov (Ma, Mb, S), None, None)) and ``lookahead_variance``
        ((None, wsq (Mb, S), fs2 of x_b (Mb, S))), gathered over the ranks when sharded."""
        Ma, Mb = x_a.shape[0], x_b.shape[0]
        want_cov = weights is None

        def call(handle, local_posts, lo):
            w = weights[:, lo:lo + len(local_posts)] if (weights is not None and weights.ndim == 2) else weights
            cov, wsq, fs2 = handle.predict_cov(x_a, x_b, w, want_cov=want_cov, want_fs2=not want_cov)
            return [cov.transpose(1, 2, 0)] if want_cov else [wsq, fs2]  # (the device's covariance is sample-first)

        r = self._device_rows(call, [("cov", (Ma, Mb))] if want_cov else [("wsq", (Mb,)), ("fs2", (Mb,))],
                              x_a, x_b, np.zeros(0) if weights is None else weights)
        return r.get("cov"), r.get("wsq"), r.get("fs2")

    def random_function(self, X_star, add_noise: bool = False):
        """One function drawn from the GP at ``X_star`` (reference :2241-2329): a hyperparameter sample is picked
        with ``np.random``, the values come from that sample's posterior N(f_mu, C) -- the prior when the GP holds
        no data -- through a factor T of C (T^T T = C, ``_robust_factor``), observation noise on request.  f_mu and
        C are ``predict_full``'s device products.  ``np.random`` is called as the reference calls it (``randint``
        for the sample, ``standard_normal`` for the M values, again for the noise), so a seeded draw is the
        reference's draw; with sharded posteriors every rank calls this with the same seed."""
        X_star = np.atleast_2d(np.asarray(X_star, dtype=float))
        s = np.random.randint(0, np.size(self.posteriors))
        mu, cov = self.predict_full(X_star)
        f_mu, C = mu[:, [s]], cov[:, :, s]
        if self.y is None:
            C = C + np.spacing(1) * np.eye(C.shape[0])  # :2287
        T = self._robust_factor(C)
        f_star = np.dot(T.T, np.random.standard_normal((T.shape[0], 1))) + f_mu
        if not add_noise:
            return f_star
        cov_N, noise_N, _ = self._counts()
        post = self.posteriors[s]
        sn2 = self.noise.compute(post.hyp[cov_N:cov_N + noise_N], X_star, None, None)
        return f_star + np.sqrt(sn2 * _sn2_mult(post)) * np.random.standard_normal(size=f_mu.shape)

    def draw_functions(self, x_star, n_draws: int = 1, add_noise: bool = False, seed: int = 0, y_star=None,
                       s2_star=None, return_jitter: bool = False):
        """``n_draws`` joint draws of the latent function at ``x_star`` from the posterior of EACH hyperparameter
        sample: f (M, n_draws, S), with ``f[:, r, s] = m_s(x*) + fmu_s + chol(C_s + tau_s I) z_{s,r}`` -- fmu_s and C_s
        are ``predict_full``'s mean part and covariance, z the seeded stream of ``_philox`` (a value depends on seed,
        sample, draw and row only).  C_s is factored without jitter first; a sample that fails is retried with
        tau_s = t mean(diag C_s), t = 1e-12 ... 1e-6 (``LinAlgError`` naming the sample if none succeeds).  With
        ``add_noise`` each value gets sqrt(sn2* sn2_mult_s) z' from noise stream 1.  ``return_jitter``: (f, tau),
        tau (S,) the absolute jitter of every sample.  With data the factorization and the product run on the device
        (gpc_draw; fp32 posteriors in fp32); a GP without data draws from the prior N(m, K**), K** from the covariance
        object and the factorization and product in NumPy.  Built-in
        covariance functions only.  Under sharding each rank draws its samples and the results are gathered:
        the same values as one process.  ``random_function`` is unchanged."""
        from . import _philox

        if not self._builtin:
            raise NotImplementedError(f"draw_functions: the covariance function {self.covariance!r} is user-defined; "
                                      "draws run on the built-in covariance functions only")
        if isinstance(n_draws, bool) or int(n_draws) != n_draws or n_draws < 1:
            raise ValueError(f"n_draws must be a positive integer, got {n_draws!r}")
        n_draws = int(n_draws)
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2**64:
            raise ValueError(f"seed must be an integer in [0, 2**64), got {seed!r}")
        seed = int(seed)
        x_star, y_star, s2_star = self._convert_shapes(x_star, y_star, s2_star)
        s_N = self.posteriors.size
        M = x_star.shape[0]
        cov_N, noise_N, _ = counts = self._counts()
        hyps = [self.posteriors[s].hyp for s in range(s_N)]
        nsd = None
        if add_noise:
            nsd = np.empty((M, s_N))
            for s in range(s_N):
                sn2 = np.asarray(self.noise.compute(hyps[s][cov_N:cov_N + noise_N], x_star, y_star, s2_star), float)
                sn2 = np.broadcast_to(sn2.reshape(-1) if sn2.size == M else sn2.reshape(-1)[:1], (M,))
                nsd[:, s] = np.sqrt(sn2 * _sn2_mult(self.posteriors[s]))

        if self.y is not None:
            f, tau = self._draw_on_device(x_star, n_draws, seed, nsd)
        else:  # no data: the prior N(m, K**), on the host
            f = np.empty((M, n_draws, s_N))
            tau = np.zeros(s_N)
            for s in range(s_N):
                K = self.covariance.compute(hyps[s][0:cov_N], x_star)
                L, tau[s] = self._jittered_cholesky(K, s)
                z = _philox.normals_block(seed, 0, M, n_draws, [s])[:, :, 0]
                f[:, :, s] = L @ z
                if add_noise:
                    f[:, :, s] += nsd[:, s:s + 1] * _philox.normals_block(seed, 1, M, n_draws, [s])[:, :, 0]
        for s in range(s_N):
            m_star = np.reshape(self.mean.compute(_mean_hyp(hyps[s], counts), x_star), (-1,))
            f[:, :, s] += m_star[:, None]
        return (f, tau) if return_jitter else f

    @_on_device
    def _draw_on_device(self, x_star, n_draws, seed, nsd):
        """draw_functions' posterior part: (f (M, n_draws, S) without the mean function, tau (S,)), gathered over the
        ranks when sharded (each rank draws its block of samples under their global indices)."""
        def call(handle, local_posts, lo):
            return handle.draw(x_star, n_draws, seed, lo, None if nsd is None else nsd[:, lo:lo + len(local_posts)])

        r = self._device_rows(call, [("f", (x_star.shape[0], n_draws)), ("tau", ())],
                              x_star, n_draws, seed, nsd is not None)
        return r["f"], r["tau"]

    def sample_paths(self, n_paths: int = 1, n_features: int = 1024, seed: int = 0):
        """``n_paths`` sampled posterior functions per hyperparameter sample, as a ``PosteriorPaths`` object that
        evaluates them -- and their gradients with respect to x -- at any points afterwards (Thompson sampling,
        max-value and entropy searches, Monte-Carlo acquisitions); ``draw_functions`` draws at fixed points only.
        Matheron's rule with ``n_features`` random Fourier features (``_paths``): the update term is exact, the prior part
        approximate.  A path depends on (seed, sample, path index) only -- not on ``n_paths``, the batch of samples or the
        sharding.  With data the features, the solve and every evaluation run on the device (gpc_paths_create /
        gpc_paths_eval, fp64 also for fp32 posteriors); a GP without data gives prior paths on the host.  Squared-
        exponential and Matern covariance functions (ARD and isotropic) only: the rational quadratic and user-defined
        covariance objects raise NotImplementedError.  Under sharding each rank holds the paths of its samples and the
        evaluations are gathered: the same values as one process."""
        from . import _paths

        if not self._builtin:
            raise NotImplementedError(f"sample_paths: the covariance function {self.covariance!r} is user-defined; "
                                      "paths need the spectral density of a built-in covariance function")
        kid, degree = self._kid()
        if kid == _paths.K_RQ:
            raise NotImplementedError("sample_paths: the rational-quadratic covariance function is not supported; "
                                      "spectral draws exist for the squared-exponential and Matern kernels")
        for name, val in (("n_paths", n_paths), ("n_features", n_features)):
            if isinstance(val, bool) or int(val) != val or val < 1:
                raise ValueError(f"{name} must be a positive integer, got {val!r}")
        n_paths, n_features = int(n_paths), int(n_features)
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2**64:
            raise ValueError(f"seed must be an integer in [0, 2**64), got {seed!r}")
        seed = int(seed)
        s_N = self.posteriors.size
        counts = self._counts()
        cov_N = counts[0]
        hyps = [np.array(self.posteriors[s].hyp, dtype=float) for s in range(s_N)]
        if self.y is None:  # no data: prior paths, v = 0, on the host
            host = [_paths.features(kid, degree, self.D, n_features, seed, s) + (_paths.weights(n_features, n_paths, seed, s),)
                    for s in range(s_N)]
            return PosteriorPaths(n_paths, n_features, seed, self.D, kid, degree, self.mean, hyps, counts, host=host)
        handle, post_range = self._paths_on_device(n_paths, n_features, seed)
        return PosteriorPaths(n_paths, n_features, seed, self.D, kid, degree, self.mean, hyps, counts, handle=handle,
                              post_range=post_range, group=self.process_group)

    @_on_device
    def _paths_on_device(self, n_paths, n_features, seed):
        """sample_paths' device part: (the ``_lib.Paths`` handle of this rank's samples or None, the shard range).
        Nothing is exchanged here (``PosteriorPaths`` gathers what it evaluates), so no ``_device_rows``."""
        self._require_posteriors()
        self._ctx()
        local_posts, lo = self._local_posteriors()
        if not local_posts:
            return None, self._post_range
        pv = self._plugin_values(np.stack([p.hyp for p in local_posts]), False)
        N = self.X.shape[0]
        ym = np.reshape(self.y, (1, -1)) - pv["m"]
        mult = np.array([float(_sn2_mult(p)) for p in local_posts])
        nsd = np.sqrt(np.broadcast_to(pv["sn2"], (len(local_posts), N)) * mult[:, None]).T
        return self._post_handle.paths(n_paths, n_features, seed, lo, ym, nsd), self._post_range

    # ------------------------------------------------------------------ gradient observations
    def _grad_obs_inputs(self, who, X_g, dy, s2_grad):
        """Validated (X_g (Ng, D), dy (Ng, D), s2_grad (Ng, D)) of ``condition_on_gradients`` / ``nll_batch_grad_obs``."""
        from . import _gradpost

        if not self._builtin:
            raise NotImplementedError(f"{who}: the covariance function {self.covariance!r} is user-defined; gradient "
                                      "observations need the derivatives of a built-in covariance function")
        kid, degree = self._kid()
        if kid in _gradpost._MATERN and degree == 1:
            raise NotImplementedError(f"{who}: the Matern kernel of degree 1 has no mean-square derivative (the prior "
                                      "variance of its gradient is infinite)")
        if self.X is None or self.y is None:
            raise ValueError(f"{who}: the GP has no training data (gradient-only data are not supported)")
        D = self.D
        X_g, dy = np.asarray(X_g, dtype=float), np.asarray(dy, dtype=float)
        if X_g.ndim != 2 or X_g.shape[1] != D or X_g.shape[0] < 1:
            raise ValueError(f"{who}: X_g must be (Ng, {D}) with Ng >= 1, got {X_g.shape}")
        Ng = X_g.shape[0]
        if dy.shape != (Ng, D):
            raise ValueError(f"{who}: dy must be (Ng, D) = ({Ng}, {D}), one gradient per row of X_g, got {dy.shape}")
        if s2_grad is None:
            raise ValueError(f"{who}: s2_grad is required (the variances of the gradient observations; 0 is allowed)")
        s2g = np.asarray(s2_grad, dtype=float)
        if s2g.ndim == 0:
            s2g = np.full((Ng, D), float(s2g))
        elif s2g.shape == (Ng,):
            s2g = np.repeat(s2g[:, None], D, axis=1)
        elif s2g.shape != (Ng, D):
            raise ValueError(f"{who}: s2_grad must be a scalar, (Ng,) = ({Ng},) or (Ng, D) = ({Ng}, {D}), got {s2g.shape}")
        if not (np.all(np.isfinite(X_g)) and np.all(np.isfinite(dy)) and np.all(np.isfinite(s2g))):
            raise ValueError(f"{who}: X_g, dy and s2_grad must be finite")
        if np.any(s2g < 0):
            raise ValueError(f"{who}: s2_grad holds negative variances")
        return np.ascontiguousarray(X_g), np.ascontiguousarray(dy), s2g

    def _grad_obs_rows(self, who, hyp, X_g, s2g):
        """(m (S, n), sn2 (S, n)) in joint order for the rows of ``hyp``: the mean function at X with its x-gradient at
        X_g, and [the noise function's variances at X | s2_grad]."""
        from . import _gradobs

        counts = self._counts()
        S, N = hyp.shape[0], self.X.shape[0]
        Ng, D = X_g.shape
        idx = _gradobs.order(N, Ng, D)
        pv = self._plugin_values(hyp, False)
        m, sn2 = np.empty((S, N + Ng * D)), np.empty((S, N + Ng * D))
        m[:, :N] = pv["m"]
        sn2[:, :N] = np.broadcast_to(pv["sn2"], (S, N))
        sn2[:, idx] = s2g
        for s in range(S):
            m[s, idx] = _mean_grad_x(self.mean, _mean_hyp(hyp[s], counts), X_g, who)
        return m, sn2

    @_on_device
    def condition_on_gradients(self, X_g, dy, s2_grad):
        """Condition every resident hyperparameter sample on the GP's data (X, y, s2) AND on gradient observations:
        ``dy`` (Ng, D), row g the observed gradient of f at ``X_g[g]`` (rows of ``X_g`` may repeat rows of X), with
        noise variances ``s2_grad`` -- a scalar, (Ng,) or (Ng, D), required, zeros allowed (they take the reference's
        low-noise branch by its own rule min(sn2) < 1e-6).  Returns a ``GradientConditionedPosterior``; the GP itself --
        its posteriors, its data -- is not modified.  The joint covariance of order n = N + Ng D and the n x M operand
        of every prediction are built on the device (gpc_posterior_batch_gobs / gpc_predict_gobs); the factorization,
        the jitter ladder and the solves are those of every other posterior.  Built-in covariance functions except the
        Matern kernel of degree 1 (NotImplementedError); ``LinAlgError`` after ten failed factorizations.  Not
        sharded: every rank holds every sample's hyperparameters, and the calling rank computes all of them."""
        who = "condition_on_gradients"
        X_g, dy, s2g = self._grad_obs_inputs(who, X_g, dy, s2_grad)
        if self.posteriors is None or len(self.posteriors) == 0 or any(p is None for p in self.posteriors):
            raise ValueError(f"{who}: the GP has no posteriors; call update() or set_hyperparameters() first")
        self._require_posteriors()  # (conditions on the RESIDENT samples: a GP whose posteriors were never computed, or cleaned, is refused)
        hyp = np.stack([np.array(p.hyp, dtype=float) for p in self.posteriors])
        nlz, handle, mult, lchol = self._grad_obs_device(who, hyp, X_g, dy, s2g, True)
        return GradientConditionedPosterior(handle, self.mean, self.noise, self._counts(), list(hyp),
                                            (self.X.shape[0], X_g.shape[0], self.D), nlz, mult, lchol)

    @_on_device
    def nll_batch_grad_obs(self, hyp, X_g, dy, s2_grad, compute_grad=False):
        """The joint negative log marginal likelihood of the GP's data and the gradient observations (arguments as
        ``condition_on_gradients``) for MANY hyperparameter vectors: ``hyp`` (S, hyp_N) -> nlZ (S,).  Priors are not
        added: the joint counterpart of ``nll_batch``.  Not sharded.

        With ``compute_grad`` the result is (nlZ (S,), dnlZ (S, hyp_N)), dnlZ ordered [cov | noise | mean] as
        ``nll_batch``'s: the analytic gradient at each sample's own jitter multiplier, held fixed.  Its covariance part,
        1/2 sum ((K + Sigma)^-1 - alpha alpha^T) o dK/dtheta, is contracted on the device with every dK entry evaluated
        from the points (gpc_nll_batch_gobs_grad; ``_gradobs`` has the formulas): no derivative plane is formed.
        ``s2_grad`` is data and has no gradient.  nlZ is the number the call without gradient returns, to the bit (a
        second, inverse-free factorization supplies it, as for ``nll_hess_batch``).  The gradient needs a built-in
        covariance function (not Matern 1), the stock ``GaussianNoise``, a stock mean function and a float64 GP:
        ``NotImplementedError`` names what is missing."""
        who = "nll_batch_grad_obs"
        X_g, dy, s2g = self._grad_obs_inputs(who, X_g, dy, s2_grad)
        if compute_grad:
            self._grad_obs_grad_check(who)
        hyp = np.atleast_2d(np.asarray(hyp, dtype=float))
        if hyp.ndim != 2 or hyp.shape[1] != sum(self._counts()):
            raise ValueError("Input hyperparameter array is the wrong shape!")
        if not np.all(np.isfinite(hyp)):
            raise ValueError(f"{who}: hyp must be finite")
        nlz = self._grad_obs_device(who, hyp, X_g, dy, s2g, False)[0]
        if not compute_grad:
            return nlz
        return nlz, self._grad_obs_grad(who, hyp, X_g, s2g)

    def _grad_obs_grad_check(self, who):
        """The refusals of the gradient of the gradient-observation likelihood beyond ``_grad_obs_inputs``'."""
        from .mean_functions import ConstantMean, NegativeQuadratic, ZeroMean
        from .noise_functions import GaussianNoise

        if self.dtype not in ("f64", "fp64", "float64"):
            raise NotImplementedError(f"{who}: the gradient is computed in fp64 only; this GP's dtype is {self.dtype!r}")
        if type(self.noise) is not GaussianNoise:
            raise NotImplementedError(f"{who}: the noise function {self.noise!r} ({type(self.noise).__name__}) is "
                                      "user-defined; the gradient needs the stock GaussianNoise")
        if type(self.mean) not in (ZeroMean, ConstantMean, NegativeQuadratic):
            raise NotImplementedError(f"{who}: the mean function {self.mean!r} ({type(self.mean).__name__}) is "
                                      "user-defined; the derivatives of its x-gradient with respect to the "
                                      "hyperparameters are unknown")

    def _grad_obs_grad(self, who, hyp, X_g, s2g):
        """dnlZ (S, hyp_N) of the joint systems of the rows of ``hyp``; the joint data are resident (``_grad_obs_device``
        ran in the same locked call)."""
        from . import _gradobs
        from .mean_functions import ConstantMean, ZeroMean

        counts = cov_N, noise_N, mean_N = self._counts()
        kid, degree = self._kid()
        S, N = hyp.shape[0], self.X.shape[0]
        Ng, D = X_g.shape
        m, sn2 = self._grad_obs_rows(who, hyp, X_g, s2g)
        pv = self._plugin_values(hyp, True)
        name = {ZeroMean: "zero", ConstantMean: "const"}.get(type(self.mean), "negquad")
        dm = dsn2 = None
        if mean_N:
            dm = np.stack([_gradobs.joint_dm(pv["dm"][s], _gradobs.mean_xgrad_dhyp(name, _mean_hyp(hyp[s], counts), X_g))
                           for s in range(S)])
        if noise_N:
            dsn2 = np.stack([_gradobs.joint_dsn2(pv["dsn2"][s], N, Ng, D) for s in range(S)])
        ctx = _lib.context(self.device)
        if ctx.gobs != (N, Ng):  # (cannot happen: the value call above made them resident under this lock)
            raise RuntimeError(f"{who}: the joint data are not resident")
        _, dnlz, _, _, info = ctx.nll_batch_gobs_grad(kid, degree, _lib.F64, hyp[:, :cov_N], m, sn2, dm, dsn2)
        if np.any(info != 0):
            raise LinAlgError("Singular matrix for L Cholesky decomposition")
        return dnlz

    def _grad_obs_objective(self, who, hyp, X_g, dy, s2_grad, compute_grad, prior):
        """``log_likelihood_grad_obs`` / ``log_posterior_grad_obs``: one vector (array or dict), the sign of
        ``log_likelihood``."""
        if isinstance(hyp, dict):
            hyp = self.hyperparameters_from_dict(hyp)[0]
        hyp = np.asarray(hyp, dtype=float).ravel()
        r = self.nll_batch_grad_obs(hyp[None, :], X_g, dy, s2_grad, compute_grad)
        nlZ = float((r[0] if compute_grad else r)[0])
        dnlZ = r[1][0] if compute_grad else None
        if prior:
            if compute_grad:
                P, dP = self.__compute_log_priors(hyp, True)
                nlZ -= P
                dnlZ = dnlZ - dP
            else:
                nlZ -= self.__compute_log_priors(hyp, False)
        return (-nlZ, -dnlZ) if compute_grad else -nlZ

    def log_likelihood_grad_obs(self, hyp, X_g, dy, s2_grad, compute_grad=False):
        """(Positive) joint log marginal likelihood of the GP's data and the gradient observations at ONE
        hyperparameter vector (array or dict): ``log_likelihood``'s joint counterpart, (lZ, dlZ) with ``compute_grad``."""
        return self._grad_obs_objective("log_likelihood_grad_obs", hyp, X_g, dy, s2_grad, compute_grad, False)

    def log_posterior_grad_obs(self, hyp, X_g, dy, s2_grad, compute_grad=False):
        """Joint log marginal likelihood plus log prior: ``log_posterior``'s joint counterpart.  The negated pair
        ``lambda h: tuple(-v for v in gp.log_posterior_grad_obs(h, X_g, dy, s2_grad, True))`` is an objective for
        ``scipy.optimize.minimize(jac=True)``."""
        return self._grad_obs_objective("log_posterior_grad_obs", hyp, X_g, dy, s2_grad, compute_grad, True)

    def _grad_obs_device(self, who, hyp, X_g, dy, s2g, keep):
        """(nlZ, handle | None, sn2_mult, L_chol) of the joint systems of the rows of ``hyp``.  The context's resident
        data become the joint data under a token of their own, so this GP (and any other) uploads its own again on
        its next call."""
        cov_N = self._counts()[0]
        kid, degree = self._kid()
        m, sn2 = self._grad_obs_rows(who, hyp, X_g, s2g)
        ctx = _lib.context(self.device)
        ctx.set_data_gobs(self.X, self.y, X_g, dy, token=object())
        args = (kid, degree, _DTYPES[self.dtype], hyp[:, :cov_N], m, sn2)
        handle = None
        if keep:
            handle, _, mult, lchol, info = ctx.posterior_batch_gobs(*args)
            if np.any(info != 0):
                handle.free()
                raise LinAlgError("Singular matrix for L Cholesky decomposition")
        try:
            # (nlZ always from the evaluation without the inverse: ONE number for the object and for nll_batch_grad_obs)
            nlz, mult_n, lchol_n, info = ctx.nll_batch_gobs(*args)
        except Exception:
            if handle is not None:
                handle.free()
            raise
        if np.any(info != 0):
            if handle is not None:
                handle.free()
            raise LinAlgError("Singular matrix for L Cholesky decomposition")
        if not keep:
            mult, lchol = mult_n, lchol_n
        return nlz, handle, mult, lchol

    @staticmethod
    def _jittered_cholesky(C, s):
        """(L, tau): the lower Cholesky factor of C + tau I, tau = 0 when C itself factors, else the first of
        t mean(diag C), t = 1e-12, 1e-11, ..., 1e-6 that does (``draw_functions``' ladder; LinAlgError names sample s)."""
        try:
            return np.linalg.cholesky(C), 0.0
        except np.linalg.LinAlgError:
            pass
        mean = np.sum(np.diag(C)) / C.shape[0]
        for e in range(-12, -5):
            tau = 10.0**e * mean
            try:
                return np.linalg.cholesky(C + tau * np.eye(C.shape[0])), tau
            except np.linalg.LinAlgError:
                pass
        raise np.linalg.LinAlgError(f"draw_functions: the prior covariance of sample {s} is not positive definite, "
                                    "even with a jitter of 1e-6 mean(diag C)")

    @staticmethod
    def _robust_factor(C):
        """T with T^T T = C for a covariance matrix that may have lost definiteness to rounding (reference
        ``__robust_cholesky``, :2331-2355): the upper Cholesky factor when LAPACK finds one; otherwise from the
        eigen-decomposition of the symmetric part, without the directions whose eigenvalue is within n ulp of the
        largest -- and a zero matrix (nothing to draw from) when a negative eigenvalue survives that cut."""
        import scipy.linalg as sla

        try:
            return sla.cholesky(C, check_finite=False)
        except sla.LinAlgError:
            pass
        w, V = sla.eig((C + C.T) / 2)
        # the reference's sign step as written (:2338-2340): with r_i the row in which column i is largest, element
        # (i, j) of the eigenvector matrix changes sign when V[r_i, j] is negative
        at_max = np.argmax(np.abs(V), axis=0)
        V = np.where(V[at_max] < 0, -V, V)
        w = np.real(w)
        keep = np.abs(w) > np.abs(np.spacing(np.max(w))) * w.shape[0]
        w = w[keep]
        if np.any(w < 0):
            return np.zeros(C.shape)
        return np.dot(np.diag(np.sqrt(w)), np.real(V[:, keep]).T)

    def __repr__(self):
        """The reference's attribute dump (``self.<name> = <summary>``, :64-81 with ``formatting.full_repr``): the public
        attributes in its order, small arrays printed with four decimals, large ones by shape; device handles and other
        private fields are left out."""
        def short(v):
            if type(v) is dict:
                return object.__repr__(v)
            if not isinstance(v, np.ndarray):
                return repr(v)
            if v.dtype != object and v.size < 10:
                txt = np.array2string(v, precision=4, suppress_small=True, separator=", ")
                if "\n" in txt:
                    txt = indent("\n" + txt, "    ")
                return txt + " : " + type(v).__name__
            return str(v.shape) + " " + type(v).__name__

        first = ["D", "covariance", "mean", "noise", "X", "y", "s2", "lower_bounds", "upper_bounds", "posteriors"]
        rest = sorted(k for k in self.__dict__ if not k.startswith("_") and k not in first)
        lines = ["self.%s = %s" % (k, short(getattr(self, k, None))) for k in first + rest]
        return "GP:\n" + indent(",\n".join(lines), "    ")

    @_on_device
    def quad(self, mu, sigma, compute_var: bool = False, separate_samples: bool = False):
        """Bayesian quadrature of the GP against Gaussian measures N(mu_j, diag(sigma_j^2))
        (reference :1818-1981; squared-exponential kernels only).  The kernel-mean vectors z,
        z.alpha and z (K + sn2 I)^-1 z^T are computed on the device for all samples."""
        from .covariance_functions import SquaredExponential
        from .mean_functions import NegativeQuadratic, ZeroMean

        if not isinstance(self.covariance, SquaredExponential):
            raise ValueError("Bayesian quadrature only supports the squared exponential kernel.")
        N, D = self.X.shape
        N_s = np.size(self.posteriors)
        cov_N, noise_N, _ = self._counts()
        mu, sigma = _quad_measures(mu, sigma, D)
        N_star = mu.shape[0]
        self._require_posteriors()
        self._ctx()  # (before the probe below, as ever: a GP without targets is refused first)
        quirks = self.reference_quirks
        iso = cov_N == 2 and D != 1
        if quirks:  # the reference evaluates exp(2 hyp[cov_N]) for every sample, variance or not: without a noise
            for p in self.posteriors:  # hyperparameter that is a mean hyperparameter, or an IndexError (:1921)
                np.exp(2 * p.hyp[cov_N])

        def call(handle, local_posts, lo):
            if quirks and iso:
                # the reference reads hyp[0:D] as length scales and hyp[D] as the output scale whatever the kernel
                # (:1898-1903): with an isotropic kernel's two hyperparameters that is [ell, sf, ...] taken for D length
                # scales.  Its kernel-mean vectors z, built here on the host from that reading, against the device's
                # factors.
                Z = np.empty((len(local_posts), N, N_star))
                for k, p in enumerate(local_posts):
                    tau = np.sqrt(sigma**2 + np.exp(p.hyp[0:D])**2)
                    lnnf = 2 * p.hyp[D] + np.sum(p.hyp[0:D]) - np.sum(np.log(tau), 1)
                    d2 = np.zeros((N_star, N))
                    for i in range(D):
                        d2 += ((mu[:, i] - np.reshape(self.X[:, i], (-1, 1))).T / tau[:, i:i + 1]) ** 2
                    Z[k] = np.exp(np.reshape(lnnf, (-1, 1)) - 0.5 * d2).T
                za, fq, _ = handle.predict_K(Z, want_var=compute_var)
                zkz = None if fq is None else -fq  # fq = -z (K + Sigma)^-1 z^T (the variance term of predict)
            else:
                za, zkz = handle.quad(mu, sigma, compute_var)
            if not compute_var:
                return [za]
            if quirks:
                zkz *= self._quad_solve_scales(local_posts, cov_N)
            return za, zkz

        r = self._device_rows(call, [("za", (N_star,))] + ([("zkz", (N_star,))] if compute_var else []), mu, sigma)
        za, zkz = r["za"], r.get("zkz")
        quadratic = isinstance(self.mean, NegativeQuadratic)
        F = np.zeros((N_star, N_s))
        F_var = np.zeros((N_star, N_s)) if compute_var else None
        for s in range(N_s):
            hyp = self.posteriors[s].hyp
            if quirks:  # (:1901-1903 as written)
                ell, ln_sf2 = np.exp(hyp[0:D]), 2 * hyp[D]
            else:
                ell = np.exp(hyp[0]) * np.ones(D) if iso else np.exp(hyp[0:D])
                ln_sf2 = 2 * hyp[cov_N - 1]
            sum_lnell = np.sum(np.log(ell))
            m0 = 0 if isinstance(self.mean, ZeroMean) else hyp[cov_N + noise_N]
            F[:, s] = za[:, s] + m0
            if quadratic:
                xm = hyp[cov_N + noise_N + 1:cov_N + noise_N + D + 1]
                omega = np.exp(hyp[cov_N + noise_N + D + 1:])
                F[:, s] += -0.5 * np.sum(1 / omega**2 * (mu**2 + sigma**2 - 2 * mu * xm + xm**2), 1)
            if compute_var:
                tau_kk = np.sqrt(2 * sigma**2 + ell**2)
                nf_kk = np.exp(ln_sf2 + sum_lnell - np.sum(np.log(tau_kk), 1))
                F_var[:, s] = np.maximum(np.spacing(1), nf_kk - zkz[:, s])
        if N_s > 1 and not separate_samples:  # (:1968-1976) the same mixture as in predict
            F, F_var, _ = _mix_samples(F, F_var)
        return (F, F_var) if compute_var else F

    @_on_device
    def quad_grad(self, mu, sigma, compute_var: bool = False, separate_samples: bool = False):
        """``quad`` and its gradients with respect to the measures' means ``mu`` and standard deviations ``sigma``:
        (F, dF_dmu, dF_dsigma), or with ``compute_var`` (F, F_var, dF_dmu, dF_dsigma, dFvar_dmu, dFvar_dsigma).  F is
        ``quad``'s to the bit, F_var to rounding (the device sums the variance in another order).  The gradients are
        (M, D), or (M, D, S) with ``separate_samples``, entry [j, l] the derivative with respect to mu[j, l] or
        sigma[j, l] of the broadcast per-row arrays (a caller who ties parameters sums them).  The z-terms run on the
        device (gpc_quad_grad); the mean function's terms, the self-term of the variance and the mixture on the host.
        Where the clamp F_var = max(eps, .) is active the variance gradient is 0.  Refuses what ``quad`` refuses, and
        (NotImplementedError) an isotropic kernel at D > 1 under ``reference_quirks``, whose z ``quad`` builds on the
        host from a misread of the hyperparameters."""
        from .covariance_functions import SquaredExponential
        from .mean_functions import NegativeQuadratic, ZeroMean

        if not isinstance(self.covariance, SquaredExponential):
            raise ValueError("Bayesian quadrature only supports the squared exponential kernel.")
        N, D = self.X.shape
        N_s = np.size(self.posteriors)
        cov_N, noise_N, _ = self._counts()
        mu, sigma = _quad_measures(mu, sigma, D)
        N_star = mu.shape[0]
        if mu.shape[1] != D:
            raise ValueError(f"quad_grad: the measures have {mu.shape[1]} dimensions, the GP {D}")
        self._require_posteriors()
        quirks = self.reference_quirks
        iso = cov_N == 2 and D != 1
        if quirks:
            for p in self.posteriors:  # (as quad: an IndexError without a noise hyperparameter)
                np.exp(2 * p.hyp[cov_N])
            if iso:
                raise NotImplementedError("quad_grad: under reference_quirks, quad builds an isotropic kernel's z on the "
                                          "host from a misread of its hyperparameters (D > 1); it has no device gradient")

        def call(handle, local_posts, lo):
            za, zkz, dza_mu, dza_sg, dzkz_mu, dzkz_sg = handle.quad_grad(mu, sigma, compute_var)
            if not compute_var:
                return za, dza_mu, dza_sg
            if quirks:  # quad's rescaling of the variance term
                scale = self._quad_solve_scales(local_posts, cov_N)
                zkz *= scale
                dzkz_mu *= scale
                dzkz_sg *= scale
            return za, dza_mu, dza_sg, zkz, dzkz_mu, dzkz_sg

        layout = [("za", (N_star,)), ("dza_mu", (N_star, D)), ("dza_sg", (N_star, D))]
        if compute_var:
            layout += [("zkz", (N_star,)), ("dzkz_mu", (N_star, D)), ("dzkz_sg", (N_star, D))]
        r = self._device_rows(call, layout, mu, sigma)
        za, dza_mu, dza_sg = r["za"], r["dza_mu"], r["dza_sg"]
        zkz, dzkz_mu, dzkz_sg = r.get("zkz"), r.get("dzkz_mu"), r.get("dzkz_sg")
        quadratic = isinstance(self.mean, NegativeQuadratic)
        F = np.zeros((N_star, N_s))
        F_var = np.zeros((N_star, N_s)) if compute_var else None
        dF_mu, dF_sg = dza_mu.copy(), dza_sg.copy()
        dV_mu = dV_sg = np.zeros((N_star, D, N_s))
        if compute_var:
            dV_mu, dV_sg = -dzkz_mu, np.empty((N_star, D, N_s))
        for s in range(N_s):  # quad's host terms and their derivatives
            hyp = self.posteriors[s].hyp
            if quirks:
                ell, ln_sf2 = np.exp(hyp[0:D]), 2 * hyp[D]
            else:
                ell = np.exp(hyp[0]) * np.ones(D) if iso else np.exp(hyp[0:D])
                ln_sf2 = 2 * hyp[cov_N - 1]
            sum_lnell = np.sum(np.log(ell))
            m0 = 0 if isinstance(self.mean, ZeroMean) else hyp[cov_N + noise_N]
            F[:, s] = za[:, s] + m0
            if quadratic:
                xm = hyp[cov_N + noise_N + 1:cov_N + noise_N + D + 1]
                omega = np.exp(hyp[cov_N + noise_N + D + 1:])
                F[:, s] += -0.5 * np.sum(1 / omega**2 * (mu**2 + sigma**2 - 2 * mu * xm + xm**2), 1)
                dF_mu[:, :, s] -= (mu - xm) / omega**2
                dF_sg[:, :, s] -= sigma / omega**2
            if compute_var:
                tau_kk = np.sqrt(2 * sigma**2 + ell**2)
                nf_kk = np.exp(ln_sf2 + sum_lnell - np.sum(np.log(tau_kk), 1))
                F_var[:, s] = np.maximum(np.spacing(1), nf_kk - zkz[:, s])
                dV_sg[:, :, s] = -nf_kk[:, None] * 2 * sigma / tau_kk**2 - dzkz_sg[:, :, s]
                held = nf_kk - zkz[:, s] <= np.spacing(1)  # the clamp: no variance gradient where it holds F_var
                dV_mu[held, :, s] = 0
                dV_sg[held, :, s] = 0
        if not separate_samples:  # the gradients of quad's mixture (one sample: the sample's own)
            dF_mu, dV_mu = _mix_sample_grads(F, dF_mu, dV_mu)
            dF_sg, dV_sg = _mix_sample_grads(F, dF_sg, dV_sg)
            if N_s > 1:
                F, F_var, _ = _mix_samples(F, F_var)
        if compute_var:
            return F, F_var, dF_mu, dF_sg, dV_mu, dV_sg
        return F, dF_mu, dF_sg

    def _quad_mixture_prepare(self, name, mu, sigma):
        """What ``quad_cov`` and ``quad_mixture`` check before any device work, as ``quad_grad`` does: (mu, sigma, D, N_s,
        cov_N, noise_N, iso)."""
        from .covariance_functions import SquaredExponential

        if not isinstance(self.covariance, SquaredExponential):
            raise ValueError("Bayesian quadrature only supports the squared exponential kernel.")
        D = self.X.shape[1]
        cov_N, noise_N, _ = self._counts()
        mu, sigma = _quad_measures(mu, sigma, D)
        if mu.shape[1] != D:
            raise ValueError(f"{name}: the measures have {mu.shape[1]} dimensions, the GP {D}")
        self._require_posteriors()
        iso = cov_N == 2 and D != 1
        if self.reference_quirks:
            for p in self.posteriors:  # (as quad: an IndexError without a noise hyperparameter)
                np.exp(2 * p.hyp[cov_N])
            if iso:
                raise NotImplementedError(f"{name}: under reference_quirks, quad builds an isotropic kernel's z on the "
                                          "host from a misread of its hyperparameters (D > 1); it has no device form")
        return mu, sigma, D, np.size(self.posteriors), cov_N, noise_N, iso

    def _quad_solve_scales(self, local_posts, cov_N):
        """``quad``'s ``reference_quirks`` rescaling of the solve term, per local sample (1 where it does not apply): the
        factor was scaled by sl = min(sn2) sn2_mult, the reference divides by exp(2 hyp[cov_N]) sn2_mult (:1921-1922,
        :1953-1958): the same thing only when the noise model is its constant term."""
        scale = np.ones(len(local_posts))
        if self.reference_quirks:
            for k, p in enumerate(local_posts):
                if p.L_chol:
                    sl = 1.0 / float(np.ravel(p.sW)[0]) ** 2
                    scale[k] = sl / (np.exp(2 * p.hyp[cov_N]) * p.sn2_mult)
        return scale

    def _quad_mean_terms(self, s, mu, sigma, cov_N, noise_N):
        """The mean function's part of sample s's integrals, as ``quad`` and ``quad_grad`` form it: (nu (M,), dnu_dmu,
        dnu_dsigma (M, D))."""
        from .mean_functions import NegativeQuadratic, ZeroMean

        hyp = self.posteriors[s].hyp
        D = mu.shape[1]
        nu = np.full(mu.shape[0], 0.0 if isinstance(self.mean, ZeroMean) else hyp[cov_N + noise_N])
        if not isinstance(self.mean, NegativeQuadratic):
            return nu, np.zeros(mu.shape), np.zeros(mu.shape)
        xm = hyp[cov_N + noise_N + 1:cov_N + noise_N + D + 1]
        omega = np.exp(hyp[cov_N + noise_N + D + 1:])
        nu = nu - 0.5 * np.sum(1 / omega**2 * (mu**2 + sigma**2 - 2 * mu * xm + xm**2), 1)
        return nu, -(mu - xm) / omega**2, -sigma / omega**2

    @_on_device
    def quad_cov(self, mu, sigma, separate_samples: bool = False):
        """The integrals of the GP against the Gaussian measures N(mu_j, diag(sigma_j^2)) and the covariance between
        them: (F, C) with F (M, S) and C (M, M, S) under ``separate_samples``, else F (M, 1) and C (M, M).
        C_s = Gamma_s - Z^T (K + Sigma)^-1 Z is formed on the device (gpc_quad_cov), symmetrised here and NOT clamped:
        its diagonal is ``quad``'s variance before the clamp.  The mixture over samples is the law of total covariance,
        the mean of the C_s plus the covariance of the F_s (with ``_mix_samples``' 1 / (S - 1)).  Refuses what
        ``quad_grad`` refuses."""
        mu, sigma, D, N_s, cov_N, noise_N, iso = self._quad_mixture_prepare("quad_cov", mu, sigma)
        M = mu.shape[0]

        def call(handle, local_posts, lo):
            za, C = handle.quad_cov(mu, sigma)
            for k, sc in enumerate(self._quad_solve_scales(local_posts, cov_N)):
                if sc != 1.0:  # quirks: Gamma - sc (Gamma - C)
                    hyp = local_posts[k].hyp
                    G = _quad_gamma(mu, sigma, np.exp(hyp[0:D]), 2 * hyp[D])
                    C[k] = G - sc * (G - C[k])
            return za, C.transpose(1, 2, 0)  # (the device's covariances are sample-first)

        za, C = self._device_rows(call, [("za", (M,)), ("C", (M, M))], mu, sigma).values()
        C = np.ascontiguousarray(C)  # (samples innermost, whatever the sharding: the sums below run in one order)
        C = 0.5 * (C + C.transpose(1, 0, 2))
        F = np.stack([za[:, s] + self._quad_mean_terms(s, mu, sigma, cov_N, noise_N)[0] for s in range(N_s)], 1)
        if separate_samples:
            return F, C
        if N_s > 1:
            dev = F - np.sum(F, 1, keepdims=True) / N_s
            C = np.sum(C, 2) / N_s + dev @ dev.T / (N_s - 1)
            F, _, _ = _mix_samples(F, None)
        else:
            C = C[:, :, 0]
        return F, C

    @_on_device
    def quad_mixture(self, mu, sigma, weights, compute_var: bool = False, compute_grad: bool = False,
                     separate_samples: bool = False):
        """Bayesian quadrature against the MIXTURE sum_j w_j N(mu_j, diag(sigma_j^2)): the mean E = sum_j w_j F_j of the
        integral and, with ``compute_var``, its variance V = w^T C w (C as ``quad_cov``), without forming C: the cross
        term collapses to zbar^T (K + Sigma)^-1 zbar with zbar = Z w, one solve per sample (gpc_quad_mix).  The weights
        are any finite reals and are not normalised.  Returns E, then V (``compute_var``), then with ``compute_grad``
        dE_dmu, dE_dsigma (M, D), dE_dw (M,) and, with ``compute_var``, dV_dmu, dV_dsigma, dV_dw of the same shapes.
        E and V are scalars, or (S,) with ``separate_samples``, which also appends a sample axis to every gradient.
        The mean function's terms, the clamp V = max(eps, .) (zero variance gradient where it holds), the mixture over
        samples and the ``reference_quirks`` rescaling are the host's, exactly as in ``quad`` and ``quad_grad``; refuses
        what ``quad_grad`` refuses."""
        from .mean_functions import NegativeQuadratic

        mu, sigma, D, N_s, cov_N, noise_N, iso = self._quad_mixture_prepare("quad_mixture", mu, sigma)
        M = mu.shape[0]
        w = np.asarray(weights, dtype=float).reshape(-1)
        if w.shape != (M,):
            raise ValueError(f"quad_mixture: {M} measures but {w.size} weights")
        if not np.all(np.isfinite(w)):
            raise ValueError("quad_mixture: the weights must be finite")
        var, grad = bool(compute_var), bool(compute_grad)
        layout = [("za", (M,))] + ([("gw", (M,)), ("zq", (M,)), ("zbkzb", ())] if var else [])
        if grad:
            layout += [(n, (M, D)) for n in ["dza_dmu", "dza_dsigma"] +
                       (["dzq_dmu", "dzq_dsigma", "dgw_dmu", "dgw_dsigma"] if var else [])]

        def call(handle, local_posts, lo):
            d = handle.quad_mix(mu, sigma, w, var, grad)
            scale = self._quad_solve_scales(local_posts, cov_N)
            if var and np.any(scale != 1.0):  # quad's rescaling of the solve term
                for n in ("zbkzb", "zq", "dzq_dmu", "dzq_dsigma"):
                    if d[n] is not None:
                        d[n] = d[n] * scale
            return [d[n] for n, _ in layout]

        d = self._device_rows(call, layout, mu, sigma, w)
        # the host terms, for all samples at once; the two dot products with w run per sample on contiguous rows, so
        # that their order of summation -- a sample's bits -- does not depend on the batch
        terms = [self._quad_mean_terms(s, mu, sigma, cov_N, noise_N) for s in range(N_s)]
        F = d["za"] + np.stack([t[0] for t in terms], 1)
        dot_w = lambda A: np.array([w @ row for row in np.ascontiguousarray(A.T)])
        E, V = dot_w(F)[None, :], None
        dE = dV = None
        if grad:
            quadratic = isinstance(self.mean, NegativeQuadratic)
            g_mu = d["dza_dmu"] + np.stack([t[1] for t in terms], 2) if quadratic else d["dza_dmu"]
            g_sg = d["dza_dsigma"] + np.stack([t[2] for t in terms], 2) if quadratic else d["dza_dsigma"]
            dE = [(w[:, None, None] * g_mu).reshape(1, M * D, N_s), (w[:, None, None] * g_sg).reshape(1, M * D, N_s),
                  F[None]]
            if not var:
                dV = [np.zeros_like(g) for g in dE]
        if var:
            gw, zq = d["gw"], d["zq"]
            raw = dot_w(gw) - d["zbkzb"]
            V = np.maximum(np.spacing(1), raw)[None, :]
            if grad:  # the clamp: no variance gradient where it holds V
                free = raw > np.spacing(1)
                w2 = (2 * w)[:, None, None]
                dV = [np.where(free, w2 * (d["dgw_dmu"] - d["dzq_dmu"]), 0.0).reshape(1, M * D, N_s),
                      np.where(free, w2 * (d["dgw_dsigma"] - d["dzq_dsigma"]), 0.0).reshape(1, M * D, N_s),
                      np.where(free, 2 * gw - 2 * zq, 0.0)[None]]
        if separate_samples:
            out = [E[0]] + ([V[0]] if var else [])
            shaped = lambda g: [g[0][0].reshape(M, D, N_s), g[1][0].reshape(M, D, N_s), g[2][0]]
        else:  # quad's mixture and its gradients (one sample: the sample's own)
            if grad:
                mixed = [_mix_sample_grads(E, a, b) for a, b in zip(dE, dV)]
                dE, dV = [m[0] for m in mixed], [m[1] for m in mixed]
            if N_s > 1:
                E, V, _ = _mix_samples(E, V)
            out = [float(E[0, 0])] + ([float(V[0, 0])] if var else [])
            shaped = lambda g: [g[0][0].reshape(M, D), g[1][0].reshape(M, D), g[2][0]]
        if grad:
            out += shaped(dE) + (shaped(dV) if var else [])
        return out[0] if len(out) == 1 else tuple(out)

    # ------------------------------------------------------------------ misc
    def _convert_shapes(self, X, y, s2):
        """Inputs (M, D), observations and per-point noise as columns (M, 1) -- M taken from ``X`` when it is given,
        from the GP's own data otherwise (reference :2523-2565: same conversions, same exceptions)."""
        given = [v is not None for v in (X, y, s2)]
        if not any(given):
            return X, y, s2
        if given[0]:
            X = X[None, :] if X.ndim == 1 else X  # one point may come as a flat vector
            if X.ndim != 2:
                raise AssertionError("X need to be an array of shape (N, D)")
            if X.shape[1] != self.D:
                raise AssertionError(
                    f"The dimension of input data {X.shape[1]}doesn't match GP's input dimension {self.D}.")
            rows = X.shape[0]
        elif isinstance(self.X, np.ndarray):
            rows = self.X.shape[0]
        else:
            raise AttributeError(f"self.X is not a numpy array, self.X = {self.X}")
        column = (rows, 1)
        if given[1]:
            y = y.reshape(column)
        if given[2]:
            if isinstance(s2, np.ndarray):
                s2 = s2.reshape(column)
            elif isinstance(s2, (float, int)):
                s2 = s2 * np.ones(column)  # one noise level for every point
            else:
                raise TypeError("s2 type need to be Union[np.ndarray, float, int, None].")
        return X, y, s2

    def __str__(self):
        """The reference's summary (:83-139), character for character -- including its line break after a Matern
        degree and its rule for the commas between the noise flags (only when ``constant_add`` is set)."""
        cov_N, noise_N, mean_N = self._counts()
        count = lambda n: ", " + str(n) + (" parameter\n" if n == 1 else " parameters\n")
        cov = "Covariance function: " + self.covariance.__class__.__name__
        if self.covariance.__class__.__name__ == "Matern":
            cov += "(degree=" + str(self.covariance.degree) + ")\n"
        noise = "Noise function: " + self.noise.__class__.__name__
        par = getattr(self.noise, "parameters", None)
        if par is not None and np.any(par):
            const, provided, rect = (int(v) for v in par)
            shown = [t for t, on in (("constant_add=True", const == 1), ("user_provided_add=True", provided == 1),
                                     ("scale_user_provided=True", provided == 2),
                                     ("rectified_linear_output_dependent_add=True", rect == 1)) if on]
            sep = ", " if const == 1 else ""
            noise += "(" + shown[0] + "".join(sep + t for t in shown[1:]) + ")"
        body = (
            "Dimension: " + str(self.D) + "\n"
            + cov + count(cov_N)
            + "Mean function: " + self.mean.__class__.__name__ + count(mean_N)
            + noise + count(noise_N)
            + "Hyperparameter priors: " + ("none\n" if self.no_prior else "present\n")
            + "Hyperparameter samples: "
            + ("0" if self.posteriors is None else str(np.size(self.posteriors)))
        )
        return "GP:\n" + indent(body, "    ")

    def __del__(self):  # pragma: no cover
        try:
            self._drop_handle()
        except Exception:
            pass
