"""Shared by tests/test_rhs_ref_cpu.py and tests/test_gpu_rhs_products.py: the extended-precision reference of the four
calls that go through the rhs_products engine of gpcore.hip (gpc_predict, gpc_predict_full, gpc_quad, gpc_predict_K) and
the problems the GPU tests run.  Plain NumPy in np.longdouble (x87 80-bit, eps = 1.1e-19); no device, nothing of the
library.

ONE formula serves both posterior forms (the device keeps W = chol(K / sl + I)^-1 for L_chol samples and L = -A^-1 for
low-noise samples): per sample, from the fp64 values K, Ks, Kss of oracle.gp_oracle.covariance,
  A = K + diag(sn2)  (cast to 80-bit),  L = chol(A),  W = L^-1,  A^-1 = W^T W,  alpha = A^-1 (y - m)
  predict       fmu = Ks^T alpha,  fs2 = kss - diag(Ks^T A^-1 Ks)
  predict_full  C   = Kss - Ks^T A^-1 Ks
  predict_K     the same with the caller's Ks, Kss;  fq = -diag(Ks^T A^-1 Ks), the term the caller adds to kss
  quad          za  = Z^T alpha,  zKz = diag(Z^T A^-1 Z),
                Z_ij = sf2 prod_l (ell_l / tau_jl) exp(-1/2 sum_l ((mu_jl - X_il) / tau_jl)^2),  tau^2 = sigma^2 + ell^2
These are the handle-level quantities: no mean function at the queries, no sample mixing, no clamp.  cond_2(A) comes
with them: eps * cond_2(A) * max |result| is the unit in which the tests state every error."""

import functools

import numpy as np

from oracle import gp_oracle as orc
from oracle.gp_oracle import _chol_ld, _tri_inv_ld

LD = np.longdouble

# ---- the reference of one sample -------------------------------------------------------------------------------------


def quad_z(hyp_cov, X, mu, sigma):
    """Z (N, M) of the SE kernel with hyperparameters hyp_cov = [ln ell_1 .. ln ell_D, ln sf] and the Gaussian measures
    N(mu_j, diag(sigma_j^2)), in 80-bit from the fp64 inputs."""
    D = X.shape[1]
    ell = np.exp(np.asarray(hyp_cov[:D], LD))
    sf2 = np.exp(2 * LD(hyp_cov[D]))
    tau = np.sqrt(np.asarray(sigma, LD) ** 2 + ell ** 2)  # (M, D)
    nf = sf2 * np.prod(ell / tau, axis=1)  # (M,)
    u = (np.asarray(mu, LD)[None, :, :] - np.asarray(X, LD)[:, None, :]) / tau[None, :, :]  # (N, M, D)
    return nf[None, :] * np.exp(-np.sum(u * u, axis=2) / 2)


def cond2(A, W):
    """cond_2 of the symmetric positive definite A from its fp64 eigenvalues, clamped below by the extended-precision
    estimate |A|_F |A^-1|_F / N where fp64 loses the small end (as oracle.gp_oracle.core_extended)."""
    N = A.shape[0]
    ev = np.linalg.eigvalsh(A.astype(np.float64))
    cond = float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf
    if cond < 1e10:  # (fp64 resolves the small end: eigvalsh errs by eps |A|_2, a 1e-6 relative part of it)
        return cond
    Ainv = W.T @ W
    cond_f = float(np.sqrt(np.sum(A * A)) * np.sqrt(np.sum(Ainv * Ainv))) / N
    return max(cond, cond_f) if np.isfinite(cond) else max(cond_f, 1.0)


class SampleRef:
    """The factorization of one sample: A = K + diag(sn2) (sn2 a scalar or (N,), the jitter multiplier included),
    r = y - m (N,)."""

    def __init__(self, K, sn2, r):
        N = K.shape[0]
        A = np.asarray(K, np.float64).astype(LD) + np.diag(np.broadcast_to(np.asarray(sn2, np.float64), (N,)).astype(LD))
        self.W = _tri_inv_ld(_chol_ld(A))
        self.alpha = self.W.T @ (self.W @ np.asarray(r, np.float64).astype(LD).ravel())
        self.cond = cond2(A, self.W)

    def lin(self, R):
        """R^T alpha for a right-hand side R (N, M) (Ks or Z)."""
        return np.asarray(R).astype(LD).T @ self.alpha

    def half(self, R):
        """V = W R: R^T A^-1 R = V^T V."""
        return self.W @ np.asarray(R).astype(LD)

    def quad(self, R):
        """diag(R^T A^-1 R)."""
        V = self.half(R)
        return np.sum(V * V, axis=0)

    def full(self, R, Kss):
        """(Kss - R^T A^-1 R, diag(R^T A^-1 R))."""
        V = self.half(R)
        return np.asarray(Kss).astype(LD) - V.T @ V, np.sum(V * V, axis=0)


# ---- the problems of tests/test_gpu_rhs_products.py -------------------------------------------------------------------

D = 3
S = 5
# L_chol (sn2 >= 1e-6) runs [1], [0, 0], [1], [0]: every run but the first starts at a non-zero sample offset
SN2 = (1e-2, 1e-7, 1e-7, 1e-2, 1e-7)
LCHOL = tuple(v >= 1e-6 for v in SN2)
KERNELS = {"se": ("se", 0), "matern5": ("matern", 5), "rq": ("rq", 0)}  # name -> (oracle kernel, degree)
# npad 128 / 256 / 384, mpad 128 / 256 / 384, the 64-wide column blocks (63 / 64 / 65), the exact tiles (64, 128) and
# the covariance download's pinned landing (M M 8 >= 32 KB: M = 64 is the first pinned size, M = 63 the last unpinned)
SHAPES = [(1, 1), (2, 65), (100, 63), (100, 64), (128, 128), (129, 129), (129, 65), (300, 1), (300, 300)]
BIG = [(129, 129), (300, 300)]
CASES = [("se", n, m) for n, m in SHAPES] + [(k, n, m) for k in ("matern5", "rq") for n, m in BIG]


def problem(kernel, N, M):
    """Inputs of one case (all fp64): X (N, D), y (N, 1), the hyperparameter rows hyp_cov (S, cov_N), the constant
    means m0 (S,), the noise variances sn2 (S,), the queries xs (M, D) and the measures mu, sigma (M, D).

    Three queries (first, middle, last; fewer when N < 3) sit ON training points: for the low-noise samples that is the
    cancellation case sf2 - q ~ sn2.  With M < 3 no query does: the only entries of the output would be the cancelled
    ones, and `scale` (the largest reference entry of that output and sample) would measure the cancellation, not the
    output."""
    rng = np.random.default_rng([N, M, sorted(KERNELS).index(kernel)])
    X = rng.uniform(-3, 3, (N, D))
    y = np.sin(np.sum(X, axis=1, keepdims=True))
    if kernel == "se":
        ell = 0.5 * np.exp(0.05 * rng.standard_normal((S, D)))
    else:
        ell = np.full((S, D), 0.6)
    cols = [np.log(ell), np.zeros((S, 1))]  # sf2 = 1
    if kernel == "rq":
        cols.append(np.zeros((S, 1)))  # alpha = 1
    hyp_cov = np.concatenate(cols, axis=1)
    m0 = 0.1 * (np.arange(S) - 2.0)
    xs = rng.uniform(-3, 3, (M, D))
    if M >= 3:
        for j, i in zip((0, M // 2, M - 1), range(min(3, N))):
            xs[j] = X[i]
    mu = rng.uniform(-1, 1, (M, D))
    sigma = 0.3 + rng.uniform(0, 1, (M, D))
    out = dict(kernel=kernel, N=N, M=M, X=X, y=y, hyp_cov=hyp_cov, m0=m0, sn2=np.array(SN2), xs=xs, mu=mu, sigma=sigma)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(kernel, N, M):
    """The 80-bit reference of one case, computed once: a dict of read-only arrays
      fmu, fs2, fq (M, S), C (S, M, M); for SE also za, zkz (M, S)      np.longdouble
      K (S, N, N), Ks (S, N, M), Kss (S, M, M)                           the oracle's fp64 covariances (predict_K's inputs)
      cond (S,)                                                          cond_2(K_s + sn2_s I)
    and "problem", the inputs."""
    p = problem(kernel, N, M)
    name, degree = KERNELS[kernel]
    out = {k: np.zeros((M, S), LD) for k in ("fmu", "fs2", "fq", "za", "zkz")}
    out.update(C=np.zeros((S, M, M), LD), K=np.zeros((S, N, N)), Ks=np.zeros((S, N, M)), Kss=np.zeros((S, M, M)),
               cond=np.zeros(S))
    for s in range(S):
        h = p["hyp_cov"][s]
        K = orc.covariance(name, h, p["X"], degree=degree)
        Ks = orc.covariance(name, h, p["X"], p["xs"], degree=degree)
        Kss = orc.covariance(name, h, p["xs"], p["xs"], degree=degree)
        ref = SampleRef(K, p["sn2"][s], p["y"][:, 0] - p["m0"][s])
        out["K"][s], out["Ks"][s], out["Kss"][s], out["cond"][s] = K, Ks, Kss, ref.cond
        out["fmu"][:, s] = ref.lin(Ks)
        out["C"][s], q = ref.full(Ks, Kss)
        out["fq"][:, s] = -q
        out["fs2"][:, s] = orc.covariance(name, h, p["xs"], compute_diag=True, degree=degree)[:, 0].astype(LD) - q
        if kernel == "se":
            Z = quad_z(h, p["X"], p["mu"], p["sigma"])
            out["za"][:, s] = ref.lin(Z)
            out["zkz"][:, s] = ref.quad(Z)
    if kernel != "se":
        del out["za"], out["zkz"]
    for v in out.values():
        v.setflags(write=False)
    out["problem"] = p
    return out
