"""One line per posterior consumer: name, dtype, output shapes and the sha256 of the raw bytes of all outputs.

    GPYREG_AMD_LIB=<some build of libgpcore.so> python tools/consumer_digest.py [out.txt]

The library documents fixed reduction orders and no atomics, so two builds that launch the same kernels in the same order
print the same lines; a refactor of the host code is checked by diffing the output of the build before against the build
after (tools/build_ref.sh builds the former); a refactor of the Python side by running this file from a checkout of the
commit before and from the tree (it imports the package of the tree it lies in) on one library.  Public Python API only, seeded data, the smallest shapes that reach each
branch: D = 3 and S = 4 hyperparameter samples whose noise is high, low, low, high (low: below the 1e-6 at which the
posterior stores -(K + Sigma)^-1 instead of the Cholesky factor), i.e. runs of 1, 2, 1 samples; N = 200 (N_pad 256),
M = 70 (M_pad 128).  Every call runs once with all samples in one chunk and once under a GPC_MEM_BUDGET_MB picked from
the call's scratch per sample so that the samples go in chunks of 3 + 1 where whole megabytes allow it (else 2 + 2 or
1 + 1 + 1 + 1; the line says which): non-resident constants, a partial last chunk, runs cut at the chunk border.
Then the epilogue-reduced forms (N = M = 1000, at least 64 128-tiles), a posterior built from a covariance object (the
caller's K), and evaluations and posteriors under a forced budget."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import scratch_sizes as ss  # noqa: E402  (the scratch per sample of every consumer, as closed forms)

from gpyreg_amd import _lib  # noqa: E402

if os.environ.get("GPYREG_AMD_LIB"):  # an older build lacks the debug entries added since: bind what it exports
    import ctypes

    probe = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SIGNATURES if n.startswith("gpc_debug_") and not hasattr(probe, n)]:
        del _lib.SIGNATURES[name]

import gpyreg_amd as gpr  # noqa: E402

D, S, N, M, MB, R_DRAW, R_PATHS, F = 3, 4, 200, 70, 130, 5, 40, 96
SN2 = (1e-2, 5e-7, 5e-7, 4e-3)
OUT = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


pad = ss.pad


def emit(name, dtype, outs, note=""):
    outs = [np.ascontiguousarray(o) for o in (outs if isinstance(outs, (tuple, list)) else (outs,)) if o is not None]
    h = hashlib.sha256()
    for o in outs:
        h.update(o.tobytes())
    line = f"{name:44s} {dtype} {'+'.join('x'.join(map(str, o.shape)) for o in outs):42s} {h.hexdigest()}{note}"
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def budget_mb(per, shared=0):
    """(MB, chunk): whole megabytes whose 80 % hold three samples' scratch beside `shared`, else the most below three."""
    best = None
    for mb in range(1, 4096):
        b = int((mb << 20) * 0.8)
        chunk = 0 if b < shared + per else min(S, (b - shared) // per)
        if chunk == 3:
            return mb, 3
        if 1 <= chunk < 3:
            best = (mb, chunk)
        if chunk > 3:
            break
    return best or (1, S)  # (scratch so small that one megabyte holds all samples: the forced path, one chunk)


def both(name, dtype, call, per, shared=0):
    """`call` with every sample in one chunk, then under the budget that chunks the samples."""
    emit(name, dtype, call())
    mb, chunk = budget_mb(per, shared)
    os.environ["GPC_MEM_BUDGET_MB"] = str(mb)
    try:
        emit(name + " [chunked]", dtype, call(), f"  budget {mb} MB, chunks of {chunk}")
    finally:
        del os.environ["GPC_MEM_BUDGET_MB"]


def make_gp(kernel, dtype, cov=None):
    cov = cov or (gpr.covariance_functions.SquaredExponential() if kernel == "se" else gpr.covariance_functions.Matern(5))
    return gpr.GP(D, cov, gpr.mean_functions.ConstantMean(), gpr.noise_functions.GaussianNoise(constant_add=True),
                  dtype=dtype)


def data(n, seed=21):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-3, 3, (n, D))
    y = np.sin(X.sum(1, keepdims=True)) + 0.05 * rng.standard_normal((n, 1))
    return X, y


def hyps(sn2s):
    rng = np.random.default_rng(5)
    return np.array([np.r_[0.05 * rng.standard_normal(D), 0.0, 0.5 * np.log(v), 0.1] for v in sn2s])


def problem(kernel, dtype, n=N, sn2s=SN2, cov=None):
    X, y = data(n)
    gp = make_gp(kernel, dtype, cov)
    gp.update(X_new=X, y_new=y, hyp=hyps(sn2s))
    kinds = [bool(p.L_chol) for p in gp.posteriors]
    assert kinds == [v >= 1e-6 for v in sn2s], kinds
    if len(sn2s) == 4:  # both kinds, in runs of 1, 2, 1
        assert kinds == [True, False, False, True], kinds
    return gp, X, y


def posterior_state(gp):
    return [a for p in gp.posteriors for a in (p.alpha, np.asarray(p.L), np.atleast_1d(p.sn2_mult))]


class PySE:
    """SE-ARD through the covariance-object protocol, NumPy only: the library gets K and Ks from here (K-mode)."""

    def hyperparameter_count(self, d):
        return d + 1

    def hyperparameter_info(self, d):
        return [("covariance_log_lengthscale", d), ("covariance_log_outputscale", 1)]

    def get_bounds_info(self, X, y):
        d = X.shape[1]
        return {"LB": np.full(d + 1, -10.0), "UB": np.full(d + 1, 10.0), "PLB": np.full(d + 1, -2.0),
                "PUB": np.full(d + 1, 2.0), "x0": np.zeros(d + 1)}

    def compute(self, hyp, X, X_star=None, compute_diag=False, compute_grad=False):
        n, d = X.shape
        ell, sf2 = np.exp(hyp[:d]), np.exp(2 * hyp[d])
        if compute_diag:
            return sf2 * np.ones((n, 1))
        Xs = X / ell
        Ys = Xs if X_star is None else X_star / ell
        K = sf2 * np.exp(-0.5 * ((Xs[:, None, :] - Ys[None, :, :]) ** 2).sum(2))
        if not compute_grad:
            return K
        dK = np.stack([K * (Xs[:, k:k + 1] - Xs[:, k:k + 1].T) ** 2 for k in range(d)] + [2 * K], axis=2)
        return K, dK


def consumers(dtype):
    w = 8 if dtype == "f64" else 4
    ctx = _lib.context()
    npad, mpad, mbpad = pad(N), pad(M), pad(MB)
    rng = np.random.default_rng(3)
    xq, xb = rng.uniform(-3, 3, (M, D)), rng.uniform(-3, 3, (MB, D))
    mu, sigma = rng.uniform(-2, 2, (M, D)), rng.uniform(0.3, 1.2, (M, D))
    wm, ws = rng.uniform(0, 1, M), rng.uniform(0, 1, (M, S))
    gp, X, y = problem("se", dtype)

    def rhs(kind="cross", want_quad=True, full=False, grad=False, qg=False, R=0):
        return (ss.rhs_per(npad, mpad, full, w, D, kind, want_quad, grad, qg, M, R),
                ss.rhs_shared(N, M, D, S, kind, full, qg, R))

    both("predict", dtype, lambda: gp.predict(xq, separate_samples=True), *rhs())
    both("predict_grad", dtype, lambda: gp.predict_grad(xq, separate_samples=True), *rhs(grad=True))
    both("predict_full", dtype, lambda: gp.predict_full(xq), *rhs(want_quad=False, full=True))
    cov_per = ss.cov_per(npad, mpad, mbpad, D, w)
    both("predict_cov", dtype, lambda: gp.predict_cov(xq, xb), cov_per, ss.cov_shared(M, MB, D, True))
    both("lookahead_variance shared weights", dtype,
         lambda: gp.lookahead_variance(xb, xq, weights=wm, separate_samples=True), cov_per, ss.cov_shared(M, MB, D, False))
    both("lookahead_variance per-sample weights", dtype,
         lambda: gp.lookahead_variance(xb, xq, weights=ws, separate_samples=True), cov_per, ss.cov_shared(M, MB, D, False))
    both("draw_functions", dtype, lambda: gp.draw_functions(xq, n_draws=R_DRAW, seed=11),
         *rhs(want_quad=False, full=True, R=R_DRAW))
    both("quad", dtype, lambda: gp.quad(mu, sigma, compute_var=True, separate_samples=True), *rhs("quad"))
    both("quad_grad with variance", dtype, lambda: gp.quad_grad(mu, sigma, compute_var=True, separate_samples=True),
         *rhs("quad", grad=True, qg=True))
    both("quad_grad", dtype, lambda: gp.quad_grad(mu, sigma, compute_var=False, separate_samples=True),
         *rhs("quad", want_quad=False, grad=True, qg=True))
    both("quad_cov", dtype, lambda: gp.quad_cov(mu, sigma, separate_samples=True), *rhs("quad", want_quad=False, full=True))
    both("quad_mixture with variance and gradient", dtype,
         lambda: gp.quad_mixture(mu, sigma, wm, compute_var=True, compute_grad=True, separate_samples=True),
         ss.quad_mix_per(npad, mpad, D, True, True), ss.quad_mix_shared(M, mpad, D))
    # gradient_posterior and predict_hess: one block of 128 queries
    for cov in ("full", "diag"):
        for val in (False, True):
            both(f"gradient_posterior {cov}" + (" with value" if val else ""), dtype,
                 lambda: gp.gradient_posterior(xq, cov=cov, with_value=val, separate_samples=True),
                 ss.grad_post_per(npad, D, cov == "diag", w), M * D * 8)
    for var in (True, False):
        both("predict_hess" + ("" if var else " without variance"), dtype,
             lambda: gp.predict_hess(xq, compute_var=var, separate_samples=True), ss.predict_hess_per(npad, D, var, w), M * D * 8)
    # cv_predict: the leave-one-out pass (five vectors per sample: one megabyte holds every sample), and three scattered
    # folds of 5, 9 and 3 points
    both("cv_predict leave-one-out", dtype, lambda: gp.cv_predict(None, separate_samples=True, return_lpd=True),
         ss.cv_loo_per(npad))
    order = np.random.default_rng(9).permutation(N)
    folds = [np.sort(order[:5]), np.sort(order[5:14]), np.sort(order[14:17])]
    per = ss.cv_fold_per(npad, len(folds), 9, 1)
    both("cv_predict scattered folds", dtype, lambda: gp.cv_predict(folds, separate_samples=True), per)
    both("cv_predict scattered folds with lpd", dtype, lambda: gp.cv_predict(folds, return_lpd=True), per)
    # cv_nll_batch on the resident posteriors (fp64 only); the weights are shared by the samples
    if dtype == "f64" and hasattr(gp, "cv_nll_batch"):
        for loss in ("lpd", "mse"):
            both(f"cv_nll_batch {loss}", dtype, lambda: gp.cv_nll_batch(loss=loss, weights=wm.repeat(3)[:N]),
                 ss.cv_grad_per(npad, D + 1), npad * 8)
    # nll_hess_batch and predict_hyp_grad on the resident posteriors (fp64 only), P = cov_N + one noise + one mean
    # hyperparameter; one block of 128 queries
    if dtype == "f64":
        cov_N, P = D + 1, D + 3
        both("nll_hess_batch", dtype, lambda: gp.nll_hess_batch(), ss.nll_hess_per(npad, cov_N, 1, 1, D * (D + 1) // 2))
        for var in (True, False):
            both("predict_hyp_grad" + ("" if var else " without variance"), dtype,
                 lambda: gp.predict_hyp_grad(xq, compute_var=var),
                 ss.hyp_grad_per(npad, D, P, 1, D, mpad, var, P + cov_N * (2 if var else 1)))
    # sample_paths: creation under both solve engines, evaluation with gradients under both engines
    try:
        for solve in (1, 2):
            ctx.set_option("paths_solve_engine", solve)
            made = {}

            def create():
                made["p"] = gp.sample_paths(n_paths=R_PATHS, n_features=F, seed=5)
                return made["p"](xq, compute_grad=True)

            both(f"sample_paths create, solve engine {solve}", dtype, create, ss.paths_create_per(npad, R_PATHS, w, solve))
            for engine in (1, 2):
                ctx.set_option("paths_engine", engine)
                both(f"sample_paths evaluate, engine {engine}", dtype, lambda: made["p"](xq, compute_grad=True),
                     ss.paths_eval_per(npad, mpad, pad(F), R_PATHS, D, engine), ss.paths_eval_shared(M, R_PATHS, S, D, True))
            ctx.set_option("paths_engine", 0)
    finally:
        ctx.set_option("paths_solve_engine", 0)
        ctx.set_option("paths_engine", 0)
    # update: rank one, and blocks of k = 8 and k = BA_GEMM_MIN_K = 17 rows under each engine (a fresh GP each)
    Xn, yn = data(17, seed=8)

    def updated(k, engine, block):
        g2, _, _ = problem("se", dtype)
        ctx.set_option("block_engine", engine)
        try:
            g2.update(X_new=Xn[:k], y_new=yn[:k], block_append=block)
        finally:
            ctx.set_option("block_engine", 0)
        return posterior_state(g2) + list(g2.predict(xq, separate_samples=True))

    emit("update rank-one", dtype, updated(1, 0, False))
    for k in (8, 17):
        for engine in (1, 2):
            both(f"update block_append k={k}, engine {engine}", dtype, lambda: updated(k, engine, True),
                 ss.append_block_per(pad(N + k), k, w, engine))


def large(dtype):
    """The forms that need at least 64 128-tiles: predict's variance and the look-ahead reduced in the products' epilogues."""
    n = m = 1000
    gp, X, y = problem("matern", dtype, n=n, sn2s=(1e-2, 5e-7))
    rng = np.random.default_rng(4)
    xa, xb = rng.uniform(-3, 3, (m, D)), rng.uniform(-3, 3, (m, D))
    emit("predict N=1000 M=1000", dtype, gp.predict(xa, separate_samples=True))
    ctx = _lib.context()
    before = ctx.get_option("cov_fused")
    emit("lookahead_variance N=1000 Ma=Mb=1000", dtype,
         gp.lookahead_variance(xb, xa, weights=rng.uniform(0, 1, m), separate_samples=True))
    assert ctx.get_option("cov_fused") > before, "the look-ahead was not reduced in the product's epilogue"


def caller_k(dtype):
    gp, X, y = problem("se", dtype, cov=PySE())
    xq = np.random.default_rng(3).uniform(-3, 3, (M, D))
    both("predict, posterior from the caller's K", dtype, lambda: gp.predict(xq, separate_samples=True),
         ss.rhs_per(pad(N), pad(M), False, 8 if dtype == "f64" else 4, D, "given"), ss.rhs_shared(N, M, D, S, "given"))


def evaluations(dtype):
    w = 8 if dtype == "f64" else 4
    for n in (200, 1000):
        X, y = data(n)
        hyp = hyps(SN2)
        gp = make_gp("matern", dtype)
        gp.update(X_new=X, y_new=y, hyp=hyp[:1], compute_posterior=False)
        both(f"nll_batch with gradient N={n}", dtype, lambda: gp.nll_batch(hyp, compute_grad=True), 3 * pad(n) ** 2 * w)

        def post():
            gp.update(hyp=hyp)
            return posterior_state(gp)

        both(f"update(hyp) N={n}", dtype, post, pad(n) ** 2 * w)


if __name__ == "__main__":
    print(f"# {_lib.LIB_PATH}", flush=True)
    for dt in ("f64", "f32"):
        consumers(dt)
        large(dt)
        caller_k(dt)
        evaluations(dt)
