"""quad vs quad_grad on an SE posterior of the cfg3 problem (N = 4096, D = 10, S = 16; bench.synthetic_problem(3, 16),
whose hyperparameters have the SE ARD layout) at M = 50 and M = 1000 measures, plus a seeded PyVBMC-sized case
(N = 400, D = 6, S = 8, M = 50), and quad_grad against the 4 D quad calls of central differences (GPU box).

    python tools/quad_grad_bench.py [--out profiles/quad_grad_cfg3.json] [--reps 5]

Wall time per call (median of --reps after one warm-up call) and the device time of the call (gpc_last_timing: whole
call, and its N^2 M products; recorded at every size: the small-problem timing option is switched on)."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import bench  # noqa: E402


def _time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def _se_gp(X, y, hyp):
    import gpyreg_amd as gpr

    gp = gpr.GP(X.shape[1], gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, hyp=hyp)
    return gp


def _pyvbmc_problem():
    """N = 400 points of a D = 6 log density, S = 8 hyperparameter samples around a fitted-looking set."""
    rng = np.random.default_rng(2024)
    N, D, S = 400, 6, 8
    X = rng.standard_normal((N, D)) * 1.5
    y = -0.5 * np.sum(X**2, 1, keepdims=True) + 0.01 * rng.standard_normal((N, 1))
    base = np.r_[np.log(1.2) * np.ones(D), np.log(3.0), np.log(0.01), 0.0]
    return X, y, base + 0.05 * rng.standard_normal((S, base.size))


def _row(gp, X, M, reps, tag):
    from gpyreg_amd import _lib

    ctx = _lib.context(gp.device)
    D = X.shape[1]
    rng = np.random.default_rng(1)
    mu = X[rng.choice(X.shape[0], M, replace=False)] + 0.1 * rng.standard_normal((M, D))
    sigma = rng.uniform(0.2, 1.0, (M, D))
    out = {}
    for key, fn in (("quad_var", lambda: gp.quad(mu, sigma, compute_var=True)),
                    ("quad_grad", lambda: gp.quad_grad(mu, sigma)),
                    ("quad_grad_var", lambda: gp.quad_grad(mu, sigma, compute_var=True))):
        out[key + "_ms"] = _time(fn, reps)
        tot, prod = ctx.last_timing()
        out["device_" + key + "_ms"] = dict(total=tot, products=prod)
    h = 1e-5

    def central():  # both moments, every mu_jl and sigma_jl: 4 D quad calls
        for x, other, first in ((mu, sigma, True), (sigma, mu, False)):
            for l in range(D):
                e = np.zeros_like(x)
                e[:, l] = h
                for sgn in (1, -1):
                    a = x + sgn * e
                    gp.quad(a, other, compute_var=True) if first else gp.quad(other, a, compute_var=True)

    out["central_differences_ms"] = _time(central, max(1, reps // 2))
    row = dict(case=tag, N=X.shape[0], D=D, S=len(gp.posteriors), M=M, **out,
               quad_calls_of_central_differences=4 * D,
               grad_var_over_quad_var=out["quad_grad_var_ms"] / out["quad_var_ms"],
               grad_over_quad_var=out["quad_grad_ms"] / out["quad_var_ms"],
               central_over_grad_var=out["central_differences_ms"] / out["quad_grad_var_ms"])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="50,1000")
    a = ap.parse_args()
    from gpyreg_amd import _lib

    X, y, hyp = bench.synthetic_problem(3, 16)
    gp = _se_gp(X, y, hyp)
    _lib.context(gp.device).set_option("small_timing", 1)
    rows = [_row(gp, X, int(m), a.reps, "cfg3_se") for m in a.sizes.split(",")]
    X, y, hyp = _pyvbmc_problem()
    rows.append(_row(_se_gp(X, y, hyp), X, 50, a.reps, "pyvbmc"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=_lib.context(gp.device).device_info(), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
