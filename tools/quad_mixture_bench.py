"""quad_mixture against quad_grad(compute_var=True) and against the host route (w^T quad_cov w plus NumPy) on an SE
posterior of the cfg3 problem (N = 4096, D = 10, S = 16; bench.synthetic_problem(3, 16), whose hyperparameters have the
SE ARD layout) at M = 50 and M = 1000 measures (GPU box).

    python tools/quad_mixture_bench.py [--out profiles/quad_mixture_cfg3.json] [--reps 7]

Wall time per call (median of --reps after one warm-up call) and the device time of the call (gpc_last_timing: the whole
call and its second figure -- for quad_mixture the solve, the triangular matrix-vector products, whose achieved bandwidth
over the bytes of W they read is reported; for the others their N^2 M products).  "quad_mix_gemms" must stay 0."""

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


def _row(gp, X, M, reps):
    from gpyreg_amd import _lib

    ctx = _lib.context(gp.device)
    N, D = X.shape
    S = len(gp.posteriors)
    rng = np.random.default_rng(1)
    mu = X[rng.choice(N, M, replace=False)] + 0.1 * rng.standard_normal((M, D))
    sigma = rng.uniform(0.2, 1.0, (M, D))
    w = rng.dirichlet(np.ones(M))

    def host_route():  # the variance only: no gradients come out of this route
        F, C = gp.quad_cov(mu, sigma, separate_samples=True)
        return w @ F, np.einsum("j,jks,k->s", w, C, w)

    out = {}
    for key, fn in (("quad_mixture", lambda: gp.quad_mixture(mu, sigma, w, compute_var=True, compute_grad=True)),
                    ("quad_mixture_var_only", lambda: gp.quad_mixture(mu, sigma, w, compute_var=True)),
                    ("quad_grad_var", lambda: gp.quad_grad(mu, sigma, compute_var=True)),
                    ("host_route", host_route)):
        out[key + "_ms"] = _time(fn, reps)
        tot, second = ctx.last_timing()
        out["device_" + key + "_ms"] = dict(total=tot, second=second)
    # the solve reads the lower triangle of W twice (v = W zbar, q = W^T v): S N_pad^2 elements in all
    npad = -(-N // 128) * 128
    solve_ms = out["device_quad_mixture_ms"]["second"]
    bytes_w = S * npad * (npad + 128) * 8
    row = dict(case="cfg3_se", N=N, D=D, S=S, M=M, **out, quad_mix_gemms=ctx.get_option("quad_mix_gemms"),
               solve_gb_per_s=bytes_w / (solve_ms * 1e-3) / 1e9 if solve_ms > 0 else None,
               mixture_over_quad_grad_var=out["quad_mixture_ms"] / out["quad_grad_var_ms"],
               device_mixture_over_quad_grad_var=out["device_quad_mixture_ms"]["total"] /
               out["device_quad_grad_var_ms"]["total"],
               host_route_over_mixture_var_only=out["host_route_ms"] / out["quad_mixture_var_only_ms"])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="50,1000")
    a = ap.parse_args()
    import gpyreg_amd as gpr
    from gpyreg_amd import _lib

    X, y, hyp = bench.synthetic_problem(3, 16)
    gp = gpr.GP(X.shape[1], gpr.covariance_functions.SquaredExponential(), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, hyp=hyp)
    _lib.context(gp.device).set_option("small_timing", 1)
    rows = [_row(gp, X, int(m), a.reps) for m in a.sizes.split(",")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=_lib.context(gp.device).device_info(), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
