"""GradientConditionedPosterior.gradient_posterior against the route a user had before it: central differences of
GradientConditionedPosterior.predict on the (2 D + 1)-point stencil (GPU box).

    python tools/grad_obs_gradpost_bench.py [--out profiles/grad_obs_gradpost.json] [--reps 5] [--cases small,vbmc,cfg3]

The three shapes of tools/grad_obs_bench.py (n = 300 / 3500 / 4000) at M = 100 and 1000 queries, cov = "full" and
"diag".  Per row: wall time of the call (median of --reps after one warm-up), the device time of the library call
(gpc_last_timing with "small_timing" on), the device time of the operand builds of that call ("gobs_grad_operand_us":
scaling, gobs_grad_operand_tile_kernel, reduction) and their share, the operand kernel's bytes per second over the
n (D + 1) M values it writes, and wall and device time of the central differences -- which give the mean's gradient and
the variance's gradient 2 C[0, 1:] only, no covariance of the gradient at all -- with their disagreement."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from grad_obs_bench import CASES  # noqa: E402  (name: (N, Ng, D, S))


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def run_case(name, reps, queries):
    import gpyreg_amd as gpr
    from gpyreg_amd import _lib

    N, Ng, D, S = CASES[name]
    n = N + Ng * D
    rng = np.random.default_rng(0)
    X, Xg = rng.uniform(-3, 3, (N, D)), rng.uniform(-3, 3, (Ng, D))
    y = np.sin(X.sum(1, keepdims=True) / np.sqrt(D)) + 0.1 * rng.standard_normal((N, 1))
    dy = np.cos(Xg.sum(1, keepdims=True) / np.sqrt(D)) / np.sqrt(D) * np.ones((1, D)) + 0.1 * rng.standard_normal((Ng, D))
    hyp = np.concatenate([np.log(1.5 * np.sqrt(D)) * np.ones(D), [0.0, np.log(0.1), 0.0]])
    hyp = hyp + 0.05 * rng.standard_normal((S, hyp.size))
    ell = np.exp(hyp[:, :D]).mean(0)
    gp = gpr.GP(D, gpr.covariance_functions.Matern(5), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, hyp=hyp)
    ctx = _lib.context(gp.device)
    ctx.set_option("small_timing", 1)
    rows = []
    with gp.condition_on_gradients(Xg, dy, 0.01) as cp:
        for M in queries:
            xs = rng.uniform(-3, 3, (M, D))
            h = 1e-3 * ell
            stencil = np.concatenate([xs] + [xs + s * h[l] * np.eye(D)[l] for l in range(D) for s in (1, -1)])

            def differences():
                mu, s2 = cp.predict(stencil, separate_samples=True)
                mu, s2 = mu.reshape(2 * D + 1, M, S), s2.reshape(2 * D + 1, M, S)
                dmu = np.stack([(mu[1 + 2 * l] - mu[2 + 2 * l]) / (2 * h[l]) for l in range(D)], axis=1)
                ds2 = np.stack([(s2[1 + 2 * l] - s2[2 + 2 * l]) / (2 * h[l]) for l in range(D)], axis=1)
                return dmu, ds2

            fd_wall = _median_ms(differences, reps)
            differences()
            fd_dev = ctx.last_timing()[0]
            dmu_fd, ds2_fd = differences()
            for form in ("full", "diag"):
                call = lambda: cp.gradient_posterior(xs, cov=form, with_value=True, separate_samples=True)
                wall = _median_ms(call, reps)
                dev, op = [], []
                for _ in range(reps):
                    mean, C = call()
                    dev.append(ctx.last_timing()[0])
                    op.append(ctx.get_option("gobs_grad_operand_us") / 1e3)
                dev_ms, op_ms = float(np.median(dev)), float(np.median(op))
                row = dict(case=name, N=N, Ng=Ng, D=D, S=S, n=n, M=M, cov=form, kernel="matern5", reps=reps,
                           wall_ms=wall, device_ms=dev_ms, operand_ms=op_ms, operand_share_of_device=op_ms / max(dev_ms, 1e-9),
                           operand_GB_per_s=8.0 * S * n * (D + 1) * M / max(op_ms, 1e-6) / 1e6,
                           central_differences_wall_ms=fd_wall, central_differences_device_ms=fd_dev,
                           speedup_over_central_differences=fd_wall / wall,
                           dmu_disagreement=float(np.abs(mean[:, 1:] - dmu_fd).max() / np.abs(mean[:, 1:]).max()))
                if form == "full":
                    row["ds2_disagreement"] = float(np.abs(2 * C[:, 0, 1:] - ds2_fd).max() / np.abs(2 * C[:, 0, 1:]).max())
                print(json.dumps(row), flush=True)
                rows.append(row)
    ctx.set_option("small_timing", 0)
    return rows, ctx.device_info()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", default="100,1000")
    ap.add_argument("--cases", default="small,vbmc,cfg3")
    a = ap.parse_args()
    rows, info = [], ""
    for name in a.cases.split(","):
        more, info = run_case(name, a.reps, [int(q) for q in a.queries.split(",")])
        rows += more
        if a.out:  # (after every case: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(dict(device=info, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
