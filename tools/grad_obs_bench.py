"""GP.condition_on_gradients + predict(M = 1000) against the route a user had before it: the joint covariance and the
cross operand formed in NumPy (gpyreg_amd._gradobs) and pushed through posterior_batch_K / predict_K (GPU box).

    python tools/grad_obs_bench.py [--out profiles/grad_obs.json] [--reps 10] [--cases vbmc,cfg3,small]

Per case: wall time of the call pair (median of --reps after one warm-up), the device time of its three library calls
(gpc_last_timing with "small_timing" on), the device time of the two new kernels on their own (one hyperparameter row
through the debug hooks: "gobs_cov_us", "gobs_cross_us"), their bytes per second over the n^2 (n M) values they write,
and the share of the call pair they account for (the joint matrix is built twice per sample: for the posterior and for
nlZ)."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

CASES = {  # name: (N, Ng, D, S)
    "vbmc": (500, 500, 6, 8),
    "cfg3": (2000, 200, 10, 16),
    "small": (100, 100, 2, 8),
}


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def run_case(name, reps, M):
    import gpyreg_amd as gpr
    from gpyreg_amd import _gradobs as go
    from gpyreg_amd import _lib

    N, Ng, D, S = CASES[name]
    n = N + Ng * D
    rng = np.random.default_rng(0)
    X, Xg = rng.uniform(-3, 3, (N, D)), rng.uniform(-3, 3, (Ng, D))
    y = np.sin(X.sum(1, keepdims=True) / np.sqrt(D)) + 0.1 * rng.standard_normal((N, 1))
    dy = np.cos(Xg.sum(1, keepdims=True) / np.sqrt(D)) / np.sqrt(D) * np.ones((1, D)) + 0.1 * rng.standard_normal((Ng, D))
    hyp = np.concatenate([np.log(1.5 * np.sqrt(D)) * np.ones(D), [0.0, np.log(0.1), 0.0]])
    hyp = hyp + 0.05 * rng.standard_normal((S, hyp.size))
    xs = rng.uniform(-3, 3, (M, D))
    s2g = 0.01
    gp = gpr.GP(D, gpr.covariance_functions.Matern(5), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, hyp=hyp)
    ctx = _lib.context(gp.device)
    ctx.set_option("small_timing", 1)
    kid, degree, cov_N = 1, 5, D + 1

    def device_pair():
        with gp.condition_on_gradients(Xg, dy, s2g) as cp:
            return cp.predict(xs, separate_samples=True)

    def device_condition():
        gp.condition_on_gradients(Xg, dy, s2g).close()

    # the joint rows, as both routes need them
    m = np.concatenate([np.repeat(hyp[:, -1:], N, 1), np.zeros((S, Ng * D))], axis=1)
    sn2 = np.concatenate([np.repeat(np.exp(2 * hyp[:, cov_N:cov_N + 1]), N, 1), np.full((S, Ng * D), s2g)], axis=1)
    target = go.to_joint(y, dy)

    def numpy_pair():
        K = np.stack([go.joint_cov(kid, degree, h[:cov_N], X, Xg) for h in hyp])
        ctx.set_data(np.zeros((n, D)), target)
        handle, mult, lchol, info = ctx.posterior_batch_K(_lib.F64, K, m, sn2, True)
        Ks = np.stack([go.joint_cross(kid, degree, h[:cov_N], X, Xg, xs) for h in hyp])
        fmu, fq, _ = handle.predict_K(Ks)
        handle.free()
        return fmu + hyp[:, -1][None, :], np.exp(2 * hyp[:, D])[None, :] + fq

    mu_d, s2_d = device_pair()
    mu_n, s2_n = numpy_pair()
    agree = float(max(np.abs(mu_d - mu_n).max() / np.abs(mu_n).max(), np.abs(s2_d - np.maximum(s2_n, 0)).max() / s2_n.max()))
    row = dict(case=name, N=N, Ng=Ng, D=D, S=S, n=n, M=M, kernel="matern5", reps=reps, routes_agree_to=agree)
    row["device_pair_wall_ms"] = _median_ms(device_pair, reps)
    row["device_condition_wall_ms"] = _median_ms(device_condition, reps)
    row["numpy_K_mode_pair_wall_ms"] = _median_ms(numpy_pair, reps)
    row["speedup"] = row["numpy_K_mode_pair_wall_ms"] / row["device_pair_wall_ms"]
    # device time of the three library calls of the device route
    ctx.set_data_gobs(X, y, Xg, dy)
    dev = {}
    for key, call in (("posterior", lambda: ctx.posterior_batch_gobs(kid, degree, _lib.F64, hyp[:, :cov_N], m, sn2)[0]),
                      ("nll", lambda: ctx.nll_batch_gobs(kid, degree, _lib.F64, hyp[:, :cov_N], m, sn2))):
        ts = []
        for _ in range(reps + 1):
            r = call()
            ts.append(ctx.last_timing()[0])
            if key == "posterior":
                r.free()
        dev[key] = float(np.median(ts[1:]))
    handle = ctx.posterior_batch_gobs(kid, degree, _lib.F64, hyp[:, :cov_N], m, sn2)[0]
    ts = []
    for _ in range(reps + 1):
        handle.predict_gobs(xs)
        ts.append(ctx.last_timing()[0])
    handle.free()
    dev["predict"] = float(np.median(ts[1:]))
    row["device_call_ms"] = dev
    # the two new kernels on their own: one hyperparameter row
    cov_us, cross_us = [], []
    for _ in range(reps + 1):
        ctx.debug_gobs_cov(kid, degree, hyp[0, :cov_N], X, Xg)
        cov_us.append(ctx.get_option("gobs_cov_us"))
        ctx.debug_gobs_cross(kid, degree, hyp[0, :cov_N], X, Xg, xs, np.ones(n))
        cross_us.append(ctx.get_option("gobs_cross_us"))
    t_cov, t_cross = float(np.median(cov_us[1:])), float(np.median(cross_us[1:]))
    row["gobs_cov_kernel_us_per_sample"] = t_cov
    row["gobs_cross_build_us_per_sample"] = t_cross
    row["gobs_cov_GB_per_s"] = 8.0 * n * n / max(t_cov, 1.0) / 1e3
    row["gobs_cross_GB_per_s"] = 8.0 * n * M / max(t_cross, 1.0) / 1e3
    row["new_kernels_share_of_device_pair"] = (2 * S * t_cov + S * t_cross) / 1e3 / row["device_pair_wall_ms"]
    ctx.set_option("small_timing", 0)
    return row, ctx.device_info()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--cases", default="small,vbmc,cfg3")
    a = ap.parse_args()
    rows, info = [], ""
    for name in a.cases.split(","):
        row, info = run_case(name, a.reps, a.queries)
        print(json.dumps(row), flush=True)
        rows.append(row)
        if a.out:  # (after every case: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(dict(device=info, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
