"""GP.nll_batch_grad_obs(compute_grad=True) against the two routes a user had before it (GPU box):

  * planes: the joint matrix and its cov_N derivative planes formed in NumPy (gpyreg_amd._gradobs) and pushed through
    nll_batch_K with a dK callback -- measured for --plane-samples hyperparameter rows (the planes of one row of the
    largest shape are 1.4 GB) and reported per row;
  * central differences: 2 hyp_N value-only rows per hyperparameter row, as ONE nll_batch_grad_obs batch.

    python tools/grad_obs_grad_bench.py [--out profiles/grad_obs_grad.json] [--reps 5] [--cases small,vbmc,cfg3]

The shapes are those of tools/grad_obs_bench.py (n = 300, 3500, 4000).  Per case: wall time of the value + gradient call
(median of --reps after one warm-up; it contains a value-only evaluation, which supplies nlZ), of the value-only call,
of the library's gradient call alone (gpc_nll_batch_gobs_grad), the device time of the contraction on its own (one
hyperparameter row through gpc_debug_gobs_trace: "gobs_trace_us") and its bytes per second over the weight bytes it
reads (the lower triangle, 4 n (n + 1))."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from grad_obs_bench import CASES, _median_ms  # noqa: E402


def run_case(name, reps, plane_samples):
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
    s2g = 0.01
    gp = gpr.GP(D, gpr.covariance_functions.Matern(5), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, hyp=hyp[:1], compute_posterior=False)
    ctx = _lib.context(gp.device)
    kid, degree, cov_N, P = 1, 5, D + 1, hyp.shape[1]

    # the joint rows, as the library calls and the planes route need them
    m = np.concatenate([np.repeat(hyp[:, -1:], N, 1), np.zeros((S, Ng * D))], axis=1)
    sn2 = np.concatenate([np.repeat(np.exp(2 * hyp[:, cov_N:cov_N + 1]), N, 1), np.full((S, Ng * D), s2g)], axis=1)
    dm = np.zeros((S, n, 1))
    dm[:, :N] = 1.0
    dsn2 = np.zeros((S, n, 1))
    dsn2[:, :N, 0] = 2 * sn2[:, :N]
    target = go.to_joint(y, dy)

    value_grad = lambda: gp.nll_batch_grad_obs(hyp, Xg, dy, s2g, compute_grad=True)
    value = lambda: gp.nll_batch_grad_obs(hyp, Xg, dy, s2g)

    def central():
        rows = np.repeat(hyp, 2 * P, 0).reshape(S, 2 * P, P)
        rows[:, np.arange(P), np.arange(P)] += 1e-5
        rows[:, P + np.arange(P), np.arange(P)] -= 1e-5
        z = gp.nll_batch_grad_obs(rows.reshape(-1, P), Xg, dy, s2g).reshape(S, 2 * P)
        return (z[:, :P] - z[:, P:]) / 2e-5

    ps = min(plane_samples, S)
    t_form = [0.0]

    def planes():
        t0 = time.perf_counter()
        K = np.stack([go.joint_cov(kid, degree, h[:cov_N], X, Xg) for h in hyp[:ps]])
        dK = [go.joint_cov_dhyp(kid, degree, h[:cov_N], X, Xg) for h in hyp[:ps]]
        t_form[0] = time.perf_counter() - t0
        ctx.set_data(np.zeros((n, D)), target)
        return ctx.nll_batch_K(_lib.F64, K, lambda s, p: dK[s][p], cov_N, m[:ps], sn2[:ps], True, True, dm[:ps],
                               dsn2[:ps])[1]

    def lib_grad():
        return ctx.nll_batch_gobs_grad(kid, degree, _lib.F64, hyp[:, :cov_N], m, sn2, dm, dsn2)[1]

    nlz, g = value_grad()
    g_fd, g_pl = central(), planes()
    scale = np.abs(g).max(1, keepdims=True)
    row = dict(case=name, N=N, Ng=Ng, D=D, S=S, n=n, hyp_N=P, kernel="matern5", reps=reps,
               agrees_with_planes_route_to=float((np.abs(g[:ps] - g_pl) / scale[:ps]).max()),
               agrees_with_central_differences_to=float((np.abs(g - g_fd) / scale).max()))
    row["value_and_gradient_wall_ms"] = _median_ms(value_grad, reps)
    row["value_only_wall_ms"] = _median_ms(value, reps)
    row["central_differences_wall_ms"] = _median_ms(central, max(1, reps // 2))
    t_planes = _median_ms(planes, 1)
    row["planes_route_rows"] = ps
    row["planes_route_wall_ms_per_row"] = t_planes / ps
    row["planes_route_numpy_formation_ms_per_row"] = t_form[0] * 1e3 / ps
    row["planes_route_wall_ms_scaled_to_S"] = t_planes / ps * S
    ctx.set_data_gobs(X, y, Xg, dy)
    row["library_gradient_call_wall_ms"] = _median_ms(lib_grad, reps)
    row["speedup_over_planes_route"] = row["planes_route_wall_ms_scaled_to_S"] / row["value_and_gradient_wall_ms"]
    row["speedup_over_central_differences"] = row["central_differences_wall_ms"] / row["value_and_gradient_wall_ms"]
    row["cost_over_value_only"] = row["value_and_gradient_wall_ms"] / row["value_only_wall_ms"]
    # the contraction on its own: one hyperparameter row, a well-scaled symmetric matrix in place of the inverse
    A = rng.standard_normal((n, n)) / np.sqrt(n)
    A = A + A.T
    al = rng.standard_normal(n) / np.sqrt(n)
    us = []
    for _ in range(reps + 1):
        ctx.debug_gobs_trace(kid, degree, hyp[0, :cov_N], X, Xg, A, al, 1.0)
        us.append(ctx.get_option("gobs_trace_us"))
    t = float(np.median(us[1:]))
    # (ONE sample's launches on an otherwise idle device: in the library call the tiles of all S samples share one launch
    # and run side by side, so S times this figure is no share of the call -- profiles/grad_obs_grad_kernels.txt has the
    # kernels' share from a kernel trace of the batched call)
    row["gobs_trace_us_one_sample_alone"] = t
    row["gobs_trace_GB_per_s_over_weight_bytes_one_sample_alone"] = 4.0 * n * (n + 1) / max(t, 1.0) / 1e3
    return row, ctx.device_info()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plane-samples", type=int, default=1)
    ap.add_argument("--cases", default="small,vbmc,cfg3")
    a = ap.parse_args()
    rows, info = [], ""
    for name in a.cases.split(","):
        row, info = run_case(name, a.reps, a.plane_samples)
        print(json.dumps(row), flush=True)
        rows.append(row)
        if a.out:  # (after every case: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(dict(device=info, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
