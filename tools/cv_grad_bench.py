"""GP.cv_nll_batch -- the leave-one-out objective with its gradient -- against the marginal likelihood's gradient on the
same rows and against what a caller has without it, central differences of the value, on two problems (GPU box):

    cfg3   N = 4096, D = 10, Matern 5, S = 16   (bench.synthetic_problem(3, 16))
    vbmc   N = 500,  D = 6,  Matern 5, S = 8    (a VBMC-sized surrogate, tools/nll_hess_bench.py's)

    python tools/cv_grad_bench.py [--out profiles/cv_grad_cfg3.json] [--reps 5] [--only cfg3|vbmc]

One process, a warm-up round first, medians of --reps rounds; every call ends in a synchronise.  Recorded per problem:
  1. cv_nll_batch with the gradient: wall time, and through the handle the device sections (gpc_last_timing: ms_total,
     ms_factor = Q, the weights, the scaling and the product) and the contraction pass ("cv_grad_trace_us");
  2. nll_batch(compute_grad=True) on the same rows: wall and device time (this code does not know the objective);
  3. central differences of the value: per sample one batch of 2 P rows of cv_nll_batch(compute_grad=False), i.e.
     posterior_batch and the leave-one-out pass of cv_predict, 2 P factorizations per gradient -- wall time, the ratio,
     and the largest deviation between the two gradients;
and, for the claim that the device time does not depend on the number of hyperparameters, the device sections of the
same data under the isotropic Matern 5 kernel (2 covariance hyperparameters instead of D + 1)."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from nll_hess_bench import _cfg3, _stats, _vbmc  # noqa: E402


def _device_sections(ctx, gp, hyp, reps):
    """(ms_total, ms_factor, contraction ms) of gpc_cv_grad alone on posteriors built for hyp, medians' raw lists."""
    from gpyreg_amd import _lib

    cov_N = gp._counts()[0]
    pv = gp._plugin_values(hyp, True)
    kid, deg = gp._kid()
    handle, _, _, info = ctx.posterior_batch(kid, deg, _lib.F64, hyp[:, :cov_N], pv["m"], pv["sn2"], pv["vec"])
    assert not np.any(info)
    tot, fac, tr = [], [], []
    try:
        for rep in range(reps + 1):
            handle.cv_grad(cov_N, "lpd")
            t, f = ctx.last_timing()
            if rep:
                tot.append(t)
                fac.append(f)
                tr.append(1e-3 * ctx.get_option("cv_grad_trace_us"))
    finally:
        handle.free()
    return tot, fac, tr


def _run(name, make, reps):
    import gpyreg_amd as gpr
    from gpyreg_amd import _lib

    gp, X, y, hyp = make()
    gp.shard = False
    gp.X, gp.y = X, y
    S, P = hyp.shape
    N, D = X.shape
    ctx = _lib.context(0)
    ctx.set_option("small_timing", 1)
    npad = -(-N // 128) * 128
    cov_N, noise_N, mean_N = gp._counts()
    step = 1e-4

    def differences():
        out = np.empty((S, P))
        for s in range(S):
            rows = np.repeat(hyp[s:s + 1], 2 * P, 0)
            rows[np.arange(P), np.arange(P)] += step
            rows[P + np.arange(P), np.arange(P)] -= step
            v, _ = gp.cv_nll_batch(rows, compute_grad=False)
            out[s] = (v[:P] - v[P:]) / (2 * step)
        return out

    wall, nll_wall, nll_dev, fd_wall = [], [], [], []
    dL = fd = None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        _, dL = gp.cv_nll_batch(hyp)
        t1 = time.perf_counter()
        gp.nll_batch(hyp, compute_grad=True)
        t2 = time.perf_counter()
        nd, _ = ctx.last_timing()
        t3 = time.perf_counter()
        fd = differences()
        t4 = time.perf_counter()
        if rep:
            wall.append(1e3 * (t1 - t0))
            nll_wall.append(1e3 * (t2 - t1))
            nll_dev.append(nd)
            fd_wall.append(1e3 * (t4 - t3))
    dev, fac, trace = _device_sections(ctx, gp, hyp, reps)
    # the same data under the isotropic kernel: 2 covariance hyperparameters
    iso = gpr.GP(D, gpr.isotropic_covariance_functions.MaternIsotropic(5), gp.mean, gp.noise)
    iso.shard = False
    iso.X, iso.y = X, y
    hyp_iso = np.c_[hyp[:, :D].mean(1), hyp[:, D:]]
    ctx = iso._ctx()
    dev_i, fac_i, trace_i = _device_sections(ctx, iso, hyp_iso, reps)
    gp._ctx()
    rel = float((np.abs(dL - fd).max(1) / np.maximum(1.0, np.abs(dL).max(1))).max())
    row = dict(problem=dict(name=name, N=N, D=D, S=S, P=P, cov_N=cov_N, kernel="matern5", N_pad=npad),
               cv_nll_batch=dict(wall_ms=_stats(wall), device_ms=_stats(dev), q_weights_product_ms=_stats(fac),
                                 trace_ms=_stats(trace)),
               isotropic=dict(cov_N=2, device_ms=_stats(dev_i), q_weights_product_ms=_stats(fac_i),
                              trace_ms=_stats(trace_i)),
               nll_batch_grad=dict(wall_ms=_stats(nll_wall), device_ms=_stats(nll_dev)),
               product_flops=float(S) * npad**3,
               differences=dict(posteriors=2 * P * S, step=step, wall_ms=_stats(fd_wall)),
               speedup_vs_differences=float(np.median(fd_wall) / np.median(wall)),
               device_over_nll_grad=float(np.median(dev) / np.median(nll_dev)),
               grad_vs_differences_max_rel=rel)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/cv_grad_cfg3.json")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    from gpyreg_amd import _lib

    rows = [_run(name, make, args.reps) for name, make in (("vbmc", _vbmc), ("cfg3", _cfg3))
            if args.only in (None, name)]
    rec = dict(device=_lib.context(0).device_info(), reps=args.reps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
