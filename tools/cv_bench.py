"""cv_predict against what a user does without it -- a refit per fold -- on the cfg3 problem (N = 4096, D = 10,
Matern-5, S = 16, fp64; bench.synthetic_problem(3, 16)) (GPU box).

    python tools/cv_bench.py [--out profiles/cv_cfg3.json] [--reps 5]

Cases: leave-one-out, 10 scattered folds (a seeded permutation), 10 contiguous folds, 5 folds, 2 folds; the fold cases
with both engines of the Gram (cv.h: 1 = fused gather + MFMA, 2 = gathered panels + library GEMM).  Per case the wall
time of GP.cv_predict (median of --reps after one warm-up call) and the device time of gpc_cv (gpc_last_timing: the
whole call and its Gram / diagonal pass).  The baseline is measured for ONE fold -- GP.update on the N - k other points,
predict_full at the fold, the joint density in NumPy -- and multiplied by the number of folds: EXTRAPOLATED, and
labelled so (leave-one-out: 4096 times one refit on N - 1 points).  Also: the leave-one-out pass's bytes over time
against the 8 TB/s HBM peak, and the Gram's flops over time against the measured fp64 MFMA ceiling (gpc_mfma_peak)."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import bench  # noqa: E402

HBM_PEAK = 8e12


def _time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def _refit_one_fold(X, y, hyp, I):
    """One fold the long way: a fresh GP on the other points, predict_full at the fold, the joint density."""
    from scipy.linalg import cholesky, solve_triangular

    keep = np.setdiff1d(np.arange(X.shape[0]), I)
    gp = bench.make_gp(3, "f64")
    gp.update(X_new=X[keep], y_new=y[keep], hyp=hyp)
    mu, cov = gp.predict_full(X[I], add_noise=True)
    lpd = np.zeros(hyp.shape[0])
    for s in range(hyp.shape[0]):
        R = cholesky(cov[:, :, s], lower=True)
        u = solve_triangular(R, y[I, 0] - mu[:, s], lower=True)
        lpd[s] = -0.5 * u @ u - np.sum(np.log(np.diag(R))) - 0.5 * I.size * np.log(2 * np.pi)
    return lpd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    from gpyreg_amd import _lib

    X, y, hyp = bench.synthetic_problem(3, 16)
    N, S = X.shape[0], hyp.shape[0]
    npad = -(-N // 128) * 128
    gp = bench.make_gp(3, "f64")
    gp.update(X_new=X, y_new=y, hyp=hyp)
    ctx = _lib.context(gp.device)
    peak = ctx.mfma_peak(_lib.F64)[0]
    perm = np.random.default_rng(7).permutation(N)
    cases = [("loo", None), ("10_scattered", [np.sort(p) for p in np.array_split(perm, 10)]),
             ("10_contiguous", list(np.array_split(np.arange(N), 10))),
             ("5_contiguous", list(np.array_split(np.arange(N), 5))), ("2_contiguous", list(np.array_split(np.arange(N), 2)))]
    rows = []
    for name, folds in cases:
        F = N if folds is None else len(folds)
        base = None
        if not a.no_baseline:
            I = np.array([N // 2]) if folds is None else folds[0]
            one = _time(lambda: _refit_one_fold(X, y, hyp, I), 1)
            base = dict(one_fold_ms=one, folds=F, extrapolated_ms=one * F, extrapolated=True)
        for engine in ((0,) if folds is None else (1, 2)):
            ctx.set_option("cv_engine", engine)
            wall = _time(lambda: gp.cv_predict(folds, add_noise=True, separate_samples=True, return_lpd=True), a.reps)
            tot, gram = ctx.last_timing()
            row = dict(case=name, N=N, S=S, F=F, engine_ran=ctx.get_option("cv_engine_ran"), wall_ms=wall, device_ms=tot,
                       gram_ms=gram, per_stage_ms=dict(gram_or_diag=gram, factor_and_epilogue=tot - gram), baseline=base)
            if base:
                row["speedup_wall_vs_extrapolated_refits"] = base["extrapolated_ms"] / wall
            if folds is None:  # the lower triangle of W of every sample, once
                nbytes = S * npad * (npad + 64) // 2 * 8
                row["loo_gb_per_s"] = nbytes / (gram * 1e-3) / 1e9 if gram > 0 else None
                row["loo_fraction_of_hbm_peak"] = nbytes / (gram * 1e-3) / HBM_PEAK if gram > 0 else None
            else:  # 2 N k^2 / 2 flops per fold over the lower triangle, the rows above the first index skipped: an upper bound N k^2
                flops = S * sum(float(N) * f.size * f.size for f in folds)
                row["gram_tflops"] = flops / (gram * 1e-3) / 1e12 if gram > 0 else None
                row["gram_fraction_of_mfma_peak"] = row["gram_tflops"] / peak if gram > 0 else None
            print(json.dumps(row), flush=True)
            rows.append(row)
    ctx.set_option("cv_engine", 0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=ctx.device_info(), mfma_peak_tflops_f64=peak, hbm_peak_bytes_per_s=HBM_PEAK, rows=rows), f,
                      indent=1)


if __name__ == "__main__":
    main()
