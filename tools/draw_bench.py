"""GP.draw_functions on the cfg3 posterior (N = 4096, D = 10, Matern 5, S = 16), R = 64 draws per sample, at M = 1000
and M = 4096 query points, against the host path it replaces: predict_full (the S covariances downloaded), then per
sample a SciPy Cholesky and the product L Z (GPU box).

    python tools/draw_bench.py [--out profiles/draw_cfg3.json] [--reps 5] [--sizes 1000,4096] [--draws 64]

Wall time per call (median of --reps after one warm-up call), the device time of the draw call (gpc_last_timing:
whole call), and the factorization's S M^3 / 3 flops as a fraction of the fp64 MFMA peak over that device time."""

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


def main():
    import scipy.linalg as sla

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,4096")
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    from gpyreg_amd import _lib

    X, y, hyp = bench.synthetic_problem(3, 16)
    gp = bench.make_gp(3, "f64")
    gp.update(X_new=X, y_new=y, hyp=hyp)
    D, S, R = X.shape[1], hyp.shape[0], a.draws
    rows = []
    for M in (int(m) for m in a.sizes.split(",")):
        xs = np.random.default_rng(1).uniform(-3, 3, (M, D))
        t_draw = _time(lambda: gp.draw_functions(xs, n_draws=R, seed=1), a.reps)
        dev = _lib.context(gp.device).last_timing()
        z = np.random.default_rng(2).standard_normal((M, R))

        def host():
            mu, cov = gp.predict_full(xs)
            for s in range(S):
                L = sla.cholesky(cov[:, :, s], lower=True, check_finite=False)
                _ = mu[:, s:s + 1] + L @ z

        t_full = _time(lambda: gp.predict_full(xs), a.host_reps)
        t_host = _time(host, a.host_reps)
        flops = S * M**3 / 3.0
        row = dict(config=3, N=X.shape[0], D=D, S=S, M=M, R=R, draw_functions_ms=t_draw,
                   device_draw_ms=dev[0], host_path_ms=t_host, host_predict_full_ms=t_full,
                   host_over_device=t_host / t_draw, factor_flops=flops,
                   factor_frac_of_fp64_peak_over_device_time=flops / (dev[0] * 1e-3) / 1e12 / bench.FP64_MFMA_PEAK_TFLOPS
                   if dev[0] > 0 else None)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=_lib.context(gp.device).device_info(), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
