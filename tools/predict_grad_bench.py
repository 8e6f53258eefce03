"""predict vs predict_grad on the cfg3 posterior (N = 4096, D = 10, Matern 5, S = 16), and predict_grad vs the
2 D + 1 predict calls of central differences, at M = 1000 and M = 8192 query points (GPU box).

    python tools/predict_grad_bench.py [--out profiles/predict_grad_cfg3.json] [--reps 5]

Wall time per call (median of --reps after one warm-up call) and the device time of the call
(gpc_last_timing: whole call, and its N^2 M product V = W K*)."""

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
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,8192")
    a = ap.parse_args()
    from gpyreg_amd import _lib

    X, y, hyp = bench.synthetic_problem(3, 16)
    gp = bench.make_gp(3, "f64")
    gp.update(X_new=X, y_new=y, hyp=hyp)
    D = X.shape[1]
    rows = []
    for M in (int(m) for m in a.sizes.split(",")):
        xs = np.random.default_rng(1).uniform(-3, 3, (M, D))
        t_pred = _time(lambda: gp.predict(xs), a.reps)
        dev_pred = _lib.context(gp.device).last_timing()
        t_grad = _time(lambda: gp.predict_grad(xs), a.reps)
        dev_grad = _lib.context(gp.device).last_timing()
        h = 1e-5 * (X.max(0) - X.min(0))

        def central():
            gp.predict(xs)
            for l in range(D):
                e = np.zeros(D)
                e[l] = h[l]
                gp.predict(xs + e)
                gp.predict(xs - e)

        t_fd = _time(central, max(1, a.reps // 2))
        row = dict(config=3, N=X.shape[0], D=D, S=hyp.shape[0], M=M, predict_ms=t_pred, predict_grad_ms=t_grad,
                   central_differences_ms=t_fd, predict_calls_of_central_differences=2 * D + 1,
                   grad_over_predict=t_grad / t_pred, central_over_grad=t_fd / t_grad,
                   device_predict_ms=dict(total=dev_pred[0], V_product=dev_pred[1]),
                   device_predict_grad_ms=dict(total=dev_grad[0], V_product=dev_grad[1]))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=_lib.context(gp.device).device_info(), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
