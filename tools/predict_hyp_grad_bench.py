"""GP.predict_hyp_grad against what a caller has without it, on the cfg3 problem (N = 4096, D = 10, Matern-5;
bench.synthetic_problem(3, S)) at S = 16 and S = 1 (the MAP use) for M in {100, 1000} queries (GPU box).

    python tools/predict_hyp_grad_bench.py [--out profiles/predict_hyp_grad_cfg3.json] [--reps 3] [--ms 100,1000]
                                           [--ss 16,1]

Routes, alternating inside one process (a warm-up round first; every call ends in a synchronise):
  (a) hyp_grad       predict_hyp_grad(xs)
  (b) hyp_grad_mean  predict_hyp_grad(xs, compute_var=False)
  (c) fd             central differences, h = 1e-4: per sample update(hyp=theta +- h e_p) for all 2 P shifted vectors in
                     one batch, then predict(xs, separate_samples=True) -- 2 P factorizations per sample, the only way
                     to these numbers without the method; the resident posteriors are restored afterwards (not timed)
Recorded: wall time per route (median, min, max), the device time of (a) and (b) (gpc_last_timing: ms_total, ms_factor =
the products with W and the planes), the flop count of the quadratic forms 2 N_pad^2 M_pad per plane and sample and
the rate it implies over ms_factor, the speed-ups over (c) and the largest relative difference between (a) and (c)
per column."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import bench  # noqa: E402


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v))


def _queries(X, M):
    rng = np.random.default_rng(M)
    return X[rng.integers(0, X.shape[0], M)] + 0.3 * X.std(0, keepdims=True) * rng.standard_normal((M, X.shape[1]))


def _time(ctx, fn, reps, after=None):
    wall, dev, prod = [], [], []
    out = None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        tot, fac = ctx.last_timing()
        if after:
            after()
        if rep:
            wall.append(1e3 * (t1 - t0))
            dev.append(tot)
            prod.append(fac)
    return out, dict(wall_ms=_stats(wall), device_ms=_stats(dev), products_ms=_stats(prod))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/predict_hyp_grad_cfg3.json")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ms", default="100,1000")
    ap.add_argument("--ss", default="16,1")
    args = ap.parse_args()
    from gpyreg_amd import _lib

    ctx = _lib.context(0)
    rows = []
    N = D = None
    for S in [int(s) for s in args.ss.split(",")]:
        X, y, hyp = bench.synthetic_problem(3, S)
        gp = bench.make_gp(3, "f64")
        gp.shard = False
        gp.update(X_new=X, y_new=y, hyp=hyp)
        N, D = X.shape
        P = hyp.shape[1]
        npad = -(-N // 128) * 128
        planes = D  # Matern ARD: one plane per lengthscale
        for M in [int(m) for m in args.ms.split(",")]:
            xs = _queries(X, M)
            mpad = -(-M // 128) * 128
            h = 1e-4

            def fd():
                dmu, ds2 = np.empty((M, P, S)), np.empty((M, P, S))
                for s in range(S):
                    gp.update(hyp=np.concatenate([hyp[s][None] + h * np.eye(P), hyp[s][None] - h * np.eye(P)]))
                    mu, s2 = gp.predict(xs, separate_samples=True)
                    dmu[:, :, s], ds2[:, :, s] = (mu[:, :P] - mu[:, P:]) / (2 * h), (s2[:, :P] - s2[:, P:]) / (2 * h)
                return dmu, ds2

            res, t = {}, {}
            res["hyp_grad"], t["hyp_grad"] = _time(ctx, lambda: gp.predict_hyp_grad(xs), args.reps)
            _, t["hyp_grad_mean"] = _time(ctx, lambda: gp.predict_hyp_grad(xs, compute_var=False), args.reps)
            res["fd"], t["fd"] = _time(ctx, fd, max(1, args.reps - 1), after=lambda: gp.update(hyp=hyp))
            del t["fd"]["device_ms"], t["fd"]["products_ms"]
            worst = {}
            for name, an, f in (("dmu", res["hyp_grad"][2], res["fd"][0]), ("ds2", res["hyp_grad"][3], res["fd"][1])):
                scale = np.abs(an).max(0)
                worst[name] = float((np.abs(an - f).max(0) / np.where(scale > 0, scale, 1.0)).max())
            flops = 2.0 * npad * npad * mpad * planes * S
            fac = t["hyp_grad"]["products_ms"]["median"]
            row = dict(S=S, M=M, M_pad=mpad, P=P, planes=planes, routes=t, fd_factorizations=2 * P * S,
                       quadratic_form_flops=flops, quadratic_form_tflops_over_ms_factor=(flops / (1e-3 * fac) / 1e12
                                                                                         if fac > 0 else None),
                       fd_vs_hyp_grad_max_rel=worst)
            for route in ("hyp_grad", "hyp_grad_mean"):
                row["speedup_%s_vs_fd" % route] = t["fd"]["wall_ms"]["median"] / t[route]["wall_ms"]["median"]
            rows.append(row)
            print(json.dumps(row))
    rec = dict(problem=dict(cfg=3, N=N, D=D, kernel="matern5", dtype="f64"), device=ctx.device_info(), reps=args.reps,
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
