"""lookahead_variance and predict_cov against the composed route -- predict_full on the concatenation [x_ref; x_cand],
then the block, its square, the weights and the sum in NumPy -- on the cfg3 problem (N = 4096, D = 10, Matern-5,
S = 16; bench.synthetic_problem(3, 16)) at (M_ref, M_cand) = (1000, 1000), (4096, 1000), (4096, 4096), plus a seeded
PyVBMC-sized case (N = 400, D = 6, S = 8, 500 x 50) (GPU box).

    python tools/lookahead_bench.py [--out profiles/lookahead_cfg3.json] [--reps 5] [--sizes 1000x1000,4096x1000]

The routes alternate inside one process: every repeat times lookahead_variance, predict_cov and the composed route one
after the other.  Wall time per call (median, min and max of --reps after one warm-up round; every call ends in a
synchronise) and the device time of the call (gpc_last_timing: whole device section, and its products; recorded at
every size: the small-problem timing option is switched on).  --composed-reps bounds the repeats of the composed route,
whose download grows with (M_ref + M_cand)^2.  --dry-run builds the problems and prints the plan without a device."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import bench  # noqa: E402


def _gp(X, y, hyp):
    import gpyreg_amd as gpr

    gp = gpr.GP(X.shape[1], gpr.covariance_functions.Matern(5), gpr.mean_functions.ConstantMean(),
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


def _points(X, Mr, Mc):
    rng = np.random.default_rng(1)
    D = X.shape[1]
    pick = lambda m: X[rng.integers(0, X.shape[0], m)] + 0.1 * rng.standard_normal((m, D))  # noqa: E731
    return pick(Mr), pick(Mc)


def flops(N, Mr, Mc, S):
    """Shape-derived flops of the products per call: (direct route, its cross product alone, composed route)."""
    cross = 2.0 * N * Mr * Mc
    return S * (N * N * (Mr + Mc) + cross), S * cross, S * (N * N * (Mr + Mc) + 2.0 * N * (Mr + Mc) ** 2)


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v))


def _row(gp, X, Mr, Mc, reps, composed_reps, tag):
    from gpyreg_amd import _lib

    ctx = _lib.context(gp.device)
    xr, xc = _points(X, Mr, Mc)
    S = len(gp.posteriors)
    cov_N, noise_N, _ = gp._counts()
    sn2 = np.array([np.exp(2 * p.hyp[cov_N]) * p.sn2_mult for p in gp.posteriors])

    def composed():
        _, C = gp.predict_full(np.vstack([xr, xc]))
        fs2 = np.einsum("iis->is", C)[Mr:]
        return np.mean(np.sum(C[:Mr, Mr:, :] ** 2, 0) / Mr / (np.maximum(fs2, 0) + sn2[None, :]), 1)

    routes = (("lookahead", lambda: gp.lookahead_variance(xc, xr), reps),
              ("predict_cov", lambda: gp.predict_cov(xr, xc), reps),
              ("composed", composed, composed_reps))
    wall = {k: [] for k, _, _ in routes}
    dev = {k: [] for k, _, _ in routes}
    prod = {k: [] for k, _, _ in routes}
    fused0 = ctx.get_option("cov_fused")
    vals = {}
    for rep in range(-1, max(reps, composed_reps)):  # (-1: the warm-up round)
        for key, fn, n in routes:
            if rep >= n:
                continue
            t0 = time.perf_counter()
            vals[key] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= 0:
                tot, pr = ctx.last_timing()
                wall[key].append(dt)
                dev[key].append(tot)
                prod[key].append(pr)
    agree = float(np.abs(vals["lookahead"][:, 0] - vals["composed"]).max() / np.abs(vals["composed"]).max())
    f_direct, f_cross, f_composed = flops(X.shape[0], Mr, Mc, S)
    row = dict(case=tag, N=X.shape[0], D=X.shape[1], S=S, M_ref=Mr, M_cand=Mc,
               reduction_in_epilogue=ctx.get_option("cov_fused") > fused0,
               wall_ms={k: _stats(v) for k, v in wall.items()}, device_ms={k: _stats(v) for k, v in dev.items()},
               device_products_ms={k: _stats(v) for k, v in prod.items()},
               flops=dict(direct=f_direct, cross_product=f_cross, composed=f_composed),
               device_lookahead_over_composed=float(np.median(dev["lookahead"]) / np.median(dev["composed"])),
               wall_lookahead_over_composed=float(np.median(wall["lookahead"]) / np.median(wall["composed"])),
               # (the composed route's product window holds V = W Ks alone, not its V^T V: no figure for it)
               products_tflops={k: f_direct / (np.median(prod[k]) * 1e9) if np.median(prod[k]) > 0 else None
                                for k in ("lookahead", "predict_cov")},
               lookahead_against_composed_rel=agree)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composed-reps", type=int, default=2)
    ap.add_argument("--sizes", default="1000x1000,4096x1000,4096x4096")
    ap.add_argument("--no-small", action="store_true")
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",") if s]
    X, y, hyp = bench.synthetic_problem(3, 16)
    Xs, ys, hs = _pyvbmc_problem()
    if a.dry_run:
        for (Mr, Mc), (Xp, S) in [(s, (X, 16)) for s in sizes] + ([] if a.no_small else [((500, 50), (Xs, 8))]):
            xr, xc = _points(Xp, Mr, Mc)
            print(json.dumps(dict(N=Xp.shape[0], D=Xp.shape[1], S=S, M_ref=xr.shape[0], M_cand=xc.shape[0],
                                  flops=flops(Xp.shape[0], Mr, Mc, S))))
        return
    from gpyreg_amd import _lib

    gp = _gp(X, y, hyp)
    _lib.context(gp.device).set_option("small_timing", 1)
    rows = [_row(gp, X, Mr, Mc, a.reps, min(a.reps, a.composed_reps), "cfg3") for Mr, Mc in sizes]
    if not a.no_small:
        rows.append(_row(_gp(Xs, ys, hs), Xs, 500, 50, a.reps, a.reps, "pyvbmc"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=_lib.context(gp.device).device_info(), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
