"""Appending k points to resident posteriors: the block append against the two routes a caller has without it, on
the cfg3 problem (N = 4096, D = 10, Matern-5, S = 16; bench.synthetic_problem(3, 16)) and the PyVBMC-sized problem
of tools/lookahead_bench.py (N = 400, D = 6, S = 8), for k in {2, 5, 16, 64, 128, 512} (GPU box).

    python tools/block_append_bench.py [--out profiles/block_append_cfg3.json] [--reps 5] [--ks 2,5,16] [--no-small]
                                       [--engines [--engine-ks 2,5,16,32,64,128]]   (the threshold's measurement, below)
                                       [--engine 1|2]   (force the skinny kernel | the MFMA GEMM in the rows themselves)

Routes, alternating inside one process (every repeat runs all three one after the other, a warm-up round first):
  (a) block        update(X_k, y_k, block_append=True)
  (b) one_by_one   k successive one-point update calls (the rank-one path)
  (c) recompute    update(X_k, y_k) with the default: the full recompute
Every repeat of every route starts from a freshly built posterior set of size N whose construction is outside the
timed window.  Wall time per route (median, min, max; every call ends in a synchronise); device time (gpc_last_timing)
of (a) -- the whole device section after the storage growth, and its products section: the two products with W and the
k x k Gram matrix, with the conversions to and from the padded panels when the MFMA engine runs -- and of (c); the
rank-one path records none.  Also the bytes and flops per stage computed from the shapes and, where the skinny kernel ran,
its achieved bytes/s against the HBM figure of the MI355X (8 TB/s).  --engines adds an "engines" section to the record:
the block route alone on both problems with the skinny kernel and with the MFMA GEMM forced, the measurement beside
BA_GEMM_MIN_K (block_append.h).  --dry-run builds the problems and prints the plan and the shape-derived figures
without a device."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import bench  # noqa: E402
from lookahead_bench import _pyvbmc_problem  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s HBM3E peak (6.3 TB/s is what a plain copy reaches)


def _gp(X, y, hyp):
    import gpyreg_amd as gpr

    gp = gpr.GP(X.shape[1], gpr.covariance_functions.Matern(5), gpr.mean_functions.ConstantMean(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    gp.update(X_new=X, y_new=y, hyp=hyp)
    return gp


def _new_points(X, y, k):
    rng = np.random.default_rng(7 + k)
    Xn = X[rng.integers(0, X.shape[0], k)] + 0.3 * X.std(0, keepdims=True) * rng.standard_normal((k, X.shape[1]))
    yn = y.mean() + y.std() * rng.standard_normal((k, 1))
    return Xn, yn


def stages(N, k, S, w=8):
    """Shape-derived bytes and flops per stage of one block append of high-noise samples (w: bytes per stored entry).
    The skinny products read the lower triangle of W once per 16 new points and product."""
    passes = -(-k // 16)
    tri = N * (N + 1) / 2
    return dict(
        cross=dict(flops=S * N * k * 1.0, bytes=S * N * k * 8.0),
        skinny=dict(flops=S * 2 * 2.0 * tri * k, bytes=S * 2 * passes * tri * w, passes_over_W=2 * passes),
        gram=dict(flops=S * 2.0 * N * k * k, bytes=S * N * k * 8.0 * (-(-k // 64))),
        schur_factor=dict(flops=S * (2.0 / 3.0) * k**3, bytes=S * 3.0 * k * k * w),
        place=dict(flops=S * N * k * (k + 1.0), bytes=S * (2.0 * N * k * w + N * k * 8.0 * (k + 1) / 2)),
        padded_gemm_flops=S * 3.0 * N * N * 128 * (-(-k // 128)),
        recompute_flops=S * 2.0 * (N + k) ** 3 / 3.0,
    )


def _stats(v):
    v = [x for x in v if x is not None]
    if not v:
        return None
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v))


def _row(X, y, hyp, k, reps, tag, engine=0, routes=("block", "one_by_one", "recompute")):
    from gpyreg_amd import _lib

    Xn, yn = _new_points(X, y, k)
    S, N = hyp.shape[0], X.shape[0]
    ctx = None
    wall = {r: [] for r in ("block", "one_by_one", "recompute")}
    dev = {r: [] for r in ("block", "recompute")}
    skinny = []
    counts = None
    preds = {}
    for rep in range(-1, reps):  # (-1: the warm-up round)
        for route in routes:
            gp = _gp(X, y, hyp)  # outside the timed window
            ctx = _lib.context(gp.device)
            ctx.set_option("small_timing", 1)
            ctx.set_option("block_engine", engine)
            c0 = (ctx.get_option("block_appended"), ctx.get_option("block_stale"))
            t0 = time.perf_counter()
            if route == "block":
                gp.update(X_new=Xn, y_new=yn, block_append=True)
            elif route == "one_by_one":
                for i in range(k):
                    gp.update(X_new=Xn[i:i + 1], y_new=yn[i:i + 1])
            else:
                gp.update(X_new=Xn, y_new=yn)
            dt = (time.perf_counter() - t0) * 1e3
            if route == "block":
                ran = {1: "skinny", 2: "mfma"}[ctx.get_option("block_engine_ran")]  # (what the call ran, from the library)
                counts = (ctx.get_option("block_appended") - c0[0], ctx.get_option("block_stale") - c0[1])
            if rep >= 0:
                wall[route].append(dt)
                if route != "one_by_one":
                    tot, part = ctx.last_timing()
                    dev[route].append(tot)
                    if route == "block":
                        skinny.append(part)
            if rep == reps - 1:
                preds[route] = gp.predict(X[:64] + 0.05, separate_samples=True)
            del gp
    st = stages(N, k, S)
    sk = float(np.median(skinny)) if (skinny and ran == "skinny") else None  # (the traffic figure is the skinny kernel's)
    row = dict(case=tag, N=N, D=X.shape[1], S=S, k=k, engine_forced=engine, engine=ran, appended_stale=counts,
               wall_ms={r: _stats(wall[r]) for r in routes}, device_ms={r: _stats(dev[r]) for r in routes if r in dev},
               device_products_ms=_stats(skinny), stages=st,
               skinny_bytes_per_s=(st["skinny"]["bytes"] / (sk * 1e-3) if sk else None),
               skinny_share_of_hbm_peak=(st["skinny"]["bytes"] / (sk * 1e-3) / HBM_BYTES_PER_S if sk else None))
    if "one_by_one" in routes and "recompute" in routes:
        row.update(wall_block_over_one_by_one=float(np.median(wall["block"]) / np.median(wall["one_by_one"])),
                   wall_block_over_recompute=float(np.median(wall["block"]) / np.median(wall["recompute"])),
                   predictions_block_against={r: float(max(np.abs(preds["block"][i] - preds[r][i]).max() for i in (0, 1)))
                                              for r in ("one_by_one", "recompute")})
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="2,5,16,64,128,512")
    ap.add_argument("--engine", type=int, default=0, help="1 / 2: force the skinny kernel / the MFMA GEMM (0: by k)")
    ap.add_argument("--engines", action="store_true", help="add the engines section: block route, both engines forced")
    ap.add_argument("--engine-ks", default="2,5,16,32,64,128")
    ap.add_argument("--no-small", action="store_true")
    ap.add_argument("--no-cfg3", action="store_true")
    ap.add_argument("--dry-run", action="store_true")
    a = ap.parse_args()
    ks = [int(v) for v in a.ks.split(",") if v]
    problems = []
    if not a.no_cfg3:
        problems.append(("cfg3",) + tuple(bench.synthetic_problem(3, 16)))
    if not a.no_small:
        problems.append(("pyvbmc",) + tuple(_pyvbmc_problem()))
    if a.dry_run:
        for tag, X, y, hyp in problems:
            for k in ks:
                Xn, yn = _new_points(X, y, k)
                print(json.dumps(dict(case=tag, N=X.shape[0], D=X.shape[1], S=hyp.shape[0], k=Xn.shape[0],
                                      stages=stages(X.shape[0], k, hyp.shape[0]))))
        return
    from gpyreg_amd import _lib

    rows = [_row(X, y, hyp, k, a.reps, tag, a.engine) for tag, X, y, hyp in problems for k in ks]
    out = dict(device=_lib.context(0).device_info(), hbm_bytes_per_s=HBM_BYTES_PER_S, rows=rows)
    if a.engines:
        eks = [int(v) for v in a.engine_ks.split(",") if v]
        out["engines"] = {name: [_row(X, y, hyp, k, a.reps, tag, e, routes=("block",))
                                 for tag, X, y, hyp in problems for k in eks]
                          for name, e in (("skinny", 1), ("mfma", 2))}
        _lib.context(0).set_option("block_engine", 0)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
