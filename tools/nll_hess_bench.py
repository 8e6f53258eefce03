"""GP.nll_hess_batch against what a caller has without it -- central differences of nll_batch's analytic gradients,
2 P gradient evaluations -- on two problems (GPU box):

    cfg3   N = 4096, D = 10, Matern 5, S = 16   (bench.synthetic_problem(3, 16))
    vbmc   N = 500,  D = 6,  Matern 5, S = 8    (a VBMC-sized surrogate)

    python tools/nll_hess_bench.py [--out profiles/nll_hess_cfg3.json] [--reps 5] [--only cfg3|vbmc]

One process, a warm-up round first, medians of --reps rounds; every call ends in a synchronise.  Recorded per problem:
wall and device time of nll_hess_batch (gpc_last_timing: ms_total, and ms_factor = the planes and their GEMMs), its Gram
pass and second-derivative contraction ("nll_hess_gram_us", "nll_hess_contract_us"), the Gram kernel's achieved HBM
bytes per second (the bytes it must read: per sample, tile pair and plane p the tile of B_p and the p + 1 mirrored
tiles), the differences' wall time (one batch of 2 P S rows, the way a caller would issue them) and the ratio, and the
largest relative deviation between the two Hessians."""

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


def _cfg3():
    X, y, hyp = bench.synthetic_problem(3, 16)
    gp = bench.make_gp(3, "f64")
    return gp, X, y, hyp


def _vbmc():
    import gpyreg_amd as gpr

    N, D, S = 500, 6, 8
    rng = np.random.default_rng(0)
    X = rng.uniform(-3, 3, (N, D))
    y = -0.5 * np.sum(X**2, 1, keepdims=True) + 0.05 * rng.standard_normal((N, 1))
    gp = gpr.GP(D, gpr.covariance_functions.Matern(5), gpr.mean_functions.NegativeQuadratic(),
                gpr.noise_functions.GaussianNoise(constant_add=True))
    cov_N, noise_N, mean_N = gp._counts()
    hyp = np.zeros((S, cov_N + noise_N + mean_N))
    hyp[:, :D] = np.log(2.0)
    hyp[:, D] = np.log(1.0)
    hyp[:, cov_N] = np.log(0.05)
    hyp[:, cov_N + noise_N + 1 + D:] = np.log(1.2)
    hyp += 0.05 * rng.standard_normal(hyp.shape)
    return gp, X, y, hyp


def _run(name, make, reps):
    from gpyreg_amd import _lib

    gp, X, y, hyp = make()
    gp.shard = False
    gp.X, gp.y = X, y
    S, P = hyp.shape
    N, D = X.shape
    ctx = _lib.context(0)
    ctx.set_option("small_timing", 1)
    npad = -(-N // 128) * 128
    cov_N, noise_N, _ = gp._counts()
    ppl = cov_N + noise_N
    step = 1e-4

    def differences():
        rows = np.repeat(hyp, 2 * P, 0).reshape(S, 2 * P, P)
        rows[:, np.arange(P), np.arange(P)] += step
        rows[:, P + np.arange(P), np.arange(P)] -= step
        _, g = gp.nll_batch(rows.reshape(-1, P), compute_grad=True)
        g = g.reshape(S, 2 * P, P)
        return (g[:, :P] - g[:, P:]) / (2 * step)

    wall, dev, prod, gram, contract, fd_wall = [], [], [], [], [], []
    H = Hfd = None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        _, _, H = gp.nll_hess_batch(hyp)
        t1 = time.perf_counter()
        # (nll_hess_batch ends with an nll_batch for the values: the counters are the Hessian call's, read before)
        g_us, c_us = ctx.get_option("nll_hess_gram_us"), ctx.get_option("nll_hess_contract_us")
        t2 = time.perf_counter()
        Hfd = differences()
        t3 = time.perf_counter()
        if rep:
            wall.append(1e3 * (t1 - t0))
            gram.append(1e-3 * g_us)
            contract.append(1e-3 * c_us)
            fd_wall.append(1e3 * (t3 - t2))
    # the device sections of the Hessian call alone, through the handle (no value evaluation after it)
    pv = gp._plugin_values(hyp, True)
    kid, deg = gp._kid()
    handle, _, _, _ = ctx.posterior_batch(kid, deg, _lib.F64, hyp[:, :cov_N], pv["m"], pv["sn2"], pv["vec"])
    for rep in range(reps + 1):
        handle.nll_hess(cov_N, pv["dm"], pv["dsn2"])
        tot, fac = ctx.last_timing()
        if rep:
            dev.append(tot)
            prod.append(fac)
    handle.free()
    nt = npad // 64
    gram_bytes = float(S) * nt * nt * sum(p + 2 for p in range(ppl)) * 64 * 64 * 8
    g_ms = float(np.median(gram))
    rel = float((np.abs(H - Hfd).max(axis=(1, 2)) / np.abs(H).max(axis=(1, 2))).max())
    row = dict(problem=dict(name=name, N=N, D=D, S=S, P=P, planes=ppl, kernel="matern5", N_pad=npad),
               nll_hess=dict(wall_ms=_stats(wall), device_ms=_stats(dev), planes_and_gemm_ms=_stats(prod),
                             gram_ms=_stats(gram), contract_ms=_stats(contract)),
               gram=dict(bytes_read=gram_bytes, achieved_bytes_per_s=gram_bytes / (1e-3 * g_ms) if g_ms > 0 else None),
               gemm_flops=2.0 * S * cov_N * npad**3,
               differences=dict(gradient_rows=2 * P * S, step=step, wall_ms=_stats(fd_wall)),
               speedup_vs_differences=float(np.median(fd_wall) / np.median(wall)),
               hess_vs_differences_max_rel=rel)
    print(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/nll_hess_cfg3.json")
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
