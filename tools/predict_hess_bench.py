"""GP.predict_hess against what a caller has without it, on the cfg3 problem (N = 4096, D = 10, Matern-5, S = 16;
bench.synthetic_problem(3, 16)) for M in {100, 1000} queries (GPU box).

    python tools/predict_hess_bench.py [--out profiles/predict_hess_cfg3.json] [--reps 5] [--ms 100,1000]
                                       [--parent-lib PATH]

Routes, alternating inside one process (a warm-up round first; every call ends in a synchronise):
  (a) hess       predict_hess(xs, separate_samples=True)
  (b) hess_mean  predict_hess(xs, compute_var=False, separate_samples=True)
  (c) gradpost   gradient_posterior(xs, with_value=True, separate_samples=True)
  (d) grad       predict_grad(xs, separate_samples=True)
  (e) fd         central differences of predict_grad's analytic gradients, h = 1e-4 ell: 2 D calls
Recorded: wall time per route (median, min, max), the device time (gpc_last_timing: ms_total, ms_factor = the products
with W; "hess_contract_us" = the contraction passes of (a) and (b), kernel + reduction), the contraction's fp64 VALU
count pairs x (sets D (D + 1) + pair evaluation) FMA-equivalents and its achieved fraction of the fp64 vector rate, and
the largest relative difference between (a) and (e).
--parent-lib: a libgpcore.so built from the parent commit; routes (c) and (d) are then timed again in a child process
that loads it (GPYREG_AMD_LIB), on the same machine, and recorded as "parent"."""

import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import bench  # noqa: E402

FP64_VALU_FLOPS = 78.6e12  # MI355X: fp64 vector peak (an FMA = 2 flops)
PAIR_EVAL_INSTR = 32       # pair evaluation, Matern 5: sqrt (9), exp (19), the two polynomials (covfun.h)
S = 16


def _stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v))


def _queries(X, M):
    rng = np.random.default_rng(M)
    return X[rng.integers(0, X.shape[0], M)] + 0.3 * X.std(0, keepdims=True) * rng.standard_normal((M, X.shape[1]))


def _setup():
    X, y, hyp = bench.synthetic_problem(3, S)
    gp = bench.make_gp(3, "f64")
    gp.shard = False
    gp.update(X_new=X, y_new=y, hyp=hyp)
    return gp, X, hyp


def _time(ctx, fn, reps):
    wall, dev, prod = [], [], []
    out = None
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        tot, fac = ctx.last_timing()
        if rep:
            wall.append(1e3 * (t1 - t0))
            dev.append(tot)
            prod.append(fac)
    return out, dict(wall_ms=_stats(wall), device_ms=_stats(dev), products_ms=_stats(prod))


def _parent_rows(ms, reps):
    """Routes (c) and (d) alone: what the child process with the parent's library prints."""
    from gpyreg_amd import _lib

    gp, X, hyp = _setup()
    ctx = _lib.context(0)
    rows = {}
    for M in ms:
        xs = _queries(X, M)
        _, gpost = _time(ctx, lambda: gp.gradient_posterior(xs, with_value=True, separate_samples=True), reps)
        _, grad = _time(ctx, lambda: gp.predict_grad(xs, separate_samples=True), reps)
        rows[str(M)] = dict(gradpost=gpost, grad=grad)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/predict_hess_cfg3.json")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ms", default="100,1000")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    ms = [int(m) for m in args.ms.split(",")]
    if args.parent_child:
        from gpyreg_amd import _lib

        for name in ("gpc_predict_hess", "gpc_debug_hess_contract"):  # (the parent's library has neither)
            _lib.SIGNATURES.pop(name, None)
        print("PARENT_ROWS " + json.dumps(_parent_rows(ms, args.reps)))
        return
    from gpyreg_amd import _lib

    gp, X, hyp = _setup()
    N, D = X.shape
    ctx = _lib.context(0)
    npad = -(-N // 128) * 128
    rows = []
    for M in ms:
        xs = _queries(X, M)
        mpad = -(-M // 128) * 128
        ell = np.exp(hyp[:, :D]).mean(0)
        contract = {"hess": [], "hess_mean": []}

        def hess(var):
            r = gp.predict_hess(xs, compute_var=var, separate_samples=True)
            contract["hess" if var else "hess_mean"].append(1e-3 * ctx.get_option("hess_contract_us"))
            return r

        def fd():
            Hm, Hv = np.empty((M, D, D, S)), np.empty((M, D, D, S))
            dev = 0.0
            for b in range(D):
                e = np.zeros(D)
                e[b] = 1e-4 * ell[b]
                _, _, dmp, dsp = gp.predict_grad(xs + e, separate_samples=True)
                dev += ctx.last_timing()[0]
                _, _, dmm, dsm = gp.predict_grad(xs - e, separate_samples=True)
                dev += ctx.last_timing()[0]
                Hm[:, :, b], Hv[:, :, b] = (dmp - dmm) / (2 * e[b]), (dsp - dsm) / (2 * e[b])
            fd.dev.append(dev)
            return Hm, Hv

        fd.dev = []
        res, t = {}, {}
        res["hess"], t["hess"] = _time(ctx, lambda: hess(True), args.reps)
        res["hess_mean"], t["hess_mean"] = _time(ctx, lambda: hess(False), args.reps)
        _, t["gradpost"] = _time(ctx, lambda: gp.gradient_posterior(xs, with_value=True, separate_samples=True), args.reps)
        _, t["grad"] = _time(ctx, lambda: gp.predict_grad(xs, separate_samples=True), args.reps)
        res["fd"], t["fd"] = _time(ctx, fd, args.reps)
        t["fd"]["device_ms"] = _stats(fd.dev[1:])
        del t["fd"]["products_ms"]
        H = res["hess"]
        worst = [float((np.abs(H[4 + i] - res["fd"][i]).max(axis=(1, 2)) / np.abs(H[4 + i]).max(axis=(1, 2))).max())
                 for i in range(2)]
        pairs = float(S) * npad * mpad
        row = dict(M=M, M_pad=mpad, routes=t, fd_calls=2 * D, fd_vs_hess_max_rel=dict(Hmu=worst[0], Hs2=worst[1]))
        for route, sets in (("hess", 2), ("hess_mean", 1)):
            c_ms = float(np.median(contract[route][1:]))
            fmas = pairs * (sets * D * (D + 1) + PAIR_EVAL_INSTR)
            row["contract_" + route] = dict(ms=_stats(contract[route][1:]), pairs=pairs, valu_fma_equivalents=fmas,
                                            achieved_fraction_of_fp64_valu=(2 * fmas / (1e-3 * c_ms) / FP64_VALU_FLOPS
                                                                            if c_ms > 0 else None))
            row["speedup_%s_vs_fd" % route] = t["fd"]["wall_ms"]["median"] / t[route]["wall_ms"]["median"]
        row["hess_over_gradpost"] = t["hess"]["wall_ms"]["median"] / t["gradpost"]["wall_ms"]["median"]
        rows.append(row)
        print(json.dumps(row))
    parent = None
    if args.parent_lib:
        # a fresh child process (this one has initialised the GPU), after this one's work is done
        env = dict(os.environ, GPYREG_AMD_LIB=os.path.abspath(args.parent_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-child", "--ms", args.ms, "--reps",
                              str(args.reps)], env=env, capture_output=True, text=True, timeout=600)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("PARENT_ROWS ")]
        if out.returncode != 0 or not line:
            raise RuntimeError("the child with the parent's library failed:\n" + out.stdout[-2000:] + out.stderr[-2000:])
        parent = json.loads(line[0][len("PARENT_ROWS "):])
    rec = dict(problem=dict(cfg=3, N=N, D=D, S=S, kernel="matern5", dtype="f64"), device=ctx.device_info(),
               reps=args.reps, fp64_valu_flops=FP64_VALU_FLOPS, pair_eval_instr=PAIR_EVAL_INSTR, rows=rows,
               parent=parent)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
