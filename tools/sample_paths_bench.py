"""GP.sample_paths on the cfg3 posterior (N = 4096, D = 10, Matern 5, S = 16): R = 64 paths per sample with F = 1024
features, created once and evaluated at M = 1000 and M = 4096 query points, without and with the gradient, by both
evaluation engines (the fused kernel and the unfused composition: operand matrices + library GEMM), beside
draw_functions at the same M and R (GPU box).

    python tools/sample_paths_bench.py [--out profiles/sample_paths_cfg3.json] [--reps 3] [--sizes 1000,4096]
                                       [--paths 64] [--features 1024]

Wall time per call (median of --reps after one warm-up call) and the device times of gpc_last_timing: the whole device
section with its transfers, and the kernels alone.  The engine of each row is what the library reports it ran
("paths_engine_ran"), not what was asked for."""

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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="1000,4096")
    ap.add_argument("--paths", type=int, default=64)
    ap.add_argument("--features", type=int, default=1024)
    a = ap.parse_args()
    from gpyreg_amd import _lib

    X, y, hyp = bench.synthetic_problem(3, 16)
    gp = bench.make_gp(3, "f64")
    gp.update(X_new=X, y_new=y, hyp=hyp)
    ctx = _lib.context(gp.device)
    D, S, R, F = X.shape[1], hyp.shape[0], a.paths, a.features
    made = []
    t_create = _time(lambda: made.append(gp.sample_paths(n_paths=R, n_features=F, seed=1)), a.reps)
    dev_create = ctx.last_timing()
    paths = made[-1]
    for p in made[:-1]:
        p.close()
    create = dict(config=3, N=X.shape[0], D=D, S=S, R=R, F=F, create_ms=t_create, device_create_ms=dev_create[0],
                  device_solve_ms=dev_create[1], solve_engine=ctx.get_option("paths_solve_engine_ran"))
    print(json.dumps(create), flush=True)
    rows = []
    for M in (int(m) for m in a.sizes.split(",")):
        xs = np.random.default_rng(1).uniform(-3, 3, (M, D))
        row = dict(config=3, N=X.shape[0], D=D, S=S, M=M, R=R, F=F)
        for engine in (1, 2):
            ctx.set_option("paths_engine", engine)
            try:
                for grad in (False, True):
                    t = _time(lambda: paths(xs, compute_grad=grad), a.reps)
                    dev = ctx.last_timing()
                    ran = {1: "fused", 2: "unfused"}[ctx.get_option("paths_engine_ran")]
                    tag = ran + ("_grad" if grad else "")
                    row[tag + "_ms"], row[tag + "_device_ms"], row[tag + "_kernels_ms"] = t, dev[0], dev[1]
            finally:
                ctx.set_option("paths_engine", 0)
        row["draw_functions_ms"] = _time(lambda: gp.draw_functions(xs, n_draws=R, seed=1), a.reps)
        row["draw_functions_device_ms"] = ctx.last_timing()[0]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(device=ctx.device_info(), create=create, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
