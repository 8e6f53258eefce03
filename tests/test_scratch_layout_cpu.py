"""Every posterior consumer's declared scratch layout against its closed form (host only: gpc_debug_scratch_bytes counts
the layout as the call itself does, and carves it for three samples on a fake aligned base that is never dereferenced).

The closed forms are scratch_sizes.py's: the formulas the calls carried by hand, plus or minus the terms DESIGN.md lists.
A layout that gains, loses or resizes an array fails here without a device; so does one whose order leaves an array that
the MFMA GEMMs or the vector panel reads touch off a 16-byte boundary."""

import ctypes as C
import itertools

import pytest

import scratch_sizes as ss
from scratch_sizes import pad

F64, F32 = 0, 1
NS, MS, DS = (90, 200, 300), (1, 70, 129), (1, 3)
S = 5


@pytest.fixture(scope="module")
def lib():
    from gpyreg_amd import _lib

    return _lib.load()


def measured(lib, name, dtype, *dims):
    arr = (C.c_int * len(dims))(*[int(d) for d in dims])
    per, shared, mis = C.c_ulonglong(), C.c_ulonglong(), C.c_int(-1)
    rc = lib.gpc_debug_scratch_bytes(name.encode(), dtype, arr, len(dims), C.byref(per), C.byref(shared), C.byref(mis))
    assert rc == 0, (name, dims, rc)
    assert mis.value == 0, (name, dtype, dims, mis.value)
    return per.value, shared.value


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_rhs_products_layout(lib, dtype):
    """predict, predict_full, quad (with and without the variance), predict_K (three forms), predict_gobs, predict_grad,
    quad_grad (with and without the variance), quad_cov and draw."""
    w = 8 if dtype == F64 else 4
    kinds = {"cross": 0, "quad": 1, "given": 2, "gobs": 3}
    # (kind, want_quad, full, grad, qg, R)
    calls = [("cross", 1, 0, 0, 0, 0), ("cross", 0, 1, 0, 0, 0), ("quad", 1, 0, 0, 0, 0), ("quad", 0, 0, 0, 0, 0),
             ("given", 1, 0, 0, 0, 0), ("given", 1, 1, 0, 0, 0), ("given", 0, 1, 0, 0, 0), ("gobs", 1, 0, 0, 0, 0),
             ("cross", 1, 0, 1, 0, 0), ("quad", 1, 0, 1, 1, 0), ("quad", 0, 0, 1, 1, 0), ("quad", 0, 1, 0, 0, 0),
             ("cross", 0, 1, 0, 0, 7), ("cross", 0, 1, 0, 0, 130)]
    for N, M, D, (kind, wq, full, grad, qg, R) in itertools.product(NS + (1000,), MS + (1000,), DS, calls):
        pts = 64 * (N // 100) if kind == "gobs" else 0
        got = measured(lib, "rhs", dtype, N, M, D, S, kinds[kind], wq, full, grad, qg, R, pts)
        want = (ss.rhs_per(pad(N), pad(M), bool(full), w, D, kind, bool(wq), bool(grad), bool(qg), M, R, pts),
                ss.rhs_shared(N, M, D, S, kind, bool(full), bool(qg), R))
        assert got == want, (N, M, D, kind, wq, full, grad, qg, R, got, want)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_sibling_layouts(lib, dtype):
    """predict_cov (stored and fused), grad_post (full and diag), predict_hess (with and without the variance)."""
    w = 8 if dtype == F64 else 4
    for N, M, D in itertools.product(NS + (1100,), MS, DS):
        npad = pad(N)
        for Mb, cov, wsq in itertools.product(MS + (1100,), (0, 1), (0, 1)):
            fused = bool(wsq and not cov and (pad(M) // 128) * (pad(Mb) // 128) >= 64)
            assert measured(lib, "predict_cov", dtype, N, M, Mb, D, cov, wsq) == \
                (ss.cov_per(npad, pad(M), pad(Mb), D, w, fused), ss.cov_shared(M, Mb, D, cov)), (N, M, Mb, D, cov, wsq)
        for flag in (0, 1):
            assert measured(lib, "grad_post", dtype, N, M, D, flag) == (ss.grad_post_per(npad, D, bool(flag), w), M * D * 8)
            assert measured(lib, "predict_hess", dtype, N, M, D, flag) == (ss.predict_hess_per(npad, D, bool(flag), w), M * D * 8)
    # the fused form of predict_cov exists from 64 128-tiles on
    assert ss.cov_per(1152, 1152, 1152, 3, w, True) > ss.cov_per(1152, 1152, 1152, 3, w, False)
    assert measured(lib, "predict_cov", dtype, 1100, 1100, 1100, 3, 0, 1)[0] == ss.cov_per(1152, 1152, 1152, 3, w, True)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_update_and_cv_layouts(lib, dtype):
    """block append (k = 1, 8, 17, both engines), removal, and both cross-validation passes (both engines)."""
    w = 8 if dtype == F64 else 4
    for N in NS:
        for k, engine in itertools.product((1, 8, 17), (1, 2)):
            assert measured(lib, "append_block", dtype, N + k, k, engine) == (ss.append_block_per(pad(N + k), k, w, engine), 0)
        for k in (1, 8, 17, 70):
            kk = min(k, 64)
            assert measured(lib, "remove", dtype, N, k) == (ss.remove_per(N, k, w), (pad(N - kk) + kk) * 4), (N, k)
        assert measured(lib, "cv_loo", dtype, N) == (ss.cv_loo_per(pad(N)), 0)
        for F, kmax, engine in itertools.product((1, 3, 10), (2, 9, 130), (1, 2)):
            assert measured(lib, "cv_fold", dtype, N, F, kmax, engine) == (ss.cv_fold_per(pad(N), F, kmax, engine), 0)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["fp64", "fp32"])
def test_layouts_declared_earlier(lib, dtype):
    """nll_hess, cv_grad, predict_hyp_grad, quad_mix and the two paths calls: the same entry against the forms their
    chunking tests use."""
    w = 8 if dtype == F64 else 4
    for N, D in itertools.product(NS, DS):
        npad, cov_N = pad(N), D + 1
        for noise_N, mean_N in ((0, 0), (1, 1), (2, 3)):
            nd2 = D * (D + 1) // 2
            assert measured(lib, "nll_hess", dtype, N, cov_N, noise_N, mean_N, nd2) == \
                (ss.nll_hess_per(npad, cov_N, noise_N, mean_N, nd2), 0)
        assert measured(lib, "cv_grad", dtype, N, cov_N) == (ss.cv_grad_per(npad, cov_N), npad * 8)
        for M, var in itertools.product(MS, (0, 1)):
            P, msb = cov_N + 2, pad(M)
            nout = P + cov_N * (2 if var else 1)
            assert measured(lib, "hyp_grad", dtype, N, D, P, 1, D, msb, var, nout) == \
                (ss.hyp_grad_per(npad, D, P, 1, D, msb, bool(var), nout), 0)
            for grad in (0, 1):
                assert measured(lib, "quad_mix", dtype, N, M, D, var, grad) == \
                    (ss.quad_mix_per(npad, pad(M), D, bool(var), bool(grad)), ss.quad_mix_shared(M, pad(M), D))
            for R, engine in itertools.product((1, 40), (1, 2)):
                assert measured(lib, "paths_create", dtype, N, R, engine) == (ss.paths_create_per(npad, R, w, engine), 0)
                fpad = 256
                assert measured(lib, "paths_eval", dtype, N, M, R, S, D, fpad, engine, var) == \
                    (ss.paths_eval_per(npad, pad(M), fpad, R, D, engine), ss.paths_eval_shared(M, R, S, D, bool(var)))


def test_the_entry_refuses_what_it_does_not_know(lib):
    per, shared, mis = C.c_ulonglong(), C.c_ulonglong(), C.c_int()
    dims = (C.c_int * 4)(200, 70, 3, 0)
    args = (C.byref(per), C.byref(shared), C.byref(mis))
    assert lib.gpc_debug_scratch_bytes(b"no such layout", F64, dims, 4, *args) == -2
    assert lib.gpc_debug_scratch_bytes(b"grad_post", F64, dims, 3, *args) == -2   # a wrong number of dims
    assert lib.gpc_debug_scratch_bytes(b"grad_post", 7, dims, 4, *args) == -2     # no such dtype
    assert lib.gpc_debug_scratch_bytes(b"grad_post", F64, None, 4, *args) == -2
    assert lib.gpc_debug_scratch_bytes(b"grad_post", F64, dims, 4, *args) == 0 and per.value > 0
