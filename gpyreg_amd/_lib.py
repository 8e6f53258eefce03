"""ctypes binding of libgpcore.so (C ABI in include/gpcore.h).

There is NO CPU fallback: if the shared library is missing, or no HIP device is
visible, every compute entry point raises ``RuntimeError``.
"""

from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GPYREG_AMD_LIB: another build of the same library (A/B measurements of kernel variants)
LIB_PATH = os.environ.get("GPYREG_AMD_LIB") or os.path.join(_HERE, "lib", "libgpcore.so")

K_SE, K_MATERN, K_RQ, K_SE_ISO, K_MATERN_ISO = range(5)
F64, F32 = 0, 1
KLO_ZERO, KLO_ROW, KLO_COL = 0, 1, 2
KHI_FULL, KHI_ROW, KHI_COL = 0, 1, 2
CV_LOSSES = {"lpd": 0, "mse": 1}  # the loss of gpc_cv_grad

# Array arguments are declared void* and passed as the integer address of the NumPy buffer: `a.ctypes.data_as(POINTER(..))`
# costs ~2 us per argument, the address ~1 us, and an evaluation has a dozen of them -- a visible share of a 90 us call.
_dp = C.c_void_p  # double*
_ip = C.c_void_p  # int*
_vp = C.c_void_p
_dpp = C.POINTER(C.c_double)  # typed, for the dK callback (its argument is wrapped as an array)

# every symbol include/gpcore.h declares: (restype, argtypes)
SIGNATURES = {
    "gpc_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "gpc_destroy": (None, [_vp]),
    "gpc_last_error": (C.c_char_p, [_vp]),
    "gpc_device_info": (C.c_char_p, [_vp]),
    "gpc_set_data": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_int]),
    "gpc_cov_count": (C.c_int, [C.c_int, C.c_int]),
    "gpc_max_n": (C.c_int, [C.c_int]),
    "gpc_kernel": (
        C.c_int,
        [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp],
    ),
    "gpc_nll_batch": (
        C.c_int,
        [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int,
         _dp, C.c_int, _dp, _dp, _dp, _ip, _ip],
    ),
    "gpc_nll_batch_cm": (
        C.c_int,
        [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, C.c_int,
         _dp, _dp, _dp, _ip, _ip],
    ),
    "gpc_posterior_batch": (
        C.c_int,
        [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, C.POINTER(_vp), _dp, _ip, _ip],
    ),
    "gpc_nll_batch_K": (
        C.c_int,
        [_vp, C.c_int, C.c_int, C.c_int, _dp, _vp, _vp, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp,
         C.c_int, _dp, _dp, _dp, _ip, _ip],
    ),
    "gpc_posterior_batch_K": (
        C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, C.POINTER(_vp), _dp, _ip, _ip]),
    "gpc_predict_K": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "gpc_set_data_gobs": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int]),
    "gpc_posterior_batch_gobs": (
        C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(_vp), _dp, _dp, _ip, _ip]),
    "gpc_nll_batch_gobs": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _ip]),
    "gpc_nll_batch_gobs_grad": (
        C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _ip,
                  _ip]),
    "gpc_predict_gobs": (C.c_int, [_vp, _dp, C.c_int, _dp, _dp]),
    "gpc_debug_gobs_trace": (
        C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, C.c_double, _dp]),
    "gpc_debug_gobs_cov": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp]),
    "gpc_debug_gobs_cross": (
        C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp]),
    "gpc_debug_gobs_grad_operand": (
        C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp]),
    "gpc_grad_post_gobs": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp]),
    "gpc_post_fetch": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp]),
    "gpc_post_free": (C.c_int, [_vp]),
    "gpc_predict": (C.c_int, [_vp, _dp, C.c_int, _dp, _dp]),
    "gpc_predict_grad": (C.c_int, [_vp, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "gpc_grad_post": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp]),
    "gpc_predict_hess": (C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gpc_nll_hess": (C.c_int, [_vp, _dp, C.c_int, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    "gpc_cv_grad": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gpc_predict_hyp_grad": (
        C.c_int, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "gpc_post_append": (C.c_int, [_vp, _dp, _dp, C.c_double, _ip]),
    "gpc_post_recompute": (C.c_int, [_vp, C.c_int, _ip, _dp, _dp, _dp, C.c_int, _dp, _ip, _ip]),
    "gpc_post_append_K": (C.c_int, [_vp, _dp, _dp, _dp, _dp, C.c_double, _ip]),
    "gpc_post_append_block": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _ip]),
    "gpc_post_append_block_K": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpc_post_remove": (C.c_int, [_vp, C.c_int, _ip, _dp, _ip]),
    "gpc_debug_remove_panel": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp]),
    "gpc_debug_remove_apply": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp]),
    "gpc_post_recompute_K": (C.c_int, [_vp, C.c_int, _ip, _dp, _dp, _dp, C.c_int, _dp, _ip, _ip]),
    "gpc_predict_full": (C.c_int, [_vp, _dp, C.c_int, _dp, _dp]),
    "gpc_predict_cov": (C.c_int, [_vp, _dp, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp]),
    "gpc_lookahead_batch": (C.c_int, [_vp, _dp, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp, C.c_int, _ip, _dp]),
    "gpc_draw": (C.c_int, [_vp, _dp, C.c_int, C.c_int, C.c_ulonglong, C.c_int, _dp, _dp, _dp]),
    "gpc_paths_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_ulonglong, C.c_int, _dp, _dp, C.POINTER(_vp)]),
    "gpc_paths_eval": (C.c_int, [_vp, _dp, C.c_int, _dp, _dp]),
    "gpc_paths_free": (C.c_int, [_vp]),
    "gpc_debug_paths_fetch": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp]),
    "gpc_quad": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_int, _dp, _dp]),
    "gpc_quad_grad": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gpc_quad_cov": (C.c_int, [_vp, _dp, _dp, C.c_int, _dp, _dp]),
    "gpc_quad_mix": (C.c_int, [_vp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_int] + [_dp] * 10),
    "gpc_cv": (C.c_int, [_vp, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, _ip]),
    "gpc_last_timing": (C.c_int, [_vp, _dp, _dp]),
    "gpc_last_lauum_timing": (C.c_int, [_vp, _dp, _dp]),
    "gpc_set_option": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "gpc_get_option": (C.c_int, [_vp, C.c_char_p, _ip]),
    "gpc_mfma_peak": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp]),
    "gpc_debug_gemm": (
        C.c_int,
        [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
         C.c_int, C.c_int, _dp, _dp, _dp],
    ),
    "gpc_debug_leaf": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, _ip]),
    "gpc_debug_factor": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip]),
    "gpc_debug_factor_plan": (C.c_int, [_vp] + [C.c_int] * 7 + [_dp] * 7 + [_ip]),
    "gpc_debug_cov": (
        C.c_int,
        [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_double, C.c_double, _dp, _dp, C.c_int, C.c_int, _dp,
         C.c_int, _dp, _dp, _dp, _dp, _dp],
    ),
    "gpc_debug_blas1": (C.c_int, [_vp, C.c_int, C.c_int, _ip, _vp, _vp, _vp, _vp]),
    "gpc_debug_block_gram": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp]),
    "gpc_debug_hess_contract": (
        C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp]),
    "gpc_debug_hyp_cross": (
        C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, C.c_int, _dp, _dp]),
    "gpc_debug_nll_plane": (
        C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "gpc_debug_nll_d2": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _dp]),
    "gpc_debug_nll_gram": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp]),
    "gpc_debug_cv_trace": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "gpc_debug_cv_weights": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    "gpc_debug_normals": (C.c_int, [_vp, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp]),
    "gpc_debug_workspace_hash": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    "gpc_debug_chunk_plan": (C.c_int, [C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_int]),
    "gpc_debug_scratch_bytes": (C.c_int, [C.c_char_p, C.c_int, _ip, C.c_int, _vp, _vp, _ip]),
    "gpc_debug_gemm_queues": (C.c_int, [C.c_int] * 8 + [_ip] * 4),
    "gpc_debug_tri_masks": (C.c_int, [C.c_int] * 3 + [_ip] * 4),
    "gpc_debug_tri_usable": (C.c_int, [C.c_int] * 11),
    "gpc_debug_gemm_form": (
        C.c_int,
        [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _dp, C.c_longlong, _dp, _dp, _ip, _ip],
    ),
}
# declared under GPC_EXPERIMENTS in include/gpcore.h: present in the experiments build only (lib/libgpcore_exp.so, which
# tests/ and tools/ select through GPYREG_AMD_LIB; the product library does not export them)
EXPERIMENT_SIGNATURES = {
    "gpc_debug_dag": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _dp, _ip, C.c_int, C.c_int]),
}
EXPERIMENTS_LIB_PATH = os.path.join(_HERE, "lib", "libgpcore_exp.so")

# int (*gpc_dk_plane_fn)(void* user, int sample, int p, double* plane)
DK_PLANE_FN = C.CFUNCTYPE(C.c_int, _vp, C.c_int, C.c_int, _dpp)


class _GemmProductStruct(C.Structure):
    """gpc_gemm_product of include/gpcore.h."""
    _fields_ = ([(n, C.c_int) for n in ("M", "N", "K", "a_kmajor", "b_kmajor", "beta", "klo", "khi", "lower_only",
                                        "lda", "ldb", "ldc")]
                + [(n, C.c_longlong) for n in ("off_a", "off_b", "off_c", "s_a", "s_b", "s_c", "size_a", "size_b",
                                               "size_c")]
                + [("alpha", C.c_double), ("A", _vp), ("B", _vp), ("C", _vp)])


class GemmProduct:
    """One product of ``Context.debug_gemm_form`` (gpc_gemm_product): A, B, C are the WHOLE allocations as flat arrays;
    sample b's operands start at element off_x + b * s_x with rows ld_x apart."""

    def __init__(self, A, B, C, M, N, K, a_kmajor=0, b_kmajor=0, alpha=1.0, beta=0, klo=0, khi=0, lower_only=0,
                 lda=None, ldb=None, ldc=None, off_a=0, off_b=0, off_c=0, s_a=0, s_b=0, s_c=0):
        self.A, self.B, self.C = _f64(A).ravel(), _f64(B).ravel(), _f64(C).ravel()
        self.M, self.N, self.K = int(M), int(N), int(K)
        self.a_kmajor, self.b_kmajor = int(bool(a_kmajor)), int(bool(b_kmajor))
        self.alpha, self.beta, self.klo, self.khi, self.lower_only = float(alpha), int(beta), klo, khi, int(bool(lower_only))
        self.lda = int(lda if lda is not None else (M if a_kmajor else K))
        self.ldb = int(ldb if ldb is not None else (N if b_kmajor else K))
        self.ldc = int(ldc if ldc is not None else N)
        self.off_a, self.off_b, self.off_c = int(off_a), int(off_b), int(off_c)
        self.s_a, self.s_b, self.s_c = int(s_a), int(s_b), int(s_c)


# `which` of gpc_debug_blas1 (include/gpcore.h), and the guard after each of its result buffers
BLAS1 = {name: code for code, name in enumerate((
    "trmv", "trmv_low", "gemv_sub", "trmv_t_part", "trmv_t_part_low", "trmv_t_sum", "dot", "mat_t_vec", "grad_tail",
    "colsum_prod", "colsum_vec", "diagq", "trace_plane", "extract", "neg_sym", "pad_load", "pad_rect", "load_K",
    "rect_copy", "grow_copy", "append_row", "append_low"))}
BLAS1_GUARD = 128

FORMS = {"plain": 0, "persist": 1, "persist_reserved": 2, "dual": 3, "colsq": 4, "wsq": 5}

_lib = None
_lock = threading.RLock()


def load():
    """Load libgpcore.so and attach prototypes.  Raises RuntimeError when missing."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"{LIB_PATH} is missing: the HIP extension has not been built "
                    "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
                    "gpyreg_amd has no CPU fallback."
                )
            lib = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)  # AttributeError if the .so does not export it
                fn.restype = res
                fn.argtypes = args
            for name, (res, args) in EXPERIMENT_SIGNATURES.items():
                fn = getattr(lib, name, None)
                if fn is not None:
                    fn.restype = res
                    fn.argtypes = args
            _lib = lib
    return _lib


def is_experiments_build() -> bool:
    """True when the loaded library is the experiments build (``GPYREG_AMD_LIB=.../libgpcore_exp.so``)."""
    return hasattr(load(), "gpc_debug_dag")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    """The bare address of an array for a ``c_void_p`` argument.  KEEP-ALIVE INVARIANT: unlike ``ctypes.data_as`` the
    integer holds no reference to the array, and the call it is passed to releases the GIL -- so ``a`` must be bound to
    a name that outlives the call (every call site converts into a local first: ``x = _f64(x)`` ... ``_ptr(x)``).
    Never ``_ptr(_f64(x))`` or ``_ptr(x.ravel())`` inline: the temporary would be freed before the library reads it."""
    if a is None:
        return None
    assert isinstance(a, np.ndarray) and a.flags.c_contiguous, "pass a named, C-contiguous ndarray (see docstring)"
    return a.ctypes.data


def _serial(method):
    """A gpc_ctx is one stream with one workspace: calls on it must not overlap (include/gpcore.h), and ctypes releases
    the GIL while a call runs.  Every entry of a Context and of its PostHandles takes the context's re-entrant lock."""
    import functools

    @functools.wraps(method)
    def locked(self, *a, **k):
        with (self.lock if isinstance(self, Context) else self.ctx.lock):
            return method(self, *a, **k)

    return locked


class Context:
    """One gpc_ctx (device stream + workspace + resident X, y)."""

    def __init__(self, device: int = 0):
        self.lock = threading.RLock()
        self._lib = load()
        h = _vp()
        rc = self._lib.gpc_create(int(device), C.byref(h))
        if rc != 0:
            msg = self._lib.gpc_last_error(None).decode()
            raise RuntimeError(f"gpc_create(device={device}) failed: {msg} (no CPU fallback)")
        self._h = h
        self.device = int(device)
        self.data_token = None
        self.N = self.D = 0
        self.gobs = None  # (N, Ng) while gradient observations are resident (set_data_gobs)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.gpc_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed (rc={rc}): {self._lib.gpc_last_error(self._h).decode()}")

    def device_info(self) -> str:
        return self._lib.gpc_device_info(self._h).decode()

    # ---- data -----------------------------------------------------------------
    @_serial
    def set_data(self, X, y, token=None):
        X = _f64(X)
        y = _f64(y).ravel()
        N, D = X.shape
        if y.size != N:  # (the library reads N values of y: a shorter array would be read past its end)
            raise ValueError(f"X has {N} points and y has {y.size}: every input needs its observation")
        self._check(self._lib.gpc_set_data(self._h, _ptr(X), _ptr(y), N, D), "gpc_set_data")
        self.N, self.D = N, D
        self.gobs = None
        self.data_token = token

    @_serial
    def set_data_gobs(self, X, y, Xg, dy, token=None):
        """gpc_set_data_gobs: values y (N,) at X (N, D) and gradients dy (Ng, D) at Xg (Ng, D).  The context's problem
        order becomes the joint order n = N + Ng D (``self.N``); ``self.gobs`` = (N, Ng)."""
        X, y, Xg, dy = _f64(X), _f64(y).ravel(), _f64(Xg), _f64(dy)
        N, D = X.shape
        Ng = Xg.shape[0]
        if y.size != N or Xg.shape != (Ng, D) or dy.shape != (Ng, D):
            raise ValueError(f"X is {X.shape}, y has {y.size} values, Xg is {Xg.shape} and dy {dy.shape}: y needs N values, "
                             "Xg and dy (Ng, D)")
        self._check(self._lib.gpc_set_data_gobs(self._h, _ptr(X), _ptr(y), N, D, _ptr(Xg), _ptr(dy), Ng),
                    "gpc_set_data_gobs")
        self.N, self.D = N + Ng * D, D
        self.gobs = (N, Ng)
        self.data_token = token

    def _gobs_args(self, hyp_cov, m, sn2):
        hyp_cov, m, sn2 = _f64(hyp_cov), _f64(m), _f64(sn2)
        S = hyp_cov.shape[0]
        if m.shape != (S, self.N) or sn2.shape != (S, self.N):
            raise ValueError(f"m and sn2 must be (S, n) = ({S}, {self.N}) in joint order")
        return hyp_cov, m, sn2, S, np.empty(S), np.empty(S), np.empty(S, dtype=np.int32), np.empty(S, dtype=np.int32)

    @_serial
    def posterior_batch_gobs(self, kid, degree, dtype, hyp_cov, m, sn2):
        """gpc_posterior_batch_gobs on the data of ``set_data_gobs``: (handle, nlz, mult, lchol, info)."""
        hyp_cov, m, sn2, S, nlz, mult, lchol, info = self._gobs_args(hyp_cov, m, sn2)
        h = _vp()
        rc = self._lib.gpc_posterior_batch_gobs(self._h, kid, degree, dtype, S, _ptr(hyp_cov), _ptr(m), _ptr(sn2),
                                                C.byref(h), _ptr(nlz), _ptr(mult), lchol.ctypes.data, info.ctypes.data)
        self._check(rc, "gpc_posterior_batch_gobs")
        return PostHandle(self, h, S, self.N), nlz, mult, lchol.astype(bool), info

    @_serial
    def nll_batch_gobs(self, kid, degree, dtype, hyp_cov, m, sn2):
        """gpc_nll_batch_gobs: (nlz, mult, lchol, info) for the rows of hyp_cov."""
        hyp_cov, m, sn2, S, nlz, mult, lchol, info = self._gobs_args(hyp_cov, m, sn2)
        rc = self._lib.gpc_nll_batch_gobs(self._h, kid, degree, dtype, S, _ptr(hyp_cov), _ptr(m), _ptr(sn2), _ptr(nlz),
                                          _ptr(mult), lchol.ctypes.data, info.ctypes.data)
        self._check(rc, "gpc_nll_batch_gobs")
        return nlz, mult, lchol.astype(bool), info

    @_serial
    def nll_batch_gobs_grad(self, kid, degree, dtype, hyp_cov, m, sn2, dm=None, dsn2=None):
        """gpc_nll_batch_gobs_grad: (nlz, dnlz (S, cov_N + noise_N + mean_N), mult, lchol, info).  dm (S, n, mean_N) and
        dsn2 (S, n, noise_N) are the joint-ordered derivative rows (None: no such hyperparameters)."""
        hyp_cov, m, sn2, S, nlz, mult, lchol, info = self._gobs_args(hyp_cov, m, sn2)
        dm = None if dm is None or dm.shape[-1] == 0 else _f64(dm)
        dsn2 = None if dsn2 is None or dsn2.shape[-1] == 0 else _f64(dsn2)
        for name, d in (("dm", dm), ("dsn2", dsn2)):
            if d is not None and d.shape[:2] != (S, self.N):
                raise ValueError(f"{name} must be (S, n, count) = ({S}, {self.N}, count) in joint order, got {d.shape}")
        mean_N = 0 if dm is None else dm.shape[2]
        noise_N = 0 if dsn2 is None else dsn2.shape[2]
        dnlz = np.empty((S, hyp_cov.shape[1] + noise_N + mean_N))
        rc = self._lib.gpc_nll_batch_gobs_grad(self._h, kid, degree, dtype, S, _ptr(hyp_cov), _ptr(m), _ptr(sn2), _ptr(dm),
                                               mean_N, _ptr(dsn2), noise_N, _ptr(nlz), _ptr(dnlz), _ptr(mult),
                                               lchol.ctypes.data, info.ctypes.data)
        self._check(rc, "gpc_nll_batch_gobs_grad")
        return nlz, dnlz, mult, lchol.astype(bool), info

    @_serial
    def debug_gobs_trace(self, kid, degree, hyp_cov, X, Xg, Ainv, alpha, sl=1.0):
        """gpc_debug_gobs_trace: (cov_N,) sums of (Ainv / sl - alpha alpha^T) o dK / dtheta_p as gobs_trace_kernel and
        its reduction compute them; only the lower triangle of Ainv (n, n) is read."""
        hyp_cov, X, Xg, Ainv, alpha = _f64(hyp_cov).ravel(), _f64(X), _f64(Xg), _f64(Ainv), _f64(alpha).ravel()
        (N, D), Ng = X.shape, Xg.shape[0]
        n = N + Ng * D
        if Ainv.shape != (n, n) or alpha.size != n:
            raise ValueError(f"Ainv must be (n, n) and alpha (n,) with n = {n} in joint order")
        out = np.empty(hyp_cov.size)
        rc = self._lib.gpc_debug_gobs_trace(self._h, kid, degree, _ptr(hyp_cov), _ptr(X), N, D, _ptr(Xg), Ng, _ptr(Ainv),
                                            _ptr(alpha), float(sl), _ptr(out))
        self._check(rc, "gpc_debug_gobs_trace")
        return out

    @_serial
    def debug_gobs_cov(self, kid, degree, hyp_cov, X, Xg):
        """gpc_debug_gobs_cov: the n x n joint covariance of one hyperparameter row, as gobs_cov_kernel writes it."""
        hyp_cov, X, Xg = _f64(hyp_cov).ravel(), _f64(X), _f64(Xg)
        (N, D), Ng = X.shape, Xg.shape[0]
        out = np.empty((N + Ng * D, N + Ng * D))
        rc = self._lib.gpc_debug_gobs_cov(self._h, kid, degree, _ptr(hyp_cov), _ptr(X), N, D, _ptr(Xg), Ng, _ptr(out))
        self._check(rc, "gpc_debug_gobs_cov")
        return out

    @_serial
    def debug_gobs_cross(self, kid, degree, hyp_cov, X, Xg, x_star, alpha=None):
        """gpc_debug_gobs_cross: (operand (n, M), the whole padded panel it is a corner of, fused column sums (M,) |
        None without alpha), as gobs_cross_tile_kernel writes them."""
        hyp_cov, X, Xg, xs = _f64(hyp_cov).ravel(), _f64(X), _f64(Xg), _f64(x_star)
        (N, D), Ng, M = X.shape, Xg.shape[0], xs.shape[0]
        n = N + Ng * D
        npad, mpad = -(-n // 128) * 128, -(-M // 128) * 128
        al = None if alpha is None else _f64(alpha).ravel()
        if al is not None and al.size != n:
            raise ValueError(f"alpha must hold n = {n} values in joint order")
        panel = np.empty((npad, mpad))
        col = None if al is None else np.empty(mpad)
        rc = self._lib.gpc_debug_gobs_cross(self._h, kid, degree, _ptr(hyp_cov), _ptr(X), N, D, _ptr(Xg), Ng, _ptr(xs), M,
                                            _ptr(al), _ptr(panel), _ptr(col))
        self._check(rc, "gpc_debug_gobs_cross")
        return panel[:n, :M].copy(), panel, (None if col is None else col[:M].copy())

    @_serial
    def debug_gobs_grad_operand(self, kid, degree, hyp_cov, X, Xg, x_star, alpha=None):
        """gpc_debug_gobs_grad_operand: (operand (n, D + 1, M), the whole padded panel (npad, D + 1, 128) it is a corner
        of, fused column sums (D + 1, M) | None without alpha), as gobs_grad_operand_tile_kernel writes them for one
        block of M <= 128 queries: slot 0 = f(x*), slot 1 + l = d f / dx*_l, rows in joint order."""
        hyp_cov, X, Xg, xs = _f64(hyp_cov).ravel(), _f64(X), _f64(Xg), _f64(x_star)
        (N, D), Ng, M = X.shape, Xg.shape[0], xs.shape[0]
        n = N + Ng * D
        npad = -(-n // 128) * 128
        al = None if alpha is None else _f64(alpha).ravel()
        if al is not None and al.size != n:
            raise ValueError(f"alpha must hold n = {n} values in joint order")
        panel = np.empty((npad, D + 1, 128))
        col = None if al is None else np.empty((D + 1, 128))
        rc = self._lib.gpc_debug_gobs_grad_operand(self._h, kid, degree, _ptr(hyp_cov), _ptr(X), N, D, _ptr(Xg), Ng,
                                                   _ptr(xs), M, _ptr(al), _ptr(panel), _ptr(col))
        self._check(rc, "gpc_debug_gobs_grad_operand")
        return panel[:n, :, :M].copy(), panel, (None if col is None else col[:, :M].copy())

    # ---- covariance.compute ---------------------------------------------------
    @_serial
    def kernel(self, kid, degree, hyp, X, X_star=None, diag=False, grad=False):
        X = _f64(X)
        hyp = _f64(hyp)
        N, D = X.shape
        cov_N = self._lib.gpc_cov_count(kid, D)
        Xs = None if X_star is None else _f64(X_star)
        M = 0 if Xs is None else Xs.shape[0]
        if diag:
            K = np.empty((N, 1))
        else:
            K = np.empty((N, M if Xs is not None else N))
        dK = np.empty((N, N, cov_N)) if grad else None
        rc = self._lib.gpc_kernel(self._h, kid, degree, _ptr(hyp), _ptr(X), N, D, _ptr(Xs), M,
                                  1 if diag else 0, _ptr(K), _ptr(dK))
        self._check(rc, "gpc_kernel")
        return (K, dK) if grad else K

    # ---- core -----------------------------------------------------------------
    @_serial
    def nll_batch(self, kid, degree, dtype, hyp_cov, m, sn2, sn2_is_vector, want_grad=False,
                  dm=None, dsn2=None):
        """hyp_cov (S,cov_N); m (S,N); sn2 (S,N) if sn2_is_vector else (S,1);
        dm (S,N,mean_N); dsn2 (S, N if sn2_is_vector else 1, noise_N)."""
        hyp_cov = _f64(hyp_cov)
        m = _f64(m)
        sn2 = _f64(sn2)
        S, cov_N = hyp_cov.shape
        vec = 1 if sn2_is_vector else 0
        if sn2.shape != (S, self.N if vec else 1) or m.shape != (S, self.N):
            raise ValueError("m must be (S,N); sn2 must be (S,N) when per-point, else (S,1)")
        mean_N = 0 if dm is None else dm.shape[2]
        noise_N = 0 if dsn2 is None else dsn2.shape[2]
        dm_c = None if dm is None or mean_N == 0 else _f64(dm)
        dsn2_c = None if dsn2 is None or noise_N == 0 else _f64(dsn2)
        hyp_N = cov_N + noise_N + mean_N
        nlz = np.empty(S)
        dnlz = np.empty((S, hyp_N)) if want_grad else None
        mult = np.empty(S)
        lchol = np.empty(S, dtype=np.int32)
        info = np.empty(S, dtype=np.int32)
        rc = self._lib.gpc_nll_batch(
            self._h, kid, degree, dtype, S, _ptr(hyp_cov), _ptr(m), _ptr(sn2), vec,
            1 if want_grad else 0, _ptr(dm_c), mean_N, _ptr(dsn2_c), noise_N, _ptr(nlz), _ptr(dnlz),
            _ptr(mult), lchol.ctypes.data, info.ctypes.data)
        self._check(rc, "gpc_nll_batch")
        return nlz, dnlz, mult, lchol.astype(bool), info

    @_serial
    def nll_batch_cm(self, kid, degree, dtype, hyp_cov, m0, sn2, sn2_is_vector, want_grad=False, dsn2=None):
        """gpc_nll_batch_cm: the stock zero / constant mean as ONE value per sample -- m0 (S,) or None for the zero
        mean; dsn2 (S, N if sn2_is_vector else 1, noise_N).  Same results as ``nll_batch`` with m = m0 and dm = 1."""
        hyp_cov = _f64(hyp_cov)
        sn2 = _f64(sn2)
        S, cov_N = hyp_cov.shape
        vec = 1 if sn2_is_vector else 0
        mean_N = 0 if m0 is None else 1
        m0_c = None if m0 is None else _f64(m0).ravel()
        if sn2.shape != (S, self.N if vec else 1) or (m0_c is not None and m0_c.shape != (S,)):
            raise ValueError("m0 must be (S,); sn2 must be (S,N) when per-point, else (S,1)")
        noise_N = 0 if dsn2 is None else dsn2.shape[2]
        dsn2_c = None if dsn2 is None or noise_N == 0 else _f64(dsn2)
        hyp_N = cov_N + noise_N + mean_N
        nlz = np.empty(S)
        dnlz = np.empty((S, hyp_N)) if want_grad else None
        mult = np.empty(S)
        lchol = np.empty(S, dtype=np.int32)
        info = np.empty(S, dtype=np.int32)
        rc = self._lib.gpc_nll_batch_cm(
            self._h, kid, degree, dtype, S, _ptr(hyp_cov), _ptr(m0_c), mean_N, _ptr(sn2), vec,
            1 if want_grad else 0, _ptr(dsn2_c), noise_N, _ptr(nlz), _ptr(dnlz), _ptr(mult), lchol.ctypes.data,
            info.ctypes.data)
        self._check(rc, "gpc_nll_batch_cm")
        return nlz, dnlz, mult, lchol.astype(bool), info

    @_serial
    def nll_batch_K(self, dtype, K, dK_plane, cov_N, m, sn2, sn2_is_vector, want_grad=False, dm=None,
                    dsn2=None):
        """gpc_nll_batch_K: K (S,N,N) from the caller's covariance object; ``dK_plane(s, p)`` returns
        the (N,N) array dK[:, :, p] of sample s (called once per sample and hyperparameter)."""
        K = _f64(K)
        m = _f64(m)
        sn2 = _f64(sn2)
        S, N = K.shape[0], K.shape[1]
        vec = 1 if sn2_is_vector else 0
        if K.shape != (S, self.N, self.N) or sn2.shape != (S, self.N if vec else 1) or m.shape != (S, self.N):
            raise ValueError("K must be (S,N,N); m (S,N); sn2 (S,N) when per-point, else (S,1)")
        mean_N = 0 if dm is None else dm.shape[2]
        noise_N = 0 if dsn2 is None else dsn2.shape[2]
        dm_c = None if dm is None or mean_N == 0 else _f64(dm)
        dsn2_c = None if dsn2 is None or noise_N == 0 else _f64(dsn2)
        hyp_N = cov_N + noise_N + mean_N
        nlz = np.empty(S)
        dnlz = np.empty((S, hyp_N)) if want_grad else None
        mult = np.empty(S)
        lchol = np.empty(S, dtype=np.int32)
        info = np.empty(S, dtype=np.int32)
        err = []

        def plane_cb(_user, s, p, out):
            try:
                np.ctypeslib.as_array(out, shape=(N, N))[...] = dK_plane(s, p)
                return 0
            except Exception as e:  # noqa: BLE001 - reported through the return code, re-raised below
                err.append(e)
                return 1

        cb = DK_PLANE_FN(plane_cb)
        rc = self._lib.gpc_nll_batch_K(
            self._h, dtype, S, cov_N, _ptr(K), C.cast(cb, _vp) if want_grad else None, None, _ptr(m),
            _ptr(sn2), vec, 1 if want_grad else 0, _ptr(dm_c), mean_N, _ptr(dsn2_c), noise_N, _ptr(nlz),
            _ptr(dnlz), _ptr(mult), lchol.ctypes.data, info.ctypes.data)
        if err:
            raise err[0]
        self._check(rc, "gpc_nll_batch_K")
        return nlz, dnlz, mult, lchol.astype(bool), info

    @_serial
    def posterior_batch_K(self, dtype, K, m, sn2, sn2_is_vector):
        K, m, sn2 = _f64(K), _f64(m), _f64(sn2)
        S = K.shape[0]
        vec = 1 if sn2_is_vector else 0
        if K.shape != (S, self.N, self.N) or sn2.shape != (S, self.N if vec else 1) or m.shape != (S, self.N):
            raise ValueError("K must be (S,N,N); m (S,N); sn2 (S,N) when per-point, else (S,1)")
        mult = np.empty(S)
        lchol = np.empty(S, dtype=np.int32)
        info = np.empty(S, dtype=np.int32)
        h = _vp()
        rc = self._lib.gpc_posterior_batch_K(self._h, dtype, S, _ptr(K), _ptr(m), _ptr(sn2), vec, C.byref(h),
                                             _ptr(mult), lchol.ctypes.data, info.ctypes.data)
        self._check(rc, "gpc_posterior_batch_K")
        return PostHandle(self, h, S, self.N), mult, lchol.astype(bool), info

    @_serial
    def posterior_batch(self, kid, degree, dtype, hyp_cov, m, sn2, sn2_is_vector):
        hyp_cov = _f64(hyp_cov)
        m = _f64(m)
        sn2 = _f64(sn2)
        S = hyp_cov.shape[0]
        vec = 1 if sn2_is_vector else 0
        if sn2.shape != (S, self.N if vec else 1) or m.shape != (S, self.N):
            raise ValueError("m must be (S,N); sn2 must be (S,N) when per-point, else (S,1)")
        mult = np.empty(S)
        lchol = np.empty(S, dtype=np.int32)
        info = np.empty(S, dtype=np.int32)
        h = _vp()
        rc = self._lib.gpc_posterior_batch(
            self._h, kid, degree, dtype, S, _ptr(hyp_cov), _ptr(m), _ptr(sn2), vec, C.byref(h),
            _ptr(mult), lchol.ctypes.data, info.ctypes.data)
        self._check(rc, "gpc_posterior_batch")
        return PostHandle(self, h, S, self.N), mult, lchol.astype(bool), info

    @_serial
    def last_timing(self):
        a, b = C.c_double(), C.c_double()
        self._lib.gpc_last_timing(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    @_serial
    def set_option(self, name: str, value: int):
        self._check(self._lib.gpc_set_option(self._h, name.encode(), int(value)), "gpc_set_option")

    @_serial
    def get_option(self, name: str) -> int:
        v = C.c_int()
        self._check(self._lib.gpc_get_option(self._h, name.encode(), C.byref(v)), "gpc_get_option")
        return v.value

    @_serial
    def last_lauum_timing(self):
        a, b = C.c_double(), C.c_double()
        self._lib.gpc_last_lauum_timing(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    @_serial
    def mfma_peak(self, dtype=F64):
        """(TFLOP/s, shader cycles per MFMA per SIMD, clock in GHz) of a bare MFMA loop."""
        t, cyc, ghz = C.c_double(), C.c_double(), C.c_double()
        rc = self._lib.gpc_mfma_peak(self._h, dtype, C.byref(t), C.byref(cyc), C.byref(ghz))
        self._check(rc, "gpc_mfma_peak")
        return t.value, cyc.value, ghz.value

    # ---- test hooks -------------------------------------------------------------
    @_serial
    def debug_gemm(self, A, B, Cm, M, N, K, a_kmajor, b_kmajor, alpha=1.0, beta=0, klo=0, khi=0,
                   lower_only=False, dtype=F64, force_bt=0):
        A, B = _f64(A), _f64(B)
        Cm = _f64(Cm).copy()
        flags = int(bool(lower_only)) | {0: 0, 64: 0x100, 128: 0x200, 12864: 0x400}[force_bt]  # (12864: experiments build)
        rc = self._lib.gpc_debug_gemm(self._h, dtype, M, N, K, int(a_kmajor), int(b_kmajor),
                                      float(alpha), int(beta), klo, khi, flags, _ptr(A),
                                      _ptr(B), _ptr(Cm))
        self._check(rc, "gpc_debug_gemm")
        return Cm

    @_serial
    def debug_gemm_form(self, form, products, batch=1, tile=128, flags=None, block_slots=0, dtype=F64, ep_w=None,
                        ep_sw=0, ep_alpha=None):
        """gpc_debug_gemm_form: ``products`` (one GemmProduct, two for "dual") through the launch form ``form`` (a key
        of FORMS) with ``flags`` in place of the GEMM flags and ``block_slots`` in place of the chip's block slots for
        this call.  Returns None when the form is unavailable on this context ("persist_reserved" without a table of
        reserved CUs), else a dict: C (the whole C allocation of every product after the launch; the inputs are not
        modified), colsq ((batch, M / 128, N), the epilogue forms, else None), counters (the 8 queue counters)."""
        prods = [products] if isinstance(products, GemmProduct) else list(products)
        outs, structs = [], []
        for p in prods:
            Cout = p.C.copy()
            outs.append(Cout)
            structs.append(_GemmProductStruct(
                p.M, p.N, p.K, p.a_kmajor, p.b_kmajor, p.beta, p.klo, p.khi, p.lower_only, p.lda, p.ldb, p.ldc,
                p.off_a, p.off_b, p.off_c, p.s_a, p.s_b, p.s_c, p.A.size, p.B.size, Cout.size, p.alpha,
                _ptr(p.A), _ptr(p.B), _ptr(Cout)))
        code = FORMS[form]
        p0 = prods[0]
        colsq = np.empty((batch, p0.M // 128, p0.N)) if code >= 4 else None
        w = al = None
        if code == 5:
            w, al = _f64(ep_w).ravel(), _f64(ep_alpha).ravel()
            if w.size != (batch - 1) * ep_sw + p0.M or al.size != batch:
                raise ValueError("debug_gemm_form: ep_w holds (batch - 1) * ep_sw + M weights, ep_alpha one factor per sample")
        counters = np.zeros(8, dtype=np.int32)
        avail = C.c_int(0)
        rc = self._lib.gpc_debug_gemm_form(
            self._h, dtype, code, int(tile), int(batch), -1 if flags is None else int(flags), int(block_slots),
            C.addressof(structs[0]), C.addressof(structs[1]) if len(structs) > 1 else None, _ptr(w), int(ep_sw),
            _ptr(al), _ptr(colsq), counters.ctypes.data, C.addressof(avail))
        self._check(rc, "gpc_debug_gemm_form")
        if not avail.value:
            return None
        return dict(C=outs, colsq=colsq, counters=counters)

    @_serial
    def debug_factor(self, A, want_inv=True, dtype=F64):
        A = _f64(A)
        n = A.shape[0]
        L, W = np.empty((n, n)), np.empty((n, n))
        Ainv = np.empty((n, n)) if want_inv else None
        logdet = C.c_double()
        info = C.c_int()
        rc = self._lib.gpc_debug_factor(self._h, dtype, n, _ptr(A), _ptr(L), _ptr(W), _ptr(Ainv),
                                        C.byref(logdet), C.byref(info))
        self._check(rc, "gpc_debug_factor")
        return L, W, Ainv, logdet.value, info.value

    @_serial
    def debug_factor_plan(self, A, W, T, nvalid, plan=0, nll_block=0, stable=False, keep_L=False, want_inv=False,
                          r=None, dtype=F64):
        """gpc_debug_factor_plan: the launch plan of plan.h on a batch, as the product runs it.  A, W, T: (batch, npad,
        npad), uploaded whole and verbatim -- padding and poison included -- and returned whole as the factorization
        left them (the arguments are not modified).  plan 0 / 1: potrf_inv with / without the whole inverse, 2:
        potrf_nll with ``nll_block``.  ``r`` (batch, npad): also the plan's forward solve z = L^-1 r.  ``want_inv``
        (plan 0): also the scratch after Ainv = W^T W went into it.  Returns a dict A, W, T, z, Ainv, logdet, info."""
        A, W, T = _f64(A).copy(), _f64(W).copy(), _f64(T).copy()
        if A.ndim != 3 or A.shape[1] != A.shape[2] or W.shape != A.shape or T.shape != A.shape:
            raise ValueError("debug_factor_plan: A, W, T (batch, npad, npad)")
        batch, npad, _ = A.shape
        rr = z = None
        if r is not None:
            rr = _f64(r)
            if rr.shape != (batch, npad):
                raise ValueError("debug_factor_plan: r (batch, npad)")
            z = np.empty((batch, npad))
        Ainv = np.empty_like(A) if want_inv else None
        logdet = np.empty(batch)
        info = np.empty(batch, dtype=np.int32)
        flags = (1 if stable else 0) | (2 if keep_L else 0) | (4 if want_inv else 0)
        rc = self._lib.gpc_debug_factor_plan(self._h, dtype, npad, int(nvalid), batch, int(plan), int(nll_block), flags,
                                             _ptr(A), _ptr(W), _ptr(T), _ptr(rr), _ptr(z), _ptr(Ainv), _ptr(logdet),
                                             info.ctypes.data)
        self._check(rc, "gpc_debug_factor_plan")
        return dict(A=A, W=W, T=T, z=z, Ainv=Ainv, logdet=logdet, info=info)

    @_serial
    def debug_cov(self, which, kid, degree, hyp_cov, X, dtype=F64, kscale=1.0, sl=1.0, dvec=None, X_star=None,
                  mat=None, vec=None):
        """gpc_debug_cov on one sample.  which = "build" | "front": A (npad, npad); "cross": Ks (npad, mpad) and the
        fused column sums Ks^T vec (mpad,); "trace": the cov_N + 1 sums and diag(Q) (npad,) for Q = mat / sl - vec vec^T.
        "grad_operand": gpc_grad_post's operand, the panel rearranged to (npad, D + 1, mpad) (slot 0 = k, slot 1 + l =
        dk/dx*_l) and its fused column sums against vec (D + 1, mpad).
        The last entry of the returned tuple is always the scaled inputs (npad, D) -- for "cross" the pair (Xs, Xss)."""
        code = {"build": 0, "front": 1, "cross": 2, "trace": 3, "grad_operand": 4}[which]
        X, hyp_cov = _f64(X), _f64(hyp_cov).ravel()
        N, D = X.shape
        npad = -(-N // 128) * 128
        dvec = None if dvec is None else _f64(dvec).ravel()
        vec = None if vec is None else _f64(vec).ravel()
        mat = None if mat is None else _f64(mat)
        Xq = None if X_star is None else _f64(X_star)
        M = 0 if Xq is None else Xq.shape[0]
        mpad = -(-M // 128) * 128
        if (dvec is not None and dvec.size != N) or (vec is not None and vec.size != N) or \
                (mat is not None and mat.shape != (N, N)) or (Xq is not None and Xq.shape[1] != D):
            raise ValueError("debug_cov: dvec (N,), vec (N,), mat (N, N), X_star (M, D)")
        xs = np.empty((npad + (mpad if code == 2 else 0), D))
        if code < 2:
            out0, out1 = np.empty((npad, npad)), None
        elif code == 2:
            out0, out1 = np.empty((npad, mpad)), np.empty(mpad)
        elif code == 4:  # per block of 128 queries: [block][npad][D + 1][128] and [block][D + 1][128]
            out0, out1 = np.empty((mpad // 128, npad, D + 1, 128)), np.empty((mpad // 128, D + 1, 128))
        else:
            out0, out1 = np.empty(self._lib.gpc_cov_count(kid, D) + 1), np.empty(npad)
        rc = self._lib.gpc_debug_cov(self._h, code, kid, degree, dtype, _ptr(hyp_cov), float(kscale), float(sl),
                                     _ptr(dvec), _ptr(X), N, D, _ptr(Xq), M, _ptr(mat), _ptr(vec), _ptr(out0),
                                     _ptr(out1), _ptr(xs))
        self._check(rc, "gpc_debug_cov")
        if code < 2:
            return out0, xs
        if code == 2:
            return out0, out1, (xs[:npad], xs[npad:])
        if code == 4:
            return (out0.transpose(1, 2, 0, 3).reshape(npad, D + 1, mpad),
                    out1.transpose(1, 0, 2).reshape(D + 1, mpad), xs)
        return out0, out1, xs

    @_serial
    def debug_blas1(self, which, ip, ins, out_sizes, dtype=F64):
        """gpc_debug_blas1: one launch of the blas1.h kernel ``which`` (a key of ``BLAS1``) with the int parameters ``ip``
        on the operands ``ins`` (at most six arrays, None: absent; uploaded whole) -- the table in include/gpcore.h gives
        both per kernel.  ``out_sizes``: the element count of every result (0: a buffer that is its guard alone).
        Returns one flat array per result, ``size + BLAS1_GUARD`` long: the buffer as the launch left it, then its
        guard."""
        if len(ins) > 6 or len(out_sizes) > 3:
            raise ValueError("debug_blas1: at most six operands and three results")
        ipa = np.zeros(8, dtype=np.int32)
        ipa[:len(ip)] = ip
        arrs = [None if a is None else _f64(a).ravel() for a in ins]
        arrs += [None] * (6 - len(arrs))
        sizes = [int(n) for n in out_sizes]
        outs = [np.empty(n + BLAS1_GUARD) for n in sizes] + [None] * (3 - len(sizes))
        in_p = (C.c_void_p * 6)(*[_ptr(a) for a in arrs])
        in_n = (C.c_longlong * 6)(*[0 if a is None else a.size for a in arrs])
        out_p = (C.c_void_p * 3)(*[_ptr(o) for o in outs])
        out_n = (C.c_longlong * 3)(*(sizes + [0] * (3 - len(sizes))))
        rc = self._lib.gpc_debug_blas1(self._h, BLAS1[which], dtype, _ptr(ipa), C.addressof(in_p), C.addressof(in_n),
                                       C.addressof(out_p), C.addressof(out_n))
        self._check(rc, "gpc_debug_blas1")
        return [o for o in outs if o is not None]

    @_serial
    def debug_remove_panel(self, D, Vp, dtype=F64):
        """gpc_debug_remove_panel: the panel kernel of the point removal on D (64, 64; lower triangle) and Vp (64, k).
        Returns (Theta (64 + k, 64 + k), Dnew (64, 64)) with [D | Vp] Theta = [Dnew | 0]."""
        D, Vp = _f64(D), _f64(Vp)
        if D.shape != (64, 64) or Vp.ndim != 2 or Vp.shape[0] != 64:
            raise ValueError("debug_remove_panel: D (64, 64) and Vp (64, k)")
        k = Vp.shape[1]
        theta, dnew = np.empty((64 + k, 64 + k)), np.empty((64, 64))
        rc = self._lib.gpc_debug_remove_panel(self._h, dtype, k, _ptr(D), _ptr(Vp), _ptr(theta), _ptr(dnew))
        self._check(rc, "gpc_debug_remove_panel")
        return theta, dnew

    @_serial
    def debug_remove_apply(self, side, a, Theta, P, Cr, dtype=F64):
        """gpc_debug_remove_apply: the apply kernel of the point removal on a given Theta (64 + k, 64 + k) for the
        panel [a, a + 64).  ``side`` "L": P (rows, 64) = L[a+64:, a:a+64], Cr (rows, k) -> [P | Cr] Theta;  "W":
        P (64, n) = W[a:a+64, :n], Cr (k, n) -> Theta^T [P ; Cr] (entries of P above the diagonal come back as given).
        Returns the new (P, Cr)."""
        Theta, P, Cr = _f64(Theta), _f64(P).copy(), _f64(Cr).copy()
        k = Theta.shape[0] - 64
        if side == "L":
            n = a + 64 + P.shape[0]
            good = P.shape == (n - a - 64, 64) and Cr.shape == (P.shape[0], k)
        else:
            n = P.shape[1]
            good = side == "W" and P.shape == (64, n) and Cr.shape == (k, n)
        if not good or Theta.shape != (64 + k, 64 + k):
            raise ValueError("debug_remove_apply: Theta (64 + k, 64 + k); L: P (rows, 64), Cr (rows, k); W: P (64, n), Cr (k, n)")
        rc = self._lib.gpc_debug_remove_apply(self._h, dtype, 0 if side == "L" else 1, int(a), n, k, _ptr(Theta), _ptr(P),
                                              _ptr(Cr))
        self._check(rc, "gpc_debug_remove_apply")
        return P, Cr

    @_serial
    def debug_block_gram(self, Y, Z=None, dtype=F64, diag_only=False):
        """gpc_debug_block_gram: Y, Z (n, Dp, M) panels (Z None: Z = Y).  Returns (M, Dp, Dp): [j, a, b] = [j, b, a] =
        sum_i Y[i, a, j] Z[i, b, j] for a >= b, accumulated in fp64 from the values stored in ``dtype``; with
        ``diag_only`` (M, Dp): sum_i Y[i, a, j] Z[i, a, j]."""
        Y = _f64(Y)
        Zc = None if Z is None else _f64(Z)
        n, Dp, M = Y.shape
        if Zc is not None and Zc.shape != Y.shape:
            raise ValueError("debug_block_gram: Y and Z (n, Dp, M)")
        out = np.empty((M, Dp) if diag_only else (M, Dp, Dp))
        rc = self._lib.gpc_debug_block_gram(self._h, dtype, n, M, Dp, _ptr(Y), _ptr(Zc), int(bool(diag_only)), _ptr(out))
        self._check(rc, "gpc_debug_block_gram")
        return out

    @_serial
    def debug_hess_contract(self, kernel_id, degree, hyp_cov, X, x_star, alpha, Q=None, dtype=F64):
        """gpc_debug_hess_contract: the contraction kernel of gpc_predict_hess on the weights alpha (N,) and, optionally,
        a dense Q (N, M) stored in ``dtype``.  Returns (out_alpha, out_q), each (M, 1 + D (D + 1) / 2): column 0 =
        sum_i w F, column 1 + a (a + 1) / 2 + b = sum_i w G d_a d_b for a >= b; out_q is None without Q."""
        X, xs, hyp, al = _f64(X), _f64(x_star), _f64(hyp_cov), _f64(alpha).ravel()
        N, D = X.shape
        M = xs.shape[0]
        Qc = None if Q is None else _f64(Q)
        if xs.shape[1] != D or al.size != N or (Qc is not None and Qc.shape != (N, M)):
            raise ValueError("debug_hess_contract: X (N, D), x_star (M, D), alpha (N,), Q (N, M)")
        npl = 1 + D * (D + 1) // 2
        out_a = np.empty((M, npl))
        out_q = None if Qc is None else np.empty((M, npl))
        rc = self._lib.gpc_debug_hess_contract(self._h, kernel_id, degree, dtype, _ptr(hyp), _ptr(X), N, D, _ptr(xs), M,
                                               _ptr(al), _ptr(Qc), _ptr(out_a), _ptr(out_q))
        self._check(rc, "gpc_debug_hess_contract")
        return out_a, out_q

    @_serial
    def debug_hyp_cross(self, kernel_id, degree, hyp_cov, X, x_star, alpha, W, Q=None):
        """gpc_debug_hyp_cross: the fused cross pass of gpc_predict_hyp_grad on the weights alpha (N,), the weight
        vectors W (P, N), P >= cov_N, and, optionally, a dense Q (N, M); without Q the mean-only kernel runs.  Returns
        (B (M, P) = sum_i k W[p], A (M, cov_N) = sum_i d_c k alpha, C (M, cov_N) = sum_i d_c k Q | None); the log sf
        column holds k itself, not 2 k."""
        X, xs, hyp, al, Wc = _f64(X), _f64(x_star), _f64(hyp_cov), _f64(alpha).ravel(), _f64(W)
        N, D = X.shape
        M = xs.shape[0]
        Qc = None if Q is None else _f64(Q)
        if xs.shape[1] != D or al.size != N or Wc.ndim != 2 or Wc.shape[1] != N or (Qc is not None and Qc.shape != (N, M)):
            raise ValueError("debug_hyp_cross: X (N, D), x_star (M, D), alpha (N,), W (P, N), Q (N, M)")
        P = Wc.shape[0]
        cov_N = self._lib.gpc_cov_count(kernel_id, D)
        out = np.empty((M, P + cov_N * (1 if Qc is None else 2)))
        rc = self._lib.gpc_debug_hyp_cross(self._h, kernel_id, degree, _ptr(hyp), _ptr(X), N, D, _ptr(xs), M, _ptr(al),
                                           _ptr(Wc), P, _ptr(Qc), _ptr(out))
        self._check(rc, "gpc_debug_hyp_cross")
        return out[:, :P], out[:, P:P + cov_N], (None if Qc is None else out[:, P + cov_N:])

    @_serial
    def debug_nll_plane(self, kernel_id, degree, hyp_cov, X, p, alpha, Q=None):
        """gpc_debug_nll_plane: the plane kernel of gpc_nll_hess for covariance hyperparameter ``p`` with weights alpha
        (N,) and a dense symmetric Q (N, N) (None: zeros).  Returns (plane (N, N), u (N,), g (2,))."""
        X, hyp, al = _f64(X), _f64(hyp_cov), _f64(alpha).ravel()
        N, D = X.shape
        Qc = None if Q is None else _f64(Q)
        if al.size != N or (Qc is not None and Qc.shape != (N, N)):
            raise ValueError("debug_nll_plane: X (N, D), alpha (N,), Q (N, N)")
        plane, u, g = np.empty((N, N)), np.empty(N), np.empty(2)
        rc = self._lib.gpc_debug_nll_plane(self._h, kernel_id, degree, _ptr(hyp), _ptr(X), N, D, int(p), _ptr(al), _ptr(Qc),
                                           _ptr(plane), _ptr(u), _ptr(g))
        self._check(rc, "gpc_debug_nll_plane")
        return plane, u, g

    @_serial
    def debug_nll_d2(self, kernel_id, degree, hyp_cov, X, alpha, Q):
        """gpc_debug_nll_d2: the second-derivative contraction of gpc_nll_hess (ARD families) with weights
        Q - alpha alpha^T over the lower triangle.  Returns (D (D + 1) / 2,): entry a (a + 1) / 2 + b, a >= b."""
        X, hyp, al, Qc = _f64(X), _f64(hyp_cov), _f64(alpha).ravel(), _f64(Q)
        N, D = X.shape
        if al.size != N or Qc.shape != (N, N):
            raise ValueError("debug_nll_d2: X (N, D), alpha (N,), Q (N, N)")
        out = np.empty(D * (D + 1) // 2)
        rc = self._lib.gpc_debug_nll_d2(self._h, kernel_id, degree, _ptr(hyp), _ptr(X), N, D, _ptr(al), _ptr(Qc), _ptr(out))
        self._check(rc, "gpc_debug_nll_d2")
        return out

    @_serial
    def debug_nll_gram(self, planes, out=None):
        """gpc_debug_nll_gram: the Gram pass of gpc_nll_hess on planes (P, npad, npad).  Returns (or fills ``out``, a
        C-contiguous view of P (P + 1) / 2 doubles) entry p (p + 1) / 2 + q = sum_ab planes[p][a][b] planes[q][b][a]."""
        pl = _f64(planes)
        P, npad, n2 = pl.shape
        if npad != n2:
            raise ValueError("debug_nll_gram: planes (P, npad, npad)")
        if out is None:
            out = np.empty(P * (P + 1) // 2)
        if out.dtype != np.float64 or out.size != P * (P + 1) // 2:
            raise ValueError("debug_nll_gram: out holds P (P + 1) / 2 doubles")
        rc = self._lib.gpc_debug_nll_gram(self._h, npad, P, _ptr(pl), _ptr(out))
        self._check(rc, "gpc_debug_nll_gram")
        return out

    @_serial
    def debug_cv_trace(self, kernel_id, degree, hyp_cov, X, M, alpha, beta):
        """gpc_debug_cv_trace: the contraction of gpc_cv_grad alone, with the weight
        G = M - (beta alpha^T + alpha beta^T) / 2 over the lower triangle (M (N, N) is read from its lower triangle).
        Returns (gsum (cov_N,) = <d_p K, G>, diagG (N,))."""
        X, hyp, Mc, al, be = _f64(X), _f64(hyp_cov), _f64(M), _f64(alpha).ravel(), _f64(beta).ravel()
        N, D = X.shape
        if al.size != N or be.size != N or Mc.shape != (N, N):
            raise ValueError("debug_cv_trace: X (N, D), M (N, N), alpha (N,), beta (N,)")
        gsum, dg = np.empty(self._lib.gpc_cov_count(kernel_id, D)), np.empty(N)
        rc = self._lib.gpc_debug_cv_trace(self._h, kernel_id, degree, _ptr(hyp), _ptr(X), N, D, _ptr(Mc), _ptr(al), _ptr(be),
                                          _ptr(gsum), _ptr(dg))
        self._check(rc, "gpc_debug_cv_trace")
        return gsum, dg

    @_serial
    def debug_cv_weights(self, loss, alpha, q, weights=None):
        """gpc_debug_cv_weights: the per-point kernel of gpc_cv_grad; ``loss`` 0 = lpd, 1 = mse.  Returns (c (N,), b (N,))."""
        al, qc = _f64(alpha).ravel(), _f64(q).ravel()
        wc = None if weights is None else _f64(weights).ravel()
        N = al.size
        if qc.size != N or (wc is not None and wc.size != N):
            raise ValueError("debug_cv_weights: alpha (N,), q (N,), weights (N,) | None")
        cw, b = np.empty(N), np.empty(N)
        rc = self._lib.gpc_debug_cv_weights(self._h, N, int(loss), _ptr(al), _ptr(qc), _ptr(wc), _ptr(cw), _ptr(b))
        self._check(rc, "gpc_debug_cv_weights")
        return cw, b

    @_serial
    def debug_normals(self, seed, stream, s, r, j0, count):
        """gpc_debug_normals: the device's z of rows j0 .. j0 + count - 1 of (seed, stream, sample s, draw r)."""
        out = np.empty(count)
        rc = self._lib.gpc_debug_normals(self._h, int(seed), stream, s, r, j0, count, _ptr(out))
        self._check(rc, "gpc_debug_normals")
        return out


class PostHandle:
    """Device-resident posteriors of one hyperparameter batch (gpc_post)."""

    def __init__(self, ctx: Context, h, S: int, N: int):
        self.ctx, self._h, self.S, self.N = ctx, h, S, N

    @_serial
    def fetch(self, s, alpha=True, sW=True, L=True):
        N = self.N
        a = np.empty(N) if alpha else None
        w = np.empty(N) if sW else None
        Lm = np.empty((N, N)) if L else None
        rc = self.ctx._lib.gpc_post_fetch(self._h, int(s), _ptr(a), _ptr(w), _ptr(Lm))
        self.ctx._check(rc, "gpc_post_fetch")
        return a, w, Lm

    @_serial
    def predict(self, x_star):
        xs = _f64(x_star)
        M = xs.shape[0]
        fmu = np.empty((M, self.S))
        fs2 = np.empty((M, self.S))
        rc = self.ctx._lib.gpc_predict(self._h, _ptr(xs), M, _ptr(fmu), _ptr(fs2))
        self.ctx._check(rc, "gpc_predict")
        return fmu, fs2

    @_serial
    def predict_gobs(self, x_star):
        """gpc_predict_gobs: fmu, fs2 (M, S) of a gradient-observation posterior (``Context.posterior_batch_gobs``)."""
        xs = _f64(x_star)
        M = xs.shape[0]
        fmu = np.empty((M, self.S))
        fs2 = np.empty((M, self.S))
        rc = self.ctx._lib.gpc_predict_gobs(self._h, _ptr(xs), M, _ptr(fmu), _ptr(fs2))
        self.ctx._check(rc, "gpc_predict_gobs")
        return fmu, fs2

    @_serial
    def predict_grad(self, x_star):
        """gpc_predict_grad: fmu, fs2 (M, S) as predict, and their gradients with respect to x_star, dfmu and dfs2
        (M, D, S).  x_star has the D columns of the training inputs."""
        xs = _f64(x_star)
        M, D = xs.shape
        fmu = np.empty((M, self.S))
        fs2 = np.empty((M, self.S))
        dfmu = np.empty((M, D, self.S))
        dfs2 = np.empty((M, D, self.S))
        rc = self.ctx._lib.gpc_predict_grad(self._h, _ptr(xs), M, _ptr(fmu), _ptr(fs2), _ptr(dfmu), _ptr(dfs2))
        self.ctx._check(rc, "gpc_predict_grad")
        return fmu, fs2, dfmu, dfs2

    @_serial
    def grad_post(self, x_star, diag_only=False):
        """gpc_grad_post: the joint posterior of (f, grad f) at x_star (M, D) per sample.  Returns fmu (M, S), dfmu
        (M, D, S) and cov (M, D + 1, D + 1, S) -- slot 0 = f, slot 1 + l = d/dx_l -- or, with ``diag_only``, its diagonal
        (M, D + 1, S).  No clamp, no noise, no mean function."""
        xs = _f64(x_star)
        M, D = xs.shape
        fmu = np.empty((M, self.S))
        dfmu = np.empty((M, D, self.S))
        cov = np.empty((M, D + 1, self.S) if diag_only else (M, D + 1, D + 1, self.S))
        rc = self.ctx._lib.gpc_grad_post(self._h, _ptr(xs), M, int(bool(diag_only)), _ptr(fmu), _ptr(dfmu), _ptr(cov))
        self.ctx._check(rc, "gpc_grad_post")
        return fmu, dfmu, cov

    @_serial
    def grad_post_gobs(self, x_star, diag_only=False):
        """gpc_grad_post_gobs: ``grad_post`` for a gradient-observation posterior (``Context.posterior_batch_gobs``):
        fmu (M, S), dfmu (M, D, S) and cov (M, D + 1, D + 1, S), or (M, D + 1, S) with ``diag_only``."""
        xs = _f64(x_star)
        M, D = xs.shape
        fmu = np.empty((M, self.S))
        dfmu = np.empty((M, D, self.S))
        cov = np.empty((M, D + 1, self.S) if diag_only else (M, D + 1, D + 1, self.S))
        rc = self.ctx._lib.gpc_grad_post_gobs(self._h, _ptr(xs), M, int(bool(diag_only)), _ptr(fmu), _ptr(dfmu), _ptr(cov))
        self.ctx._check(rc, "gpc_grad_post_gobs")
        return fmu, dfmu, cov

    @_serial
    def predict_hess(self, x_star, compute_var=True):
        """gpc_predict_hess: fmu, fs2 (M, S), dfmu, dfs2 (M, D, S) as predict_grad, and the Hessians hmu, hs2
        (M, D, D, S) of the mean and the variance with respect to x_star, symmetric to the bit.  Without
        ``compute_var`` the three variance entries are None and no product is launched."""
        xs = _f64(x_star)
        M, D = xs.shape
        S = self.S
        fmu, dfmu, hmu = np.empty((M, S)), np.empty((M, D, S)), np.empty((M, D, D, S))
        fs2 = np.empty((M, S)) if compute_var else None
        dfs2 = np.empty((M, D, S)) if compute_var else None
        hs2 = np.empty((M, D, D, S)) if compute_var else None
        rc = self.ctx._lib.gpc_predict_hess(self._h, _ptr(xs), M, int(bool(compute_var)), _ptr(fmu), _ptr(fs2), _ptr(dfmu),
                                            _ptr(dfs2), _ptr(hmu), _ptr(hs2))
        self.ctx._check(rc, "gpc_predict_hess")
        return fmu, fs2, dfmu, dfs2, hmu, hs2

    @_serial
    def nll_hess(self, cov_N, dm=None, dsn2=None):
        """gpc_nll_hess: ``cov_N`` covariance hyperparameters (gpc_cov_count of the posterior's kernel); dm (S, N, mean_N) | None, dsn2 (S, 1 | N, noise_N) | None (without the jitter multiplier).
        Returns H (S, P, P) without the plugins' second-derivative terms, dnlz (S, P), alpha (S, N) and
        diagq = diag(Q - alpha alpha^T) (S, N)."""
        S, N = self.S, self.N
        dm_c = None if dm is None or dm.shape[2] == 0 else _f64(dm)
        ds_c = None if dsn2 is None or dsn2.shape[2] == 0 else _f64(dsn2)
        mean_N = 0 if dm_c is None else dm_c.shape[2]
        noise_N = 0 if ds_c is None else ds_c.shape[2]
        rows = 1 if ds_c is None else ds_c.shape[1]
        if (dm_c is not None and dm_c.shape[:2] != (S, N)) or (ds_c is not None and (ds_c.shape[0] != S or rows not in (1, N))):
            raise ValueError("nll_hess: dm (S, N, mean_N); dsn2 (S, 1 or N, noise_N)")
        P = int(cov_N) + noise_N + mean_N
        H, g, al, dq = np.empty((S, P, P)), np.empty((S, P)), np.empty((S, N)), np.empty((S, N))
        rc = self.ctx._lib.gpc_nll_hess(self._h, _ptr(dm_c), mean_N, _ptr(ds_c), rows, noise_N, _ptr(H), _ptr(g), _ptr(al),
                                        _ptr(dq))
        self.ctx._check(rc, "gpc_nll_hess")
        return H, g, al, dq

    @_serial
    def cv_grad(self, cov_N, loss="lpd", weights=None):
        """gpc_cv_grad: ``cov_N`` covariance hyperparameters (gpc_cov_count of the posterior's kernel); ``loss`` "lpd" or
        "mse"; weights (N,) | None.  Returns the six arrays gsum (S, cov_N) = <d_p K, G>, diagG (S, N) = diag(G), beta,
        alpha, q = diag(Q) and c (S, N each) of the leave-one-out objective (``_cvgrad`` has the formulas)."""
        S, N = self.S, self.N
        if loss not in CV_LOSSES:
            raise ValueError(f"cv_grad: loss must be one of {sorted(CV_LOSSES)}, got {loss!r}")
        wc = None if weights is None else _f64(weights).ravel()
        if wc is not None and wc.size != N:
            raise ValueError("cv_grad: weights (N,)")
        gsum = np.empty((S, int(cov_N)))
        dg, be, al, q, cw = (np.empty((S, N)) for _ in range(5))
        rc = self.ctx._lib.gpc_cv_grad(self._h, CV_LOSSES[loss], _ptr(wc), _ptr(gsum), _ptr(dg), _ptr(be), _ptr(al),
                                       _ptr(q), _ptr(cw))
        self.ctx._check(rc, "gpc_cv_grad")
        return gsum, dg, be, al, q, cw

    @_serial
    def predict_hyp_grad(self, x_star, cov_N, sn2, dsn2=None, dm=None, compute_var=True):
        """gpc_predict_hyp_grad: ``cov_N`` covariance hyperparameters (gpc_cov_count of the posterior's kernel); sn2 (S, 1 | N), dsn2 (S, 1 | N, noise_N) | None (both without the jitter multiplier),
        dm (S, N, mean_N) | None.  Returns fmu, fs2 (M, S) and dfmu, dfs2 (M, P, S), P = cov_N + noise_N + mean_N, the
        latent prediction (no mean function, unclamped) and its derivatives.  Without ``compute_var`` fs2 and dfs2 are
        None and no product is launched."""
        xs = _f64(x_star)
        M = xs.shape[0]
        S, N = self.S, self.N
        sn2_c = _f64(sn2).reshape(S, -1)
        rows = sn2_c.shape[1]
        dm_c = None if dm is None or dm.shape[2] == 0 else _f64(dm)
        ds_c = None if dsn2 is None or dsn2.shape[2] == 0 else _f64(dsn2)
        mean_N = 0 if dm_c is None else dm_c.shape[2]
        noise_N = 0 if ds_c is None else ds_c.shape[2]
        if rows not in (1, N) or (dm_c is not None and dm_c.shape[:2] != (S, N)) or \
                (ds_c is not None and ds_c.shape[:2] != (S, rows)):
            raise ValueError("predict_hyp_grad: sn2 (S, 1 or N); dsn2 (S, 1 or N, noise_N) with sn2's rows; dm (S, N, mean_N)")
        P = int(cov_N) + noise_N + mean_N
        fmu, dfmu = np.empty((M, S)), np.empty((M, P, S))
        fs2 = np.empty((M, S)) if compute_var else None
        dfs2 = np.empty((M, P, S)) if compute_var else None
        rc = self.ctx._lib.gpc_predict_hyp_grad(self._h, _ptr(xs), M, int(bool(compute_var)), _ptr(sn2_c), _ptr(ds_c), rows,
                                                noise_N, _ptr(dm_c), mean_N, _ptr(fmu), _ptr(fs2), _ptr(dfmu), _ptr(dfs2))
        self.ctx._check(rc, "gpc_predict_hyp_grad")
        return fmu, fs2, dfmu, dfs2

    @_serial
    def predict_K(self, Ks, Kss=None, want_var=True):
        """gpc_predict_K: Ks (S,N,M) caller-provided cross covariances; returns fmu (M,S), the
        variance term fq (M,S; add kss) and, with Kss (S,M,M), the full covariances (S,M,M)."""
        Ks = _f64(Ks)
        M = Ks.shape[2]
        fmu = np.empty((M, self.S))
        fq = np.empty((M, self.S)) if want_var else None
        Kss_c = None if Kss is None else _f64(Kss)
        cov = None if Kss is None else np.empty((self.S, M, M))
        rc = self.ctx._lib.gpc_predict_K(self._h, M, _ptr(Ks), _ptr(Kss_c), _ptr(fmu), _ptr(fq), _ptr(cov))
        self.ctx._check(rc, "gpc_predict_K")
        return fmu, fq, cov

    @_serial
    def append(self, m_star, sn2_star, y_new):
        """Rank-one append of the point already added to the context's data.  Returns the
        per-sample outcome (bool array): False entries must be recomputed (``recompute``)."""
        m_star, sn2_star = _f64(m_star).ravel(), _f64(sn2_star).ravel()
        ok = np.zeros(self.S, dtype=np.int32)
        rc = self.ctx._lib.gpc_post_append(self._h, _ptr(m_star), _ptr(sn2_star), float(y_new),
                                           ok.ctypes.data)
        self.ctx._check(rc, "gpc_post_append")
        self.N += 1
        return ok.astype(bool)

    @_serial
    def append_K(self, Ks, kss, m_star, sn2_star, y_new):
        """``append`` for posteriors built from a caller's covariance object: Ks (S, n) = k_s(X_old, x_new),
        kss (S,) = k_s(x_new, x_new)."""
        Ks, kss = _f64(Ks), _f64(kss).ravel()
        m_star, sn2_star = _f64(m_star).ravel(), _f64(sn2_star).ravel()
        if Ks.shape != (self.S, self.N) or kss.shape != (self.S,):
            raise ValueError("Ks must be (S, n) and kss (S,)")
        ok = np.zeros(self.S, dtype=np.int32)
        rc = self.ctx._lib.gpc_post_append_K(self._h, _ptr(Ks), _ptr(kss), _ptr(m_star), _ptr(sn2_star),
                                             float(y_new), ok.ctypes.data)
        self.ctx._check(rc, "gpc_post_append_K")
        self.N += 1
        return ok.astype(bool)

    @_serial
    def append_block(self, m_star, sn2_star, y_new):
        """Block append of the k points already added to the context's data (gpc_post_append_block): m_star (S, k),
        sn2_star (S,), y_new (k,).  Returns the per-sample outcome (bool array): False entries were left stale and
        must be recomputed (``recompute``)."""
        y_new = _f64(y_new).ravel()
        k = y_new.size
        m_star, sn2_star = _f64(m_star).ravel(), _f64(sn2_star).ravel()
        if m_star.size != self.S * k or sn2_star.shape != (self.S,):
            raise ValueError("m_star must be (S, k) and sn2_star (S,)")
        ok = np.zeros(self.S, dtype=np.int32)
        rc = self.ctx._lib.gpc_post_append_block(self._h, k, _ptr(m_star), _ptr(sn2_star), _ptr(y_new),
                                                 ok.ctypes.data)
        self.ctx._check(rc, "gpc_post_append_block")
        self.N += k
        return ok.astype(bool)

    @_serial
    def append_block_K(self, Ks, Kss, m_star, sn2_star, y_new):
        """``append_block`` for posteriors built from a caller's covariance object: Ks (S, n, k) = k_s(X_old, X_new),
        Kss (S, k, k) = k_s(X_new, X_new)."""
        y_new = _f64(y_new).ravel()
        k = y_new.size
        Ks, Kss = _f64(Ks), _f64(Kss)
        m_star, sn2_star = _f64(m_star).ravel(), _f64(sn2_star).ravel()
        if (Ks.shape != (self.S, self.N, k) or Kss.shape != (self.S, k, k) or m_star.size != self.S * k
                or sn2_star.shape != (self.S,)):
            raise ValueError("Ks must be (S, n, k), Kss (S, k, k), m_star (S, k) and sn2_star (S,)")
        ok = np.zeros(self.S, dtype=np.int32)
        rc = self.ctx._lib.gpc_post_append_block_K(self._h, k, _ptr(Ks), _ptr(Kss), _ptr(m_star), _ptr(sn2_star),
                                                   _ptr(y_new), ok.ctypes.data)
        self.ctx._check(rc, "gpc_post_append_block_K")
        self.N += k
        return ok.astype(bool)

    @_serial
    def remove(self, idx, ym):
        """Removal of the rows ``idx`` (sorted, distinct; numbered in the posterior's N rows) that have already left the
        context's data (gpc_post_remove): ym (S, N - k) = y - m_s(X) on the kept rows.  Returns the per-sample outcome
        (bool array): False entries were left stale in the compacted storage and must be recomputed (``recompute``)."""
        idx = np.ascontiguousarray(idx, dtype=np.int32).ravel()
        k = idx.size
        ym = _f64(ym)
        if ym.shape != (self.S, self.N - k):
            raise ValueError("ym must be (S, N - k)")
        ok = np.zeros(self.S, dtype=np.int32)
        rc = self.ctx._lib.gpc_post_remove(self._h, k, idx.ctypes.data, _ptr(ym), ok.ctypes.data)
        self.ctx._check(rc, "gpc_post_remove")
        self.N -= k
        return ok.astype(bool)

    @_serial
    def recompute(self, idx, hyp_cov, m, sn2, sn2_is_vector, K=None):
        """Full recompute of the listed samples in place (the reference's ``full_updates``).  ``K`` (cnt, N, N):
        the caller's covariance matrices on the extended data (posteriors built from a covariance object)."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        m, sn2 = _f64(m), _f64(sn2)
        cnt = idx.size
        mult = np.empty(cnt)
        lchol = np.empty(cnt, dtype=np.int32)
        info = np.empty(cnt, dtype=np.int32)
        if K is not None:
            K = _f64(K)
            rc = self.ctx._lib.gpc_post_recompute_K(
                self._h, cnt, idx.ctypes.data, _ptr(K), _ptr(m), _ptr(sn2),
                1 if sn2_is_vector else 0, _ptr(mult), lchol.ctypes.data, info.ctypes.data)
            self.ctx._check(rc, "gpc_post_recompute_K")
            return mult, lchol.astype(bool), info
        hyp_cov = _f64(hyp_cov)
        rc = self.ctx._lib.gpc_post_recompute(
            self._h, cnt, idx.ctypes.data, _ptr(hyp_cov), _ptr(m), _ptr(sn2),
            1 if sn2_is_vector else 0, _ptr(mult), lchol.ctypes.data, info.ctypes.data)
        self.ctx._check(rc, "gpc_post_recompute")
        return mult, lchol.astype(bool), info

    @_serial
    def predict_full(self, x_star):
        xs = _f64(x_star)
        M = xs.shape[0]
        fmu = np.empty((M, self.S))
        cov = np.empty((self.S, M, M))
        rc = self.ctx._lib.gpc_predict_full(self._h, _ptr(xs), M, _ptr(fmu), _ptr(cov))
        self.ctx._check(rc, "gpc_predict_full")
        return fmu, cov

    @_serial
    def predict_cov(self, x_a, x_b, weights=None, want_cov=True, want_fs2=False):
        """gpc_predict_cov: (cov, wsq, fs2b).  cov (S, Ma, Mb) is the posterior covariance between the rows of x_a and
        of x_b (None without ``want_cov``); wsq (Mb, S) = sum_i w_i cov[s, i, j]^2 for ``weights`` (Ma,) or (Ma, S)
        (None without weights); fs2b (Mb, S) is ``predict``'s variance of x_b (None without ``want_fs2``)."""
        xa, xb = _f64(x_a), _f64(x_b)
        Ma, Mb = xa.shape[0], xb.shape[0]
        w = None if weights is None else _f64(weights)
        if w is not None and w.shape not in ((Ma,), (Ma, self.S)):
            raise ValueError(f"predict_cov: weights must be ({Ma},) or ({Ma}, {self.S}), got {w.shape}")
        if w is None and not want_cov:
            raise ValueError("predict_cov: nothing to compute (neither the covariance nor a weighted reduction)")
        cov = np.empty((self.S, Ma, Mb)) if want_cov else None
        wsq = np.empty((Mb, self.S)) if w is not None else None
        fs2b = np.empty((Mb, self.S)) if want_fs2 else None
        rc = self.ctx._lib.gpc_predict_cov(self._h, _ptr(xa), Ma, _ptr(xb), Mb, _ptr(w),
                                           1 if (w is not None and w.ndim == 2) else 0, _ptr(fs2b), _ptr(cov), _ptr(wsq))
        self.ctx._check(rc, "gpc_predict_cov")
        return cov, wsq, fs2b

    @_serial
    def lookahead_batch(self, x_ref, x_cand, q, weights, noise):
        """gpc_lookahead_batch: (idx (q,), gain (q, S)) of q greedy look-ahead steps.  ``weights`` (Mr,) or (Mr, S);
        ``noise`` (Mc, S) is the predictive noise of every candidate under every sample."""
        xr, xc = _f64(x_ref), _f64(x_cand)
        Mr, Mc = xr.shape[0], xc.shape[0]
        w, nz = _f64(weights), _f64(noise)
        if w.shape not in ((Mr,), (Mr, self.S)):
            raise ValueError(f"lookahead_batch: weights must be ({Mr},) or ({Mr}, {self.S}), got {w.shape}")
        if nz.shape != (Mc, self.S):
            raise ValueError(f"lookahead_batch: noise must be ({Mc}, {self.S}), got {nz.shape}")
        q = int(q)
        idx = np.empty(max(q, 0), dtype=np.int32)
        gain = np.empty((max(q, 0), self.S))
        rc = self.ctx._lib.gpc_lookahead_batch(self._h, _ptr(xr), Mr, _ptr(xc), Mc, _ptr(w), 1 if w.ndim == 2 else 0,
                                               _ptr(nz), q, idx.ctypes.data, _ptr(gain))
        self.ctx._check(rc, "gpc_lookahead_batch")
        return idx.astype(np.int64), gain

    @_serial
    def draw(self, x_star, n_draws, seed, s_offset=0, noise_sd=None):
        """gpc_draw: f (M, n_draws, S) = fmu + L z (+ noise_sd z'), without the mean function, and the jitter tau (S,)
        each sample needed.  s_offset is the global index of this posterior's first sample (the random stream's key);
        noise_sd (M, S) or None.  A sample that cannot be factored raises numpy.linalg.LinAlgError."""
        xs = _f64(x_star)
        M = xs.shape[0]
        f = np.empty((M, n_draws, self.S))
        tau = np.empty(self.S)
        nsd = None if noise_sd is None else _f64(noise_sd)
        rc = self.ctx._lib.gpc_draw(self._h, _ptr(xs), M, n_draws, int(seed), s_offset, _ptr(nsd), _ptr(f), _ptr(tau))
        if rc == -3:
            raise np.linalg.LinAlgError(self.ctx._lib.gpc_last_error(self.ctx._h).decode())
        self.ctx._check(rc, "gpc_draw")
        return f, tau

    @_serial
    def paths(self, n_paths, n_features, seed, s_offset, ym, noise_sd):
        """gpc_paths_create: a ``Paths`` handle of ``n_paths`` pathwise samples per posterior sample.  ym (S, N) =
        y - m_s(X), noise_sd (N, S) = sqrt(sn2 sn2_mult); s_offset is the global index of this posterior's first sample."""
        ym, nsd = _f64(ym), _f64(noise_sd)
        if ym.shape != (self.S, self.N) or nsd.shape != (self.N, self.S):
            raise ValueError(f"paths: ym must be (S, N) = {(self.S, self.N)} and noise_sd (N, S), got {ym.shape} and "
                             f"{nsd.shape}")
        h = _vp()
        rc = self.ctx._lib.gpc_paths_create(self._h, int(n_paths), int(n_features), int(seed), int(s_offset), _ptr(ym),
                                            _ptr(nsd), C.byref(h))
        self.ctx._check(rc, "gpc_paths_create")
        return Paths(self.ctx, h, self.S, self.N, self.ctx.D, int(n_paths), int(n_features))

    @_serial
    def quad(self, mu, sigma, compute_var):
        mu, sigma = _f64(mu), _f64(sigma)
        M = mu.shape[0]
        za = np.empty((M, self.S))
        zkz = np.empty((M, self.S)) if compute_var else None
        rc = self.ctx._lib.gpc_quad(self._h, _ptr(mu), _ptr(sigma), M, 1 if compute_var else 0, _ptr(za), _ptr(zkz))
        self.ctx._check(rc, "gpc_quad")
        return za, zkz

    @_serial
    def quad_grad(self, mu, sigma, compute_var):
        """gpc_quad_grad: za, zkz (M, S) as quad, and the gradients of each with respect to mu and sigma (M, D, S):
        (za, zkz, dza_dmu, dza_dsigma, dzkz_dmu, dzkz_dsigma); the zkz entries are None without compute_var."""
        mu, sigma = _f64(mu), _f64(sigma)
        if mu.ndim != 2 or sigma.shape != mu.shape:
            raise ValueError(f"quad_grad: mu and sigma must both be (M, D), got {mu.shape} and {sigma.shape}")
        M, D = mu.shape
        za = np.empty((M, self.S))
        dza = np.empty((M, D, self.S)), np.empty((M, D, self.S))
        zkz = np.empty((M, self.S)) if compute_var else None
        dzkz = (np.empty((M, D, self.S)), np.empty((M, D, self.S))) if compute_var else (None, None)
        rc = self.ctx._lib.gpc_quad_grad(self._h, _ptr(mu), _ptr(sigma), M, 1 if compute_var else 0, _ptr(za),
                                         _ptr(zkz), _ptr(dza[0]), _ptr(dza[1]), _ptr(dzkz[0]), _ptr(dzkz[1]))
        self.ctx._check(rc, "gpc_quad_grad")
        return za, zkz, dza[0], dza[1], dzkz[0], dzkz[1]

    @_serial
    def quad_cov(self, mu, sigma):
        """gpc_quad_cov: za (M, S) as quad, and cov (S, M, M) = Gamma_s - Z^T (K + Sigma)^-1 Z, neither symmetrised nor
        clamped."""
        mu, sigma = _f64(mu), _f64(sigma)
        if mu.ndim != 2 or sigma.shape != mu.shape:
            raise ValueError(f"quad_cov: mu and sigma must both be (M, D), got {mu.shape} and {sigma.shape}")
        M = mu.shape[0]
        za = np.empty((M, self.S))
        cov = np.empty((self.S, M, M))
        rc = self.ctx._lib.gpc_quad_cov(self._h, _ptr(mu), _ptr(sigma), M, _ptr(za), _ptr(cov))
        self.ctx._check(rc, "gpc_quad_cov")
        return za, cov

    @_serial
    def quad_mix(self, mu, sigma, w, compute_var, compute_grad):
        """gpc_quad_mix, the device's share of GP.quad_mixture as a dict: za (M, S); with compute_var zbkzb (S,), gw and
        zq (M, S); with compute_grad dza_dmu, dza_dsigma (M, D, S); with both dzq_dmu, dzq_dsigma, dgw_dmu, dgw_dsigma
        (M, D, S).  What a flag does not ask for is None."""
        mu, sigma, w = _f64(mu), _f64(sigma), _f64(w)
        if mu.ndim != 2 or sigma.shape != mu.shape or w.shape != (mu.shape[0],):
            raise ValueError(f"quad_mix: mu and sigma must both be (M, D) and w (M,), got {mu.shape}, {sigma.shape} "
                             f"and {w.shape}")
        M, D = mu.shape
        S = self.S
        row = lambda on: np.empty((M, S)) if on else None
        plane = lambda on: np.empty((M, D, S)) if on else None
        both = compute_var and compute_grad
        r = dict(za=row(True), zbkzb=np.empty(S) if compute_var else None, gw=row(compute_var), zq=row(compute_var),
                 dza_dmu=plane(compute_grad), dza_dsigma=plane(compute_grad), dzq_dmu=plane(both),
                 dzq_dsigma=plane(both), dgw_dmu=plane(both), dgw_dsigma=plane(both))
        rc = self.ctx._lib.gpc_quad_mix(self._h, _ptr(mu), _ptr(sigma), _ptr(w), M, 1 if compute_var else 0,
                                        1 if compute_grad else 0, *[_ptr(v) for v in r.values()])
        self.ctx._check(rc, "gpc_quad_mix")
        return r

    @_serial
    def cv(self, folds=None):
        """gpc_cv: leave-fold-out predictions from the resident posterior.  ``folds``: None (leave-one-out) or a
        sequence of index arrays, each strictly ascending, pairwise disjoint.  Returns (dmu, s2, quad, logdet, info):
        dmu and s2 (N, S), NaN at points in no fold; quad, logdet and info (F, S), or (N, S) for leave-one-out."""
        N, S = self.N, self.S
        dmu, s2 = np.empty((N, S)), np.empty((N, S))
        if folds is None:
            F, ptr, idx = 0, None, None
        else:
            F = len(folds)
            if F == 0:
                raise ValueError("cv: folds must not be an empty sequence")
            ptr = np.zeros(F + 1, dtype=np.int32)
            ptr[1:] = np.cumsum([len(f) for f in folds])
            idx = np.ascontiguousarray(np.concatenate([np.asarray(f).ravel() for f in folds]), dtype=np.int32)
        n_out = F if F else N
        quad, logdet = np.empty((n_out, S)), np.empty((n_out, S))
        info = np.empty((n_out, S), dtype=np.int32)
        rc = self.ctx._lib.gpc_cv(self._h, F, _ptr(ptr), _ptr(idx), _ptr(dmu), _ptr(s2), _ptr(quad), _ptr(logdet),
                                  _ptr(info))
        self.ctx._check(rc, "gpc_cv")
        return dmu, s2, quad, logdet, info

    @_serial
    def free(self):
        if self._h:
            self.ctx._lib.gpc_post_free(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            if self.ctx._h:
                self.free()
        except Exception:
            pass


class Paths:
    """Pathwise posterior samples of one posterior set (gpc_paths): owns its device copies, outlives the PostHandle."""

    def __init__(self, ctx: Context, h, S: int, N: int, D: int, R: int, F: int):
        self.ctx, self._h, self.S, self.N, self.D, self.R, self.F = ctx, h, S, N, D, R, F

    @_serial
    def eval(self, x_star, compute_grad=False):
        """gpc_paths_eval: f (M, R, S) and, with the gradient, df (M, D, R, S), without the mean function."""
        if not self._h:
            raise ValueError("paths: the handle has been closed")
        xs = _f64(x_star)
        if xs.ndim != 2 or xs.shape[1] != self.D:
            raise ValueError(f"paths: x_star must be (M, {self.D}), got {xs.shape}")
        M = xs.shape[0]
        f = np.empty((M, self.R, self.S))
        df = np.empty((M, self.D, self.R, self.S)) if compute_grad else None
        rc = self.ctx._lib.gpc_paths_eval(self._h, _ptr(xs), M, _ptr(f), _ptr(df))
        self.ctx._check(rc, "gpc_paths_eval")
        return (f, df) if compute_grad else f

    @_serial
    def fetch(self, s):
        """gpc_debug_paths_fetch: (theta (F, D), b (F,), wt (F, R), v (N, R)) of sample ``s`` (tests)."""
        theta, b = np.empty((self.F, self.D)), np.empty(self.F)
        wt, v = np.empty((self.F, self.R)), np.empty((self.N, self.R))
        rc = self.ctx._lib.gpc_debug_paths_fetch(self._h, int(s), _ptr(theta), _ptr(b), _ptr(wt), _ptr(v))
        self.ctx._check(rc, "gpc_debug_paths_fetch")
        return theta, b, wt, v

    @_serial
    def free(self):
        if self._h:
            self.ctx._lib.gpc_paths_free(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            if self.ctx._h:
                self.free()
        except Exception:
            pass


def gemm_queues(ntiles, batch, flags, tiles_m=0, tiles_n=0, klo=0, khi=0, lower_only=0, want_tiles=False,
                want_xcd=False):
    """gpc_debug_gemm_queues (no device needed): (queues, totals, tiles, xcd).  queues: per tile queue of a persistent
    launch the (tile, sample) pairs it hands out, in order (8 entries; the flat queue of a launch without flag 8 is
    entry 0); totals: the 8 queue lengths as the kernel computes them; tiles: (ntiles, 2) array of the (ti, tj) of every position of the dispatch order, or None; xcd: (batch, ntiles, 2)
    array of the item (bx, by) workgroup (bx, by) of a plain launch takes, or None."""
    lib = load()
    n = int(ntiles) * int(batch)
    q_total = np.zeros(8, dtype=np.int32)
    q_items = np.full((max(n, 1), 2), -1, dtype=np.int32)
    tiles = np.full((ntiles, 2), -1, dtype=np.int32) if want_tiles else None
    xcd = np.full((batch, ntiles, 2), -1, dtype=np.int32) if want_xcd else None
    rc = lib.gpc_debug_gemm_queues(int(ntiles), int(batch), int(flags), int(tiles_m), int(tiles_n), int(klo), int(khi),
                                   int(bool(lower_only)), q_total.ctypes.data, q_items.ctypes.data, _ptr(tiles),
                                   _ptr(xcd))
    if rc != 0:
        raise RuntimeError(f"gpc_debug_gemm_queues failed (rc={rc})")
    ends = np.concatenate([[0], np.cumsum(np.minimum(q_total, n))])
    queues = [q_items[ends[q]:ends[q + 1]].copy() for q in range(8)]
    return queues, q_total, tiles, xcd


# GemmArgs::tri of gemm.h, and where gpc_debug_gemm_form's flags carry it
TRI_A_FIRST, TRI_A_LAST, TRI_B_FIRST, TRI_B_LAST, TRI_DIAG_LOWER = 1, 2, 3, 4, 8
TRI_FLAGS_SHIFT = 8


def tri_masks(tri, diag_tile, slab):
    """gpc_debug_tri_masks (no device needed): (frag_rows (4, 4), frag_cols (4, 4), issued (4, 4, 4), stored (4, 4, 4)) of
    the zero-skipping GEMM instantiation ``tri`` in k-slab ``slab`` of the triangular block, per wave 2 wr + wc."""
    lib = load()
    rows, cols = np.zeros((4, 4), dtype=np.int32), np.zeros((4, 4), dtype=np.int32)
    issued, stored = np.zeros((4, 4, 4), dtype=np.int32), np.zeros((4, 4, 4), dtype=np.int32)
    rc = lib.gpc_debug_tri_masks(int(tri), int(bool(diag_tile)), int(slab), rows.ctypes.data, cols.ctypes.data,
                                 issued.ctypes.data, stored.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"gpc_debug_tri_masks failed (rc={rc})")
    return rows, cols, issued, stored


def tri_usable(tri, a_kmajor, b_kmajor, klo, khi, lower_only, M, N, K, tile=128, dtype=F64):
    """gpc_debug_tri_usable (no device needed): the zero-skipping instantiation the launcher picks (0: the plain kernel)."""
    rc = load().gpc_debug_tri_usable(int(dtype), int(tile), int(bool(a_kmajor)), int(bool(b_kmajor)), int(klo), int(khi),
                                     int(bool(lower_only)), int(M), int(N), int(K), int(tri))
    if rc < 0:
        raise RuntimeError(f"gpc_debug_tri_usable failed (rc={rc})")
    return rc


_contexts = {}


def default_device() -> int:
    return int(os.environ.get("GPYREG_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def context(device: int | None = None) -> Context:
    """Process-wide context of a device (created on first use)."""
    dev = default_device() if device is None else int(device)
    with _lock:
        ctx = _contexts.get(dev)
        if ctx is None or ctx._h is None:
            ctx = Context(dev)
            _contexts[dev] = ctx
    return ctx
