"""The yardstick of tests/test_gpu_rhs_products.py (tests/rhs_ref.py) checked on the CPU: against the oracle's fp64
restatement of the reference, against the reference's own recorded output (tests/golden/full_cases.npz), its quadrature
vectors against Gauss-Hermite quadrature of the kernel, and the conditioning of the problems the GPU tests run."""

import os

import numpy as np
import pytest
from numpy.polynomial.hermite import hermgauss

import rhs_ref as rr
from conftest import parse_core_name
from oracle import gp_oracle as orc
from rhs_ref import LD

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "full_cases.npz")


def _f(a):
    return np.asarray(a).astype(np.float64)


def test_reference_matches_the_oracle_on_a_mixed_batch():
    """orc.predict on orc.posteriors (LAPACK, fp64) for the mixed L_chol batch of the GPU tests at (129, 65): mean and
    variance per sample to 1e-10 of the largest entry (the oracle's own error is eps cond ~ 1e-14 here; its clamp at 0
    does not bind, the smallest variance is sn2 = 1e-7)."""
    ref = rr.reference("se", 129, 65)
    p = ref["problem"]
    model = dict(kernel="se", degree=0, mean="const", noise=(1, 0, 0))
    hyp = np.concatenate([p["hyp_cov"], 0.5 * np.log(p["sn2"])[:, None], p["m0"][:, None]], axis=1)
    assert np.allclose(np.exp(2 * hyp[:, 4]), p["sn2"], rtol=1e-14, atol=0)  # (the oracle's noise: exp of a logarithm)
    posts = orc.posteriors(model, hyp, p["X"], p["y"], None)
    assert [bool(q.L_chol) for q in posts] == list(rr.LCHOL) and all(q.sn2_mult == 1 for q in posts)
    mu, s2 = orc.predict(model, posts, p["X"], p["y"], p["xs"], separate_samples=True)
    want_mu = _f(ref["fmu"]) + p["m0"][None, :]
    assert np.abs(mu - want_mu).max() <= 1e-10 * np.abs(want_mu).max()
    assert _f(ref["fs2"]).min() > 0 and np.abs(s2 - _f(ref["fs2"])).max() <= 1e-10 * _f(ref["fs2"]).max()
    # the identities between the outputs: diag C = fs2 = kss + fq
    assert np.abs(_f(np.einsum("sii->is", ref["C"]) - ref["fs2"])).max() <= 1e-18
    assert np.abs(_f(ref["fs2"] - (1 + ref["fq"]))).max() <= 1e-18


def test_reference_matches_the_recorded_predict_full():
    """C and fmu + mean against *_pf_cov, *_pf_mu of all five recorded cases (per-point noise, negative-quadratic mean
    and the zero-noise low-noise case included) at the goldens' 1e-8.  The noise is the oracle's, times the jitter
    multiplier its factorization settled on."""
    g = np.load(GOLDEN, allow_pickle=False)
    assert len(g["names"]) == 5
    lownoise = 0
    for name in g["names"]:
        tag, model, N, D, _ = parse_core_name(str(name) + "|plain")
        X, y, hyp, xs = g[tag + "_X"], g[tag + "_y"], g[tag + "_hyp"], g[tag + "_xs"]
        s2 = g[tag + "_s2"] if tag + "_s2" in g.files else None
        kernel, degree = model["kernel"], model["degree"]
        cov_N, noise_N = orc.cov_count(kernel, D), orc.noise_count(model["noise"])
        posts = orc.posteriors(model, hyp, X, y, s2)
        want_mu, want_C = g[tag + "_pf_mu"], g[tag + "_pf_cov"]
        for s, post in enumerate(posts):
            h_cov, h_noise, h_mean = hyp[s, :cov_N], hyp[s, cov_N:cov_N + noise_N], hyp[s, cov_N + noise_N:]
            sn2 = np.asarray(orc.noise(model["noise"], h_noise, X, y, s2)) * post.sn2_mult
            lownoise += not post.L_chol
            ref = rr.SampleRef(orc.covariance(kernel, h_cov, X, degree=degree), sn2.ravel(),
                               y[:, 0] - orc.mean(model["mean"], h_mean, X))
            Ks = orc.covariance(kernel, h_cov, X, xs, degree=degree)
            C, _ = ref.full(Ks, orc.covariance(kernel, h_cov, xs, xs, degree=degree))
            mu = _f(ref.lin(Ks)) + orc.mean(model["mean"], h_mean, xs)
            assert np.allclose(mu, want_mu[:, s], rtol=1e-8, atol=1e-8), (name, s)
            assert np.abs(_f(C) - want_C[:, :, s]).max() <= 1e-8 * np.abs(want_C).max(), (name, s, ref.cond)
    assert lownoise == 3  # (the `zero` case: sn2 = eps)


@pytest.mark.parametrize("D", [1, 2])
def test_quad_z_against_gauss_hermite(D):
    """Z_ij is the integral of k(x, X_i) against N(mu_j, diag(sigma_j^2)): Gauss-Hermite quadrature (80 nodes per
    dimension; the integrand in t is exp(-a t^2 + b t), a = sigma^2 / ell^2 <= 1.3, and the rule's error falls like
    (a / (1 + a))^n) to 1e-12 relative, every entry."""
    rng = np.random.default_rng(40 + D)
    N, M = 7, 5
    X = rng.uniform(-2, 2, (N, D))
    mu = rng.uniform(-1, 1, (M, D))
    sigma = 0.3 + 0.6 * rng.uniform(0, 1, (M, D))
    hyp = np.concatenate([np.log(0.8 + 0.2 * rng.uniform(0, 1, D)), [0.3]])
    Z = rr.quad_z(hyp, X, mu, sigma)
    t, w = hermgauss(80)
    t, w = t.astype(LD), w.astype(LD) / np.sqrt(LD(np.pi))
    ell, sf2 = np.exp(hyp[:D].astype(LD)), np.exp(2 * LD(hyp[D]))
    for i in range(N):
        for j in range(M):
            # the kernel factorizes over the dimensions, and so does the tensor rule
            val = sf2
            for l in range(D):
                x = LD(mu[j, l]) + np.sqrt(LD(2)) * LD(sigma[j, l]) * t
                val = val * np.sum(w * np.exp(-((x - LD(X[i, l])) / ell[l]) ** 2 / 2))
            assert abs(Z[i, j] - val) <= 1e-12 * abs(val), (i, j, float(Z[i, j]), float(val))
    # and the kernel the rule integrates is the oracle's
    k = orc.covariance("se", hyp, X, mu)
    kld = sf2 * np.exp(-np.sum(((mu.astype(LD)[None] - X.astype(LD)[:, None]) / ell) ** 2, axis=2) / 2)
    assert np.abs(k - _f(kld)).max() <= 1e-15 * float(sf2)


def test_gpu_problems_are_well_conditioned():
    """Every sample of every case the GPU tests run: cond_2(K_s + sn2_s I) <= 1e4 and the oracle's factorization at
    jitter multiplier 1 (no case is left out for its conditioning)."""
    assert len(rr.CASES) == 13
    worst = 0.0
    for kernel, N, M in rr.CASES:
        ref = rr.reference(kernel, N, M)
        p = ref["problem"]
        assert ref["cond"].shape == (rr.S,) and np.all(ref["cond"] <= 1e4), (kernel, N, M, ref["cond"])
        worst = max(worst, ref["cond"].max())
        name, degree = rr.KERNELS[kernel]
        model = dict(kernel=name, degree=degree, mean="const", noise=(1, 0, 0))
        hyp = np.concatenate([p["hyp_cov"], 0.5 * np.log(p["sn2"])[:, None], p["m0"][:, None]], axis=1)
        posts = orc.posteriors(model, hyp, p["X"], p["y"], None)
        assert all(q.sn2_mult == 1 for q in posts) and [bool(q.L_chol) for q in posts] == list(rr.LCHOL), (kernel, N, M)
    print("largest cond_2 over the GPU cases: %.3g" % worst)
