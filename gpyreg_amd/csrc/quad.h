// quad.h -- gradients of the Bayesian quadrature products (gpc_quad_grad) with respect to the means and the widths of
// the Gaussian measures N(mu_j, diag(sigma_j^2)).
//
// With tau_jl^2 = sigma_jl^2 + ell_l^2, d_ijl = mu_jl - X_il (the raw inputs and the length scales quad_z_kernel uses)
// and z_ij = nf_j exp(-1/2 sum_l d_ijl^2 / tau_jl^2), ln nf_j = ln sf2 + sum_l (ln ell_l - ln tau_jl):
//   dz_ij / dmu_jl    = -z_ij d_ijl / tau_jl^2
//   dz_ij / dsigma_jl =  z_ij sigma_jl (d_ijl^2 / tau_jl^2 - 1) / tau_jl^2
// so for a weight vector w_:j (alpha_i z_ij for z.alpha; q_ij z_ij, q = (K + Sigma)^-1 z, for z (K + Sigma)^-1 z^T)
// every derivative is one of two contractions over the training points, with u_ijl = d_ijl / tau_jl:
//   P_jl = sum_i w_ij u_ijl,   R_jl = sum_i w_ij (u_ijl^2 - 1)
//   d(z.alpha) / dmu = -P / tau,  d(z.alpha) / dsigma = sigma R / tau^2;  d(z Kinv z^T): 2 x the same (Kinv symmetric).
// The differences d_ijl are formed per pair before any product.  The moment form mu^2 sum w - 2 mu sum w X + sum w X^2
// would be a plain GEMM but cancels catastrophically when the measures sit far from the origin relative to tau.
#pragma once
#include "covfun.h"

namespace gpc {

// Per-measure constants of sample b, once per measure rather than once per pair (layout [l][mpad]: coalesced in j):
//   con[b][l][j] = 1 / tau_jl (l < D),  con[b][D][j] = ln nf_j;  mut[l][j] = mu_jl (sample independent, blockIdx.y 0).
// Padding columns j >= m hold 0.  grid = (mpad / 256, batch)
__global__ __launch_bounds__(256) void quad_grad_prep_kernel(const double* __restrict__ mu, const double* __restrict__ sigma,
                                                             const double* __restrict__ dv_all,
                                                             const double* __restrict__ sp_all, int m, int mpad, int D,
                                                             double* __restrict__ mut, double* __restrict__ con_all) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= mpad) return;
  const double* ell = dv_all + (size_t)b * D;
  double* con = con_all + (size_t)b * (D + 1) * mpad;
  double lnnf = log(sp_all[(size_t)b * SP_STRIDE + SP_SF2]);
  for (int l = 0; l < D; ++l) {
    double it = 0.0, mv = 0.0;
    if (j < m) {
      const double sg = sigma[(size_t)j * D + l];
      const double tau = sqrt(sg * sg + ell[l] * ell[l]);
      lnnf += log(ell[l]) - log(tau);
      it = 1.0 / tau;
      mv = mu[(size_t)j * D + l];
    }
    con[(size_t)l * mpad + j] = it;
    if (b == 0) mut[(size_t)l * mpad + j] = mv;
  }
  con[(size_t)D * mpad + j] = j < m ? lnnf : 0.0;
}

constexpr int QCH = 32;  // dimensions of the training inputs staged in LDS per pass

// One 64 x 64 tile (training points i0.., measures j0..) of sample b: the column sums over the tile's 64 rows of
//   part[b][ti][0][l][j] = P (alpha weights), [1] = R (alpha weights); with VAR also [2] = P, [3] = R under the weights
//   qs * Qstored_ij * z_ij  (qs = 1/sl, Qstored = W^T V for L_chol samples; qs = -1, Qstored = G = L Z otherwise).
// Lane = measure j, wave w = rows 16 w .. 16 w + 15 of the tile: the staged inputs are wave-uniform LDS reads
// (broadcast).  z is recomputed in fp64 with one exp per pair; the four waves' sums are added in wave order through LDS.
// Every order is fixed by the shape: a sample's partials do not depend on the batch, the chunking or the other measures.
// grid = (mpad / 64, npad / 64, batch), 256 threads, 24 KB of LDS.
template <typename T, bool VAR>
__global__ __launch_bounds__(256) void quad_grad_tile_kernel(const double* __restrict__ X, int D,
                                                             const double* __restrict__ mut,
                                                             const double* __restrict__ con_all,
                                                             const double* __restrict__ alpha_all, int astride,
                                                             const T* __restrict__ Q_all, long long sQ,
                                                             const double* __restrict__ sp_all, int lch, int n, int m,
                                                             int mpad, double* __restrict__ part_all) {
  constexpr int NQ = VAR ? 4 : 2;
  __shared__ double xt[QCH][CT];    // the tile's training inputs, transposed: xt[l - h0][r]
  __shared__ double red[4][4][CT];  // per-wave sums [wave][quantity][measure]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.z;
  const int i0 = blockIdx.y * CT, j = blockIdx.x * CT + lane, r0 = 16 * w;
  const double* con = con_all + (size_t)b * (D + 1) * mpad;
  auto stage = [&](int h0, int dc) {
    __syncthreads();  // the previous chunk is read
    for (int e = t; e < dc * CT; e += 256) {
      const int h = e / CT, r = e % CT, i = i0 + r;
      xt[h][r] = i < n ? X[(size_t)i * D + h0 + h] : 0.0;
    }
    __syncthreads();
  };
  // pass 1: sum_l u^2 per pair, then z and the weights
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  for (int h0 = 0; h0 < D; h0 += QCH) {
    const int dc = min(QCH, D - h0);
    stage(h0, dc);
    for (int h = 0; h < dc; ++h) {
      const double mj = mut[(size_t)(h0 + h) * mpad + j], ij = con[(size_t)(h0 + h) * mpad + j];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const double u = (mj - xt[h][r0 + k]) * ij;
        acc[k] = fma(u, u, acc[k]);
      }
    }
  }
  const double lnnf = con[(size_t)D * mpad + j];
  const double* alpha = alpha_all + (size_t)b * astride;
  const T* Q = Q_all + (size_t)b * sQ;
  const double qs = lch ? 1.0 / sp_all[(size_t)b * SP_STRIDE + SP_SL] : -1.0;
  double wa[16], wq[VAR ? 16 : 1];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int i = i0 + r0 + k;
    const bool in = i < n && j < m;
    const double z = in ? exp(lnnf - 0.5 * acc[k]) : 0.0;
    wa[k] = in ? alpha[i] * z : 0.0;
    if constexpr (VAR) wq[k] = in ? (double)Q[(size_t)i * mpad + j] * qs * z : 0.0;
  }
  // pass 2: the contractions, one dimension at a time (the last chunk is still staged when D <= QCH)
  double* part = part_all + ((size_t)b * gridDim.y + blockIdx.y) * NQ * D * mpad;
  for (int h0 = 0; h0 < D; h0 += QCH) {
    const int dc = min(QCH, D - h0);
    if (D > QCH) stage(h0, dc);
    for (int h = 0; h < dc; ++h) {
      const int l = h0 + h;
      const double mj = mut[(size_t)l * mpad + j], ij = con[(size_t)l * mpad + j];
      double s[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q) s[q] = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const double u = (mj - xt[h][r0 + k]) * ij;
        const double v = fma(u, u, -1.0);
        s[0] = fma(wa[k], u, s[0]);
        s[1] = fma(wa[k], v, s[1]);
        if constexpr (VAR) {
          s[2] = fma(wq[k], u, s[2]);
          s[3] = fma(wq[k], v, s[3]);
        }
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) red[w][q][lane] = s[q];
      __syncthreads();
      if (w < NQ)  // wave w adds quantity w over the four waves, in wave order
        part[((size_t)w * D + l) * mpad + j] = ((red[0][w][lane] + red[1][w][lane]) + red[2][w][lane]) + red[3][w][lane];
      __syncthreads();
    }
  }
}

// The tile partials of each sample summed in ascending tile order and turned into the derivatives
//   res[q][b][j][l]:  q = 0 d(z.alpha)/dmu = -P it,  1 d(z.alpha)/dsigma = sigma R it^2,  (nq = 4:) 2, 3 the same forms
//   of the variance weights times 2  (it = 1/tau; the variance weights carry qs).  plane = the stride of q.
// One thread per (j, q, l): nt loads each, coalesced in j.  grid = (mpad / 256, nq * D, batch)
__global__ __launch_bounds__(256) void quad_grad_reduce_kernel(const double* __restrict__ part, int nt, int D, int nq,
                                                               int m, int mpad, const double* __restrict__ sigma,
                                                               const double* __restrict__ con_all,
                                                               double* __restrict__ res, size_t plane) {
  const int b = blockIdx.z, j = blockIdx.x * 256 + threadIdx.x;
  const int q = blockIdx.y / D, l = blockIdx.y % D;
  if (j >= mpad) return;
  const double it = con_all[((size_t)b * (D + 1) + l) * mpad + j];
  const double sg = j < m ? sigma[(size_t)j * D + l] : 0.0;
  double s = 0.0;
  for (int k = 0; k < nt; ++k) s += part[((((size_t)b * nt + k) * nq + q) * D + l) * mpad + j];
  const double f = (q & 1) ? sg * (s * it) * it : -(s * it);
  res[(size_t)q * plane + ((size_t)b * mpad + j) * D + l] = q >= 2 ? 2.0 * f : f;
}

}  // namespace gpc
