// quad_mix.h -- Bayesian quadrature against a MIXTURE sum_j w_j N(mu_j, diag(sigma_j^2)) (gpc_quad_mix) and the
// covariance between the integrals against the single measures (gpc_quad_cov).
//
// With z_ij as quad_z_kernel forms it, zbar = Z w (one N-vector per sample) and q = (K + Sigma)^-1 zbar:
//   E = sum_j w_j (z_j . alpha + nu_j),   V = w^T Gamma w - zbar . q,
//   Gamma_jk = sf2 prod_l ell_l / sqrt(t_jkl) exp(-1/2 sum_l (mu_jl - mu_kl)^2 / t_jkl),  t_jkl = ell_l^2 + sigma_jl^2 + sigma_kl^2
// (Gamma_jj is quad's nf_kk).  The cross term needs one pair of triangular matrix-vector products per sample where
// quad's diagonal needs an N^2 M product, and every gradient of it is quad.h's contraction with the VECTOR q in place of
// the N x M matrix Q.  Z is never stored: both passes over the (training point, measure) tiles recompute z in fp64.
//   d1 Gamma_jk / dmu_jl    = -Gamma_jk (mu_jl - mu_kl) / t_jkl
//   d1 Gamma_jk / dsigma_jl =  Gamma_jk sigma_jl ((mu_jl - mu_kl)^2 / t_jkl - 1) / t_jkl        (first slot only)
// As in quad.h every difference is formed per pair, never expanded into moments, and every order of summation is fixed
// by the shape: a sample's bits do not depend on the batch or on the chunking.
#pragma once
#include "quad.h"

namespace gpc {

// Gamma of sample b as a dense block (gpc_quad_cov: where predict_full puts K**), zero padding.
// grid = (mpad / 64, mpad / 4, batch), block = (64, 4)
template <typename T>
__global__ void quad_gamma_kernel(const double* __restrict__ mu, const double* __restrict__ sigma,
                                  const double* __restrict__ dv_all, const double* __restrict__ sp_all, int m, int mpad,
                                  int D, T* __restrict__ G_all, long long sG) {
  const int b = blockIdx.z;
  const int k = blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y * 4 + threadIdx.y;
  if (j >= mpad || k >= mpad) return;
  double v = 0.0;
  if (j < m && k < m) {
    const double* ell = dv_all + (size_t)b * D;
    double lng = log(sp_all[(size_t)b * SP_STRIDE + SP_SF2]), acc = 0.0;
    for (int l = 0; l < D; ++l) {
      const double sj = sigma[(size_t)j * D + l], sk = sigma[(size_t)k * D + l];
      const double t = ell[l] * ell[l] + (sj * sj + sk * sk);  // (symmetric in j, k to the bit)
      const double d = mu[(size_t)j * D + l] - mu[(size_t)k * D + l];
      lng += log(ell[l]) - 0.5 * log(t);
      acc += d * d / t;
    }
    v = exp(lng - 0.5 * acc);
  }
  G_all[(size_t)b * sG + (size_t)j * mpad + k] = (T)v;
}

// What the pair kernel reads per measure, sample independent: sgt[l][j] = sigma_jl (transposed like quad.h's mut) and
// wpad[j] = w_j, both 0 in the padding.  grid = (mpad / 256)
__global__ __launch_bounds__(256) void quad_mix_prep_kernel(const double* __restrict__ sigma, const double* __restrict__ w,
                                                            int m, int mpad, int D, double* __restrict__ sgt,
                                                            double* __restrict__ wpad) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= mpad) return;
  for (int l = 0; l < D; ++l) sgt[(size_t)l * mpad + j] = j < m ? sigma[(size_t)j * D + l] : 0.0;
  wpad[j] = j < m ? w[j] : 0.0;
}

// First sweep.  One 64 x 64 tile (training points i0.., measures j0..) of sample b, z recomputed per pair as in
// quad_grad_tile_kernel (lane = measure, wave w = rows 16 w .. 16 w + 15):
//   cpart[b][ti][j] = sum over the tile's rows    of alpha_i z_ij   (the four waves added in wave order)
//   rpart[b][tj][i] = sum over the tile's measures of w_j z_ij      (a butterfly over the wave's 64 lanes)
// colpart_reduce_kernel adds the tiles in ascending order: z . alpha and zbar.
// grid = (mpad / 64, npad / 64, batch), 256 threads, 18 KB of LDS.
__global__ __launch_bounds__(256) void quad_mix_sum_tile_kernel(const double* __restrict__ X, int D,
                                                                const double* __restrict__ mut,
                                                                const double* __restrict__ con_all,
                                                                const double* __restrict__ alpha_all, int astride,
                                                                const double* __restrict__ wpad, int n, int m, int mpad,
                                                                int npad, double* __restrict__ cpart_all,
                                                                double* __restrict__ rpart_all) {
  __shared__ double xt[QCH][CT];
  __shared__ double red[4][CT];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.z;
  const int i0 = blockIdx.y * CT, j = blockIdx.x * CT + lane, r0 = 16 * w;
  const double* con = con_all + (size_t)b * (D + 1) * mpad;
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  for (int h0 = 0; h0 < D; h0 += QCH) {
    const int dc = min(QCH, D - h0);
    __syncthreads();  // the previous chunk is read
    for (int e = t; e < dc * CT; e += 256) {
      const int h = e / CT, r = e % CT, i = i0 + r;
      xt[h][r] = i < n ? X[(size_t)i * D + h0 + h] : 0.0;
    }
    __syncthreads();
    for (int h = 0; h < dc; ++h) {
      const double mj = mut[(size_t)(h0 + h) * mpad + j], ij = con[(size_t)(h0 + h) * mpad + j];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const double u = (mj - xt[h][r0 + k]) * ij;
        acc[k] = fma(u, u, acc[k]);
      }
    }
  }
  const double lnnf = con[(size_t)D * mpad + j], wj = wpad[j];
  const double* alpha = alpha_all + (size_t)b * astride;
  double ca = 0.0, mine = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int i = i0 + r0 + k;
    const bool in = i < n && j < m;
    const double z = in ? exp(lnnf - 0.5 * acc[k]) : 0.0;
    ca = fma(in ? alpha[i] : 0.0, z, ca);
    const double rs = wave_sum(wj * z);
    if (lane == k) mine = rs;
  }
  if (lane < 16) rpart_all[((size_t)b * gridDim.x + blockIdx.x) * npad + i0 + r0 + lane] = mine;
  red[w][lane] = ca;
  __syncthreads();
  if (w == 0)
    cpart_all[((size_t)b * gridDim.y + blockIdx.y) * mpad + j] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// Second sweep, after the solve: quad_grad_tile_kernel with the variance weights q_i z_ij, q a VECTOR per sample (it
// carries the posterior's scaling: W^T W zbar / sl, or -(L zbar)).  Per tile
//   zqpart[b][ti][j] = sum over the tile's rows of q_i z_ij
// and with GRAD the four column sums of quad_grad_tile_kernel<T, true>, in its layout (part[b][ti][0..3][l][j]: P and R
// under the alpha weights, P and R under the q weights), for quad_grad_reduce_kernel.
// grid = (mpad / 64, npad / 64, batch), 256 threads, 24 KB of LDS.
template <bool GRAD>
__global__ __launch_bounds__(256) void quad_mix_q_tile_kernel(const double* __restrict__ X, int D,
                                                              const double* __restrict__ mut,
                                                              const double* __restrict__ con_all,
                                                              const double* __restrict__ alpha_all, int astride,
                                                              const double* __restrict__ q_all, int n, int m, int mpad,
                                                              int npad, double* __restrict__ zqpart_all,
                                                              double* __restrict__ part_all) {
  __shared__ double xt[QCH][CT];
  __shared__ double red[4][4][CT];
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
  const double* q = q_all + (size_t)b * npad;
  double wa[GRAD ? 16 : 1], wq[16], cq = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int i = i0 + r0 + k;
    const bool in = i < n && j < m;
    const double z = in ? exp(lnnf - 0.5 * acc[k]) : 0.0;
    if constexpr (GRAD) wa[k] = in ? alpha[i] * z : 0.0;
    wq[k] = in ? q[i] * z : 0.0;
    cq += wq[k];
  }
  __syncthreads();  // (red is free: nothing has used it yet, and xt is not touched here)
  red[w][0][lane] = cq;
  __syncthreads();
  if (w == 0)
    zqpart_all[((size_t)b * gridDim.y + blockIdx.y) * mpad + j] =
        ((red[0][0][lane] + red[1][0][lane]) + red[2][0][lane]) + red[3][0][lane];
  if constexpr (GRAD) {
    __syncthreads();
    double* part = part_all + ((size_t)b * gridDim.y + blockIdx.y) * 4 * D * mpad;
    for (int h0 = 0; h0 < D; h0 += QCH) {
      const int dc = min(QCH, D - h0);
      if (D > QCH) stage(h0, dc);
      for (int h = 0; h < dc; ++h) {
        const int l = h0 + h;
        const double mj = mut[(size_t)l * mpad + j], ij = con[(size_t)l * mpad + j];
        double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const double u = (mj - xt[h][r0 + k]) * ij;
          const double v = fma(u, u, -1.0);
          s[0] = fma(wa[k], u, s[0]);
          s[1] = fma(wa[k], v, s[1]);
          s[2] = fma(wq[k], u, s[2]);
          s[3] = fma(wq[k], v, s[3]);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) red[w][p][lane] = s[p];
        __syncthreads();
        // wave w adds quantity w over the four waves, in wave order
        part[((size_t)w * D + l) * mpad + j] = ((red[0][w][lane] + red[1][w][lane]) + red[2][w][lane]) + red[3][w][lane];
        __syncthreads();
      }
    }
  }
}

// Gamma pair kernel.  One 64 x 64 tile of measure pairs (j0.. in the lanes, k0.. in the rows: wave w takes
// k0 + 16 w .. + 15) of sample b; the partner's means and squared widths are staged in LDS and read wave-uniformly.
//   part[b][tk][0][j]         = sum over the tile's k of w_k Gamma_jk
//   part[b][tk][1 + l][j]     = sum_k w_k d1 Gamma_jk / dmu_jl                          (GRAD)
//   part[b][tk][1 + D + l][j] = sum_k w_k d1 Gamma_jk / dsigma_jl                       (GRAD)
// ln Gamma is summed from logarithms (a product of D ratios ell^2 / t underflows at large D).
// grid = (mpad / 64, mpad / 64, batch), 256 threads, 36 KB of LDS.
template <bool GRAD>
__global__ __launch_bounds__(256) void quad_mix_gamma_tile_kernel(const double* __restrict__ mut,
                                                                  const double* __restrict__ sgt,
                                                                  const double* __restrict__ wpad,
                                                                  const double* __restrict__ dv_all,
                                                                  const double* __restrict__ sp_all, int D, int m,
                                                                  int mpad, double* __restrict__ part_all) {
  __shared__ double mk[QCH][CT];
  __shared__ double sk[QCH][CT];  // sigma_kl^2
  __shared__ double red[4][2][CT];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, b = blockIdx.z;
  const int k0 = blockIdx.y * CT, j = blockIdx.x * CT + lane, r0 = 16 * w;
  const int nq = GRAD ? 1 + 2 * D : 1;
  const double* ell = dv_all + (size_t)b * D;
  auto stage = [&](int h0, int dc) {
    __syncthreads();  // the previous chunk is read
    for (int e = t; e < dc * CT; e += 256) {
      const int h = e / CT, r = e % CT;
      const double s = sgt[(size_t)(h0 + h) * mpad + k0 + r];
      mk[h][r] = mut[(size_t)(h0 + h) * mpad + k0 + r];
      sk[h][r] = s * s;
    }
    __syncthreads();
  };
  double acc[16], lg[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = lg[k] = 0.0;
  double lnc = log(sp_all[(size_t)b * SP_STRIDE + SP_SF2]);
  for (int h0 = 0; h0 < D; h0 += QCH) {
    const int dc = min(QCH, D - h0);
    stage(h0, dc);
    for (int h = 0; h < dc; ++h) {
      const double el = ell[h0 + h], mj = mut[(size_t)(h0 + h) * mpad + j], sj = sgt[(size_t)(h0 + h) * mpad + j];
      const double base = fma(el, el, sj * sj);
      lnc += log(el);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const double tt = base + sk[h][r0 + k], d = mj - mk[h][r0 + k];
        acc[k] = fma(d * d, 1.0 / tt, acc[k]);
        lg[k] += log(tt);
      }
    }
  }
  double G[16], s0 = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int kk = k0 + r0 + k;
    G[k] = (j < m && kk < m) ? wpad[kk] * exp(lnc - 0.5 * (lg[k] + acc[k])) : 0.0;
    s0 += G[k];
  }
  double* part = part_all + ((size_t)b * gridDim.y + blockIdx.y) * nq * mpad;
  __syncthreads();
  red[w][0][lane] = s0;
  __syncthreads();
  if (w == 0) part[j] = ((red[0][0][lane] + red[1][0][lane]) + red[2][0][lane]) + red[3][0][lane];
  if constexpr (GRAD) {
    __syncthreads();
    for (int h0 = 0; h0 < D; h0 += QCH) {
      const int dc = min(QCH, D - h0);
      if (D > QCH) stage(h0, dc);
      for (int h = 0; h < dc; ++h) {
        const int l = h0 + h;
        const double el = ell[l], mj = mut[(size_t)l * mpad + j], sj = sgt[(size_t)l * mpad + j];
        const double base = fma(el, el, sj * sj);
        double sm = 0.0, ss = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const double it = 1.0 / (base + sk[h][r0 + k]), d = mj - mk[h][r0 + k];
          const double di = d * it;
          sm = fma(-G[k], di, sm);
          ss = fma(G[k], fma(d, di, -1.0) * it, ss);
        }
        red[w][0][lane] = sm;
        red[w][1][lane] = ss * sj;
        __syncthreads();
        if (w < 2)  // wave 0 adds the mu plane, wave 1 the sigma plane, in wave order
          part[(size_t)(1 + w * D + l) * mpad + j] = ((red[0][w][lane] + red[1][w][lane]) + red[2][w][lane]) + red[3][w][lane];
        __syncthreads();
      }
    }
  }
}

// The pair tiles of each sample summed in ascending tile order: gw[b][j] (quantity 0) and, for nq = 1 + 2 D, the planes
// res[p][b][j][l] (p = 0: mu, 1: sigma; plane = the stride of p), quad_grad_reduce_kernel's layout.
// grid = (mpad / 256, nq, batch)
__global__ __launch_bounds__(256) void quad_mix_gamma_reduce_kernel(const double* __restrict__ part, int nt, int D, int nq,
                                                                    int mpad, double* __restrict__ gw,
                                                                    double* __restrict__ res, size_t plane) {
  const int b = blockIdx.z, q = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= mpad) return;
  double s = 0.0;
  for (int k = 0; k < nt; ++k) s += part[(((size_t)b * nt + k) * nq + q) * mpad + j];
  if (q == 0) {
    gw[(size_t)b * mpad + j] = s;
  } else {
    const int p = (q - 1) / D, l = (q - 1) % D;
    res[(size_t)p * plane + ((size_t)b * mpad + j) * D + l] = s;
  }
}

}  // namespace gpc
