// cvgrad.h -- the leave-one-out cross-validation objective and its gradient with respect to the hyperparameters
// (gpc_cv_grad; DESIGN.md "Cross-validation objective").
//
// Sigma = K + mult diag(sn2) at the posterior's own jitter multiplier (held fixed), Q = Sigma^-1, alpha = Q (y - m),
// q_i = Q_ii.  Leaving point i out predicts y_i with mean y_i - alpha_i / q_i and variance 1 / q_i (Rasmussen & Williams
// 5.4.2).  With per-point weights w_i >= 0:
//   loss "lpd":  L = -sum_i w_i (1/2 log q_i - alpha_i^2 / (2 q_i) - 1/2 log 2 pi)
//                c_i = w_i (1 + alpha_i^2 / q_i) / (2 q_i)        b_i = w_i alpha_i / q_i
//   loss "mse":  L =  sum_i w_i (alpha_i / q_i)^2
//                c_i = 2 w_i alpha_i^2 / q_i^3                    b_i = 2 w_i alpha_i / q_i^2
// (c = -dL/dq, b = dL/dalpha).  Every derivative of L collapses onto ONE symmetric weight matrix: with beta = Q b,
//   G = Q diag(c) Q - 1/2 (beta alpha^T + alpha beta^T)
//   dL / d theta_p = <d_p K, G>                  covariance hyperparameter p (the planes of nll_hess.h: F d_a^2 | 2 K | Ka)
//                  = mult sum_i G_ii d_n sn2_i   noise hyperparameter n
//                  = -beta . d_k m               mean hyperparameter k
// which is the contraction of the marginal likelihood's gradient (trace_kernel, weight Q - alpha alpha^T) with another
// weight: no plane d_p K is ever formed, and the cost does not depend on the number of hyperparameters.
//
// The kernels below: c and b per point (cvg_weights_kernel) and the contraction over the lower 64 x 64 tiles
// (cvg_trace_kernel).  Q, beta = Q b and the column scaling Q diag(c) are nll_hess.h's kernels, M = Q diag(c) Q the plain
// fp64 GEMM over the lower tiles.  Every reduction has an order fixed by the shape alone: no atomics, the same bits for
// a sample in any batch or chunk.  All fp64.
#pragma once
#include "nll_hess.h"

namespace gpc {

enum { CVG_LPD = 0, CVG_MSE = 1 };  // the loss of gpc_cv_grad

// ---------------------------------------------------------------------------------
// q_i and the loss's c_i, b_i (the header's formulas) for i < n; zeros in the padding.  q_i = qsrc[b sq + i qstep]: the
// diagonal of the dense Q itself (qstep = npad + 1), which is diagq_i + alpha_i^2 of nh_form_q_kernel without the
// cancellation, or a plain vector (qstep = 1).  omega: the weights, one vector of npad for all samples.
// grid = (npad / 256 rounded up, batch), one thread per point
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cvg_weights_kernel(const double* __restrict__ alpha_all,
                                                          const double* __restrict__ qsrc, long long sq, int qstep,
                                                          const double* __restrict__ omega, int n, int npad, int loss,
                                                          double* __restrict__ q_all, double* __restrict__ c_all,
                                                          double* __restrict__ b_all) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  const size_t o = (size_t)blockIdx.y * npad + i;
  double q = 0.0, cv = 0.0, bv = 0.0;
  if (i < n) {
    const double a = alpha_all[o], w = omega[i];
    q = qsrc[(size_t)blockIdx.y * sq + (size_t)i * qstep];
    if (loss == CVG_LPD) {
      cv = w * (1.0 + a * a / q) / (2.0 * q);
      bv = w * a / q;
    } else {
      cv = 2.0 * w * a * a / (q * q * q);
      bv = 2.0 * w * a / (q * q);
    }
  }
  q_all[o] = q;
  c_all[o] = cv;
  b_all[o] = bv;
}

// ---------------------------------------------------------------------------------
// The contraction <d_p K, G> over the lower triangle, a sibling of the fp64 trace_kernel with the weight
//   G_ij = M_ij - 1/2 (beta_i alpha_j + alpha_i beta_j)      (2 G_ij off the diagonal)
// M read from its lower triangle (the lower tiles the GEMM wrote):
//   part[b][tile][p], p < P = cov_N:  sum_ij w_ij G_ij dK_ij / d theta_p
//   diagG[b][i] = G_ii   (0 in the padding)
// Distances from tile_r2 (the same r2 to the bit as every covariance kernel), F, K and Ka from one pair_eval_t per
// pair; a pair at r2 = 0 is dropped from the lengthscale sums.  The second sweep over the dimensions and the wave_sum4
// reductions are trace_kernel's.  Dynamic LDS: 4 x P4 doubles, P4 = P rounded up to a multiple of 4, + 4.
// grid = (lower tiles of npad / 64, batch).  T is double (the dispatch macro's parameter).
// ---------------------------------------------------------------------------------
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void cvg_trace_kernel(CovDesc cd, const double* __restrict__ Xs_all,
                                                        const double* __restrict__ sp_all,
                                                        const double* __restrict__ alpha_all,
                                                        const double* __restrict__ beta_all, int n, int npad,
                                                        const T* __restrict__ M_all, long long sM,
                                                        double* __restrict__ part_all, int ntiles,
                                                        double* __restrict__ diagG_all) {
  __shared__ double xi[CT][DCH + 1];
  __shared__ double xj[CT][DCH + 1];
  extern __shared__ double wpart[];  // [4][P4]
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, b = blockIdx.y;
  const int lane = t & 63, w = t >> 6;
  const int P = cd.cov_N;
  const int P4 = ((P + 3) & ~3) + 4;
  constexpr bool ISO = (KIND == K_SE_ISO || KIND == K_MATERN_ISO);
  int ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int i0 = ti * CT, j0 = tj * CT;
  const double* Xs = Xs_all + (size_t)b * npad * cd.D;
  const double* sp = sp_all + (size_t)b * SP_STRIDE;
  const double* alpha = alpha_all + (size_t)b * npad;
  const double* beta = beta_all + (size_t)b * npad;
  const T* Mm = M_all + (size_t)b * sM;
  double* part = part_all + ((size_t)b * ntiles + blockIdx.x) * P;

  // the 16 entries of M of this thread first: their latency hides under the distance sweep (entries above the diagonal
  // of a diagonal tile are loaded and not used)
  T min_[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) min_[a][c] = Mm[(size_t)(i0 + ty + 16 * a) * npad + j0 + tx + 16 * c];
  double r2[4][4];
  tile_r2(r2, xi, xj, Xs, cd.D, i0, j0, t, tx, ty);
  double al_i[4], al_j[4], be_i[4], be_j[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    al_i[a] = alpha[i0 + ty + 16 * a];
    al_j[a] = alpha[j0 + tx + 16 * a];
    be_i[a] = beta[i0 + ty + 16 * a];
    be_j[a] = beta[j0 + tx + 16 * a];
  }

  const double sf2 = sp[SP_SF2], rqa = sp[SP_RQA];
  ExpC ex;
  ex.load();
  double gF[4][4];
  double g_sf = 0.0, g_a = 0.0, g_iso = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
      const bool valid = (i < n) && (j <= i);
      double gf = 0.0;
      if (valid) {
        const double G = fma(-0.5, fma(be_i[a], al_j[c], al_i[a] * be_j[c]), (double)min_[a][c]);
        const double gw = (i == j) ? G : 2.0 * G;
        const PairVal pv = pair_eval_t<KIND, DEG>(r2[a][c], sf2, rqa, ex);
        g_sf = fma(gw, 2.0 * pv.K, g_sf);
        if constexpr (KIND == K_RQ) g_a = fma(gw, pv.Ka, g_a);
        if (r2[a][c] > 0.0) gf = gw * pv.F;
        if constexpr (ISO) g_iso = fma(gf, r2[a][c], g_iso);
        if (i == j) diagG_all[(size_t)b * npad + i] = G;
      } else if (i == j) {
        diagG_all[(size_t)b * npad + i] = 0.0;  // the padding's diagonal
      }
      gF[a][c] = gf;  // masked entries and pairs at r2 = 0: exactly 0
    }

  const int own = lane >> 4;  // which of the four values of a wave_sum4 this lane ends up holding
  if constexpr (ISO) {
    const double u = wave_sum4(g_iso, g_sf, 0.0, 0.0, lane);
    if ((lane & 15) == 0 && own < 2) wpart[w * P4 + own] = u;  // slots 0, 1
  } else {
    // second sweep over the input dimensions, four at a time: sum_e gF[e] * d_h[e]^2
    for (int h0 = 0; h0 < cd.D; h0 += DCH) {
      const int dc = min(DCH, cd.D - h0);
      if (cd.D > DCH) {  // restage (single pass when D <= 32: LDS still holds it)
        __syncthreads();
        stage_x(xi, Xs, cd.D, i0, h0, dc, t);
        stage_x(xj, Xs, cd.D, j0, h0, dc, t);
        __syncthreads();
      }
      for (int h = 0; h < dc; h += 4) {
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int hh = h + q;
          if (hh >= dc) break;  // block-uniform: the surplus slots of the last group stay 0 and are not stored
          double vi[4], vj[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) vi[a] = xi[ty + 16 * a][hh];
#pragma unroll
          for (int c = 0; c < 4; ++c) vj[c] = xj[tx + 16 * c][hh];
          double s = 0.0;
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const double d = vi[a] - vj[c];
              s = fma(gF[a][c] * d, d, s);
            }
          s4[q] = s;
        }
        const double u = wave_sum4(s4[0], s4[1], s4[2], s4[3], lane);
        if ((lane & 15) == 0 && h + own < dc) wpart[w * P4 + h0 + h + own] = u;
      }
    }
    const double u = wave_sum4(g_sf, g_a, 0.0, 0.0, lane);
    if ((lane & 15) == 0) {
      if (own == 0) wpart[w * P4 + cd.D] = u;
      if (own == 1 && KIND == K_RQ) wpart[w * P4 + cd.D + 1] = u;
    }
  }
  __syncthreads();
  for (int p = t; p < P; p += 256)
    part[p] = wpart[p] + wpart[P4 + p] + wpart[2 * P4 + p] + wpart[3 * P4 + p];
}

}  // namespace gpc
