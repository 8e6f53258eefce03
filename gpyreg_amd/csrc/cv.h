// cv.h -- leave-fold-out cross-validation from the resident posterior (gpc_cv; DESIGN.md "Cross-validation").
//
// With M = K + Sigma and P = M^-1 the predictive distribution of a held-out index set I given the other points, the
// hyperparameters fixed, has covariance C_I = (P_II)^-1 and mean y_I - C_I alpha_I (Rasmussen & Williams 5.4.2).
//   high noise (L_chol: W = Lo^-1, P = W^T W / sl):  G = W[:, I]^T W[:, I],  C = sl G^-1
//   low noise  (A = -(K + Sigma)^-1):                G = -A[I, I],           C = G^-1
// G = R R^T is factored by the library's blocked factorization in fp64 (plan.h), Wf = R^-1, and with u = Wf alpha_I
//   quad = sc u.u,   dmu = sc Wf^T u,   s2_j = sc sum_i Wf[i][j]^2,   logdet = k log sc - log det G.
// No covariance function is evaluated: the call serves posteriors of any origin.  Everything after the load of W or A
// is fp64 whatever the storage type T.  Every kernel takes (fold, sample) from blockIdx and sums in an order fixed
// by (N, I): the numbers of a fold do not depend on the other folds, the batch or the chunking.
#pragma once
#include "block_append.h"
#include "common.h"
#include "gemm.h"

namespace gpc {

constexpr int CV_T = 64;          // tile of G, and the columns a block of the leave-one-out pass owns
constexpr int CV_RS = 32;         // rows of W per slab of the fused Gram kernel
constexpr int CV_LD = CV_T + 16;  // LDS stride of a slab (k-major image as gemm.h's: ds_read_b64 fragments conflict free)
// The engine of the fold Gram: 1 = fused gather + MFMA (cv_gram_kernel), 2 = gathered panels + the library GEMM.
// Measured at cfg3 (N = 4096, S = 16, fp64; tools/cv_bench.py, profiles/cv_cfg3.json), device time of the Gram,
// engine 1 / engine 2: 10 scattered folds 5.6 / 5.8 ms, 10 contiguous 3.5 / 4.4, 5 contiguous 5.0 / 5.1, 2 contiguous
// 9.4 / 8.4.  The fused kernel wins or ties from 5 folds on and needs no panel scratch (engine 2: F N_pad kp doubles
// per sample, 134 MB at 2 folds); the library GEMM is 10 % faster at 2 folds of 2048 points, where the factorization
// (5.5 ms) and not the Gram decides the call.  Engine 1 is the default for every shape.
constexpr int CV_DEFAULT_ENGINE = 1;

// ---- leave-one-out: P_ii, one bandwidth pass -------------------------------------------------------------------
// L_chol samples: a block owns 64 columns of W and walks the 64-row slabs from its diagonal slab down, ascending, with
// 16-byte loads; every thread keeps the sums of squares of its 16 / sizeof(T) columns in fp64 registers, and the
// 256 / (64 / VEC) row groups are added in group order at the end.  Low-noise samples read the diagonal of A.
// With p = P_ii:  s2 = 1 / p,  dmu = alpha_i / p,  quad = alpha_i^2 / p,  logdet = -log p;  info = 1 and NaN when p is
// not positive.  Planes of npad per sample.  par: block_append.h's per-sample parameters (BA_SL, BA_LCH).
// grid = (ceil(N / 64), batch), 256 threads
template <typename T>
__global__ __launch_bounds__(256) void cv_diag_kernel(const T* __restrict__ A_all, const T* __restrict__ W_all, long long sM,
                                                      int npad, int N, const double* __restrict__ alpha_all,
                                                      const double* __restrict__ par, double* __restrict__ dmu,
                                                      double* __restrict__ s2, double* __restrict__ quad,
                                                      double* __restrict__ logdet, int* __restrict__ info) {
  constexpr int VEC = 16 / (int)sizeof(T), TPR = CV_T / VEC, GR = 256 / TPR;
  __shared__ double red[GR][CV_T];
  const int b = blockIdx.y, t = threadIdx.x, c0 = blockIdx.x * CV_T;
  const bool lch = par[(size_t)b * BA_STRIDE + BA_LCH] != 0.0;
  double p = 0.0;
  if (lch) {
    const T* W = W_all + (size_t)b * sM;
    const int g = t / TPR, cc = (t % TPR) * VEC;
    double acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
    for (int r0 = c0; r0 < N; r0 += CV_T) {
#pragma unroll
      for (int q = 0; q < CV_T / GR; ++q) {
        const int r = r0 + g + GR * q;
        if (r >= N) continue;
        const typename MM<T>::vec_t v = *reinterpret_cast<const typename MM<T>::vec_t*>(W + (size_t)r * npad + c0 + cc);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const double x = (c0 + cc + e <= r) ? (double)v[e] : 0.0;  // (above the diagonal W is not defined)
          acc[e] = fma(x, x, acc[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[g][cc + e] = acc[e];
    __syncthreads();
    if (t < CV_T) {
      double s = 0.0;
      for (int q = 0; q < GR; ++q) s += red[q][t];
      p = s / par[(size_t)b * BA_STRIDE + BA_SL];
    }
  } else if (t < CV_T && c0 + t < N) {
    p = -(double)A_all[(size_t)b * sM + (size_t)(c0 + t) * npad + c0 + t];
  }
  const int i = c0 + t;
  if (t >= CV_T || i >= N) return;
  const size_t o = (size_t)b * npad + i;
  const bool ok = p > 0.0 && p <= 1.7e308;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double a = alpha_all[o], v = 1.0 / p;
  dmu[o] = ok ? a * v : nan;
  s2[o] = ok ? v : nan;
  quad[o] = ok ? a * a * v : nan;
  logdet[o] = ok ? -log(p) : nan;
  info[o] = ok ? 0 : 1;
}

// ---- fold Gram, engine 1: gather + MFMA, the panel never leaves the chip --------------------------------------------
// One 64 x 64 tile (ti >= tj, tri_tile order) of G of fold f = blockIdx.y and sample blockIdx.z.  The rows of W are
// walked in slabs of CV_RS, ascending, from the slab of the first column index of tile ti: W[r][a] W[r][b] vanishes for
// r < max(a, b) and the indices ascend, so nothing before it contributes.  The slab's entries of the two column sets
// are gathered into LDS as fp64 (zero above W's diagonal, below row N and in the padding columns) and multiplied with
// v_mfma_f64_16x16x4_f64: 2 x 2 waves of 32 x 32, fragments laid out as gemm.h's k-major operands.  The tile and its
// mirror image are stored; rows and columns from k on are the identity.
// G_all: [(sample * F + f)][kp][kp].   grid = (tk (tk + 1) / 2, F, batch) with tk = kp / 64, 256 threads, 40 KB of LDS
template <typename T>
__global__ __launch_bounds__(256) void cv_gram_kernel(const T* __restrict__ W_all, long long sM, int npad, int N, int F,
                                                      const int* __restrict__ fptr, const int* __restrict__ fidx, int kp,
                                                      double* __restrict__ G_all) {
  using acc_t = MM<double>::acc_t;
  __shared__ double shA[CV_RS * CV_LD], shB[CV_RS * CV_LD];
  __shared__ int ia[CV_T], ib[CV_T];
  int ti, tj;
  tri_tile(blockIdx.x, ti, tj);
  const int f = blockIdx.y, b = blockIdx.z, t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int k = fptr[f + 1] - fptr[f];
  const int* __restrict__ I = fidx + fptr[f];
  double* __restrict__ G = G_all + ((size_t)b * F + f) * kp * kp;
  const int a0 = ti * CV_T, b0 = tj * CV_T;
  const bool diag = ti == tj;
  if (a0 >= k) {  // (block-uniform) a tile of the padding alone
    for (int e = t; e < CV_T * CV_T; e += 256) {
      const int r = e >> 6, c = e & 63;
      const double v = (diag && r == c) ? 1.0 : 0.0;
      G[(size_t)(a0 + r) * kp + b0 + c] = v;
      G[(size_t)(b0 + c) * kp + a0 + r] = v;
    }
    return;
  }
  if (t < CV_T) {
    ia[t] = a0 + t < k ? I[a0 + t] : -1;
    ib[t] = b0 + t < k ? I[b0 + t] : -1;
  }
  __syncthreads();
  const T* __restrict__ W = W_all + (size_t)b * sM;
  acc_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = acc_t{0, 0, 0, 0};
  const double* pb = diag ? shA : shB;
  for (int r0 = (ia[0] / CV_RS) * CV_RS; r0 < N; r0 += CV_RS) {
#pragma unroll
    for (int p = 0; p < CV_RS * CV_T / 256; ++p) {
      const int e = t + 256 * p, rr = e >> 6, cc = e & 63, r = r0 + rr;
      const int ca = ia[cc];
      shA[rr * CV_LD + cc] = (ca >= 0 && r < N && ca <= r) ? (double)W[(size_t)r * npad + ca] : 0.0;
      if (!diag) {
        const int cb = ib[cc];
        shB[rr * CV_LD + cc] = (cb >= 0 && r < N && cb <= r) ? (double)W[(size_t)r * npad + cb] : 0.0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < CV_RS; kk += 4) {
      const int row = (kk + (lane >> 4)) * CV_LD + (lane & 15);
      double af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = shA[row + wr * 32 + i * 16];
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = pb[row + wc * 32 + j * 16];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = MM<double>::mma(af[i], bf[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = a0 + wr * 32 + i * 16 + MM<double>::row_of(lane, q);
        const int col = b0 + wc * 32 + j * 16 + (lane & 15);
        double v = acc[i][j][q];
        if (row >= k || col >= k) v = row == col ? 1.0 : 0.0;
        G[(size_t)row * kp + col] = v;
        if (!diag) G[(size_t)col * kp + row] = v;
      }
}

// ---- fold Gram, engine 2: the k-major panel W[:, I] (npad x kp, fp64, zero padding) for the library GEMM ---------------
// panel: [(sample * F + f)][npad][kp].   grid = (kp / 64, npad / 4, F * batch), block = (64, 4)
template <typename T>
__global__ void cv_panel_kernel(const T* __restrict__ W_all, long long sM, int npad, int N, int F,
                                const int* __restrict__ fptr, const int* __restrict__ fidx, int kp,
                                double* __restrict__ panel) {
  const int f = blockIdx.z % F, b = blockIdx.z / F;
  const int j = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
  if (j >= kp || r >= npad) return;
  const int k = fptr[f + 1] - fptr[f];
  double v = 0.0;
  if (j < k && r < N) {
    const int c = fidx[fptr[f] + j];
    if (c <= r) v = (double)W_all[(size_t)b * sM + (size_t)r * npad + c];
  }
  panel[(((size_t)b * F + f) * npad + r) * kp + j] = v;
}

// the identity in the padding of G after the GEMM (its padded rows and columns are zero)     grid = (F, batch)
__global__ __launch_bounds__(256) void cv_pad_diag_kernel(int F, const int* __restrict__ fptr, int kp,
                                                          double* __restrict__ G_all) {
  const int f = blockIdx.x, b = blockIdx.y;
  double* G = G_all + ((size_t)b * F + f) * kp * kp;
  for (int j = fptr[f + 1] - fptr[f] + threadIdx.x; j < kp; j += 256) G[(size_t)j * kp + j] = 1.0;
}

// ---- low noise: G = -A[I, I] with the identity in the padding ----------------------------------------------------------
// grid = ((kp / 64) * (kp / 4), F, batch), block = (64, 4)
template <typename T>
__global__ void cv_gather_low_kernel(const T* __restrict__ A_all, long long sM, int npad, int F,
                                     const int* __restrict__ fptr, const int* __restrict__ fidx, int kp,
                                     double* __restrict__ G_all) {
  const int f = blockIdx.y, b = blockIdx.z, nx = kp / 64;
  const int j = (blockIdx.x % nx) * 64 + threadIdx.x, i = (blockIdx.x / nx) * 4 + threadIdx.y;
  if (i >= kp || j >= kp) return;
  const int k = fptr[f + 1] - fptr[f];
  const int* I = fidx + fptr[f];
  double v = i == j ? 1.0 : 0.0;
  if (i < k && j < k) {
    const int hi = max(i, j), lo = min(i, j);  // (the lower triangle, mirrored)
    v = -(double)A_all[(size_t)b * sM + (size_t)I[hi] * npad + I[lo]];
  }
  G_all[((size_t)b * F + f) * kp * kp + (size_t)i * kp + j] = v;
}

// ---- fold epilogue -------------------------------------------------------------------------------------------------
// u = Wf alpha_I (Wf = R^-1 lower triangular, kp x kp): one wave per row, lanes along the row, wave_sum.
// u_all: [(sample * F + f)][kp].   grid = (kp / 64, F, batch), 256 threads: wave w takes rows 64 bx + w, + 4, ...
__global__ __launch_bounds__(256) void cv_fold_u_kernel(const double* __restrict__ Wf_all, int kp, int F,
                                                        const int* __restrict__ fptr, const int* __restrict__ fidx,
                                                        const double* __restrict__ alpha_all, int npad,
                                                        double* __restrict__ u_all) {
  const int f = blockIdx.y, b = blockIdx.z, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k = fptr[f + 1] - fptr[f];
  const int* __restrict__ I = fidx + fptr[f];
  const double* __restrict__ Wf = Wf_all + ((size_t)b * F + f) * kp * kp;
  const double* __restrict__ alpha = alpha_all + (size_t)b * npad;
  for (int i = blockIdx.x * 64 + w; i < min(k, blockIdx.x * 64 + 64); i += 4) {
    double s = 0.0;
    for (int j = lane; j <= i; j += 64) s = fma(Wf[(size_t)i * kp + j], alpha[I[j]], s);
    s = wave_sum(s);
    if (lane == 0) u_all[((size_t)b * F + f) * kp + i] = s;
  }
}

// dmu = sc Wf^T u and s2_j = sc sum_i Wf[i][j]^2 for 64 columns of a fold; the block of the first columns also writes
// quad = sc u.u and logdet = k log sc - 2 ld (ld = the factorization's sum of log R_jj).  NaN where info != 0.
// Thread (c = t % 64, q = t / 64) sums rows j0 + q, + 4, ... of column c; the four partial sums are added in order.
// grid = (kp / 64, F, batch), 256 threads
__global__ __launch_bounds__(256) void cv_fold_out_kernel(const double* __restrict__ Wf_all, int kp, int F,
                                                          const int* __restrict__ fptr, const int* __restrict__ fidx,
                                                          const double* __restrict__ u_all, const double* __restrict__ par,
                                                          const double* __restrict__ ld, const int* __restrict__ finfo,
                                                          int npad, double* __restrict__ dmu, double* __restrict__ s2,
                                                          double* __restrict__ quad, double* __restrict__ logdet) {
  __shared__ double red[2][4][CV_T];
  __shared__ double sh4[4];
  const int f = blockIdx.y, b = blockIdx.z, t = threadIdx.x, c = t & 63, q = t >> 6;
  const int k = fptr[f + 1] - fptr[f], j0 = blockIdx.x * CV_T;
  if (j0 >= k) return;
  const size_t p = (size_t)b * F + f;
  const int* __restrict__ I = fidx + fptr[f];
  const double* __restrict__ Wf = Wf_all + p * kp * kp;
  const double* __restrict__ u = u_all + p * kp;
  const bool ok = finfo[p] == 0;
  const double sc = par[(size_t)b * BA_STRIDE + BA_LCH] != 0.0 ? par[(size_t)b * BA_STRIDE + BA_SL] : 1.0;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int j = j0 + c;
  double sm = 0.0, sv = 0.0;
  for (int i = j0 + q; i < k; i += 4) {
    const double wv = (j <= i) ? Wf[(size_t)i * kp + j] : 0.0;
    sm = fma(wv, u[i], sm);
    sv = fma(wv, wv, sv);
  }
  red[0][q][c] = sm;
  red[1][q][c] = sv;
  __syncthreads();
  if (q == 0 && j < k) {
    const double m = ((red[0][0][c] + red[0][1][c]) + red[0][2][c]) + red[0][3][c];
    const double v = ((red[1][0][c] + red[1][1][c]) + red[1][2][c]) + red[1][3][c];
    const size_t o = (size_t)b * npad + I[j];
    dmu[o] = ok ? sc * m : nan;
    s2[o] = ok ? sc * v : nan;
  }
  if (blockIdx.x == 0) {
    double s = 0.0;
    for (int i = t; i < k; i += 256) s = fma(u[i], u[i], s);
    s = block_sum_256(s, sh4);
    if (t == 0) {
      quad[p] = ok ? sc * s : nan;
      logdet[p] = ok ? (double)k * log(sc) - 2.0 * ld[p] : nan;
    }
  }
}

}  // namespace gpc
