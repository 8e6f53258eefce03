// Kernels of the block append: k new training points appended to resident posteriors in O(N^2 k)
// (gpc_post_append_block; DESIGN.md "Block posterior append").
//
// Per sample, with n old points, B = K(X_old, X_new), Knn = K(X_new, X_new), sl the fitted noise:
//   high noise (A = Lo, W = Lo^-1):  V = W B,  S = Knn / sl + I - V^T V / sl^2,  L22 = chol(S), W22 = L22^-1,
//                                    Pt = V^T W / sl,  W21 = -W22 Pt,  Lo[n + j][:n] = V[:, j] / sl
//   low noise  (A = -(K + Sigma)^-1): G = -A B,  S = Knn + sn2 I - B^T G,  Si = W22^T W22,
//                                    A <- [[A - G Si G^T, G Si], [(G Si)^T, -Si]]
// All vectors and k-wide panels are fp64 scratch whatever the storage type T of A and W; the k x k
// factorization is the library's blocked one (plan.h) in T.  Every kernel takes its samples from
// blockIdx and touches only that sample's data: the bits of a sample do not depend on the batch.
#pragma once
#include "common.h"
#include "covfun.h"

namespace gpc {

constexpr int BA_R = 16;  // right-hand sides per block of the skinny product
constexpr int BA_T = 64;  // rows / columns of the streamed matrix per tile
// k from which the two products with W run as launches of the MFMA GEMM on panels padded to 128 columns instead of
// ceil(k / 16) passes of the skinny kernel.  Measured at cfg3 (N = 4096, S = 16, fp64; tools/block_append_bench.py
// --engines, profiles/block_append_cfg3.json "engines"; rounded to 0.1 ms): device time of the two products, skinny /
// MFMA, at k = 5 and 16: 1.7 / 1.7 ms, 32: 2.5 / 1.7, 64: 4.0 / 1.7, 128: 6.9 / 1.9 -- one pass of the skinny kernel costs
// what a 128-column MFMA panel costs there, so the skinny kernel keeps exactly the batches that are ONE pass (and
// needs no panels in the storage type).  The threshold was set from this cfg3 comparison alone; fp32 storage was not
// measured separately.  (Callers learn which engine a call ran from the get-only option "block_engine_ran", not from
// this constant: tools/block_append_bench.py labels its rows with it.)
constexpr int BA_GEMM_MIN_K = BA_R + 1;
enum { BA_SL = 0, BA_SN2 = 1, BA_LCH = 2, BA_PRE = 3, BA_STRIDE = 4 };  // per-sample parameters (doubles)

// the sample's outcome, decided on the device: the host's preconditions and the Schur factorization's info
__device__ __forceinline__ bool ba_ok(const double* __restrict__ par, const int* __restrict__ info, int b) {
  return par[(size_t)b * BA_STRIDE + BA_PRE] != 0.0 && info[b] == 0;
}

// Bx[b] (npad x kq, row-major): rows i < n hold B[i][j] = k(x_i, x_{n+j}), rows n <= i < n + k hold Knn, zero
// elsewhere (columns j >= k included).  Xs: the scaled inputs, the new points are rows n .. n+k-1.
// grid = (ceil(npad * kq / 256), batch)
__global__ __launch_bounds__(256) void ba_cross_kernel(CovDesc cd, const double* __restrict__ Xs_all,
                                                       const double* __restrict__ sp_all, int n, int k, int npad,
                                                       int kq, double* __restrict__ Bx_all) {
  const int b = blockIdx.y;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)npad * kq) return;
  const int i = (int)(e / kq), j = (int)(e - (long long)i * kq);
  double v = 0.0;
  if (i < n + k && j < k) {
    const double* xi = Xs_all + ((size_t)b * npad + i) * cd.D;
    const double* xj = Xs_all + ((size_t)b * npad + n + j) * cd.D;
    double r2 = 0.0;
    for (int h = 0; h < cd.D; ++h) {
      const double d = xi[h] - xj[h];
      r2 += d * d;
    }
    const double* sp = sp_all + (size_t)b * SP_STRIDE;
    v = pair_eval(cd.kind, cd.degree, r2, sp[SP_SF2], sp[SP_RQA]).K;
  }
  Bx_all[(size_t)b * npad * kq + e] = v;
}

// Skinny product: a matrix M (R x C valid entries, leading dimension ldm, TM = the posterior's storage type or
// double) is streamed ONCE per 16 right-hand sides, a 64 x 64 tile at a time, two adjacent entries per load (16 bytes
// in fp64, 8 in fp32), against a panel X
// of BA_R columns kept in LDS.
//   TRANS = false: out[i][j] = f * sum_{l < C, (TRI: l <= i)} M[i][l] X[l][j]     i < R   (W B row-wise)
//   TRANS = true : out[l][j] = f * sum_{i < R, (TRI: i >= l)} M[i][l] X[i][j]     l < C   (V^T W column-wise)
// f = cmul, divided by par[b][BA_SL] when by_sl.  OUT_T stores out transposed (out[j][row], leading dimension ldo).
// The sum runs over the tiles in ascending order in one block: a fixed order, no atomics.  Only samples whose
// parametrisation (par[b][BA_LCH]) equals `want` are computed (want < 0: all).
// grid = (ceil(rows_out / 64), kq / 16, batch), 256 threads: thread (c = t % 64, jq = t / 64) owns out[row c][4 jq .. 4 jq + 3]
template <typename TM, bool TRANS, bool TRI, bool OUT_T>
__global__ __launch_bounds__(256) void ba_skinny_kernel(const TM* __restrict__ M_all, long long sM, int ldm, int R, int C,
                                                        const double* __restrict__ X_all, long long sX, int ldx,
                                                        double* __restrict__ out_all, long long sO, int ldo,
                                                        double cmul, int by_sl, const double* __restrict__ par,
                                                        int want) {
  __shared__ double shM[BA_T][BA_T + 1];
  __shared__ double shX[BA_T][BA_R];
  const int b = blockIdx.z;
  if (want >= 0 && (int)par[(size_t)b * BA_STRIDE + BA_LCH] != want) return;
  const TM* M = M_all + (size_t)b * sM;
  const double* X = X_all + (size_t)b * sX;
  double* out = out_all + (size_t)b * sO;
  const int t = threadIdx.x, c = t & 63, jq = t >> 6;
  const int o0 = blockIdx.x * BA_T;   // first output row of this block
  const int j0 = blockIdx.y * BA_R;   // first right-hand side
  const int Q = TRANS ? R : C;        // length of the sum
  int q_lo = 0, q_hi = Q;             // [q_lo, q_hi): the part of the sum that is not structurally zero
  if (TRI) {
    if (TRANS) q_lo = o0;
    else q_hi = min(Q, o0 + BA_T);
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int q0 = q_lo; q0 < q_hi; q0 += BA_T) {
    // tile of M: rows r0 .., columns c0 .. (as stored), two adjacent entries per load
    const int r0 = TRANS ? q0 : o0, c0 = TRANS ? o0 : q0;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int rr = (t >> 5) + 8 * p, cc = (t & 31) * 2;
      const int r = r0 + rr, cg = c0 + cc;
      double v0 = 0.0, v1 = 0.0;
      if (r < R && cg < ldm) {
        if constexpr (sizeof(TM) == 8) {
          const double2 w = *reinterpret_cast<const double2*>(M + (size_t)r * ldm + cg);
          v0 = w.x;
          v1 = w.y;
        } else {
          const float2 w = *reinterpret_cast<const float2*>(M + (size_t)r * ldm + cg);
          v0 = (double)w.x;
          v1 = (double)w.y;
        }
        if (cg >= C || (TRI && cg > r)) v0 = 0.0;
        if (cg + 1 >= C || (TRI && cg + 1 > r)) v1 = 0.0;
      }
      shM[rr][cc] = v0;
      shM[rr][cc + 1] = v1;
    }
    {
      const int rr = t >> 2, cc = (t & 3) * 4;
      const int q = q0 + rr;
      double2 a = make_double2(0.0, 0.0), d = a;
      if (q < Q) {
        const double* px = X + (size_t)q * ldx + j0 + cc;
        a = *reinterpret_cast<const double2*>(px);
        d = *reinterpret_cast<const double2*>(px + 2);
      }
      shX[rr][cc] = a.x;
      shX[rr][cc + 1] = a.y;
      shX[rr][cc + 2] = d.x;
      shX[rr][cc + 3] = d.y;
    }
    __syncthreads();
#pragma unroll 8
    for (int q = 0; q < BA_T; ++q) {
      const double m = TRANS ? shM[q][c] : shM[c][q];
      const double* x = &shX[q][jq * 4];
      acc[0] += m * x[0];
      acc[1] += m * x[1];
      acc[2] += m * x[2];
      acc[3] += m * x[3];
    }
    __syncthreads();
  }
  const int o = o0 + c;
  if (o >= (TRANS ? C : R)) return;
  double f = cmul;
  if (by_sl) f /= par[(size_t)b * BA_STRIDE + BA_SL];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = j0 + jq * 4 + e;
    if (OUT_T) out[(size_t)j * ldo + o] = f * acc[e];
    else out[(size_t)o * ldo + j] = f * acc[e];
  }
}

// ---- the padded-MFMA engine of the same two products (k above BA_GEMM_MIN_K): panels in the storage type T ----
// Bt[b] (npad x kp, zero padding) = (T) Bx[b][:n][:k]        grid = (kp / 64, npad / 4, batch), block = (64, 4)
template <typename T>
__global__ void ba_to_panel_kernel(const double* __restrict__ Bx_all, int n, int k, int kq, int npad, int kp,
                                   T* __restrict__ Bt_all) {
  const int b = blockIdx.z;
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int i = blockIdx.y * 4 + threadIdx.y;
  if (i >= npad || j >= kp) return;
  const double v = (i < n && j < k) ? Bx_all[(size_t)b * npad * kq + (size_t)i * kq + j] : 0.0;
  Bt_all[(size_t)b * npad * kp + (size_t)i * kp + j] = (T)v;
}

// Back to the fp64 panels of the rest of the pipeline, samples of parametrisation `want` only:
//   transpose = 0: out[i][j] (ld kq) = in[i][j]            i < n, j < kq       (V | G)
//   transpose = 1: out[j][i] (ld npad) = in[i][j] / sl     i < n, j < kq       (Pt)
// grid = (ceil(n / 64), kq / 4, batch), block = (64, 4): threadIdx.x runs over i (the coalesced side of Pt)
template <typename T>
__global__ void ba_from_panel_kernel(const T* __restrict__ in_all, int n, int kq, int npad, int kp, int transpose,
                                     const double* __restrict__ par, int want, double* __restrict__ out_all) {
  const int b = blockIdx.z;
  if ((int)par[(size_t)b * BA_STRIDE + BA_LCH] != want) return;
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y * 4 + threadIdx.y;
  if (i >= n || j >= kq) return;
  const double v = (double)in_all[(size_t)b * npad * kp + (size_t)i * kp + j];
  double* out = out_all + (size_t)b * npad * kq;
  if (transpose) out[(size_t)j * npad + i] = v / par[(size_t)b * BA_STRIDE + BA_SL];
  else out[(size_t)i * kq + j] = v;
}

// The Schur complement as the operand of the blocked factorization: Sc[b] (kp x kp, identity padding)
//   high noise: Knn / sl + I - C / sl^2 (C = V^T V)      low noise: Knn + sn2 I - C (C = B^T G)
// Knn = rows n .. n+k-1 of Bx; C (k x kq).  Built from the lower triangle and mirrored.
// grid = (kp / 64, kp / 4, batch), block = (64, 4)
template <typename T>
__global__ void ba_schur_kernel(const double* __restrict__ Bx_all, long long sB, int n, int k, int kq,
                                const double* __restrict__ C_all, const double* __restrict__ par, int kp,
                                T* __restrict__ Sc_all) {
  const int b = blockIdx.z;
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int i = blockIdx.y * 4 + threadIdx.y;
  if (i >= kp || j >= kp) return;
  double v = (i == j) ? 1.0 : 0.0;
  if (i < k && j < k) {
    const int hi = max(i, j), lo = min(i, j);
    const double* p = par + (size_t)b * BA_STRIDE;
    const double knn = Bx_all[(size_t)b * sB + (size_t)(n + hi) * kq + lo];
    const double cv = C_all[(size_t)b * kq * kq + (size_t)hi * kq + lo];
    if (p[BA_LCH] != 0.0) v = knn / p[BA_SL] + v - cv / (p[BA_SL] * p[BA_SL]);
    else v = knn + v * p[BA_SN2] - cv;
  }
  Sc_all[(size_t)b * kp * kp + (size_t)i * kp + j] = (T)v;
}

// e[b][j] = y_new[j] - m_star[b][j] - sum_{l < n} B[l][j] alpha[b][l]      grid = (k, batch), 256 threads
__global__ __launch_bounds__(256) void ba_innov_kernel(const double* __restrict__ Bx_all, long long sB, int n, int kq,
                                                       const double* __restrict__ alpha_all, int npad,
                                                       const double* __restrict__ y_new,
                                                       const double* __restrict__ m_star, int k,
                                                       double* __restrict__ e_all) {
  __shared__ double sh4[4];
  const int b = blockIdx.y, j = blockIdx.x;
  const double* B = Bx_all + (size_t)b * sB;
  const double* alpha = alpha_all + (size_t)b * npad;
  double s = 0.0;
  for (int l = threadIdx.x; l < n; l += 256) s += B[(size_t)l * kq + j] * alpha[l];
  s = block_sum_256(s, sh4);
  if (threadIdx.x == 0) e_all[(size_t)b * kq + j] = y_new[j] - m_star[(size_t)b * k + j] - s;
}

// t = W22 e, z = W22^T t (W22 lower triangular, kp x kp).  High noise: t = u2 and z / sl are the new alpha rows;
// low noise: z = Si e = a2.   grid = (batch), 256 threads
template <typename T>
__global__ __launch_bounds__(256) void ba_small_vec_kernel(const T* __restrict__ W22_all, int kp, int k, int kq,
                                                           const double* __restrict__ e_all,
                                                           double* t_all, double* __restrict__ z_all) {
  const int b = blockIdx.x;
  const T* W22 = W22_all + (size_t)b * kp * kp;
  const double* e = e_all + (size_t)b * kq;
  double* tv = t_all + (size_t)b * kq;
  double* z = z_all + (size_t)b * kq;
  for (int j = threadIdx.x; j < k; j += 256) {
    double s = 0.0;
    for (int i = 0; i <= j; ++i) s += (double)W22[(size_t)j * kp + i] * e[i];
    tv[j] = s;
  }
  __syncthreads();  // (one block per sample: its own global stores are visible to it after the barrier)
  for (int j = threadIdx.x; j < k; j += 256) {
    double s = 0.0;
    for (int i = j; i < k; ++i) s += (double)W22[(size_t)i * kp + j] * tv[i];
    z[j] = s;
  }
}

// High-noise placement of the k new rows of Lo (in A) and of W, samples with ba_ok only:
//   Lo[n+j][l] = V[l][j] / sl,   W[n+j][l] = -sum_{j' <= j} W22[j][j'] Pt[j'][l]        l < n
//   Lo[n+j][n+j'] = L22[j][j'],  W[n+j][n+j'] = W22[j][j']  (j' <= j), zero to the right
// grid = (npad / 256, k, batch), 256 threads
template <typename T>
__global__ __launch_bounds__(256) void ba_place_high_kernel(T* __restrict__ A_all, T* __restrict__ W_all, long long sM,
                                                            int npad, int n, int k, int kq, int kp,
                                                            const double* __restrict__ V_all,
                                                            const double* __restrict__ Pt_all,
                                                            const T* __restrict__ L22_all, const T* __restrict__ W22_all,
                                                            const double* __restrict__ par, const int* __restrict__ info) {
  const int b = blockIdx.z, j = blockIdx.y, l = blockIdx.x * 256 + threadIdx.x;
  if (l >= npad || par[(size_t)b * BA_STRIDE + BA_LCH] == 0.0 || !ba_ok(par, info, b)) return;
  const T* L22 = L22_all + (size_t)b * kp * kp;
  const T* W22 = W22_all + (size_t)b * kp * kp;
  T a = (T)0, w = (T)0;
  if (l < n) {
    const double sl = par[(size_t)b * BA_STRIDE + BA_SL];
    a = (T)(V_all[(size_t)b * npad * kq + (size_t)l * kq + j] / sl);
    const double* Pt = Pt_all + (size_t)b * npad * kq;
    double s = 0.0;
    for (int jj = 0; jj <= j; ++jj) s += (double)W22[(size_t)j * kp + jj] * Pt[(size_t)jj * npad + l];
    w = (T)(-s);
  } else if (l - n <= j) {
    a = L22[(size_t)j * kp + (l - n)];
    w = W22[(size_t)j * kp + (l - n)];
  }
  A_all[(size_t)b * sM + (size_t)(n + j) * npad + l] = a;
  W_all[(size_t)b * sM + (size_t)(n + j) * npad + l] = w;
}

// alpha of samples with ba_ok:   high noise: alpha[l] -= sum_j Pt[j][l] z[j] / sl,  alpha[n+j] = z[j] / sl
//                                low noise:  alpha[l] -= sum_j G[l][j] z[j],        alpha[n+j] = z[j]
// grid = (npad / 256, batch), 256 threads
__global__ __launch_bounds__(256) void ba_alpha_kernel(double* __restrict__ alpha_all, int npad, int n, int k, int kq,
                                                       const double* __restrict__ Pt_all,
                                                       const double* __restrict__ G_all,
                                                       const double* __restrict__ z_all,
                                                       const double* __restrict__ par, const int* __restrict__ info) {
  const int b = blockIdx.y, l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n + k || !ba_ok(par, info, b)) return;
  const bool lch = par[(size_t)b * BA_STRIDE + BA_LCH] != 0.0;
  const double f = lch ? 1.0 / par[(size_t)b * BA_STRIDE + BA_SL] : 1.0;
  const double* z = z_all + (size_t)b * kq;
  double* alpha = alpha_all + (size_t)b * npad;
  if (l >= n) {
    alpha[l] = z[l - n] * f;
    return;
  }
  double s = 0.0;
  if (lch) {
    const double* Pt = Pt_all + (size_t)b * npad * kq;
    for (int j = 0; j < k; ++j) s += Pt[(size_t)j * npad + l] * z[j];
  } else {
    const double* G = G_all + (size_t)b * npad * kq;
    for (int j = 0; j < k; ++j) s += G[(size_t)l * kq + j] * z[j];
  }
  alpha[l] -= s * f;
}

// Low noise, the two triangular products that make GS = G Si = (G W22^T) W22 (n x k panels, row-major, ld kq):
//   pass 0: out[i][m] = sum_{j <= m} in[i][j] W22[m][j]        pass 1: out[i][j] = sum_{m >= j} in[i][m] W22[m][j]
// grid = (ceil(n * k / 256), batch), 256 threads
template <typename T>
__global__ __launch_bounds__(256) void ba_panel_w22_kernel(const double* __restrict__ in_all, double* __restrict__ out_all,
                                                           long long sP, int n, int k, int kq,
                                                           const T* __restrict__ W22_all, int kp, int pass,
                                                           const double* __restrict__ par) {
  const int b = blockIdx.y;
  if (par[(size_t)b * BA_STRIDE + BA_LCH] != 0.0) return;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)n * k) return;
  const int i = (int)(e / k), j = (int)(e - (long long)i * k);
  const T* W22 = W22_all + (size_t)b * kp * kp;
  const double* in = in_all + (size_t)b * sP + (size_t)i * kq;
  double s = 0.0;
  if (pass == 0)
    for (int q = 0; q <= j; ++q) s += in[q] * (double)W22[(size_t)j * kp + q];
  else
    for (int q = j; q < k; ++q) s += in[q] * (double)W22[(size_t)q * kp + j];
  out_all[(size_t)b * sP + (size_t)i * kq + j] = s;
}

// Low-noise placement, samples with ba_ok only: the rank-k update of the FULL symmetric A = -(K + Sigma)^-1 and
// its k new rows and columns,
//   A[i][l] -= sum_j GS[i][j] G[l][j]  (i, l < n);   A[i][n+j] = A[n+j][i] = GS[i][j];   A[n+j][n+j'] = -Si[j][j']
// Si = W22^T W22.  The old part is updated with (GS[i].G[l] + GS[l].G[i]) / 2, two sums that swap roles between
// (i, l) and (l, i): A stays symmetric to the BIT however often rows are appended.  The panels of G and GS a block
// needs (64 rows for its columns, 16 for its rows) are staged in LDS, 16 columns at a time.
// grid = (ceil((n + k) / 64), ceil((n + k) / 16), batch), block = (64, 4): thread (tx, ty) owns A[i0 + 4 ty + e][l0 + tx]
template <typename T>
__global__ __launch_bounds__(256) void ba_place_low_kernel(T* __restrict__ A_all, long long sM, int npad, int n, int k,
                                                           int kq, int kp, const double* __restrict__ G_all,
                                                           const double* __restrict__ GS_all,
                                                           const T* __restrict__ W22_all,
                                                           const double* __restrict__ par, const int* __restrict__ info) {
  __shared__ double shG[64][BA_R + 1], shGS[64][BA_R + 1];  // rows l0 .. of G and GS
  __shared__ double shS[16][BA_R], shGi[16][BA_R];           // rows i0 .. of GS and G
  const int b = blockIdx.z;
  if (par[(size_t)b * BA_STRIDE + BA_LCH] != 0.0 || !ba_ok(par, info, b)) return;
  const int tx = threadIdx.x, ty = threadIdx.y, t = ty * 64 + tx;
  const int l0 = blockIdx.x * 64, i0 = blockIdx.y * 16;
  const int l = l0 + tx;
  T* A = A_all + (size_t)b * sM;
  const double* G = G_all + (size_t)b * npad * kq;
  const double* GS = GS_all + (size_t)b * npad * kq;
  const T* W22 = W22_all + (size_t)b * kp * kp;
  const int nn = n + k;
  double acc[4] = {0.0, 0.0, 0.0, 0.0}, acc2[4] = {0.0, 0.0, 0.0, 0.0};
  if (l0 < n && i0 < n) {  // (uniform per block) the block has entries of the old n x n part
    for (int j0 = 0; j0 < kq; j0 += BA_R) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int e = t + 256 * p, rr = e >> 4, cc = e & 15;
        shG[rr][cc] = (l0 + rr < n) ? G[(size_t)(l0 + rr) * kq + j0 + cc] : 0.0;
        shGS[rr][cc] = (l0 + rr < n) ? GS[(size_t)(l0 + rr) * kq + j0 + cc] : 0.0;
      }
      {
        const int rr = t >> 4, cc = t & 15;
        shS[rr][cc] = (i0 + rr < n) ? GS[(size_t)(i0 + rr) * kq + j0 + cc] : 0.0;
        shGi[rr][cc] = (i0 + rr < n) ? G[(size_t)(i0 + rr) * kq + j0 + cc] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < BA_R; ++q) {
        const double g = shG[tx][q], gs = shGS[tx][q];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[e] += shS[ty * 4 + e][q] * g;    // GS[i].G[l]
          acc2[e] += gs * shGi[ty * 4 + e][q];  // GS[l].G[i]: the same products in the same order as (l, i)'s first sum
        }
      }
      __syncthreads();
    }
  }
  if (l >= nn) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = i0 + ty * 4 + e;
    if (i >= nn) continue;
    T* p = A + (size_t)i * npad + l;
    if (i < n && l < n) {
      *p = (T)((double)*p - 0.5 * (acc[e] + acc2[e]));
    } else if (i < n) {
      *p = (T)GS[(size_t)i * kq + (l - n)];
    } else if (l < n) {
      *p = (T)GS[(size_t)l * kq + (i - n)];
    } else {
      const int ja = i - n, jb = l - n;
      double s = 0.0;
      for (int m = max(ja, jb); m < k; ++m) s += (double)W22[(size_t)m * kp + ja] * (double)W22[(size_t)m * kp + jb];
      *p = (T)(-s);
    }
  }
}

}  // namespace gpc
