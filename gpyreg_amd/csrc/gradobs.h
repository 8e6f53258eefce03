// gradobs.h -- gradient observations: the joint covariance of values and gradients, and its cross operand for
// queries (gpc_posterior_batch_gobs / gpc_nll_batch_gobs / gpc_predict_gobs; DESIGN.md "Gradient observations").
//
// Data: values at X (N x D) and gradients at X_g (Ng x D).  With xs the scaled inputs (scale_x_kernel),
// c_l = mul_l / dv_l, and for a pair (p, q) d = xs_p - xs_q, r2 = |d|^2 and (k, F, G) the pair functor's value and
// radial factors at r2 (covfun.h: pair_eval_t, pair_eval_fg_t):
//   cov(f(x_p), f(x_q))         = k
//   cov(d_a f(x_p), f(x_q))     = -c_a F d_a                          (0 at r2 = 0)
//   cov(d_a f(x_p), d_b f(x_q)) = c_a c_b (F delta_ab - G d_a d_b)    (c_a^2 F0 delta_ab at r2 = 0: hess.h's convention)
//
// JOINT ORDER.  n = N + Ng D rows: the values first, then the gradient rows DIMENSION-MAJOR, row N + l Ng + g =
// d_l f(X_g[g]).  Reason (as gradpost.h's slot-major planes): in both kernels a lane is a point, so for a fixed pair of
// dimensions a wave writes consecutive addresses; with (point, dimension) interleaved its stores would be D apart.
//
// POINT LIST.  Both kernels read ONE list of scaled points, P = pad64(N) + pad64(Ng) rows: X in rows [0, N), X_g in
// rows [pad64(N), pad64(N) + Ng), zero rows between.  A 64-tile of the list is therefore of one kind -- value points
// or gradient points -- and the kind is uniform per block.
#pragma once
#include "covfun.h"

namespace gpc {

struct GobsDims {
  int N = 0, Ng = 0, D = 0;
  __host__ __device__ int Np() const { return (N + CT - 1) / CT * CT; }
  __host__ __device__ int Ngp() const { return (Ng + CT - 1) / CT * CT; }
  __host__ __device__ int P() const { return Np() + Ngp(); }  // rows of the point list
  __host__ __device__ long long n() const { return (long long)N + (long long)Ng * D; }  // joint order
};

// ---------------------------------------------------------------------------------
// The joint covariance: one 64 x 64 tile of pairs of the point list, every entry those pairs own -- 1 (value, value),
// D (gradient, value | value, gradient) or D^2 (gradient, gradient) per pair -- into the dense n x n fp64 matrix `out`
// (leading dimension n: what load_K_kernel reads).  (k, F, G) are evaluated once per pair; distances by tile_r2_ab
// (the same r2 bits as every other covariance kernel), differences before products.
// The grid is the FULL square of tiles, not a triangle: block (ti, tj) writes its own entries with lanes along the
// columns, so every store is a run of consecutive addresses (the mirrored entries of a triangle's block would be n
// doubles apart per lane).  The matrix is still symmetric to the bit: block (tj, ti) sees d -> -d exactly, so r2, k, F,
// G and d_a d_b carry the same bits, and F d_a only flips its sign.
// Gradient / gradient tiles stage the a-dimensions DCH at a time (xi, xj) and ONE b-dimension at a time (bi, bj): any D
// is served within the LDS of the sibling kernels.
// grid = (P/64, P/64), 256 threads
// ---------------------------------------------------------------------------------
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void gobs_cov_kernel(GobsDims gd, const double* __restrict__ Xs,
                                                       const double* __restrict__ sp, const double* __restrict__ mul,
                                                       const double* __restrict__ dv, T* __restrict__ out) {
  __shared__ double xi[CT][DCH + 1];
  __shared__ double xj[CT][DCH + 1];
  __shared__ double bi[CT], bj[CT];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int N = gd.N, Ng = gd.Ng, D = gd.D, Np = gd.Np();
  const size_t n = (size_t)gd.n();
  const int i0 = blockIdx.y * CT, j0 = blockIdx.x * CT;  // rows of the point list
  const bool gi = i0 >= Np, gj = j0 >= Np;                // gradient points?
  const int pi0 = gi ? i0 - Np : i0, ni = gi ? Ng : N;    // first point of the tile within its kind, points of the kind
  const int pj0 = gj ? j0 - Np : j0, nj = gj ? Ng : N;
  double r2[4][4];
  tile_r2_ab(r2, xi, xj, Xs, Xs, D, i0, j0, t, tx, ty);
  const double sf2 = sp[SP_SF2], rqa = sp[SP_RQA];
  ExpC ex;
  ex.load();
  bool ok[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) ok[a][c] = (pi0 + ty + 16 * a) < ni && (pj0 + tx + 16 * c) < nj;

  if (!gi && !gj) {  // value / value
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (ok[a][c])
          out[(size_t)(pi0 + ty + 16 * a) * n + (pj0 + tx + 16 * c)] = (T)pair_eval_t<KIND, DEG>(r2[a][c], sf2, rqa, ex).K;
    return;
  }
  double f[4][4], g[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const PairFG fg = pair_eval_fg_t<KIND, DEG>(r2[a][c], sf2, rqa, ex);
      f[a][c] = fg.F;
      g[a][c] = r2[a][c] > 0.0 ? fg.G : 0.0;  // the G term is dropped at coincident points (Matern 3: G = inf there)
    }

  if (gi != gj) {  // gradient / value (rows N + l Ng + p, column q) | value / gradient (row p, columns N + l Ng + q)
    for (int h0 = 0; h0 < D; h0 += DCH) {
      const int dc = min(DCH, D - h0);
      __syncthreads();
      stage_x(xi, Xs, D, i0, h0, dc, t);
      stage_x(xj, Xs, D, j0, h0, dc, t);
      __syncthreads();
      for (int h = 0; h < dc; ++h) {
        const int l = h0 + h;
        const double cl = mul[l] / dv[l];
        double vi[4], vj[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) vi[a] = xi[ty + 16 * a][h];
#pragma unroll
        for (int c = 0; c < 4; ++c) vj[c] = xj[tx + 16 * c][h];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (!ok[a][c]) continue;
            const int p = pi0 + ty + 16 * a, q = pj0 + tx + 16 * c;
            const double w = (cl * f[a][c]) * (vi[a] - vj[c]);  // c_l F (xs_p - xs_q)_l
            // the derivative is taken at the row's point (gi) or at the column's (gj): -w | +w; exactly 0 at r2 = 0
            const double v = r2[a][c] > 0.0 ? (gi ? -w : w) : 0.0;
            const size_t row = gi ? (size_t)N + (size_t)l * Ng + p : (size_t)p;
            const size_t col = gj ? (size_t)N + (size_t)l * Ng + q : (size_t)q;
            out[row * n + col] = (T)v;
          }
      }
    }
    return;
  }

  // gradient / gradient: rows N + la Ng + p, columns N + lb Ng + q
  for (int h0 = 0; h0 < D; h0 += DCH) {
    const int dc = min(DCH, D - h0);
    __syncthreads();
    stage_x(xi, Xs, D, i0, h0, dc, t);
    stage_x(xj, Xs, D, j0, h0, dc, t);
    for (int lb = 0; lb < D; ++lb) {
      __syncthreads();  // (the a-chunk above is staged; the previous lb's readers are done)
      if (t < CT)
        bi[t] = Xs[(size_t)(i0 + t) * D + lb];
      else if (t < 2 * CT)
        bj[t - CT] = Xs[(size_t)(j0 + t - CT) * D + lb];
      __syncthreads();
      const double cb = mul[lb] / dv[lb];
      double db[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) db[a][c] = bi[ty + 16 * a] - bj[tx + 16 * c];
      for (int h = 0; h < dc; ++h) {
        const int la = h0 + h;
        const double cab = (mul[la] / dv[la]) * cb;
        double vi[4], vj[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) vi[a] = xi[ty + 16 * a][h];
#pragma unroll
        for (int c = 0; c < 4; ++c) vj[c] = xj[tx + 16 * c][h];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (!ok[a][c]) continue;
            const int p = pi0 + ty + 16 * a, q = pj0 + tx + 16 * c;
            const double dd = (vi[a] - vj[c]) * db[a][c];
            const double v = cab * fma(-g[a][c], dd, la == lb ? f[a][c] : 0.0);
            out[((size_t)N + (size_t)la * Ng + p) * n + ((size_t)N + (size_t)lb * Ng + q)] = (T)v;
          }
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// The joint cross operand: one 64 x 64 tile of (point of the list, query) pairs of sample b, the rows of the n x M
// operand those pairs own -- k(X_i, x*_j) in row i for a value tile; -c_l F (xs_g - xs*_j)_l in rows N + l Ng + g,
// l < D, for a gradient tile (0 at r2 = 0) -- into the panel Ks[b] (npad x mb, leading dimension mb).  Queries >= m are
// written as zeros; the rows [n, npad) belong to no tile and are zeroed by the launcher.
// Fused mean product, as cross_tile_kernel's mupart: part[b][tile row][j] = sum over every row the tile wrote of the
// STORED value times alpha[row] (dimensions ascending, then the tile's points); colpart_reduce_kernel adds the tile
// rows in ascending order.  No atomics.
// grid = (mb/64, P/64, batch), 256 threads.  Xp: batch lists of P x D; Xss: batch x mb x D
// ---------------------------------------------------------------------------------
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void gobs_cross_tile_kernel(
    GobsDims gd, const double* __restrict__ Xp_all, const double* __restrict__ Xss_all,
    const double* __restrict__ sp_all, const double* __restrict__ mul_all, const double* __restrict__ dv_all,
    const double* __restrict__ alpha_all, int astride, int m, int mb, T* __restrict__ Ks_all, long long sKs,
    double* __restrict__ part_all) {
  __shared__ double xi[CT][DCH + 1];
  __shared__ double xj[CT][DCH + 1];
  __shared__ double red[4][CT];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, b = blockIdx.z;
  const int lane = t & 63, w = t >> 6;
  const int N = gd.N, Ng = gd.Ng, D = gd.D, Np = gd.Np(), P = gd.P();
  const int i0 = blockIdx.y * CT, j0 = blockIdx.x * CT;
  const bool gi = i0 >= Np;
  const int pi0 = gi ? i0 - Np : i0, ni = gi ? Ng : N;
  const double* Xp = Xp_all + (size_t)b * P * D;
  const double* Xss = Xss_all + (size_t)b * mb * D;
  const double* sp = sp_all + (size_t)b * SP_STRIDE;
  const double* mul = mul_all + (size_t)b * D;
  const double* dv = dv_all + (size_t)b * D;
  const double* alpha = alpha_all + (size_t)b * astride;
  T* Ks = Ks_all + (size_t)b * sKs;
  double r2[4][4];
  tile_r2_ab(r2, xi, xj, Xp, Xss, D, i0, j0, t, tx, ty);
  const double sf2 = sp[SP_SF2], rqa = sp[SP_RQA];
  ExpC ex;
  ex.load();
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (!gi) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int i = pi0 + ty + 16 * a;
      if (i >= ni) continue;
      const double al = alpha[i];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + tx + 16 * c;
        const T vt = (T)(j < m ? pair_eval_t<KIND, DEG>(r2[a][c], sf2, rqa, ex).K : 0.0);
        Ks[(size_t)i * mb + j] = vt;
        s[c] = fma((double)vt, al, s[c]);
      }
    }
  } else {
    double fw[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool live = (pi0 + ty + 16 * a) < ni && (j0 + tx + 16 * c) < m && r2[a][c] > 0.0;
        fw[a][c] = live ? pair_eval_t<KIND, DEG>(r2[a][c], sf2, rqa, ex).F : 0.0;
      }
    for (int h0 = 0; h0 < D; h0 += DCH) {
      const int dc = min(DCH, D - h0);
      __syncthreads();
      stage_x(xi, Xp, D, i0, h0, dc, t);
      stage_x(xj, Xss, D, j0, h0, dc, t);
      __syncthreads();
      for (int h = 0; h < dc; ++h) {
        const int l = h0 + h;
        const double cl = mul[l] / dv[l];
        double vi[4], vj[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) vi[a] = xi[ty + 16 * a][h];
#pragma unroll
        for (int c = 0; c < 4; ++c) vj[c] = xj[tx + 16 * c][h];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int p = pi0 + ty + 16 * a;
          if (p >= ni) continue;
          const size_t row = (size_t)N + (size_t)l * Ng + p;
          const double al = alpha[row];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const double wv = (cl * fw[a][c]) * (vi[a] - vj[c]);
            const T vt = (T)(fw[a][c] != 0.0 ? -wv : 0.0);
            Ks[row * mb + j0 + tx + 16 * c] = vt;
            s[c] = fma((double)vt, al, s[c]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    s[c] += __shfl_xor(s[c], 16, 64);
    s[c] += __shfl_xor(s[c], 32, 64);
  }
  if ((lane >> 4) == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) red[w][tx + 16 * c] = s[c];
  }
  __syncthreads();
  if (t < CT) part_all[((size_t)b * (P / CT) + blockIdx.y) * mb + j0 + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
}

// The scaled point lists of `batch` samples from the raw list `pts` (P x D, zero rows between the kinds)
inline void launch_gobs_scale(hipStream_t st, const GobsDims& gd, const double* pts, const double* mul, const double* dv,
                              int batch, double* xs) {
  const long long tot = (long long)gd.P() * gd.D;
  hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)((tot + 255) / 256), batch), dim3(256), 0, st, pts, gd.P(), gd.P(), gd.D,
                     mul, dv, xs);
}

// The joint covariance of ONE sample into `out` (n x n doubles) from its scaled point list
inline void launch_gobs_cov(hipStream_t st, const CovDesc& cd, const GobsDims& gd, const double* xs, const double* sp,
                            const double* mul, const double* dv, double* out) {
  const int pt = gd.P() / CT;
  GPC_COV_DISPATCH(gobs_cov_kernel, double, cd, dim3(pt, pt), dim3(256), 0, st, gd, xs, sp, mul, dv, out);
}

// The cross operands of `batch` samples (panels sKs apart, npad x mb) with their mean products: part: batch x P/64 x mb
// partials, mu: batch x mb.  The rows [n, npad) of every panel are zeroed here.
template <typename T>
inline hipError_t launch_gobs_cross(hipStream_t st, const CovDesc& cd, const GobsDims& gd, const double* xp,
                                    const double* xss, const double* sp, const double* mul, const double* dv,
                                    const double* alpha, int astride, int npad, int m, int mb, int batch, T* Ks,
                                    long long sKs, double* part, double* mu) {
  const size_t n = (size_t)gd.n();
  if ((size_t)npad > n) {
    hipError_t e = hipMemset2DAsync(Ks + n * mb, (size_t)sKs * sizeof(T), 0, ((size_t)npad - n) * mb * sizeof(T), batch, st);
    if (e != hipSuccess) return e;
  }
  GPC_COV_DISPATCH(gobs_cross_tile_kernel, T, cd, dim3(mb / CT, gd.P() / CT, batch), dim3(256), 0, st, gd, xp, xss, sp, mul,
                   dv, alpha, astride, m, mb, Ks, sKs, part);
  hipLaunchKernelGGL(colpart_reduce_kernel, dim3((mb + 255) / 256, batch), dim3(256), 0, st, (const double*)part,
                     gd.P() / CT, mb, mu);
  return hipGetLastError();
}

}  // namespace gpc
