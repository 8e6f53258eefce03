// hess.h -- Hessians of the predictive mean and variance with respect to the query point (gpc_predict_hess; DESIGN.md
// "Predictive Hessians").
//
// With xs the scaled inputs, c_l = mul_l / dv_l, d = xs*_j - xs_i, r2 = |d|^2, F the radial factor of the pair functor
// (dk/dx*_a = -c_a F d_a) and G = -2 dF/d(r2) (covfun.h: pair_eval_fg_t),
//   d^2 k / dx*_a dx*_b = c_a c_b (G d_a d_b - F delta_ab)
// so for a weight w_ij per (training point, query) pair -- alpha_i for the mean, Q_ij = ((K + Sigma)^-1 k*_j)_i for the
// variance -- the query's Hessian term is
//   c_a c_b ( sum_i w_ij G_ij d_a d_b  -  delta_ab sum_i w_ij F_ij ).
// The kernel below forms the two sums of one 64 x 64 tile of pairs; the factors c_a c_b, the delta_ab term, the mirror
// to the upper triangle and the variance's -2 (P + .) are applied once per query by the caller.
#pragma once
#include "covfun.h"

namespace gpc {

constexpr int HCH = 8;  // dimensions per side of a block of (a, b) pairs: 2 x 8 accumulators per lane

inline __host__ __device__ int hess_pairs(int D) { return D * (D + 1) / 2; }
// planes of one weight set: [w F | w G d_a d_b at a (a + 1) / 2 + b, a >= b]
inline __host__ __device__ int hess_planes(int D) { return 1 + hess_pairs(D); }

// ---------------------------------------------------------------------------------
// The fused Hessian contraction: one 64 x 64 tile of (training point, query) pairs of sample b.  Distances are staged
// and summed as in cross_grad_tile_kernel (same r2 to the bit); F and G come from ONE pair evaluation per pair and stay
// in registers for both weight sets.  For the weight sets w = alpha_i and (WITHQ) w = qs Q_ij, in turn, it writes the
// column sums over the tile's 64 rows of
//   w F                      (plane 0 of the set), and
//   w G d_a d_b, a >= b      (plane 1 + a (a + 1) / 2 + b),
//   part[b][ti][set * hess_planes(D) + plane][j].
// colpart_reduce_kernel adds the tile rows in ascending order afterwards: no atomics, an order fixed by the shape alone.
//
// DIFFERENCES FIRST: d_a and d_b are xs*_j - xs_i, taken before any product (as grad_contract), never
// sum w x_a x_b - ...: that form cancels for inputs far from the origin.
// A pair with r2 = 0 contributes 0 to the G term (the limit: G d_a d_b -> 0 also where G is infinite, Matern 3) and its
// full F(0) to the F term -- unlike the gradient, where such a pair contributes nothing.  Rows >= n and queries >= m
// contribute 0 to both.
//
// Engine: fp64 VALU through LDS with a lane per query, as grad_contract: per pair D (D + 1) / 2 FMAs and D
// differences on top of the pair evaluation.  The weights G w of the tile lie in LDS (32 KB, overlaying the staging of
// the distances); the (a, b) pairs are worked on in blocks of HCH x HCH dimensions, block (A, B) with A >= B: the
// training coordinates of the two dimension chunks are staged (2 x 64 x 9 doubles), wave v takes rows a = v and v + 4
// of the block against all 8 columns b, a lane holds its query's 10 coordinates and 16 accumulators in registers.  The
// sets are processed in turn because two weight tiles would not fit beside the coordinates (LDS use: 43 KB + 2 KB).
// WITHQ = false (the mean alone) has no Q operand and never reads one.
// grid = (mb/64, npad/64, batch), 256 threads
// ---------------------------------------------------------------------------------
template <typename T, int KIND, int DEG, bool WITHQ>
__device__ __forceinline__ void hess_tile_body(const CovDesc& cd, const double* __restrict__ Xs_all,
                                               const double* __restrict__ Xss_all, const double* __restrict__ sp_all,
                                               const double* __restrict__ alpha_all, int astride,
                                               const T* __restrict__ Q_all, long long sQ, int ldq, int lch, int n, int npad,
                                               int m, int mb, double* __restrict__ part_all) {
  // [xi | xj] while the distances form, then [weights | xa | xb]
  __shared__ double shm[CT * CT + 2 * CT * (HCH + 1)];
  __shared__ double red[4][CT];
  static_assert(2 * CT * (DCH + 1) <= CT * CT + 2 * CT * (HCH + 1), "LDS overlay");
  double(*xi)[DCH + 1] = reinterpret_cast<double(*)[DCH + 1]>(shm);
  double(*xj)[DCH + 1] = reinterpret_cast<double(*)[DCH + 1]>(shm + CT * (DCH + 1));
  double(*wt)[CT] = reinterpret_cast<double(*)[CT]>(shm);
  double(*xa)[HCH + 1] = reinterpret_cast<double(*)[HCH + 1]>(shm + CT * CT);
  double(*xb)[HCH + 1] = reinterpret_cast<double(*)[HCH + 1]>(shm + CT * CT + CT * (HCH + 1));
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, b = blockIdx.z;
  const int lane = t & 63, w = t >> 6;
  const int D = cd.D, npl = hess_planes(D);
  const int i0 = blockIdx.y * CT, j0 = blockIdx.x * CT;
  const double* Xs = Xs_all + (size_t)b * npad * D;
  const double* Xss = Xss_all + (size_t)b * mb * D;
  const double* sp = sp_all + (size_t)b * SP_STRIDE;
  const double* alpha = alpha_all + (size_t)b * astride;
  double r2[4][4];
  tile_r2_ab(r2, xi, xj, Xs, Xss, D, i0, j0, t, tx, ty);
  const double sf2 = sp[SP_SF2], rqa = sp[SP_RQA];
  ExpC ex;
  ex.load();
  double fw[4][4], gw[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
      fw[a][c] = gw[a][c] = 0.0;
      if (i < n && j < m) {
        const PairFG pv = pair_eval_fg_t<KIND, DEG>(r2[a][c], sf2, rqa, ex);
        fw[a][c] = pv.F;
        if (r2[a][c] > 0.0) gw[a][c] = pv.G;
      }
    }
  const size_t nt = npad / CT;
  double* const part = part_all + ((size_t)b * nt + blockIdx.y) * (size_t)(WITHQ ? 2 : 1) * npl * mb;
  const int jq = j0 + lane;  // the lane's query in the contraction (a row of Xss: rows >= m are zero padding)
#pragma unroll 1
  for (int set = 0; set < (WITHQ ? 2 : 1); ++set) {
    double wv[4][4];
    if (set == 0) {
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const int i = i0 + ty + 16 * a;
        const double al = i < n ? alpha[i] : 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) wv[a][c] = al;
      }
    } else {
      if constexpr (WITHQ) {
        const T* Q = Q_all + (size_t)b * sQ;
        const double qs = lch ? 1.0 / sp[SP_SL] : -1.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
            wv[a][c] = (i < n && j < m) ? (double)Q[(size_t)i * ldq + j] * qs : 0.0;
          }
      }
    }
    double* const out = part + (size_t)set * npl * mb;
    // plane 0: the column sums of w F -- the 4 row groups of a wave by two exchanges, the 4 waves through LDS
    {
      double s[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s[c] = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) s[c] = fma(wv[a][c], fw[a][c], s[c]);
        s[c] += __shfl_xor(s[c], 16, 64);
        s[c] += __shfl_xor(s[c], 32, 64);
      }
      __syncthreads();  // xi / xj are read | the previous set has read red and the weights
      if ((lane >> 4) == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) red[w][tx + 16 * c] = s[c];
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) wt[ty + 16 * a][tx + 16 * c] = wv[a][c] * gw[a][c];
      __syncthreads();
      if (t < CT) out[j0 + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
    }
    // planes 1 ..: sum_i (w G)_i d_a d_b, blocks of HCH x HCH dimension pairs, A0 >= B0
    for (int A0 = 0; A0 < D; A0 += HCH) {
      const int da = min(HCH, D - A0);
      for (int B0 = 0; B0 <= A0; B0 += HCH) {
        const int db = min(HCH, D - B0);
        __syncthreads();  // the weights are written | the previous block has read xa / xb
        for (int e = t; e < CT * HCH; e += 256) {
          const int r = e / HCH, h = e % HCH;
          xa[r][h] = h < da ? Xs[(size_t)(i0 + r) * D + A0 + h] : 0.0;
          xb[r][h] = h < db ? Xs[(size_t)(i0 + r) * D + B0 + h] : 0.0;
        }
        __syncthreads();
        if (w >= da) continue;  // (wave uniform; the barriers are above)
        double qa[2], qb[HCH], acc[2][HCH];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int h = w + 4 * q;
          qa[q] = h < da ? Xss[(size_t)jq * D + A0 + h] : 0.0;
#pragma unroll
          for (int k = 0; k < HCH; ++k) acc[q][k] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < HCH; ++k) qb[k] = k < db ? Xss[(size_t)jq * D + B0 + k] : 0.0;
        for (int i = 0; i < CT; ++i) {
          const double p = wt[i][lane];
          double dbv[HCH];
#pragma unroll
          for (int k = 0; k < HCH; ++k) dbv[k] = qb[k] - xb[i][k];
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const double pa = p * (qa[q] - xa[i][w + 4 * q]);
#pragma unroll
            for (int k = 0; k < HCH; ++k) acc[q][k] = fma(pa, dbv[k], acc[q][k]);
          }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int k = 0; k < HCH; ++k) {
            const int a = A0 + w + 4 * q, bb = B0 + k;
            if (w + 4 * q < da && k < db && bb <= a) out[(size_t)(1 + a * (a + 1) / 2 + bb) * mb + jq] = acc[q][k];
          }
      }
    }
  }
}

// the two weight sets (alpha | Q): gpc_predict_hess with the variance
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void hess_tile_kernel(CovDesc cd, const double* __restrict__ Xs_all,
                                                        const double* __restrict__ Xss_all,
                                                        const double* __restrict__ sp_all,
                                                        const double* __restrict__ alpha_all, int astride,
                                                        const T* __restrict__ Q_all, long long sQ, int ldq, int lch, int n,
                                                        int npad, int m, int mb, double* __restrict__ part_all) {
  hess_tile_body<T, KIND, DEG, true>(cd, Xs_all, Xss_all, sp_all, alpha_all, astride, Q_all, sQ, ldq, lch, n, npad, m, mb,
                                     part_all);
}
// the mean alone: no Q operand
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void hess_tile_mean_kernel(CovDesc cd, const double* __restrict__ Xs_all,
                                                             const double* __restrict__ Xss_all,
                                                             const double* __restrict__ sp_all,
                                                             const double* __restrict__ alpha_all, int astride, int n,
                                                             int npad, int m, int mb, double* __restrict__ part_all) {
  hess_tile_body<T, KIND, DEG, false>(cd, Xs_all, Xss_all, sp_all, alpha_all, astride, (const T*)nullptr, 0LL, 0, 0, n, npad,
                                      m, mb, part_all);
}

// One query's Hessian from its reduced sums `sums` (planes of hess_planes(D), mb apart, at column jj), both triangles
// from the one lower entry: H[a][b] = c_a c_b (sums[1 + a (a + 1) / 2 + b] - delta_ab sums[0])
inline void hess_assemble(const double* sums, int mb, int jj, int D, const double* c, double* H) {
  const double f = sums[jj];
  for (int a = 0; a < D; ++a)
    for (int b = 0; b <= a; ++b) {
      const double v = c[a] * c[b] * (sums[(size_t)(1 + a * (a + 1) / 2 + b) * mb + jj] - (a == b ? f : 0.0));
      H[(size_t)a * D + b] = H[(size_t)b * D + a] = v;
    }
}

}  // namespace gpc
