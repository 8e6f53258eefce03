// nll_hess.h -- the Hessian of the negative log marginal likelihood with respect to the hyperparameters (gpc_nll_hess;
// DESIGN.md "Marginal-likelihood Hessian").
//
// Sigma = K + mult diag(sn2) at the posterior's own jitter multiplier, Q = Sigma^-1, alpha = Q (y - m),
// Qm = Q - alpha alpha^T (the weight of trace_kernel).  Every covariance and noise hyperparameter p is a PLANE with
// d_p Sigma;  B_p = Q d_p Sigma,  u_p = d_p Sigma alpha,  w_p = Q u_p,  and for mean hyperparameter k  v_k = Q d_k m:
//   H[p,q] = -1/2 tr(B_p B_q) + u_p . w_q + 1/2 <Qm, d2_pq Sigma>        planes p, q
//   H[p,k] =  w_p . d_k m                                                 plane p, mean k
//   H[k,l] =  d_k m . v_l  ( - alpha . d2_kl m: the caller's )            mean k, l
// On log scales, with the pair functor's radial factors F and G = -2 dF/d(r2) (covfun.h: pair_eval_fg_t), d_a the
// difference of the scaled coordinates in dimension a and r2 = sum_a d_a^2:
//   d K / d log ell_a = F d_a^2  (isotropic: F r2),   d K / d log sf = 2 K,   d K / d log alpha_RQ = Ka
//   ell_a x ell_b:  G d_a^2 d_b^2 - 2 delta_ab F d_a^2      (isotropic: G r2^2 - 2 F r2)
//   sf x ell_a:     2 F d_a^2         sf x sf: 4 K          sf x shape: 2 Ka
//   shape x ell_a:  Fa d_a^2,   Fa = dF / d log alpha = F (h + r2 / (2 alpha M))
//   shape x shape:  Kaa = dKa / d log alpha = K (h^2 + h + r2^2 / (4 alpha M^2))
//       (M = 1 + r2 / (2 alpha),  h = r2 / (2 M) - alpha log M,  Ka = K h)
// A pair with r2 = 0 contributes nothing to any lengthscale term (Matern 3 has G = +inf there: the term is dropped, as
// in hess.h).  The Matern kernel of degree 1 has no G (pair_eval_fg_t returns 0 for it) and F = +inf on the diagonal:
// gpc_nll_hess refuses it.
//
// The kernels below: Q as a dense symmetric matrix with zero padding (nh_form_q_kernel); one plane d_p K as a dense
// operand of the plain fp64 GEMM, with u_p and the sums <Qm, d_p K>, <Qm, second factor> fused in (nh_plane_kernel);
// the noise planes' B, a column scaling (nh_noise_plane_kernel); products with Q for a set of vectors
// (nh_matvec_kernel); the streaming Gram pass tr(B_p B_q) (nh_gram_kernel); and the contraction
// sum Qm G d_a^2 d_b^2 over the lower triangle for the ARD families (nh_d2_kernel).  Every reduction has an order fixed
// by the shape alone (per-tile partials, summed in tile order by reduce_parts_kernel / colpart_reduce_kernel): no
// atomics, the same bits for a sample in any batch or chunk.  All fp64.
#pragma once
#include "covfun.h"

namespace gpc {

enum { NH_LS = 0, NH_SF = 1, NH_SHAPE = 2 };  // what a covariance plane differentiates

constexpr int NH_LD = CT + 2;    // row stride (doubles) of the Gram kernel's transposed tile: rows stay 16-byte aligned
constexpr int NH_MAXP = 128;     // planes of one sample the Gram kernel takes
constexpr int NH_D2_MAX = 860;   // pairs (a >= b) whose per-wave sums fit beside the staged coordinates in 64 KB of LDS

inline __host__ __device__ int nh_pairs(int n) { return n * (n + 1) / 2; }

// ---------------------------------------------------------------------------------
// Q[i][j] = scale src[max(i,j)][min(i,j)] for i, j < n, 0 in the padding; scale = 1 / sl for an L_chol sample (src = the
// lower tiles of W^T W) and -1 otherwise (src = -(K + Sigma)^-1).  Read from the lower triangle alone, so Q is symmetric
// to the bit.  diagq[i] = Q_ii - alpha_i^2 (0 in the padding).
// grid = (npad^2 / 256, batch)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nh_form_q_kernel(const double* __restrict__ src_all, long long sS, int lds,
                                                        const double* __restrict__ sp_all, int lch,
                                                        const double* __restrict__ alpha_all, int n, int npad,
                                                        double* __restrict__ Q_all, long long sQ,
                                                        double* __restrict__ diagq_all) {
  const int b = blockIdx.y;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(idx / npad), j = (int)(idx % npad);
  const double scale = lch ? 1.0 / sp_all[(size_t)b * SP_STRIDE + SP_SL] : -1.0;
  double v = 0.0;
  if (i < n && j < n) {
    const int hi = i > j ? i : j, lo = i > j ? j : i;
    v = src_all[(size_t)b * sS + (size_t)hi * lds + lo] * scale;
  }
  Q_all[(size_t)b * sQ + idx] = v;
  if (i == j) {
    const double al = i < n ? alpha_all[(size_t)b * npad + i] : 0.0;
    diagq_all[(size_t)b * npad + i] = i < n ? fma(-al, al, v) : 0.0;
  }
}

// The rational quadratic's derivatives with respect to log alpha beside (K, F): Fa = dF / d log alpha and
// Kaa = dKa / d log alpha (the header's formulas)
struct PairRQ2 {
  double Fa, Kaa;
};
__device__ __forceinline__ PairRQ2 pair_rq2(double r2, double rqa, double K, double F) {
  const double Mv = fma(r2, 0.5 / rqa, 1.0);
  const double rM = rcp_fast(Mv);
  const double hr = 0.5 * r2 * rM;
  const double h = fma(-rqa, log(Mv), hr);
  PairRQ2 o;
  o.Fa = F * (h + hr / rqa);
  o.Kaa = K * fma(h, h, h + hr * hr / rqa);
  return o;
}

// ---------------------------------------------------------------------------------
// One 64 x 64 tile of the plane d_p K of sample b, written dense (zero in the padding) as the GEMM's right operand:
//   mode NH_LS:    F d_dim^2   (isotropic families: F r2; `dim` is ignored)
//   mode NH_SF:    2 K
//   mode NH_SHAPE: Ka          (rational quadratic)
// Distances as every covariance kernel forms them (tile_r2: differences before products, the same r2 to the bit); for
// D > 32 the 32-dimension chunk holding `dim` is staged again, as trace_kernel restages.  Fused in:
//   upart[b][tj][i] = sum over the tile's 64 columns j of plane_ij alpha_j      (u_p = d_p K alpha, summed over tj after)
//   gpart[b][ti * nt + tj][0] = sum_ij Qm_ij plane_ij                            (the gradient's sum)
//   gpart[b][ti * nt + tj][1] = sum_ij Qm_ij second_ij,  second = G r2^2 (NH_LS, isotropic) | Fa d_dim^2 (NH_LS, RQ)
//                                                                 | Kaa (NH_SHAPE) | 0
// grid = (npad / 64, npad / 64, batch): x = tile column tj, y = tile row ti
// ---------------------------------------------------------------------------------
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void nh_plane_kernel(CovDesc cd, const double* __restrict__ Xs_all,
                                                       const double* __restrict__ sp_all,
                                                       const double* __restrict__ alpha_all, int n, int npad, int mode,
                                                       int dim, const double* __restrict__ Q_all, long long sQ,
                                                       double* __restrict__ P_all, long long sP,
                                                       double* __restrict__ upart_all, double* __restrict__ gpart_all) {
  __shared__ double xi[CT][DCH + 1];
  __shared__ double xj[CT][DCH + 1];
  __shared__ double red[4][2];
  constexpr bool ISO = (KIND == K_SE_ISO || KIND == K_MATERN_ISO);
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, b = blockIdx.z;
  const int lane = t & 63, w = t >> 6;
  const int nt = npad / CT, D = cd.D;
  const int i0 = blockIdx.y * CT, j0 = blockIdx.x * CT;
  const double* Xs = Xs_all + (size_t)b * npad * D;
  const double* sp = sp_all + (size_t)b * SP_STRIDE;
  const double* alpha = alpha_all + (size_t)b * npad;
  const double* Q = Q_all + (size_t)b * sQ;
  double* P = P_all + (size_t)b * sP;
  double r2[4][4];
  tile_r2(r2, xi, xj, Xs, D, i0, j0, t, tx, ty);
  int hl = 0;  // `dim` within the staged chunk
  if (!ISO && mode == NH_LS) {
    const int h0 = (dim / DCH) * DCH;
    hl = dim - h0;
    if (D > DCH) {  // (block uniform)
      const int dc = min(DCH, D - h0);
      __syncthreads();
      stage_x(xi, Xs, D, i0, h0, dc, t);
      stage_x(xj, Xs, D, j0, h0, dc, t);
      __syncthreads();
    }
  }
  const double sf2 = sp[SP_SF2], rqa = sp[SP_RQA];
  ExpC ex;
  ex.load();
  double al_i[4], al_j[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    al_i[a] = alpha[i0 + ty + 16 * a];
    al_j[a] = alpha[j0 + tx + 16 * a];
  }
  double g1 = 0.0, g2 = 0.0, rs[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    rs[a] = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
      double val = 0.0, sec = 0.0;
      if (i < n && j < n) {
        const double rr = r2[a][c];
        const PairVal pv = pair_eval_t<KIND, DEG>(rr, sf2, rqa, ex);
        if (mode == NH_SF) {
          val = 2.0 * pv.K;
        } else if (mode == NH_SHAPE) {
          if constexpr (KIND == K_RQ) {
            val = pv.Ka;
            sec = pair_rq2(rr, rqa, pv.K, pv.F).Kaa;
          }
        } else if (rr > 0.0) {
          if constexpr (ISO) {
            const PairFG fg = pair_eval_fg_t<KIND, DEG>(rr, sf2, rqa, ex);
            val = pv.F * rr;
            sec = fg.G * rr * rr;
          } else {
            const double d = xi[ty + 16 * a][hl] - xj[tx + 16 * c][hl];
            const double dd = d * d;
            val = pv.F * dd;
            if constexpr (KIND == K_RQ) sec = pair_rq2(rr, rqa, pv.K, pv.F).Fa * dd;
          }
        }
        const double qm = fma(-al_i[a], al_j[c], Q[(size_t)i * npad + j]);
        g1 = fma(qm, val, g1);
        g2 = fma(qm, sec, g2);
        rs[a] = fma(val, al_j[c], rs[a]);
      }
      P[(size_t)i * npad + j] = val;
    }
  }
  // the row sums over the tile's columns: the 16 lanes of a row group, a fixed exchange order
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) rs[a] += __shfl_xor(rs[a], o, 64);
    if (tx == 0) upart_all[((size_t)b * nt + blockIdx.x) * npad + i0 + ty + 16 * a] = rs[a];
  }
  const double u = wave_sum4(g1, g2, 0.0, 0.0, lane);
  const int own = lane >> 4;
  if ((lane & 15) == 0 && own < 2) red[w][own] = u;
  __syncthreads();
  if (t < 2)
    gpart_all[(((size_t)b * nt + blockIdx.y) * nt + blockIdx.x) * 2 + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
}

// ---------------------------------------------------------------------------------
// The B plane of a noise hyperparameter, B = Q diag(e), e = mult d sn2 / d theta (zero in the padding): a column scaling,
// no product.  Row 0 of the grid also writes u = e o alpha.
// grid = (npad^2 / 256, batch)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nh_noise_plane_kernel(const double* __restrict__ Q_all, long long sQ,
                                                             const double* __restrict__ e_all,
                                                             const double* __restrict__ alpha_all, int npad,
                                                             double* __restrict__ B_all, long long sB,
                                                             double* __restrict__ u_all) {
  const int b = blockIdx.y;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(idx / npad), j = (int)(idx % npad);
  const double e = e_all[(size_t)b * npad + j];
  B_all[(size_t)b * sB + idx] = Q_all[(size_t)b * sQ + idx] * e;
  if (i == 0) u_all[(size_t)b * npad + j] = e * alpha_all[(size_t)b * npad + j];
}

// ---------------------------------------------------------------------------------
// y[v][b][i] = sum_j Q[b][i][j] x[v][b][j]: a wave per row, lanes stride the columns (coalesced), the lanes' sums added
// in wave_sum's fixed order.  grid = (npad / 4, nvec, batch)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nh_matvec_kernel(const double* __restrict__ Q_all, long long sQ, int npad,
                                                        const double* __restrict__ x_all, double* __restrict__ y_all) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + w, v = blockIdx.y, b = blockIdx.z, batch = gridDim.z;
  const double* q = Q_all + (size_t)b * sQ + (size_t)i * npad;
  const double* x = x_all + ((size_t)v * batch + b) * npad;
  double s = 0.0;
  for (int j = lane; j < npad; j += 64) s = fma(q[j], x[j], s);
  s = wave_sum(s);
  if (lane == 0) y_all[((size_t)v * batch + b) * npad + i] = s;
}

// ---------------------------------------------------------------------------------
// The streaming Gram pass: for plane p of sample b and the 64 x 64 tile pair (I, J),
//   part[b][I * nt + J][p (p + 1) / 2 + q] = sum over a in tile I, c in tile J of B_p[a][c] B_q[c][a],   q <= p,
// which summed over the tiles (reduce_parts_kernel, tile order) is tr(B_p B_q).  Tile (I, J) of B_p is read once with
// 16-byte loads and held TRANSPOSED in LDS (rows NH_LD doubles apart: every row 16-byte aligned, the stride off the 256-byte
// bank row), then the mirrored tiles (J, I) of B_0 .. B_p stream past it, each read once with 16-byte loads against
// 16-byte LDS reads of consecutive addresses.  One value per (tile, pair): the lanes' sums by wave_sum, the four
// waves in order.  HBM traffic: (p + 2) tiles per block, half of reading both tiles for every pair.
// grid = (nt^2, planes, batch)
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nh_gram_kernel(const double* __restrict__ B_all, long long sPlane,
                                                      long long sSample, int npad, int npl,
                                                      double* __restrict__ part_all) {
  __shared__ __attribute__((aligned(16))) double tl[CT][NH_LD];
  __shared__ double red[4][NH_MAXP];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int c2 = t & 31, r8 = t >> 5;
  const int nt = npad / CT, tile = blockIdx.x, I = tile / nt, J = tile % nt;
  const int p = blockIdx.y, b = blockIdx.z;
  const double* Bs = B_all + (size_t)b * sSample;
  const double* Bp = Bs + (size_t)p * sPlane;
#pragma unroll
  for (int ps = 0; ps < 8; ++ps) {
    const int row = r8 + 8 * ps;
    const double2 v = *reinterpret_cast<const double2*>(Bp + (size_t)(I * CT + row) * npad + J * CT + 2 * c2);
    tl[2 * c2][row] = v.x;
    tl[2 * c2 + 1][row] = v.y;
  }
  __syncthreads();
  for (int q = 0; q <= p; ++q) {
    const double* Bq = Bs + (size_t)q * sPlane;
    double s = 0.0;
#pragma unroll
    for (int ps = 0; ps < 8; ++ps) {
      const int row = r8 + 8 * ps;
      const double2 v = *reinterpret_cast<const double2*>(Bq + (size_t)(J * CT + row) * npad + I * CT + 2 * c2);
      const double2 m = *reinterpret_cast<const double2*>(&tl[row][2 * c2]);
      s = fma(v.x, m.x, s);
      s = fma(v.y, m.y, s);
    }
    s = wave_sum(s);
    if (lane == 0) red[w][q] = s;
  }
  __syncthreads();
  double* part = part_all + ((size_t)b * nt * nt + tile) * nh_pairs(npl) + nh_pairs(p);
  for (int q = t; q <= p; q += 256) part[q] = red[0][q] + red[1][q] + red[2][q] + red[3][q];
}

// ---------------------------------------------------------------------------------
// The second-derivative contraction of the ARD families, a sibling of trace_kernel: over the lower triangle with weight
// Qm = Q - alpha alpha^T (2 Qm off the diagonal),
//   part[b][tile][a (a + 1) / 2 + c] = sum_ij w_ij G_ij d_a^2 d_c^2,   a >= c,
// G from pair_eval_fg_t, a pair with r2 = 0 dropped.  Differences before products.  Per dimension a the 16 products
// w G d_a^2 of a thread stay in registers while c runs over 0 .. a, four sums per wave_sum4.  For D <= 32 the coordinates
// are the ones tile_r2 left in LDS; beyond, they are read from the scaled inputs directly (a path for completeness,
// not for speed).  Dynamic LDS: 4 x P4 doubles, P4 = pairs rounded up to a multiple of 4, + 4.
// grid = (lower tiles of npad / 64, batch)
// ---------------------------------------------------------------------------------
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void nh_d2_kernel(CovDesc cd, const double* __restrict__ Xs_all,
                                                    const double* __restrict__ sp_all,
                                                    const double* __restrict__ alpha_all, int n, int npad,
                                                    const double* __restrict__ Q_all, long long sQ,
                                                    double* __restrict__ part_all, int ntiles) {
  __shared__ double xi[CT][DCH + 1];
  __shared__ double xj[CT][DCH + 1];
  extern __shared__ double wpart[];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, b = blockIdx.y;
  const int lane = t & 63, w = t >> 6;
  const int D = cd.D, np = nh_pairs(D), P4 = ((np + 3) & ~3) + 4;
  int ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int i0 = ti * CT, j0 = tj * CT;
  const double* Xs = Xs_all + (size_t)b * npad * D;
  const double* sp = sp_all + (size_t)b * SP_STRIDE;
  const double* alpha = alpha_all + (size_t)b * npad;
  const double* Q = Q_all + (size_t)b * sQ;
  double r2[4][4];
  tile_r2(r2, xi, xj, Xs, D, i0, j0, t, tx, ty);
  const double sf2 = sp[SP_SF2], rqa = sp[SP_RQA];
  ExpC ex;
  ex.load();
  double gw[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
      double g = 0.0;
      if (i < n && j <= i && r2[a][c] > 0.0) {
        const double qm = fma(-alpha[i], alpha[j], Q[(size_t)i * npad + j]);
        g = (i == j ? qm : 2.0 * qm) * pair_eval_fg_t<KIND, DEG>(r2[a][c], sf2, rqa, ex).G;
      }
      gw[a][c] = g;
    }
  const bool staged = D <= DCH;
  const int own = lane >> 4;
  for (int da = 0; da < D; ++da) {
    double pa[4][4], vi[4], vj[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      vi[a] = staged ? xi[ty + 16 * a][da] : Xs[(size_t)(i0 + ty + 16 * a) * D + da];
      vj[a] = staged ? xj[tx + 16 * a][da] : Xs[(size_t)(j0 + tx + 16 * a) * D + da];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double d = vi[a] - vj[c];
        pa[a][c] = gw[a][c] * d * d;
      }
    for (int c0 = 0; c0 <= da; c0 += 4) {
      double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int dc = c0 + q;
        if (dc > da) break;  // (block uniform)
        double ui[4], uj[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          ui[a] = staged ? xi[ty + 16 * a][dc] : Xs[(size_t)(i0 + ty + 16 * a) * D + dc];
          uj[a] = staged ? xj[tx + 16 * a][dc] : Xs[(size_t)(j0 + tx + 16 * a) * D + dc];
        }
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const double d = ui[a] - uj[c];
            s = fma(pa[a][c] * d, d, s);
          }
        s4[q] = s;
      }
      const double u = wave_sum4(s4[0], s4[1], s4[2], s4[3], lane);
      if ((lane & 15) == 0 && c0 + own <= da) wpart[w * P4 + nh_pairs(da) + c0 + own] = u;
    }
  }
  __syncthreads();
  double* part = part_all + ((size_t)b * ntiles + blockIdx.x) * np;
  for (int p = t; p < np; p += 256) part[p] = wpart[p] + wpart[P4 + p] + wpart[2 * P4 + p] + wpart[3 * P4 + p];
}

}  // namespace gpc
