// hypgrad.h -- derivatives of the latent predictive mean and variance with respect to the hyperparameters
// (gpc_predict_hyp_grad; DESIGN.md "Hyperparameter gradients of predictions").
//
// Sigma = K + mult diag(sn2) at the posterior's own jitter multiplier (held fixed), Q = Sigma^-1, alpha = Q (y - m);
// for query j: k_j = k(X, x*_j), q_j = Q k_j, fmu_j = k_j . alpha, fs2_j = k** - k_j . q_j.  Hyperparameters ordered
// [cov | noise | mean], P of them.  Every hyperparameter p has a weight vector w_p (N entries):
//   lengthscale, RQ shape   w_p = Q (d_p K alpha)
//   log sf                  w_p = 2 alpha - 2 mult Q (sn2 o alpha)      (= Q (2 K alpha): no plane)
//   noise n                 w_p = mult Q (dsn2_n o alpha)
//   mean k                  w_p = Q d_k m
// and, with d_p k_ij the cross plane (F d_a^2 | F r2 | 2 k | Ka, as nll_hess.h),
//   dfmu_j / dtheta_p = sum_i d_p k_ij alpha_i - sum_i k_ij w_p,i             (first sum: covariance p only)
//   dfs2_j / dtheta_p = -2 sum_i d_p k_ij q_ij + q_j^T (d_p K) q_j            lengthscale, RQ shape
//                     = 2 fs2_j - 2 mult sum_i sn2_i q_ij^2                   log sf
//                     = mult sum_i dsn2_n,i q_ij^2                            noise n;     0 for a mean hyperparameter
// A pair with r2 = 0 contributes 0 to a lengthscale term.  The Matern kernel of degree 1 (F infinite on the diagonal)
// is refused by the caller.
//
// The kernels below: one plane d_p K with u_p = d_p K alpha fused in (hg_plane_kernel: nh_plane_kernel without its Q
// sums; the dense plane only when the variance is wanted); the vectors' elementwise steps; the fused cross pass over
// (training point, query) tiles (hg_cross_kernel); and the streaming column dots of the quadratic forms
// (hg_coldot_kernel).  Every reduction has an order fixed by the shape alone (per-tile partials, summed in tile order by
// colpart_reduce_kernel): no atomics, the same bits for a sample in any batch, chunk or rank.  All fp64.
#pragma once
#include "covfun.h"
#include "nll_hess.h"

namespace gpc {

// sums of one (query, sample) the cross pass leaves: [B_p, p < P | A_c, c < cov_N | C_c, c < cov_N (with Q)]
inline __host__ __device__ int hg_cross_sums(int P, int cov_N, bool withq) { return P + cov_N * (withq ? 2 : 1); }
// the column of log sf among the covariance hyperparameters
inline __host__ __device__ int hg_sf_col(const CovDesc& cd) { return cov_is_iso(cd.kind) ? 1 : cd.D; }

// ---------------------------------------------------------------------------------
// One 64 x 64 tile of the plane d_p K of sample b (mode NH_LS: F d_dim^2, isotropic F r2; NH_SHAPE: Ka), as
// nh_plane_kernel forms it (tile_r2: the library's distances to the bit), with
//   upart[b][tj][i] = sum over the tile's 64 columns j of plane_ij alpha_j
// fused in.  P_all != nullptr: the plane is also written dense (zero in the padding), the GEMM's left operand.
// grid = (npad / 64, npad / 64, batch): x = tile column tj, y = tile row ti
// ---------------------------------------------------------------------------------
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void hg_plane_kernel(CovDesc cd, const double* __restrict__ Xs_all,
                                                       const double* __restrict__ sp_all,
                                                       const double* __restrict__ alpha_all, int n, int npad, int mode,
                                                       int dim, double* __restrict__ P_all, long long sP,
                                                       double* __restrict__ upart_all) {
  __shared__ double xi[CT][DCH + 1];
  __shared__ double xj[CT][DCH + 1];
  constexpr bool ISO = (KIND == K_SE_ISO || KIND == K_MATERN_ISO);
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, b = blockIdx.z;
  const int nt = npad / CT, D = cd.D;
  const int i0 = blockIdx.y * CT, j0 = blockIdx.x * CT;
  const double* Xs = Xs_all + (size_t)b * npad * D;
  const double* sp = sp_all + (size_t)b * SP_STRIDE;
  const double* alpha = alpha_all + (size_t)b * npad;
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
  double al_j[4], rs[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) al_j[c] = (j0 + tx + 16 * c) < n ? alpha[j0 + tx + 16 * c] : 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    rs[a] = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
      double val = 0.0;
      if (i < n && j < n) {
        const double rr = r2[a][c];
        const PairVal pv = pair_eval_t<KIND, DEG>(rr, sf2, rqa, ex);
        if (mode == NH_SHAPE) {
          val = pv.Ka;
        } else if (rr > 0.0) {
          if constexpr (ISO) {
            val = pv.F * rr;
          } else {
            const double d = xi[ty + 16 * a][hl] - xj[tx + 16 * c][hl];
            val = pv.F * (d * d);
          }
        }
        rs[a] = fma(val, al_j[c], rs[a]);
      }
      if (P_all) P_all[(size_t)b * sP + (size_t)i * npad + j] = val;
    }
  }
  // the row sums over the tile's columns: the 16 lanes of a row group, a fixed exchange order
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) rs[a] += __shfl_xor(rs[a], o, 64);
    if (tx == 0) upart_all[((size_t)b * nt + blockIdx.x) * npad + i0 + ty + 16 * a] = rs[a];
  }
}

// x[v][b][i] *= alpha[b][i] for the vectors v of the launch (e o alpha: the noise columns and log sf's).
// grid = (ceil(npad / 256), nvec, batch)
__global__ __launch_bounds__(256) void hg_mul_alpha_kernel(double* __restrict__ x_all, const double* __restrict__ alpha_all,
                                                           int npad) {
  const int i = blockIdx.x * 256 + threadIdx.x, v = blockIdx.y, b = blockIdx.z, batch = gridDim.z;
  if (i >= npad) return;
  x_all[((size_t)v * batch + b) * npad + i] *= alpha_all[(size_t)b * npad + i];
}

// log sf's weight from y = mult Q (sn2 o alpha): w[b][i] = 2 alpha[b][i] - 2 y[b][i].  grid = (ceil(npad / 256), batch)
__global__ __launch_bounds__(256) void hg_sf_weight_kernel(double* __restrict__ w_all, const double* __restrict__ alpha_all,
                                                           int npad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  const size_t e = (size_t)blockIdx.y * npad + i;
  w_all[e] = 2.0 * alpha_all[e] - 2.0 * w_all[e];
}

// ---------------------------------------------------------------------------------
// The fused cross pass: one 64 x 64 tile of (training point, query) pairs of sample b.  Distances are staged and summed
// as in cross_tile_kernel (the same r2 and K to the bit); K, F and (rational quadratic) Ka come from ONE pair
// evaluation per pair.  With q_ij = qs[b] Q[b][i][j] (WITHQ) the tile's column sums over its 64 rows of
//   B_p = k_ij w_p,i                         p < P                         part[b][ti][p][j]
//   A_c = d_c k_ij alpha_i                   c < cov_N                     part[b][ti][P + c][j]
//   C_c = d_c k_ij q_ij                      c < cov_N  (WITHQ)            part[b][ti][P + cov_N + c][j]
// are written, the cross plane d_c k being F d_a^2 (lengthscale a; isotropic F r2), k ITSELF for log sf (the caller
// doubles it: A_sf = fmu, C_sf = k_j . q_j) and Ka for the RQ shape.  colpart_reduce_kernel adds the tile rows in
// ascending order afterwards.
//
// DIFFERENCES FIRST: d_a = xs*_ja - xs_ia, taken before any product.  A pair with r2 = 0 contributes 0 to a
// lengthscale sum.  Rows >= n and queries >= m contribute 0 to every sum.
//
// Engine: fp64 VALU through LDS with a lane per query, as hess_tile_kernel: the tile of K, then of F (F r2), then of Ka
// lies in LDS (32 KB, overlaying the staging of the distances); a wave takes every fourth sum of a phase and adds its
// 64 rows in ascending order, the row's weight (w_p,i, alpha_i, a training coordinate) a broadcast load, q_ij a
// coalesced one.  WITHQ = false (the mean alone) has no Q operand and never reads one: its A and B sums are the same
// instructions on the same operands, the same bits.
// grid = (mpad/64, npad/64, batch), 256 threads
// ---------------------------------------------------------------------------------
template <typename T, int KIND, int DEG, bool WITHQ>
__device__ __forceinline__ void hg_cross_body(const CovDesc& cd, const double* __restrict__ Xs_all,
                                              const double* __restrict__ Xss_all, const double* __restrict__ sp_all,
                                              const double* __restrict__ alpha_all, const double* __restrict__ W_all, int P,
                                              const double* __restrict__ Q_all, long long sQ, int ldq,
                                              const double* __restrict__ qs_all, int n, int npad, int m, int mpad,
                                              double* __restrict__ part_all) {
  constexpr int STG = 2 * CT * (DCH + 1);
  __shared__ double shm[STG > CT * CT ? STG : CT * CT];  // [xi | xj] while the distances form, then the tile
  constexpr bool ISO = (KIND == K_SE_ISO || KIND == K_MATERN_ISO);
  double(*xi)[DCH + 1] = reinterpret_cast<double(*)[DCH + 1]>(shm);
  double(*xj)[DCH + 1] = reinterpret_cast<double(*)[DCH + 1]>(shm + CT * (DCH + 1));
  double(*tk)[CT] = reinterpret_cast<double(*)[CT]>(shm);
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, b = blockIdx.z, batch = gridDim.z;
  const int lane = t & 63, w = t >> 6;
  const int D = cd.D, cov_N = cd.cov_N, nout = hg_cross_sums(P, cov_N, WITHQ), sfc = hg_sf_col(cd);
  const int i0 = blockIdx.y * CT, j0 = blockIdx.x * CT;
  const double* Xs = Xs_all + (size_t)b * npad * D;
  const double* Xss = Xss_all + (size_t)b * mpad * D;
  const double* sp = sp_all + (size_t)b * SP_STRIDE;
  const double* alpha = alpha_all + (size_t)b * npad;
  double r2[4][4];
  tile_r2_ab(r2, xi, xj, Xs, Xss, D, i0, j0, t, tx, ty);
  const double sf2 = sp[SP_SF2], rqa = sp[SP_RQA];
  ExpC ex;
  ex.load();
  double kv[4][4], fv[4][4], av[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
      kv[a][c] = fv[a][c] = av[a][c] = 0.0;
      if (i < n && j < m) {
        const PairVal pv = pair_eval_t<KIND, DEG>(r2[a][c], sf2, rqa, ex);
        kv[a][c] = pv.K;
        av[a][c] = pv.Ka;
        if (r2[a][c] > 0.0) fv[a][c] = ISO ? pv.F * r2[a][c] : pv.F;
      }
    }
  const int rows = min(CT, n - i0);  // (<= 0 for a tile row of padding: every sum is 0)
  const int jq = j0 + lane;          // the lane's query (a row of Xss: rows >= m are zero padding)
  double* const out = part_all + ((size_t)b * (npad / CT) + blockIdx.y) * (size_t)nout * mpad;
  const double* q = nullptr;
  double qs = 0.0;
  if constexpr (WITHQ) {
    q = Q_all + (size_t)b * sQ + (size_t)i0 * ldq + jq;
    qs = qs_all[b];
  }
  // sums of the tile against alpha and q: column c of the A and C sums
  auto plain = [&](int c) {
    double sa = 0.0, sc = 0.0;
    for (int i = 0; i < rows; ++i) {
      const double v = tk[i][lane];
      sa = fma(v, alpha[i0 + i], sa);
      if constexpr (WITHQ) sc = fma(v, qs * q[(size_t)i * ldq], sc);
    }
    out[(size_t)(P + c) * mpad + jq] = sa;
    if constexpr (WITHQ) out[(size_t)(P + cov_N + c) * mpad + jq] = sc;
  };
  // phase 1: the tile of K -- the P sums B_p and log sf's column
  __syncthreads();  // xi / xj are read
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) tk[ty + 16 * a][tx + 16 * c] = kv[a][c];
  __syncthreads();
  for (int u = w; u <= P; u += 4) {  // (wave uniform)
    if (u == P) {
      plain(sfc);
      continue;
    }
    const double* wp = W_all + ((size_t)u * batch + b) * npad + i0;
    double s = 0.0;
    for (int i = 0; i < rows; ++i) s = fma(tk[i][lane], wp[i], s);
    out[(size_t)u * mpad + jq] = s;
  }
  // phase 2: the tile of F (isotropic: F r2) -- the lengthscale columns
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) tk[ty + 16 * a][tx + 16 * c] = fv[a][c];
  __syncthreads();
  if constexpr (ISO) {
    if (w == 0) plain(0);
  } else {
    for (int a = w; a < D; a += 4) {
      const double xq = Xss[(size_t)jq * D + a];
      double sa = 0.0, sc = 0.0;
      for (int i = 0; i < rows; ++i) {
        const double d = xq - Xs[(size_t)(i0 + i) * D + a];
        const double fd = tk[i][lane] * (d * d);
        sa = fma(fd, alpha[i0 + i], sa);
        if constexpr (WITHQ) sc = fma(fd, qs * q[(size_t)i * ldq], sc);
      }
      out[(size_t)(P + a) * mpad + jq] = sa;
      if constexpr (WITHQ) out[(size_t)(P + cov_N + a) * mpad + jq] = sc;
    }
  }
  // phase 3 (rational quadratic): the tile of Ka -- the shape column
  if constexpr (KIND == K_RQ) {
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) tk[ty + 16 * a][tx + 16 * c] = av[a][c];
    __syncthreads();
    if (w == 0) plain(D + 1);
  }
}

// with the variance: the sums against Q too
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void hg_cross_kernel(CovDesc cd, const double* __restrict__ Xs_all,
                                                       const double* __restrict__ Xss_all,
                                                       const double* __restrict__ sp_all,
                                                       const double* __restrict__ alpha_all,
                                                       const double* __restrict__ W_all, int P,
                                                       const double* __restrict__ Q_all, long long sQ, int ldq,
                                                       const double* __restrict__ qs_all, int n, int npad, int m, int mpad,
                                                       double* __restrict__ part_all) {
  hg_cross_body<T, KIND, DEG, true>(cd, Xs_all, Xss_all, sp_all, alpha_all, W_all, P, Q_all, sQ, ldq, qs_all, n, npad, m,
                                    mpad, part_all);
}
// the mean alone: no Q operand
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void hg_cross_mean_kernel(CovDesc cd, const double* __restrict__ Xs_all,
                                                            const double* __restrict__ Xss_all,
                                                            const double* __restrict__ sp_all,
                                                            const double* __restrict__ alpha_all,
                                                            const double* __restrict__ W_all, int P, int n, int npad, int m,
                                                            int mpad, double* __restrict__ part_all) {
  hg_cross_body<T, KIND, DEG, false>(cd, Xs_all, Xss_all, sp_all, alpha_all, W_all, P, nullptr, 0LL, 0, nullptr, n, npad,
                                     m, mpad, part_all);
}

// ---------------------------------------------------------------------------------
// The streaming column dots of the quadratic forms: for the 64-row segment `seg` of sample b and the stored panel
// Qs (npad x mpad; q = qs Qs, the caller applies qs^2),
//   part[b][seg][0][j]            = sum_i Qs_ij T_ij             (T != nullptr: T = d_p K Qs, so the sum is q_j^T d_p K q_j)
//   part[b][seg][hasT + v][j]     = sum_i vec_v,i Qs_ij^2        v < nvec; vec == nullptr: the one vector of ones
// over the rows i < n of the segment.  A lane owns two adjacent queries (16-byte loads), a wave every fourth row in
// ascending order, the four waves are added in order; colpart_reduce_kernel adds the segments.  vec: [v][b][npad].
// grid = (mpad / 128, npad / 64, batch), 256 threads
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hg_coldot_kernel(const double* __restrict__ Q_all, long long sQ,
                                                        const double* __restrict__ T_all, long long sT, int ld,
                                                        const double* __restrict__ vec_all, int nvec, int n, int npad,
                                                        double* __restrict__ part_all) {
  __shared__ double2 red[4][64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int b = blockIdx.z, batch = gridDim.z, seg = blockIdx.y, nseg = gridDim.y;
  const int j = blockIdx.x * 128 + 2 * lane;
  const int r0 = seg * CT, r1 = min(r0 + CT, n);
  const int hasT = T_all ? 1 : 0, nout = hasT + nvec;
  const double* Q = Q_all + (size_t)b * sQ + j;
  const double* Tm = T_all ? T_all + (size_t)b * sT + j : nullptr;
  for (int o = 0; o < nout; ++o) {
    double2 s = make_double2(0.0, 0.0);
    if (o < hasT) {
      for (int i = r0 + w; i < r1; i += 4) {
        const double2 qv = *reinterpret_cast<const double2*>(Q + (size_t)i * ld);
        const double2 tv = *reinterpret_cast<const double2*>(Tm + (size_t)i * ld);
        s.x = fma(qv.x, tv.x, s.x);
        s.y = fma(qv.y, tv.y, s.y);
      }
    } else {
      const double* vec = vec_all ? vec_all + ((size_t)(o - hasT) * batch + b) * npad : nullptr;
      for (int i = r0 + w; i < r1; i += 4) {
        const double2 qv = *reinterpret_cast<const double2*>(Q + (size_t)i * ld);
        const double vi = vec ? vec[i] : 1.0;
        s.x = fma(vi * qv.x, qv.x, s.x);
        s.y = fma(vi * qv.y, qv.y, s.y);
      }
    }
    __syncthreads();  // the previous sum has been read
    red[w][lane] = s;
    __syncthreads();
    if (w == 0) {
      double2 r;
      r.x = ((red[0][lane].x + red[1][lane].x) + red[2][lane].x) + red[3][lane].x;
      r.y = ((red[0][lane].y + red[1][lane].y) + red[2][lane].y) + red[3][lane].y;
      *reinterpret_cast<double2*>(part_all + (((size_t)b * nseg + seg) * nout + o) * ld + j) = r;
    }
  }
}

}  // namespace gpc
