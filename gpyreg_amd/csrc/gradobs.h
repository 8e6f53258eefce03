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
#include "gradpost.h"

namespace gpc {

struct GobsDims {
  int N = 0, Ng = 0, D = 0;
  __host__ __device__ int Np() const { return (N + CT - 1) / CT * CT; }
  __host__ __device__ int Ngp() const { return (Ng + CT - 1) / CT * CT; }
  __host__ __device__ int P() const { return Np() + Ngp(); }  // rows of the point list
  __host__ __device__ long long n() const { return (long long)N + (long long)Ng * D; }  // joint order
  __host__ __device__ int vt() const { return Np() / CT; }   // tiles of value points, of gradient points
  __host__ __device__ int gt() const { return Ngp() / CT; }
  // rows of gobs_trace_kernel's partials: [vv tiles of the lower triangle | gv tiles | gg tiles x D]
  __host__ __device__ long long trace_rows() const {
    return (long long)vt() * (vt() + 1) / 2 + (long long)vt() * gt() + (long long)gt() * gt() * D;
  }
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

// ---------------------------------------------------------------------------------
// The hyperparameter gradient of the joint likelihood (gpc_nll_batch_gobs_grad; DESIGN.md "Gradient-observation
// likelihood gradient"): out_p = sum_IJ Wt_IJ d K_IJ / d theta_p over the n x n joint matrix, Wt = Tm / sl - alpha alpha^T
// read from the LOWER triangle of Tm, every d K entry evaluated here from the point list -- no plane exists anywhere.
// One 64 x 64 tile of pairs of the list per block, 4 x 4 pairs per thread as gobs_cov_kernel; the stored entries I >= J
// are summed, an off-diagonal one counted twice (m = 2, the diagonal m = 1, above it m = 0).  Three launches, one per
// kind of tile (TK), so that each kind has its own registers and no block is launched for nothing:
//   TK = 0  value / value tiles of the lower triangle;
//   TK = 1  gradient / value tiles, all of them;
//   TK = 2  gradient / gradient tiles, ALL of them: the blocks (a, b) with a > b lie below the diagonal whole, those
//           with a = b for the pairs p >= q only.  A block of the grid owns one tile and ONE b: the blocks (a >= b, b).
// With (k, F, G, H) of the pair (pair_eval_fgh_t; G = H = 0 at r2 = 0: the terms they carry are dropped there), d the
// scaled difference, u_a = c_a d_a and Wm = m Wt, theta_l = log ell_l gets
//   value / value:        Wm F d_l^2
//   gradient / value:     -G d_l^2 A + 2 F Wm_l u_l,                                  A  = sum_a Wm_a u_a
//   gradient / gradient:  d_l^2 (G T1 - H T2) - 2 F Wm_ll c_l^2 + 2 G u_l R_l,        T1 = sum_a Wm_aa c_a^2,
//                         T2 = sum_ab Wm_ab u_a u_b,  R_l = sum_b (Wm_lb + Wm_bl) u_b
// so a pair costs O(D^2) for the sums and O(D) for all outputs: pass 1 walks the blocks once (each weight is read
// once, lanes along consecutive addresses of the block's 64 x 64 patch) and adds what belongs to a single dimension --
// x = Wm_ab u_a u_b gives 2 G x to outputs a and b -- and pass 2 adds Z d_l^2 per dimension with the pair's scalar
// Z = Wm F | -G A | G T1 - H T2 (linear in T1 and T2: a gradient / gradient block runs pass 2 on the share of its b).
// log sf gets twice the contracted entries (Wm k | -F A | F T1 - G T2), the rational quadratic's log alpha those with
// (Ka, Fa, Ga) in place of (k, F, G); an isotropic kernel's one length scale the sum over l.  The a-dimensions are
// staged DCH at a time: any D.
// Loads carry no branch: a pair beyond the points of its kind reads the last point's entry and a pair above the
// diagonal of a diagonal block its mirror image (max, min) -- both in the lower triangle -- and m = 0 removes them.
// Sums: fp64; a thread adds its 16 pairs, the wave its lanes (wave_sum), lane 0 adds into its wave's row of `red`; the
// block writes the four rows' sum to its row of `part` (p < cov_N of pst slots), and reduce_parts_kernel adds the rows
// [vv tiles | gv tiles | gg tiles x D] in that order.  No atomics, a fixed order.
// 256 threads, 4 cov_N doubles of dynamic LDS.  grids: (vt (vt + 1) / 2, 1, batch) | (vt, gt, batch) | (gt^2, D, batch)
// ---------------------------------------------------------------------------------
struct GobsTraceArgs {
  GobsDims gd;
  int cov_N, ld, astride, pst;
  long long sT;
  const double *Xs, *sp, *mul, *dv, *alpha;
  const void* Tm;
  double* part;
};

template <typename T, int KIND, int DEG, int TK>
__device__ __forceinline__ void gobs_trace_tile(const GobsTraceArgs& A_, int ti, int tj, int lb, long long prow, int bz) {
  __shared__ double xi[CT][DCH + 1];
  __shared__ double xj[CT][DCH + 1];
  __shared__ double bi[CT], bj[CT];
  extern __shared__ double gobs_red[];  // [4][cov_N]
  constexpr bool ISO = KIND == K_SE_ISO || KIND == K_MATERN_ISO;
  constexpr bool gi = TK >= 1, gj = TK == 2;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lane = t & 63;
  const GobsDims gd = A_.gd;
  const int N = gd.N, Ng = gd.Ng, D = gd.D, Np = gd.Np(), P = gd.P(), cov_N = A_.cov_N, ld = A_.ld;
  const int i0 = ti * CT, j0 = tj * CT;
  const int pi0 = gi ? i0 - Np : i0, ni = gi ? Ng : N;
  const int pj0 = gj ? j0 - Np : j0, nj = gj ? Ng : N;
  double* part = A_.part + ((size_t)bz * gd.trace_rows() + prow) * A_.pst;
  const double* Xs = A_.Xs + (size_t)bz * P * D;
  const double* sp = A_.sp + (size_t)bz * SP_STRIDE;
  const double* mul = A_.mul + (size_t)bz * D;
  const double* dv = A_.dv + (size_t)bz * D;
  const T* Tm = static_cast<const T*>(A_.Tm) + (size_t)bz * A_.sT;
  const double* alpha = A_.alpha + (size_t)bz * A_.astride;
  double* red = gobs_red + (size_t)(t >> 6) * cov_N;
  for (int p = t; p < 4 * cov_N; p += 256) gobs_red[p] = 0.0;
  double r2[4][4];
  tile_r2_ab(r2, xi, xj, Xs, Xs, D, i0, j0, t, tx, ty);  // (its barriers order the zeroing of `red` before its first use)
  const double sf2 = sp[SP_SF2], rqa = sp[SP_RQA], invsl = 1.0 / sp[SP_SL];
  ExpC ex;
  ex.load();
  const int sfi = ISO ? 1 : D;
  // the multiplicity of the entry a pair owns (mult): in a block ON the diagonal of the joint matrix (value / value, and
  // gradient / gradient with a = b) the points decide, in every other block it is 2; from three 16-bit masks, bit
  // 4 a + c: both points exist | p < q | p == q.  pc / qc: the points read
  unsigned okm = 0, ltm = 0, eqm = 0;
  int pc[4], qc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) pc[a] = min(pi0 + ty + 16 * a, ni - 1);
#pragma unroll
  for (int c = 0; c < 4; ++c) qc[c] = min(pj0 + tx + 16 * c, nj - 1);
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int p = pi0 + ty + 16 * a, q = pj0 + tx + 16 * c;
      okm |= (unsigned)(p < ni && q < nj) << (4 * a + c);
      ltm |= (unsigned)(p < q) << (4 * a + c);
      eqm |= (unsigned)(p == q) << (4 * a + c);
    }
  const auto mult = [&](int a, int c, bool diag) -> double {
    const unsigned b = 1u << (4 * a + c);
    return !(okm & b) || (diag && (ltm & b)) ? 0.0 : (diag && (eqm & b)) ? 1.0 : 2.0;
  };
  double Z[4][4];    // pass 2's scalar of the pair
  double ssf = 0.0;  // this thread's share of the log sf output, and of log alpha
  double sal = 0.0;

  if constexpr (TK == 0) {
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const double ap = alpha[pc[a]];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int r = max(pc[a], qc[c]), cc = min(pc[a], qc[c]);
        const double w = mult(a, c, true) * fma((double)Tm[(size_t)r * ld + cc], invsl, -ap * alpha[qc[c]]);
        const PairVal pv = pair_eval_t<KIND, DEG>(r2[a][c], sf2, rqa, ex);
        Z[a][c] = w * pv.F;
        ssf = fma(w, pv.K, ssf);
        if constexpr (KIND == K_RQ) sal = fma(w, pv.Ka, sal);
      }
    }
    ssf *= 2.0;
  } else {
    double f[4][4], g[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const PairFG fg = pair_eval_fg_t<KIND, DEG>(r2[a][c], sf2, rqa, ex);
        f[a][c] = fg.F;
        g[a][c] = r2[a][c] > 0.0 ? fg.G : 0.0;
      }
    if constexpr (TK == 1) {  // gradient / value: rows N + l Ng + p, column q
      double A[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) A[a][c] = 0.0;
      double aq[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) aq[c] = alpha[qc[c]];
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
          double s = 0.0;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const size_t row = (size_t)N + (size_t)l * Ng + pc[a];
            const double ap = alpha[row];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const double w = mult(a, c, false) * fma((double)Tm[row * ld + qc[c]], invsl, -ap * aq[c]);
              const double wu = w * (cl * (vi[a] - vj[c]));  // Wm_l u_l
              A[a][c] += wu;
              s = fma(f[a][c], wu, s);
            }
          }
          s = wave_sum(2.0 * s);
          if (lane == 0) red[ISO ? 0 : l] += s;
        }
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          Z[a][c] = -g[a][c] * A[a][c];
          ssf = fma(-f[a][c], A[a][c], ssf);
          if constexpr (KIND == K_RQ) sal = fma(-pair_eval_fgh_t<KIND, DEG>(r2[a][c], sf2, rqa, ex).Fa, A[a][c], sal);
        }
      ssf *= 2.0;
    } else {  // gradient / gradient: rows N + la Ng + p, columns N + lb Ng + q, the blocks la >= lb of this block's lb
      double T1[4][4], T2[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) T1[a][c] = T2[a][c] = 0.0;
      if (t < CT)
        bi[t] = Xs[(size_t)(i0 + t) * D + lb];
      else if (t < 2 * CT)
        bj[t - CT] = Xs[(size_t)(j0 + t - CT) * D + lb];
      __syncthreads();
      const double cb = mul[lb] / dv[lb];
      double db[4][4], aq[4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) db[a][c] = bi[ty + 16 * a] - bj[tx + 16 * c];
#pragma unroll
      for (int c = 0; c < 4; ++c) aq[c] = alpha[(size_t)N + (size_t)lb * Ng + qc[c]];
      for (int h0 = 0; h0 < D; h0 += DCH) {
        const int dc = min(DCH, D - h0);
        if (h0 + dc <= lb) continue;  // (no la >= lb in this chunk)
        __syncthreads();
        stage_x(xi, Xs, D, i0, h0, dc, t);
        stage_x(xj, Xs, D, j0, h0, dc, t);
        __syncthreads();
        for (int h = max(0, lb - h0); h < dc; ++h) {
          const int la = h0 + h;
          const bool dg = la == lb;
          if (dg && ti < tj) continue;  // (a tile above the diagonal owns nothing of a diagonal block)
          const double ca = mul[la] / dv[la], cab = ca * cb;
          double vi[4], vj[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) vi[a] = xi[ty + 16 * a][h];
#pragma unroll
          for (int c = 0; c < 4; ++c) vj[c] = xj[tx + 16 * c][h];
          double sg = 0.0, sf = 0.0;
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const size_t row = (size_t)N + (size_t)la * Ng + pc[a];
            const double ap = alpha[row];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const size_t col = (size_t)N + (size_t)lb * Ng + qc[c];
              // (a diagonal block is read through its mirror image where the pair lies above the diagonal)
              const size_t r = dg ? max(row, col) : row, cc = dg ? min(row, col) : col;
              const double m = mult(a, c, dg);
              const double w = m * fma((double)Tm[r * ld + cc], invsl, -ap * aq[c]);
              const double x = (w * cab) * ((vi[a] - vj[c]) * db[a][c]);  // Wm_ab u_a u_b
              T2[a][c] += x;
              sg = fma(g[a][c], x, sg);
              if (dg) {
                T1[a][c] = fma(w, cab, T1[a][c]);
                sf = fma(f[a][c], w, sf);
              }
            }
          }
          // 2 G x to the outputs la and lb (twice to one output when they are the same), -2 F Wm_ll c_l^2 to l
          sg = wave_sum(dg ? 4.0 * sg - 2.0 * cab * sf : 2.0 * sg);
          if (lane == 0) {
            red[ISO ? 0 : la] += sg;
            if (!dg) red[ISO ? 0 : lb] += sg;
          }
        }
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const PairFGH pv = pair_eval_fgh_t<KIND, DEG>(r2[a][c], sf2, rqa, ex);
          // (the H term is dropped at r2 = 0 and below 1e-200, where Matern 3's t^3 leaves the fp64 range: with T2 =
          // O(r2) and d_l^2 <= r2 what is dropped is below 1e-100 of the weights)
          const double ht = r2[a][c] > 1e-200 ? pv.H * T2[a][c] : 0.0;
          Z[a][c] = fma(g[a][c], T1[a][c], -ht);
          ssf += fma(f[a][c], T1[a][c], -g[a][c] * T2[a][c]);
          if constexpr (KIND == K_RQ) sal += fma(pv.Fa, T1[a][c], -pv.Ga * T2[a][c]);
        }
      ssf *= 2.0;
    }
  }

  // pass 2: Z d_l^2 to every dimension's output
  for (int h0 = 0; h0 < D; h0 += DCH) {
    const int dc = min(DCH, D - h0);
    __syncthreads();
    stage_x(xi, Xs, D, i0, h0, dc, t);
    stage_x(xj, Xs, D, j0, h0, dc, t);
    __syncthreads();
    for (int h = 0; h < dc; ++h) {
      double vi[4], vj[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) vi[a] = xi[ty + 16 * a][h];
#pragma unroll
      for (int c = 0; c < 4; ++c) vj[c] = xj[tx + 16 * c][h];
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double d = vi[a] - vj[c];
          s = fma(Z[a][c], d * d, s);
        }
      s = wave_sum(s);
      if (lane == 0) red[ISO ? 0 : h0 + h] += s;
    }
  }
  ssf = wave_sum(ssf);
  if (lane == 0) red[sfi] += ssf;
  if constexpr (KIND == K_RQ) {
    sal = wave_sum(sal);
    if (lane == 0) red[D + 1] += sal;
  }
  __syncthreads();
  for (int p = t; p < cov_N; p += 256)
    part[p] = (gobs_red[p] + gobs_red[cov_N + p]) + (gobs_red[2 * cov_N + p] + gobs_red[3 * cov_N + p]);
}

template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void gobs_trace_vv_kernel(GobsTraceArgs a) {
  int ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  gobs_trace_tile<T, KIND, DEG, 0>(a, ti, tj, 0, blockIdx.x, blockIdx.z);
}
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void gobs_trace_gv_kernel(GobsTraceArgs a) {
  const int vt = a.gd.vt();
  gobs_trace_tile<T, KIND, DEG, 1>(a, vt + blockIdx.y, blockIdx.x, 0,
                                   (long long)vt * (vt + 1) / 2 + (long long)blockIdx.y * vt + blockIdx.x, blockIdx.z);
}
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void gobs_trace_gg_kernel(GobsTraceArgs a) {
  const int vt = a.gd.vt(), gt = a.gd.gt();
  gobs_trace_tile<T, KIND, DEG, 2>(a, vt + blockIdx.x / gt, vt + blockIdx.x % gt, blockIdx.y,
                                   (long long)vt * (vt + 1) / 2 + (long long)vt * gt + (long long)blockIdx.x * a.gd.D + blockIdx.y,
                                   blockIdx.z);
}

// ---------------------------------------------------------------------------------
// The derivative operand of the joint system (gpc_grad_post_gobs; DESIGN.md "Gradient posterior under gradient
// observations"): one 64 x 64 tile of (point of the list, query) pairs of sample b, all D + 1 slots, into gradpost.h's
// panel -- npad x (D + 1) mb, slot-major planes: column s mb + j is slot s of query j, slot 0 = f(x*), slot 1 + l =
// d f / dx*_l -- with the rows in joint order.  The sibling of grad_operand_tile_kernel and of gobs_cross_tile_kernel:
//   value tile, row i:                 slot 0      k                                     (grad_operand_tile_kernel's
//                                      slot 1 + l  -c_l F (xs*_l - xs_il), 0 at r2 = 0    expressions, in its order)
//   gradient tile, row N + a Ng + g:   slot 0      -c_a F d_a, 0 at r2 = 0               (gobs_cross_tile_kernel's)
//   (d = xs_g - xs*)                   slot 1 + l  c_a c_l (F delta_al - G d_a d_l); c_a^2 F0 delta_al at r2 = 0, the G
//                                                  term dropped              (gobs_cov_kernel's, with p = g and q = *)
// Distances by tile_r2_ab, differences before products, (k, F, G) evaluated once per pair.  Queries >= m are written as
// zeros; a value tile leaves the rows of the points it does not have alone (they are gradient rows); the rows
// [n, npad) belong to no tile and are zeroed by the launcher.
// A gradient tile works ONE SLOT per pass over its registers (slot_pass: F and G of the 16 pairs stay, 32 doubles per
// thread; slot 1 + l adds its 4 + 4 coordinates of dimension l), the a-dimensions staged DCH at a time and the slot's
// dimension on its own (bi, bj) as gobs_cov_kernel does: any D.  With D <= DCH the one chunk is staged once for all
// slots.  Registers (gfx950, DESIGN.md has the table): 215 .. 247 VGPRs, no AGPRs, no scratch, two waves per SIMD --
// the bound is asked for: left alone the scheduler interleaves the 16 entries of a row dimension up to 256 VGPRs + 8
// AGPRs (one wave), and at three waves (168 VGPRs) it spills ~290 bytes per lane.
// Fused mean product, per slot: part[b][tile row of the list][slot mb + j] = sum over every row the tile wrote of the
// STORED value times alpha[row] (dimensions ascending, then the tile's points); colpart_reduce_kernel adds the tile
// rows in ascending order.  No atomics.  f0[b] receives F0 (block (0, 0) only).
// grid = (mb/64, P/64, batch), 256 threads.  Xp: batch lists of P x D; Xss: batch x mb x D
// ---------------------------------------------------------------------------------
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256, 2) void gobs_grad_operand_tile_kernel(
    GobsDims gd, const double* __restrict__ Xp_all, const double* __restrict__ Xss_all,
    const double* __restrict__ sp_all, const double* __restrict__ mul_all, const double* __restrict__ dv_all,
    const double* __restrict__ alpha_all, int astride, int m, int mb, T* __restrict__ P_all, long long sP,
    double* __restrict__ part_all, double* __restrict__ f0_all) {
  __shared__ double xi[CT][DCH + 1];
  __shared__ double xj[CT][DCH + 1];
  __shared__ double bi[CT], bj[CT];
  __shared__ double red[2][4][CT];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, b = blockIdx.z;
  const int lane = t & 63, w = t >> 6;
  const int N = gd.N, Ng = gd.Ng, D = gd.D, Np = gd.Np(), P = gd.P(), ld = (D + 1) * mb;
  const int i0 = blockIdx.y * CT, j0 = blockIdx.x * CT;
  const bool gi = i0 >= Np;
  const int pi0 = gi ? i0 - Np : i0, ni = gi ? Ng : N;
  const double* Xp = Xp_all + (size_t)b * P * D;
  const double* Xss = Xss_all + (size_t)b * mb * D;
  const double* sp = sp_all + (size_t)b * SP_STRIDE;
  const double* mul = mul_all + (size_t)b * D;
  const double* dv = dv_all + (size_t)b * D;
  const double* alpha = alpha_all + (size_t)b * astride;
  T* Pn = P_all + (size_t)b * sP;
  double* part = part_all + ((size_t)b * (P / CT) + blockIdx.y) * ld;
  double r2[4][4];
  tile_r2_ab(r2, xi, xj, Xp, Xss, D, i0, j0, t, tx, ty);
  const double sf2 = sp[SP_SF2], rqa = sp[SP_RQA];
  ExpC ex;
  ex.load();
  if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) f0_all[b] = pair_eval_t<KIND, DEG>(0.0, sf2, rqa, ex).F;
  // column sums of one slot over the rows the tile wrote: the 4 row groups of a wave by two exchanges, the 4 waves
  // through LDS (two buffers in turn: one barrier per slot), as grad_operand_tile_kernel
  auto column_sums = [&](const double (&sc)[4], int slot) {
    double (*rb)[CT] = red[slot & 1];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double v = sc[c];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if ((lane >> 4) == 0) rb[w][tx + 16 * c] = v;
    }
    __syncthreads();
    if (t < CT) part[(size_t)slot * mb + j0 + t] = rb[0][t] + rb[1][t] + rb[2][t] + rb[3][t];
  };
  double fw[4][4];

  if (!gi) {  // value points: rows i < N
    double al[4], s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 4; ++a) al[a] = (i0 + ty + 16 * a) < ni ? alpha[i0 + ty + 16 * a] : 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
        double v = 0.0;
        fw[a][c] = 0.0;
        if (i < ni && j < m) {
          const PairVal pv = pair_eval_t<KIND, DEG>(r2[a][c], sf2, rqa, ex);
          v = pv.K;
          if (r2[a][c] > 0.0) fw[a][c] = pv.F;
        }
        const T vt = (T)v;
        if (i < ni) Pn[(size_t)i * ld + j] = vt;
        s[c] = fma((double)vt, al[a], s[c]);
      }
    column_sums(s, 0);
    for (int h0 = 0; h0 < D; h0 += DCH) {
      const int dc = min(DCH, D - h0);
      __syncthreads();
      stage_x(xi, Xp, D, i0, h0, dc, t);
      stage_x(xj, Xss, D, j0, h0, dc, t);
      __syncthreads();
      for (int h = 0; h < dc; ++h) {
        const int slot = 1 + h0 + h;
        const double cl = mul[h0 + h] / dv[h0 + h];
        double vi[4], vj[4], sd[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < 4; ++a) vi[a] = xi[ty + 16 * a][h];
#pragma unroll
        for (int c = 0; c < 4; ++c) vj[c] = xj[tx + 16 * c][h];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
            const T vt = (T)(-cl * fw[a][c] * (vj[c] - vi[a]));
            if (i < ni) Pn[(size_t)i * ld + (size_t)slot * mb + j] = vt;
            sd[c] = fma((double)vt, al[a], sd[c]);
          }
        column_sums(sd, slot);
      }
    }
    return;
  }

  // gradient points: rows N + a Ng + g.  ok: the pair exists (bit 4 a + c); nz: r2 > 0
  double gw[4][4];
  unsigned ok = 0, nz = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool e = (pi0 + ty + 16 * a) < ni && (j0 + tx + 16 * c) < m, p = r2[a][c] > 0.0;
      const PairFG fg = pair_eval_fg_t<KIND, DEG>(r2[a][c], sf2, rqa, ex);
      fw[a][c] = e ? fg.F : 0.0;
      gw[a][c] = e && p ? fg.G : 0.0;  // the G term is dropped at coincident points (Matern 3: G = inf there)
      ok |= (unsigned)e << (4 * a + c);
      nz |= (unsigned)p << (4 * a + c);
    }
  const bool one = D <= DCH;  // one chunk of a-dimensions: staged once for all slots
  if (one) {
    __syncthreads();
    stage_x(xi, Xp, D, i0, 0, D, t);
    stage_x(xj, Xss, D, j0, 0, D, t);
  }
  // one slot: the a-dimensions in ascending order.  entry(a, c, d_a, la, c_a) is the pair's value in row dimension la
  auto slot_pass = [&](int slot, auto&& entry) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int h0 = 0; h0 < D; h0 += DCH) {
      const int dc = min(DCH, D - h0);
      if (!one) {
        __syncthreads();
        stage_x(xi, Xp, D, i0, h0, dc, t);
        stage_x(xj, Xss, D, j0, h0, dc, t);
        __syncthreads();
      }
#pragma unroll 1
      for (int h = 0; h < dc; ++h) {
        const int la = h0 + h;
        const double ca = mul[la] / dv[la];
        double vj[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) vj[c] = xj[tx + 16 * c][h];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int p = pi0 + ty + 16 * a;
          if (p >= ni) continue;
          const size_t row = (size_t)N + (size_t)la * Ng + p;
          const double al = alpha[row], va = xi[ty + 16 * a][h];
          T* pr = Pn + row * ld + (size_t)slot * mb + j0 + tx;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const double v = entry(a, c, va - vj[c], la, ca);
            const T vt = (T)((ok & (1u << (4 * a + c))) ? v : 0.0);
            pr[16 * c] = vt;
            s[c] = fma((double)vt, al, s[c]);
          }
        }
      }
    }
    column_sums(s, slot);
  };
  __syncthreads();  // (the chunk above is staged)
  slot_pass(0, [&](int a, int c, double d, int, double ca) {  // -c_a F d_a; exactly 0 at r2 = 0
    const double f = (nz & (1u << (4 * a + c))) ? fw[a][c] : 0.0;
    const double wv = (ca * f) * d;
    return f != 0.0 ? -wv : 0.0;
  });
  for (int l = 0; l < D; ++l) {
    __syncthreads();  // (the previous slot's readers of bi, bj, xi and xj are done)
    if (t < CT)
      bi[t] = Xp[(size_t)(i0 + t) * D + l];
    else if (t < 2 * CT)
      bj[t - CT] = Xss[(size_t)(j0 + t - CT) * D + l];
    __syncthreads();
    const double cl = mul[l] / dv[l];
    double bv[4], bq[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) bv[a] = bi[ty + 16 * a];
#pragma unroll
    for (int c = 0; c < 4; ++c) bq[c] = bj[tx + 16 * c];
    slot_pass(1 + l, [&](int a, int c, double d, int la, double ca) {  // c_a c_l (F delta_al - G d_a d_l)
      return (ca * cl) * fma(-gw[a][c], d * (bv[a] - bq[c]), la == l ? fw[a][c] : 0.0);
    });
  }
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

// out[b][p], p < cov_N, of `batch` samples (rows of `pst` doubles; a slot p >= cov_N is left as it is) from their scaled
// point lists, Tm (ld x ld, sT apart) and alpha (astride apart); part: batch x gd.trace_rows() x pst partials
inline void launch_gobs_trace(hipStream_t st, const CovDesc& cd, const GobsDims& gd, int batch, const double* xs,
                              const double* sp, const double* mul, const double* dv, const double* Tm, long long sT, int ld,
                              const double* alpha, int astride, double* part, int pst, double* out) {
  const int vt = gd.vt(), gt = gd.gt();
  const size_t shm = 4 * (size_t)cd.cov_N * sizeof(double);
  GobsTraceArgs a{gd, cd.cov_N, ld, astride, pst, sT, xs, sp, mul, dv, alpha, Tm, part};
  GPC_COV_DISPATCH(gobs_trace_vv_kernel, double, cd, dim3(vt * (vt + 1) / 2, 1, batch), dim3(256), shm, st, a);
  GPC_COV_DISPATCH(gobs_trace_gv_kernel, double, cd, dim3(vt, gt, batch), dim3(256), shm, st, a);
  GPC_COV_DISPATCH(gobs_trace_gg_kernel, double, cd, dim3(gt * gt, gd.D, batch), dim3(256), shm, st, a);
  hipLaunchKernelGGL(reduce_parts_kernel, dim3(cd.cov_N, batch), dim3(256), 0, st, (const double*)part,
                     (int)gd.trace_rows(), pst, out);
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

// The derivative operands of `batch` samples for one block of mb = GQB queries (panels sP apart, npad x (D + 1) mb) with
// their mean products: part: batch x P/64 x (D + 1) mb partials, mean: batch x (D + 1) mb, f0: batch.  The rows
// [n, npad) of every panel are zeroed here.
template <typename T>
inline hipError_t launch_gobs_grad_operand(hipStream_t st, const CovDesc& cd, const GobsDims& gd, const double* xp,
                                           const double* xsq, const double* sp, const double* mul, const double* dv,
                                           const double* alpha, int astride, int npad, int m, int batch, T* P,
                                           long long sP, double* part, double* mean, double* f0) {
  const int mb = GQB, ld = (gd.D + 1) * mb;
  const size_t n = (size_t)gd.n();
  if ((size_t)npad > n) {
    hipError_t e = hipMemset2DAsync(P + n * ld, (size_t)sP * sizeof(T), 0, ((size_t)npad - n) * ld * sizeof(T), batch, st);
    if (e != hipSuccess) return e;
  }
  GPC_COV_DISPATCH(gobs_grad_operand_tile_kernel, T, cd, dim3(mb / CT, gd.P() / CT, batch), dim3(256), 0, st, gd, xp, xsq,
                   sp, mul, dv, alpha, astride, m, mb, P, sP, part, f0);
  hipLaunchKernelGGL(colpart_reduce_kernel, dim3((ld + 255) / 256, batch), dim3(256), 0, st, (const double*)part,
                     gd.P() / CT, ld, mean);
  return hipGetLastError();
}

}  // namespace gpc
