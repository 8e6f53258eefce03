// paths.h -- pathwise posterior samples (gpc_paths_create / gpc_paths_eval; DESIGN.md "Pathwise samples").
//
// Matheron's rule with random Fourier features.  Per hyperparameter sample s (global index) and path r < R:
//   f_{s,r}(x) = p_{s,r}(x) + k_s(x, X) v_{s,r}                                   (the mean function is the caller's)
//   p_{s,r}(x) = sqrt(2 sf2 / F) sum_{f<F} wt[f][r] cos(theta[f] . xs(x) + b[f])
//   v_{s,r}    = (K + Sigma)^-1 (y - m(X) - p_{s,r}(X) - eps_{s,r}),   eps_{s,r}[i] = noise_sd[i] e[i][r]
// xs: the scaled inputs of scale_x_kernel.  On scaled inputs theta[f][l] = z[f][l] (SE) or z[f][l] / sqrt(c[f]),
// c[f] = sum_{q<d} g[f][q]^2 (Matern of degree d: the multivariate Student-t with d degrees of freedom).
// Random stream: draw.h's normals4 under the key (seed, stream), streams 2 (z: r = l, j = f), 3 (g: r = q, j = f),
// 4 (b[f] = 2 pi (word >> 11) 2^-53, r = 0, j = f), 5 (wt: r = r, j = f), 6 (e: r = r, j = i); gpyreg_amd/_paths.py
// restates it.  A value depends on (seed, stream, s, r, j) only: path r of sample s does not depend on R, on the batch
// of samples, on the chunking or on the sharding.
//
// Evaluation (the hot path) never writes K* or the feature matrix: a block forms one 64 x 64 operand tile at a time in
// LDS -- cross covariances by the compile-time pair functor, then cos / sin features -- and multiplies it straight
// into the v (then wt) panel with v_mfma_f64_16x16x4_f64.  Tiles are walked in ascending order by one block, no
// atomics: a value depends on (x, s, r) alone, not on M, the row's place in the batch or the other rows.
#pragma once
#include "block_append.h"
#include "common.h"
#include "covfun.h"
#include "draw.h"

namespace gpc {

constexpr int PA_LD = CT + 4;  // row stride of the LDS operand tile: the 16 x 4 fragment reads and the 4 x 4 writes spread over the banks
constexpr int PA_SLOTS = 4;    // operands a block accumulates: slot 0 = f, slot 1 + l = df / dx_l
constexpr int PA_CG = 4;       // 16-column groups of the panel per block (64 paths)
// The evaluation engine gpc_paths_eval runs by default: 1 = the fused kernel below, 2 = the unfused composition
// (operand matrices written to memory, then the library GEMM).  NOT YET DECIDED BY MEASUREMENT: the comparison at cfg3
// (N = 4096, D = 10, S = 16, Matern-5, fp64; R = 64, F = 1024, M = 1000 and 4096; tools/sample_paths_bench.py writes
// profiles/sample_paths_cfg3.json with both engines) has not been run; the fused kernel is the default because it
// moves no N x M operand through memory.  Whoever runs the benchmark puts the figures here and flips the constant if
// the fused kernel loses.  (Callers learn which engine a call ran from the get-only option "paths_engine_ran".)
constexpr int PA_DEFAULT_ENGINE = 1;

// theta[b][f][l] (fpad x D, zero rows from F on) and bph[b][f].  One thread per (quad of features, dimension).
// grid = (ceil(fpad / 256), ceil(D / 4), batch), block = (64, 4)
template <int DEG>
__global__ __launch_bounds__(256) void paths_features_kernel(unsigned long long seed, long long s_base, int F, int fpad,
                                                             int D, double* __restrict__ theta_all,
                                                             double* __restrict__ bph_all) {
  const int q = blockIdx.x * 64 + threadIdx.x, l = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
  if (4 * q >= fpad || l >= D) return;
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  if (4 * q < F) {
    normals4(seed, 2, s_base + b, l, q, z);
    if constexpr (DEG > 0) {
      double c[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int d = 0; d < DEG; ++d) {
        double g[4];
        normals4(seed, 3, s_base + b, d, q, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) c[e] = fma(g[e], g[e], c[e]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) z[e] = z[e] / sqrt(c[e]);
    }
  }
  double* theta = theta_all + (size_t)b * fpad * D;
#pragma unroll
  for (int e = 0; e < 4; ++e) theta[(size_t)(4 * q + e) * D + l] = (4 * q + e < F) ? z[e] : 0.0;
  if (l == 0) {
    PhiloxWords p = {{0ull, 0ull, 0ull, 0ull}};
    if (4 * q < F)
      p = philox4x64_10((unsigned long long)q + 1ull, 0ull, (unsigned long long)(s_base + b), 0ull, seed, 4ull);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      bph_all[(size_t)b * fpad + 4 * q + e] = (4 * q + e < F) ? 2.0 * M_PI * ((double)(p.w[e] >> 11) * 0x1p-53) : 0.0;
  }
}

// wt[b][f][r] (fpad x kq, zero outside F x R).  One thread per (quad of features, path).
// grid = (ceil(kq / 64), ceil(fpad / 16), batch), block = (64, 4)
__global__ __launch_bounds__(256) void paths_weights_kernel(unsigned long long seed, long long s_base, int F, int fpad,
                                                            int R, int kq, double* __restrict__ wt_all) {
  const int r = blockIdx.x * 64 + threadIdx.x, q = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
  if (r >= kq || 4 * q >= fpad) return;
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  if (r < R && 4 * q < F) normals4(seed, 5, s_base + b, r, q, z);
#pragma unroll
  for (int e = 0; e < 4; ++e) wt_all[((size_t)b * fpad + 4 * q + e) * kq + r] = (4 * q + e < F) ? z[e] : 0.0;
}

// The right-hand sides of the solve: P[b][i][r] (npad x kq, zero outside N x R) = ym[b][i] - pX[(i R + r) cnt + b]
// - nsd[i S + s_loc + b] e[i][r], e of stream 6 computed here.  One thread per (quad of rows, path).
// grid = (ceil(kq / 64), npad / 16, batch), block = (64, 4)
__global__ __launch_bounds__(256) void paths_rhs_kernel(unsigned long long seed, long long s_base, int n, int npad, int R,
                                                        int kq, const double* __restrict__ ym_all,
                                                        const double* __restrict__ pX, int cnt,
                                                        const double* __restrict__ nsd, int S, int s_loc,
                                                        double* __restrict__ P_all) {
  const int r = blockIdx.x * 64 + threadIdx.x, q = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
  if (r >= kq || 4 * q >= npad) return;
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  if (r < R && 4 * q < n) normals4(seed, 6, s_base + b, r, q, z);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = 4 * q + e;
    double v = 0.0;
    if (i < n && r < R)
      v = ym_all[(size_t)b * n + i] - pX[((size_t)i * R + r) * cnt + b] - nsd[(size_t)i * S + s_loc + b] * z[e];
    P_all[((size_t)b * npad + i) * kq + r] = v;
  }
}

// v[b][i][j] (ld kq) = f in[b][i][j] (ld kp, the storage type), i < n, j < kq, samples of parametrisation `want`:
// f = cmul, divided by par[b][BA_SL] when by_sl (the MFMA engine of the solve: block_append.h's panels)
// grid = (kq / 64 rounded up, ceil(n / 4), batch), block = (64, 4)
template <typename T>
__global__ void paths_from_panel_kernel(const T* __restrict__ in_all, int n, int kq, int npad, int kp, double cmul,
                                        int by_sl, const double* __restrict__ par, int want,
                                        double* __restrict__ v_all) {
  const int b = blockIdx.z;
  if ((int)par[(size_t)b * BA_STRIDE + BA_LCH] != want) return;
  const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
  if (i >= n || j >= kq) return;
  const double f = by_sl ? cmul / par[(size_t)b * BA_STRIDE + BA_SL] : cmul;
  v_all[((size_t)b * npad + i) * kq + j] = f * (double)in_all[((size_t)b * npad + i) * kp + j];
}

struct PathsEvalArgs {
  const double* xs;     // [b][npad][D]  scaled training inputs
  const double* xq;     // [b][mpad][D]  scaled query points (zero rows from m on)
  const double* sp;     // [b][SP_STRIDE]
  const double* mul;    // [b][D]
  const double* dv;     // [b][D]
  const double* v;      // [b][npad][kq]
  const double* theta;  // [b][fpad][D]
  const double* bph;    // [b][fpad]
  const double* wt;     // [b][fpad][kq]
  int n, npad, m, mpad, F, fpad, R, kq;
  int nslots;           // 1: f alone; 1 + D: with the gradient
  double* f;            // [(j R + r) S_out + s_out0 + b]
  double* df;           // [((j D + l) R + r) S_out + s_out0 + b]
  int S_out, s_out0;
};

// dot[a][c] = theta_row(ty + 16 a) . xq_row(tx + 16 c), dimensions in ascending order (tile_r2_ab's staging)
__device__ __forceinline__ void tile_dot_ab(double (&dot)[4][4], double (*xi)[DCH + 1], double (*xj)[DCH + 1],
                                            const double* __restrict__ Xa, const double* __restrict__ Xb, int D, int i0,
                                            int j0, int t, int tx, int ty) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) dot[a][c] = 0.0;
  for (int h0 = 0; h0 < D; h0 += DCH) {
    const int dc = min(DCH, D - h0);
    __syncthreads();
    stage_x(xi, Xa, D, i0, h0, dc, t);
    stage_x(xj, Xb, D, j0, h0, dc, t);
    __syncthreads();
    for (int h = 0; h < dc; ++h) {
      double vi[4], vj[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) vi[a] = xi[ty + 16 * a][h];
#pragma unroll
      for (int c = 0; c < 4; ++c) vj[c] = xj[tx + 16 * c][h];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) dot[a][c] = fma(vi[a], vj[c], dot[a][c]);
    }
  }
}

// acc[g] (16 query rows of wave w x 16 panel columns) += op[16 w ..][0 .. 63] panel[0 .. 63][16 (g0 + g) ..]: sixteen
// k-steps of v_mfma_f64_16x16x4_f64.  A operand: lane holds op[row = lane & 15][k = lane >> 4]; B operand: lane holds
// panel[k = lane >> 4][column = lane & 15] (common.h: MM<double>).  `panel` points at the tile's first row.
__device__ __forceinline__ void paths_mma_tile(MM<double>::acc_t (&acc)[PA_CG], const double (*op)[PA_LD],
                                               const double* __restrict__ panel, int kq, int g0, int ng, int lane, int w) {
  const int row = 16 * w + (lane & 15), kl = lane >> 4, col = 16 * g0 + (lane & 15);
#pragma unroll 4
  for (int kk = 0; kk < CT / 4; ++kk) {
    const double a = op[row][4 * kk + kl];
    const double* prow = panel + (size_t)(4 * kk + kl) * kq + col;
#pragma unroll
    for (int g = 0; g < PA_CG; ++g)
      if (g < ng) acc[g] = MM<double>::mma(a, prow[16 * g], acc[g]);
  }
}

// One 64-row tile of query points of sample b against all training points and all features, for up to PA_SLOTS
// operands (slot 0: the value; slot 1 + l: the derivative with respect to x_l) and up to 64 paths.
//   kernel part, slot 0:     op[j][i] = K_ij                                 (pair_eval_t, as cross_tile_kernel)
//                slot 1 + l: op[j][i] = -c_l F_ij (xs*_jl - xs_il)           (F, c_l as gpc_predict_grad; 0 at distance 0)
//   feature part, slot 0:    op[j][f] = sc cos(theta_f . xs*_j + b_f),  sc = sqrt(2 sf2 / F)
//                slot 1 + l: op[j][f] = -c_l theta_fl sc sin(.)
// The slots of a block share the pair evaluation and the sincos; every slot has its own accumulators and the same
// ascending walk, so f carries the same bits with and without the gradient.
// grid = (ceil(m / 64), ceil(nslots / PA_SLOTS) * ceil(kq / 64), batch), 256 threads, 34 KB of LDS
#ifndef GPC_PATHS_WPS
#define GPC_PATHS_WPS 1  // workgroups per CU the kernel is compiled for (297 registers at 1; 2 caps them at 256 and spills)
#endif
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256, GPC_PATHS_WPS) void paths_eval_kernel(CovDesc cd, PathsEvalArgs a) {
  // [xi | xj] while the distances / dot products form, then the operand tile
  __shared__ double shm[CT * PA_LD];
  static_assert(2 * CT * (DCH + 1) <= CT * PA_LD, "LDS overlay");
  double(*xi)[DCH + 1] = reinterpret_cast<double(*)[DCH + 1]>(shm);
  double(*xj)[DCH + 1] = reinterpret_cast<double(*)[DCH + 1]>(shm + CT * (DCH + 1));
  double(*op)[PA_LD] = reinterpret_cast<double(*)[PA_LD]>(shm);
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lane = t & 63, w = t >> 6, b = blockIdx.z;
  const int D = cd.D;
  const int ncb = (a.kq + 16 * PA_CG - 1) / (16 * PA_CG);
  const int cb = blockIdx.y % ncb, sg = blockIdx.y / ncb;
  const int q0 = sg * PA_SLOTS, nq = min(PA_SLOTS, a.nslots - q0);
  const int g0 = cb * PA_CG, ng = min(PA_CG, a.kq / 16 - g0);
  const int j0 = blockIdx.x * CT;
  const double* Xs = a.xs + (size_t)b * a.npad * D;
  const double* Xq = a.xq + (size_t)b * a.mpad * D;
  const double* sp = a.sp + (size_t)b * SP_STRIDE;
  const double* mul = a.mul + (size_t)b * D;
  const double* dv = a.dv + (size_t)b * D;
  const double* V = a.v + (size_t)b * a.npad * a.kq;
  const double* Th = a.theta + (size_t)b * a.fpad * D;
  const double* bph = a.bph + (size_t)b * a.fpad;
  const double* Wt = a.wt + (size_t)b * a.fpad * a.kq;
  const double sf2 = sp[SP_SF2], rqa = sp[SP_RQA];
  ExpC ex;
  ex.load();
  MM<double>::acc_t acc[PA_SLOTS][PA_CG];
#pragma unroll
  for (int qq = 0; qq < PA_SLOTS; ++qq)
#pragma unroll
    for (int g = 0; g < PA_CG; ++g) acc[qq][g] = MM<double>::acc_t{0.0, 0.0, 0.0, 0.0};

  // ---- k(x*, X) v: the training points in tiles of 64
  for (int i0 = 0; i0 < a.n; i0 += CT) {
    double r2[4][4], kv[4][4], fv[4][4];
    tile_r2_ab(r2, xi, xj, Xs, Xq, D, i0, j0, t, tx, ty);
#pragma unroll
    for (int ai = 0; ai < 4; ++ai)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = i0 + ty + 16 * ai, j = j0 + tx + 16 * c;
        kv[ai][c] = fv[ai][c] = 0.0;
        if (i < a.n && j < a.m) {
          const PairVal pv = pair_eval_t<KIND, DEG>(r2[ai][c], sf2, rqa, ex);
          kv[ai][c] = pv.K;
          if (r2[ai][c] > 0.0) fv[ai][c] = pv.F;
        }
      }
#pragma unroll
    for (int qq = 0; qq < PA_SLOTS; ++qq) {
      if (qq >= nq) break;
      const int q = q0 + qq;
      __syncthreads();  // xi / xj (or the previous operand) are read: the tile overlays them
      if (q == 0) {
#pragma unroll
        for (int ai = 0; ai < 4; ++ai)
#pragma unroll
          for (int c = 0; c < 4; ++c) op[tx + 16 * c][ty + 16 * ai] = kv[ai][c];
      } else {
        const int l = q - 1;
        const double ncl = -(mul[l] / dv[l]);
        double xil[4], xjl[4];
#pragma unroll
        for (int ai = 0; ai < 4; ++ai) xil[ai] = Xs[(size_t)(i0 + ty + 16 * ai) * D + l];
#pragma unroll
        for (int c = 0; c < 4; ++c) xjl[c] = Xq[(size_t)(j0 + tx + 16 * c) * D + l];
#pragma unroll
        for (int ai = 0; ai < 4; ++ai)
#pragma unroll
          for (int c = 0; c < 4; ++c) op[tx + 16 * c][ty + 16 * ai] = ncl * (fv[ai][c] * (xjl[c] - xil[ai]));
      }
      __syncthreads();
      paths_mma_tile(acc[qq], op, V + (size_t)i0 * a.kq, a.kq, g0, ng, lane, w);
    }
  }

  // ---- p(x*): the features in tiles of 64
  const double sc = sqrt(2.0 * sf2 / (double)a.F);
  for (int f0 = 0; f0 < a.F; f0 += CT) {
    double dt[4][4], cs[4][4], sn[4][4];
    tile_dot_ab(dt, xi, xj, Th, Xq, D, f0, j0, t, tx, ty);
#pragma unroll
    for (int ai = 0; ai < 4; ++ai) {
      const int f = f0 + ty + 16 * ai;
      const double bf = bph[f];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = j0 + tx + 16 * c;
        double s_ = 0.0, c_ = 0.0;
        if (f < a.F && j < a.m) sincos(dt[ai][c] + bf, &s_, &c_);
        cs[ai][c] = sc * c_;
        sn[ai][c] = sc * s_;
      }
    }
#pragma unroll
    for (int qq = 0; qq < PA_SLOTS; ++qq) {
      if (qq >= nq) break;
      const int q = q0 + qq;
      __syncthreads();
      if (q == 0) {
#pragma unroll
        for (int ai = 0; ai < 4; ++ai)
#pragma unroll
          for (int c = 0; c < 4; ++c) op[tx + 16 * c][ty + 16 * ai] = cs[ai][c];
      } else {
        const int l = q - 1;
        const double ncl = -(mul[l] / dv[l]);
#pragma unroll
        for (int ai = 0; ai < 4; ++ai) {
          const double th = Th[(size_t)(f0 + ty + 16 * ai) * D + l];
#pragma unroll
          for (int c = 0; c < 4; ++c) op[tx + 16 * c][ty + 16 * ai] = ncl * (th * sn[ai][c]);
        }
      }
      __syncthreads();
      paths_mma_tile(acc[qq], op, Wt + (size_t)f0 * a.kq, a.kq, g0, ng, lane, w);
    }
  }

  // ---- results, in the caller's layout
  const size_t so = (size_t)a.s_out0 + b;
#pragma unroll
  for (int qq = 0; qq < PA_SLOTS; ++qq) {
    if (qq >= nq) break;
    const int q = q0 + qq;
#pragma unroll
    for (int g = 0; g < PA_CG; ++g) {
      if (g >= ng) break;
      const int r = 16 * (g0 + g) + (lane & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + 16 * w + MM<double>::row_of(lane, e);
        if (j >= a.m || r >= a.R) continue;
        if (q == 0)
          a.f[((size_t)j * a.R + r) * a.S_out + so] = acc[qq][g][e];
        else
          a.df[(((size_t)j * D + (q - 1)) * a.R + r) * a.S_out + so] = acc[qq][g][e];
      }
    }
  }
}

// ---- the unfused engine (test option "paths_engine" = 2): the operand matrices written to memory, one slot at a
// time, and multiplied by the library GEMM.
// op[b][i][j] (npad x mpad, row-major, zero padding): the kernel part of slot `slot` (see paths_eval_kernel), by the
// run-time pair functor as cross_kernel.   grid = (mpad / 64, npad / 4, batch), block = (64, 4)
__global__ void paths_cross_op_kernel(CovDesc cd, const double* __restrict__ Xs_all, const double* __restrict__ Xq_all,
                                      const double* __restrict__ sp_all, const double* __restrict__ mul_all,
                                      const double* __restrict__ dv_all, int n, int npad, int m, int mpad, int slot,
                                      double* __restrict__ op_all) {
  const int b = blockIdx.z;
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int i = blockIdx.y * 4 + threadIdx.y;
  if (i >= npad || j >= mpad) return;
  double v = 0.0;
  if (i < n && j < m) {
    const double* xi = Xs_all + ((size_t)b * npad + i) * cd.D;
    const double* xj = Xq_all + ((size_t)b * mpad + j) * cd.D;
    double r2 = 0.0;
    for (int h = 0; h < cd.D; ++h) {
      const double d = xi[h] - xj[h];
      r2 = fma(d, d, r2);
    }
    const double* sp = sp_all + (size_t)b * SP_STRIDE;
    const PairVal pv = pair_eval(cd.kind, cd.degree, r2, sp[SP_SF2], sp[SP_RQA]);
    if (slot == 0) {
      v = pv.K;
    } else if (r2 > 0.0) {
      const int l = slot - 1;
      v = -(mul_all[(size_t)b * cd.D + l] / dv_all[(size_t)b * cd.D + l]) * (pv.F * (xj[l] - xi[l]));
    }
  }
  op_all[((size_t)b * npad + i) * mpad + j] = v;
}

// op[b][f][j] (fpad x mpad, row-major, zero padding): the feature part of slot `slot`.
// grid = (mpad / 64, fpad / 4, batch), block = (64, 4)
__global__ void paths_feat_op_kernel(int D, const double* __restrict__ theta_all, const double* __restrict__ bph_all,
                                     const double* __restrict__ Xq_all, const double* __restrict__ sp_all,
                                     const double* __restrict__ mul_all, const double* __restrict__ dv_all, int F,
                                     int fpad, int m, int mpad, int slot, double* __restrict__ op_all) {
  const int b = blockIdx.z;
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int f = blockIdx.y * 4 + threadIdx.y;
  if (f >= fpad || j >= mpad) return;
  double v = 0.0;
  if (f < F && j < m) {
    const double* th = theta_all + ((size_t)b * fpad + f) * D;
    const double* xj = Xq_all + ((size_t)b * mpad + j) * D;
    double dot = 0.0;
    for (int h = 0; h < D; ++h) dot = fma(th[h], xj[h], dot);
    const double sc = sqrt(2.0 * sp_all[(size_t)b * SP_STRIDE + SP_SF2] / (double)F);
    const double arg = dot + bph_all[(size_t)b * fpad + f];
    if (slot == 0) {
      v = sc * cos(arg);
    } else {
      const int l = slot - 1;
      v = -(mul_all[(size_t)b * D + l] / dv_all[(size_t)b * D + l]) * (th[l] * (sc * sin(arg)));
    }
  }
  op_all[((size_t)b * fpad + f) * mpad + j] = v;
}

// out[b][i][j] (rows x ldo, zero from column ldi on) = in[b][i][j] (rows x ldi): a panel widened to the GEMM's 128
// columns.   grid = (ldo / 64, rows / 4, batch), block = (64, 4)
__global__ void paths_widen_kernel(const double* __restrict__ in_all, int rows, int ldi, int ldo,
                                   double* __restrict__ out_all) {
  const int b = blockIdx.z;
  const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
  if (i >= rows || j >= ldo) return;
  out_all[((size_t)b * rows + i) * ldo + j] = j < ldi ? in_all[((size_t)b * rows + i) * ldi + j] : 0.0;
}

// The product C[b] (mpad x rp) of the unfused engine into the caller's layout (see PathsEvalArgs).
// grid = (ceil(R / 64), ceil(m / 4), batch), block = (64, 4)
__global__ void paths_scatter_kernel(const double* __restrict__ C_all, int m, int mpad, int rp, int R, int D, int slot,
                                     int S_out, int s_out0, double* __restrict__ f, double* __restrict__ df) {
  const int b = blockIdx.z;
  const int r = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
  if (j >= m || r >= R) return;
  const double v = C_all[((size_t)b * mpad + j) * rp + r];
  const size_t so = (size_t)s_out0 + b;
  if (slot == 0)
    f[((size_t)j * R + r) * S_out + so] = v;
  else
    df[(((size_t)j * D + (slot - 1)) * R + r) * S_out + so] = v;
}

}  // namespace gpc
