// gradpost.h -- the posterior of the gradient: the joint Gaussian of (f(x*), grad f(x*)) per hyperparameter sample
// (gpc_grad_post; DESIGN.md "Gradient posterior").
//
// For sample s and query x*_j, with xs the scaled inputs (scale_x_kernel), c_l = mul_l / dv_l and F the radial factor of
// the pair functor (dK/dlog ell_l = F d_l), the operand is the N x (D + 1) matrix
//   B_j = [ k(X, x*_j) | G_j ],   G_j[i, l] = dk(x*_j, X_i) / dx*_jl = -c_l F_ij (xs*_jl - xs_il),
// and the joint covariance of slot 0 = f, slot 1 + l = d/dx_l is
//   C_j = H - V_j^T V_j / sl,  V_j = W B_j          (L_chol samples)
//   C_j = H + B_j^T (L B_j)                          (low noise, L = -inv)
// with the prior block H = diag(kss, F0 c_1^2, ..., F0 c_D^2), F0 = the functor's F at r2 = 0 (stationary kernels: the
// value / derivative cross terms vanish at coincident points).  The mean is B_j^T alpha.
//
// PANEL LAYOUT.  Queries are worked on in blocks of GQB = 128.  The panel of a block is N_pad x ((D + 1) * 128), row
// major, SLOT-MAJOR PLANES: column a * 128 + j holds slot a of query j.  Reason: in both new kernels a lane is a query.
// The operand kernel then writes, and the Gram kernel reads, 64 consecutive elements per wave and slot (one 512-byte
// line run for fp64) -- with (query, slot) interleaved a lane's Gram reads would be (D + 1) elements apart and every
// wave load would touch D + 1 times the lines it uses.  Each plane is one 128-tile of columns, so the panel is a valid
// right-hand side of the 128-tile products of gemm.h as it stands, padding included (zero columns give zero columns).
#pragma once
#include "covfun.h"

namespace gpc {

constexpr int GQB = TILE;  // queries per block: one 128-tile of panel columns per slot, whatever N_pad and D are
constexpr int GTB = 8;     // slots per register tile of the Gram kernel

// ---------------------------------------------------------------------------------
// The derivative operand: one 64 x 64 tile of (training point, query) pairs of sample b, all D + 1 slots.  Distances
// are staged and summed as in cross_tile_kernel (same r2, same K to the bit); F comes from the same pair evaluation.
// The differences xs*_jl - xs_il are taken before the products (as cross_grad_tile_kernel: no cancellation far from
// the origin); a pair with r2 = 0 contributes 0 to G.  Rows >= n and queries >= m are written as zeros.
// Fused mean product, as cross_tile_kernel's mupart: part[b][ti][a * mb + j] = sum over the 64 rows of tile row ti of
// the STORED panel value times alpha_i; colpart_reduce_kernel adds the tile rows in ascending order, so
// (fmu, dfmu) = B^T alpha never re-reads the panel.  f0[b] receives F0 (block (0, 0) only).
// grid = (mb/64, npad/64, batch), 256 threads
// ---------------------------------------------------------------------------------
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void grad_operand_tile_kernel(
    CovDesc cd, const double* __restrict__ Xs_all, const double* __restrict__ Xss_all,
    const double* __restrict__ sp_all, const double* __restrict__ mul_all, const double* __restrict__ dv_all,
    const double* __restrict__ alpha_all, int astride, int n, int npad, int m, int mb, T* __restrict__ P_all,
    long long sP, double* __restrict__ part_all, double* __restrict__ f0_all) {
  __shared__ double xi[CT][DCH + 1];
  __shared__ double xj[CT][DCH + 1];
  __shared__ double red[2][4][CT];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, b = blockIdx.z;
  const int lane = t & 63, w = t >> 6;
  const int D = cd.D, ld = (D + 1) * mb;
  const int i0 = blockIdx.y * CT, j0 = blockIdx.x * CT;
  const double* Xs = Xs_all + (size_t)b * npad * D;
  const double* Xss = Xss_all + (size_t)b * mb * D;
  const double* sp = sp_all + (size_t)b * SP_STRIDE;
  const double* mul = mul_all + (size_t)b * D;
  const double* dv = dv_all + (size_t)b * D;
  const double* alpha = alpha_all + (size_t)b * astride;
  T* P = P_all + (size_t)b * sP;
  double* part = part_all + ((size_t)b * (npad / CT) + blockIdx.y) * ld;
  double r2[4][4];
  tile_r2_ab(r2, xi, xj, Xs, Xss, D, i0, j0, t, tx, ty);
  const double sf2 = sp[SP_SF2], rqa = sp[SP_RQA];
  ExpC ex;
  ex.load();
  if (blockIdx.x == 0 && blockIdx.y == 0 && t == 0) f0_all[b] = pair_eval_t<KIND, DEG>(0.0, sf2, rqa, ex).F;
  double al[4], fw[4][4], s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int a = 0; a < 4; ++a) al[a] = (i0 + ty + 16 * a) < n ? alpha[i0 + ty + 16 * a] : 0.0;
  // column sums of one slot over the tile's 64 rows: the 4 row groups of a wave by two exchanges, the 4 waves through
  // LDS (two buffers in turn: one barrier per slot)
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
  // slot 0: the covariance itself
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
      double v = 0.0;
      fw[a][c] = 0.0;
      if (i < n && j < m) {
        const PairVal pv = pair_eval_t<KIND, DEG>(r2[a][c], sf2, rqa, ex);
        v = pv.K;
        if (r2[a][c] > 0.0) fw[a][c] = pv.F;
      }
      const T vt = (T)v;
      P[(size_t)i * ld + j] = vt;
      s[c] = fma((double)vt, al[a], s[c]);
    }
  column_sums(s, 0);
  // slots 1 .. D: the derivatives, DCH dimensions staged at a time
  for (int h0 = 0; h0 < D; h0 += DCH) {
    const int dc = min(DCH, D - h0);
    __syncthreads();
    stage_x(xi, Xs, D, i0, h0, dc, t);
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
          P[(size_t)i * ld + (size_t)slot * mb + j] = vt;
          sd[c] = fma((double)vt, al[a], sd[c]);
        }
      column_sums(sd, slot);
    }
  }
}

// ---------------------------------------------------------------------------------
// The block Gram: per query j the (D + 1) x (D + 1) matrix  sum_i Y[i][a, j] Z[i][b, j]  over the n rows of two panels
// in the layout above (Y = Z = V for L_chol samples; Y = the panel, Z = L panel otherwise), accumulated in fp64
// whatever T is.  Only a >= b is computed and both [a][b] and [b][a] are written from the one accumulator: symmetric to
// the bit.  DIAG: the D + 1 entries a = b only, out[j][a].
//
// Engine: fp64 VALU in registers, not v_mfma_f64_16x16x4_f64 and not LDS.  This is a streaming pass: each panel element
// is read once and takes part in (D + 1) / 2 FMAs of the lower triangle, ~(D + 1) / 8 flops per byte at fp64 -- at
// D = 10 and the ~4 TB/s a streaming read holds that is ~6 TFLOP/s, under a tenth of the fp64 rate.  On gfx950 the fp64
// MFMA and the fp64 VALU share the DP units and have the SAME peak, so the matrix instruction
// buys no rate; it would spend it worse: one 16 x 16 accumulator tile per query uses (D + 1)^2 / 256 of each
// instruction (47 % at D = 10, and the upper triangle is computed for nothing), its A / B fragments want 4 rows x 16
// slots of ONE query per instruction, i.e. reads a plane apart (or, with interleaved columns, D + 1 apart across the
// queries of a wave), and a block-diagonal result cannot share accumulators between queries.  With a lane per query the
// loads are whole 512-byte runs, the operands go from the load straight into FMAs (no LDS round trip: two LDS reads per
// FMA would cost more than the HBM read they serve), and only the needed products are formed up to the 8 x 8 register
// tile: a block takes slots [8 ta, 8 ta + 8) x [8 tb, 8 tb + 8), ta >= tb, so any D is served (D + 1 <= 8: one tile;
// beyond, the panels are re-read once per tile pair, from L2 for the most part).
// Order: the rows are cut into nseg segments (by n ALONE: gram_segments), a segment into 4 equal runs, one per wave;
// a wave adds its rows in ascending order, the waves' sums are added in ascending order through LDS, and with
// nseg > 1 the segments' partial matrices are added in ascending order by gram_reduce_kernel.  No atomics.
// grid = (mb/64, tile pairs, batch * nseg), 256 threads; Y, Z: batch panels sP apart with leading dimension Dp * mb;
// out: batch x nseg x mb x Dp x Dp (DIAG: ... x Dp)
// ---------------------------------------------------------------------------------
inline int gram_segments(int n) { return std::max(1, std::min(16, n / 512)); }

template <typename T, bool DIAG>
__global__ __launch_bounds__(256) void block_gram_kernel(const T* __restrict__ Y_all, const T* __restrict__ Z_all,
                                                         long long sP, int n, int mb, int Dp, int nseg,
                                                         double* __restrict__ out_all) {
  __shared__ double buf[3][GTB][WAVE];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int b = blockIdx.z / nseg, seg = blockIdx.z % nseg;
  const int j = blockIdx.x * WAVE + lane, ld = Dp * mb;
  int ta, tb;
  if constexpr (DIAG)
    ta = tb = blockIdx.y;
  else
    lower_tile(blockIdx.y, ta, tb);
  const int a0 = ta * GTB, b0 = tb * GTB;
  const int rps = (((n + nseg - 1) / nseg + 3) / 4) * 4, rpw = rps / 4;
  const int r0 = min(n, seg * rps + w * rpw), r1 = min(n, r0 + rpw);
  const T* Y = Y_all + (size_t)b * sP + j;
  const T* Z = Z_all + (size_t)b * sP + j;
  double acc[GTB][DIAG ? 1 : GTB];
#pragma unroll
  for (int ia = 0; ia < GTB; ++ia)
#pragma unroll
    for (int ib = 0; ib < (DIAG ? 1 : GTB); ++ib) acc[ia][ib] = 0.0;
#pragma unroll 2
  for (int i = r0; i < r1; ++i) {
    const T* yr = Y + (size_t)i * ld;
    const T* zr = Z + (size_t)i * ld;
    double ya[GTB], zb[GTB];
#pragma unroll
    for (int k = 0; k < GTB; ++k) {
      ya[k] = a0 + k < Dp ? (double)yr[(size_t)(a0 + k) * mb] : 0.0;
      zb[k] = b0 + k < Dp ? (double)zr[(size_t)(b0 + k) * mb] : 0.0;
    }
#pragma unroll
    for (int ia = 0; ia < GTB; ++ia) {
      if constexpr (DIAG) {
        acc[ia][0] = fma(ya[ia], zb[ia], acc[ia][0]);
      } else {
#pragma unroll
        for (int ib = 0; ib < GTB; ++ib) acc[ia][ib] = fma(ya[ia], zb[ib], acc[ia][ib]);
      }
    }
  }
  // the four waves' sums, ascending, one row of the register tile at a time
#pragma unroll
  for (int ib = 0; ib < (DIAG ? 1 : GTB); ++ib) {
    __syncthreads();
    if (w > 0) {
#pragma unroll
      for (int ia = 0; ia < GTB; ++ia) buf[w - 1][ia][lane] = acc[ia][ib];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int ia = 0; ia < GTB; ++ia) acc[ia][ib] = ((acc[ia][ib] + buf[0][ia][lane]) + buf[1][ia][lane]) + buf[2][ia][lane];
    }
  }
  if (w != 0) return;
  if constexpr (DIAG) {
    double* out = out_all + (((size_t)b * nseg + seg) * mb + j) * Dp;
#pragma unroll
    for (int ia = 0; ia < GTB; ++ia)
      if (a0 + ia < Dp) out[a0 + ia] = acc[ia][0];
  } else {
    double* out = out_all + (((size_t)b * nseg + seg) * mb + j) * Dp * Dp;
#pragma unroll
    for (int ia = 0; ia < GTB; ++ia)
#pragma unroll
      for (int ib = 0; ib < GTB; ++ib) {
        const int a = a0 + ia, bb = b0 + ib;
        if (a < Dp && bb <= a) {
          out[(size_t)a * Dp + bb] = acc[ia][ib];
          out[(size_t)bb * Dp + a] = acc[ia][ib];
        }
      }
  }
}

// out[b][e] = sum_seg part[b][seg][e], seg ascending (e < per).  grid = (per/256, batch)
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double* __restrict__ part, int nseg, long long per,
                                                          double* __restrict__ out) {
  const int b = blockIdx.y;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= per) return;
  double s = 0.0;
  for (int k = 0; k < nseg; ++k) s += part[((size_t)b * nseg + k) * per + e];
  out[(size_t)b * per + e] = s;
}

// The Gram matrices of `batch` panels into out (batch x mb x Dp x Dp, DIAG: batch x mb x Dp); part: room for
// batch * nseg of them when gram_segments(n) > 1 (else unused)
template <typename T>
inline hipError_t launch_block_gram(hipStream_t st, const T* Y, const T* Z, long long sP, int n, int mb, int Dp, int batch,
                                    bool diag, double* part, double* out) {
  const int nseg = gram_segments(n), nt = (Dp + GTB - 1) / GTB;
  const long long per = (long long)mb * Dp * (diag ? 1 : Dp);
  double* dst = nseg > 1 ? part : out;
  const dim3 grid(mb / WAVE, diag ? nt : nt * (nt + 1) / 2, batch * nseg);
  if (diag)
    hipLaunchKernelGGL((block_gram_kernel<T, true>), grid, dim3(256), 0, st, Y, Z, sP, n, mb, Dp, nseg, dst);
  else
    hipLaunchKernelGGL((block_gram_kernel<T, false>), grid, dim3(256), 0, st, Y, Z, sP, n, mb, Dp, nseg, dst);
  if (nseg > 1)
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)((per + 255) / 256), batch), dim3(256), 0, st,
                       (const double*)part, nseg, per, out);
  return hipGetLastError();
}

}  // namespace gpc
