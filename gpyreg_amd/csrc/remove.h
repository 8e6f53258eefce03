// Kernels of the point removal: k training points taken out of resident posteriors in O(N^2 k)
// (gpc_post_remove; DESIGN.md "Point removal").  The inverse of the block append (block_append.h); no covariance is
// evaluated anywhere, so posteriors of either origin (device kernel, caller-provided K) take the same path.
//
// Per sample, I = the sorted removed rows, R = the kept rows in order, n = N - k:
//   high noise (A = Lo, W = Lo^-1):  Lr = Lo[R, R], Wr = W[R, R] (both still lower triangular), V = Lo[R, I] (n x k),
//     C = W[I, R] (k x n).  L' L'^T = Lr Lr^T + V V^T: for every 64-column panel [a, b) from the one that holds the
//     first removed row on, an orthogonal Theta of order 64 + k with [D | Vp] Theta = [D' | 0] (D = Lr[a:b, a:b],
//     Vp = V[a:b, :]) is formed by Householder reflections (rm_panel_kernel) and applied (rm_apply_kernel):
//       [Lr[b:, a:b] | V[b:, :]] <- [Lr[b:, a:b] | V[b:, :]] Theta,     [Wr[a:b, :b] ; C] <- Theta^T [Wr[a:b, :b] ; C]
//     After the last panel Lr = L', Wr = W' = L'^-1; alpha' = W'^T (W' (y_R - m_R)) / sl from the factor, never from
//     the old alpha.
//   low noise  (A = -(K + Sigma)^-1 = -Q, full symmetric):  Q_II = Lq Lq^T, Wq = Lq^-1 (the library's blocked
//     factorization, no jitter), H = A[R, I] Wq^T:   A' = A[R, R] + H H^T,   alpha' = alpha_R + A[R, I] Wq^T Wq alpha_I
// The carriers V, C, H and Theta are fp64 scratch whatever the storage type T of A and W.  Every kernel takes its
// sample from blockIdx, touches only that sample's data and sums in an order fixed by the shape: the bits of a sample
// do not depend on the batch.
#pragma once
#include "block_append.h"
#include "common.h"

namespace gpc {

constexpr int RM_P = 64;      // columns of a panel
constexpr int RM_KMAX = 64;   // rows one sweep removes; a larger k goes in consecutive sweeps
constexpr int RM_MP = RM_P + RM_KMAX;  // largest order of Theta
// The two limits inside which GP.remove_points takes the device path; outside it takes the full recompute (the get-only
// options "remove_max_panels" / "remove_min_rows" hand the constants to the Python layer, the test option
// "remove_force" lifts both).  RM_SWEEP_MAX_PANELS: the most panels a removal may sweep, summed over its sweeps;
// RM_MIN_KEPT_ROWS: the kept rows n = N - k must exceed it.  Measured on an MI355X (tools/remove_points_bench.py,
// profiles/remove_points_cfg3.json; fp64, wall ms, device path / full recompute on the reduced data):
//   N = 4096, S = 16, 64 panels:  last rows (no sweep) 2.4 / 14.2 at k = 1 .. 64, 4.1 / 13.2 at k = 128;
//     middle rows (32 panels) 10.4 / 14.5 at k = 1 .. 16 but 20.8 / 14.5 at k = 64 and 39.9 / 13.5 at k = 128;
//     first rows (64 panels) 19.1 / 14.5 at k = 1 .. 16, 40.0 / 14.7 at k = 64, 78.0 / 13.4 at k = 128
//   N = 400, S = 8, 7 panels:     last rows 0.43 / 0.70 at k = 1, 0.35 / 0.66 at 16, 0.40 / 0.67 at 64, 1.12 / 1.19 at 128 (two
//     sweeps, three panels); middle rows (4 panels) 1.01 / 0.73 at k = 5, 1.72 / 0.64 at 64; first rows 1.61 / 0.46 at k = 1
//   N = 100, S = 8, 2 panels:     last rows 0.36 / 0.19 at k = 1, 0.33 / 0.18 at 5, 0.35 / 0.18 at 16; middle 0.49 / 0.18;
//     first 0.62 / 0.18
// A panel costs 0.17 to 0.26 ms for k <= 16 and 0.35 to 0.58 ms at k = 64 whatever N and S: the chain of 64 dependent
// reflections in ONE workgroup per sample (rm_panel_kernel) is latency, not arithmetic, and the sweep is a chain of
// N / 64 of them.  So every sweep of more than one panel loses at N = 400, and at N = 4096 only a sweep of at most half
// the panels with k <= 16 wins (0.72 of the recompute).  One panel is the longest sweep that won at both sizes; the
// N = 4096 middle-rows win is given up with it rather than guessed at for sizes in between that were not measured.
// At N = 100 the device path loses at EVERY shape, the last rows included: compaction, carriers and the fixed launches
// cost 0.16 ms of device time where the whole recompute of one 128-tile (the two-launch small path) takes 0.18 ms of
// wall time.  So the reduced problem has to be larger than one tile; between 128 and 400 rows nothing was measured.
constexpr int RM_SWEEP_MAX_PANELS = 1;
constexpr int RM_MIN_KEPT_ROWS = TILE;

// k rounded up to the MFMA's K step of 16: the leading dimension of V, the row count of C; Theta's order is 64 + that
inline int rm_kq(int k) { return ((k + 15) / 16) * 16; }

// does sample b take the sweep (high noise) / the rank-k correction (low noise)?  par: block_append.h's layout
__device__ __forceinline__ bool rm_high(const double* __restrict__ par, int b) {
  return par[(size_t)b * BA_STRIDE + BA_LCH] != 0.0 && par[(size_t)b * BA_STRIDE + BA_PRE] != 0.0;
}

// ---- compaction -------------------------------------------------------------------------------------------------
// An[i][l] = Ao[R[i]][R[l]], Wn likewise (i, l < n), identity padding up to ldn.  W, and the factor of a high-noise
// sample, are written with exact zeros above the diagonal (blas1.h's triangular products read the diagonal tile
// whole).  The n x n part of a low-noise sample that takes the correction is left to rm_low_kernel, which streams it
// from the old storage with the correction added (one pass over it, not two); its padding is written here.
// rmap[i] = R[i].      grid = (ldn / 64, ldn / 4, batch), block = (64, 4)
template <typename T>
__global__ void rm_compact_kernel(const T* __restrict__ Ao_all, const T* __restrict__ Wo_all, long long sMo, int ldo,
                                  T* __restrict__ An_all, T* __restrict__ Wn_all, long long sMn, int ldn, int n,
                                  const int* __restrict__ rmap, const double* __restrict__ par) {
  const int b = blockIdx.z;
  const int l = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
  if (i >= ldn || l >= ldn) return;
  T a = (i == l) ? (T)1 : (T)0, w = a;
  bool write_a = true;
  if (i < n && l < n) {
    const size_t src = (size_t)b * sMo + (size_t)rmap[i] * ldo + rmap[l];
    const bool lch = par[(size_t)b * BA_STRIDE + BA_LCH] != 0.0;
    a = (lch && l > i) ? (T)0 : Ao_all[src];
    w = (l > i) ? (T)0 : Wo_all[src];
    write_a = lch || par[(size_t)b * BA_STRIDE + BA_PRE] == 0.0;
  }
  if (write_a) An_all[(size_t)b * sMn + (size_t)i * ldn + l] = a;
  Wn_all[(size_t)b * sMn + (size_t)i * ldn + l] = w;
}

// The carriers, extracted from the OLD storage in fp64:  V[i][j] = A[R[i]][I[j]] (ldn x kq; high noise: zero where
// R[i] < I[j], the factor is lower triangular),  C[j][i] = W[I[j]][R[i]] (kq x ldn; high noise only, zero where
// R[i] > I[j]).  Zero padding in both.      grid = (ceil(ldn * kq / 256), batch), 256 threads
template <typename T>
__global__ __launch_bounds__(256) void rm_carrier_kernel(const T* __restrict__ Ao_all, const T* __restrict__ Wo_all,
                                                         long long sMo, int ldo, int n, int k, int kq, int ldn,
                                                         const int* __restrict__ rmap, const int* __restrict__ idx,
                                                         const double* __restrict__ par, double* __restrict__ V_all,
                                                         double* __restrict__ C_all) {
  const int b = blockIdx.y;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)ldn * kq) return;
  const int i = (int)(e / kq), j = (int)(e - (long long)i * kq);
  double v = 0.0, cw = 0.0;
  if (i < n && j < k) {
    const bool lch = par[(size_t)b * BA_STRIDE + BA_LCH] != 0.0;
    const int r = rmap[i], q = idx[j];
    if (!lch || r > q) v = (double)Ao_all[(size_t)b * sMo + (size_t)r * ldo + q];
    if (lch && r < q) cw = (double)Wo_all[(size_t)b * sMo + (size_t)q * ldo + r];
  }
  V_all[(size_t)b * ldn * kq + (size_t)i * kq + j] = v;
  C_all[(size_t)b * ldn * kq + (size_t)j * ldn + i] = cw;
}

// alpha_n[i] = alpha_o[R[i]] (zero padding)       grid = (ldn / 256 rounded up, batch), 256 threads
__global__ __launch_bounds__(256) void rm_alpha_gather_kernel(const double* __restrict__ ao_all, int ldo,
                                                              double* __restrict__ an_all, int ldn, int n,
                                                              const int* __restrict__ rmap) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ldn) return;
  an_all[(size_t)b * ldn + i] = i < n ? ao_all[(size_t)b * ldo + rmap[i]] : 0.0;
}

// Low noise: the operand of the k x k factorization, Sc[b] (kp x kp, identity padding) = Q_II = -A[I, I] (high-noise
// samples get the identity: they ride through the batched factorization untouched), and aI[b][j] = alpha_o[I[j]].
// grid = (kp / 64, kp / 4, batch), block = (64, 4)
template <typename T>
__global__ void rm_qii_kernel(const T* __restrict__ Ao_all, long long sMo, int ldo, int k, int kq, int kp,
                              const int* __restrict__ idx, const double* __restrict__ par,
                              const double* __restrict__ ao_all, int ldao, T* __restrict__ Sc_all,
                              double* __restrict__ aI_all) {
  const int b = blockIdx.z;
  const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
  if (i >= kp || j >= kp) return;
  const bool low = par[(size_t)b * BA_STRIDE + BA_LCH] == 0.0;
  T v = (i == j) ? (T)1 : (T)0;
  if (low && i < k && j < k) {
    const int hi = max(i, j), lo = min(i, j);  // (built from the lower triangle and mirrored)
    v = -Ao_all[(size_t)b * sMo + (size_t)idx[hi] * ldo + idx[lo]];
  }
  Sc_all[(size_t)b * kp * kp + (size_t)i * kp + j] = v;
  if (i == 0 && j < kq) aI_all[(size_t)b * kq + j] = j < k ? ao_all[(size_t)b * ldao + idx[j]] : 0.0;
}

// ---- panel kernel -----------------------------------------------------------------------------------------------
// One workgroup per sample: Theta of one panel.  D (64 x 64 lower triangular, read in place at (a, a) of the factor)
// and Vp (rows a .. a+63 of V, fp64) are loaded TRANSPOSED into LDS: column j of [D | Vp]^T is (D[j][j], zeros, Vp[j][:])
// below its diagonal -- the rows j+1 .. 63 are structurally zero and stay so -- so reflection j is
//   H_j = I - tau_j u_j u_j^T,   u_j = e_j + [0 ; vn_j],  vn_j of length k
// built for a POSITIVE new diagonal (beta = +sqrt(d^2 + sigma), u1 = d - beta computed as -sigma / (d + beta): no
// cancellation; sigma = 0: H_j = I exactly).  Forward, j = 0 .. 63: the new column j of D' and the update of the columns
// to its right.  Backward, j = 63 .. 0: Theta = H_0 (H_1 (... H_63 I)); applying H_j changes row j (still e_j then:
// it is finished and goes straight to memory) and the bottom k rows, which live in LDS.  Sums run over i in four (two)
// fixed interleaved parts added in a fixed order.  D' is written in place (lower triangle only), Vp zeroed.
// Theta: mp x mp row-major, mp = 64 + kq, the padding rows / columns are the identity's.
// grid = (batch), 256 threads
template <typename T>
__global__ __launch_bounds__(256) void rm_panel_kernel(T* __restrict__ A_all, long long sA, int lda, int a,
                                                       double* __restrict__ V_all, long long sV, int kq,
                                                       double* __restrict__ Th_all, const double* __restrict__ par) {
  __shared__ double Dt[RM_P][RM_P + 1];        // Dt[j][c] = D[c][j]
  __shared__ double Vt[RM_KMAX][RM_P + 1];     // Vt[i][c] = Vp[c][i]; after step j column j holds vn_j
  __shared__ double Xb[RM_KMAX][RM_MP + 1];    // the bottom rows of Theta while it is accumulated
  __shared__ double red[4][RM_MP];
  __shared__ double tau[RM_P];
  const int b = blockIdx.x;
  if (!rm_high(par, b)) return;
  const int t = threadIdx.x, c = t & 63, g = t >> 6, lane = t & 63;
  const int mp = RM_P + kq;
  T* A = A_all + (size_t)b * sA + (size_t)a * lda + a;
  double* V = V_all + (size_t)b * sV + (size_t)a * kq;
  double* Th = Th_all + (size_t)b * mp * mp;
  for (int e = t; e < RM_P * RM_P; e += 256) {
    const int r = e >> 6, cc = e & 63;
    Dt[cc][r] = cc <= r ? (double)A[(size_t)r * lda + cc] : 0.0;
  }
  for (int e = t; e < RM_KMAX * RM_P; e += 256) {
    const int r = e / RM_KMAX, i = e - r * RM_KMAX;
    Vt[i][r] = i < kq ? V[(size_t)r * kq + i] : 0.0;
  }
  __syncthreads();
  // forward: the reflections, D' into Dt, vn_j into column j of Vt
  for (int j = 0; j < RM_P; ++j) {
    const double vj = Vt[lane][j];  // (every wave forms sigma for itself, in the same order)
    const double sigma = wave_sum(vj * vj);
    if (sigma == 0.0) {  // (block-uniform) nothing to annihilate: H_j = I
      if (t == 0) tau[j] = 0.0;
      continue;
    }
    const double d = Dt[j][j];
    const double beta = sqrt(d * d + sigma);
    const double u1 = -sigma / (d + beta);
    const double inv = 1.0 / u1, tj = -u1 / beta;
    // (row j of Dt is written by wave 0 alone, after the barrier below: every wave takes its copy BEFORE it, so that a
    // wave that lags behind wave 0 cannot see the updated entry)
    const double djc = Dt[j][c];
    double p = 0.0;
    if (c > j)
      for (int i = g; i < kq; i += 4) p += Vt[i][j] * Vt[i][c];
    red[g][c] = p;
    __syncthreads();
    if (c > j) {
      const double w = djc + inv * (((red[0][c] + red[1][c]) + red[2][c]) + red[3][c]);
      const double tw = tj * w;
      if (g == 0) Dt[j][c] = djc - tw;
      for (int i = g; i < kq; i += 4) Vt[i][c] -= tw * (Vt[i][j] * inv);
    }
    __syncthreads();
    if (c == j) {  // (column j is read by nobody until the backward pass)
      for (int i = g; i < kq; i += 4) Vt[i][j] *= inv;
      if (g == 0) {
        Dt[j][j] = beta;
        tau[j] = tj;
      }
    }
  }
  __syncthreads();
  for (int e = t; e < RM_P * RM_P; e += 256) {
    const int r = e >> 6, cc = e & 63;
    if (cc <= r) A[(size_t)r * lda + cc] = (T)Dt[cc][r];
  }
  for (int e = t; e < RM_P * kq; e += 256) V[e] = 0.0;
  // backward: Theta = H_0 ... H_63
  for (int e = t; e < RM_KMAX * RM_MP; e += 256) {
    const int i = e / RM_MP, q = e - i * RM_MP;
    Xb[i][q] = q == RM_P + i ? 1.0 : 0.0;
  }
  __syncthreads();
  const int q = t & (RM_MP - 1), h = t >> 7;
  for (int j = RM_P - 1; j >= 0; --j) {
    const double tj = tau[j];
    if (tj == 0.0) {  // (block-uniform)
      if (h == 0 && q < mp) Th[(size_t)j * mp + q] = q == j ? 1.0 : 0.0;
      continue;
    }
    double p = 0.0;
    if (q < mp)
      for (int i = h; i < kq; i += 2) p += Vt[i][j] * Xb[i][q];
    red[h][q] = p;
    __syncthreads();
    if (q < mp) {
      const double w = (q == j ? 1.0 : 0.0) + (red[0][q] + red[1][q]);
      const double tw = tj * w;
      if (h == 0) Th[(size_t)j * mp + q] = (q == j ? 1.0 : 0.0) - tw;
      for (int i = h; i < kq; i += 2) Xb[i][q] -= tw * Vt[i][j];
    }
    __syncthreads();
  }
  for (int e = t; e < kq * mp; e += 256) {
    const int i = e / mp, qq = e - i * mp;
    Th[(size_t)(RM_P + i) * mp + qq] = Xb[i][qq];
  }
}

// ---- apply kernel -----------------------------------------------------------------------------------------------
// Theta of panel [a, a + 64) applied to both sides in one launch, fp64 MFMA (16 x 16 x 4) with fp64 accumulation
// whatever the storage type.  Blocks x < nLb own 64 rows r0 = a + 64 + 64 x .. of the L side,
//   [Lr[r][a : a+64] | V[r][:]] <- [Lr[r][a : a+64] | V[r][:]] Theta
// the others 64 columns c0 = 64 (x - nLb) .. of the W side,
//   [Wr[a : a+64][c] ; C[:][c]] <- Theta^T [Wr[a : a+64][c] ; C[:][c]]
// (Wr is read and written on and below the diagonal only; C over all n columns).  A block stages ALL 64 + kq inputs
// of its rows (columns) in LDS before the barrier and stores after it, and no two blocks share an entry: in place is
// safe.  The four waves split the 16-wide tiles of the 64 + kq outputs (tile w and w + 4), each against the four tiles
// of the block's 64 rows (columns); Theta is read from memory, every entry once per block.  No atomics; the k sum runs
// in ascending order.
// grid = (nLb + nWb, batch), 256 threads
template <typename T>
__global__ __launch_bounds__(256) void rm_apply_kernel(T* __restrict__ A_all, T* __restrict__ W_all, long long sM, int ld,
                                                       int n, int a, double* __restrict__ V_all, double* __restrict__ C_all,
                                                       long long sV, int ldc, int kq, const double* __restrict__ Th_all,
                                                       int nLb, const double* __restrict__ par) {
  __shared__ double sh[RM_MP * (RM_P + 1)];  // L side: X[64][mp + 1]; W side: Z[mp][64 + 1]
  using acc_t = MM<double>::acc_t;
  const int b = blockIdx.y;
  if (!rm_high(par, b)) return;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int mp = RM_P + kq, ntile = mp / 16;
  const int li = lane & 15, lk = lane >> 4;
  const double* Th = Th_all + (size_t)b * mp * mp;
  double* V = V_all + (size_t)b * sV;
  double* C = C_all + (size_t)b * sV;
  acc_t acc[2][4];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = acc_t{0.0, 0.0, 0.0, 0.0};
  if ((int)blockIdx.x < nLb) {
    T* A = A_all + (size_t)b * sM;
    const int r0 = a + RM_P + (int)blockIdx.x * 64, ldx = mp + 1;
    for (int e = t; e < 64 * mp; e += 256) {
      const int r = e / mp, q = e - r * mp, row = r0 + r;
      double v = 0.0;
      if (row < n) v = q < RM_P ? (double)A[(size_t)row * ld + a + q] : V[(size_t)row * kq + (q - RM_P)];
      sh[r * ldx + q] = v;
    }
    __syncthreads();
    for (int q0 = 0; q0 < mp; q0 += 4) {
      double av[4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) av[rt] = sh[(rt * 16 + li) * ldx + q0 + lk];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int ct = w + 4 * u;
        if (ct < ntile) {  // (wave-uniform)
          const double bv = Th[(size_t)(q0 + lk) * mp + ct * 16 + li];
#pragma unroll
          for (int rt = 0; rt < 4; ++rt) acc[u][rt] = MM<double>::mma(av[rt], bv, acc[u][rt]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int ct = w + 4 * u;
      if (ct >= ntile) continue;
      const int col = ct * 16 + li;
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = r0 + rt * 16 + MM<double>::row_of(lane, e);
          if (row >= n) continue;
          if (col < RM_P) A[(size_t)row * ld + a + col] = (T)acc[u][rt][e];
          else V[(size_t)row * kq + (col - RM_P)] = acc[u][rt][e];
        }
    }
  } else {
    T* W = W_all + (size_t)b * sM;
    const int c0 = ((int)blockIdx.x - nLb) * 64, ldz = RM_P + 1;
    for (int e = t; e < mp * 64; e += 256) {
      const int q = e >> 6, cc = e & 63, col = c0 + cc;
      double v = 0.0;
      if (q < RM_P) {
        if (col <= a + q && a + q < n) v = (double)W[(size_t)(a + q) * ld + col];
      } else {
        v = C[(size_t)(q - RM_P) * ldc + col];
      }
      sh[q * ldz + cc] = v;
    }
    __syncthreads();
    for (int q0 = 0; q0 < mp; q0 += 4) {
      double bv[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) bv[ct] = sh[(q0 + lk) * ldz + ct * 16 + li];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int pt = w + 4 * u;
        if (pt < ntile) {
          const double av = Th[(size_t)(q0 + lk) * mp + pt * 16 + li];  // Theta^T[pt 16 + li][q0 + lk]
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) acc[u][ct] = MM<double>::mma(av, bv[ct], acc[u][ct]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int pt = w + 4 * u;
      if (pt >= ntile) continue;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int col = c0 + ct * 16 + li;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int p = pt * 16 + MM<double>::row_of(lane, e);
          if (p < RM_P) {
            if (col <= a + p && a + p < n) W[(size_t)(a + p) * ld + col] = (T)acc[u][ct][e];
          } else if (col < n) {
            C[(size_t)(p - RM_P) * ldc + col] = acc[u][ct][e];
          }
        }
      }
    }
  }
}

// ---- alpha of the high-noise samples: alpha[i] = au[i] / sl (au = W'^T W' (y_R - m_R)), i < n ----------------------
// grid = (ceil(npad / 256), batch), 256 threads
__global__ __launch_bounds__(256) void rm_alpha_high_kernel(double* __restrict__ alpha_all, int npad, int n,
                                                            const double* __restrict__ au_all,
                                                            const double* __restrict__ par) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npad || !rm_high(par, b)) return;
  alpha_all[(size_t)b * npad + i] = i < n ? au_all[(size_t)b * npad + i] / par[(size_t)b * BA_STRIDE + BA_SL] : 0.0;
}

// ---- low noise --------------------------------------------------------------------------------------------------
// alpha[i] += sum_j V[i][j] z[j]  (z = Q_II^-1 alpha_I), samples with ba_ok only.   grid = (ceil(n / 256), batch)
__global__ __launch_bounds__(256) void rm_alpha_low_kernel(double* __restrict__ alpha_all, int ldn, int n, int k, int kq,
                                                           const double* __restrict__ V_all,
                                                           const double* __restrict__ z_all,
                                                           const double* __restrict__ par, const int* __restrict__ info) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || par[(size_t)b * BA_STRIDE + BA_LCH] != 0.0 || !ba_ok(par, info, b)) return;
  const double* Vr = V_all + (size_t)b * ldn * kq + (size_t)i * kq;
  const double* z = z_all + (size_t)b * kq;
  double s = 0.0;
  for (int j = 0; j < k; ++j) s += Vr[j] * z[j];
  alpha_all[(size_t)b * ldn + i] += s;
}

// The rank-k correction while compacting, streamed from the OLD storage:  An[i][l] = Ao[R[i]][R[l]] + sum_j H[i][j] H[l][j]
// (i, l < n; H = A[R, I] Wq^T, n x k with leading dimension kq: its padding columns are never written and never
// read).  Every low-noise sample that the host's preconditions let through gets its n x n part from this kernel
// alone (rm_compact_kernel leaves it out): with the correction where Q_II factorized, the plain gather where not.  The sum runs over j in ascending order and its
// products commute: (i, l) and (l, i) get the same bits, the matrix stays symmetric to the bit.  The rows of H a block
// needs (64 for its columns, 16 for its rows) are staged in LDS, 16 columns at a time.
// grid = (ceil(n / 64), ceil(n / 16), batch), block = (64, 4): thread (tx, ty) owns An[i0 + 4 ty + e][l0 + tx]
template <typename T>
__global__ __launch_bounds__(256) void rm_low_kernel(const T* __restrict__ Ao_all, long long sMo, int ldo,
                                                     T* __restrict__ An_all, long long sMn, int ldn, int n, int k,
                                                     int kq, const int* __restrict__ rmap, const double* __restrict__ H_all,
                                                     const double* __restrict__ par, const int* __restrict__ info) {
  __shared__ double shL[64][BA_R + 1];
  __shared__ double shI[16][BA_R];
  const int b = blockIdx.z;
  if (par[(size_t)b * BA_STRIDE + BA_LCH] != 0.0 || par[(size_t)b * BA_STRIDE + BA_PRE] == 0.0) return;
  const bool corrected = info[b] == 0;  // (block-uniform) Q_II did not factorize: the plain gather, a stale sample
  const int tx = threadIdx.x, ty = threadIdx.y, t = ty * 64 + tx;
  const int l0 = blockIdx.x * 64, i0 = blockIdx.y * 16;
  const double* H = H_all + (size_t)b * ldn * kq;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < kq; j0 += BA_R) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int e = t + 256 * p, rr = e >> 4, cc = e & 15;
      shL[rr][cc] = (l0 + rr < n && j0 + cc < k) ? H[(size_t)(l0 + rr) * kq + j0 + cc] : 0.0;
    }
    {
      const int rr = t >> 4, cc = t & 15;
      shI[rr][cc] = (i0 + rr < n && j0 + cc < k) ? H[(size_t)(i0 + rr) * kq + j0 + cc] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < BA_R; ++q) {
      const double hl = shL[tx][q];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += shI[ty * 4 + e][q] * hl;
    }
    __syncthreads();
  }
  const int l = l0 + tx;
  if (l >= n) return;
  const int rl = rmap[l];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = i0 + ty * 4 + e;
    if (i >= n) continue;
    const double old = (double)Ao_all[(size_t)b * sMo + (size_t)rmap[i] * ldo + rl];
    An_all[(size_t)b * sMn + (size_t)i * ldn + l] = corrected ? (T)(old + acc[e]) : Ao_all[(size_t)b * sMo + (size_t)rmap[i] * ldo + rl];
  }
}

}  // namespace gpc
