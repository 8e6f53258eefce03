// lookahead_batch.h -- the step loop of the greedy look-ahead batch (gpc_lookahead_batch; DESIGN.md "Greedy look-ahead
// batch").  Per sample s the state is the posterior covariance C_s of [x_ref; x_cand] against x_cand, fp64 whatever the
// posterior's storage type: (Mr + Mc) rows of ld = Mc_pad doubles, the Mr reference rows first, zero in the padding
// columns.  Step t picks the candidate c_t with the largest mean gain and conditions on it:
//   l_s(a) = C_s^t(a, c_t) / sqrt(den_s(c_t)),   C_s^{t+1}(a, b) = C_s^t(a, b) - l_s(a) l_s(Mr + b)
// The REFERENCE block (rows < Mr) is kept current in place: lab_step_kernel applies the downdate of step t - 1 while it
// streams the block for the column sums of step t -- one read and one write of Mr x Mc doubles per step, whatever t.
// The CANDIDATE block (rows >= Mr) is never rewritten: only its column c_t is needed per step, and lab_col_kernel forms it
// from the stored C^0 and the l panels, C^0(a, c_t) - sum_{u < t} l_u(a) l_u(Mr + c_t), in ascending u.
// Every kernel takes its sample from blockIdx and adds in an order fixed by the shape alone; no atomics.  The launches of
// a step talk through device memory only (cur, sd, the l panel): the host enqueues all q steps without waiting.
#pragma once
#include "common.h"

namespace gpc {

constexpr int LB_T = 64;  // columns of a block and rows of a slab of the step kernel

// dst[b] (nr x ld doubles) = src[b] (T, leading dimension ld): the valid columns j < nc of the first nr rows of a
// product's padded result, zero in the padding columns.  grid = (ld / 64, ceil(nr / 4)), block = (64, 4)
template <typename T>
__global__ void lab_load_kernel(const T* __restrict__ src, int ld, int nr, int nc, double* __restrict__ dst) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int i = blockIdx.y * 4 + threadIdx.y;
  if (i >= nr || j >= ld) return;
  dst[(size_t)i * ld + j] = j < nc ? (double)src[(size_t)i * ld + j] : 0.0;
}

// One pass over the reference block of a step: C[r][j] -= lprev[r] lprev[Mr + j] (lprev: the l vector of the previous
// step, Mr + ld doubles per sample, zero behind the candidates; nullptr at step 0: nothing is written), then
//   part[b][slab][j] = sum_{r in slab} w[r] C[r][j]^2.
// A block owns 64 rows x 64 columns: thread (cx = t % 32, rg = t / 32) loads two adjacent columns (16 bytes) of the rows
// rg, rg + 8, ... of the slab, all eight loads issued before the first use, and adds them in ascending order; the eight
// row groups are added in ascending order through LDS.  grid = (ld / 64, ceil(Mr / 64), batch), 256 threads
__global__ __launch_bounds__(256) void lab_step_kernel(double* __restrict__ C_all, long long sC, int ld, int Mr,
                                                       const double* __restrict__ w_all,
                                                       const double* __restrict__ lprev_all, long long sL,
                                                       double* __restrict__ part_all, int nslab) {
  __shared__ double2 red[8][LB_T / 2];
  const int b = blockIdx.z, slab = blockIdx.y;
  const int cx = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int j = blockIdx.x * LB_T + 2 * cx;
  double* Cb = C_all + (size_t)b * sC;
  const double* w = w_all + (size_t)b * Mr;
  const double* lp = lprev_all ? lprev_all + (size_t)b * sL : nullptr;
  const int r0 = slab * LB_T + rg;
  double2 v[8];
  double wr[8], lr[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int r = r0 + 8 * k;
    const bool in = r < Mr;
    v[k] = in ? *reinterpret_cast<const double2*>(Cb + (size_t)r * ld + j) : make_double2(0.0, 0.0);
    wr[k] = in ? w[r] : 0.0;
    lr[k] = (in && lp) ? lp[r] : 0.0;
  }
  double lc0 = 0.0, lc1 = 0.0;
  if (lp) {
    lc0 = lp[Mr + j];
    lc1 = lp[Mr + j + 1];
  }
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int r = r0 + 8 * k;
    if (r < Mr) {
      if (lp) {
        v[k].x = fma(-lr[k], lc0, v[k].x);
        v[k].y = fma(-lr[k], lc1, v[k].y);
        *reinterpret_cast<double2*>(Cb + (size_t)r * ld + j) = v[k];
      }
      a0 = fma(wr[k] * v[k].x, v[k].x, a0);
      a1 = fma(wr[k] * v[k].y, v[k].y, a1);
    }
  }
  red[rg][cx] = make_double2(a0, a1);
  __syncthreads();
  if (threadIdx.x < LB_T) {
    const double* col = reinterpret_cast<const double*>(&red[0][0]) + threadIdx.x;
    double s = col[0];
#pragma unroll
    for (int g = 1; g < 8; ++g) s += col[g * LB_T];
    part_all[((size_t)b * nslab + slab) * ld + blockIdx.x * LB_T + threadIdx.x] = s;
  }
}

// gains[b][c] = (sum of the slab partials, ascending) / den, den = max(v[b][c], 0) + noise[b][c], 0 where den <= 0;
// score[c] = (sum over the samples, ascending) / batch, a NaN counted as -inf.  A block owns 64 columns (ld is a
// multiple of 64): thread (lane = t % 64, g = t / 64) forms the gains of column c under the samples g, g + 4, ...; the
// score needs them all, so after the barrier the g = 0 thread of a column adds what its block wrote, in ascending order
// whatever the split.  grid = (ld / 64), 256 threads
__global__ __launch_bounds__(256) void lab_score_kernel(const double* __restrict__ part, int nslab, int ld, int batch,
                                                        const double* __restrict__ v, const double* __restrict__ noise,
                                                        double* gains, double* __restrict__ score) {
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  for (int b = g; b < batch; b += 4) {
    const double* p = part + (size_t)b * nslab * ld + c;
    double wsq = p[0];
    for (int k = 1; k < nslab; ++k) wsq += p[(size_t)k * ld];
    const double den = fmax(v[(size_t)b * ld + c], 0.0) + noise[(size_t)b * ld + c];
    gains[(size_t)b * ld + c] = den > 0.0 ? wsq / den : 0.0;
  }
  __syncthreads();
  if (g != 0) return;
  double sc = 0.0;
  for (int b = 0; b < batch; ++b) sc += gains[(size_t)b * ld + c];
  sc /= (double)batch;
  score[c] = sc != sc ? -INFINITY : sc;
}

// is (va, ia) ahead of (vb, ib)?  The larger value, then the lower index; ib < 0: nothing yet.  A total order on the
// pairs, so the result of any reduction tree is the same.
__device__ __forceinline__ bool lab_ahead(double va, int ia, double vb, int ib) {
  return ia >= 0 && (ib < 0 || va > vb || (va == vb && ia < ib));
}

// Step t's choice: c_t = argmax of score over the candidates c < Mc not yet chosen.  Writes idx[t] = cur[0] = c_t,
// chosen[c_t] = 1, gain_out[t * batch + b] = gains[b][c_t] and sd[b] = sqrt(den_b(c_t)) (0 where den <= 0: the
// downdate of that sample is skipped).  One block of 256 threads.
__global__ __launch_bounds__(256) void lab_pick_kernel(const double* __restrict__ score, int Mc, int ld, int batch, int t,
                                                       const double* __restrict__ gains, const double* __restrict__ v,
                                                       const double* __restrict__ noise, int* __restrict__ chosen,
                                                       int* __restrict__ idx, int* __restrict__ cur,
                                                       double* __restrict__ sd, double* __restrict__ gain_out) {
  __shared__ double bv[256];
  __shared__ int bi[256];
  const int tid = threadIdx.x;
  double best = 0.0;
  int at = -1;
  for (int c = tid; c < Mc; c += 256) {
    if (chosen[c]) continue;
    const double s = score[c];
    if (lab_ahead(s, c, best, at)) best = s, at = c;
  }
  bv[tid] = best;
  bi[tid] = at;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h && lab_ahead(bv[tid + h], bi[tid + h], bv[tid], bi[tid])) {
      bv[tid] = bv[tid + h];
      bi[tid] = bi[tid + h];
    }
    __syncthreads();
  }
  const int ct = bi[0];  // (>= 0: the host launches at most Mc steps)
  if (ct < 0) return;
  for (int b = tid; b < batch; b += 256) {
    const double den = fmax(v[(size_t)b * ld + ct], 0.0) + noise[(size_t)b * ld + ct];
    sd[b] = den > 0.0 ? sqrt(den) : 0.0;
    gain_out[(size_t)t * batch + b] = gains[(size_t)b * ld + ct];
  }
  if (tid == 0) {
    idx[t] = ct;
    cur[0] = ct;
    chosen[ct] = 1;
  }
}

// Step t's l vector: lt[b][a] = C_b^t(a, c_t) / sd[b] for every row a < Mr + Mc (0 where sd[b] = 0), c_t = cur[0].
// Reference rows read the block that lab_step_kernel keeps current; candidate rows read the stored C^0 and take off the
// earlier steps' corrections from the l panels lpan[b][u][.] (u < t, Rl doubles each), ascending.  Candidate rows also
// lower their variance: v[b][a - Mr] -= l^2.  grid = (ceil((Mr + Mc) / 256), batch), 256 threads
__global__ __launch_bounds__(256) void lab_col_kernel(const double* __restrict__ C_all, long long sC, int ld, int Mr,
                                                      int Mc, const int* __restrict__ cur,
                                                      const double* __restrict__ sd, double* __restrict__ lpan_all,
                                                      long long sL, int Rl, int t, double* __restrict__ v) {
  const int b = blockIdx.y;
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= Mr + Mc) return;
  const int ct = cur[0];
  const double s = sd[b];
  double* lpan = lpan_all + (size_t)b * sL;
  double l = 0.0;
  if (s > 0.0) {
    double val = C_all[(size_t)b * sC + (size_t)a * ld + ct];
    if (a >= Mr)
      for (int u = 0; u < t; ++u) val = fma(-lpan[(size_t)u * Rl + a], lpan[(size_t)u * Rl + Mr + ct], val);
    l = val / s;
  }
  lpan[(size_t)t * Rl + a] = l;
  if (a >= Mr) v[(size_t)b * ld + (a - Mr)] -= l * l;
}

}  // namespace gpc
