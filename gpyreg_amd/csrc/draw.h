// draw.h -- joint posterior draws (gpc_draw): the Gaussian random stream and the element-wise passes around the
// batched factorization of C_s and the product F = L Z.
//
// Random stream (include/gpcore.h; restated in NumPy by gpyreg_amd/_philox.py): Philox4x64-10 under the key
// (seed, stream); the 64-bit word of row j of draw r of sample s (global index) is lane j % 4 of the block at
// counter (j / 4 + 1, r, s, 0).  Rows (2t, 2t + 1) form one Box-Muller pair.  A value depends on (seed, stream, s,
// r, j) only, so draws do not change with M, R, the chunking or the sharding.
#pragma once
#include "common.h"

namespace gpc {

struct PhiloxWords {
  unsigned long long w[4];
};

__device__ __forceinline__ PhiloxWords philox4x64_10(unsigned long long c0, unsigned long long c1,
                                                     unsigned long long c2, unsigned long long c3,
                                                     unsigned long long k0, unsigned long long k1) {
  constexpr unsigned long long M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
  constexpr unsigned long long W0 = 0x9E3779B97F4A7C15ull, W1 = 0xBB67AE8584CAA73Bull;
#pragma unroll
  for (int rnd = 0; rnd < 10; ++rnd) {
    if (rnd) {
      k0 += W0;
      k1 += W1;
    }
    const unsigned long long hi0 = __umul64hi(M0, c0), lo0 = M0 * c0;
    const unsigned long long hi1 = __umul64hi(M1, c2), lo1 = M1 * c2;
    const unsigned long long n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
  }
  return {{c0, c1, c2, c3}};
}

// the four normals of rows 4q .. 4q + 3 (two Box-Muller pairs from one Philox block)
__device__ __forceinline__ void normals4(unsigned long long seed, int stream, long long s, int r, long long q,
                                         double z[4]) {
  const PhiloxWords p = philox4x64_10((unsigned long long)q + 1ull, (unsigned long long)r, (unsigned long long)s, 0ull,
                                      seed, (unsigned long long)stream);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const double u1 = ((double)(p.w[2 * h] >> 11) + 1.0) * 0x1p-53;
    const double u2 = (double)(p.w[2 * h + 1] >> 11) * 0x1p-53;
    const double rad = sqrt(-2.0 * log(u1));
    const double ang = 2.0 * M_PI * u2;
    z[2 * h] = rad * cos(ang);
    z[2 * h + 1] = rad * sin(ang);
  }
}

// Z[b] (mpad x ldz, row-major: row j, column r) = z of rows j < M and draws r < R, 0 elsewhere (identity-padded
// factor: padding rows and columns stay out of the valid entries of L Z).  One thread per (4-row quad, column).
// grid = (ldz / 64, mpad / 16, batch), block = (64, 4)
template <typename T>
__global__ __launch_bounds__(256) void normals_kernel(unsigned long long seed, int stream, long long s_base, int M,
                                                      int R, int mpad, int ldz, T* __restrict__ Z_all, long long sZ) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  const int q = blockIdx.y * 4 + threadIdx.y;
  const int b = blockIdx.z;
  if (r >= ldz || 4 * q >= mpad) return;
  T* Z = Z_all + (size_t)b * sZ + (size_t)(4 * q) * ldz + r;
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  if (r < R && 4 * q < M) normals4(seed, stream, s_base + b, r, q, z);
#pragma unroll
  for (int e = 0; e < 4; ++e) Z[(size_t)e * ldz] = (4 * q + e < M) ? (T)z[e] : (T)0;
}

// out[b][j][r] (M x R doubles) = fmu[b][j] + F[b][j][r] (+ nsd[j * S + s_loc + b] z'[j][r], z' of stream 1 computed
// here: the noise is not a product operand).  One thread per (quad, column).   grid = (ceil(R / 64), mpad / 16,
// batch), block = (64, 4)
template <typename T>
__global__ __launch_bounds__(256) void draw_assemble_kernel(const T* __restrict__ F_all, long long sF, int ldf,
                                                            const double* __restrict__ fmu_all, int mpad, int M, int R,
                                                            const double* __restrict__ nsd, int S, int s_loc,
                                                            unsigned long long seed, long long s_base,
                                                            double* __restrict__ out_all) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  const int q = blockIdx.y * 4 + threadIdx.y;
  const int b = blockIdx.z;
  if (r >= R || 4 * q >= M) return;
  double zn[4] = {0.0, 0.0, 0.0, 0.0};
  if (nsd) normals4(seed, 1, s_base + b, r, q, zn);
  const T* F = F_all + (size_t)b * sF;
  const double* fmu = fmu_all + (size_t)b * mpad;
  double* out = out_all + (size_t)b * M * R;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = 4 * q + e;
    if (j >= M) break;
    double v = fmu[j] + (double)F[(size_t)j * ldf + r];
    if (nsd) v += nsd[(size_t)j * S + s_loc + b] * zn[e];
    out[(size_t)j * R + r] = v;
  }
}

// A[b] = lower triangle of C[b] + tau I on the M valid rows, zeros above the diagonal, identity padding: the input
// of the factorization (plan.h reads the lower tiles only; the zeros make the diagonal tiles of L clean triangular
// operands of F = L Z, the leaf writes the lower triangle only).   grid = (mpad / 64, mpad / 4, batch), block = (64, 4)
template <typename T>
__global__ void jitter_load_kernel(const T* __restrict__ C_all, T* __restrict__ A_all, long long sM, int mpad, int M,
                                   double tau) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int i = blockIdx.y * 4 + threadIdx.y;
  const int b = blockIdx.z;
  if (i >= mpad || j >= mpad) return;
  T v;
  if (i < M && j < M)
    v = j < i ? C_all[(size_t)b * sM + (size_t)i * mpad + j]
              : (j == i ? (T)((double)C_all[(size_t)b * sM + (size_t)i * mpad + j] + tau) : (T)0);
  else
    v = (i == j) ? (T)1 : (T)0;
  A_all[(size_t)b * sM + (size_t)i * mpad + j] = v;
}

// Zero the strictly upper part of every 128 x 128 diagonal tile of L[b]: the trailing updates A22 -= T21 T21^T (plan.h
// step 3) write whole diagonal tiles and the leaf leaves their upper part as it found it, while F = L Z reads the
// diagonal tiles whole.   grid = (mpad / 128, batch), block = 256
template <typename T>
__global__ __launch_bounds__(256) void diag_tile_upper_zero_kernel(T* __restrict__ L_all, long long sM, int mpad) {
  T* L = L_all + (size_t)blockIdx.y * sM + (size_t)blockIdx.x * TILE * ((size_t)mpad + 1);
  for (int idx = threadIdx.x; idx < TILE * TILE; idx += 256) {
    const int row = idx / TILE, col = idx % TILE;
    if (col > row) L[(size_t)row * mpad + col] = (T)0;
  }
}

// out[i] = z of rows j0 .. j0 + count - 1 of (stream, s, r) (gpc_debug_normals).   grid = ceil(count / 256), 256
__global__ void debug_normals_kernel(unsigned long long seed, int stream, long long s, int r, long long j0, int count,
                                     double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const long long j = j0 + i;
  double z[4];
  normals4(seed, stream, s, r, j >> 2, z);
  out[i] = z[j & 3];
}

}  // namespace gpc
