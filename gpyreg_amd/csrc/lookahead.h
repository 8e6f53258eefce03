// lookahead.h -- the stored-C form of the look-ahead reduction (gpc_predict_cov): weighted column sums of squares of a
// posterior cross covariance C (mapad x mbpad, row-major, zero padding) that the product has written.  The launches of
// at least 64 128-tiles never write C: their reduction runs in the product's epilogue (gemm.h: EPI = 2).
#pragma once
#include "common.h"

namespace gpc {

// out[b][j] = sum_i w[b][i] C[b][i][j]^2 over rows < nrows, in fp64 whatever T: wave q adds the rows q, q + 4, ...
// in ascending order, then the four waves are added in order -- fixed by the shape alone.  Rows of weight 0 (the
// padding) hold finite values and add exactly 0.  grid = (mpad/64, batch)
template <typename T>
__global__ __launch_bounds__(256) void wsq_col_kernel(const T* __restrict__ C_all, long long sC, int ld,
                                                      const double* __restrict__ w_all, int wstride, int nrows,
                                                      int mpad, double* __restrict__ out_all) {
  __shared__ double red[4][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const T* Cm = C_all + (size_t)b * sC;
  const double* w = w_all + (size_t)b * wstride;
  double s = 0.0;
  for (int i = q; i < nrows; i += 4) {
    const double v = (double)Cm[(size_t)i * ld + j];
    s = fma(w[i] * v, v, s);
  }
  red[q][lane] = s;
  __syncthreads();
  if (q == 0) out_all[(size_t)b * mpad + j] = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
}

// dst[i][j] (double, nr x nc dense) = src[i][j]: the valid corner of a padded rectangular matrix.
// grid = (ceil(nc/64), ceil(nr/4)), block = (64, 4)
template <typename T>
__global__ void extract_rect_kernel(const T* __restrict__ src, int ld, int nr, int nc, double* __restrict__ dst) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  const int i = blockIdx.y * 4 + threadIdx.y;
  if (i >= nr || j >= nc) return;
  dst[(size_t)i * nc + j] = (double)src[(size_t)i * ld + j];
}

}  // namespace gpc
