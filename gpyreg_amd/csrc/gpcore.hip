// gpcore.hip -- libgpcore.so: C ABI (include/gpcore.h) over the HIP kernels.
//
// Path implemented (reference lines in parentheses):
//   covariance.compute              (covariance_functions.py:135-367, isotropic_...:104-221)
//   GP.__core_computation           (gaussian_process.py:2357-2521)
//   GP.update full-recompute loop   (gaussian_process.py:870-884)   -> gpc_posterior_batch
//   GP.predict K* solves            (gaussian_process.py:1741-1764) -> gpc_predict
// Data layout in HBM: every N x N matrix is row-major, padded to a multiple of 128 with
// an identity block (exactly inert for Cholesky, inverse, log-det and traces), one slab
// per hyperparameter sample, samples contiguous (batch stride = npad^2).
#include "../../include/gpcore.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>

#include "blas1.h"
#include "block_append.h"
#include "common.h"
#include "covfun.h"
#include "cv.h"
#include "cvgrad.h"
#include "draw.h"
#include "gemm.h"
#include "gradobs.h"
#include "gradpost.h"
#include "hess.h"
#include "hypgrad.h"
#include "nll_hess.h"
#include "leaf.h"
#include "lookahead.h"
#include "lookahead_batch.h"
#include "paths.h"
#include "plan.h"
#include "quad.h"
#include "quad_mix.h"
#include "remove.h"
#include "scratch.h"
#ifdef GPC_EXPERIMENTS
// Schedules that were built, measured and rejected -- the tile-level dataflow graph, independent
// per-sample pipelines, rectangular / eight-wave tiles, right-looking panels -- are compiled only into the experiments
// build (gpyreg_amd/build.py --experiments -> lib/libgpcore_exp.so), which tests/ and tools/ opt into through
// GPYREG_AMD_LIB.  The product library contains the shipped stream-ordered schedule and nothing else.
#include "dag.h"
#endif

using namespace gpc;

namespace {

std::string g_create_err;

// bumped whenever a device buffer is (re)allocated: cached launch graphs hold raw pointers
inline unsigned long long g_alloc_epoch = 0;

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t ensure(size_t need) {
    if (need <= bytes) return hipSuccess;
    ++g_alloc_epoch;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, need);
    if (e == hipSuccess) bytes = need;
    return e;
  }
  // for buffers no captured launch graph refers to (a posterior's private constants): no epoch bump
  hipError_t ensure_private(size_t need) {
    if (need <= bytes) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, need);
    if (e == hipSuccess) bytes = need;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <typename U>
  U* as() const {
    return reinterpret_cast<U*>(p);
  }
};

// Page-locked host staging for transfers between the caller's (pageable) arrays and HBM.
// Copies straight from/to pageable memory go through the runtime's pin-on-demand path, measured
// at ~20 ms of fixed host time for the first multi-MB copy of a call (S=1024, N=500: 30 ms per
// batched evaluation, 6 ms with staging); staging through long-lived pinned blocks costs a host
// memcpy (~30 GB/s) and makes the copy truly asynchronous.  Lifetime: begin() at the top of an
// entry point (the stream is idle there: every entry point ends with a sync), finish() after
// the final sync delivers the downloads.
// Gathered transfers of one call.  The boundary hands over 5-7 small host arrays per call (hyperparameter rows, mean,
// noise, their gradients' inputs) and takes back 3-6 (log det, quadratic form, info, gradients): as separate
// hipMemcpyAsync's each is a blit kernel of its own on the stream (~10 us apiece, 100-190 us per call against
// 250 us of device work for a single evaluation at N = 200).  Here the host side stages everything in ONE pinned
// block and one kernel moves the segments (the pinned block is mapped: the kernel reads / writes host memory over
// the bus directly) and zeroes the scalar block on the way.
struct XferSeg {
  void* dst;
  const void* src;
  unsigned long long n8;  // 8-byte words
};
struct XferDesc {
  static constexpr int MAXSEG = 8;
  XferSeg seg[MAXSEG];
  int nseg;
  void* zero;
  unsigned long long zero8;
  // optional: the scaled inputs of all samples (covfun.h: scale_x_kernel's arithmetic), mul / dv read from the
  // staged host copies, so that the first kernel of the pipeline is the covariance build itself
  const double* X = nullptr;
  const double* mul = nullptr;
  const double* dv = nullptr;
  double* xs = nullptr;
  int n = 0, npad = 0, D = 0, cnt = 0;
  // optional (gpc_nll_batch_cm: constant mean, and / or scalar noise): what the host would otherwise compute per point
  // and upload -- r[b][i] = y[i] - m0[b] from the RESIDENT y and the per-sample constant, dvec[b][i] = dval[b] (1 in
  // the identity padding) -- formed here; m0 / dval are staged host copies (one value per sample)
  const double* y = nullptr;
  const double* m0 = nullptr;
  double* r_out = nullptr;
  const double* dval = nullptr;
  double* dvec_out = nullptr;
  int fn = 0, fnpad = 0, fcnt = 0;
  // optional (the download launch of a call, round 6): the launch announces its own completion in host memory -- every
  // block makes its stores visible system-wide and counts itself in `done_ctr` (a device word the upload launch of the same
  // call zeroed), the last one stores `seq` into `flag` -- so that the host can watch that word instead of waiting for the
  // runtime's end-of-kernel signal (several microseconds later)
  unsigned long long* flag = nullptr;
  unsigned long long seq = 0;
  int* done_ctr = nullptr;
};
__device__ __forceinline__ void xfer_body_noxs(const XferDesc& d, unsigned long long gt, unsigned long long stride) {
  // the segments as ONE index space: a thread's words are independent loads from (mapped) host memory, all in flight
  // together -- a loop per segment made nseg dependent PCIe round trips of ~2.5 us each out of a small upload
  unsigned long long total = 0;
  for (int k = 0; k < d.nseg; ++k) total += d.seg[k].n8;
  // ... dealt to the blocks in contiguous chunks of equal size (a small upload read by the first block alone queues
  // behind that one CU's outstanding host reads: 8 us for 2.6 KB against 3.6 us for a third of it)
  const unsigned long long nblk = stride / 256, blk = gt / 256, lt = gt % 256;
  const unsigned long long chunk = (total + nblk - 1) / nblk;
  const unsigned long long hi = chunk * (blk + 1) < total ? chunk * (blk + 1) : total;
  for (unsigned long long i = chunk * blk + lt; i < hi; i += 256) {
    unsigned long long j = i;
    int k = 0;
    while (j >= d.seg[k].n8) {
      j -= d.seg[k].n8;
      ++k;
    }
    reinterpret_cast<unsigned long long*>(d.seg[k].dst)[j] = reinterpret_cast<const unsigned long long*>(d.seg[k].src)[j];
  }
  unsigned long long* z = reinterpret_cast<unsigned long long*>(d.zero);
  for (unsigned long long i = gt; i < d.zero8; i += stride) z[i] = 0ull;
  if (d.r_out || d.dvec_out) {
    const unsigned long long tot = (unsigned long long)d.fnpad * d.fcnt;
    for (unsigned long long q = gt; q < tot; q += stride) {
      // the sample index is the same for the 64 lanes of a wave (gt is wave-contiguous from a multiple of 64, stride
      // a multiple of 256, fnpad a multiple of 128): the two per-sample constants are read from the mapped host block
      // ONCE per wave through the scalar unit, not once per element (S * npad uncached PCIe reads)
      const int b = __builtin_amdgcn_readfirstlane((int)(q / d.fnpad));
      const int i = (int)(q - (unsigned long long)b * d.fnpad);
      if (d.r_out) {
        const double m0b = d.m0[b];
        d.r_out[q] = i < d.fn ? d.y[i] - m0b : 0.0;
      }
      if (d.dvec_out) {
        const double dvb = d.dval[b];
        d.dvec_out[q] = i < d.fn ? dvb : 1.0;
      }
    }
  }
}
__device__ __forceinline__ void xfer_body(const XferDesc& d, unsigned long long gt, unsigned long long stride) {
  xfer_body_noxs(d, gt, stride);
  if (d.xs) {
    const unsigned long long per = (unsigned long long)d.npad * d.D, tot = per * d.cnt;
    for (unsigned long long q = gt; q < tot; q += stride) {
      const unsigned long long b = q / per, idx = q - b * per;
      const int i = (int)(idx / d.D), h = (int)(idx % d.D);
      double v = 0.0;
      if (i < d.n) v = d.X[(size_t)i * d.D + h] * d.mul[b * d.D + h] / d.dv[b * d.D + h];
      d.xs[q] = v;
    }
  }
}
__global__ __launch_bounds__(256) void xfer_kernel(XferDesc d) {
  xfer_body(d, (unsigned long long)blockIdx.x * 256 + threadIdx.x, (unsigned long long)gridDim.x * 256);
  if (d.flag) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
      // (done_ctr == nullptr: a launch of ONE workgroup -- it is its own last one)
      const int before = d.done_ctr ? __hip_atomic_fetch_add(d.done_ctr, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) : 0;
      if (before == (int)gridDim.x - 1) __hip_atomic_store(d.flag, d.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// Problems that are one 128 x 128 leaf (N <= 128): the upload kernel and the covariance build in ONE launch.
// grid = (3 lower 64-tiles, samples).  Every block takes its share of the gathered upload (xfer_body: the segments land
// in their device buffers for the kernels that follow), then scales the 128 rows of its sample's inputs by itself --
// every block of a sample writes the same values: each needs rows of both halves -- and builds its tile, reading the
// per-sample scalars and the diagonal term from the STAGED HOST COPIES (`sp_h`, `dvec_h`: mapped pinned memory; the
// device copies are being written by other blocks of this very launch and are not ordered against this read).
template <typename T, int KIND, int DEG>
__global__ __launch_bounds__(256) void small_front_kernel(XferDesc d, CovDesc cd, const double* __restrict__ sp_h,
                                                          const double* __restrict__ dvec_h, int dvec_vec,
                                                          T* __restrict__ A_all, long long sA) {
  __shared__ double xi[CT][DCH + 1];
  __shared__ double xj[CT][DCH + 1];
  // this sample's host-resident inputs, fetched ONCE: a load from mapped host memory is a PCIe round trip (~2.5 us),
  // and the code below would otherwise make four dependent ones (scaling factors, scalars, diagonal term)
  constexpr int DL = 64;  // input dimensions whose scaling factors are kept in LDS (more: read from the host copy)
  __shared__ double h_sp[SP_STRIDE], h_dvec[TILE], h_mul[DL], h_dv[DL];
  const int b = blockIdx.y, t = threadIdx.x;
#ifdef GPC_FRONT_TRACE
  long long ts[6];
  ts[0] = wall_clock64();
#endif
  const bool dl = d.D <= DL;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  // the diagonal term is read by the diagonal tiles only (tile 0: rows 0..63, tile 2: rows 64..127)
  const int drow = blockIdx.x == 2 ? CT : 0;
  const bool dg = blockIdx.x != 1 && t < CT;
  // (dvec_vec = 0: one value per sample -- scalar noise; the padding rows carry 1 either way)
  if (dg) v0 = dvec_vec ? dvec_h[(size_t)b * TILE + drow + t] : (drow + t < d.n ? dvec_h[b] : 1.0);
  if (t < SP_STRIDE) v1 = sp_h[(size_t)b * SP_STRIDE + t];
  if (dl && t < d.D) {
    v2 = d.mul[(size_t)b * d.D + t];
    v3 = d.dv[(size_t)b * d.D + t];
  }
  xfer_body_noxs(d, ((unsigned long long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x,
                 (unsigned long long)gridDim.x * gridDim.y * 256);
#ifdef GPC_FRONT_TRACE
  ts[1] = wall_clock64();
#endif
  if (dg) h_dvec[drow + t] = v0;
  if (t < SP_STRIDE) h_sp[t] = v1;
  if (dl && t < d.D) {
    h_mul[t] = v2;
    h_dv[t] = v3;
  }
  __syncthreads();
#ifdef GPC_FRONT_TRACE
  ts[2] = wall_clock64();
#endif
  double* xs = d.xs + (size_t)b * d.npad * d.D;
  const double* mulp = dl ? h_mul : d.mul + (size_t)b * d.D;
  const double* dvp = dl ? h_dv : d.dv + (size_t)b * d.D;
  for (int q = t; q < d.npad * d.D; q += 256) {
    const int i = q / d.D, h = q - i * d.D;
    xs[q] = i < d.n ? d.X[(size_t)i * d.D + h] * mulp[h] / dvp[h] : 0.0;
  }
  __syncthreads();  // (a block reads back only what it wrote itself)
#ifdef GPC_FRONT_TRACE
  ts[3] = wall_clock64();
#endif
  // sample index 0 for the scalars and the diagonal term: the LDS copies hold this block's sample only
  build_tile_at<T, KIND, DEG>(cd, d.xs, h_sp, h_dvec, d.n, d.npad, A_all, sA, d.npad, blockIdx.x, b, 0, xi, xj);
#ifdef GPC_FRONT_TRACE
  __syncthreads();
  ts[4] = wall_clock64();
  if (t == 0 && b == 0)
    printf("front tile %d: copy %lld  lds %lld  xs %lld  build %lld  (10 ns ticks)\n", (int)blockIdx.x, ts[1] - ts[0],
           ts[2] - ts[1], ts[3] - ts[2], ts[4] - ts[3]);
#endif
}

struct PinBuf {
  struct Blk {
    char* p;
    size_t bytes, used;
  };
  struct Pending {
    void* dst;
    const void* src;
    size_t n;
  };
  std::vector<Blk> blks;
  std::vector<Pending> pend;
  static constexpr size_t kMin = 32u << 10;    // smaller copies: the runtime's own staging is fine
  static constexpr size_t kMax = 512ull << 20; // larger ones amortise the pin-on-demand cost themselves

  void begin() {
    pend.clear();
    if (blks.size() > 1) {  // the previous call outgrew its block: one block of the total next time
      size_t tot = 0;
      for (Blk& b : blks) {
        tot += b.bytes;
        (void)hipHostFree(b.p);
      }
      blks.clear();
      (void)alloc(tot);
    }
    for (Blk& b : blks) b.used = 0;
  }
  void* alloc(size_t n) {
    n = (n + 255) & ~(size_t)255;
    if (!blks.empty() && blks.back().used + n <= blks.back().bytes) {
      void* r = blks.back().p + blks.back().used;
      blks.back().used += n;
      return r;
    }
    Blk b{nullptr, std::max(n + n / 2, (size_t)4 << 20), 0};
    if (hipHostMalloc(reinterpret_cast<void**>(&b.p), b.bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    b.used = n;
    blks.push_back(b);
    return b.p;
  }
  hipError_t up(void* dst, const void* src, size_t n, hipStream_t st) {
    if (n >= kMin && n <= kMax)
      if (void* h = alloc(n)) {
        memcpy(h, src, n);
        src = h;
      }
    return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st);
  }
  // the data lands in dst at finish(), which the caller runs after synchronising the stream
  hipError_t down(void* dst, const void* src, size_t n, hipStream_t st) {
    if (n >= kMin && n <= kMax)
      if (void* h = alloc(n)) {
        pend.push_back({dst, h, n});
        dst = h;
      }
    return hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st);
  }
  void finish() {
    for (Pending& q : pend) memcpy(q.dst, q.src, q.n);
    pend.clear();
  }
  // ---- gathered form: stage() any number of uploads (<= MAXSEG), flush_up() moves them with one kernel;
  // gather() downloads likewise, flush_down() + (after the stream is synchronised) finish().
  // Falls back to individual copies when a segment is not 8-byte sized, the total is large enough for the copy
  // engines to win (kGather), or pinned memory is not to be had.
  static constexpr size_t kGather = 2u << 20;
  XferDesc upd{}, downd{};
  std::vector<Pending> up_fallback;
  void begin_gather() {
    upd.nseg = downd.nseg = 0;
    upd.xs = nullptr;
    upd.r_out = upd.dvec_out = nullptr;
    upd.zero = downd.zero = nullptr;
    upd.zero8 = downd.zero8 = 0;
    up_fallback.clear();
    gathered_bytes = 0;
    down_plain = false;
  }
  size_t gathered_bytes = 0;
  // returns the staged (pinned, device-readable) copy, or nullptr when the segment travels by itself
  const void* stage(void* dst, const void* src, size_t n) {
    if (n == 0) return nullptr;
    void* h = (n % 8 == 0 && upd.nseg < XferDesc::MAXSEG && gathered_bytes + n <= kGather) ? alloc(n) : nullptr;
    if (!h) {
      up_fallback.push_back({dst, src, n});
      return nullptr;
    }
    memcpy(h, src, n);
    upd.seg[upd.nseg++] = {dst, h, (unsigned long long)(n / 8)};
    gathered_bytes += n;
    return h;
  }
  hipError_t flush_up(hipStream_t st, void* zero, size_t zero_bytes) {
    for (Pending& q : up_fallback) {
      hipError_t e = up(q.dst, q.src, q.n, st);
      if (e != hipSuccess) return e;
    }
    up_fallback.clear();
    if (zero_bytes % 8) {
      hipError_t e = hipMemsetAsync(zero, 0, zero_bytes, st);
      if (e != hipSuccess) return e;
      zero_bytes = 0;
    }
    upd.zero = zero;
    upd.zero8 = zero_bytes / 8;
    if (upd.nseg == 0 && upd.zero8 == 0 && !upd.xs && !upd.r_out && !upd.dvec_out) return hipSuccess;
    const unsigned long long words = gathered_bytes / 8 + upd.zero8 + (upd.xs ? (unsigned long long)upd.npad * upd.D * upd.cnt : 0ull) +
                                     ((upd.r_out || upd.dvec_out) ? (unsigned long long)upd.fnpad * upd.fcnt : 0ull);
    const int blocks = (int)std::min<unsigned long long>(256, (words + 255) / 256);
    hipLaunchKernelGGL(xfer_kernel, dim3(std::max(1, blocks)), dim3(256), 0, st, upd);
    upd.nseg = 0;
    return hipGetLastError();
  }
  // flush_up without the launch: the fallback copies go out, `out` receives the descriptor of the gathered segments
  // (the caller's own kernel moves them: small_front_kernel)
  hipError_t take_up(hipStream_t st, void* zero, size_t zero_bytes, XferDesc& out) {
    for (Pending& q : up_fallback) {
      hipError_t e = up(q.dst, q.src, q.n, st);
      if (e != hipSuccess) return e;
    }
    up_fallback.clear();
    if (zero_bytes % 8) {
      hipError_t e = hipMemsetAsync(zero, 0, zero_bytes, st);
      if (e != hipSuccess) return e;
      zero_bytes = 0;
    }
    upd.zero = zero;
    upd.zero8 = zero_bytes / 8;
    out = upd;
    upd.nseg = 0;
    return hipSuccess;
  }
  // dst: host; the data lands there at finish()
  bool down_plain = false;  // a download of this call travelled as a plain copy (the gathered launch does not cover it)
  hipError_t gather(void* dst, const void* src, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    void* h = (n % 8 == 0 && downd.nseg < XferDesc::MAXSEG && n <= kGather / 8) ? alloc(n) : nullptr;
    if (!h) {
      down_plain = true;
      return hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st);
    }
    pend.push_back({dst, h, n});
    downd.seg[downd.nseg++] = {h, src, (unsigned long long)(n / 8)};
    return hipSuccess;
  }
  // flag / seq / done_ctr: see XferDesc (nullptr: the caller synchronises the stream)
  hipError_t flush_down(hipStream_t st, unsigned long long* flag = nullptr, unsigned long long seq = 0, int* done_ctr = nullptr) {
    if (downd.nseg == 0) return hipSuccess;
    unsigned long long words = 0;
    for (int k = 0; k < downd.nseg; ++k) words += downd.seg[k].n8;
    int blocks = (int)std::min<unsigned long long>(64, (words + 255) / 256);
    if (flag && !done_ctr) blocks = 1;  // (no zeroed counter at hand: one workgroup moves the few KB and announces itself)
    downd.flag = flag;
    downd.seq = seq;
    downd.done_ctr = done_ctr;
    hipLaunchKernelGGL(xfer_kernel, dim3(std::max(1, blocks)), dim3(256), 0, st, downd);
    downd.nseg = 0;
    downd.flag = nullptr;
    return hipGetLastError();
  }
  void release() {
    for (Blk& b : blks) (void)hipHostFree(b.p);
    blks.clear();
    pend.clear();
  }
};

}  // namespace

struct gpc_ctx {
  int device = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  static constexpr int MAXG = 8;
  hipStream_t gst[MAXG] = {};  // sample-group streams
  hipStream_t sst[MAXG + 1] = {};  // side streams of the deferred inverse products (plan.h), one per group + main
  static constexpr int NDEV = 64;
  hipEvent_t dev_ev[MAXG + 1][NDEV] = {};
  hipEvent_t ev_bfork[MAXG + 1] = {}, ev_btail[MAXG + 1] = {};  // split kernel build (device_section)
  // GPC_DEFER_MIN: node size from which U = T21 W11 runs on the side stream (0 off, -1 auto: the top two
  // levels when the batch is small enough for latency-bound phases to matter); GPC_DEFER_RESERVE: CUs per
  // XCD the deferred launch keeps empty (2, 4, 8, 12)
  int defer_min = -1, defer_reserve = 8;
  // The device's own numbering of shader engines and CUs, probed at gpc_create (probe_cu_map): cu_seen[xcc * 8 + se]
  // = bit mask of the CU_IDs workgroups were observed on.  The table of reserved CUs (rsv_tbl, same indexing; read
  // by common.h: cu_reserve_bail) is derived from it, so nothing about the harvesting map is assumed.  cu_map_ok:
  // the probe saw every CU the runtime reports, the same number in every engine; otherwise the deferred schedule
  // (which needs empty CUs to pay) is off.
  unsigned cu_seen[64] = {};
  bool cu_map_ok = false;
  DevBuf rsv_tbl;
  // NLL-only evaluations: largest diagonal block that gets its inverse (plan.h: potrf_nll).  0: round-2 scheme (every
  // left child inverted); -1: automatic -- 512 from npad = 2048 on, else 0.  The choice depends on the problem size
  // ONLY, never on the batch: a row of a batch must carry the bits of its single evaluation (the speculative slice
  // sampler relies on it, slice_sample.py), and the two schemes differ in rounding.
  // Measured (round-3 sweep, script since removed; ms per batch at block 0 / 256 / 512 / 1024): cfg3 S=16 8.85 / 8.50 / 8.41 / 8.46;
  // N=8192 S=8 29.8 / 28.1 / 27.5 / 27.5; N=2048 S=16 1.98 / 1.95 / 1.89 / 2.00; single samples and small batches are
  // launch-bound and lose with the extra launches of the blocked solves (N=4096 S=1 2.28 / 2.42 / 2.30 / 2.28;
  // N=2048 S=1 0.96 / 1.01 / 0.98 / 0.98; N=1000 S=8 0.52 / 0.53 / 0.54 / 0.54): below npad = 2048 the round-2 scheme stays.
  int nll_block = -1;
  int tri_skip = 1;  // option: the evaluation pipeline's launches name their triangular operands (plan.h: Factor::tri_skip)
  int solves_beside_lauum = 1;  // option: the two triangular mat-vecs of a gradient evaluation run under the W^T W launch
#ifdef GPC_EXPERIMENTS
  // right-looking panels with look-ahead for NLL-only evaluations (plan.h: potrf_rl): panel height; 0 = off (default)
  int rl_panel = 0;
  int rl_ahead_max = 8;  // look-ahead (side stream + reserved CUs) only for batches with S (npad/4096)^3 <= this
#endif
  int stable = 0;        // option: every factorization in stable mode (plan.h), not only the jitter retries
  int small_path = 1;    // option: problems of one 128 x 128 leaf take the two-launch pipeline (Pipe::small_section)
  // One-leaf evaluations without gradient (round 6): the host watches a word of a COHERENT pinned block that the last
  // block of the call writes, instead of hipStreamSynchronize (the runtime's completion path costs several microseconds
  // after the kernel's last store), and the four timing events of a call -- each a barrier packet on the stream -- are
  // recorded only when "small_timing" is set (gpc_last_timing then reports the device section; 0 otherwise).
  int small_poll = 1, small_timing = 0;
  double* land_blk = nullptr;            // hipHostMallocCoherent, LAND_BYTES
  static constexpr size_t LAND_BYTES = 64u << 10;
  unsigned long long land_seq = 0;
  unsigned long long small_polled = 0, small_synced = 0;  // statistics ("small_polled" / "small_synced")
  int last_chunk = 0;  // what plan_chunk last returned ("last_chunk")
  unsigned long long grad_post_gram_us = 0;  // Gram passes of the last gpc_grad_post, device microseconds ("grad_post_gram_us")
  unsigned long long gobs_trace_us = 0;  // the contraction (kernel + reduction) of the last gpc_debug_gobs_trace, device microseconds
  unsigned long long gobs_grad_operand_us = 0;  // the operand builds of the last gpc_grad_post_gobs (timed calls) / gpc_debug_gobs_grad_operand, device microseconds
  unsigned long long gobs_cov_us = 0, gobs_cross_us = 0;  // the kernel of the last gpc_debug_gobs_cov / the build of the last gpc_debug_gobs_cross, device microseconds
  unsigned long long hess_contract_us = 0;  // contraction passes of the last gpc_predict_hess, device microseconds ("hess_contract_us")
  unsigned long long nll_hess_gram_us = 0, nll_hess_contract_us = 0;  // Gram pass / second-derivative contraction of the last gpc_nll_hess, device microseconds
  unsigned long long cv_grad_trace_us = 0;  // contraction pass of the last gpc_cv_grad, device microseconds ("cv_grad_trace_us")
  unsigned long long lookahead_batch_loop_us = 0;  // the q steps of the last gpc_lookahead_batch, device microseconds
  unsigned long long cov_fused = 0;  // gpc_predict_cov calls whose reduction ran in the product's epilogue ("cov_fused")
  unsigned long long quad_mix_gemms = 0;  // MFMA GEMM launches inside gpc_quad_mix ("quad_mix_gemms"; there should be none)
  int check_queues = 0;  // debug option: verify after every pipeline that the tile queues of its persistent launches were drained
  hipEvent_t ev_up = nullptr, ev_done[MAXG] = {};
  int groups = 2;
  hipEvent_t ev_l0[MAXG + 1] = {}, ev_l1[MAXG + 1] = {};  // around the lauum launch of each group
  double ms_lauum = 0, flops_lauum = 0;  // slowest group's lauum launch of the last call
  int lauum_groups = 0;
  std::string err;
  std::string devinfo;
  // resident training data
  int N = 0, D = 0, npad = 0;
  DevBuf dX;  // N x D
  DevBuf dY;  // N (gpc_nll_batch_cm forms r = y - m0 on the device)
  // gradient observations (gpc_set_data_gobs; gradobs.h): gobs.Ng > 0 says that N above is the JOINT order N + Ng D and
  // hy / dY the joint target; dX is not used then -- the raw point list (gobs.P() x D) is gpts, gxs its scaled copies
  GobsDims gobs;
  DevBuf gpts, gxs;
  std::vector<double> hy;
  // workspace
  DevBuf mA, mW, mT;             // matrices of the current chunk
  DevBuf xs, spb, mulb, divb;    // scaled inputs and per-sample scalars
  DevBuf dvec, rvec, zvec, avec; // per-sample vectors (npad each)
  DevBuf tpart;                  // W^T z partial sums
  DevBuf scal;                   // logdet | quad | (ints) info
  DevBuf parts, gout, diagq;     // trace pass
  DevBuf dmb, dsn2b, mg, ng;     // mean / noise gradient inputs and outputs
  // Consumer scratch: every posterior consumer declares its device arrays once (scratch.h: a *Scratch struct's layout())
  // and carves them from ONE block.  Calls on a context are serial, so the consumers that never run inside one another
  // share `cs`: rhs_products (predict, predict_full, quad, quad_grad, predict_K, predict_gobs, draw), grad_post,
  // predict_hess, append_block, remove (its sweeps), cv (both passes; the fold pass follows the leave-one-out pass of a
  // mixed call, it does not run inside it), paths_create, paths_eval and predict_hyp_grad's raw queries.  The nesting
  // there is: lookahead_batch_impl runs cov_products while its own `lab` is live (gpc_predict_cov runs it alone), so
  // cov_products carves from `covs`, a block of its own; posterior_q (under nll_hess and cv_grad) writes into its
  // caller's nhs block and takes nothing itself.
  DevBuf cs, covs;
  DevBuf qmix;                   // quad_mix: the whole scratch of a chunk, carved up in quad_mix_impl
  DevBuf nhs;                    // nll_hess: the whole scratch of a chunk, carved up in nll_hess_impl (scratch.h: NhScratch)
  DevBuf lab;                    // lookahead_batch: the resident state of the step loop, carved up in lookahead_batch_impl (scratch.h: LabScratch)
  DevBuf hgs;                    // predict_hyp_grad: the whole scratch of a chunk, carved up in hyp_grad_impl (scratch.h: HgScratch)
  DevBuf dbg1, dbg2, dbg3;       // debug hooks / fetch staging / the pipeline's K-mode and trace staging
  PinBuf pin;                    // pinned staging for host<->device transfers (see PinBuf)
  // Launch graphs of the device pipeline for small problems (npad <= graph_max_npad, one sample
  // group): a single evaluation at N = 200 is ~20 dependent launches of a few microseconds each,
  // so the launch sequence is captured once per shape and replayed (hipGraphLaunch).
  struct GraphEntry {
    unsigned long long key[4] = {0, 0, 0, 0};
    unsigned long long epoch = 0;
    hipGraphExec_t exec = nullptr;
    unsigned long long last_use = 0;
    double flops = 0;  // algorithmic flops of the captured sequence (host-side bookkeeping)
  };
  static constexpr int NGRAPH = 16;
  GraphEntry graphs[NGRAPH];
  unsigned long long graph_clock = 0;
  int graph_max_npad = 4096;     // GPC_GRAPH_MAX_NPAD (0 disables)
  bool capturing = false;
  DevBuf tile_ctr;               // counters of the persistent GEMM launches, CTR_PER_GROUP per sample group
  static constexpr int CTR_PER_GROUP = 1024;
  // Freed posterior storage, kept for the next gpc_posterior_batch: hipMalloc/hipFree of the
  // multi-GB S x npad^2 factors cost more than computing them (update() in a fit / active-learning
  // loop creates a new posterior set and drops the previous one every iteration).
  std::vector<DevBuf> pool;
  DevBuf pool_take(size_t need) {
    int best = -1;
    for (int i = 0; i < (int)pool.size(); ++i)
      if (pool[i].bytes >= need && pool[i].bytes <= need + need / 2 &&
          (best < 0 || pool[i].bytes < pool[best].bytes))
        best = i;
    DevBuf r;
    if (best >= 0) {
      r = pool[best];
      pool.erase(pool.begin() + best);
    }
    return r;
  }
  void pool_give(DevBuf& b) {
    if (!b.p) return;
    pool.push_back(b);
    b.p = nullptr;
    b.bytes = 0;
    while (pool.size() > 6) {  // two generations of (A, W, alpha)
      pool.front().release();
      pool.erase(pool.begin());
    }
  }
  void pool_drain() {
    for (DevBuf& b : pool) b.release();
    pool.clear();
  }
  double ms_total = 0, ms_factor = 0;
  double last_flops = 0;
  // test hooks (gpc_set_option): first jitter multiplier of every factorization (the reference
  // starts at 1, gaussian_process.py:2402) and samples whose rank-one append is declared unstable
  double start_mult = 1.0;
  unsigned append_fail_mask = 0;
  int block_engine_ran = 0;  // the engine the last gpc_post_append_block ran (1: skinny kernel, 2: MFMA GEMM; get-only)
  int block_engine = 0;  // test hook: the engine of the block append's products with W (0: by k, 1: skinny kernel, 2: MFMA GEMM)
  long long block_appended = 0, block_stale = 0;  // samples gpc_post_append_block appended / left stale (get-only options)
  unsigned remove_fail_mask = 0;  // test hook: samples gpc_post_remove declares stale
  int remove_force = 0;           // test hook: "remove_max_panels" / "remove_min_rows" report no limit (GP.remove_points takes the device path whatever the shape)
  long long points_removed = 0, remove_stale = 0;  // samples gpc_post_remove shrank / left stale (get-only options "removed" / "remove_stale")
  int paths_engine = 0;      // test hook: the engine of gpc_paths_eval (0: paths.h's PA_DEFAULT_ENGINE, 1: fused kernel, 2: operand matrices + library GEMM)
  int paths_engine_ran = 0;  // the engine the last gpc_paths_eval ran (get-only)
  int paths_solve_engine = 0;      // test hook: the products of gpc_paths_create's solve (0 / 1: skinny kernel, 2: MFMA GEMM)
  int paths_solve_engine_ran = 0;  // the engine the last gpc_paths_create ran (get-only)
  int cv_engine = 0;      // test hook: the engine of gpc_cv's fold Gram (0: cv.h's CV_DEFAULT_ENGINE, 1: fused gather + MFMA, 2: panels + library GEMM)
  int cv_engine_ran = 0;  // the engine the last gpc_cv ran (get-only; 0: the leave-one-out pass, which has none)
  int retry_runs = 0;  // device pipelines spent on jitter retries by the last call (one per level)
#ifdef GPC_EXPERIMENTS
  // ---- tile-level dataflow (dag.h).  Option "dag": 0 off, 1 wherever the plan supports it, -1 automatic (by what was
  // measured to win).  The arithmetic is that of the stream-ordered schedule bit for bit, so the choice may follow the
  // batch size.
  int dag = 0;
  int dag_small_tiles = 40;  // launches with fewer 128-tiles per sample than this become 64-tile tasks (urgent ring)
  int dag_lauum = 1;         // W^T W inside the graph (its tiles fill the CUs other samples' chains leave idle)
  int dag_leaf_blocks = 0;   // leaf servers; 0: min(samples, 8)
  int dag_gate = 0;          // > 0: sample s starts when sample s - dag_gate has finished the leaf at dag_gate_pct % of its chain
  int dag_gate_pct = 50;
  int dag_urgent_cus = 0;    // > 0: CUs per shader engine (on a team's urgent XCD) whose workgroups serve the urgent ring only
  int dag_crit_pct = 15;     // tasks with less slack than this share of the critical path go to the urgent / crit rings
  int dag_timeout_ms = 2000; // a workgroup that finds nothing to do for this long aborts the graph
  int dag_runs = 0, dag_aborts = 0;  // statistics (gpc_get_option "dag_runs" / "dag_aborts")
  bool dag_used = false;     // the pipeline in flight runs a graph: its abort word rides back with the results
  struct DagEntry {
    unsigned long long key = 0;
    gpc::DagPlan plan;  // (host vectors are released after the upload; the counts stay)
    DevBuf tasks, succ, launches_rel;
    unsigned long long last_use = 0;
  };
  std::vector<DagEntry> dag_cache;
  unsigned long long dag_clock = 0;
  DevBuf dag_pending, dag_slots, dag_ctl, dag_launches;
  DevBuf rsv_tbl1;  // cu_reserve_bail table with ONE CU per XCD (the leaf servers' room)
  DevBuf rsv_tbl4;  // ... with one CU per shader engine (independent pipelines)
  // Independent pipelines for small batches of large problems (option "indep"; round 5): every sample its own stream and
  // pipeline, every chip-filling launch CU-reserving, so that one sample's leaves and small launches run beside another's bulk
  int indep = 0, indep_max = 4, indep_min_tiles = 64;
#endif  // GPC_EXPERIMENTS
};

struct gpc_post {
  gpc_ctx* ctx = nullptr;
  int dtype = GPC_F64;
  int S = 0, N = 0, D = 0, npad = 0;
  CovDesc cd{};
  DevBuf A, W;  // per-sample: A = Cholesky factor (L_chol) or -(K+Sigma)^-1 ; W = L^-1
  DevBuf alpha; // S x npad (double)
  std::vector<double> sp, mul, dv;  // host copies of per-sample scalars (SP_STRIDE), scaling
  std::vector<double> sW, mult;
  std::vector<int> lchol, info;
  // What every predict / quad call of this posterior needs again -- the per-sample scalars, the input scaling and
  // the scaled training inputs -- stays on the device once the first call has put it there (three uploads and a
  // kernel less per call); any change of sp / mul / dv / N clears the flag.
  DevBuf dsp, dmul, ddv, dxs;
  bool dev_consts = false;
  // A gradient-observation posterior (gpc_posterior_batch_gobs): gobs.Ng > 0, N is the joint order, and the handle owns
  // the raw point list its predictions are built from (gradobs.h; dxs then holds the scaled LISTS, gobs.P() rows each)
  GobsDims gobs;
  DevBuf gpts;
};

// Pathwise posterior samples (paths.h): everything an evaluation needs, copied at creation -- the handle describes the
// posterior as it was then and outlives it.  All fp64, whatever the posterior's storage type.
struct gpc_paths {
  gpc_ctx* ctx = nullptr;
  int S = 0, N = 0, D = 0, npad = 0, R = 0, F = 0;
  int kq = 0;    // R rounded up to 16: leading dimension of v and wt
  int fpad = 0;  // F rounded up to 128
  CovDesc cd{};
  DevBuf xs, sp, mul, dv;  // scaled training inputs (S x npad x D), per-sample scalars and scaling
  DevBuf theta, bph, wt;   // features (S x fpad x D, S x fpad) and weights (S x fpad x kq)
  DevBuf v;                // S x npad x kq
  void release() {
    for (DevBuf* b : {&xs, &sp, &mul, &dv, &theta, &bph, &wt, &v}) b->release();
  }
};

#define HIPCHK(ctx, expr)                                                                   \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                       \
      return -1;                                                                            \
    }                                                                                       \
  } while (0)

#define FAIL(ctx, msg)   \
  do {                   \
    (ctx)->err = (msg);  \
    return -2;           \
  } while (0)

// ScratchCarver::carve reports the arrays that missed their alignment: the call fails before it launches anything
#define CARVECHK(ctx, fn, expr)                                                             \
  do {                                                                                      \
    if ((expr) != 0) {                                                                      \
      (ctx)->err = std::string(fn) + ": internal error: a scratch array is misaligned";    \
      return -1;                                                                            \
    }                                                                                       \
  } while (0)

namespace {

// Which (XCC_ID, SE_ID, CU_ID) triples does this device run workgroups on?  Enough short-lived blocks to cover every
// CU several times over; each marks the CU it finds itself on and lingers a few microseconds so that the
// dispatcher has to spread the grid.
__global__ __launch_bounds__(256) void cu_probe_kernel(unsigned* __restrict__ seen, long long spin_ticks) {
  if (threadIdx.x == 0) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    atomicOr(seen + (xcc & 7) * 8 + ((hw >> 13) & 0x7), 1u << ((hw >> 8) & 0xf));
  }
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < spin_ticks) {
  }
}

int probe_cu_map(gpc_ctx* c, int n_cus) {
  HIPCHK(c, c->dbg1.ensure(64 * sizeof(unsigned)));
  HIPCHK(c, hipMemsetAsync(c->dbg1.p, 0, 64 * sizeof(unsigned), c->st));
  int seen_total = 0;
  for (int attempt = 0; attempt < 3 && seen_total < n_cus; ++attempt) {
    hipLaunchKernelGGL(cu_probe_kernel, dim3(16 * std::max(n_cus, 1)), dim3(256), 0, c->st, c->dbg1.as<unsigned>(), 500ll);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->cu_seen, c->dbg1.p, sizeof c->cu_seen, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    seen_total = 0;
    for (unsigned m : c->cu_seen) seen_total += __builtin_popcount(m);
  }
  // usable for reserving CUs: every CU accounted for, and every engine that exists has the same number of them
  int per_engine = -1, engines = 0;
  bool uniform = true;
  for (unsigned m : c->cu_seen) {
    if (!m) continue;
    ++engines;
    const int k = __builtin_popcount(m);
    if (per_engine < 0) per_engine = k;
    uniform = uniform && k == per_engine;
  }
  c->cu_map_ok = seen_total == n_cus && uniform && engines > 0;
  char buf[160];
  snprintf(buf, sizeof buf, " cu_map=%s(%d CUs seen in %d engines of %d)", c->cu_map_ok ? "ok" : "UNRECOGNISED: deferred schedule off",
           seen_total, engines, per_engine);
  c->devinfo += buf;
  return 0;
}

#ifdef GPC_EXPERIMENTS
// XCDs the CU probe saw workgroups on: the dataflow graph serves the urgent ring of team x from XCD x only, so it needs all
// NQ of them (a partitioned device would stall every graph until its time-out: ADVICE r5)
int xcds_seen(const gpc_ctx* c) {
  int n = 0;
  for (int x = 0; x < 8; ++x) {
    unsigned any = 0;
    for (int se = 0; se < 8; ++se) any |= c->cu_seen[x * 8 + se];
    n += any != 0;
  }
  return n;
}
#endif

// rsv_tbl for `reserve` CUs per XCD: the highest-numbered CUs of each shader engine -- 2: one in every other engine,
// 4: one per engine, 8: two, 12: three, ...; >= 32 (test hook): every CU, which leaves the work to the one block the
// survivor rule of cu_reserve_bail keeps.
int build_reserve_table(gpc_ctx* c) {
  unsigned short tbl[64] = {};
  const int r = c->defer_reserve;
  for (int x = 0; x < 8; ++x) {
    int engine_no = 0;
    for (int se = 0; se < 8; ++se) {
      unsigned m = c->cu_seen[x * 8 + se];
      if (!m) continue;
      int k = r >= 32 ? 16 : (r == 2 ? (engine_no % 2 == 0 ? 1 : 0) : r / 4);
      ++engine_no;
      unsigned out = 0;
      for (int cu = 15; cu >= 0 && k > 0; --cu)
        if ((m >> cu) & 1u) {
          out |= 1u << cu;
          --k;
        }
      tbl[x * 8 + se] = (unsigned short)out;
    }
  }
  HIPCHK(c, c->rsv_tbl.ensure(sizeof tbl));
  HIPCHK(c, hipMemcpyAsync(c->rsv_tbl.p, tbl, sizeof tbl, hipMemcpyHostToDevice, c->st));
#ifdef GPC_EXPERIMENTS
  // the dataflow schedule (dag.h) keeps ONE CU per XCD free of GEMM workgroups for its leaf servers: the
  // highest-numbered CU of the first shader engine seen in each XCD
  unsigned short tbl1[64] = {};
  for (int x = 0; x < 8; ++x)
    for (int se = 0; se < 8; ++se) {
      const unsigned m = c->cu_seen[x * 8 + se];
      if (!m) continue;
      tbl1[x * 8 + se] = (unsigned short)(1u << (31 - __builtin_clz(m)));
      break;
    }
  HIPCHK(c, c->rsv_tbl1.ensure(sizeof tbl1));
  HIPCHK(c, hipMemcpyAsync(c->rsv_tbl1.p, tbl1, sizeof tbl1, hipMemcpyHostToDevice, c->st));
  unsigned short tbl4[64] = {};  // the highest-numbered CU of EVERY shader engine (every engine can drain its share of a grid)
  for (int i = 0; i < 64; ++i)
    if (c->cu_seen[i]) tbl4[i] = (unsigned short)(1u << (31 - __builtin_clz(c->cu_seen[i])));
  HIPCHK(c, c->rsv_tbl4.ensure(sizeof tbl4));
  HIPCHK(c, hipMemcpyAsync(c->rsv_tbl4.p, tbl4, sizeof tbl4, hipMemcpyHostToDevice, c->st));
#endif
  HIPCHK(c, hipStreamSynchronize(c->st));
  return 0;
}

int cov_count_of(int kind, int D) {
  switch (kind) {
    case K_SE:
    case K_MATERN:
      return D + 1;
    case K_RQ:
      return D + 2;
    case K_SE_ISO:
    case K_MATERN_ISO:
      return 2;
    default:
      return -1;
  }
}

bool valid_kernel(int kind, int degree) {
  if (kind < K_SE || kind > K_MATERN_ISO) return false;
  if ((kind == K_MATERN || kind == K_MATERN_ISO) && degree != 1 && degree != 3 && degree != 5) return false;
  return true;
}

// input scaling exactly as the reference applies it before the distance computation
void scaling_of(int kind, int degree, int D, const double* hyp, double* mul, double* dv, double* sf2,
                double* rqa) {
  const double snu = std::sqrt((double)degree);
  *rqa = 1.0;
  if (cov_is_iso(kind)) {
    const double ell = std::exp(hyp[0]);
    *sf2 = std::exp(2 * hyp[1]);
    for (int h = 0; h < D; ++h) {
      mul[h] = (kind == K_MATERN_ISO) ? snu : 1.0;  // X * sqrt(nu) / ell   |  X / ell
      dv[h] = ell;
    }
    return;
  }
  *sf2 = std::exp(2 * hyp[D]);
  if (kind == K_RQ) *rqa = std::exp(hyp[D + 1]);
  for (int h = 0; h < D; ++h) {
    const double ell = std::exp(hyp[h]);
    if (kind == K_SE) {
      mul[h] = 1.0;  // X / ell
      dv[h] = ell;
    } else if (kind == K_MATERN) {
      mul[h] = snu / ell;  // X @ diag(sqrt(nu)/ell)
      dv[h] = 1.0;
    } else {
      mul[h] = 1.0 / ell;  // X @ diag(1/ell)
      dv[h] = 1.0;
    }
  }
}

// host-side description of a batch of hyperparameter samples
struct Batch {
  int S = 0, N = 0, D = 0, npad = 0;
  CovDesc cd{};
  bool vec_noise = false;
  bool m_const = false;  // m holds ONE value per sample (constant / zero mean: gpc_nll_batch_cm); r is formed on the device
  const double* hyp_cov = nullptr;
  const double* m = nullptr;
  const double* sn2 = nullptr;
  const double* y = nullptr;
  std::vector<double> mul, dv, sp, dvec, r;
  std::vector<double> smin, mult, sl;
  std::vector<int> lchol, tries, info;
  double mult0 = 1.0;  // first jitter multiplier (1 in the reference; a test hook can raise it)

  void init() {
    mul.assign((size_t)S * D, 1.0);
    dv.assign((size_t)S * D, 1.0);
    sp.assign((size_t)S * SP_STRIDE, 0.0);
    dvec.assign((size_t)S * npad, 1.0);
    if (!m_const) r.assign((size_t)S * npad, 0.0);
    smin.assign(S, 0.0);
    mult.assign(S, mult0);
    sl.assign(S, 1.0);
    lchol.assign(S, 0);
    tries.assign(S, 0);
    info.assign(S, 0);
    for (int s = 0; s < S; ++s) {
      double sf2 = 0.0, rqa = 1.0;
      if (hyp_cov)  // built-in kernel; with a caller-provided K (cd.kind < 0) there is nothing to scale
        scaling_of(cd.kind, cd.degree, D, hyp_cov + (size_t)s * cd.cov_N, &mul[(size_t)s * D],
                   &dv[(size_t)s * D], &sf2, &rqa);
      sp[(size_t)s * SP_STRIDE + SP_SF2] = sf2;
      sp[(size_t)s * SP_STRIDE + SP_RQA] = rqa;
      const double* sn = sn2 + (size_t)s * (vec_noise ? N : 1);
      double mn = sn[0];
      if (vec_noise)
        for (int i = 1; i < N; ++i) mn = std::min(mn, sn[i]);
      smin[s] = mn;
      lchol[s] = (mn >= 1e-6) ? 1 : 0;  // gaussian_process.py:2404
      if (!m_const)
        for (int i = 0; i < N; ++i) r[(size_t)s * npad + i] = y[i] - m[(size_t)s * N + i];
      apply_mult(s);
    }
  }

  // (re)derive the scaled system of sample s for its current jitter multiplier
  // (gaussian_process.py:2406-2439)
  void apply_mult(int s) {
    const double* sn = sn2 + (size_t)s * (vec_noise ? N : 1);
    double* d = &dvec[(size_t)s * npad];
    if (lchol[s]) {
      const double sn2_div = smin[s];  // scalar noise: the value itself
      sl[s] = sn2_div * mult[s];
      for (int i = 0; i < N; ++i) d[i] = vec_noise ? sn[i] / sn2_div : 1.0;
    } else {
      sl[s] = 1.0;
      for (int i = 0; i < N; ++i) d[i] = mult[s] * (vec_noise ? sn[i] : sn[0]);
    }
    for (int i = N; i < npad; ++i) d[i] = 1.0;
    sp[(size_t)s * SP_STRIDE + SP_KSCALE] = sl[s];  // K is DIVIDED by this
    sp[(size_t)s * SP_STRIDE + SP_SL] = sl[s];
  }
};


enum Mode { MODE_NLL = 0, MODE_GRAD = 1, MODE_POST = 2 };

// GPC_HOSTTIME=1: host wall-clock of the phases of a call, to stderr (diagnostics only)
struct HostClock {
  bool on;
  const char* tag;
  std::chrono::steady_clock::time_point t;
  explicit HostClock(const char* tg) : on(getenv("GPC_HOSTTIME") != nullptr), tag(tg) {
    if (on) t = std::chrono::steady_clock::now();
  }
  void lap(const char* what) {
    if (!on) return;
    auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "[gpc %s] %-10s %8.3f ms\n", tag, what, std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};

// the table of CUs a deferred / split launch stays off (Pipe::reserve_tbl, gpc_debug_gemm_form)
inline const unsigned short* ctx_reserve_tbl(const gpc_ctx* c) {
  return (c->cu_map_ok && c->defer_reserve > 0) ? c->rsv_tbl.as<unsigned short>() : nullptr;
}

template <typename T>
struct Pipe {
  gpc_ctx* c;
  Batch* B;
  Mode mode;
  // matrices for the chunk being processed (sample 0 of the chunk)
  T* A;
  T* W;
  T* Tm;
  long long sM;
  // gradient side inputs (whole batch, host pointers)
  const double* dm = nullptr;
  int mean_N = 0;
  const double* dsn2 = nullptr;
  int noise_N = 0;
  // outputs (whole batch, host)
  std::vector<double> logdet, quad, G, mg, ng;
  // caller-provided covariance ("K-mode", gpc_nll_batch_K / gpc_posterior_batch_K): host pointer to the
  // N x N matrix of every sample of the batch, and the callback that delivers dK one plane at a time
  std::vector<const double*> Kptr;
  gpc_dk_plane_fn dk_cb = nullptr;
  void* dk_user = nullptr;
  std::vector<int> orig;  // index of each sample in the caller's numbering (for the callback)
  // gradient observations (gobs.Ng > 0): the K-mode pipeline with the staging buffer filled by gobs_cov_kernel from the
  // context's point list instead of an upload (b.N is the joint order, b.hyp_cov the kernel's hyperparameters)
  GobsDims gobs;
  bool kmode() const { return !Kptr.empty() || gobs.Ng > 0; }

  int P() const { return B->cd.cov_N + 1; }

  // K-mode: sum_ij Q_ij dK_ij/dtheta_p for the sample in workspace slot `slot`, one plane at a time
  // (the caller's compute() produced dK on the host; only one N x N plane is ever resident here).
  int trace_planes(int s, int slot) {
    Batch& b = *B;
    const int N = b.N, npad = b.npad, cov_N = b.cd.cov_N, Pn = P();
    hipStream_t st = c->st;
    const size_t pb = (size_t)N * N * sizeof(double);
    HIPCHK(c, c->dbg1.ensure(pb));
    const int nblk = (int)std::min<long long>(1024, ((long long)N * N + 255) / 256);
    HIPCHK(c, c->dbg2.ensure((size_t)nblk * sizeof(double) + 64));
    std::vector<double> plane((size_t)N * N);
    for (int p = 0; p < cov_N; ++p) {
      if (dk_cb(dk_user, orig.empty() ? s : orig[s], p, plane.data()) != 0) FAIL(c, "the dK callback reported an error");
      HIPCHK(c, hipMemcpyAsync(c->dbg1.p, plane.data(), pb, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL((trace_plane_kernel<T>), dim3(nblk), dim3(256), 0, st, (const T*)(Tm + (size_t)slot * sM), npad,
                         (const double*)(c->avec.as<double>() + (size_t)slot * npad),
                         (const double*)(c->spb.as<double>() + (size_t)slot * SP_STRIDE), c->dbg1.as<double>(), N,
                         c->dbg2.as<double>());
      hipLaunchKernelGGL(reduce_parts_kernel, dim3(1, 1), dim3(256), 0, st, (const double*)c->dbg2.p, nblk, 1,
                         c->dbg2.as<double>() + nblk);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(&G[(size_t)s * Pn + p], c->dbg2.as<double>() + nblk, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));  // `plane` is reused for the next hyperparameter
    }
    return 0;
  }

  // Device kernels for `n` samples of the current chunk starting at chunk index `off`
  // (all per-sample buffers are indexed by chunk position), issued on stream `st`.
  int device_section(hipStream_t st, int off, int n, hipEvent_t f0, hipEvent_t f1, int gidx = gpc_ctx::MAXG) {
    Batch& b = *B;
    const int npad = b.npad, N = b.N, D = b.D;
    T* Ac = A + (size_t)off * sM;
    T* Wc = W + (size_t)off * sM;
    T* Tc = Tm + (size_t)off * sM;
    double* xs = c->xs.as<double>() + (size_t)off * npad * D;
    double* spb = c->spb.as<double>() + (size_t)off * SP_STRIDE;
    double* rvec = c->rvec.as<double>() + (size_t)off * npad;
    double* zvec = c->zvec.as<double>() + (size_t)off * npad;
    double* avec = c->avec.as<double>() + (size_t)off * npad;
    double* d_logdet = c->scal.as<double>() + off;
    double* d_quad = c->scal.as<double>() + chunk_cnt + off;
    int* d_info = reinterpret_cast<int*>(c->scal.as<double>() + 2 * chunk_cnt) + off;
    const int t64 = npad / CT, ntl = t64 * (t64 + 1) / 2;
    split_build = false;
    if (kmode()) {
      // A = K / (sn2_div * sn2_mult) + diag from the caller's matrix, one sample at a time through one
      // N x N staging buffer (stream order keeps the upload of sample i+1 behind the kernel reading i)
      HIPCHK(c, c->dbg1.ensure((size_t)N * N * sizeof(double)));
      const size_t gper = (size_t)gobs.P() * D;
      if (gobs.Ng > 0) {
        HIPCHK(c, c->gxs.ensure((size_t)chunk_cnt * gper * sizeof(double)));
        launch_gobs_scale(st, gobs, c->gpts.as<double>(), c->mulb.as<double>() + (size_t)off * D,
                          c->divb.as<double>() + (size_t)off * D, n, c->gxs.as<double>() + (size_t)off * gper);
      }
      for (int i = 0; i < n; ++i) {
        if (gobs.Ng > 0)
          launch_gobs_cov(st, b.cd, gobs, c->gxs.as<double>() + (size_t)(off + i) * gper, spb + (size_t)i * SP_STRIDE,
                          c->mulb.as<double>() + (size_t)(off + i) * D, c->divb.as<double>() + (size_t)(off + i) * D,
                          c->dbg1.as<double>());
        else
          HIPCHK(c, hipMemcpyAsync(c->dbg1.p, Kptr[chunk_s0 + off + i], (size_t)N * N * sizeof(double),
                                   hipMemcpyHostToDevice, st));
        dim3 gl(npad / 64, npad / 4), bl(64, 4);
        hipLaunchKernelGGL((load_K_kernel<T>), gl, bl, 0, st, (const double*)c->dbg1.p, N, npad,
                           (const double*)(spb + (size_t)i * SP_STRIDE),
                           (const double*)(c->dvec.as<double>() + (size_t)(off + i) * npad), Ac + (size_t)i * sM);
      }
    } else {
      if (!prescaled) {
        const long long tot = (long long)npad * D;
        dim3 grid((unsigned)((tot + 255) / 256), n);
        hipLaunchKernelGGL(scale_x_kernel, grid, dim3(256), 0, st, c->dX.as<double>(), N, npad, D,
                           c->mulb.as<double>() + (size_t)off * D, c->divb.as<double>() + (size_t)off * D, xs);
      }
      // With the deferred schedule the build is split: the tiles of the first 1024 rows on this stream, the
      // rest as a persistent, CU-reserving launch on the side stream under the first subtree (plan.h waits
      // for it before the first launch that reads rows >= 1024).
      const int head64 = 1024 / CT, ntl_head = head64 * (head64 + 1) / 2;
      split_build = (defer_node > 0 || use_rl) && !c->capturing && gpc::g_persist_spare >= 0 && npad >= 2048 && reserve_tbl();
      const double* dv = c->dvec.as<double>() + (size_t)off * npad;
      if (split_build) {
        GPC_COV_DISPATCH(build_kernel, T, b.cd, dim3(ntl_head, n), dim3(256), 0, st, b.cd, (const double*)xs,
                         (const double*)spb, dv, N, npad, Ac, sM, npad, 0);
        hipStream_t sd = c->sst[gidx];
        int* bctr = c->tile_ctr.as<int>() + (size_t)gidx * gpc_ctx::CTR_PER_GROUP + gpc_ctx::CTR_PER_GROUP - CTR_STRIDE;
        HIPCHK(c, hipMemsetAsync(bctr, 0, CTR_STRIDE * sizeof(int), st));
        HIPCHK(c, hipEventRecord(c->ev_bfork[gidx], st));
        HIPCHK(c, hipStreamWaitEvent(sd, c->ev_bfork[gidx], 0));
        GPC_COV_DISPATCH(build_persist_kernel, T, b.cd, dim3(4 * gpc::g_block_slots / 2 + 128), dim3(256), 0, sd, b.cd,
                         (const double*)xs, (const double*)spb, dv, N, npad, Ac, sM, npad, ntl_head, ntl, n,
                         reserve_tbl(), bctr);
        HIPCHK(c, hipEventRecord(c->ev_btail[gidx], sd));
      } else {
        GPC_COV_DISPATCH(build_kernel, T, b.cd, dim3(ntl, n), dim3(256), 0, st, b.cd, (const double*)xs,
                         (const double*)spb, dv, N, npad, Ac, sM, npad, 0);
      }
    }
    HIPCHK(c, hipGetLastError());

    if (f0 && !c->capturing) HIPCHK(c, hipEventRecord(f0, st));
    Factor<T> F;
    F.st = st;
    F.batch = n;
    F.npad = npad;
    F.A = Ac;
    F.W = Wc;
    F.Tm = Tc;
    F.sA = F.sW = F.sT = sM;
    F.logdet = d_logdet;
    F.info = d_info;
    F.nvalid = N;
    F.stable = stable || c->stable;
    F.tri_skip = c->tri_skip != 0;
    if ((defer_node > 0 || use_rl) && !c->capturing && gpc::g_persist_spare >= 0) {
      F.side = c->sst[gidx];
      F.evs = c->dev_ev[gidx];
      F.nev = gpc_ctx::NDEV - 2;  // (the last two belong to the solves beside W^T W)
      F.defer_min = defer_node;
      F.reserve = reserve_tbl();
    }
#ifdef GPC_EXPERIMENTS
    if (indep_mode && !c->capturing) {
      F.reserve = c->rsv_tbl4.template as<unsigned short>();
      F.reserved_small_bt = 64;
      F.reserve_all = true;
      F.reserve_min = c->indep_min_tiles;
    }
#endif
    if (c->check_queues && !c->capturing) F.qlog = &qlog;
    if (split_build) {
      F.ev_tail = c->ev_btail[gidx];
      F.tail_row0 = 1024;
    }
    if (gpc::g_persist_spare >= 0) {
      // (the last counters of the group belong to the split build, already in flight on the side stream)
      F.ctr = c->tile_ctr.as<int>() + (size_t)gidx * gpc_ctx::CTR_PER_GROUP;
      F.ctr_cap = gpc_ctx::CTR_PER_GROUP - CTR_STRIDE;
      // (no launch of a small problem is persistent -- its largest, W^T W, has tm (tm + 1) / 2 tiles per sample --
      // and the zeroing would be a launch of its own on the critical path)
      const long long tmx = npad / TILE, biggest = tmx * (tmx + 1) / 2 * n;
      if (defer_node > 0 || F.reserve_all || biggest >= std::min<long long>(gpc::g_small_launch_blocks, gpc::g_block_slots - gpc::g_persist_spare))
        HIPCHK(c, hipMemsetAsync(F.ctr, 0, (gpc_ctx::CTR_PER_GROUP - CTR_STRIDE) * sizeof(int), st));
      else
        F.ctr = nullptr;
    }
    // NLL only: the inverse of the whole matrix is not needed (only of left children)
    const bool full_inv = (mode != MODE_NLL);
    const int nll_blk = c->nll_block >= 0 ? c->nll_block
                                          : (npad >= 2048 ? 512 : 0);
    const bool nll_blocked = !use_rl && mode == MODE_NLL && nll_blk >= TILE && npad > nll_blk;
    bool dag_done = false, dag_has_lauum = false;
    if (nll_blocked) F.nll_block = nll_blk;  // (the blocked forward solve below reads it, whichever schedule factors)
#ifdef GPC_EXPERIMENTS
    if (use_dag && !use_rl) {
      int rc = dag_section(st, gidx, F, nll_blocked ? nll_blk : 0, full_inv, dag_has_lauum);
      if (rc < 0) return rc;
      dag_done = rc == 0;  // (rc > 0: the plan is not one the graph executes -- the stream-ordered schedule below)
      if (dag_done && getenv("GPC_DAG_SYNC")) {
        (void)hipStreamSynchronize(c->sst[gidx]);
        (void)hipStreamSynchronize(st);
      }
    }
    if (!dag_done && use_rl) {
      F.rl_panel = c->rl_panel;
      F.rl_lookahead = (double)n * std::pow((double)npad / 4096.0, 3.0) <= (double)c->rl_ahead_max;
      F.potrf_rl();
      dag_done = true;  // (the factorization has been issued)
    }
#endif
    if (dag_done) {
      // (experiments build: the factorization -- and W^T W when it is part of the graph -- has been issued)
    } else if (nll_blocked) {
      F.nll_block = nll_blk;
      F.potrf_nll(0, npad);
    } else {
      F.potrf_inv(0, npad, full_inv, mode == MODE_POST);
    }
    // z = L^-1 r ; quad = z.z ; alpha = W^T z / sl -- two triangular matrix-vector products over W, HBM-bound and
    // independent of W^T W.  With the gradient they run UNDER the W^T W launch (round 3): its two resident blocks per
    // CU use 2 x 240 of the 512 VGPRs per lane and 147 of 160 KB of LDS, so kernels of at most 32 VGPRs (trmv_low_kernel,
    // trmv_t_part_low_kernel, blas1.h) are dispatched beside them and take their bytes while the GEMM is
    // MFMA-bound; forked on the side stream just before the launch, joined before the gradient contraction, which
    // needs alpha.  (Eager one- or multi-group pipelines; a captured graph keeps the serial order.)
    // (fp64 only: the fp32 GEMM uses 249 VGPRs, two of its blocks leave no register for anything else)
    const bool solves_beside_lauum = mode == MODE_GRAD && !c->capturing && !kmode() && c->solves_beside_lauum &&
                                     sizeof(T) == 8 && npad >= 2048 && gpc::g_persist_spare >= 0 && !dag_has_lauum && !indep_mode;
    auto solves = [&](hipStream_t sx) -> int {
      const hipStream_t keep = F.st;
      F.st = sx;
      F.low_regs = sx != st;
#ifdef GPC_EXPERIMENTS
      if (use_rl)
        F.forward_solve_rl(rvec, zvec);
      else
#endif
      if (nll_blocked)
        F.forward_solve_nll(0, npad, rvec, zvec);
      else
        F.forward_solve(0, npad, full_inv, rvec, zvec);
      F.st = keep;
      F.low_regs = false;
      if (mode == MODE_NLL) {
        hipLaunchKernelGGL(dot_kernel, dim3(1, n), dim3(256), 0, sx, (const double*)zvec, (const double*)zvec,
                           npad, npad, d_quad);
      } else {  // quad = z.z rides in the first block of the transposed product
        double* tpart = c->tpart.as<double>() + (size_t)off * (npad / TRC) * npad;
        const dim3 gt((npad + 64 * MM<T>::VEC - 1) / (64 * MM<T>::VEC), npad / TRC, n);
        if (sx != st)
          hipLaunchKernelGGL((trmv_t_part_low_kernel<T>), gt, dim3(256), 0, sx, (const T*)Wc, sM, npad, (const double*)zvec,
                             npad, tpart, d_quad);
        else
          hipLaunchKernelGGL((trmv_t_part_kernel<T, 8>), gt, dim3(256), 0, sx, (const T*)Wc, sM, npad, (const double*)zvec,
                             npad, tpart, d_quad);
        hipLaunchKernelGGL(trmv_t_sum_kernel, dim3(npad / 128, n), dim3(128), 0, sx, (const double*)tpart, npad,
                           (const double*)spb, (int)SP_STRIDE, (int)SP_SL, avec);
      }
      HIPCHK(c, hipGetLastError());
      return 0;
    };
    hipEvent_t ev_solved = nullptr;
    if (mode == MODE_GRAD) {
      if (solves_beside_lauum) {
        hipStream_t sx = c->sst[gidx];
        hipEvent_t ev_fork = c->dev_ev[gidx][gpc_ctx::NDEV - 1];
        ev_solved = c->dev_ev[gidx][gpc_ctx::NDEV - 2];
        HIPCHK(c, hipEventRecord(ev_fork, st));
        HIPCHK(c, hipStreamWaitEvent(sx, ev_fork, 0));
        if (int rc = solves(sx)) return rc;
        HIPCHK(c, hipEventRecord(ev_solved, sx));
      }
      if (!dag_has_lauum) {
        if (!c->capturing) HIPCHK(c, hipEventRecord(c->ev_l0[gidx], st));
        // the readers of Tc: trace_kernel uses j <= i only (it loads the rest of a diagonal 64-tile and drops it),
        // diagq_kernel the diagonal; the plane-by-plane contraction of a user kernel is given whole diagonal tiles
        F.lauum(Tc, sM, !kmode());
        if (!c->capturing) {
          HIPCHK(c, hipEventRecord(c->ev_l1[gidx], st));
          lauum_n[gidx] = n;
        }
      }
    }
    HIPCHK(c, F.err);
    HIPCHK(c, hipGetLastError());
    if (f1 && !c->capturing) HIPCHK(c, hipEventRecord(f1, st));
    c->last_flops += F.flops;

    if (ev_solved)
      HIPCHK(c, hipStreamWaitEvent(st, ev_solved, 0));
    else if (int rc = solves(st))
      return rc;
    HIPCHK(c, hipGetLastError());

    const int Pn = P();
    if (mode == MODE_GRAD) {
      double* parts = c->parts.as<double>() + (size_t)off * ntl * Pn;
      double* diagq = c->diagq.as<double>() + (size_t)off * npad;
      if (kmode()) {
        // diag(Q) and trace(Q) now; the covariance slots are filled plane by plane after the sync (trace_planes) -- or,
        // with gradient observations, here on the stream by the fused contraction of gradobs.h: no plane, no round trip
        hipLaunchKernelGGL((diagq_kernel<T>), dim3(1, n), dim3(256), 0, st, (const T*)Tc, sM, npad, (const double*)avec,
                           (const double*)spb, N, diagq, c->gout.as<double>() + (size_t)off * Pn, Pn);
        if (gobs.Ng > 0) {
          if constexpr (sizeof(T) == 8) {
            GobsTraceScratch z;
            CARVECHK(c, "gpc_nll_batch_gobs_grad", ScratchCarver::carve(z, c->parts.p, chunk_cnt, gobs, Pn));
            const size_t gper = (size_t)gobs.P() * D, tiles = (size_t)gobs.trace_rows();
            launch_gobs_trace(st, b.cd, gobs, n, c->gxs.as<double>() + (size_t)off * gper, spb,
                              c->mulb.as<double>() + (size_t)off * D, c->divb.as<double>() + (size_t)off * D,
                              (const double*)Tc, sM, npad, avec, npad, z.part + (size_t)off * tiles * Pn, Pn,
                              c->gout.as<double>() + (size_t)off * Pn);
          } else {
            FAIL(c, "the gradient of the gradient-observation likelihood is fp64 only");
          }
        }
      } else {
        GPC_COV_DISPATCH(trace_kernel, T, b.cd, dim3(ntl, n), dim3(256), 4 * (((Pn + 3) & ~3) + 4) * sizeof(double), st,
                         b.cd, (const double*)xs, (const double*)spb, (const double*)avec, N, npad, (const T*)Tc, sM,
                         npad, parts, ntl, diagq);
        // the reduction of the tile partials and the mean / noise gradient products: one launch
        const int mN = mean_N > 0 ? mean_N : 0, nN = (noise_N > 0 && b.vec_noise) ? noise_N : 0;
        hipLaunchKernelGGL(grad_tail_kernel, dim3(Pn + mN + nN, n), dim3(256), 0, st, (const double*)parts, ntl, Pn,
                           c->gout.as<double>() + (size_t)off * Pn,
                           (mN && dm) ? (const double*)(c->dmb.as<double>() + (size_t)off * N * mean_N) : nullptr, N, mN,
                           (const double*)avec, mN ? c->mg.as<double>() + (size_t)off * mean_N : nullptr,
                           nN ? (const double*)(c->dsn2b.as<double>() + (size_t)off * N * noise_N) : nullptr, nN,
                           (const double*)diagq, nN ? c->ng.as<double>() + (size_t)off * noise_N : nullptr, npad);
        HIPCHK(c, hipGetLastError());
        return 0;
      }
      if (mean_N > 0)
        hipLaunchKernelGGL(mat_t_vec_kernel, dim3(mean_N, n), dim3(256), 0, st,
                           (const double*)(c->dmb.as<double>() + (size_t)off * N * mean_N), N, mean_N,
                           (const double*)avec, npad, c->mg.as<double>() + (size_t)off * mean_N);
      if (noise_N > 0 && b.vec_noise)
        hipLaunchKernelGGL(mat_t_vec_kernel, dim3(noise_N, n), dim3(256), 0, st,
                           (const double*)(c->dsn2b.as<double>() + (size_t)off * N * noise_N), N, noise_N,
                           (const double*)diagq, npad, c->ng.as<double>() + (size_t)off * noise_N);
      HIPCHK(c, hipGetLastError());
    }
    return 0;
  }

#ifdef GPC_EXPERIMENTS
  // ---- tile-level dataflow (dag.h) ----------------------------------------------------------------------------
  bool use_dag = false;  // run(): this pipeline's factorization goes through the task graph
  bool indep_mode = false;  // run(): one pipeline per sample, chip-filling launches CU-reserving
  int dag_trace_n = 0;
  // "dag" = -1: where the graph was measured to win
  bool dag_auto(int cnt, int npad) const { return false; }

  // The graph of (npad, plan variant): recorded from plan.h with placeholder buffer addresses, cut into tile tasks,
  // uploaded once and kept.  Returns nullptr when the plan holds something the graph does not execute.
  gpc_ctx::DagEntry* dag_plan(int nll_blk, bool full_inv, bool with_lauum, double* flops1) {
    Batch& b = *B;
    const int npad = b.npad;
    const unsigned long long key = (unsigned long long)npad | ((unsigned long long)sizeof(T) << 20) |
                                   ((unsigned long long)nll_blk << 24) | ((unsigned long long)full_inv << 40) |
                                   ((unsigned long long)with_lauum << 41) | ((unsigned long long)mode << 42) |
                                   ((unsigned long long)c->dag_small_tiles << 44) | ((unsigned long long)c->dag_crit_pct << 56);
    for (auto& e : c->dag_cache)
      if (e.key == key) {
        e.last_use = ++c->dag_clock;
        *flops1 = e.plan.work_us;  // (work_us is reused to carry the algorithmic flops of one sample, see below)
        return e.plan.ntasks > 0 ? &e : nullptr;
      }
    PlanRecorder rec;
    Factor<T> F;
    F.rec = &rec;
    F.st = nullptr;
    F.batch = 1;
    F.npad = npad;
    F.A = static_cast<T*>(const_cast<void*>(dag_fake_base(0)));
    F.W = static_cast<T*>(const_cast<void*>(dag_fake_base(1)));
    F.Tm = static_cast<T*>(const_cast<void*>(dag_fake_base(2)));
    F.sA = F.sW = F.sT = sM;
    F.nvalid = b.N;
    F.dual_launch = false;
    if (nll_blk > 0) {
      F.nll_block = nll_blk;
      F.potrf_nll(0, npad);
    } else {
      F.potrf_inv(0, npad, full_inv, false);
    }
    if (with_lauum) F.lauum(F.Tm, sM);
    if (c->dag_cache.size() >= 8) {  // least recently used entry goes
      size_t old = 0;
      for (size_t i = 1; i < c->dag_cache.size(); ++i)
        if (c->dag_cache[i].last_use < c->dag_cache[old].last_use) old = i;
      c->dag_cache[old].tasks.release();
      c->dag_cache[old].succ.release();
      c->dag_cache[old].launches_rel.release();
      c->dag_cache.erase(c->dag_cache.begin() + old);
    }
    c->dag_cache.emplace_back();
    gpc_ctx::DagEntry& e = c->dag_cache.back();
    e.key = key;
    e.last_use = ++c->dag_clock;
    const void* bases[3] = {dag_fake_base(0), dag_fake_base(1), dag_fake_base(2)};
    DagPlan& P = e.plan;
    if (!build_dag(rec, bases, npad, sizeof(T), c->dag_small_tiles, P, false, c->dag_crit_pct / 100.0)) {
      P = DagPlan{};
      P.work_us = F.flops;
      *flops1 = F.flops;
      return nullptr;
    }
    if (getenv("GPC_DAG_LOG"))
      fprintf(stderr, "[gpcore] dag npad=%d nll_blk=%d lauum=%d: %d tasks (%d leaves, %d x 64, %d x 128), %lld edges, %zu launches; "
                      "rings: %d urgent, %d crit, %d bulk; model: critical path %.0f us, work %.0f CU-us\n", npad, nll_blk, (int)with_lauum, P.ntasks, P.nleaf, P.n64, P.n128,
              P.nedges, P.launches.size(), P.n_urgent, P.n_crit, P.n_bulk, P.crit_us, P.work_us);
    auto put = [&](DevBuf& d, const void* src, size_t n) -> hipError_t {
      hipError_t er = d.ensure(std::max<size_t>(n, 16));
      if (er != hipSuccess) return er;
      return hipMemcpy(d.p, src, n, hipMemcpyHostToDevice);
    };
    if (put(e.tasks, P.tasks.data(), P.tasks.size() * sizeof(DagTask)) != hipSuccess ||
        put(e.succ, P.succ.data(), P.succ.size() * sizeof(int)) != hipSuccess ||
        put(e.launches_rel, P.launches.data(), P.launches.size() * sizeof(GemmArgs)) != hipSuccess) {
      c->dag_cache.pop_back();
      return nullptr;
    }
    P.work_us = F.flops;  // from here on: algorithmic flops of one sample (tile-exact, as plan.h counts them)
    std::vector<DagTask>().swap(P.tasks);
    std::vector<int>().swap(P.succ);
    *flops1 = F.flops;
    return &e;
  }

  // Issues the graph for the n samples of F.  0: issued; > 0: not applicable (the caller falls back); < 0: error.
  int dag_section(hipStream_t st, int gidx, Factor<T>& F, int nll_blk, bool full_inv, bool& has_lauum) {
    const int n = F.batch, npad = F.npad;
    const bool with_lauum = mode == MODE_GRAD && c->dag_lauum != 0;
    double flops1 = 0;
    gpc_ctx::DagEntry* e = dag_plan(nll_blk, full_inv, with_lauum, &flops1);
    if (!e) return 1;
    const DagPlan& P = e->plan;
    const int nlaunch = (int)P.launches.size();
    // ring storage: urgent | NQ bulk rings | leaf
    DagDev d{};
    int off = 0;
    d.nteams = std::min(n, (int)NQ);
    for (int q = 0; q < NQ; ++q) {  // team q holds the samples q, q + nteams, ...
      const int members = q < d.nteams ? (n - q + d.nteams - 1) / d.nteams : 0;
      d.ring_base[DAG_RING_URGENT + q] = off;
      off += members * P.n_urgent;
      d.ring_base[DAG_RING_CRIT0 + q] = off;
      off += members * P.n_crit;
      d.ring_base[DAG_RING_BULK0 + q] = off;
      off += members * P.n_bulk;
    }
    // staggered starts: with more samples than teams the chains of all samples would otherwise run in phase (every
    // sample in its latency-bound stretches at the same time, nothing to fill the chip with)
    d.gate = c->dag_gate > 0 && c->dag_gate < n ? c->dag_gate : 0;
    d.gate_task = P.leaf_task.empty() ? 0 : P.leaf_task[std::min<size_t>(P.leaf_task.size() - 1,
                                                                       (size_t)(P.leaf_task.size() * (size_t)c->dag_gate_pct / 100))];
    d.ring_base[DAG_RING_LEAF] = off;
    off += n * P.nleaf;
    HIPCHK(c, c->dag_slots.ensure((size_t)std::max(off, 4) * sizeof(int)));
    HIPCHK(c, c->dag_pending.ensure((size_t)n * P.ntasks * sizeof(int)));
    HIPCHK(c, c->dag_ctl.ensure(sizeof(DagCtl)));
    HIPCHK(c, c->dag_launches.ensure((size_t)std::max(nlaunch, 1) * sizeof(GemmArgs)));
    d.tasks = e->tasks.template as<DagTask>();
    d.succ = e->succ.template as<int>();
    d.launches_rel = e->launches_rel.template as<GemmArgs>();
    d.launches_w = c->dag_launches.template as<GemmArgs>();
    d.launches = d.launches_w;
    d.nlaunch = nlaunch;
    d.base[0] = F.A;
    d.base[1] = F.W;
    d.base[2] = F.Tm;
    d.pending = c->dag_pending.template as<int>();
    d.slots = c->dag_slots.template as<int>();
    d.ctl = c->dag_ctl.template as<DagCtl>();
    d.ntasks = P.ntasks;
    d.S = n;
    d.A = F.A;
    d.W = F.W;
    d.sA = F.sA;
    d.sW = F.sW;
    d.npad = npad;
    d.nvalid = F.nvalid;
    d.logdet = F.logdet;
    d.info = F.info;
    d.rsv = c->rsv_tbl1.template as<unsigned short>();
    d.timeout_ticks = (long long)c->dag_timeout_ms * 100000ll;  // wall_clock64: 100 MHz
    d.trace = nullptr;
    if (getenv("GPC_DAG_TRACE")) {
      HIPCHK(c, c->dbg2.ensure((size_t)n * P.ntasks * 6 * sizeof(long long)));
      HIPCHK(c, hipMemsetAsync(c->dbg2.p, 0, (size_t)n * P.ntasks * 6 * sizeof(long long), st));
      d.trace = c->dbg2.template as<long long>();
      dag_trace_n = n * P.ntasks;
    }
    HIPCHK(c, hipMemsetAsync(d.slots, 0, (size_t)off * sizeof(int), st));
    HIPCHK(c, hipMemsetAsync(d.ctl, 0, sizeof(DagCtl), st));
    const long long items = (long long)n * P.ntasks;
    hipLaunchKernelGGL(dag_init_kernel, dim3((unsigned)std::min<long long>(1024, (items + 255) / 256)), dim3(256), 0, st, d);
    // The leaf servers run on the pipeline's own stream (created with the greatest priority: they are the latency-bound
    // chain), the GEMM workers on the side stream (least priority, like every chip-filling side launch of plan.h).
    hipStream_t sd = c->sst[gidx];
    hipEvent_t ev_fork = c->dev_ev[gidx][0], ev_join = c->dev_ev[gidx][1];
    HIPCHK(c, hipEventRecord(ev_fork, st));
    HIPCHK(c, hipStreamWaitEvent(sd, ev_fork, 0));
    if (mode == MODE_GRAD && with_lauum) HIPCHK(c, hipEventRecord(c->ev_l0[gidx], sd));
    // EXACTLY two workgroups per CU (74 KB of LDS each: the grid fills every CU by pigeonhole); the two that land on the
    // reserved CU of each XCD return at once and leave it empty for a leaf server.  No surplus: workgroups that cannot
    // be placed stay pending in the dispatcher, and a dispatch with pending workgroups kept the YOUNGER leaf launch from
    // starting at all (measured: an oversized grid drained only through the shader engine that holds the reserved CU,
    // 24 of 80 surplus workgroups; the leaf servers started 12 us after the workers had given up).
    d.urgent_cus = c->dag_urgent_cus;
    d.leaf_servers = c->dag_leaf_blocks >= 0 ? std::max(1, std::min(c->dag_leaf_blocks > 0 ? c->dag_leaf_blocks : std::min(n, 8), 8)) : 0;
    hipLaunchKernelGGL((dag_worker_kernel<T>), dim3(gpc::g_block_slots), dim3(256), 0, sd, d);
    if (mode == MODE_GRAD && with_lauum) {
      HIPCHK(c, hipEventRecord(c->ev_l1[gidx], sd));
      lauum_n[gidx] = -n;  // negative: the timed launch is the whole graph (run() prices it as S N^3 flops)
    }
    HIPCHK(c, hipEventRecord(ev_join, sd));
    // (test hook: dag_leaf_blocks < 0 starts NO leaf server -- the graph stalls at its first leaf, the workers' bounded
    // waits run out, the graph aborts and run() falls back to the stream-ordered schedule)
    const int nl = std::max(1, std::min(c->dag_leaf_blocks > 0 ? c->dag_leaf_blocks : std::min(n, 8), 8));
    if (c->dag_leaf_blocks >= 0)
      hipLaunchKernelGGL((dag_leaf_kernel<T>), dim3(nl), dim3(256), 0, st, d, gpc::g_leaf_fault);
    HIPCHK(c, hipStreamWaitEvent(st, ev_join, 0));
    HIPCHK(c, hipGetLastError());
    F.flops += flops1 * n;
    F.launches += 2;
    has_lauum = with_lauum;
    c->dag_used = true;
    ++c->dag_runs;
    return 0;
  }
#else
  // (the product library runs the stream-ordered schedule only: the conditions below fold away)
  static constexpr bool use_dag = false, indep_mode = false, use_rl = false;
#endif
  // device_section through a cached launch graph (one sample group, main stream)
  int graph_section(int cnt) {
    Batch& b = *B;
    hipStream_t st = c->st;
    const unsigned long long key[4] = {
        ((unsigned long long)mode << 60) | ((unsigned long long)sizeof(T) << 52) | ((unsigned long long)b.vec_noise << 48) |
            ((unsigned long long)prescaled << 49) | ((unsigned long long)(stable || c->stable) << 50) |
            ((unsigned long long)cnt << 24) | (unsigned long long)b.N,
        ((unsigned long long)b.cd.kind << 48) | ((unsigned long long)b.cd.degree << 40) | ((unsigned long long)b.D << 20) |
            ((unsigned long long)mean_N << 10) | (unsigned long long)noise_N,
        (unsigned long long)(uintptr_t)A, (unsigned long long)(uintptr_t)W ^ ((unsigned long long)(uintptr_t)Tm << 1)};
    gpc_ctx::GraphEntry* hit = nullptr;
    gpc_ctx::GraphEntry* victim = &c->graphs[0];
    for (auto& g : c->graphs) {
      if (g.exec && g.epoch == g_alloc_epoch && g.key[0] == key[0] && g.key[1] == key[1] && g.key[2] == key[2] &&
          g.key[3] == key[3])
        hit = &g;
      if (g.last_use < victim->last_use) victim = &g;
    }
    if (!hit) {
      if (victim->exec) {
        (void)hipGraphExecDestroy(victim->exec);
        victim->exec = nullptr;
      }
      hipGraph_t graph = nullptr;
      const double flops_before = c->last_flops;
      HIPCHK(c, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      c->capturing = true;
      const int rc = device_section(st, 0, cnt, nullptr, nullptr);
      c->capturing = false;
      victim->flops = c->last_flops - flops_before;
      const hipError_t e = hipStreamEndCapture(st, &graph);
      if (rc) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
      }
      HIPCHK(c, e);
      const hipError_t ei = hipGraphInstantiate(&victim->exec, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      HIPCHK(c, ei);
      for (int i = 0; i < 4; ++i) victim->key[i] = key[i];
      victim->epoch = g_alloc_epoch;
      hit = victim;
    } else {
      c->last_flops += hit->flops;
    }
    hit->last_use = ++c->graph_clock;
    if (timing_on) HIPCHK(c, hipEventRecord(c->ev[1], st));
    HIPCHK(c, hipGraphLaunch(hit->exec, st));
    if (timing_on) HIPCHK(c, hipEventRecord(c->ev[2], st));
    return 0;
  }

  // the table of CUs a deferred / split launch stays off, or nullptr when the device's CU numbering was not
  // recognised or no CU is to be reserved (the launches are then plain persistent ones)
  const unsigned short* reserve_tbl() const { return ctx_reserve_tbl(c); }
  std::vector<typename Factor<T>::QueueCheck> qlog;  // debug option check_queues

  // check_queues: every tile queue of every persistent launch of the pipeline that just ran must have handed out all
  // its tiles (a queue counter below its total = tiles nobody computed: the grid was starved)
  int verify_queues() {
    if (qlog.empty()) return 0;
    std::vector<int> h((gpc_ctx::MAXG + 1) * gpc_ctx::CTR_PER_GROUP);
    HIPCHK(c, hipMemcpy(h.data(), c->tile_ctr.p, h.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (const auto& q : qlog) {
      const int* v = h.data() + (q.slot - c->tile_ctr.as<int>());
      long long drawn = 0;
      const bool affine = (gpc::g_gemm_flags & 8) != 0;
      if (!affine) {
        drawn = std::min<long long>(v[0], (long long)q.ntiles * q.batch);
      } else {
        const int nclass = gpc::queue_nclass(q.batch);
        for (int k = 0; k < NQ; ++k) {
          int cls, smp;
          const int nsq = gpc::queue_of(q.batch, nclass, k, cls, smp);
          const long long total = nsq > 0 ? gpc::queue_total(q.ntiles, nclass, cls, nsq) : 0;
          drawn += std::min<long long>(v[k], total);
        }
      }
      if (drawn != (long long)q.ntiles * q.batch) {
        qlog.clear();
        c->err = "internal error: a persistent GEMM launch ended with tiles left in its queues";
        return -3;
      }
    }
    qlog.clear();
    return 0;
  }

  int chunk_cnt = 0;
  int chunk_s0 = 0;  // first sample (batch numbering) of the chunk being processed
  int defer_node = 0;  // plan.h: nodes at least this large run their U product on the side stream (0: none)
  bool split_build = false;
#ifdef GPC_EXPERIMENTS
  bool use_rl = false;  // plan.h: right-looking panels with look-ahead for this pipeline
#endif
  bool stable = false;  // plan.h: refined panel solves (jitter retries; gpc_set_option "stable")
  bool prescaled = false;  // the transfer kernel of this chunk has written the scaled inputs (run())
  bool timing_on = true;   // run_once(): this call records its timing events (always from N_pad = 2048 on; below on request)
  std::vector<double> r_expanded;  // run(): r = y - m0 formed on the host when no pinned block was to be had
  int lauum_n[gpc_ctx::MAXG + 1] = {};

  // The pipeline of a chunk whose matrices are single 128 x 128 leaves (see run()).  A, W, Tm point at the chunk's slot.
  int small_section(int s0, int cnt, const double* hsp, const double* hmul, const double* hdv, const double* hdvec,
                    const double* rsrc, size_t scal_bytes, HostClock& hc) {
    Batch& b = *B;
    const int npad = b.npad, N = b.N, D = b.D, Pn = P();
    hipStream_t st = c->st;
    double* d_logdet = c->scal.as<double>();
    double* d_quad = d_logdet + cnt;
    int* d_info = reinterpret_cast<int*>(d_quad + cnt);
    // (without gradient -- an evaluation, or a posterior: L in A, W and alpha are what it keeps -- the three scalars of a
    // sample are all that comes back)
    // (the landing block: the context's coherent block when the results fit and polling is on -- its last word is the
    // completion flag --, else a piece of the staging block and a stream synchronisation)
    // (a gradient evaluation ends with the gathered download launch instead, which announces itself the same way:
    // XferDesc::flag)
    const bool poll = c->small_poll && c->land_blk && scal_bytes + 16 <= gpc_ctx::LAND_BYTES && cnt <= 64;
    double* land = mode != MODE_GRAD ? (poll ? c->land_blk : static_cast<double*>(c->pin.alloc(scal_bytes))) : nullptr;
    unsigned long long* flag = poll ? reinterpret_cast<unsigned long long*>(c->land_blk + (gpc_ctx::LAND_BYTES / 8 - 1)) : nullptr;
    const unsigned long long seq = ++c->land_seq;
    int* done_ctr = reinterpret_cast<int*>(reinterpret_cast<char*>(c->scal.p) + scal_bytes);  // zeroed with the scalars
    const bool timing = c->small_timing != 0;
    XferDesc u;
    HIPCHK(c, c->pin.take_up(st, c->scal.p, scal_bytes + 8, u));
    u.X = c->dX.as<double>();
    u.mul = hmul;
    u.dv = hdv;
    u.xs = c->xs.as<double>();
    u.n = N;
    u.npad = npad;
    u.D = D;
    u.cnt = cnt;
    if (timing) HIPCHK(c, hipEventRecord(c->ev[1], st));
    GPC_COV_DISPATCH(small_front_kernel, T, b.cd, dim3(3, cnt), dim3(256), 0, st, u, b.cd, hsp, hdvec, b.vec_noise ? 1 : 0,
                     A, sM);
    hipLaunchKernelGGL((leaf_solve_kernel<T>), dim3(cnt), dim3(256), 0, st, A, sM, npad, W, sM, npad, d_logdet, d_info, N,
                       gpc::g_leaf_fault, rsrc, c->zvec.as<double>(), d_quad,
                       mode != MODE_NLL ? c->avec.as<double>() : nullptr, (const double*)c->spb.as<double>(),
                       (int)SP_STRIDE, (int)SP_SL, land, cnt, mode != MODE_GRAD ? flag : nullptr, seq, done_ctr);
    HIPCHK(c, hipGetLastError());
    c->last_flops += (2.0 / 3.0) * TILE * (double)TILE * TILE * cnt;
    if (mode == MODE_GRAD) {
      Factor<T> F;
      F.st = st;
      F.batch = cnt;
      F.npad = npad;
      F.A = A;
      F.W = W;
      F.Tm = Tm;
      F.sA = F.sW = F.sT = sM;
      F.lauum(Tm, sM);
      HIPCHK(c, F.err);
      c->last_flops += F.flops;
      HIPCHK(c, hipEventRecord(c->ev[2], st));
      const int t64 = npad / CT, ntl = t64 * (t64 + 1) / 2;
      double* parts = c->parts.as<double>();
      double* diagq = c->diagq.as<double>();
      GPC_COV_DISPATCH(trace_kernel, T, b.cd, dim3(ntl, cnt), dim3(256), 4 * (((Pn + 3) & ~3) + 4) * sizeof(double), st, b.cd,
                       (const double*)c->xs.as<double>(), (const double*)c->spb.as<double>(),
                       (const double*)c->avec.as<double>(), N, npad, (const T*)Tm, sM, npad, parts, ntl, diagq);
      const int mN = mean_N > 0 ? mean_N : 0, nN = (noise_N > 0 && b.vec_noise) ? noise_N : 0;
      hipLaunchKernelGGL(grad_tail_kernel, dim3(Pn + mN + nN, cnt), dim3(256), 0, st, (const double*)parts, ntl, Pn,
                         c->gout.as<double>(), (mN && dm) ? (const double*)c->dmb.as<double>() : nullptr, N, mN,
                         (const double*)c->avec.as<double>(), mN ? c->mg.as<double>() : nullptr,
                         nN ? (const double*)c->dsn2b.as<double>() : nullptr, nN, (const double*)diagq,
                         nN ? c->ng.as<double>() : nullptr, npad);
      HIPCHK(c, hipGetLastError());
    } else if (timing) {
      HIPCHK(c, hipEventRecord(c->ev[2], st));
    }
    if (timing) HIPCHK(c, hipEventRecord(c->ev[3], st));
    hc.lap("launch");
    std::vector<double> hscal(scal_bytes / 8);
    if (mode == MODE_GRAD) {
      HIPCHK(c, c->pin.gather(hscal.data(), d_logdet, scal_bytes, st));
      HIPCHK(c, c->pin.gather(&G[(size_t)s0 * Pn], c->gout.p, (size_t)cnt * Pn * 8, st));
      if (mean_N > 0) HIPCHK(c, c->pin.gather(&mg[(size_t)s0 * mean_N], c->mg.p, (size_t)cnt * mean_N * 8, st));
      if (noise_N > 0 && b.vec_noise)
        HIPCHK(c, c->pin.gather(&ng[(size_t)s0 * noise_N], c->ng.p, (size_t)cnt * noise_N * 8, st));
      const bool fl = poll && !c->pin.down_plain;
      HIPCHK(c, c->pin.flush_down(st, fl ? flag : nullptr, seq, done_ctr));
      if (!fl) flag = nullptr;
    } else if (!land) {
      HIPCHK(c, hipMemcpyAsync(hscal.data(), d_logdet, scal_bytes, hipMemcpyDeviceToHost, st));
    }
    // (bounded: a call that has not announced itself after 150 us -- a large batch, a busy device -- is waited for the
    // ordinary way, which also covers a device that never writes the word)
    const bool seen = poll && flag && !timing && poll_word(flag, seq, 150.0);
    if (seen) {
      ++c->small_polled;  // every store of the call is visible (the flag was its last); the stream drains by itself
    } else {
      HIPCHK(c, hipStreamSynchronize(st));
      ++c->small_synced;
    }
    c->pin.finish();
    if (land) memcpy(hscal.data(), land, scal_bytes);
    memcpy(&logdet[s0], hscal.data(), (size_t)cnt * 8);
    memcpy(&quad[s0], hscal.data() + cnt, (size_t)cnt * 8);
    if (getenv("GPC_SCALAR_LOG"))
      for (int i = 0; i < cnt; ++i)
        fprintf(stderr, "[gpcore] sample %d logdet %.17g quad %.17g\n", s0 + i, logdet[s0 + i], quad[s0 + i]);
    const int* hinfo = reinterpret_cast<const int*>(hscal.data() + 2 * (size_t)cnt);
    hc.lap("d2h+sync");
    for (int i = 0; i < cnt; ++i) b.info[s0 + i] = hinfo[i];
    for (int i = 0; i < cnt; ++i)
      if (hinfo[i] & LEAF_TIMEOUT) {
        c->err = "internal error: a hand-off between the waves of a 128 x 128 leaf factorization timed out (sample " +
                 std::to_string(s0 + i) + "); the results of this call are invalid";
        return -3;
      }
    if (timing) {
      float t03 = 0, t12 = 0;
      (void)hipEventElapsedTime(&t03, c->ev[0], c->ev[3]);
      (void)hipEventElapsedTime(&t12, c->ev[1], c->ev[2]);
      c->ms_total += t03;
      c->ms_factor += t12;
    }
    return 0;
  }

  // run the device pipeline for samples [s0, s0+cnt) whose matrices start at slot `slot`.
  // The chunk is split into sample groups on separate HIP streams: the latency-bound
  // phases of one group (leaves, deep recursion levels) run beside the throughput-bound
  // GEMMs of the other.
  // One pipeline for the samples [s0, s0 + cnt).  A dataflow graph that aborted (a bounded wait ran out: never
  // expected) is not an error of the call: the batch goes again on the stream-ordered schedule.
#ifdef GPC_EXPERIMENTS
  static constexpr int DAG_RETRY = 77;
  bool dag_off_once = false;
  int run(int s0, int cnt, int slot) {
    int rc = run_once(s0, cnt, slot);
    if (rc == DAG_RETRY) {
      ++c->dag_aborts;
      if (getenv("GPC_DAG_LOG")) fprintf(stderr, "[gpcore] dataflow graph aborted; re-running on the stream-ordered schedule\n");
      dag_off_once = true;
      rc = run_once(s0, cnt, slot);
      dag_off_once = false;
    }
    return rc;
  }
#else
  int run(int s0, int cnt, int slot) { return run_once(s0, cnt, slot); }
#endif

  int run_once(int s0, int cnt, int slot) {
    Batch& b = *B;
    const int npad = b.npad, N = b.N, D = b.D;
    hipStream_t st = c->st;
    const size_t vb = (size_t)npad * sizeof(double);
    const int t64 = npad / CT, ntl = t64 * (t64 + 1) / 2;
    const int Pn = P();
    chunk_cnt = cnt;
    chunk_s0 = s0;
    // the pipe's matrix pointers are relative to chunk position 0
    T* A0 = A;
    T* W0 = W;
    T* T0 = Tm;
    A = A0 + (size_t)slot * sM;
    W = W0 + (size_t)slot * sM;
    Tm = T0 + (size_t)slot * sM;
    struct Restore {
      Pipe* p;
      T *a, *w, *t;
      ~Restore() { p->A = a; p->W = w; p->Tm = t; }
    } restore{this, A0, W0, T0};

    HIPCHK(c, c->xs.ensure((size_t)cnt * npad * D * sizeof(double)));
    HIPCHK(c, c->spb.ensure((size_t)cnt * SP_STRIDE * sizeof(double)));
    HIPCHK(c, c->mulb.ensure((size_t)cnt * D * sizeof(double)));
    HIPCHK(c, c->divb.ensure((size_t)cnt * D * sizeof(double)));
    HIPCHK(c, c->dvec.ensure(cnt * vb));
    HIPCHK(c, c->rvec.ensure(cnt * vb));
    HIPCHK(c, c->zvec.ensure(cnt * vb));
    HIPCHK(c, c->avec.ensure(cnt * vb));
    HIPCHK(c, c->tpart.ensure((size_t)cnt * (npad / TRC + 1) * vb));
    HIPCHK(c, c->scal.ensure((size_t)cnt * (2 * sizeof(double) + sizeof(int)) + 64));
    double* d_logdet = c->scal.as<double>();
    double* d_quad = d_logdet + cnt;
    int* d_info = reinterpret_cast<int*>(d_quad + cnt);
    if (mode == MODE_GRAD) {
      // (gradient observations: the contraction's per-tile partials, scratch.h's GobsTraceScratch, take the place of the
      // built-in kernels' -- one block serves either)
      const size_t gtb = gobs.Ng > 0 ? ScratchCarver::count<GobsTraceScratch>(cnt, gobs, Pn) : 0;
      HIPCHK(c, c->parts.ensure(std::max((size_t)cnt * ntl * Pn * sizeof(double), gtb)));
      HIPCHK(c, c->gout.ensure((size_t)cnt * Pn * sizeof(double)));
      HIPCHK(c, c->diagq.ensure(cnt * vb));
      if (mean_N > 0) {
        if (dm) HIPCHK(c, c->dmb.ensure((size_t)cnt * N * mean_N * 8));
        HIPCHK(c, c->mg.ensure((size_t)cnt * mean_N * 8));
      }
      if (noise_N > 0 && b.vec_noise) {
        HIPCHK(c, c->dsn2b.ensure((size_t)cnt * N * noise_N * 8));
        HIPCHK(c, c->ng.ensure((size_t)cnt * noise_N * 8));
      }
    }

    HostClock hc("run");
    c->pin.begin();
    c->pin.begin_gather();
    auto up = [&](void* dst, const void* src, size_t n) { return c->pin.stage(dst, src, n); };
    // (a one-leaf evaluation records its timing events only on request: each is a barrier packet on a 45 us pipeline)
    const bool small_cand = c->small_path && npad == TILE && !kmode() && !(stable || c->stable) && gpc::g_leaf_version == 5;
    // ... and so does every problem below N_pad = 2048, whose call is 0.1 - 1 ms of dependent launches (the timing of the
    // larger ones feeds bench.py's roofline figures and costs them nothing measurable)
    timing_on = c->small_timing != 0 || npad >= 2048;
    if (timing_on) HIPCHK(c, hipEventRecord(c->ev[0], st));
    const void* hsp = up(c->spb.p, &b.sp[(size_t)s0 * SP_STRIDE], (size_t)cnt * SP_STRIDE * 8);
    const void* hmul = up(c->mulb.p, &b.mul[(size_t)s0 * D], (size_t)cnt * D * 8);
    const void* hdv = up(c->divb.p, &b.dv[(size_t)s0 * D], (size_t)cnt * D * 8);
    // the scaled inputs of the whole chunk ride in the transfer kernel (device_section then starts with the build)
    prescaled = hmul && hdv && !kmode() && (size_t)cnt * npad * D * 8 <= (PinBuf::kGather << 2);
    if (prescaled) {
      XferDesc& u = c->pin.upd;
      u.X = c->dX.as<double>();
      u.mul = static_cast<const double*>(hmul);
      u.dv = static_cast<const double*>(hdv);
      u.xs = c->xs.as<double>();
      u.n = N;
      u.npad = npad;
      u.D = D;
      u.cnt = cnt;
    }
    // Problems that are ONE 128 x 128 leaf take a pipeline of their own (small_section below); there the diagonal term
    // is read from its staged host copy by the build itself and needs no device copy
    const bool small_ok = small_cand && hsp && hmul && hdv;
    // The diagonal term and r = y - m.  Scalar noise / a constant mean (gpc_nll_batch_cm) are ONE value per sample:
    // they are staged as such and expanded on the device by the upload kernel (no S x N arrays cross the bus).
    const void* hdvec = nullptr;
    const void* hr = nullptr;
    bool fill_dvec = false, fill_r = false;
    XferDesc& fu = c->pin.upd;
    if (!b.vec_noise && !kmode()) {
      if (void* h = c->pin.alloc((size_t)cnt * 8)) {
        for (int i = 0; i < cnt; ++i) static_cast<double*>(h)[i] = b.dvec[(size_t)(s0 + i) * npad];
        if (small_ok) {
          hdvec = h;  // read by the build of the one-leaf pipeline directly
        } else {
          fu.dval = static_cast<const double*>(h);
          fu.dvec_out = c->dvec.as<double>();
          fill_dvec = true;
        }
      }
    } else if (small_ok) {
      if (void* h = c->pin.alloc(cnt * vb)) {
        memcpy(h, &b.dvec[(size_t)s0 * npad], cnt * vb);
        hdvec = h;
      }
    }
    if (!hdvec && !fill_dvec) up(c->dvec.p, &b.dvec[(size_t)s0 * npad], cnt * vb);
    if (b.m_const) {
      if (void* h = c->pin.alloc((size_t)cnt * 8)) {
        memcpy(h, b.m + s0, (size_t)cnt * 8);
        fu.y = c->dY.as<double>();
        fu.m0 = static_cast<const double*>(h);
        fu.r_out = c->rvec.as<double>();
        fill_r = true;
      } else {
        // no pinned block for the per-sample constants: r = y - m0 (the same subtraction, so the same bits) is expanded
        // here and travels like every other staged input, with its plain-copy fallback
        r_expanded.assign((size_t)cnt * npad, 0.0);
        for (int i = 0; i < cnt; ++i)
          for (int k = 0; k < N; ++k) r_expanded[(size_t)i * npad + k] = b.y[k] - b.m[s0 + i];
        up(c->rvec.p, r_expanded.data(), cnt * vb);
      }
    } else {
      // r = y - m is read from its staged copy by the kernel that needs it (leaf_solve_kernel, at its start: the round
      // trip to host memory hides under the factorization)
      if (small_ok && hdvec)
        if (void* h = c->pin.alloc(cnt * vb)) {
          memcpy(h, &b.r[(size_t)s0 * npad], cnt * vb);
          hr = h;
        }
      if (!hr) up(c->rvec.p, &b.r[(size_t)s0 * npad], cnt * vb);
    }
    if (fill_dvec || fill_r) {
      fu.fn = N;
      fu.fnpad = npad;
      fu.fcnt = cnt;
    }
    // (dm == nullptr with mean_N = 1: the constant mean's derivative, all ones -- nothing to upload)
    if (mode == MODE_GRAD && mean_N > 0 && dm) up(c->dmb.p, dm + (size_t)s0 * N * mean_N, (size_t)cnt * N * mean_N * 8);
    if (mode == MODE_GRAD && noise_N > 0 && b.vec_noise)
      up(c->dsn2b.p, dsn2 + (size_t)s0 * N * noise_N, (size_t)cnt * N * noise_N * 8);
    // Problems that are ONE 128 x 128 leaf (N <= 128; decided by the problem size only, so that a row of a batch carries
    // the bits of its single evaluation): upload + build in one launch, leaf + both triangular products in one launch,
    // and an evaluation without gradient writes its three scalars straight into the host's landing block.  Two
    // launches instead of six (NLL), six instead of ten (gradient).  gpc_set_option("small_path", 0) turns it off.
    const size_t scal_bytes0 = (((size_t)cnt * (2 * sizeof(double) + sizeof(int))) + 7) & ~(size_t)7;
    if (small_ok && hdvec) {
      int rc = small_section(s0, cnt, static_cast<const double*>(hsp), static_cast<const double*>(hmul),
                             static_cast<const double*>(hdv), static_cast<const double*>(hdvec),
                             hr ? static_cast<const double*>(hr) : (const double*)c->rvec.as<double>(), scal_bytes0, hc);
      return rc;
    }
    // one kernel: every staged segment and the zeroing of [logdet | quad | info] (padded to whole words)
    // (+ 8 bytes: the counter of the download launch's completion flag, see XferDesc)
    HIPCHK(c, c->pin.flush_up(st, c->scal.p, scal_bytes0 + 8));

    hc.lap("h2d");
    int groups = c->groups;
    if (cnt < 2 * groups || npad < 1024 || kmode()) groups = 1;
    // Two sample groups on two streams pay for their half-size launches only when the batch is large: measured with
    // the final kernels (tools/batch_latency.py), one group is faster up to S (npad/4096)^3 = 64 in both modes --
    // N=1000 S=8: 0.78 -> 0.54 ms (NLL), 0.92 -> 0.68 ms (gradient); N=2000 S=8 NLL 1.78 -> 1.36 ms; cfg3 NLL-only
    // 9.44 -> 9.04 ms -- and two groups by 1-2 % beyond (N=4096 S=128).
    if ((double)cnt * std::pow((double)npad / 4096.0, 3.0) <= 64.0) groups = 1;
    // Deferred inverse products (plan.h): measured on MI355X (round-2 sweep, script since removed) they pay whenever the
    // latency-bound phases are a visible share of the batch -- S (npad/4096)^3 <= 64 with at least 4 samples:
    // N=2048 S=16 4.42 -> 4.04 ms, N=4096 S=4 8.59 -> 7.47, N=4096 S=16 21.5 -> 20.2, N=4096 S=32 39.4 -> 38.7
    // -- and cost a little beyond (N=8192 S=64: 556 -> 584 ms).  With them one sample group is better than two.
    defer_node = 0;
    if (mode != MODE_NLL && c->defer_min != 0 && (c->cu_map_ok || c->defer_min > 0)) {
      const double work = (double)cnt * std::pow((double)npad / 4096.0, 3.0);
      if (c->defer_min > 0)
        defer_node = c->defer_min;
      else if (cnt >= 4 && npad >= 2048 && work <= 64.0)
        defer_node = (npad / 2 / TILE) * TILE;
      // one or two samples of a large problem: the right child of the root is latency-bound for a long stretch
      // (top two levels, as above: N=8192 S=1 12.95 -> 12.2 ms, S=2 20.87 -> 19.97 ms; N=16384 fp32 S=1 40.0 -> 38.9 ms;
      // N=4096 S=1 loses 2 %, so not below work = 8)
      else if (cnt < 4 && work >= 8.0 && work <= 64.0)
        defer_node = (npad / 2 / TILE) * TILE;
      if (defer_node > 0) groups = 1;
    }
#ifdef GPC_EXPERIMENTS
    // right-looking panels with look-ahead (NLL-only evaluations; side stream + CU reservation: eager)
    use_rl = mode == MODE_NLL && c->rl_panel >= TILE && npad >= 4 * c->rl_panel && !(stable || c->stable) && !kmode();
    // Launch graphs: every one-group pipeline whose schedule lives on ONE stream (the deferred products and the split
    // build fork to side streams with CU-reserving launches and stay eager).  Round 3: up to npad = 4096 (round 2
    // stopped at 1024) -- N = 2000: 1.171 -> 1.137 ms, N = 4096: 3.03 -> 2.97 ms per single NLL+grad evaluation.
    // Tile-level dataflow (dag.h) instead of one launch per product: same tile arithmetic, so the choice may follow
    // the batch size.  One sample group, no deferred launches (the graph overlaps them by itself), eager.
    use_dag = false;
    c->dag_used = false;
    if (c->dag != 0 && !dag_off_once && !kmode() && !(stable || c->stable) && mode != MODE_POST && !use_rl &&
        gpc::g_leaf_version == 5 && c->cu_map_ok && xcds_seen(c) == NQ && npad >= 2 * TILE && c->dag_aborts < 3) {
      use_dag = c->dag > 0 || dag_auto(cnt, npad);
      if (use_dag) {
        groups = 1;
        defer_node = 0;
      }
    }
    // Independent pipelines (option "indep"): a batch of 2 .. indep_max samples of a large problem as one pipeline PER
    // SAMPLE on its own stream, every chip-filling launch persistent and off one CU per shader engine -- the leaves and small
    // launches of one sample then run on those CUs while another sample's products fill the rest (lock-step runs every
    // sample's chain at the same time and nothing beside it).  Same tiles, same bits.
    indep_mode = c->indep != 0 && !use_dag && !use_rl && !kmode() && !(stable || c->stable) && mode != MODE_POST && c->cu_map_ok &&
                 cnt >= 2 && cnt <= c->indep_max && npad >= 2048 && gpc::g_persist_spare >= 0;
    if (indep_mode) {
      groups = cnt;
      defer_node = 0;
    }
#endif
    // Launch graphs: every one-group pipeline whose schedule lives on ONE stream (the deferred products and the split
    // build fork to side streams with CU-reserving launches and stay eager), up to npad = 4096.
    if (groups == 1 && defer_node == 0 && !use_rl && !use_dag && c->graph_max_npad > 0 && npad <= c->graph_max_npad && !kmode()) {
      int rc = graph_section(cnt);
      if (rc) return rc;
    } else if (groups == 1) {
      int rc = device_section(st, 0, cnt, timing_on ? c->ev[1] : nullptr, timing_on ? c->ev[2] : nullptr);
      if (rc) return rc;
    } else {
      HIPCHK(c, hipEventRecord(c->ev_up, st));
      for (int g = 0; g < groups; ++g) {
        const int lo = (int)((long long)cnt * g / groups), hi = (int)((long long)cnt * (g + 1) / groups);
        hipStream_t sg = c->gst[g];
        HIPCHK(c, hipStreamWaitEvent(sg, c->ev_up, 0));
        int rc = device_section(sg, lo, hi - lo, (g == 0 && timing_on) ? c->ev[1] : nullptr, nullptr, g);
        if (rc) {  // the groups already launched still read this call's buffers: let them drain
          for (int h = 0; h <= g; ++h) (void)hipStreamSynchronize(c->gst[h]);
          (void)hipStreamSynchronize(st);
          return rc;
        }
        HIPCHK(c, hipEventRecord(c->ev_done[g], sg));
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_done[g], 0));
      }
      if (timing_on) HIPCHK(c, hipEventRecord(c->ev[2], st));
    }
    if (timing_on) HIPCHK(c, hipEventRecord(c->ev[3], st));

    hc.lap("launch");
    // results back
    std::vector<int> hinfo((cnt + 1) & ~1);
    // [logdet | quad | info] are contiguous on the device: one segment (info padded to a whole word)
    const size_t scal_bytes = (((size_t)cnt * (2 * sizeof(double) + sizeof(int))) + 7) & ~(size_t)7;
    std::vector<double> hscal(scal_bytes / 8);
    HIPCHK(c, c->pin.gather(hscal.data(), d_logdet, scal_bytes, st));
    if (mode == MODE_GRAD) {
      HIPCHK(c, c->pin.gather(&G[(size_t)s0 * Pn], c->gout.p, (size_t)cnt * Pn * 8, st));
      if (mean_N > 0) HIPCHK(c, c->pin.gather(&mg[(size_t)s0 * mean_N], c->mg.p, (size_t)cnt * mean_N * 8, st));
      if (noise_N > 0 && b.vec_noise)
        HIPCHK(c, c->pin.gather(&ng[(size_t)s0 * noise_N], c->ng.p, (size_t)cnt * noise_N * 8, st));
    }
#ifdef GPC_EXPERIMENTS
    int dag_words[2] = {0, 0};  // [abort, leaf servers started] of the graph, when one ran
    if (c->dag_used)
      HIPCHK(c, c->pin.gather(dag_words, reinterpret_cast<char*>(c->dag_ctl.p) + offsetof(DagCtl, abort), 8, st));
#endif
    // The call ends with the gathered download launch.  Below N_pad = 2048 the host watches the word that launch writes
    // last (XferDesc::flag) instead of the stream: the runtime's completion path costs several microseconds that a call
    // of 0.1 - 1 ms notices.  Bounded: after 2 ms without the word the stream is waited for the ordinary way.
    const bool poll = !timing_on && c->small_poll && c->land_blk && !kmode() && !c->pin.down_plain && !c->check_queues &&
                      c->pin.downd.nseg > 0;
    unsigned long long* flag = poll ? reinterpret_cast<unsigned long long*>(c->land_blk + (gpc_ctx::LAND_BYTES / 8 - 1)) : nullptr;
    const unsigned long long seq = ++c->land_seq;
    HIPCHK(c, c->pin.flush_down(st, flag, seq, reinterpret_cast<int*>(reinterpret_cast<char*>(c->scal.p) + scal_bytes0)));
    const bool seen = poll && poll_word(flag, seq, 2000.0);
    if (seen) {
      ++c->small_polled;
    } else {
      HIPCHK(c, hipStreamSynchronize(st));
      if (poll) ++c->small_synced;
    }
    c->pin.finish();
#ifdef GPC_EXPERIMENTS
    if (c->dag_used && dag_trace_n > 0 && getenv("GPC_DAG_TRACE")) {  // every (sample, task)'s times, one line each, to the named file
      std::vector<long long> tr((size_t)dag_trace_n * 6);
      (void)hipMemcpy(tr.data(), c->dbg2.p, tr.size() * sizeof(long long), hipMemcpyDeviceToHost);
      if (FILE* f = fopen(getenv("GPC_DAG_TRACE"), "w")) {
        for (int t = 0; t < dag_trace_n; ++t)
          fprintf(f, "%d %lld %lld %lld %lld %lld %lld\n", t, tr[(size_t)t * 6], tr[(size_t)t * 6 + 1], tr[(size_t)t * 6 + 2],
                  tr[(size_t)t * 6 + 3], tr[(size_t)t * 6 + 4], tr[(size_t)t * 6 + 5]);
        fclose(f);
      }
      dag_trace_n = 0;
    }
#ifdef GPC_TILE_TRACE
    if (c->dag_used && getenv("GPC_DAG_STATS")) {
      unsigned long long tt[2][4];
      (void)hipMemcpyFromSymbol(tt, HIP_SYMBOL(gpc::g_tile_trace), sizeof tt);
      unsigned long long zero[2][4] = {};
      (void)hipMemcpyToSymbol(HIP_SYMBOL(gpc::g_tile_trace), zero, sizeof zero);
      for (int q = 0; q < 2; ++q)
        if (tt[q][3])
          fprintf(stderr, "[gpcore] %s-tile tasks: %llu; us per task (thread 0): prologue %.2f, k-loop %.2f, epilogue (loads of C, stores issued) %.2f\n",
                  q ? "64" : "128", tt[q][3], tt[q][0] / 100.0 / tt[q][3], tt[q][1] / 100.0 / tt[q][3], tt[q][2] / 100.0 / tt[q][3]);
    }
#endif
    if (c->dag_used && getenv("GPC_DAG_STATS")) {
      DagCtl h;
      (void)hipMemcpy(&h, c->dag_ctl.p, sizeof h, hipMemcpyDeviceToHost);
      const double w = std::max<double>(1.0, (double)h.n_workers), k = 1e-3 / 100.0;  // clock64: 100 MHz constant clock -> us
      fprintf(stderr, "[gpcore] dag stats: %llu workers, %llu tasks (%llu kept); per worker us: life %.0f = pop %.0f + acquire %.0f + run %.0f + complete %.0f; "
                      "per task us: pop %.2f acquire %.2f run %.2f complete %.2f\n", h.n_workers, h.n_tasks, h.n_kept, h.t_life / w * k * 1e3,
              h.t_pop / w * k * 1e3, h.t_acq / w * k * 1e3, h.t_exec / w * k * 1e3, h.t_done / w * k * 1e3,
              h.t_pop * k * 1e3 / std::max<double>(1.0, (double)h.n_tasks), h.t_acq * k * 1e3 / std::max<double>(1.0, (double)h.n_tasks),
              h.t_exec * k * 1e3 / std::max<double>(1.0, (double)h.n_tasks), h.t_done * k * 1e3 / std::max<double>(1.0, (double)h.n_tasks));
    }
    if (c->dag_used && dag_words[0] != 0) {
      if (getenv("GPC_DAG_LOG")) {
        DagCtl h;
        (void)hipMemcpy(&h, c->dag_ctl.p, sizeof h, hipMemcpyDeviceToHost);
        fprintf(stderr, "[gpcore] dag abort code %d, leaf servers started %d, remaining %d, reserve started %d survivors %d; rings (head/tail):",
                h.abort, h.leaf_alive, h.remaining, h.reserve_ctr[CTR_STARTED], h.reserve_ctr[CTR_SURVIVORS]);
        for (int r = 0; r < DAG_NRINGS; ++r) fprintf(stderr, " %d/%d", *h.ring[r].head(), *h.ring[r].tail());
        fprintf(stderr, "; us: leaf server start %d, first worker start %d, first worker exit %d; leaf servers saw (head tail remaining | exit us):",
                h.pad[0], h.pad[1], h.pad[2]);
        for (int q = 0; q < 4; ++q) fprintf(stderr, " [%d %d %d | %d]", h.pad[4 + 4 * q], h.pad[5 + 4 * q], h.pad[6 + 4 * q], h.pad[7 + 4 * q]);
        fprintf(stderr, "\n");
      }
      for (int g = 0; g <= gpc_ctx::MAXG; ++g) lauum_n[g] = 0;
      return DAG_RETRY;
    }
#endif
    memcpy(&logdet[s0], hscal.data(), (size_t)cnt * 8);
    memcpy(&quad[s0], hscal.data() + cnt, (size_t)cnt * 8);
    if (getenv("GPC_SCALAR_LOG"))
      for (int i = 0; i < cnt; ++i)
        fprintf(stderr, "[gpcore] sample %d logdet %.17g quad %.17g\n", s0 + i, logdet[s0 + i], quad[s0 + i]);
    memcpy(hinfo.data(), hscal.data() + 2 * (size_t)cnt, (size_t)cnt * sizeof(int));
    hc.lap("d2h+sync");
    for (int i = 0; i < cnt; ++i) b.info[s0 + i] = hinfo[i];
    for (int i = 0; i < cnt; ++i)
      if (hinfo[i] & LEAF_TIMEOUT) {
        c->err = "internal error: a hand-off between the waves of a 128 x 128 leaf factorization timed out (sample " +
                 std::to_string(s0 + i) + "); the results of this call are invalid";
        return -3;
      }
    if (c->check_queues) {
      int rc = verify_queues();
      if (rc) return rc;
    }
    if (kmode() && mode == MODE_GRAD && gobs.Ng == 0)
      for (int i = 0; i < cnt; ++i)
        if (hinfo[i] == 0) {
          int rc = trace_planes(s0 + i, slot + i);
          if (rc) return rc;
        }
    if (timing_on) {
      float t03 = 0, t12 = 0;
      (void)hipEventElapsedTime(&t03, c->ev[0], c->ev[3]);
      (void)hipEventElapsedTime(&t12, c->ev[1], c->ev[2]);
      c->ms_total += t03;
      c->ms_factor += t12;
    }
    if (mode == MODE_GRAD) {  // the dominant single kernel: the lauum launch of each group
      for (int g = 0; g <= gpc_ctx::MAXG; ++g)
        if (lauum_n[g] != 0) {
          float t = 0;
          if (timing_on) (void)hipEventElapsedTime(&t, c->ev_l0[g], c->ev_l1[g]);  // (else the stream was not waited for)
          if (t > c->ms_lauum) {
            c->ms_lauum = t;
            // (negative count: the timed launch is the dataflow graph -- factorization, inverse and W^T W of every
            // sample: S N^3 algorithmic flops)
            c->flops_lauum = lauum_n[g] > 0 ? (double)lauum_n[g] * (double)b.N * b.N * b.N / 3.0
                                            : (double)(-lauum_n[g]) * (double)b.N * b.N * b.N;
          }
          lauum_n[g] = 0;
        }
    }
    return 0;
  }

  // Jitter escalation (gaussian_process.py:2413-2421): every sample of [s0, s0+cnt) whose
  // factorization failed goes again with sn2_mult *= 10, up to 10 tries -- ALL failed samples of
  // a level as ONE batch (a 1024-point design with many non-PD rows costs at most 9 extra device
  // pipelines, not 9 per failed sample).  The sub-batch is computed in the scratch matrices
  // wA/wW/wT (slot i = i-th failed sample); commit(s, i) runs after a level for every sample s
  // that succeeded in slot i, before the next level overwrites the slots.
  template <typename Commit>
  int retry_failed(int s0, int cnt, T* wA, T* wW, T* wT, Commit&& commit) {
    Batch& b = *B;
    const int N = b.N, cov_N = b.cd.cov_N, Pn = P();
    const int nsn = b.vec_noise ? N : 1;
    std::vector<int> fail;
    for (int s = s0; s < s0 + cnt; ++s)
      if (b.info[s] != 0) {
        fail.push_back(s);
        b.tries[s] = 1;
      }
    // The attempt that failed ran in fast mode (trsm as a product with an explicit inverse: not backward stable when
    // the factor is ill-conditioned, plan.h).  The first retry repeats the SAME multiplier in stable mode -- where
    // LAPACK, i.e. the reference, may well succeed -- and every later level (x 10 each, ten levels in all like
    // :2413-2421) runs in stable mode too.
    bool same_level = !(stable || c->stable);
    while (!fail.empty() && (same_level || b.tries[fail[0]] < 10)) {
      const int nf = (int)fail.size();
      Batch sb;
      sb.S = nf;
      sb.N = N;
      sb.D = b.D;
      sb.npad = b.npad;
      sb.cd = b.cd;
      sb.vec_noise = b.vec_noise;
      sb.y = b.y;
      std::vector<double> hc(b.hyp_cov ? (size_t)nf * cov_N : 0), mm((size_t)nf * (b.m_const ? 1 : N)), sn((size_t)nf * nsn), gdm, gds;
      const bool gm = mode == MODE_GRAD && mean_N > 0 && dm, gn = mode == MODE_GRAD && noise_N > 0 && b.vec_noise;
      sb.m_const = b.m_const;
      if (gm) gdm.resize((size_t)nf * N * mean_N);
      if (gn) gds.resize((size_t)nf * N * noise_N);
      for (int i = 0; i < nf; ++i) {
        const int s = fail[i];
        if (b.hyp_cov) std::copy_n(b.hyp_cov + (size_t)s * cov_N, cov_N, &hc[(size_t)i * cov_N]);
        if (b.m_const)
          mm[i] = b.m[s];
        else
          std::copy_n(b.m + (size_t)s * N, N, &mm[(size_t)i * N]);
        std::copy_n(b.sn2 + (size_t)s * nsn, nsn, &sn[(size_t)i * nsn]);
        if (gm) std::copy_n(dm + (size_t)s * N * mean_N, (size_t)N * mean_N, &gdm[(size_t)i * N * mean_N]);
        if (gn) std::copy_n(dsn2 + (size_t)s * N * noise_N, (size_t)N * noise_N, &gds[(size_t)i * N * noise_N]);
      }
      sb.hyp_cov = b.hyp_cov ? hc.data() : nullptr;
      sb.m = mm.data();
      sb.sn2 = sn.data();
      sb.init();
      for (int i = 0; i < nf; ++i) {
        const int s = fail[i];
        if (!same_level) {
          b.mult[s] *= 10.0;
          b.tries[s] += 1;
          b.apply_mult(s);
        }
        sb.mult[i] = b.mult[s];
        sb.apply_mult(i);
      }
      same_level = false;
      Pipe<T> q;
      q.c = c;
      q.B = &sb;
      q.mode = mode;
      q.stable = true;
      q.A = wA;
      q.W = wW;
      q.Tm = wT;
      q.sM = sM;
      q.dm = gm ? gdm.data() : dm;  // scalar-noise dsn2 / absent dm are not read by the device
      q.mean_N = mean_N;
      q.dsn2 = gn ? gds.data() : dsn2;
      q.noise_N = noise_N;
      q.gobs = gobs;
      if (!Kptr.empty()) {
        q.dk_cb = dk_cb;
        q.dk_user = dk_user;
        for (int i = 0; i < nf; ++i) {
          q.Kptr.push_back(Kptr[fail[i]]);
          q.orig.push_back(orig.empty() ? fail[i] : orig[fail[i]]);
        }
      }
      q.logdet.assign(nf, 0.0);
      q.quad.assign(nf, 0.0);
      q.G.assign((size_t)nf * Pn, 0.0);
      q.mg.assign((size_t)nf * std::max(mean_N, 1), 0.0);
      q.ng.assign((size_t)nf * std::max(noise_N, 1), 0.0);
      int rc = q.run(0, nf, 0);
      if (rc) return rc;
      ++c->retry_runs;
      std::vector<int> still;
      for (int i = 0; i < nf; ++i) {
        const int s = fail[i];
        b.info[s] = sb.info[i];
        if (sb.info[i] != 0) {
          still.push_back(s);
          continue;
        }
        logdet[s] = q.logdet[i];
        quad[s] = q.quad[i];
        if (mode == MODE_GRAD) {
          std::copy_n(&q.G[(size_t)i * Pn], Pn, &G[(size_t)s * Pn]);
          if (mean_N > 0) std::copy_n(&q.mg[(size_t)i * mean_N], mean_N, &mg[(size_t)s * mean_N]);
          if (noise_N > 0) std::copy_n(&q.ng[(size_t)i * noise_N], noise_N, &ng[(size_t)s * noise_N]);
        }
        rc = commit(s, i);
        if (rc) return rc;
      }
      fail.swap(still);
    }
    return 0;
  }
};

size_t free_device_bytes() {
  // GPC_MEM_BUDGET_MB caps what the library considers free (tests use it to force the
  // sample-chunking paths)
  if (const char* e = getenv("GPC_MEM_BUDGET_MB")) return (size_t)atoll(e) << 20;
  size_t f = 0, t = 0;
  if (hipMemGetInfo(&f, &t) != hipSuccess) return (size_t)8 << 30;
  return f;
}

// ---- what every posterior consumer shares (DESIGN.md "Posterior consumers") ---------------------------------------
// The samples per chunk of a call (common.h: chunk_from_budget): all S when the scratch held from earlier calls `fits`
// and no budget is forced (GPC_MEM_BUDGET_MB, the tests' way into the chunked paths).  Otherwise the pool is given back
// and 80 % of [free memory + `held`, the scratch this call may regrow, - `reserve`, what it allocates beside] is divided;
// a forced budget stands for the scratch alone.  Returns 0 with c->err = what(budget) when a caller that does not clamp
// to one sample cannot fit one.  (hipMemGetInfo is slow: consulted here only.)
template <typename What = std::string (*)(size_t)>
int plan_chunk(gpc_ctx* c, int S, size_t per, size_t shared, size_t held, bool fits, size_t reserve, bool clamp_to_one,
               What&& what = nullptr) {
  const bool forced = getenv("GPC_MEM_BUDGET_MB") != nullptr;
  if (!forced && fits) return c->last_chunk = S;
  c->pool_drain();
  size_t avail = free_device_bytes() + (forced ? 0 : held);
  if (!forced) avail = avail > reserve ? avail - reserve : 0;
  const size_t budget = (size_t)(avail * 0.8);
  const int chunk = chunk_from_budget(S, per, shared, budget, clamp_to_one);
  if (!chunk) c->err = what(budget);
  return c->last_chunk = chunk;
}

// A consumer reads every sample's factor: none may have failed
inline int require_factorized(const gpc_post* po, const char* fn) {
  for (int s = 0; s < po->S; ++s)
    if (po->info[s] != 0) FAIL(po->ctx, std::string(fn) + ": posterior contains a failed factorization");
  return 0;
}

// Posteriors over values AND gradients have joint rows no other consumer knows how to build operands for
inline int refuse_gobs(const gpc_post* po, const char* fn) {
  if (po->gobs.Ng > 0)
    FAIL(po->ctx, std::string(fn) + ": this posterior was conditioned on gradient observations (gpc_posterior_batch_gobs); "
                  "only gpc_predict_gobs, gpc_grad_post_gobs, gpc_post_fetch and gpc_post_free work on it");
  return 0;
}

// fn(a, len, lch) for every run of equal L_chol among samples s0 .. s0 + cnt - 1 (the run starts at s0 + a and shares
// launches).  Every kernel works per sample in an order fixed by the shape: cutting runs or chunks changes no bit.
template <typename Fn>
int for_lchol_runs(const gpc_post* po, int s0, int cnt, Fn&& fn) {
  for (int a = 0; a < cnt;) {
    int e = a;
    while (e < cnt && po->lchol[s0 + e] == po->lchol[s0 + a]) ++e;
    if (int rc = fn(a, e - a, po->lchol[s0 + a] != 0)) return rc;
    a = e;
  }
  return 0;
}

// C = A B for a batch of n x n left operands A (stride sA) and n x ncols panels B, C (stride sB, leading dimension
// ld): `lower` = A is lower triangular, tile row ti needs k < (ti + 1) 128 only (KHI_ROW)
inline GemmArgs tri_gemm_args(const void* A, long long sA, int n, bool lower, const void* B, void* C, long long sB, int ld,
                              int ncols) {
  GemmArgs g;
  g.A = A, g.B = B, g.C = C;
  g.sA = sA, g.sB = g.sC = sB;
  g.lda = n, g.ldb = g.ldc = ld;
  g.M = n, g.N = ncols, g.K = n;
  g.alpha = 1.0, g.beta = 0;
  g.klo = KLO_ZERO, g.khi = lower ? KHI_ROW : KHI_FULL, g.lower_only = 0;
  return g;
}
// ... with the posterior's own left operand from sample s_first on: V = W R (L_chol) | G = L R (L = -inv, full)
template <typename T>
GemmArgs tri_product_args(const gpc_post* po, int s_first, bool lch, const T* B, T* C, long long sB, int ldb, int ncols) {
  const long long sM = (long long)po->npad * po->npad;
  return tri_gemm_args((lch ? po->W.as<T>() : po->A.as<T>()) + (size_t)s_first * sM, sM, po->npad, lch, B, C, sB, ldb, ncols);
}

// ... and the second product of an L_chol run on top of such a g: Q = W^T V (launched with the A operand transposed:
// the upper triangular W^T, k from the tile row's diagonal block on)
inline GemmArgs wt_product_args(GemmArgs g, const void* V, void* Q) {
  g.B = V, g.C = Q;
  g.klo = KLO_ROW, g.khi = KHI_FULL;
  return g;
}

// The four timing events of a call: gpc_last_timing reports ev[0] -> ev[3] as its device time, ev[1] -> ev[2] as its
// products'.  Each is a barrier packet on the stream: below N_pad = 2048 recorded on request only ("small_timing").
struct CallTimer {
  gpc_ctx* c;
  bool on;
  static bool wanted(const gpc_ctx* c, int npad) { return c->small_timing != 0 || npad >= 2048; }
  hipError_t record(int i) { return on ? hipEventRecord(c->ev[i], c->st) : hipSuccess; }
  hipError_t start() { return record(0); }
  hipError_t mark1() { return record(1); }
  hipError_t mark2() { return record(2); }
  hipError_t stop() { return record(3); }
  void accumulate() {  // (after the stream has been waited for)
    if (!on) return;
    float t03 = 0, t12 = 0;
    (void)hipEventElapsedTime(&t03, c->ev[0], c->ev[3]);
    (void)hipEventElapsedTime(&t12, c->ev[1], c->ev[2]);
    c->ms_total += t03;
    c->ms_factor += t12;
  }
};

// Landing block of a chunk's results: pinned when there is room, else pageable (uninitialised: all of it is downloaded)
inline double* landing_block(gpc_ctx* c, size_t bytes, std::unique_ptr<double[]>& spare) {
  double* p = bytes <= PinBuf::kMax ? static_cast<double*>(c->pin.alloc(bytes)) : nullptr;
  if (!p) {
    spare.reset(new double[bytes / 8]);
    p = spare.get();
  }
  return p;
}
// out[jl * S + s0 + i] = f * plane[i * ss + jl], jl < n: the chunk's samples side by side, the output written in order
inline void scatter_plane(double* out, const double* plane, size_t n, size_t ss, int S, int s0, int cnt, double f = 1.0) {
  for (size_t jl = 0; jl < n; ++jl) {
    double* o = out + jl * S + s0;
    for (int i = 0; i < cnt; ++i) o[i] = f * plane[i * ss + jl];
  }
}

// caller-provided covariance matrices (K-mode): S matrices of N x N doubles, and the dK plane callback
// (K == nullptr with gobs.Ng > 0: the matrices are built on the device from gradient observations, gradobs.h)
struct KArgs {
  const double* K = nullptr;
  gpc_dk_plane_fn cb = nullptr;
  void* user = nullptr;
  GobsDims gobs;
};
template <typename PipeT>
void set_kmode(PipeT& p, const KArgs* km, int S, int N) {
  if (!km) return;
  p.gobs = km->gobs;
  for (int s = 0; km->K && s < S; ++s) p.Kptr.push_back(km->K + (size_t)s * N * N);
  p.dk_cb = km->cb;
  p.dk_user = km->user;
}

template <typename T>
int nll_impl(gpc_ctx* c, Batch& b, int want_grad, const double* dm, int mean_N, const double* dsn2,
             int noise_N, double* nlz, double* dnlz, double* sn2_mult, int* L_chol, int* info,
             const KArgs* km = nullptr) {
  const int S = b.S, npad = b.npad, N = b.N;
  const size_t per = 3ull * npad * npad * sizeof(T);
  const size_t one = (size_t)npad * npad * sizeof(T);
  // (when the workspace must grow, the chunk is sized to what is free; one sample runs whatever the budget says)
  const int chunk = plan_chunk(c, S, per, 0, c->mA.bytes + c->mW.bytes + c->mT.bytes,
                               (size_t)S * one <= std::min(c->mA.bytes, std::min(c->mW.bytes, c->mT.bytes)), 0, true);
  HIPCHK(c, c->mA.ensure((size_t)chunk * npad * npad * sizeof(T)));
  HIPCHK(c, c->mW.ensure((size_t)chunk * npad * npad * sizeof(T)));
  HIPCHK(c, c->mT.ensure((size_t)chunk * npad * npad * sizeof(T)));

  Pipe<T> p;
  p.c = c;
  p.B = &b;
  p.mode = want_grad ? MODE_GRAD : MODE_NLL;
  p.A = c->mA.as<T>();
  p.W = c->mW.as<T>();
  p.Tm = c->mT.as<T>();
  p.sM = (long long)npad * npad;
  p.dm = dm;
  p.mean_N = mean_N;
  p.dsn2 = dsn2;
  p.noise_N = noise_N;
  set_kmode(p, km, S, N);
  const int Pn = p.P();
  p.logdet.assign(S, 0.0);
  p.quad.assign(S, 0.0);
  p.G.assign((size_t)S * Pn, 0.0);
  p.mg.assign((size_t)S * std::max(mean_N, 1), 0.0);
  p.ng.assign((size_t)S * std::max(noise_N, 1), 0.0);

  c->ms_total = c->ms_factor = 0;
  c->ms_lauum = c->flops_lauum = 0;
  c->last_flops = 0;
  c->retry_runs = 0;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    int rc = p.run(s0, cnt, 0);
    if (rc) return rc;
    rc = p.retry_failed(s0, cnt, p.A, p.W, p.Tm, [](int, int) { return 0; });
    if (rc) return rc;
  }
  const int cov_N = b.cd.cov_N;
  const int hyp_N = cov_N + noise_N + mean_N;
  for (int s = 0; s < S; ++s) {
    const double sl = b.sl[s];
    nlz[s] = 0.5 * p.quad[s] / sl + p.logdet[s] + N * std::log(2 * M_PI * sl) / 2;
    sn2_mult[s] = b.mult[s];
    L_chol[s] = b.lchol[s];
    info[s] = b.info[s];
    if (want_grad) {
      double* g = dnlz + (size_t)s * hyp_N;
      for (int h = 0; h < cov_N; ++h) g[h] = p.G[(size_t)s * Pn + h] / 2;  // :2487-2488
      const double trQ = p.G[(size_t)s * Pn + cov_N];
      for (int i = 0; i < noise_N; ++i) {
        if (b.vec_noise)
          g[cov_N + i] = 0.5 * b.mult[s] * p.ng[(size_t)s * noise_N + i];  // :2500-2504
        else
          g[cov_N + i] = 0.5 * b.mult[s] * dsn2[(size_t)s * noise_N + i] * trQ;  // :2491-2498
      }
      for (int i = 0; i < mean_N; ++i) g[cov_N + noise_N + i] = -p.mg[(size_t)s * mean_N + i];  // :2507-2508
    }
  }
  return 0;
}

int check_batch_args(gpc_ctx* c, int kernel_id, int degree, int dtype, int S, bool gobs = false) {
  if (!c) return -2;
  if (c->N <= 0) FAIL(c, "gpc_set_data has not been called");
  if (gobs != (c->gobs.Ng > 0) && kernel_id != -1)
    FAIL(c, gobs ? "the resident data hold no gradient observations: call gpc_set_data_gobs first"
                 : "the resident data hold gradient observations (gpc_set_data_gobs): only the _gobs and _K entry points "
                   "evaluate them; call gpc_set_data for the others");
  if (kernel_id != -1 && !valid_kernel(kernel_id, degree)) FAIL(c, "unknown covariance kernel / degree");
  if (dtype != GPC_F64 && dtype != GPC_F32) FAIL(c, "dtype must be GPC_F64 or GPC_F32");
  if (S <= 0) FAIL(c, "S must be positive");
  if (c->N > gpc_max_n(dtype))
    FAIL(c, "N is beyond what this device's memory holds for this dtype (three padded N x N slabs of one sample must fit "
            "in 80 % of it: gpc_max_n)");
  return 0;
}

void fill_batch(gpc_ctx* c, Batch& b, int kernel_id, int degree, int S, const double* hyp_cov,
                const double* m, const double* sn2, int vec, bool m_const = false) {
  b.m_const = m_const;
  b.S = S;
  b.N = c->N;
  b.D = c->D;
  b.npad = c->npad;
  b.cd.kind = kernel_id;
  b.cd.degree = degree;
  b.cd.D = c->D;
  b.cd.cov_N = kernel_id < 0 ? degree : cov_count_of(kernel_id, c->D);  // K-mode: `degree` carries cov_N
  b.vec_noise = vec != 0;
  b.hyp_cov = hyp_cov;
  b.m = m;
  b.sn2 = sn2;
  b.y = c->hy.data();
  b.mult0 = c->start_mult;
  b.init();
}

template <typename T>
int post_impl(gpc_ctx* c, Batch& b, gpc_post* po, double* sn2_mult, int* L_chol, int* info,
              const KArgs* km = nullptr, double* nlz = nullptr) {
  const int S = b.S, npad = b.npad;
  const size_t msz = (size_t)npad * npad * sizeof(T);
  HostClock hc("post");
  po->A = c->pool_take(S * msz);
  po->W = c->pool_take(S * msz);
  po->alpha = c->pool_take((size_t)S * npad * sizeof(double));
  if (!po->A.p || !po->W.p) c->pool_drain();  // nothing reusable: give the memory back before growing
  HIPCHK(c, po->A.ensure(S * msz));
  HIPCHK(c, po->W.ensure(S * msz));
  HIPCHK(c, po->alpha.ensure((size_t)S * npad * sizeof(double)));
  hc.lap("alloc A,W");
  const int chunk = plan_chunk(c, S, msz, 0, c->mT.bytes, (size_t)S * msz <= c->mT.bytes, 0, true);
  HIPCHK(c, c->mT.ensure((size_t)chunk * msz));
  hc.lap("alloc T");

  Pipe<T> p;
  p.c = c;
  p.B = &b;
  p.mode = MODE_POST;
  p.sM = (long long)npad * npad;
  set_kmode(p, km, S, b.N);
  p.logdet.assign(S, 0.0);
  p.quad.assign(S, 0.0);
  c->ms_total = c->ms_factor = 0;
  c->last_flops = 0;
  c->retry_runs = 0;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    // matrices of sample s live at po->A + s*sM; the pipe indexes from `slot`
    p.A = po->A.as<T>() + (size_t)s0 * p.sM;
    p.W = po->W.as<T>() + (size_t)s0 * p.sM;
    p.Tm = c->mT.as<T>();
    int rc = p.run(s0, cnt, 0);
    if (rc) return rc;
    auto save_alpha = [&](int s, int src_slot) -> int {
      HIPCHK(c, hipMemcpyAsync(po->alpha.as<double>() + (size_t)s * npad,
                               c->avec.as<double>() + (size_t)src_slot * npad, npad * sizeof(double),
                               hipMemcpyDeviceToDevice, c->st));
      return 0;
    };
    int nfail = 0;
    for (int i = 0; i < cnt; ++i) {
      if (b.info[s0 + i] == 0 && save_alpha(s0 + i, i)) return -1;
      nfail += b.info[s0 + i] != 0;
    }
    if (nfail) {  // retried in scratch matrices, successes copied into the posterior's slots
      HIPCHK(c, c->mA.ensure((size_t)nfail * msz));
      HIPCHK(c, c->mW.ensure((size_t)nfail * msz));
      rc = p.retry_failed(s0, cnt, c->mA.as<T>(), c->mW.as<T>(), c->mT.as<T>(), [&](int s, int i) -> int {
        HIPCHK(c, hipMemcpyAsync(po->A.as<T>() + (size_t)s * p.sM, c->mA.as<T>() + (size_t)i * p.sM, msz,
                                 hipMemcpyDeviceToDevice, c->st));
        HIPCHK(c, hipMemcpyAsync(po->W.as<T>() + (size_t)s * p.sM, c->mW.as<T>() + (size_t)i * p.sM, msz,
                                 hipMemcpyDeviceToDevice, c->st));
        return save_alpha(s, i);
      });
      if (rc) return rc;
    }
    // low-noise samples: Posterior.L = -(K + mult*Sigma)^-1  (gaussian_process.py:2441-2448)
    for (int s = s0; s < s0 + cnt; ++s)
      if (!b.lchol[s] && b.info[s] == 0) {
        Factor<T> F;
        F.st = c->st;
        F.batch = 1;
        F.npad = npad;
        F.A = po->A.as<T>() + (size_t)s * p.sM;
        F.W = po->W.as<T>() + (size_t)s * p.sM;
        F.Tm = c->mT.as<T>();
        F.sA = F.sW = F.sT = p.sM;
        F.lauum(F.Tm, p.sM);
        HIPCHK(c, F.err);
        dim3 g1(npad / 64, npad / 4, 1), blk(64, 4);
        hipLaunchKernelGGL((neg_sym_kernel<T>), g1, blk, 0, c->st, F.Tm, p.sM, npad, npad);
        HIPCHK(c, hipMemcpyAsync(F.A, F.Tm, msz, hipMemcpyDeviceToDevice, c->st));
        HIPCHK(c, hipGetLastError());
      }
    HIPCHK(c, hipStreamSynchronize(c->st));
  }
  hc.lap("device");
  po->dev_consts = false;
  po->sp = b.sp;
  po->mul = b.mul;
  po->dv = b.dv;
  po->mult = b.mult;
  po->lchol = b.lchol;
  po->info = b.info;
  po->sW.resize(S);
  for (int s = 0; s < S; ++s) {
    po->sW[s] = 1.0 / std::sqrt(b.smin[s] * b.mult[s]);  // :2517
    if (nlz) nlz[s] = 0.5 * p.quad[s] / b.sl[s] + p.logdet[s] + b.N * std::log(2 * M_PI * b.sl[s]) / 2;  // (as nll_impl)
    sn2_mult[s] = b.mult[s];
    L_chol[s] = b.lchol[s];
    info[s] = b.info[s];
  }
  return 0;
}

// A gpc_draw request (rhs_products with mode_full): the covariances C_s stay resident and are factored and
// multiplied on the device instead of being downloaded.
struct DrawReq {
  unsigned long long seed;
  int R;
  int s_offset;       // global index of the posterior's first sample (the random stream is keyed on it)
  const double* nsd;  // M x S noise standard deviations, or null
  double* f;          // M x R x S
  double* tau;        // S
};

// One chunk of draws: C_s (z.Kss, chunk layout) -> A = C_s + tau_s I -> L (batched Factor, stable retries with
// jitter for the samples that failed; the diagonal tiles cleaned above the diagonal) -> Z (normals_kernel) -> F = L Z (gemm.h: lower A operand, KHI_ROW skips the
// zero upper tiles) -> fmu + F (+ noise) into z.dout, copied to hout.  Every step is per sample with a reduction order
// fixed by the shape (the leaf and the product library do not depend on the batch), so a sample's draws carry the same
// bits in any batch or chunk.  Returns -3 with a message when a sample cannot be factored with the largest jitter.
template <typename T>
int draw_chunk(gpc_post* po, const DrawReq& d, int s0, int cnt, int M, const RhsScratch<T>& z, const double* d_nsd,
               double* hout) {
  gpc_ctx* c = po->ctx;
  hipStream_t st = c->st;
  const int mpad = pad_tile(M), R = d.R, rpad = pad_tile(R);
  const long long sKss = (long long)mpad * mpad, sZ = (long long)mpad * rpad;
  T* C = z.Kss;
  T* A = c->mA.as<T>();
  const double* d_mu = z.mu;
  double* logdet = z.logdet;
  int* info = z.info;
  const dim3 blk(64, 4);
  auto factor = [&](int i0, int n, double tau, bool stable) -> int {
    HIPCHK(c, hipMemsetAsync(logdet + i0, 0, (size_t)n * 8, st));
    HIPCHK(c, hipMemsetAsync(info + i0, 0, (size_t)n * sizeof(int), st));
    hipLaunchKernelGGL((jitter_load_kernel<T>), dim3(mpad / 64, mpad / 4, n), blk, 0, st, (const T*)(C + i0 * sKss),
                       A + i0 * sKss, sKss, mpad, M, tau);
    Factor<T> F;
    F.st = st;
    F.batch = n;
    F.npad = mpad;
    F.nvalid = M;
    F.A = A + i0 * sKss;
    F.W = c->mW.as<T>() + i0 * sKss;
    F.Tm = c->mT.as<T>() + i0 * sKss;
    F.sA = F.sW = F.sT = sKss;
    F.logdet = logdet + i0;
    F.info = info + i0;
    F.stable = stable;
    F.potrf_inv(0, mpad, false, true);
    HIPCHK(c, F.err);
    HIPCHK(c, hipGetLastError());
    return 0;
  };
  int rc = factor(0, cnt, 0.0, false);
  if (rc) return rc;
  std::vector<int> hinfo(cnt);
  HIPCHK(c, hipMemcpyAsync(hinfo.data(), info, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  for (int i = 0; i < cnt; ++i) {
    double tau = 0.0;
    if (hinfo[i] & LEAF_TIMEOUT) FAIL(c, "gpc_draw: internal error: a leaf of the factorization timed out");
    if (hinfo[i] != 0) {
      // jitter ladder: tau = t mean(diag C_s), t = 1e-12 .. 1e-6, stable mode, this sample alone
      std::vector<T> dg(M);
      HIPCHK(c, hipMemcpy2DAsync(dg.data(), sizeof(T), C + i * sKss, (size_t)(mpad + 1) * sizeof(T), sizeof(T), M,
                                 hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
      double mean = 0.0;
      for (int j = 0; j < M; ++j) mean += (double)dg[j];
      mean /= M;
      bool ok = false;
      for (int e = -12; e <= -6 && !ok; ++e) {
        tau = std::pow(10.0, (double)e) * mean;
        rc = factor(i, 1, tau, true);
        if (rc) return rc;
        int inf = 0;
        HIPCHK(c, hipMemcpyAsync(&inf, info + i, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (inf & LEAF_TIMEOUT) FAIL(c, "gpc_draw: internal error: a leaf of the factorization timed out");
        ok = inf == 0 && tau > 0;
      }
      if (!ok) {
        c->err = "gpc_draw: the posterior covariance of sample " + std::to_string(d.s_offset + s0 + i) +
                 " is not positive definite, even with a jitter of 1e-6 mean(diag C)";
        return -3;
      }
    }
    d.tau[s0 + i] = tau;
  }
  hipLaunchKernelGGL((diag_tile_upper_zero_kernel<T>), dim3(mpad / TILE, cnt), dim3(256), 0, st, A, sKss, mpad);
  const long long s_base = (long long)d.s_offset + s0;
  hipLaunchKernelGGL((normals_kernel<T>), dim3(rpad / 64, mpad / 16, cnt), blk, 0, st, d.seed, 0, s_base, M, R, mpad,
                     rpad, z.Z, sZ);
  const GemmArgs g = tri_gemm_args(A, sKss, mpad, true, z.Z, z.F, sZ, rpad, rpad);  // F = L Z
  HIPCHK(c, launch_gemm<T>(st, g, false, true, cnt));
  hipLaunchKernelGGL((draw_assemble_kernel<T>), dim3((R + 63) / 64, mpad / 16, cnt), blk, 0, st, (const T*)z.F,
                     sZ, rpad, d_mu, mpad, M, R, d_nsd, po->S, s0, d.seed, s_base, z.dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(hout, z.dout, (size_t)cnt * M * R * 8, hipMemcpyDeviceToHost, st));
  return 0;
}

// The constants of ALL samples of a posterior on the device (see gpc_post): the kernel's scalars, the input scaling and
// the scaled training inputs, uploaded and formed once per posterior
int post_consts_resident(gpc_post* po) {
  if (po->dev_consts) return 0;
  gpc_ctx* c = po->ctx;
  const int S = po->S, N = po->N, D = po->D, npad = po->npad;
  hipStream_t st = c->st;
  HIPCHK(c, po->dsp.ensure_private((size_t)S * SP_STRIDE * 8));
  HIPCHK(c, po->dmul.ensure_private((size_t)S * D * 8));
  HIPCHK(c, po->ddv.ensure_private((size_t)S * D * 8));
  HIPCHK(c, po->dxs.ensure_private((size_t)S * npad * D * 8));
  HIPCHK(c, hipMemcpyAsync(po->dsp.p, po->sp.data(), (size_t)S * SP_STRIDE * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(po->dmul.p, po->mul.data(), (size_t)S * D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(po->ddv.p, po->dv.data(), (size_t)S * D * 8, hipMemcpyHostToDevice, st));
  if (po->gobs.Ng > 0) {  // the scaled point lists of a gradient-observation posterior, from its own raw list
    HIPCHK(c, po->dxs.ensure_private((size_t)S * po->gobs.P() * D * 8));
    launch_gobs_scale(st, po->gobs, po->gpts.as<double>(), po->dmul.as<double>(), po->ddv.as<double>(), S,
                      po->dxs.as<double>());
    HIPCHK(c, hipGetLastError());
    po->dev_consts = true;
    return 0;
  }
  const long long tot = (long long)npad * D;
  hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)((tot + 255) / 256), S), dim3(256), 0, st, c->dX.as<double>(), N,
                     npad, D, po->dmul.as<double>(), po->ddv.as<double>(), po->dxs.as<double>());
  HIPCHK(c, hipGetLastError());
  po->dev_consts = true;
  return 0;
}

// The posterior's per-sample constants as the kernels of a chunk read them: the resident copies when the call works on
// all samples at once (the usual case), else the context's buffers, refilled for every chunk by stage().  The
// context's buffers are sized for a chunk either way: they count towards what later calls' planning finds held and free
struct ChunkConsts {
  gpc_post* po = nullptr;
  bool resident = false;
  const double *spb = nullptr, *mulb = nullptr, *divb = nullptr, *xsb = nullptr;
  int init(gpc_post* po_, int chunk, bool may_be_resident = true) {
    po = po_;
    resident = may_be_resident && chunk == po->S;
    gpc_ctx* c = po->ctx;
    HIPCHK(c, c->xs.ensure((size_t)chunk * po->npad * po->D * 8));
    HIPCHK(c, c->spb.ensure((size_t)chunk * SP_STRIDE * 8));
    HIPCHK(c, c->mulb.ensure((size_t)chunk * po->D * 8));
    HIPCHK(c, c->divb.ensure((size_t)chunk * po->D * 8));
    if (resident)
      if (int rc = post_consts_resident(po)) return rc;
    spb = resident ? po->dsp.as<double>() : c->spb.as<double>();
    mulb = resident ? po->dmul.as<double>() : c->mulb.as<double>();
    divb = resident ? po->ddv.as<double>() : c->divb.as<double>();
    xsb = resident ? po->dxs.as<double>() : c->xs.as<double>();
    return 0;
  }
  // samples s0 .. s0 + cnt - 1 into the context's buffers; need_xs: the scaled training inputs too
  int stage(int s0, int cnt, bool need_xs) {
    if (resident) return 0;
    gpc_ctx* c = po->ctx;
    const int D = po->D;
    HIPCHK(c, hipMemcpyAsync(c->spb.p, &po->sp[(size_t)s0 * SP_STRIDE], (size_t)cnt * SP_STRIDE * 8,
                             hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(c->mulb.p, &po->mul[(size_t)s0 * D], (size_t)cnt * D * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(c->divb.p, &po->dv[(size_t)s0 * D], (size_t)cnt * D * 8, hipMemcpyHostToDevice, c->st));
    if (need_xs) {
      const long long tot = (long long)po->npad * D;
      hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)((tot + 255) / 256), cnt), dim3(256), 0, c->st,
                         c->dX.as<double>(), po->N, po->npad, D, mulb, divb, c->xs.as<double>());
    }
    return 0;
  }
};

// Shared by predict / predict_full / quad: for every posterior sample s build a right-hand
// side matrix R_s (npad x mpad: cross covariances, or quadrature kernel means), then
//   lin[j*S+s]  = R_s[:, j] . alpha_s
//   quad[j*S+s] = |W_s R_s[:, j]|^2          (L_chol;  the caller divides by sl)
//               = R_s[:, j] . (L_s R_s[:, j]) (low noise, L = -inv)
//   full[s]     = Kss_s - (W R)^T (W R) / sl   or   Kss_s + R^T (L R)
//   dlin / dquad [(j*D + l)*S + s] = d lin / dx*_jl and d(kss - k*^T (K + Sigma)^-1 k*) / dx*_jl  (CROSS with
//                 want_quad only; covfun.h: cross_grad_tile_kernel): V is written (no EPI = 1 product), Q = W^T V
//                 is one more product of the same size (L_chol; the other samples use G = L R as it is)
//   draw        with `full`: C_s is factored and multiplied on the device (draw_chunk), not downloaded
//   qg          (QUAD_Z only; quad.h) d lin / d xa, d lin / d xb and, with want_quad, d quad / d xa, d quad / d xb, the
//                 last two under quad's convention (scaled by 1/sl or negated) and complete, [(j*D + l)*S + s].  Without
//                 want_quad there is no product at all; with it V is written as for dlin and Q = W^T V is formed
struct QuadGradOut {
  double* p[4];  // dza_dmu, dza_dsigma, dzkz_dmu, dzkz_dsigma
};
struct RhsRequest {
  enum Rhs {  // (RhsDims::of takes the values)
    CROSS = 0,    // cross covariance of xa (M x D) with the training inputs
    QUAD_Z = 1,   // quadrature vectors z of the Gaussian measures N(xa[j], diag(xb[j]^2)) (gaussian_process.py:1908-1921)
    GIVEN_KS = 2, // the caller's own Ks_s (xa: S x N x M doubles) and, with `full`, K**_s (xb: S x M x M): K-mode posteriors
    GOBS = 3      // the joint cross operand [k(X, xa) ; dk(X_g, xa)/dx_g] of a gradient-observation posterior (gradobs.h)
  };
  Rhs rhs = CROSS;
  const double* xa = nullptr;
  const double* xb = nullptr;
  int M = 0;
  bool want_quad = false;
  double* lin = nullptr;    // M x S, always
  double* quad = nullptr;   // M x S (want_quad)
  double* full = nullptr;   // S x M x M; with `draw`: only says that C_s is formed (it stays on the device)
  double* dlin = nullptr;   // CROSS with want_quad: the gradients of lin and of the variance, M x D x S each
  double* dquad = nullptr;
  const DrawReq* draw = nullptr;
  const QuadGradOut* qg = nullptr;  // QUAD_Z: the gradients with respect to the measures
};

// One rhs_products call: the sizes, the scratch and the landing blocks of the call, and the steps of a chunk in the
// order they go onto the stream.  Every step works per sample in an order fixed by the shape, so a sample carries the
// same bits in any batch, chunk or run.
template <typename T>
struct RhsCall {
  gpc_post* const po;
  const RhsRequest& r;
  gpc_ctx* const c;
  const hipStream_t st;
  const int S, N, D, npad, M, mpad;
  const long long sKs, sKss;
  const bool full, grad, gq;  // gq: the gradient pass reads Q (not without a product)
  // gnt: tile rows of the gradient pass; gpl: its result planes, [dmu | ds2] (CROSS) or [dza_dmu | dza_dsigma (| dzkz_dmu |
  // dzkz_dsigma)] (qg)
  const int gnt, gpl;
  int chunk = 0;
  CallTimer tm;
  ChunkConsts k;
  RhsScratch<T> z;
  RhsShared zs;
  // landing blocks of the per-chunk results
  std::unique_ptr<double[]> hmu_v, hdraw_v, hgrad_v;
  double *hmu = nullptr, *hv = nullptr, *hfull = nullptr, *hdraw = nullptr, *hgrad = nullptr;

  RhsCall(gpc_post* po_, const RhsRequest& r_)
      : po(po_), r(r_), c(po_->ctx), st(po_->ctx->st), S(po_->S), N(po_->N), D(po_->D), npad(po_->npad), M(r_.M),
        mpad(pad_tile(r_.M)), sKs((long long)npad * mpad), sKss((long long)mpad * mpad), full(r_.full != nullptr),
        grad(r_.dlin != nullptr || r_.qg != nullptr), gq(grad && (!r_.qg || r_.want_quad)), gnt(npad / CT),
        gpl(r_.qg && r_.want_quad ? 4 : 2), tm{po_->ctx, CallTimer::wanted(po_->ctx, po_->npad)} {}

  T* Ks() const { return z.Ks; }
  T* V() const { return z.V; }
  double* d_mu() const { return z.mu; }
  double* d_v() const { return d_mu() + (size_t)chunk * mpad; }
  const double* alpha(int s) const { return po->alpha.as<double>() + (size_t)s * npad; }
  bool colsq_form() const { return RhsDims::colsq_form(npad, mpad, full, grad); }
  RhsDims dims() const {
    return RhsDims::of(N, M, D, S, (int)r.rhs, r.want_quad, full, grad, r.qg != nullptr, r.draw ? r.draw->R : 0,
                       r.rhs == RhsRequest::GOBS ? po->gobs.P() : 0);
  }

  // The scratch of one sample, the samples per chunk, and the block of a chunk
  int plan() {
    const RhsDims d = dims();
    // (a draw factors in the factorization's own three slabs: they count beside the block)
    const size_t slab = d.template slab_bytes<T>();
    const size_t own = ScratchCarver::count<RhsScratch<T>>(1, d), per = own + 3 * slab;
    const size_t shared = ScratchCarver::count<RhsShared>(d);
    const size_t held = c->cs.bytes + (r.draw ? c->mA.bytes + c->mW.bytes + c->mT.bytes : 0);
    const bool fits = shared + (size_t)S * own <= c->cs.bytes && (size_t)S * slab <= std::min({c->mA.bytes, c->mW.bytes, c->mT.bytes});
    // (draws refuse a sample that does not fit; everything else runs one sample at a time whatever the budget says)
    chunk = plan_chunk(c, S, per, shared, held, fits, 0, !r.draw, [&](size_t budget) {
      return "gpc_draw: the scratch of one sample (" + std::to_string(per >> 20) + " MB) exceeds the device memory "
             "budget (" + std::to_string(budget >> 20) + " MB)";
    });
    if (!chunk) return -2;
    HIPCHK(c, c->cs.ensure(shared + (size_t)chunk * own));
    for (DevBuf* m : {&c->mA, &c->mW, &c->mT}) HIPCHK(c, m->ensure((size_t)chunk * slab));
    CARVECHK(c, "rhs_products", ScratchCarver::carve(z, c->cs.p, chunk, d) +
                                    ScratchCarver::carve(zs, c->cs.as<char>() + (size_t)chunk * own, d));
    return 0;
  }

  // The call's own uploads, the landing blocks of the per-chunk results and the posterior's constants
  int begin() {
    c->pin.begin();
    c->pin.begin_gather();
    if (r.rhs != RhsRequest::GIVEN_KS) {
      HIPCHK(c, c->pin.up(zs.xa, r.xa, (size_t)M * D * 8, st));
      if (r.xb) HIPCHK(c, c->pin.up(zs.xb, r.xb, (size_t)M * D * 8, st));
    }
    // (one block for lin and quad: the device keeps [mu | v] contiguous too, so a call's results come back in ONE copy)
    hmu = landing_block(c, 2 * (size_t)chunk * mpad * 8, hmu_v);
    hv = hmu + (size_t)chunk * mpad;
    if (full && !r.draw && (size_t)M * M * 8 >= PinBuf::kMin && (size_t)M * M * 8 <= PinBuf::kMax)
      hfull = static_cast<double*>(c->pin.alloc((size_t)M * M * 8));
    if (r.draw) {  // a chunk's draws, M x R per sample
      hdraw = landing_block(c, (size_t)chunk * M * r.draw->R * 8, hdraw_v);
      if (r.draw->nsd) HIPCHK(c, hipMemcpyAsync(zs.nsd, r.draw->nsd, (size_t)M * S * 8, hipMemcpyHostToDevice, st));
    }
    if (grad) hgrad = landing_block(c, (size_t)gpl * chunk * mpad * D * 8, hgrad_v);  // the gradient planes of a chunk
    // all samples in one chunk (the usual case): the posterior's constants are resident, see gpc_post
    return k.init(po, chunk, r.rhs != RhsRequest::GIVEN_KS);
  }

  // ---- the right-hand sides R_s of a chunk (into Ks) and lin = R_s^T alpha_s ----
  // cross covariances in 64 x 64 tiles with the mean product fused in (covfun.h: cross_tile_kernel)
  int build_cross(int s0, int cnt) {
    const long long tot = (long long)mpad * D;
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)((tot + 255) / 256), cnt), dim3(256), 0, st,
                       (const double*)zs.xa, M, mpad, D, k.mulb, k.divb, z.xss);
    GPC_COV_DISPATCH(cross_tile_kernel, T, po->cd, dim3(mpad / CT, npad / CT, cnt), dim3(256), 0, st, po->cd, k.xsb,
                     (const double*)z.xss, k.spb, alpha(s0), npad, N, npad, M, mpad, Ks(), sKs,
                     z.part);
    if (full)
      hipLaunchKernelGGL((cross_kernel<T>), dim3(mpad / 64, mpad / 4, cnt), dim3(64, 4), 0, st, po->cd,
                         z.xss, z.xss, k.spb, M, mpad, M, mpad, z.Kss, sKss);
    hipLaunchKernelGGL(colpart_reduce_kernel, dim3((mpad + 255) / 256, cnt), dim3(256), 0, st,
                       (const double*)z.part, npad / CT, mpad, d_mu());
    return 0;
  }
  // the joint cross operand of a gradient-observation posterior with the mean product fused in (gradobs.h:
  // gobs_cross_tile_kernel), from the posterior's own point list
  int build_gobs(int s0, int cnt) {
    const GobsDims& gd = po->gobs;
    const long long tot = (long long)mpad * D;
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)((tot + 255) / 256), cnt), dim3(256), 0, st,
                       (const double*)zs.xa, M, mpad, D, k.mulb, k.divb, z.xss);
    const double* xp = k.xsb;  // (all samples in one chunk: the posterior's resident scaled lists)
    if (!k.resident) {
      HIPCHK(c, c->gxs.ensure((size_t)cnt * gd.P() * D * 8));
      launch_gobs_scale(st, gd, po->gpts.as<double>(), k.mulb, k.divb, cnt, c->gxs.as<double>());
      xp = c->gxs.as<double>();
    }
    HIPCHK(c, launch_gobs_cross<T>(st, po->cd, gd, xp, z.xss, k.spb, k.mulb, k.divb, alpha(s0), npad, npad, M,
                                   mpad, cnt, Ks(), sKs, z.part, d_mu()));
    return 0;
  }
  // caller-provided cross covariances Ks_s (N x M doubles, xa) and, with `full`, K**_s (M x M, xb)
  int build_given(int s0, int cnt) {
    for (int i = 0; i < cnt; ++i) {
      HIPCHK(c, hipMemcpyAsync(zs.given, r.xa + (size_t)(s0 + i) * N * M, (size_t)N * M * 8, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL((pad_rect_kernel<T>), dim3(mpad / 64, npad / 4), dim3(64, 4), 0, st, (const double*)zs.given, N,
                         M, npad, mpad, Ks() + (size_t)i * sKs);
      if (full) {
        HIPCHK(c, hipMemcpyAsync(zs.given, r.xb + (size_t)(s0 + i) * M * M, (size_t)M * M * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL((pad_rect_kernel<T>), dim3(mpad / 64, mpad / 4), dim3(64, 4), 0, st, (const double*)zs.given,
                           M, M, mpad, mpad, z.Kss + (size_t)i * sKss);
      }
    }
    return column_sums(s0, cnt);
  }
  int build_quad_z(int s0, int cnt) {
    hipLaunchKernelGGL((quad_z_kernel<T>), dim3(mpad / 64, npad / 4, cnt), dim3(64, 4), 0, st, c->dX.as<double>(),
                       (const double*)zs.xa, (const double*)zs.xb, k.mulb, k.divb, k.spb, N, npad, M, mpad, D, Ks(), sKs);
    if (r.qg)
      hipLaunchKernelGGL(quad_grad_prep_kernel, dim3((mpad + 255) / 256, cnt), dim3(256), 0, st, (const double*)zs.xa,
                         (const double*)zs.xb, k.divb, k.spb, M, mpad, D, zs.mut, z.qcon);
    if (full)  // gpc_quad_cov: Gamma where CROSS puts K** (quad_mix.h)
      hipLaunchKernelGGL((quad_gamma_kernel<T>), dim3(mpad / 64, mpad / 4, cnt), dim3(64, 4), 0, st,
                         (const double*)zs.xa, (const double*)zs.xb, k.divb, k.spb, M, mpad, D, z.Kss, sKss);
    return column_sums(s0, cnt);
  }
  int column_sums(int s0, int cnt) {  // (the builders without a fused mean product)
    hipLaunchKernelGGL((colsum_vec_kernel<T>), dim3(mpad / 64, cnt), dim3(256), 0, st, (const T*)Ks(), sKs, mpad,
                       alpha(s0), npad, npad, mpad, d_mu());
    return 0;
  }

  // ---- one run of equal L_chol: the product, the variance term, the gradient tiles, the full covariance ----
  int run_products(int s0, int cnt, int a, int len, bool lch) {
    const bool last = a + len == cnt;
    T* const Ksa = Ks() + (size_t)a * sKs;
    T* const Va = V() + (size_t)a * sKs;
    GemmArgs g = tri_product_args<T>(po, s0 + a, lch, Ksa, Va, sKs, mpad, mpad);  // V = W R | G = L R
    if (lch && colsq_form()) {
      // the variance needs the column sums of squares of V only: the product's epilogue forms them per tile row and V
      // is never written (gemm.h: EPI = 1); a small reduction over the tile rows follows
      const int tmr = npad / TILE;
      int* qctr = c->tile_ctr.as<int>() + (size_t)gpc_ctx::MAXG * gpc_ctx::CTR_PER_GROUP;
      HIPCHK(c, hipMemsetAsync(qctr, 0, CTR_STRIDE * sizeof(int), st));
      HIPCHK(c, tm.mark1());
      g.colsq = z.colsq;
      HIPCHK(c, launch_gemm_colsq<T>(st, g, len, qctr));
      if (last) HIPCHK(c, tm.mark2());
      hipLaunchKernelGGL(colpart_reduce_kernel, dim3((mpad + 255) / 256, len), dim3(256), 0, st,
                         (const double*)z.colsq, tmr, mpad, d_v() + (size_t)a * mpad);
      return 0;
    }
    HIPCHK(c, launch_gemm<T>(st, g, false, true, len));
    if (last) HIPCHK(c, tm.mark2());  // (several runs: the first launch to the last, with what lies between)
    hipLaunchKernelGGL((colsum_prod_kernel<T>), dim3(mpad / 64, len), dim3(256), 0, st, (const T*)(lch ? Va : Ksa), sKs,
                       (const T*)Va, sKs, mpad, npad, mpad, d_v() + (size_t)a * mpad);
    if (grad) {
      // Q = W^T V (L_chol: the upper triangular A operand W^T, k from the tile row's diagonal block on) | G as it is
      const T* Qs = Va;
      if (lch) {
        T* const Qa = z.Q + (size_t)a * sKs;
        HIPCHK(c, launch_gemm<T>(st, wt_product_args(g, Va, Qa), true, true, len));
        Qs = Qa;
      }
      if (r.rhs == RhsRequest::QUAD_Z) {
        if (last) HIPCHK(c, tm.mark2());  // (quad_grad: with Q)
        hipLaunchKernelGGL((quad_grad_tile_kernel<T, true>), dim3(mpad / CT, npad / CT, len), dim3(256), 0, st,
                           (const double*)c->dX.as<double>(), D, (const double*)zs.mut,
                           (const double*)(z.qcon + (size_t)a * (D + 1) * mpad), alpha(s0 + a), npad, Qs, sKs,
                           k.spb + (size_t)a * SP_STRIDE, lch ? 1 : 0, N, M, mpad,
                           z.gpart + (size_t)a * gnt * gpl * D * mpad);
      } else {
        GPC_COV_DISPATCH(cross_grad_tile_kernel, T, po->cd, dim3(mpad / CT, npad / CT, len), dim3(256), 0, st, po->cd,
                         k.xsb + (size_t)a * npad * D, (const double*)(z.xss + (size_t)a * mpad * D),
                         k.spb + (size_t)a * SP_STRIDE, alpha(s0 + a), npad, Qs, sKs, lch ? 1 : 0, N, npad, M, mpad,
                         z.gpart + (size_t)a * gnt * 2 * D * mpad);
      }
    }
    if (full) {
      // Kss -= V^T V / sl  (per sample: alpha differs)   |   Kss += R^T G
      for (int i = a; i < a + len; ++i) {
        GemmArgs f;
        f.A = lch ? (const void*)(V() + (size_t)i * sKs) : (const void*)(Ks() + (size_t)i * sKs);
        f.B = V() + (size_t)i * sKs;
        f.C = z.Kss + (size_t)i * sKss;
        f.sA = f.sB = f.sC = 0;
        f.lda = f.ldb = f.ldc = mpad;
        f.M = f.N = mpad, f.K = npad;
        f.alpha = lch ? -1.0 / po->sp[(size_t)(s0 + i) * SP_STRIDE + SP_SL] : 1.0, f.beta = 1;
        f.klo = KLO_ZERO, f.khi = KHI_FULL, f.lower_only = 0;
        HIPCHK(c, launch_gemm<T>(st, f, true, true, 1));
      }
    }
    return 0;
  }

  // ---- the gradient planes of a chunk: the tile partials reduced and on their way to the host ----
  int reduce_gradients(int s0, int cnt) {
    if (r.qg && !r.want_quad)  // no product: the alpha weights only, the whole chunk in one launch
      hipLaunchKernelGGL((quad_grad_tile_kernel<T, false>), dim3(mpad / CT, npad / CT, cnt), dim3(256), 0, st,
                         (const double*)c->dX.as<double>(), D, (const double*)zs.mut, (const double*)z.qcon, alpha(s0), npad,
                         (const T*)nullptr, 0LL, k.spb, 0, N, M, mpad, z.gpart);
    if (!grad) return 0;
    double* d_dmu = z.gres;
    double* d_ds2 = d_dmu + (size_t)chunk * mpad * D;
    if (r.qg)
      hipLaunchKernelGGL(quad_grad_reduce_kernel, dim3((mpad + 255) / 256, gpl * D, cnt), dim3(256), 0, st,
                         (const double*)z.gpart, gnt, D, gpl, M, mpad, (const double*)zs.xb,
                         (const double*)z.qcon, d_dmu, (size_t)chunk * mpad * D);
    else
      hipLaunchKernelGGL(grad_reduce_kernel, dim3((mpad + 255) / 256, cnt), dim3(256), 0, st,
                         (const double*)z.gpart, gnt, D, mpad, k.mulb, k.divb, d_dmu, d_ds2);
    HIPCHK(c, hipMemcpyAsync(hgrad, d_dmu, (size_t)gpl * chunk * mpad * D * 8, hipMemcpyDeviceToHost, st));
    return 0;
  }

  // ---- lin and quad to the host (`poll`: through the gathered download launch, which carries the completion word),
  // then the draws or the full covariances ----
  int download(int s0, int cnt, bool poll) {
    const bool want_quad = r.want_quad;
    if (poll) {
      const size_t out_bytes = (want_quad ? 2 : 1) * (size_t)chunk * mpad * 8;
      HIPCHK(c, c->pin.gather(hmu, d_mu(), want_quad ? out_bytes : (size_t)cnt * mpad * 8, st));
    } else if (want_quad && cnt == chunk)  // d_v = d_mu + chunk * mpad: one contiguous block
      HIPCHK(c, hipMemcpyAsync(hmu, d_mu(), 2 * (size_t)chunk * mpad * 8, hipMemcpyDeviceToHost, st));
    else {
      HIPCHK(c, hipMemcpyAsync(hmu, d_mu(), (size_t)cnt * mpad * 8, hipMemcpyDeviceToHost, st));
      if (want_quad) HIPCHK(c, hipMemcpyAsync(hv, d_v(), (size_t)cnt * mpad * 8, hipMemcpyDeviceToHost, st));
    }
    if (r.draw) return draw_chunk<T>(po, *r.draw, s0, cnt, M, z, r.draw->nsd ? zs.nsd : nullptr, hdraw);
    if (full) {
      for (int i = 0; i < cnt; ++i) {
        dim3 gn((M + 63) / 64, (M + 3) / 4), blk(64, 4);
        hipLaunchKernelGGL((extract_kernel<T>), gn, blk, 0, st, (const T*)(z.Kss + (size_t)i * sKss),
                           mpad, M, 2, zs.fullout);
        double* dst = r.full + (size_t)(s0 + i) * M * M;
        HIPCHK(c, hipMemcpyAsync(hfull ? hfull : dst, zs.fullout, (size_t)M * M * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (hfull) memcpy(dst, hfull, (size_t)M * M * 8);
      }
    }
    return 0;
  }

  // ---- the end of a chunk on the host: on the polled word of the download launch when there is one (bounded: after
  // 2 ms the stream is waited for after all), else on the stream ----
  int wait(bool poll) {
    bool seen = false;
    if (poll && !c->pin.down_plain) {
      unsigned long long* flag = reinterpret_cast<unsigned long long*>(c->land_blk + (gpc_ctx::LAND_BYTES / 8 - 1));
      const unsigned long long seq = ++c->land_seq;
      HIPCHK(c, c->pin.flush_down(st, flag, seq, nullptr));
      seen = poll_word(flag, seq, 2000.0);
    } else if (poll) {
      HIPCHK(c, c->pin.flush_down(st));
    }
    if (seen) {
      ++c->small_polled;
    } else {
      HIPCHK(c, hipStreamSynchronize(st));
      if (poll) ++c->small_synced;
    }
    c->pin.finish();
    return 0;
  }

  // ---- a chunk's results into the caller's layout: [j*S + s], f[(j*R + r)*S + s], [(j*D + l)*S + s] ----
  void scatter(int s0, int cnt) {
    scatter_plane(r.lin, hmu, M, mpad, S, s0, cnt);
    if (r.want_quad) scatter_plane(r.quad, hv, M, mpad, S, s0, cnt);
    if (r.draw) scatter_plane(r.draw->f, hdraw, (size_t)M * r.draw->R, (size_t)M * r.draw->R, S, s0, cnt);
    if (grad) {
      double* outs[4] = {r.dlin, r.dquad, nullptr, nullptr};
      if (r.qg) std::copy_n(r.qg->p, 4, outs);
      const size_t ss = (size_t)mpad * D;
      for (int p = 0; p < gpl; ++p) scatter_plane(outs[p], hgrad + (size_t)p * chunk * ss, (size_t)M * D, ss, S, s0, cnt);
    }
  }

  int chunk_steps(int s0, int cnt) {
    HIPCHK(c, tm.start());
    if (int rc = k.stage(s0, cnt, r.rhs == RhsRequest::CROSS)) return rc;
    if (int rc = r.rhs == RhsRequest::CROSS      ? build_cross(s0, cnt)
                 : r.rhs == RhsRequest::GIVEN_KS ? build_given(s0, cnt)
                 : r.rhs == RhsRequest::GOBS     ? build_gobs(s0, cnt)
                                                 : build_quad_z(s0, cnt))
      return rc;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, tm.mark1());
    HIPCHK(c, tm.mark2());
    if (r.want_quad || full)
      if (int rc = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) { return run_products(s0, cnt, a, len, lch); }))
        return rc;
    if (int rc = reduce_gradients(s0, cnt)) return rc;
    HIPCHK(c, hipGetLastError());
    const size_t out_bytes = (r.want_quad ? 2 : 1) * (size_t)chunk * mpad * 8;
    const bool poll = !tm.on && !full && !grad && c->small_poll && c->land_blk && cnt == chunk && out_bytes <= PinBuf::kGather / 8;
    if (int rc = download(s0, cnt, poll)) return rc;
    HIPCHK(c, tm.stop());
    if (int rc = wait(poll)) return rc;
    tm.accumulate();
    scatter(s0, cnt);
    return 0;
  }
};

template <typename T>
int rhs_products(gpc_post* po, const RhsRequest& r) {
  RhsCall<T> call(po, r);
  if (int rc = call.plan()) return rc;
  if (int rc = call.begin()) return rc;
  // gpc_last_timing after a predict / predict_full / quad call: device time of the call (first upload to last result
  // ready) and of its N^2 M products V = W Ks (the launches of gemm.h), summed over the chunks
  po->ctx->ms_total = po->ctx->ms_factor = 0;
  for (int s0 = 0; s0 < po->S; s0 += call.chunk)
    if (int rc = call.chunk_steps(s0, std::min(call.chunk, po->S - s0))) return rc;
  return 0;
}
int rhs_products(gpc_post* po, const RhsRequest& r) {
  return po->dtype == GPC_F64 ? rhs_products<double>(po, r) : rhs_products<float>(po, r);
}
// gpc_quad, gpc_quad_grad, gpc_quad_cov: z . alpha and, with want_var, z (K + Sigma)^-1 z of the measures N(mu_j, sigma_j^2)
RhsRequest quad_request(const double* mu, const double* sigma, int M, bool want_var, double* zalpha, double* zKz) {
  RhsRequest r;
  r.rhs = RhsRequest::QUAD_Z;
  r.xa = mu;
  r.xb = sigma;
  r.M = M;
  r.want_quad = want_var;
  r.lin = zalpha;
  r.quad = zKz;
  return r;
}

template <typename T>
int predict_impl(gpc_post* po, const double* xstar, int M, double* fmu, double* fs2, double* dfmu = nullptr,
                 double* dfs2 = nullptr, RhsRequest::Rhs rhs = RhsRequest::CROSS) {
  // (with dfmu: the gradients come back complete -- kss is constant for stationary kernels, and the 1/sl of the
  // L_chol samples is applied to Q on the device)
  RhsRequest r;
  r.rhs = rhs;
  r.xa = xstar;
  r.M = M;
  r.want_quad = true;
  r.lin = fmu;
  r.quad = fs2;
  r.dlin = dfmu;
  r.dquad = dfs2;
  int rc = rhs_products<T>(po, r);
  if (rc) return rc;
  const int S = po->S;
  for (int s = 0; s < S; ++s) {
    const double sf2 = po->sp[(size_t)s * SP_STRIDE + SP_SF2];
    const double sl = po->sp[(size_t)s * SP_STRIDE + SP_SL];
    for (int j = 0; j < M; ++j) {
      const double q = fs2[(size_t)j * S + s];
      // L_chol: kss - sum(V*V), V = sW * (W Ks), sW^2 = 1/sl   (:1752-1760)
      // else  : kss + sum(Ks * (L Ks))                          (:1762-1764)
      fs2[(size_t)j * S + s] = po->lchol[s] ? sf2 - q / sl : sf2 + q;
    }
  }
  return 0;
}

// gpc_predict_cov: the posterior covariance between two query sets, rhs_products' sibling.  Per sample
//   Ks_a = K(X, xa) (npad x mapad), Ks_b = K(X, xb) (npad x mbpad), K_ab = K(xa, xb) (mapad x mbpad, zero padding)
//   L_chol:    V_a = W Ks_a, V_b = W Ks_b,  C = K_ab - V_a^T V_b / sl,   fs2b_j = sf2 - |V_b[:, j]|^2 / sl
//   low noise: G_b = L Ks_b,                C = K_ab + Ks_a^T G_b,       fs2b_j = sf2 + Ks_b[:, j] . G_b[:, j]
//   wsq_j = sum_i w_i C_ij^2
// Runs of equal L_chol share the triangular products' launches.  The cross product is a rectangular launch with both
// operands k-major.  Two forms, chosen by the shape ALONE (never by the number of samples: a sample of a batch carries
// the bits of its single evaluation):
//   stored  C is written (one beta = 1 launch per sample, as predict_full's) and, for wsq, reduced by wsq_col_kernel;
//   fused   (no covariance wanted and at least 64 128-tiles) C is never written: the product's epilogue reads K_ab and
//           forms the weighted column sums of squares per tile row (gemm.h: EPI = 2), colpart_reduce_kernel adds the
//           tile rows in ascending order.  No atomics.
// Scratch: CovScratch per sample and CovShared once per call, carved from a block of the call's own (c->covs:
// gpc_lookahead_batch runs this while its resident state is live), chunked over the samples under the same budget as
// rhs_products.

template <typename T>
int cov_products(gpc_post* po, const double* xa, int Ma, const double* xb, int Mb, const double* w, int w_per_sample,
                 double* fs2b, double* cov, double* wsq, double* keep = nullptr) {
  gpc_ctx* c = po->ctx;
  const int S = po->S, N = po->N, D = po->D, npad = po->npad;
  const int mapad = pad_tile(Ma), mbpad = pad_tile(Mb);
  hipStream_t st = c->st;
  const long long sKa = (long long)npad * mapad, sKb = (long long)npad * mbpad, sC = (long long)mapad * mbpad;
  const int tma = mapad / TILE;
  const bool fused = cov_fused_form(mapad, mbpad, wsq != nullptr, cov != nullptr);
  const size_t per = ScratchCarver::count<CovScratch<T>>(1, npad, mapad, mbpad, D, fused);
  const size_t shared = ScratchCarver::count<CovShared>(Ma, Mb, D, cov != nullptr), held = c->covs.bytes;
  const int chunk = plan_chunk(c, S, per, shared, held, shared + (size_t)S * per <= held, 0, false, [&](size_t budget) {
    return "gpc_predict_cov: the scratch of one sample (" + std::to_string(per >> 10) + " KB: N_pad = " +
           std::to_string(npad) + ", Ma_pad = " + std::to_string(mapad) + ", Mb_pad = " + std::to_string(mbpad) +
           ") exceeds the device memory budget (" + std::to_string(budget >> 10) + " KB)";
  });
  if (!chunk) return -2;
  HIPCHK(c, c->covs.ensure(shared + (size_t)chunk * per));
  CovScratch<T> z;  // (carved once, for the planned chunk: its size is the stride of [v | q] and of the weights)
  CovShared zs;
  CARVECHK(c, "gpc_predict_cov", ScratchCarver::carve(z, c->covs.p, chunk, npad, mapad, mbpad, D, fused) +
                                     ScratchCarver::carve(zs, c->covs.as<char>() + (size_t)chunk * per, Ma, Mb, D, cov != nullptr));
  double *const xsa = z.xsa, *const xsbq = z.xsbq, *const d_xa = zs.xa, *const d_xb = zs.xb;
  double *const d_w = z.w, *const d_al = d_w + (size_t)chunk * mapad;
  double *const d_v = z.vq, *const d_q = d_v + (size_t)chunk * mbpad;
  c->pin.begin();
  c->pin.begin_gather();
  CallTimer tm{c, CallTimer::wanted(c, npad)};
  HIPCHK(c, c->pin.up(d_xa, xa, (size_t)Ma * D * 8, st));
  HIPCHK(c, c->pin.up(d_xb, xb, (size_t)Mb * D * 8, st));
  std::vector<double> hw((size_t)chunk * (mapad + 1)), hout(2 * (size_t)chunk * mbpad);
  double* hcov = nullptr;
  if (cov && (size_t)Ma * Mb * 8 >= PinBuf::kMin && (size_t)Ma * Mb * 8 <= PinBuf::kMax)
    hcov = static_cast<double*>(c->pin.alloc((size_t)Ma * Mb * 8));

  ChunkConsts k;
  if (int rc = k.init(po, chunk)) return rc;
  const double *spb = k.spb, *mulb = k.mulb, *divb = k.divb, *xsb = k.xsb;

  // gpc_last_timing: device time of the call and of its products (the first triangular product to the cross product)
  c->ms_total = c->ms_factor = 0;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    HIPCHK(c, tm.start());
    if (int rc = k.stage(s0, cnt, true)) return rc;
    // the weights of the chunk's samples (zero in the padding) and the factor of each sample's cross product
    std::fill(hw.begin(), hw.end(), 0.0);
    for (int i = 0; i < cnt; ++i) {
      if (w)
        for (int r = 0; r < Ma; ++r) hw[(size_t)i * mapad + r] = w_per_sample ? w[(size_t)r * S + s0 + i] : w[r];
      hw[(size_t)chunk * mapad + i] = po->lchol[s0 + i] ? -1.0 / po->sp[(size_t)(s0 + i) * SP_STRIDE + SP_SL] : 1.0;
    }
    HIPCHK(c, hipMemcpyAsync(d_w, hw.data(), hw.size() * 8, hipMemcpyHostToDevice, st));
    T *const Ksa = z.Ksa, *const Ksb = z.Ksb, *const Va = z.Va, *const Vb = z.Vb, *const Kab = z.Kab;
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)mapad * D + 255) / 256), cnt), dim3(256), 0, st,
                       (const double*)d_xa, Ma, mapad, D, mulb, divb, xsa);
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)mbpad * D + 255) / 256), cnt), dim3(256), 0, st,
                       (const double*)d_xb, Mb, mbpad, D, mulb, divb, xsbq);
    // (the builder's fused mean product lands in z.part and is not used: the covariance does not involve alpha)
    const double* al = po->alpha.as<double>() + (size_t)s0 * npad;
    GPC_COV_DISPATCH(cross_tile_kernel, T, po->cd, dim3(mapad / CT, npad / CT, cnt), dim3(256), 0, st, po->cd, xsb,
                     (const double*)xsa, spb, al, npad, N, npad, Ma, mapad, Ksa, sKa, z.part);
    GPC_COV_DISPATCH(cross_tile_kernel, T, po->cd, dim3(mbpad / CT, npad / CT, cnt), dim3(256), 0, st, po->cd, xsb,
                     (const double*)xsbq, spb, al, npad, N, npad, Mb, mbpad, Ksb, sKb, z.part);
    hipLaunchKernelGGL((cross_kernel<T>), dim3(mbpad / 64, mapad / 4, cnt), dim3(64, 4), 0, st, po->cd,
                       (const double*)xsa, (const double*)xsbq, spb, Ma, mapad, Mb, mbpad, Kab, sC);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, tm.mark1());
    const int rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
      // V_b = W Ks_b (and V_a = W Ks_a) | G_b = L Ks_b: the samples of the run in one launch each
      HIPCHK(c, launch_gemm<T>(st, tri_product_args<T>(po, s0 + a, lch, Ksb + (size_t)a * sKb, Vb + (size_t)a * sKb, sKb, mbpad, mbpad),
                               false, true, len));
      if (lch)
        HIPCHK(c, launch_gemm<T>(st, tri_product_args<T>(po, s0 + a, lch, Ksa + (size_t)a * sKa, Va + (size_t)a * sKa, sKa, mapad, mapad),
                                 false, true, len));
      if (fs2b) {
        const T* left = lch ? (const T*)(Vb + (size_t)a * sKb) : (const T*)(Ksb + (size_t)a * sKb);
        hipLaunchKernelGGL((colsum_prod_kernel<T>), dim3(mbpad / 64, len), dim3(256), 0, st, left, sKb,
                           (const T*)(Vb + (size_t)a * sKb), sKb, mbpad, npad, mbpad, d_v + (size_t)a * mbpad);
      }
      // the cross product C = K_ab + alpha A^T B, A = V_a | Ks_a, B = V_b | G_b
      const T* Aop = lch ? Va : Ksa;
      GemmArgs f;
      f.lda = mapad;
      f.ldb = f.ldc = mbpad;
      f.M = mapad;
      f.N = mbpad;
      f.K = npad;
      f.beta = 1;
      f.klo = KLO_ZERO;
      f.khi = KHI_FULL;
      f.lower_only = 0;
      if (fused) {
        f.A = Aop + (size_t)a * sKa;
        f.B = Vb + (size_t)a * sKb;
        f.C = Kab + (size_t)a * sC;
        f.sA = sKa;
        f.sB = sKb;
        f.sC = sC;
        f.alpha = 0.0;  // (per sample: ep_alpha)
        f.ep_alpha = d_al + a;
        f.ep_w = d_w + (size_t)a * mapad;
        f.ep_sw = mapad;
        f.colsq = z.wpart + (size_t)a * tma * mbpad;
        HIPCHK(c, launch_gemm_wsq<T>(st, f, len));
        hipLaunchKernelGGL(colpart_reduce_kernel, dim3((mbpad + 255) / 256, len), dim3(256), 0, st,
                           (const double*)f.colsq, tma, mbpad, d_q + (size_t)a * mbpad);
      } else {
        for (int i = a; i < a + len; ++i) {  // (per sample: alpha differs)
          f.A = Aop + (size_t)i * sKa;
          f.B = Vb + (size_t)i * sKb;
          f.C = Kab + (size_t)i * sC;
          f.sA = f.sB = f.sC = 0;
          f.alpha = hw[(size_t)chunk * mapad + i];
          HIPCHK(c, launch_gemm<T>(st, f, true, true, 1));
        }
        if (wsq)
          hipLaunchKernelGGL((wsq_col_kernel<T>), dim3(mbpad / 64, len), dim3(256), 0, st,
                             (const T*)(Kab + (size_t)a * sC), sC, mbpad, (const double*)(d_w + (size_t)a * mapad), mapad,
                             Ma, mbpad, d_q + (size_t)a * mbpad);
      }
      return 0;
    });
    if (rc_runs) return rc_runs;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, tm.mark2());
    if (keep)  // gpc_lookahead_batch: the stored C of every sample stays on the device, in fp64 (Ma x mbpad each)
      for (int i = 0; i < cnt; ++i)
        hipLaunchKernelGGL((lab_load_kernel<T>), dim3(mbpad / 64, (Ma + 3) / 4), dim3(64, 4), 0, st,
                           (const T*)(Kab + (size_t)i * sC), mbpad, Ma, Mb, keep + (size_t)(s0 + i) * Ma * mbpad);
    HIPCHK(c, hipMemcpyAsync(hout.data(), d_v, 2 * (size_t)chunk * mbpad * 8, hipMemcpyDeviceToHost, st));
    if (cov) {
      for (int i = 0; i < cnt; ++i) {
        hipLaunchKernelGGL((extract_rect_kernel<T>), dim3((Mb + 63) / 64, (Ma + 3) / 4), dim3(64, 4), 0, st,
                           (const T*)(Kab + (size_t)i * sC), mbpad, Ma, Mb, zs.cov);
        double* dst = cov + (size_t)(s0 + i) * Ma * Mb;
        HIPCHK(c, hipMemcpyAsync(hcov ? hcov : dst, zs.cov, (size_t)Ma * Mb * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (hcov) memcpy(dst, hcov, (size_t)Ma * Mb * 8);
      }
    }
    HIPCHK(c, tm.stop());
    HIPCHK(c, hipStreamSynchronize(st));
    c->pin.finish();
    tm.accumulate();
    for (int i = 0; i < cnt; ++i) {
      const int s = s0 + i;
      const double sf2 = po->sp[(size_t)s * SP_STRIDE + SP_SF2], sl = po->sp[(size_t)s * SP_STRIDE + SP_SL];
      for (int j = 0; j < Mb; ++j) {
        if (fs2b) {  // as gpc_predict forms it
          const double q = hout[(size_t)i * mbpad + j];
          fs2b[(size_t)j * S + s] = po->lchol[s] ? sf2 - q / sl : sf2 + q;
        }
        if (wsq) wsq[(size_t)j * S + s] = hout[((size_t)chunk + i) * mbpad + j];
      }
    }
  }
  if (fused) ++c->cov_fused;
  return 0;
}

struct GramClock {  // one timed device section of a call: the Gram passes of "grad_post_gram_us", the step loop below
  hipEvent_t e[2] = {nullptr, nullptr};
  bool on;
  explicit GramClock(bool on_) : on(on_) {
    if (on && (hipEventCreate(&e[0]) != hipSuccess || hipEventCreate(&e[1]) != hipSuccess)) on = false;
  }
  ~GramClock() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  hipError_t record(int i, hipStream_t st) { return on ? hipEventRecord(e[i], st) : hipSuccess; }
  double elapsed_us() {
    float ms = 0;
    if (on) (void)hipEventElapsedTime(&ms, e[0], e[1]);
    return 1e3 * ms;
  }
};

// ---- gpc_lookahead_batch: q greedy look-ahead steps on the device (lookahead_batch.h) ----------------------------------

template <typename T>
int lookahead_batch_impl(gpc_post* po, const double* xr, int Mr, const double* xc, int Mc, const double* w, int w_per_sample,
                         const double* noise, int q, int* idx, double* gain) {
  gpc_ctx* c = po->ctx;
  const int S = po->S, D = po->D, Ma = Mr + Mc, ld = pad_tile(Mc), nslab = (Mr + LB_T - 1) / LB_T, Rl = Mr + ld;
  hipStream_t st = c->st;
  const size_t need = ScratchCarver::count<LabScratch>(S, Mr, Mc, ld, q);
  // the budget of the resident state: what plan_chunk gives a consumer's scratch, for all samples at once
  const bool forced = getenv("GPC_MEM_BUDGET_MB") != nullptr;
  if (forced || need > c->lab.bytes) {
    c->pool_drain();
    const size_t budget = (size_t)((free_device_bytes() + (forced ? 0 : c->lab.bytes)) * 0.8);
    if (need > budget)
      FAIL(c, "gpc_lookahead_batch: the resident state of the step loop (" + std::to_string(need >> 10) + " KB: S = " +
                  std::to_string(S) + ", Mr = " + std::to_string(Mr) + ", Mc_pad = " + std::to_string(ld) + ", q = " +
                  std::to_string(q) + "; S (Mr + Mc) Mc_pad doubles and the l panels, not chunked over the samples) "
                  "exceeds the device memory budget (" + std::to_string(budget >> 10) + " KB)");
  }
  HIPCHK(c, c->lab.ensure(need));
  LabScratch z;
  ScratchCarver::carve(z, c->lab.p, S, Mr, Mc, ld, q);
  // C^0 of [x_ref; x_cand] against x_cand and predict's variance of the candidates: cov_products' stored form, chunked
  // over the samples under its own budget; the covariances stay on the device
  std::vector<double> xa((size_t)Ma * D), fs2((size_t)Mc * S);
  std::copy_n(xr, (size_t)Mr * D, xa.begin());
  std::copy_n(xc, (size_t)Mc * D, xa.begin() + (size_t)Mr * D);
  if (int rc = cov_products<T>(po, xa.data(), Ma, xc, Mc, nullptr, 0, fs2.data(), nullptr, nullptr, z.C)) return rc;
  // per-sample rows of the variances, the noise and the weights (zero in the padding: den = 0 there)
  std::vector<double> hv((size_t)S * ld, 0.0), hn((size_t)S * ld, 0.0), hw((size_t)S * Mr);
  for (int s = 0; s < S; ++s) {
    for (int j = 0; j < Mc; ++j) {
      hv[(size_t)s * ld + j] = fs2[(size_t)j * S + s];
      hn[(size_t)s * ld + j] = noise[(size_t)j * S + s];
    }
    for (int r = 0; r < Mr; ++r) hw[(size_t)s * Mr + r] = w_per_sample ? w[(size_t)r * S + s] : w[r];
  }
  HIPCHK(c, hipMemcpyAsync(z.v, hv.data(), hv.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(z.noise, hn.data(), hn.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(z.w, hw.data(), hw.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(z.lpan, 0, (size_t)S * q * Rl * 8, st));
  HIPCHK(c, hipMemsetAsync(z.chosen, 0, (size_t)ld * sizeof(int), st));
  const long long sC = (long long)Ma * ld, sL = (long long)q * Rl;
  GramClock clk(true);
  HIPCHK(c, clk.record(0, st));
  // all q steps, enqueued without waiting: a step's launches hand c_t and sqrt(den) on through device memory
  for (int t = 0; t < q; ++t) {
    hipLaunchKernelGGL(lab_step_kernel, dim3(ld / LB_T, nslab, S), dim3(256), 0, st, z.C, sC, ld, Mr, (const double*)z.w,
                       t ? (const double*)(z.lpan + (size_t)(t - 1) * Rl) : (const double*)nullptr, sL, z.part, nslab);
    hipLaunchKernelGGL(lab_score_kernel, dim3(ld / LB_T), dim3(256), 0, st, (const double*)z.part, nslab, ld, S,
                       (const double*)z.v, (const double*)z.noise, z.gains, z.score);
    hipLaunchKernelGGL(lab_pick_kernel, dim3(1), dim3(256), 0, st, (const double*)z.score, Mc, ld, S, t,
                       (const double*)z.gains, (const double*)z.v, (const double*)z.noise, z.chosen, z.idx, z.cur, z.sd,
                       z.gain_out);
    if (t + 1 < q)
      hipLaunchKernelGGL(lab_col_kernel, dim3((Ma + 255) / 256, S), dim3(256), 0, st, (const double*)z.C, sC, ld, Mr, Mc,
                         (const int*)z.cur, (const double*)z.sd, z.lpan, sL, Rl, t, z.v);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, clk.record(1, st));
  std::vector<char> ho(z.out_bytes);
  HIPCHK(c, hipMemcpyAsync(ho.data(), z.gain_out, z.out_bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  c->lookahead_batch_loop_us = (unsigned long long)clk.elapsed_us();
  memcpy(gain, ho.data(), (size_t)q * S * 8);
  memcpy(idx, ho.data() + LabScratch::even((size_t)S * q) * 8, (size_t)q * sizeof(int));
  return 0;
}

// gpc_grad_post: the joint posterior of (f, grad f) at every query, rhs_products' sibling (gradpost.h).  The queries are
// worked on in blocks of GQB = 128 whatever the shape or the budget; per block and sample
//   panel = [ k(X, x*) | dk/dx*_1 | ... | dk/dx*_D ]  (npad x (D + 1) 128, slot-major planes; the mean product fused in)
//   L_chol:    V = W panel,   Gram = per query V_j^T V_j,         C_j = H - Gram / sl
//   low noise: Z = L panel,   Gram = per query panel_j^T Z_j,     C_j = H + Gram
// `diag`: the D + 1 variances only -- for L_chol samples the column sums of squares of V from the product's epilogue
// (gemm.h: EPI = 1, V is never written), for the others the diagonal form of the Gram kernel.  The forms depend on
// (npad, D, diag) alone, so a sample carries the same bits in any batch, chunk or run.  The budget decides the samples
// per chunk only; a sample with one query block that does not fit is refused.
// gpc_last_timing: the device sections of all (chunk, block) steps and, of these, the products with W (or L).
// gpc_grad_post_gobs (a posterior with gradient observations: po->gobs.Ng > 0) differs by the operand builder alone: the
// scaled point list (launch_gobs_scale) and gradobs.h's gobs_grad_operand_tile_kernel, whose partials have one row per
// 64-tile of the LIST; the panel is npad x (D + 1) 128 with npad = pad128(N + Ng D), and everything after it is the same
// code.  "gobs_grad_operand_us": the operand builds (scaling, kernel, reduction) of a timed call.

template <typename T>
int grad_post_impl(gpc_post* po, const double* xstar, int M, bool diag, double* fmu, double* dfmu, double* cov) {
  gpc_ctx* c = po->ctx;
  const int S = po->S, N = po->N, D = po->D, npad = po->npad, Dp = D + 1, mb = GQB, ld = Dp * mb;
  const bool gobs = po->gobs.Ng > 0;
  const std::string fn = gobs ? "gpc_grad_post_gobs" : "gpc_grad_post";
  hipStream_t st = c->st;
  const long long sP = (long long)npad * ld;
  const int nt64 = gobs ? po->gobs.P() / CT : npad / CT, tmr = npad / TILE, nseg = gram_segments(npad);
  const size_t gper = (size_t)mb * Dp * (diag ? 1 : Dp);  // doubles of a sample's Gram result
  const size_t per = ScratchCarver::count<BlockScratch<T>>(1, npad, D, true, false, diag ? 1 : D + 1, diag, (size_t)0, nt64), shared = (size_t)M * D * 8;
  const size_t held = c->cs.bytes;
  const int chunk = plan_chunk(c, S, per, shared, held, shared + (size_t)S * per <= held, 0, false, [&](size_t budget) {
    return fn + ": the scratch of one sample with one query block (" + std::to_string(per) + " bytes: N_pad = " +
           std::to_string(npad) + ", D = " + std::to_string(D) + ", block = " + std::to_string(mb) +
           " queries) exceeds the device memory budget (" + std::to_string(budget) + " bytes)";
  });
  if (!chunk) return -2;
  HIPCHK(c, c->cs.ensure(shared + (size_t)chunk * per));
  BlockScratch<T> z;
  CARVECHK(c, fn.c_str(), ScratchCarver::carve(z, c->cs.p, chunk, npad, D, true, false, diag ? 1 : D + 1, diag, (size_t)0, nt64));
  T *const P = z.P, *const V = z.V;
  double *const xsq = z.xsq, *const d_mean = z.mean, *const d_gram = z.gram, *const d_f0 = z.f0;
  double* const d_xa = reinterpret_cast<double*>(c->cs.as<char>() + (size_t)chunk * per);  // shared: the raw queries
  c->pin.begin();
  c->pin.begin_gather();
  CallTimer tm{c, CallTimer::wanted(c, npad)};
  GramClock gc(tm.on), oc(gobs && tm.on);
  HIPCHK(c, c->pin.up(d_xa, xstar, (size_t)M * D * 8, st));
  std::vector<double> hmean((size_t)chunk * ld), hgram((size_t)chunk * gper), hf0(chunk);
  ChunkConsts k;
  if (int rc = k.init(po, chunk)) return rc;
  c->ms_total = c->ms_factor = 0;
  double gram_us = 0, operand_us = 0;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    if (int rc = k.stage(s0, cnt, !gobs)) return rc;
    const double* xp = k.xsb;  // (gobs, all samples in one chunk: the posterior's resident scaled lists)
    if (gobs && !k.resident) {
      HIPCHK(c, c->gxs.ensure((size_t)cnt * po->gobs.P() * D * 8));
      launch_gobs_scale(st, po->gobs, po->gpts.as<double>(), k.mulb, k.divb, cnt, c->gxs.as<double>());
      xp = c->gxs.as<double>();
    }
    for (int q0 = 0; q0 < M; q0 += mb) {
      const int mq = std::min(mb, M - q0);
      HIPCHK(c, tm.start());
      HIPCHK(c, oc.record(0, st));
      hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)mb * D + 255) / 256), cnt), dim3(256), 0, st,
                         (const double*)(d_xa + (size_t)q0 * D), mq, mb, D, k.mulb, k.divb, xsq);
      if (gobs) {
        HIPCHK(c, launch_gobs_grad_operand<T>(st, po->cd, po->gobs, xp, xsq, k.spb, k.mulb, k.divb,
                                              po->alpha.as<double>() + (size_t)s0 * npad, npad, npad, mq, cnt, P, sP,
                                              z.part, d_mean, d_f0));
      } else {
        GPC_COV_DISPATCH(grad_operand_tile_kernel, T, po->cd, dim3(mb / CT, npad / CT, cnt), dim3(256), 0, st, po->cd, k.xsb,
                         (const double*)xsq, k.spb, k.mulb, k.divb, po->alpha.as<double>() + (size_t)s0 * npad, npad, N, npad,
                         mq, mb, P, sP, z.part, d_f0);
        hipLaunchKernelGGL(colpart_reduce_kernel, dim3((ld + 255) / 256, cnt), dim3(256), 0, st,
                           (const double*)z.part, nt64, ld, d_mean);
      }
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, oc.record(1, st));
      HIPCHK(c, tm.mark1());
      // the products of every run of equal L_chol, then (second pass) what reduces them
      int rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
        GemmArgs g = tri_product_args<T>(po, s0 + a, lch, P + (size_t)a * sP, V + (size_t)a * sP, sP, ld, ld);
        if (diag && lch) {
          int* qctr = c->tile_ctr.as<int>() + (size_t)gpc_ctx::MAXG * gpc_ctx::CTR_PER_GROUP;
          HIPCHK(c, hipMemsetAsync(qctr, 0, CTR_STRIDE * sizeof(int), st));
          g.colsq = z.colsq + (size_t)a * tmr * ld;
          HIPCHK(c, launch_gemm_colsq<T>(st, g, len, qctr));
        } else {
          HIPCHK(c, launch_gemm<T>(st, g, false, true, len));
        }
        return 0;
      });
      if (rc_runs) return rc_runs;
      HIPCHK(c, tm.mark2());
      HIPCHK(c, gc.record(0, st));
      rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
        if (diag && lch)  // [b][a * mb + j]: the panel's own column order
          hipLaunchKernelGGL(colpart_reduce_kernel, dim3((ld + 255) / 256, len), dim3(256), 0, st,
                             (const double*)(z.colsq + (size_t)a * tmr * ld), tmr, ld, d_gram + (size_t)a * gper);
        else
          HIPCHK(c, launch_block_gram<T>(st, (lch ? V : P) + (size_t)a * sP, V + (size_t)a * sP, sP, npad, mb, Dp, len, diag,
                                         nseg > 1 ? z.gpart + (size_t)a * nseg * gper : nullptr,
                                         d_gram + (size_t)a * gper));
        return 0;
      });
      if (rc_runs) return rc_runs;
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, gc.record(1, st));
      HIPCHK(c, hipMemcpyAsync(hmean.data(), d_mean, (size_t)cnt * ld * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipMemcpyAsync(hgram.data(), d_gram, (size_t)cnt * gper * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipMemcpyAsync(hf0.data(), d_f0, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, tm.stop());
      HIPCHK(c, hipStreamSynchronize(st));
      tm.accumulate();
      gram_us += gc.elapsed_us();
      operand_us += oc.elapsed_us();
      // into the caller's layout: C = H - Gram / sl | H + Gram, H = diag(sf2, F0 c_1^2, ..., F0 c_D^2)
      for (int i = 0; i < cnt; ++i) {
        const int s = s0 + i;
        const bool lch = po->lchol[s] != 0;
        const double gs = lch ? -1.0 / po->sp[(size_t)s * SP_STRIDE + SP_SL] : 1.0;
        std::vector<double> H(Dp);
        H[0] = po->sp[(size_t)s * SP_STRIDE + SP_SF2];
        for (int l = 0; l < D; ++l) {
          const double cl = po->mul[(size_t)s * D + l] / po->dv[(size_t)s * D + l];
          H[1 + l] = hf0[i] * cl * cl;
        }
        const double* mean = &hmean[(size_t)i * ld];
        const double* gram = &hgram[(size_t)i * gper];
        for (int jj = 0; jj < mq; ++jj) {
          const size_t j = (size_t)q0 + jj;
          fmu[j * S + s] = mean[jj];
          for (int l = 0; l < D; ++l) dfmu[(j * D + l) * S + s] = mean[(size_t)(1 + l) * mb + jj];
          if (diag) {
            for (int a = 0; a < Dp; ++a)
              cov[(j * Dp + a) * S + s] = H[a] + gs * (lch ? gram[(size_t)a * mb + jj] : gram[(size_t)jj * Dp + a]);
          } else {
            for (int a = 0; a < Dp; ++a)
              for (int b = 0; b < Dp; ++b)
                cov[((j * Dp + a) * Dp + b) * S + s] = (a == b ? H[a] : 0.0) + gs * gram[((size_t)jj * Dp + a) * Dp + b];
          }
        }
      }
    }
  }
  c->pin.finish();
  c->grad_post_gram_us = (unsigned long long)gram_us;
  if (gobs) c->gobs_grad_operand_us = (unsigned long long)operand_us;
  return 0;
}

// gpc_predict_hess: the Hessians of the predictive mean and variance with respect to x*, gpc_grad_post's sibling
// (hess.h).  Per block of GQB = 128 queries and sample, with the variance:
//   panel = [ k | dk/dx*_1 .. dk/dx*_D ]  (grad_operand_tile_kernel; (fmu, dfmu) = panel^T alpha fused in)
//   L_chol:    V = W panel, Gram = V_j^T V_j,      Q = W^T V[slot 0] / sl     fs2 = sf2 - Gram_00 / sl
//   low noise: Z = L panel, Gram = panel_j^T Z_j,  Q = -Z[slot 0]             fs2 = sf2 + Gram_00
//   dfs2_a = 2 gs Gram_0a,  P_ab = -gs Gram_ab  (gs = -1 / sl | 1),  the contraction with the weights (alpha | Q)
//   Hmu = c c^T o (S_G[alpha] - I S_F[alpha]),   Hs2 = -2 (P + c c^T o (S_G[Q] - I S_F[Q]))
// Without the variance no product is launched: the operand kernel (for fmu, dfmu: the same bits as with it) and the
// contraction with the weights alpha alone.  Every form depends on (npad, D, compute_var) alone.
template <typename T>
int hess_impl(gpc_post* po, const double* xstar, int M, bool var, double* fmu, double* fs2, double* dfmu, double* dfs2,
              double* hmu, double* hs2) {
  gpc_ctx* c = po->ctx;
  const int S = po->S, N = po->N, D = po->D, npad = po->npad, Dp = D + 1, mb = GQB, ld = Dp * mb;
  hipStream_t st = c->st;
  const long long sP = (long long)npad * ld, sQ = (long long)npad * mb;
  const int nt64 = npad / CT, nseg = gram_segments(npad);
  const int npl = hess_planes(D), nset = var ? 2 : 1;
  const size_t gper = var ? (size_t)mb * Dp * Dp : 0;   // doubles of a sample's Gram result
  const size_t hper = (size_t)nset * npl * mb;          // ... of its reduced Hessian sums
  const size_t per = ScratchCarver::count<BlockScratch<T>>(1, npad, D, var, var, var ? Dp : 0, false, hper);
  const size_t shared = (size_t)M * D * 8, held = c->cs.bytes;
  const int chunk = plan_chunk(c, S, per, shared, held, shared + (size_t)S * per <= held, 0, false, [&](size_t budget) {
    return "gpc_predict_hess: the scratch of one sample with one query block (" + std::to_string(per) +
           " bytes: N_pad = " + std::to_string(npad) + ", D = " + std::to_string(D) + ", block = " + std::to_string(mb) +
           " queries) exceeds the device memory budget (" + std::to_string(budget) + " bytes)";
  });
  if (!chunk) return -2;
  HIPCHK(c, c->cs.ensure(shared + (size_t)chunk * per));
  BlockScratch<T> z;
  CARVECHK(c, "gpc_predict_hess", ScratchCarver::carve(z, c->cs.p, chunk, npad, D, var, var, var ? Dp : 0, false, hper));
  T *const P = z.P, *const V = z.V, *const Q = z.Q;
  double *const xsq = z.xsq, *const d_mean = z.mean, *const d_gram = z.gram, *const d_hpart = z.hpart, *const d_hsum = z.hsum;
  double* const d_xa = reinterpret_cast<double*>(c->cs.as<char>() + (size_t)chunk * per);  // shared: the raw queries
  c->pin.begin();
  c->pin.begin_gather();
  CallTimer tm{c, CallTimer::wanted(c, npad)};
  GramClock hc(tm.on);  // the contraction passes, for the "hess_contract_us" counter
  double contract_us = 0;
  HIPCHK(c, c->pin.up(d_xa, xstar, (size_t)M * D * 8, st));
  std::vector<double> hmean((size_t)chunk * ld), hgram((size_t)chunk * gper), hsum((size_t)chunk * hper), cs(D),
      Ha((size_t)D * D), Hq((size_t)D * D);
  ChunkConsts k;
  if (int rc = k.init(po, chunk)) return rc;
  c->ms_total = c->ms_factor = 0;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    if (int rc = k.stage(s0, cnt, true)) return rc;
    for (int q0 = 0; q0 < M; q0 += mb) {
      const int mq = std::min(mb, M - q0);
      const double* alpha = po->alpha.as<double>() + (size_t)s0 * npad;
      HIPCHK(c, tm.start());
      hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)mb * D + 255) / 256), cnt), dim3(256), 0, st,
                         (const double*)(d_xa + (size_t)q0 * D), mq, mb, D, k.mulb, k.divb, xsq);
      GPC_COV_DISPATCH(grad_operand_tile_kernel, T, po->cd, dim3(mb / CT, npad / CT, cnt), dim3(256), 0, st, po->cd, k.xsb,
                       (const double*)xsq, k.spb, k.mulb, k.divb, alpha, npad, N, npad, mq, mb, P, sP,
                       z.part, z.f0);
      hipLaunchKernelGGL(colpart_reduce_kernel, dim3((ld + 255) / 256, cnt), dim3(256), 0, st,
                         (const double*)z.part, nt64, ld, d_mean);
      HIPCHK(c, hipGetLastError());
      if (var) {
        HIPCHK(c, tm.mark1());
        // the products of every run of equal L_chol: V = W panel | Z = L panel, then Q from slot 0 alone
        int rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
          GemmArgs g = tri_product_args<T>(po, s0 + a, lch, P + (size_t)a * sP, V + (size_t)a * sP, sP, ld, ld);
          HIPCHK(c, launch_gemm<T>(st, g, false, true, len));
          if (lch) {  // Q = W^T V[slot 0]: W^T upper triangular, k from the tile row's diagonal block on
            GemmArgs q = wt_product_args(g, V + (size_t)a * sP, Q + (size_t)a * sQ);
            q.sC = sQ;
            q.ldc = mb;
            q.N = mb;
            HIPCHK(c, launch_gemm<T>(st, q, true, true, len));
          }
          return 0;
        });
        if (rc_runs) return rc_runs;
        HIPCHK(c, tm.mark2());
        rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
          HIPCHK(c, launch_block_gram<T>(st, (lch ? V : P) + (size_t)a * sP, V + (size_t)a * sP, sP, npad, mb, Dp, len, false,
                                         nseg > 1 ? z.gpart + (size_t)a * nseg * gper : nullptr,
                                         d_gram + (size_t)a * gper));
          return 0;
        });
        if (rc_runs) return rc_runs;
        HIPCHK(c, hc.record(0, st));
        rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
          GPC_COV_DISPATCH(hess_tile_kernel, T, po->cd, dim3(mb / CT, npad / CT, len), dim3(256), 0, st, po->cd,
                           k.xsb + (size_t)a * npad * D, (const double*)(xsq + (size_t)a * mb * D),
                           k.spb + (size_t)a * SP_STRIDE, alpha + (size_t)a * npad, npad,
                           (const T*)(lch ? Q + (size_t)a * sQ : V + (size_t)a * sP), lch ? sQ : sP, lch ? mb : ld,
                           lch ? 1 : 0, N, npad, mq, mb, d_hpart + (size_t)a * nt64 * hper);
          return 0;
        });
        if (rc_runs) return rc_runs;
      } else {
        HIPCHK(c, hc.record(0, st));
        GPC_COV_DISPATCH(hess_tile_mean_kernel, T, po->cd, dim3(mb / CT, npad / CT, cnt), dim3(256), 0, st, po->cd, k.xsb,
                         (const double*)xsq, k.spb, alpha, npad, N, npad, mq, mb, d_hpart);
      }
      hipLaunchKernelGGL(colpart_reduce_kernel, dim3((unsigned)((hper + 255) / 256), cnt), dim3(256), 0, st,
                         (const double*)d_hpart, nt64, (int)hper, d_hsum);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hc.record(1, st));
      HIPCHK(c, hipMemcpyAsync(hmean.data(), d_mean, (size_t)cnt * ld * 8, hipMemcpyDeviceToHost, st));
      if (var) HIPCHK(c, hipMemcpyAsync(hgram.data(), d_gram, (size_t)cnt * gper * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipMemcpyAsync(hsum.data(), d_hsum, (size_t)cnt * hper * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, tm.stop());
      HIPCHK(c, hipStreamSynchronize(st));
      if (var) tm.accumulate();
      else if (tm.on) {  // no product: the whole device section, nothing in it a product's
        float t03 = 0;
        (void)hipEventElapsedTime(&t03, c->ev[0], c->ev[3]);
        c->ms_total += t03;
      }
      contract_us += hc.elapsed_us();
      // into the caller's layout, once per query: c_a c_b, the delta_ab term, the mirror, the variance's -2 (P + .)
      for (int i = 0; i < cnt; ++i) {
        const int s = s0 + i;
        const bool lch = po->lchol[s] != 0;
        const double gs = lch ? -1.0 / po->sp[(size_t)s * SP_STRIDE + SP_SL] : 1.0;
        const double sf2 = po->sp[(size_t)s * SP_STRIDE + SP_SF2];
        for (int l = 0; l < D; ++l) cs[l] = po->mul[(size_t)s * D + l] / po->dv[(size_t)s * D + l];
        const double* mean = &hmean[(size_t)i * ld];
        const double* gram = var ? &hgram[(size_t)i * gper] : nullptr;
        const double* sums = &hsum[(size_t)i * hper];
        for (int jj = 0; jj < mq; ++jj) {
          const size_t j = (size_t)q0 + jj;
          fmu[j * S + s] = mean[jj];
          for (int l = 0; l < D; ++l) dfmu[(j * D + l) * S + s] = mean[(size_t)(1 + l) * mb + jj];
          hess_assemble(sums, mb, jj, D, cs.data(), Ha.data());
          for (int e = 0; e < D * D; ++e) hmu[(j * D * D + e) * S + s] = Ha[e];
          if (!var) continue;
          const double* gj = gram + (size_t)jj * Dp * Dp;
          fs2[j * S + s] = sf2 + gs * gj[0];
          for (int l = 0; l < D; ++l) dfs2[(j * D + l) * S + s] = 2.0 * gs * gj[(size_t)(1 + l) * Dp];
          hess_assemble(sums + (size_t)npl * mb, mb, jj, D, cs.data(), Hq.data());
          for (int a = 0; a < D; ++a)
            for (int b = 0; b < D; ++b)
              hs2[((j * D + a) * D + b) * S + s] = -2.0 * (-gs * gj[(size_t)(1 + a) * Dp + 1 + b] + Hq[(size_t)a * D + b]);
        }
      }
    }
  }
  c->pin.finish();
  c->hess_contract_us = (unsigned long long)contract_us;
  return 0;
}

// ---- gpc_nll_hess: the Hessian of the negative log marginal likelihood (nll_hess.h) -----------------------------------
// The plane of covariance hyperparameter p: what it differentiates and, for an ARD lengthscale, its dimension
inline void nh_plane_of(const CovDesc& cd, int p, int* mode, int* dim) {
  *dim = 0;
  if (cov_is_iso(cd.kind)) {
    *mode = p == 0 ? NH_LS : NH_SF;
  } else if (p < cd.D) {
    *mode = NH_LS;
    *dim = p;
  } else {
    *mode = p == cd.D ? NH_SF : NH_SHAPE;
  }
}

// One covariance plane of `cnt` samples: the operand into Op, u into X[p], the two sums into gsum[p]
int nh_launch_plane(gpc_ctx* c, const CovDesc& cd, const NhScratch& z, int cnt, int p, const double* xs, const double* sp,
                    const double* alpha, int N) {
  hipStream_t st = c->st;
  const int npad = z.npad;
  const long long n2 = (long long)npad * npad;
  int mode, dim;
  nh_plane_of(cd, p, &mode, &dim);
  GPC_COV_DISPATCH(nh_plane_kernel, double, cd, dim3(z.nt, z.nt, cnt), dim3(256), 0, st, cd, xs, sp, alpha, N, npad, mode, dim,
                   (const double*)z.Q, n2, z.Op, n2, z.upart, z.gpart);
  hipLaunchKernelGGL(colpart_reduce_kernel, dim3((npad + 255) / 256, cnt), dim3(256), 0, st, (const double*)z.upart, z.nt,
                     npad, z.X + (size_t)p * cnt * npad);
  hipLaunchKernelGGL(reduce_parts_kernel, dim3(2, cnt), dim3(256), 0, st, (const double*)z.gpart, z.nt * z.nt, 2,
                     z.gsum + (size_t)p * cnt * 2);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// tr(B_p B_q), p >= q, of `cnt` samples into grsum[b][pair]
int nh_launch_gram(gpc_ctx* c, const NhScratch& z, int cnt) {
  const long long n2 = (long long)z.npad * z.npad;
  hipLaunchKernelGGL(nh_gram_kernel, dim3(z.nt * z.nt, z.ppl, cnt), dim3(256), 0, c->st, (const double*)z.B, n2, z.ppl * n2,
                     z.npad, z.ppl, z.grpart);
  hipLaunchKernelGGL(reduce_parts_kernel, dim3(z.npairs, cnt), dim3(256), 0, c->st, (const double*)z.grpart, z.nt * z.nt,
                     z.npairs, z.grsum);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// sum Qm G d_a^2 d_b^2 of `cnt` samples (ARD families) into d2sum[b][pair]
int nh_launch_d2(gpc_ctx* c, const CovDesc& cd, const NhScratch& z, int cnt, const double* xs, const double* sp,
                 const double* alpha, int N) {
  const long long n2 = (long long)z.npad * z.npad;
  const size_t shm = 4 * (size_t)(((z.nd2 + 3) & ~3) + 4) * sizeof(double);
  GPC_COV_DISPATCH(nh_d2_kernel, double, cd, dim3(z.ntl, cnt), dim3(256), shm, c->st, cd, xs, sp, alpha, N, z.npad,
                   (const double*)z.Q, n2, z.d2part, z.ntl);
  hipLaunchKernelGGL(reduce_parts_kernel, dim3(z.nd2, cnt), dim3(256), 0, c->st, (const double*)z.d2part, z.ntl, z.nd2,
                     z.d2sum);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// <Qm, d2_pq K> for two covariance hyperparameters p >= q from a sample's sums: g[2 p] = <Qm, d_p K>, g[2 p + 1] the
// plane's second sum, sg the ARD contraction (nll_hess.h: the table in the header)
inline double nh_second(const CovDesc& cd, int p, int q, const double* g, int gstride, const double* sg) {
  auto g1 = [&](int h) { return g[(size_t)h * gstride]; };
  auto g2 = [&](int h) { return g[(size_t)h * gstride + 1]; };
  if (cov_is_iso(cd.kind)) {
    if (p == 0) return g2(0) - 2.0 * g1(0);
    return q == 0 ? 2.0 * g1(0) : 2.0 * g1(1);
  }
  const int D = cd.D;
  if (p < D) return sg[p * (p + 1) / 2 + q] - (p == q ? 2.0 * g1(p) : 0.0);
  if (p == D) return q < D ? 2.0 * g1(q) : 2.0 * g1(D);
  if (q < D) return g2(q);             // shape x lengthscale
  return q == D ? 2.0 * g1(D + 1) : g2(D + 1);  // shape x sf | shape x shape
}

// Q = W^T W / sl (L_chol; the lower tiles of the product land in `tiles`, a buffer of cnt n x n matrices that the caller
// overwrites later) | -A of samples s0 .. s0 + cnt - 1, with diag Q.  Shared by gpc_nll_hess and gpc_cv_grad (fp64)
int posterior_q(gpc_post* po, const ChunkConsts& k, int s0, int cnt, double* tiles, double* Q, double* diagq) {
  gpc_ctx* c = po->ctx;
  hipStream_t st = c->st;
  const int N = po->N, npad = po->npad;
  const long long n2 = (long long)npad * npad;
  const double* alpha = po->alpha.as<double>() + (size_t)s0 * npad;
  return for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
    const double* src = po->A.as<double>() + (size_t)(s0 + a) * n2;
    if (lch) {
      Factor<double> F;
      F.st = st;
      F.batch = len;
      F.npad = npad;
      F.A = po->A.as<double>() + (size_t)(s0 + a) * n2;
      F.W = po->W.as<double>() + (size_t)(s0 + a) * n2;
      F.Tm = tiles + (size_t)a * n2;
      F.sA = F.sW = F.sT = n2;
      F.lauum(F.Tm, n2);
      HIPCHK(c, F.err);
      src = F.Tm;
    }
    hipLaunchKernelGGL(nh_form_q_kernel, dim3((unsigned)(n2 / 256), len), dim3(256), 0, st, src, n2, npad,
                       k.spb + (size_t)a * SP_STRIDE, lch ? 1 : 0, alpha + (size_t)a * npad, N, npad, Q + (size_t)a * n2, n2,
                       diagq + (size_t)a * npad);
    HIPCHK(c, hipGetLastError());
    return 0;
  });
}

int nll_hess_impl(gpc_post* po, const double* dm, int mean_N, const double* dsn2, int dsn2_rows, int noise_N, double* H,
                  double* dnlz, double* alpha_out, double* diagq_out) {
  gpc_ctx* c = po->ctx;
  const int S = po->S, N = po->N, npad = po->npad, cov_N = po->cd.cov_N;
  const int ppl = cov_N + noise_N, P = ppl + mean_N, nvec = ppl + mean_N;
  const bool ard = !cov_is_iso(po->cd.kind);
  const int nd2 = ard ? nh_pairs(po->D) : 0;
  hipStream_t st = c->st;
  const long long n2 = (long long)npad * npad;
  const size_t per = ScratchCarver::count<NhScratch>(1, npad, cov_N, noise_N, mean_N, nd2);
  const size_t held = c->nhs.bytes;
  const int chunk = plan_chunk(c, S, per, 0, held, (size_t)S * per <= held, 0, false, [&](size_t budget) {
    return "gpc_nll_hess: the scratch of one sample (" + std::to_string(per) + " bytes: N_pad = " + std::to_string(npad) +
           ", planes = " + std::to_string(ppl) + ": Q, one B per plane and one operand) exceeds the device memory budget (" +
           std::to_string(budget) + " bytes)";
  });
  if (!chunk) return -2;
  HIPCHK(c, c->nhs.ensure((size_t)chunk * per));
  NhScratch z;
  ScratchCarver::carve(z, c->nhs.p, chunk, npad, cov_N, noise_N, mean_N, nd2);
  CallTimer tm{c, CallTimer::wanted(c, npad)};
  GramClock gc(tm.on), cc(tm.on);
  double gram_us = 0, contract_us = 0;
  ChunkConsts k;
  if (int rc = k.init(po, chunk)) return rc;
  c->ms_total = c->ms_factor = 0;
  const size_t vlen = (size_t)chunk * npad;
  std::vector<double> hx((size_t)(mean_N + noise_N) * vlen), hX((size_t)ppl * vlen), hY((size_t)nvec * vlen), hal(vlen),
      hdq(vlen), hgr((size_t)chunk * z.npairs), hg((size_t)cov_N * chunk * 2), hd2((size_t)chunk * nd2), uw((size_t)ppl * ppl);
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    ScratchCarver::carve(z, c->nhs.p, cnt, npad, cov_N, noise_N, mean_N, nd2);
    if (int rc = k.stage(s0, cnt, true)) return rc;
    const double* alpha = po->alpha.as<double>() + (size_t)s0 * npad;
    // the mean planes d_k m (rows of X after the u's) and the noise planes' e = mult d sn2, zero in the padding
    std::fill(hx.begin(), hx.end(), 0.0);
    double* hdm = hx.data();
    double* he = hx.data() + (size_t)mean_N * cnt * npad;
    for (int i = 0; i < cnt; ++i) {
      const int s = s0 + i;
      for (int kk = 0; kk < mean_N; ++kk)
        for (int a = 0; a < N; ++a) hdm[((size_t)kk * cnt + i) * npad + a] = dm[((size_t)s * N + a) * mean_N + kk];
      for (int nz = 0; nz < noise_N; ++nz)
        for (int a = 0; a < N; ++a)
          he[((size_t)nz * cnt + i) * npad + a] =
              po->mult[s] * dsn2[((size_t)s * dsn2_rows + (dsn2_rows == 1 ? 0 : a)) * noise_N + nz];
    }
    if (mean_N)
      HIPCHK(c, hipMemcpyAsync(z.X + (size_t)ppl * cnt * npad, hdm, (size_t)mean_N * cnt * npad * 8, hipMemcpyHostToDevice, st));
    if (noise_N) HIPCHK(c, hipMemcpyAsync(z.E, he, (size_t)noise_N * cnt * npad * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, tm.start());
    // a. Q of every sample: W^T W / sl (L_chol; the lower tiles land in the operand buffer) | -A
    if (int rc = posterior_q(po, k, s0, cnt, z.Op, z.Q, z.diagq)) return rc;
    HIPCHK(c, tm.mark1());
    // b, c. the covariance planes: operand, then B_p = Q d_p K on the plain batched GEMM
    for (int p = 0; p < cov_N; ++p) {
      if (int rc = nh_launch_plane(c, po->cd, z, cnt, p, k.xsb, k.spb, alpha, N)) return rc;
      GemmArgs g;
      g.A = z.Q, g.B = z.Op, g.C = z.B + (size_t)p * n2;
      g.sA = n2, g.sB = n2, g.sC = (long long)ppl * n2;
      g.lda = g.ldb = g.ldc = npad;
      g.M = g.N = g.K = npad;
      g.alpha = 1.0, g.beta = 0;
      g.klo = KLO_ZERO, g.khi = KHI_FULL, g.lower_only = 0;
      g.tiles_n = npad / TILE;
      HIPCHK(c, launch_gemm<double>(st, g, false, true, cnt));
    }
    HIPCHK(c, tm.mark2());
    for (int nz = 0; nz < noise_N; ++nz) {  // (a batch of planes cov_N + nz: sample stride ppl n2)
      hipLaunchKernelGGL(nh_noise_plane_kernel, dim3((unsigned)(n2 / 256), cnt), dim3(256), 0, st, (const double*)z.Q, n2,
                         (const double*)(z.E + (size_t)nz * cnt * npad), alpha, npad, z.B + (size_t)(cov_N + nz) * n2,
                         (long long)ppl * n2, z.X + (size_t)(cov_N + nz) * cnt * npad);
    }
    // f. w_p = Q u_p and v_k = Q d_k m
    hipLaunchKernelGGL(nh_matvec_kernel, dim3(npad / 4, nvec, cnt), dim3(256), 0, st, (const double*)z.Q, n2, npad,
                       (const double*)z.X, z.Y);
    HIPCHK(c, hipGetLastError());
    // d. the Gram pass, e. the second-derivative contraction
    HIPCHK(c, gc.record(0, st));
    if (int rc = nh_launch_gram(c, z, cnt)) return rc;
    HIPCHK(c, gc.record(1, st));
    HIPCHK(c, cc.record(0, st));
    if (ard)
      if (int rc = nh_launch_d2(c, po->cd, z, cnt, k.xsb, k.spb, alpha, N)) return rc;
    HIPCHK(c, cc.record(1, st));
    HIPCHK(c, tm.stop());
    HIPCHK(c, hipMemcpyAsync(hX.data(), z.X, (size_t)ppl * cnt * npad * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hY.data(), z.Y, (size_t)nvec * cnt * npad * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hal.data(), alpha, (size_t)cnt * npad * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hdq.data(), z.diagq, (size_t)cnt * npad * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hgr.data(), z.grsum, (size_t)cnt * z.npairs * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hg.data(), z.gsum, (size_t)cov_N * cnt * 2 * 8, hipMemcpyDeviceToHost, st));
    if (nd2) HIPCHK(c, hipMemcpyAsync(hd2.data(), z.d2sum, (size_t)cnt * nd2 * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    tm.accumulate();
    gram_us += gc.elapsed_us();
    contract_us += cc.elapsed_us();
    // the small dot products and the assembly: the lower triangle, mirrored
    for (int i = 0; i < cnt; ++i) {
      const int s = s0 + i;
      const double* al = &hal[(size_t)i * npad];
      const double* dq = &hdq[(size_t)i * npad];
      auto uvec = [&](int p) { return &hX[((size_t)p * cnt + i) * npad]; };
      auto yvec = [&](int v) { return &hY[((size_t)v * cnt + i) * npad]; };
      auto dmv = [&](int kk) { return &hdm[((size_t)kk * cnt + i) * npad]; };
      auto dot = [&](const double* x, const double* y) {
        double t = 0.0;
        for (int a = 0; a < N; ++a) t = std::fma(x[a], y[a], t);
        return t;
      };
      double* Hs = H + (size_t)s * P * P;
      double* gs = dnlz + (size_t)s * P;
      const double* g = &hg[(size_t)i * 2];  // sample i's pair of plane p at g[p * cnt * 2]
      const int gstride = cnt * 2;
      for (int p = 0; p < ppl; ++p) {
        const double g1 = p < cov_N ? g[(size_t)p * gstride] : dot(dq, &he[((size_t)(p - cov_N) * cnt + i) * npad]);
        gs[p] = 0.5 * g1;
        for (int q = 0; q <= p; ++q) {
          const double second = p < cov_N ? nh_second(po->cd, p, q, g, gstride, &hd2[(size_t)i * nd2]) : 0.0;
          const double v = -0.5 * hgr[(size_t)i * z.npairs + p * (p + 1) / 2 + q] + dot(uvec(p), yvec(q)) + 0.5 * second;
          Hs[(size_t)p * P + q] = Hs[(size_t)q * P + p] = v;
        }
      }
      for (int kk = 0; kk < mean_N; ++kk) {
        const int r = ppl + kk;
        gs[r] = -dot(al, dmv(kk));
        for (int p = 0; p < ppl; ++p) Hs[(size_t)r * P + p] = Hs[(size_t)p * P + r] = dot(yvec(p), dmv(kk));
        for (int l = 0; l <= kk; ++l) Hs[(size_t)r * P + ppl + l] = Hs[(size_t)(ppl + l) * P + r] = dot(dmv(kk), yvec(ppl + l));
      }
      std::copy(al, al + N, alpha_out + (size_t)s * N);
      std::copy(dq, dq + N, diagq_out + (size_t)s * N);
    }
  }
  c->nll_hess_gram_us = (unsigned long long)gram_us;
  c->nll_hess_contract_us = (unsigned long long)contract_us;
  return 0;
}

// ---- gpc_cv_grad: the leave-one-out objective's weight matrix and its contraction (cvgrad.h) ---------------------------

// <d_p K, G> of `cnt` samples into gsum[b][p], diag(G) into diagG: the contraction and the sum of its per-tile partials
int cvg_launch_trace(gpc_ctx* c, const CovDesc& cd, int cnt, int N, int npad, const double* xs, const double* sp,
                     const double* alpha, const double* beta, const double* M, double* part, double* gsum, double* diagG) {
  const int nt = npad / CT, ntl = nt * (nt + 1) / 2, P = cd.cov_N;
  const size_t shm = 4 * (size_t)(((P + 3) & ~3) + 4) * sizeof(double);
  GPC_COV_DISPATCH(cvg_trace_kernel, double, cd, dim3(ntl, cnt), dim3(256), shm, c->st, cd, xs, sp, alpha, beta, N, npad, M,
                   (long long)npad * npad, part, ntl, diagG);
  hipLaunchKernelGGL(reduce_parts_kernel, dim3(P, cnt), dim3(256), 0, c->st, (const double*)part, ntl, P, gsum);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int cv_grad_impl(gpc_post* po, int loss, const double* weights, double* gsum_out, double* diagG_out, double* beta_out,
                 double* alpha_out, double* q_out, double* c_out) {
  gpc_ctx* c = po->ctx;
  const int S = po->S, N = po->N, npad = po->npad, cov_N = po->cd.cov_N;
  hipStream_t st = c->st;
  const long long n2 = (long long)npad * npad;
  const size_t per = ScratchCarver::count<CvgScratch>(1, npad, cov_N), shared = (size_t)npad * 8;
  const size_t held = c->nhs.bytes;
  const int chunk = plan_chunk(c, S, per, shared, held, shared + (size_t)S * per <= held, 0, false, [&](size_t budget) {
    return "gpc_cv_grad: the scratch of one sample (" + std::to_string(per) + " bytes: N_pad = " + std::to_string(npad) +
           ": Q, Q diag(c) and their product) exceeds the device memory budget (" + std::to_string(budget) + " bytes)";
  });
  if (!chunk) return -2;
  HIPCHK(c, c->nhs.ensure(shared + (size_t)chunk * per));
  double* d_omega = c->nhs.as<double>();  // the weights, shared by the samples, ahead of the chunk's scratch
  std::vector<double> hw(npad, 0.0);
  for (int i = 0; i < N; ++i) hw[i] = weights ? weights[i] : 1.0;
  HIPCHK(c, hipMemcpyAsync(d_omega, hw.data(), (size_t)npad * 8, hipMemcpyHostToDevice, st));
  CvgScratch z;
  CallTimer tm{c, CallTimer::wanted(c, npad)};
  GramClock tc(tm.on);
  double trace_us = 0;
  ChunkConsts k;
  if (int rc = k.init(po, chunk)) return rc;
  c->ms_total = c->ms_factor = 0;
  const size_t vlen = (size_t)chunk * npad;
  ScratchCarver::carve(z, d_omega + npad, chunk, npad, cov_N);
  std::vector<double> ho(z.out_bytes / 8), hal(vlen);
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    ScratchCarver::carve(z, d_omega + npad, cnt, npad, cov_N);
    if (int rc = k.stage(s0, cnt, true)) return rc;
    const double* alpha = po->alpha.as<double>() + (size_t)s0 * npad;
    HIPCHK(c, tm.start());
    HIPCHK(c, tm.mark1());
    // a. Q of every sample: W^T W / sl (L_chol; the lower tiles land in M's buffer, overwritten in d) | -A
    if (int rc = posterior_q(po, k, s0, cnt, z.M, z.Q, z.diagq)) return rc;
    // b. c and b per point, beta = Q b
    hipLaunchKernelGGL(cvg_weights_kernel, dim3((npad + 255) / 256, cnt), dim3(256), 0, st, alpha, (const double*)z.Q, n2,
                       npad + 1, (const double*)d_omega, N, npad, loss, z.q, z.cw, z.b);
    hipLaunchKernelGGL(nh_matvec_kernel, dim3(npad / 4, 1, cnt), dim3(256), 0, st, (const double*)z.Q, n2, npad,
                       (const double*)z.b, z.beta);
    // c. QC = Q diag(c): the noise planes' column scaling
    hipLaunchKernelGGL(nh_noise_plane_kernel, dim3((unsigned)(n2 / 256), cnt), dim3(256), 0, st, (const double*)z.Q, n2,
                       (const double*)z.cw, alpha, npad, z.QC, n2, z.u);
    HIPCHK(c, hipGetLastError());
    // d. M = QC Q^T, the lower tiles only (Q is symmetric to the bit: its rows serve as the k-major operand)
    {
      GemmArgs g;
      g.A = z.QC, g.B = z.Q, g.C = z.M;
      g.sA = g.sB = g.sC = n2;
      g.lda = g.ldb = g.ldc = npad;
      g.M = g.N = g.K = npad;
      g.alpha = 1.0, g.beta = 0;
      g.klo = KLO_ZERO, g.khi = KHI_FULL, g.lower_only = 1;
      HIPCHK(c, launch_gemm<double>(st, g, false, true, cnt));
    }
    HIPCHK(c, tm.mark2());
    // e. the contraction <d_p K, G>
    HIPCHK(c, tc.record(0, st));
    if (int rc = cvg_launch_trace(c, po->cd, cnt, N, npad, k.xsb, k.spb, alpha, z.beta, z.M, z.part, z.gsum, z.diagG)) return rc;
    HIPCHK(c, tc.record(1, st));
    HIPCHK(c, tm.stop());
    // f. the sums and the vectors; the value and the noise and mean columns are the caller's
    HIPCHK(c, hipMemcpyAsync(ho.data(), z.out, z.out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hal.data(), alpha, (size_t)cnt * npad * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    tm.accumulate();
    trace_us += tc.elapsed_us();
    const double* hg = ho.data();
    const double* hv = hg + (size_t)cnt * cov_N;  // diagG | beta | q | cw, cnt x npad each
    const size_t pl = (size_t)cnt * npad;
    for (int i = 0; i < cnt; ++i) {
      const size_t s = s0 + i, o = (size_t)i * npad;
      std::copy(hg + (size_t)i * cov_N, hg + (size_t)(i + 1) * cov_N, gsum_out + s * cov_N);
      std::copy(hv + o, hv + o + N, diagG_out + s * N);
      std::copy(hv + pl + o, hv + pl + o + N, beta_out + s * N);
      std::copy(hv + 2 * pl + o, hv + 2 * pl + o + N, q_out + s * N);
      std::copy(hv + 3 * pl + o, hv + 3 * pl + o + N, c_out + s * N);
      std::copy(hal.begin() + o, hal.begin() + o + N, alpha_out + s * N);
    }
  }
  c->cv_grad_trace_us = (unsigned long long)trace_us;
  return 0;
}

// ---- gpc_predict_hyp_grad: derivatives of the latent prediction with respect to the hyperparameters (hypgrad.h) --------
// The covariance hyperparameters that are planes (a lengthscale or the RQ shape: everything but log sf), in order
inline std::vector<int> hg_plane_cols(const CovDesc& cd) {
  std::vector<int> cols;
  for (int p = 0; p < cd.cov_N; ++p) {
    int mode, dim;
    nh_plane_of(cd, p, &mode, &dim);
    if (mode != NH_SF) cols.push_back(p);
  }
  return cols;
}

// Per chunk of samples and super-block of queries (all of the call's queries unless the budget says otherwise), with
// the variance:
//   panel K* = k(X, x*) (cross_tile_kernel),  Qs = W^T (W K*) (L_chol; q = Qs / sl) | L K* (low noise; q = -Qs)
//   per plane (lengthscale, RQ shape): d_p K dense with u_p = d_p K alpha fused in (hg_plane_kernel),
//     T = d_p K Qs on the plain fp64 GEMM, q_j^T d_p K q_j by hg_coldot_kernel (the first plane's pass also leaves the
//     weighted column sums of squares sum_i v_i q_ij^2)
//   w_p = Q u_p for all P vectors: two triangular matrix-vector products (L_chol) | one symmetric (low noise)
//   the fused cross pass (hg_cross_kernel) and the assembly on the host.
// Without the variance: the planes' u_p alone (nothing dense), the same weights, hg_cross_mean_kernel -- no product
// with W, no GEMM; fmu and dfmu are the same instructions on the same operands.  The planes are rebuilt per super-block.
// gpc_last_timing: the device sections and, of these, the interval of the products with W and the planes' build, GEMM
// and column dots.
int hyp_grad_impl(gpc_post* po, const double* xstar, int M, bool var, const double* sn2, const double* dsn2, int rows,
                  int noise_N, const double* dm, int mean_N, double* fmu, double* fs2, double* dfmu, double* dfs2) {
  gpc_ctx* c = po->ctx;
  const int S = po->S, N = po->N, D = po->D, npad = po->npad, cov_N = po->cd.cov_N;
  const int P = cov_N + noise_N + mean_N, sfc = hg_sf_col(po->cd);
  const std::vector<int> gcols = hg_plane_cols(po->cd);
  const int ngp = (int)gcols.size(), nvv = rows == 1 ? 1 : 1 + noise_N;
  const int nout = hg_cross_sums(P, cov_N, var), nt = npad / CT, nch = npad / TRC;
  hipStream_t st = c->st;
  const long long n2 = (long long)npad * npad, sM = n2;
  // the super-block: all queries, halved until one sample fits
  int msb = pad_tile(M), chunk = 0;
  size_t per = 0;
  for (;;) {
    per = ScratchCarver::count<HgScratch>(1, npad, D, P, nvv, ngp, msb, var, nout);
    const size_t held = c->hgs.bytes;
    const int blk = msb;
    chunk = plan_chunk(c, S, per, 0, held, (size_t)S * per <= held, 0, false, [&](size_t budget) {
      return "gpc_predict_hyp_grad: the scratch of one sample with one query block (" + std::to_string(per) +
             " bytes: N_pad = " + std::to_string(npad) + ", planes = " + std::to_string(ngp) + ", block = " +
             std::to_string(blk) + " queries) exceeds the device memory budget (" + std::to_string(budget) + " bytes)";
    });
    if (chunk || msb == TILE) break;
    msb = pad_tile(msb / 2);
  }
  if (!chunk) return -2;
  const long long sK = (long long)npad * msb;
  HIPCHK(c, c->hgs.ensure((size_t)chunk * per));
  HIPCHK(c, c->cs.ensure((size_t)M * D * 8));  // (the raw queries: all the consumers' block holds for this call)
  double* const d_xa = c->cs.as<double>();
  HgScratch z;
  CallTimer tm{c, CallTimer::wanted(c, npad)};
  HIPCHK(c, hipMemcpyAsync(d_xa, xstar, (size_t)M * D * 8, hipMemcpyHostToDevice, st));
  ChunkConsts k;
  if (int rc = k.init(po, chunk)) return rc;
  c->ms_total = c->ms_factor = 0;
  const size_t vlen = (size_t)chunk * npad;
  const size_t dper = ((size_t)ngp + nvv) * msb;  // doubles of a sample's quadratic-form sums
  std::vector<double> hX((size_t)P * vlen), hV(var ? (size_t)nvv * vlen : 0), hqs(chunk), hc((size_t)chunk * nout * msb),
      hd(var ? (size_t)chunk * dper : 0);
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    ScratchCarver::carve(z, c->hgs.p, cnt, npad, D, P, nvv, ngp, msb, var, nout);
    if (int rc = k.stage(s0, cnt, true)) return rc;
    const double* alpha = po->alpha.as<double>() + (size_t)s0 * npad;
    // what the weights start from, zero in the padding: mult sn2 (log sf), mult d_n sn2 (noise n), d_k m (mean k); the
    // planes' rows are written on the device.  For the column dots: sn2 and d_n sn2 per point
    std::fill(hX.begin(), hX.end(), 0.0);
    std::fill(hV.begin(), hV.end(), 0.0);
    for (int i = 0; i < cnt; ++i) {
      const int s = s0 + i;
      const double mult = po->mult[s];
      hqs[i] = po->lchol[s] ? 1.0 / po->sp[(size_t)s * SP_STRIDE + SP_SL] : -1.0;
      for (int a = 0; a < N; ++a) {
        const size_t r = (size_t)s * rows + (rows == 1 ? 0 : a);
        hX[((size_t)sfc * cnt + i) * npad + a] = mult * sn2[r];
        for (int nz = 0; nz < noise_N; ++nz) hX[((size_t)(cov_N + nz) * cnt + i) * npad + a] = mult * dsn2[r * noise_N + nz];
        for (int kk = 0; kk < mean_N; ++kk)
          hX[((size_t)(cov_N + noise_N + kk) * cnt + i) * npad + a] = dm[((size_t)s * N + a) * mean_N + kk];
        if (var && rows != 1) {
          hV[(size_t)i * npad + a] = sn2[r];
          for (int nz = 0; nz < noise_N; ++nz) hV[((size_t)(1 + nz) * cnt + i) * npad + a] = dsn2[r * noise_N + nz];
        }
      }
    }
    if (var && rows != 1) HIPCHK(c, hipMemcpyAsync(z.Vn, hV.data(), (size_t)nvv * cnt * npad * 8, hipMemcpyHostToDevice, st));
    if (var) HIPCHK(c, hipMemcpyAsync(z.qs, hqs.data(), (size_t)cnt * 8, hipMemcpyHostToDevice, st));
    for (int b0 = 0; b0 < M; b0 += msb) {
      const int mq = std::min(msb, M - b0);
      HIPCHK(c, hipMemcpyAsync(z.X + (size_t)sfc * cnt * npad, &hX[(size_t)sfc * cnt * npad], (size_t)cnt * npad * 8,
                               hipMemcpyHostToDevice, st));
      if (P > cov_N)
        HIPCHK(c, hipMemcpyAsync(z.X + (size_t)cov_N * cnt * npad, &hX[(size_t)cov_N * cnt * npad],
                                 (size_t)(P - cov_N) * cnt * npad * 8, hipMemcpyHostToDevice, st));
      HIPCHK(c, tm.start());
      hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)msb * D + 255) / 256), cnt), dim3(256), 0, st,
                         (const double*)(d_xa + (size_t)b0 * D), mq, msb, D, k.mulb, k.divb, z.xss);
      if (var) {
        GPC_COV_DISPATCH(cross_tile_kernel, double, po->cd, dim3(msb / CT, npad / CT, cnt), dim3(256), 0, st, po->cd, k.xsb,
                         (const double*)z.xss, k.spb, alpha, npad, N, npad, mq, msb, z.KP, sK, z.mupart);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, tm.mark1());
        // the products of every run of equal L_chol: Qs = W^T (W K*) | L K*
        const int rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
          GemmArgs g = tri_product_args<double>(po, s0 + a, lch, z.KP + (size_t)a * sK, (lch ? z.VP : z.Qa) + (size_t)a * sK,
                                                sK, msb, msb);
          HIPCHK(c, launch_gemm<double>(st, g, false, true, len));
          if (lch) {  // W^T upper triangular: k from the tile row's diagonal block on
            HIPCHK(c, launch_gemm<double>(st, wt_product_args(g, z.VP + (size_t)a * sK, z.Qa + (size_t)a * sK), true, true, len));
          }
          return 0;
        });
        if (rc_runs) return rc_runs;
      }
      // the planes: u_p and, with the variance, the quadratic forms through T = d_p K Qs (T overlays the panel K*)
      for (int gi = 0; gi < ngp; ++gi) {
        const int p = gcols[gi];
        int mode, dim;
        nh_plane_of(po->cd, p, &mode, &dim);
        GPC_COV_DISPATCH(hg_plane_kernel, double, po->cd, dim3(nt, nt, cnt), dim3(256), 0, st, po->cd, k.xsb, k.spb, alpha, N,
                         npad, mode, dim, var ? z.Op : (double*)nullptr, n2, z.upart);
        hipLaunchKernelGGL(colpart_reduce_kernel, dim3((npad + 255) / 256, cnt), dim3(256), 0, st, (const double*)z.upart, nt,
                           npad, z.X + (size_t)p * cnt * npad);
        HIPCHK(c, hipGetLastError());
        if (!var) continue;
        GemmArgs g;
        g.A = z.Op, g.B = z.Qa, g.C = z.KP;
        g.sA = n2, g.sB = g.sC = sK;
        g.lda = npad, g.ldb = g.ldc = msb;
        g.M = npad, g.N = msb, g.K = npad;
        g.alpha = 1.0, g.beta = 0;
        g.klo = KLO_ZERO, g.khi = KHI_FULL, g.lower_only = 0;
        g.tiles_n = msb / TILE;
        HIPCHK(c, launch_gemm<double>(st, g, false, true, cnt));
        const int nv = gi == 0 ? nvv : 0;  // the first plane's pass also takes the weighted sums of squares
        hipLaunchKernelGGL(hg_coldot_kernel, dim3(msb / TILE, nt, cnt), dim3(256), 0, st, (const double*)z.Qa, sK,
                           (const double*)z.KP, sK, msb, (const double*)(rows == 1 ? nullptr : z.Vn), nv, N, npad, z.dpart);
        double* const dst = gi == 0 ? z.dsum : z.dsum + (size_t)cnt * (1 + nvv) * msb + (size_t)(gi - 1) * cnt * msb;
        hipLaunchKernelGGL(colpart_reduce_kernel, dim3((unsigned)(((size_t)(1 + nv) * msb + 255) / 256), cnt), dim3(256), 0, st,
                           (const double*)z.dpart, nt, (1 + nv) * msb, dst);
        HIPCHK(c, hipGetLastError());
      }
      if (var) HIPCHK(c, tm.mark2());
      // the weights: e o alpha, then w = Q x for all P vectors, then log sf's 2 alpha - 2 (.)
      hipLaunchKernelGGL(hg_mul_alpha_kernel, dim3((npad + 255) / 256, 1, cnt), dim3(256), 0, st,
                         z.X + (size_t)sfc * cnt * npad, alpha, npad);
      if (noise_N)
        hipLaunchKernelGGL(hg_mul_alpha_kernel, dim3((npad + 255) / 256, noise_N, cnt), dim3(256), 0, st,
                           z.X + (size_t)cov_N * cnt * npad, alpha, npad);
      for (int p = 0; p < P; ++p) {
        const double* xp = z.X + (size_t)p * cnt * npad;
        double* const yp = z.Y + (size_t)p * cnt * npad;
        const int rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
          if (lch) {
            const double* W = po->W.as<double>() + (size_t)(s0 + a) * sM;
            hipLaunchKernelGGL((trmv_kernel<double>), dim3(npad / 4, len), dim3(256), 0, st, W, sM, npad, xp + (size_t)a * npad,
                               npad, z.tmp + (size_t)a * npad, 0);
            hipLaunchKernelGGL((trmv_t_part_kernel<double, 8>), dim3((npad + 64 * MM<double>::VEC - 1) / (64 * MM<double>::VEC), nch, len),
                               dim3(256), 0, st, W, sM, npad, (const double*)(z.tmp + (size_t)a * npad), npad,
                               z.tpart + (size_t)a * nch * npad, (double*)nullptr);
            hipLaunchKernelGGL(trmv_t_sum_kernel, dim3(npad / 128, len), dim3(128), 0, st,
                               (const double*)(z.tpart + (size_t)a * nch * npad), npad, k.spb + (size_t)a * SP_STRIDE,
                               (int)SP_STRIDE, (int)SP_SL, yp + (size_t)a * npad);
          } else {  // y = 0 - L x (L = -(K + Sigma)^-1, full symmetric)
            HIPCHK(c, hipMemsetAsync(yp + (size_t)a * npad, 0, (size_t)len * npad * 8, st));
            hipLaunchKernelGGL((gemv_sub_kernel<double>), dim3(npad / 4, len), dim3(256), 0, st,
                               (const double*)(po->A.as<double>() + (size_t)(s0 + a) * sM), sM, npad, xp + (size_t)a * npad,
                               yp + (size_t)a * npad, npad, 0, 0, npad);
          }
          return 0;
        });
        if (rc_runs) return rc_runs;
      }
      hipLaunchKernelGGL(hg_sf_weight_kernel, dim3((npad + 255) / 256, cnt), dim3(256), 0, st,
                         z.Y + (size_t)sfc * cnt * npad, alpha, npad);
      HIPCHK(c, hipGetLastError());
      // the fused cross pass
      if (var)
        GPC_COV_DISPATCH(hg_cross_kernel, double, po->cd, dim3(msb / CT, npad / CT, cnt), dim3(256), 0, st, po->cd, k.xsb,
                         (const double*)z.xss, k.spb, alpha, (const double*)z.Y, P, (const double*)z.Qa, sK, msb,
                         (const double*)z.qs, N, npad, mq, msb, z.cpart);
      else
        GPC_COV_DISPATCH(hg_cross_mean_kernel, double, po->cd, dim3(msb / CT, npad / CT, cnt), dim3(256), 0, st, po->cd, k.xsb,
                         (const double*)z.xss, k.spb, alpha, (const double*)z.Y, P, N, npad, mq, msb, z.cpart);
      hipLaunchKernelGGL(colpart_reduce_kernel, dim3((unsigned)(((size_t)nout * msb + 255) / 256), cnt), dim3(256), 0, st,
                         (const double*)z.cpart, nt, nout * msb, z.csum);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(hc.data(), z.csum, (size_t)cnt * nout * msb * 8, hipMemcpyDeviceToHost, st));
      if (var) HIPCHK(c, hipMemcpyAsync(hd.data(), z.dsum, (size_t)cnt * dper * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, tm.stop());
      HIPCHK(c, hipStreamSynchronize(st));
      if (var) tm.accumulate();
      else if (tm.on) {  // no product: the whole device section, nothing in it a product's
        float t03 = 0;
        (void)hipEventElapsedTime(&t03, c->ev[0], c->ev[3]);
        c->ms_total += t03;
      }
      // into the caller's layout
      for (int i = 0; i < cnt; ++i) {
        const int s = s0 + i;
        const double mult = po->mult[s], qs2 = hqs[i] * hqs[i], sf2 = po->sp[(size_t)s * SP_STRIDE + SP_SF2];
        const double* cs = &hc[(size_t)i * nout * msb];
        const double* d0 = var ? &hd[(size_t)i * (1 + nvv) * msb] : nullptr;
        for (int jj = 0; jj < mq; ++jj) {
          const size_t j = (size_t)b0 + jj;
          auto Bs = [&](int p) { return cs[(size_t)p * msb + jj]; };
          auto As = [&](int cc) { return cs[(size_t)(P + cc) * msb + jj]; };
          auto Cs = [&](int cc) { return cs[(size_t)(P + cov_N + cc) * msb + jj]; };
          fmu[j * S + s] = As(sfc);
          for (int p = 0; p < P; ++p)
            dfmu[(j * P + p) * S + s] = p < cov_N ? (p == sfc ? 2.0 * As(p) : As(p)) - Bs(p) : -Bs(p);
          if (!var) continue;
          const double f2 = sf2 - Cs(sfc);
          fs2[j * S + s] = f2;
          auto vsum = [&](int v) { return d0[(size_t)(1 + v) * msb + jj]; };
          for (int gi = 0; gi < ngp; ++gi) {
            const double quad = gi == 0 ? d0[jj] : hd[(size_t)cnt * (1 + nvv) * msb + ((size_t)(gi - 1) * cnt + i) * msb + jj];
            dfs2[(j * P + gcols[gi]) * S + s] = -2.0 * Cs(gcols[gi]) + qs2 * quad;
          }
          const double sq = rows == 1 ? sn2[s] * vsum(0) : vsum(0);
          dfs2[(j * P + sfc) * S + s] = 2.0 * f2 - 2.0 * mult * qs2 * sq;
          for (int nz = 0; nz < noise_N; ++nz)
            dfs2[(j * P + cov_N + nz) * S + s] =
                mult * qs2 * (rows == 1 ? dsn2[(size_t)s * noise_N + nz] * vsum(0) : vsum(1 + nz));
          for (int kk = 0; kk < mean_N; ++kk) dfs2[(j * P + cov_N + noise_N + kk) * S + s] = 0.0;
        }
      }
    }
  }
  return 0;
}

}  // namespace

// test-hook helpers
namespace {
template <typename T>
int upload_as(gpc_ctx* c, DevBuf& buf, const double* src, size_t n) {
  HIPCHK(c, buf.ensure(n * sizeof(T)));
  if constexpr (sizeof(T) == 8) {
    HIPCHK(c, hipMemcpyAsync(buf.p, src, n * 8, hipMemcpyHostToDevice, c->st));
  } else {
    std::vector<float> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = (float)src[i];
    HIPCHK(c, hipMemcpyAsync(buf.p, tmp.data(), n * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
  }
  return 0;
}
template <typename T>
int download_as(gpc_ctx* c, const T* src, double* dst, size_t n) {
  if constexpr (sizeof(T) == 8) {
    HIPCHK(c, hipMemcpyAsync(dst, src, n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
  } else {
    std::vector<float> tmp(n);
    HIPCHK(c, hipMemcpyAsync(tmp.data(), src, n * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    for (size_t i = 0; i < n; ++i) dst[i] = tmp[i];
  }
  return 0;
}

template <typename T>
int debug_gemm_impl(gpc_ctx* c, int M, int N, int K, int akm, int bkm, double alpha, int beta, int klo,
                    int khi, int lower, const double* A, const double* B, double* C) {
  if (upload_as<T>(c, c->dbg1, A, (size_t)M * K)) return -1;
  if (upload_as<T>(c, c->dbg2, B, (size_t)N * K)) return -1;
  if (upload_as<T>(c, c->dbg3, C, (size_t)M * N)) return -1;
  GemmArgs g;
  g.A = c->dbg1.p;
  g.B = c->dbg2.p;
  g.C = c->dbg3.p;
  g.sA = g.sB = g.sC = 0;
  g.lda = akm ? M : K;
  g.ldb = bkm ? N : K;
  g.ldc = N;
  g.M = M;
  g.N = N;
  g.K = K;
  g.alpha = alpha;
  g.beta = beta;
  g.klo = klo;
  g.khi = khi;
  g.lower_only = lower & 1;
  g.tiles_n = N / TILE;
  HIPCHK(c, launch_gemm<T>(c->st, g, akm != 0, bkm != 0, 1, (lower & 0x100) ? 64 : ((lower & 0x200) ? 128 : ((lower & 0x400) ? 12864 : 0))));  // (12864: experiments build)
  return download_as<T>(c, c->dbg3.as<T>(), C, (size_t)M * N);
}

// ---- gpc_debug_gemm_form: one product (two for the dual form) through a chosen launch form of gemm.h ----
// device allocations of one hook call, freed when it returns (whatever the way out)
struct HookMem {
  std::vector<void*> ps;
  ~HookMem() {
    for (void* p : ps) (void)hipFree(p);
  }
  hipError_t get(void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e == hipSuccess) ps.push_back(*p);
    return e;
  }
};
// the globals of gemm.h a hook call overrides, put back when it returns
struct GemmGlobalsGuard {
  const int flags = gpc::g_gemm_flags, slots = gpc::g_block_slots, spare = gpc::g_persist_spare;
  ~GemmGlobalsGuard() {
    gpc::g_gemm_flags = flags;
    gpc::g_block_slots = slots;
    gpc::g_persist_spare = spare;
  }
};

// Every element the kernels may address lies inside the caller's allocations (the staging loads go through unbounded
// buffer descriptors: nothing else stops a bad description).  vec: elements per 16-byte staging vector.
const char* form_product_error(const gpc_gemm_product& p, int batch, int vec) {
  constexpr long long CAP = 1ll << 27;  // elements per allocation: every 32-bit offset of the kernels stays far away
  if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.M % TILE || p.N % TILE || p.K % TILE) return "sizes must be multiples of 128";
  if (p.lower_only && p.M != p.N) return "lower_only needs M == N";
  if ((p.beta != 0 && p.beta != 1) || p.klo < 0 || p.klo > 2 || p.khi < 0 || p.khi > 2) return "beta is 0 or 1, klo and khi 0..2";
  if (!p.A || !p.B || !p.C) return "A, B and C are required";
  const long long ra = p.a_kmajor ? p.K : p.M, ca = p.a_kmajor ? p.M : p.K;
  const long long rb = p.b_kmajor ? p.K : p.N, cb = p.b_kmajor ? p.N : p.K;
  struct Op {
    long long rows, cols, ld, off, stride, size;
    bool staged;
  } ops[3] = {{ra, ca, p.lda, p.off_a, p.s_a, p.size_a, true},
              {rb, cb, p.ldb, p.off_b, p.s_b, p.size_b, true},
              {p.M, p.N, p.ldc, p.off_c, p.s_c, p.size_c, false}};
  for (const Op& o : ops) {
    if (o.ld < o.cols || o.off < 0 || o.stride < 0 || o.size <= 0 || o.size > CAP || o.ld > CAP || o.stride > CAP)
      return "leading dimension below the extent, or a negative / oversized offset, stride or allocation";
    const long long span = (o.rows - 1) * o.ld + o.cols;
    if (o.off + (batch - 1) * o.stride + span > o.size) return "an operand reaches past its allocation";
    if (o.staged && (o.ld % vec || o.off % vec || o.stride % vec))
      return "lda, ldb and the offsets and strides of A and B must be multiples of the 16-byte vector";
    if (!o.staged && batch > 1 && o.stride < span) return "the C blocks of two samples overlap";
  }
  return nullptr;
}

template <typename T>
int debug_gemm_form_impl(gpc_ctx* c, int form, int tile, int batch, int flags, int block_slots,
                         const gpc_gemm_product* const* prods, int nprod, const double* ep_w, long long ep_sw,
                         const double* ep_alpha, double* colsq, int* counters, int* available) {
  HookMem mem;
  GemmGlobalsGuard guard;
  // bits 0-4: the GEMM flags of the call; bits 8-11: GemmArgs::tri of its products (a TRI_* kind, + 8 = TRI_DIAG_LOWER) --
  // the caller then vouches for the operands it uploads
  if (flags >= 0) gpc::g_gemm_flags = flags & 0xff;
  const int tri = flags >= 0 ? (flags >> 8) & 15 : (int)TRI_NONE;
  if (block_slots > 0) {
    gpc::g_block_slots = block_slots;
    gpc::g_persist_spare = 0;
  }
  const unsigned short* rsv = nullptr;
  if (form == GPC_FORM_PERSIST_RESERVED) {
    rsv = ctx_reserve_tbl(c);
    if (!rsv) {
      *available = 0;
      return 0;
    }
  }
  *available = 1;
  GemmArgs g[2];
  T* dC[2] = {nullptr, nullptr};
  auto up = [&](const double* src, long long n, T** dst) -> int {
    HIPCHK(c, mem.get(reinterpret_cast<void**>(dst), (size_t)n * sizeof(T)));
    if constexpr (sizeof(T) == 8) {
      HIPCHK(c, hipMemcpyAsync(*dst, src, (size_t)n * 8, hipMemcpyHostToDevice, c->st));
      HIPCHK(c, hipStreamSynchronize(c->st));
    } else {
      std::vector<float> tmp((size_t)n);
      for (long long i = 0; i < n; ++i) tmp[(size_t)i] = (float)src[i];
      HIPCHK(c, hipMemcpyAsync(*dst, tmp.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->st));
      HIPCHK(c, hipStreamSynchronize(c->st));
    }
    return 0;
  };
  for (int i = 0; i < nprod; ++i) {
    const gpc_gemm_product& p = *prods[i];
    T *dA = nullptr, *dB = nullptr;
    if (up(p.A, p.size_a, &dA) || up(p.B, p.size_b, &dB) || up(p.C, p.size_c, &dC[i])) return -1;
    GemmArgs& a = g[i];
    a.A = dA + p.off_a;
    a.B = dB + p.off_b;
    a.C = dC[i] + p.off_c;
    a.sA = p.s_a;
    a.sB = p.s_b;
    a.sC = p.s_c;
    a.lda = p.lda;
    a.ldb = p.ldb;
    a.ldc = p.ldc;
    a.M = p.M;
    a.N = p.N;
    a.K = p.K;
    a.alpha = p.alpha;
    a.beta = p.beta;
    a.klo = p.klo;
    a.khi = p.khi;
    a.lower_only = p.lower_only ? 1 : 0;
    a.tri = tri;
  }
  int* ctr = nullptr;  // the hook's own CTR_STRIDE counters, zeroed
  HIPCHK(c, mem.get(reinterpret_cast<void**>(&ctr), CTR_STRIDE * sizeof(int)));
  HIPCHK(c, hipMemsetAsync(ctr, 0, CTR_STRIDE * sizeof(int), c->st));
  const gpc_gemm_product& p0 = *prods[0];
  const size_t ncolsq = (size_t)batch * (p0.M / TILE) * p0.N;
  double* dcolsq = nullptr;
  if (form == GPC_FORM_COLSQ || form == GPC_FORM_WSQ) {
    HIPCHK(c, mem.get(reinterpret_cast<void**>(&dcolsq), ncolsq * sizeof(double)));
    HIPCHK(c, hipMemsetAsync(dcolsq, 0xff, ncolsq * sizeof(double), c->st));  // NaN: an entry nobody wrote shows
    g[0].colsq = dcolsq;
  }
  if (form == GPC_FORM_WSQ) {
    double *dw = nullptr, *da = nullptr;
    const size_t nw = (size_t)(batch - 1) * ep_sw + p0.M;
    HIPCHK(c, mem.get(reinterpret_cast<void**>(&dw), nw * sizeof(double)));
    HIPCHK(c, mem.get(reinterpret_cast<void**>(&da), (size_t)batch * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(dw, ep_w, nw * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(da, ep_alpha, (size_t)batch * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    g[0].ep_w = dw;
    g[0].ep_sw = ep_sw;
    g[0].ep_alpha = da;
  }
  const bool akm = p0.a_kmajor != 0, bkm = p0.b_kmajor != 0;
  switch (form) {
    case GPC_FORM_PLAIN:
    case GPC_FORM_PERSIST:
    case GPC_FORM_PERSIST_RESERVED: {
      int* qc = form == GPC_FORM_PLAIN ? nullptr : ctr;
      if (tile == 64)
        HIPCHK(c, (launch_gemm_bt<T, 64, 4>(c->st, g[0], akm, bkm, batch, qc, rsv)));
      else
        HIPCHK(c, (launch_gemm_bt<T, 128, 4>(c->st, g[0], akm, bkm, batch, qc, rsv)));
      break;
    }
    case GPC_FORM_DUAL:
      HIPCHK(c, launch_gemm_dual_small<T>(c->st, g[0], g[1], batch));
      break;
    case GPC_FORM_COLSQ:
      HIPCHK(c, launch_gemm_colsq<T>(c->st, g[0], batch, ctr));
      break;
    default:
      HIPCHK(c, launch_gemm_wsq<T>(c->st, g[0], batch));
      break;
  }
  HIPCHK(c, hipStreamSynchronize(c->st));
  for (int i = 0; i < nprod; ++i)
    if (download_as<T>(c, dC[i], prods[i]->C, (size_t)prods[i]->size_c)) return -1;
  if (dcolsq) HIPCHK(c, hipMemcpy(colsq, dcolsq, ncolsq * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(counters, ctr, NQ * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

template <typename T>
int debug_factor_impl(gpc_ctx* c, int n, const double* A, double* L, double* W, double* Ainv,
                      double* logdet, int* info) {
  const int npad = pad_tile(n);
  const size_t msz = (size_t)npad * npad;
  HIPCHK(c, c->mA.ensure(msz * sizeof(T)));
  HIPCHK(c, c->mW.ensure(msz * sizeof(T)));
  HIPCHK(c, c->mT.ensure(msz * sizeof(T)));
  HIPCHK(c, c->dbg1.ensure((size_t)n * n * 8));
  HIPCHK(c, c->scal.ensure(64));
  HIPCHK(c, hipMemcpyAsync(c->dbg1.p, A, (size_t)n * n * 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(c, hipMemsetAsync(c->scal.p, 0, 64, c->st));
  dim3 blk(64, 4), gp(npad / 64, npad / 4);
  hipLaunchKernelGGL((pad_load_kernel<T>), gp, blk, 0, c->st, c->dbg1.as<double>(), n, npad, c->mA.as<T>());
  Factor<T> F;
  F.st = c->st;
  F.batch = 1;
  F.npad = npad;
  F.A = c->mA.as<T>();
  F.W = c->mW.as<T>();
  F.Tm = c->mT.as<T>();
  F.sA = F.sW = F.sT = (long long)msz;
  F.logdet = c->scal.as<double>();
  F.info = reinterpret_cast<int*>(c->scal.as<double>() + 1);
  F.nvalid = n;
  F.potrf_inv(0, npad, true, true);
  HIPCHK(c, F.err);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, c->dbg3.ensure((size_t)n * n * 8));
  dim3 gn((n + 63) / 64, (n + 3) / 4);
  if (L) {
    hipLaunchKernelGGL((extract_kernel<T>), gn, blk, 0, c->st, (const T*)F.A, npad, n, 0, c->dbg3.as<double>());
    HIPCHK(c, hipMemcpyAsync(L, c->dbg3.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
  }
  if (W) {
    hipLaunchKernelGGL((extract_kernel<T>), gn, blk, 0, c->st, (const T*)F.W, npad, n, 0, c->dbg3.as<double>());
    HIPCHK(c, hipMemcpyAsync(W, c->dbg3.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
  }
  if (Ainv) {
    F.lauum(F.Tm, F.sT);
    HIPCHK(c, F.err);
    hipLaunchKernelGGL((extract_kernel<T>), gn, blk, 0, c->st, (const T*)F.Tm, npad, n, 0, c->dbg3.as<double>());
    HIPCHK(c, hipMemcpyAsync(Ainv, c->dbg3.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
  }
  double h[2];
  HIPCHK(c, hipMemcpyAsync(h, c->scal.p, 16, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  if (logdet) *logdet = h[0];
  if (info) memcpy(info, &h[1], sizeof(int));
  return 0;
}

// gpc_debug_cov: the covariance kernels of the evaluation and prediction paths on one sample, launched as
// device_section / small_section / predict launch them (same scaling kernel, same grids), on buffers of its own.
struct ScratchDev {
  std::vector<void*> ps;
  ~ScratchDev() {
    for (void* p : ps) (void)hipFree(p);
  }
  template <typename U>
  U* get(size_t n) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(U)) != hipSuccess) return nullptr;
    ps.push_back(p);
    return static_cast<U*>(p);
  }
};

// gpc_debug_factor_plan: the plan of plan.h on a batch, in every mode the product runs it in (debug_factor_impl above
// runs one sample, fast mode, full inverse, keep_L).  The buffers are the caller's, cast and uploaded whole, and come
// back whole: what a launch reads outside the plan's contract is what the caller put there, what it writes shows.
template <typename T>
int debug_factor_plan_impl(gpc_ctx* c, int npad, int nvalid, int batch, int plan, int nll_block, int flags, double* A,
                           double* W, double* Tm, const double* r, double* z, double* Ainv, double* logdet, int* info) {
  const size_t msz = (size_t)npad * npad, tot = msz * batch, vtot = (size_t)npad * batch;
  ScratchDev sd;
  T* dA = sd.get<T>(tot);
  T* dW = sd.get<T>(tot);
  T* dT = sd.get<T>(tot);
  double* dld = sd.get<double>(batch);
  int* dinfo = sd.get<int>(batch);
  double* dr = r ? sd.get<double>(vtot) : nullptr;
  double* dz = r ? sd.get<double>(vtot) : nullptr;
  if (!dA || !dW || !dT || !dld || !dinfo || (r && (!dr || !dz))) FAIL(c, "gpc_debug_factor_plan: out of device memory");
  auto up = [&](T* dst, const double* src) -> int {
    std::vector<T> h(src, src + tot);  // a plain cast: a NaN stays a NaN
    HIPCHK(c, hipMemcpy(dst, h.data(), tot * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  };
  if (up(dA, A) || up(dW, W) || up(dT, Tm)) return -1;
  HIPCHK(c, hipMemsetAsync(dld, 0, batch * sizeof(double), c->st));
  HIPCHK(c, hipMemsetAsync(dinfo, 0, batch * sizeof(int), c->st));
  if (r) {
    HIPCHK(c, hipMemcpyAsync(dr, r, vtot * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemsetAsync(dz, 0xff, vtot * 8, c->st));  // NaN: an entry no launch wrote shows
  }
  Factor<T> F;
  F.st = c->st;
  F.batch = batch;
  F.npad = npad;
  F.nvalid = nvalid;
  F.A = dA;
  F.W = dW;
  F.Tm = dT;
  F.sA = F.sW = F.sT = (long long)msz;
  F.logdet = dld;
  F.info = dinfo;
  F.stable = (flags & 1) != 0;
  F.tri_skip = c->tri_skip != 0;
  const bool keep_L = (flags & 2) != 0;
  if (plan == 2) {
    F.nll_block = nll_block;
    F.potrf_nll(0, npad);
  } else {
    F.potrf_inv(0, npad, plan == 0, keep_L);
  }
  HIPCHK(c, F.err);
  HIPCHK(c, hipGetLastError());
  if (r) {
    if (plan == 2)
      F.forward_solve_nll(0, npad, dr, dz);
    else
      F.forward_solve(0, npad, plan == 0, dr, dz);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipStreamSynchronize(c->st));
  if (download_as<T>(c, dA, A, tot) || download_as<T>(c, dW, W, tot) || download_as<T>(c, dT, Tm, tot)) return -1;
  if (r) HIPCHK(c, hipMemcpy(z, dz, vtot * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(logdet, dld, batch * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(info, dinfo, batch * sizeof(int), hipMemcpyDeviceToHost));
  if (flags & 4) {
    F.lauum(F.Tm, F.sT);
    HIPCHK(c, F.err);
    HIPCHK(c, hipGetLastError());
    if (download_as<T>(c, dT, Ainv, tot)) return -1;
  }
  return 0;
}

template <typename T>
int debug_cov_impl(gpc_ctx* c, int which, CovDesc cd, const double* hyp, double kscale, double sl, const double* dvec,
                   const double* X, int N, const double* Xstar, int M, const double* mat, const double* vec,
                   double* out0, double* out1, double* xs_out) {
  hipStream_t st = c->st;
  const int D = cd.D, npad = pad_tile(N), mpad = M > 0 ? pad_tile(M) : 0, Pn = cd.cov_N + 1;
  const int t64 = npad / CT, ntl = t64 * (t64 + 1) / 2;
  std::vector<double> mul(D), dv(D), sp(SP_STRIDE, 0.0), hd(npad, 1.0), hv(npad, 0.0);
  double sf2 = 0.0, rqa = 1.0;
  scaling_of(cd.kind, cd.degree, D, hyp, mul.data(), dv.data(), &sf2, &rqa);
  sp[SP_SF2] = sf2;
  sp[SP_RQA] = rqa;
  sp[SP_KSCALE] = kscale;
  sp[SP_SL] = sl;
  if (dvec) std::copy(dvec, dvec + N, hd.begin());
  if (vec) std::copy(vec, vec + N, hv.begin());
  ScratchDev sd;
  double* dX = sd.get<double>((size_t)N * D);
  double* dmul = sd.get<double>(D);
  double* ddv = sd.get<double>(D);
  double* dsp = sd.get<double>(SP_STRIDE);
  double* dd = sd.get<double>(npad);
  double* dvv = sd.get<double>(npad);
  double* xs = sd.get<double>((size_t)npad * D);
  if (!dX || !dmul || !ddv || !dsp || !dd || !dvv || !xs) FAIL(c, "gpc_debug_cov: out of device memory");
  HIPCHK(c, hipMemcpyAsync(dX, X, (size_t)N * D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(dmul, mul.data(), (size_t)D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(ddv, dv.data(), (size_t)D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(dsp, sp.data(), SP_STRIDE * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(dd, hd.data(), (size_t)npad * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(dvv, hv.data(), (size_t)npad * 8, hipMemcpyHostToDevice, st));
  const long long tot = (long long)npad * D;
  if (which != 1)  // (the small front scales the inputs itself)
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)((tot + 255) / 256), 1), dim3(256), 0, st, (const double*)dX, N, npad,
                       D, (const double*)dmul, (const double*)ddv, xs);
  const size_t msz = (size_t)npad * npad;
  if (which == 0 || which == 1) {
    T* A = sd.get<T>(msz);
    if (!A) FAIL(c, "gpc_debug_cov: out of device memory");
    HIPCHK(c, hipMemsetAsync(A, 0, msz * sizeof(T), st));  // the tiles above the diagonal are not built
    if (which == 0) {
      GPC_COV_DISPATCH(build_kernel, T, cd, dim3(ntl, 1), dim3(256), 0, st, cd, (const double*)xs, (const double*)dsp,
                       (const double*)dd, N, npad, A, (long long)msz, npad, 0);
    } else {
      XferDesc u{};
      u.nseg = 0;
      u.X = dX;
      u.mul = dmul;
      u.dv = ddv;
      u.xs = xs;
      u.n = N;
      u.npad = npad;
      u.D = D;
      u.cnt = 1;
      GPC_COV_DISPATCH(small_front_kernel, T, cd, dim3(3, 1), dim3(256), 0, st, u, cd, (const double*)dsp,
                       (const double*)dd, 1, A, (long long)msz);
    }
    HIPCHK(c, hipGetLastError());
    if (download_as<T>(c, A, out0, msz)) return -1;
  } else if (which == 2) {
    double* dXq = sd.get<double>((size_t)M * D);
    double* xss = sd.get<double>((size_t)mpad * D);
    T* Ks = sd.get<T>((size_t)npad * mpad);
    double* mupart = sd.get<double>((size_t)t64 * mpad);
    double* mu = sd.get<double>(mpad);
    if (!dXq || !xss || !Ks || !mupart || !mu) FAIL(c, "gpc_debug_cov: out of device memory");
    HIPCHK(c, hipMemcpyAsync(dXq, Xstar, (size_t)M * D * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)mpad * D + 255) / 256), 1), dim3(256), 0, st,
                       (const double*)dXq, M, mpad, D, (const double*)dmul, (const double*)ddv, xss);
    GPC_COV_DISPATCH(cross_tile_kernel, T, cd, dim3(mpad / CT, npad / CT, 1), dim3(256), 0, st, cd, (const double*)xs,
                     (const double*)xss, (const double*)dsp, (const double*)dvv, npad, N, npad, M, mpad, Ks,
                     (long long)npad * mpad, mupart);
    hipLaunchKernelGGL(colpart_reduce_kernel, dim3((mpad + 255) / 256, 1), dim3(256), 0, st, (const double*)mupart, t64,
                       mpad, mu);
    HIPCHK(c, hipGetLastError());
    if (download_as<T>(c, Ks, out0, (size_t)npad * mpad)) return -1;
    HIPCHK(c, hipMemcpyAsync(out1, mu, (size_t)mpad * 8, hipMemcpyDeviceToHost, st));
    if (xs_out) HIPCHK(c, hipMemcpyAsync(xs_out + (size_t)npad * D, xss, (size_t)mpad * D * 8, hipMemcpyDeviceToHost, st));
  } else if (which == 4) {
    // the derivative operand as gpc_grad_post launches it: one launch per block of GQB queries.  out0: the panels,
    // [block][npad][(D + 1) GQB]; out1: the fused column sums against vec, [block][(D + 1) GQB]
    const int mb = GQB, ld = (D + 1) * mb, nblk = (M + mb - 1) / mb;
    const size_t psz = (size_t)npad * ld;
    double* dXq = sd.get<double>((size_t)M * D);
    double* xss = sd.get<double>((size_t)mb * D);
    T* P = sd.get<T>(psz);
    double* part = sd.get<double>((size_t)t64 * ld);
    double* sums = sd.get<double>(ld);
    double* f0 = sd.get<double>(1);
    if (!dXq || !xss || !P || !part || !sums || !f0) FAIL(c, "gpc_debug_cov: out of device memory");
    HIPCHK(c, hipMemcpyAsync(dXq, Xstar, (size_t)M * D * 8, hipMemcpyHostToDevice, st));
    for (int q = 0; q < nblk; ++q) {
      const int mq = std::min(mb, M - q * mb);
      hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)mb * D + 255) / 256), 1), dim3(256), 0, st,
                         (const double*)(dXq + (size_t)q * mb * D), mq, mb, D, (const double*)dmul, (const double*)ddv, xss);
      GPC_COV_DISPATCH(grad_operand_tile_kernel, T, cd, dim3(mb / CT, npad / CT, 1), dim3(256), 0, st, cd, (const double*)xs,
                       (const double*)xss, (const double*)dsp, (const double*)dmul, (const double*)ddv, (const double*)dvv,
                       npad, N, npad, mq, mb, P, (long long)psz, part, f0);
      hipLaunchKernelGGL(colpart_reduce_kernel, dim3((ld + 255) / 256, 1), dim3(256), 0, st, (const double*)part, t64, ld, sums);
      HIPCHK(c, hipGetLastError());
      if (download_as<T>(c, P, out0 + (size_t)q * psz, psz)) return -1;
      HIPCHK(c, hipMemcpyAsync(out1 + (size_t)q * ld, sums, (size_t)ld * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
    }
  } else {
    std::vector<double> hT(msz, 0.0);
    for (int i = 0; i < N; ++i) std::copy(mat + (size_t)i * N, mat + (size_t)i * N + N, hT.begin() + (size_t)i * npad);
    T* Tm = sd.get<T>(msz);
    double* parts = sd.get<double>((size_t)ntl * Pn);
    double* diagq = sd.get<double>(npad);
    double* gout = sd.get<double>(Pn);
    if (!Tm || !parts || !diagq || !gout) FAIL(c, "gpc_debug_cov: out of device memory");
    if constexpr (sizeof(T) == 8) {
      HIPCHK(c, hipMemcpyAsync(Tm, hT.data(), msz * 8, hipMemcpyHostToDevice, st));
    } else {
      std::vector<float> tmp(hT.begin(), hT.end());
      HIPCHK(c, hipMemcpyAsync(Tm, tmp.data(), msz * 4, hipMemcpyHostToDevice, st));
      HIPCHK(c, hipStreamSynchronize(st));
    }
    HIPCHK(c, hipMemsetAsync(diagq, 0, (size_t)npad * 8, st));
    GPC_COV_DISPATCH(trace_kernel, T, cd, dim3(ntl, 1), dim3(256), 4 * (((Pn + 3) & ~3) + 4) * sizeof(double), st, cd,
                     (const double*)xs, (const double*)dsp, (const double*)dvv, N, npad, (const T*)Tm, (long long)msz, npad,
                     parts, ntl, diagq);
    hipLaunchKernelGGL(grad_tail_kernel, dim3(Pn, 1), dim3(256), 0, st, (const double*)parts, ntl, Pn, gout,
                       (const double*)nullptr, N, 0, (const double*)dvv, (double*)nullptr, (const double*)nullptr, 0,
                       (const double*)diagq, (double*)nullptr, npad);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out0, gout, (size_t)Pn * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(out1, diagq, (size_t)npad * 8, hipMemcpyDeviceToHost, st));
  }
  if (xs_out) HIPCHK(c, hipMemcpyAsync(xs_out, xs, (size_t)npad * D * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return 0;
}
}  // namespace

// gpc_debug_block_gram: the block Gram kernel of gpc_grad_post on caller-provided panels
namespace {
template <typename T>
int debug_block_gram_impl(gpc_ctx* c, int n, int M, int Dp, const double* Y, const double* Z, bool diag, double* out) {
  hipStream_t st = c->st;
  const int mb = pad_tile(M), ld = Dp * mb, nseg = gram_segments(n);
  const size_t psz = (size_t)n * ld, gper = (size_t)mb * Dp * (diag ? 1 : Dp);
  // the caller's n x (Dp M) planes into planes of width mb (zero padding), in the storage type
  auto padded = [&](const double* src) {
    std::vector<T> h(psz, (T)0);
    for (int i = 0; i < n; ++i)
      for (int a = 0; a < Dp; ++a)
        for (int j = 0; j < M; ++j) h[(size_t)i * ld + (size_t)a * mb + j] = (T)src[((size_t)i * Dp + a) * M + j];
    return h;
  };
  ScratchDev sd;
  T* dY = sd.get<T>(psz);
  T* dZ = Z ? sd.get<T>(psz) : dY;
  double* part = sd.get<double>(nseg > 1 ? nseg * gper : 1);
  double* res = sd.get<double>(gper);
  if (!dY || !dZ || !part || !res) FAIL(c, "gpc_debug_block_gram: out of device memory");
  const std::vector<T> hY = padded(Y), hZ = Z ? padded(Z) : std::vector<T>();
  HIPCHK(c, hipMemcpy(dY, hY.data(), psz * sizeof(T), hipMemcpyHostToDevice));
  if (Z) HIPCHK(c, hipMemcpy(dZ, hZ.data(), psz * sizeof(T), hipMemcpyHostToDevice));
  HIPCHK(c, launch_block_gram<T>(st, dY, dZ, (long long)psz, n, mb, Dp, 1, diag, part, res));
  std::vector<double> h(gper);
  HIPCHK(c, hipMemcpyAsync(h.data(), res, gper * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  std::copy(h.begin(), h.begin() + (size_t)M * Dp * (diag ? 1 : Dp), out);
  return 0;
}
}  // namespace

// gpc_debug_hess_contract: the Hessian contraction of gpc_predict_hess (hess.h) on caller-provided weights, one launch
// per block of GQB queries as the product path; Q (optional): dense N x M, taken with factor 1
namespace {
template <typename T>
int debug_hess_impl(gpc_ctx* c, CovDesc cd, const double* hyp, const double* X, int N, const double* Xstar, int M,
                    const double* alpha, const double* Qd, double* out_a, double* out_q) {
  hipStream_t st = c->st;
  const int D = cd.D, npad = pad_tile(N), mb = GQB, nt64 = npad / CT, npl = hess_planes(D), nset = Qd ? 2 : 1;
  const size_t hper = (size_t)nset * npl * mb;
  std::vector<double> mul(D), dv(D), sp(SP_STRIDE, 0.0), hal(npad, 0.0);
  double sf2 = 0.0, rqa = 1.0;
  scaling_of(cd.kind, cd.degree, D, hyp, mul.data(), dv.data(), &sf2, &rqa);
  sp[SP_SF2] = sf2;
  sp[SP_RQA] = rqa;
  sp[SP_KSCALE] = 1.0;
  sp[SP_SL] = 1.0;  // (with lch = 1: Q is taken as it is)
  std::copy(alpha, alpha + N, hal.begin());
  ScratchDev sd;
  double* dX = sd.get<double>((size_t)N * D);
  double* dXq = sd.get<double>((size_t)M * D);
  double* dmul = sd.get<double>(D);
  double* ddv = sd.get<double>(D);
  double* dsp = sd.get<double>(SP_STRIDE);
  double* dal = sd.get<double>(npad);
  double* xs = sd.get<double>((size_t)npad * D);
  double* xss = sd.get<double>((size_t)mb * D);
  T* dQ = sd.get<T>((size_t)npad * mb);
  double* part = sd.get<double>((size_t)nt64 * hper);
  double* sums = sd.get<double>(hper);
  if (!dX || !dXq || !dmul || !ddv || !dsp || !dal || !xs || !xss || !dQ || !part || !sums)
    FAIL(c, "gpc_debug_hess_contract: out of device memory");
  HIPCHK(c, hipMemcpy(dX, X, (size_t)N * D * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dXq, Xstar, (size_t)M * D * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dmul, mul.data(), (size_t)D * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(ddv, dv.data(), (size_t)D * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dsp, sp.data(), SP_STRIDE * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dal, hal.data(), (size_t)npad * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)npad * D + 255) / 256), 1), dim3(256), 0, st,
                     (const double*)dX, N, npad, D, (const double*)dmul, (const double*)ddv, xs);
  std::vector<T> hQ((size_t)npad * mb);
  std::vector<double> h(hper);
  for (int q0 = 0; q0 < M; q0 += mb) {
    const int mq = std::min(mb, M - q0);
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)mb * D + 255) / 256), 1), dim3(256), 0, st,
                       (const double*)(dXq + (size_t)q0 * D), mq, mb, D, (const double*)dmul, (const double*)ddv, xss);
    if (Qd) {
      std::fill(hQ.begin(), hQ.end(), (T)0);
      for (int i = 0; i < N; ++i)
        for (int jj = 0; jj < mq; ++jj) hQ[(size_t)i * mb + jj] = (T)Qd[(size_t)i * M + q0 + jj];
      HIPCHK(c, hipMemcpy(dQ, hQ.data(), hQ.size() * sizeof(T), hipMemcpyHostToDevice));
      GPC_COV_DISPATCH(hess_tile_kernel, T, cd, dim3(mb / CT, npad / CT, 1), dim3(256), 0, st, cd, (const double*)xs,
                       (const double*)xss, (const double*)dsp, (const double*)dal, npad, (const T*)dQ,
                       (long long)npad * mb, mb, 1, N, npad, mq, mb, part);
    } else {
      GPC_COV_DISPATCH(hess_tile_mean_kernel, T, cd, dim3(mb / CT, npad / CT, 1), dim3(256), 0, st, cd, (const double*)xs,
                       (const double*)xss, (const double*)dsp, (const double*)dal, npad, N, npad, mq, mb, part);
    }
    hipLaunchKernelGGL(colpart_reduce_kernel, dim3((unsigned)((hper + 255) / 256), 1), dim3(256), 0, st,
                       (const double*)part, nt64, (int)hper, sums);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h.data(), sums, hper * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int jj = 0; jj < mq; ++jj)
      for (int p = 0; p < npl; ++p) {
        out_a[(size_t)(q0 + jj) * npl + p] = h[(size_t)p * mb + jj];
        if (Qd) out_q[(size_t)(q0 + jj) * npl + p] = h[(size_t)(npl + p) * mb + jj];
      }
  }
  return 0;
}
}  // namespace

// gpc_debug_hyp_cross: the fused cross pass of gpc_predict_hyp_grad (hypgrad.h) on caller-provided weights, one launch
// over all queries; Q (optional): dense N x M, taken with factor 1; without it the mean-only kernel runs
namespace {
int debug_hyp_cross_impl(gpc_ctx* c, CovDesc cd, const double* hyp, const double* X, int N, const double* Xstar, int M,
                         const double* alpha, const double* Wv, int P, const double* Qd, double* out) {
  hipStream_t st = c->st;
  const int D = cd.D, npad = pad_tile(N), mpad = pad_tile(M), nt = npad / CT;
  const int nout = hg_cross_sums(P, cd.cov_N, Qd != nullptr);
  std::vector<double> mul(D), dv(D), sp(SP_STRIDE, 0.0), hal(npad, 0.0), hW((size_t)P * npad, 0.0);
  double sf2 = 0.0, rqa = 1.0;
  scaling_of(cd.kind, cd.degree, D, hyp, mul.data(), dv.data(), &sf2, &rqa);
  sp[SP_SF2] = sf2;
  sp[SP_RQA] = rqa;
  sp[SP_KSCALE] = 1.0;
  sp[SP_SL] = 1.0;
  std::copy(alpha, alpha + N, hal.begin());
  for (int p = 0; p < P; ++p) std::copy(Wv + (size_t)p * N, Wv + (size_t)(p + 1) * N, hW.begin() + (size_t)p * npad);
  ScratchDev sd;
  double* dX = sd.get<double>((size_t)N * D);
  double* dXq = sd.get<double>((size_t)M * D);
  double* dmul = sd.get<double>(D);
  double* ddv = sd.get<double>(D);
  double* dsp = sd.get<double>(SP_STRIDE);
  double* dal = sd.get<double>(npad);
  double* dW = sd.get<double>((size_t)P * npad);
  double* xs = sd.get<double>((size_t)npad * D);
  double* xss = sd.get<double>((size_t)mpad * D);
  double* dQ = sd.get<double>((size_t)npad * mpad);
  double* dqs = sd.get<double>(1);
  double* part = sd.get<double>((size_t)nt * nout * mpad);
  double* sums = sd.get<double>((size_t)nout * mpad);
  if (!dX || !dXq || !dmul || !ddv || !dsp || !dal || !dW || !xs || !xss || !dQ || !dqs || !part || !sums)
    FAIL(c, "gpc_debug_hyp_cross: out of device memory");
  const double one = 1.0;
  HIPCHK(c, hipMemcpy(dX, X, (size_t)N * D * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dXq, Xstar, (size_t)M * D * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dmul, mul.data(), (size_t)D * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(ddv, dv.data(), (size_t)D * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dsp, sp.data(), SP_STRIDE * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dal, hal.data(), (size_t)npad * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dW, hW.data(), hW.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dqs, &one, 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)npad * D + 255) / 256), 1), dim3(256), 0, st,
                     (const double*)dX, N, npad, D, (const double*)dmul, (const double*)ddv, xs);
  hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)mpad * D + 255) / 256), 1), dim3(256), 0, st,
                     (const double*)dXq, M, mpad, D, (const double*)dmul, (const double*)ddv, xss);
  if (Qd) {
    std::vector<double> hQ((size_t)npad * mpad, 0.0);
    for (int i = 0; i < N; ++i) std::copy(Qd + (size_t)i * M, Qd + (size_t)(i + 1) * M, hQ.begin() + (size_t)i * mpad);
    HIPCHK(c, hipMemcpy(dQ, hQ.data(), hQ.size() * 8, hipMemcpyHostToDevice));
    GPC_COV_DISPATCH(hg_cross_kernel, double, cd, dim3(mpad / CT, npad / CT, 1), dim3(256), 0, st, cd, (const double*)xs,
                     (const double*)xss, (const double*)dsp, (const double*)dal, (const double*)dW, P, (const double*)dQ,
                     (long long)npad * mpad, mpad, (const double*)dqs, N, npad, M, mpad, part);
  } else {
    GPC_COV_DISPATCH(hg_cross_mean_kernel, double, cd, dim3(mpad / CT, npad / CT, 1), dim3(256), 0, st, cd, (const double*)xs,
                     (const double*)xss, (const double*)dsp, (const double*)dal, (const double*)dW, P, N, npad, M, mpad, part);
  }
  hipLaunchKernelGGL(colpart_reduce_kernel, dim3((unsigned)(((size_t)nout * mpad + 255) / 256), 1), dim3(256), 0, st,
                     (const double*)part, nt, nout * mpad, sums);
  HIPCHK(c, hipGetLastError());
  std::vector<double> h((size_t)nout * mpad);
  HIPCHK(c, hipMemcpyAsync(h.data(), sums, h.size() * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  for (int j = 0; j < M; ++j)
    for (int o = 0; o < nout; ++o) out[(size_t)j * nout + o] = h[(size_t)o * mpad + j];
  return 0;
}
}  // namespace

namespace {
// The posterior's storage regrown to npn padded rows: A and W copied with identity padding, alpha with zeros.  The
// old buffers go to the context's pool (the next gpc_posterior_batch reuses them) or back to the device.
template <typename T>
int grow_storage(gpc_post* po, int npn, bool to_pool) {
  gpc_ctx* c = po->ctx;
  hipStream_t st = c->st;
  const int S = po->S, np = po->npad;
  DevBuf nA, nW, nal;
  HIPCHK(c, nA.ensure((size_t)S * npn * npn * sizeof(T)));
  HIPCHK(c, nW.ensure((size_t)S * npn * npn * sizeof(T)));
  HIPCHK(c, nal.ensure((size_t)S * npn * sizeof(double)));
  dim3 g(npn / 64, npn / 4, S), blk(64, 4);
  hipLaunchKernelGGL((grow_copy_kernel<T>), g, blk, 0, st, (const T*)po->A.as<T>(), np, nA.as<T>(), npn);
  hipLaunchKernelGGL((grow_copy_kernel<T>), g, blk, 0, st, (const T*)po->W.as<T>(), np, nW.as<T>(), npn);
  HIPCHK(c, hipMemsetAsync(nal.p, 0, (size_t)S * npn * sizeof(double), st));
  HIPCHK(c, hipMemcpy2DAsync(nal.p, (size_t)npn * 8, po->alpha.p, (size_t)np * 8, (size_t)np * 8, S,
                             hipMemcpyDeviceToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));
  for (DevBuf* b : {&po->A, &po->W, &po->alpha}) {
    if (to_pool)
      c->pool_give(*b);
    else
      b->release();
  }
  po->A = nA;
  po->W = nW;
  po->alpha = nal;
  po->npad = npn;
  return 0;
}

// rank-one append (scalar noise; checked by the caller): high-noise samples get a new last row
// of the factor and of its inverse (:776-817), low-noise samples a rank-one update of -inv (:819-827)
// Ks_h / kss_h: the cross covariances and prior variances at the new point from the caller's own covariance object
// (K-mode posteriors); nullptr: built on the device from the posterior's kernel
template <typename T>
int append_impl(gpc_post* po, const double* m_star, const double* sn2_star, double y_new, int* ok,
                const double* Ks_h = nullptr, const double* kss_h = nullptr) {
  gpc_ctx* c = po->ctx;
  const int S = po->S, D = po->D, n = po->N;  // the new point is row n of the context's X
  hipStream_t st = c->st;
  if (c->N != n + 1) FAIL(c, "gpc_post_append: call gpc_set_data with the extended X, y first");
  // grow the padded storage by one tile when the new row does not fit
  if (n + 1 > po->npad)
    if (int rc = grow_storage<T>(po, po->npad + TILE, true)) return rc;
  const int npad = po->npad;
  const long long sM = (long long)npad * npad;
  const size_t vb = (size_t)npad * 8;
  HIPCHK(c, c->xs.ensure((size_t)S * npad * D * 8));
  HIPCHK(c, c->spb.ensure((size_t)S * SP_STRIDE * 8));
  HIPCHK(c, c->mulb.ensure((size_t)S * D * 8));
  HIPCHK(c, c->divb.ensure((size_t)S * D * 8));
  HIPCHK(c, c->rvec.ensure(S * vb));
  HIPCHK(c, c->zvec.ensure(S * vb));
  HIPCHK(c, c->avec.ensure(S * vb));
  HIPCHK(c, c->tpart.ensure((size_t)S * (npad / TRC + 1) * vb));
  HIPCHK(c, c->scal.ensure((size_t)S * 10 * 8));
  HIPCHK(c, hipMemcpyAsync(c->spb.p, po->sp.data(), (size_t)S * SP_STRIDE * 8, hipMemcpyHostToDevice, st));
  if (!Ks_h) {
    HIPCHK(c, hipMemcpyAsync(c->mulb.p, po->mul.data(), (size_t)S * D * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->divb.p, po->dv.data(), (size_t)S * D * 8, hipMemcpyHostToDevice, st));
    const long long tot = (long long)npad * D;
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)((tot + 255) / 256), S), dim3(256), 0, st,
                       c->dX.as<double>(), n + 1, npad, D, c->mulb.as<double>(), c->divb.as<double>(),
                       c->xs.as<double>());
  }
  double* ks = c->rvec.as<double>();  // Ks
  double* lv = c->zvec.as<double>();  // l = W Ks
  double* au = c->avec.as<double>();  // W^T l
  double* d_ll = c->scal.as<double>();
  double* d_ka = d_ll + S;
  if (Ks_h) {  // rows of n values, zero beyond (the padding rows of W are identity rows)
    HIPCHK(c, hipMemsetAsync(ks, 0, S * vb, st));
    HIPCHK(c, hipMemcpy2DAsync(ks, vb, Ks_h, (size_t)n * 8, (size_t)n * 8, S, hipMemcpyHostToDevice, st));
  } else {
    hipLaunchKernelGGL(cross_vec_kernel, dim3((npad + 255) / 256, S), dim3(256), 0, st, po->cd,
                       c->xs.as<double>(), c->spb.as<double>(), n, npad, ks);
  }
  hipLaunchKernelGGL((trmv_kernel<T>), dim3(npad / 4, S), dim3(256), 0, st, (const T*)po->W.as<T>(), sM, npad,
                     (const double*)ks, npad, lv, 0);
  hipLaunchKernelGGL(dot_kernel, dim3(1, S), dim3(256), 0, st, (const double*)lv, (const double*)lv, n, npad, d_ll);
  hipLaunchKernelGGL(dot_kernel, dim3(1, S), dim3(256), 0, st, (const double*)ks,
                     (const double*)po->alpha.as<double>(), n, npad, d_ka);
  // the padding rows of W are identity rows: l[i >= n] = Ks[i] = 0, harmless in W^T l
  double* tpart = c->tpart.as<double>();
  hipLaunchKernelGGL((trmv_t_part_kernel<T>), dim3((npad + 64 * MM<T>::VEC - 1) / (64 * MM<T>::VEC), npad / TRC, S), dim3(256), 0, st,
                     (const T*)po->W.as<T>(), sM, npad, (const double*)lv, npad, tpart, (double*)nullptr);
  hipLaunchKernelGGL(trmv_t_sum_kernel, dim3(npad / 128, S), dim3(128), 0, st, (const double*)tpart, npad,
                     (const double*)nullptr, 0, 0, au);
  HIPCHK(c, hipGetLastError());
  // low-noise samples (Posterior.L = -(K + Sigma)^-1, a FULL symmetric matrix; :819-827):
  //   au = -L Ks,  Ks.au (-> predictive variance),  per sample (their W is not used)
  double* au_low = c->dvec.as<double>();
  double* d_kau = d_ka + S;
  HIPCHK(c, c->dvec.ensure(S * vb));
  au_low = c->dvec.as<double>();
  bool any_low = false;
  for (int s = 0; s < S; ++s) {
    if (po->lchol[s]) continue;
    any_low = true;
    HIPCHK(c, hipMemsetAsync(au_low + (size_t)s * npad, 0, vb, st));
    hipLaunchKernelGGL((gemv_sub_kernel<T>), dim3(npad / 4, 1), dim3(256), 0, st,
                       (const T*)(po->A.as<T>() + (size_t)s * sM), 0ll, npad, (const double*)(ks + (size_t)s * npad),
                       au_low + (size_t)s * npad, npad, 0, 0, npad);
  }
  if (any_low)
    hipLaunchKernelGGL(dot_kernel, dim3(1, S), dim3(256), 0, st, (const double*)ks, (const double*)au_low, n, npad,
                       d_kau);
  HIPCHK(c, hipGetLastError());
  std::vector<double> ll(S), ka(S), kau(S, 0.0), coef((size_t)S * 5);
  HIPCHK(c, hipMemcpyAsync(ll.data(), d_ll, S * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(ka.data(), d_ka, S * 8, hipMemcpyDeviceToHost, st));
  if (any_low) HIPCHK(c, hipMemcpyAsync(kau.data(), d_kau, S * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  for (int s = 0; s < S; ++s) {
    const double sf2 = kss_h ? kss_h[s] : po->sp[(size_t)s * SP_STRIDE + SP_SF2];  // k(x_new, x_new)
    const double sl = po->sp[(size_t)s * SP_STRIDE + SP_SL];  // = sn2 * sn2_mult of the fitted noise (L_chol)
    const double sn2_eff = sn2_star[s] * po->mult[s];
    const double mu_star = m_star[s] + ka[s];  // predictive mean at the new point
    double* cf = &coef[(size_t)s * 5];
    ok[s] = 0;
    if (po->info[s] != 0 || ((c->append_fail_mask >> (s & 31)) & 1u)) continue;
    if (po->lchol[s]) {
      // gaussian_process.py:784-788 (K = kss = sf2)
      const double sqrt_arg = sn2_eff * sn2_eff + sf2 * sn2_eff - ll[s];
      if (!(sqrt_arg > 0.0 && std::abs(sn2_eff - sl) <= 1e-12 * sl)) continue;
      const double dl = std::sqrt(sqrt_arg) / sn2_eff;   // new diagonal entry of the factor (:814)
      const double v_star = sf2 - ll[s] / sl + sn2_eff;  // predictive variance incl. noise (:756)
      cf[0] = 1.0 / sn2_eff;                             // Lo[n][:n] = l / sn2_eff  (:811)
      cf[1] = dl;
      cf[2] = -1.0 / (dl * sn2_eff);                     // W[n][:n] = -(l/sn2_eff)^T W / dl
      cf[3] = (mu_star - y_new) / v_star;                // alpha update weight (:842)
      cf[4] = 1.0 / sn2_eff;                             // alpha_update = W^T l / sn2_eff (:800-808)
    } else {
      // s2 = kss + Ks.(L Ks) = sf2 - Ks.au, clamped at 0 (:1762-1770), plus the noise (:1779)
      const double v_star = std::max(sf2 - kau[s], 0.0) + sn2_eff;
      cf[0] = 1.0 / v_star;                // v = -au / v_star (:821); new L = [[L + v au^T, -v], [-v^T, -1/v_star]]
      cf[3] = (mu_star - y_new) / v_star;  // alpha += cf3 * au, alpha[n] = -cf3 (:840-844)
    }
    ok[s] = 1;
  }
  double* d_coef = c->scal.as<double>() + 3 * S;
  HIPCHK(c, hipMemcpyAsync(d_coef, coef.data(), coef.size() * 8, hipMemcpyHostToDevice, st));
  // Samples that cannot be appended keep their old rows: the caller recomputes them on the grown
  // storage (gpc_post_recompute) -- the reference's per-posterior fallback (:789-798, :866-869).
  for (int s = 0; s < S; ++s) {
    if (!ok[s]) continue;
    if (po->lchol[s])
      hipLaunchKernelGGL((append_row_kernel<T>), dim3((n + 256) / 256, 1), dim3(256), 0, st,
                         po->A.as<T>() + (size_t)s * sM, po->W.as<T>() + (size_t)s * sM, sM, npad, n,
                         (const double*)(lv + (size_t)s * npad), (const double*)(au + (size_t)s * npad), npad,
                         (const double*)(d_coef + (size_t)s * 5), po->alpha.as<double>() + (size_t)s * npad);
    else
      hipLaunchKernelGGL((append_low_kernel<T>), dim3((n + 64) / 64, (n + 4) / 4), dim3(64, 4), 0, st,
                         po->A.as<T>() + (size_t)s * sM, npad, n, (const double*)(au_low + (size_t)s * npad),
                         (const double*)(d_coef + (size_t)s * 5), po->alpha.as<double>() + (size_t)s * npad);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(st));
  po->N = n + 1;
  po->dev_consts = false;
  return 0;
}

// Block append of k points (block_append.h has the algebra and the kernels).  Everything per sample is decided on
// the device; `ok` comes back in one download of the Schur factorizations' info.
// Ks_h (S x n x k) / Kss_h (S x k x k): the caller's cross covariances (K-mode posteriors); nullptr: built on the device.
template <typename T>
int append_block_impl(gpc_post* po, int k, const double* m_star, const double* sn2_star, const double* y_new, int* ok,
                      const double* Ks_h = nullptr, const double* Kss_h = nullptr) {
  gpc_ctx* c = po->ctx;
  const int S = po->S, D = po->D, n = po->N;  // the new points are rows n .. n+k-1 of the context's X
  hipStream_t st = c->st;
  const int npn = pad_tile(n + k);
  const int kq = ((k + BA_R - 1) / BA_R) * BA_R, kp = pad_tile(k);
  const bool use_gemm = c->block_engine ? c->block_engine == 2 : k >= BA_GEMM_MIN_K;
  c->block_engine_ran = use_gemm ? 2 : 1;
  const int np_scr = std::max(npn, po->npad);  // the padded size after the growth below
  const size_t per = ScratchCarver::count<AppendScratch<T>>(1, np_scr, kq, kp, use_gemm);
  const bool grow = npn > po->npad;
  const size_t grow_bytes = grow ? (size_t)S * npn * ((size_t)npn * 2 * sizeof(T) + 8) : 0;
  // the scratch is the consumers' block: kept between calls, so that an acquisition loop pays no allocation per
  // batch; budgeted like gpc_predict_cov's when it has to grow
  const size_t held = c->cs.bytes;
  // (a forced budget plans on every call, pool_drain included: it is the tests' way into the chunked path, not a
  // setting for an acquisition loop, which without it allocates only when the scratch or the storage grows.
  // GPC_MEM_BUDGET_MB budgets the SCRATCH; the device's real free memory has to hold the grown storage as well)
  const int chunk = plan_chunk(c, S, per, 0, held, (size_t)S * per <= held && !grow, grow_bytes, false, [&](size_t budget) {
    return "gpc_post_append_block: the scratch of one sample (" + std::to_string(per >> 10) + " KB: N_pad = " +
           std::to_string(npn) + ", k = " + std::to_string(k) + ") exceeds the device memory budget (" +
           std::to_string(budget >> 10) + " KB" +
           (grow ? " beside " + std::to_string(grow_bytes >> 10) + " KB of grown storage)" : ")");
  });
  if (!chunk) return -2;
  // grow the padded storage by as many tiles as the k rows need (the old storage goes back to the device: the scratch
  // was budgeted beside the grown one)
  if (grow)
    if (int rc = grow_storage<T>(po, npn, false)) return rc;
  const int npad = po->npad;
  const long long sM = (long long)npad * npad;
  const long long sP = (long long)npad * kq;
  // per-sample parameters and the preconditions the host can decide: a factorized sample, the fitted scalar noise
  std::vector<double> par((size_t)S * BA_STRIDE);
  for (int s = 0; s < S; ++s) {
    const double sl = po->sp[(size_t)s * SP_STRIDE + SP_SL];
    const double sn2_eff = sn2_star[s] * po->mult[s];
    bool pre = po->info[s] == 0 && !((c->append_fail_mask >> (s & 31)) & 1u) && sn2_eff > 0.0;
    if (po->lchol[s]) pre = pre && std::abs(sn2_eff - sl) <= 1e-12 * sl;
    par[(size_t)s * BA_STRIDE + BA_SL] = sl;
    par[(size_t)s * BA_STRIDE + BA_SN2] = sn2_eff;
    par[(size_t)s * BA_STRIDE + BA_LCH] = po->lchol[s] ? 1.0 : 0.0;
    par[(size_t)s * BA_STRIDE + BA_PRE] = pre ? 1.0 : 0.0;
  }
  HIPCHK(c, c->spb.ensure((size_t)S * SP_STRIDE * 8));
  HIPCHK(c, c->avec.ensure((size_t)S * BA_STRIDE * 8));
  HIPCHK(c, c->rvec.ensure(((size_t)S * k + k) * 8));
  HIPCHK(c, c->scal.ensure((size_t)S * 16));
  double* d_par = c->avec.as<double>();
  double* d_ms = c->rvec.as<double>();
  double* d_y = d_ms + (size_t)S * k;
  double* d_logdet = c->scal.as<double>();
  int* d_info = reinterpret_cast<int*>(d_logdet + S);
  HIPCHK(c, hipMemcpyAsync(c->spb.p, po->sp.data(), (size_t)S * SP_STRIDE * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_par, par.data(), par.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_ms, m_star, (size_t)S * k * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_y, y_new, (size_t)k * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(c->scal.p, 0, (size_t)S * 16, st));
  if (!Ks_h) {
    HIPCHK(c, c->xs.ensure((size_t)S * npad * D * 8));
    HIPCHK(c, c->mulb.ensure((size_t)S * D * 8));
    HIPCHK(c, c->divb.ensure((size_t)S * D * 8));
    HIPCHK(c, hipMemcpyAsync(c->mulb.p, po->mul.data(), (size_t)S * D * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->divb.p, po->dv.data(), (size_t)S * D * 8, hipMemcpyHostToDevice, st));
    const long long tot = (long long)npad * D;
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)((tot + 255) / 256), S), dim3(256), 0, st, c->dX.as<double>(),
                       n + k, npad, D, c->mulb.as<double>(), c->divb.as<double>(), c->xs.as<double>());
  }
  HIPCHK(c, c->cs.ensure((size_t)chunk * per));
  AppendScratch<T> z;
  bool any_high = false, any_low = false;
  for (int s = 0; s < S; ++s) (po->lchol[s] ? any_high : any_low) = true;
  // gpc_last_timing: device time of the call (after the growth) and of the skinny products (the last chunk's)
  c->ms_total = c->ms_factor = 0;
  CallTimer tm{c, true};
  HIPCHK(c, tm.start());
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    CARVECHK(c, "gpc_post_append_block", ScratchCarver::carve(z, c->cs.p, cnt, npad, kq, kp, use_gemm));
    HIPCHK(c, hipMemsetAsync(c->cs.p, 0, (size_t)cnt * per, st));
    double *const Bx = z.Bx, *const V = z.V, *const Pt = z.Pt, *const GS = z.GS, *const Cm = z.Cm;
    double *const ev = z.ev, *const tv = z.tv, *const zv = z.zv;
    T *const fA = z.fA, *const fW = z.fW, *const fT = z.fT, *const Bt = z.Bt, *const Vt = z.Vt, *const Qt = z.Qt;
    const double* parc = d_par + (size_t)s0 * BA_STRIDE;
    T* Ac = po->A.as<T>() + (size_t)s0 * sM;
    T* Wc = po->W.as<T>() + (size_t)s0 * sM;
    double* alc = po->alpha.as<double>() + (size_t)s0 * npad;
    // 1. cross covariances
    if (Ks_h) {
      for (int i = 0; i < cnt; ++i) {
        HIPCHK(c, hipMemcpy2DAsync(Bx + (size_t)i * sP, (size_t)kq * 8, Ks_h + (size_t)(s0 + i) * n * k, (size_t)k * 8,
                                   (size_t)k * 8, n, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpy2DAsync(Bx + (size_t)i * sP + (size_t)n * kq, (size_t)kq * 8,
                                   Kss_h + (size_t)(s0 + i) * k * k, (size_t)k * 8, (size_t)k * 8, k,
                                   hipMemcpyHostToDevice, st));
      }
    } else {
      hipLaunchKernelGGL(ba_cross_kernel, dim3((unsigned)((sP + 255) / 256), cnt), dim3(256), 0, st, po->cd,
                         (const double*)(c->xs.as<double>() + (size_t)s0 * npad * D),
                         (const double*)(c->spb.as<double>() + (size_t)s0 * SP_STRIDE), n, k, npad, kq, Bx);
    }
    // 2. the skinny products and the k x k Gram matrices
    const dim3 gn((n + BA_T - 1) / BA_T, kq / BA_R, cnt), gk((k + BA_T - 1) / BA_T, kq / BA_R, cnt);
    HIPCHK(c, tm.mark1());
    if (use_gemm) {
      // the same products as launches of the MFMA GEMM on panels padded to 128 columns, in runs of one parametrisation
      const long long sK = (long long)npad * kp;
      hipLaunchKernelGGL((ba_to_panel_kernel<T>), dim3(kp / 64, npad / 4, cnt), dim3(64, 4), 0, st, (const double*)Bx, n, k,
                         kq, npad, kp, Bt);
      const int rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
        GemmArgs g = tri_product_args<T>(po, s0 + a, lch, Bt + (size_t)a * sK, Vt + (size_t)a * sK, sK, kp, kp);  // V = W B | G = -A B
        g.alpha = lch ? 1.0 : -1.0;
        g.tiles_n = kp / TILE;
        HIPCHK(c, launch_gemm<T>(st, g, false, true, len));
        if (lch) {  // Q = W^T V (k from the tile row's diagonal block on)
          HIPCHK(c, launch_gemm<T>(st, wt_product_args(g, Vt + (size_t)a * sK, Qt + (size_t)a * sK), true, true, len));
        }
        return 0;
      });
      if (rc_runs) return rc_runs;
      const dim3 gf((n + 63) / 64, kq / 4, cnt);
      for (int want = 0; want < 2; ++want) {
        if (!(want ? any_high : any_low)) continue;
        hipLaunchKernelGGL((ba_from_panel_kernel<T>), gf, dim3(64, 4), 0, st, (const T*)Vt, n, kq, npad, kp, 0, parc, want, V);
        if (want)
          hipLaunchKernelGGL((ba_from_panel_kernel<T>), gf, dim3(64, 4), 0, st, (const T*)Qt, n, kq, npad, kp, 1, parc, 1, Pt);
        hipLaunchKernelGGL((ba_skinny_kernel<double, true, false, false>), gk, dim3(256), 0, st,
                           (const double*)(want ? V : Bx), sP, kq, n, k, (const double*)V, sP, kq, Cm, (long long)kq * kq, kq,
                           1.0, 0, parc, want);
      }
    } else {
    if (any_high) {
      hipLaunchKernelGGL((ba_skinny_kernel<T, false, true, false>), gn, dim3(256), 0, st, (const T*)Wc, sM, npad, n, n,
                         (const double*)Bx, sP, kq, V, sP, kq, 1.0, 0, parc, 1);
      hipLaunchKernelGGL((ba_skinny_kernel<double, true, false, false>), gk, dim3(256), 0, st, (const double*)V, sP, kq, n,
                         k, (const double*)V, sP, kq, Cm, (long long)kq * kq, kq, 1.0, 0, parc, 1);
      hipLaunchKernelGGL((ba_skinny_kernel<T, true, true, true>), gn, dim3(256), 0, st, (const T*)Wc, sM, npad, n, n,
                         (const double*)V, sP, kq, Pt, sP, npad, 1.0, 1, parc, 1);
    }
    if (any_low) {
      hipLaunchKernelGGL((ba_skinny_kernel<T, false, false, false>), gn, dim3(256), 0, st, (const T*)Ac, sM, npad, n, n,
                         (const double*)Bx, sP, kq, V, sP, kq, -1.0, 0, parc, 0);
      hipLaunchKernelGGL((ba_skinny_kernel<double, true, false, false>), gk, dim3(256), 0, st, (const double*)Bx, sP, kq,
                         n, k, (const double*)V, sP, kq, Cm, (long long)kq * kq, kq, 1.0, 0, parc, 0);
    }
    }
    HIPCHK(c, tm.mark2());
    // 3. Schur complement, its factor and inverse factor: the blocked factorization, no jitter
    hipLaunchKernelGGL((ba_schur_kernel<T>), dim3(kp / 64, kp / 4, cnt), dim3(64, 4), 0, st, (const double*)Bx, sP, n, k,
                       kq, (const double*)Cm, parc, kp, fA);
    HIPCHK(c, hipGetLastError());
    Factor<T> F;
    F.st = st;
    F.batch = cnt;
    F.npad = kp;
    F.A = fA;
    F.W = fW;
    F.Tm = fT;
    F.sA = F.sW = F.sT = (long long)kp * kp;
    F.logdet = d_logdet + s0;
    F.info = d_info + s0;
    F.nvalid = k;
    F.potrf_inv(0, kp, true, true);
    HIPCHK(c, F.err);
    HIPCHK(c, hipGetLastError());
    const int* infoc = d_info + s0;
    // 4. the new alpha and the new rows, placed where the factorization succeeded
    hipLaunchKernelGGL(ba_innov_kernel, dim3(k, cnt), dim3(256), 0, st, (const double*)Bx, sP, n, kq, (const double*)alc,
                       npad, (const double*)d_y, (const double*)(d_ms + (size_t)s0 * k), k, ev);
    hipLaunchKernelGGL((ba_small_vec_kernel<T>), dim3(cnt), dim3(256), 0, st, (const T*)fW, kp, k, kq, (const double*)ev,
                       tv, zv);
    hipLaunchKernelGGL(ba_alpha_kernel, dim3((npad + 255) / 256, cnt), dim3(256), 0, st, alc, npad, n, k, kq,
                       (const double*)Pt, (const double*)V, (const double*)zv, parc, infoc);
    if (any_high)
      hipLaunchKernelGGL((ba_place_high_kernel<T>), dim3((npad + 255) / 256, k, cnt), dim3(256), 0, st, Ac, Wc, sM, npad,
                         n, k, kq, kp, (const double*)V, (const double*)Pt, (const T*)fA, (const T*)fW, parc, infoc);
    if (any_low) {
      const dim3 gp((unsigned)(((long long)n * k + 255) / 256), cnt);
      hipLaunchKernelGGL((ba_panel_w22_kernel<T>), gp, dim3(256), 0, st, (const double*)V, Pt, sP, n, k, kq,
                         (const T*)fW, kp, 0, parc);
      hipLaunchKernelGGL((ba_panel_w22_kernel<T>), gp, dim3(256), 0, st, (const double*)Pt, GS, sP, n, k, kq,
                         (const T*)fW, kp, 1, parc);
      hipLaunchKernelGGL((ba_place_low_kernel<T>), dim3((n + k + 63) / 64, (n + k + 15) / 16, cnt), dim3(64, 4), 0, st,
                         Ac, sM, npad, n, k, kq, kp, (const double*)V, (const double*)GS, (const T*)fW, parc, infoc);
    }
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, tm.stop());
  std::vector<int> info(S);
  HIPCHK(c, hipMemcpyAsync(info.data(), d_info, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  tm.accumulate();  // (one span over all chunks; the products' time is the last chunk's)
  for (int s = 0; s < S; ++s) {
    ok[s] = (par[(size_t)s * BA_STRIDE + BA_PRE] != 0.0 && info[s] == 0) ? 1 : 0;
    ++(ok[s] ? c->block_appended : c->block_stale);
  }
  po->N = n + k;
  po->dev_consts = false;
  return 0;
}

int append_block_check(gpc_post* po, int k, const char* fn) {
  gpc_ctx* c = po->ctx;
  const std::string f(fn);
  if (k < 1) FAIL(c, f + ": k must be at least 1");
  if ((long long)po->N + k > gpc_max_n(po->dtype))
    FAIL(c, f + ": N + k = " + std::to_string((long long)po->N + k) + " exceeds gpc_max_n = " +
            std::to_string(gpc_max_n(po->dtype)));
  if (c->N != po->N + k) FAIL(c, f + ": call gpc_set_data with the extended X, y (N + k rows) first");
  return 0;
}

// ---- removal of k points (remove.h has the algebra and the kernels) ------------------------------------------------

// One sweep: the kk <= RM_KMAX sorted rows idx[] leave a posterior of po->N rows.  New storage at the padded size of
// n = N - kk (pool first), the old one to the pool.  dead[s] != 0: the sample is stale already and is only compacted;
// a low-noise sample whose Q_II does not factorize becomes dead.  d_par: the samples' parameters (block_append.h).
template <typename T>
int remove_sweep(gpc_post* po, int kk, const int* idx, int chunk, std::vector<double>& par, std::vector<int>& dead,
                 bool timed, double& sweep_ms) {
  gpc_ctx* c = po->ctx;
  hipStream_t st = c->st;
  const int S = po->S, No = po->N, n = No - kk, ldo = po->npad, npn = pad_tile(n);
  const int kq = rm_kq(kk), kp = pad_tile(kk), mp = RM_P + kq;
  const long long sMo = (long long)ldo * ldo, sMn = (long long)npn * npn, sV = (long long)npn * kq;
  const size_t per = ScratchCarver::count<RmScratch<T>>(1, npn, kq, kp);
  // the kept rows, and the panel that holds the first removed one (in the compacted numbering)
  std::vector<int> maps((size_t)npn + kk, -1);
  for (int i = 0, r = 0, j = 0; r < No; ++r) {
    if (j < kk && idx[j] == r) ++j;
    else maps[i++] = r;
  }
  std::copy_n(idx, kk, maps.begin() + npn);
  const int a0 = (idx[0] / RM_P) * RM_P;
  for (int s = 0; s < S; ++s) par[(size_t)s * BA_STRIDE + BA_PRE] = dead[s] ? 0.0 : 1.0;
  DevBuf nA = c->pool_take((size_t)S * sMn * sizeof(T)), nW = c->pool_take((size_t)S * sMn * sizeof(T)),
         nal = c->pool_take((size_t)S * npn * sizeof(double));
  std::vector<hipEvent_t> evs;  // around the panel loop of every chunk (timed calls)
  auto fail = [&](int rc) {
    for (DevBuf* b : {&nA, &nW, &nal}) b->release();
    for (hipEvent_t e : evs) (void)hipEventDestroy(e);
    return rc;
  };
  auto mark = [&]() -> hipError_t {
    if (!timed) return hipSuccess;
    hipEvent_t e;
    if (hipError_t rc = hipEventCreate(&e)) return rc;
    evs.push_back(e);
    return hipEventRecord(e, st);
  };
#define RM_CHK(expr)                                                  \
  do {                                                                \
    hipError_t _e = (expr);                                           \
    if (_e != hipSuccess) {                                           \
      c->err = std::string(#expr) + ": " + hipGetErrorString(_e);     \
      return fail(-1);                                                \
    }                                                                 \
  } while (0)
  RM_CHK(nA.ensure((size_t)S * sMn * sizeof(T)));
  RM_CHK(nW.ensure((size_t)S * sMn * sizeof(T)));
  RM_CHK(nal.ensure((size_t)S * npn * sizeof(double)));
  RM_CHK(c->cs.ensure((size_t)chunk * per + maps.size() * sizeof(int)));
  RM_CHK(c->dvec.ensure((size_t)S * BA_STRIDE * 8));
  RM_CHK(c->scal.ensure((size_t)S * 16));
  double* d_par = c->dvec.as<double>();
  double* d_logdet = c->scal.as<double>();
  int* d_info = reinterpret_cast<int*>(d_logdet + S);
  int* const d_rmap = reinterpret_cast<int*>(c->cs.as<char>() + (size_t)chunk * per);
  const int* d_idx = d_rmap + npn;
  // (pageable sources: the copies are staged before the calls return)
  RM_CHK(hipMemcpy(d_rmap, maps.data(), maps.size() * sizeof(int), hipMemcpyHostToDevice));
  RM_CHK(hipMemcpy(d_par, par.data(), par.size() * 8, hipMemcpyHostToDevice));
  RM_CHK(hipMemsetAsync(c->scal.p, 0, (size_t)S * 16, st));
  bool any_high = false, any_low = false;
  for (int s = 0; s < S; ++s)
    if (!dead[s]) (po->lchol[s] ? any_high : any_low) = true;
  RmScratch<T> z;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    if (ScratchCarver::carve(z, c->cs.p, cnt, npn, kq, kp) != 0) {
      c->err = "gpc_post_remove: internal error: a scratch array is misaligned";
      return fail(-1);
    }
    const double* parc = d_par + (size_t)s0 * BA_STRIDE;
    const T* Ao = po->A.as<T>() + (size_t)s0 * sMo;
    const T* Wo = po->W.as<T>() + (size_t)s0 * sMo;
    const double* alo = po->alpha.as<double>() + (size_t)s0 * ldo;
    T* An = nA.as<T>() + (size_t)s0 * sMn;
    T* Wn = nW.as<T>() + (size_t)s0 * sMn;
    double* aln = nal.as<double>() + (size_t)s0 * npn;
    // 1. compaction and the carriers
    hipLaunchKernelGGL((rm_compact_kernel<T>), dim3(npn / 64, npn / 4, cnt), dim3(64, 4), 0, st, Ao, Wo, sMo, ldo, An, Wn,
                       sMn, npn, n, d_rmap, parc);
    hipLaunchKernelGGL((rm_carrier_kernel<T>), dim3((unsigned)((sV + 255) / 256), cnt), dim3(256), 0, st, Ao, Wo, sMo, ldo,
                       n, kk, kq, npn, d_rmap, d_idx, parc, z.V, z.C);
    hipLaunchKernelGGL(rm_alpha_gather_kernel, dim3((npn + 255) / 256, cnt), dim3(256), 0, st, alo, ldo, aln, npn, n,
                       d_rmap);
    RM_CHK(hipGetLastError());
    // 2. high noise: the sweep, two launches per panel, stream-ordered
    RM_CHK(mark());
    if (any_high) {
      for (int a = a0; a < n; a += RM_P) {
        hipLaunchKernelGGL((rm_panel_kernel<T>), dim3(cnt), dim3(256), 0, st, An, sMn, npn, a, z.V, sV, kq, z.Th, parc);
        const int nLb = std::max(0, (n - (a + RM_P) + 63) / 64), nWb = (n + 63) / 64;
        hipLaunchKernelGGL((rm_apply_kernel<T>), dim3(nLb + nWb, cnt), dim3(256), 0, st, An, Wn, sMn, npn, n, a, z.V, z.C,
                           sV, npn, kq, (const double*)z.Th, nLb, parc);
      }
      RM_CHK(hipGetLastError());
    }
    RM_CHK(mark());
    // 3. low noise: Q_II through the blocked factorization (no jitter), the correction while compacting
    if (any_low) {
      hipLaunchKernelGGL((rm_qii_kernel<T>), dim3(kp / 64, kp / 4, cnt), dim3(64, 4), 0, st, Ao, sMo, ldo, kk, kq, kp,
                         d_idx, parc, alo, ldo, z.fA, z.aI);
      RM_CHK(hipGetLastError());
      Factor<T> F;
      F.st = st;
      F.batch = cnt;
      F.npad = kp;
      F.A = z.fA;
      F.W = z.fW;
      F.Tm = z.fT;
      F.sA = F.sW = F.sT = (long long)kp * kp;
      F.logdet = d_logdet + s0;
      F.info = d_info + s0;
      F.nvalid = kk;
      F.potrf_inv(0, kp, true, true);
      RM_CHK(F.err);
      RM_CHK(hipGetLastError());
      const int* infoc = d_info + s0;
      hipLaunchKernelGGL((ba_small_vec_kernel<T>), dim3(cnt), dim3(256), 0, st, (const T*)z.fW, kp, kk, kq,
                         (const double*)z.aI, z.tv, z.zv);
      hipLaunchKernelGGL(rm_alpha_low_kernel, dim3((n + 255) / 256, cnt), dim3(256), 0, st, aln, npn, n, kk, kq,
                         (const double*)z.V, (const double*)z.zv, parc, infoc);
      hipLaunchKernelGGL((ba_panel_w22_kernel<T>), dim3((unsigned)(((long long)n * kk + 255) / 256), cnt), dim3(256), 0, st,
                         (const double*)z.V, z.H, sV, n, kk, kq, (const T*)z.fW, kp, 0, parc);
      hipLaunchKernelGGL((rm_low_kernel<T>), dim3((n + 63) / 64, (n + 15) / 16, cnt), dim3(64, 4), 0, st, Ao, sMo, ldo, An,
                         sMn, npn, n, kk, kq, d_rmap, (const double*)z.H, parc, infoc);
      RM_CHK(hipGetLastError());
    }
  }
  std::vector<int> info(S, 0);
  RM_CHK(hipMemcpyAsync(info.data(), d_info, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, st));
  RM_CHK(hipStreamSynchronize(st));
#undef RM_CHK
  for (size_t i = 0; i + 1 < evs.size(); i += 2) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, evs[i], evs[i + 1]);
    sweep_ms += ms;
  }
  for (hipEvent_t e : evs) (void)hipEventDestroy(e);
  for (int s = 0; s < S; ++s)
    if (!po->lchol[s] && info[s] != 0) dead[s] = 1;
  for (DevBuf* b : {&po->A, &po->W, &po->alpha}) c->pool_give(*b);
  po->A = nA;
  po->W = nW;
  po->alpha = nal;
  po->npad = npn;
  po->N = n;
  return 0;
}

// the scratch of one sample in the largest sweep of a removal of k rows from N
template <typename T>
size_t remove_per_sample(int N, int k) {
  const int kk = std::min(k, RM_KMAX);
  return ScratchCarver::count<RmScratch<T>>(1, pad_tile(N - kk), rm_kq(kk), pad_tile(kk));
}

template <typename T>
int remove_impl(gpc_post* po, int k, const int* idx, const double* ym, int* ok) {
  gpc_ctx* c = po->ctx;
  hipStream_t st = c->st;
  const int S = po->S, nfin = po->N - k;
  // every sweep's scratch is bounded by the first one's (the most rows, and k or RM_KMAX removed rows)
  const size_t per = remove_per_sample<T>(po->N, k);
  const int np1 = pad_tile(po->N - std::min(k, RM_KMAX));
  const size_t new_bytes = (size_t)S * np1 * ((size_t)np1 * 2 * sizeof(T) + 8);
  // (shared: the row maps of a sweep)
  const size_t shared = ((size_t)np1 + std::min(k, RM_KMAX)) * sizeof(int), held = c->cs.bytes;
  const int chunk = plan_chunk(c, S, per, shared, held, shared + (size_t)S * per <= held, new_bytes, false, [&](size_t budget) {
    return "gpc_post_remove: the scratch of one sample (" + std::to_string(per >> 10) + " KB: N_pad = " +
           std::to_string(np1) + ", k = " + std::to_string(k) + ") exceeds the device memory budget (" +
           std::to_string(budget >> 10) + " KB beside " + std::to_string(new_bytes >> 10) + " KB of compacted storage)";
  });
  if (!chunk) return -2;
  std::vector<double> par((size_t)S * BA_STRIDE, 0.0);
  std::vector<int> dead(S, 0);
  for (int s = 0; s < S; ++s) {
    par[(size_t)s * BA_STRIDE + BA_SL] = po->sp[(size_t)s * SP_STRIDE + SP_SL];
    par[(size_t)s * BA_STRIDE + BA_LCH] = po->lchol[s] ? 1.0 : 0.0;
    dead[s] = (po->info[s] != 0 || ((c->remove_fail_mask >> (s & 31)) & 1u)) ? 1 : 0;
  }
  // gpc_last_timing: device time of the call, and of the panel loops alone, summed over the chunks and the sweeps
  c->ms_total = c->ms_factor = 0;
  CallTimer tm{c, true};
  double sweep_ms = 0;
  HIPCHK(c, tm.start());
  HIPCHK(c, tm.mark1());
  HIPCHK(c, tm.mark2());
  std::vector<int> grp(RM_KMAX);
  for (int j0 = 0; j0 < k; j0 += RM_KMAX) {  // the rows before a group are gone by the time it is removed
    const int kk = std::min(RM_KMAX, k - j0);
    for (int j = 0; j < kk; ++j) grp[j] = idx[j0 + j] - j0;
    if (int rc = remove_sweep<T>(po, kk, grp.data(), chunk, par, dead, tm.on, sweep_ms)) return rc;
  }
  po->dev_consts = false;
  // alpha of the high-noise samples from the new factor: W'^T (W' (y_R - m_R)) / sl
  const int npad = po->npad;
  const long long sM = (long long)npad * npad;
  const size_t vb = (size_t)npad * 8;
  bool any_high = false;
  for (int s = 0; s < S; ++s) any_high = any_high || (po->lchol[s] && !dead[s]);
  if (any_high) {
    HIPCHK(c, c->rvec.ensure(S * vb));
    HIPCHK(c, c->zvec.ensure(S * vb));
    HIPCHK(c, c->avec.ensure(S * vb));
    HIPCHK(c, c->tpart.ensure((size_t)S * (npad / TRC + 1) * vb));
    double* r = c->rvec.as<double>();
    double* lv = c->zvec.as<double>();
    double* au = c->avec.as<double>();
    double* tpart = c->tpart.as<double>();
    HIPCHK(c, hipMemsetAsync(r, 0, S * vb, st));
    HIPCHK(c, hipMemcpy2DAsync(r, vb, ym, (size_t)nfin * 8, (size_t)nfin * 8, S, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((trmv_kernel<T>), dim3(npad / 4, S), dim3(256), 0, st, (const T*)po->W.as<T>(), sM, npad,
                       (const double*)r, npad, lv, 0);
    hipLaunchKernelGGL((trmv_t_part_kernel<T>), dim3((npad + 64 * MM<T>::VEC - 1) / (64 * MM<T>::VEC), npad / TRC, S),
                       dim3(256), 0, st, (const T*)po->W.as<T>(), sM, npad, (const double*)lv, npad, tpart, (double*)nullptr);
    hipLaunchKernelGGL(trmv_t_sum_kernel, dim3(npad / 128, S), dim3(128), 0, st, (const double*)tpart, npad,
                       (const double*)nullptr, 0, 0, au);
    hipLaunchKernelGGL(rm_alpha_high_kernel, dim3((npad + 255) / 256, S), dim3(256), 0, st, po->alpha.as<double>(), npad,
                       nfin, (const double*)au, (const double*)c->dvec.as<double>());
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, tm.stop());
  HIPCHK(c, hipStreamSynchronize(st));
  tm.accumulate();
  c->ms_factor = sweep_ms;
  for (int s = 0; s < S; ++s) {
    ok[s] = dead[s] ? 0 : 1;
    ++(ok[s] ? c->points_removed : c->remove_stale);
  }
  return 0;
}

// gpc_debug_remove_panel / gpc_debug_remove_apply: the two kernels of the sweep alone, on buffers of their own laid out
// as remove_sweep lays them out (storage in T, carriers and Theta in fp64)
template <typename T>
int debug_remove_panel_impl(gpc_ctx* c, int k, const double* D, const double* Vp, double* Theta, double* Dnew) {
  const int kq = rm_kq(k), mp = RM_P + kq, m = RM_P + k;
  ScratchDev sd;
  T* dA = sd.get<T>(RM_P * RM_P);
  double* dV = sd.get<double>((size_t)RM_P * kq);
  double* dTh = sd.get<double>((size_t)mp * mp);
  double* dpar = sd.get<double>(BA_STRIDE);
  if (!dA || !dV || !dTh || !dpar) FAIL(c, "gpc_debug_remove_panel: out of device memory");
  std::vector<T> hA(D, D + RM_P * RM_P);
  std::vector<double> hV((size_t)RM_P * kq, 0.0), hTh((size_t)mp * mp);
  for (int r = 0; r < RM_P; ++r) std::copy_n(Vp + (size_t)r * k, k, &hV[(size_t)r * kq]);
  const double par[BA_STRIDE] = {1.0, 0.0, 1.0, 1.0};
  HIPCHK(c, hipMemcpy(dA, hA.data(), hA.size() * sizeof(T), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dV, hV.data(), hV.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dpar, par, sizeof(par), hipMemcpyHostToDevice));
  hipLaunchKernelGGL((rm_panel_kernel<T>), dim3(1), dim3(256), 0, c->st, dA, (long long)RM_P * RM_P, RM_P, 0, dV,
                     (long long)RM_P * kq, kq, dTh, (const double*)dpar);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->st));
  HIPCHK(c, hipMemcpy(hTh.data(), dTh, hTh.size() * 8, hipMemcpyDeviceToHost));
  for (int i = 0; i < m; ++i) std::copy_n(&hTh[(size_t)i * mp], m, Theta + (size_t)i * m);
  return download_as<T>(c, dA, Dnew, (size_t)RM_P * RM_P);
}

// which = 0: P = L[a+64 : n, a : a+64] ((n - a - 64) x 64), Cr = V[a+64 : n, :k];  which = 1: P = W[a : a+64, :n]
// (64 x n; what lies above the diagonal is neither read nor written), Cr = C (k x n)
template <typename T>
int debug_remove_apply_impl(gpc_ctx* c, int which, int a, int n, int k, const double* Theta, double* P, double* Cr) {
  const int kq = rm_kq(k), mp = RM_P + kq, m = RM_P + k, ld = pad_tile(std::max(n, a + RM_P));
  const size_t msz = (size_t)ld * ld, vsz = (size_t)ld * kq;
  const int rows = n - a - RM_P;
  ScratchDev sd;
  T* dM = sd.get<T>(msz);
  double* dV = sd.get<double>(vsz);
  double* dTh = sd.get<double>((size_t)mp * mp);
  double* dpar = sd.get<double>(BA_STRIDE);
  if (!dM || !dV || !dTh || !dpar) FAIL(c, "gpc_debug_remove_apply: out of device memory");
  std::vector<T> hM(msz, (T)0);
  std::vector<double> hV(vsz, 0.0), hTh((size_t)mp * mp, 0.0);
  for (int i = 0; i < mp; ++i) hTh[(size_t)i * mp + i] = 1.0;
  for (int i = 0; i < m; ++i) std::copy_n(Theta + (size_t)i * m, m, &hTh[(size_t)i * mp]);
  if (which == 0) {
    for (int r = 0; r < rows; ++r) {
      for (int q = 0; q < RM_P; ++q) hM[(size_t)(a + RM_P + r) * ld + a + q] = (T)P[(size_t)r * RM_P + q];
      std::copy_n(Cr + (size_t)r * k, k, &hV[(size_t)(a + RM_P + r) * kq]);
    }
  } else {
    for (int q = 0; q < RM_P; ++q)
      for (int l = 0; l < n; ++l) hM[(size_t)(a + q) * ld + l] = (T)P[(size_t)q * n + l];
    for (int j = 0; j < k; ++j) std::copy_n(Cr + (size_t)j * n, n, &hV[(size_t)j * ld]);
  }
  const double par[BA_STRIDE] = {1.0, 0.0, 1.0, 1.0};
  HIPCHK(c, hipMemcpy(dM, hM.data(), msz * sizeof(T), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dV, hV.data(), vsz * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dTh, hTh.data(), hTh.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dpar, par, sizeof(par), hipMemcpyHostToDevice));
  const int nLb = which == 0 ? (rows + 63) / 64 : 0, nWb = which == 0 ? 0 : (n + 63) / 64;
  hipLaunchKernelGGL((rm_apply_kernel<T>), dim3(nLb + nWb, 1), dim3(256), 0, c->st, dM, dM, (long long)msz, ld, n, a, dV, dV,
                     (long long)vsz, ld, kq, (const double*)dTh, nLb, (const double*)dpar);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->st));
  std::vector<double> oM(msz);
  if (int rc = download_as<T>(c, dM, oM.data(), msz)) return rc;
  HIPCHK(c, hipMemcpy(hV.data(), dV, vsz * 8, hipMemcpyDeviceToHost));
  if (which == 0) {
    for (int r = 0; r < rows; ++r) {
      for (int q = 0; q < RM_P; ++q) P[(size_t)r * RM_P + q] = oM[(size_t)(a + RM_P + r) * ld + a + q];
      std::copy_n(&hV[(size_t)(a + RM_P + r) * kq], k, Cr + (size_t)r * k);
    }
  } else {
    for (int q = 0; q < RM_P; ++q)
      for (int l = 0; l < n; ++l) P[(size_t)q * n + l] = oM[(size_t)(a + q) * ld + l];
    for (int j = 0; j < k; ++j) std::copy_n(&hV[(size_t)j * ld], n, Cr + (size_t)j * n);
  }
  return 0;
}
}  // namespace


// ---- cross-validation (cv.h; DESIGN.md "Cross-validation") --------------------------------------------------------
namespace {

// per-sample parameters of the kernels of cv.h (block_append.h's layout), uploaded into c->avec
int cv_upload_par(gpc_post* po, double** d_par) {
  gpc_ctx* c = po->ctx;
  const int S = po->S;
  std::vector<double> par((size_t)S * BA_STRIDE, 0.0);
  for (int s = 0; s < S; ++s) {
    par[(size_t)s * BA_STRIDE + BA_SL] = po->sp[(size_t)s * SP_STRIDE + SP_SL];
    par[(size_t)s * BA_STRIDE + BA_LCH] = po->lchol[s] ? 1.0 : 0.0;
    par[(size_t)s * BA_STRIDE + BA_PRE] = 1.0;
  }
  HIPCHK(c, c->avec.ensure((size_t)S * BA_STRIDE * 8));
  // (pageable source: the copy is staged before the call returns)
  HIPCHK(c, hipMemcpy(c->avec.p, par.data(), par.size() * 8, hipMemcpyHostToDevice));
  *d_par = c->avec.as<double>();
  return 0;
}

// Leave-one-out: cv_diag_kernel over the samples of a chunk, five planes of N_pad per sample and nothing else.
// All outputs are N x S.
template <typename T>
int cv_loo_impl(gpc_post* po, double* dmu, double* s2, double* quad, double* logdet, int* info) {
  gpc_ctx* c = po->ctx;
  hipStream_t st = c->st;
  const int S = po->S, N = po->N, npad = po->npad;
  const long long sM = (long long)npad * npad;
  c->cv_engine_ran = 0;
  const size_t per = ScratchCarver::count<CvLooScratch>(1, npad);
  const int chunk = plan_chunk(c, S, per, 0, c->cs.bytes, (size_t)S * per <= c->cs.bytes, 0, false, [&](size_t budget) {
    return "gpc_cv: the scratch of one sample (" + std::to_string(per >> 10) + " KB: N_pad = " + std::to_string(npad) +
           ", F = 0, k_max = 1) exceeds the device memory budget (" + std::to_string(budget >> 10) + " KB)";
  });
  if (!chunk) return -2;
  double* d_par = nullptr;
  if (int rc = cv_upload_par(po, &d_par)) return rc;
  HIPCHK(c, c->cs.ensure((size_t)chunk * per));
  CvLooScratch z;
  std::unique_ptr<double[]> spare;
  c->pin.begin();
  double* h = landing_block(c, (size_t)chunk * per, spare);
  c->ms_total = c->ms_factor = 0;
  CallTimer tm{c, true};
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    const size_t pl = (size_t)cnt * npad;
    CARVECHK(c, "gpc_cv", ScratchCarver::carve(z, c->cs.p, cnt, npad));
    double* const d = z.dmu;  // (the five planes are one block: one download)
    HIPCHK(c, tm.start());
    HIPCHK(c, tm.mark1());
    hipLaunchKernelGGL((cv_diag_kernel<T>), dim3((N + CV_T - 1) / CV_T, cnt), dim3(256), 0, st,
                       (const T*)(po->A.as<T>() + (size_t)s0 * sM), (const T*)(po->W.as<T>() + (size_t)s0 * sM), sM, npad, N,
                       (const double*)(po->alpha.as<double>() + (size_t)s0 * npad),
                       (const double*)(d_par + (size_t)s0 * BA_STRIDE), z.dmu, z.s2, z.quad, z.logdet, z.info);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, tm.mark2());
    HIPCHK(c, tm.stop());
    HIPCHK(c, hipMemcpyAsync(h, d, 5 * pl * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    tm.accumulate();
    scatter_plane(dmu, h, N, npad, S, s0, cnt);
    scatter_plane(s2, h + pl, N, npad, S, s0, cnt);
    if (quad) scatter_plane(quad, h + 2 * pl, N, npad, S, s0, cnt);
    if (logdet) scatter_plane(logdet, h + 3 * pl, N, npad, S, s0, cnt);
    if (info) {
      const int* hi = reinterpret_cast<const int*>(h + 4 * pl);
      for (int i = 0; i < N; ++i)
        for (int q = 0; q < cnt; ++q) info[(size_t)i * S + s0 + q] = hi[(size_t)q * npad + i];
    }
  }
  return 0;
}

// Folds of more than one point: Gram (or gather) -> one batched fp64 factorization of all (sample, fold) pairs of the
// chunk -> epilogue.  fold_ptr / fold_idx have been validated.
template <typename T>
int cv_fold_impl(gpc_post* po, int F, const int* fold_ptr, const int* fold_idx, double* dmu, double* s2, double* quad,
                 double* logdet, int* info) {
  gpc_ctx* c = po->ctx;
  hipStream_t st = c->st;
  const int S = po->S, N = po->N, npad = po->npad;
  const long long sM = (long long)npad * npad;
  int kmax = 0;
  for (int f = 0; f < F; ++f) kmax = std::max(kmax, fold_ptr[f + 1] - fold_ptr[f]);
  const int kp = pad_tile(kmax), total = fold_ptr[F];
  const int engine = c->cv_engine ? c->cv_engine : CV_DEFAULT_ENGINE;
  c->cv_engine_ran = engine;
  const size_t kk = (size_t)kp * kp;
  // scratch of one sample: G, its inverse factor and the factorization's third slab for every fold, the vectors u, the
  // two output planes, [quad | logdet | ld | info] per fold, and engine 2's gathered panels
  const size_t per = ScratchCarver::count<CvFoldScratch>(1, npad, F, kp, engine == 2);
  int chunk = plan_chunk(c, S, per, 0, c->cs.bytes, (size_t)S * per <= c->cs.bytes, 0, false, [&](size_t budget) {
    return "gpc_cv: the scratch of one sample (" + std::to_string(per >> 10) + " KB: N_pad = " + std::to_string(npad) +
           ", F = " + std::to_string(F) + ", k_max = " + std::to_string(kmax) + ") exceeds the device memory budget (" +
           std::to_string(budget >> 10) + " KB)";
  });
  if (!chunk) return -2;
  chunk = std::min(chunk, 65535 / F);  // (sample, fold) pairs are one grid dimension of the batched launches
  double* d_par = nullptr;
  if (int rc = cv_upload_par(po, &d_par)) return rc;
  HIPCHK(c, c->rvec.ensure((size_t)(F + 1 + total) * sizeof(int)));
  int* d_ptr = c->rvec.as<int>();
  int* d_idx = d_ptr + F + 1;
  HIPCHK(c, hipMemcpy(d_ptr, fold_ptr, (size_t)(F + 1) * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(d_idx, fold_idx, (size_t)total * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(c, c->cs.ensure((size_t)chunk * per));
  CvFoldScratch z;
  const size_t out_doubles = 2 * (size_t)chunk * npad + 4 * (size_t)chunk * F;
  std::unique_ptr<double[]> spare;
  c->pin.begin();
  double* h = landing_block(c, out_doubles * 8, spare);
  c->ms_total = c->ms_factor = 0;
  CallTimer tm{c, true};
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0), np = cnt * F;
    CARVECHK(c, "gpc_cv", ScratchCarver::carve(z, c->cs.p, cnt, npad, F, kp, engine == 2));
    double *const G = z.G, *const Wf = z.Wf, *const Tm = z.Tm, *const panel = z.panel, *const uv = z.uv;
    double *const o_dmu = z.o_dmu, *const o_s2 = z.o_s2, *const o_quad = z.o_quad, *const o_logdet = z.o_logdet;
    double* const d_ld = z.ld;
    int* const d_info = z.info;
    HIPCHK(c, tm.start());
    HIPCHK(c, hipMemsetAsync(G, 0, 3 * (size_t)np * kk * 8, st));
    HIPCHK(c, hipMemsetAsync(o_dmu, 0xff, 2 * (size_t)cnt * npad * 8, st));  // NaN: points in no fold
    HIPCHK(c, hipMemsetAsync(o_quad, 0, 4 * (size_t)np * 8, st));            // (ld and info start from zero)
    const double* parc = d_par + (size_t)s0 * BA_STRIDE;
    const double* alc = po->alpha.as<double>() + (size_t)s0 * npad;
    HIPCHK(c, tm.mark1());
    const int tk = kp / CV_T;
    const int rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
      double* Gr = G + (size_t)a * F * kk;
      if (!lch) {
        hipLaunchKernelGGL((cv_gather_low_kernel<T>), dim3(tk * (kp / 4), F, len), dim3(64, 4), 0, st,
                           (const T*)(po->A.as<T>() + (size_t)(s0 + a) * sM), sM, npad, F, (const int*)d_ptr,
                           (const int*)d_idx, kp, Gr);
      } else if (engine == 1) {
        hipLaunchKernelGGL((cv_gram_kernel<T>), dim3(tk * (tk + 1) / 2, F, len), dim3(256), 0, st,
                           (const T*)(po->W.as<T>() + (size_t)(s0 + a) * sM), sM, npad, N, F, (const int*)d_ptr,
                           (const int*)d_idx, kp, Gr);
      } else {
        double* pr = panel + (size_t)a * F * npad * kp;
        for (int i = 0; i < len; ++i)  // (F blocks in z per launch)
          hipLaunchKernelGGL((cv_panel_kernel<T>), dim3(kp / 64, npad / 4, F), dim3(64, 4), 0, st,
                             (const T*)(po->W.as<T>() + (size_t)(s0 + a + i) * sM), sM, npad, N, F, (const int*)d_ptr,
                             (const int*)d_idx, kp, pr + (size_t)i * F * npad * kp);
        GemmArgs g;
        g.A = pr, g.B = pr, g.C = Gr;
        g.sA = g.sB = (long long)npad * kp, g.sC = (long long)kk;
        g.lda = g.ldb = g.ldc = kp;
        g.M = g.N = kp, g.K = npad;
        g.alpha = 1.0, g.beta = 0;
        g.klo = KLO_ZERO, g.khi = KHI_FULL, g.lower_only = 1;
        HIPCHK(c, launch_gemm<double>(st, g, true, true, len * F));
        hipLaunchKernelGGL(cv_pad_diag_kernel, dim3(F, len), dim3(256), 0, st, F, (const int*)d_ptr, kp, Gr);
      }
      HIPCHK(c, hipGetLastError());
      return 0;
    });
    if (rc_runs) return rc_runs;
    HIPCHK(c, tm.mark2());
    // one batched factorization of every (sample, fold) operand: factor and inverse factor, no jitter
    Factor<double> Fc;
    Fc.st = st;
    Fc.batch = np;
    Fc.npad = kp;
    Fc.A = G;
    Fc.W = Wf;
    Fc.Tm = Tm;
    Fc.sA = Fc.sW = Fc.sT = (long long)kk;
    Fc.logdet = d_ld;
    Fc.info = d_info;
    Fc.nvalid = kmax;
    Fc.potrf_inv(0, kp, true, true);
    HIPCHK(c, Fc.err);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(cv_fold_u_kernel, dim3(tk, F, cnt), dim3(256), 0, st, (const double*)Wf, kp, F, (const int*)d_ptr,
                       (const int*)d_idx, alc, npad, uv);
    hipLaunchKernelGGL(cv_fold_out_kernel, dim3(tk, F, cnt), dim3(256), 0, st, (const double*)Wf, kp, F, (const int*)d_ptr,
                       (const int*)d_idx, (const double*)uv, parc, (const double*)d_ld, (const int*)d_info, npad, o_dmu,
                       o_s2, o_quad, o_logdet);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, tm.stop());
    const size_t nd = 2 * (size_t)cnt * npad + 4 * (size_t)np;
    HIPCHK(c, hipMemcpyAsync(h, o_dmu, nd * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    tm.accumulate();
    const double* hq = h + 2 * (size_t)cnt * npad;
    const int* hi = reinterpret_cast<const int*>(hq + 3 * (size_t)np);
    for (int i = 0; i < np; ++i)
      if (hi[i] & LEAF_TIMEOUT) {
        c->err = "gpc_cv: internal error: a leaf of the factorization timed out";
        return -3;
      }
    scatter_plane(dmu, h, N, npad, S, s0, cnt);
    scatter_plane(s2, h + (size_t)cnt * npad, N, npad, S, s0, cnt);
    if (quad) scatter_plane(quad, hq, F, F, S, s0, cnt);
    if (logdet) scatter_plane(logdet, hq + np, F, F, S, s0, cnt);
    if (info)
      for (int f = 0; f < F; ++f)
        for (int q = 0; q < cnt; ++q) info[(size_t)f * S + s0 + q] = hi[(size_t)q * F + f];
  }
  return 0;
}

}  // namespace


// ---- pathwise posterior samples (paths.h; DESIGN.md "Pathwise samples") -------------------------------------------
namespace {

hipError_t launch_paths_eval(hipStream_t st, const CovDesc& cd, const PathsEvalArgs& a, int cnt) {
  const int ncb = (a.kq + 16 * PA_CG - 1) / (16 * PA_CG), nsg = (a.nslots + PA_SLOTS - 1) / PA_SLOTS;
  const dim3 grid((a.m + CT - 1) / CT, nsg * ncb, cnt);
  GPC_COV_DISPATCH(paths_eval_kernel, double, cd, grid, dim3(256), 0, st, cd, a);
  return hipGetLastError();
}

// Features, weights, the panel p(X) + eps and the solve for v, chunked over the samples.  The panel p(X) comes from the
// evaluation kernel itself (no training tiles, the training inputs as query points): the N x F feature matrix is never
// stored.  The solve is gpc_predict_grad's Q = (K + Sigma)^-1 R with block_append.h's product engines:
//   L_chol:    V1 = W P (lower triangular),  v = W^T V1 / sl          low noise (A = -(K + Sigma)^-1):  v = -(A P)
// The skinny kernel serves every 16 columns by itself, so a path's v does not depend on R; the MFMA engine (test option
// "paths_solve_engine" = 2) pads the panel to 128 columns in the storage type.
template <typename T>
int paths_create_impl(gpc_post* po, gpc_paths* pa, unsigned long long seed, int s_offset, const double* ym,
                      const double* noise_sd) {
  gpc_ctx* c = po->ctx;
  hipStream_t st = c->st;
  const int S = po->S, N = po->N, D = po->D, npad = po->npad, R = pa->R, F = pa->F, kq = pa->kq, fpad = pa->fpad;
  const int kp = pad_tile(R);
  const bool use_gemm = c->paths_solve_engine == 2;
  c->paths_solve_engine_ran = use_gemm ? 2 : 1;
  // scratch of one sample: three fp64 N_pad x kq panels (p(X), P, V1) and, for the MFMA engine, three N_pad x kp
  // panels in the storage type (and 64 spare bytes)
  const long long sP = (long long)npad * kq, sK = (long long)npad * kp;
  const size_t per = ScratchCarver::count<PathsCreateScratch<T>>(1, npad, kq, kp, use_gemm), held = c->cs.bytes;
  const int chunk = plan_chunk(c, S, per, 0, held, (size_t)S * per <= held, 0, false, [&](size_t budget) {
    return "gpc_paths_create: the scratch of one sample (" + std::to_string(per >> 10) + " KB: N_pad = " +
           std::to_string(npad) + ", R = " + std::to_string(R) + ") exceeds the device memory budget (" +
           std::to_string(budget >> 10) + " KB)";
  });
  if (!chunk) return -2;
  // the handle's own constants
  HIPCHK(c, pa->sp.ensure_private((size_t)S * SP_STRIDE * 8));
  HIPCHK(c, pa->mul.ensure_private((size_t)S * D * 8));
  HIPCHK(c, pa->dv.ensure_private((size_t)S * D * 8));
  HIPCHK(c, pa->xs.ensure_private((size_t)S * npad * D * 8));
  HIPCHK(c, pa->theta.ensure_private((size_t)S * fpad * D * 8));
  HIPCHK(c, pa->bph.ensure_private((size_t)S * fpad * 8));
  HIPCHK(c, pa->wt.ensure_private((size_t)S * fpad * kq * 8));
  HIPCHK(c, pa->v.ensure_private((size_t)S * npad * kq * 8));
  HIPCHK(c, hipMemcpyAsync(pa->sp.p, po->sp.data(), (size_t)S * SP_STRIDE * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(pa->mul.p, po->mul.data(), (size_t)S * D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(pa->dv.p, po->dv.data(), (size_t)S * D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(pa->v.p, 0, (size_t)S * npad * kq * 8, st));
  std::vector<double> par((size_t)S * BA_STRIDE, 0.0);
  bool any_high = false, any_low = false;
  for (int s = 0; s < S; ++s) {
    par[(size_t)s * BA_STRIDE + BA_SL] = po->sp[(size_t)s * SP_STRIDE + SP_SL];
    par[(size_t)s * BA_STRIDE + BA_LCH] = po->lchol[s] ? 1.0 : 0.0;
    par[(size_t)s * BA_STRIDE + BA_PRE] = 1.0;
    (po->lchol[s] ? any_high : any_low) = true;
  }
  HIPCHK(c, c->avec.ensure((size_t)S * BA_STRIDE * 8));
  HIPCHK(c, c->rvec.ensure(2 * (size_t)S * N * 8));
  double* d_par = c->avec.as<double>();
  double* d_ym = c->rvec.as<double>();
  double* d_nsd = d_ym + (size_t)S * N;
  HIPCHK(c, hipMemcpyAsync(d_par, par.data(), par.size() * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_ym, ym, (size_t)S * N * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_nsd, noise_sd, (size_t)S * N * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, c->cs.ensure((size_t)chunk * per));
  PathsCreateScratch<T> z;
  c->ms_total = c->ms_factor = 0;
  CallTimer tm{c, true};
  HIPCHK(c, tm.start());
  {
    const long long tot = (long long)npad * D;
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)((tot + 255) / 256), S), dim3(256), 0, st, c->dX.as<double>(), N,
                       npad, D, pa->mul.as<double>(), pa->dv.as<double>(), pa->xs.as<double>());
    const dim3 gf((fpad / 4 + 63) / 64, (D + 3) / 4, S), blk(64, 4);
    const bool matern = pa->cd.kind == K_MATERN || pa->cd.kind == K_MATERN_ISO;
    const int deg = matern ? pa->cd.degree : 0;
    double* th = pa->theta.as<double>();
    double* bp = pa->bph.as<double>();
    const long long sb = s_offset;
    if (deg == 0) hipLaunchKernelGGL((paths_features_kernel<0>), gf, blk, 0, st, seed, sb, F, fpad, D, th, bp);
    else if (deg == 1) hipLaunchKernelGGL((paths_features_kernel<1>), gf, blk, 0, st, seed, sb, F, fpad, D, th, bp);
    else if (deg == 3) hipLaunchKernelGGL((paths_features_kernel<3>), gf, blk, 0, st, seed, sb, F, fpad, D, th, bp);
    else hipLaunchKernelGGL((paths_features_kernel<5>), gf, blk, 0, st, seed, sb, F, fpad, D, th, bp);
    hipLaunchKernelGGL(paths_weights_kernel, dim3((kq + 63) / 64, fpad / 16, S), blk, 0, st, seed, sb, F, fpad, R, kq,
                       pa->wt.as<double>());
    HIPCHK(c, hipGetLastError());
  }
  const long long sM = (long long)npad * npad;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    CARVECHK(c, "gpc_paths_create", ScratchCarver::carve(z, c->cs.p, cnt, npad, kq, kp, use_gemm));
    double *const pX = z.pX, *const P = z.P, *const V1 = z.V1;
    T *const Bt = z.Bt, *const Vt = z.Vt, *const Qt = z.Qt;
    const double* parc = d_par + (size_t)s0 * BA_STRIDE;
    const T* Wc = po->W.as<T>() + (size_t)s0 * sM;
    const T* Ac = po->A.as<T>() + (size_t)s0 * sM;
    double* vc = pa->v.as<double>() + (size_t)s0 * sP;
    // 1. p(X): the evaluation kernel on the training inputs, features only
    PathsEvalArgs a{};
    a.xq = pa->xs.as<double>() + (size_t)s0 * npad * D;
    a.sp = pa->sp.as<double>() + (size_t)s0 * SP_STRIDE;
    a.mul = pa->mul.as<double>() + (size_t)s0 * D;
    a.dv = pa->dv.as<double>() + (size_t)s0 * D;
    a.theta = pa->theta.as<double>() + (size_t)s0 * fpad * D;
    a.bph = pa->bph.as<double>() + (size_t)s0 * fpad;
    a.wt = pa->wt.as<double>() + (size_t)s0 * fpad * kq;
    a.n = 0;
    a.npad = npad;
    a.m = N;
    a.mpad = npad;
    a.F = F;
    a.fpad = fpad;
    a.R = R;
    a.kq = kq;
    a.nslots = 1;
    a.f = pX;
    a.S_out = cnt;
    a.s_out0 = 0;
    HIPCHK(c, launch_paths_eval(st, pa->cd, a, cnt));
    // 2. P = y - m(X) - p(X) - eps
    hipLaunchKernelGGL(paths_rhs_kernel, dim3((kq + 63) / 64, npad / 16, cnt), dim3(64, 4), 0, st, seed,
                       (long long)s_offset + s0, N, npad, R, kq, (const double*)(d_ym + (size_t)s0 * N), (const double*)pX,
                       cnt, (const double*)d_nsd, S, s0, P);
    HIPCHK(c, hipGetLastError());
    // 3. v = (K + Sigma)^-1 P
    HIPCHK(c, tm.mark1());
    if (use_gemm) {
      hipLaunchKernelGGL((ba_to_panel_kernel<T>), dim3(kp / 64, npad / 4, cnt), dim3(64, 4), 0, st, (const double*)P, N, R,
                         kq, npad, kp, Bt);
      const int rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {
        GemmArgs g = tri_product_args<T>(po, s0 + a, lch, Bt + (size_t)a * sK, Vt + (size_t)a * sK, sK, kp, kp);  // V1 = W P | -(A P)
        g.alpha = lch ? 1.0 : -1.0;
        HIPCHK(c, launch_gemm<T>(st, g, false, true, len));
        if (lch)  // W^T V1 (k from the tile row's diagonal block on)
          HIPCHK(c, launch_gemm<T>(st, wt_product_args(g, Vt + (size_t)a * sK, Qt + (size_t)a * sK), true, true, len));
        return 0;
      });
      if (rc_runs) return rc_runs;
      const dim3 gp((kq + 63) / 64, (N + 3) / 4, cnt);
      if (any_high)
        hipLaunchKernelGGL((paths_from_panel_kernel<T>), gp, dim3(64, 4), 0, st, (const T*)Qt, N, kq, npad, kp, 1.0, 1, parc,
                           1, vc);
      if (any_low)
        hipLaunchKernelGGL((paths_from_panel_kernel<T>), gp, dim3(64, 4), 0, st, (const T*)Vt, N, kq, npad, kp, 1.0, 0, parc,
                           0, vc);
    } else {
      const dim3 gn((N + BA_T - 1) / BA_T, kq / BA_R, cnt);
      if (any_high) {
        hipLaunchKernelGGL((ba_skinny_kernel<T, false, true, false>), gn, dim3(256), 0, st, Wc, sM, npad, N, N,
                           (const double*)P, sP, kq, V1, sP, kq, 1.0, 0, parc, 1);
        hipLaunchKernelGGL((ba_skinny_kernel<T, true, true, false>), gn, dim3(256), 0, st, Wc, sM, npad, N, N,
                           (const double*)V1, sP, kq, vc, sP, kq, 1.0, 1, parc, 1);
      }
      if (any_low)
        hipLaunchKernelGGL((ba_skinny_kernel<T, false, false, false>), gn, dim3(256), 0, st, Ac, sM, npad, N, N,
                           (const double*)P, sP, kq, vc, sP, kq, -1.0, 0, parc, 0);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, tm.mark2());
  }
  HIPCHK(c, tm.stop());
  HIPCHK(c, hipStreamSynchronize(st));
  tm.accumulate();
  return 0;
}

// f and (optionally) df of all samples of the handle at M query points; the results are written on the device in the
// caller's layout and come back in one copy each.  Scratch per sample: the scaled query points and, for the unfused
// engine, one operand matrix, the widened panels and the product; chunked over the samples under the budget of
// gpc_predict_cov, beside the results themselves.
int paths_eval_impl(gpc_paths* pa, const double* xstar, int M, double* f, double* df) {
  gpc_ctx* c = pa->ctx;
  hipStream_t st = c->st;
  const int S = pa->S, N = pa->N, D = pa->D, npad = pa->npad, R = pa->R, F = pa->F, kq = pa->kq, fpad = pa->fpad;
  const int mpad = pad_tile(M), rp = pad_tile(R), nslots = df ? 1 + D : 1;
  const int engine = c->paths_engine ? c->paths_engine : PA_DEFAULT_ENGINE;
  c->paths_engine_ran = engine;
  const size_t fbytes = (size_t)M * R * S * 8, dfbytes = df ? fbytes * D : 0;
  const size_t per = ScratchCarver::count<PathsEvalScratch>(1, npad, fpad, mpad, rp, D, engine == 2);
  const size_t shared = ScratchCarver::count<PathsEvalShared>(M, R, S, D, df != nullptr), held = c->cs.bytes;
  const int chunk = plan_chunk(c, S, per, shared, held, shared + (size_t)S * per <= held, 0, false, [&](size_t budget) {
    return "gpc_paths_eval: the results (" + std::to_string(shared >> 10) + " KB) and the scratch of one "
           "sample (" + std::to_string(per >> 10) + " KB: M_pad = " + std::to_string(mpad) + ") exceed the device "
           "memory budget (" + std::to_string(budget >> 10) + " KB)";
  });
  if (!chunk) return -2;
  HIPCHK(c, c->cs.ensure(shared + (size_t)chunk * per));
  PathsEvalScratch z;
  PathsEvalShared zs;
  CARVECHK(c, "gpc_paths_eval", ScratchCarver::carve(zs, c->cs.as<char>() + (size_t)chunk * per, M, R, S, D, df != nullptr));
  double* const d_x = zs.x;
  c->pin.begin();
  c->ms_total = c->ms_factor = 0;
  CallTimer tm{c, true};
  HIPCHK(c, tm.start());
  HIPCHK(c, c->pin.up(d_x, xstar, (size_t)M * D * 8, st));
  HIPCHK(c, tm.mark1());
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    CARVECHK(c, "gpc_paths_eval", ScratchCarver::carve(z, c->cs.p, cnt, npad, fpad, mpad, rp, D, engine == 2));
    double *const xq = z.xq, *const op = z.op, *const Cb = z.Cb, *const Vp = z.Vp, *const Wp = z.Wp;
    const long long tot = (long long)mpad * D;
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)((tot + 255) / 256), cnt), dim3(256), 0, st, (const double*)d_x, M,
                       mpad, D, (const double*)(pa->mul.as<double>() + (size_t)s0 * D),
                       (const double*)(pa->dv.as<double>() + (size_t)s0 * D), xq);
    PathsEvalArgs a{};
    a.xs = pa->xs.as<double>() + (size_t)s0 * npad * D;
    a.xq = xq;
    a.sp = pa->sp.as<double>() + (size_t)s0 * SP_STRIDE;
    a.mul = pa->mul.as<double>() + (size_t)s0 * D;
    a.dv = pa->dv.as<double>() + (size_t)s0 * D;
    a.v = pa->v.as<double>() + (size_t)s0 * npad * kq;
    a.theta = pa->theta.as<double>() + (size_t)s0 * fpad * D;
    a.bph = pa->bph.as<double>() + (size_t)s0 * fpad;
    a.wt = pa->wt.as<double>() + (size_t)s0 * fpad * kq;
    a.n = N;
    a.npad = npad;
    a.m = M;
    a.mpad = mpad;
    a.F = F;
    a.fpad = fpad;
    a.R = R;
    a.kq = kq;
    a.nslots = nslots;
    a.f = zs.f;
    a.df = df ? zs.df : nullptr;
    a.S_out = S;
    a.s_out0 = s0;
    if (engine != 2) {
      HIPCHK(c, launch_paths_eval(st, pa->cd, a, cnt));
      continue;
    }
    const dim3 blk(64, 4);
    hipLaunchKernelGGL(paths_widen_kernel, dim3(rp / 64, npad / 4, cnt), blk, 0, st, a.v, npad, kq, rp, Vp);
    hipLaunchKernelGGL(paths_widen_kernel, dim3(rp / 64, fpad / 4, cnt), blk, 0, st, a.wt, fpad, kq, rp, Wp);
    for (int slot = 0; slot < nslots; ++slot) {
      hipLaunchKernelGGL(paths_cross_op_kernel, dim3(mpad / 64, npad / 4, cnt), blk, 0, st, pa->cd, a.xs, a.xq, a.sp, a.mul,
                         a.dv, N, npad, M, mpad, slot, op);
      GemmArgs g;  // C = op^T Vp: both operands k-major
      g.A = op;
      g.B = Vp;
      g.C = Cb;
      g.sA = (long long)npad * mpad;
      g.sB = (long long)npad * rp;
      g.sC = (long long)mpad * rp;
      g.lda = mpad;
      g.ldb = g.ldc = rp;
      g.M = mpad;
      g.N = rp;
      g.K = npad;
      g.alpha = 1.0;
      g.beta = 0;
      g.klo = KLO_ZERO;
      g.khi = KHI_FULL;
      g.lower_only = 0;
      HIPCHK(c, launch_gemm<double>(st, g, true, true, cnt));
      hipLaunchKernelGGL(paths_feat_op_kernel, dim3(mpad / 64, fpad / 4, cnt), blk, 0, st, D, a.theta, a.bph, a.xq, a.sp,
                         a.mul, a.dv, F, fpad, M, mpad, slot, op);
      g.B = Wp;
      g.sA = (long long)fpad * mpad;
      g.sB = (long long)fpad * rp;
      g.K = fpad;
      g.beta = 1;
      HIPCHK(c, launch_gemm<double>(st, g, true, true, cnt));
      hipLaunchKernelGGL(paths_scatter_kernel, dim3((R + 63) / 64, (M + 3) / 4, cnt), blk, 0, st, (const double*)Cb, M, mpad,
                         rp, R, D, slot, S, s0, a.f, a.df);
    }
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, tm.mark2());
  HIPCHK(c, hipMemcpyAsync(f, zs.f, fbytes, hipMemcpyDeviceToHost, st));
  if (df) HIPCHK(c, hipMemcpyAsync(df, zs.df, dfbytes, hipMemcpyDeviceToHost, st));
  HIPCHK(c, tm.stop());
  HIPCHK(c, hipStreamSynchronize(st));
  c->pin.finish();
  tm.accumulate();
  return 0;
}
}  // namespace

// =====================================================================================
// C ABI
// =====================================================================================
namespace {
template <typename T>
__global__ void tile_hash_kernel(const T* __restrict__ M, int npad, unsigned long long* __restrict__ out) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  unsigned long long h = 0;
  for (int e = threadIdx.x; e < TILE * TILE; e += 256) {
    const T v = M[(size_t)(ti * TILE + e / TILE) * npad + tj * TILE + e % TILE];
    unsigned long long b = 0;
    memcpy(&b, &v, sizeof(T));
    h += b * (unsigned long long)(2 * e + 1);
  }
  __shared__ unsigned long long sh[256];
  sh[threadIdx.x] = h;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[ti * gridDim.x + tj] = sh[0];
}
}  // namespace

namespace {
struct QuadMixOut {
  double *zalpha, *zbkzb, *gw, *zq;
  double* plane[6];  // dza_dmu, dza_dsigma, dzq_dmu, dzq_dsigma, dgw_dmu, dgw_dsigma
};

// gpc_quad_mix (quad_mix.h).  Per chunk of samples, all launches on the library's stream:
//   1  the measures' constants (quad_grad_prep_kernel, quad_mix_prep_kernel)
//   2  quad_mix_sum_tile_kernel + two ascending reductions: z . alpha (mpad) and zbar = Z w (npad)
//   3  (var) the solve, runs of equal L_chol sharing launches: v = W zbar, q = W^T v / sl with v . v riding in the
//      transposed product (the launches that form alpha), or q = -(L zbar) and zbar . q
//   4  (var) quad_mix_q_tile_kernel: z_j . q and, with grad, the four contractions; (grad only) quad_grad_tile_kernel's
//      alpha weights; quad_grad_reduce_kernel
//   5  (var) quad_mix_gamma_tile_kernel + quad_mix_gamma_reduce_kernel
// and ONE download of [za | zq | gw | scal | the planes].  No MFMA GEMM launch.
template <typename T>
int quad_mix_impl(gpc_post* po, const double* mu, const double* sigma, const double* w, int M, bool var, bool grad,
                  const QuadMixOut& o) {
  gpc_ctx* c = po->ctx;
  const int S = po->S, N = po->N, D = po->D, npad = po->npad;
  const int mpad = pad_tile(M);
  hipStream_t st = c->st;
  const long long sM = (long long)npad * npad;
  const int gnt = npad / CT, mnt = mpad / CT, nch = npad / TRC;
  const int gpl = grad ? (var ? 4 : 2) : 0;      // planes of quad_grad_reduce_kernel
  const int gnq = var ? (grad ? 1 + 2 * D : 1) : 0;  // quantities of the pair kernel
  const int npl = gpl + (var && grad ? 2 : 0);
  const size_t ss = (size_t)mpad * D;
  const size_t n_res = 3 * (size_t)mpad + 2 + (size_t)npl * ss;  // doubles of a sample's results
  const size_t shared = ScratchCarver::count<QuadMixShared>(M, mpad, D);
  const size_t per = ScratchCarver::count<QuadMixScratch>(1, npad, mpad, D, var, grad);
  const int chunk = plan_chunk(c, S, per, shared, c->qmix.bytes, (size_t)S * per + shared <= c->qmix.bytes, 0, false, [&](size_t budget) {
    return "gpc_quad_mix: the scratch of one sample (" + std::to_string((per + shared) >> 10) + " KB: N_pad = " +
           std::to_string(npad) + ", M_pad = " + std::to_string(mpad) + ", D = " + std::to_string(D) +
           ") exceeds the device memory budget (" + std::to_string(budget >> 10) + " KB)";
  });
  if (!chunk) return -2;
  HIPCHK(c, c->qmix.ensure((size_t)chunk * per + shared));
  HIPCHK(c, c->spb.ensure((size_t)chunk * SP_STRIDE * 8));
  HIPCHK(c, c->divb.ensure((size_t)chunk * D * 8));
  QuadMixShared zs;
  QuadMixScratch z;
  ScratchCarver::carve(zs, c->qmix.p, M, mpad, D);
  ScratchCarver::carve(z, c->qmix.as<char>() + shared, chunk, npad, mpad, D, var, grad);
  double *const d_mut = zs.mut, *const d_sgt = zs.sgt, *const d_wpad = zs.wpad, *const d_mu = zs.mu, *const d_sg = zs.sg, *const d_w = zs.w;
  double *const d_con = z.con, *const d_cpart = z.cpart, *const d_rpart = z.rpart, *const d_zbar = z.zbar, *const d_v = z.v, *const d_q = z.q;
  double *const d_tpart = z.tpart, *const d_zqpart = z.zqpart, *const d_gpart = z.gpart, *const d_gmpart = z.gmpart, *const d_res = z.res;
  double* d_za = d_res;
  double* d_zq = d_za + (size_t)chunk * mpad;
  double* d_gw = d_zq + (size_t)chunk * mpad;
  double* d_scal = d_gw + (size_t)chunk * mpad;
  double* d_gres = d_scal + 2 * (size_t)chunk;
  double* d_gmres = d_gres + (size_t)gpl * chunk * ss;
  std::unique_ptr<double[]> hres(new double[chunk * n_res]);  // (uninitialised: every entry read is downloaded first)
  const double* spb = c->spb.as<double>();
  const double* divb = c->divb.as<double>();
  const double* X = c->dX.as<double>();
  HIPCHK(c, hipMemcpyAsync(d_mu, mu, (size_t)M * D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_sg, sigma, (size_t)M * D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_w, w, (size_t)M * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(quad_mix_prep_kernel, dim3((mpad + 255) / 256), dim3(256), 0, st, (const double*)d_sg,
                     (const double*)d_w, M, mpad, D, d_sgt, d_wpad);
  CallTimer tm{c, CallTimer::wanted(c, npad)};
  // gpc_last_timing: device time of the call and, as ms_factor, of the solve (step 3), summed over the chunks
  c->ms_total = c->ms_factor = 0;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cnt = std::min(chunk, S - s0);
    HIPCHK(c, tm.start());
    HIPCHK(c, hipMemcpyAsync(c->spb.p, &po->sp[(size_t)s0 * SP_STRIDE], (size_t)cnt * SP_STRIDE * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->divb.p, &po->dv[(size_t)s0 * D], (size_t)cnt * D * 8, hipMemcpyHostToDevice, st));
    const double* alpha = po->alpha.as<double>() + (size_t)s0 * npad;
    hipLaunchKernelGGL(quad_grad_prep_kernel, dim3((mpad + 255) / 256, cnt), dim3(256), 0, st, (const double*)d_mu,
                       (const double*)d_sg, divb, spb, M, mpad, D, d_mut, d_con);
    hipLaunchKernelGGL(quad_mix_sum_tile_kernel, dim3(mnt, gnt, cnt), dim3(256), 0, st, X, D, (const double*)d_mut,
                       (const double*)d_con, alpha, npad, (const double*)d_wpad, N, M, mpad, npad, d_cpart, d_rpart);
    hipLaunchKernelGGL(colpart_reduce_kernel, dim3((mpad + 255) / 256, cnt), dim3(256), 0, st, (const double*)d_cpart,
                       gnt, mpad, d_za);
    hipLaunchKernelGGL(colpart_reduce_kernel, dim3((npad + 255) / 256, cnt), dim3(256), 0, st, (const double*)d_rpart,
                       mnt, npad, d_zbar);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, tm.mark1());
    if (!var) HIPCHK(c, tm.mark2());
    if (var) {
      const int rc_runs = for_lchol_runs(po, s0, cnt, [&](int a, int len, bool lch) -> int {  // runs of equal L_chol share launches
        const double* zb = d_zbar + (size_t)a * npad;
        if (lch) {
          const T* W = po->W.as<T>() + (size_t)(s0 + a) * sM;
          double* tp = d_tpart + (size_t)a * nch * npad;
          hipLaunchKernelGGL((trmv_kernel<T>), dim3(npad / 4, len), dim3(256), 0, st, W, sM, npad, zb, npad,
                             d_v + (size_t)a * npad, 0);
          hipLaunchKernelGGL((trmv_t_part_kernel<T, 8>), dim3((npad + 64 * MM<T>::VEC - 1) / (64 * MM<T>::VEC), nch, len),
                             dim3(256), 0, st, W, sM, npad, (const double*)(d_v + (size_t)a * npad), npad, tp, d_scal + a);
          hipLaunchKernelGGL(trmv_t_sum_kernel, dim3(npad / 128, len), dim3(128), 0, st, (const double*)tp, npad,
                             spb + (size_t)a * SP_STRIDE, (int)SP_STRIDE, (int)SP_SL, d_q + (size_t)a * npad);
        } else {  // q = 0 - L zbar (L = -(K + Sigma)^-1, full symmetric)
          HIPCHK(c, hipMemsetAsync(d_q + (size_t)a * npad, 0, (size_t)len * npad * 8, st));
          hipLaunchKernelGGL((gemv_sub_kernel<T>), dim3(npad / 4, len), dim3(256), 0, st,
                             (const T*)(po->A.as<T>() + (size_t)(s0 + a) * sM), sM, npad, zb, d_q + (size_t)a * npad, npad,
                             0, 0, npad);
          hipLaunchKernelGGL(dot_kernel, dim3(1, len), dim3(256), 0, st, zb, (const double*)(d_q + (size_t)a * npad), N,
                             npad, d_scal + a);
        }
        return 0;
      });
      if (rc_runs) return rc_runs;
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, tm.mark2());
      if (grad)
        hipLaunchKernelGGL((quad_mix_q_tile_kernel<true>), dim3(mnt, gnt, cnt), dim3(256), 0, st, X, D,
                           (const double*)d_mut, (const double*)d_con, alpha, npad, (const double*)d_q, N, M, mpad, npad,
                           d_zqpart, d_gpart);
      else
        hipLaunchKernelGGL((quad_mix_q_tile_kernel<false>), dim3(mnt, gnt, cnt), dim3(256), 0, st, X, D,
                           (const double*)d_mut, (const double*)d_con, alpha, npad, (const double*)d_q, N, M, mpad, npad,
                           d_zqpart, (double*)nullptr);
      hipLaunchKernelGGL(colpart_reduce_kernel, dim3((mpad + 255) / 256, cnt), dim3(256), 0, st,
                         (const double*)d_zqpart, gnt, mpad, d_zq);
      if (grad)
        hipLaunchKernelGGL((quad_mix_gamma_tile_kernel<true>), dim3(mnt, mnt, cnt), dim3(256), 0, st,
                           (const double*)d_mut, (const double*)d_sgt, (const double*)d_wpad, divb, spb, D, M, mpad,
                           d_gmpart);
      else
        hipLaunchKernelGGL((quad_mix_gamma_tile_kernel<false>), dim3(mnt, mnt, cnt), dim3(256), 0, st,
                           (const double*)d_mut, (const double*)d_sgt, (const double*)d_wpad, divb, spb, D, M, mpad,
                           d_gmpart);
      hipLaunchKernelGGL(quad_mix_gamma_reduce_kernel, dim3((mpad + 255) / 256, gnq, cnt), dim3(256), 0, st,
                         (const double*)d_gmpart, mnt, D, gnq, mpad, d_gw, d_gmres, (size_t)chunk * ss);
    } else if (grad) {  // the alpha weights only: quad_grad's own pass
      hipLaunchKernelGGL((quad_grad_tile_kernel<T, false>), dim3(mnt, gnt, cnt), dim3(256), 0, st, X, D,
                         (const double*)d_mut, (const double*)d_con, alpha, npad, (const T*)nullptr, 0LL, spb, 0, N, M,
                         mpad, d_gpart);
    }
    if (grad)
      hipLaunchKernelGGL(quad_grad_reduce_kernel, dim3((mpad + 255) / 256, gpl * D, cnt), dim3(256), 0, st,
                         (const double*)d_gpart, gnt, D, gpl, M, mpad, (const double*)d_sg, (const double*)d_con, d_gres,
                         (size_t)chunk * ss);
    HIPCHK(c, hipGetLastError());
    // (without var the blocks zq, gw and scal come back unwritten and unread)
    HIPCHK(c, hipMemcpyAsync(hres.get(), d_res, chunk * n_res * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, tm.stop());
    HIPCHK(c, hipStreamSynchronize(st));
    tm.accumulate();
    const double* hza = hres.get();
    const double* hzq = hza + (size_t)chunk * mpad;
    const double* hgw = hzq + (size_t)chunk * mpad;
    const double* hsc = hgw + (size_t)chunk * mpad;
    const double* hpl = hsc + 2 * (size_t)chunk;
    scatter_plane(o.zalpha, hza, M, mpad, S, s0, cnt);
    if (var) {
      scatter_plane(o.zq, hzq, M, mpad, S, s0, cnt);
      scatter_plane(o.gw, hgw, M, mpad, S, s0, cnt);
      // zbar (K + Sigma)^-1 zbar: |W zbar|^2 / sl (L_chol) or zbar . q = -(zbar . L zbar)
      for (int i = 0; i < cnt; ++i)
        o.zbkzb[s0 + i] = po->lchol[s0 + i] ? hsc[i] / po->sp[(size_t)(s0 + i) * SP_STRIDE + SP_SL] : hsc[i];
    }
    // [(j*D + l)*S + s].  Tile pass: dza_dmu, dza_dsigma (, dzq_dmu, dzq_dsigma: the reduce kernel doubled them for
    // quad_grad -- halved here, exactly); pair pass: dgw_dmu, dgw_dsigma
    for (int pl = 0; pl < npl; ++pl)
      scatter_plane(o.plane[pl < gpl ? pl : 4 + (pl - gpl)], hpl + (size_t)pl * chunk * ss, (size_t)M * D, ss, S, s0, cnt,
                    (pl >= 2 && pl < gpl) ? 0.5 : 1.0);
  }
  return 0;
}
}  // namespace

// gpc_debug_blas1: ONE launch of one blas1.h kernel, with the grid and block of the production call named at each case,
// on buffers that live for this call only (ScratchDev frees them): nothing of the context's workspace is touched, so
// what a kernel reads outside its contract is what the caller put there, and what it writes outside shows in the result.
namespace {
constexpr long long B1_GUARD = 128;  // elements after every result buffer (include/gpcore.h)
struct Blas1Call {
  const double* const* in;
  const long long* in_n;
  double* const* out;
  const long long* out_n;
  ScratchDev sd;
  void* dev[3] = {nullptr, nullptr, nullptr};
  bool ok = true;  // false: out of device memory, or a copy failed

  // operand k, uploaded whole as U: a plain cast of the caller's doubles (a NaN stays a NaN)
  template <typename U>
  const U* up(int k) {
    if (!in[k] || in_n[k] <= 0) return nullptr;
    const size_t n = (size_t)in_n[k];
    U* d = sd.get<U>(n);
    std::vector<U> h(in[k], in[k] + n);
    if (!d || hipMemcpy(d, h.data(), n * sizeof(U), hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return d;
  }
  // result k as U: out_n[k] quiet NaNs -- or, for a kernel that works in place, operand `from` -- and the NaN guard
  template <typename U>
  U* res(int k, int from = -1) {
    if (!out[k] || out_n[k] < 0) return nullptr;  // (out_n[k] = 0: the guard alone)
    const size_t n = (size_t)out_n[k];
    std::vector<U> h(n + B1_GUARD, std::numeric_limits<U>::quiet_NaN());
    if (from >= 0)
      for (size_t i = 0; i < n; ++i) h[i] = (U)in[from][i];
    U* d = sd.get<U>(h.size());
    if (!d || hipMemcpy(d, h.data(), h.size() * sizeof(U), hipMemcpyHostToDevice) != hipSuccess) ok = false;
    dev[k] = d;
    return d;
  }
  // the whole of result k, guard included, back to the caller
  template <typename U>
  bool down(int k) {
    if (!dev[k]) return true;
    std::vector<U> h((size_t)(out_n[k] + B1_GUARD));
    if (hipMemcpy(h.data(), dev[k], h.size() * sizeof(U), hipMemcpyDeviceToHost) != hipSuccess) return false;
    std::copy(h.begin(), h.end(), out[k]);
    return true;
  }
};

#define B1_REQ(cond) \
  if (!(cond)) FAIL(c, "gpc_debug_blas1: the arguments must satisfy " #cond)

template <typename T>
int debug_blas1_impl(gpc_ctx* c, int which, const int* ip, const double* const* in, const long long* in_n,
                     double* const* out, const long long* out_n) {
  constexpr int VEC = MM<T>::VEC;
  hipStream_t st = c->st;
  Blas1Call q{in, in_n, out, out_n};
  auto has_in = [&](int k, long long n) { return in[k] != nullptr && in_n[k] >= n; };
  auto has_out = [&](int k, long long n) { return out[k] != nullptr && out_n[k] == n; };
  // entries [first, first + count) of every row of `stride` of operand k: the vector a triangular product multiplies
  // with the exact zeros of W above the diagonal, which it reads unmasked (blas1.h: trmv_kernel)
  auto finite = [&](int k, long long batch, long long stride, long long first, long long count) {
    for (long long b = 0; b < batch; ++b)
      for (long long i = first; i < first + count; ++i)
        if (!std::isfinite(in[k][b * stride + i])) return false;
    return true;
  };
  const dim3 blk(64, 4);
  int nT = 0;  // the first nT results are stored as T
  // (every case: the argument check that keeps the launch inside the buffers, the buffers, the launch)
  switch (which) {
    case 0:    // trmv_kernel: plan.h:424 (forward_solve; :331 and :401 launch it with the same grid)
    case 1: {  // trmv_low_kernel: plan.h:421
      const long long npad = ip[0], batch = ip[1];
      const int row0 = which == 0 ? ip[2] : 0, rows = which == 0 ? ip[3] : (int)npad;
      B1_REQ(npad > 0 && npad % TILE == 0 && batch > 0 && row0 >= 0 && row0 % TILE == 0 && rows > 0 && rows % 16 == 0 &&
             row0 + rows <= npad);
      B1_REQ(has_in(0, batch * npad * npad) && has_in(1, batch * npad) && has_out(0, batch * npad));
      B1_REQ(finite(1, batch, npad, row0, rows));
      const T* W = q.up<T>(0);
      const double* r = q.up<double>(1);
      double* z = q.res<double>(0);
      if (!q.ok) break;
      if (which == 0)
        hipLaunchKernelGGL((trmv_kernel<T>), dim3(rows / 4, batch), dim3(256), 0, st, W, npad * npad, (int)npad, r, (int)npad,
                           z, row0);
      else
        hipLaunchKernelGGL((trmv_low_kernel<T>), dim3(npad / 16, batch), dim3(256), 0, st, W, npad * npad, (int)npad, r,
                           (int)npad, z);
      break;
    }
    case 2: {  // gemv_sub_kernel: plan.h:434 (forward_solve; :339 and :405 launch it with the same grid)
      const long long npad = ip[0], batch = ip[1];
      const int row0 = ip[2], nrows = ip[3], col0 = ip[4], ncols = ip[5];
      B1_REQ(npad > 0 && npad % TILE == 0 && batch > 0 && row0 >= 0 && nrows > 0 && nrows % 4 == 0 && row0 + nrows <= npad &&
             col0 >= 0 && col0 % TILE == 0 && ncols > 0 && ncols % TILE == 0 && col0 + ncols <= npad);
      B1_REQ(has_in(0, batch * npad * npad) && has_in(1, batch * npad) && has_in(2, batch * npad) && has_out(0, batch * npad));
      const T* A = q.up<T>(0);
      const double* z = q.up<double>(1);
      double* r = q.res<double>(0, 2);
      if (!q.ok) break;
      hipLaunchKernelGGL((gemv_sub_kernel<T>), dim3(nrows / 4, batch), dim3(256), 0, st, A, npad * npad, (int)npad, z, r,
                         (int)npad, row0, col0, ncols);
      break;
    }
    case 3:    // trmv_t_part_kernel<T, 8>: gpcore.hip:1152
    case 4: {  // trmv_t_part_low_kernel: gpcore.hip:1149
      const long long npad = ip[0], batch = ip[1];
      const bool quad = ip[2] != 0;
      B1_REQ(npad > 0 && npad % TILE == 0 && batch > 0);
      B1_REQ(has_in(0, batch * npad * npad) && has_in(1, batch * npad) && has_out(0, batch * (npad / TRC) * npad) &&
             (!quad || has_out(1, batch)));
      B1_REQ(finite(1, batch, npad, 0, npad));
      const T* W = q.up<T>(0);
      const double* z = q.up<double>(1);
      double* part = q.res<double>(0);
      double* qd = quad ? q.res<double>(1) : nullptr;
      if (!q.ok) break;
      const dim3 gt((npad + 64 * VEC - 1) / (64 * VEC), npad / TRC, batch);
      if (which == 3)
        hipLaunchKernelGGL((trmv_t_part_kernel<T, 8>), gt, dim3(256), 0, st, W, npad * npad, (int)npad, z, (int)npad, part, qd);
      else
        hipLaunchKernelGGL((trmv_t_part_low_kernel<T>), gt, dim3(256), 0, st, W, npad * npad, (int)npad, z, (int)npad, part,
                           qd);
      break;
    }
    case 5: {  // trmv_t_sum_kernel: gpcore.hip:1154 (with the scale), :5043 (without)
      const long long npad = ip[0], batch = ip[1];
      const int sp_stride = ip[2], sp_off = ip[3];
      B1_REQ(npad > 0 && npad % TILE == 0 && batch > 0);
      B1_REQ(has_in(0, batch * (npad / TRC) * npad) && has_out(0, batch * npad) &&
             (!in[1] || (sp_off >= 0 && sp_off < sp_stride && has_in(1, batch * sp_stride))));
      const double* part = q.up<double>(0);
      const double* sp = q.up<double>(1);
      double* o = q.res<double>(0);
      if (!q.ok) break;
      hipLaunchKernelGGL(trmv_t_sum_kernel, dim3(npad / 128, batch), dim3(128), 0, st, part, (int)npad, sp, sp_stride, sp_off, o);
      break;
    }
    case 6: {  // dot_kernel: gpcore.hip:1143
      const long long n = ip[0], stride = ip[1], batch = ip[2];
      B1_REQ(n > 0 && stride >= n && batch > 0);
      B1_REQ(has_in(0, batch * stride) && has_in(1, batch * stride) && has_out(0, batch));
      const double* x = q.up<double>(0);
      const double* y = q.up<double>(1);
      double* o = q.res<double>(0);
      if (!q.ok) break;
      hipLaunchKernelGGL(dot_kernel, dim3(1, batch), dim3(256), 0, st, x, y, (int)n, (int)stride, o);
      break;
    }
    case 7: {  // mat_t_vec_kernel: gpcore.hip:1215
      const long long n = ip[0], P = ip[1], vstride = ip[2], batch = ip[3];
      B1_REQ(n > 0 && P > 0 && vstride >= n && batch > 0);
      B1_REQ(has_in(0, batch * n * P) && has_in(1, batch * vstride) && has_out(0, batch * P));
      const double* M = q.up<double>(0);
      const double* v = q.up<double>(1);
      double* o = q.res<double>(0);
      if (!q.ok) break;
      hipLaunchKernelGGL(mat_t_vec_kernel, dim3(P, batch), dim3(256), 0, st, M, (int)n, (int)P, v, (int)vstride, o);
      break;
    }
    case 8: {  // grad_tail_kernel: gpcore.hip:1205
      const long long ntiles = ip[0], P = ip[1], n = ip[2], mN = ip[3], nN = ip[4], vstride = ip[5], batch = ip[6];
      B1_REQ(ntiles > 0 && P > 0 && n > 0 && mN >= 0 && nN >= 0 && vstride >= n && batch > 0);
      // alpha and diagq are always there, as in the production call; mg and ng always have a buffer -- without mean or
      // noise slots the guard alone, where the production call passes nullptr: a stray write shows instead of faulting
      B1_REQ(has_in(0, batch * ntiles * P) && has_in(2, batch * vstride) && has_in(4, batch * vstride) &&
             has_out(0, batch * P) && has_out(1, batch * mN) && has_out(2, batch * nN));
      B1_REQ((mN == 0 || !in[1] || has_in(1, batch * n * mN)) && (nN == 0 || has_in(3, batch * n * nN)));
      const double* part = q.up<double>(0);
      const double* dm = mN ? q.up<double>(1) : nullptr;
      const double* al = q.up<double>(2);
      const double* ds = nN ? q.up<double>(3) : nullptr;
      const double* dq = q.up<double>(4);
      double* gout = q.res<double>(0);
      double* mg = q.res<double>(1);
      double* ng = q.res<double>(2);
      if (!q.ok) break;
      hipLaunchKernelGGL(grad_tail_kernel, dim3(P + mN + nN, batch), dim3(256), 0, st, part, (int)ntiles, (int)P, gout, dm,
                         (int)n, (int)mN, al, mg, ds, (int)nN, dq, ng, (int)vstride);
      break;
    }
    case 9:     // colsum_prod_kernel: gpcore.hip:2885
    case 10: {  // colsum_vec_kernel: gpcore.hip:2853
      const long long ld = ip[0], nrows = ip[1], mpad = ip[2], vstride = which == 10 ? ip[3] : 0,
                      batch = which == 10 ? ip[4] : ip[3];
      B1_REQ(mpad > 0 && mpad % 64 == 0 && ld >= mpad && nrows > 0 && batch > 0);
      B1_REQ(has_in(0, batch * nrows * ld) && in_n[0] % batch == 0 && has_out(0, batch * mpad));
      B1_REQ(which == 10 ? (vstride >= nrows && has_in(1, batch * vstride)) : (in[1] != nullptr && in_n[1] == in_n[0]));
      const long long sA = in_n[0] / batch;
      const T* A = q.up<T>(0);
      const T* Bm = which == 9 ? q.up<T>(1) : nullptr;
      const double* v = which == 10 ? q.up<double>(1) : nullptr;
      double* o = q.res<double>(0);
      if (!q.ok) break;
      if (which == 9)
        hipLaunchKernelGGL((colsum_prod_kernel<T>), dim3(mpad / 64, batch), dim3(256), 0, st, A, sA, Bm, sA, (int)ld, (int)nrows,
                           (int)mpad, o);
      else
        hipLaunchKernelGGL((colsum_vec_kernel<T>), dim3(mpad / 64, batch), dim3(256), 0, st, A, sA, (int)ld, v, (int)vstride,
                           (int)nrows, (int)mpad, o);
      break;
    }
    case 11: {  // diagq_kernel: gpcore.hip:1197
      const long long n = ip[0], ld = ip[1], P = ip[2], batch = ip[3];
      B1_REQ(n > 0 && n <= ld && P > 0 && batch > 0);
      B1_REQ(has_in(0, batch * ld * ld) && has_in(1, batch * ld) && has_in(2, batch * SP_STRIDE) && has_out(0, batch * ld) &&
             has_out(1, batch * P));
      const T* Ai = q.up<T>(0);
      const double* al = q.up<double>(1);
      const double* sp = q.up<double>(2);
      double* dq = q.res<double>(0);
      double* o = q.res<double>(1);
      if (!q.ok) break;
      hipLaunchKernelGGL((diagq_kernel<T>), dim3(1, batch), dim3(256), 0, st, Ai, ld * ld, (int)ld, al, sp, (int)n, dq, o, (int)P);
      break;
    }
    case 12: {  // trace_plane_kernel: gpcore.hip:966
      const long long n = ip[0], ld = ip[1], nblk = ip[2];
      B1_REQ(n > 0 && n <= ld && nblk > 0 && nblk <= 1024);
      B1_REQ(has_in(0, n * ld) && has_in(1, n) && has_in(2, SP_STRIDE) && has_in(3, n * n) && has_out(0, nblk));
      const T* Ai = q.up<T>(0);
      const double* al = q.up<double>(1);
      const double* sp = q.up<double>(2);
      const double* dK = q.up<double>(3);
      double* part = q.res<double>(0);
      if (!q.ok) break;
      hipLaunchKernelGGL((trace_plane_kernel<T>), dim3(nblk), dim3(256), 0, st, Ai, (int)ld, al, sp, dK, (int)n, part);
      break;
    }
    case 13: {  // extract_kernel: gpcore.hip:4605 (mode 0), :2969 (mode 2); mode 1 has no caller left: the same grid
      const long long n = ip[0], ld = ip[1];
      const int mode = ip[2];
      B1_REQ(n > 0 && n <= ld && mode >= 0 && mode <= 2);
      B1_REQ(has_in(0, n * ld) && has_out(0, n * n));
      const T* src = q.up<T>(0);
      double* dst = q.res<double>(0);
      if (!q.ok) break;
      hipLaunchKernelGGL((extract_kernel<T>), dim3((n + 63) / 64, (n + 3) / 4), blk, 0, st, src, (int)ld, (int)n, mode, dst);
      break;
    }
    case 14: {  // neg_sym_kernel: gpcore.hip:2473
      const long long npad = ip[0], ld = ip[1], batch = ip[2];
      B1_REQ(npad > 0 && npad % TILE == 0 && ld >= npad && batch > 0);
      B1_REQ(has_in(0, batch * npad * ld) && in_n[0] % batch == 0 && has_out(0, in_n[0]));
      T* buf = q.res<T>(0, 0);
      nT = 1;
      if (!q.ok) break;
      hipLaunchKernelGGL((neg_sym_kernel<T>), dim3(npad / 64, npad / 4, batch), blk, 0, st, buf, in_n[0] / batch, (int)ld,
                         (int)npad);
      break;
    }
    case 15: {  // pad_load_kernel: gpcore.hip:4587
      const long long n = ip[0], npad = ip[1];
      B1_REQ(n > 0 && n <= npad && npad % TILE == 0);
      B1_REQ(has_in(0, n * n) && has_out(0, npad * npad));
      const double* src = q.up<double>(0);
      T* dst = q.res<T>(0);
      nT = 1;
      if (!q.ok) break;
      hipLaunchKernelGGL((pad_load_kernel<T>), dim3(npad / 64, npad / 4), blk, 0, st, src, (int)n, (int)npad, dst);
      break;
    }
    case 16: {  // pad_rect_kernel: gpcore.hip:2831
      const long long r = ip[0], cc = ip[1], rpad = ip[2], cpad = ip[3];
      B1_REQ(r > 0 && cc > 0 && r <= rpad && cc <= cpad && rpad % TILE == 0 && cpad % TILE == 0);
      B1_REQ(has_in(0, r * cc) && has_out(0, rpad * cpad));
      const double* src = q.up<double>(0);
      T* dst = q.res<T>(0);
      nT = 1;
      if (!q.ok) break;
      hipLaunchKernelGGL((pad_rect_kernel<T>), dim3(cpad / 64, rpad / 4), blk, 0, st, src, (int)r, (int)cc, (int)rpad, (int)cpad,
                         dst);
      break;
    }
    case 17: {  // load_K_kernel: gpcore.hip:1005
      const long long n = ip[0], npad = ip[1];
      B1_REQ(n > 0 && n <= npad && npad % TILE == 0);
      B1_REQ(has_in(0, n * n) && has_in(1, SP_STRIDE) && has_in(2, n) && has_out(0, npad * npad));
      const double* K = q.up<double>(0);
      const double* sp = q.up<double>(1);
      const double* dv = q.up<double>(2);
      T* A = q.res<T>(0);
      nT = 1;
      if (!q.ok) break;
      hipLaunchKernelGGL((load_K_kernel<T>), dim3(npad / 64, npad / 4), blk, 0, st, K, (int)n, (int)npad, sp, dv, A);
      break;
    }
    case 18: {  // rect_copy_kernel: plan.h:273
      const long long rows = ip[0], cols = ip[1], lds_ = ip[2], ldd = ip[3], batch = ip[4];
      B1_REQ(rows > 0 && rows % 32 == 0 && cols > 0 && cols % TILE == 0 && lds_ >= cols && ldd >= cols && lds_ % 4 == 0 &&
             ldd % 4 == 0 && batch > 0);  // (16-byte aligned rows in either type)
      B1_REQ(has_in(0, batch * rows * lds_) && has_in(1, batch * rows * ldd) && in_n[0] % (4 * batch) == 0 &&
             in_n[1] % (4 * batch) == 0 && has_out(0, in_n[1]));
      const T* src = q.up<T>(0);
      T* dst = q.res<T>(0, 1);
      nT = 1;
      if (!q.ok) break;
      hipLaunchKernelGGL((rect_copy_kernel<T>), dim3((cols + 64 * VEC - 1) / (64 * VEC), rows / 32, batch), blk, 0, st, src,
                         in_n[0] / batch, (int)lds_, dst, in_n[1] / batch, (int)ldd, (int)rows, (int)cols);
      break;
    }
    case 19: {  // grow_copy_kernel: gpcore.hip:4968
      const long long np = ip[0], npn = ip[1], batch = ip[2];
      B1_REQ(np > 0 && np <= npn && npn % TILE == 0 && batch > 0);
      B1_REQ(has_in(0, batch * np * np) && has_out(0, batch * npn * npn));
      const T* src = q.up<T>(0);
      T* dst = q.res<T>(0);
      nT = 1;
      if (!q.ok) break;
      hipLaunchKernelGGL((grow_copy_kernel<T>), dim3(npn / 64, npn / 4, batch), blk, 0, st, src, (int)np, dst, (int)npn);
      break;
    }
    case 20: {  // append_row_kernel: gpcore.hip:5104 (there one launch per sample)
      const long long npad = ip[0], n = ip[1], batch = ip[2];
      B1_REQ(npad > 0 && npad % TILE == 0 && n >= 0 && n < npad && batch > 0);
      B1_REQ(has_in(0, batch * npad * npad) && has_in(1, batch * npad * npad) && has_in(2, batch * npad) &&
             has_in(3, batch * npad) && has_in(4, batch * 5) && has_in(5, batch * npad));
      B1_REQ(has_out(0, batch * npad * npad) && has_out(1, batch * npad * npad) && has_out(2, batch * npad));
      T* A = q.res<T>(0, 0);
      T* W = q.res<T>(1, 1);
      const double* l = q.up<double>(2);
      const double* au = q.up<double>(3);
      const double* cf = q.up<double>(4);
      double* al = q.res<double>(2, 5);
      nT = 2;
      if (!q.ok) break;
      hipLaunchKernelGGL((append_row_kernel<T>), dim3((n + 256) / 256, batch), dim3(256), 0, st, A, W, npad * npad, (int)npad,
                         (int)n, l, au, (int)npad, cf, al);
      break;
    }
    case 21: {  // append_low_kernel: gpcore.hip:5109
      const long long ld = ip[0], n = ip[1];
      B1_REQ(ld > 0 && n >= 0 && n < ld);
      B1_REQ(has_in(0, ld * ld) && has_in(1, std::max<long long>(n, 1)) && has_in(2, 5) && has_in(3, ld) && has_out(0, ld * ld) &&
             has_out(1, ld));
      T* A = q.res<T>(0, 0);
      const double* au = q.up<double>(1);
      const double* cf = q.up<double>(2);
      double* al = q.res<double>(1, 3);
      nT = 1;
      if (!q.ok) break;
      hipLaunchKernelGGL((append_low_kernel<T>), dim3((n + 64) / 64, (n + 4) / 4), blk, 0, st, A, (int)ld, (int)n, au, cf, al);
      break;
    }
    default:
      FAIL(c, "gpc_debug_blas1: which must be 0 .. 21");
  }
  if (!q.ok) FAIL(c, "gpc_debug_blas1: out of device memory, or a copy failed");
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(st));
  for (int k = 0; k < 3; ++k)
    if (!(k < nT ? q.down<T>(k) : q.down<double>(k))) FAIL(c, "gpc_debug_blas1: the copy of a result failed");
  return 0;
}
#undef B1_REQ
}  // namespace


extern "C" {

int gpc_create(int device, gpc_ctx** out) {
  if (!out) return -2;
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    g_create_err = std::string("no HIP device: ") + hipGetErrorString(e);
    return -1;
  }
  if (device < 0 || device >= count) {
    g_create_err = "device index out of range";
    return -2;
  }
  e = hipSetDevice(device);
  if (e != hipSuccess) {
    g_create_err = hipGetErrorString(e);
    return -1;
  }
  gpc_ctx* c = new gpc_ctx();
  c->device = device;
  hipDeviceProp_t prop{};
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
    char buf[512];
    snprintf(buf, sizeof buf, "%s arch=%s CUs=%d clock=%dMHz mem=%.1fGB lds/block=%zuKB", prop.name,
             prop.gcnArchName, prop.multiProcessorCount, prop.clockRate / 1000,
             prop.totalGlobalMem / 1073741824.0, prop.sharedMemPerBlock / 1024);
    c->devinfo = buf;
  }
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);  // lo = least, hi = greatest priority
  if (hipStreamCreateWithPriority(&c->st, hipStreamNonBlocking, prio_hi) != hipSuccess) {
    g_create_err = "hipStreamCreate failed";
    delete c;
    return -1;
  }
  for (auto& ev : c->ev)
    if (hipEventCreate(&ev) != hipSuccess) {
      g_create_err = "hipEventCreate failed";
      delete c;
      return -1;
    }
  bool ok = hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming) == hipSuccess;
  for (int g = 0; g <= gpc_ctx::MAXG && ok; ++g)
    ok = hipEventCreate(&c->ev_l0[g]) == hipSuccess && hipEventCreate(&c->ev_l1[g]) == hipSuccess;
  for (int g = 0; g < gpc_ctx::MAXG && ok; ++g)
    ok = hipStreamCreateWithPriority(&c->gst[g], hipStreamNonBlocking, prio_hi) == hipSuccess &&
         hipEventCreateWithFlags(&c->ev_done[g], hipEventDisableTiming) == hipSuccess;
  for (int g = 0; g <= gpc_ctx::MAXG && ok; ++g) {
    ok = hipStreamCreateWithPriority(&c->sst[g], hipStreamNonBlocking, prio_lo) == hipSuccess;
    for (int i = 0; i < gpc_ctx::NDEV && ok; ++i)
      ok = hipEventCreateWithFlags(&c->dev_ev[g][i], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->ev_bfork[g], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->ev_btail[g], hipEventDisableTiming) == hipSuccess;
  }
  if (const char* e = getenv("GPC_DEFER_MIN")) c->defer_min = atoi(e);
  if (const char* e = getenv("GPC_DEFER_RESERVE")) c->defer_reserve = atoi(e);
  if (!ok) {
    g_create_err = "creating the sample-group streams failed";
    delete c;
    return -1;
  }
  if (const char* e = getenv("GPC_PERSIST_SPARE")) gpc::g_persist_spare = atoi(e);  // < 0: no persistent launches
  gpc::g_block_slots = 2 * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256);
  if (c->tile_ctr.ensure((gpc_ctx::MAXG + 1) * gpc_ctx::CTR_PER_GROUP * sizeof(int)) != hipSuccess) {
    g_create_err = "allocating the tile counters failed";
    delete c;
    return -1;
  }
  {  // the landing block of one-leaf evaluations: coherent (fine-grained) host memory, so that a word the device writes
     // in the middle of a kernel is seen by a polling host; without it those calls wait on the stream as before
    void* lp = nullptr;
    if (hipHostMalloc(&lp, gpc_ctx::LAND_BYTES, hipHostMallocCoherent) == hipSuccess) {
      memset(lp, 0, gpc_ctx::LAND_BYTES);
      c->land_blk = static_cast<double*>(lp);
    } else {
      (void)hipGetLastError();
    }
  }
  if (const char* e = getenv("GPC_SMALL_POLL")) c->small_poll = atoi(e) != 0;
  if (probe_cu_map(c, prop.multiProcessorCount) != 0 || build_reserve_table(c) != 0) {
    g_create_err = "probing the CU map failed: " + c->err;
    delete c;
    return -1;
  }
  if (const char* e = getenv("GPC_LEAF")) gpc::g_leaf_version = atoi(e) == 3 ? 3 : 5;
  if (const char* e = getenv("GPC_SMALL_PATH")) c->small_path = atoi(e) != 0;
  if (const char* e = getenv("GPC_GRAPH_MAX_NPAD")) c->graph_max_npad = atoi(e);
#ifdef GPC_EXPERIMENTS
  if (const char* e = getenv("GPC_RL_PANEL")) c->rl_panel = atoi(e) <= 0 ? 0 : std::max(TILE, (atoi(e) / TILE) * TILE);
  if (const char* e = getenv("GPC_RECT_MIN")) gpc::g_rect_min_blocks = atoi(e);
#endif
  if (const char* e = getenv("GPC_NLL_BLOCK")) c->nll_block = atoi(e) < 0 ? -1 : (atoi(e) == 0 ? 0 : std::max(TILE, (atoi(e) / TILE) * TILE));
  if (const char* e = getenv("GPC_GROUPS")) c->groups = std::max(1, std::min((int)gpc_ctx::MAXG, atoi(e)));
  if (const char* e = getenv("GPC_SMALL_BLOCKS")) gpc::g_small_launch_blocks = atoi(e);
  if (const char* e = getenv("GPC_DUAL")) gpc::g_dual_launch = atoi(e) != 0;
  if (const char* e = getenv("GPC_GEMM_FLAGS")) gpc::g_gemm_flags = atoi(e);
  if (const char* e = getenv("GPC_XCD_AFFINE")) gpc::g_gemm_flags = atoi(e) ? (gpc::g_gemm_flags | 8) : (gpc::g_gemm_flags & ~8);
  *out = c;
  return 0;
}

void gpc_destroy(gpc_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->st);
  DevBuf* bufs[] = {&c->dX,   &c->dY,  &c->gpts,  &c->gxs, &c->mA,    &c->mW,  &c->mT,   &c->xs,   &c->spb,  &c->mulb, &c->divb,
                    &c->dvec, &c->rvec,  &c->zvec, &c->avec, &c->scal, &c->parts, &c->gout, &c->diagq,
                    &c->dmb,  &c->dsn2b, &c->mg,  &c->ng,   &c->cs,   &c->covs,
                    &c->dbg1, &c->dbg2,  &c->dbg3, &c->tpart, &c->qmix, &c->nhs, &c->hgs, &c->lab, &c->tile_ctr, &c->rsv_tbl};
  for (auto& g : c->graphs)
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
  for (DevBuf* b : bufs) b->release();
  c->pool_drain();
  c->pin.release();
  if (c->land_blk) (void)hipHostFree(c->land_blk);
  for (auto& ev : c->ev)
    if (ev) (void)hipEventDestroy(ev);
  if (c->ev_up) (void)hipEventDestroy(c->ev_up);
  for (int g = 0; g <= gpc_ctx::MAXG; ++g) {
    if (c->ev_l0[g]) (void)hipEventDestroy(c->ev_l0[g]);
    if (c->ev_l1[g]) (void)hipEventDestroy(c->ev_l1[g]);
  }
  for (int g = 0; g <= gpc_ctx::MAXG; ++g) {
    for (int i = 0; i < gpc_ctx::NDEV; ++i)
      if (c->dev_ev[g][i]) (void)hipEventDestroy(c->dev_ev[g][i]);
    if (c->ev_bfork[g]) (void)hipEventDestroy(c->ev_bfork[g]);
    if (c->ev_btail[g]) (void)hipEventDestroy(c->ev_btail[g]);
    if (c->sst[g]) (void)hipStreamDestroy(c->sst[g]);
  }
  for (int g = 0; g < gpc_ctx::MAXG; ++g) {
    if (c->ev_done[g]) (void)hipEventDestroy(c->ev_done[g]);
    if (c->gst[g]) (void)hipStreamDestroy(c->gst[g]);
  }
  if (c->st) (void)hipStreamDestroy(c->st);
  delete c;
}

const char* gpc_last_error(const gpc_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

const char* gpc_device_info(gpc_ctx* c) { return c ? c->devinfo.c_str() : ""; }

int gpc_cov_count(int kernel_id, int D) { return cov_count_of(kernel_id, D); }

int gpc_debug_chunk_plan(int S, unsigned long long per, unsigned long long shared, unsigned long long budget,
                         int clamp_to_one) {
  if (S <= 0 || per == 0) return -2;
  return chunk_from_budget(S, (size_t)per, (size_t)shared, (size_t)budget, clamp_to_one != 0);
}

int gpc_debug_scratch_bytes(const char* name, int dtype, const int* dims, int ndims, unsigned long long* per,
                            unsigned long long* shared, int* misaligned) {
  if (!name || !dims || ndims < 1 || !per || !shared || !misaligned || (dtype != GPC_F64 && dtype != GPC_F32)) return -2;
  return dtype == GPC_F64 ? scratch_bytes_of<double>(name, dims, ndims, per, shared, misaligned)
                          : scratch_bytes_of<float>(name, dims, ndims, per, shared, misaligned);
}

int gpc_max_n(int dtype) {
  // A memory-budget answer (round 6; rounds 1-5: 16384 / 23168, the reach of one 32-bit byte offset over a k-major
  // operand panel, which gemm.h no longer has): the largest N, a multiple of 128, whose three padded slabs A, W and
  // scratch (plan.h) of ONE sample fit in 80 % of the current device's memory -- what nll_impl / post_impl budget a chunk
  // with.  Without a device: the MI355X's 288 GB.
  const long long w = dtype == GPC_F32 ? 4 : 8;
  size_t fr = 0, total = 0;
  if (hipMemGetInfo(&fr, &total) != hipSuccess || total == 0) {
    (void)hipGetLastError();
    total = (size_t)288 << 30;
  }
  const double budget = 0.8 * (double)total / (3.0 * (double)w);
  long long n = (long long)std::floor(std::sqrt(budget) / TILE) * TILE;
  // (tile and element counts are 32-bit in the kernels' index arithmetic up to (npad / 64)^2 tiles: far beyond any memory)
  return (int)std::max<long long>(TILE, std::min<long long>(n, 1 << 20));
}

int gpc_set_data(gpc_ctx* c, const double* X, const double* y, int N, int D) {
  if (!c) return -2;
  if (!X || !y || N <= 0 || D <= 0) FAIL(c, "gpc_set_data: X, y must be non-null and N, D positive");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->dX.ensure((size_t)N * D * sizeof(double)));
  c->pin.begin();
  HIPCHK(c, c->pin.up(c->dX.p, X, (size_t)N * D * sizeof(double), c->st));
  HIPCHK(c, c->dY.ensure((size_t)N * sizeof(double)));
  HIPCHK(c, hipMemcpyAsync(c->dY.p, y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  c->hy.assign(y, y + N);
  c->N = N;
  c->D = D;
  c->npad = pad_tile(N);
  c->gobs = GobsDims();
  return 0;
}

int gpc_kernel(gpc_ctx* c, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
               const double* Xstar, int M, int diag, double* K, double* dK) {
  if (!c) return -2;
  if (!valid_kernel(kernel_id, degree)) FAIL(c, "unknown covariance kernel / degree");
  if (!hyp_cov || !X || !K || N <= 0 || D <= 0) FAIL(c, "gpc_kernel: bad arguments");
  if (Xstar && dK) FAIL(c, "X_star should be None when compute_grad is True.");
  HIPCHK(c, hipSetDevice(c->device));
  CovDesc cd{kernel_id, degree, D, cov_count_of(kernel_id, D)};
  std::vector<double> mul(D), dv(D);
  double sf2, rqa;
  scaling_of(kernel_id, degree, D, hyp_cov, mul.data(), dv.data(), &sf2, &rqa);
  if (diag) {  // zero distance: covariance_functions.py:162-163
    for (int i = 0; i < N; ++i) K[i] = sf2;
    return 0;
  }
  const int Mc = Xstar ? M : N;
  if (Mc <= 0) FAIL(c, "gpc_kernel: M must be positive with Xstar");
  hipStream_t st = c->st;
  // dbg1: raw X | raw X* | mul | div ; dbg2: scaled Xa | scaled Xb ; dbg3: K | dK
  const size_t nraw = (size_t)N * D + (size_t)Mc * D + 2 * (size_t)D;
  HIPCHK(c, c->dbg1.ensure(nraw * 8));
  HIPCHK(c, c->dbg2.ensure(((size_t)N * D + (size_t)Mc * D) * 8));
  const size_t nK = (size_t)N * Mc, ndK = dK ? nK * cd.cov_N : 0;
  HIPCHK(c, c->dbg3.ensure((nK + ndK) * 8));
  double* d_xa = c->dbg1.as<double>();
  double* d_xb = d_xa + (size_t)N * D;
  double* d_mul = d_xb + (size_t)Mc * D;
  double* d_div = d_mul + D;
  c->pin.begin();
  HIPCHK(c, c->pin.up(d_xa, X, (size_t)N * D * 8, st));
  HIPCHK(c, c->pin.up(d_xb, Xstar ? Xstar : X, (size_t)Mc * D * 8, st));
  HIPCHK(c, hipMemcpyAsync(d_mul, mul.data(), D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_div, dv.data(), D * 8, hipMemcpyHostToDevice, st));
  double* s_xa = c->dbg2.as<double>();
  double* s_xb = s_xa + (size_t)N * D;
  hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)N * D + 255) / 256), 1), dim3(256), 0, st,
                     (const double*)d_xa, N, N, D, (const double*)d_mul, (const double*)d_div, s_xa);
  hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)Mc * D + 255) / 256), 1), dim3(256), 0, st,
                     (const double*)d_xb, Mc, Mc, D, (const double*)d_mul, (const double*)d_div, s_xb);
  double* d_K = c->dbg3.as<double>();
  double* d_dK = dK ? d_K + nK : nullptr;
  hipLaunchKernelGGL(full_cov_kernel, dim3((Mc + 63) / 64, (N + 3) / 4), dim3(64, 4), 0, st, cd,
                     (const double*)s_xa, (const double*)s_xb, sf2, rqa, N, Mc, d_K, d_dK);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, c->pin.down(K, d_K, nK * 8, st));
  if (dK) HIPCHK(c, c->pin.down(dK, d_dK, ndK * 8, st));
  HIPCHK(c, hipStreamSynchronize(st));
  c->pin.finish();
  return 0;
}

int gpc_nll_batch(gpc_ctx* c, int kernel_id, int degree, int dtype, int S, const double* hyp_cov,
                  const double* m, const double* sn2, int sn2_is_vector, int want_grad, const double* dm,
                  int mean_N, const double* dsn2, int noise_N, double* nlz, double* dnlz, double* sn2_mult,
                  int* L_chol, int* info) {
  int rc = check_batch_args(c, kernel_id, degree, dtype, S);
  if (rc) return rc;
  if (!hyp_cov || !m || !sn2 || !nlz || !sn2_mult || !L_chol || !info) FAIL(c, "gpc_nll_batch: null argument");
  if (want_grad && (!dnlz || (mean_N > 0 && !dm) || (noise_N > 0 && !dsn2)))
    FAIL(c, "gpc_nll_batch: gradient requested without dnlz/dm/dsn2");
  HIPCHK(c, hipSetDevice(c->device));
  HostClock hc("nll");
  Batch b;
  fill_batch(c, b, kernel_id, degree, S, hyp_cov, m, sn2, sn2_is_vector);
  hc.lap("fill_batch");
  if (dtype == GPC_F64)
    return nll_impl<double>(c, b, want_grad, dm, mean_N, dsn2, noise_N, nlz, dnlz, sn2_mult, L_chol, info);
  return nll_impl<float>(c, b, want_grad, dm, mean_N, dsn2, noise_N, nlz, dnlz, sn2_mult, L_chol, info);
}

int gpc_nll_batch_cm(gpc_ctx* c, int kernel_id, int degree, int dtype, int S, const double* hyp_cov,
                     const double* m0, int mean_N, const double* sn2, int sn2_is_vector, int want_grad,
                     const double* dsn2, int noise_N, double* nlz, double* dnlz, double* sn2_mult, int* L_chol,
                     int* info) {
  int rc = check_batch_args(c, kernel_id, degree, dtype, S);
  if (rc) return rc;
  if (!hyp_cov || !sn2 || !nlz || !sn2_mult || !L_chol || !info) FAIL(c, "gpc_nll_batch_cm: null argument");
  if (mean_N < 0 || mean_N > 1 || (mean_N == 1 && !m0)) FAIL(c, "gpc_nll_batch_cm: mean_N must be 0 (zero mean) or 1 (m0 given)");
  if (want_grad && (!dnlz || (noise_N > 0 && !dsn2))) FAIL(c, "gpc_nll_batch_cm: gradient requested without dnlz/dsn2");
  HIPCHK(c, hipSetDevice(c->device));
  HostClock hc("nll");
  std::vector<double> zero;
  if (!m0) {
    zero.assign(S, 0.0);
    m0 = zero.data();
  }
  Batch b;
  fill_batch(c, b, kernel_id, degree, S, hyp_cov, m0, sn2, sn2_is_vector, true);
  hc.lap("fill_batch");
  // dm = nullptr with mean_N = 1: the constant mean's derivative (ones), summed on the device
  if (dtype == GPC_F64)
    return nll_impl<double>(c, b, want_grad, nullptr, mean_N, dsn2, noise_N, nlz, dnlz, sn2_mult, L_chol, info);
  return nll_impl<float>(c, b, want_grad, nullptr, mean_N, dsn2, noise_N, nlz, dnlz, sn2_mult, L_chol, info);
}

int gpc_posterior_batch(gpc_ctx* c, int kernel_id, int degree, int dtype, int S, const double* hyp_cov,
                        const double* m, const double* sn2, int sn2_is_vector, gpc_post** post,
                        double* sn2_mult, int* L_chol, int* info) {
  int rc = check_batch_args(c, kernel_id, degree, dtype, S);
  if (rc) return rc;
  if (!hyp_cov || !m || !sn2 || !post || !sn2_mult || !L_chol || !info) FAIL(c, "gpc_posterior_batch: null argument");
  HIPCHK(c, hipSetDevice(c->device));
  Batch b;
  fill_batch(c, b, kernel_id, degree, S, hyp_cov, m, sn2, sn2_is_vector);
  gpc_post* po = new gpc_post();
  po->ctx = c;
  po->dtype = dtype;
  po->S = S;
  po->N = c->N;
  po->D = c->D;
  po->npad = c->npad;
  po->cd = b.cd;
  rc = (dtype == GPC_F64) ? post_impl<double>(c, b, po, sn2_mult, L_chol, info)
                          : post_impl<float>(c, b, po, sn2_mult, L_chol, info);
  if (rc) {
    c->pool_give(po->A);
    c->pool_give(po->W);
    c->pool_give(po->alpha);
    delete po;
    return rc;
  }
  *post = po;
  return 0;
}

int gpc_nll_batch_K(gpc_ctx* c, int dtype, int S, int cov_N, const double* K, gpc_dk_plane_fn dk_plane, void* user,
                    const double* m, const double* sn2, int sn2_is_vector, int want_grad, const double* dm,
                    int mean_N, const double* dsn2, int noise_N, double* nlz, double* dnlz, double* sn2_mult,
                    int* L_chol, int* info) {
  int rc = check_batch_args(c, -1, 0, dtype, S);
  if (rc) return rc;
  if (!K || !m || !sn2 || !nlz || !sn2_mult || !L_chol || !info || cov_N < 0) FAIL(c, "gpc_nll_batch_K: bad argument");
  if (want_grad && (!dnlz || (cov_N > 0 && !dk_plane) || (mean_N > 0 && !dm) || (noise_N > 0 && !dsn2)))
    FAIL(c, "gpc_nll_batch_K: gradient requested without dnlz / dK callback / dm / dsn2");
  HIPCHK(c, hipSetDevice(c->device));
  Batch b;
  fill_batch(c, b, -1, cov_N, S, nullptr, m, sn2, sn2_is_vector);
  KArgs km{K, dk_plane, user};
  if (dtype == GPC_F64)
    return nll_impl<double>(c, b, want_grad, dm, mean_N, dsn2, noise_N, nlz, dnlz, sn2_mult, L_chol, info, &km);
  return nll_impl<float>(c, b, want_grad, dm, mean_N, dsn2, noise_N, nlz, dnlz, sn2_mult, L_chol, info, &km);
}

int gpc_posterior_batch_K(gpc_ctx* c, int dtype, int S, const double* K, const double* m, const double* sn2,
                          int sn2_is_vector, gpc_post** post, double* sn2_mult, int* L_chol, int* info) {
  int rc = check_batch_args(c, -1, 0, dtype, S);
  if (rc) return rc;
  if (!K || !m || !sn2 || !post || !sn2_mult || !L_chol || !info) FAIL(c, "gpc_posterior_batch_K: null argument");
  HIPCHK(c, hipSetDevice(c->device));
  Batch b;
  fill_batch(c, b, -1, 0, S, nullptr, m, sn2, sn2_is_vector);
  gpc_post* po = new gpc_post();
  po->ctx = c;
  po->dtype = dtype;
  po->S = S;
  po->N = c->N;
  po->D = c->D;
  po->npad = c->npad;
  po->cd = b.cd;
  KArgs km{K, nullptr, nullptr};
  rc = (dtype == GPC_F64) ? post_impl<double>(c, b, po, sn2_mult, L_chol, info, &km)
                          : post_impl<float>(c, b, po, sn2_mult, L_chol, info, &km);
  if (rc) {
    c->pool_give(po->A);
    c->pool_give(po->W);
    c->pool_give(po->alpha);
    delete po;
    return rc;
  }
  *post = po;
  return 0;
}

int gpc_predict_K(gpc_post* po, int M, const double* Ks, const double* Kss, double* fmu, double* fq, double* cov) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!Ks || !fmu || M <= 0 || (!fq && !cov) || (cov && !Kss)) FAIL(c, "gpc_predict_K: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (int rc = require_factorized(po, "gpc_predict_K")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  RhsRequest r;
  r.rhs = RhsRequest::GIVEN_KS;
  r.xa = Ks;
  r.xb = Kss;
  r.M = M;
  r.want_quad = fq != nullptr;
  r.lin = fmu;
  r.quad = fq;
  r.full = cov;
  int rc = rhs_products(po, r);
  if (rc || !fq) return rc;
  for (int s = 0; s < po->S; ++s) {  // the term the caller adds to kss (:1752-1764)
    const double sl = po->sp[(size_t)s * SP_STRIDE + SP_SL];
    for (int j = 0; j < M; ++j) {
      double& q = fq[(size_t)j * po->S + s];
      q = po->lchol[s] ? -q / sl : q;
    }
  }
  return 0;
}

// ---- gradient observations (gradobs.h): the K-mode pipeline with the joint matrix built on the device ----
namespace {
int gobs_kernel_check(gpc_ctx* c, int kernel_id, int degree, const char* fn) {
  if (kernel_id < 0 || !valid_kernel(kernel_id, degree))
    FAIL(c, std::string(fn) + ": unknown covariance kernel / degree (gradient observations need a built-in kernel)");
  if ((kernel_id == K_MATERN || kernel_id == K_MATERN_ISO) && degree == 1)
    FAIL(c, std::string(fn) + ": the Matern kernel of degree 1 has no mean-square derivative (the prior variance of its "
                              "gradient is infinite)");
  return 0;
}
int gobs_dims_check(gpc_ctx* c, const GobsDims& gd, const char* fn) {
  if (gd.N <= 0 || gd.Ng <= 0 || gd.D <= 0) FAIL(c, std::string(fn) + ": N, Ng and D must be positive");
  if (gd.n() > (1 << 20)) FAIL(c, std::string(fn) + ": the joint order N + Ng D is beyond 2^20");
  return 0;
}
// the raw point list of gradobs.h: X in rows [0, N), X_g from row pad64(N) on, zero rows elsewhere
void gobs_point_list(const GobsDims& gd, const double* X, const double* Xg, std::vector<double>& pts) {
  pts.assign((size_t)gd.P() * gd.D, 0.0);
  std::copy_n(X, (size_t)gd.N * gd.D, pts.begin());
  std::copy_n(Xg, (size_t)gd.Ng * gd.D, pts.begin() + (size_t)gd.Np() * gd.D);
}
}  // namespace

int gpc_set_data_gobs(gpc_ctx* c, const double* X, const double* y, int N, int D, const double* Xg, const double* dy,
                      int Ng) {
  if (!c) return -2;
  if (!X || !y || !Xg || !dy) FAIL(c, "gpc_set_data_gobs: null argument");
  GobsDims gd;
  gd.N = N, gd.Ng = Ng, gd.D = D;
  if (int rc = gobs_dims_check(c, gd, "gpc_set_data_gobs")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const int n = (int)gd.n();
  std::vector<double> pts, t((size_t)n);
  gobs_point_list(gd, X, Xg, pts);
  std::copy_n(y, N, t.begin());
  for (int g = 0; g < Ng; ++g)
    for (int l = 0; l < D; ++l) t[(size_t)N + (size_t)l * Ng + g] = dy[(size_t)g * D + l];  // dimension-major joint rows
  HIPCHK(c, c->gpts.ensure(pts.size() * sizeof(double)));
  HIPCHK(c, c->dY.ensure((size_t)n * sizeof(double)));
  HIPCHK(c, hipMemcpyAsync(c->gpts.p, pts.data(), pts.size() * sizeof(double), hipMemcpyHostToDevice, c->st));
  HIPCHK(c, hipMemcpyAsync(c->dY.p, t.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  c->hy = t;
  c->N = n;
  c->D = D;
  c->npad = pad_tile(n);
  c->gobs = gd;
  return 0;
}

int gpc_posterior_batch_gobs(gpc_ctx* c, int kernel_id, int degree, int dtype, int S, const double* hyp_cov,
                             const double* m, const double* sn2, gpc_post** post, double* nlz, double* sn2_mult,
                             int* L_chol, int* info) {
  if (!c) return -2;
  if (int rc = gobs_kernel_check(c, kernel_id, degree, "gpc_posterior_batch_gobs")) return rc;
  if (int rc = check_batch_args(c, kernel_id, degree, dtype, S, true)) return rc;
  if (!hyp_cov || !m || !sn2 || !post || !sn2_mult || !L_chol || !info) FAIL(c, "gpc_posterior_batch_gobs: null argument");
  HIPCHK(c, hipSetDevice(c->device));
  Batch b;
  fill_batch(c, b, kernel_id, degree, S, hyp_cov, m, sn2, 1);
  gpc_post* po = new gpc_post();
  po->ctx = c;
  po->dtype = dtype;
  po->S = S;
  po->N = c->N;
  po->D = c->D;
  po->npad = c->npad;
  po->cd = b.cd;
  po->gobs = c->gobs;
  KArgs km;
  km.gobs = c->gobs;
  const size_t pb = (size_t)c->gobs.P() * c->D * sizeof(double);
  hipError_t e = po->gpts.ensure_private(pb);
  if (e == hipSuccess) e = hipMemcpyAsync(po->gpts.p, c->gpts.p, pb, hipMemcpyDeviceToDevice, c->st);
  int rc = 0;
  if (e != hipSuccess) {
    c->err = std::string("gpc_posterior_batch_gobs: ") + hipGetErrorString(e);
    rc = -1;
  } else {
    rc = (dtype == GPC_F64) ? post_impl<double>(c, b, po, sn2_mult, L_chol, info, &km, nlz)
                            : post_impl<float>(c, b, po, sn2_mult, L_chol, info, &km, nlz);
  }
  if (rc) {
    c->pool_give(po->A);
    c->pool_give(po->W);
    c->pool_give(po->alpha);
    po->gpts.release();
    delete po;
    return rc;
  }
  *post = po;
  return 0;
}

int gpc_nll_batch_gobs(gpc_ctx* c, int kernel_id, int degree, int dtype, int S, const double* hyp_cov, const double* m,
                       const double* sn2, double* nlz, double* sn2_mult, int* L_chol, int* info) {
  if (!c) return -2;
  if (int rc = gobs_kernel_check(c, kernel_id, degree, "gpc_nll_batch_gobs")) return rc;
  if (int rc = check_batch_args(c, kernel_id, degree, dtype, S, true)) return rc;
  if (!hyp_cov || !m || !sn2 || !nlz || !sn2_mult || !L_chol || !info) FAIL(c, "gpc_nll_batch_gobs: null argument");
  HIPCHK(c, hipSetDevice(c->device));
  Batch b;
  fill_batch(c, b, kernel_id, degree, S, hyp_cov, m, sn2, 1);
  KArgs km;
  km.gobs = c->gobs;
  if (dtype == GPC_F64) return nll_impl<double>(c, b, 0, nullptr, 0, nullptr, 0, nlz, nullptr, sn2_mult, L_chol, info, &km);
  return nll_impl<float>(c, b, 0, nullptr, 0, nullptr, 0, nlz, nullptr, sn2_mult, L_chol, info, &km);
}

int gpc_nll_batch_gobs_grad(gpc_ctx* c, int kernel_id, int degree, int dtype, int S, const double* hyp_cov, const double* m,
                            const double* sn2, const double* dm, int mean_N, const double* dsn2, int noise_N, double* nlz,
                            double* dnlz, double* sn2_mult, int* L_chol, int* info) {
  if (!c) return -2;
  if (int rc = gobs_kernel_check(c, kernel_id, degree, "gpc_nll_batch_gobs_grad")) return rc;
  if (int rc = check_batch_args(c, kernel_id, degree, dtype, S, true)) return rc;
  if (dtype != GPC_F64)
    FAIL(c, "gpc_nll_batch_gobs_grad: fp64 only (the contraction reads the inverse in the precision it accumulates in); "
            "dtype must be GPC_F64");
  if (!hyp_cov || !m || !sn2 || !nlz || !dnlz || !sn2_mult || !L_chol || !info) FAIL(c, "gpc_nll_batch_gobs_grad: null argument");
  if (mean_N < 0 || noise_N < 0 || (mean_N > 0 && !dm) || (noise_N > 0 && !dsn2))
    FAIL(c, "gpc_nll_batch_gobs_grad: mean_N / noise_N hyperparameters need their joint-ordered rows dm / dsn2");
  HIPCHK(c, hipSetDevice(c->device));
  Batch b;
  fill_batch(c, b, kernel_id, degree, S, hyp_cov, m, sn2, 1);
  KArgs km;
  km.gobs = c->gobs;
  return nll_impl<double>(c, b, 1, dm, mean_N, dsn2, noise_N, nlz, dnlz, sn2_mult, L_chol, info, &km);
}

int gpc_predict_gobs(gpc_post* po, const double* xstar, int M, double* fmu, double* fs2) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!xstar || !fmu || !fs2 || M <= 0) FAIL(c, "gpc_predict_gobs: bad arguments");
  if (po->gobs.Ng <= 0)
    FAIL(c, "gpc_predict_gobs: this posterior holds no gradient observations (gpc_posterior_batch_gobs builds those); use "
            "gpc_predict");
  if (int rc = require_factorized(po, "gpc_predict_gobs")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? predict_impl<double>(po, xstar, M, fmu, fs2, nullptr, nullptr, RhsRequest::GOBS)
                              : predict_impl<float>(po, xstar, M, fmu, fs2, nullptr, nullptr, RhsRequest::GOBS);
}

namespace {
// what both debug hooks start from: one sample's raw and scaled point list, scaling and scalars in dbg2
struct GobsDebug {
  GobsDims gd;
  CovDesc cd{};
  double *pts = nullptr, *xs = nullptr, *mul = nullptr, *dv = nullptr, *sp = nullptr, *rest = nullptr;
};
int gobs_debug_begin(gpc_ctx* c, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                     const double* Xg, int Ng, size_t extra_doubles, GobsDebug& g, const char* fn) {
  if (int rc = gobs_kernel_check(c, kernel_id, degree, fn)) return rc;
  if (!hyp_cov || !X || !Xg) FAIL(c, std::string(fn) + ": null argument");
  g.gd.N = N, g.gd.Ng = Ng, g.gd.D = D;
  if (int rc = gobs_dims_check(c, g.gd, fn)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  g.cd = CovDesc{kernel_id, degree, D, cov_count_of(kernel_id, D)};
  const size_t pd = (size_t)g.gd.P() * D;
  std::vector<double> h(2 * (size_t)D + SP_STRIDE, 0.0);
  scaling_of(kernel_id, degree, D, hyp_cov, &h[0], &h[D], &h[2 * D + SP_SF2], &h[2 * D + SP_RQA]);
  h[2 * D + SP_KSCALE] = h[2 * D + SP_SL] = 1.0;
  std::vector<double> pts;
  gobs_point_list(g.gd, X, Xg, pts);
  HIPCHK(c, c->dbg2.ensure((2 * pd + h.size() + extra_doubles) * 8));
  g.pts = c->dbg2.as<double>();
  g.xs = g.pts + pd;
  g.mul = g.xs + pd;
  g.dv = g.mul + D;
  g.sp = g.dv + D;
  g.rest = g.sp + SP_STRIDE;
  HIPCHK(c, hipMemcpyAsync(g.pts, pts.data(), pd * 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(c, hipMemcpyAsync(g.mul, h.data(), h.size() * 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));  // (the host vectors go out of scope)
  launch_gobs_scale(c->st, g.gd, g.pts, g.mul, g.dv, 1, g.xs);
  HIPCHK(c, hipGetLastError());
  return 0;
}
}  // namespace

int gpc_debug_gobs_cov(gpc_ctx* c, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                       const double* Xg, int Ng, double* out) {
  if (!c) return -2;
  if (!out) FAIL(c, "gpc_debug_gobs_cov: null argument");
  GobsDebug g;
  if (int rc = gobs_debug_begin(c, kernel_id, degree, hyp_cov, X, N, D, Xg, Ng, 0, g, "gpc_debug_gobs_cov")) return rc;
  const size_t nn = (size_t)g.gd.n() * (size_t)g.gd.n();
  HIPCHK(c, c->dbg1.ensure(nn * 8));
  HIPCHK(c, hipMemsetAsync(c->dbg1.p, 0xFF, nn * 8, c->st));  // (NaN: an entry no block wrote shows)
  GramClock clk(true);
  HIPCHK(c, clk.record(0, c->st));
  launch_gobs_cov(c->st, g.cd, g.gd, g.xs, g.sp, g.mul, g.dv, c->dbg1.as<double>());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, clk.record(1, c->st));
  HIPCHK(c, hipMemcpyAsync(out, c->dbg1.p, nn * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  c->gobs_cov_us = (unsigned long long)clk.elapsed_us();
  return 0;
}

int gpc_debug_gobs_trace(gpc_ctx* c, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                         const double* Xg, int Ng, const double* Ainv, const double* alpha, double sl, double* out) {
  if (!c) return -2;
  if (!Ainv || !alpha || !out || !(sl > 0.0)) FAIL(c, "gpc_debug_gobs_trace: bad arguments");
  GobsDims gd;
  gd.N = N, gd.Ng = Ng, gd.D = D;
  if (int rc = gobs_dims_check(c, gd, "gpc_debug_gobs_trace")) return rc;
  if (kernel_id < 0 || !valid_kernel(kernel_id, degree)) FAIL(c, "gpc_debug_gobs_trace: unknown covariance kernel / degree");
  const size_t n = (size_t)gd.n();
  const int cov_N = cov_count_of(kernel_id, D);
  // after the common part: alpha n | the sums cov_N | the per-tile partials (scratch.h: GobsTraceScratch)
  const size_t head = (n + cov_N + 1) & ~(size_t)1;
  const size_t extra = head + ScratchCarver::count<GobsTraceScratch>(1, gd, cov_N) / 8;
  GobsDebug g;
  if (int rc = gobs_debug_begin(c, kernel_id, degree, hyp_cov, X, N, D, Xg, Ng, extra, g, "gpc_debug_gobs_trace")) return rc;
  double* d_alpha = g.rest;
  double* d_out = d_alpha + n;
  GobsTraceScratch z;
  CARVECHK(c, "gpc_debug_gobs_trace", ScratchCarver::carve(z, g.rest + head, 1, gd, cov_N));
  hipStream_t st = c->st;
  HIPCHK(c, c->dbg1.ensure(n * n * 8));
  HIPCHK(c, hipMemcpyAsync(c->dbg1.p, Ainv, n * n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_alpha, alpha, n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(g.sp + SP_SL, &sl, 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));
  GramClock clk(true);
  HIPCHK(c, clk.record(0, st));
  launch_gobs_trace(st, g.cd, g.gd, 1, g.xs, g.sp, g.mul, g.dv, c->dbg1.as<double>(), 0, (int)n, d_alpha, 0, z.part, cov_N,
                    d_out);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, clk.record(1, st));
  HIPCHK(c, hipMemcpyAsync(out, d_out, (size_t)cov_N * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  c->gobs_trace_us = (unsigned long long)clk.elapsed_us();
  return 0;
}

int gpc_debug_gobs_cross(gpc_ctx* c, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                         const double* Xg, int Ng, const double* xstar, int M, const double* alpha, double* out,
                         double* colsum) {
  if (!c) return -2;
  if (!xstar || !out || M <= 0) FAIL(c, "gpc_debug_gobs_cross: bad arguments");
  const int mpad = pad_tile(M);
  GobsDims gd;
  gd.N = N, gd.Ng = Ng, gd.D = D;
  if (int rc = gobs_dims_check(c, gd, "gpc_debug_gobs_cross")) return rc;
  const int n = (int)gd.n(), npad = pad_tile(n), pt = gd.P() / CT;
  // after the common part: raw queries M x D | scaled queries mpad x D | alpha npad | partials pt x mpad | sums mpad
  const size_t extra = (size_t)M * D + (size_t)mpad * D + npad + (size_t)pt * mpad + mpad;
  GobsDebug g;
  if (int rc = gobs_debug_begin(c, kernel_id, degree, hyp_cov, X, N, D, Xg, Ng, extra, g, "gpc_debug_gobs_cross")) return rc;
  double* d_xq = g.rest;
  double* d_xss = d_xq + (size_t)M * D;
  double* d_alpha = d_xss + (size_t)mpad * D;
  double* d_part = d_alpha + npad;
  double* d_mu = d_part + (size_t)pt * mpad;
  hipStream_t st = c->st;
  HIPCHK(c, hipMemcpyAsync(d_xq, xstar, (size_t)M * D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(d_alpha, 0, (size_t)npad * 8, st));
  if (alpha) HIPCHK(c, hipMemcpyAsync(d_alpha, alpha, (size_t)n * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)mpad * D + 255) / 256), 1), dim3(256), 0, st,
                     (const double*)d_xq, M, mpad, D, (const double*)g.mul, (const double*)g.dv, d_xss);
  const size_t pb = (size_t)npad * mpad * 8;
  HIPCHK(c, c->dbg1.ensure(pb));
  HIPCHK(c, hipMemsetAsync(c->dbg1.p, 0xFF, pb, st));  // (NaN: padding the kernel left unwritten shows)
  GramClock clk(true);
  HIPCHK(c, clk.record(0, st));
  HIPCHK(c, launch_gobs_cross<double>(st, g.cd, g.gd, g.xs, d_xss, g.sp, g.mul, g.dv, d_alpha, npad, npad, M, mpad, 1,
                                      c->dbg1.as<double>(), (long long)npad * mpad, d_part, d_mu));
  HIPCHK(c, clk.record(1, st));
  HIPCHK(c, hipMemcpyAsync(out, c->dbg1.p, pb, hipMemcpyDeviceToHost, st));
  if (colsum) HIPCHK(c, hipMemcpyAsync(colsum, d_mu, (size_t)mpad * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  c->gobs_cross_us = (unsigned long long)clk.elapsed_us();
  return 0;
}

int gpc_debug_gobs_grad_operand(gpc_ctx* c, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                                const double* Xg, int Ng, const double* xstar, int M, const double* alpha, double* out,
                                double* colsum) {
  if (!c) return -2;
  if (!xstar || !out || M <= 0 || M > GQB) FAIL(c, "gpc_debug_gobs_grad_operand: bad arguments (one block: M <= 128)");
  const int mb = GQB, ld = (D + 1) * mb;
  GobsDims gd;
  gd.N = N, gd.Ng = Ng, gd.D = D;
  if (int rc = gobs_dims_check(c, gd, "gpc_debug_gobs_grad_operand")) return rc;
  const int n = (int)gd.n(), npad = pad_tile(n), pt = gd.P() / CT;
  // after the common part: raw queries M x D | scaled queries mb x D | alpha npad | partials pt x ld | sums ld | F0 (2)
  const size_t extra = (size_t)M * D + (size_t)mb * D + npad + (size_t)pt * ld + ld + 2;
  GobsDebug g;
  if (int rc = gobs_debug_begin(c, kernel_id, degree, hyp_cov, X, N, D, Xg, Ng, extra, g, "gpc_debug_gobs_grad_operand"))
    return rc;
  double* d_xq = g.rest;
  double* d_xss = d_xq + (size_t)M * D;
  double* d_alpha = d_xss + (size_t)mb * D;
  double* d_part = d_alpha + npad;
  double* d_mu = d_part + (size_t)pt * ld;
  double* d_f0 = d_mu + ld;
  hipStream_t st = c->st;
  HIPCHK(c, hipMemcpyAsync(d_xq, xstar, (size_t)M * D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(d_alpha, 0, (size_t)npad * 8, st));
  if (alpha) HIPCHK(c, hipMemcpyAsync(d_alpha, alpha, (size_t)n * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)mb * D + 255) / 256), 1), dim3(256), 0, st,
                     (const double*)d_xq, M, mb, D, (const double*)g.mul, (const double*)g.dv, d_xss);
  const size_t pb = (size_t)npad * ld * 8;
  HIPCHK(c, c->dbg1.ensure(pb));
  HIPCHK(c, hipMemsetAsync(c->dbg1.p, 0xFF, pb, st));  // (NaN: an entry nobody wrote shows)
  GramClock clk(true);
  HIPCHK(c, clk.record(0, st));
  HIPCHK(c, launch_gobs_grad_operand<double>(st, g.cd, g.gd, g.xs, d_xss, g.sp, g.mul, g.dv, d_alpha, npad, npad, M, 1,
                                             c->dbg1.as<double>(), (long long)npad * ld, d_part, d_mu, d_f0));
  HIPCHK(c, clk.record(1, st));
  HIPCHK(c, hipMemcpyAsync(out, c->dbg1.p, pb, hipMemcpyDeviceToHost, st));
  if (colsum) HIPCHK(c, hipMemcpyAsync(colsum, d_mu, (size_t)ld * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  c->gobs_grad_operand_us = (unsigned long long)clk.elapsed_us();
  return 0;
}

int gpc_post_fetch(gpc_post* po, int s, double* alpha, double* sW, double* L) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (s < 0 || s >= po->S) FAIL(c, "gpc_post_fetch: sample index out of range");
  HIPCHK(c, hipSetDevice(c->device));
  const int N = po->N, npad = po->npad;
  c->pin.begin();
  if (alpha) HIPCHK(c, c->pin.down(alpha, po->alpha.as<double>() + (size_t)s * npad, N * sizeof(double), c->st));
  if (sW)
    for (int i = 0; i < N; ++i) sW[i] = po->sW[s];
  if (L) {
    HIPCHK(c, c->dbg3.ensure((size_t)N * N * 8));
    dim3 grid((N + 63) / 64, (N + 3) / 4), blk(64, 4);
    const int mode = po->lchol[s] ? 0 : 2;  // low-noise: A already holds the full -inv
    if (po->dtype == GPC_F64)
      hipLaunchKernelGGL((extract_kernel<double>), grid, blk, 0, c->st,
                         (const double*)(po->A.as<double>() + (size_t)s * npad * npad), npad, N, mode,
                         c->dbg3.as<double>());
    else
      hipLaunchKernelGGL((extract_kernel<float>), grid, blk, 0, c->st,
                         (const float*)(po->A.as<float>() + (size_t)s * npad * npad), npad, N, mode,
                         c->dbg3.as<double>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, c->pin.down(L, c->dbg3.p, (size_t)N * N * 8, c->st));
  }
  HIPCHK(c, hipStreamSynchronize(c->st));
  c->pin.finish();
  return 0;
}

int gpc_post_free(gpc_post* po) {
  if (!po) return 0;
  (void)hipSetDevice(po->ctx->device);
  (void)hipStreamSynchronize(po->ctx->st);
  po->ctx->pool_give(po->A);
  po->ctx->pool_give(po->W);
  po->ctx->pool_give(po->alpha);
  po->dsp.release();
  po->dmul.release();
  po->ddv.release();
  po->dxs.release();
  po->gpts.release();
  delete po;
  return 0;
}

int gpc_post_append(gpc_post* po, const double* m_star, const double* sn2_star, double y_new, int* ok) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!m_star || !sn2_star || !ok) FAIL(c, "gpc_post_append: null argument");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0) FAIL(c, "gpc_post_append: not available for posteriors built from caller-provided K");
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? append_impl<double>(po, m_star, sn2_star, y_new, ok)
                              : append_impl<float>(po, m_star, sn2_star, y_new, ok);
}

int gpc_post_append_K(gpc_post* po, const double* Ks, const double* kss, const double* m_star,
                      const double* sn2_star, double y_new, int* ok) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!Ks || !kss || !m_star || !sn2_star || !ok) FAIL(c, "gpc_post_append_K: null argument");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind >= 0) FAIL(c, "gpc_post_append_K: this posterior was built from a device kernel; use gpc_post_append");
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? append_impl<double>(po, m_star, sn2_star, y_new, ok, Ks, kss)
                              : append_impl<float>(po, m_star, sn2_star, y_new, ok, Ks, kss);
}

namespace {
// full recompute of the listed samples of a resident posterior set, in place (device kernel: hyp_cov; K-mode: K)
int recompute_impl(gpc_post* po, int cnt, const int* idx, const double* hyp_cov, const double* K, const double* m,
                   const double* sn2, int sn2_is_vector, double* sn2_mult, int* L_chol, int* info) {
  gpc_ctx* c = po->ctx;
  if (c->N != po->N || c->D != po->D) FAIL(c, "gpc_post_recompute: the context's data do not match the posterior");
  for (int i = 0; i < cnt; ++i)
    if (idx[i] < 0 || idx[i] >= po->S) FAIL(c, "gpc_post_recompute: sample index out of range");
  HIPCHK(c, hipSetDevice(c->device));
  Batch b;
  if (K)
    fill_batch(c, b, -1, 0, cnt, nullptr, m, sn2, sn2_is_vector);
  else
    fill_batch(c, b, po->cd.kind, po->cd.degree, cnt, hyp_cov, m, sn2, sn2_is_vector);
  gpc_post tmp;
  tmp.ctx = c;
  tmp.dtype = po->dtype;
  tmp.S = cnt;
  tmp.N = c->N;
  tmp.D = c->D;
  tmp.npad = c->npad;
  tmp.cd = b.cd;
  if (tmp.npad != po->npad) FAIL(c, "gpc_post_recompute: padded size mismatch");
  KArgs km{K, nullptr, nullptr};
  int rc = (po->dtype == GPC_F64) ? post_impl<double>(c, b, &tmp, sn2_mult, L_chol, info, K ? &km : nullptr)
                                  : post_impl<float>(c, b, &tmp, sn2_mult, L_chol, info, K ? &km : nullptr);
  if (rc == 0) {
    const size_t w = po->dtype == GPC_F64 ? 8 : 4, msz = (size_t)po->npad * po->npad * w;
    for (int i = 0; i < cnt && rc == 0; ++i) {
      const int s = idx[i];
      hipError_t e = hipMemcpyAsync((char*)po->A.p + (size_t)s * msz, (char*)tmp.A.p + (size_t)i * msz, msz,
                                    hipMemcpyDeviceToDevice, c->st);
      if (e == hipSuccess)
        e = hipMemcpyAsync((char*)po->W.p + (size_t)s * msz, (char*)tmp.W.p + (size_t)i * msz, msz,
                           hipMemcpyDeviceToDevice, c->st);
      if (e == hipSuccess)
        e = hipMemcpyAsync(po->alpha.as<double>() + (size_t)s * po->npad, tmp.alpha.as<double>() + (size_t)i * po->npad,
                           (size_t)po->npad * 8, hipMemcpyDeviceToDevice, c->st);
      if (e != hipSuccess) {
        c->err = std::string("gpc_post_recompute copy: ") + hipGetErrorString(e);
        rc = -1;
        break;
      }
      po->dev_consts = false;
      std::copy_n(&tmp.sp[(size_t)i * SP_STRIDE], SP_STRIDE, &po->sp[(size_t)s * SP_STRIDE]);
      std::copy_n(&tmp.mul[(size_t)i * po->D], po->D, &po->mul[(size_t)s * po->D]);
      std::copy_n(&tmp.dv[(size_t)i * po->D], po->D, &po->dv[(size_t)s * po->D]);
      po->mult[s] = tmp.mult[i];
      po->lchol[s] = tmp.lchol[i];
      po->info[s] = tmp.info[i];
      po->sW[s] = tmp.sW[i];
    }
    (void)hipStreamSynchronize(c->st);
  }
  c->pool_give(tmp.A);
  c->pool_give(tmp.W);
  c->pool_give(tmp.alpha);
  return rc;
}
}  // namespace

int gpc_post_recompute(gpc_post* po, int cnt, const int* idx, const double* hyp_cov, const double* m,
                       const double* sn2, int sn2_is_vector, double* sn2_mult, int* L_chol, int* info) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (cnt <= 0 || !idx || !hyp_cov || !m || !sn2 || !sn2_mult || !L_chol || !info)
    FAIL(c, "gpc_post_recompute: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0) FAIL(c, "gpc_post_recompute: this posterior was built from caller-provided K; use gpc_post_recompute_K");
  return recompute_impl(po, cnt, idx, hyp_cov, nullptr, m, sn2, sn2_is_vector, sn2_mult, L_chol, info);
}

int gpc_post_append_block(gpc_post* po, int k, const double* m_star, const double* sn2_star, const double* y_new,
                          int* ok) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!m_star || !sn2_star || !y_new || !ok) FAIL(c, "gpc_post_append_block: null argument");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_post_append_block: not available for posteriors built from caller-provided K; use gpc_post_append_block_K");
  if (int rc = append_block_check(po, k, "gpc_post_append_block")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? append_block_impl<double>(po, k, m_star, sn2_star, y_new, ok)
                              : append_block_impl<float>(po, k, m_star, sn2_star, y_new, ok);
}

int gpc_post_append_block_K(gpc_post* po, int k, const double* Ks, const double* Kss, const double* m_star,
                            const double* sn2_star, const double* y_new, int* ok) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!Ks || !Kss || !m_star || !sn2_star || !y_new || !ok) FAIL(c, "gpc_post_append_block_K: null argument");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind >= 0)
    FAIL(c, "gpc_post_append_block_K: this posterior was built from a device kernel; use gpc_post_append_block");
  if (int rc = append_block_check(po, k, "gpc_post_append_block_K")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? append_block_impl<double>(po, k, m_star, sn2_star, y_new, ok, Ks, Kss)
                              : append_block_impl<float>(po, k, m_star, sn2_star, y_new, ok, Ks, Kss);
}

int gpc_post_remove(gpc_post* po, int k, const int* idx, const double* ym, int* ok) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!idx || !ym || !ok) FAIL(c, "gpc_post_remove: null argument");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (k < 1 || k >= po->N)
    FAIL(c, "gpc_post_remove: k = " + std::to_string(k) + " must be at least 1 and less than N = " + std::to_string(po->N));
  for (int j = 0; j < k; ++j)
    if (idx[j] < 0 || idx[j] >= po->N || (j > 0 && idx[j] <= idx[j - 1]))
      FAIL(c, "gpc_post_remove: the indices must be sorted, distinct and in [0, N)");
  if (c->N != po->N - k || c->D != po->D)
    FAIL(c, "gpc_post_remove: call gpc_set_data with the reduced X, y (N - k rows) first");
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? remove_impl<double>(po, k, idx, ym, ok) : remove_impl<float>(po, k, idx, ym, ok);
}

int gpc_debug_remove_panel(gpc_ctx* c, int dtype, int k, const double* D, const double* Vp, double* Theta, double* Dnew) {
  if (!c) return -2;
  if (!D || !Vp || !Theta || !Dnew) FAIL(c, "gpc_debug_remove_panel: null argument");
  if (k < 1 || k > RM_KMAX) FAIL(c, "gpc_debug_remove_panel: k must be in 1 .. 64");
  HIPCHK(c, hipSetDevice(c->device));
  return dtype == GPC_F64 ? debug_remove_panel_impl<double>(c, k, D, Vp, Theta, Dnew)
                          : debug_remove_panel_impl<float>(c, k, D, Vp, Theta, Dnew);
}

int gpc_debug_remove_apply(gpc_ctx* c, int dtype, int which, int a, int n, int k, const double* Theta, double* P,
                           double* Cr) {
  if (!c) return -2;
  if (!Theta || !P || !Cr) FAIL(c, "gpc_debug_remove_apply: null argument");
  if (k < 1 || k > RM_KMAX || a < 0 || a % RM_P || (which != 0 && which != 1) || n > 4096 ||
      (which == 0 ? n <= a + RM_P : n <= a))
    FAIL(c, "gpc_debug_remove_apply: bad shape (k in 1 .. 64, a a multiple of 64, n beyond the panel and at most 4096)");
  HIPCHK(c, hipSetDevice(c->device));
  return dtype == GPC_F64 ? debug_remove_apply_impl<double>(c, which, a, n, k, Theta, P, Cr)
                          : debug_remove_apply_impl<float>(c, which, a, n, k, Theta, P, Cr);
}

int gpc_post_recompute_K(gpc_post* po, int cnt, const int* idx, const double* K, const double* m, const double* sn2,
                         int sn2_is_vector, double* sn2_mult, int* L_chol, int* info) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (cnt <= 0 || !idx || !K || !m || !sn2 || !sn2_mult || !L_chol || !info)
    FAIL(c, "gpc_post_recompute_K: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind >= 0) FAIL(c, "gpc_post_recompute_K: this posterior was built from a device kernel; use gpc_post_recompute");
  return recompute_impl(po, cnt, idx, nullptr, K, m, sn2, sn2_is_vector, sn2_mult, L_chol, info);
}

int gpc_predict(gpc_post* po, const double* xstar, int M, double* fmu, double* fs2) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!xstar || !fmu || !fs2 || M <= 0) FAIL(c, "gpc_predict: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0) FAIL(c, "gpc_predict: this posterior was built from caller-provided K; use gpc_predict_K");
  if (int rc = require_factorized(po, "gpc_predict")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? predict_impl<double>(po, xstar, M, fmu, fs2)
                              : predict_impl<float>(po, xstar, M, fmu, fs2);
}

int gpc_predict_grad(gpc_post* po, const double* xstar, int M, double* fmu, double* fs2, double* dfmu, double* dfs2) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!xstar || !fmu || !fs2 || !dfmu || !dfs2 || M <= 0) FAIL(c, "gpc_predict_grad: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_predict_grad: this posterior was built from caller-provided K; a caller-provided kernel has no "
            "derivative with respect to x*");
  if (int rc = require_factorized(po, "gpc_predict_grad")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? predict_impl<double>(po, xstar, M, fmu, fs2, dfmu, dfs2)
                              : predict_impl<float>(po, xstar, M, fmu, fs2, dfmu, dfs2);
}

int gpc_grad_post(gpc_post* po, const double* xstar, int M, int diag_only, double* fmu, double* dfmu, double* cov) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!xstar || !fmu || !dfmu || !cov || M <= 0) FAIL(c, "gpc_grad_post: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_grad_post: this posterior was built from caller-provided K; a caller-provided kernel has no "
            "derivative with respect to x*");
  if ((po->cd.kind == K_MATERN || po->cd.kind == K_MATERN_ISO) && po->cd.degree == 1)
    FAIL(c, "gpc_grad_post: the Matern kernel of degree 1 has no mean-square derivative (its gradient has infinite "
            "prior variance)");
  if (int rc = require_factorized(po, "gpc_grad_post")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? grad_post_impl<double>(po, xstar, M, diag_only != 0, fmu, dfmu, cov)
                              : grad_post_impl<float>(po, xstar, M, diag_only != 0, fmu, dfmu, cov);
}

int gpc_grad_post_gobs(gpc_post* po, const double* xstar, int M, int diag_only, double* fmu, double* dfmu, double* cov) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!xstar || !fmu || !dfmu || !cov || M <= 0) FAIL(c, "gpc_grad_post_gobs: bad arguments");
  if (po->gobs.Ng <= 0)
    FAIL(c, "gpc_grad_post_gobs: this posterior holds no gradient observations (gpc_posterior_batch_gobs builds those); "
            "use gpc_grad_post");
  if (int rc = require_factorized(po, "gpc_grad_post_gobs")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? grad_post_impl<double>(po, xstar, M, diag_only != 0, fmu, dfmu, cov)
                              : grad_post_impl<float>(po, xstar, M, diag_only != 0, fmu, dfmu, cov);
}

int gpc_predict_hess(gpc_post* po, const double* xstar, int M, int compute_var, double* fmu, double* fs2, double* dfmu,
                     double* dfs2, double* hmu, double* hs2) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  const bool var = compute_var != 0;
  if (!xstar || !fmu || !dfmu || !hmu || (var && (!fs2 || !dfs2 || !hs2)) || M <= 0)
    FAIL(c, "gpc_predict_hess: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_predict_hess: this posterior was built from caller-provided K; a caller-provided kernel has no "
            "derivative with respect to x*");
  if ((po->cd.kind == K_MATERN || po->cd.kind == K_MATERN_ISO) && po->cd.degree == 1)
    FAIL(c, "gpc_predict_hess: the Matern kernel of degree 1 has no second derivative with respect to x*");
  if (int rc = require_factorized(po, "gpc_predict_hess")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? hess_impl<double>(po, xstar, M, var, fmu, fs2, dfmu, dfs2, hmu, hs2)
                              : hess_impl<float>(po, xstar, M, var, fmu, fs2, dfmu, dfs2, hmu, hs2);
}

int gpc_nll_hess(gpc_post* po, const double* dm, int mean_N, const double* dsn2, int dsn2_rows, int noise_N, double* H,
                 double* dnlz, double* alpha, double* diagq) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!H || !dnlz || !alpha || !diagq || mean_N < 0 || noise_N < 0 || (mean_N > 0 && !dm) || (noise_N > 0 && !dsn2) ||
      (noise_N > 0 && dsn2_rows != 1 && dsn2_rows != po->N))
    FAIL(c, "gpc_nll_hess: bad arguments (H, dnlz, alpha, diagq are required; dm with mean_N > 0; dsn2 with noise_N > 0 "
            "and dsn2_rows 1 or N)");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_nll_hess: this posterior was built from caller-provided K; a caller-provided kernel has no second "
            "derivative with respect to its hyperparameters");
  if (po->dtype != GPC_F64) FAIL(c, "gpc_nll_hess: the Hessian is fp64 only; this posterior is stored in fp32");
  if ((po->cd.kind == K_MATERN || po->cd.kind == K_MATERN_ISO) && po->cd.degree == 1)
    FAIL(c, "gpc_nll_hess: the Matern kernel of degree 1 has no second radial factor (and an infinite first one on the "
            "diagonal)");
  if (po->cd.cov_N + noise_N > NH_MAXP)
    FAIL(c, "gpc_nll_hess: " + std::to_string(po->cd.cov_N + noise_N) + " covariance and noise hyperparameters; the Gram "
            "pass takes at most " + std::to_string(NH_MAXP));
  if (!cov_is_iso(po->cd.kind) && nh_pairs(po->D) > NH_D2_MAX)
    FAIL(c, "gpc_nll_hess: D = " + std::to_string(po->D) + " has " + std::to_string(nh_pairs(po->D)) +
            " lengthscale pairs; the contraction holds at most " + std::to_string(NH_D2_MAX));
  if (int rc = require_factorized(po, "gpc_nll_hess")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return nll_hess_impl(po, dm, mean_N, dsn2, dsn2_rows, noise_N, H, dnlz, alpha, diagq);
}

int gpc_cv_grad(gpc_post* po, int loss, const double* weights, double* gsum, double* diagG, double* beta, double* alpha,
                double* q, double* cw) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if ((loss != CVG_LPD && loss != CVG_MSE) || !gsum || !diagG || !beta || !alpha || !q || !cw)
    FAIL(c, "gpc_cv_grad: bad arguments (loss 0 = lpd or 1 = mse; the six outputs are required)");
  if (weights)
    for (int i = 0; i < po->N; ++i)
      if (!(weights[i] >= 0.0) || !std::isfinite(weights[i])) FAIL(c, "gpc_cv_grad: the weights must be finite and >= 0");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_cv_grad: this posterior was built from caller-provided K; a caller-provided kernel has no derivative "
            "with respect to its hyperparameters");
  if (po->dtype != GPC_F64) FAIL(c, "gpc_cv_grad: the cross-validation gradient is fp64 only; this posterior is stored in fp32");
  if ((po->cd.kind == K_MATERN || po->cd.kind == K_MATERN_ISO) && po->cd.degree == 1)
    FAIL(c, "gpc_cv_grad: the Matern kernel of degree 1 has an infinite radial factor on the diagonal");
  if (int rc = require_factorized(po, "gpc_cv_grad")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return cv_grad_impl(po, loss, weights, gsum, diagG, beta, alpha, q, cw);
}

int gpc_predict_hyp_grad(gpc_post* po, const double* xstar, int M, int compute_var, const double* sn2, const double* dsn2,
                         int noise_rows, int noise_N, const double* dm, int mean_N, double* fmu, double* fs2, double* dfmu,
                         double* dfs2) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  const bool var = compute_var != 0;
  if (!xstar || M <= 0 || !sn2 || !fmu || !dfmu || (var && (!fs2 || !dfs2)) || noise_N < 0 || mean_N < 0 ||
      (noise_N > 0 && !dsn2) || (mean_N > 0 && !dm) || (noise_rows != 1 && noise_rows != po->N))
    FAIL(c, "gpc_predict_hyp_grad: bad arguments (xstar, sn2, fmu, dfmu are required, fs2 and dfs2 with compute_var; dsn2 "
            "with noise_N > 0; dm with mean_N > 0; noise_rows 1 or N)");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_predict_hyp_grad: this posterior was built from caller-provided K; a caller-provided kernel has no "
            "derivative with respect to its hyperparameters");
  if (po->dtype != GPC_F64)
    FAIL(c, "gpc_predict_hyp_grad: the hyperparameter gradients are fp64 only; this posterior is stored in fp32");
  if ((po->cd.kind == K_MATERN || po->cd.kind == K_MATERN_ISO) && po->cd.degree == 1)
    FAIL(c, "gpc_predict_hyp_grad: the Matern kernel of degree 1 has an infinite radial factor on the diagonal; its "
            "lengthscale planes are not formed");
  if (int rc = require_factorized(po, "gpc_predict_hyp_grad")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return hyp_grad_impl(po, xstar, M, var, sn2, dsn2, noise_rows, noise_N, dm, mean_N, fmu, fs2, dfmu, dfs2);
}

int gpc_draw(gpc_post* po, const double* xstar, int M, int R, unsigned long long seed, int s_offset,
             const double* noise_sd, double* f, double* tau) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!xstar || !f || !tau || M <= 0 || R <= 0 || s_offset < 0) FAIL(c, "gpc_draw: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0) FAIL(c, "gpc_draw: this posterior was built from caller-provided K; there is no K** to draw from");
  if (int rc = require_factorized(po, "gpc_draw")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  DrawReq req{seed, R, s_offset, noise_sd, f, tau};
  std::vector<double> fmu((size_t)M * po->S);
  // (`full` only marks the covariance build: draw_chunk consumes C_s on the device, nothing M x M is written)
  RhsRequest r;
  r.xa = xstar;
  r.M = M;
  r.lin = fmu.data();
  r.full = f;
  r.draw = &req;
  return rhs_products(po, r);
}

int gpc_debug_normals(gpc_ctx* c, unsigned long long seed, int stream, int s, int r, int j0, int count, double* out) {
  if (!c) return -2;
  if (!out || count <= 0 || s < 0 || r < 0 || j0 < 0 || (stream != 0 && stream != 1))
    FAIL(c, "gpc_debug_normals: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->dbg1.ensure((size_t)count * 8));
  hipLaunchKernelGGL(debug_normals_kernel, dim3((count + 255) / 256), dim3(256), 0, c->st, seed, stream, (long long)s, r,
                     (long long)j0, count, c->dbg1.as<double>());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, c->dbg1.p, (size_t)count * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  return 0;
}

int gpc_paths_create(gpc_post* po, int R, int F, unsigned long long seed, int s_offset, const double* ym,
                     const double* noise_sd, gpc_paths** out) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!ym || !noise_sd || !out) FAIL(c, "gpc_paths_create: null argument (ym, noise_sd and out are required)");
  if (R < 1 || F < 1) FAIL(c, "gpc_paths_create: R and F must be at least 1 (R = " + std::to_string(R) + ", F = " + std::to_string(F) + ")");
  if (R > (1 << 16) || F > (1 << 22) || s_offset < 0) FAIL(c, "gpc_paths_create: bad arguments (R <= 65536, F <= 4194304, s_offset >= 0)");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_paths_create: this posterior was built from caller-provided K; a caller-provided kernel has no "
            "spectral density to draw features from");
  if (po->cd.kind == K_RQ)
    FAIL(c, "gpc_paths_create: the rational-quadratic kernel is not supported (spectral draws exist for the "
            "squared-exponential and Matern kernels)");
  if (int rc = require_factorized(po, "gpc_paths_create")) return rc;
  if (c->N != po->N || c->D != po->D)
    FAIL(c, "gpc_paths_create: the context's data (gpc_set_data) is not the data this posterior was built on");
  HIPCHK(c, hipSetDevice(c->device));
  gpc_paths* pa = new gpc_paths;
  pa->ctx = c;
  pa->S = po->S;
  pa->N = po->N;
  pa->D = po->D;
  pa->npad = po->npad;
  pa->R = R;
  pa->F = F;
  pa->kq = ((R + BA_R - 1) / BA_R) * BA_R;
  pa->fpad = pad_tile(F);
  pa->cd = po->cd;
  const int rc = po->dtype == GPC_F64 ? paths_create_impl<double>(po, pa, seed, s_offset, ym, noise_sd)
                                      : paths_create_impl<float>(po, pa, seed, s_offset, ym, noise_sd);
  if (rc) {
    (void)hipStreamSynchronize(c->st);
    pa->release();
    delete pa;
    return rc;
  }
  *out = pa;
  return 0;
}

int gpc_paths_eval(gpc_paths* pa, const double* xstar, int M, double* f, double* df) {
  if (!pa) return -2;
  gpc_ctx* c = pa->ctx;
  if (!xstar || !f || M <= 0) FAIL(c, "gpc_paths_eval: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  return paths_eval_impl(pa, xstar, M, f, df);
}

int gpc_paths_free(gpc_paths* pa) {
  if (!pa) return 0;
  (void)hipSetDevice(pa->ctx->device);
  (void)hipStreamSynchronize(pa->ctx->st);
  pa->release();
  delete pa;
  return 0;
}

int gpc_debug_paths_fetch(gpc_paths* pa, int s, double* theta, double* b, double* wt, double* v) {
  if (!pa) return -2;
  gpc_ctx* c = pa->ctx;
  if (s < 0 || s >= pa->S) FAIL(c, "gpc_debug_paths_fetch: sample index out of range");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->st;
  const int D = pa->D, F = pa->F, R = pa->R, N = pa->N, kq = pa->kq;
  if (theta)
    HIPCHK(c, hipMemcpyAsync(theta, pa->theta.as<double>() + (size_t)s * pa->fpad * D, (size_t)F * D * 8,
                             hipMemcpyDeviceToHost, st));
  if (b) HIPCHK(c, hipMemcpyAsync(b, pa->bph.as<double>() + (size_t)s * pa->fpad, (size_t)F * 8, hipMemcpyDeviceToHost, st));
  if (wt)
    HIPCHK(c, hipMemcpy2DAsync(wt, (size_t)R * 8, pa->wt.as<double>() + (size_t)s * pa->fpad * kq, (size_t)kq * 8,
                               (size_t)R * 8, F, hipMemcpyDeviceToHost, st));
  if (v)
    HIPCHK(c, hipMemcpy2DAsync(v, (size_t)R * 8, pa->v.as<double>() + (size_t)s * pa->npad * kq, (size_t)kq * 8,
                               (size_t)R * 8, N, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return 0;
}

int gpc_predict_full(gpc_post* po, const double* xstar, int M, double* fmu, double* cov) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!xstar || !fmu || !cov || M <= 0) FAIL(c, "gpc_predict_full: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0) FAIL(c, "gpc_predict_full: this posterior was built from caller-provided K; use gpc_predict_K");
  if (int rc = require_factorized(po, "gpc_predict_full")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  RhsRequest r;
  r.xa = xstar;
  r.M = M;
  r.lin = fmu;
  r.full = cov;
  return rhs_products(po, r);
}

int gpc_predict_cov(gpc_post* po, const double* xa, int Ma, const double* xb, int Mb, const double* w, int w_per_sample,
                    double* fs2b, double* cov, double* wsq) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!xa || !xb || Ma <= 0 || Mb <= 0 || (!cov && !wsq) || (wsq && !w)) FAIL(c, "gpc_predict_cov: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_predict_cov: this posterior was built from caller-provided K; there is no k(xa, xb) to start from");
  if (int rc = require_factorized(po, "gpc_predict_cov")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? cov_products<double>(po, xa, Ma, xb, Mb, w, w_per_sample, fs2b, cov, wsq)
                              : cov_products<float>(po, xa, Ma, xb, Mb, w, w_per_sample, fs2b, cov, wsq);
}

int gpc_lookahead_batch(gpc_post* po, const double* xr, int Mr, const double* xc, int Mc, const double* w, int w_per_sample,
                        const double* noise, int q, int* idx, double* gain) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!xr || !xc || !w || !noise || !idx || !gain || Mr <= 0 || Mc <= 0 || q < 1 || q > Mc)
    FAIL(c, "gpc_lookahead_batch: bad arguments (Mr = " + std::to_string(Mr) + ", Mc = " + std::to_string(Mc) +
                ", q = " + std::to_string(q) + "; 1 <= q <= Mc, no null pointers)");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_lookahead_batch: this posterior was built from caller-provided K; there is no k(xa, xb) to start from");
  if (int rc = require_factorized(po, "gpc_lookahead_batch")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return po->dtype == GPC_F64 ? lookahead_batch_impl<double>(po, xr, Mr, xc, Mc, w, w_per_sample, noise, q, idx, gain)
                              : lookahead_batch_impl<float>(po, xr, Mr, xc, Mc, w, w_per_sample, noise, q, idx, gain);
}

namespace {
// z (K + sn2_eff I)^-1 z^T: |W z|^2 / sl (L_chol) or -(z . L z) (L = -inv)   (:1946-1962)
void quad_scale_zkz(const gpc_post* po, int M, double* zKz) {
  for (int s = 0; s < po->S; ++s) {
    const double sl = po->sp[(size_t)s * SP_STRIDE + SP_SL];
    for (int j = 0; j < M; ++j) {
      double& q = zKz[(size_t)j * po->S + s];
      q = po->lchol[s] ? q / sl : -q;
    }
  }
}
}  // namespace

int gpc_quad(gpc_post* po, const double* mu, const double* sigma, int M, int compute_var, double* zalpha,
             double* zKz) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!mu || !sigma || !zalpha || M <= 0 || (compute_var && !zKz)) FAIL(c, "gpc_quad: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (int rc = require_factorized(po, "gpc_quad")) return rc;
  if (po->cd.kind != K_SE && po->cd.kind != K_SE_ISO)
    FAIL(c, "Bayesian quadrature only supports the squared exponential kernel.");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = rhs_products(po, quad_request(mu, sigma, M, compute_var != 0, zalpha, zKz));
  if (rc || !compute_var) return rc;
  quad_scale_zkz(po, M, zKz);
  return 0;
}

int gpc_quad_grad(gpc_post* po, const double* mu, const double* sigma, int M, int compute_var, double* zalpha,
                  double* zKz, double* dza_dmu, double* dza_dsigma, double* dzkz_dmu, double* dzkz_dsigma) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!mu || !sigma || !zalpha || M <= 0 || (compute_var && !zKz) || !dza_dmu || !dza_dsigma ||
      (compute_var && (!dzkz_dmu || !dzkz_dsigma)))
    FAIL(c, "gpc_quad_grad: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind != K_SE && po->cd.kind != K_SE_ISO)
    FAIL(c, "Bayesian quadrature only supports the squared exponential kernel.");
  if (int rc = require_factorized(po, "gpc_quad_grad")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const QuadGradOut g{{dza_dmu, dza_dsigma, compute_var ? dzkz_dmu : nullptr, compute_var ? dzkz_dsigma : nullptr}};
  RhsRequest r = quad_request(mu, sigma, M, compute_var != 0, zalpha, zKz);
  r.qg = &g;
  int rc = rhs_products(po, r);
  if (rc || !compute_var) return rc;
  quad_scale_zkz(po, M, zKz);  // (the dzkz planes come back scaled on the device: qs rides in the weights)
  return 0;
}

int gpc_quad_cov(gpc_post* po, const double* mu, const double* sigma, int M, double* zalpha, double* cov) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  if (!mu || !sigma || !zalpha || !cov || M <= 0) FAIL(c, "gpc_quad_cov: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_quad_cov: this posterior was built from caller-provided K; it has no kernel to integrate");
  if (po->cd.kind != K_SE && po->cd.kind != K_SE_ISO)
    FAIL(c, "Bayesian quadrature only supports the squared exponential kernel.");
  if (int rc = require_factorized(po, "gpc_quad_cov")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  RhsRequest r = quad_request(mu, sigma, M, false, zalpha, nullptr);
  r.full = cov;
  return rhs_products(po, r);
}

int gpc_quad_mix(gpc_post* po, const double* mu, const double* sigma, const double* w, int M, int compute_var,
                 int compute_grad, double* zalpha, double* zbkzb, double* gw, double* zq, double* dza_dmu,
                 double* dza_dsigma, double* dzq_dmu, double* dzq_dsigma, double* dgw_dmu, double* dgw_dsigma) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  const bool var = compute_var != 0, grad = compute_grad != 0;
  if (!mu || !sigma || !w || !zalpha || M <= 0 || (var && (!zbkzb || !gw || !zq)) || (grad && (!dza_dmu || !dza_dsigma)) ||
      (var && grad && (!dzq_dmu || !dzq_dsigma || !dgw_dmu || !dgw_dsigma)))
    FAIL(c, "gpc_quad_mix: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (po->cd.kind < 0)
    FAIL(c, "gpc_quad_mix: this posterior was built from caller-provided K; it has no kernel to integrate");
  if (po->cd.kind != K_SE && po->cd.kind != K_SE_ISO)
    FAIL(c, "Bayesian quadrature only supports the squared exponential kernel.");
  if (int rc = require_factorized(po, "gpc_quad_mix")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const QuadMixOut o{zalpha, zbkzb, gw, zq, {dza_dmu, dza_dsigma, dzq_dmu, dzq_dsigma, dgw_dmu, dgw_dsigma}};
  const long long gemms0 = gpc::g_gemm_launches;
  const int rc = po->dtype == GPC_F64 ? quad_mix_impl<double>(po, mu, sigma, w, M, var, grad, o)
                                      : quad_mix_impl<float>(po, mu, sigma, w, M, var, grad, o);
  c->quad_mix_gemms += (unsigned long long)(gpc::g_gemm_launches - gemms0);
  return rc;
}

int gpc_cv(gpc_post* po, int F, const int* fold_ptr, const int* fold_idx, double* dmu, double* s2, double* quad,
           double* logdet, int* info) {
  if (!po) return -2;
  gpc_ctx* c = po->ctx;
  const int N = po->N, S = po->S;
  if (!dmu || !s2 || F < 0 || (F > 0 && (!fold_ptr || !fold_idx)) || (F == 0 && (fold_ptr || fold_idx)))
    FAIL(c, "gpc_cv: bad arguments");
  if (int rc = refuse_gobs(po, __func__)) return rc;
  if (N < 2) FAIL(c, "gpc_cv: cross-validation needs at least two training points");
  if (F > 65535) FAIL(c, "gpc_cv: at most 65535 folds per call, got " + std::to_string(F));
  bool singletons = true;
  if (F > 0) {
    if (fold_ptr[0] != 0) FAIL(c, "gpc_cv: fold_ptr must start at 0");
    std::vector<int> owner(N, -1);
    for (int f = 0; f < F; ++f) {
      const int lo = fold_ptr[f], k = fold_ptr[f + 1] - lo;
      const std::string name = "gpc_cv: fold " + std::to_string(f);
      if (k <= 0) FAIL(c, name + " is empty");
      if (k >= N) FAIL(c, name + " holds all " + std::to_string(N) + " points: nothing is left to predict from");
      singletons = singletons && k == 1;
      for (int j = 0; j < k; ++j) {
        const int i = fold_idx[lo + j];
        if (i < 0 || i >= N)
          FAIL(c, name + " has index " + std::to_string(i) + " out of range [0, " + std::to_string(N) + ")");
        if (j > 0 && i <= fold_idx[lo + j - 1]) FAIL(c, name + " is unsorted: its indices must ascend strictly");
        if (owner[i] >= 0)
          FAIL(c, name + " overlaps fold " + std::to_string(owner[i]) + " at index " + std::to_string(i));
        owner[i] = f;
      }
    }
  }
  if (int rc = require_factorized(po, "gpc_cv")) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const bool f64 = po->dtype == GPC_F64;
  if (F == 0) return f64 ? cv_loo_impl<double>(po, dmu, s2, quad, logdet, info) : cv_loo_impl<float>(po, dmu, s2, quad, logdet, info);
  if (!singletons)
    return f64 ? cv_fold_impl<double>(po, F, fold_ptr, fold_idx, dmu, s2, quad, logdet, info)
               : cv_fold_impl<float>(po, F, fold_ptr, fold_idx, dmu, s2, quad, logdet, info);
  // explicit singletons: the leave-one-out pass itself (the same bits), its per-point values picked per fold
  const size_t ns = (size_t)N * S;
  std::vector<double> tm_(ns), ts(ns), tq(ns), tl(ns);
  std::vector<int> ti(ns);
  if (int rc = f64 ? cv_loo_impl<double>(po, tm_.data(), ts.data(), tq.data(), tl.data(), ti.data())
                   : cv_loo_impl<float>(po, tm_.data(), ts.data(), tq.data(), tl.data(), ti.data()))
    return rc;
  std::fill(dmu, dmu + ns, std::nan(""));
  std::fill(s2, s2 + ns, std::nan(""));
  for (int f = 0; f < F; ++f) {
    const size_t i = (size_t)fold_idx[fold_ptr[f]];
    for (int s = 0; s < S; ++s) {
      dmu[i * S + s] = tm_[i * S + s];
      s2[i * S + s] = ts[i * S + s];
      if (quad) quad[(size_t)f * S + s] = tq[i * S + s];
      if (logdet) logdet[(size_t)f * S + s] = tl[i * S + s];
      if (info) info[(size_t)f * S + s] = ti[i * S + s];
    }
  }
  return 0;
}

int gpc_last_timing(gpc_ctx* c, double* ms_total, double* ms_factor) {
  if (!c) return -2;
  if (ms_total) *ms_total = c->ms_total;
  if (ms_factor) *ms_factor = c->ms_factor;
  return 0;
}

namespace {
// One row per name of gpc_set_option / gpc_get_option.  `get` reads the value (null: a test hook that is only ever
// set), `set` stores it with the option's own clamp and returns non-zero when what it triggers fails (null: a counter
// or a report, get only).
struct Option {
  const char* name;
  int (*get)(gpc_ctx*);
  int (*set)(gpc_ctx*, int);
};
#ifdef GPC_EXPERIMENTS
constexpr int IS_EXPERIMENTS_BUILD = 1;
#else
constexpr int IS_EXPERIMENTS_BUILD = 0;
#endif
int clamp_to(int lo, int hi, int v) { return std::max(lo, std::min(hi, v)); }
int tile_multiple(int v) { return std::max(TILE, (v / TILE) * TILE); }
int engine_choice(int v) { return v == 1 || v == 2 ? v : 0; }
#define GPC_GET(expr) [](gpc_ctx* c) -> int { (void)c; return (int)(expr); }
#define GPC_SET(stmt) [](gpc_ctx* c, int v) -> int { (void)c; stmt; return 0; }
#define GPC_COUNTER(field) GPC_GET(c->field & 0x7fffffff), nullptr
const Option OPTIONS[] = {
    {"groups", GPC_GET(c->groups), GPC_SET(c->groups = clamp_to(1, gpc_ctx::MAXG, v))},
    {"small_blocks", GPC_GET(gpc::g_small_launch_blocks), GPC_SET(gpc::g_small_launch_blocks = v)},
    {"dual_launch", GPC_GET(gpc::g_dual_launch ? 1 : 0), GPC_SET(gpc::g_dual_launch = v != 0)},  // syrk + inverse product of a node in one launch (default 1)
    {"leaf", GPC_GET(gpc::g_leaf_version), GPC_SET(gpc::g_leaf_version = v == 3 ? 3 : 5)},  // 5: pipelined leaf (default), 3: barrier-per-phase leaf (A/B and bit-identity tests)
    {"defer_min", GPC_GET(c->defer_min), GPC_SET(c->defer_min = v)},  // deferred inverse products: node size from which U runs on the side stream (0 off, -1 auto)
    // CUs per XCD a deferred launch stays off (2, 4, 8, 12; >= 32: all of them, a test hook): the table is rebuilt
    {"defer_reserve", GPC_GET(c->defer_reserve), [](gpc_ctx* c, int v) -> int { return c->defer_reserve = v, build_reserve_table(c); }},
    {"leaf_fault", nullptr, GPC_SET(gpc::g_leaf_fault = v != 0)},  // test hook: the pipelined leaf runs with a missing wave, its hand-offs time out
    {"nll_block", GPC_GET(c->nll_block), GPC_SET(c->nll_block = v < 0 ? -1 : (v == 0 ? 0 : tile_multiple(v)))},  // NLL-only: largest diagonal block with an inverse (multiple of 128; 0: left children inverted)
    {"solves_beside_lauum", GPC_GET(c->solves_beside_lauum), GPC_SET(c->solves_beside_lauum = v != 0)},  // 0: the triangular mat-vecs after the W^T W launch (round-2 order)
    {"tri_skip", GPC_GET(c->tri_skip), GPC_SET(c->tri_skip = v != 0)},  // 0: no GEMM launch of the evaluation pipeline skips the zero MFMAs of triangular diagonal blocks (gemm.h: GemmArgs::tri; same bits either way)
    {"stable", GPC_GET(c->stable), GPC_SET(c->stable = v != 0)},  // every factorization in stable mode (refined panel solves, plan.h), not only the jitter retries
    {"small_path", GPC_GET(c->small_path), GPC_SET(c->small_path = v != 0)},  // 0: problems of one leaf take the general pipeline too (A/B and cross-checks)
    {"check_queues", GPC_GET(c->check_queues), GPC_SET(c->check_queues = v != 0)},  // debug: verify the tile queues of persistent launches after every pipeline
    {"small_poll", GPC_GET(c->small_poll), GPC_SET(c->small_poll = v != 0)},  // 0: one-leaf evaluations wait on the stream instead of polling their landing block
    {"small_timing", GPC_GET(c->small_timing), GPC_SET(c->small_timing = v != 0)},  // 1: one-leaf evaluations record their timing events (gpc_last_timing is 0 for them otherwise)
    {"small_polled", GPC_COUNTER(small_polled)},  // one-leaf calls completed by the polled word ...
    {"small_synced", GPC_COUNTER(small_synced)},  // ... and by a stream synchronisation
    {"hess_contract_us", GPC_COUNTER(hess_contract_us)},  // device time of the contraction passes (kernel + reduction) of the last gpc_predict_hess (timed calls only)
    {"nll_hess_gram_us", GPC_COUNTER(nll_hess_gram_us)},  // device time of the Gram pass (kernel + reduction) of the last gpc_nll_hess (timed calls only)
    {"nll_hess_contract_us", GPC_COUNTER(nll_hess_contract_us)},  // ... of its second-derivative contraction (ARD families; 0 for the isotropic ones)
    {"cv_grad_trace_us", GPC_COUNTER(cv_grad_trace_us)},  // device time of the contraction pass (kernel + reduction) of the last gpc_cv_grad (timed calls only)
    {"gobs_cov_us", GPC_COUNTER(gobs_cov_us)},      // device time of the kernel of the last gpc_debug_gobs_cov
    {"gobs_trace_us", GPC_COUNTER(gobs_trace_us)},  // device time of the contraction of the last gpc_debug_gobs_trace
    {"gobs_grad_operand_us", GPC_COUNTER(gobs_grad_operand_us)},  // device time of the operand builds of the last gpc_grad_post_gobs (timed calls only) / of the last gpc_debug_gobs_grad_operand
    {"gobs_cross_us", GPC_COUNTER(gobs_cross_us)},  // device time of the build (operand + mean product) of the last gpc_debug_gobs_cross
    {"grad_post_gram_us", GPC_COUNTER(grad_post_gram_us)},  // device time of the Gram passes of the last gpc_grad_post (timed calls only)
    {"lookahead_batch_loop_us", GPC_COUNTER(lookahead_batch_loop_us)},  // device time of the step loop (all q steps, without the formation of C^0) of the last gpc_lookahead_batch
    {"cov_fused", GPC_COUNTER(cov_fused)},       // gpc_predict_cov calls reduced in the product's epilogue
    {"quad_mix_gemms", GPC_COUNTER(quad_mix_gemms)},  // MFMA GEMM launches inside gpc_quad_mix
    {"start_mult_log10", nullptr, GPC_SET(c->start_mult = std::pow(10.0, clamp_to(0, 9, v)))},  // test hook: first jitter multiplier 10^value
    {"append_fail_mask", nullptr, GPC_SET(c->append_fail_mask = (unsigned)v)},  // test hook: samples whose rank-one append is declared unstable
    // test hooks: 1 / 2 force an engine (0: the default), and what the last call ran (1 / 2; 0: none yet) --
    // gpc_post_append_block: skinny kernel / MFMA GEMM, by k
    {"block_engine", GPC_GET(c->block_engine), GPC_SET(c->block_engine = engine_choice(v))},
    {"block_engine_ran", GPC_GET(c->block_engine_ran), nullptr},
    {"paths_engine", GPC_GET(c->paths_engine), GPC_SET(c->paths_engine = engine_choice(v))},  // gpc_paths_eval: fused kernel / unfused composition
    {"paths_engine_ran", GPC_GET(c->paths_engine_ran), nullptr},
    {"paths_solve_engine", GPC_GET(c->paths_solve_engine), GPC_SET(c->paths_solve_engine = engine_choice(v))},  // the solve of gpc_paths_create: skinny kernel (0 / 1) / MFMA GEMM
    {"paths_solve_engine_ran", GPC_GET(c->paths_solve_engine_ran), nullptr},
    {"cv_engine", GPC_GET(c->cv_engine), GPC_SET(c->cv_engine = engine_choice(v))},  // gpc_cv's fold Gram: fused gather + MFMA / gathered panels + library GEMM
    {"cv_engine_ran", GPC_GET(c->cv_engine_ran), nullptr},
    {"block_appended", GPC_COUNTER(block_appended)},  // samples gpc_post_append_block appended ...
    {"block_stale", GPC_COUNTER(block_stale)},        // ... and left stale for gpc_post_recompute
    {"remove_fail_mask", nullptr, GPC_SET(c->remove_fail_mask = (unsigned)v)},  // test hook: samples gpc_post_remove leaves stale
    {"remove_force", GPC_GET(c->remove_force), GPC_SET(c->remove_force = v != 0)},  // test hook: lifts the limit below
    // the longest sweep (in panels) that GP.remove_points gives to gpc_post_remove (remove.h: RM_SWEEP_MAX_PANELS)
    {"remove_max_panels", GPC_GET(c->remove_force ? (1 << 30) : RM_SWEEP_MAX_PANELS), nullptr},
    // ... and the number of kept rows it has to exceed (remove.h: RM_MIN_KEPT_ROWS)
    {"remove_min_rows", GPC_GET(c->remove_force ? 0 : RM_MIN_KEPT_ROWS), nullptr},
    {"removed", GPC_COUNTER(points_removed)},         // samples gpc_post_remove shrank ...
    {"remove_stale", GPC_COUNTER(remove_stale)},      // ... and left stale for gpc_post_recompute[_K]
    {"last_chunk", GPC_GET(c->last_chunk), nullptr},  // samples per chunk that the last posterior consumer planned (plan_chunk; 0: it refused)
    {"experiments", GPC_GET(IS_EXPERIMENTS_BUILD), nullptr},  // 1: this library is the experiments build (tests/ and tools/ ask before they use its options)
};
#ifdef GPC_EXPERIMENTS
// options of the schedules that exist in the experiments build only (see the include of dag.h)
#define GPC_INT_OPTION(name, lvalue, clamped) {name, GPC_GET(lvalue), GPC_SET(lvalue = (clamped))}
const Option EXPERIMENT_OPTIONS[] = {
    GPC_INT_OPTION("rect_min", gpc::g_rect_min_blocks, v),  // launches of at least this many 128-tiles (x samples) below the 128-tile threshold run as 128 x 64 tiles (0: off)
    GPC_INT_OPTION("rect_mode", gpc::g_rect_mode, v != 0),  // what "rect_min" selects: 0 = 128 x 64 tiles of four waves, 1 = 128 x 128 tiles of eight waves
    GPC_INT_OPTION("indep", c->indep, v),  // independent pipelines for batches of 2 .. indep_max samples at npad >= 2048 (0: lock-step)
    GPC_INT_OPTION("indep_max", c->indep_max, clamp_to(2, gpc_ctx::MAXG, v)),
    GPC_INT_OPTION("indep_min_tiles", c->indep_min_tiles, std::max(1, v)),
    GPC_INT_OPTION("rl_ahead_max", c->rl_ahead_max, v),  // look-ahead of the right-looking plan only up to this batch work S (npad/4096)^3
    GPC_INT_OPTION("rl_panel", c->rl_panel, v <= 0 ? 0 : tile_multiple(v)),  // NLL-only: right-looking panels of this many rows with look-ahead (0: off)
    GPC_INT_OPTION("dag", c->dag, v),
    GPC_INT_OPTION("dag_small_tiles", c->dag_small_tiles, v),
    GPC_INT_OPTION("dag_lauum", c->dag_lauum, v),
    GPC_INT_OPTION("dag_leaf_blocks", c->dag_leaf_blocks, v),
    GPC_INT_OPTION("dag_aborts", c->dag_aborts, v),  // (tests: forget earlier aborts -- three of them switch the graph off for the context)
    GPC_INT_OPTION("dag_runs", c->dag_runs, v),
    GPC_INT_OPTION("dag_urgent_cus", c->dag_urgent_cus, clamp_to(0, 15, v)),
    GPC_INT_OPTION("dag_gate", c->dag_gate, v),
    GPC_INT_OPTION("dag_gate_pct", c->dag_gate_pct, clamp_to(0, 100, v)),
    GPC_INT_OPTION("dag_crit_pct", c->dag_crit_pct, clamp_to(0, 100, v)),
    GPC_INT_OPTION("dag_timeout_ms", c->dag_timeout_ms, std::max(1, v)),  // (a wait of no length would abort every graph at once: ADVICE r5)
};
#undef GPC_INT_OPTION
#endif
#undef GPC_GET
#undef GPC_SET
#undef GPC_COUNTER

const Option* find_option(const char* name) {
  for (const Option& o : OPTIONS)
    if (!strcmp(o.name, name)) return &o;
#ifdef GPC_EXPERIMENTS
  for (const Option& o : EXPERIMENT_OPTIONS)
    if (!strcmp(o.name, name)) return &o;
#endif
  return nullptr;
}
}  // namespace

int gpc_set_option(gpc_ctx* c, const char* name, int value) {
  if (!c || !name) return -2;
  const Option* o = find_option(name);
  if (!o || !o->set) FAIL(c, "gpc_set_option: unknown option");
  if (o->set(c, value)) return -1;
  ++g_alloc_epoch;  // cached launch graphs captured the old launch shapes
  return 0;
}

int gpc_get_option(gpc_ctx* c, const char* name, int* value) {
  if (!c || !name || !value) return -2;
  const Option* o = find_option(name);
  if (!o || !o->get) FAIL(c, "gpc_get_option: unknown option");
  *value = o->get(c);
  return 0;
}

int gpc_last_lauum_timing(gpc_ctx* c, double* ms, double* flops) {
  if (!c) return -2;
  if (ms) *ms = c->ms_lauum;
  if (flops) *flops = c->flops_lauum;
  return 0;
}

int gpc_mfma_peak(gpc_ctx* c, int dtype, double* tflops, double* cycles_per_mfma, double* clock_ghz) {
  if (!c || !tflops) return -2;
  HIPCHK(c, hipSetDevice(c->device));
  hipDeviceProp_t prop;
  HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
  const int iters = 2048;
  HIPCHK(c, c->dbg1.ensure((size_t)prop.multiProcessorCount * 2 * 256 * 8));
  HIPCHK(c, c->dbg2.ensure(64));
  long long* d_clk = c->dbg2.as<long long>();
  double best = 0, best_cyc = 0, best_ghz = 0;
  if (dtype >= 2) {  // 2: f64 VALU FMA, 3: f32 VALU FMA (16 independent chains, 1 or 2 waves/SIMD)
    for (int wps : {1, 2}) {
      const int blocks = prop.multiProcessorCount * wps;
      auto launch = [&]() {
        if (dtype == 2)
          hipLaunchKernelGGL((valu_peak_kernel<double>), dim3(blocks), dim3(256), 0, c->st, c->dbg1.as<double>(), iters, d_clk);
        else
          hipLaunchKernelGGL((valu_peak_kernel<float>), dim3(blocks), dim3(256), 0, c->st, c->dbg1.as<float>(), iters, d_clk);
      };
      launch();
      HIPCHK(c, hipStreamSynchronize(c->st));
      HIPCHK(c, hipEventRecord(c->ev[0], c->st));
      for (int r = 0; r < 4; ++r) launch();
      HIPCHK(c, hipEventRecord(c->ev[1], c->st));
      HIPCHK(c, hipStreamSynchronize(c->st));
      float ms = 0;
      HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
      const double tf = 4.0 * blocks * 256.0 * iters * 16 * 2.0 / (ms * 1e-3) / 1e12;
      long long hclk[2] = {0, 0};
      HIPCHK(c, hipMemcpy(hclk, d_clk, sizeof hclk, hipMemcpyDeviceToHost));
      if (tf > best) {
        best = tf;
        best_cyc = (double)hclk[0] / ((double)iters * 16) / wps;  // cycles per wave-instruction per SIMD
        best_ghz = hclk[1] > 0 ? (double)hclk[0] / ((double)hclk[1] * 10.0) : 0.0;
      }
    }
    *tflops = best;
    if (cycles_per_mfma) *cycles_per_mfma = best_cyc;
    if (clock_ghz) *clock_ghz = best_ghz;
    return 0;
  }
  // variants: accumulators per wave x waves per SIMD; the best one is the ceiling
  for (int nacc : {4, 16})
    for (int wps : {1, 2}) {
      const int blocks = prop.multiProcessorCount * wps;
      auto launch = [&]() {
        if (dtype == GPC_F64) {
          if (nacc == 4)
            hipLaunchKernelGGL((mfma_peak_kernel<double, 4>), dim3(blocks), dim3(256), 0, c->st, c->dbg1.as<double>(), iters, d_clk);
          else
            hipLaunchKernelGGL((mfma_peak_kernel<double, 16>), dim3(blocks), dim3(256), 0, c->st, c->dbg1.as<double>(), iters, d_clk);
        } else {
          if (nacc == 4)
            hipLaunchKernelGGL((mfma_peak_kernel<float, 4>), dim3(blocks), dim3(256), 0, c->st, c->dbg1.as<float>(), iters, d_clk);
          else
            hipLaunchKernelGGL((mfma_peak_kernel<float, 16>), dim3(blocks), dim3(256), 0, c->st, c->dbg1.as<float>(), iters, d_clk);
        }
      };
      launch();
      HIPCHK(c, hipStreamSynchronize(c->st));
      HIPCHK(c, hipEventRecord(c->ev[0], c->st));
      const int reps = 4;
      for (int r = 0; r < reps; ++r) launch();
      HIPCHK(c, hipEventRecord(c->ev[1], c->st));
      HIPCHK(c, hipStreamSynchronize(c->st));
      float ms = 0;
      HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
      const double flops = (double)reps * blocks * 4.0 * iters * nacc * (2.0 * 16 * 16 * 4);
      const double tf = flops / (ms * 1e-3) / 1e12;
      long long hclk[2] = {0, 0};
      HIPCHK(c, hipMemcpy(hclk, d_clk, sizeof hclk, hipMemcpyDeviceToHost));
      if (tf > best) {
        best = tf;
        best_ghz = hclk[1] > 0 ? (double)hclk[0] / ((double)hclk[1] * 10.0) : 0.0;
        // issue interval of one SIMD, from the aggregate rate and the measured shader clock
        best_cyc = best_ghz * 1e9 * (4.0 * prop.multiProcessorCount) * (2.0 * 16 * 16 * 4) / (tf * 1e12);
      }
    }
  *tflops = best;
  if (cycles_per_mfma) *cycles_per_mfma = best_cyc;
  if (clock_ghz) *clock_ghz = best_ghz;
  return 0;
}

// ------------------------------- test hooks ------------------------------------------

int gpc_debug_gemm(gpc_ctx* c, int dtype, int M, int N, int K, int a_kmajor, int b_kmajor, double alpha,
                   int beta, int klo, int khi, int lower_only, const double* A, const double* B, double* C) {
  if (!c) return -2;
  if (M % TILE || N % TILE || K % TILE || M <= 0 || N <= 0 || K <= 0) FAIL(c, "gpc_debug_gemm: sizes must be multiples of 128");
  if ((lower_only & 1) && M != N) FAIL(c, "gpc_debug_gemm: lower_only needs M == N");
#ifndef GPC_EXPERIMENTS
  if (lower_only & 0x400) FAIL(c, "gpc_debug_gemm: the rectangular tile exists in the experiments build only");
#endif
  HIPCHK(c, hipSetDevice(c->device));
  return dtype == GPC_F64
             ? debug_gemm_impl<double>(c, M, N, K, a_kmajor, b_kmajor, alpha, beta, klo, khi, lower_only, A, B, C)
             : debug_gemm_impl<float>(c, M, N, K, a_kmajor, b_kmajor, alpha, beta, klo, khi, lower_only, A, B, C);
}

int gpc_debug_gemm_queues(int ntiles, int batch, int flags, int tiles_m, int tiles_n, int klo, int khi, int lower_only,
                          int* q_total, int* q_items, int* tile_ij, int* xcd_items) {
  if (ntiles <= 0 || batch <= 0 || !q_total || (long long)ntiles * batch > (1ll << 24)) return -2;
  for (int q = 0; q < NQ; ++q) q_total[q] = 0;
  int* out = q_items;
  if (!(flags & 8)) {
    q_total[0] = ntiles * batch;
    for (int idx = 0; out && idx < q_total[0]; ++idx, out += 2) flat_queue_item(batch, idx, out[0], out[1]);
  } else {
    const int nclass = queue_nclass(batch);
    for (int q = 0; q < NQ; ++q) {
      int nsq, cls, smp;
      nsq = queue_of(batch, nclass, q, cls, smp);
      if (nsq <= 0) continue;
      q_total[q] = queue_total(ntiles, nclass, cls, nsq);
      for (int idx = 0; out && idx < q_total[q]; ++idx, out += 2) {
        // (a queue that would hand out more than the launch holds must not write past the caller's 2 ntiles batch ints)
        if (out - q_items >= 2ll * ntiles * batch) return -3;
        queue_item(q_total[q], nsq, nclass, cls, smp, idx, out[0], out[1]);
      }
    }
  }
  if (tile_ij) {
    if (tiles_m <= 0 || tiles_n <= 0 || klo < 0 || klo > 2 || khi < 0 || khi > 2) return -2;
    if (ntiles != (lower_only ? tiles_m * (tiles_m + 1) / 2 : tiles_m * tiles_n)) return -2;
    for (int bx = 0; bx < ntiles; ++bx) tile_of_bx(klo, khi, lower_only, tiles_m, tiles_n, bx, tile_ij[2 * bx], tile_ij[2 * bx + 1]);
  }
  if (xcd_items) {
    for (int by = 0; by < batch; ++by)
      for (int bx = 0; bx < ntiles; ++bx) {
        int x = bx, y = by;
        if ((flags & 16) && batch >= 8) xcd_order(ntiles, batch, x, y);
        xcd_items[2 * (by * ntiles + bx)] = x;
        xcd_items[2 * (by * ntiles + bx) + 1] = y;
      }
  }
  return 0;
}

int gpc_debug_tri_masks(int tri, int diag_tile, int slab, int* frag_rows, int* frag_cols, int* issued, int* stored) {
  const int kind = tri & TRI_KIND;
  if (tri < 0 || tri > 15 || kind > TRI_B_LAST || slab < 0 || slab > 7 || !frag_rows || !frag_cols || !issued || !stored) return -2;
  for (int w = 0; w < 4; ++w) {
    const int wr = w / 2, wc = w % 2;
    for (int i = 0; i < 4; ++i) {
      frag_rows[w * 4 + i] = tri_frag(wr, i);
      frag_cols[w * 4 + i] = tri_frag(wc, i);
      for (int j = 0; j < 4; ++j) {
        issued[(w * 4 + i) * 4 + j] = tri_issued(tri, diag_tile != 0, slab, i, j) ? 1 : 0;
        stored[(w * 4 + i) * 4 + j] = tri_stored(tri, diag_tile != 0, wr, wc, i, j) ? 1 : 0;
      }
    }
  }
  return 0;
}

int gpc_debug_tri_usable(int dtype, int tile, int a_kmajor, int b_kmajor, int klo, int khi, int lower_only, int M, int N,
                         int K, int tri) {
  if ((dtype != GPC_F64 && dtype != GPC_F32) || (tile != 64 && tile != 128) || tri < 0 || tri > 15) return -2;
  GemmArgs g;
  g.M = M, g.N = N, g.K = K;
  g.klo = klo, g.khi = khi, g.lower_only = lower_only ? 1 : 0;
  g.tri = tri;
  const bool akm = a_kmajor != 0, bkm = b_kmajor != 0;
  if (dtype == GPC_F64) return tile == 128 ? tri_usable<double, 128, 4>(g, akm, bkm) : tri_usable<double, 64, 4>(g, akm, bkm);
  return tile == 128 ? tri_usable<float, 128, 4>(g, akm, bkm) : tri_usable<float, 64, 4>(g, akm, bkm);
}

int gpc_debug_gemm_form(gpc_ctx* c, int dtype, int form, int tile, int batch, int flags, int block_slots,
                        const gpc_gemm_product* p1, const gpc_gemm_product* p2, const double* ep_w, long long ep_sw,
                        const double* ep_alpha, double* colsq, int* counters, int* available) {
  if (!c) return -2;
  if (!p1 || !counters || !available || batch <= 0 || batch > 64 || form < GPC_FORM_PLAIN || form > GPC_FORM_WSQ ||
      (tile != 64 && tile != 128) || (dtype != GPC_F64 && dtype != GPC_F32) || (flags >= 0 && ((flags & 0xff) > 31 || (flags >> 8) > 15)) ||
      block_slots > 4096)
    FAIL(c, "gpc_debug_gemm_form: bad arguments");
  const int vec = dtype == GPC_F64 ? 2 : 4;
  const gpc_gemm_product* prods[2] = {p1, p2};
  const int nprod = form == GPC_FORM_DUAL ? 2 : 1;
  if (nprod == 2 && !p2) FAIL(c, "gpc_debug_gemm_form: the dual form takes two products");
  for (int i = 0; i < nprod; ++i)
    if (const char* e = form_product_error(*prods[i], batch, vec)) {
      c->err = std::string("gpc_debug_gemm_form: ") + e;
      return -2;
    }
  if (form == GPC_FORM_DUAL && (p1->a_kmajor || p1->b_kmajor || p2->a_kmajor || !p2->b_kmajor))
    FAIL(c, "gpc_debug_gemm_form: the dual launch is m-major x m-major beside m-major x k-major");
  if (form == GPC_FORM_COLSQ && (p1->a_kmajor || !p1->b_kmajor || p1->lower_only || !colsq))
    FAIL(c, "gpc_debug_gemm_form: colsq is m-major x k-major over all tiles and needs the colsq output");
  if (form == GPC_FORM_WSQ && (!p1->a_kmajor || !p1->b_kmajor || p1->lower_only || !colsq || !ep_w || !ep_alpha ||
                               (batch > 1 && ep_sw != 0 && ep_sw < p1->M) || ep_sw < 0 || ep_sw > (1ll << 27)))
    FAIL(c, "gpc_debug_gemm_form: wsq is k-major x k-major over all tiles and needs colsq, ep_w, ep_alpha");
  HIPCHK(c, hipSetDevice(c->device));
  return dtype == GPC_F64 ? debug_gemm_form_impl<double>(c, form, tile, batch, flags, block_slots, prods, nprod, ep_w, ep_sw,
                                                         ep_alpha, colsq, counters, available)
                          : debug_gemm_form_impl<float>(c, form, tile, batch, flags, block_slots, prods, nprod, ep_w, ep_sw,
                                                        ep_alpha, colsq, counters, available);
}

int gpc_debug_leaf(gpc_ctx* c, int dtype, const double* A, double* L, double* W, double* logdet, int* info) {
  return gpc_debug_factor(c, dtype, TILE, A, L, W, nullptr, logdet, info);
}

int gpc_debug_factor(gpc_ctx* c, int dtype, int n, const double* A, double* L, double* W, double* Ainv,
                     double* logdet, int* info) {
  if (!c) return -2;
  if (!A || n <= 0) FAIL(c, "gpc_debug_factor: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  return dtype == GPC_F64 ? debug_factor_impl<double>(c, n, A, L, W, Ainv, logdet, info)
                          : debug_factor_impl<float>(c, n, A, L, W, Ainv, logdet, info);
}

int gpc_debug_factor_plan(gpc_ctx* c, int dtype, int npad, int nvalid, int batch, int plan, int nll_block, int flags,
                          double* A, double* W, double* T, const double* r, double* z, double* Ainv, double* logdet,
                          int* info) {
  if (!c) return -2;
  if (dtype != GPC_F64 && dtype != GPC_F32) FAIL(c, "gpc_debug_factor_plan: dtype must be GPC_F64 or GPC_F32");
  // (2304 as well: the 18-tile root, odd halves of 9 tiles below it -- tests/test_gpu_tri_skip.py)
  if (npad < TILE || npad % TILE != 0 || (npad > 2048 && npad != 2304))
    FAIL(c, "gpc_debug_factor_plan: npad must be a multiple of 128 in 128 .. 2048, or 2304");
  if (batch < 1 || batch > 16) FAIL(c, "gpc_debug_factor_plan: batch must be 1 .. 16");
  if (plan < 0 || plan > 2) FAIL(c, "gpc_debug_factor_plan: plan must be 0, 1 or 2");
  if (plan == 2 && (nll_block < TILE || nll_block % TILE != 0 || nll_block > npad))
    FAIL(c, "gpc_debug_factor_plan: nll_block must be a multiple of 128 in 128 .. npad");
  if (flags < 0 || flags > 7) FAIL(c, "gpc_debug_factor_plan: flags has bits 0 .. 2");
  if ((flags & 4) && plan != 0) FAIL(c, "gpc_debug_factor_plan: the inverse (bit 2) belongs to plan 0");
  if (nvalid < 0 || !A || !W || !T || !logdet || !info || (r && !z) || ((flags & 4) && !Ainv))
    FAIL(c, "gpc_debug_factor_plan: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  return dtype == GPC_F64 ? debug_factor_plan_impl<double>(c, npad, nvalid, batch, plan, nll_block, flags, A, W, T, r, z,
                                                           Ainv, logdet, info)
                          : debug_factor_plan_impl<float>(c, npad, nvalid, batch, plan, nll_block, flags, A, W, T, r, z,
                                                          Ainv, logdet, info);
}

int gpc_debug_cov(gpc_ctx* c, int which, int kernel_id, int degree, int dtype, const double* hyp_cov, double kscale,
                  double sl, const double* dvec, const double* X, int N, int D, const double* Xstar, int M,
                  const double* mat, const double* vec, double* out0, double* out1, double* xs_out) {
  if (!c) return -2;
  if (!valid_kernel(kernel_id, degree) || !hyp_cov || !X || N <= 0 || D <= 0 || !out0 || which < 0 || which > 4)
    FAIL(c, "gpc_debug_cov: bad arguments");
  if (which == 1 && N > TILE) FAIL(c, "gpc_debug_cov: the small front builds one 128 x 128 leaf (N <= 128)");
  if ((which == 2 || which == 4) && (!Xstar || M <= 0 || !vec || !out1))
    FAIL(c, "gpc_debug_cov: cross needs X*, alpha and both outputs");
  if (which == 3 && (!mat || !vec || !out1)) FAIL(c, "gpc_debug_cov: trace needs T, a and both outputs");
  HIPCHK(c, hipSetDevice(c->device));
  CovDesc cd;
  cd.kind = kernel_id;
  cd.degree = degree;
  cd.D = D;
  cd.cov_N = cov_count_of(kernel_id, D);
  return dtype == GPC_F64
             ? debug_cov_impl<double>(c, which, cd, hyp_cov, kscale, sl, dvec, X, N, Xstar, M, mat, vec, out0, out1, xs_out)
             : debug_cov_impl<float>(c, which, cd, hyp_cov, kscale, sl, dvec, X, N, Xstar, M, mat, vec, out0, out1, xs_out);
}

int gpc_debug_block_gram(gpc_ctx* c, int dtype, int n, int M, int Dp, const double* Y, const double* Z, int diag_only,
                         double* out) {
  if (!c) return -2;
  if (!Y || !out || n <= 0 || M <= 0 || Dp <= 0 || (dtype != GPC_F64 && dtype != GPC_F32))
    FAIL(c, "gpc_debug_block_gram: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  return dtype == GPC_F64 ? debug_block_gram_impl<double>(c, n, M, Dp, Y, Z, diag_only != 0, out)
                          : debug_block_gram_impl<float>(c, n, M, Dp, Y, Z, diag_only != 0, out);
}

int gpc_debug_blas1(gpc_ctx* c, int which, int dtype, const int* ip, const double* const* in, const long long* in_n,
                    double* const* out, const long long* out_n) {
  if (!c) return -2;
  if (!ip || !in || !in_n || !out || !out_n || (dtype != GPC_F64 && dtype != GPC_F32))
    FAIL(c, "gpc_debug_blas1: bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  return dtype == GPC_F64 ? debug_blas1_impl<double>(c, which, ip, in, in_n, out, out_n)
                          : debug_blas1_impl<float>(c, which, ip, in, in_n, out, out_n);
}

int gpc_debug_hess_contract(gpc_ctx* c, int kernel_id, int degree, int dtype, const double* hyp_cov, const double* X, int N,
                            int D, const double* xstar, int M, const double* alpha, const double* Q, double* out_alpha,
                            double* out_q) {
  if (!c) return -2;
  if (!valid_kernel(kernel_id, degree) || !hyp_cov || !X || N <= 0 || D <= 0 || !xstar || M <= 0 || !alpha || !out_alpha ||
      (Q && !out_q) || (dtype != GPC_F64 && dtype != GPC_F32))
    FAIL(c, "gpc_debug_hess_contract: bad arguments");
  if ((kernel_id == K_MATERN || kernel_id == K_MATERN_ISO) && degree == 1)
    FAIL(c, "gpc_debug_hess_contract: the Matern kernel of degree 1 has no second derivative with respect to x*");
  HIPCHK(c, hipSetDevice(c->device));
  CovDesc cd;
  cd.kind = kernel_id;
  cd.degree = degree;
  cd.D = D;
  cd.cov_N = cov_count_of(kernel_id, D);
  return dtype == GPC_F64 ? debug_hess_impl<double>(c, cd, hyp_cov, X, N, xstar, M, alpha, Q, out_alpha, out_q)
                          : debug_hess_impl<float>(c, cd, hyp_cov, X, N, xstar, M, alpha, Q, out_alpha, out_q);
}

int gpc_debug_hyp_cross(gpc_ctx* c, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                        const double* xstar, int M, const double* alpha, const double* W, int P, const double* Q,
                        double* out) {
  if (!c) return -2;
  if (!valid_kernel(kernel_id, degree) || !hyp_cov || !X || N <= 0 || D <= 0 || !xstar || M <= 0 || !alpha || !W || P <= 0 ||
      !out)
    FAIL(c, "gpc_debug_hyp_cross: bad arguments");
  if ((kernel_id == K_MATERN || kernel_id == K_MATERN_ISO) && degree == 1)
    FAIL(c, "gpc_debug_hyp_cross: the Matern kernel of degree 1 has an infinite radial factor on the diagonal");
  HIPCHK(c, hipSetDevice(c->device));
  CovDesc cd;
  cd.kind = kernel_id;
  cd.degree = degree;
  cd.D = D;
  cd.cov_N = cov_count_of(kernel_id, D);
  if (P < cd.cov_N) FAIL(c, "gpc_debug_hyp_cross: P must cover the covariance hyperparameters");
  return debug_hyp_cross_impl(c, cd, hyp_cov, X, N, xstar, M, alpha, W, P, Q, out);
}

// gpc_debug_nll_plane / gpc_debug_nll_d2: the plane kernel and the second-derivative contraction of gpc_nll_hess
// (nll_hess.h) on one sample with caller-given alpha and dense symmetric Q (null: zeros), launched as the call launches
// them; gpc_debug_nll_gram: its Gram pass on caller-given planes.
namespace {
struct NhHookSample {
  ScratchDev sd;
  NhScratch z;
  CovDesc cd;
  int N = 0, npad = 0;
  double *xs = nullptr, *sp = nullptr, *al = nullptr;
  int init(gpc_ctx* c, const char* fn, int kernel_id, int degree, const double* hyp, const double* X, int N_, int D,
           const double* alpha, const double* Qd) {
    cd.kind = kernel_id, cd.degree = degree, cd.D = D, cd.cov_N = cov_count_of(kernel_id, D);
    N = N_, npad = pad_tile(N);
    const int nd2 = cov_is_iso(kernel_id) ? 0 : nh_pairs(D);
    std::vector<double> mul(D), dv(D), hsp(SP_STRIDE, 0.0), hal(npad, 0.0), hq((size_t)npad * npad, 0.0);
    double sf2 = 0.0, rqa = 1.0;
    scaling_of(kernel_id, degree, D, hyp, mul.data(), dv.data(), &sf2, &rqa);
    hsp[SP_SF2] = sf2, hsp[SP_RQA] = rqa, hsp[SP_KSCALE] = 1.0, hsp[SP_SL] = 1.0;
    std::copy(alpha, alpha + N, hal.begin());
    if (Qd)
      for (int i = 0; i < N; ++i) std::copy(Qd + (size_t)i * N, Qd + (size_t)(i + 1) * N, hq.begin() + (size_t)i * npad);
    double* dX = sd.get<double>((size_t)N * D);
    double* dmul = sd.get<double>(D);
    double* ddv = sd.get<double>(D);
    sp = sd.get<double>(SP_STRIDE);
    al = sd.get<double>(npad);
    xs = sd.get<double>((size_t)npad * D);
    char* blk = sd.get<char>(ScratchCarver::count<NhScratch>(1, npad, cd.cov_N, 0, 0, nd2));
    if (!dX || !dmul || !ddv || !sp || !al || !xs || !blk) FAIL(c, std::string(fn) + ": out of device memory");
    ScratchCarver::carve(z, blk, 1, npad, cd.cov_N, 0, 0, nd2);
    HIPCHK(c, hipMemcpy(dX, X, (size_t)N * D * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dmul, mul.data(), (size_t)D * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(ddv, dv.data(), (size_t)D * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(sp, hsp.data(), SP_STRIDE * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(al, hal.data(), (size_t)npad * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(z.Q, hq.data(), hq.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(scale_x_kernel, dim3((unsigned)(((long long)npad * D + 255) / 256), 1), dim3(256), 0, c->st,
                       (const double*)dX, N, npad, D, (const double*)dmul, (const double*)ddv, xs);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
};
bool nh_hook_kernel_ok(int kernel_id, int degree) {
  return valid_kernel(kernel_id, degree) && !((kernel_id == K_MATERN || kernel_id == K_MATERN_ISO) && degree == 1);
}
}  // namespace

int gpc_debug_nll_plane(gpc_ctx* c, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D, int p,
                        const double* alpha, const double* Q, double* plane, double* u, double* g) {
  if (!c) return -2;
  if (!nh_hook_kernel_ok(kernel_id, degree) || !hyp_cov || !X || N <= 0 || D <= 0 || !alpha || !plane || !u || !g || p < 0 ||
      p >= cov_count_of(kernel_id, D))
    FAIL(c, "gpc_debug_nll_plane: bad arguments (Matern 1 has no Hessian; p < cov_N)");
  HIPCHK(c, hipSetDevice(c->device));
  NhHookSample h;
  if (int rc = h.init(c, "gpc_debug_nll_plane", kernel_id, degree, hyp_cov, X, N, D, alpha, Q)) return rc;
  if (int rc = nh_launch_plane(c, h.cd, h.z, 1, p, h.xs, h.sp, h.al, N)) return rc;
  const int npad = h.npad;
  std::vector<double> hp((size_t)npad * npad), hu(npad);
  HIPCHK(c, hipMemcpyAsync(hp.data(), h.z.Op, hp.size() * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipMemcpyAsync(hu.data(), h.z.X + (size_t)p * npad, (size_t)npad * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipMemcpyAsync(g, h.z.gsum + (size_t)p * 2, 16, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  for (int i = 0; i < N; ++i) std::copy(hp.begin() + (size_t)i * npad, hp.begin() + (size_t)i * npad + N, plane + (size_t)i * N);
  std::copy(hu.begin(), hu.begin() + N, u);
  return 0;
}

int gpc_debug_nll_d2(gpc_ctx* c, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                     const double* alpha, const double* Q, double* out) {
  if (!c) return -2;
  if (!nh_hook_kernel_ok(kernel_id, degree) || cov_is_iso(kernel_id) || !hyp_cov || !X || N <= 0 || D <= 0 ||
      nh_pairs(D) > NH_D2_MAX || !alpha || !Q || !out)
    FAIL(c, "gpc_debug_nll_d2: bad arguments (ARD families only; Matern 1 has no Hessian)");
  HIPCHK(c, hipSetDevice(c->device));
  NhHookSample h;
  if (int rc = h.init(c, "gpc_debug_nll_d2", kernel_id, degree, hyp_cov, X, N, D, alpha, Q)) return rc;
  if (int rc = nh_launch_d2(c, h.cd, h.z, 1, h.xs, h.sp, h.al, N)) return rc;
  HIPCHK(c, hipMemcpyAsync(out, h.z.d2sum, (size_t)nh_pairs(D) * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  return 0;
}

int gpc_debug_nll_gram(gpc_ctx* c, int npad, int P, const double* planes, double* out) {
  if (!c) return -2;
  if (npad <= 0 || npad % CT || npad > 4096 || P <= 0 || P > NH_MAXP || !planes || !out)
    FAIL(c, "gpc_debug_nll_gram: bad arguments (npad a multiple of 64 up to 4096, 1 <= P <= 128)");
  HIPCHK(c, hipSetDevice(c->device));
  ScratchDev sd;
  NhScratch z;
  char* blk = sd.get<char>(ScratchCarver::count<NhScratch>(1, npad, P, 0, 0, 0));
  if (!blk) FAIL(c, "gpc_debug_nll_gram: out of device memory");
  ScratchCarver::carve(z, blk, 1, npad, P, 0, 0, 0);
  HIPCHK(c, hipMemcpy(z.B, planes, (size_t)P * npad * npad * 8, hipMemcpyHostToDevice));
  if (int rc = nh_launch_gram(c, z, 1)) return rc;
  HIPCHK(c, hipMemcpyAsync(out, z.grsum, (size_t)z.npairs * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  return 0;
}

// gpc_debug_cv_trace: the contraction of gpc_cv_grad (cvgrad.h) alone on one sample with caller-given lower-triangular M
// and the vectors alpha, beta, launched as the call launches it; gpc_debug_cv_weights: its per-point kernel.
int gpc_debug_cv_trace(gpc_ctx* c, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                       const double* M, const double* alpha, const double* beta, double* gsum, double* diagG) {
  if (!c) return -2;
  if (!nh_hook_kernel_ok(kernel_id, degree) || !hyp_cov || !X || N <= 0 || D <= 0 || !M || !alpha || !beta || !gsum || !diagG)
    FAIL(c, "gpc_debug_cv_trace: bad arguments (the Matern kernel of degree 1 is not served)");
  HIPCHK(c, hipSetDevice(c->device));
  NhHookSample h;
  if (int rc = h.init(c, "gpc_debug_cv_trace", kernel_id, degree, hyp_cov, X, N, D, alpha, M)) return rc;  // (M in Q's place)
  const int npad = h.npad, nt = npad / CT, ntl = nt * (nt + 1) / 2, P = h.cd.cov_N;
  std::vector<double> hb(npad, 0.0), hd(npad);
  std::copy(beta, beta + N, hb.begin());
  double* be = h.sd.get<double>(npad);
  double* part = h.sd.get<double>((size_t)ntl * P);
  double* sum = h.sd.get<double>(P);
  double* dg = h.sd.get<double>(npad);
  if (!be || !part || !sum || !dg) FAIL(c, "gpc_debug_cv_trace: out of device memory");
  HIPCHK(c, hipMemcpy(be, hb.data(), (size_t)npad * 8, hipMemcpyHostToDevice));
  if (int rc = cvg_launch_trace(c, h.cd, 1, N, npad, h.xs, h.sp, h.al, be, h.z.Q, part, sum, dg)) return rc;
  HIPCHK(c, hipMemcpyAsync(gsum, sum, (size_t)P * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipMemcpyAsync(hd.data(), dg, (size_t)npad * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  std::copy(hd.begin(), hd.begin() + N, diagG);
  return 0;
}

int gpc_debug_cv_weights(gpc_ctx* c, int N, int loss, const double* alpha, const double* q, const double* weights,
                         double* cw, double* b) {
  if (!c) return -2;
  if (N <= 0 || (loss != CVG_LPD && loss != CVG_MSE) || !alpha || !q || !cw || !b)
    FAIL(c, "gpc_debug_cv_weights: bad arguments (loss 0 = lpd or 1 = mse)");
  HIPCHK(c, hipSetDevice(c->device));
  const int npad = pad_tile(N);
  std::vector<double> hin(3 * (size_t)npad, 0.0), hout(3 * (size_t)npad);
  std::copy(alpha, alpha + N, hin.begin());
  std::copy(q, q + N, hin.begin() + npad);
  for (int i = 0; i < N; ++i) hin[2 * (size_t)npad + i] = weights ? weights[i] : 1.0;
  ScratchDev sd;
  double* din = sd.get<double>(3 * (size_t)npad);
  double* dout = sd.get<double>(3 * (size_t)npad);
  if (!din || !dout) FAIL(c, "gpc_debug_cv_weights: out of device memory");
  HIPCHK(c, hipMemcpy(din, hin.data(), hin.size() * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(cvg_weights_kernel, dim3((npad + 255) / 256, 1), dim3(256), 0, c->st, (const double*)din,
                     (const double*)(din + npad), 0ll, 1, (const double*)(din + 2 * (size_t)npad), N, npad, loss, dout,
                     dout + npad, dout + 2 * (size_t)npad);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(hout.data(), dout, hout.size() * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  std::copy(hout.begin() + npad, hout.begin() + npad + N, cw);
  std::copy(hout.begin() + 2 * (size_t)npad, hout.begin() + 2 * (size_t)npad + N, b);
  return 0;
}

// Debug: a 64-bit hash (sum of the bit patterns, wrapping) of every 128 x 128 tile of one workspace matrix of the LAST call
// (which: 0 = A, 1 = W, 2 = T; `sample` = position in the last chunk) -- to find the tile where two schedules differ.
int gpc_debug_workspace_hash(gpc_ctx* c, int dtype, int which, int sample, unsigned long long* out) {
  if (!c || !out || which < 0 || which > 2) return -2;
  HIPCHK(c, hipSetDevice(c->device));
  const int npad = c->npad, nt = npad / TILE;
  DevBuf& m = which == 0 ? c->mA : (which == 1 ? c->mW : c->mT);
  const size_t esz = dtype == GPC_F64 ? 8 : 4;
  if (m.bytes < (size_t)(sample + 1) * npad * npad * esz) FAIL(c, "gpc_debug_workspace_hash: no such sample in the workspace");
  HIPCHK(c, c->dbg3.ensure((size_t)nt * nt * 8));
  if (dtype == GPC_F64)
    hipLaunchKernelGGL((tile_hash_kernel<double>), dim3(nt, nt), dim3(256), 0, c->st, m.as<double>() + (size_t)sample * npad * npad, npad,
                       c->dbg3.as<unsigned long long>());
  else
    hipLaunchKernelGGL((tile_hash_kernel<float>), dim3(nt, nt), dim3(256), 0, c->st, m.as<float>() + (size_t)sample * npad * npad, npad,
                       c->dbg3.as<unsigned long long>());
  HIPCHK(c, hipMemcpyAsync(out, c->dbg3.p, (size_t)nt * nt * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  return 0;
}

#ifdef GPC_EXPERIMENTS
// Host-only (no device call): the tile-task graph dag.h derives for a factorization of an npad x npad matrix.
int gpc_debug_dag(int npad, int plan, int nll_blk, int small_tiles, int* counts, int* tasks_out, double* alpha_out,
                  int* succ_out, int cap_tasks, int cap_edges) {
  if (npad <= 0 || npad % TILE || !counts) return -2;
  PlanRecorder rec;
  Factor<double> F;
  F.rec = &rec;
  F.st = nullptr;
  F.batch = 1;
  F.npad = npad;
  F.A = static_cast<double*>(const_cast<void*>(dag_fake_base(0)));
  F.W = static_cast<double*>(const_cast<void*>(dag_fake_base(1)));
  F.Tm = static_cast<double*>(const_cast<void*>(dag_fake_base(2)));
  F.sA = F.sW = F.sT = (long long)npad * npad;
  F.dual_launch = false;
  if (plan == 0) {  // NLL only
    if (nll_blk > 0) {
      F.nll_block = nll_blk;
      F.potrf_nll(0, npad);
    } else {
      F.potrf_inv(0, npad, false, false);
    }
  } else {
    F.potrf_inv(0, npad, true, false);
    if (plan == 1) F.lauum(F.Tm, F.sT);
  }
  const void* bases[3] = {dag_fake_base(0), dag_fake_base(1), dag_fake_base(2)};
  DagPlan P;
  if (!build_dag(rec, bases, npad, sizeof(double), small_tiles, P, true)) return -1;
  counts[0] = P.ntasks;
  counts[1] = (int)P.nedges;
  counts[2] = (int)P.launches.size();
  counts[3] = P.nleaf;
  if (!tasks_out) return 0;
  if (cap_tasks < P.ntasks || cap_edges < (int)P.nedges) return -3;
  for (int t = 0; t < P.ntasks; ++t) {
    const DagTask& d = P.tasks[t];
    const DagPlan::Info& in = P.info[t];
    int* o = tasks_out + (size_t)t * 24;
    o[0] = d.kind == DAG_KIND_LEAF ? 1 : 0;
    o[1] = in.bt;
    o[2] = (d.kind >> 2) & 1;
    o[3] = (d.kind >> 1) & 1;
    o[4] = in.beta;
    const DagPlan::Region* rg[3] = {&in.c, &in.a, &in.b};
    for (int q = 0; q < 3; ++q) {
      o[5 + 5 * q] = rg[q]->buf;
      o[6 + 5 * q] = rg[q]->r0;
      o[7 + 5 * q] = rg[q]->r1;
      o[8 + 5 * q] = rg[q]->c0;
      o[9 + 5 * q] = rg[q]->c1;
    }
    o[20] = d.npred;
    o[21] = d.succ_begin;
    o[22] = d.succ_count;
    o[23] = d.ring;
    alpha_out[t] = in.alpha;
  }
  memcpy(succ_out, P.succ.data(), P.succ.size() * sizeof(int));
  return 0;
}

#endif  // GPC_EXPERIMENTS

}  // extern "C"
