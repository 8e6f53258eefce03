// scratch.h -- the device scratch of every posterior consumer, declared once.  Host only, no HIP call.
//
// A consumer's struct lists the arrays of `cnt` samples once, through ScratchCarver::take (common.h), in its
// layout(sc, cnt, dims...): the same list counts the bytes per sample that gpcore.hip's plan_chunk divides the budget by
// and hands out the pointers, so the two cannot disagree.  What a call needs once (raw uploads, staging, results in the
// caller's layout) is a second struct, *Shared, carved behind the samples' arrays in the same block.
//
// Alignment: the separate allocations these layouts replace were 256-byte aligned; a carved array is only as aligned as
// what precedes it.  The MFMA GEMM operands and the panels read through MM<T>::vec_t need 16 bytes, so a layout puts the
// storage-type matrices first (all multiples of 128^2 elements), then the double arrays of even length, and odd-length
// vectors and scalars last; sizes are never rounded.  take(n, 16) checks and counts a miss, and the call fails before
// it launches anything (gpcore.hip: CARVECHK).  scratch_bytes_of, at the end, counts any layout by name without a
// device (gpc_debug_scratch_bytes; tests/test_scratch_layout_cpu.py holds it against closed forms).
#pragma once
#include <algorithm>
#include <string>

#include "blas1.h"
#include "block_append.h"
#include "common.h"
#include "covfun.h"
#include "cv.h"
#include "gradobs.h"
#include "gradpost.h"
#include "hess.h"
#include "lookahead_batch.h"
#include "remove.h"

namespace gpc {

// ---- rhs_products: predict, predict_full, quad, quad_grad, predict_K, predict_gobs, draw --------------------------------
// The device scratch of one rhs_products call, declared once (ScratchCarver): RhsScratch lists the arrays of `cnt`
// samples -- carved once per call for the planned chunk, whose size is the stride of [mu | v] and of the gradient
// planes -- and RhsShared what exists once per call, behind them in the same block.  The storage-type matrices come
// first, then the double arrays of even length (16-byte aligned, as the separate allocations they replace were), the
// odd-length ones last.  The three slabs a draw factors in (mA mW mT) are the factorization's workspace, not listed.
struct RhsDims {
  int N, npad, M, mpad, D, S;
  bool full, gq, qg, given;
  int gpl;   // gradient planes (0: no gradient pass)
  int prow;  // tile rows of the builder's fused mean product (CROSS: npad / 64, GOBS: its points / 64, else 0)
  int crow;  // tile rows of the products' column sums of squares (gemm.h: EPI = 1; 0: V is written instead)
  int R;     // draws per sample (0: not a draw)
  // kind: RhsRequest::Rhs; grad: a gradient pass (dlin or qg); gobs_pts: the points of a gradient-observation posterior
  static RhsDims of(int N, int M, int D, int S, int kind, bool want_quad, bool full, bool grad, bool qg, int R, int gobs_pts) {
    RhsDims d;
    d.N = N, d.npad = pad_tile(N), d.M = M, d.mpad = pad_tile(M), d.D = D, d.S = S;
    d.full = full, d.qg = qg, d.given = kind == 2;
    d.gq = grad && (!qg || want_quad);  // the gradient pass reads Q (not without a product)
    d.gpl = !grad ? 0 : qg && want_quad ? 4 : 2;
    d.prow = kind == 0 ? d.npad / CT : kind == 3 ? gobs_pts / CT : 0;
    d.crow = want_quad && colsq_form(d.npad, d.mpad, full, grad) ? d.npad / TILE : 0;
    d.R = R;
    return d;
  }
  // (problems whose product is a handful of 128-tiles keep the 64-tile product + column-sum pass: latency regime.
  // Decided by the problem size only, never by the number of samples: the two forms add in different orders, and a
  // sample of a batch must carry the bits of its single evaluation)
  static bool colsq_form(int npad, int mpad, bool full, bool grad) {
    return !full && !grad && (long long)(npad / TILE) * (mpad / TILE) >= 64;
  }
  template <typename T>
  size_t slab_bytes() const { return R ? (size_t)mpad * mpad * sizeof(T) : 0; }  // each of mA mW mT, per sample
};

template <typename T>
struct RhsScratch {
  T *Ks, *V, *Q, *Kss, *Z, *F;
  double *gpart, *gres, *qcon, *xss, *mu, *part, *colsq, *dout, *logdet;
  int* info;
  void layout(ScratchCarver& sc, int cnt, const RhsDims& d) {
    const size_t c = cnt, mp = d.mpad, sKs = (size_t)d.npad * mp, sZ = d.R ? mp * pad_tile(d.R) : 0;
    Ks = sc.take<T>(c * sKs, 16);                      // the right-hand sides R_s
    V = sc.take<T>(c * sKs, 16);                       // V = W R | G = L R
    Q = sc.take<T>(d.gq ? c * sKs : 0, 16);            // Q = W^T V
    Kss = sc.take<T>(d.full ? c * mp * mp : 0, 16);    // K** and then the full covariance C_s
    Z = sc.take<T>(c * sZ, 16);                        // draw: the normals and F = L Z
    F = sc.take<T>(c * sZ, 16);
    gpart = sc.take(c * (d.npad / CT) * d.gpl * d.D * mp, 16);  // the gradient pass's per-tile partials
    gres = sc.take(c * d.gpl * mp * d.D, 16);                   // ... and its planes, [plane][sample][mpad x D]
    qcon = sc.take(d.qg ? c * (d.D + 1) * mp : 0, 16);          // quad_grad: 1/tau_jl (D x mpad) and ln nf_j (mpad)
    xss = sc.take(d.given ? 0 : c * mp * d.D, 16);              // the scaled queries
    mu = sc.take(2 * c * mp, 16);                               // [mu | v]: one download
    part = sc.take(c * d.prow * mp, 16);
    colsq = sc.take(c * d.crow * mp, 16);
    dout = sc.take(c * d.M * d.R);                              // the draws, M x R
    logdet = sc.take(d.R ? c : 0);
    info = sc.take<int>(d.R ? 2 * c : 0);  // (8 bytes per sample: what follows the chunk's arrays stays 8-byte aligned)
  }
};

struct RhsShared {
  double *mut, *given, *fullout, *xa, *xb, *nsd;
  void layout(ScratchCarver& sc, const RhsDims& d) {
    const size_t M = d.M;
    mut = sc.take(d.qg ? (size_t)d.D * d.mpad : 0);                 // quad_grad: mu_jl transposed
    given = sc.take(d.given ? (size_t)std::max(d.N, d.M) * M : 0);  // GIVEN_KS: one sample's Ks or K** on its way in
    fullout = sc.take(d.full && !d.R ? M * M : 0);                  // one sample's full covariance on its way out
    xa = sc.take(d.given ? 0 : M * d.D);                            // the raw uploads
    xb = sc.take(d.given ? 0 : M * d.D);
    nsd = sc.take(d.R ? M * d.S : 0);                               // draw: the noise standard deviations
  }
};

// ---- gpc_predict_cov and the look-ahead's C^0 (cov_products) -----------------------------------------------------------
inline bool cov_fused_form(int mapad, int mbpad, bool want_wsq, bool want_cov) {
  return want_wsq && !want_cov && (long long)(mapad / TILE) * (mbpad / TILE) >= 64;
}
template <typename T>
struct CovScratch {
  T *Ksa, *Ksb, *Va, *Vb, *Kab;
  double *part, *wpart, *xsa, *xsbq, *vq, *w;
  void layout(ScratchCarver& sc, int cnt, int npad, int mapad, int mbpad, int D, bool fused) {
    const size_t c = cnt, sKa = (size_t)npad * mapad, sKb = (size_t)npad * mbpad;
    Ksa = sc.take<T>(c * sKa, 16);
    Ksb = sc.take<T>(c * sKb, 16);
    Va = sc.take<T>(c * sKa, 16);
    Vb = sc.take<T>(c * sKb, 16);
    Kab = sc.take<T>(c * mapad * mbpad, 16);
    part = sc.take(c * (npad / CT) * std::max(mapad, mbpad), 16);          // the builder's fused mean product (unused)
    wpart = sc.take(fused ? c * (mapad / TILE) * mbpad : 0, 16);           // fused form: the tile rows' weighted sums
    xsa = sc.take(c * mapad * D, 16);                                      // the scaled queries
    xsbq = sc.take(c * mbpad * D, 16);
    vq = sc.take(2 * c * mbpad, 16);                                       // [v | q]: one download
    w = sc.take(c * (mapad + 1));  // [weights: cnt x mapad | the products' factors: cnt]: one upload
  }
};

struct CovShared {
  double *cov, *xa, *xb;
  void layout(ScratchCarver& sc, int Ma, int Mb, int D, bool want_cov) {
    cov = sc.take(want_cov ? (size_t)Ma * Mb : 0);  // one sample's covariance on its way out
    xa = sc.take((size_t)Ma * D);                   // the raw uploads
    xb = sc.take((size_t)Mb * D);
  }
};

// ---- gpc_lookahead_batch ------------------------------------------------------------------------------------------------
// The resident state of ALL samples, carved from one allocation (c->lab): the score of a step needs every sample, so the
// step loop cannot be chunked over them.  C comes first (its rows are read 16 bytes at a time); every double block has
// an even length; the block that is downloaded (the gains, then the indices) is contiguous.
struct LabScratch {
  double *C, *lpan, *part, *gains, *score, *v, *noise, *w, *sd, *gain_out;
  int *idx, *cur, *chosen;
  size_t out_bytes = 0;
  static size_t even(size_t n) { return (n + 1) & ~(size_t)1; }
  void layout(ScratchCarver& sc, int S, int Mr, int Mc, int ld, int q) {
    const size_t s = S, nslab = (Mr + LB_T - 1) / LB_T;
    C = sc.take(s * (Mr + Mc) * ld);
    lpan = sc.take(even(s * q * (Mr + ld)));
    part = sc.take(s * nslab * ld);
    gains = sc.take(s * ld);
    score = sc.take(ld);
    v = sc.take(s * ld);
    noise = sc.take(s * ld);
    w = sc.take(even(s * Mr));
    sd = sc.take(even(s));
    const size_t before_out = sc.bytes;
    gain_out = sc.take(even(s * q));
    idx = sc.take<int>(even(q));
    out_bytes = sc.bytes - before_out;
    cur = sc.take<int>(2);
    chosen = sc.take<int>(ld);
  }
};

// ---- gpc_grad_post, gpc_predict_hess ----------------------------------------------------------------------------------
// The arrays of `cnt` samples with one block of GQB queries, for gpc_grad_post and gpc_predict_hess alike (the raw
// queries, M x D doubles once per call, follow them in the block)
template <typename T>
struct BlockScratch {
  T *P, *V, *Q;
  double *part, *colsq, *hpart, *hsum, *gpart, *gram, *mean, *xsq, *f0;
  // vprod: V = W panel is formed; qprod: Q = W^T V[slot 0] too; gram_w: width of a query's Gram result (0: none);
  // colsq: the diagonal form's column sums of squares; hper: doubles of a sample's reduced Hessian sums (0: none);
  // prow: tile rows of the operand kernel's fused mean product (0: npad / 64; gpc_grad_post_gobs: the rows of its point
  // list / 64, which can exceed npad / 64 -- N = 65, Ng = 1, D = 1 has 3 against 2)
  void layout(ScratchCarver& sc, int cnt, int npad, int D, bool vprod, bool qprod, int gram_w, bool colsq_, size_t hper,
              int prow = 0) {
    const size_t c = cnt, mb = GQB, ld = (size_t)(D + 1) * mb, sP = (size_t)npad * ld, nt64 = npad / CT;
    const size_t pt = prow > 0 ? (size_t)prow : nt64;
    const size_t gper = mb * (D + 1) * gram_w, nseg = gram_segments(npad);
    P = sc.take<T>(c * sP, 16);                           // [ k | dk/dx*_1 .. dk/dx*_D ]
    V = sc.take<T>(vprod ? c * sP : 0, 16);               // V = W panel | Z = L panel
    Q = sc.take<T>(qprod ? c * npad * mb : 0, 16);
    part = sc.take(c * pt * ld, 16);                      // the operand kernel's fused mean product, per tile row
    colsq = sc.take(colsq_ ? c * (npad / TILE) * ld : 0, 16);
    hpart = sc.take(c * nt64 * hper, 16);                 // the contraction's per-tile partials and their sums
    hsum = sc.take(c * hper, 16);
    gpart = sc.take(nseg > 1 ? c * nseg * gper : 0, 16);  // the Gram kernel's segments
    gram = sc.take(c * gper, 16);
    mean = sc.take(c * ld, 16);
    xsq = sc.take(c * mb * D, 16);                        // the scaled queries of the block
    f0 = sc.take(c);
  }
};

// ---- gpc_nll_hess, gpc_cv_grad, gpc_predict_hyp_grad -------------------------------------------------------------------
// Device buffers of a chunk of `cnt` samples, carved from one allocation (all doubles; vectors are [plane][sample][npad])
struct NhScratch {
  int npad = 0, ppl = 0, cov_N = 0, noise_N = 0, mean_N = 0, nt = 0, ntl = 0, npairs = 0, nd2 = 0;
  double *Q, *B, *Op, *X, *Y, *E, *diagq, *upart, *gpart, *gsum, *grpart, *grsum, *d2part, *d2sum;
  void layout(ScratchCarver& sc, int cnt, int npad_, int cov_N_, int noise_N_, int mean_N_, int nd2_) {
    npad = npad_, cov_N = cov_N_, noise_N = noise_N_, mean_N = mean_N_, nd2 = nd2_;
    ppl = cov_N + noise_N, nt = npad / CT, ntl = nt * (nt + 1) / 2, npairs = ppl * (ppl + 1) / 2;
    const size_t n2 = (size_t)npad * npad, c = cnt;
    Q = sc.take(c * n2);
    B = sc.take(c * ppl * n2);
    Op = sc.take(c * n2);
    X = sc.take(c * (ppl + mean_N) * npad);
    Y = sc.take(c * (ppl + mean_N) * npad);
    E = sc.take(c * noise_N * npad);
    diagq = sc.take(c * npad);
    upart = sc.take(c * nt * npad);
    gpart = sc.take(c * nt * nt * 2);
    gsum = sc.take(c * cov_N * 2);
    grpart = sc.take(c * nt * nt * npairs);
    grsum = sc.take(c * npairs);
    d2part = sc.take(c * ntl * nd2);
    d2sum = sc.take(c * nd2);
  }
};

// Device buffers of a chunk of `cnt` samples, carved from one allocation (all doubles; vectors are [sample][npad])
struct CvgScratch {
  double *Q, *QC, *M, *diagq, *u, *b, *part, *out;
  // the block that is downloaded, in order: gsum [cnt][cov_N] | diagG | beta | q | cw, [cnt][npad] each
  double *gsum, *diagG, *beta, *q, *cw;
  size_t out_bytes = 0;
  void layout(ScratchCarver& sc, int cnt, int npad, int cov_N) {
    const size_t n2 = (size_t)npad * npad, nt = npad / CT, ntl = nt * (nt + 1) / 2, c = cnt;
    Q = sc.take(c * n2);
    QC = sc.take(c * n2);
    M = sc.take(c * n2);
    diagq = sc.take(c * npad);
    u = sc.take(c * npad);
    b = sc.take(c * npad);
    part = sc.take(c * ntl * cov_N);
    const size_t before_out = sc.bytes;
    out = gsum = sc.take(c * cov_N);
    diagG = sc.take(c * npad);
    beta = sc.take(c * npad);
    q = sc.take(c * npad);
    cw = sc.take(c * npad);
    out_bytes = sc.bytes - before_out;
  }
};

// Device buffers of a chunk of `cnt` samples and one super-block of `msb` queries, carved from one allocation (all
// doubles; vectors are [vector][sample][npad], panels [sample][npad][msb])
struct HgScratch {
  double *Op, *KP, *VP, *Qa, *X, *Y, *Vn, *tmp, *tpart, *upart, *mupart, *cpart, *csum, *dpart, *dsum, *xss, *qs;
  void layout(ScratchCarver& sc, int cnt, int npad, int D, int P, int nvv, int ngp, int msb, bool var, int nout) {
    const size_t n2 = (size_t)npad * npad, nt = npad / CT, nch = npad / TRC, np = npad, mm = msb, c = cnt;
    Op = sc.take(var ? c * n2 : 0);
    KP = sc.take(var ? c * np * mm : 0);
    VP = sc.take(var ? c * np * mm : 0);
    Qa = sc.take(var ? c * np * mm : 0);
    dpart = sc.take(var ? c * nt * (1 + (size_t)nvv) * mm : 0);
    dsum = sc.take(var ? c * ((size_t)ngp + nvv) * mm : 0);
    mupart = sc.take(var ? c * nt * mm : 0);
    Vn = sc.take(var ? c * (size_t)nvv * np : 0);
    X = sc.take(c * P * np);
    Y = sc.take(c * P * np);
    tmp = sc.take(c * np);
    tpart = sc.take(c * nch * np);
    upart = sc.take(c * nt * np);
    cpart = sc.take(c * nt * nout * mm);
    csum = sc.take(c * nout * mm);
    xss = sc.take(c * mm * D);
    qs = sc.take(c);
  }
};

// ---- gpc_post_append_block, gpc_post_remove --------------------------------------------------------------------------
// Device arrays of a chunk of `cnt` samples of a block append: the three slabs of the k x k factorization and (MFMA
// engine) B, V | G and W^T V in the storage type, then four n x k panels, the k x k products and three vectors
template <typename T>
struct AppendScratch {
  T *fA, *fW, *fT, *Bt, *Vt, *Qt;
  double *Bx, *V, *Pt, *GS, *Cm, *ev, *tv, *zv;
  void layout(ScratchCarver& sc, int cnt, int npad, int kq, int kp, bool use_gemm) {
    const size_t c = cnt, panel = (size_t)npad * kq, tpanel = use_gemm ? (size_t)npad * kp : 0;
    fA = sc.take<T>(c * kp * kp, 16);
    fW = sc.take<T>(c * kp * kp, 16);
    fT = sc.take<T>(c * kp * kp, 16);
    Bt = sc.take<T>(c * tpanel, 16);
    Vt = sc.take<T>(c * tpanel, 16);
    Qt = sc.take<T>(c * tpanel, 16);
    Bx = sc.take(c * panel, 16);  // the cross covariances
    V = sc.take(c * panel, 16);   // high noise: W B;  low noise: G = -A B
    Pt = sc.take(c * panel, 16);  // high noise: (V^T W / sl), k x n;  low noise: H = G W22^T, n x k
    GS = sc.take(c * panel, 16);  // low noise: G Si
    Cm = sc.take(c * kq * kq, 16);  // V^T V | B^T G
    ev = sc.take(c * kq, 16);
    tv = sc.take(c * kq, 16);
    zv = sc.take(c * kq, 16);
  }
};

// Device buffers of one sweep over a chunk of `cnt` samples, carved from the consumers' block; the sweep's row maps
// (npn + kk ints, once per sweep) follow them
template <typename T>
struct RmScratch {
  T *fA, *fW, *fT;
  double *V, *C, *H, *Th, *aI, *tv, *zv;
  void layout(ScratchCarver& sc, int cnt, int npn, int kq, int kp) {
    const size_t c = cnt, panel = (size_t)npn * kq, mp = RM_P + kq;
    fA = sc.take<T>(c * kp * kp, 16);  // the three slabs of the k x k factorization
    fW = sc.take<T>(c * kp * kp, 16);
    fT = sc.take<T>(c * kp * kp, 16);
    V = sc.take(c * panel, 16);    // A[R, I]: the L-side carrier | the low-noise panel
    C = sc.take(c * panel, 16);    // W[I, R]: the W-side carrier
    H = sc.take(c * panel, 16);    // low noise: A[R, I] Wq^T
    Th = sc.take(c * mp * mp, 16);
    aI = sc.take(c * kq, 16);
    tv = sc.take(c * kq, 16);
    zv = sc.take(c * kq, 16);
  }
};

// ---- gpc_cv ---------------------------------------------------------------------------------------------------------------
// Device arrays of a chunk of `cnt` samples.  Leave-one-out: five planes of N_pad per sample, downloaded as one block
// (the info plane is as wide as the others: N_pad ints and as many bytes unused)
struct CvLooScratch {
  double *dmu, *s2, *quad, *logdet;
  int* info;
  void layout(ScratchCarver& sc, int cnt, int npad) {
    const size_t pl = (size_t)cnt * npad;
    dmu = sc.take(pl, 16);
    s2 = sc.take(pl, 16);
    quad = sc.take(pl, 16);
    logdet = sc.take(pl, 16);
    info = sc.take<int>(2 * pl, 16);
  }
};

// Folds: G, its inverse factor and the factorization's third slab for every (sample, fold) pair (one memset), engine
// 2's gathered panels, the vectors u, and the block that is downloaded: [dmu | s2 | quad | logdet | ld | info]
struct CvFoldScratch {
  double *G, *Wf, *Tm, *panel, *uv, *o_dmu, *o_s2, *o_quad, *o_logdet, *ld;
  int* info;
  void layout(ScratchCarver& sc, int cnt, int npad, int F, int kp, bool panels) {
    const size_t c = cnt, np = c * F, kk = (size_t)kp * kp;
    G = sc.take(np * kk, 16);
    Wf = sc.take(np * kk, 16);
    Tm = sc.take(np * kk, 16);
    panel = sc.take(panels ? np * npad * kp : 0, 16);
    uv = sc.take(np * kp, 16);
    o_dmu = sc.take(c * npad, 16);
    o_s2 = sc.take(c * npad, 16);
    o_quad = sc.take(np);
    o_logdet = sc.take(np);
    ld = sc.take(np);
    info = sc.take<int>(2 * np);  // (as wide as the planes beside it: the download counts in doubles)
  }
};

// ---- gpc_paths_create, gpc_paths_eval -----------------------------------------------------------------------------------
// gpc_paths_create's arrays of `cnt` samples: three fp64 N_pad x kq panels (p(X), P, V1) and, for the MFMA engine,
// three N_pad x kp panels in the storage type (and 64 spare bytes per sample)
template <typename T>
struct PathsCreateScratch {
  double *pX, *P, *V1;
  T *Bt, *Vt, *Qt;
  void layout(ScratchCarver& sc, int cnt, int npad, int kq, int kp, bool use_gemm) {
    const size_t c = cnt, sP = (size_t)npad * kq, sK = use_gemm ? (size_t)npad * kp : 0;
    pX = sc.take(c * sP, 16);
    P = sc.take(c * sP, 16);
    V1 = sc.take(c * sP, 16);
    Bt = sc.take<T>(c * sK, 16);
    Vt = sc.take<T>(c * sK, 16);
    Qt = sc.take<T>(c * sK, 16);
    sc.take<char>(c * 64);
  }
};

// gpc_paths_eval's: the unfused engine's operand, product, and v and the weights widened to whole tiles, then the
// scaled queries; once per call the results in the caller's layout and the raw queries
struct PathsEvalScratch {
  double *op, *Cb, *Vp, *Wp, *xq;
  void layout(ScratchCarver& sc, int cnt, int npad, int fpad, int mpad, int rp, int D, bool unfused) {
    const size_t c = unfused ? cnt : 0;
    op = sc.take(c * std::max(npad, fpad) * mpad, 16);
    Cb = sc.take(c * mpad * rp, 16);
    Vp = sc.take(c * npad * rp, 16);
    Wp = sc.take(c * fpad * rp, 16);
    xq = sc.take((size_t)cnt * mpad * D, 16);
  }
};

struct PathsEvalShared {
  double *f, *df, *x;
  void layout(ScratchCarver& sc, int M, int R, int S, int D, bool grad) {
    const size_t n = (size_t)M * R * S;
    f = sc.take(n);
    df = sc.take(grad ? n * D : 0);
    x = sc.take((size_t)M * D);
  }
};

// ---- gpc_quad_mix ---------------------------------------------------------------------------------------------------------
// The scratch of gpc_quad_mix, one allocation (c->qmix): the measures' block that the samples share, then the arrays of
// `cnt` samples
struct QuadMixShared {
  double *mut, *sgt, *wpad, *mu, *sg, *w;
  void layout(ScratchCarver& sc, int M, int mpad, int D) {
    mut = sc.take((size_t)mpad * D);
    sgt = sc.take((size_t)mpad * D);
    wpad = sc.take(mpad);
    mu = sc.take((size_t)M * D);
    sg = sc.take((size_t)M * D);
    w = sc.take(M);
  }
};

struct QuadMixScratch {
  double *con, *cpart, *rpart, *zbar, *v, *q, *tpart, *zqpart, *gpart, *gmpart, *res;
  void layout(ScratchCarver& sc, int cnt_, int npad, int mpad, int D, bool var, bool grad) {
    const size_t cnt = cnt_, gnt = npad / CT, mnt = mpad / CT, nch = npad / TRC;
    const size_t gpl = grad ? (var ? 4 : 2) : 0, gnq = var ? (grad ? 1 + 2 * D : 1) : 0, npl = gpl + (var && grad ? 2 : 0);
    con = sc.take(cnt * (D + 1) * mpad);
    cpart = sc.take(cnt * gnt * mpad);
    rpart = sc.take(cnt * mnt * npad);
    zbar = sc.take(cnt * npad);
    v = sc.take(var ? cnt * npad : 0);
    q = sc.take(var ? cnt * npad : 0);
    tpart = sc.take(var ? cnt * nch * npad : 0);
    zqpart = sc.take(var ? cnt * gnt * mpad : 0);
    gpart = sc.take(cnt * gnt * gpl * D * mpad);
    gmpart = sc.take(cnt * mnt * gnq * mpad);
    // the results, one block: [za | zq | gw | scal (2 per sample) | planes of the tile pass | planes of the pair pass]
    res = sc.take(cnt * (3 * (size_t)mpad + 2 + npl * (size_t)mpad * D));
  }
};

// ---- gpc_nll_batch_gobs_grad, gpc_debug_gobs_trace ---------------------------------------------------------------------
// The partials of gradobs.h's gobs_trace kernels for a chunk of `cnt` samples: one row of `pst` doubles (the covariance
// hyperparameters, and whatever else the caller's output row holds) per block of their three grids -- the value / value
// tiles of the lower triangle, the gradient / value tiles, and D per gradient / gradient tile (GobsDims::trace_rows)
struct GobsTraceScratch {
  double* part;
  void layout(ScratchCarver& sc, int cnt, const GobsDims& gd, int pst) {
    part = sc.take((size_t)cnt * (size_t)gd.trace_rows() * pst);
  }
};

// ---- any layout by name ---------------------------------------------------------------------------------------------------
// per_layout(sc, cnt) / shared_layout(sc): a consumer's two lists.  Counted, then carved -- three samples and the shared
// part behind them -- on a 256-byte aligned base that is never dereferenced
template <typename PerFn, typename SharedFn>
int scratch_report(PerFn&& per_layout, SharedFn&& shared_layout, size_t beside, unsigned long long* per,
                   unsigned long long* shared, int* misaligned) {
  ScratchCarver one, sh;
  per_layout(one, 1);
  shared_layout(sh);
  char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);
  ScratchCarver cp(base), cs(base + 3 * one.bytes);
  per_layout(cp, 3);
  shared_layout(cs);
  *per = one.bytes + beside;
  *shared = sh.bytes;
  *misaligned = one.misaligned + cp.misaligned + cs.misaligned;
  return 0;
}
template <typename T>
int scratch_bytes_of(const std::string& name, const int* d, int n, unsigned long long* per, unsigned long long* shared,
                     int* mis) {
  const auto none = [](ScratchCarver&) {};
  const int npad = n > 0 ? pad_tile(d[0]) : 0;
  if (name == "rhs" && n == 11) {  // N, M, D, S, kind, want_quad, full, grad, qg, R, gobs points
    const RhsDims rd = RhsDims::of(d[0], d[1], d[2], d[3], d[4], d[5] != 0, d[6] != 0, d[7] != 0, d[8] != 0, d[9], d[10]);
    return scratch_report([&](ScratchCarver& sc, int cnt) { RhsScratch<T>().layout(sc, cnt, rd); },
                          [&](ScratchCarver& sc) { RhsShared().layout(sc, rd); }, 3 * rd.template slab_bytes<T>(), per, shared, mis);
  }
  if (name == "predict_cov" && n == 6) {  // N, Ma, Mb, D, want_cov, want_wsq
    const int ma = pad_tile(d[1]), mb = pad_tile(d[2]);
    const bool fused = cov_fused_form(ma, mb, d[5] != 0, d[4] != 0);
    return scratch_report([&](ScratchCarver& sc, int cnt) { CovScratch<T>().layout(sc, cnt, npad, ma, mb, d[3], fused); },
                          [&](ScratchCarver& sc) { CovShared().layout(sc, d[1], d[2], d[3], d[4] != 0); }, 0, per, shared, mis);
  }
  if ((name == "grad_post" || name == "predict_hess") && n == 4) {  // N, M, D, diag | var
    const bool hess = name == "predict_hess", f = d[3] != 0;
    const int D = d[2];
    const size_t hper = hess ? (size_t)(f ? 2 : 1) * hess_planes(D) * GQB : 0;
    return scratch_report(
        [&](ScratchCarver& sc, int cnt) {
          if (hess) BlockScratch<T>().layout(sc, cnt, npad, D, f, f, f ? D + 1 : 0, false, hper);
          else BlockScratch<T>().layout(sc, cnt, npad, D, true, false, f ? 1 : D + 1, f, hper);
        },
        [&](ScratchCarver& sc) { sc.take((size_t)d[1] * D); }, 0, per, shared, mis);
  }
  if (name == "grad_post_gobs" && n == 4) {  // N, Ng, D, diag: one block of queries (the raw queries are the caller's M x D)
    GobsDims gd;
    gd.N = d[0], gd.Ng = d[1], gd.D = d[2];
    const bool f = d[3] != 0;
    const int jpad = pad_tile((int)gd.n());
    return scratch_report(
        [&](ScratchCarver& sc, int cnt) {
          BlockScratch<T>().layout(sc, cnt, jpad, gd.D, true, false, f ? 1 : gd.D + 1, f, (size_t)0, gd.P() / CT);
        },
        none, 0, per, shared, mis);
  }
  if (name == "append_block" && n == 3) {  // N + k, k, engine
    const int k = d[1], kq = ((k + BA_R - 1) / BA_R) * BA_R;
    return scratch_report([&](ScratchCarver& sc, int cnt) { AppendScratch<T>().layout(sc, cnt, npad, kq, pad_tile(k), d[2] == 2); },
                          none, 0, per, shared, mis);
  }
  if (name == "remove" && n == 2) {  // N, k: the first sweep
    const int kk = std::min(d[1], RM_KMAX), npn = pad_tile(d[0] - kk);
    return scratch_report([&](ScratchCarver& sc, int cnt) { RmScratch<T>().layout(sc, cnt, npn, rm_kq(kk), pad_tile(kk)); },
                          [&](ScratchCarver& sc) { sc.take<int>((size_t)npn + kk); }, 0, per, shared, mis);
  }
  if (name == "cv_loo" && n == 1)
    return scratch_report([&](ScratchCarver& sc, int cnt) { CvLooScratch().layout(sc, cnt, npad); }, none, 0, per, shared, mis);
  if (name == "cv_fold" && n == 4)  // N, F, k_max, engine
    return scratch_report([&](ScratchCarver& sc, int cnt) { CvFoldScratch().layout(sc, cnt, npad, d[1], pad_tile(d[2]), d[3] == 2); },
                          none, 0, per, shared, mis);
  if (name == "paths_create" && n == 3) {  // N, R, solve engine
    const int kq = ((d[1] + BA_R - 1) / BA_R) * BA_R;
    return scratch_report([&](ScratchCarver& sc, int cnt) { PathsCreateScratch<T>().layout(sc, cnt, npad, kq, pad_tile(d[1]), d[2] == 2); },
                          none, 0, per, shared, mis);
  }
  if (name == "paths_eval" && n == 8)  // N, M, R, S, D, F_pad, engine, grad
    return scratch_report(
        [&](ScratchCarver& sc, int cnt) { PathsEvalScratch().layout(sc, cnt, npad, d[5], pad_tile(d[1]), pad_tile(d[2]), d[4], d[6] == 2); },
        [&](ScratchCarver& sc) { PathsEvalShared().layout(sc, d[1], d[2], d[3], d[4], d[7] != 0); }, 0, per, shared, mis);
  if (name == "nll_hess" && n == 5)  // N, cov_N, noise_N, mean_N, nd2
    return scratch_report([&](ScratchCarver& sc, int cnt) { NhScratch().layout(sc, cnt, npad, d[1], d[2], d[3], d[4]); }, none, 0,
                          per, shared, mis);
  if (name == "cv_grad" && n == 2)  // N, cov_N
    return scratch_report([&](ScratchCarver& sc, int cnt) { CvgScratch().layout(sc, cnt, npad, d[1]); },
                          [&](ScratchCarver& sc) { sc.take(npad); }, 0, per, shared, mis);
  if (name == "hyp_grad" && n == 8)  // N, D, P, nvv, ngp, msb, var, nout
    return scratch_report([&](ScratchCarver& sc, int cnt) { HgScratch().layout(sc, cnt, npad, d[1], d[2], d[3], d[4], d[5], d[6] != 0, d[7]); },
                          none, 0, per, shared, mis);
  if (name == "gobs_trace" && n == 4) {  // N, Ng, D, doubles per row
    GobsDims gd;
    gd.N = d[0], gd.Ng = d[1], gd.D = d[2];
    return scratch_report([&](ScratchCarver& sc, int cnt) { GobsTraceScratch().layout(sc, cnt, gd, d[3]); }, none, 0, per, shared, mis);
  }
  if (name == "quad_mix" && n == 5)  // N, M, D, var, grad
    return scratch_report([&](ScratchCarver& sc, int cnt) { QuadMixScratch().layout(sc, cnt, npad, pad_tile(d[1]), d[2], d[3] != 0, d[4] != 0); },
                          [&](ScratchCarver& sc) { QuadMixShared().layout(sc, d[1], pad_tile(d[1]), d[2]); }, 0, per, shared, mis);
  return -2;
}

}  // namespace gpc
