/*
 * gpcore.h -- C ABI of libgpcore.so, the MI355X (gfx950) dense Gaussian-process core.
 *
 * The reference (acerbilab/gpyreg) is pure Python and has no FFI; its boundary for
 * this path is the duck-typed plugin protocol GP.__init__(D, covariance, mean, noise)
 * (gaussian_process.py:43-49).  The entry points below are what a ctypes binding on
 * the reference side would call in place of the NumPy/SciPy bodies cited per function
 * (see INTEGRATION.md for the stub).  Plain pointers and sizes only; all arrays are
 * caller-owned host memory, row-major (C order) float64 unless stated; the library
 * copies inputs to the device and copies results back before returning.
 *
 * Return value: 0 = OK; -1 = HIP error, -2 = usage error, -3 = internal error (a wave hand-off inside a
 * 128 x 128 leaf factorization timed out; the results of that call are invalid) -- text via gpc_last_error;
 * per-sample numerical failure (a matrix that is not positive definite after the reference's ten jitter
 * levels, gaussian_process.py:2413-2421, :2450-2453) is reported in info[] (>0), never as a return code.
 *
 * Thread-safety: one gpc_ctx per host thread / per device; calls on one ctx serialize.
 */
#ifndef GPCORE_H
#define GPCORE_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpc_ctx gpc_ctx;   /* one per (process, device): streams, workspace, X, y */
typedef struct gpc_post gpc_post; /* device-resident posteriors of one hyp batch        */

/* covariance families: covariance_functions.py:131 (SE), :189 (Matern), :288 (RQ-ARD),
 * isotropic_covariance_functions.py:164 (SE iso), :86 (Matern iso). */
enum { GPC_K_SE = 0, GPC_K_MATERN = 1, GPC_K_RQ = 2, GPC_K_SE_ISO = 3, GPC_K_MATERN_ISO = 4 };
/* arithmetic type of the factorization (kernel build and reductions are always f64) */
enum { GPC_F64 = 0, GPC_F32 = 1 };

/* ---- lifetime ---------------------------------------------------------------- */
int gpc_create(int device, gpc_ctx** out);
void gpc_destroy(gpc_ctx* ctx);
/* last error text of ctx (or of the failed gpc_create when ctx == NULL) */
const char* gpc_last_error(const gpc_ctx* ctx);
/* "gfx950 ..." style description of the device and library build */
const char* gpc_device_info(gpc_ctx* ctx);

/* ---- training data (GP.update stores X, y: gaussian_process.py:846-862) -------- */
/* X: N x D, y: N.  Kept resident in HBM until the next gpc_set_data. */
int gpc_set_data(gpc_ctx* ctx, const double* X, const double* y, int N, int D);

/* number of covariance hyperparameters (covariance_functions.py:59-73, :291-292;
 * isotropic_covariance_functions.py:14-28) */
int gpc_cov_count(int kernel_id, int D);
/* Largest N the dense stages accept for a dtype: a MEMORY-BUDGET answer (round 6) -- the largest multiple of 128 whose
 * three padded N x N slabs of one sample (matrix / factor, inverse factor, scratch) fit in 80 % of the current device's
 * memory (fp64 on a 288 GB MI355X: 101 504; fp32: 143 488).  The reference factorizes whatever fits host memory
 * (gaussian_process.py:2415-2417, :2477-2484); so does this library with device memory.  (Rounds 1-5 answered 16384 /
 * 23168: one 32-bit byte offset spanned a k-major operand panel.  The GEMM now advances a 64-bit base per k-slab.)
 * The batch entry points return -2 above it.  Without a visible device the answer assumes 288 GB.                       */
int gpc_max_n(int dtype);

/* ---- covariance.compute() (covariance_functions.py:135-186, :221-285, :301-367;
 *      isotropic_covariance_functions.py:104-161, :173-221) ------------------------
 * Xstar == NULL, diag == 0 : K is N x N; if dK != NULL it receives N x N x cov_N.
 * Xstar != NULL            : K is N x M (cross covariance), dK must be NULL.
 * diag != 0                : K is N (x1): the self-covariance diagonal.            */
int gpc_kernel(gpc_ctx* ctx, int kernel_id, int degree, const double* hyp_cov,
               const double* X, int N, int D, const double* Xstar, int M, int diag,
               double* K, double* dK);

/* ---- GP.__core_computation(hyp, 1, want_grad) for S hyperparameter vectors -------
 * (gaussian_process.py:2357-2512).  The covariance part runs on the device from
 * hyp_cov; mean and noise plugins are evaluated by the caller (they are O(N*D)
 * boundary plugins, mean_functions.py / noise_functions.py) and passed as arrays:
 *   hyp_cov  S x cov_N
 *   m        S x N           mean function values
 *   sn2      S x (sn2_is_vector ? N : 1)   noise variance (noise_functions.py:249-278)
 *   dm       S x N x mean_N  (want_grad && mean_N > 0, else NULL)
 *   dsn2     S x (sn2_is_vector ? N : 1) x noise_N (want_grad && noise_N > 0)
 * Outputs:
 *   nlz      S               negative log marginal likelihood
 *   dnlz     S x (cov_N+noise_N+mean_N), order [cov | noise | mean] (:2367-2369)
 *   sn2_mult S               final jitter multiplier (power of 10, :2413-2421)
 *   L_chol   S               1 if min(sn2) >= 1e-6 (:2404)
 *   info     S               0 ok; >0: still not positive definite after 10 tries
 *                            (the caller raises LinAlgError, :2450-2453)            */
int gpc_nll_batch(gpc_ctx* ctx, int kernel_id, int degree, int dtype, int S,
                  const double* hyp_cov, const double* m, const double* sn2,
                  int sn2_is_vector, int want_grad, const double* dm, int mean_N,
                  const double* dsn2, int noise_N, double* nlz, double* dnlz,
                  double* sn2_mult, int* L_chol, int* info);

/* ---- the same call for the stock ZeroMean / ConstantMean (mean_functions.py:82-131, :210-260): the mean is ONE value
 * per sample, m0[S] (mean_N = 1; NULL with mean_N = 0 for the zero mean), and its derivative is all ones -- so neither
 * m (S x N) nor dm (S x N x 1) crosses the bus: r = y - m0 is formed on the device from the resident y, and with a scalar
 * noise model so is the diagonal term.  Results are those of gpc_nll_batch with m[s][i] = m0[s], dm = 1, to the bit.     */
int gpc_nll_batch_cm(gpc_ctx* ctx, int kernel_id, int degree, int dtype, int S, const double* hyp_cov,
                     const double* m0, int mean_N, const double* sn2, int sn2_is_vector, int want_grad,
                     const double* dsn2, int noise_N, double* nlz, double* dnlz, double* sn2_mult,
                     int* L_chol, int* info);

/* ---- the same for ANY covariance object: caller-provided K and dK -------------------------------
 * The reference calls whatever object it was given -- `covariance.compute(hyp, X, compute_grad)`
 * (gaussian_process.py:2388-2390; AbstractKernel, covariance_functions.py:9-20).  A kernel this
 * library does not know is evaluated by the caller; the factorization, solves and the gradient
 * contraction still run on the device:
 *   K        S x N x N (row-major; symmetric)
 *   dk_plane callback: fill plane[N*N] (row-major) with dK[:, :, p] of sample `sample`; called once
 *            per (sample, p < cov_N) when want_grad, so the (N, N, cov_N) tensor is streamed one
 *            plane at a time and never resident on the device.  Return 0, or nonzero to abort.
 * Everything else (m, sn2, dm, dsn2, outputs, jitter escalation) as gpc_nll_batch; dnlz is ordered
 * [cov (cov_N) | noise | mean].                                                                     */
typedef int (*gpc_dk_plane_fn)(void* user, int sample, int p, double* plane);
int gpc_nll_batch_K(gpc_ctx* ctx, int dtype, int S, int cov_N, const double* K, gpc_dk_plane_fn dk_plane,
                    void* user, const double* m, const double* sn2, int sn2_is_vector, int want_grad,
                    const double* dm, int mean_N, const double* dsn2, int noise_N, double* nlz,
                    double* dnlz, double* sn2_mult, int* L_chol, int* info);
/* Posteriors from caller-provided K (GP.update with a user-defined kernel).  Use gpc_predict_K with
 * them; gpc_post_fetch / gpc_post_free as usual.                                                   */
int gpc_posterior_batch_K(gpc_ctx* ctx, int dtype, int S, const double* K, const double* m,
                          const double* sn2, int sn2_is_vector, gpc_post** post, double* sn2_mult,
                          int* L_chol, int* info);
/* Predictive products from caller-provided cross covariances Ks (S x N x M) -- works for posteriors
 * of either origin:
 *   fmu[j*S + s] = Ks_s[:, j] . alpha_s
 *   fq [j*S + s] = -colsum(V*V) (L_chol) or +colsum(Ks * (L Ks)): ADD kss to get s2 (:1752-1764); may be NULL
 *   cov[s]       = Kss_s - V^T V  or  Kss_s + Ks^T (L Ks)   (M x M; needs Kss, S x M x M); may be NULL  */
int gpc_predict_K(gpc_post* post, int M, const double* Ks, const double* Kss, double* fmu, double* fq,
                  double* cov);

/* ---- GP.__core_computation(hyp, 0, 0) -> Posterior, for S vectors
 *      (gaussian_process.py:2514-2521; GP.update loop :870-884) ---------------------
 * The factors stay in HBM inside *post (freed by gpc_post_free).                   */
int gpc_posterior_batch(gpc_ctx* ctx, int kernel_id, int degree, int dtype, int S,
                        const double* hyp_cov, const double* m, const double* sn2,
                        int sn2_is_vector, gpc_post** post, double* sn2_mult,
                        int* L_chol, int* info);
/* Posterior fields of sample s (gaussian_process.py:2568-2586).  Any pointer may be
 * NULL.  alpha: N.  sW: N.  L: N x N row-major holding, when L_chol, the LOWER
 * factor Lo with Lo Lo^T = (K + mult*Sigma)/sl -- the reference's upper factor is
 * its transpose (a free NumPy view) -- else -(K + mult*Sigma)^-1 (:2441-2448).      */
int gpc_post_fetch(gpc_post* post, int s, double* alpha, double* sW, double* L);
int gpc_post_free(gpc_post* post);

/* ---- GP.predict K* solves (gaussian_process.py:1741-1764) --------------------------
 * xstar: M x D.  For every posterior sample s:
 *   fmu[j*S + s]  = Ks^T alpha                (caller adds the mean function m*)
 *   fs2[j*S + s]  = kss - colsum(V*V)   or   kss + colsum(Ks * (L Ks))   (unclamped) */
int gpc_predict(gpc_post* post, const double* xstar, int M, double* fmu, double* fs2);

/* ---- GP.predict_grad: gradients of the predictive mean and variance with respect to x* -------------
 * fmu, fs2 as gpc_predict; for every sample s, query point j and input dimension l (D of gpc_set_data):
 *   dfmu[(j*D + l)*S + s] = d fmu_js / d x*_jl = -c_l sum_i alpha_i F_ij (xs*_jl - xs_il)
 *   dfs2[(j*D + l)*S + s] = d fs2_js / d x*_jl = -2 sum_i Q_ij dk_ij / dx*_jl
 *                         =  2 c_l sum_i Q_ij F_ij (xs*_jl - xs_il)
 * with xs = x mul / dv the scaled inputs of the kernel family, c_l = mul_l / dv_l, F the radial factor of
 * the covariance (dK / dlog ell_l = F d_l), and Q = (K + Sigma)^-1 K* under the posterior's own scaling:
 * W^T (W K*) / sl for L_chol samples, -(A K*) otherwise.  kss is constant (stationary kernels): it adds
 * nothing.  A pair with x* equal to a training point contributes 0 (Matern nu = 1: by convention).  The
 * mean function's gradient, the clamp of fs2 at 0 and the mixture over samples are the caller's.
 * Posteriors from caller-provided K fail with a message, as in gpc_predict.                             */
int gpc_predict_grad(gpc_post* post, const double* xstar, int M, double* fmu, double* fs2, double* dfmu,
                     double* dfs2);

/* ---- GP.gradient_posterior: the joint posterior of (f(x*), grad f(x*)) per sample ----------------------
 * With B_j = [ k(X, x*_j) | G_j ], G_j[i, l] = dk(x*_j, X_i) / dx*_jl = -c_l F_ij (xs*_jl - xs_il) (F, c_l, xs of
 * gpc_predict_grad; a pair at distance 0 contributes 0 to G) and the prior block H = diag(kss, F0 c_1^2, ..., F0 c_D^2),
 * F0 = F at distance 0 (stationary kernels: the value / derivative cross terms vanish at coincident points):
 *   fmu[j*S + s]            = B_j^T alpha, slot 0                         (as gpc_predict)
 *   dfmu[(j*D + l)*S + s]   = B_j^T alpha, slot 1 + l                     (as gpc_predict_grad)
 *   cov[((j*(D+1) + a)*(D+1) + b)*S + s] = C_j[a, b],   slot 0 = f, slot 1 + l = d/dx_l,
 *     C_j = H - V_j^T V_j / sl, V_j = W B_j (L_chol samples)   |   C_j = H + B_j^T (L B_j) (L = -inv)
 *   diag_only != 0:  cov[(j*(D+1) + a)*S + s] = C_j[a, a] only (no Gram matrix is formed for L_chol samples)
 * C_j[0, 0] is gpc_predict's fs2, C_j[0, 1 + l] half of gpc_predict_grad's dfs2.  The full matrix is symmetric to the
 * bit (the lower triangle is computed and mirrored) and returned as computed: no clamp, no projection to PSD, no
 * noise, no mean function -- those are the caller's.  The queries are worked on in blocks of 128 whatever the memory
 * budget (GPC_MEM_BUDGET_MB), which decides the samples per chunk only: a sample's results do not depend on it.
 * Returns -2 with a message of its own for: bad arguments; a posterior from caller-provided K; the Matern kernel of
 * degree 1 (ARD or isotropic: no mean-square derivative, F0 is infinite); a posterior that holds a failed
 * factorization; one sample with one query block exceeding the budget (the message names N_pad, D, the block size and
 * the bytes).  gpc_last_timing: ms_total = the device sections, ms_factor = the products with W (or L).               */
int gpc_grad_post(gpc_post* post, const double* xstar, int M, int diag_only, double* fmu, double* dfmu, double* cov);

/* ---- GP.predict_hess: Hessians of the predictive mean and variance with respect to x*, per sample ------------------
 * With d = xs*_j - xs_i, r2 = |d|^2, F and c_l of gpc_predict_grad and the second radial factor G = -2 dF/d(r2)
 * (SE: K; Matern 3: e / t; Matern 5: e / 3, e = sf2 exp(-t), t = sqrt(r2); RQ: (alpha + 1) / alpha F / m),
 *   d^2 k / dx*_a dx*_b = c_a c_b (G d_a d_b - F delta_ab),
 *   hmu[((j*D + a)*D + b)*S + s] = c_a c_b ( sum_i alpha_i G_ij d_a d_b - delta_ab sum_i alpha_i F_ij )
 *   hs2[((j*D + a)*D + b)*S + s] = -2 ( P_j[a, b] + c_a c_b ( sum_i Q_ij G_ij d_a d_b - delta_ab sum_i Q_ij F_ij ) )
 *   P_j[a, b] = (d_a k*)^T (K + Sigma)^-1 (d_b k*): the derivative block of gpc_grad_post's Gram matrix,
 * Q = (K + Sigma)^-1 k* as gpc_predict_grad forms it.  A pair at r2 = 0 contributes 0 to the G term (its limit, also
 * where G is infinite) and its full F(0) to the diagonal term.  fmu, fs2, dfmu, dfs2 are laid out as gpc_predict_grad's
 * and come from the operand panel and the Gram matrix of gpc_grad_post (they agree with gpc_predict_grad's to
 * rounding, not to the bit).  Every matrix is symmetric to the bit (the lower triangle is computed and mirrored);
 * results are unclamped, without noise or mean function.  Queries are worked on in blocks of 128 whatever the memory
 * budget, which decides the samples per chunk only: a sample's results do not depend on it.
 * compute_var == 0: no product with W or L is launched; fs2, dfs2, hs2 may be NULL and are not written; fmu, dfmu and
 * hmu carry the same bits as with the variance; gpc_last_timing's ms_factor is 0.
 * Returns -2 with a message of its own for: bad arguments; a posterior from caller-provided K; the Matern kernel of
 * degree 1 (no second derivative); a posterior that holds a failed factorization; one sample with one query block
 * exceeding the budget (the message names N_pad, D, the block size and the bytes).                                   */
int gpc_predict_hess(gpc_post* post, const double* xstar, int M, int compute_var, double* fmu, double* fs2, double* dfmu,
                     double* dfs2, double* hmu, double* hs2);

/* ---- GP.nll_hess_batch: the Hessian of the negative log marginal likelihood with respect to the hyperparameters ------
 * Per sample of the posterior, at the posterior's own jitter multiplier `mult` (held fixed), with
 * Sigma = K + mult diag(sn2), Q = Sigma^-1, alpha = Q (y - m), Qm = Q - alpha alpha^T, hyperparameters ordered
 * [cov | noise | mean] as gpc_nll_batch's dnlz, P = cov_N + noise_N + mean_N.  Every covariance and noise
 * hyperparameter p is a plane d_p Sigma (lengthscale a: F o d_a^2 on the scaled inputs, isotropic: F o r2; log sf: 2 K;
 * RQ shape: Ka; noise n: mult diag(dsn2_n));  B_p = Q d_p Sigma, u_p = d_p Sigma alpha, w_p = Q u_p, v_k = Q d_k m:
 *   H[s][p][q] = -1/2 tr(B_p B_q) + u_p . w_q + 1/2 <Qm, d2_pq K>       planes p, q
 *   H[s][p][k] =  w_p . d_k m                                            plane p, mean k
 *   H[s][k][l] =  d_k m . v_l                                            mean k, l
 * d2_pq K on log scales as gpyreg_amd/csrc/nll_hess.h lists them (G = -2 dF/d(r2) of gpc_predict_hess; a pair at
 * r2 = 0 contributes nothing to a lengthscale term).  H EXCLUDES the two terms that need second derivatives of the
 * plugins: 1/2 mult sum_a diagq[a] d2 sn2_a (noise x noise) and -alpha . d2 m (mean x mean); the call returns
 * alpha (S x N) and diagq = diag(Qm) (S x N) for the caller to add them.  dnlz (S x P) is the gradient from the same
 * sums: gpc_nll_batch's to rounding, not to the bit.  H is symmetric to the bit (lower triangle computed, mirrored).
 *   dm   S x N x mean_N (may be NULL with mean_N = 0);  dsn2  S x dsn2_rows x noise_N, dsn2_rows = 1 (one noise value)
 *   or N (per point), WITHOUT the multiplier.
 * Device work per sample: Q formed once (W^T W / sl for L_chol samples, -L for the low-noise ones: one path after
 * that); per covariance hyperparameter one dense plane (u and the sums <Qm, .> fused in) and one plain fp64 GEMM
 * B_p = Q d_p K -- the log sf plane included, because the posterior does not keep sn2; the noise planes are column
 * scalings of Q; a streaming Gram pass for tr(B_p B_q); for the ARD families the contraction sum Qm G d_a^2 d_b^2; the
 * dot products of the downloaded vectors and the assembly on the host.  Every reduction's order is fixed by the shape:
 * a sample's results are the same bits whatever the batch, the other samples or the chunking (GPC_MEM_BUDGET_MB).
 * Scratch per sample: (cov_N + noise_N + 2) N_pad^2 doubles (Q, the B planes, one operand) and vectors.
 * gpc_last_timing: ms_total = the device sections, ms_factor = the planes and their products; options
 * "nll_hess_gram_us" / "nll_hess_contract_us": the Gram pass and the contraction of the last call.
 * Returns -2 with a message of its own for: bad arguments; a posterior from caller-provided K; an fp32 posterior (the
 * Hessian is fp64 only); the Matern kernel of degree 1 (no second radial factor G); more than 128 planes or more than
 * 860 lengthscale pairs; a failed factorization; one sample's scratch exceeding the budget (N_pad, planes, bytes). */
int gpc_nll_hess(gpc_post* post, const double* dm, int mean_N, const double* dsn2, int dsn2_rows, int noise_N, double* H,
                 double* dnlz, double* alpha, double* diagq);

/* ---- GP.cv_nll_batch: the leave-one-out cross-validation objective's gradient with respect to the hyperparameters ----
 * Per sample of the posterior, at the posterior's own jitter multiplier `mult` (held fixed), with
 * Sigma = K + mult diag(sn2), Q = Sigma^-1, alpha = Q (y - m), q_i = Q_ii: leaving point i out predicts y_i with mean
 * y_i - alpha_i / q_i and variance 1 / q_i.  With weights w_i >= 0 (NULL: ones; one vector of N for all samples):
 *   loss 0 ("lpd"):  L = -sum_i w_i (1/2 log q_i - alpha_i^2 / (2 q_i) - 1/2 log 2 pi)
 *                    c_i = w_i (1 + alpha_i^2 / q_i) / (2 q_i)         b_i = w_i alpha_i / q_i
 *   loss 1 ("mse"):  L =  sum_i w_i (alpha_i / q_i)^2
 *                    c_i = 2 w_i alpha_i^2 / q_i^3                     b_i = 2 w_i alpha_i / q_i^2
 *   beta = Q b,   G = Q diag(c) Q - 1/2 (beta alpha^T + alpha beta^T)   (symmetric)
 *   dL / d theta_p = <d_p K, G>   covariance hyperparameter p (planes F o d_a^2 | F o r2 | 2 K | Ka as gpc_nll_hess; a
 *                                 pair at r2 = 0 contributes nothing to a lengthscale term)
 *                  = mult sum_i G_ii d_n sn2_i  (noise n)      = -beta . d_k m  (mean k)
 * The call returns what needs the device: gsum (S x cov_N) = <d_p K, G>, diagG (S x N) = diag(G), beta, alpha, q and
 * c (S x N each).  The value L and the noise and mean columns are O(N P) and the caller's.
 * Device work per sample: Q formed once (W^T W / sl for L_chol samples, -L for the low-noise ones: one path after
 * that); c, b per point and beta = Q b; the column scaling Q diag(c); ONE plain fp64 GEMM over the lower tiles,
 * M = (Q diag(c)) Q; one contraction pass over the lower 64 x 64 tiles, the marginal likelihood's gradient pass with the
 * weight G in place of Q - alpha alpha^T.  No plane d_p K is formed: the cost does not depend on cov_N.  No atomics: a
 * sample's results are the same bits whatever the batch, the other samples or the chunking (GPC_MEM_BUDGET_MB).
 * Scratch per sample: 3 N_pad^2 doubles (Q, Q diag(c), M) and vectors.
 * gpc_last_timing: ms_total = the device sections, ms_factor = everything up to and including the product; option
 * "cv_grad_trace_us": the contraction pass of the last call.
 * Returns -2 with a message of its own for: bad arguments (weights negative or not finite among them); a posterior from
 * caller-provided K; an fp32 posterior (fp64 only); the Matern kernel of degree 1 (F infinite on the diagonal); a failed
 * factorization; one sample's scratch exceeding the budget (N_pad, bytes).                                              */
int gpc_cv_grad(gpc_post* post, int loss, const double* weights, double* gsum, double* diagG, double* beta, double* alpha,
                double* q, double* c);

/* ---- GP.predict_hyp_grad: derivatives of the latent prediction with respect to the hyperparameters, per sample -------
 * Sigma = K + mult diag(sn2) at each sample's own jitter multiplier, held fixed; Q = Sigma^-1, alpha = Q (y - m); for
 * query j: k_j = k(X, x*_j), q_j = Q k_j, fmu_j = k_j . alpha, fs2_j = k** - k_j . q_j.  Hyperparameters ordered
 * [cov | noise | mean] on the scales gpc_nll_batch differentiates on, P = cov_N + noise_N + mean_N.  With the weight
 * vectors  w_p = Q (d_p K alpha) (lengthscale, RQ shape) | 2 alpha - 2 mult Q (sn2 o alpha) (log sf) |
 * mult Q (dsn2_n o alpha) (noise n) | Q d_k m (mean k)  and the cross planes d_p k_ij = F d_a^2 (isotropic: F r2) |
 * 2 k | Ka of gpc_nll_hess (a pair at r2 = 0 contributes nothing to a lengthscale term):
 *   dfmu[(j*P + p)*S + s] = sum_i d_p k_ij alpha_i - sum_i k_ij w_p,i        (first sum: covariance p only)
 *   dfs2[(j*P + p)*S + s] = -2 sum_i d_p k_ij q_ij + q_j^T (d_p K) q_j       lengthscale, RQ shape
 *                         = 2 fs2_j - 2 mult sum_i sn2_i q_ij^2              log sf
 *                         = mult sum_i dsn2_n,i q_ij^2                       noise n;      0 for a mean hyperparameter
 * fmu, fs2 are laid out as gpc_predict's (M x S, [j*S + s]).  Results are unclamped, without noise at x* and without
 * a mean function (the caller adds d_k m(x*_j) to the mean columns of dfmu).
 *   sn2   S x noise_rows,  dsn2  S x noise_rows x noise_N (may be NULL with noise_N = 0), both WITHOUT the multiplier;
 *   noise_rows = 1 (one noise value) or N (per point);  dm  S x N x mean_N (may be NULL with mean_N = 0).
 * Device work per sample: the panel Q k* for all queries of a super-block (two products with W for L_chol samples, one
 * with L otherwise); per lengthscale / shape plane the dense d_p K (u_p = d_p K alpha fused in), one plain fp64 GEMM
 * T = d_p K (Q k*) and a streaming column dot for q_j^T d_p K q_j (the first plane's pass also takes the weighted
 * column sums of squares); w_p by triangular matrix-vector products; one fused pass over (training point, query)
 * tiles for every other sum.  No atomics: a sample's results are the same bits whatever the batch, the other samples
 * or the chunking (GPC_MEM_BUDGET_MB).  The budget decides the samples per chunk and, when the panels of all queries
 * do not fit, the queries per super-block (a multiple of 128; the planes are rebuilt per super-block).
 * compute_var == 0: no product with W or L and no GEMM is launched; fs2, dfs2 may be NULL and are not written; fmu and
 * dfmu carry the same bits as with the variance; gpc_last_timing's ms_factor is 0.
 * gpc_last_timing: ms_total = the device sections, ms_factor = the products with W (or L) and the planes (build, GEMM,
 * column dots).
 * Returns -2 with a message of its own for: bad arguments; a posterior from caller-provided K; an fp32 posterior (fp64
 * only); the Matern kernel of degree 1 (F infinite on the diagonal); a failed factorization; one sample with one block
 * of 128 queries exceeding the budget (the message names N_pad, the planes, the block and the bytes).                 */
int gpc_predict_hyp_grad(gpc_post* post, const double* xstar, int M, int compute_var, const double* sn2, const double* dsn2,
                         int noise_rows, int noise_N, const double* dm, int mean_N, double* fmu, double* fs2, double* dfmu,
                         double* dfs2);

/* ---- GP.draw_functions: joint posterior draws, n_draws per sample (extends gaussian_process.py:2241-2329) ----
 * For every sample s of the posterior (global index s_offset + s), draw r < R and query point j < M:
 *   f[(j*R + r)*S + s] = fmu_js + (L_s z_{s,r})_j  (+ noise_sd[j*S + s] z'_{s,r,j})
 * with fmu as gpc_predict, C_s = K** - V^T V the covariance of gpc_predict_full, L_s the lower Cholesky factor
 * of C_s + tau_s I.  C_s is factored first without jitter; a sample that fails is retried alone in stable mode
 * with tau_s = t mean(diag C_s), t = 1e-12, 1e-11, ..., 1e-6, the first success kept; tau[s] receives the
 * absolute jitter (0 when none was needed).  If every level fails the call returns -3 and gpc_last_error
 * names the global sample index.  noise_sd (M x S, may be NULL) is the caller's sqrt(sn2* sn2_mult).  The
 * mean function is the caller's.  fp32 posteriors factor and multiply in fp32.  A sample's draws are the
 * same bits whatever the batch of samples, the chunking (GPC_MEM_BUDGET_MB) or R beyond r.  Returns -2
 * with a message when one sample's scratch (three M x M slabs of the factorization, Z and L Z) does not
 * fit the memory budget.
 * Random stream: Philox4x64-10 with key (seed, stream), stream 0 for z, 1 for z'.  The 64-bit word of row j
 * is lane j % 4 of the block at counter (j / 4 + 1, r, s_global, 0) -- the first block numpy's
 * Philox(key=[seed, stream], counter=[j / 4, r, s_global, 0]).random_raw(4) returns.  Rows (2t, 2t+1):
 *   u1 = ((w[2t] >> 11) + 1) 2^-53,  u2 = (w[2t+1] >> 11) 2^-53,
 *   z[2t] = sqrt(-2 ln u1) cos(2 pi u2),  z[2t+1] = sqrt(-2 ln u1) sin(2 pi u2)
 * (odd M: the last row's partner is computed and unused).  gpyreg_amd/_philox.py restates it.           */
int gpc_draw(gpc_post* post, const double* xstar, int M, int R, unsigned long long seed, int s_offset,
             const double* noise_sd, double* f, double* tau);
/* out[i] = z of row j0 + i, i < count, of (seed, stream, sample s, draw r), computed on the device (tests). */
int gpc_debug_normals(gpc_ctx* ctx, unsigned long long seed, int stream, int s, int r, int j0, int count,
                      double* out);

/* ---- GP.sample_paths: pathwise posterior samples (Matheron's rule with random Fourier features) ------------
 * A posterior FUNCTION per hyperparameter sample s and path r < R, to be evaluated -- with its gradient -- at any
 * points afterwards (Thompson sampling, max-value and entropy searches, Monte-Carlo acquisitions):
 *   f_{s,r}(x) = p_{s,r}(x) + k_s(x, X) v_{s,r}                                    (the mean function is the caller's)
 *   p_{s,r}(x) = sqrt(2 sf2_s / F) sum_{f<F} wt_s[f][r] cos(theta_s[f] . xs(x) + b_s[f])
 *   v_{s,r}    = (K_s + Sigma_s)^-1 (ym_s - p_{s,r}(X) - eps_{s,r}),   eps_{s,r}[i] = noise_sd[i*S + s] e_s[i][r]
 * xs = x mul / dv are the scaled inputs of the kernel family (as gpc_predict_grad).  On scaled inputs the spectral
 * draw is theta[f][l] = z[f][l] for GPC_K_SE / GPC_K_SE_ISO and z[f][l] / sqrt(c[f]), c[f] = sum_{q<d} g[f][q]^2, for
 * Matern of degree d (the multivariate Student-t with d degrees of freedom).  The update term is exact; only the
 * prior part is approximated, and F is the caller's choice.  Features are shared by the R paths of a sample.
 * Random stream: gpc_draw's Philox4x64-10 and Box-Muller, key (seed, stream), sample index s_offset + s:
 *   stream 2: z[f][l] = normal(r = l, j = f)     stream 3: g[f][q] = normal(r = q, j = f)
 *   stream 4: b[f] = 2 pi (word(r = 0, j = f) >> 11) 2^-53
 *   stream 5: wt[f][r] = normal(r, j = f)        stream 6: e[i][r] = normal(r, j = i)
 * (gpyreg_amd/_paths.py restates all of it), so path r of sample s does not depend on R, on the batch of samples, on
 * the chunking or on the sharding.
 *
 * gpc_paths_create: ym (S x N) = y - m_s(X), noise_sd (N x S) = sqrt(sn2_s[i] sn2_mult_s), both the caller's.
 * Generates theta, b and wt on the device, forms the N x R panel p(X) + eps with the evaluation kernel (the N x F
 * feature matrix is never stored) and solves for v with the resident factors as gpc_predict_grad forms Q: W^T (W r) / sl
 * for L_chol samples, -(A r) otherwise.  The products are the skinny kernel of gpc_post_append_block, 16 right-hand
 * sides per pass whatever R is -- so v of path r carries the same bits for any R; the test option
 * "paths_solve_engine" = 2 runs them as MFMA GEMM launches on panels padded to 128 columns instead (get-only
 * "paths_solve_engine_ran" tells which ran).  v, the features and the evaluation are fp64 whatever the posterior's
 * storage type; fp32 posteriors only change what the solve reads.  The handle owns copies of everything evaluation
 * needs (scaled training inputs, per-sample scalars and scaling, v, theta, b, wt): it describes the posterior at
 * creation time and stays valid after the posterior is updated, appended to or freed (not after gpc_destroy).
 * Scratch (three fp64 N_pad x R_pad16 panels per sample, three N_pad x R_pad128 panels in the storage type more for
 * the MFMA engine) is budgeted like gpc_predict_cov's (GPC_MEM_BUDGET_MB) and chunked over the samples.  Returns -2
 * with a message for R < 1 or F < 1, a posterior from caller-provided K, a sample whose factorization failed,
 * GPC_K_RQ, null arguments, a context whose data is no longer the posterior's, or one sample's scratch exceeding
 * the budget.  gpc_last_timing: the device section, and the solve's products.
 *
 * gpc_paths_eval: xstar M x D.  f[(j*R + r)*S + s]; df (may be NULL) [((j*D + l)*R + r)*S + s] = d f / d x*_jl:
 *   d/dx*_jl k(x*_j, X_i) = -c_l F_ij (xs*_jl - xs_il)   (F, c_l of gpc_predict_grad; a pair at distance 0 gives 0)
 *   d/dx*_jl p            = -c_l sqrt(2 sf2 / F) sum_f wt[f][r] theta[f][l] sin(theta[f] . xs* + b[f])
 * One fused kernel: per 64-row tile of query points it forms 64 x 64 operand tiles in LDS -- cross covariances by the
 * compile-time pair functor of gpc_predict, then the features -- and multiplies each straight into the v (wt) panel
 * with v_mfma_f64_16x16x4_f64; neither K* nor the feature matrix is written.  Sums run over the tiles in ascending
 * order without atomics: a value depends on (x, s, r) only -- not on M, the row's place, the other rows, or on
 * whether df was asked for.  The test option "paths_engine" = 2 runs the unfused composition instead (operand
 * matrices written to memory, then the library GEMM; equal to rounding), get-only "paths_engine_ran" tells which
 * ran.  The results and the scratch (the scaled query points; for the unfused engine an operand matrix and padded
 * panels per sample) are budgeted and chunked as above; -2 with a message when they do not fit.
 * gpc_last_timing: the device section with the transfers, and the kernels alone.
 * gpc_debug_paths_fetch (tests): theta (F x D), b (F), wt (F x R), v (N x R) of sample s; any may be NULL. */
typedef struct gpc_paths gpc_paths;
int gpc_paths_create(gpc_post* post, int R, int F, unsigned long long seed, int s_offset, const double* ym,
                     const double* noise_sd, gpc_paths** out);
int gpc_paths_eval(gpc_paths* p, const double* xstar, int M, double* f, double* df);
int gpc_paths_free(gpc_paths* p);
int gpc_debug_paths_fetch(gpc_paths* p, int s, double* theta, double* b, double* wt, double* v);

/* ---- rank-one append of ONE training point to resident posteriors (GP.update fast path,
 *      gaussian_process.py:750-844; scalar noise) ------------------------------------------------
 * Call gpc_set_data with the extended X (N+1 rows; the new point last) and y first.
 *   m_star[s]   mean function of sample s at the new point
 *   sn2_star[s] noise variance of sample s at the new point (noise.compute(hyp, x_new, y_new, 0))
 * High-noise samples (L_chol): l = W Ks, sqrt_arg = sn2_eff^2 + kss sn2_eff - l.l (:784-788); the
 * factor, its inverse and alpha get their new last row in O(N^2) (:800-817).  Low-noise samples
 * (Posterior.L = -inv): the rank-one update of -inv of :819-827.  The storage of EVERY sample grows
 * to N+1.  ok[s] = 1 if sample s was appended; ok[s] = 0 (sqrt_arg <= 0, a failed factorization,
 * or a noise value that is not the fitted scalar) leaves sample s stale: the caller recomputes
 * exactly those samples with gpc_post_recompute -- the reference's per-posterior fallback
 * (full_updates, :789-798 and :866-869).                                                        */
int gpc_post_append(gpc_post* post, const double* m_star, const double* sn2_star, double y_new, int* ok);
/* Recompute samples idx[0..cnt) of a resident posterior set in place from the context's current
 * data (__core_computation(hyp, 0, 0) for those samples, :866-869).  Arrays as gpc_posterior_batch,
 * one row per listed sample.                                                                      */
int gpc_post_recompute(gpc_post* post, int cnt, const int* idx, const double* hyp_cov, const double* m,
                       const double* sn2, int sn2_is_vector, double* sn2_mult, int* L_chol, int* info);
/* The same two steps for a posterior set built from caller-provided covariances (gpc_posterior_batch_K): the
 * reference's rank-one path calls self.covariance.compute whatever the object is (gaussian_process.py:771-772),
 * so the caller hands over what that call returns.  Ks: S x n (row s = k_s(X_old, x_new), the n = N - 1 points the
 * posterior was built on; gpc_set_data has been called with the extended X, y), kss: S (k_s(x_new, x_new)).
 * gpc_post_recompute_K: K = cnt x N x N matrices of the listed samples on the extended data.              */
int gpc_post_append_K(gpc_post* post, const double* Ks, const double* kss, const double* m_star,
                      const double* sn2_star, double y_new, int* ok);
int gpc_post_recompute_K(gpc_post* post, int cnt, const int* idx, const double* K, const double* m,
                         const double* sn2, int sn2_is_vector, double* sn2_mult, int* L_chol, int* info);

/* ---- block append of k >= 1 training points to resident posteriors in O(N^2 k) (GP.update(block_append=True);
 *      scalar noise).  The reference has no such path (it recomputes); the algebra is the rank-one path's with a
 *      k x k block where that has a scalar.
 * Call gpc_set_data with the extended X (N+k rows; the new points last, in order) and y first.
 *   m_star[s*k + j]  mean function of sample s at new point j
 *   sn2_star[s]      noise variance of sample s at the new points (scalar noise: one value)
 *   y_new[j]         the new observations
 * With n old points, B = K(X_old, X_new) (n x k), Knn = K(X_new, X_new), e = y_new - m_star - B^T alpha, sl the
 * fitted noise of the sample (sn2_eff = sn2_star * sn2_mult must equal it to 1e-12 relative):
 *   high-noise samples (L_chol; A = Lo, W = Lo^-1):  V = W B,  S = Knn / sl + I - V^T V / sl^2,  L22 = chol(S),
 *     W22 = L22^-1;  new rows Lo[n:, :n] = V^T / sl, Lo[n:, n:] = L22,  W[n:, :n] = -W22 (V^T W) / sl, W[n:, n:] = W22;
 *     alpha = [alpha - W21^T u2 ... ] with u2 = W22 e:  alpha[:n] += W21^T u2 / sl,  alpha[n:] = W22^T u2 / sl.
 *   low-noise samples (Posterior.L = -(K + Sigma)^-1, full symmetric):  G = inv B,  S = Knn + sn2_eff I - B^T G,
 *     Si = S^-1 through its Cholesky factor;  inv <- [[inv + G Si G^T, -G Si], [-(G Si)^T, Si]];  a2 = Si e,
 *     alpha = [alpha - G a2 ; a2].
 * The two products with W (and the one with the low-noise inverse) have two engines: for k <= 16 a skinny kernel
 * that streams the N x N matrix once per product with the 16 right-hand sides in LDS, for larger k launches of the
 * MFMA GEMM on panels padded to 128 columns (block_append.h: BA_GEMM_MIN_K, with the measurement; the test option
 * "block_engine" = 1 / 2 forces one of them; the get-only option "block_engine_ran" tells which one the last call ran).  The bits of a sample depend on the engine, not on the batch.
 * S is factorized by the library's blocked factorization WITHOUT jitter, for all samples at once, and every sample
 * is decided on the device: ok comes back in one download.  The storage of EVERY sample grows to N+k (by as many
 * 128-tiles as that needs).  ok[s] = 1 if sample s was appended; ok[s] = 0 (S not positive definite, a sample whose
 * own factorization had failed, a noise value that is not the fitted scalar, or a sample named by the test option
 * "append_fail_mask") leaves sample s exactly as it was apart from the growth: the caller recomputes exactly those
 * samples with gpc_post_recompute.  Scratch (four fp64 N_pad x k panels per sample, three more in the storage type
 * for the MFMA engine) lives in the context's consumer scratch block, is budgeted like gpc_predict_cov's
 * (GPC_MEM_BUDGET_MB) and chunked over the samples.  gpc_last_timing: the device section after the growth, and
 * the products with W.
 * Returns -2 with a message for k < 1, N + k > gpc_max_n, data that was not extended first, a posterior of the
 * other origin (device kernel / caller-provided K), null arguments, or one sample's scratch exceeding the budget.
 * The get-only options "block_appended" / "block_stale" count the samples that ended either way (ok = 1 / ok = 0)
 * over the life of the context.                                                                          */
int gpc_post_append_block(gpc_post* post, int k, const double* m_star, const double* sn2_star,
                          const double* y_new, int* ok);
/* The same for a posterior set built from caller-provided covariances (gpc_posterior_batch_K):
 * Ks: S x n x k (Ks[s] = k_s(X_old, X_new)), Kss: S x k x k (k_s(X_new, X_new)); the stale samples are
 * recomputed with gpc_post_recompute_K.                                                                  */
int gpc_post_append_block_K(gpc_post* post, int k, const double* Ks, const double* Kss, const double* m_star,
                            const double* sn2_star, const double* y_new, int* ok);

/* ---- removal of k >= 1 training points from resident posteriors in O(N^2 k) (GP.remove_points; scalar noise).
 *      The inverse of the block append; the reference has no such path (it recomputes).  No covariance is evaluated:
 *      posteriors of either origin (device kernel, caller-provided K) take the same call.
 * Call gpc_set_data with the reduced X, y (N-k rows) first.
 *   idx[j]        the removed rows, numbered in the posterior's N rows: sorted, distinct, in [0, N)
 *   ym[s*n + i]   y_R - m_s(X_R), the centred observations of the n = N-k kept rows, per sample
 * With I = idx, R = the kept rows in order:
 *   high-noise samples (L_chol; A = Lo, W = Lo^-1):  Lr = Lo[R, R], Wr = W[R, R], V = Lo[R, I], C = W[I, R];  the new
 *     factor has L' L'^T = Lr Lr^T + V V^T (a rank-k UPDATE: always positive definite).  For every 64-column panel
 *     [a, b) from the one that holds the first removed row on, an orthogonal Theta of order 64 + k with
 *     [Lr[a:b, a:b] | V[a:b, :]] Theta = [D' | 0] is formed by Householder reflections in fp64 (positive diagonal) and
 *     applied with fp64 MFMA:  [Lr[b:, a:b] | V[b:, :]] <- [...] Theta,  [Wr[a:b, :b] ; C] <- Theta^T [...].  Rows
 *     above the first removed one keep their bits; removing the LAST rows only truncates.  alpha = W'^T (W' ym) / sl
 *     from the new factor, never from the old alpha: repeated removals do not drift away from the factor.
 *   low-noise samples (A = -(K + Sigma)^-1 = -Q, full symmetric):  Q_II = Lq Lq^T through the library's blocked
 *     factorization WITHOUT jitter, H = A[R, I] Lq^-T:  A' = A[R, R] + H H^T,  alpha' = alpha_R + A[R, I] Q_II^-1 alpha_I.
 * Up to 64 rows leave in one sweep; a larger k goes in consecutive sweeps of at most 64.  The storage of EVERY sample is
 * compacted to the padded size of N-k (it shrinks by whole 128-tiles when that allows: the layout of a fresh
 * posterior), the old buffers go to the context's pool.  ok[s] = 1 if sample s was shrunk; ok[s] = 0 (a low-noise
 * sample whose Q_II is not positive definite, a sample whose own factorization had failed, or one named by the test
 * option "remove_fail_mask") leaves a stale sample in the compacted storage: the caller recomputes exactly those with
 * gpc_post_recompute[_K].  Scratch (three fp64 N_pad x k panels, Theta and the k x k factorization per sample) lives
 * in the context's consumer scratch block, is budgeted like gpc_post_append_block's (GPC_MEM_BUDGET_MB) and chunked
 * over the samples; the bits of a sample depend neither on the batch nor on the chunk.  No host synchronisation
 * between the panels of a sweep.  gpc_last_timing: the device section, and the panel loops alone (summed over chunks and sweeps).
 * Returns -2 with a message, the posterior untouched, for k < 1, k >= N, indices that are unsorted, repeated or out
 * of range, data that was not reduced first, null arguments, or one sample's scratch exceeding the budget.
 * The get-only options "removed" / "remove_stale" count the samples that ended either way over the life of the
 * context.  The get-only options "remove_max_panels" (the longest sweep, in panels summed over the sweeps) and
 * "remove_min_rows" (the number of kept rows that has to be exceeded) bound the shapes for which the call was measured
 * to beat the full recompute (remove.h: RM_SWEEP_MAX_PANELS, RM_MIN_KEPT_ROWS, with the measurement): the entry point
 * itself does whatever it is given, GP.remove_points recomputes outside the limits; the test option "remove_force" = 1
 * makes both options report no limit.                                                                     */
int gpc_post_remove(gpc_post* post, int k, const int* idx, const double* ym, int* ok);

/* ---- GP.predict_full (gaussian_process.py:1603-1650) -------------------------------------
 * fmu[j*S + s] = Ks^T alpha;  cov[s] (M x M, row-major) = K** - V^T V  or  K** + Ks^T (L Ks)
 * (the caller symmetrises and adds noise, :1647-1659).                                    */
int gpc_predict_full(gpc_post* post, const double* xstar, int M, double* fmu, double* cov);

/* ---- GP.predict_cov / GP.lookahead_variance: posterior covariance between TWO query sets ------------
 * xa: Ma x D, xb: Mb x D.  With Ka = K_s(X, xa), Kb = K_s(X, xb) and, for L_chol samples, Va = W Ka,
 * Vb = W Kb (sl the sample's noise scaling, as in gpc_predict):
 *   cov[s] (Ma x Mb, row-major; may be NULL) = K_s(xa, xb) - Va^T Vb / sl      (L_chol)
 *                                            = K_s(xa, xb) + Ka^T (L Kb)       (L = -inv)
 *   wsq[j*S + s]  = sum_i w_i(s) cov_s[i][j]^2   (may be NULL; needs w: Ma doubles shared by the samples,
 *                   or Ma x S as w[i*S + s] when w_per_sample)
 *   fs2b[j*S + s] = gpc_predict's fs2 of xb (may be NULL): Vb is at hand, no second N^2 Mb product runs
 * At least one of cov / wsq must be given.  No noise term and no symmetrisation: the block is not square.
 * The library adds nothing else: the denominators of the look-ahead, the clamp and the mixture over
 * samples are the caller's.  Without cov, and from 64 128-tiles of the Ma x Mb block on, the block is
 * never written: the product's epilogue forms the weighted sums per tile row (fp64, also for fp32
 * posteriors), which are added in ascending order; gpc_get_option(ctx, "cov_fused") counts those calls.
 * The form depends on the shape only, so a sample's results are the same bits whatever the batch of
 * samples or the chunking (GPC_MEM_BUDGET_MB).  Returns -2 with a message that names the sizes when one
 * sample's scratch (2 N_pad (Ma_pad + Mb_pad) + Ma_pad Mb_pad elements) does not fit the memory budget,
 * on a posterior from caller-provided K, on one that holds a failed factorization and on bad arguments. */
int gpc_predict_cov(gpc_post* post, const double* xa, int Ma, const double* xb, int Mb, const double* w,
                    int w_per_sample, double* fs2b, double* cov, double* wsq);

/* ---- GP.lookahead_batch: q greedy look-ahead steps without the host ----------------------------------
 * xr: Mr x D reference points, xc: Mc x D candidates, w as gpc_predict_cov's (Mr doubles, or Mr x S as
 * w[r*S + s] when w_per_sample), noise[c*S + s] the predictive noise of candidate c under sample s (the
 * noise function's value times the sample's multiplier), 1 <= q <= Mc.  Per sample C^0 is gpc_predict_cov's
 * covariance of [xr; xc] against xc and v^0 gpc_predict's unclamped variance of xc; for t = 0 .. q-1
 *   den_s(c)  = max(v_s(c), 0) + noise[c*S + s]
 *   gain_s(c) = sum_r w_rs C_s(r, c)^2 / den_s(c)          (0 where den_s(c) <= 0)
 *   c_t       = argmax_c (1/S) sum_s gain_s(c) over the candidates not yet chosen, the lowest index on a tie
 *               (samples added in ascending order; a NaN score counts as -inf)
 *   l_s(a)    = C_s(a, c_t) / sqrt(den_s(c_t)) for every row a (0 where den_s(c_t) <= 0),
 *   C_s(a, b) -= l_s(a) l_s(Mr + b),   v_s(b) -= l_s(Mr + b)^2
 * idx[t] = c_t, gain[t*S + s] = gain_s(c_t) at step t.  The posterior is not modified.  C^0 is formed by
 * gpc_predict_cov's stored form, chunked over the samples under the same budget, and kept on the device in
 * fp64 (also for fp32 posteriors): the step loop is fp64.  Its reference rows are updated in place, one
 * read and one write per step; the Mc x Mc candidate block is never rewritten -- its column c_t is formed
 * from C^0 and the stored l vectors.  All q steps are enqueued without a host synchronisation; idx and gain
 * come back in one transfer.  Fixed summation orders and no atomics: the same bits on every call, whatever
 * the chunking of the formation.  Returns -2 with a message that names the sizes when the resident state
 * (S (Mr + Mc) Mc_pad doubles and q l vectors per sample; it cannot be chunked over the samples) does not
 * fit the memory budget (GPC_MEM_BUDGET_MB), on a posterior from caller-provided K, on one that holds a
 * failed factorization and on bad arguments.  gpc_get_option "lookahead_batch_loop_us": the device time
 * of the step loop. */
int gpc_lookahead_batch(gpc_post* post, const double* xr, int Mr, const double* xc, int Mc, const double* w,
                        int w_per_sample, const double* noise, int q, int* idx, double* gain);

/* ---- GP.quad: Bayesian quadrature products (gaussian_process.py:1908-1966), SE kernels ----
 * mu, sigma: M x D (means and standard deviations of the Gaussian measures).  With z the
 * kernel mean vector of measure j under sample s:
 *   zalpha[j*S + s] = z . alpha                      (the caller adds the mean-function terms)
 *   zKz[j*S + s]    = z (K + sn2_eff I)^-1 z^T       (only if compute_var)
 * Fails with a message on a gradient-observation posterior, on one that holds a failed
 * factorization, on a kernel that is not squared exponential and on bad arguments.          */
int gpc_quad(gpc_post* post, const double* mu, const double* sigma, int M, int compute_var,
             double* zalpha, double* zKz);

/* ---- GP.quad_grad: gradients of the quadrature products with respect to the measures ---------------
 * zalpha, zKz as gpc_quad (zKz already divided by sl or negated); for every sample s, measure j and
 * dimension l, with tau_jl^2 = sigma_jl^2 + ell_l^2, d_ijl = mu_jl - X_il and q = (K + Sigma)^-1 z under
 * the posterior's own scaling (W^T W z / sl for L_chol samples, -(L z) otherwise):
 *   dza_dmu[(j*D + l)*S + s]     = d zalpha_js / d mu_jl    = -sum_i alpha_i z_ij d_ijl / tau_jl^2
 *   dza_dsigma[(j*D + l)*S + s]  = d zalpha_js / d sigma_jl =  sum_i alpha_i z_ij sigma_jl
 *                                                               (d_ijl^2 / tau_jl^2 - 1) / tau_jl^2
 *   dzkz_dmu, dzkz_dsigma        = d zKz_js / d mu_jl, d sigma_jl: 2 x the same sums with q_ij for alpha_i
 *                                  (only if compute_var; K + Sigma is symmetric)
 * sigma is the standard deviation, as in gpc_quad.  Without compute_var no N^2 M product runs; with it
 * V = W z is written and Q = W^T V is one more product of the same size.  The differences d_ijl are
 * formed per pair, never expanded into moments.  The mean function's terms, the self-term nf_kk of the
 * variance, the clamp and the mixture over samples are the caller's.  Fails with a message where
 * gpc_quad fails, and on a posterior that holds a failed factorization.                                */
int gpc_quad_grad(gpc_post* post, const double* mu, const double* sigma, int M, int compute_var,
                  double* zalpha, double* zKz, double* dza_dmu, double* dza_dsigma, double* dzkz_dmu,
                  double* dzkz_dsigma);

/* ---- GP.quad_cov: covariance between the integrals against the single measures --------------------
 * With Z_s the N x M matrix of kernel means of sample s and
 *   Gamma_jk = sf2 prod_l ell_l / sqrt(t_jkl) exp(-1/2 sum_l (mu_jl - mu_kl)^2 / t_jkl),
 *   t_jkl = ell_l^2 + sigma_jl^2 + sigma_kl^2                      (Gamma_jj is the self-term of gpc_quad's variance)
 *   zalpha[j*S + s] = z_j . alpha                                  (as gpc_quad)
 *   cov[s] (M x M, row-major) = Gamma_s - Z^T (K + Sigma)^-1 Z     under the posterior's own scaling, as gpc_quad
 *                               scales zKz: Gamma - V^T V / sl (L_chol, V = W Z) or Gamma + Z^T (L Z)
 * Gamma is formed on the device where gpc_predict_full puts K**; the products, the chunking over samples and the
 * memory budget are gpc_predict_full's.  No symmetrisation and no clamp: both are the caller's.  Fails with a
 * message where gpc_quad_grad fails.                                                                   */
int gpc_quad_cov(gpc_post* post, const double* mu, const double* sigma, int M, double* zalpha, double* cov);

/* ---- GP.quad_mixture: quadrature against the mixture sum_j w_j N(mu_j, diag(sigma_j^2)) -------------
 * w: M finite reals, not normalised.  With zbar = Z w and q = (K + Sigma)^-1 zbar under the posterior's own
 * scaling (W^T W zbar / sl for L_chol samples, -(L zbar) otherwise) the library returns the device's share:
 *   zalpha[j*S + s] = z_j . alpha                                        (always)
 *   zbkzb[s]        = zbar . q                                           (compute_var)
 *   gw[j*S + s]     = (Gamma_s w)_j                                      (compute_var)
 *   zq[j*S + s]     = z_j . q                                            (compute_var)
 *   dza_dmu, dza_dsigma [(j*D + l)*S + s]   as gpc_quad_grad             (compute_grad)
 *   dzq_dmu, dzq_dsigma [(j*D + l)*S + s] = sum_i q_i dz_ij / dmu_jl, dsigma_jl           (both flags)
 *   dgw_dmu, dgw_dsigma [(j*D + l)*S + s] = sum_k w_k d1 Gamma_jk / dmu_jl, dsigma_jl     (both flags; d1: the
 *                                           derivative in the first slot only)
 * so that the mixture mean is sum_j w_j (zalpha_j + nu_j), the variance w . gw - zbkzb, dV/dw_j = 2 gw_j - 2 zq_j
 * and dV/dmu_jl = 2 w_j (dgw_dmu_jl - dzq_dmu_jl); the factors w_j and 2, the mean function's terms, the clamp and the
 * mixture over samples are the caller's.  Outputs a flag does not ask for may be NULL.  z is recomputed per pair in
 * fp64 in two passes over 64 x 64 tiles and never stored; the solve is one pair of triangular matrix-vector products
 * per sample; no MFMA GEMM launch runs (gpc_get_option "quad_mix_gemms" counts any that do).  Every order of
 * summation is fixed by the shape: a sample's bits do not depend on the batch or on the chunking
 * (GPC_MEM_BUDGET_MB).  fp32 posteriors form z, zbar, Gamma and every reduction in fp64; only the products with W
 * (or L) read the storage type.  Returns -2 with a message that names the sizes when one sample's scratch does not
 * fit the memory budget; fails with a message where gpc_quad_grad fails, and on a posterior from caller-provided K. */
int gpc_quad_mix(gpc_post* post, const double* mu, const double* sigma, const double* w, int M, int compute_var,
                 int compute_grad, double* zalpha, double* zbkzb, double* gw, double* zq, double* dza_dmu,
                 double* dza_dsigma, double* dzq_dmu, double* dzq_dsigma, double* dgw_dmu, double* dgw_dsigma);

/* ---- cross-validation ------------------------------------------------------------
 * Leave-fold-out predictive distributions of the training points themselves, from the resident posterior alone, the
 * hyperparameters held fixed (Rasmussen & Williams 5.4.2): with P = (K + Sigma)^-1 the held-out set I given the rest
 * has covariance C = (P_II)^-1 and mean y_I - C alpha_I.  No covariance or mean function is evaluated and no
 * gpc_set_data state is read: the call serves posteriors from gpc_posterior_batch, from caller-provided K, and ones
 * grown by gpc_post_append[_block] alike.
 * fold_ptr holds F + 1 offsets into fold_idx; fold f is fold_idx[fold_ptr[f] .. fold_ptr[f+1]): indices in [0, N),
 * strictly ascending, folds pairwise disjoint, none empty, at most N - 1 long; they need not cover all points.
 * F == 0 with NULL arrays: every point its own fold (leave-one-out), one streaming pass over W; explicit folds that
 * are all singletons take that same pass and give the same bits.
 * Per sample s and fold f (sc = the fitted noise of an L_chol sample, 1 otherwise):
 *   dmu[i*S + s]    = (C alpha_I)_j for i = I[j]          (the caller forms mu_i = y_i - dmu)
 *   s2[i*S + s]     = C_jj, the variance of the noisy observation
 *   quad[f*S + s]   = alpha_I^T C alpha_I,   logdet[f*S + s] = log det C
 *   info[f*S + s]   = 0, or nonzero when the fold's operand (W[:, I]^T W[:, I], or -A[I, I]) was not positive definite
 *                     in floating point: its outputs are NaN then, no jitter is applied.
 * With F == 0 quad, logdet and info are N x S, one per point.  Points in no fold get NaN in dmu and s2.  quad, logdet and
 * info may be NULL.  Everything after the load of W (or A) is fp64, for fp32 posteriors too; the operands of all folds
 * and samples of a chunk are factored in one batched fp64 factorization padded to k_max rounded up to 128.  The
 * numbers of (sample, fold) depend on the sample, the fold and the engine only: not on F, the other folds, the batch
 * or the chunking (GPC_MEM_BUDGET_MB).  Test option "cv_engine": 1 = fused gather + MFMA Gram (default), 2 = gathered
 * panels + the library GEMM (equal to rounding); get-only "cv_engine_ran" tells which one the last call ran (0: the
 * leave-one-out pass).  gpc_last_timing: ms_total = the device section, ms_factor = the Gram or diagonal pass.
 * Returns -2 with a message of its own for an index out of range, an unsorted fold, overlapping folds, an empty fold,
 * a fold of all N points, a failed posterior, and (naming N_pad, F and k_max) when one sample's scratch does not fit
 * the memory budget; -3 when a leaf of the factorization timed out. */
int gpc_cv(gpc_post* post, int F, const int* fold_ptr, const int* fold_idx, double* dmu, double* s2, double* quad,
           double* logdet, int* info);

/* ---- instrumentation -------------------------------------------------------------
 * GPU time (ms, hipEvent on the library's stream) of the last gpc_nll_batch /
 * gpc_posterior_batch: whole device section, and the part spent in the MFMA GEMM
 * launches + leaf factorizations (the N^3 work).  Calls below N_pad = 2048 record
 * these events only under gpc_set_option(ctx, "small_timing", 1): both are 0 otherwise. */
int gpc_last_timing(gpc_ctx* ctx, double* ms_total, double* ms_factor);
/* (after gpc_predict / gpc_predict_full / gpc_quad: ms_total = device time of the call, ms_factor = the
 * duration of its N^2 M product V = W Ks, the GEMM launch of gaussian_process.py:1752-1760; after
 * gpc_quad_grad: that of its products V = W z and Q = W^T V, ~0 without compute_var; after
 * gpc_predict_cov: ms_factor = its triangular products and the cross product, with the reduction;
 * after gpc_quad_mix: ms_factor = its solve, the triangular matrix-vector products, 0 without compute_var;
 * after gpc_cv: ms_factor = its Gram (or gather) launches, or the leave-one-out pass) */
/* The dominant single kernel of the last gpc_nll_batch with gradient: the W^T W ("lauum")
 * launch of gemm_kernel<T, true, true, ...>.  ms = its duration (hipEvents on the stream it
 * was launched on; the slowest sample group), flops = its algorithmic flops
 * (samples in that launch x N^3/3).                                                     */
int gpc_last_lauum_timing(gpc_ctx* ctx, double* ms, double* flops);
/* Tuning switches (also settable through the environment at gpc_create: GPC_GROUPS,
 * GPC_SMALL_BLOCKS, GPC_DEFER_MIN, GPC_DEFER_RESERVE): "groups" = sample groups on separate HIP
 * streams (1..8), "small_blocks" = launch size below which 64x64 tiles are used, "defer_min" = node
 * size from which the inverse product U = T21 W11 runs on a side stream (0 off, -1 auto),
 * "defer_reserve" = CUs per XCD that launch keeps empty (2 | 4 | 8 | 12), "tri_skip" (default 1) = the GEMM launches
 * of the evaluation pipeline name their triangular operands and the fp64 128-tile kernel skips the MFMAs of the zero
 * halves (gemm.h: GemmArgs::tri; 0: every launch is the plain one -- the same bits either way).  Test hooks:
 * "start_mult_log10" = k starts the jitter escalation of every factorization at 10^k instead of 1
 * (gaussian_process.py:2402), "append_fail_mask" = bit s declares the rank-one append of sample s
 * unstable (:789-798).  "experiments" (get only): 1 when the loaded library is the experiments build.
 * Round 6, calls below N_pad = 2048 (single evaluations of the sampler and the optimiser on small training sets:
 * slice_sample.py:442, gaussian_process.py:1540): "small_poll" (default 1) = the call returns when a word that its last
 * launch writes into coherent host memory shows up, instead of waiting for the stream (bounded: after 0.15 - 2 ms it waits
 * for the stream after all); "small_timing" (default 0) = such calls record their timing events, so that gpc_last_timing
 * reports their device section (it reports 0 for them otherwise; from N_pad = 2048 on the events are always recorded).
 * "small_polled" / "small_synced" (get only): how many calls ended either way.
 * "last_chunk" (get only): how many samples per chunk the last posterior consumer (predictions, gradients, Hessians,
 * cross-validation, quadrature, paths, appends) planned for its scratch; S when the call ran whole, 0 when it refused.
 * "cov_fused" (get only): how many gpc_predict_cov calls formed their reduction in the product's epilogue.
 * "lookahead_batch_loop_us" (get only): device microseconds of the step loop of the last gpc_lookahead_batch.
 * "quad_mix_gemms" (get only): MFMA GEMM launches issued inside gpc_quad_mix over the life of the context (0 by design).
 * "paths_engine" / "paths_solve_engine" (test hooks) and "paths_engine_ran" / "paths_solve_engine_ran" (get only): see
 * gpc_paths_create / gpc_paths_eval.  "cv_engine" (test hook) and "cv_engine_ran" (get only): see gpc_cv. */
int gpc_set_option(gpc_ctx* ctx, const char* name, int value);
/* Current value of a tuning switch (so that a caller that changes one for a measurement can put it back). */
int gpc_get_option(gpc_ctx* ctx, const char* name, int* value);
/* fp64/fp32 MFMA issue-rate microbenchmark: achieved TFLOP/s of a register-resident
 * v_mfma_{f64,f32}_16x16x4 loop on all CUs (2 waves per SIMD), the shader cycles one
 * SIMD spends per MFMA, and the clock (GHz) the chip held while running it.  Used to
 * calibrate the roofline against what the silicon sustains rather than the datasheet. */
int gpc_mfma_peak(gpc_ctx* ctx, int dtype, double* tflops, double* cycles_per_mfma,
                  double* clock_ghz);

/* ---- test hooks (exercise one kernel through the ABI; used by tests/ only) --------
 * C[M x N] = beta*C + alpha*op(A)op(B) with the library's tiled MFMA GEMM.
 * a_kmajor: A stored K x M (else M x K); b_kmajor: B stored K x N (else N x K).
 * M, N, K multiples of 128.  klo/khi/lower_only: per-tile k-range modes (see
 * gpyreg_amd/csrc/gemm.h); lower_only bit 0 = lower tiles only, 0x100 / 0x200 force the 64- / 128-tile kernel variant
 * (0x400, experiments build only: the 128 x 64 tile).                              */
int gpc_debug_gemm(gpc_ctx* ctx, int dtype, int M, int N, int K, int a_kmajor,
                   int b_kmajor, double alpha, int beta, int klo, int khi,
                   int lower_only, const double* A, const double* B, double* C);
/* In-LDS leaf: A (128 x 128 SPD, lower used) -> L (lower) and W = L^-1; logdet, info */
int gpc_debug_leaf(gpc_ctx* ctx, int dtype, const double* A, double* L, double* W,
                   double* logdet, int* info);
/* Blocked factorization of an n x n SPD matrix (any n): L, W = L^-1, Ainv (lower).   */
int gpc_debug_factor(gpc_ctx* ctx, int dtype, int n, const double* A, double* L,
                     double* W, double* Ainv, double* logdet, int* info);
/* The launch plan of gpyreg_amd/csrc/plan.h as the product runs it: `batch` samples of npad x npad (a multiple of 128,
 * at most 2048, or 2304; batch 1 .. 16) in one call, on buffers of the hook's own.  A, W, T: [batch][npad][npad], uploaded WHOLE
 * and verbatim (a plain cast for fp32) -- identity padding, the part above the diagonal and whatever the caller poisons
 * W and the scratch T with included -- and downloaded whole after the factorization, so that a read of something no
 * launch wrote and a write outside the plan's contract both show.  nvalid: rows below it are data, the rest padding.
 *   plan   0  potrf_inv(0, npad, need_inv = true, keep_L)     1  potrf_inv(0, npad, need_inv = false, keep_L)
 *          2  potrf_nll(0, npad) with nll_block (a multiple of 128 in 128 .. npad)
 *   flags  bit 0: stable mode;  bit 1: keep_L;  bit 2 (plan 0 only): after the download, Ainv = W^T W (lauum) goes into
 *          the scratch and the whole scratch comes back in Ainv[batch][npad][npad]
 * r, z (optional, [batch][npad] each): z = L^-1 r by the forward solve that belongs to the plan -- forward_solve with
 * the plan's need_inv, forward_solve_nll for plan 2 -- on a device copy of r (the solve consumes it).  r must be finite,
 * padding included (blas1.h: trmv_kernel).  logdet, info: [batch].  No persistent-launch counters, no side stream;
 * "dual_launch" and "leaf" follow gpc_set_option.  Anything else is refused (-2).                                      */
int gpc_debug_factor_plan(gpc_ctx* ctx, int dtype, int npad, int nvalid, int batch, int plan, int nll_block, int flags,
                          double* A, double* W, double* T, const double* r, double* z, double* Ainv, double* logdet,
                          int* info);
/* The covariance kernels of the evaluation and prediction paths on ONE sample, launched as those paths launch them
 * (the inputs scaled by scale_x_kernel from hyp_cov, the per-sample scalars sf2 / alpha_rq from hyp_cov, kscale and sl
 * from the caller), on buffers of the hook's own; npad / mpad = N / M rounded up to 128.  which:
 *   0  build_kernel:        out0[npad x npad] = K / kscale + diag(dvec[N]), identity padding (tiles above the diagonal 0)
 *   1  small_front_kernel:  the same through the one-leaf front (N <= 128)
 *   2  cross_tile_kernel:   out0[npad x mpad] = K(X, Xstar[M x D]), out1[mpad] = the fused column sums Ks^T vec[N]
 *   3  trace_kernel + the reduction of its partials: Q = mat / sl - vec vec^T over the lower triangle of mat[N x N]
 *      (stored in `dtype`): out0[cov_N + 1] = sum_ij w_ij Q_ij dK_ij/dtheta_p, last slot trace(Q); out1[npad] = diag(Q)
 *   4  grad_operand_tile_kernel (gpc_grad_post's operand), one launch per block of 128 queries as the product path
 *      launches it: out0[block][npad][(D + 1) 128] = the panels, slot-major planes (column a 128 + j: slot a of query j
 *      of the block; slot 0 = k, slot 1 + l = dk/dx*_l), zero padding; out1[block][(D + 1) 128] = the fused column sums
 *      against vec[N]
 * xs_out (optional): the scaled inputs, npad x D (which = 2: followed by the mpad x D of Xstar).                        */
int gpc_debug_cov(gpc_ctx* ctx, int which, int kernel_id, int degree, int dtype, const double* hyp_cov,
                  double kscale, double sl, const double* dvec, const double* X, int N, int D,
                  const double* Xstar, int M, const double* mat, const double* vec, double* out0,
                  double* out1, double* xs_out);

/* ONE launch of one kernel of gpyreg_amd/csrc/blas1.h, with the grid and block of the production call it mirrors, on
 * buffers of the hook's own (allocated for the call and freed before it returns).  in[0..5]: the operands, in_n[k]
 * doubles each (NULL / 0: absent), uploaded whole and verbatim -- padding and whatever lies outside the kernel's
 * contract included; operands the kernel reads as `dtype` are converted with a plain cast, the others stay double.
 * out[0..2]: every result buffer has out_n[k] elements plus a guard of 128; it is filled with quiet NaNs before the
 * launch -- or, for a kernel that updates in place, starts from the operand named below -- and comes back WHOLE, the
 * guard included, as out_n[k] + 128 doubles: "not written" and "written past the end" both show.  All matrices are
 * dense with the natural batch stride.  grad_tail_kernel always gets alpha, diagq and all three results: without mean
 * or noise slots mg / ng are the guard alone (out_n = 0), so that a write there shows.  (T): stored in `dtype`.
 * which, ip[], in[], out[]:
 *    0 trmv_kernel              npad, batch, row0, rows              W (T), r                    z[batch npad]
 *    1 trmv_low_kernel          npad, batch                          W (T), r                    z
 *    2 gemv_sub_kernel          npad, batch, row0, nrows, col0, ncols  A (T), z, r               r, in place (in[2])
 *    3 trmv_t_part_kernel<T, 8> npad, batch, quad (0 | 1)            W (T), z                    part[batch npad/128 npad],
 *                                                                                               quad[batch]
 *    4 trmv_t_part_low_kernel   as 3
 *    5 trmv_t_sum_kernel        npad, batch, sp_stride, sp_off       part, sp (NULL: no scale)   out[batch npad]
 *    6 dot_kernel               n, stride, batch                     x, y                        out[batch]
 *    7 mat_t_vec_kernel         n, P, vstride, batch                 Mat, vec                    out[batch P]
 *    8 grad_tail_kernel         ntiles, P, n, mean_N, noise_N, vstride, batch
 *                                                part, dm (NULL: ones), alpha, dsn2, diagq       gout[batch P], mg[batch mean_N],
 *                                                                                               ng[batch noise_N]
 *    9 colsum_prod_kernel       ld, nrows, mpad, batch               A (T), B (T)                out[batch mpad]
 *   10 colsum_vec_kernel        ld, nrows, mpad, vstride, batch      A (T), v                    out[batch mpad]
 *   11 diagq_kernel             n, ld, P, batch                      Ainv (T), alpha, sp[batch 4]   diagq[batch ld], out[batch P]
 *   12 trace_plane_kernel       n, ld, blocks                        Ainv (T), alpha, sp[4], dK  part[blocks]
 *   13 extract_kernel           n, ld, mode                          src (T)                     dst[n n]
 *   14 neg_sym_kernel           npad, ld, batch                      buf (T)                     buf (T), in place (in[0])
 *   15 pad_load_kernel          n, npad                              src                         dst (T)[npad npad]
 *   16 pad_rect_kernel          r, c, rpad, cpad                     src                         dst (T)[rpad cpad]
 *   17 load_K_kernel            n, npad                              K, sp[4], dvec              A (T)[npad npad]
 *   18 rect_copy_kernel         rows, cols, lds, ldd, batch          src (T), dst (T)            dst (T), in place (in[1])
 *   19 grow_copy_kernel         np, npn, batch                       src (T)                     dst (T)[batch npn npn]
 *   20 append_row_kernel        npad, n, batch          A (T), W (T), l, au, coef[batch 5], alpha   A (T), W (T), alpha, in place
 *                                                                                               (in[0], in[1], in[5])
 *   21 append_low_kernel        ld, n                   A (T), au, coef[5], alpha                A (T), alpha, in place
 *                                                                                               (in[0], in[3])
 * A launch that would read or write outside these buffers is refused (-2), and so is a vector of which = 0, 1, 3, 4
 * that is not finite over the rows of the launch: those kernels read W's diagonal tiles unmasked (blas1.h).             */
int gpc_debug_blas1(gpc_ctx* ctx, int which, int dtype, const int* ip, const double* const* in, const long long* in_n,
                    double* const* out, const long long* out_n);

/* The panel kernel of gpc_post_remove alone on one 64 x 64 block (remove.h: rm_panel_kernel), launched as the sweep
 * launches it: D (64 x 64, row major; the lower triangle is read, cast to `dtype`), Vp (64 x k, fp64), 1 <= k <= 64.
 * Theta ((64 + k) x (64 + k), row major): the orthogonal matrix with [D | Vp] Theta = [Dnew | 0];  Dnew (64 x 64): the
 * block as stored afterwards (lower triangular with a positive diagonal; the upper triangle is D's, untouched).    */
int gpc_debug_remove_panel(gpc_ctx* ctx, int dtype, int k, const double* D, const double* Vp, double* Theta,
                           double* Dnew);

/* The apply kernel of gpc_post_remove alone (remove.h: rm_apply_kernel) on a given Theta ((64 + k)^2, row major) for
 * the panel [a, a + 64) of a matrix of n rows (a a multiple of 64), storage in `dtype`, carriers fp64, in place:
 *   which = 0, the L side:  P = L[a+64 : n, a : a+64] ((n - a - 64) x 64),  Cr = V[a+64 : n, :] ((n - a - 64) x k):
 *                           [P | Cr] <- [P | Cr] Theta                                              (n > a + 64)
 *   which = 1, the W side:  P = W[a : a+64, :n] (64 x n; rows a + p >= n and entries above the diagonal are neither
 *                           read nor written),  Cr = C (k x n):   [P ; Cr] <- Theta^T [P ; Cr]      (n > a)     */
int gpc_debug_remove_apply(gpc_ctx* ctx, int dtype, int which, int a, int n, int k, const double* Theta, double* P,
                           double* Cr);

/* gpc_grad_post's block Gram kernel on caller-provided panels Y, Z: n rows x (Dp planes of M queries), row major
 * ([i][a][j]), stored in `dtype` and padded to the pipeline's plane width.  Z = NULL: Z = Y.  out[j][a][b] = out[j][b][a]
 * = sum_i Y[i][a][j] Z[i][b][j] for a >= b (the lower triangle, mirrored), accumulated in fp64 in an order fixed by n alone;
 * diag_only != 0: out[j][a] = sum_i Y[i][a][j] Z[i][a][j].                                                            */
int gpc_debug_block_gram(gpc_ctx* ctx, int dtype, int n, int M, int Dp, const double* Y, const double* Z, int diag_only,
                         double* out);

/* gpc_predict_hess's contraction kernel on caller-provided weights, one launch per block of 128 queries as the product
 * path launches it (inputs scaled from hyp_cov as in gpc_debug_cov; Q stored in `dtype`).  With P = 1 + D (D + 1) / 2:
 *   out_alpha[j][0] = sum_i alpha_i F_ij,   out_alpha[j][1 + a (a + 1) / 2 + b] = sum_i alpha_i G_ij d_a d_b  (a >= b)
 *   out_q[j][.]     = the same with the weights Q[i][j] (dense N x M; optional: NULL runs the kernel of the mean alone)  */
int gpc_debug_hess_contract(gpc_ctx* ctx, int kernel_id, int degree, int dtype, const double* hyp_cov, const double* X,
                            int N, int D, const double* xstar, int M, const double* alpha, const double* Q,
                            double* out_alpha, double* out_q);

/* gpc_predict_hyp_grad's fused cross pass on caller-provided weights, one launch over all queries (inputs scaled from
 * hyp_cov as in gpc_debug_cov): alpha[N], W[P x N] the weight vectors (P >= cov_N), Q dense N x M taken with factor 1
 * (optional: NULL runs the kernel of the mean alone, which leaves the C sums out).  out[j][.], rows of P + cov_N (+ cov_N):
 *   out[j][p]             = sum_i k_ij W[p][i]                                             p < P
 *   out[j][P + c]         = sum_i d_c k_ij alpha_i                                         c < cov_N
 *   out[j][P + cov_N + c] = sum_i d_c k_ij Q[i][j]                                         c < cov_N  (with Q)
 * d_c k = F d_a^2 (lengthscale a; isotropic F r2) | k itself for log sf (the caller doubles it) | Ka (RQ shape).     */
int gpc_debug_hyp_cross(gpc_ctx* ctx, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                        const double* xstar, int M, const double* alpha, const double* W, int P, const double* Q,
                        double* out);

/* gpc_nll_hess's plane kernel on one sample, launched as the call launches it (inputs scaled from hyp_cov as in
 * gpc_debug_cov): covariance hyperparameter p < cov_N, weights alpha[N] and a dense symmetric Q[N x N] (NULL: zeros).
 *   plane[N x N] = d K / d theta_p;   u[N] = plane alpha;   g[0] = <Q - alpha alpha^T, plane>;
 *   g[1] = <Q - alpha alpha^T, second>, second = G r2^2 (isotropic lengthscale) | dF/dlog(alpha) d_p^2 (RQ lengthscale)
 *          | dKa/dlog(alpha) (RQ shape) | 0                                                                              */
int gpc_debug_nll_plane(gpc_ctx* ctx, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                        int p, const double* alpha, const double* Q, double* plane, double* u, double* g);

/* gpc_nll_hess's second-derivative contraction (ARD families) on caller-given weights: over the lower triangle,
 *   out[a (a + 1) / 2 + b] = sum_ij w_ij (Q_ij - alpha_i alpha_j) G_ij d_a^2 d_b^2,  a >= b,  w = 1 on the diagonal, else 2 */
int gpc_debug_nll_d2(gpc_ctx* ctx, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                     const double* alpha, const double* Q, double* out);

/* gpc_nll_hess's Gram pass on caller-given planes[P][npad][npad] (npad a multiple of 64, at most 4096; P <= 128):
 *   out[p (p + 1) / 2 + q] = sum_ab planes[p][a][b] planes[q][b][a],  q <= p  (P (P + 1) / 2 values, nothing beyond)   */
int gpc_debug_nll_gram(gpc_ctx* ctx, int npad, int P, const double* planes, double* out);

/* gpc_cv_grad's contraction alone on one sample, launched as the call launches it (inputs scaled from hyp_cov as in
 * gpc_debug_cov): M[N x N] read from its lower triangle, alpha[N], beta[N];  G_ij = M_ij - (beta_i alpha_j + alpha_i beta_j) / 2:
 *   gsum[p] = sum over i >= j of w_ij G_ij d_p K_ij,  p < cov_N,  w = 1 on the diagonal, else 2;   diagG[i] = G_ii       */
int gpc_debug_cv_trace(gpc_ctx* ctx, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                       const double* M, const double* alpha, const double* beta, double* gsum, double* diagG);

/* gpc_cv_grad's per-point kernel: c[N] and b[N] of `loss` (0 = lpd, 1 = mse) from alpha[N], q[N] and weights[N] (NULL:
 * ones), the formulas of gpc_cv_grad.                                                                                   */
int gpc_debug_cv_weights(gpc_ctx* ctx, int N, int loss, const double* alpha, const double* q, const double* weights,
                         double* c, double* b);

/* Debug: wrapping-sum hash of every 128 x 128 tile of one workspace matrix as the LAST call left it (which: 0 = A, 1 = W,
 * 2 = T; sample: position in the last chunk); out[(npad/128)^2].  Finds the tile where two schedules differ.          */
int gpc_debug_workspace_hash(gpc_ctx* ctx, int dtype, int which, int sample, unsigned long long* out);

/* Debug, HOST ONLY (no device needed): the samples per chunk every posterior consumer and evaluation works on when
 * each sample needs `per` bytes of scratch beside `shared` bytes for the whole call and `budget` bytes may be used
 * (the callers pass 80 % of what is free, or of GPC_MEM_BUDGET_MB).  min(S, (budget - shared) / per); when not even
 * one sample fits: 0 (the caller refuses), or 1 with clamp_to_one (the caller runs one sample at a time anyway).
 * -2 for S <= 0 or per = 0.                                                                                          */
int gpc_debug_chunk_plan(int S, unsigned long long per, unsigned long long shared, unsigned long long budget,
                         int clamp_to_one);
/* Debug, HOST ONLY (no device needed): the device scratch a posterior consumer declares (its layout, counted as the
 * call itself counts it).  per: bytes of one sample, what the planner above divides by (a draw's includes the three
 * slabs it factors in); shared: bytes the call needs once; misaligned: arrays that would miss their alignment when
 * the layout is carved for three samples on a 256-byte aligned base (nothing is allocated or dereferenced) -- 0, or
 * the call itself would fail.  name and dims (N is the number of training points, not padded):
 *   "rhs"          N, M, D, S, kind (0 cross, 1 quadrature, 2 given Ks, 3 gradient observations), want_quad, full,
 *                  grad, quad_grad, R (draws; 0: none), points of a gradient-observation posterior
 *   "predict_cov"  N, Ma, Mb, D, want_cov, want_wsq          "grad_post" N, M, D, diag   "predict_hess" N, M, D, var
 *   "append_block" N + k, k, engine                          "remove" N, k               "cv_loo" N
 *   "cv_fold"      N, F, k_max, engine                       "paths_create" N, R, solve engine
 *   "paths_eval"   N, M, R, S, D, F_pad, engine, grad        "nll_hess" N, cov_N, noise_N, mean_N, nd2
 *   "cv_grad"      N, cov_N      "hyp_grad" N, D, P, nvv, ngp, msb, var, nout            "quad_mix" N, M, D, var, grad
 * -2 for an unknown name, a wrong ndims or a null argument.                                                          */
int gpc_debug_scratch_bytes(const char* name, int dtype, const int* dims, int ndims, unsigned long long* per,
                            unsigned long long* shared, int* misaligned);
/* Debug, HOST ONLY (no device needed): the index arithmetic of the GEMM launch forms (gemm.h) enumerated for one
 * launch of `ntiles` tiles and `batch` samples -- tile_of_bx and xcd_order, which the kernels call themselves, and
 * queue_of / queue_total / queue_item / flat_queue_item, the host's restatement of gemm_persist_kernel's queues.
 *   q_total[8]              items of each tile queue of a persistent launch (flags & 8: the eight XCD-affine queues;
 *                           otherwise the one flat queue in slot 0, the rest 0)
 *   q_items[2 ntiles batch] optional: the (tile, sample) pairs the queues hand out, queue after queue in the order of
 *                           their counters
 *   tile_ij[2 ntiles]       optional: the tile (ti, tj) of every position bx of the dispatch order of a square-tile
 *                           launch with tiles_m x tiles_n tiles and the k-range modes klo / khi / lower_only (ntiles
 *                           must be what such a launch has)
 *   xcd_items[2 ntiles batch] optional: the item (bx, by) that workgroup L = by * ntiles + bx of a plain (ntiles, batch)
 *                           grid takes -- the XCD-aware order when flags & 16 and batch >= 8, else the identity
 * Returns 0, -2 (bad arguments), -3 (the queues hold more than ntiles * batch items).                                */
int gpc_debug_gemm_queues(int ntiles, int batch, int flags, int tiles_m, int tiles_n, int klo, int khi, int lower_only,
                          int* q_total, int* q_items, int* tile_ij, int* xcd_items);
/* Debug, HOST ONLY (no device needed): what the zero-skipping instantiation `tri` of the fp64 128-tile GEMM (gemm.h:
 * GemmArgs::tri -- 1 A-first, 2 A-last, 3 B-first, 4 B-last, + 8 diag-lower) does in k-slab `slab` (0..7) of the
 * triangular diagonal 128-block of a tile's k-range, per wave w = 2 wr + wc of the block, through the mask types the
 * kernel is built from.  diag_tile: the tile is a diagonal output tile of a lower_only launch.
 *   frag_rows[4 * 4], frag_cols[4 * 4]  the 16-row / 16-column fragment of the 128-tile that slot i / j of wave w owns
 *   issued[4 * 4 * 4]                   1 where wave w issues the MFMAs of its fragment (i, j) in that slab
 *   stored[4 * 4 * 4]                   1 where wave w stores its fragment (i, j) at the end of the tile
 * Returns 0 or -2 (bad arguments).                                                                                   */
int gpc_debug_tri_masks(int tri, int diag_tile, int slab, int* frag_rows, int* frag_cols, int* issued, int* stored);
/* Debug, HOST ONLY: the instantiation (the `tri` of gpc_debug_tri_masks; 0: the plain kernel) that launch_gemm_bt picks
 * for a launch of `tile`-tiles (64 | 128) that gives the guarantee `tri` with these orientations, k-range modes and
 * sizes -- gemm.h: tri_usable, the function the launcher calls.  -2: bad arguments.                                  */
int gpc_debug_tri_usable(int dtype, int tile, int a_kmajor, int b_kmajor, int klo, int khi, int lower_only, int M, int N,
                         int K, int tri);

/* One product of gpc_debug_gemm_form, as the kernels see it: C[b] (M x N, rows ldc apart, at element off_c + b s_c of
 * an allocation of size_c elements) = beta C[b] + alpha op(A[b]) op(B[b]); A stored K x M when a_kmajor (else M x K)
 * with rows lda apart at off_a + b s_a, B stored K x N when b_kmajor (else N x K).  Leading dimensions may exceed the
 * extents, a stride may be 0 (an operand every sample shares); lda, ldb and the offsets and strides of A and B are
 * multiples of the 16-byte vector (2 fp64 / 4 fp32 elements).  A, B, C: the WHOLE allocations (host, fp64; converted
 * for an fp32 launch); C is overwritten with the whole allocation as the launch left it.                            */
typedef struct gpc_gemm_product {
  int M, N, K;
  int a_kmajor, b_kmajor;
  int beta, klo, khi, lower_only;
  int lda, ldb, ldc;
  long long off_a, off_b, off_c;
  long long s_a, s_b, s_c;
  long long size_a, size_b, size_c;
  double alpha;
  const double* A;
  const double* B;
  double* C;
} gpc_gemm_product;
enum { GPC_FORM_PLAIN = 0, GPC_FORM_PERSIST = 1, GPC_FORM_PERSIST_RESERVED = 2, GPC_FORM_DUAL = 3, GPC_FORM_COLSQ = 4,
       GPC_FORM_WSQ = 5 };
/* Test hook: one product through ONE launch form of gemm.h, by the launchers the product uses.  form:
 *   PLAIN              launch_gemm_bt without counters: gemm_kernel (XCD-aware order with flags & 16 and batch >= 8)
 *   PERSIST            launch_gemm_bt with counters: gemm_persist_kernel when the launch has more items than block
 *                      slots (128-tiles; a 64-tile launch without a reservation is always plain), flat queue or, with
 *                      flags & 8, the eight XCD-affine queues
 *   PERSIST_RESERVED   the same behind cu_reserve_bail with the context's own table of reserved CUs; *available = 0
 *                      and nothing is launched when the context has none
 *   DUAL               launch_gemm_dual_small: p1 (m-major x m-major) and p2 (m-major x k-major) as 64-tiles in one grid
 *   COLSQ              launch_gemm_colsq (EPI 1; m-major x k-major, 128-tiles, persistent as PERSIST): C is not stored,
 *                      colsq[(b tiles_m + ti) N + col] = sum over the 128 rows of tile row ti of (alpha acc)^2
 *   WSQ                launch_gemm_wsq (EPI 2; k-major x k-major, 128-tiles, plain): C is read, colsq[...] = sum over
 *                      those rows of ep_w[b ep_sw + row] (C + ep_alpha[b] acc)^2; ep_w holds (batch - 1) ep_sw + M values
 * tile: 64 or 128 (PLAIN, PERSIST, PERSIST_RESERVED).  flags >= 0 replaces the GEMM flags (bit 3: XCD-affine queues,
 * bit 4: XCD-aware order) and block_slots > 0 the block slots of the chip (and clears persist_spare) for this call
 * only.  Bits 8-11 of flags >= 0 are the GemmArgs::tri of the products (1 A-first, 2 A-last, 3 B-first, 4 B-last: the
 * operand is lower triangular in the first / last 128-block of each tile's k-range; + 8 diag-lower: the fragments above
 * the diagonal of the diagonal tiles of a lower_only launch may stay unwritten): the CALLER vouches that the operands it
 * uploads are zero there -- the fp64 128-tile forms then do not multiply by that half, every other form ignores the
 * bits (gpc_debug_tri_usable says which instantiation a launch gets).  The hook checks that every operand lies inside its allocation, allocates and zeroes its own counters, and
 * returns the eight queue counters as the launch left them (all 0 after a plain launch).  colsq[batch (M / 128) N]
 * (COLSQ, WSQ) is preset to NaN.                                                                                     */
int gpc_debug_gemm_form(gpc_ctx* ctx, int dtype, int form, int tile, int batch, int flags, int block_slots,
                        const gpc_gemm_product* p1, const gpc_gemm_product* p2, const double* ep_w, long long ep_sw,
                        const double* ep_alpha, double* colsq, int* counters, int* available);

/* ---- Gradient observations (gpyreg_amd/csrc/gradobs.h; DESIGN.md "Gradient observations") -------------------------
 * Conditioning on values y at X (N x D) AND gradients dy (Ng x D, row g = grad f(Xg[g])) at Xg (Ng x D; rows may repeat
 * rows of X).  The joint system has order n = N + Ng D; its rows are the values first, then the gradient rows
 * DIMENSION-MAJOR: row N + l Ng + g = d f / dx_l at Xg[g].  Every S x n array below (m, sn2) and every fetched alpha / L
 * is in that order.  The joint covariance is built on the device (k, -c_a F d_a, c_a c_b (F delta_ab - G d_a d_b) with
 * the pair functor's radial factors); from there on it is the caller-provided-K pipeline: the reference's scaling by
 * min(sn2) over the JOINT noise vector, its branch rule min(sn2) >= 1e-6, the x 10 jitter ladder, alpha, log det.
 * Built-in kernels only; the Matern kernel of degree 1 (no mean-square derivative) is an error.
 *
 * gpc_set_data_gobs makes the points and the joint target [y | dy in joint order] resident; the context's problem
 * order becomes n (gpc_max_n applies to n).  While such data are resident only the _gobs and _K entry points evaluate
 * them; gpc_set_data switches back.                                                                                  */
int gpc_set_data_gobs(gpc_ctx* ctx, const double* X, const double* y, int N, int D, const double* Xg, const double* dy,
                      int Ng);
/* Posteriors of S hyperparameter rows.  m: S x n, the mean function at X and its x-gradient at Xg in joint order;
 * sn2: S x n joint noise variances (always per row; zeros are allowed and take the low-noise branch by the rule
 * above).  nlz (S; may be NULL): the joint negative log marginal likelihood as this pipeline rounds it --
 * gpc_nll_batch_gobs factors without the inverse and agrees with it to rounding, not to the bit.  sn2_mult, L_chol,
 * info as gpc_posterior_batch.  The handle is a GRADIENT-OBSERVATION posterior: it owns a copy of the points,
 * gpc_predict_gobs, gpc_grad_post_gobs, gpc_post_fetch (alpha: n, L: n x n) and gpc_post_free work on it, and every
 * other consumer (gpc_predict, gpc_predict_grad, gpc_grad_post, gpc_post_append*, gpc_post_remove, gpc_draw,
 * gpc_paths_create, gpc_cv, gpc_quad*, gpc_predict_K, ...) returns an error that says so.                             */
int gpc_posterior_batch_gobs(gpc_ctx* ctx, int kernel_id, int degree, int dtype, int S, const double* hyp_cov,
                             const double* m, const double* sn2, gpc_post** post, double* nlz, double* sn2_mult,
                             int* L_chol, int* info);
/* The joint negative log marginal likelihood alone, for S arbitrary hyperparameter rows (no posterior is kept, no
 * gradient: gpc_nll_batch_gobs_grad has it).                                                                        */
int gpc_nll_batch_gobs(gpc_ctx* ctx, int kernel_id, int degree, int dtype, int S, const double* hyp_cov,
                       const double* m, const double* sn2, double* nlz, double* sn2_mult, int* L_chol, int* info);
/* gpc_nll_batch_gobs with the hyperparameter gradient: dnlz (S x (cov_N + noise_N + mean_N), ordered
 * [cov | noise | mean] like gpc_nll_batch) = d nlz / d theta at each sample's final jitter multiplier.  The covariance
 * part is 1/2 sum_IJ ((K + Sigma)^-1 - alpha alpha^T)_IJ dK_IJ / d theta_p with every dK entry evaluated on the device
 * from the point list (gradobs.h: gobs_trace_kernel; the third radial factor H = -2 dG/d(r2)) -- no derivative plane
 * exists on either side of the bus.  dm: S x n x mean_N, the theta-derivatives of the joint mean rows (the mean at X,
 * its x-gradient at Xg); dsn2: S x n x noise_N, those of the joint noise rows (zeros on the gradient rows: their noise
 * is data).  Either may be NULL when its count is 0.  nlz is the number of THIS pipeline (it forms the inverse) and
 * agrees with gpc_nll_batch_gobs to rounding, not to the bit.  fp64 only: any other dtype is an error.               */
int gpc_nll_batch_gobs_grad(gpc_ctx* ctx, int kernel_id, int degree, int dtype, int S, const double* hyp_cov,
                            const double* m, const double* sn2, const double* dm, int mean_N, const double* dsn2,
                            int noise_N, double* nlz, double* dnlz, double* sn2_mult, int* L_chol, int* info);
/* gpc_predict for a gradient-observation posterior: the n x M operand [k(X, x*) ; -c_l F (xs_g - xs*)_l] is built on
 * the device with the mean product fused in; fmu (caller adds m*) and fs2 (unclamped) as gpc_predict, [j*S + s].    */
int gpc_predict_gobs(gpc_post* post, const double* xstar, int M, double* fmu, double* fs2);
/* gpc_grad_post for a gradient-observation posterior: the joint posterior of (f(x*), grad f(x*)) given values AND
 * gradients.  Arguments, layouts and semantics are gpc_grad_post's (fmu [j*S + s], dfmu [(j*D + l)*S + s], cov
 * [((j*(D+1) + a)*(D+1) + b)*S + s] or, with diag_only, [(j*(D+1) + a)*S + s]; slot 0 = f, slot 1 + l = d/dx_l; no
 * clamp, no noise, no mean function; symmetric to the bit).  The operand is the npad x (D + 1) 128 panel of the JOINT
 * system per block of 128 queries (gradobs.h: gobs_grad_operand_tile_kernel -- value rows [k | -c_l F (xs* - xs_i)_l],
 * gradient rows N + a Ng + g [-c_a F d_a | c_a c_l (F delta_al - G d_a d_l)], d = xs_g - xs*), with the mean product
 * fused in; the products with the factor, the per-query Gram matrices and the diagonal form are gpc_grad_post's own.
 * A handle without gradient observations, or one that is not factorized, is an error.  Counter
 * "gobs_grad_operand_us": the device time of the operand builds of a timed call.                                     */
int gpc_grad_post_gobs(gpc_post* post, const double* xstar, int M, int diag_only, double* fmu, double* dfmu, double* cov);
/* Test hooks: the kernels of gradobs.h on their own, fp64, one hyperparameter row.
 * gpc_debug_gobs_cov: out = the dense n x n joint covariance (preset to NaN, so an entry nobody wrote shows).
 * gpc_debug_gobs_cross: out = the WHOLE panel, pad128(n) x pad128(M) row-major (preset to NaN; rows >= n and columns
 * >= M must come back as zeros); colsum (pad128(M); may be NULL) = the fused products out^T alpha with alpha (n; NULL:
 * zeros) in joint order.
 * gpc_debug_gobs_grad_operand: gobs_grad_operand_tile_kernel as gpc_grad_post_gobs launches it for ONE block of queries
 * (M <= 128): out = the WHOLE panel, pad128(n) x (D + 1) 128 row-major, column a 128 + j = slot a of query j (preset to
 * NaN; rows >= n and queries >= M must come back as zeros); colsum ((D + 1) 128; may be NULL) = the fused products
 * out^T alpha.  Counter "gobs_grad_operand_us": the device time of the build.                                         */
int gpc_debug_gobs_cov(gpc_ctx* ctx, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                       const double* Xg, int Ng, double* out);
int gpc_debug_gobs_cross(gpc_ctx* ctx, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                         const double* Xg, int Ng, const double* xstar, int M, const double* alpha, double* out,
                         double* colsum);
int gpc_debug_gobs_grad_operand(gpc_ctx* ctx, int kernel_id, int degree, const double* hyp_cov, const double* X, int N,
                                int D, const double* Xg, int Ng, const double* xstar, int M, const double* alpha,
                                double* out, double* colsum);
/* gpc_debug_gobs_trace: gobs_trace_kernel and its reduction alone.  Ainv: n x n row-major, of which only the LOWER
 * triangle is read (the weight is Ainv / sl - alpha alpha^T, taken symmetric); alpha: n; sl > 0.  out (cov_N) =
 * sum_IJ weight_IJ dK_IJ / d theta_p.  Counter "gobs_trace_us": the device time of the contraction.                   */
int gpc_debug_gobs_trace(gpc_ctx* ctx, int kernel_id, int degree, const double* hyp_cov, const double* X, int N, int D,
                         const double* Xg, int Ng, const double* Ainv, const double* alpha, double sl, double* out);
/* ---- experiments build only (hipcc -DGPC_EXPERIMENTS -> lib/libgpcore_exp.so; NOT part of the product library) --------
 * Schedules that were built, measured and rejected (tile-level dataflow graph, independent pipelines,
 * rectangular / eight-wave tiles, right-looking panels) and their gpc_set_option names live there;
 * gpc_get_option(ctx, "experiments") says which build is loaded.                                                        */
#ifdef GPC_EXPERIMENTS
/* The tile-task graph of the dataflow schedule (gpyreg_amd/csrc/dag.h) for an npad x npad factorization --
 * HOST ONLY, no device needed: tests/test_dag_model.py executes it with NumPy tiles in random valid orders.
 * plan: 0 = NLL only (blocked solves above nll_blk rows when nll_blk > 0), 1 = factor + inverse + W^T W,
 * 2 = factor + inverse.  counts[4] = tasks, edges, launches, leaves.  With tasks_out == NULL only the counts are
 * written.  tasks_out: 24 ints per task [is_leaf, tile, a_kmajor, b_kmajor, beta, C/A/B region as (buffer, r0, r1,
 * c0, c1) each, predecessors, first successor, successors, ring]; alpha_out: one double per task; succ_out: the
 * successor lists.  Returns 0, -1 (plan not supported), -2 (bad arguments), -3 (buffers too small).               */
int gpc_debug_dag(int npad, int plan, int nll_blk, int small_tiles, int* counts, int* tasks_out,
                  double* alpha_out, int* succ_out, int cap_tasks, int cap_edges);

#endif /* GPC_EXPERIMENTS */

#ifdef __cplusplus
}
#endif
#endif /* GPCORE_H */
