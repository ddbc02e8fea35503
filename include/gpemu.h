/*
 * gpemu.h -- C ABI of libgpemu.so: the MI355X (gfx950) implementation of the GP-emulator +
 * MCMC log-posterior hot path of jdmulligan/bayesian-inference.
 *
 * The reference has no FFI of its own (it is pure Python); each entry point below replaces the
 * arithmetic behind one reference call site, cited as  ref: <file>:<lines>  relative to
 * /root/reference/src/bayesian_inference/, and  skl: <file>:<lines>  for the scikit-learn 1.7.2
 * code the reference delegates to.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  All real arrays are row-major float64, indices int64.
 *   - Buffers are caller-allocated.  Functions named *_dev take DEVICE pointers and a hipStream_t (passed as void*), on
 *     which all their work is enqueued; the others take HOST pointers, copy, run and synchronise before returning.
 *     What NULL means and whether a *_dev call waits for its stream before it returns depends on the family:
 *       - gpemu_gp_predict_dev, gpemu_predict_full_dev, gpemu_logpost_dev, gpemu_gp_predict_grad_dev and
 *         gpemu_logpost_grad_dev: NULL = the model's own stream; they do not synchronise (a first call, or one that
 *         has to regrow the model's workspace, allocates and frees, which may wait for the device);
 *       - every other *_dev entry waits for its stream before it returns, because its scratch goes with the call or its
 *         results are host arrays; its section says what NULL means: the model's stream for the entries bound to a
 *         model, the null stream for the device-wide families.
 *     A model's own stream is a non-blocking stream: it is NOT ordered with the null stream or with any other stream.
 *     Work the caller enqueued elsewhere must have finished before a call on the model's stream reads it, and
 *     gpemu_model_sync comes before anything else reads the results.
 *     The *_dev entries of the weighted chain summaries take their stream and their workspace limit
 *     together, in a gpemu_call_ctx; their section says what a NULL stream means, and each of them waits for its stream
 *     before it returns.
 *   - A call writes only the elements of its outputs that its section names.  It does not write padding (ld > n),
 *     gaps of a strided view, or anything before or after.  It does not write its inputs.  Its results do not depend
 *     on the previous contents of the outputs or on memory beside the inputs.  A declined call writes nothing.  (A
 *     section that leaves elements of an output unwritten says which.)  Pointers need the natural alignment of their
 *     element type, 8 bytes for double and int64, and no more.  tests/guard_cases.py holds every *_dev entry to this.
 *   - Every function returns int: 0 = ok, <0 = argument / runtime error, >0 = numerical failure
 *     (e.g. index+1 of a non-positive Cholesky pivot).  gpemu_last_error() gives the thread-local
 *     message of the last failure.
 *   - Opaque handles own all device memory they allocate and are bound to one HIP device.  A handle
 *     is not thread-safe (one host thread per handle); calls release no Python state, so ctypes may
 *     drop the GIL around them.
 *   - There is NO CPU implementation behind these symbols: without a HIP device every compute
 *     entry point fails with GPEMU_ERR_NO_DEVICE.
 */
#ifndef GPEMU_H
#define GPEMU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPEMU_OK 0
#define GPEMU_ERR_ARG (-1)
#define GPEMU_ERR_HIP (-2)
#define GPEMU_ERR_NO_DEVICE (-3)
#define GPEMU_ERR_STATE (-4)
#define GPEMU_ERR_UNSUPPORTED (-5)

/* kernel_kind (ref: emulation.py:133-149) */
#define GPEMU_KERNEL_RBF 0    /* skl gaussian_process/kernels.py:1553-1582 */
#define GPEMU_KERNEL_MATERN 1 /* skl gaussian_process/kernels.py:1708-1781: any nu > 0 (0.5 / 1.5 / 2.5 closed forms, +inf = RBF, else K_nu) */

/* gpemu_logpost mode */
#define GPEMU_LOGPOST_LOWRANK 0 /* k x k Woodbury form, the throughput path          */
#define GPEMU_LOGPOST_EXACT 1   /* materialise Sigma (F x F) + batched Cholesky, reference form  */

typedef struct gpemu_model gpemu_model;     /* one emulation group on one device */
typedef struct gpemu_sampler gpemu_sampler; /* stretch-move ensemble over >= 1 groups */
typedef struct gpemu_fit gpemu_fit;         /* GP fit workspace for one design matrix */

/* ---- library / device ------------------------------------------------------------------- */
const char *gpemu_version(void);
const char *gpemu_last_error(void);
int gpemu_device_count(void); /* number of HIP devices, 0 if none (never an error) */
int gpemu_device_name(int device, char *buf, int64_t buflen);
/* PCI bus id of the device ("0000:c1:00.0"): with the host name it tells whether two ranks of a job share a GPU
 * (gpemu_sampler_peer_share) */
int gpemu_device_bus_id(int device, char *buf, int64_t buflen);
/* free / total device memory in bytes (hipMemGetInfo): the fit sizes its batches within what is free */
int gpemu_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes);

/* ---- model: one emulation group --------------------------------------------------------- */
/* Replaces the per-worker state of ref: log_posterior.py:26-38 (initialize_pool_variables) and
 * the sklearn objects in the results dict of ref: emulation.py:181-192.
 *   X_train[N*d]     design (GaussianProcessRegressor.X_train_)
 *   ls[k*d]          per-PC ARD length scales of kernel_ (not logs)
 *   constv[k]        ConstantKernel value per PC   (read iff has_const)
 *   noise[k]         WhiteKernel noise level per PC (read iff has_noise)
 *   alpha[k*N]       GaussianProcessRegressor.alpha_
 *   L[k*N*N]         GaussianProcessRegressor.L_ (lower; the strict upper triangle is ignored)
 *   components[k*F]  pca.components_[:k]
 *   scaler_mean[F], scaler_scale[F]   StandardScaler
 *   cov_unexplained[F*F]  ref: emulation.py:246-249, or NULL (then 0)
 * The factor is inverted on the device once (W = L^-1) so that prediction is a triangular GEMM.
 * 1 <= d <= 16 (GPEMU_ERR_ARG beyond): d <= 8 runs on 8-wide padded rows, 9 .. 16 on 16-wide ones, whose samplers
 * take the general path (no fused sharded half-step, no small-emulator launch: the sharded run falls back).
 *
 * One model serves a whole analysis.  Calls on it may come in any order and from any handle built on it (samplers of
 * every kind, design handles), one after the other -- not concurrently: the handles share the model's workspace, its
 * caches and its stream.  What came before does not matter: a call on a used model returns, bit for bit, what the same
 * call returns on a model created for it alone (tests/test_gpu_handle_reuse.py), and it uses the likelihood setup
 * current at the call.
 */
int gpemu_model_create(gpemu_model **out, int device, int64_t N, int64_t d, int64_t F, int64_t k,
                       int kernel_kind, double nu, int has_const, int has_noise,
                       const double *X_train, const double *ls, const double *constv,
                       const double *noise, const double *alpha, const double *L,
                       const double *components, const double *scaler_mean,
                       const double *scaler_scale, const double *cov_unexplained);
int gpemu_model_destroy(gpemu_model *m);
int gpemu_model_dims(const gpemu_model *m, int64_t *N, int64_t *d, int64_t *F, int64_t *k);
int gpemu_model_device(const gpemu_model *m);
int gpemu_model_sync(gpemu_model *m); /* wait for the handle's stream */
/* Measurement aid for bench.py: when enabled, every launch of the two hot kernels is bracketed by
 * HIP events on the stream it is launched on.  read -> ms_total[2], launches[2]:
 * [0] = trmm_vsq_kernel (triangular GEMM, MFMA f64), [1] = kstar_kernel (cross-kernel build). */
int gpemu_model_profile(gpemu_model *m, int enable);
int gpemu_model_profile_read(gpemu_model *m, double *ms_total, int64_t *launches);

/* ref: emulation.py:494-499 -> skl _gpr.py:441-494 (predict(X, return_std=True), std squared):
 * X[B*d] -> mean_out[B*k], var_out[B*k]  (negative variances clipped to 0, skl _gpr.py:479-485) */
int gpemu_gp_predict(gpemu_model *m, int64_t B, const double *X, double *mean_out, double *var_out);
int gpemu_gp_predict_dev(gpemu_model *m, int64_t B, const double *dX, double *dmean, double *dvar,
                         void *stream);

/* skl _gpr.py:367-469 predict(X, return_cov=True), per PC: cov_out[p*M1*M2 + a*M2 + b] = kernel_(x1_a, x2_b)
 * - V1_a . V2_b.  X2 == NULL: the symmetric form on X1 (noise on the diagonal, exactly symmetric output).
 * mean_out[M1*k] may be NULL.  workspace_bytes = 0: sized from free device memory.  The _dev form works on `stream`
 * (NULL = the model's) and waits for it before it returns: its workspace goes with the call. */
int gpemu_gp_predict_cov(gpemu_model *m, int64_t M1, const double *X1, int64_t M2, const double *X2,
                         int64_t workspace_bytes, double *mean_out, double *cov_out);
int gpemu_gp_predict_cov_dev(gpemu_model *m, int64_t M1, const double *dX1, int64_t M2, const double *dX2,
                             int64_t workspace_bytes, double *dmean, double *dcov, void *stream);
/* skl _gpr.py:498-531 sample_y: draws_out[p*M*n + a*n + s] = mean_p(x_a) + (chol(C_p + tau_p I) z_p)[a, s],
 * z[k*M*n] standard normals, tau_out[k] the jitter each PC needed; returns p+1 if PC p's ladder is exhausted. */
int gpemu_gp_sample(gpemu_model *m, int64_t M, const double *X, int64_t n_draws, const double *z,
                    double *draws_out, double *tau_out);

/* ref: emulation.py:466-548 (predict_emulation_group): central_value[B*F], cov[B*F*F];
 * n_div = the reference's n_samples divisor of the truncation covariance (emulation.py:531-532).
 * _dev: where dcov is 16-byte aligned and F is even (F <= 512, k <= 16) the covariances are written by the matrix-core
 * writer, which stores two doubles at a time; otherwise by the row-wise writer.  The two add in another order and
 * differ in the last place, so the bits of cov depend on dcov's alignment modulo 16 (and on nothing else
 * about the pointer).  An 8-byte aligned dcov is not declined. */
int gpemu_predict_full(gpemu_model *m, int64_t B, const double *X, double n_div, double *cv_out,
                       double *cov_out);
int gpemu_predict_full_dev(gpemu_model *m, int64_t B, const double *dX, double n_div, double *dcv,
                           double *dcov, void *stream);

/* Cross-validation of the group's emulators at their fitted theta: every point i is predicted by the GP
 * fitted, at the same kernel_ hyper-parameters, to the points of the other folds -- what
 * GaussianProcessRegressor(kernel=gp.kernel_, alpha, optimizer=None).fit(X[R], y[R]).predict(X[I], return_std=True)
 * gives (skl _gpr.py:346-364, 441-494), from the closed form mu_I = y_I - (A_II)^-1 (A y)_I, var = diag((A_II)^-1) -
 * alpha (clipped at 0), A = K^-1.  The scaler and the PCA stay at the full-data fit.
 * fold[N]: labels in [0, n_folds), no fold empty, 2 <= n_folds <= N (else GPEMU_ERR_ARG).  y_train[N*k] = the group's
 * Y_pca_truncated.  -> mean_pc[N*k], var_pc[N*k] (std squared, ref: emulation.py:497-499); central_value[N*F] and the
 * diagonal of the reference's cov, variance[N*F], of predict_emulation_group for one sample (ref: emulation.py:466-548,
 * n_div = 1); either may be NULL. */
int gpemu_model_cross_validate(gpemu_model *m, int64_t n_folds, const int32_t *fold, const double *y_train,
                               double *mean_pc, double *var_pc, double *central_value, double *variance);

/* ref: log_posterior.py:63-64, 73-74, 92-94: box prior + experimental data for this group's
 * features (already gathered into the group's column order).  n_div as above (1 for MCMC).
 * block_start[n_blocks+1]: first feature of every observable of the group (ascending, 0 .. F).
 * The reference's merge keeps only within-observable covariance blocks (ref: emulation.py:370-388),
 * so the likelihood factorises over these blocks.  n_blocks <= 0 or NULL = one block (whole group).
 * A setup may be replaced at any time between calls.  Every call uses the setup current at the call: a sampler created
 * before a new setup and run after it evaluates the new one (its stored log-probabilities are the old setup's until
 * gpemu_sampler_set_state re-evaluates them).  A stacked sampler reads data vector c for chain c where the current setup
 * carries at least one per chain and the one vector for every chain where it carries one.  A setup with fewer vectors
 * than the sampler has chains (but more than one), or groups with correlated sources (n_src > 0) that carry different
 * numbers of vectors, make gpemu_sampler_set_state (where it evaluates), gpemu_sampler_run and
 * gpemu_sampler_step_host_rng of that sampler return GPEMU_ERR_STATE before they copy or launch anything: the sampler
 * is left as it was. */
int gpemu_likelihood_setup(gpemu_model *m, const double *y_exp, const double *y_err,
                           const double *lo, const double *hi, double n_div, int64_t n_blocks,
                           const int64_t *block_start);

/* The same for SEVERAL data vectors against the same uncertainties: the closure tests of ref: steer_analysis.py:168-183
 * condition one chain each on the pseudo-data of one validation point (ref: data_IO.py:362-372).  y_exp[n_chains*F];
 * chain c of a sampler created with gpemu_sampler_create_chains then uses vector c.  Calls outside a multi-chain
 * sampler (gpemu_logpost) use vector 0. */
int gpemu_likelihood_setup_chains(gpemu_model *m, int n_chains, const double *y_exp, const double *y_err,
                                  const double *lo, const double *hi, double n_div, int64_t n_blocks,
                                  const int64_t *block_start);

/* Correlated experimental uncertainties: the data covariance of the group is
 *     C_d = blockdiag_o(C_o) + sum_{s < n_src} b_s b_s^T
 * instead of diag(y_err^2).  cov[F*F] (row-major, this group's column order) holds C_o on the observable blocks and
 * zeros across them (GPEMU_ERR_ARG otherwise); NULL = diag(y_err^2), as gpemu_likelihood_setup_chains.  sources[n_src*F]
 * are the group's columns of n_src fully correlated systematic sources, 0 <= n_src <= GPEMU_MAX_SOURCES (else
 * GPEMU_ERR_ARG); a source may span several observables and several groups, so with n_src > 0 the log-posterior of a
 * set of groups is NOT the sum of the groups' log-posteriors: evaluate them together (gpemu_logpost_groups, or one
 * sampler over all groups), each group set up with its own columns of the same sources.  With cov = NULL and
 * n_src = 0 this is gpemu_likelihood_setup_chains, bit for bit.  GPEMU_LOGPOST_EXACT reads cov; with n_src > 0 it
 * returns GPEMU_ERR_UNSUPPORTED.  The fused sharded run and the peer transport decline sampler groups with n_src > 0
 * (gpemu_sampler_run_sharded takes the collective transport).  A stacked sampler over groups with n_src > 0 needs the
 * same number of data vectors in every group (GPEMU_ERR_STATE from its calls otherwise: gpemu_likelihood_setup). */
#define GPEMU_MAX_SOURCES 16
int gpemu_likelihood_setup_cov(gpemu_model *m, int n_chains, const double *y_exp, const double *y_err,
                               const double *cov, int64_t n_src, const double *sources, const double *lo,
                               const double *hi, double n_div, int64_t n_blocks, const int64_t *block_start);

/* The log-posterior of X[B*d] summed over n_groups models set up on the same device with the same parameter box:
 * out[B].  Where any group has sources, all must have the same n_src (GPEMU_ERR_STATE otherwise) and their term is
 * added once for the set.  n_div: each model's current setup. */
int gpemu_logpost_groups(gpemu_model *const *models, int n_groups, int64_t B, const double *X, double *out, int mode);

/* ref: log_posterior.py:42-101 + 104-146: X[B*d] -> out[B]; rows outside the open box -> -inf.
 * A non-positive-definite covariance yields NaN (the reference does not detect it either,
 * log_posterior.py:125-135). */
int gpemu_logpost(gpemu_model *m, int64_t B, const double *X, double *out, int mode);
int gpemu_logpost_dev(gpemu_model *m, int64_t B, const double *dX, double *dout, int mode,
                      void *stream);

/* ---- derivatives with respect to the parameters ------------------------------------------------
 * Supported: RBF and Matern nu = 1.5, 2.5, inf; with or without constant and noise; 1 <= d <= 16; k <= 64; any number of
 * observable blocks; a dense within-observable data covariance.  Declined before any launch with
 * GPEMU_ERR_UNSUPPORTED: Matern 0.5 and any other nu (the derivative needs K_{nu-1} and is singular or discontinuous at
 * r = 0 for nu < 1), groups with correlated sources (n_src > 0), a likelihood set up for several data vectors, and
 * mode = GPEMU_LOGPOST_EXACT.  A row's results have the same bits whatever else is in the batch.
 * One stream per model: the derivative calls share a workspace that belongs to the model (allocated by the first of
 * them, regrown when a likelihood setup changes the number of observable blocks), as the value calls share theirs.  The
 * _dev forms do not synchronise: calls on one model must be ordered on ONE stream -- two streams at a time, or
 * alternating streams without a synchronisation between the calls, race on that workspace.
 *
 * Jacobians of the PCs' GPs: mean[B*k], var[B*k] (clipped at 0, NULL in the _dev form: not wanted), dmean_dx[B*k*d],
 * dvar_dx[B*k*d] (0 where the variance was clipped: the derivative of the function as it is computed). */
int gpemu_gp_predict_grad(gpemu_model *m, int64_t B, const double *X, double *mean, double *var, double *dmean_dx,
                          double *dvar_dx);
int gpemu_gp_predict_grad_dev(gpemu_model *m, int64_t B, const double *dX, double *dmean, double *dvar,
                              double *ddmean_dx, double *ddvar_dx, void *stream);
/* Log-posterior and its gradient after a likelihood setup: lp[B], grad[B*d].  Rows outside the open box (a NaN
 * parameter included): lp = -inf, grad = 0.  A row whose lp is NaN (a covariance that is not positive definite, as in the
 * value call) has a NaN gradient.  lp is held to the same reference as the value-only call; it need not have
 * the same bits (the distances are taken directly from the coordinates, the sums run in another order). */
int gpemu_logpost_grad(gpemu_model *m, int64_t B, const double *X, double *lp, double *grad, int mode);
int gpemu_logpost_grad_dev(gpemu_model *m, int64_t B, const double *dX, double *dlp, double *dgrad, int mode,
                           void *stream);
/* ... summed over n_groups models on one device with one parameter box */
int gpemu_logpost_groups_grad(gpemu_model *const *models, int n_groups, int64_t B, const double *X, double *lp,
                              double *grad, int mode);
/* Which instances of the derivative path ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_grad_path {
  GPEMU_GRAD_PATH_CHUNK = 0,         /* one pass of up to 1024 rows of one group: K_*^T, V = W K_*^T, U = W^T V      */
  GPEMU_GRAD_PATH_LOGLIK,            /* grad_loglik_kernel: the likelihood with the adjoints a_p, b_p (per pass)     */
  GPEMU_GRAD_PATH_CONTRACT_8,        /* grad_contract_kernel, 8-wide rows (d <= 8), the log-posterior's gradient     */
  GPEMU_GRAD_PATH_CONTRACT_16,       /* ... 16-wide rows (d = 9 .. 16)                                               */
  GPEMU_GRAD_PATH_JACOBIAN_8,        /* grad_contract_kernel, 8-wide rows, the GP Jacobians                          */
  GPEMU_GRAD_PATH_JACOBIAN_16,       /* ... 16-wide rows                                                             */
  GPEMU_GRAD_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_GRAD_PATH_COUNT)) = the counters; returns GPEMU_GRAD_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_grad_path_counts(int64_t *out, int64_t n);

/* ---- GP fit: kernel matrix, Cholesky, log-marginal likelihood + gradient -------------------------
 * Replaces the arithmetic inside ref: emulation.py:169-172 (GaussianProcessRegressor(...).fit):
 * skl _gpr.py:537-652 log_marginal_likelihood(theta, eval_gradient=True) and :346-364 (final L_,
 * alpha_).  theta = log([l_1..l_d, (constant_value), (noise_level)]) in sklearn's order
 * (skl kernels.py:733-760, 861-866); jitter = GaussianProcessRegressor(alpha=...).  The optimiser
 * (L-BFGS-B + restarts, skl _gpr.py:299-337) stays on the host and calls gpemu_fit_lml.
 * A non-positive-definite kernel matrix returns > 0 (index + 1 of the failing pivot); sklearn
 * raises LinAlgError there (skl _gpr.py:350-358).
 * 1 <= d <= 16 (GPEMU_ERR_ARG beyond); d > 8 takes the 16-wide kernel-matrix and gradient instances.
 */
int gpemu_fit_create(gpemu_fit **out, int device, int64_t N, int64_t d, const double *X,
                     int kernel_kind, double nu, int has_const, int has_noise, double jitter);
int gpemu_fit_destroy(gpemu_fit *f);
/* lml and, if grad != NULL, d lml / d theta [n_theta] for target y[N] */
int gpemu_fit_lml(gpemu_fit *f, const double *y, const double *theta, int64_t n_theta, double *lml,
                  double *grad);
/* The same for n_problems (target, theta) pairs AT ONCE: ys[n_problems*N], thetas[n_problems*n_theta] ->
 * lml[n_problems], grad[n_problems*n_theta] (or NULL), info[n_problems] (0, or the failing pivot of a kernel matrix
 * that is not positive definite: that problem's lml / grad are meaningless, the others are valid).  Every launch of the
 * evaluation chain serves the whole batch: the k GPs x (1 + n_restarts) independent maximisations of
 * ref: emulation.py:169-172 (n_restarts: 50 in config/jet_substructure.yaml:80) advance in lock step. */
int gpemu_fit_lml_batch(gpemu_fit *f, int64_t n_problems, const double *ys, const double *thetas, int64_t n_theta,
                        double *lml, double *grad, int32_t *info);
/* L_out[N*N] (lower, zeros above), alpha_out[N], lml at theta; any output may be NULL */
int gpemu_fit_factor(gpemu_fit *f, const double *y, const double *theta, int64_t n_theta,
                     double *L_out, double *alpha_out, double *lml);
/* K_out[N*N] = kernel_(X) (+ jitter on the diagonal): skl kernels.py:1553-1582, 1708-1781 */
int gpemu_kernel_matrix(int device, int64_t N, int64_t d, const double *X, const double *theta,
                        int64_t n_theta, int kernel_kind, double nu, int has_const, int has_noise,
                        double jitter, double *K_out);
/* in-place lower Cholesky of a symmetric positive definite N x N matrix (scipy.linalg.cholesky
 * (lower=True), skl _gpr.py:349): blocked, MFMA f64 SYRK trailing updates */
int gpemu_cholesky(int device, int64_t N, double *A_inout);

/* ---- StandardScaler + PCA ---------------------------------------------------------------------
 * Replaces ref: emulation.py:109-118: scaler.fit_transform(Y) followed by
 * PCA(n_components, svd_solver='full').fit_transform (skl preprocessing/_data.py:1015-1051,
 * decomposition/_pca.py:544-702, svd_flip utils/extmath.py:944-952).  Y[N*F] row-major.
 * n_components <= 0 means min(N, F).  Outputs: scaler mean_/scale_/var_ [F], pca mean_ [F],
 * components_ [nc*F], explained_variance_ / _ratio_ [nc], Y_pca [N*nc] (= U S), flip_argmax [nc]
 * (index of the max-|.| entry of each component row: the svd_flip sign decision), n_sweeps.
 * Environment GPEMU_SVD_FLIP=u (read per call): the u-based decision of the scikit-learn the reference pins (ref:
 * pdm.lock:1998-1999 -> 1.3.0: per column of U; flip_argmax then holds the deciding ROW of U); default v: the rule of
 * scikit-learn >= 1.5 the goldens were made with.  Physical-space outputs do not depend on it.
 * Y must be finite: a NaN or an infinity anywhere in it is GPEMU_ERR_ARG (the error text names the element), decided
 * on the host before anything is copied or launched, as sklearn's PCA.fit raises.
 * The iteration stops after the first sweep in which no cosine between two columns exceeded 4 sqrt(m) eps
 * (m = max(N, F), eps = 2^-52).  If 60 sweeps do not get there the call returns GPEMU_PCA_NOT_CONVERGED (> 0, like the
 * info of gpemu_cholesky), the error text names the largest cosine of the last sweep and the tolerance, n_sweeps holds
 * the sweeps made and no other output is written. */
#define GPEMU_PCA_NOT_CONVERGED 1
int gpemu_pca_fit(int device, int64_t N, int64_t F, const double *Y, int64_t n_components,
                  double *scaler_mean, double *scaler_scale, double *scaler_var, double *pca_mean,
                  double *components, double *explained_variance, double *explained_variance_ratio,
                  double *Y_pca, int64_t *flip_argmax, int64_t *n_sweeps);

/* ---- truncation covariance ----------------------------------------------------------------------
 * Replaces ref: emulation.py:227-251 (compute_emulator_group_cov_unexplained):
 *   cov_out[F*F] = S_{>k} diag(explained_variance_{>k}) S_{>k}^T,  S = components^T,
 * components[n_comp*F] = pca.components_, explained_variance[n_comp], k = n_pc: one F x F x (n_comp - n_pc)
 * product on the f64 matrix cores.  The reference divides it by the batch size at use (emulation.py:531-532);
 * that stays with the callers (n_div). */
int gpemu_truncation_cov(int device, int64_t n_comp, int64_t F, int64_t n_pc, const double *components,
                         const double *explained_variance, double *cov_out);

/* ---- stretch-move ensemble sampler ------------------------------------------------------------
 * Replaces ref: mcmc.py:77-107, 187-204: emcee.EnsembleSampler(n_walkers, ndim, log_posterior,
 * pool=Pool()) with its default StretchMove(a=2) and the pool.map over walkers.  The ensemble,
 * the proposals, the accept/reject and the chain live on the device; the log-posterior is the sum
 * over the given emulation groups (block-diagonal covariance, ref: emulation.py:346-406), each with
 * n_div = 1 (emcee evaluates one walker per call).
 */
int gpemu_sampler_create(gpemu_sampler **out, gpemu_model *const *groups, int n_groups, int64_t W,
                         double a, uint64_t seed);
/* n_chains INDEPENDENT ensembles of W walkers each sharing the groups' emulators -- the reference's closure loop
 * (ref: steer_analysis.py:168-183: one MCMC per validation design point) as one batched run: the proposals of all
 * chains are stacked into the same cross-kernel / triangular-GEMM / likelihood launches.  Chain c draws from its own
 * Philox key seeds[c] and is, bit for bit, the chain gpemu_sampler_create(..., W, a, seeds[c]) produces on the data
 * vector c.  State, chain and counters are laid out chain after chain: walker c W + w. */
int gpemu_sampler_create_chains(gpemu_sampler **out, gpemu_model *const *groups, int n_groups, int64_t W,
                                double a, const uint64_t *seeds, int n_chains);
/* Parallel tempering: n_temps rungs of Wc walkers each, stacked as the chains above (rung t owns
 * walkers t Wc .. t Wc + Wc - 1 and draws its stretch moves from seeds[t]), all on the groups' ONE data vector
 * (GPEMU_ERR_STATE for a group set up with several).  Rung t accepts a proposal iff
 *     betas[t] == 1:  factor + ll' - ll > log u           (the untempered test, bit for bit)
 *     otherwise:      ll' finite and factor + betas[t] (ll' - ll) > log u,
 * and after step s, when swap_every > 0 and (s + 1) % swap_every == 0, walker column w of rungs t and t - 1
 * (t = n_temps-1 .. 1) exchange states iff both ll are finite and
 *     log u < (betas[t-1] - betas[t]) (ll[t][w] - ll[t-1][w]),  u from Philox(c = (w, 5, s_lo, s_hi), key = seeds[t]).
 * The stored chain row of a step is the state after the swaps; the stored log-probabilities are the untempered ll.
 * Ladder: 2 <= n_temps <= 64, betas[0] = 1 >= betas[1] >= ... >= betas[n_temps-1] >= 0 (else GPEMU_ERR_ARG).
 * gpemu_sampler_run_sharded, the peer transport and gpemu_sampler_step_host_rng return GPEMU_ERR_UNSUPPORTED. */
int gpemu_sampler_create_tempered(gpemu_sampler **out, gpemu_model *const *groups, int n_groups, int64_t Wc, double a,
                                  const uint64_t *seeds, const double *betas, int n_temps, int swap_every);
int gpemu_sampler_set_betas(gpemu_sampler *s, const double *betas /*[n_temps], validated as above*/);
/* swap counters since the last reset, per rung pair (t, t + 1) and column: accepted / attempted [(n_temps-1)*Wc] */
int gpemu_sampler_get_swap_counts(gpemu_sampler *s, int64_t *accepted, int64_t *attempted);
/* out[t] = mean of the stored log-likelihoods of rung t over chain rows [first, first + n) and its Wc walkers
 * (a fixed-order device reduction: the same bits on every call) -- the thermodynamic-integration input */
int gpemu_sampler_mean_loglik(gpemu_sampler *s, int64_t first, int64_t n, double *out /*[n_temps]*/);
int gpemu_sampler_destroy(gpemu_sampler *s);
/* The stream of every later call on the sampler; NULL = the first group's stream.  Waits for the stream in use so far.
 * The caller's stream must outlive its use; gpemu_sampler_run waits for it before it returns. */
int gpemu_sampler_set_stream(gpemu_sampler *s, void *stream);
/* X0[W*d]; logp0[W] or NULL to evaluate it (ref: mcmc.py:88, emcee State(initial_state)) */
int gpemu_sampler_set_state(gpemu_sampler *s, const double *X0, const double *logp0);
int gpemu_sampler_get_state(gpemu_sampler *s, double *X, double *logp);
int gpemu_sampler_reset(gpemu_sampler *s); /* emcee sampler.reset(): drop chain + acceptance (and swap) counts */
/* `steps` full stretch-move steps with device-side Philox randomness; returns 1 if any proposal's
 * log-probability was NaN (emcee raises ValueError). */
int gpemu_sampler_run(gpemu_sampler *s, int64_t steps, int store_chain);
/* One step with host-supplied randomness in emcee's draw order: inds[W] = the shuffled split,
 * then for split 0 (first ceil(W/2) entries) and split 1 (rest): zz = ((a-1)u+1)^2/a, rint in
 * [0, Nc), logu = log(u').  Used to replay a numpy RandomState stream. */
int gpemu_sampler_step_host_rng(gpemu_sampler *s, const int32_t *inds, const double *zz,
                                const int64_t *rint, const double *logu, int store_chain);
/* chain_out[n*W*d] (emcee get_chain()[first:first+n]), logp_out[n*W] (get_log_prob()) */
int gpemu_sampler_get_chain(gpemu_sampler *s, int64_t first, int64_t n, double *chain_out,
                            double *logp_out);
/* the same for walkers [w0, w0 + nw) only (a chain of a stacked sampler, a rung of a tempered one):
 * chain_out[n*nw*d], logp_out[n*nw] */
int gpemu_sampler_get_chain_walkers(gpemu_sampler *s, int64_t first, int64_t n, int64_t w0, int64_t nw,
                                    double *chain_out, double *logp_out);
int gpemu_sampler_get_counts(gpemu_sampler *s, int64_t *naccepted /*[W]*/, int64_t *iterations,
                             int64_t *chain_len);
/* The compacted half-step (one untempered chain, one group without correlated sources, halves of more than 128
 * proposals; GPEMU_NO_COMPACT=1 turns it off) evaluates only the proposals inside the prior box: live_proposals[0] of
 * the live_proposals[1] proposals it has formed since the sampler was created.  Both 0: nothing went that way. */
int gpemu_sampler_live_counts(gpemu_sampler *s, int64_t *live_proposals /*[2]*/);
/* the same over every sampler of this model, since gpemu_model_profile was last called (either way) */
int gpemu_model_live_counts(gpemu_model *m, int64_t *live_proposals /*[2]*/);
/* Walker-averaged normalised autocorrelation function of the stored chain rows [first, first + n_steps), walkers
 * [w0, w0 + nw) (a chain of a stacked sampler), lags [lag0, lag0 + n_lags): f_out[n_lags][d],
 *     f[l][dd] = 1/nw sum_w acf_(w,dd)[l] / acf_(w,dd)[0],  acf[l] = sum_t (x[t] - mean)(x[t + l] - mean),
 * i.e. emcee.autocorr.function_1d averaged as emcee.autocorr.integrated_time does (emcee 3.1.x, third party; call
 * site ref: mcmc.py:111-119 sampler.get_autocorr_time()).  The host asks for blocks of lags (lag0 a multiple of 16,
 * the first block at lag0 = 0) until Sokal's window closes, so the chain never has to leave HBM for it.
 * A block with lag0 > 0 continues the estimate of the last lag0 = 0 block: it must name the same (first, n_steps, w0,
 * nw), else GPEMU_ERR_ARG, and the chain must be the one that block read: after a run that stores, a reserve, a reset
 * or a restore of the sampler (what invalidates a gpemu_diag) the continuation returns GPEMU_ERR_STATE before any
 * launch and writes nothing; start again at lag 0.  n_lags <= min(4096, n_steps).
 * A series whose n_steps values are all equal (a walker that never moved in the range; every series at n_steps = 1)
 * centres to exact zeros and has acf[0] = 0: its parameter's f is NaN at every lag, the other parameters are not
 * touched.  A series with a non-finite value makes its parameter NaN as well. */
int gpemu_sampler_acf(gpemu_sampler *s, int64_t first, int64_t n_steps, int64_t w0, int64_t nw, int64_t lag0,
                      int64_t n_lags, double *f_out);
/* Phases of one step for the multi-GPU driver: every rank holds the whole ensemble and draws the
 * same randomness; rank r evaluates proposals [lo, hi) of the half (the log-probabilities land in
 * dnewlp_slice[0 .. hi-lo), typically the caller's all-gather input) and the ranks all-gather them
 * (RCCL, done by the caller on the sampler's stream) before every rank accepts identically; the
 * accept kernels also record the chain row when store_chain is set.  dnewlp_* are DEVICE pointers. */
int gpemu_sampler_reserve_chain(gpemu_sampler *s, int64_t additional_steps); /* grow the chain buffer once, up front */
int gpemu_sampler_begin_step(gpemu_sampler *s);
int gpemu_sampler_half_propose_eval(gpemu_sampler *s, int half, int64_t lo, int64_t hi,
                                    double *dnewlp_slice);
int gpemu_sampler_half_accept(gpemu_sampler *s, int half, const double *dnewlp_all, int store_chain);
int gpemu_sampler_end_step(gpemu_sampler *s, int store_chain);
int gpemu_sampler_check(gpemu_sampler *s); /* synchronise; 1 if a NaN log-probability was seen */

/* ---- RCCL communicator (one rank per GPU) and the sharded run in a single call ----------------
 * Replaces the multiprocessing pool of ref: mcmc.py:77-85 across GPUs.  librccl is bound with dlopen:
 * pass the path of the copy the process already uses (torch.distributed's) or NULL for "librccl.so".
 * Rank 0 obtains a 128-byte id with gpemu_comm_unique_id and ships it to the other ranks by any means
 * (torch.distributed broadcast, a file, MPI); every rank then calls gpemu_comm_create (collective). */
typedef struct gpemu_comm gpemu_comm;
int gpemu_comm_unique_id(const char *librccl_path, char *id_out128);
int gpemu_comm_create(gpemu_comm **out, int device, int rank, int world, const char *id128,
                      const char *librccl_path);
int gpemu_comm_destroy(gpemu_comm *c);
int gpemu_comm_dims(const gpemu_comm *c, int *rank, int *world);
/* all-gather of `count` doubles per rank, DEVICE pointers, enqueued on `stream` (NULL = the null stream); does not wait */
int gpemu_comm_all_gather(gpemu_comm *c, const double *dsend, double *drecv, int64_t count, void *stream);
/* `steps` stretch-move steps with each half's proposals split over the communicator's ranks (contiguous
 * blocks of ceil(n/world)); one 8-byte-per-proposal all-gather per half-step, no host round trip inside
 * the loop.  Same chain as gpemu_sampler_run on every rank.  emulate_world > 0 (one-rank communicator
 * only): evaluate just the share of rank 0 of an emulate_world-rank job -- a timing aid, not a valid chain; `c` may
 * be NULL then where the fused two-launch half-step applies (GPEMU_ERR_UNSUPPORTED otherwise). */
int gpemu_sampler_run_sharded(gpemu_sampler *s, gpemu_comm *c, int64_t steps, int store_chain,
                              int emulate_world);

/* One-off check of the peer exchange before a chain depends on it: this rank stores a token into every rank's buffer
 * through the pointers of gpemu_sampler_peer_import and waits (bounded, seconds) for all ranks' tokens in its own.
 * Collective in effect: call on every rank at about the same time (after a barrier).  0 = all tokens arrived. */
int gpemu_sampler_peer_selftest(gpemu_sampler *s);

/* ---- sharded run without a collective: peer stores over xGMI ---------------------------------------------
 * Every rank owns a small "gather" buffer; after evaluating its share of a half's proposals a rank stores each new
 * log-probability (8 bytes) straight into every rank's buffer.  Setup: each rank exports a 64-byte IPC handle of its
 * buffer (gpemu_sampler_peer_export), the ranks exchange the handles by any means (torch.distributed all_gather),
 * and each imports all of them (handles[world*64], its own entry is ignored).  gpemu_sampler_run_peer then runs
 * `steps` stretch-move steps with one front launch + one triangular GEMM per emulation group per half-step and no RCCL
 * call; same chain as gpemu_sampler_run on every rank.  Takes up to 8 emulation groups of up to 64 PCs each, one chain,
 * d <= 7 parameters (else GPEMU_ERR_UNSUPPORTED from the export / import: use gpemu_sampler_run_sharded).  The ranks must enter every call
 * together (a barrier on the host side): a peer's stores may arrive as soon as it has started.  A peer that does not
 * deliver within GPEMU_PEER_TIMEOUT_MS (5000) ends the run with GPEMU_ERR_STATE on every rank.
 * Replaces ref: mcmc.py:77-85 (the pool.map over walkers). */
int gpemu_sampler_peer_export(gpemu_sampler *s, char *handle_out64);
/* How many ranks of the job run their samplers on THIS device (default 1: one process per GPU, the production layout of
 * ref: mcmc.py:77-85's pool).  Call before gpemu_sampler_peer_import.  With one rank per device a fused launch needs no
 * residency rule (its waits only target workgroups dispatched before the waiters); with several ranks on one device
 * (one-GPU rehearsals) all their launches must be resident together, which the import then checks against the runtime's
 * occupancy figure -- failing with GPEMU_ERR_UNSUPPORTED (fall back to gpemu_sampler_run_sharded) instead of a time-out. */
int gpemu_sampler_peer_share(gpemu_sampler *s, int ranks_on_device);
int gpemu_sampler_peer_import(gpemu_sampler *s, int world, int rank, const char *handles);
int gpemu_sampler_run_peer(gpemu_sampler *s, int64_t steps, int store_chain);

/* Snapshot / restore of the chain state on the device (ensemble, log-probabilities, acceptance counters, step and
 * chain counters).  A block of steps whose peer exchange was lost (GPEMU_ERR_STATE from gpemu_sampler_run_peer) is
 * rerun from the snapshot over a collective transport: the random stream is counter based, so the rerun draws what the
 * failed attempt drew and the chain is that of an unbroken run.  Replaces nothing in the reference (its pool has no
 * recovery: ref: mcmc.py:77-107); part of the sharded run that replaces the pool. */
int gpemu_sampler_snapshot(gpemu_sampler *s);
int gpemu_sampler_restore(gpemu_sampler *s);

/* Launches so far, in this process, of the one-launch cross-kernel + triangular GEMM for small emulators (at most 256
 * design points and 32 PCs per group, at most 128 rows: csrc/k_halfstep.hip; what a sampler's half-step and a small
 * batched log-posterior take there).  For tests: which path ran.  GPEMU_NO_HALFSTEP=1 switches that path off. */
int64_t gpemu_halfstep_small_launches(void);

/* Launch decisions so far, in this process, per path of the predict / likelihood pipeline (host-side counters, one
 * relaxed increment per decision; nothing on the device).  For tests: which tiling, schedule and epilogue ran. */
enum gpemu_path {
  GPEMU_PATH_KSTAR_SMALL = 0,        /* cross-kernel, B <= KSTAR_SMALL_MAX columns (32-row workgroups)              */
  GPEMU_PATH_KSTAR_BIG,              /* cross-kernel, more columns (64-row workgroups)                               */
  GPEMU_PATH_KSTAR_KSTEPS2,          /* cross-kernel with 2 MFMA k-steps (d <= 7)                                    */
  GPEMU_PATH_KSTAR_KSTEPS3,          /* ... 3 k-steps (d = 8)                                                        */
  GPEMU_PATH_KSTAR_DIRECT,           /* the instance with the direct distance of near pairs (Matern 0.5, nu < 1)     */
  GPEMU_PATH_TRMM_SMALL_44,          /* small-batch triangular GEMM, trmm_vsq_small_kernel<4,4>                      */
  GPEMU_PATH_TRMM_SMALL_36,          /* ... <3,6> (at least 5 num_cu items)                                          */
  GPEMU_PATH_TRMM_SMALL_XCD,         /* ... XCD-aware placement of whole (PC, column block) groups                  */
  GPEMU_PATH_TRMM_SMALL_LEFTOVER,    /* ... every group left over (fewer than 8 groups): plain LPT                  */
  GPEMU_PATH_TRMM_SMALL_FEW_ITEMS,   /* ... fewer items than workers                                                 */
  GPEMU_PATH_TRMM_SMALL_FALLBACK,    /* ... more than ST_MAX_ITEMS items per worker: the large-batch kernel instead */
  GPEMU_PATH_TRMM_DMA_LPT,           /* large-batch trmm_vsq_dma_kernel, plain LPT schedule                          */
  GPEMU_PATH_TRMM_DMA_XCD,           /* ... XCD-aware schedule                                                       */
  GPEMU_PATH_TRMM_DMA_WHOLE,         /* ... the batch in one launch                                                  */
  GPEMU_PATH_TRMM_DMA_PIECES,        /* ... the batch split into pieces of trmm_piece_cols (counted once per batch)  */
  GPEMU_PATH_HALFSTEP_SMALL,         /* one-launch cross-kernel + GEMM for small emulators (k_halfstep.hip)          */
  GPEMU_PATH_HALFSTEP_GENERAL,       /* the same request on the general cross-kernel + GEMM launches                 */
  GPEMU_PATH_LOGLIK_LOWRANK,         /* loglik_lowrank_kernel / _lds_kernel                                          */
  GPEMU_PATH_LOGLIK_GROUPS,          /* loglik_groups_kernel                                                         */
  GPEMU_PATH_LOGLIK_TASKS_ONE,       /* loglik_tasks_kernel, one workgroup per proposal                              */
  GPEMU_PATH_LOGLIK_TASKS_MULTI,     /* ... several workgroups per proposal (tickets), at most 256 rows               */
  GPEMU_PATH_LOGLIK_TASKS_MULTI_BIG, /* ... several workgroups per proposal, more than 256 rows                       */
  GPEMU_PATH_PREDICT_PASS,           /* one pass of at most MAX_CHUNK (2048) rows of the predict pipeline            */
  GPEMU_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_PATH_COUNT)) = the counters; returns GPEMU_PATH_COUNT (or GPEMU_ERR_ARG for out == NULL, n < 0). */
int gpemu_path_counts(int64_t *out, int64_t n);

/* The same for the fit side (csrc/k_fit.hip: gpemu_fit_*, gpemu_kernel_matrix, gpemu_cholesky and the factorisations
 * of the model, likelihood and cross-validation setup that share its Cholesky and inverse).  A set of its own, so that
 * the predict / likelihood set above keeps its size and indices. */
enum gpemu_fit_path {
  GPEMU_FIT_PATH_KMAT = 0,           /* kernel matrix, kmat_kernel<8, false> (RBF, Matern 0.5 / 1.5 / 2.5)            */
  GPEMU_FIT_PATH_KMAT_NU,            /* ... kmat_kernel<8, true> (Matern of general nu)                               */
  GPEMU_FIT_PATH_CHOL_PANEL,         /* blocked Cholesky: one fused chol_panel_kernel launch per 256-wide panel       */
  GPEMU_FIT_PATH_CHOL_STEPS,         /* ... one panel of the three-launch steps (diagonal factor, solve, update)      */
  GPEMU_FIT_PATH_CHOL_LOOKAHEAD,     /* ... one look-ahead update of the columns beyond the next panel, side stream   */
  GPEMU_FIT_PATH_CHOL_HEADS_ONE_XCD, /* ... one fused panel launch with its four heads placed on one XCD              */
  GPEMU_FIT_PATH_TRTRI_RAGGED,       /* triangular inverse: one merge of a ragged pair (second block shorter)        */
  GPEMU_FIT_PATH_GRAD,               /* LML gradient, lml_grad_kernel<8, false>                                       */
  GPEMU_FIT_PATH_GRAD_NU,            /* ... lml_grad_kernel<8, true>                                                  */
  GPEMU_FIT_PATH_BATCH,              /* one fit evaluation of more than one problem at once                           */
  GPEMU_FIT_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_FIT_PATH_COUNT)) = the counters; returns GPEMU_FIT_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_fit_path_counts(int64_t *out, int64_t n);

/* Which instances of padded width 16 (models and fit handles of 9 to 16 parameters) ran.  Their launches still count in
 * the sets above where those do not name a width (KSTAR_SMALL / _BIG, KSTAR_DIRECT, HALFSTEP_GENERAL, the LOGLIK_* and
 * TRMM_* entries, the fit's CHOL_* / TRTRI_* / BATCH); KSTAR_KSTEPS2 / _KSTEPS3, FIT_PATH_KMAT* and FIT_PATH_GRAD* count
 * the 8-wide instances only, and their 16-wide counterparts count here. */
enum gpemu_wide_path {
  GPEMU_WIDE_PATH_KSTAR_KSTEPS3 = 0, /* cross-kernel, 16-wide rows, 3 MFMA k-steps (d = 9 .. 11)                      */
  GPEMU_WIDE_PATH_KSTAR_KSTEPS4,     /* ... 4 k-steps (d = 12 .. 15)                                                  */
  GPEMU_WIDE_PATH_KSTAR_KSTEPS5,     /* ... 5 k-steps (d = 16)                                                        */
  GPEMU_WIDE_PATH_FIT_KMAT,          /* kernel matrix, kmat_kernel<16, ..>                                            */
  GPEMU_WIDE_PATH_FIT_GRAD,          /* LML gradient, lml_grad_kernel<16, ..>                                         */
  GPEMU_WIDE_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_WIDE_PATH_COUNT)) = the counters; returns GPEMU_WIDE_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_wide_path_counts(int64_t *out, int64_t n);

/* The launches of the correlated-source likelihood (gpemu_likelihood_setup_cov).  A set of its own: the sets above keep
 * their sizes and indices. */
enum gpemu_src_path {
  GPEMU_SRC_PATH_CORRECTION = 0,     /* source_correction_kernel: the per-proposal Woodbury term of the sources       */
  GPEMU_SRC_PATH_SETUP_COV,          /* a likelihood setup that read a dense within-observable covariance            */
  GPEMU_SRC_PATH_SETUP_SOURCES,      /* a likelihood setup with n_src > 0                                             */
  GPEMU_SRC_PATH_EXACT_COV,          /* loglik_exact_kernel with a dense within-observable covariance                */
  GPEMU_SRC_PATH_SETUP_BLOCKED,      /* an observable block of > 256 features, with cov or sources, through the blocked
                                        setup (lik_z_kernel / lik_gram_kernel)                                        */
  GPEMU_SRC_PATH_CORRECTION_K64,     /* source_correction_kernel with a group of 33 .. 64 PCs (over 64 KB of LDS)     */
  GPEMU_SRC_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_SRC_PATH_COUNT)) = the counters; returns GPEMU_SRC_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_src_path_counts(int64_t *out, int64_t n);

/* ---- exact order statistics and posterior-predictive summaries ------------------------------------
 * Replaces ref: mcmc.py credible_interval (np.quantile over the chain; call sites ref: plot_qhat.py:102-109) and the
 * per-bin bands of ref: plot_mcmc.py:343-371 (_plot_posterior_observables: predict on draws of the chain, then
 * quantiles per feature), for the WHOLE chain instead of a few hundred draws of it.
 *
 * Selection: out[r*n_ranks + i] = the ranks[i]-th smallest element (0-based) of row r of V[R*S] -- an element of the
 * input, equal as a double to np.sort(V[r])[ranks[i]].  +0 and -0 compare equal, so the sign of a returned zero is not
 * specified; a row that holds a NaN returns NaN for every rank (np.quantile); +-inf order as usual.  Radix select on the
 * order-preserving 64-bit key of a double, eight 8-bit passes shared by all ranks of a row, whatever the data (a row of
 * equal values takes the same passes).  Selection is exact and its counters are integers: the result bits do not depend
 * on the grid, on the scratch or on the run.  R, S, n_ranks >= 1 and every rank in [0, S), else GPEMU_ERR_ARG.
 * The _dev form reads element j of row r at dV[r*row_stride + j*elem_stride] (strides in doubles, > 0: a parameter of
 * the device chain [steps][W][d] is the "row" j with row_stride 1, elem_stride d); ranks[] is a HOST array, dout
 * [R*n_ranks] a device array; works on `stream` (NULL = the null stream) and waits for it before it returns (its scratch
 * goes with the call). */
int gpemu_select(int device, int64_t R, int64_t S, const double *V, int64_t n_ranks, const int64_t *ranks, double *out);
int gpemu_select_dev(int device, int64_t R, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                     int64_t n_ranks, const int64_t *ranks, double *dout, void *stream);

/* Summaries over the S rows of X[S*d] of the group's prediction for one sample (ref: emulation.py:466-548, n_div = 1):
 * with mu_f(theta) = central_value and sigma2_f(theta) = the diagonal of cov (gpemu_model_cross_validate's `variance`),
 *   mean[F]                 mean over the rows of mu_f
 *   var_param[F]            population variance (ddof 0) of mu_f, two passes
 *   var_emu[F]              mean over the rows of sigma2_f  (var_param + var_emu = the predictive variance)
 *   order_stats[F*n_ranks]  order statistic ranks[i] of mu_f, as gpemu_select
 * Each output may be NULL; n_ranks = 0 skips the selection.  Rows are not checked against a prior box; the host form
 * refuses non-finite rows (GPEMU_ERR_ARG).  The F x F covariances and the S x F variances are never formed.
 * workspace_bytes = 0: half of the free device memory.  Resident: the PC means and variances, 16*S*k bytes, and
 * GPEMU_POSTPRED_FIXED_BYTES of scratch; what is left holds the feature-major central values, 8*S bytes per feature, for
 * all features or for blocks of a multiple of 16 of them.  If not even 16 features fit: GPEMU_ERR_HIP, sizes in
 * the error text.  Every sum over rows runs over chunks fixed by the row index: the results, bit for bit, do not depend
 * on workspace_bytes, on the feature blocks or on the run.
 * _dev: row r is read at dX + ((r / block_rows)*block_stride_rows + r % block_rows)*d, S = n_blocks*block_rows -- the
 * sampler's chain in place: thinned by steps, one rung of a tempered chain, one chain of a stacked sampler.  Outputs
 * are device arrays, ranks[] a HOST array; works on `stream` (NULL = the model's) and waits for it before returning. */
#define GPEMU_POSTPRED_FIXED_BYTES (32ll << 20)
int gpemu_posterior_predictive(gpemu_model *m, int64_t S, const double *X, int64_t n_ranks, const int64_t *ranks,
                               int64_t workspace_bytes, double *mean, double *var_param, double *var_emu,
                               double *order_stats);
int gpemu_posterior_predictive_dev(gpemu_model *m, const double *dX, int64_t n_blocks, int64_t block_rows,
                                   int64_t block_stride_rows, int64_t n_ranks, const int64_t *ranks,
                                   int64_t workspace_bytes, double *dmean, double *dvar_param, double *dvar_emu,
                                   double *dorder_stats, void *stream);
/* Device address of step `first` of the stored chain [steps][W][d] and the number of steps from there on; valid until
 * the next run, reserve, reset or restore of the sampler.  Waits for the sampler's stream. */
int gpemu_sampler_chain_ptr(gpemu_sampler *s, int64_t first, const double **dchain, int64_t *n_steps);
/* Which forms of the two ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_postpred_path {
  GPEMU_POSTPRED_PATH_WHOLE = 0,        /* a reduction whose features all fit the workspace at once                 */
  GPEMU_POSTPRED_PATH_FEATURE_BLOCKED,  /* ... that went through the workspace in blocks of features                */
  GPEMU_POSTPRED_PATH_FEATURE_BLOCK,    /* one block of features: projection, moments, selection                    */
  GPEMU_POSTPRED_PATH_SELECT_PASS,      /* one histogram + scan pass of the radix select                            */
  GPEMU_POSTPRED_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_POSTPRED_PATH_COUNT)) = the counters; returns GPEMU_POSTPRED_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_postpred_path_counts(int64_t *out, int64_t n);

/* ---- Hamiltonian Monte Carlo -----------------------------------------------------------------------
 * W independent chains in lock step on the gradient of gpemu_logpost_groups_grad; chain w is "walker" w of the
 * sampler's chain layout, so gpemu_sampler_run, _set_state (logp0 is not read: lp and the gradient of the start come
 * from the gradient path), _get_state, _reset, _get_chain*, _get_counts, _acf, _chain_ptr, _snapshot and _restore work
 * on the handle.  One iteration: eps_w = eps (1 + jitter (2 u - 1)); p = z / sqrt(minv); n_leapfrog leapfrog steps with
 * reflection at the faces of the prior box; accept iff log u' < H_old - H_new, H = -lp + 1/2 sum minv p^2.  A
 * non-finite H_new or H_new - H_old > 1000 (away from a face, where lp = -inf is the ordinary reject) is a rejected
 * divergence.  Inverse metric: diagonal, default (hi - lo)^2 / 12.  Random stream: Philox4x32-10 keyed by seed, a
 * chain's draws depend on its index and the step only: chains 0 .. n-1 of a larger sampler are those of a smaller one.
 * Declines (GPEMU_ERR_UNSUPPORTED) at create, before any launch, whatever gpemu_logpost_grad declines; on the handle:
 * gpemu_sampler_run_sharded, the peer transport, the phase calls, gpemu_sampler_step_host_rng, the tempered setters. */
int gpemu_sampler_create_hmc(gpemu_sampler **out, gpemu_model *const *groups, int n_groups, int64_t W, int n_leapfrog,
                             double eps0, double jitter, uint64_t seed);
int gpemu_sampler_hmc_set_metric(gpemu_sampler *s, const double *minv /*[d], > 0*/);
int gpemu_sampler_hmc_get_metric(gpemu_sampler *s, double *minv /*[d]*/);
/* the step size; with the adaptation on, setting it restarts the averaging there */
int gpemu_sampler_hmc_set_step_size(gpemu_sampler *s, double eps);
int gpemu_sampler_hmc_get_step_size(gpemu_sampler *s, double *eps); /* waits for the sampler's stream */
/* Dual averaging of the step size (Hoffman & Gelman 2014: gamma 0.05, t0 10, kappa 0.75, mu = log(10 eps)), updated on
 * the device after every iteration from the chains' mean accept probability.  on: (re)start the averaging at the
 * current step size; off: freeze the step size at the averaged one. */
int gpemu_sampler_hmc_adapt(gpemu_sampler *s, int on, double target_accept);
/* one iteration with the caller's momenta p0[W*d], log-uniforms logu[W] and step sizes eps_w[W] */
int gpemu_sampler_hmc_step_host_rng(gpemu_sampler *s, const double *p0, const double *logu, const double *eps_w,
                                    int store_chain);
/* per-chain accepts and divergences [W] since the last reset (either may be NULL), the mean over iterations and
 * chains of min(1, exp(H_old - H_new)) since then, and that of the last iteration alone */
int gpemu_sampler_hmc_stats(gpemu_sampler *s, int64_t *naccepted, int64_t *divergences, double *mean_accept_prob,
                            double *last_accept_prob);
/* what iteration `step` of the device stream draws (for tests): the normals z[W*d] and the two uniforms [W] */
int gpemu_sampler_hmc_draws(gpemu_sampler *s, uint64_t step, double *z, double *u_accept, double *u_jitter);
/* Pooled mean[d] and variance[d] (divisor: the number of points) of steps [first, first + n) of ANY sampler's stored
 * chain, all walkers, computed where the chain lies: two passes, sums in a fixed order. */
int gpemu_sampler_chain_moments(gpemu_sampler *s, int64_t first, int64_t n, double *mean, double *var);
/* Which launches of the HMC sampler ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_hmc_path {
  GPEMU_HMC_PATH_BEGIN = 0,         /* momentum draw (Philox), first kick, drift, reflection                         */
  GPEMU_HMC_PATH_BEGIN_HOST_RNG,    /* ... with the caller's momenta                                                 */
  GPEMU_HMC_PATH_LEAPFROG,          /* the fused kick-kick-drift-reflect between two gradient evaluations            */
  GPEMU_HMC_PATH_FINISH,            /* last kick, energies, accept, counters, state and chain row                    */
  GPEMU_HMC_PATH_ADAPT,             /* mean accept probability + dual-averaging update                               */
  GPEMU_HMC_PATH_ACCEPT_MEAN,       /* mean accept probability alone (adaptation off)                                */
  GPEMU_HMC_PATH_MOMENTS,           /* gpemu_sampler_chain_moments                                                   */
  GPEMU_HMC_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_HMC_PATH_COUNT)) = the counters; returns GPEMU_HMC_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_hmc_path_counts(int64_t *out, int64_t n);

/* ---- chain diagnostics: exact ranks, rank-normalised split-Rhat, bulk / tail ESS -----------------------
 * The convergence statistics of Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021), computed where the chain lies.
 * The reference's only convergence statistic is emcee's integrated autocorrelation time (ref: mcmc.py:111-119), which
 * gpemu_sampler_acf covers; these compare chains with each other.
 *
 * Ranks: ranks_out[r*S + j] = the average 1-based rank of element j among the S elements of row r, as a double equal
 * to scipy.stats.rankdata(V[r], 'average')[j].  -0 and +0 are tied; a row that holds a NaN returns NaN everywhere;
 * +-inf order as usual.  Key-only LSD radix sort of the order-preserving 64-bit keys (eight stable 8-bit passes: per-tile
 * digit histograms, a scan over (digit, tile), a stable scatter), then the lower and upper bound of every element in
 * the sorted keys: rank = (lo + hi + 1) / 2.  All counters are integers and the sorted key array is unique: the bits
 * do not depend on the grid, on the batches or on the run.  R, S >= 1 and S < 2^31, else GPEMU_ERR_ARG.
 * _dev addresses as gpemu_select_dev does (element j of row r at dV[r*row_stride + j*elem_stride]); dranks is a dense
 * device array [R][S].  Rows go through the workspace in batches, 16*S + 1024*ceil(S/2048) + 4 bytes per row;
 * workspace_bytes = 0: half of the free device memory.  If not one row fits: GPEMU_ERR_HIP, sizes in the error text.
 * stream NULL = the null stream; waits for it before returning. */
int gpemu_rank(int device, int64_t R, int64_t S, const double *V, double *ranks_out);
int gpemu_rank_dev(int device, int64_t R, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                   double *dranks, int64_t workspace_bytes, void *stream);

/* A segment x[n][M][d] of a chain (n stored steps, M chains or walkers) and its split, transformed series.
 * N = floor(n / 2) >= 4 (else GPEMU_ERR_ARG); split chain (h, m) is half h of chain m: rows [0, N) and [n - N, n).
 * _create copies a host chain [n][W][d]; _create_dev borrows walkers [w0, w0 + nw) of a device chain whose steps are
 * step_stride doubles apart and whose rows are [..][d] (the pointer is to walker 0 of the first step);
 * gpemu_sampler_diag_create borrows steps first, first + thin, ... (n of them) of the stored chain in place: valid until
 * the next run that stores, reserve, reset or restore of the sampler, GPEMU_ERR_STATE from every call after that.
 * Memory: one buffer of n*nw*d doubles (the transformed series Y, or the dense segment while a median or quantile is
 * selected), the select's and the sort's scratch for a batch of parameters (gpemu_rank_dev's bound with S = 2*N*nw,
 * within workspace_bytes; 0 = half of the free memory) and the lag-block scratch of gpemu_sampler_acf.
 * _create_dev works on `stream` (NULL = the null stream) and waits for it; the handle's later calls run on that stream
 * and wait for it, so it must outlive the handle.
 *
 * gpemu_diag_transform writes Y[N][2*nw*d], series (h*nw + w)*d + dd, for one of the kinds below and returns the split
 * chains' moments, sums in a fixed order (two passes, then a tree): grand_mean[d] = the mean of the 2*nw chain means,
 * mean_var[d] = W, the mean of the ddof-1 chain variances, var_of_means[d] = b, the ddof-1 variance of the chain means.
 *   IDENTITY        x
 *   RANK_Z          normcdfinv((r - 3/8) / (S + 1/4)), r the pooled average rank among the S = 2*N*nw split values
 *   FOLDED_RANK_Z   the same of |x - median|, the np.median of the pooled unsplit segment (gpemu_select)
 *   INDICATOR_LE    1[x <= q], q = np.quantile(pooled unsplit segment, prob) as gpemu.select.quantile computes it
 * gpemu_diag_range: min[d] and max[d] over the current Y (exact); gpemu_diag_series: Y itself, Y_out[N*2*nw*d] on the
 * host.  gpemu_diag_acov: g_out[l*d + dd] = the mean over the
 * 2*nw split chains of the biased autocovariance 1/N sum_t c[t] c[t + l], c = y - chain mean, of the current Y, for
 * lags [lag0, lag0 + n_lags): gpemu_sampler_acf's protocol (lag0 a multiple of 16, n_lags <= min(4096, N), the first
 * block after a transform at lag 0).  gpemu_diag_pooled: mean, ddof-1 standard deviation, np.median, min and max of the
 * pooled unsplit segment, [d] each (any may be NULL); a parameter with a NaN gives NaN.  Arguments are checked before
 * any launch.  The bits depend on (n, nw, d) and the values alone. */
typedef struct gpemu_diag gpemu_diag;
#define GPEMU_DIAG_IDENTITY 0
#define GPEMU_DIAG_RANK_Z 1
#define GPEMU_DIAG_FOLDED_RANK_Z 2
#define GPEMU_DIAG_INDICATOR_LE 3
int gpemu_diag_create(gpemu_diag **out, int device, const double *chain, int64_t n, int64_t W, int d);
int gpemu_diag_create_dev(gpemu_diag **out, int device, const double *dchain, int64_t n, int64_t step_stride, int64_t w0,
                          int64_t nw, int d, int64_t workspace_bytes, void *stream);
int gpemu_sampler_diag_create(gpemu_diag **out, gpemu_sampler *s, int64_t first, int64_t n, int64_t thin, int64_t w0,
                              int64_t nw);
int gpemu_diag_transform(gpemu_diag *h, int kind, double prob, double *grand_mean, double *mean_var,
                         double *var_of_means);
int gpemu_diag_range(gpemu_diag *h, double *min, double *max);
int gpemu_diag_series(gpemu_diag *h, double *Y_out);
int gpemu_diag_acov(gpemu_diag *h, int64_t lag0, int64_t n_lags, double *g_out);
int gpemu_diag_pooled(gpemu_diag *h, double *mean, double *sd_ddof1, double *median, double *min, double *max);
void gpemu_diag_destroy(gpemu_diag *h);
/* Which launches of the diagnostics ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_diag_path {
  GPEMU_DIAG_PATH_SORT_PASS = 0,    /* one histogram + scan + scatter pass of the radix sort, for one batch of rows    */
  GPEMU_DIAG_PATH_RANK_LOOKUP,      /* the lower / upper bound lookup of one batch of rows                            */
  GPEMU_DIAG_PATH_TRANSFORM,        /* one gpemu_diag_transform                                                       */
  GPEMU_DIAG_PATH_ACOV_BLOCK,       /* one lag block of gpemu_diag_acov                                               */
  GPEMU_DIAG_PATH_ROW_BATCH,        /* one batch of rows through the sort's workspace                                 */
  GPEMU_DIAG_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_DIAG_PATH_COUNT)) = the counters; returns GPEMU_DIAG_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_diag_path_counts(int64_t *out, int64_t n);

/* ---- global (Sobol') sensitivity of the emulators ----------------------------------------------------
 * The variance-based counterpart of the local sensitivities the reference takes by a 10 % forward difference at one
 * point (ref: plot_qhat.py:172-258; the analytic Jacobian: gpemu_gp_predict_grad): over base matrices A, B [n*d]
 * (rows in the prior box) the pick-freeze rows AB_i = A with column i from B.
 *
 * gpemu_gp_mean_pick_freeze: Z_out[(d+2)*n*k] = the PC means (ref: emulation.py:494-499, the mean of
 * GaussianProcessRegressor.predict) of the rows of A (slot 0), of B (slot 1) and of AB_0 .. AB_(d-1) (slots 2 ..),
 * Z_out[(slot*n + r)*k + p].  K_* is never stored and the variance GEMM is not run.
 *
 * gpemu_sobol_moments: row r belongs to batch floor(r*n_batches / n).  Per batch t, about the pivot c (returned: the
 * mean of z over the first min(n, 1024) rows of A and of B), with zA, zB the means of the batch's rows and
 * D_i = z(AB_i) - z(A):
 *   count[T]        rows of the batch
 *   sumA, sumB[T*k] sum (zA - c), sum (zB - c)
 *   C2[T*k*k]       sum (zA - c)(zA - c)^T + sum (zB - c)(zB - c)^T
 *   sumD[T*d*k]     per i: sum D_i
 *   M[T*d*k*k]      per i: sum (zB - c) D_i^T       (Saltelli et al. 2010: the first-order index)
 *   D[T*d*k*k]      per i: sum D_i D_i^T            (Jansen 1999: the total-effect index)
 * from which gpemu.sensitivity.indices_from_moments forms the indices of every feature as k x k quadratic forms (the
 * back-projection is linear, ref: emulation.py:516-548: no n x F array exists).  Every sum runs over slices of the
 * rows fixed by n and n_batches and is added in a fixed order, no floating-point atomics: the results, bit for bit, do
 * not depend on workspace_bytes or on the run.  workspace_bytes bounds the chunk of PC means, 8*(d+2)*k bytes per row
 * (0: half of the free device memory; at least one slice of min(n, 256) rows, else GPEMU_ERR_HIP); the per-slice
 * partial sums are allocated beside it.  n >= 1, 1 <= n_batches <= n, a model with d <= 16 and k <= 64, else
 * GPEMU_ERR_ARG; the host forms refuse non-finite rows (GPEMU_ERR_ARG) before any launch.
 * _dev: dA, dB are device arrays, the outputs HOST arrays; works on `stream` (NULL = the model's) and waits for it. */
int gpemu_gp_mean_pick_freeze(gpemu_model *m, int64_t n, const double *A, const double *B, double *Z_out);
int gpemu_sobol_moments(gpemu_model *m, int64_t n, const double *A, const double *B, int64_t n_batches,
                        int64_t workspace_bytes, double *pivot, int64_t *count, double *sumA, double *sumB, double *C2,
                        double *sumD, double *M, double *D);
int gpemu_sobol_moments_dev(gpemu_model *m, int64_t n, const double *dA, const double *dB, int64_t n_batches,
                            int64_t workspace_bytes, double *pivot, int64_t *count, double *sumA, double *sumB,
                            double *C2, double *sumD, double *M, double *D, void *stream);
/* Which launches of the two ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_sobol_path {
  GPEMU_SOBOL_PATH_CALL = 0,   /* one gpemu_sobol_moments[_dev]                                                       */
  GPEMU_SOBOL_PATH_CHUNK,      /* one chunk of rows through the workspace                                             */
  GPEMU_SOBOL_PATH_WHOLE,      /* a call whose rows all fitted one chunk                                              */
  GPEMU_SOBOL_PATH_DP8,        /* a launch of the mean kernel, 8-wide instance (d <= 8)                               */
  GPEMU_SOBOL_PATH_DP16,       /* ... 16-wide instance (9 <= d <= 16)                                                 */
  GPEMU_SOBOL_PATH_KIND0,      /* ... by base kernel: RBF / nu = inf, then Matern 0.5, 1.5, 2.5, general nu           */
  GPEMU_SOBOL_PATH_KIND1,
  GPEMU_SOBOL_PATH_KIND2,
  GPEMU_SOBOL_PATH_KIND3,
  GPEMU_SOBOL_PATH_KIND4,
  GPEMU_SOBOL_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_SOBOL_PATH_COUNT)) = the counters; returns GPEMU_SOBOL_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_sobol_path_counts(int64_t *out, int64_t n);

/* ---- second-order Sobol' indices: the pair rows AB_ij --------------------------------------------------
 * Where T_if - S_if is clearly above zero, parameter i acts on bin f through interactions; these moments say with
 * which other parameter.  For a pair i < j the row AB_ij is row A with columns i and j from B, and with the notation
 * above (z the PC means, c the returned pivot) D_ij = z(AB_ij) - z(A).  Per batch t, about the pivot:
 *   sumD2[T*P*k]    per pair: sum D_ij
 *   M2[T*P*k*k]     per pair: sum (zB - c) D_ij^T    (the first-order estimator applied to the pair row)
 *   D2[T*P*k*k]     per pair: sum D_ij D_ij^T        (Jansen's, for the total effect of the pair)
 * in the order of `pairs` [n_pairs][2] (i < j < d, no repeats).  Re-centred on the host exactly as M_i and D_i are
 * (gpemu.sensitivity.pair_indices_from_moments), per feature f with V_f the variance:
 *   closed pair index   Sc_ij,f = s_f^2 c_f^T M_ij c_f / V_f          (Saltelli et al. 2010)
 *   interaction index   S_ij,f  = Sc_ij,f - S_i,f - S_j,f
 *   total of the pair   T_ij,f  = s_f^2 c_f^T D_ij c_f / (2 V_f)      (Jansen 1999)
 * The first eight outputs are gpemu_sobol_moments' of the same arguments, byte for byte.  Every pair distance is a sum
 * of non-negative terms (for a fixed i the kernel walks j upward with a running sum; nothing is formed by
 * cancellation); a row with a_i == b_i IS the row AB_j and takes that row's mean as the first-order pass computed it,
 * one with a_j == b_j that of AB_i, one with both that of A: B = A gives exact zeros in sumD2, M2, D2, and a column B
 * shares with A gives the first-order row's M and D, bit for bit.  The sums run over the slices of gpemu_sobol_moments in its fixed order: the results, bit
 * for bit, do not depend on workspace_bytes, on the run, or on which other pairs were asked for.  workspace_bytes
 * bounds the chunk of PC means, 8*(d+2+n_pairs)*k bytes per row (0: half of the free device memory; at least one slice
 * of min(n, 256) rows, else GPEMU_ERR_HIP).  GPEMU_ERR_ARG, before any launch or allocation, for n < 1, n_batches
 * outside 1 .. n, n_pairs < 1, an index outside 0 .. d-1, i >= j, a repeated pair, non-finite rows, and a model of
 * d == 1.  A, B and every output are HOST arrays; the call works on the model's stream and waits for it. */
int gpemu_sobol_moments_pairs(gpemu_model *m, int64_t n, const double *A, const double *B, int64_t n_batches,
                              int64_t n_pairs, const int32_t *pairs, int64_t workspace_bytes, double *pivot,
                              int64_t *count, double *sumA, double *sumB, double *C2, double *sumD, double *M, double *D,
                              double *sumD2, double *M2, double *D2);
/* Which launches of gpemu_sobol_moments_pairs ran.  A set of its own: the other sets keep their sizes and indices, and
 * the call does not move gpemu_sobol_path_counts. */
enum gpemu_sobol_pairs_path {
  GPEMU_SOBOL_PAIRS_PATH_CALL = 0,   /* one gpemu_sobol_moments_pairs                                                 */
  GPEMU_SOBOL_PAIRS_PATH_CHUNK,      /* one chunk of rows through the workspace                                       */
  GPEMU_SOBOL_PAIRS_PATH_WHOLE,      /* a call whose rows all fitted one chunk                                        */
  GPEMU_SOBOL_PAIRS_PATH_DP8,        /* a launch of the pair-row mean kernel, 8-wide instance (d <= 8)                */
  GPEMU_SOBOL_PAIRS_PATH_DP16,       /* ... 16-wide instance (9 <= d <= 16)                                           */
  GPEMU_SOBOL_PAIRS_PATH_KIND0,      /* ... by base kernel: RBF / nu = inf, then Matern 0.5, 1.5, 2.5, general nu     */
  GPEMU_SOBOL_PAIRS_PATH_KIND1,
  GPEMU_SOBOL_PAIRS_PATH_KIND2,
  GPEMU_SOBOL_PAIRS_PATH_KIND3,
  GPEMU_SOBOL_PAIRS_PATH_KIND4,
  GPEMU_SOBOL_PAIRS_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_SOBOL_PAIRS_PATH_COUNT)) = the counters; returns GPEMU_SOBOL_PAIRS_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_sobol_pairs_path_counts(int64_t *out, int64_t n);

/* ---- marginal posteriors: histograms, highest-density intervals, kernel density ----------------------
 * The data of a corner plot from the WHOLE chain, where it lies: what ref: plot_mcmc.py _plot_posterior_pairplot draws
 * from a subsample (a Gaussian KDE of every parameter, every pair of parameters, the shaded highest-density interval)
 * and the narrowest-window rule of ref: mcmc.py:150-158 (credible_interval, interval_type 'hpd').
 *
 * Histograms: over the S rows of X[S*d], 1 <= d <= 16,
 *   hist1[d*nb1]           hist1[j*nb1 + b] = the rows with edges1[j][b] <= x_j < edges1[j][b+1], the last bin closed on
 *                          the right: np.histogram(x[:, j], bins=edges1[j])
 *   hist2[n_pairs*nb2*nb2] for the pairs (i, j), i < j, in row-major order, [pair][bin of x_i][bin of x_j]:
 *                          np.histogram2d(x[:, i], x[:, j], bins=[edges2[i], edges2[j]]); NULL allowed for d = 1
 *   n_inside1[d]           the rows counted in hist1[j]
 * edges1[d*(nb1+1)] and edges2[d*(nb2+1)] are HOST arrays in both forms, every row finite and strictly increasing (else
 * GPEMU_ERR_ARG).  The bin is guessed from (x - e0) / (eN - e0) * nb and corrected against the edges themselves, so a
 * value on an edge is counted as numpy counts it; rows outside [e0, eN] and NaN are not counted; -0 = +0.  One sweep
 * over the rows fills, per workgroup, private 16-bit counters in LDS (two to a word, LDS integer atomics; a workgroup
 * takes at most 65280 rows, so no counter overflows) for a group of pairs and, where they fit beside the last group,
 * the 1-D histograms; a row's d doubles are loaded once per sweep and every bin index is found once.  Non-zero counters
 * are added to the 64-bit outputs with global integer atomics.  Sweeps: ceil(n_pairs / floor(group_counters / nb2^2)),
 * plus one where the d*nb1 1-D counters do not fit beside the last group (and d = 1: one).  group_counters = 0: 73728
 * (144 KiB); otherwise max(nb1, nb2^2) <= group_counters <= 73728.  Counters are integers: the result does not depend
 * on the grid, on group_counters or on the run.  1 <= nb1 <= 4096, 1 <= nb2 <= 256, 1 <= S < 2^31, else GPEMU_ERR_ARG,
 * before any launch.
 * _dev: row r is read at dX + ((r / block_rows)*block_stride_rows + r % block_rows)*d, S = n_blocks*block_rows, as
 * gpemu_posterior_predictive_dev; the outputs are device arrays.
 *
 * Highest-density intervals: with s the sorted row r of V[R*S] and, per level l, n_out[l] in [1, S] points left outside,
 *   i* = the smallest i in [0, n_out) that minimises s[S - n_out + i] - s[i] (the difference rounded as a double),
 *   out[(r*n_levels + l)*2 + {0, 1}] = s[i*], s[S - n_out + i*]
 * -- elements of the input (a zero may come back as +0).  A row that holds a NaN, or whose smallest or largest element
 * is infinite, returns NaN for both ends at every level.  The rows are sorted by gpemu_rank_dev's radix sort, in batches
 * that fit workspace_bytes (16*S + 1024*ceil(S/2048) + 4 bytes per row, and 16 bytes per 4096 windows and level beside
 * it; 0 = half of the free device memory; if not one row fits: GPEMU_ERR_HIP, sizes in the error text); the window is a
 * reduction over the sorted keys on the key (width, i), one launch for all levels of a batch and one that combines its
 * chunks.  R >= 1, 1 <= n_levels <= 4096, 1 <= S < 2^31, else GPEMU_ERR_ARG before any launch.  n_out[] is a HOST array.
 * _dev addresses as gpemu_select_dev does (element j of row r at dV[r*row_stride + j*elem_stride]); dout is a device
 * array.
 *
 * Kernel density: dens[r*G + g] = 1 / (S h_r sqrt(2 pi)) sum_j exp(-(grid[r*G + g] - x_rj)^2 / (2 h_r^2)), the direct sum
 * over all S elements of row r: no binning, no truncation.  grid[R*G] and h[R] (finite, > 0) are HOST arrays.  Workgroup
 * (row, tile of up to 1024 grid points, chunk of 8192 samples): the grid points sit in registers, the samples are staged
 * through LDS once and added in index order into four interleaved sums; the chunk sums of a grid point are then added
 * by a lane-strided sum in chunk order and a fixed tree.  The order is fixed by S alone: the bits do not depend on the
 * grid or on the run.  The row is read once per tile of 1024 grid points.  R, G, S >= 1, else GPEMU_ERR_ARG.
 * _dev addresses as gpemu_select_dev does; ddens[R*G] is a device array.
 *
 * gpemu_marginal_dense_dev copies the rows of the block layout above into ddense[S*d]; gpemu_marginal_moments_dev
 * returns mean[d] and var[d] (divisor S; HOST arrays) of a dense device matrix dX[S*d], two passes, sums in a fixed
 * order (gpemu_sampler_chain_moments' kernels).
 * Every _dev form works on `stream` (NULL = the null stream) and waits for it before it returns. */
int gpemu_marginal_hist(int device, int64_t S, int d, const double *X, int nb1, const double *edges1, int nb2,
                        const double *edges2, int64_t group_counters, int64_t *hist1, int64_t *hist2,
                        int64_t *n_inside1);
int gpemu_marginal_hist_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows,
                            int64_t block_stride_rows, int d, int nb1, const double *edges1, int nb2,
                            const double *edges2, int64_t group_counters, int64_t *dhist1, int64_t *dhist2,
                            int64_t *dn_inside1, void *stream);
int gpemu_hpd(int device, int64_t R, int64_t S, const double *V, int64_t n_levels, const int64_t *n_out, double *out);
int gpemu_hpd_dev(int device, int64_t R, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                  int64_t n_levels, const int64_t *n_out, double *dout, int64_t workspace_bytes, void *stream);
int gpemu_kde1d(int device, int64_t R, int64_t S, const double *V, int64_t G, const double *grid, const double *h,
                double *dens);
int gpemu_kde1d_dev(int device, int64_t R, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                    int64_t G, const double *grid, const double *h, double *ddens, void *stream);
int gpemu_marginal_dense_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows,
                             int64_t block_stride_rows, int d, double *ddense, void *stream);
int gpemu_marginal_moments_dev(int device, const double *dX, int64_t S, int d, double *mean, double *var, void *stream);
/* Which launches of the three ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_marginal_path {
  GPEMU_MARGINAL_PATH_HIST_SWEEP = 0,  /* one sweep of the histogram kernel over the rows                             */
  GPEMU_MARGINAL_PATH_PAIR_GROUP,      /* ... that carried a group of pairs                                           */
  GPEMU_MARGINAL_PATH_SORT_BATCH,      /* one batch of rows through the sort's workspace (eight passes)               */
  GPEMU_MARGINAL_PATH_WINDOW_SEARCH,   /* the narrowest-window reduction of one batch, all levels                     */
  GPEMU_MARGINAL_PATH_KDE,             /* one launch of the density kernel (a batch of rows) and of its chunk sum      */
  GPEMU_MARGINAL_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_MARGINAL_PATH_COUNT)) = the counters; returns GPEMU_MARGINAL_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_marginal_path_counts(int64_t *out, int64_t n);

/* ---- 2-D kernel densities of parameter pairs ----------------------------------------------------------
 * The smooth off-diagonal panels of a corner plot from the WHOLE chain.  For pair p = (i, j), i != j, with shear beta,
 * bandwidths (h_a, h_b) = bandwidth[2p], bandwidth[2p+1], grids g_a = grid_a[p*G ..], g_b = grid_b[p*G ..] and
 * v_s = fma(-beta, x_si, x_sj),
 *   out[(p*G + a)*G + b] = 1 / (S 2 pi h_a h_b) sum_s exp(-((g_a[a] - x_si) / h_a)^2 / 2) exp(-((g_b[b] - v_s) / h_b)^2 / 2),
 * the direct sum over all S rows: no binning, no truncation.  With beta = C_ij / C_ii, h_a^2 = f^2 C_ii and
 * h_b^2 = f^2 (C_jj - C_ij^2 / C_ii) this is scipy.stats.gaussian_kde's full-covariance density at the points
 * (g_a[a], g_b[b] + beta g_a[a]); with beta = 0 the axis-aligned product-kernel density.
 * The sum is a G x S by S x G matrix product whose operands are generated in the kernel (never stored) and multiplied
 * on the fp64 matrix cores: workgroup (chunk of 8192 samples, 128 x 128 tile of the panel -- 64 x 64 where G <= 64 --,
 * pair) writes a partial tile; a second kernel adds a panel element's partial tiles in chunk order and scales once by
 * 1 / (S 2 pi h_a h_b).  No
 * floating-point atomics: the order of every sum depends on S and G alone, so two calls give the same bytes, whatever
 * the number of pairs, the batches or the device's free memory.  The rounding error of v_s is carried beside it, so the
 * argument of the second factor is as accurate as that of the first.  A factor whose exponent is below -746 is exactly 0.
 * A NaN in column i or j makes every element of the pair's panel NaN.
 * Pairs are processed in batches whose partial tiles (8 G^2 ceil(S / 8192) bytes per pair) fit workspace_bytes (0 = half
 * of the free device memory; if not one pair fits: GPEMU_ERR_HIP, sizes in the error text).
 * pairs[2P] (int64), shear[P], bandwidth[2P], grid_a[P*G], grid_b[P*G] are HOST arrays in both forms.  GPEMU_ERR_ARG,
 * before any launch: P < 1; G outside [1, 512]; d outside [1, 16]; S < 1 or S >= 2^31; a pair index outside [0, d) or
 * i = j; a bandwidth that is not finite and > 0; a grid value or shear that is not finite; workspace_bytes < 0.
 * gpemu_kde2d takes host samples X[S*d] and host out[P*G*G]; _dev reads the rows in the block layout of
 * gpemu_marginal_hist_dev in place, writes the device array dout[P*G*G], works on `stream` (NULL = the null stream) and
 * waits for it; so does gpemu_pair_moments_dev.
 *
 * gpemu_pair_moments_dev: what the default plan needs of device rows in the same layout.  mean[d] and cov[d*d] (the
 * full covariance, divisor S; both NULL: skipped) by two passes with sums in a fixed order; for n_pairs > 0 pairs with
 * their shear, ext[2p], ext[2p+1] = the minimum and maximum over the rows of fma(-shear[p], x_i, x_j), the expression
 * the density kernel evaluates (NaN rows are passed over).  mean, cov, ext, pairs and shear are HOST arrays. */
#define GPEMU_MAX_GRID_2D 512
int gpemu_kde2d(int device, int64_t S, int d, const double *X, int64_t n_pairs, const int64_t *pairs, const double *shear,
                const double *bandwidth, int G, const double *grid_a, const double *grid_b, double *out,
                int64_t workspace_bytes);
int gpemu_kde2d_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride_rows, int d,
                    int64_t n_pairs, const int64_t *pairs, const double *shear, const double *bandwidth, int G,
                    const double *grid_a, const double *grid_b, double *dout, int64_t workspace_bytes, void *stream);
int gpemu_pair_moments_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride_rows,
                           int d, double *mean, double *cov, int64_t n_pairs, const int64_t *pairs, const double *shear,
                           double *ext, void *stream);
/* Which launches ran.  A set of its own: gpemu_marginal_path keeps its five. */
enum gpemu_kde2d_path {
  GPEMU_KDE2D_PATH_DENSITY = 0,   /* one launch of the density kernel (the partial tiles of a batch of pairs)          */
  GPEMU_KDE2D_PATH_PAIR_BATCH,    /* one batch of pairs through the partial-tile workspace                             */
  GPEMU_KDE2D_PATH_PARTIAL_SUM,   /* one launch of the kernel that adds a batch's partial tiles in chunk order          */
  GPEMU_KDE2D_PATH_MOMENTS,       /* one mean-and-covariance computation of gpemu_pair_moments_dev                      */
  GPEMU_KDE2D_PATH_EXTENTS,       /* one extents computation of gpemu_pair_moments_dev                                  */
  GPEMU_KDE2D_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_KDE2D_PATH_COUNT)) = the counters; returns GPEMU_KDE2D_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_kde2d_path_counts(int64_t *out, int64_t n);

/* ---- per-observable log-likelihoods, PSIS-LOO and WAIC ------------------------------------------------
 * Which observable does what to the posterior, and how well is each predicted by all the others -- what the reference
 * answers by a second analysis on a subset of the observables and otherwise leaves open (ref: plot_analyses.py:144,
 * plot_qhat.py:116, "one could also plot some type of information gain metric").
 *
 * Terms: the merged covariance keeps only the within-observable blocks (ref: emulation.py:370-388), so the
 * log-likelihood of a group (ref: log_posterior.py:87-99) is a sum of per-observable terms.  T[o*ldt + s] = the term of
 * observable block o for row s, in gpemu_logpost's normalisation (no 2 pi constant): block-major, ldt >= S, one
 * contiguous row per observable.  A likelihood: the prior box is not applied; a row with a non-finite coordinate gives
 * NaN terms.  chain selects the data vector of gpemu_likelihood_setup_chains (0 otherwise).  No likelihood setup:
 * GPEMU_ERR_STATE; a setup with n_src > 0 (the sources span the blocks: no sum of terms): GPEMU_ERR_UNSUPPORTED, before
 * any launch.  A dense within-observable covariance only changes the setup's constants.  PC means / variances through
 * gpemu_gp_predict_dev in chunks of 2048 logical rows, then one wave per (row, block) with the likelihood's own
 * per-block function.  _dev reads row r at dX + ((r / block_rows)*block_stride_rows + r % block_rows)*d, S =
 * n_blocks*block_rows, as gpemu_posterior_predictive_dev; works on `stream` (NULL = the model's) and waits for it.
 * The host form writes T[n_blocks_of_the_model][B].  gpemu_model_observable_blocks: the blocks of the last setup.
 *
 * gpemu_psis: per row r of V[R*S] (log-likelihoods of one observable, or sums of several) with r_eff[r] (NULL: 1; HOST):
 *   x_s = -V_s - max(-V); tail size M = ceil(min(S/5, 3 sqrt(S / r_eff))); cutoff x_c = max(x_(max(S-M-1, 0)),
 *   log DBL_MIN) (ascending, 0-based); the tail = the n elements strictly above x_c (ties at the cutoff shorten it);
 *   n <= 4: pareto_k = +inf, raw weights.  Else the generalised Pareto fit of Zhang & Stephens (2009) to t_i =
 *   exp(x_(i)) - exp(x_c) (m = 30 + floor(sqrt(n)) grid points, weights below 10*2^-52 dropped, pareto_k = (n*k + 5) /
 *   (n + 10)); tail element i gets log(exp(x_c) + sigma*expm1(-pareto_k*log1p(-(i + 1/2)/n))/pareto_k), at most 0; tied
 *   raw values share the mean of their positions' values, so nothing depends on an order among equals; log-sum-exp
 *   normalisation.  out[r*GPEMU_PSIS_NOUT + .]: the indices below; p_waic is the sample variance of V with divisor S - 1
 *   (Vehtari, Gelman, Gabry 2017; NaN for S = 1).  logw (NULL: not wanted): the normalised log-weights [R*S], dense, in
 *   the input's order.  A row that holds a NaN or an infinity: NaN everywhere.  The row is sorted by gpemu_rank_dev's radix sort; every
 *   sum over samples runs over chunks of 4096 fixed by the index, in a fixed tree: the bits do not depend on
 *   workspace_bytes, on the grid or on the run.  Rows go through the workspace in batches (the sort's 16*S +
 *   1024*ceil(S/2048) + 4 bytes per row, 16 bytes per tail element and 40 per chunk beside it; 0 = half of the free
 *   device memory; if not one row fits: GPEMU_ERR_HIP, sizes in the error text).  R >= 1, 1 <= S < 2^31, r_eff finite
 *   and > 0, else GPEMU_ERR_ARG before any launch.  _dev addresses as gpemu_select_dev does; dout and dlogw are device
 *   arrays; stream NULL = the null stream; waits for it.
 *
 * gpemu_weighted_moments_dev: for the rows x_s of the block layout above (d <= 16) and R rows of log-weights
 * dlogw[r*ldw + s]: dmean[r*d + j] = sum_s w x_sj / sum_s w, dvar[r*d + j] = sum_s w (x_sj - mean)^2 / sum_s w, w =
 * exp(logw): the leave-one-observable-out posterior moments.  Two passes, the same fixed tree.
 * gpemu_loo_group_rows_dev: dout[g*ldo + s] = the sum of rows rows[group_start[g] .. group_start[g+1]) of dT[R][ldt] at s,
 * added in the given order (group_start, rows: HOST): a class of observables left out together.
 * Both work on `stream` (NULL = the null stream) and wait for it, as gpemu_psis_dev does. */
#define GPEMU_PSIS_ELPD_LOO 0
#define GPEMU_PSIS_LPPD 1
#define GPEMU_PSIS_P_LOO 2
#define GPEMU_PSIS_PARETO_K 3
#define GPEMU_PSIS_N_TAIL 4
#define GPEMU_PSIS_ESS_W 5
#define GPEMU_PSIS_P_WAIC 6
#define GPEMU_PSIS_ELPD_WAIC 7
#define GPEMU_PSIS_CUTOFF 8
#define GPEMU_PSIS_NOUT 9
int gpemu_model_observable_blocks(const gpemu_model *m, int64_t *n_blocks);
int gpemu_loglik_pointwise(gpemu_model *m, int chain, int64_t B, const double *X, double *T);
int gpemu_loglik_pointwise_dev(gpemu_model *m, int chain, const double *dX, int64_t n_blocks, int64_t block_rows,
                               int64_t block_stride_rows, double *dT, int64_t ldt, void *stream);
int gpemu_psis(int device, int64_t R, int64_t S, const double *V, const double *r_eff, int64_t workspace_bytes, double *out,
               double *logw);
int gpemu_psis_dev(int device, int64_t R, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                   const double *r_eff, double *dout, double *dlogw, int64_t workspace_bytes, void *stream);
int gpemu_weighted_moments_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows,
                               int64_t block_stride_rows, int d, int64_t R, const double *dlogw, int64_t ldw,
                               double *dmean, double *dvar, void *stream);
int gpemu_loo_group_rows_dev(int device, int64_t R, int64_t S, const double *dT, int64_t ldt, int64_t n_groups,
                             const int64_t *group_start, const int64_t *rows, double *dout, int64_t ldo, void *stream);
/* Which launches of these ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_loo_path {
  GPEMU_LOO_PATH_SORT_PASS = 0,   /* one pass of the radix sort, for one batch of rows                                */
  GPEMU_LOO_PATH_ROW_SMOOTHED,    /* a row whose tail (n > 4) was fitted and smoothed                                 */
  GPEMU_LOO_PATH_ROW_RAW,         /* a row left with its raw weights (n <= 4, or a NaN)                               */
  GPEMU_LOO_PATH_CHUNK,           /* one chunk of 2048 rows through gpemu_gp_predict_dev and the terms kernel         */
  GPEMU_LOO_PATH_ROW_BATCH,       /* one batch of rows through the sort's workspace                                   */
  GPEMU_LOO_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_LOO_PATH_COUNT)) = the counters; returns GPEMU_LOO_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_loo_path_counts(int64_t *out, int64_t n);

/* ---- sequential design: where to run the model next -------------------------------------------------
 * Active learning in Cohn's sense (integrated variance reduction) at the fitted hyper-parameters.  With c_p(x, x') the
 * two-set predictive covariance of PC p (gpemu_gp_predict_cov with X2: it carries no noise), a reference set x_s (s < S, weights
 * omega_s >= 0 that the call normalises to sum 1) and candidates x_c (c < M):
 *     IV_p = sum_s omega_s c_p(x_s, x_s),       den_p(c) = c_p(x_c, x_c) + tau_p
 *     score(c) = sum_p pc_weight[p] * [sum_s omega_s c_p(x_s, x_c)^2] / den_p(c)
 * -- the amount by which a model run at x_c, carrying noise variance tau_p, lowers sum_p pc_weight[p] IV_p.  A PC whose
 * den_p(c) <= min_variance * kernel_.diag_p contributes exactly 0 (the emulator is exact there already).  Conditioning
 * on a pick c* replaces every covariance by c(a, b) - u(a) u(b), u(.) = c(., c*) / sqrt(den(c*)) (u = 0 for a PC under
 * the floor at c*): u is appended to the two GEMM operands, den_p(c) -= u(c)^2 and IV_p -= sum_s omega_s u(s)^2 in place.
 *
 * The handle keeps V = W K(X_train, .)^T of the reference rows and of the candidates per PC, k-major, with max_picks
 * (rounded up to 16) spare rows, and a copy of both sets of rows; the S x M covariance is never stored: the score kernel
 * (MFMA f64) forms 64 x 64 tiles of it in registers, squares, weights and sums the 64 rows of a tile in a fixed order and
 * writes one partial per (PC, row tile, candidate); the partials of a candidate are added in index order.  No
 * floating-point atomics: the bits depend neither on workspace_bytes nor on the run.  workspace_bytes (0: half of the
 * free device memory) bounds the operands, the work array of the create call (N64 * max(S64, M64) doubles) and the
 * partials, which are chunked over candidate tiles; if the operands and one tile of partials do not fit: GPEMU_ERR_ARG
 * with the bytes needed in the error text.
 *
 * Checked before any launch (GPEMU_ERR_ARG): 1 <= S, M <= 4194240, k <= 64, 0 <= max_picks <= 256, min_variance finite
 * and >= 0, pc_weight and tau (NULL: the White level of each PC, 0 without one) finite and >= 0, w_ref (NULL: 1 / S;
 * always a HOST array) finite and >= 0 with a positive sum, finite rows in the host form.  The _dev form reads its rows
 * from device memory unchecked: reference row r at dXref + ((r / block_rows)*block_stride_rows + r % block_rows)*d, S =
 * n_blocks*block_rows, as gpemu_posterior_predictive_dev (a stored chain in place); dXcand[M*d] dense; `stream` (NULL:
 * none) is waited for before the rows are read.  All work runs on the model's stream; every call waits for it.
 * The model must outlive the handle.
 * gpemu_design_scores: score[M] and, if not NULL, score_pc[k*M] (the PCs' weighted terms), HOST arrays.
 * gpemu_design_condition: GPEMU_ERR_ARG for a candidate outside [0, M) or beyond max_picks picks.
 * gpemu_design_state: iv[k] (unweighted IV_p), den[k*M] or NULL, n_picks or NULL. */
typedef struct gpemu_design gpemu_design;
int gpemu_design_create(gpemu_design **out, gpemu_model *m, int64_t S, const double *Xref, const double *w_ref,
                        int64_t M, const double *Xcand, const double *pc_weight, const double *tau,
                        double min_variance, int64_t max_picks, int64_t workspace_bytes);
int gpemu_design_create_dev(gpemu_design **out, gpemu_model *m, const double *dXref, int64_t n_blocks,
                            int64_t block_rows, int64_t block_stride_rows, const double *w_ref, int64_t M,
                            const double *dXcand, const double *pc_weight, const double *tau, double min_variance,
                            int64_t max_picks, int64_t workspace_bytes, void *stream);
int gpemu_design_scores(gpemu_design *h, double *score, double *score_pc);
int gpemu_design_condition(gpemu_design *h, int64_t candidate);
int gpemu_design_state(gpemu_design *h, double *iv, double *den, int64_t *n_picks);
int gpemu_design_destroy(gpemu_design *h);
/* Which launches ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_design_path {
  GPEMU_DESIGN_PATH_SCORES = 0,   /* one gpemu_design_scores call                                                      */
  GPEMU_DESIGN_PATH_CHUNK,        /* one chunk of candidate tiles through the score and finish kernels                 */
  GPEMU_DESIGN_PATH_DP8,          /* ... on 8-wide rows (d <= 8)                                                       */
  GPEMU_DESIGN_PATH_DP16,         /* ... on 16-wide rows (9 <= d <= 16)                                                */
  GPEMU_DESIGN_PATH_KIND_RBF,     /* ... with the RBF kernel (and Matern nu = inf)                                     */
  GPEMU_DESIGN_PATH_KIND_M05,     /* ... Matern 0.5                                                                    */
  GPEMU_DESIGN_PATH_KIND_M15,     /* ... Matern 1.5                                                                    */
  GPEMU_DESIGN_PATH_KIND_M25,     /* ... Matern 2.5                                                                    */
  GPEMU_DESIGN_PATH_KIND_NU,      /* ... Matern of any other nu (the out-of-line Bessel call)                          */
  GPEMU_DESIGN_PATH_COLUMN,       /* one conditioning step (the column kernel and the in-place updates)                */
  GPEMU_DESIGN_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_DESIGN_PATH_COUNT)) = the counters; returns GPEMU_DESIGN_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_design_path_counts(int64_t *out, int64_t n);

/* ---- information gain and KL divergence of chains by k-th nearest neighbours --------------------------
 * How many nats the data taught about each parameter, each pair and all of them jointly, and how far apart two
 * posteriors are -- the question the reference leaves open twice ("one could also plot some type of information gain
 * metric, e.g. KL divergence"; ref: plot_qhat.py:116, plot_analyses.py:144).  Under the uniform prior on the box the
 * gain is minus the differential entropy of u = (x - lower) / (upper - lower); the estimators (Kozachenko-Leonenko;
 * Wang, Kulkarni, Verdu 2009; Perez-Cruz 2008) need the distance of every row to its k-th nearest neighbour.
 *
 * gpemu_unit_rows_dev: dU[i*d + j] = (x_j - lower[j]) * (1 / (upper[j] - lower[j])) of logical row floor(i*S / n),
 * i < n <= S = n_blocks*block_rows < 2^31: two separately rounded operations, the bits of the same numpy expression.
 * Logical row r is at dX + (r / block_rows)*block_stride + (r % block_rows)*d: block_stride counts ELEMENTS (a step of
 * a chain may be padded to a length that is no multiple of d) and holds at least a block.  A row with a non-finite coordinate becomes a row of NaN -- the search passes it over -- and is
 * counted in *n_skipped.  lower, upper, n_skipped: HOST.  Works on `stream` (NULL = the null stream) and waits for it.
 *
 * gpemu_knn_dist: queries UQ[nq*d], references UR[nr*d] (NULL: the queries themselves, nr = nq), n_subsets subsets of
 * the d coordinates as 32-bit masks (bit j: coordinate j; HOST), 1 <= k <= 16:
 *   r2[p*nq + i]    = the squared Euclidean distance of query i to its k-th nearest reference in the coordinates of
 *                     subset p: acc = fma(diff, diff, acc) over the subset's coordinates in increasing order, from the
 *                     differences (never |x|^2 + |y|^2 - 2 x.y, which cancels at neighbour distances);
 *   zeros[p*nq + i] = the number of references at squared distance exactly 0.
 * Zero-distance rule: a reference at squared distance exactly 0 in the subset is a copy of the query; it is counted in
 * zeros and is NOT a neighbour.  In a self search that excludes the query itself (no index test), and it excludes the
 * repeated states of an ensemble chain.  Fewer than k references that are no copies: r2 = +inf.  A reference with a
 * non-finite coordinate in the subset is passed over; a query with one gets r2 = NaN, zeros = 0.
 * One thread owns a query and keeps its k smallest distances sorted in registers; the references stream through LDS
 * GPEMU_KNN_REF_TILE at a time; the grid is (256-query tiles, subsets, reference splits Z), and a second kernel merges
 * the Z lists and adds the Z zero counts.  The k smallest of a set do not depend on its order: r2 and zeros are the
 * same bits for every Z, every tile and every workspace_bytes.  splits = 0 chooses Z (so that a launch has some 2048
 * workgroups, a split at least 64 references, Z <= 64); splits in [1, 64] forces it (for tests).  The Z partial lists
 * ((8 k + 4) Z nq bytes per subset) go through workspace_bytes (0 = half of the free device memory) in batches of
 * subsets; a chosen Z shrinks to what fits; if a forced Z does not fit for one subset: GPEMU_ERR_HIP.
 * GPEMU_ERR_ARG before any launch: k outside [1, 16]; d outside [1, 16]; a mask that is 0 or has a bit >= d; nq or nr
 * outside [1, 2^31); n_subsets outside [1, 2^20]; splits outside [0, 64]; workspace_bytes < 0; no references and
 * nr != nq.  _dev reads dense device rows, writes the device arrays dr2 and dzeros, works on `stream` (NULL = the null
 * stream) and waits for it.
 *
 * gpemu_knn_logsum_dev: per subset p of dr2[n_subsets*n] (and dzeros, or NULL), counts[3p ..] = n_used (rows whose
 * distance is finite), n_short (+inf), copies (the sum of zeros); sums[2p ..] = the sum of v and of v^2 over the used
 * rows, v = log r2.  With dnu2 (the same shape): v = log nu2 - log r2, and a row is used if both are finite, short if
 * one is +inf.  A NaN distance passes the row over.  Blocks of 1024 rows and then the blocks, each in a fixed tree.
 * counts (int64) and sums: HOST.  Works on `stream` (NULL = the null stream) and waits for it. */
#define GPEMU_KNN_MAX_K 16
#define GPEMU_KNN_REF_TILE 256
int gpemu_unit_rows_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride, int d,
                        const double *lower, const double *upper, int64_t n, double *dU, int64_t *n_skipped, void *stream);
int gpemu_knn_dist(int device, int64_t nq, int64_t nr, int d, const double *UQ, const double *UR, int64_t n_subsets,
                   const uint32_t *masks, int k, int splits, int64_t workspace_bytes, double *r2, int32_t *zeros);
int gpemu_knn_dist_dev(int device, int64_t nq, int64_t nr, int d, const double *dUQ, const double *dUR, int64_t n_subsets,
                       const uint32_t *masks, int k, int splits, int64_t workspace_bytes, double *dr2, int32_t *dzeros,
                       void *stream);
int gpemu_knn_logsum_dev(int device, int64_t n_subsets, int64_t n, const double *dr2, const int32_t *dzeros,
                         const double *dnu2, int64_t *counts, double *sums, void *stream);
/* Which launches ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_knn_path {
  GPEMU_KNN_PATH_UNIT_ROWS = 0,   /* one launch of the unit-box kernel                                                 */
  GPEMU_KNN_PATH_SEARCH,          /* one launch of the search kernel (a batch of subsets of one width)                 */
  GPEMU_KNN_PATH_MERGE,           /* one launch of the kernel that merges the Z partial lists (Z > 1 only)             */
  GPEMU_KNN_PATH_SUBSET_BATCH,    /* one batch of subsets through the partial-list workspace                           */
  GPEMU_KNN_PATH_LOGSUM,          /* one gpemu_knn_logsum_dev call (the partial and the final kernel)                  */
  GPEMU_KNN_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_KNN_PATH_COUNT)) = the counters; returns GPEMU_KNN_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_knn_path_counts(int64_t *out, int64_t n);

/* ---- row-wise log-sum-exp of pairwise Gaussian log-weights: expected information gain -----------------
 * Which MEASUREMENT would constrain the parameters most?  With a Gaussian likelihood of constant covariance, whitened
 * by its Cholesky factor, the nested Monte Carlo estimator of the expected information gain (Ryan 2003; Huan and
 * Marzouk 2013) needs log (1/S) sum_j exp(-|y_i - z_j|^2 / 2) for n simulated outcomes y_i against S whitened
 * predictions z_j: n x S x F multiply-adds and n x S exponentials, whose n x S matrix never exists.
 *
 * gpemu_pair_lse: rows Y[n*F] and Z[S*F]; a_ij = -|y_i - z_j|^2 / 2; per row i
 *   lse[i] = m_i + log s1_i,  m_i = max_j a_ij,  s1_i = sum_j exp(a_ij - m_i);
 *   ess[i] = s1_i^2 / s2_i,   s2_i = sum_j exp(2 (a_ij - m_i)): the effective number of columns that carry row i
 *            (ess may be NULL).
 * self (int64 [n], or NULL): pair (i, self[i]) is left out of row i's sums; -1 leaves nothing out.  A row whose every
 * pair is left out has lse = -inf, ess = 0; no NaN is formed.
 * The rows are centred first: centre[F] is subtracted from Y and Z alike (one rounded operation per element; distances
 * are unchanged), and a_ij = y.z - |y_i|^2 / 2 - |z_j|^2 / 2 of the centred rows, y.z on the fp64 matrix cores
 * (v_mfma_f64_16x16x4_f64, a chain of 4 ceil(F / 4) terms), the half norms one fma chain per row.  The error of a_ij
 * is absolute, of order u (F + c) (|y_i|^2 + |z_j|^2) / 2 in the centred rows.  centre = NULL: the column means of Z,
 * by the pooled-moments kernel (gpemu_pairlse_centre_dev gives the same numbers).
 * A workgroup owns GPEMU_PAIRLSE_TILE_ROWS rows of Y and one chunk of GPEMU_PAIRLSE_CHUNK columns of Z and keeps an
 * online (m, s1, s2) per row; a second kernel merges the chunks in chunk order.  No floating-point atomics; the chunks
 * depend on S alone: lse and ess are the same bits for every workspace_bytes and every run.
 * workspace_bytes bounds the memory of the row blocks in flight, GPEMU_PAIRLSE_BLOCK_BYTES(S, F) each (0 = half of the
 * free device memory); the blocks go through it in batches; less than one block: GPEMU_ERR_HIP.  The centred copy of Z
 * (8 S (F + 17) bytes at most) is allocated besides.
 * GPEMU_ERR_ARG before any launch: n or S outside [1, 2^31); F outside [1, 65536]; a self[i] outside [-1, S); a leading
 * dimension below F; workspace_bytes < 0; a null Y, Z or lse.
 * _dev: every array is DEVICE memory (dself, dcentre, dess may be NULL); row i of Y starts at dY + i*ldy, of Z at
 * dZ + i*ldz; works on `stream` (NULL = the null stream) and waits for it (dself is copied to the host and checked
 * first); so does gpemu_pairlse_centre_dev. */
#define GPEMU_PAIRLSE_CHUNK 2048
#define GPEMU_PAIRLSE_TILE_ROWS 64
#define GPEMU_PAIRLSE_BLOCK_BYTES(S, F) \
  (8LL * GPEMU_PAIRLSE_TILE_ROWS * ((((F) + 15) / 16 * 16 + 1) + 3 * (((S) + GPEMU_PAIRLSE_CHUNK - 1) / GPEMU_PAIRLSE_CHUNK)))
int gpemu_pair_lse(int device, int64_t n, int64_t S, int64_t F, const double *Y, const double *Z, const int64_t *self,
                   const double *centre, int64_t workspace_bytes, double *lse, double *ess);
int gpemu_pair_lse_dev(int device, int64_t n, int64_t S, int64_t F, const double *dY, int64_t ldy, const double *dZ,
                       int64_t ldz, const int64_t *dself, const double *dcentre, int64_t workspace_bytes, double *dlse,
                       double *dess, void *stream);
/* dcentre[F] (DEVICE) = the column means of the device rows dZ: what the calls above subtract where centre is NULL. */
int gpemu_pairlse_centre_dev(int device, int64_t S, int64_t F, const double *dZ, int64_t ldz, double *dcentre, void *stream);
/* Which launches ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_pairlse_path {
  GPEMU_PAIRLSE_PATH_CENTRE = 0,   /* one launch of the centring pre-pass (Z once, Y once per batch of row blocks)      */
  GPEMU_PAIRLSE_PATH_PARTIAL,      /* one launch of the partial kernel                                                  */
  GPEMU_PAIRLSE_PATH_MERGE,        /* one launch of the kernel that merges the chunks' triples                          */
  GPEMU_PAIRLSE_PATH_ROW_BATCH,    /* one batch of row blocks through the workspace                                     */
  GPEMU_PAIRLSE_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_PAIRLSE_PATH_COUNT)) = the counters; returns GPEMU_PAIRLSE_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_pairlse_path_counts(int64_t *out, int64_t n);

/* ---- importance reweighting of a chain and weighted summaries -----------------------------------------
 * The posterior under another prior or under other data, from the chain that exists: the log-posterior takes constant
 * priors inside a box (ref: log_posterior.py:97) while the reference's own prior sampler draws c_1, c_2, c_3 with a
 * uniform LOGARITHM (ref: plot_qhat.py:298-326).  The stored samples are importance-reweighted to the new target;
 * gpemu_psis_dev smooths the ratios and its Pareto k-hat says when a rerun is needed instead.
 *
 * gpemu_logprior: L[r*ldl + s] = sum_{i < d} f_ri(x_si), the log of the new prior over the flat one without its
 * constants, added in index order with one rounding per addition, for R scenarios with HOST tables kind[R*d] (int),
 * a[R*d], b[R*d]:
 *   kind 0 flat          f = 0
 *   kind 1 log-uniform   f = -log x                               (needs lower[i] > 0)
 *   kind 2 normal        f = -(x - a)^2 / (2 b^2)
 *   kind 3 log-normal    f = -log x - (log x - a)^2 / (2 b^2)     (needs lower[i] > 0)
 * lower[d] (HOST) is the box's lower bounds; the box itself is not applied.  GPEMU_ERR_ARG before any launch: d outside
 * [1, 16], R outside [1, 64], an unknown kind, kind 1 / 3 with lower[i] <= 0, kind 2 / 3 with a non-finite a or b or
 * b <= 0, ldl below the number of rows.  One lane per sample, the tables in LDS.  The host form takes X[S*d] and writes
 * L[R*S]; _dev reads the rows in the block layout of gpemu_marginal_hist_dev in place and writes the device array dL.
 *
 * gpemu_logmeanexp_dev: per row of dL[R][ldl], dlme[r] = logsumexp_s(L_rs) - log S (NULL: not wanted) and
 * dlw[r*S + s] = L_rs - logsumexp(L_r) (NULL: not wanted; dense), both DEVICE arrays.  The sum runs over chunks of 4096
 * fixed by the index -- a lane adds its 16 terms exp(L - max) in index order, then the wave tree, the chunks in order --
 * so the bits do not depend on the grid or on the run.  A row with a NaN or +inf gives NaN, a row of -inf gives -inf.
 *
 * gpemu_weights_fixed_dev: dq[r*ldq + s] = (uint64) rint(exp(dlw[r*ldw + s]) * 2^52) and dQ[r] = sum_s dq[r][s], an
 * exact integer sum (a NaN weight counts 0).  For normalised weights and S < 2^31, Q < 2^53: every partial sum of a row
 * is an exact integer and exact in a double, so no sum below depends on its order.
 *
 * gpemu_weighted_select: out[(w*R_v + v)*n_targets + i] = the smallest element x of value row v with
 * sum_{x_s <= x} q[w][s] >= targets[w*n_targets + i] -- the inverted weighted ECDF, an element of the input (a zero may
 * come back with either sign).  targets[R_w*n_targets] is a HOST array, in any order, every one in [1, 2^53]; a target
 * above the row's total weight returns NaN, and so does every target of a value row that holds a NaN.  The radix select
 * of gpemu_select with histograms of weight sums: eight passes of 8 bits, 64-bit LDS integer atomics, non-zero bins
 * flushed with 64-bit global integer atomics, a sample's weight loaded only when its key matches a live prefix; targets
 * in groups of 16.  The (w, v) pairs go through the state (33 288 bytes each) in batches of at most 512 that fit
 * workspace_bytes (0 = half of the free device memory; not one pair: GPEMU_ERR_HIP).  R_v, R_w >= 1, R_v*R_w < 2^31,
 * 1 <= S < 2^31, 1 <= n_targets < 2^24, else GPEMU_ERR_ARG before any launch.  _dev addresses the values as
 * gpemu_select_dev does (element j of row v at dV[v*row_stride + j*elem_stride]); dq[R_w][ldq] and dout are device arrays.
 *
 * gpemu_weighted_hist: gpemu_marginal_hist's histograms -- the same edges, binning rule and limits -- with q[w][s] added
 * where it adds 1: hist1[R_w*d*nb1], hist2[R_w*n_pairs*nb2*nb2] (NULL allowed for d = 1), w_inside1[R_w*d] = the weight
 * counted in hist1[w][j].  LDS holds 64-bit bins: group_bins per sweep (0: 18432 = 144 KiB; else max(nb1, nb2) <=
 * group_bins <= 18432); a pair whose nb2^2 bins do not fit is swept in bands of floor(group_bins / nb2) bins of its
 * first index.  One weight row per workgroup (grid.y).  1 <= R_w <= 65535.
 * Every _dev form works on `stream` (NULL = the null stream) and waits for it before it returns. */
int gpemu_logprior(int device, int64_t S, int d, const double *X, int R, const int *kind, const double *a,
                   const double *b, const double *lower, double *L);
int gpemu_logprior_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows, int64_t block_stride_rows,
                       int d, int R, const int *kind, const double *a, const double *b, const double *lower, double *dL,
                       int64_t ldl, void *stream);
int gpemu_logmeanexp_dev(int device, int64_t R, int64_t S, const double *dL, int64_t ldl, double *dlme, double *dlw,
                         void *stream);
int gpemu_weights_fixed_dev(int device, int64_t R, int64_t S, const double *dlw, int64_t ldw, uint64_t *dq, int64_t ldq,
                            uint64_t *dQ, void *stream);
int gpemu_weighted_select(int device, int64_t R_v, int64_t S, const double *V, int64_t R_w, const uint64_t *q,
                          int64_t n_targets, const uint64_t *targets, double *out);
int gpemu_weighted_select_dev(int device, int64_t R_v, int64_t S, const double *dV, int64_t row_stride,
                              int64_t elem_stride, int64_t R_w, const uint64_t *dq, int64_t ldq, int64_t n_targets,
                              const uint64_t *targets, double *dout, int64_t workspace_bytes, void *stream);
int gpemu_weighted_hist(int device, int64_t S, int d, const double *X, int64_t R_w, const uint64_t *q, int nb1,
                        const double *edges1, int nb2, const double *edges2, int64_t group_bins, uint64_t *hist1,
                        uint64_t *hist2, uint64_t *w_inside1);
int gpemu_weighted_hist_dev(int device, const double *dX, int64_t n_blocks, int64_t block_rows,
                            int64_t block_stride_rows, int d, int64_t R_w, const uint64_t *dq, int64_t ldq, int nb1,
                            const double *edges1, int nb2, const double *edges2, int64_t group_bins, uint64_t *dhist1,
                            uint64_t *dhist2, uint64_t *dw_inside1, void *stream);
/* Which launches of these ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_reweight_path {
  GPEMU_REWEIGHT_PATH_LOGPRIOR = 0,      /* one launch of the log-prior kernel                                          */
  GPEMU_REWEIGHT_PATH_QUANTISE,          /* one launch of the fixed-point weights kernel                                */
  GPEMU_REWEIGHT_PATH_LOGSUMEXP,         /* one log-sum-exp of a matrix of rows (maximum, sum and their finish kernels) */
  GPEMU_REWEIGHT_PATH_WSEL_HIST_PASS,    /* one pass of the weighted select's histogram kernel, for one batch of pairs  */
  GPEMU_REWEIGHT_PATH_WSEL_SCAN,         /* one launch of the scan that walks the cumulative weight                     */
  GPEMU_REWEIGHT_PATH_WHIST_SWEEP,       /* one sweep of the weighted histogram kernel over the rows                    */
  GPEMU_REWEIGHT_PATH_WHIST_PAIR_GROUP,  /* ... that carried a group of pairs (or a band of one)                        */
  GPEMU_REWEIGHT_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_REWEIGHT_PATH_COUNT)) = the counters; returns GPEMU_REWEIGHT_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_reweight_path_counts(int64_t *out, int64_t n);

/* ---- weighted bands, highest-density intervals and densities of a reweighted chain ---------------------
 * What a user takes from a chain next, under the fixed-point weights q[R_w][S] (uint64, Q_w = sum_s q_ws < 2^53) of
 * gpemu_weights_fixed_dev: a double holds every q and every partial sum of q exactly.  Integer sums use integer
 * atomics; every floating-point sum runs in a tree fixed by the logical sample index: no bit depends on the order of an
 * atomic, on the grid, on the workspace or on the run.  1 <= R_w <= 64 and 1 <= S < 2^31 everywhere below, every target
 * in [1, 2^53]; an argument error returns GPEMU_ERR_ARG before any launch or allocation.
 *
 * The _dev forms take, instead of a stream and a workspace limit of their own, */
typedef struct { void *stream; int64_t workspace_bytes; } gpemu_call_ctx;
/* ctx == NULL means stream NULL and workspace_bytes 0 (sized from the free device memory).  gpemu_weighted_hpd_dev and
 * gpemu_weighted_kde1d_dev work on ctx->stream (NULL = the null stream) and each waits for it before returning;
 * gpemu_posterior_predictive_weighted_dev works on ctx->stream (NULL = the model's) and waits for it before returning.
 *
 * gpemu_posterior_predictive_weighted: gpemu_posterior_predictive's reduction under every weight row w, with mu_f and
 * sigma^2_f as defined there:
 *   mean[w*F + f]      = sum_s q_ws mu_fs / Q_w
 *   var_param[w*F + f] = sum_s q_ws (mu_fs - mean[w][f])^2 / Q_w                                   (two passes)
 *   var_emu[w*F + f]   = (sum_p comp[p][f] vbar_wp comp[p][f] + cov_unexplained[f][f]) scale_f^2,
 *                        vbar_wp = sum_s q_ws var_p(theta_s) / Q_w
 *   quantiles[(w*F + f)*n_targets + i] = gpemu_weighted_select's answer to targets[w*n_targets + i] on feature f's row
 * each NULL where not wanted (n_targets = 0: no quantiles).  The predict stages, the projection, the workspace rule and
 * the whole / feature-blocked paths are gpemu_posterior_predictive's.  The weighted row reduction reads, per workgroup,
 * 4 rows of central values and 4 weight rows once for their 16 sums over a chunk of 4096 samples: a lane adds its 16
 * terms fma((double)q, x, .) in index order (a term of weight 0 is left out), then the wave butterfly, the waves in
 * order, the chunks in order, and the sum is divided by (double)Q_w.  With q_s = 2^e the mean and var_emu are
 * gpemu_posterior_predictive's bits.  Q_w = 0 gives NaN.  targets[] is a HOST array; the host form takes X[S*d] and
 * q[R_w*S]; _dev reads the rows in the block layout of gpemu_posterior_predictive_dev in place, dq[R_w][ldq], and
 * writes device arrays.
 *
 * gpemu_weighted_hpd: for value row v, weight row w and target mass t = targets[w*n_levels + l], over every sample value
 * a of the row, with b(a) the smallest sample value >= a with sum_{a <= x_s <= b} q_ws >= t, the (a, b(a)) of the
 * smallest double-rounded width b - a, equal widths to the smaller a:
 *   out[((w*R_v + v)*n_levels + l)*2 + {0, 1}] = a, b
 * both elements of the input (a zero comes back as +0).  NaN where t exceeds Q_w, where the row holds a NaN, and where
 * its smallest or largest element is infinite, as in gpemu_hpd.  Under equal weights q_s = c and t = c (S - n_out + 1)
 * it returns gpemu_hpd's two ends for n_out.  Per batch of value rows: gpemu_hpd's key sort once, then per weight row the
 * weights placed by value (a binary search for the first sorted position of the sample's key, a 64-bit integer atomic
 * there), an inclusive 64-bit prefix sum in three launches (chunk sums, their scan, apply), and the window search: every
 * run start i finds the first j with C[j] - C[i-1] >= t by bisection, and (width, i) is reduced lexicographically as in
 * gpemu_hpd.  A (w, v) pair of a batch holds 24*S + 1032*ceil(S/2048) + 16*n_levels*ceil(S/4096) + 4 bytes of workspace
 * (sorted keys twice, digit histograms, cumulative weights, chunk sums, window minima); the pairs of a weight row go
 * through it in batches that fit workspace_bytes (0 = half of the free device memory); not one pair: GPEMU_ERR_HIP with
 * the sizes in the error text.  1 <= n_levels <= 4096.  _dev addresses the values as gpemu_select_dev does.
 *
 * gpemu_weighted_kde1d: dens[(w*R_v + v)*G + g] = 1 / (Q_w h sqrt(2 pi)) sum_s q_ws exp(-(grid - x_vs)^2 / (2 h^2)) with
 * the HOST arrays grid[R_w*R_v*G] and h[R_w*R_v], one grid and bandwidth per (w, v) pair.  gpemu_kde1d's tiling and
 * order of summation with fma((double)q, exp(.), .) where it adds exp(.): with q_s = 2^e its bits.  A sample with q = 0
 * contributes nothing.  Q_w = 0 gives NaN; a non-finite or non-positive h and a non-finite grid point: GPEMU_ERR_ARG.
 * The pairs go in batches of about 256 MiB of chunk sums, as gpemu_kde1d's rows do. */
int gpemu_posterior_predictive_weighted(gpemu_model *m, int64_t S, const double *X, int64_t R_w, const uint64_t *q,
                                        int64_t n_targets, const uint64_t *targets, int64_t workspace_bytes,
                                        double *mean, double *var_param, double *var_emu, double *quantiles);
int gpemu_posterior_predictive_weighted_dev(gpemu_model *m, const double *dX, int64_t n_blocks, int64_t block_rows,
                                            int64_t block_stride_rows, int64_t R_w, const uint64_t *dq, int64_t ldq,
                                            int64_t n_targets, const uint64_t *targets, double *dmean,
                                            double *dvar_param, double *dvar_emu, double *dquantiles,
                                            const gpemu_call_ctx *ctx);
int gpemu_weighted_hpd(int device, int64_t R_v, int64_t S, const double *V, int64_t R_w, const uint64_t *q,
                       int64_t n_levels, const uint64_t *targets, double *out);
int gpemu_weighted_hpd_dev(int device, int64_t R_v, int64_t S, const double *dV, int64_t row_stride, int64_t elem_stride,
                           int64_t R_w, const uint64_t *dq, int64_t ldq, int64_t n_levels, const uint64_t *targets,
                           double *dout, const gpemu_call_ctx *ctx);
int gpemu_weighted_kde1d(int device, int64_t R_v, int64_t S, const double *V, int64_t R_w, const uint64_t *q, int64_t G,
                         const double *grid, const double *h, double *dens);
int gpemu_weighted_kde1d_dev(int device, int64_t R_v, int64_t S, const double *dV, int64_t row_stride,
                             int64_t elem_stride, int64_t R_w, const uint64_t *dq, int64_t ldq, int64_t G,
                             const double *grid, const double *h, double *ddens, const gpemu_call_ctx *ctx);
/* Which launches of these ran.  A set of its own: the other sets keep their sizes and indices. */
enum gpemu_wsummary_path {
  GPEMU_WSUMMARY_PATH_BANDS_WHOLE = 0,        /* a weighted reduction whose features all fit the workspace at once    */
  GPEMU_WSUMMARY_PATH_BANDS_FEATURE_BLOCKED,  /* ... that went through the workspace in blocks of features            */
  GPEMU_WSUMMARY_PATH_ROW_REDUCE,             /* one launch of the weighted row reduction                             */
  GPEMU_WSUMMARY_PATH_SELECT_PASS,            /* one histogram + scan pass of the weighted select on the workspace    */
  GPEMU_WSUMMARY_PATH_HPD_SORT_BATCH,         /* the key sort of one batch of value rows                              */
  GPEMU_WSUMMARY_PATH_HPD_PLACE,              /* one launch that places a weight row's weights by value               */
  GPEMU_WSUMMARY_PATH_HPD_SCAN,               /* one prefix sum of the placed weights (three launches)                */
  GPEMU_WSUMMARY_PATH_HPD_WINDOW,             /* one window search with its finish                                    */
  GPEMU_WSUMMARY_PATH_KDE,                    /* one batch of pairs of the weighted density (partial sums + their sum) */
  GPEMU_WSUMMARY_PATH_COUNT
};
/* out[0 .. min(n, GPEMU_WSUMMARY_PATH_COUNT)) = the counters; returns GPEMU_WSUMMARY_PATH_COUNT (or GPEMU_ERR_ARG). */
int gpemu_wsummary_path_counts(int64_t *out, int64_t n);

/* ---- fit handle: test-only entry points ---------------------------------------------------------------------------
 * For the tests of the fit side only; nothing in the library's own flow calls them.
 * gpemu_fit_workspace: out[N*N] = problem z of the last evaluation (gpemu_fit_lml / _lml_batch / _factor) as the
 * handle holds it, the lower triangle (zeros above the diagonal): which = GPEMU_FIT_WS_L (the Cholesky factor),
 * GPEMU_FIT_WS_W (its inverse W = L^-1) or GPEMU_FIT_WS_KINV (K^-1 = W^T W: only after an evaluation with gradient,
 * else GPEMU_ERR_STATE).  z >= the last evaluation's number of problems: GPEMU_ERR_ARG.
 * gpemu_fit_poison: every byte of the handle's workspace (K, Dinv, W, T, K^-1, y, v, alpha, gpart, gstage, scal, grad,
 * hyper-parameters) set to 0xff -- a NaN in every double -- on the handle's stream: an evaluation that reads anything
 * it has not written first shows it. */
#define GPEMU_FIT_WS_L 0
#define GPEMU_FIT_WS_W 1
#define GPEMU_FIT_WS_KINV 2
int gpemu_fit_workspace(gpemu_fit *f, int which, int64_t z, double *out);
int gpemu_fit_poison(gpemu_fit *f);

/* ---- device memory: test-only entry points --------------------------------------------------------------------------
 * For the tests of the library's resource handling only; nothing in the library's own flow calls them.  One ledger per
 * process counts every device allocation and free the library makes, and the streams and events its handles create.
 * It does not count the IPC handles and mapped buffers of the peer transport, nor what RCCL allocates for itself.
 * gpemu_devmem_stats: out[0 .. min(n, GPEMU_DEVMEM_STAT_COUNT)) = the counters below; returns GPEMU_DEVMEM_STAT_COUNT
 * (or GPEMU_ERR_ARG).  ALLOCS - FREES = LIVE_BLOCKS at every reading.
 * gpemu_devmem_refuse_nth: nth >= 1 makes the nth device allocation from now (of any host thread) fail, once, with
 * GPEMU_ERR_HIP and an error text that holds "refused" and the bytes asked for; it is decided on the host before the
 * allocator is called, allocates nothing and touches no device state, and disarms itself when it fires.  nth = 0
 * disarms.  *still_armed (may be null) = 1 if an earlier arming had not fired yet, else 0.  nth < 0: GPEMU_ERR_ARG. */
enum gpemu_devmem_stat {
  GPEMU_DEVMEM_LIVE_BLOCKS = 0,   /* device allocations that exist now                                 */
  GPEMU_DEVMEM_LIVE_BYTES,        /* ... and the bytes asked for them                                  */
  GPEMU_DEVMEM_ALLOCS,            /* allocations made since the library was loaded                     */
  GPEMU_DEVMEM_FREES,             /* frees of a live block since then (a free of null counts nothing)  */
  GPEMU_DEVMEM_LIVE_STREAMS,      /* streams the library's handles own now                             */
  GPEMU_DEVMEM_LIVE_EVENTS,       /* events the library's handles own now                              */
  GPEMU_DEVMEM_STAT_COUNT
};
int gpemu_devmem_stats(int64_t *out, int64_t n);
int gpemu_devmem_refuse_nth(int64_t nth, int64_t *still_armed);

/* ---- PCA: test-only entry point --------------------------------------------------------------------------------------
 * For the test of gpemu_pca_fit's non-convergence report only; nothing in the library's own flow calls it.
 * gpemu_pca_sweep_limit_next: 1 <= limit <= 60 makes the next gpemu_pca_fit (of any host thread) that passes its
 * argument checks stop after `limit` sweeps instead of 60, once: that call disarms it whether it converges or not, and
 * the calls after it run as in a fresh process.  limit = 0 disarms.  *still_armed (may be null) = 1 if an earlier
 * arming had not been used yet, else 0.  limit outside [0, 60]: GPEMU_ERR_ARG.  It is decided on the host, allocates
 * nothing and touches no device state. */
int gpemu_pca_sweep_limit_next(int64_t limit, int64_t *still_armed);

/* Philox4x32-10 block function (host copy of the device generator; for tests) */
int gpemu_philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                     uint32_t *out4);

#ifdef __cplusplus
}
#endif
#endif /* GPEMU_H */
