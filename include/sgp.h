/*
 * sgp.h -- C ABI of the MI355X-native sparse-GP objective+gradient path.
 *
 * Drop-in boundary for luisdamiano/sparseRGPs' native layer and hot path.
 * Plain C: pointers, sizes and enums only; no torch/HIP types in signatures
 * (streams are passed as `void*` = hipStream_t).  Matrices use R's layout:
 * column-major fp64 with an explicit leading dimension.
 *
 * Layer 1 (elementwise fillers, host buffers) replaces the Rcpp .Call routines
 * registered in src/RcppExports.cpp:284-311:
 *   sgp_make_cov      <- make_cov_matC     src/covariance_functionsC.cpp:72-169
 *                        make_cov_mat_ardC src/covariance_functionsC.cpp:191-252
 *   sgp_dsig_dtheta   <- dsig_dthetaC      src/covariance_function_derivativesC.cpp:307-552
 *                        dsig_dtheta_ardC  src/covariance_function_derivativesC.cpp:555-722
 *   sgp_kernel_pair / sgp_dkernel_pair <- the per-pair exports cov_fun_*C, dsqexp_*C
 *                        (covariance_functionsC.cpp:5-52, covariance_function_derivativesC.cpp:35-171)
 *
 * Layer 2 (fused evaluation over a device-resident context) replaces the R-level
 * hot path that calls those routines once per optimizer iteration:
 *   sgp_eval_vi     <- elbo_fun (R/vi_functions.R:64-121) + delbo_dcov_par (126-602),
 *                      with K12/K22/Z built as in norm_grad_ascent_vi (vi_functions.R:1089-1128)
 *   sgp_eval_fitc   <- obj_fun_norm (R/laplace_approx_obj_funs.R:6-52) + dlogp_dcov_par
 *                      (R/laplace_approx_gradient.R:720-1135), Z as in norm_grad_ascent
 *                      (R/laplace_gradient_ascent.R:1568-1593)
 *   sgp_vi_phase1/2, sgp_vi_finish: the same VI evaluation split at its two
 *                      row-sum reductions so a caller can all-reduce across GPUs.
 *   sgp_eval_laplace <- newtrap_sparseGP (R/newtrap_sparseGP.R:6-186) + dlogq_dcov_par
 *                      (R/laplace_approx_gradient.R:25-553), Poisson likelihood or, after
 *                      sgp_lap_set_family, Bernoulli
 *   sgp_eval_full_laplace <- newtrapGP (R/newtrapGP.R:6-177) + dlogq_dcov_par_full
 *                      (R/laplace_approx_gradient.R:558-711), the same two families
 *
 * Hyperparameters are passed as `theta` laid out [sigma, l_1..l_L, tau] with
 * L = 1 (sqexp, exp) or L = d (ard).  Gradients are d/d log(theta) in that order
 * (the reference's trans_par scale, R/laplace_approx_gradient.R:850-853).
 *
 * Errors: every entry point returns an sgp_status; sgp_last_error() gives a
 * thread-local message.  A failed Cholesky returns SGP_ENOTPD (R's chol() error,
 * caught by try() in R/knot_proposal_functions.R:641-642).
 */
#ifndef SGP_H
#define SGP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGP_ABI_VERSION 1

typedef enum {
  SGP_OK = 0,
  SGP_EINVAL = 1,  /* bad argument: unknown kernel/parameter, size, NULL        */
  SGP_ENOTPD = 2,  /* Cholesky pivot <= 0 or non-finite; see sgp_last_error()    */
  SGP_EHIP = 3,    /* HIP runtime failure                                        */
  SGP_ENOMEM = 4   /* device allocation failed                                   */
} sgp_status;

typedef enum {
  SGP_KERNEL_SQEXP = 0, /* "sqexp": sigma^2 exp(-|x-u|^2/(2 l^2))                */
  SGP_KERNEL_ARD = 1,   /* "ard":   sigma^2 exp(-sum_c ((x_c-u_c)/l_c)^2 / 2)      */
  SGP_KERNEL_EXP = 2    /* "exp":   sigma^2 exp(-sum_c |x_c-u_c| / l)  (L1)        */
} sgp_kernel;

/* flags for the fused evaluations */
#define SGP_FLAG_R_DET 1u /* reproduce R's det() overflow in log(det(K22)) */
/* objective only (elbo_fun, obj_fun_norm, newtrap_sparseGP without dlogq_dcov_par): every
 * gradient pass is skipped and grad may be NULL; the knot posterior stays available */
#define SGP_FLAG_OBJ_ONLY 2u

const char* sgp_last_error(void);
int sgp_abi_version(void);
int sgp_device_count(int* count);

/* number of hyperparameters for a kernel and input dimension d: 3 or d + 2 */
int sgp_num_params(int kernel, int d);

/* ---------------- Layer 1: elementwise fillers (host in/out) ---------------- */

/* K(x_i, x'_j) for all pairs.  x: n x d (ldx >= n), xp: np x d (ldxp >= np) or NULL for the
 * symmetric mode (R's x_pred = matrix()), which adds tau^2 + delta on the diagonal.
 * out: n x np column-major (ldo >= n).  Runs on `device` (HIP). */
int sgp_make_cov(int device, int kernel, const double* x, int64_t n, int64_t ldx,
                 const double* xp, int64_t np, int64_t ldxp, int d,
                 const double* theta, double delta, double* out, int64_t ldo);

/* d K / d log(theta_p) for all pairs; param indexes theta's layout.  Reproduces the
 * reference's quirks: tau -> 2 tau^2 iff all coordinates equal; "exp" derivatives use the
 * L2 distance; "exp" cross-mode tau returns zeros. */
int sgp_dsig_dtheta(int device, int kernel, const double* x, int64_t n, int64_t ldx,
                    const double* xp, int64_t np, int64_t ldxp, int d,
                    const double* theta, int param, double* out, int64_t ldo);

/* per-pair scalar forms (host-only, for the R shim's cov_fun_*C / dsqexp_*C exports) */
double sgp_kernel_pair(int kernel, const double* x1, const double* x2, int d, const double* theta);
double sgp_dkernel_pair(int kernel, const double* x1, const double* x2, int d,
                        const double* theta, int param);

/* ---------------- Layer 2: device-resident context + fused evaluation ---------------- */

typedef struct sgp_ctx sgp_ctx;

/* Copy X (n x d, column-major, ldx >= n), y and mu (n) to HBM on `device`; reserve work
 * space for up to m_max inducing points.  The context owns all device memory; nothing is
 * allocated per evaluation.  A context is externally synchronized (one host thread). */
int sgp_ctx_create(sgp_ctx** out, int device, const double* X, int64_t n, int64_t ldx, int d,
                   const double* y, const double* mu, int64_t m_max);
int sgp_ctx_destroy(sgp_ctx* ctx);

/* Row-sharded context over several GPUs of one node (config C4; BASELINE north_star: "sharding
 * the n observation rows across the 8 GPUs of one node with an RCCL all-reduce", SURVEY 8(b)'s
 * sgp_ctx_create(X, y, mu, n, d, ngpus)).  Shard k (k < nshards) holds the contiguous row block
 * [k*n/N + min(k, n%N), ...) -- sparsergps_amd.dist.shard_rows -- on device devices[k] (NULL:
 * device k).  The library drives the shards itself: one host thread per distinct device, the
 * row-sum reductions of every evaluation (VI and FITC: two; Laplace: two per NR iteration and
 * two for the gradient) summed on each device over its shards (fixed order) and then over the
 * devices by an in-process RCCL all-reduce (ncclCommInitAll over the distinct devices, on each
 * device's stream, in place).  A device may repeat (several shards on one GPU).
 * The handle is used with the ordinary entry points: sgp_eval_vi / sgp_eval_fitc /
 * sgp_eval_laplace / sgp_lap_nr, sgp_lap_set_f / sgp_lap_set_expo / sgp_lap_set_family /
 * sgp_lap_get_f / sgp_lap_get_grad_psi (n values
 * in the global row order) / sgp_lap_objective_values, sgp_posterior_u, sgp_ctx_enable_knot_grad,
 * sgp_knot_gradient (bounds NULL = the knot bounds of ALL rows), sgp_ctx_row_bounds (all rows),
 * sgp_ctx_set_data, sgp_ctx_rows (all rows), the three candidate scorers (each VI candidate as an
 * objective-only evaluation at [U; cand_t], m + 1 <= m_max), sgp_ego_scan (shard by shard; the
 * winner over all rows, vectors in the global row order), the timing calls (shard 0's
 * record) and sgp_ctx_destroy.  The phase-level entry points (sgp_vi_phase1 ... sgp_lap_step),
 * sgp_ctx_set_stream, sgp_ctx_set_packed_reduction, sgp_eval_full, sgp_eval_full_laplace and
 * sgp_full_laplace_state return SGP_EINVAL.
 * 1 <= nshards <= min(n, 64). */
int sgp_ctx_create_multi(sgp_ctx** out, const int* devices, int nshards, const double* X,
                         int64_t n, int64_t ldx, int d, const double* y, const double* mu,
                         int64_t m_max);
/* shards and distinct devices of a context (1 and 1 for sgp_ctx_create's) */
int sgp_ctx_shards(const sgp_ctx* ctx, int* nshards, int* ndevices);
/* launch on this hipStream_t; NULL selects the context's own (non-blocking) stream */
int sgp_ctx_set_stream(sgp_ctx* ctx, void* hip_stream);
/* replace y / mu (e.g. Laplace pseudo-data); host buffers of length n */
int sgp_ctx_set_data(sgp_ctx* ctx, const double* y, const double* mu);
int64_t sgp_ctx_rows(const sgp_ctx* ctx);

/* Titsias ELBO and d ELBO / d log theta at knots U (m x d column-major, ldu >= m).
 * K22 = Kuu + delta I, Z = tau^2 + delta (vi_functions.R:733-753).  grad: num_params. */
int sgp_eval_vi(sgp_ctx* ctx, int kernel, const double* theta, const double* U, int64_t m,
                int64_t ldu, double delta, unsigned flags, double* obj, double* grad);

/* FITC log marginal likelihood and gradient (obj_fun_norm + dlogp_dcov_par). */
int sgp_eval_fitc(sgp_ctx* ctx, int kernel, const double* theta, const double* U, int64_t m,
                  int64_t ldu, double delta, unsigned flags, double* obj, double* grad);

/* Multi-GPU VI: each rank owns a row block of X.  phase1 writes its partial first
 * reduction (sgp_vi_red1_count doubles) to the DEVICE buffer red1; the caller sums red1
 * over ranks in place (e.g. RCCL all-reduce); phase2 consumes the reduced red1 and writes
 * its partial second reduction (sgp_vi_red2_count doubles) to red2; after summing red2 over
 * ranks, sgp_vi_finish returns the objective and gradient.  n_global = total rows. */
int64_t sgp_vi_red1_count(int64_t m);
int64_t sgp_vi_red2_count(int kernel, int d);
int sgp_vi_phase1(sgp_ctx* ctx, int kernel, const double* theta, const double* U, int64_t m,
                  int64_t ldu, double delta, double* red1);
int sgp_vi_phase2(sgp_ctx* ctx, const double* red1, int64_t n_global, unsigned flags, double* red2);
int sgp_vi_finish(sgp_ctx* ctx, const double* red2, double* obj, double* grad);
/* Packed first reduction (multi-GPU VI): with packing on, phase1 writes S as its lower 64 x 64
 * blocks only -- the (mp/64)(mp/64 + 1)/2 blocks of 4096 doubles, block (r, c) with r >= c
 * at index r (r + 1) / 2 + c, row-major inside -- followed by t (mp) and r'r, i.e.
 * sgp_vi_red1_packed_count(m) doubles instead of sgp_vi_red1_count(m) (53 % of it at
 * m = 1024), and phase2 unpacks the summed buffer on the device.  Only the all-reduce between
 * the phases sees the layout; the result is the same. */
int64_t sgp_vi_red1_packed_count(int64_t m);
int sgp_ctx_set_packed_reduction(sgp_ctx* ctx, int enable);

/* Multi-GPU FITC (three steps, two all-reduces): red1 = [S_D, t, r'D^-1 r, sum log Z],
 * red2 = [S_omega, ..., sum omega, contraction records]; sgp_fitc_finish runs the replicated
 * m x m tail on the device and returns the objective and gradient. */
int64_t sgp_fitc_red1_count(int64_t m);
int64_t sgp_fitc_red2_count(int kernel, int d, int64_t m);
int sgp_fitc_phase1(sgp_ctx* ctx, int kernel, const double* theta, const double* U, int64_t m,
                    int64_t ldu, double delta, double* red1);
int sgp_fitc_phase2(sgp_ctx* ctx, const double* red1, int64_t n_global, unsigned flags,
                    double* red2);
int sgp_fitc_finish(sgp_ctx* ctx, const double* red2, double* obj, double* grad);

/* Sparse Laplace (config 5; Poisson likelihood unless sgp_lap_set_family chose another): one
 * evaluation = newtrap_sparseGP warm-started from the
 * context's latent vector f (R/newtrap_sparseGP.R:6-186, obj_fun_pois
 * R/laplace_approx_obj_funs.R:108-174) followed by dlogq_dcov_par at the mode
 * (R/laplace_approx_gradient.R:25-553), exactly as one iteration of laplace_grad_ascent
 * (R/laplace_gradient_ascent.R:510-541).  K22 = Kuu + (tau^2 + delta) I (quirk Q1).
 * expo = the Poisson exposure `m` of the reference's likelihood helpers
 * (R/derivative_functions_of_data_likelihoods.R:7-61): a positive scalar for every row, or
 * SGP_EXPO_ROWS for the per-row exposure of sgp_lap_set_expo; tol/maxit = tol_nr/maxit_nr.
 * The mode f stays resident in the context and warm-starts the next evaluation; its value
 * at context creation is 0, the reference starts at log(mean(y)) - log(expo)
 * (R/optimize_gp.R:480): set it with sgp_lap_set_f.  obj = the last NR objective value
 * (log q(y | theta, xu, f_hat)); nr_iters = length(objective_function_values).
 * maxit = 0 skips the NR loop: objective and dlogq_dcov_par at the resident f as given. */
int sgp_lap_set_f(sgp_ctx* ctx, const double* f /* n host values, or NULL */, double fill);
/* Per-row Poisson exposure: the reference's `m` is "a vector of the areas of each grid cell"
 * (R/derivative_functions_of_data_likelihoods.R:38), passed through unchanged from
 * optimize_gp's `a` (R/optimize_gp.R:461-468) and used element-wise (-m * exp(ff), y * log(m)).
 * a = n host values (each > 0 and finite; SGP_EINVAL names the first that is not), or NULL for
 * every row = fill.  The vector stays resident; a Laplace evaluation (sgp_eval_laplace,
 * sgp_lap_nr, sgp_lap_begin, sgp_lap_candidates) called with expo = SGP_EXPO_ROWS uses it, and
 * a positive expo keeps meaning that exposure on every row.  Multi-device contexts take the n
 * values in the global row order. */
#define SGP_EXPO_ROWS 0.0
int sgp_lap_set_expo(sgp_ctx* ctx, const double* a /* n host values, or NULL */, double fill);
/* Likelihood family of the sparse Laplace path.  The setting is resident on the context (as
 * the per-row exposure is; default SGP_FAM_POISSON) and honoured by sgp_eval_laplace,
 * sgp_lap_nr, sgp_lap_begin / sgp_lap_step, sgp_lap_candidates, sgp_lap_get_grad_psi and
 * sgp_posterior_u; a multi-device context forwards it to every shard.
 * SGP_FAM_BERNOULLI is the reference's family = "bernoulli" (R/optimize_gp.R:570-665): the same
 * newtrap_sparseGP / dlogq_dcov_par algebra with, for pi = 1/(1 + exp(-f)) and pi' = pi (1 - pi),
 *   d1 = y (1 - pi) - pi + y pi        (R/derivative_functions_of_data_likelihoods.R:182)
 *   W = d2 = (1 - 2 pi)(y - pi) - (y (1 - pi)^2 + pi^2 + y pi^2)       (l.108-109; the same in
 *        obj_fun_bern, R/laplace_approx_obj_funs.R:225-226)
 *   W3 = d3 = -2 pi' (y - pi) - pi' (1 - 2 pi) - (2 y (1 - pi)(-pi') + 2 pi pi' + 2 y pi pi')
 *        (l.141-142)
 *   log p = sum y plogis(f, log.p = TRUE) + (1 - y) plogis(-f, log.p = TRUE)
 *        (obj_fun_bern, R/laplace_approx_obj_funs.R:209-210, 249-251)
 * reproduced as written: for y = 1 that W is -pi - pi^2 rather than -pi (1 - pi) (DESIGN.md
 * quirk Q19).  The exposure argument is validated as for Poisson but not read; the reference
 * starts NR at f = 0 (R/optimize_gp.R:583).  Every response must be 0 or 1: SGP_EINVAL names the
 * first that is not, checked here and whenever sgp_ctx_set_data replaces y under this family
 * (not per evaluation); the family is left as it was.  An unknown family is SGP_EINVAL. */
enum { SGP_FAM_POISSON = 0, SGP_FAM_BERNOULLI = 1,
       SGP_FAM_GAUSSIAN = 2 /* sgp_nlp / sgp_predict_nlp only: sgp_lap_set_family refuses it */ };
int sgp_lap_set_family(sgp_ctx* ctx, int family);
int sgp_lap_get_f(sgp_ctx* ctx, double* f /* n host values */);
/* grad psi of the last Newton-Raphson step (n host values): the `gradient` element
 * newtrap_sparseGP returns (R/newtrap_sparseGP.R:183-184) -- evaluated at the mode estimate
 * that step started from, as the reference's loop leaves it.  SGP_EINVAL unless an NR step
 * has run since the last NR run began (sgp_lap_begin; a maxit = 0 evaluation takes no step),
 * and after sgp_lap_set_f or OAT candidate scoring. */
int sgp_lap_get_grad_psi(sgp_ctx* ctx, double* grad_psi);
/* objective_function_values of the last NR run (first min(count, max_n) copied; *count = all) */
int sgp_lap_objective_values(sgp_ctx* ctx, double* out, int max_n, int* count);
int sgp_eval_laplace(sgp_ctx* ctx, int kernel, const double* theta, const double* U, int64_t m,
                     int64_t ldu, double delta, double expo, double tol, int maxit,
                     double* obj, double* grad, int* nr_iters);

/* Multi-GPU Laplace as a reduction state machine.  sgp_lap_begin writes this rank's partial
 * sums (count doubles) to the DEVICE buffer red_out; the caller sums them over ranks in place,
 * then calls sgp_lap_step(red_in = the summed buffer, red_out = a different buffer) until
 * *done; each step reports the next count.  Every rank takes identical decisions (they
 * are functions of the summed buffers only).  Buffers hold sgp_lap_red_count doubles. */
int64_t sgp_lap_red_count(int kernel, int d, int64_t m);
int sgp_lap_begin(sgp_ctx* ctx, int kernel, const double* theta, const double* U, int64_t m,
                  int64_t ldu, double delta, double expo, double tol, int maxit, unsigned flags,
                  double* red_out, int64_t* count);
int sgp_lap_step(sgp_ctx* ctx, const double* red_in, double* red_out, int64_t* count,
                 int* done, double* obj, double* grad, int* nr_iters);
/* newtrap_sparseGP alone (R/newtrap_sparseGP.R:6-186): the NR loop from the resident f, f left
 * at the mode; obj = the last entry of objective_function_values (= sgp_lap_begin with
 * SGP_FLAG_OBJ_ONLY driven to completion) */
int sgp_lap_nr(sgp_ctx* ctx, int kernel, const double* theta, const double* U, int64_t m,
               int64_t ldu, double delta, double expo, double tol, int maxit, double* obj,
               int* nr_iters);

/* Full (non-sparse) Gaussian GP over the context's n rows (config 1; requires m_max >= n):
 * obj = log dmvnorm(y; mu, Sigma11) (obj_fun_norm_full, R/laplace_approx_obj_funs.R:56-61) and
 * grad = dlogp_dcov_par_full (R/laplace_approx_gradient.R:1140-1269; its alpha is Sigma11^-1 y,
 * not Sigma11^-1 (y - mu)), Sigma11 = k(xy, xy) + (tau^2 + delta) I.  SGP_FLAG_OBJ_ONLY skips
 * the gradient (grad may be NULL). */
int sgp_eval_full(sgp_ctx* ctx, int kernel, const double* theta, double delta, unsigned flags,
                  double* obj, double* grad);

/* Full (non-sparse) Laplace GP over the context's n rows for the Poisson or Bernoulli family
 * (optimize_gp.R:687-732; requires m_max >= n; SGP_KERNEL_EXP and multi-device contexts are
 * refused as by sgp_eval_full): one evaluation = newtrapGP warm-started from the context's
 * resident f (R/newtrapGP.R:6-177 with obj_fun_pois_full / obj_fun_bern_full,
 * R/laplace_approx_obj_funs.R:67-102, 346-397, and grad_loglik_fn_pois_full / _bern_full,
 * R/derivative_functions_of_data_likelihoods.R:65-84, 239-267) followed by dlogq_dcov_par_full at
 * the mode (R/laplace_approx_gradient.R:558-711), exactly as one iteration of
 * laplace_grad_ascent_full (R/laplace_gradient_ascent.R:742-771, 957-985).
 * Sigma = k(xy, xy) + (tau^2 + delta) I.  Family, exposure and f are the context's resident ones
 * (sgp_lap_set_family, sgp_lap_set_expo / expo as for sgp_eval_laplace, sgp_lap_set_f /
 * sgp_lap_get_f); the mode stays resident and warm-starts the next evaluation.  tol / maxit =
 * tol_nr / maxit_nr: the first update always runs (newtrapGP.R:63-75), then the loop continues
 * while iter < maxit && (|obj_k - obj_{k-1}| > tol || any(|grad psi| > tol)) (l.77) with
 * grad psi = d1 - Sigma^-1 (f - mu) at the iterate the last update started from.  maxit = 0
 * skips the NR loop: objective and dlogq_dcov_par_full at the resident f as given.
 * obj = the last NR objective value; nr_iters = length(objective_function_values) (may be NULL).
 * SGP_FLAG_OBJ_ONLY is newtrapGP alone (grad may be NULL).  sgp_lap_objective_values and
 * sgp_lap_get_grad_psi serve this path as they serve the sparse one.  SGP_ENOTPD names the
 * matrix (Sigma, or I + sqrt(-W) Sigma sqrt(-W)) that is not positive definite or not finite. */
int sgp_eval_full_laplace(sgp_ctx* ctx, int kernel, const double* theta, double delta,
                          double expo, double tol, int maxit, unsigned flags, double* obj,
                          double* grad, int* nr_iters);
/* newtrapGP's returned `W` and `grad_log_py_ff` (R/newtrapGP.R:96-99), n host values each: the
 * likelihood's second and first derivatives at the iterate the LAST UPDATE STARTED FROM, not at
 * the returned mode, as the reference's loop leaves them (l.69-72, 83-86) and as
 * predict_laplace_full consumes them.  SGP_EINVAL unless a full-Laplace NR step has run since
 * the mode was last set (a maxit = 0 evaluation takes no step). */
int sgp_full_laplace_state(sgp_ctx* ctx, double* W, double* grad_log_py_ff);

/* Posterior of the knot values u at the end of a fit, from the context's last completed
 * evaluation (VI: vi_functions.R:1161-1180; FITC: laplace_gradient_ascent.R:1635-1655;
 * Laplace: newtrap_sparseGP.R:137-176).  muu, u_mean: m host values; u_var: m x m host,
 * column-major (ld m).
 * "Completed" is exact: an evaluation forgets its predecessor when it starts (it overwrites
 * m, the knots and the m x m state this reads) and counts only once it has returned SGP_OK.
 * After an evaluation that failed (SGP_ENOTPD included), after any of the three candidate
 * scorers below, and on a new context, this returns SGP_EINVAL ("no completed evaluation");
 * sgp_knot_gradient follows the same rule.  Evaluate again to ask again. */
int sgp_posterior_u(sgp_ctx* ctx, const double* muu, double* u_mean, double* u_var);

/* Sparse prediction at x_pred (np x d, column-major, ld ldxp) from a knot posterior:
 *   SGP_PRED_VI      predict_vi      (R/vi_functions.R:1222-1333; gaussian only)
 *   SGP_PRED_LAPLACE predict_laplace (R/laplace_approx_prediction.R:3-123; FITC or Laplace fits,
 *                    gaussian != 0 selects the family == "gaussian" Sigma22)
 *   SGP_PRED_FULL    predict_gp_full (R/laplace_approx_prediction.R:281-405): a full Gaussian
 *                    GP -- U = xy, u_mean = y, muu = mu, u_var unused (may be NULL)
 *   SGP_PRED_LAPLACE_FULL predict_laplace_full (R/laplace_approx_prediction.R:128-214): a full
 *                    Poisson / Bernoulli Laplace fit -- U = xy, u_mean = grad_log_py_ff and
 *                    muu = W as sgp_full_laplace_state returns them (every W <= 0, else
 *                    SGP_EINVAL), u_var unused (may be NULL):
 *                      pred_mean = mu_pred + k(x_pred, xy) grad_log_py_ff                (l.209)
 *                      pred_var  = Sigma11(x_pred) - k(x_pred, xy) R k(xy, x_pred),
 *                                  R = sqrt(-W) (I + sqrt(-W) Sigma sqrt(-W))^-1 sqrt(-W)
 *                                  (= t(v) %*% v, l.169, 188, 206)
 *                    The reference defines pred_mean only when full_cov is FALSE (l.190-210) and
 *                    fails otherwise; here the mean is returned in both forms.
 * as dispatched by predict_gp (R/laplace_approx_prediction.R:408-542).  u_var is m x m
 * column-major (ld ldv).  pred_var: np values, or with full_cov the np x np matrix
 * (column-major, ld ldpv).  Host buffers; device work space is allocated per call.
 * SGP_KERNEL_EXP is refused with SGP_EINVAL before any device work: the reference's fits never
 * carry that kernel (optimize_gp.R:263), so there is no fitted posterior to predict from. */
enum { SGP_PRED_VI = 0, SGP_PRED_LAPLACE = 1, SGP_PRED_FULL = 2, SGP_PRED_LAPLACE_FULL = 3 };
int sgp_predict(int device, int kernel, const double* theta, double delta, int method,
                int gaussian, const double* U, int64_t m, int64_t ldu, const double* u_mean,
                const double* muu, const double* u_var, int64_t ldv, const double* x_pred,
                int64_t np, int64_t ldxp, int d, const double* mu_pred, int full_cov,
                double* pred_mean, double* pred_var, int64_t ldpv);

/* Held-out scoring: the reference's my_nlp(mc = FALSE, mv = FALSE) (R/evaluation_functions.R:12-145)
 * over n test rows -- nlp[i] = -log int p(y_i | f) N(f; pred_mean_i, pred_var_i) df:
 *   SGP_FAM_GAUSSIAN   -dnorm(y, pred_mean, sqrt(pred_var + tau^2), log = TRUE) (l.14-20), par = tau;
 *                      pred_var + tau^2 as written, although the sparse predictors' pred_var
 *                      already holds tau^2
 *   SGP_FAM_BERNOULLI  p = dbinom(y, 1, my_logistic(f)) (l.30-52); par is ignored
 *   SGP_FAM_POISSON    p = dpois(y, exp(f) m) (l.84-110), par = the scalar exposure m > 0 (the
 *                      reference's par$m), or expo = n per-row exposures (par is then not read)
 * The reference calls R's integrate() once per row in a loop; here every row's integral is taken
 * in one launch by a fixed rule accurate to fp64 rounding (mode, level set, 128-point midpoint
 * rule in log space: DESIGN.md sec. 0j).  integrate()'s infinite-range rule misses narrow
 * integrands and returns 0 (nlp = Inf), and its linear-space integrand underflows; neither is
 * reproduced (quirks Q21, Q22).
 * stats[4] = {sum of the finite nlp values, their count, the count of NaN rows,
 * sum (pred_mean - y)^2}, each added in a fixed order (bit-identical on repeat).
 * SGP_EINVAL before any device call for: a NULL pointer (expo may be NULL), n < 1, an unknown
 * family, a non-finite y, a bernoulli y outside {0, 1}, a poisson y that is negative or not an
 * integer (R: a warning and probability 0; quirk Q24), a poisson exposure that is not positive and
 * finite, a gaussian tau that is not finite or < 0, expo given for another family than poisson.
 * Data problems are not errors: a row whose pred_mean is not finite, or whose variance (gaussian:
 * pred_var + tau^2) is not finite or <= 0, gets nlp = NaN and is counted in stats[2]; every other
 * row is unaffected (the reference stops in integrate with "non-finite function value"). */
int sgp_nlp(int device, int family, const double* y, const double* pred_mean,
            const double* pred_var, int64_t n, double par, const double* expo, double* nlp,
            double* stats /* 4 */);

/* sgp_predict(..., full_cov = 0) followed by sgp_nlp of its result against y_pred (np values),
 * as the reference's experiment scripts do (exec/boston.R:191-201, exec/airfoil.R:181-191,
 * exec/ccpp.R:168-178), without the round trip: the prediction's device stages run as in
 * sgp_predict, pred_mean and pred_var are formed and scored on the device, and the np-vectors are
 * read back once.  pred_mean and pred_var are bit-identical to sgp_predict's and nlp / stats to
 * sgp_nlp's on those vectors.  Arguments and errors as the two entries'. */
int sgp_predict_nlp(int device, int kernel, const double* theta, double delta, int method,
                    int gaussian, const double* U, int64_t m, int64_t ldu, const double* u_mean,
                    const double* muu, const double* u_var, int64_t ldv, const double* x_pred,
                    int64_t np, int64_t ldxp, int d, const double* mu_pred, double* pred_mean,
                    double* pred_var, int family, const double* y_pred, double par,
                    const double* expo, double* nlp, double* stats /* 4 */);

/* A resident predictor: sgp_predict(full_cov = 0) split into the work that
 * depends on the fit alone, done once by sgp_predictor_create, and the work per batch of
 * prediction rows, done by the run entries on any number of batches of any size.  The same
 * reference functions, by `method` (all four SGP_PRED_*): predict_vi (R/vi_functions.R:1222-1333),
 * predict_laplace (R/laplace_approx_prediction.R:3-123), predict_gp_full
 * (R/laplace_approx_prediction.R:281-405) and predict_laplace_full
 * (R/laplace_approx_prediction.R:128-214), as dispatched by predict_gp
 * (R/laplace_approx_prediction.R:408-542).  Every method is
 *   pred_mean_i = mu_pred_i + k_i^T w,   pred_var_i = c0 + k_i^T T22 k_i,   k_i = k(x_pred_i, U)
 * with w (m), T22 (m x m, symmetric) and c0 fixed by the fit.
 *
 * create: arguments, their meaning per method and the errors are sgp_predict's.  SGP_EINVAL
 * before the first device call (sgp_diag_predictor_args, sgp_diag.h, is the same check) for: a
 * kernel other than SGP_KERNEL_SQEXP / SGP_KERNEL_ARD (SGP_KERNEL_EXP: optimize_gp.R:263), d
 * outside [1, 32], an unknown method, a NULL pointer (u_var may be NULL for SGP_PRED_FULL and
 * SGP_PRED_LAPLACE_FULL), m < 1, ldu < m, ldv < m (sparse methods), a non-finite theta, delta,
 * u_mean, muu, U or u_var entry, sigma <= 0, tau < 0, a length scale <= 0, a W > 0
 * (SGP_PRED_LAPLACE_FULL), and SGP_PRED_VI with gaussian = 0 (the reference's message).  A
 * Sigma22 that is not positive definite is SGP_ENOTPD with sgp_predict's text and leading-minor
 * order.  create runs sgp_predict's m x m stage once on a stream the predictor owns and keeps U,
 * w, T22 (also in the symmetric block form the batches use) and c0 on `device`; full_cov stays
 * with sgp_predict.
 *
 * run: host buffers.  x_pred (np x d column-major, ld ldxp) is streamed in chunks of rows (a
 * multiple of 128 whose m-wide K work space stays within a fixed byte budget); np is limited by
 * host memory only.  The K12 builder's form is chosen once from the column range of the whole
 * x_pred, so every chunk uses it.  A row's result has a fixed summation order: it does not
 * depend on the chunking or the repeat (bit-identical).
 *
 * run_nlp: run, then sgp_nlp of the result against y_pred without the round trip.  pred_mean and
 * pred_var are bit-identical to run's, nlp and stats to sgp_nlp's on those vectors.  The
 * scoring kernel's final pass adds its 256-row partials in an order that spans all rows (thread
 * t takes tiles t, t + 256, ...), so stats cannot be carried from chunk to chunk bit for bit:
 * pred_mean and pred_var are assembled on the device (16 np bytes) and scored once there.
 * Arguments and errors of the scoring part as sgp_nlp's.
 *
 * run_dev: x_pred, mu_pred, pred_mean, pred_var are device pointers on the predictor's device
 * (x_pred column-major with ld ldxp); the work is queued on `stream` (a hipStream_t, NULL = the
 * null stream) and the call does not wait for it.  box_lo / box_hi: d host values each bounding
 * every coordinate of x_pred (a wrong box costs accuracy in K, never memory safety), or NULL for
 * the builder's exact-difference form.  With the box equal to x_pred's column range the result
 * is bit-identical to run's.
 *
 * A predictor serves one run at a time (its chunk work space is shared): calls from one host
 * thread on one stream are ordered by that stream; a caller that changes streams, or mixes
 * run_dev with the host entries, synchronises the earlier stream first.  destroy waits for the
 * predictor's own stream; NULL is SGP_EINVAL for run and destroy. */
typedef struct sgp_predictor sgp_predictor;
int sgp_predictor_create(sgp_predictor** out, int device, int kernel, const double* theta,
                         double delta, int method, int gaussian, const double* U, int64_t m,
                         int64_t ldu, int d, const double* u_mean, const double* muu,
                         const double* u_var, int64_t ldv);
int sgp_predictor_destroy(sgp_predictor* p);
int sgp_predictor_run(sgp_predictor* p, const double* x_pred, int64_t np, int64_t ldxp,
                      const double* mu_pred, double* pred_mean, double* pred_var);
int sgp_predictor_run_nlp(sgp_predictor* p, const double* x_pred, int64_t np, int64_t ldxp,
                          const double* mu_pred, double* pred_mean, double* pred_var, int family,
                          const double* y_pred, double par, const double* expo, double* nlp,
                          double* stats /* 4 */);
int sgp_predictor_run_dev(sgp_predictor* p, const double* x_pred, int64_t np, int64_t ldxp,
                          const double* mu_pred, double* pred_mean, double* pred_var,
                          const double* box_lo, const double* box_hi, void* stream);

/* A batch of small-knot VI problems: B independent Titsias-VI problems, each
 * with its own rows, theta and at most SGP_BATCH_MMAX knots, evaluated together in four kernel
 * launches (the folds of a cross-validation, repeated splits, the starts of a multi-start search).
 * Per problem the semantics are exactly sgp_eval_vi's: K22 = Kuu + delta I, Z = tau^2 + delta,
 * elbo_fun (R/vi_functions.R:64-121), trace_term_fun (R/vi_functions.R:14-27) and delbo_dcov_par
 * (R/vi_functions.R:126-419) with the gradient in log theta in sgp_num_params order, knots fixed,
 * the tau coincidence rule (quirk Q5) for rows that equal a knot exactly, and SGP_FLAG_R_DET /
 * SGP_FLAG_OBJ_ONLY with their sgp_eval_vi meaning (SGP_FLAG_OBJ_ONLY skips the second row pass).
 *
 * create: X (nrows x d column-major, ld ldx), y and mu (nrows each) are uploaded once; problem b's
 * rows are [row0[b], row0[b] + nrow[b]) of them.  Ranges may overlap or coincide (a multi-start
 * aliases one range B times).  The batch owns all its device memory; an evaluation allocates
 * nothing.  An sgp_batch is externally synchronised, like an sgp_ctx, and lives on one device.
 *
 * eval_vi: theta is P x B (column b = problem b, ld ldt), problem b's knots are m[b] x d
 * column-major with ld m[b] at U + uoff[b]; grad is P x B with ld ldg (not read or written under
 * SGP_FLAG_OBJ_ONLY, where it may be NULL).  active (B bytes, NULL = all): where active[b] == 0
 * nothing of problem b is computed and nothing is written to its obj / grad / status or to its
 * posterior state.  SGP_EINVAL before the first device call (sgp_diag_batch_args, sgp_diag.h, is
 * the same check) for: a NULL pointer, B < 1, d outside [1, 32], nrow[b] < 1, a range leaving
 * [0, nrows), ldx < nrows, an active m[b] outside [1, SGP_BATCH_MMAX], ldt or ldg < P, a kernel
 * other than SGP_KERNEL_SQEXP / SGP_KERNEL_ARD (SGP_KERNEL_EXP is refused as sgp_predict refuses
 * it), a non-finite delta or knot, and a theta entry that is not finite and positive.
 * A problem whose K22 or K22 + K21 Z^-1 K12 is not positive definite does not fail the call:
 * status[b] is the 1-based order of the first non-positive leading minor, positive for Sigma22
 * (K22) and negative for K22 + K21 Z^-1 K12, its obj and grad are NaN, the other problems are
 * unaffected, the call returns SGP_OK and sgp_last_error() names the first such problem (the
 * per-candidate convention of sgp_vi_candidates).  status[b] = 0 otherwise.
 * Every sum has a fixed order: a problem's obj, grad, status and posterior depend on its own rows,
 * theta, U, m, delta and flags only -- not on B, its position, the other problems, `active` or
 * the repeat -- bit for bit.
 *
 * posterior_u: the knot posterior (R/vi_functions.R:1161-1180) of each problem's last successful
 * evaluation, as sgp_posterior_u gives it for a context; muu and u_mean are packed like U's
 * columns (sum m_b values), u_var as m_b x m_b column-major blocks (sum m_b^2), with m_b the knot
 * count of that evaluation; a problem that has none takes no entries (m_b = 0), and SGP_EINVAL
 * when no problem has one.  set_data replaces y and mu (nrows values each) and drops the
 * posteriors. */
#define SGP_BATCH_MMAX 64
typedef struct sgp_batch sgp_batch;
int sgp_batch_create(sgp_batch** out, int device, const double* X, int64_t nrows, int64_t ldx,
                     int d, const double* y, const double* mu, const int64_t* row0,
                     const int64_t* nrow, int64_t B);
int sgp_batch_destroy(sgp_batch* b);
int sgp_batch_set_data(sgp_batch* b, const double* y, const double* mu);
int sgp_batch_eval_vi(sgp_batch* b, int kernel, const double* theta, int64_t ldt, const double* U,
                      const int64_t* uoff, const int64_t* m, double delta, unsigned flags,
                      const unsigned char* active, double* obj, double* grad, int64_t ldg,
                      int* status);
int sgp_batch_posterior_u(sgp_batch* b, const double* muu, double* u_mean, double* u_var);

/* sgp_batch_eval_vi with the knot gradient: delbo_dcov_par's knot branch
 * (R/vi_functions.R:425-593) with dsqexp_dx2 / dsqexp_dx2_ard
 * (R/covariance_function_derivatives.R:178-302), the derivative kind following `kernel`, as
 * optimize_gp's xu_opt = "simultaneous" uses it (R/optimize_gp.R:317-333, 396-412).  The
 * arguments up to status are sgp_batch_eval_vi's, and obj, grad, status and the posterior state
 * are bit-identical to what sgp_batch_eval_vi gives for them: the same four launches run, and two
 * more behind them.
 *   bounds: per problem a d x 2 column-major [lower | upper] block, problem b's at
 *           bounds + 2 d b: the gradient is with respect to the unbounded knot coordinate of the
 *           reference's transform, dELBO/du_kc * (ub_c - lb_c) / ((u_kc - lb_c)(ub_c - u_kc) + 1e-4)
 *           (quirk Q8).  NULL: the factor is 1 and the result is the plain dELBO/du_kc.
 *   grad_knot: problem b's m[b] d values at grad_knot + uoff[b], knot-major (entry k d + c is knot
 *           k's coordinate c; quirk Q16) -- U's packing, so U's length serves.
 * A problem that is not positive definite gets a NaN grad_knot beside its NaN obj and grad; where
 * active[b] == 0 nothing of problem b's grad_knot is written.  SGP_EINVAL before the first device
 * call (sgp_diag_batch_knot_args, sgp_diag.h, is the same check) for what sgp_batch_eval_vi
 * refuses and for a NULL grad_knot, SGP_FLAG_OBJ_ONLY and a non-finite bound of an active problem.
 * The call makes one copy to the device and one back and allocates nothing.  The fixed-order rule
 * of sgp_batch_eval_vi covers grad_knot: bit for bit independent of B, the position, the other
 * problems, `active` and the repeat. */
int sgp_batch_eval_vi_knots(sgp_batch* b, int kernel, const double* theta, int64_t ldt,
                            const double* U, const int64_t* uoff, const int64_t* m, double delta,
                            unsigned flags, const unsigned char* active, double* obj, double* grad,
                            int64_t ldg, int* status, const double* bounds /* NULL: raw */,
                            double* grad_knot);

/* The batch's other Gaussian objective, FITC: what optimize_gp(vi = FALSE), the
 * reference's own default, fits.  The arguments, their check (the same sgp_diag_batch_args, before
 * the first device call), the limits, `active`, the status convention and the fixed-order rule are
 * sgp_batch_eval_vi's; per problem the semantics are exactly sgp_eval_fitc's: K22 = Kuu + delta I,
 * Z_i = sigma^2 + tau^2 + delta - k_i^T K22^-1 k_i (R/laplace_gradient_ascent.R:1238-1263),
 * obj_fun_norm (R/laplace_approx_obj_funs.R:6-52) and dlogp_dcov_par
 * (R/laplace_approx_gradient.R:720-971) with the gradient in log theta in sgp_num_params order,
 * knots fixed, dK22 / dlog tau = 0 (l.899-902), the tau coincidence rule (quirk Q5: a row that
 * equals a knot exactly gets dK12 / dlog tau = 2 tau^2), and SGP_FLAG_R_DET / SGP_FLAG_OBJ_ONLY
 * with their sgp_eval_fitc meaning.  Five kernel launches evaluate the whole batch (three under
 * SGP_FLAG_OBJ_ONLY, which skips the gradient's row pass and its m x m stage).
 * status[b] = +k when the first non-positive leading minor, of order k, is in Sigma22 (K22) and
 * -k when it is in K22 + K21 Z^-1 K12; obj and grad of that problem are NaN and the call returns
 * SGP_OK.  A row whose Z_i is not positive and finite (the reference's log(Z) is NaN there; with
 * an SPD K22 Z_i >= tau^2 + delta up to rounding, so only a negative delta reaches it) makes the
 * problem's obj and grad NaN with status[b] = 0.  Either way the problem writes nothing to its
 * posterior state.
 * The posterior state of a successful problem is Bm^-1, u = Bm^-1 t (no 1 / z) and its
 * parameters, where sgp_batch_eval_vi leaves them, with the objective recorded beside them:
 * sgp_batch_posterior_u then gives laplace_gradient_ascent.R:1635-1655 (u_mean - muu = K22 u,
 * u_var = K22 Bm^-1 K22) and sgp_batch_predict gives predict_laplace(family = "gaussian")
 * (R/laplace_approx_prediction.R:3-123):
 *   pred_mean_i = mu_i + k_i^T u
 *   pred_var_i  = (sigma^2 + tau^2) + k_i^T (Bm^-1 - K22^-1) k_i        -- no delta, unlike predict_vi
 * and the same nlp_i, for every problem whose last successful evaluation was FITC; one batch may
 * hold problems of both kinds.  A problem's FITC result does not depend on whether earlier calls
 * on the batch were VI or FITC, nor does a VI result. */
int sgp_batch_eval_fitc(sgp_batch* b, int kernel, const double* theta, int64_t ldt,
                        const double* U, const int64_t* uoff, const int64_t* m, double delta,
                        unsigned flags, const unsigned char* active, double* obj, double* grad,
                        int64_t ldg, int* status);

/* Laplace fits on a batch: Poisson counts and Bernoulli classes, what
 * optimize_gp(family = "poisson" / "bernoulli", sparse = TRUE) fits (R/optimize_gp.R:440-665).
 *
 * sgp_batch_lap_init: family is SGP_FAM_POISSON or SGP_FAM_BERNOULLI (SGP_FAM_GAUSSIAN and unknown
 * values: SGP_EINVAL).  expo: nrows host values, resident like y, each finite and > 0, or NULL for
 * 1 on every row: the reference's `m` (R/derivative_functions_of_data_likelihoods.R:7-61); it is
 * validated for both families and read only by Poisson.  Under Bernoulli every y in any problem's
 * range must be 0 or 1 (SGP_EINVAL names the first that is not), and sgp_batch_set_data repeats
 * that check once the family is set.  The call allocates all the device and pinned memory a
 * Laplace evaluation needs (the evaluation allocates nothing), among it the latent vectors,
 * indexed by (problem, local row): sum nrow[b] doubles packed in problem order, never by resident
 * row, so aliased row ranges (a multi-start) need nothing further.  f starts at 0.  The call may
 * be repeated: it then replaces family and exposure and resets f.  sgp_diag_batch_lap_args
 * (sgp_diag.h) is the same check without a device.
 *
 * sgp_batch_lap_set_f / sgp_batch_lap_get_f: f is packed by problem (sum nrow[b] values).  With
 * f == NULL, fill holds B values, one per problem: the reference starts Poisson at
 * log(mean y) - log(expo) (R/optimize_gp.R:480) and Bernoulli at 0 (R/optimize_gp.R:583).
 *
 * sgp_batch_eval_laplace: the arguments up to status are sgp_batch_eval_vi's, checked by the same
 * function (sgp_diag_batch_args) before the first device call; then tol, maxit and nr_iters (B).
 * Per problem the semantics are exactly sgp_eval_laplace's: K22 = Kuu + (tau^2 + delta) I (quirk
 * Q1); newtrap_sparseGP (R/newtrap_sparseGP.R:6-186) warm-started from the problem's resident f:
 * the objective at the start, one update unconditionally, then the reference's stop rule (l.100:
 * while iter < maxit and (|obj step| > tol or any |grad psi| > tol)); obj[b] is the last NR
 * objective, nr_iters[b] = length(objective_function_values); maxit = 0 means objective and
 * gradient at f as given; then dlogq_dcov_par (R/laplace_approx_gradient.R:25-336) at the mode, in
 * log theta in sgp_num_params order with the knots fixed, with the tau terms of DESIGN.md sec. 3.3
 * and quirk Q5.  SGP_FLAG_OBJ_ONLY is NR alone (grad may be NULL); SGP_FLAG_R_DET is not read.
 * The three m-vector solves of an evaluation take one step of iterative refinement under
 * Bernoulli and none under Poisson, as the context route's do.  The resident
 * f of an evaluated problem is left at the mode.
 * status[b] = +k when the first non-positive leading minor, of order k, is in Sigma22 (K22) and
 * -k when it is in K22 + S_Z or K22 + S_B; obj and grad of that problem are then NaN, the call
 * returns SGP_OK, the neighbours are unaffected, and the problem's resident f is unspecified until
 * sgp_batch_lap_set_f or sgp_batch_lap_init sets it again.
 * Every stop decision is taken on the device from the problem's own fixed-order sums; the host
 * reads back only the count of problems still running, once per iteration.
 * The posterior state of a successful problem is what sgp_posterior_u gives after
 * sgp_eval_laplace (R/newtrap_sparseGP.R:137-176): u_mean - muu = K22 (K22 + S_Z)^-1 t_Z(f) and
 * u_var = K22 (K22 + S_B(W_prev))^-1 K22 with the loop's last, one-step-stale W, where VI and FITC
 * leave theirs; sgp_batch_posterior_u then gives laplace_posterior_u and sgp_batch_predict gives
 * predict_laplace(family != "gaussian") (R/laplace_approx_prediction.R:3-123): Sigma22 with
 * tau^2 + delta on its diagonal and the constant sigma^2 + tau^2; pred_mean and pred_var are of the
 * latent f, and the nlp output, which is my_nlp(family = "gaussian"), is not this family's score.
 * No atomics, every sum in an order that depends on the problem alone, nothing read from another
 * problem: obj, grad, f, nr_iters and the posterior are bit-identical whatever the batch, the
 * position, `active`, the repeat (from the same f) and the VI / FITC calls in between. */
int sgp_batch_lap_init(sgp_batch* b, int family, const double* expo /* NULL: 1 */);
int sgp_batch_lap_set_f(sgp_batch* b, const double* f /* NULL: fill */, const double* fill);
int sgp_batch_lap_get_f(sgp_batch* b, double* f);
int sgp_batch_eval_laplace(sgp_batch* b, int kernel, const double* theta, int64_t ldt,
                           const double* U, const int64_t* uoff, const int64_t* m, double delta,
                           unsigned flags, const unsigned char* active, double* obj, double* grad,
                           int64_t ldg, int* status, double tol, int maxit, int* nr_iters);

/* Held-out prediction and scoring for a batch: predict_vi
 * (R/vi_functions.R:1222-1336) and my_nlp(family = "gaussian") (R/evaluation_functions.R:14-20,
 * with quirk Q23: pred_var + tau^2 as written) for every problem of the batch in three launches,
 * from the state each problem's last successful evaluation left on the device -- what
 * sgp_batch_posterior_u reads; a later evaluation of the problem that was not positive definite
 * does not disturb it.  With u = Bm^-1 t / z of that evaluation, u_mean - muu = K22 u and
 * u_var = K22 Bm^-1 K22, so muu cancels and, with k_i = k(x_i, U) without a nugget,
 *   pred_mean_i = mu_i + k_i^T u
 *   pred_var_i  = (tau^2 + sigma^2) + delta + k_i^T (Bm^-1 - K22^-1) k_i
 *   nlp_i       = -dnorm(y_i, pred_mean_i, sqrt(pred_var_i + tau^2), log = TRUE)
 * with the problem's own theta, knots, m and delta.  For a problem whose last successful
 * evaluation was sgp_batch_eval_fitc the same launches give predict_laplace(family = "gaussian"):
 * u carries no 1 / z and the constant is sigma^2 + tau^2 without delta (see sgp_batch_eval_fitc
 * above).
 *
 * set_test: Xt (ntest x d column-major, ld ldxt), yt (ntest values, or NULL: predict only) and
 * mut (ntest values) are uploaded once; problem b's test rows are [trow0[b], trow0[b] + tnrow[b]).
 * Ranges may overlap or coincide; tnrow[b] = 0 is allowed (nothing is written for b).  The call
 * may be repeated and then replaces the test rows; sgp_batch_set_data leaves them alone.  All
 * device and pinned memory sgp_batch_predict needs is allocated here: predict allocates nothing.
 *
 * predict: outputs are packed per problem in problem order: problem b's rows start at
 * toff[b] = sum of tnrow[b'] over all b' < b (active or not), so pred_mean, pred_var and nlp hold
 * sum tnrow values; problem b's stats are stats[4 b .. 4 b + 3] = {sum of the finite nlp, their
 * count, the count of NaN rows, sum (pred_mean - y)^2}, as sgp_nlp defines them.  nlp and stats
 * are both given or both NULL (no scoring).  active (B bytes, NULL = all): where active[b] == 0
 * nothing of problem b is computed or written.  A non-finite mut entry is data: that row's mean is
 * not finite, its nlp is NaN and it counts in stats[2] (sgp_nlp's rule).
 * SGP_EINVAL before the first device call (sgp_diag_batch_test_args, sgp_diag.h, is the same
 * check) for: a NULL handle or required pointer, ntest < 1, ldxt < ntest, tnrow[b] < 0, a range
 * leaving [0, ntest), a non-finite Xt or yt, predict before set_test, nlp with yt = NULL, exactly
 * one of nlp / stats NULL, and an active problem without a posterior (the first is named).
 * Every sum has a fixed order and no problem reads another's data: a problem's outputs do not
 * depend on B, its position, the other problems, `active` or the repeat -- bit for bit. */
int sgp_batch_set_test(sgp_batch* b, const double* Xt, int64_t ntest, int64_t ldxt,
                       const double* yt /* NULL: predict only */, const double* mut,
                       const int64_t* trow0, const int64_t* tnrow);
int sgp_batch_predict(sgp_batch* b, const unsigned char* active, double* pred_mean,
                      double* pred_var, double* nlp /* NULL: no scoring */,
                      double* stats /* 4 x B, NULL iff nlp is NULL */);

/* Joint predictive scoring and draws from a Gaussian process: the branches of
 * the reference that use a full covariance -- my_nlp(mv = TRUE), my_nlp(family = "bernoulli",
 * mc = TRUE), my_kl(mv = TRUE) (R/evaluation_functions.R:21-26, 53-80, 120-133, 153-164) -- and the
 * mvtnorm::rmvnorm draws its vignettes and exec/simulated_examples.R:15 begin with.  Device-level
 * calls with host buffers, like sgp_nlp; covariances are n x n column-major, symmetric, and only
 * their lower triangle is read.  They are factored A = L L^T on the device (right-looking
 * Cholesky in 64-wide steps); one that is not positive definite is SGP_ENOTPD, naming the matrix
 * and, as R's chol(), the order of the first leading minor that is not.
 *
 * The normal stream.  R's stream (rnorm by inversion on Mersenne-Twister, rmvnorm through an
 * eigen-decomposition) cannot be reproduced; the draws come from a counter-based stream that is
 * part of this interface, so that a host can regenerate every one:
 *   generator  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9,
 *              0xBB67AE85), key = (seed low 32 bits, seed high 32 bits)
 *   output     words w0..w3: a = ((w1 << 32) | w0) >> 12, b = ((w3 << 32) | w2) >> 12,
 *              u1 = (a + 0.5) 2^-52, u2 = (b + 0.5) 2^-52 (exact in fp64, inside (0, 1)),
 *              r = sqrt(-2 log u1); the pair r cos(2 pi u2), r sin(2 pi u2)
 *   stream 0   joint draws: draw s (0-based, 64-bit), row j (0-based) has the counter
 *              (s low, s high, j >> 1, 0) and takes the cosine value for even j, the sine value
 *              for odd j
 *   stream 1   per-row Monte Carlo: draw t of row i has the counter (q low, q high, i, 1) with
 *              q = t >> 1 and takes the cosine value for even t, the sine value for odd t
 * Draw s is f = mean + L z with z_j the stream-0 normal of (s, j).  No result depends on how the
 * draws are chunked or on the grid, and a repeat gives the same bits.
 *
 * SGP_EINVAL before any device call for: a NULL pointer (expo may be NULL), n < 1, S < 1 (where
 * draws are taken), a leading dimension below n (ldo below S), an unknown family, sgp_nlp's per-row
 * checks of y, par and expo, a non-finite mean, and n above SGP_JOINT_NMAX. */
#define SGP_JOINT_NMAX 16384
/* S draws from N(mean, cov): out is S x n column-major (ld ldo >= S), one draw per row, as
 * rmvnorm returns them.  cov is used as given: the caller adds any nugget. */
int sgp_sample_mvn(int device, const double* mean, const double* cov, int64_t n, int64_t ldc,
                   int64_t S, uint64_t seed, double* out, int64_t ldo);
/* my_nlp(mv = TRUE): out = {nlp, mcsd, nlp_se}.
 *   SGP_FAM_GAUSSIAN   -dmvnorm(y, pred_mean, pred_cov + tau^2 I, log = TRUE) (l.23-25), par = tau,
 *                      tau^2 added as written (quirk Q23); mcsd = nlp_se = NaN, S and seed unused
 *   SGP_FAM_BERNOULLI, SGP_FAM_POISSON
 *                      the reference's Monte Carlo estimate over S joint draws f_s (l.66-80,
 *                      120-133), in log space: ll_s = sum_i log p(y_i | f_si) with
 *                      p = dbinom(y, 1, my_logistic(f)) or dpois(y, exp(f) m) (par = m, or expo =
 *                      n per-row exposures), lmax = max ll, w = exp(ll - lmax);
 *                      nlp = -(lmax + log mean(w)), mcsd = exp(lmax) sd(w) (R's n - 1 form: NaN
 *                      at S = 1; may underflow to 0), nlp_se = sd(w) / (mean(w) sqrt(S)).
 *                      The reference's poisson branch calls dpois(x, size = 1, prob = ...), an R
 *                      error; the evident intent dpois(y, exp(f) m) is built (quirk Q28). */
int sgp_joint_nlp(int device, int family, const double* y, const double* pred_mean,
                  const double* pred_cov, int64_t n, int64_t ldc, double par, const double* expo,
                  int64_t S, uint64_t seed, double* out /* 3 */);
/* my_kl(mv = TRUE) as written (l.155-163):
 *   kl = 1/2 (tr(sigma2^-1 sigma1) + (mean2 - mean1)^T sigma2^-1 (mean2 - mean1) - n
 *             + sum log diag chol2 - sum log diag chol1)
 * whose last two terms are half the log-determinant difference, so the value is not the KL
 * divergence (quirk Q29; parity is with the code). */
int sgp_joint_kl(int device, const double* mean1, const double* mean2, const double* sigma1,
                 int64_t ld1, const double* sigma2, int64_t ld2, int64_t n, double* kl);
/* my_nlp(family = "bernoulli", mc = TRUE) (l.53-65): row i draws S values
 * f = pred_mean_i + sqrt(pred_var_i) z from stream 1, ll = dbinom(y_i, 1, my_logistic(f));
 * nlp[i] = -log mean(ll), mcsd[i] = sd(ll) (n - 1 form), in linear space as the reference. */
int sgp_mc_nlp(int device, const double* y, const double* pred_mean, const double* pred_var,
               int64_t n, int64_t S, uint64_t seed, double* nlp, double* mcsd);

/* Knot gradients (xu_opt = "simultaneous"; the knot branches of delbo_dcov_par
 * R/vi_functions.R:425-593, dlogp_dcov_par R/laplace_approx_gradient.R:973-1126 and
 * dlogq_dcov_par 341-543, with dsqexp_dx2 / dsqexp_dx2_ard
 * R/covariance_function_derivatives.R:178-302 as dcov_fun_dknot).  When enabled,
 * every evaluation also contracts G against dK12/du in the same GEMM epilogue, and the
 * multi-GPU second reduction buffers grow by sgp_knot_red_extra(d, m) doubles (VI, FITC;
 * sgp_lap_red_count already has room).  sgp_knot_gradient then returns, row-major
 * (knot-major, quirk Q16), d obj / d u_kc times the reference's factor
 * (ub - lb) / ((u - lb)(ub - u) + 1e-4) (quirk Q8) with bounds = d x 2 column-major
 * [lower | upper], or NULL for the reference's knot_bounds from this context's rows
 * (vi_functions.R:175-178; multi-GPU callers pass the global bounds, see
 * sgp_ctx_row_bounds). */
int sgp_ctx_enable_knot_grad(sgp_ctx* ctx, int enable);
int64_t sgp_knot_red_extra(int d, int64_t m);
int sgp_knot_gradient(sgp_ctx* ctx, const double* bounds, double* grad_knot);
int sgp_ctx_row_bounds(sgp_ctx* ctx, double* col_min, double* col_max);

/* OAT knot proposal scoring (VI): the ELBO at knots [U; cand_t] for each of T candidate knots
 * (cand: T x d, column-major, ld ldc) at fixed theta -- the meta-model y values of
 * knot_prop_random_norm_vi / knot_prop_ego_norm_vi (R/vi_functions.R:2196-2300, 1584-) --
 * from bordered Schur complements instead of T rebuilds of K12.  NaN marks a candidate whose
 * bordered K22 or Bm is not positive definite (the reference's try-error).  m <= m_max is
 * enough on one device (nothing is built at m + 1; a row-sharded context rebuilds and needs
 * m + 1 <= m_max).  Afterwards the context holds the base system at (theta, U) without its
 * second phase, which is no completed evaluation: sgp_posterior_u and sgp_knot_gradient
 * refuse until the next evaluation, also when (theta, U) are those of the evaluation before. */
int sgp_vi_candidates(sgp_ctx* ctx, int kernel, const double* theta, const double* U, int64_t m,
                      int64_t ldu, double delta, unsigned flags, const double* cand, int64_t T,
                      int64_t ldc, double* obj_out);

/* OAT knot proposal scoring for FITC (knot_prop_random_norm / knot_prop_ego_norm,
 * R/knot_proposal_functions.R:1176-1363, 498-): obj_fun_norm at knots [U; cand_t] with
 * Sigma22 = Kuu + delta I, for each of T candidates (m + 1 <= m_max).  NaN = try-error; the
 * candidates after it are scored as usual.  Afterwards the context's state is the last
 * candidate's: sgp_posterior_u and sgp_knot_gradient refuse until the next evaluation. */
int sgp_fitc_candidates(sgp_ctx* ctx, int kernel, const double* theta, const double* U,
                        int64_t m, int64_t ldu, double delta, unsigned flags, const double* cand,
                        int64_t T, int64_t ldc, double* obj_out);

/* OAT knot proposal scoring for Poisson Laplace (knot_prop_random / knot_prop_ego,
 * R/knot_proposal_functions.R:1001-1173, 46-): for each candidate, newtrap_sparseGP at knots
 * [U; cand_t] warm-started from the resident f (the fit's fmax); obj_out[t] = its last
 * objective value.  The resident f is restored afterwards, also past a try-error (NaN).
 * sgp_posterior_u, sgp_knot_gradient and sgp_lap_get_grad_psi refuse until the next
 * evaluation. */
int sgp_lap_candidates(sgp_ctx* ctx, int kernel, const double* theta, const double* U, int64_t m,
                       int64_t ldu, double delta, double expo, double tol, int maxit,
                       const double* cand, int64_t T, int64_t ldc, double* obj_out);

/* The EGO knot proposal's scan (knot_prop_ego_norm_vi R/vi_functions.R:1927-1950, 2074-2097;
 * knot_prop_ego_norm / knot_prop_ego R/knot_proposal_functions.R:355-379, 457-478, 832-855,
 * 964-985): after every refit of the meta-model GP of the objective -- T points xm (T x d,
 * column-major, ld ldxm) with objective values vals -- the reference predicts the objective at
 * every data row outside the knots and takes the row of largest expected improvement:
 *   K12 = make_cov_matC(xy_setminus_xu, xm)  (cross mode: no nugget, even on a coincident pair)
 *   K22 = make_cov_matC(xm) = k(xm, xm) + (tau^2 + delta_meta) I   (the reference passes delta/1000)
 *   pred_i = vals[0] + K12[i,] K22^-1 (vals - vals[0])
 *   var_i  = sigma^2 + tau^2 - K12[i,] K22^-1 K12[i,]^T
 *   EI_i   = sqrt(var_i) (z pnorm(z) + dnorm(z)), z = (pred_i - max vals) / sqrt(var_i), when
 *            var_i > tau^2 (strictly; false for NaN), else 0;  pnorm(z) = erfc(-z / sqrt 2) / 2
 *   best_row = which.max(EI) over the rows not in excl: ties to the lowest row, a NaN never wins,
 *            all zero -> the first such row
 * as one pass over the context's resident rows (R: one dense solve per row in a loop over n).
 * kernel: SGP_KERNEL_EXP (the reference's default ego_cov_fun, L1 distance,
 * src/covariance_functionsC.cpp:45-52) or SGP_KERNEL_SQEXP; SGP_KERNEL_ARD is refused (the
 * reference's make_cov_matC returns a 0 x 0 matrix for it).  theta_meta = [sigma, l, tau] with
 * sigma > 0, l > 0, tau >= 0 (the reference's default ego_cov_par$tau is 0); delta_meta >= 0.
 * excl (E x d column-major, ld ldexcl, or NULL): a data row is excluded when all d of its
 * coordinates equal (==) those of some row of excl -- the reference's xy_setminus_xu
 * (vi_functions.R:1679-1687) with excl = the knots.  (The reference also drops data rows that
 * duplicate earlier data rows; that cannot change the winner's coordinates.)
 * best_row: 0-based row of the context's X; best_ei: its EI.  ei_out / mean_out / var_out: n host
 * values each or NULL -- pred and var for every row, EI with NaN on the excluded rows.
 * 1 <= T <= SGP_EGO_TMAX.  SGP_EINVAL before any device call for NULL arguments, T or a leading
 * dimension out of range, non-finite vals / theta_meta / xm, sigma <= 0, l <= 0, tau < 0 or
 * delta_meta < 0; SGP_EINVAL ("no data row outside the knots") when every row is excluded;
 * SGP_ENOTPD naming "meta-model K22" when K22 is not positive definite.  A completed evaluation
 * is left as it was (sgp_posterior_u still answers for it).  Multi-device contexts: rows and
 * vectors in the global row order. */
#define SGP_EGO_TMAX 128
int sgp_ego_scan(sgp_ctx* ctx, int kernel, const double* theta_meta, double delta_meta,
                 const double* xm, int64_t T, int64_t ldxm, const double* vals,
                 const double* excl, int64_t E, int64_t ldexcl, int64_t* best_row,
                 double* best_ei, double* ei_out, double* mean_out, double* var_out);

/* The cheap knot proposals' scan (knot_prop_var / knot_prop_error,
 * R/knot_proposal_functions.R:4-42): the reference predicts at every training row with
 * predict_laplace(full_cov = FALSE) (R/laplace_approx_prediction.R:3-123; x_pred = xy, mu = the
 * fit's mean) and takes which.max of the variance or of the error.  Here it is one pass over the
 * context's resident rows and mean, for a fit with knots U (m x d, column-major, ld ldu), knot
 * posterior u_mean / u_var (m x m, column-major, ld ldv) and knot prior mean muu:
 *   K22    = Kuu + delta I when gaussian, else Kuu + (tau^2 + delta) I   (l.25-62)
 *   w      = K22^-1 (u_mean - muu),   A = K22^-1 - K22^-1 u_var K22^-1
 *   mean_i = mu_i + k_i^T w           (the cross covariance k_i carries no nugget)
 *   var_i  = sigma^2 + tau^2 - k_i^T A k_i                                (l.114)
 *   key_i  = var_i                        (SGP_SCAN_VAR)
 *          = |exp(f_i) - exp(mean_i)|     (SGP_SCAN_ERROR; l.38, as written for every family)
 *   best_row = which.max(key) over the rows not in excl: ties to the lowest row, a NaN never wins
 * kernel: SGP_KERNEL_SQEXP or SGP_KERNEL_ARD (SGP_KERNEL_EXP is refused, as sgp_predict refuses
 * it); theta as the evaluations take it ([sigma, l.., tau]) with sigma > 0, l > 0, tau >= 0;
 * delta >= 0.  f: n host values, or NULL for the context's resident Laplace mode (what
 * sgp_lap_get_f returns; SGP_EINVAL when no Laplace evaluation has run); read in
 * SGP_SCAN_ERROR only.  excl (E x d column-major, ld ldexcl, or NULL): as sgp_ego_scan's -- a row
 * is excluded when all d of its coordinates equal (==) those of some row of excl.  The reference
 * excludes nothing: excl = NULL is the parity setting.  best_row: 0-based row of the context's X;
 * best_key: its key.  key_out / mean_out / var_out: n host values each or NULL -- key with NaN on
 * the excluded rows.
 * 1 <= m <= SGP_EGO_TMAX.  SGP_EINVAL before any device call for NULL arguments, m, a leading
 * dimension or mode out of range, non-finite theta / U / u_mean / muu / u_var, sigma <= 0,
 * l <= 0, tau < 0 or delta < 0; SGP_EINVAL for a multi-device context and when every row is
 * excluded; SGP_ENOTPD naming "scan K22" when K22 is not positive definite.  A completed
 * evaluation is left as it was (sgp_posterior_u still answers for it).  Bit-identical on repeat. */
enum { SGP_SCAN_VAR = 0, SGP_SCAN_ERROR = 1 };
int sgp_fit_scan(sgp_ctx* ctx, int kernel, const double* theta, double delta, int gaussian,
                 const double* U, int64_t m, int64_t ldu, const double* u_mean, const double* muu,
                 const double* u_var, int64_t ldv, int mode, const double* f,
                 const double* excl, int64_t E, int64_t ldexcl, int64_t* best_row, double* best_key,
                 double* key_out, double* mean_out, double* var_out);

/* Per-phase timing (HIP events on the launch stream).  Enabling clears the record; every
 * evaluation after it appends its phases, and sgp_ctx_timings returns the per-phase totals
 * over those sgp_ctx_timing_evals() evaluations (names: '\n'-separated phase names; ms: their
 * total durations, max n entries).  Nothing is read back while evaluations run. */
int sgp_ctx_enable_timing(sgp_ctx* ctx, int enable);
/* record only the phase called `name` (NULL: every phase) -- bench.py times its dominant
 * kernel inside the timed region this way, with no other event records in the stream */
int sgp_ctx_timing_filter(sgp_ctx* ctx, const char* name);
int64_t sgp_ctx_timing_evals(const sgp_ctx* ctx);
int sgp_ctx_timings(sgp_ctx* ctx, char* names, int64_t names_len, double* ms, int max_n, int* count);

#ifdef __cplusplus
}
#endif
#endif /* SGP_H */
