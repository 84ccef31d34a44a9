/*
 * sgp_diag.h -- diagnostic entry points of libsgp.so.
 *
 * Not part of the drop-in boundary (the reference has no counterpart): they let the GPU tests
 * and bench.py pin, on the hardware, claims the fused evaluations make internally.  Plain C,
 * host buffers, same status codes and sgp_last_error() as sgp.h.
 */
#ifndef SGP_DIAG_H
#define SGP_DIAG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The two m x m SPD inverses of a VI evaluation's phase 2 (the Gauss-Jordan chains that replace
 * R's chol / solve of Sigma22 and Sigma22 + t(Sigma12) %*% ZSig12, R/vi_functions.R:87-103,
 * 231-239), launched together as the evaluation launches them: inv(A) in place on a second
 * stream (K22's chain on `aux`) and inv(A + beta B) formed as the chain reads it on the first
 * (Bm's chain on the launch stream).  per_step = 0: the persistent one-launch chains (m <= 4096,
 * what the evaluations run); 1: one launch per 64-wide pivot step (the pre-round-5 chain, and
 * the product's chain above m = 4096).  The two must agree bit for bit (k_dense.hip).
 * A, B: m x m column-major, symmetric; invA, invS: m x m column-major; logdet[0] = log det A,
 * logdet[1] = log det(A + beta B).  SGP_ENOTPD as the evaluations (R's chol() message);
 * SGP_EHIP naming the watchdog when a chain's inter-workgroup wait expired. */
int sgp_diag_gj_pair(int device, int64_t m, const double* A, const double* B, double beta,
                     int per_step, double* invA, double* invS, double* logdet);

/* The HBM store ceiling of this device for the K12 builder's roofline: `reps` passes of plain
 * 16-byte non-temporal vector stores over `bytes` bytes, laid out as the builder stores (per
 * wave instruction 4 rows x 256 B of a row-major matrix with 1024-double rows; pattern 1) or as
 * one linear stream (pattern 0).  *gbs = the best pass in GB/s (1e9 B/s). */
int sgp_diag_store_bw(int device, int64_t bytes, int reps, int pattern, double* gbs);

/* Host only (no device is touched): the row-chunk plan a VI evaluation's S = K12^T K12 takes with
 * n rows and m knots.  *plan: 0 the packed plan (equal chunks, every diagonal 64-block in full),
 * 1 two chunk lengths (diagonal 128-tiles on longer chunks), 2 the work-balanced plan (every
 * workgroup the same modelled MFMA count), 3 the m <= 256 kernel; *workgroups: its grid;
 * *t_balanced, *t_packed: the modelled makespans of the work-balanced and the packed plan in
 * MFMA slots per wave (*t_balanced = 0 where the work-balanced plan does not apply). */
int sgp_diag_syrk_plan(int64_t n, int64_t m, int* plan, int* workgroups, double* t_balanced,
                       double* t_packed);

/* The device exp functions every covariance entry goes through, applied entry by entry by one tiny
 * kernel that calls the very inline functions of the builders: out[i] for x[0..n).  which = 0:
 * sgp_exp_nonpos(x), the direct-difference builder's, the batched kernels' and the scans' (x <= 0;
 * NaN in, NaN out).  which = 1: sgp_exp_tab(fmin(fmax(x, -746), hi)), the matrix-core builder's,
 * with the table staged in LDS and the argument clamped as that builder does; hi is the clamp's
 * upper end (the builder passes log sigma^2; at most log(DBL_MAX) = 709.78...; ignored with which
 * = 0).  SGP_EINVAL (before any device call) for a NULL pointer, n < 1, another `which`, or a hi
 * that is NaN or above log(DBL_MAX). */
int sgp_diag_exp(int device, int which, const double* x, int64_t n, double hi, double* out);

/* K12 = sigma^2 exp(-1/2 |x~ - u~|^2) as the fused evaluations build it, entry by entry: X (n x d,
 * column-major, ld ldx) and U (m x d, ld ldu) are uploaded zero-padded to n_pad = round_up(n, 128)
 * rows and m_p = round_up(m, 128) knots, the builder's centre and span guard are set from the
 * knots and the data's column ranges as a context sets them, and K receives the whole padded
 * n_pad x m_p row-major matrix (rows >= n and columns >= m are +0.0).  theta as sgp_eval_vi's
 * (sigma, the length scales, tau; tau is not used).  With r (n values; NULL: none) the builder's
 * fused t = K^T r rides along: t receives its m_p reduced values (summed as the VI evaluation sums
 * the builder's partial rows) and *t_rows the number of partial rows.
 * Three knobs, 0 = the product's behaviour:
 *   route     0: the span guard decides; 1: the matrix-core builder; 2: the direct-difference one.
 *             *route_taken = 1 or 2.
 *   max_rows  a cap on the workgroup rows of the builder's grid (1: one workgroup row walks every
 *             64-row block, i.e. the persistent loop at any n).
 *   shared_rb the leading row blocks built by the shared-occupancy launch (-1: as many as beside a
 *             K22 chain; 0: none).
 * K must not depend on max_rows or shared_rb; t may (its partial sums are per workgroup row) but is
 * the same bits on a repeat.  SGP_EINVAL, before any device call: a NULL X, U, K, theta or
 * route_taken; r without t and t_rows; n < 1, ldx < n, m < 1, ldu < m; d outside 1..32; route
 * outside 0..2, max_rows < 0, shared_rb < -1; SGP_KERNEL_EXP or an unknown kernel; sigma or a
 * length scale that is not positive. */
int sgp_diag_build_knm(int device, int kernel, int d, const double* theta, const double* X,
                       int64_t n, int64_t ldx, const double* U, int64_t m, int64_t ldu,
                       const double* r, int route, int64_t max_rows, int64_t shared_rb, double* K,
                       double* t, int* route_taken, int64_t* t_rows);

/* Host only (no device is touched): the argument checks sgp_ego_scan (sgp.h) runs before its
 * first device call, for rows of dimension d -- the very function it calls, so a machine without
 * a GPU can test every SGP_EINVAL case.  SGP_OK or SGP_EINVAL with sgp_last_error(). */
int sgp_diag_ego_args(int d, int kernel, const double* theta_meta, double delta_meta,
                      const double* xm, int64_t T, int64_t ldxm, const double* vals,
                      const double* excl, int64_t E, int64_t ldexcl);

/* Host only (no device is touched): the argument checks sgp_fit_scan (sgp.h) runs before its
 * first device call, for rows of dimension d -- the very function it calls.  SGP_OK or SGP_EINVAL
 * with sgp_last_error(). */
int sgp_diag_fit_scan_args(int d, int kernel, const double* theta, double delta, const double* U,
                           int64_t m, int64_t ldu, const double* u_mean, const double* muu,
                           const double* u_var, int64_t ldv, int mode, const double* excl,
                           int64_t E, int64_t ldexcl);

/* sgp_nlp (sgp.h) with its grid exposed: max_blocks = the cap on the scoring kernel's workgroups
 * (0 = the product's, eight per compute unit).  The result must not depend on it.  *kernel_ms
 * (or NULL): the scoring launches alone, by HIP events, without the copies. */
int sgp_diag_nlp(int device, int family, int max_blocks, const double* y,
                 const double* pred_mean, const double* pred_var, int64_t n, double par,
                 const double* expo, double* nlp, double* stats, double* kernel_ms);

/* The Cholesky factor the joint entries (sgp.h) use: A = L L^T for the n x n column-major A (ld
 * lda; its lower triangle is read), L column-major (ld ldl) with its strict upper triangle zero,
 * *logdet = 2 sum log L_ii.  SGP_ENOTPD with R's chol() message and order. */
int sgp_diag_chol(int device, const double* A, int64_t n, int64_t lda, double* L, int64_t ldl,
                  double* logdet);

/* The normal stream of sgp.h as the device generates it: out is S x n column-major (ld S),
 * out[s + S j] = the normal of draw s, row j of stream 0 or 1. */
int sgp_diag_normals(int device, uint64_t seed, int stream, int64_t S, int64_t n, double* out);

/* The yardstick of the draws' products: the generic f64 matrix-core GEMM they run on, timed on one
 * square n x n x n product (n a multiple of 64) by HIP events; *best_ms = the best of reps launches
 * after a warm-up. */
int sgp_diag_gemm64(int device, int64_t n, int reps, double* best_ms);

/* sgp_sample_mvn and sgp_joint_nlp (sgp.h) with their chunking and grid exposed: chunk_draws =
 * draws per chunk (0 = the product's: the two n_p x S_c work matrices under 512 MB), max_blocks =
 * the cap on the fill and scoring kernels' workgroups (0 = the product's).  The result must not
 * depend on either.  stage_ms (or NULL): 4 doubles, the time by HIP events of the factor, the Z
 * fills, the products and the scoring (with the final pass), each summed over the chunks. */
int sgp_diag_sample_mvn(int device, int chunk_draws, int max_blocks, const double* mean,
                        const double* cov, int64_t n, int64_t ldc, int64_t S, uint64_t seed,
                        double* out, int64_t ldo, double* stage_ms);
int sgp_diag_joint_nlp(int device, int family, int chunk_draws, int max_blocks, const double* y,
                       const double* pred_mean, const double* pred_cov, int64_t n, int64_t ldc,
                       double par, const double* expo, int64_t S, uint64_t seed, double* out,
                       double* stage_ms);

/* Host only (no device is touched): the argument checks sgp_predictor_create (sgp.h) runs before
 * its first device call -- the very function it calls.  SGP_OK or SGP_EINVAL with
 * sgp_last_error(). */
int sgp_diag_predictor_args(int d, int kernel, const double* theta, double delta, int method,
                            int gaussian, const double* U, int64_t m, int64_t ldu,
                            const double* u_mean, const double* muu, const double* u_var,
                            int64_t ldv);

/* Host only: the chunk plan of a predictor run over np rows with m knots.  budget_bytes = the K
 * work space's byte budget (0 = the product's).  *chunk_rows: the largest multiple of 128 rows
 * whose chunk_rows x round_up(m, 128) doubles stay within the budget (never below 128, never
 * more than round_up(np, 128)); *nchunks = ceil(np / chunk_rows); per 128-row tile with nb =
 * round_up(m, 128) / 128 column blocks, *block_products_sym = nb (nb + 1) / 2 128^3 block
 * products of the symmetric block form and *block_products_full = nb^2 of the full one. */
int sgp_diag_predictor_plan(int64_t m, int d, int64_t np, int64_t budget_bytes,
                            int64_t* chunk_rows, int64_t* nchunks, int64_t* block_products_sym,
                            int64_t* block_products_full);

/* sgp_predictor_run (sgp.h) with its chunking and route exposed.  chunk_rows: rows per chunk, a
 * multiple of 128 (0 = the product's; the work space grows to it).  route: 0 the product's; 1 the
 * tile route (K built into the work space, the symmetric block form: k_pred.hip); 2
 * sgp_predict's arithmetic on the chunk (the mean's row pass over K, then the full nb^2
 * quadratic form): the A/B yardstick and a second cross-check; 3 the register route (K formed in
 * registers, no K work space; SGP_EINVAL above 128 knots).  Routes agree to rounding, each is
 * bit-identical over chunk_rows and on repeat.  stage_ms (or NULL): 4 doubles, the time by HIP
 * events of the uploads, the K build, the mean / variance stage and the downloads, each summed
 * over the chunks (with stage_ms the call waits for every chunk). */
struct sgp_predictor;
int sgp_diag_predictor_run(struct sgp_predictor* p, int64_t chunk_rows, int route,
                           const double* x_pred, int64_t np, int64_t ldxp, const double* mu_pred,
                           double* pred_mean, double* pred_var, double* stage_ms);

/* Host only (no device is touched): the argument checks of the batched VI path (sgp.h) -- the very
 * functions sgp_batch_create (stage 0: the arguments up to B) and sgp_batch_eval_vi (stage 1:
 * create's, then the rest) run before their first device call.  SGP_OK or SGP_EINVAL with
 * sgp_last_error(). */
int sgp_diag_batch_args(int stage, const double* X, int64_t nrows, int64_t ldx, int d,
                        const double* y, const double* mu, const int64_t* row0,
                        const int64_t* nrow, int64_t B, int kernel, const double* theta,
                        int64_t ldt, const double* U, const int64_t* uoff, const int64_t* m,
                        double delta, unsigned flags, const unsigned char* active,
                        const double* obj, const double* grad, int64_t ldg, const int* status);

/* Host only: the segment plan of a batch.  A segment is a run of at most SGP_BATCH_SEG_ROWS rows
 * of one problem, counted from the problem's first row, so a problem's segments do not depend on
 * the rest of the batch; both row passes run one workgroup per segment and the per-problem stages
 * add the segments' records in this order.  *nseg = the number of segments; the first
 * min(cap, *nseg) of them are written to seg_prob / seg_row0 / seg_rows (may be NULL with cap =
 * 0); *seg_rows_max (or NULL) = SGP_BATCH_SEG_ROWS. */
#define SGP_BATCH_SEG_ROWS 512
int sgp_diag_batch_plan(const int64_t* row0, const int64_t* nrow, int64_t B, int64_t cap,
                        int64_t* nseg, int64_t* seg_prob, int64_t* seg_row0, int64_t* seg_rows,
                        int64_t* seg_rows_max);

/* stage_ms (4 doubles, or NULL): the times by HIP events of row pass 1, the m x m stage, row pass 2
 * and the finish of the batch's last evaluation (zeros when they were not recorded); enable != 0
 * records them from the next evaluation on. */
struct sgp_batch;
int sgp_diag_batch_timing(struct sgp_batch* b, int enable, double* stage_ms);

/* Host only: the checks sgp_batch_eval_vi_knots (sgp.h) makes beyond sgp_batch_eval_vi's, the very
 * function it runs first: grad_knot NULL, SGP_FLAG_OBJ_ONLY in flags, and a non-finite entry in an
 * active problem's block of bounds (NULL bounds are allowed).  SGP_OK or SGP_EINVAL with
 * sgp_last_error() naming the argument. */
int sgp_diag_batch_knot_args(int d, int64_t B, unsigned flags, const unsigned char* active,
                             const double* bounds, const double* grad_knot);

/* stage_ms (2 doubles, or NULL): the times by HIP events of the knot pass and the knot finish of
 * the batch's last sgp_batch_eval_vi_knots (zeros when they were not recorded); enable != 0 records
 * them from the next such call on.  sgp_diag_batch_timing covers that call's first four stages. */
int sgp_diag_batch_knot_timing(struct sgp_batch* b, int enable, double* stage_ms);

/* stage_ms (5 doubles, or NULL): the times by HIP events of K22's stage, the weighted first row
 * pass, Bm's stage, the gradient's row pass and the G22 stage of the batch's last
 * sgp_batch_eval_fitc (zeros when they were not recorded; the last two are zero under
 * SGP_FLAG_OBJ_ONLY); enable != 0 records them from the next such call on. */
int sgp_diag_batch_fitc_timing(struct sgp_batch* b, int enable, double* stage_ms);

/* Host only: the argument checks of the batched Laplace path (sgp.h), the very
 * functions sgp_batch_lap_init (on the batch's own y, rows and problems) and
 * sgp_batch_eval_laplace (after sgp_diag_batch_args' stage 1; family < 0: none set) run before
 * their first device call.  SGP_OK or SGP_EINVAL with sgp_last_error(). */
int sgp_diag_batch_lap_args(const double* y, int64_t nrows, const int64_t* row0,
                            const int64_t* nrow, int64_t B, int family, const double* expo);
int sgp_diag_batch_lap_eval_args(int family, double tol, int maxit, const int* nr_iters);

/* The Newton iteration's objective values of problem `prob` in the last sgp_batch_eval_laplace
 * that evaluated it (newtrap_sparseGP's objective_function_values, as sgp_lap_objective_values
 * gives them for a context): *count = nr_iters, of which the first
 * min(*count, max_n, SGP_BATCH_LAP_NOBJ) are written to out (a bounded per-problem record). */
#define SGP_BATCH_LAP_NOBJ 256
int sgp_diag_batch_lap_objective_values(struct sgp_batch* b, int64_t prob, double* out, int max_n,
                                        int* count);

/* stage_ms (11 doubles, or NULL): the times by HIP events of the batch's last
 * sgp_batch_eval_laplace (zeros when they were not recorded): K22's stage, the Z pass, the
 * K22 + S_Z stage | summed over the Newton iterations: the objective pass (the first one
 * included), the C stage, NR's part a, x2 | the gradient's part a, its vector stage, its part b
 * and the G22 stage (zero under SGP_FLAG_OBJ_ONLY); enable != 0 records them from the next such
 * call on. */
int sgp_diag_batch_laplace_timing(struct sgp_batch* b, int enable, double* stage_ms);

/* Host only: the argument checks of sgp_batch_set_test (stage 0: d, B and the arguments Xt ..
 * tnrow) and of sgp_batch_predict (stage 1: B and the arguments from have_test on) -- the very
 * function both run before their first device call.  have_test / have_yt: whether set_test was
 * called, and with a yt; has_state (B bytes): which problems have a posterior.  SGP_OK or
 * SGP_EINVAL with sgp_last_error(). */
int sgp_diag_batch_test_args(int stage, int d, int64_t B, const double* Xt, int64_t ntest,
                             int64_t ldxt, const double* yt, const double* mut,
                             const int64_t* trow0, const int64_t* tnrow, int have_test,
                             int have_yt, const unsigned char* has_state,
                             const unsigned char* active, const double* pred_mean,
                             const double* pred_var, const double* nlp, const double* stats);

/* Host only: the test-segment plan of sgp_batch_set_test: sgp_diag_batch_plan's rule applied to
 * (trow0, tnrow), where tnrow[b] = 0 is allowed and yields no segment; seg_row0 is a row of Xt.
 * toff (B + 1 values, or NULL): the problems' first rows in the packed outputs, toff[B] = sum
 * tnrow. */
int sgp_diag_batch_test_plan(const int64_t* trow0, const int64_t* tnrow, int64_t B, int64_t cap,
                             int64_t* nseg, int64_t* seg_prob, int64_t* seg_row0,
                             int64_t* seg_rows, int64_t* toff);

/* stage_ms (3 doubles, or NULL): the times by HIP events of the m x m stage, the row pass and the
 * finish of the batch's last sgp_batch_predict (zeros when they were not recorded); enable != 0
 * records them from the next call on. */
int sgp_diag_batch_predict_timing(struct sgp_batch* b, int enable, double* stage_ms);

#ifdef __cplusplus
}
#endif
#endif /* SGP_DIAG_H */
