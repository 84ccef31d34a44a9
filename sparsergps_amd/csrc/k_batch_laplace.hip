// Batched small-knot Laplace evaluation (sgp_batch_eval_laplace): B independent
// problems with a Poisson or Bernoulli likelihood, each with its own rows, theta, latent f and
// m <= 64 knots.  Per problem the semantics are sgp_eval_laplace's: newtrap_sparseGP
// (R/newtrap_sparseGP.R:6-186) warm-started from the resident f, then dlogq_dcov_par
// (R/laplace_approx_gradient.R:25-336), in adjoint form:
//   per theta
//     A = K22^-1, log|K22|, K22 = Kuu + (tau^2 + delta) I            k_bl_k22, per problem
//     q_i = k_i^T A k_i, Z_i = sigma^2 + tau^2 + delta - q_i (kept), S_Z = sum k_i k_i^T / Z_i
//                                                                    k_bl_passz, per segment
//     (K22 + S_Z)^-1                                                 k_bl_mmz, per problem
//   per Newton iteration, for the problems still running
//     y1 = K x1, psi' = d1 - (r - y1) / Z, v2 = K^T (psi' / (1 - Z W)), max |psi'|
//                                                                    k_bl_nra, per segment
//     x2 = C v2                                                      k_bl_x2, per problem
//     f += (Z d1 - r + y1 + K x2) / (1 - Z W); at the new f: B = 1 / (Z - 1 / W),
//     S_B = sum B_i k_i k_i^T, t_Z = K^T (r / Z), r^T r / Z, log p(y | f), sum log(1 - W Z)
//                                                                    k_bl_obj, per segment
//     C = (K22 + S_B)^-1, log|K22 + S_B|, x1 = (K22 + S_Z)^-1 t_Z, the objective, the stop rule
//     (and, on stopping, the knot posterior's state)                 k_bl_mm, per problem
//     the count of problems still running                            k_bl_count
//   the gradient at the mode
//     p_i = k_i^T C k_i, c2, sv, K^T c2, K^T d1, K^T (B sv)          k_bl_ga, per segment
//     s = A K^T c2, GG = A K^T d1, C w                               k_bl_gm, per problem
//     h, a, G = c2 s^T - h GG^T - B K C - 2 a K A, W = G o K and its per-parameter sums,
//     sum a, the coincident G_ij, S_a = sum a_i k_i k_i^T            k_bl_gb, per segment
//     G22 = (A - C) / 2 - s s^T / 2 + sym(C w GG^T) / 2 + A S_a A, the gradient
//                                                                    k_bl_gf, per problem
// The first objective (before any update) is k_bl_obj without the update.  The likelihood enters
// through LapLik<FAM>'s four row terms (sgp_lap_lik.h), as in the context route's kernels.
// The segments, the 64-row steps and the per-row bounds test are the VI batch's (k_batch.hip);
// k's operand layout (lane l on row l & 15 and knots 4 s + (l >> 4)), the rank updates through a
// wave-private transposition, the tails of the row passes and the pieces of the m x m stages
// are sgp_batch_dev.h's: S_Z and S_B have both operands scaled by the root of their positive
// weight (rank_update_root), S_a one operand scaled by a_i, which takes both signs
// (rank_update_signed).  This file keeps the row terms, G and the Newton iteration's vector
// stages; k_bl_obj's body, k_bl_mmz's and k_bl_mm's build loops and k_bl_mm's posterior store
// write a shared piece's text out where its function form cost time (each says so).  f and Z are indexed by (problem, local row), so aliased row ranges need nothing
// further.  A problem that stopped, failed or is inactive returns at once from every launch.
// Every sum and the maximum have a fixed order, no kernel uses atomics, and nothing a problem
// computes reads another problem's data.
#include <math.h>

#include "sgp_internal.h"
#include "sgp_batch_dev.h"
#include "sgp_lap_lik.h"

namespace {

// the step's X rows and its rows of f, y, mu, Z and the exposure (rv: 5 x 64)
__device__ __forceinline__ void stage_rows(const BatchArgs& a, const BatchLapArgs& l, int64_t row0,
                                           int64_t loc, int rows, int step, double* xs,
                                           double* rv) {
  const int tid = threadIdx.x;
  stage_x(a.X, a.ldx, row0, rows, step, a.d, xs);
  if (tid < 64) {
    const int row = step * 64 + tid;
    const bool ok = row < rows;
    rv[tid] = ok ? l.f[loc + row] : 0.0;
    rv[64 + tid] = ok ? a.y[row0 + row] : 0.0;
    rv[128 + tid] = ok ? a.mu[row0 + row] : 0.0;
    rv[192 + tid] = ok ? l.zv[loc + row] : 1.0;
    rv[256 + tid] = (ok && l.expo) ? l.expo[row0 + row] : 1.0;
  }
}

// x = Ainv b and, under the Bernoulli family, sec. 3.4's one refinement step
// x += Ainv (b - A x), as the context route's lap_refine_solve takes it.  b_s, x_s, r_s in LDS.
template <int FAM>
__device__ __forceinline__ void solve_refined(const double* __restrict__ A,
                                              const double* __restrict__ Ainv, const double* b_s,
                                              double* x_s, double* r_s, int m) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid < m) x_s[tid] = mat_vec_row(Ainv, b_s, tid, m);
  __syncthreads();
  if (FAM == SGP_FAM_BERNOULLI) {
    if (tid < m) r_s[tid] = b_s[tid] - mat_vec_row(A, x_s, tid, m);
    __syncthreads();
    double dx = 0.0;
    if (tid < m) dx = mat_vec_row(Ainv, r_s, tid, m);
    __syncthreads();
    if (tid < m) x_s[tid] = x_s[tid] + dx;
    __syncthreads();
  }
}

__device__ __forceinline__ bool bl_skip(const BatchArgs& a, const BatchLapArgs& l, int prob,
                                        bool running) {
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return true;
  if (a.out[(int64_t)prob * BATCH_OUT + 1] != 0.0) return true;   // not positive definite
  return running && l.lc[(int64_t)prob * BATCH_LC + LC_RUN] == 0.0;
}

// ------------------------------------------------------------------------------ K22's stage
__global__ void __launch_bounds__(256) k_bl_k22(BatchArgs a, BatchLapArgs l) {
  __shared__ __attribute__((aligned(16))) double A[MM * MM];
  __shared__ double ck[MM];
  const int prob = blockIdx.x, tid = threadIdx.x;
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  const int m = (int)P[BP_M];
  double* out = a.out + (int64_t)prob * BATCH_OUT;
  double* lw = l.lw + (int64_t)prob * BATCH_LW;
  double* lc = l.lc + (int64_t)prob * BATCH_LC;
  double ld22 = 0.0;
  const int st = k22_inverse(P, a.d, P[BP_TAU2] + P[BP_DELTA], A, ck, &ld22);   // quirk Q1
  if (tid == 0) {
    out[0] = st ? NAN : 0.0;
    out[1] = (double)st;
    lw[LW_LD] = ld22;
    lc[LC_RUN] = st ? 0.0 : 1.0;
    lc[LC_IT] = 0.0;
    lc[LC_OBJ] = 0.0;
  }
  if (st) return;
  for_mm(m, [&](int i, int j) { lw[LW_A + i * MM + j] = A[i * MM + j]; });
}

// ------------------------------------------------------------------------------ Z and S_Z
template <int NT>
__device__ __forceinline__ void bl_passz_body(const BatchArgs& a, const BatchLapArgs& l,
                                              const double* __restrict__ P,
                                              const double* __restrict__ lw, int64_t row0,
                                              int64_t loc, int rows, double* __restrict__ rec,
                                              double* xu_s, double* pa_s, double* vec_s,
                                              double* xs, double* wt_s) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2];
  const double c0 = (sig2 + P[BP_TAU2]) + P[BP_DELTA];
  double* sw_s = vec_s;        // 64: 1 / sqrt(Z)
  double* rl_s = vec_s + MM;   // d
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  double* wt = wt_s + wv * 16 * FXS;

  stage_knots(P, d, Mp, SN, xu_s, rl_s);
  stage_mat(lw + LW_A, m, Mp, pa_s);
  d4 acc[NT * (NT + 1) / 2];
#pragma unroll
  for (int p = 0; p < NT * (NT + 1) / 2; ++p) acc[p] = d4{0.0, 0.0, 0.0, 0.0};

  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();
    stage_x(a.X, a.ldx, row0, rows, step, d, xs);
    __syncthreads();

    double e2[SN], kf[SN];
    const bool iv = rows_k<SN>(xs, xu_s, rl_s, d, m, sig2, rows, step, e2, kf);
    d4 qa[NT];
    kmat<NT>(pa_s, kf, qa);
    const double z = c0 - row_dot<NT>(qa, kf);   // newtrap_sparseGP.R:63-66
    if (g == 0) {
      const int i = wv * 16 + r16;
      if (iv) l.zv[loc + step * 64 + i] = z;
      sw_s[i] = iv ? sqrt(1.0 / z) : 0.0;
    }
    put_ktile<SN>(wt, kf);
    __syncthreads();   // the k tile and the weights are read across the wave's lanes
    rank_update_root<NT, false>(wt, sw_s, nullptr, acc, nullptr);
  }
  store_pairs<NT>(acc, pa_s, rec);   // over A, which is dead
}

__global__ void __launch_bounds__(256) k_bl_passz(BatchArgs a, BatchLapArgs l) {
  __shared__ __attribute__((aligned(16))) double xu_s[SGP_MAXD * MM], pa_s[MM * MM];
  __shared__ double vec_s[MM + SGP_MAXD], xs[SGP_MAXD * 64], wt_s[4 * 16 * FXS];
  const int seg = blockIdx.x;
  const int prob = a.seg_prob[seg];
  if (bl_skip(a, l, prob, false)) return;
  const double* P = a.par + (int64_t)prob * a.pst;
  const double* lw = l.lw + (int64_t)prob * BATCH_LW;
  const int64_t row0 = a.seg_row0[seg], loc = l.seg_loc[seg];
  const int rows = a.seg_rows[seg];
  double* rec = a.rec1 + (int64_t)seg * BATCH_REC1;
  SGP_BATCH_NT(P[BP_M],
               bl_passz_body<NT>(a, l, P, lw, row0, loc, rows, rec, xu_s, pa_s, vec_s, xs, wt_s))
}

// ------------------------------------------------------------------------------ (K22 + S_Z)^-1
__global__ void __launch_bounds__(256) k_bl_mmz(BatchArgs a, BatchLapArgs l) {
  __shared__ __attribute__((aligned(16))) double Bm[MM * MM];
  __shared__ double ck[MM];
  const int prob = blockIdx.x, tid = threadIdx.x;
  if (bl_skip(a, l, prob, false)) return;
  const double* P = a.par + (int64_t)prob * a.pst;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2], dg = P[BP_TAU2] + P[BP_DELTA];
  const int seg0 = (int)P[BP_SEG0], nseg = (int)P[BP_NSEG];
  double* out = a.out + (int64_t)prob * BATCH_OUT;
  double* lw = l.lw + (int64_t)prob * BATCH_LW;
  const double* rec = a.rec1 + (int64_t)seg0 * BATCH_REC1;
  // for_mm's map written out: as a lambda this loop cost two VGPRs and 5 % of the stage
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    const double s = rec_sum(rec + i * MM + j, BATCH_REC1, nseg);
    const double v = k22(P, d, i, j, sig2, dg) + s;
    Bm[i * MM + j] = v;
    lw[LW_BZ + i * MM + j] = v;
  }
  double ldz = 0.0;
  const int st = sweep_spd(Bm, m, ck, &ldz);
  if (st) {
    if (tid == 0) {
      out[0] = NAN;
      out[1] = (double)-st;
      l.lc[(int64_t)prob * BATCH_LC + LC_RUN] = 0.0;
    }
    return;
  }
  for_mm(m, [&](int i, int j) { lw[LW_BZI + i * MM + j] = Bm[i * MM + j]; });
}

// ------------------------------------------------------------------------------ NR, part a
// grad_loglik_fn (derivative_functions_of_data_likelihoods.R:34-61, 188-235) and the first half
// of newtrap_sparseGP_update (newtrap_sparseGP.R:252-289) at the resident f
template <int NT, int FAM>
__device__ __forceinline__ void bl_nra_body(const BatchArgs& a, const BatchLapArgs& l,
                                            const double* __restrict__ P,
                                            const double* __restrict__ lw, int64_t row0,
                                            int64_t loc, int rows, double* __restrict__ rec,
                                            double* xu_s, double* vec_s, double* xs,
                                            double* wt_s, double* tw) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2];
  double* x1_s = vec_s;              // [g][s]
  double* rv = vec_s + MM;           // 5 x 64: f, y, mu, Z, the exposure
  double* wr_s = vec_s + 6 * MM;     // 64: psi' / (1 - Z W)
  double* red = vec_s + 7 * MM;      // 64
  double* rl_s = vec_s + 8 * MM;     // d
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  double* wt = wt_s + wv * 16 * FXS;

  stage_knots(P, d, Mp, SN, xu_s, rl_s);
  stage_vec(lw + LW_X1, m, Mp, SN, x1_s);
  double tacc[NT];
#pragma unroll
  for (int b = 0; b < NT; ++b) tacc[b] = 0.0;
  double gmax = 0.0;

  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();
    stage_rows(a, l, row0, loc, rows, step, xs, rv);
    __syncthreads();

    double e2[SN], kf[SN];
    const bool iv = rows_k<SN>(xs, xu_s, rl_s, d, m, sig2, rows, step, e2, kf);
    const double y1 = k_dot<SN>(kf, x1_s, g);
    if (g == 0) {
      const int i = wv * 16 + r16;
      const double fi = rv[i], yi = rv[64 + i], zi = rv[192 + i];
      const LapLik<FAM> lik(fi, yi, rv[256 + i]);
      const double W = lik.W();
      const double gi = lik.d1(yi);
      const double iz = 1.0 / zi;
      const double om = 1.0 - zi * W;
      const double gp = gi + (-iz * (fi - rv[128 + i]) + iz * y1);
      if (iv) gmax = fmax(gmax, fabs(gp));
      wr_s[i] = iv ? (1.0 / om) * gp : 0.0;
    }
    put_ktile<SN>(wt, kf);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * q + g;
      const double wr = wr_s[wv * 16 + i];
#pragma unroll
      for (int b = 0; b < NT; ++b) tacc[b] = fma(wt[i * FXS + 16 * b + r16], wr, tacc[b]);
    }
  }
  __syncthreads();
  fold_tacc<NT>(tacc, tw);
  if (g == 0) red[wv * 16 + r16] = gmax;
  __syncthreads();
  if (tid < Mp) rec[tid] = wave_sum4(tw, tid);
  if (tid == 0) {
    double v = 0.0;
    for (int q = 0; q < 64; ++q) v = fmax(v, red[q]);   // wave, then row lane
    rec[LR_GMAX] = v;
  }
}

template <int FAM>
__global__ void __launch_bounds__(256) k_bl_nra(BatchArgs a, BatchLapArgs l) {
  __shared__ __attribute__((aligned(16))) double xu_s[SGP_MAXD * MM];
  __shared__ double vec_s[8 * MM + SGP_MAXD], xs[SGP_MAXD * 64], wt_s[4 * 16 * FXS], tw[4 * MM];
  const int seg = blockIdx.x;
  const int prob = a.seg_prob[seg];
  if (bl_skip(a, l, prob, true)) return;
  const double* P = a.par + (int64_t)prob * a.pst;
  const double* lw = l.lw + (int64_t)prob * BATCH_LW;
  const int64_t row0 = a.seg_row0[seg], loc = l.seg_loc[seg];
  const int rows = a.seg_rows[seg];
  double* rec = l.lrec + (int64_t)seg * BATCH_LREC;
  SGP_BATCH_NT(P[BP_M], bl_nra_body<NT, FAM>(a, l, P, lw, row0, loc, rows, rec, xu_s, vec_s, xs,
                                             wt_s, tw))
}

// ------------------------------------------------------------------------------ x2 = C v2
template <int FAM>
__global__ void __launch_bounds__(256) k_bl_x2(BatchArgs a, BatchLapArgs l) {
  __shared__ double b_s[MM], x_s[MM], r_s[MM];
  const int prob = blockIdx.x, tid = threadIdx.x;
  if (bl_skip(a, l, prob, true)) return;
  const double* P = a.par + (int64_t)prob * a.pst;
  const int m = (int)P[BP_M];
  const int seg0 = (int)P[BP_SEG0], nseg = (int)P[BP_NSEG];
  double* lw = l.lw + (int64_t)prob * BATCH_LW;
  const int it = (int)l.lc[(int64_t)prob * BATCH_LC + LC_IT];
  const double* Cm = lw + LW_C + ((it - 1) & 1) * BR_T;   // the last objective's C
  const double* rec = l.lrec + (int64_t)seg0 * BATCH_LREC;
  if (tid < m) b_s[tid] = rec_sum(rec + tid, BATCH_LREC, nseg);
  solve_refined<FAM>(lw + LW_BB, Cm, b_s, x_s, r_s, m);
  if (tid < m) lw[LW_X2 + tid] = x_s[tid];
}

// ------------------------------------------------------------------------------ update, objective rows
// With upd the second half of newtrap_sparseGP_update (A11 - A12 + A13 + A2) on the resident f
// first; then obj_fun_pois / obj_fun_bern's rows (laplace_approx_obj_funs.R:108-174, 189-341) at
// the resident f and the weighted rank update S_B
template <int NT, int FAM>
__device__ __forceinline__ void bl_obj_body(const BatchArgs& a, const BatchLapArgs& l,
                                            const double* __restrict__ P,
                                            const double* __restrict__ lw, bool upd,
                                            int64_t row0, int64_t loc, int rows,
                                            double* __restrict__ rec, double* xu_s, double* S_s,
                                            double* vec_s, double* xs, double* wt_s, double* tw) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2];
  double* x1_s = vec_s;              // [g][s]
  double* x2_s = vec_s + MM;
  double* rv = vec_s + 2 * MM;       // 5 x 64: f, y, mu, Z, the exposure
  double* sw_s = vec_s + 7 * MM;     // 64: sqrt(B)
  double* wr_s = vec_s + 8 * MM;     // 64: r / Z
  double* red = vec_s + 9 * MM;      // 3 x 64
  double* rl_s = vec_s + 12 * MM;    // d
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  double* wt = wt_s + wv * 16 * FXS;

  stage_knots(P, d, Mp, SN, xu_s, rl_s);
  if (upd) {
    stage_vec(lw + LW_X1, m, Mp, SN, x1_s);
    stage_vec(lw + LW_X2, m, Mp, SN, x2_s);
  }
  d4 acc[NT * (NT + 1) / 2];
#pragma unroll
  for (int p = 0; p < NT * (NT + 1) / 2; ++p) acc[p] = d4{0.0, 0.0, 0.0, 0.0};
  double tacc[NT];
#pragma unroll
  for (int b = 0; b < NT; ++b) tacc[b] = 0.0;
  double srr = 0.0, slp = 0.0, slz = 0.0;

  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();
    stage_rows(a, l, row0, loc, rows, step, xs, rv);
    __syncthreads();

    // rows_k, rank_update_root<NT, true> and pass1_tail written out in this body: through the
    // header's functions this kernel, the largest of the file, came out 1 % slower; written out
    // it compiles to the registers and spills it had before they were shared.  The text is
    // theirs, operation for operation.
    const bool iv = step * 64 + wv * 16 + r16 < rows;
    const double* xr = xs + wv * 16 + r16;
    double e2[SN], kf[SN];
#pragma unroll
    for (int s = 0; s < SN; ++s) e2[s] = 0.0;
    for (int c = 0; c < d; ++c) {
      const double xc = xr[c * 64], rl = rl_s[c];
      const double* u = xu_s + (c * 4 + g) * SN;
#pragma unroll
      for (int s = 0; s < SN; ++s) {
        const double t = (xc - u[s]) * rl;
        e2[s] = fma(t, t, e2[s]);
      }
    }
#pragma unroll
    for (int s = 0; s < SN; ++s) {
      const double v = sig2 * sgp_exp_nonpos(-0.5 * e2[s]);
      kf[s] = (iv && 4 * s + g < m) ? v : 0.0;
    }
    double y1 = 0.0, y2 = 0.0;
    if (upd) {
      y1 = k_dot<SN>(kf, x1_s, g);
      y2 = k_dot<SN>(kf, x2_s, g);
    }
    if (g == 0) {
      const int i = wv * 16 + r16;
      double fi = rv[i];
      const double yi = rv[64 + i], mui = rv[128 + i], zi = rv[192 + i], ai = rv[256 + i];
      if (upd) {
        const LapLik<FAM> old(fi, yi, ai);
        const double om = 1.0 - zi * old.W();
        const double a11 = (zi / om) * old.d1(yi);
        const double a12 = (1.0 / om) * (fi - mui);
        const double a13 = y1 / om;
        const double a2 = y2 / om;
        fi = fi + (a11 - a12 + a13 + a2);
        if (iv) l.f[loc + step * 64 + i] = fi;
      }
      const LapLik<FAM> lik(fi, yi, ai);
      const double W = lik.W();
      const double bi = 1.0 / (zi - 1.0 / W);
      const double r = fi - mui;
      const double tv = (1.0 / zi) * r;
      if (iv) {
        srr = fma(tv, r, srr);
        slp += lik.logp(fi, yi, LapLik<FAM>::logexpo(l.expo, ai, 0.0));
        const double sw = sqrt(-W);
        slz += log(1.0 + sw * zi * sw);
      }
      sw_s[i] = iv ? sqrt(bi) : 0.0;
      wr_s[i] = iv ? tv : 0.0;
    }
    put_ktile<SN>(wt, kf);
    __syncthreads();   // the k tile and the weights are read across the wave's lanes
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * q + g;
      const double sq = sw_s[wv * 16 + i], wr = wr_s[wv * 16 + i];
      double kw[NT];
#pragma unroll
      for (int b = 0; b < NT; ++b) {
        const double k1 = wt[i * FXS + 16 * b + r16];
        tacc[b] = fma(k1, wr, tacc[b]);
        kw[b] = k1 * sq;
      }
      int p = 0;
#pragma unroll
      for (int bi = 0; bi < NT; ++bi)
#pragma unroll
        for (int bj = bi; bj < NT; ++bj, ++p)
          acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(kw[bi], kw[bj], acc[p], 0, 0, 0);
    }
  }

  store_pairs<NT>(acc, S_s, rec);
#pragma unroll
  for (int b = 0; b < NT; ++b) {
    double t = tacc[b];
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    if (g == 0) tw[wv * MM + 16 * b + r16] = t;
  }
  if (g == 0) {
    red[wv * 16 + r16] = srr;
    red[MM + wv * 16 + r16] = slp;
    red[2 * MM + wv * 16 + r16] = slz;
  }
  __syncthreads();
  if (tid < Mp) rec[BR_T + tid] = ((tw[tid] + tw[MM + tid]) + tw[2 * MM + tid]) + tw[3 * MM + tid];
  if (tid < 3) {
    double v = 0.0;
    for (int q = 0; q < 64; ++q) v += red[tid * MM + q];
    rec[BR_RR + tid] = v;
  }
}

template <int FAM>
__global__ void __launch_bounds__(256) k_bl_obj(BatchArgs a, BatchLapArgs l, int upd) {
  __shared__ __attribute__((aligned(16))) double xu_s[SGP_MAXD * MM], S_s[MM * MM];
  __shared__ double vec_s[12 * MM + SGP_MAXD], xs[SGP_MAXD * 64], wt_s[4 * 16 * FXS], tw[4 * MM];
  const int seg = blockIdx.x;
  const int prob = a.seg_prob[seg];
  if (bl_skip(a, l, prob, upd != 0)) return;
  const double* P = a.par + (int64_t)prob * a.pst;
  const double* lw = l.lw + (int64_t)prob * BATCH_LW;
  const int64_t row0 = a.seg_row0[seg], loc = l.seg_loc[seg];
  const int rows = a.seg_rows[seg];
  double* rec = a.rec1 + (int64_t)seg * BATCH_REC1;
  SGP_BATCH_NT(P[BP_M], bl_obj_body<NT, FAM>(a, l, P, lw, upd != 0, row0, loc, rows, rec, xu_s,
                                             S_s, vec_s, xs, wt_s, tw))
}

// ------------------------------------------------------------------------------ C, x1, the objective, the stop rule
template <int FAM>
__global__ void __launch_bounds__(256) k_bl_mm(BatchArgs a, BatchLapArgs l, int first) {
  __shared__ __attribute__((aligned(16))) double Bm[MM * MM];
  __shared__ double t_s[MM], x_s[MM], r_s[MM], ck[MM], red[256], gm_s[1];
  const int prob = blockIdx.x, tid = threadIdx.x;
  if (bl_skip(a, l, prob, first == 0)) return;
  const double* P = a.par + (int64_t)prob * a.pst;
  double* out = a.out + (int64_t)prob * BATCH_OUT;
  double* lw = l.lw + (int64_t)prob * BATCH_LW;
  double* lc = l.lc + (int64_t)prob * BATCH_LC;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2], dg = P[BP_TAU2] + P[BP_DELTA];
  const int seg0 = (int)P[BP_SEG0], nseg = (int)P[BP_NSEG];
  const int it = first ? 0 : (int)lc[LC_IT];   // the objective values before this one
  const double prev = lc[LC_OBJ];
  const double* rec = a.rec1 + (int64_t)seg0 * BATCH_REC1;

  const double rr = rec_sum(rec + BR_RR, BATCH_REC1, nseg);
  const double logpy = rec_sum(rec + BR_RR + 1, BATCH_REC1, nseg);
  const double logz2 = rec_sum(rec + BR_RR + 2, BATCH_REC1, nseg);
  // for_mm's map written out, as in k_bl_mmz: the stage runs once per Newton iteration
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    const double s = rec_sum(rec + i * MM + j, BATCH_REC1, nseg);
    const double v = k22(P, d, i, j, sig2, dg) + s;
    Bm[i * MM + j] = v;
    lw[LW_BB + i * MM + j] = v;
  }
  if (tid < m) t_s[tid] = rec_sum(rec + BR_T + tid, BATCH_REC1, nseg);
  if (tid == 0) {   // max |grad psi| of the update that led here, in segment order
    double v = 0.0;
    if (!first) {
      const double* lr = l.lrec + (int64_t)seg0 * BATCH_LREC + LR_GMAX;
      for (int q = 0; q < nseg; ++q) v = fmax(v, lr[(int64_t)q * BATCH_LREC]);
    }
    gm_s[0] = v;
  }

  double ldB = 0.0;
  const int st = sweep_spd(Bm, m, ck, &ldB);
  if (st) {
    if (tid == 0) {
      out[0] = NAN;
      out[1] = (double)-st;
      lc[LC_RUN] = 0.0;
    }
    return;
  }
  double* Cm = lw + LW_C + (it & 1) * BR_T;
  for_mm(m, [&](int i, int j) { Cm[i * MM + j] = Bm[i * MM + j]; });
  solve_refined<FAM>(lw + LW_BZ, lw + LW_BZI, t_s, x_s, r_s, m);
  const double tu = block_sum(tid < m ? t_s[tid] * x_s[tid] : 0.0, red);
  // laplace_approx_obj_funs.R:158-172: quad + log p(y|f) + det_part_1 + det_part_2
  const double ld22 = lw[LW_LD];
  const double obj = (-0.5 * rr + 0.5 * tu) + logpy + (-0.5 * (-ld22 + ldB)) + (-0.5 * logz2);
  // newtrap_sparseGP.R:79-100: one update whatever the first value is (maxit = 0: none), then
  // while (iter < maxit && (|obj step| > tol || any |grad psi| > tol))
  const int n_obj = it + 1;
  const bool run = first ? l.maxit > 0
                         : (n_obj < l.maxit && (fabs(obj - prev) > l.tol || gm_s[0] > l.tol));
  if (tid < m) lw[LW_X1 + tid] = x_s[tid];
  if (tid == 0) {
    out[0] = obj;
    lc[LC_OBJ] = obj;
    lc[LC_IT] = (double)n_obj;
    lc[LC_RUN] = run ? 1.0 : 0.0;
    if (it < BATCH_LAP_NOBJ) l.objs[(int64_t)prob * BATCH_LAP_NOBJ + it] = obj;
  }
  if (run) return;
  // the knot posterior's state (newtrap_sparseGP.R:137-176), where VI and FITC leave theirs:
  // (K22 + S_B(W_prev))^-1 with the loop's last, one-step-stale W, and x1 at the mode.  Not
  // store_post: the matrix comes from HBM or from LDS by entry, and two inlined copies of the
  // helper moved this kernel's schedule (the stage is the largest of a cold Bernoulli run)
  double* post = a.post + (int64_t)prob * a.post_stride;
  const double* Cp = lw + LW_C + ((it + 1) & 1) * BR_T;   // the previous objective's C
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    post[i * MM + j] = n_obj >= 2 ? Cp[i * MM + j] : Bm[i * MM + j];
  }
  if (tid < m) post[MM * MM + tid] = x_s[tid];
  for (int q = tid; q < a.pst; q += 256) post[MM * MM + MM + q] = P[q];
}

// the problems whose Newton iteration goes on
__global__ void __launch_bounds__(256) k_bl_count(BatchArgs a, BatchLapArgs l) {
  __shared__ double red[256];
  double v = 0.0;
  for (int p = threadIdx.x; p < a.B; p += 256)
    if (!bl_skip(a, l, p, true)) v += 1.0;
  const double s = block_sum(v, red);
  if (threadIdx.x == 0) *l.count = (int)s;
}

// ------------------------------------------------------------------------------ gradient, part a
// laplace_approx_gradient.R:133-178 at the mode: c2, d1, B sv and their K^T products
template <int NT, int FAM>
__device__ __forceinline__ void bl_ga_body(const BatchArgs& a, const BatchLapArgs& l,
                                           const double* __restrict__ P,
                                           const double* __restrict__ lw,
                                           const double* __restrict__ Cm, int64_t row0,
                                           int64_t loc, int rows, double* __restrict__ rec,
                                           double* xu_s, double* pb_s, double* vec_s, double* xs,
                                           double* wt_s, double* tw) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2];
  double* x1_s = vec_s;              // [g][s]
  double* rv = vec_s + MM;           // 5 x 64
  double* w3_s = vec_s + 6 * MM;     // 3 x 64: c2, d1, B sv
  double* rl_s = vec_s + 9 * MM;     // d
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  double* wt = wt_s + wv * 16 * FXS;

  stage_knots(P, d, Mp, SN, xu_s, rl_s);
  stage_vec(lw + LW_X1, m, Mp, SN, x1_s);
  stage_mat(Cm, m, Mp, pb_s);
  double tacc[3][NT];
#pragma unroll
  for (int v = 0; v < 3; ++v)
#pragma unroll
    for (int b = 0; b < NT; ++b) tacc[v][b] = 0.0;

  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();
    stage_rows(a, l, row0, loc, rows, step, xs, rv);
    __syncthreads();

    double e2[SN], kf[SN];
    const bool iv = rows_k<SN>(xs, xu_s, rl_s, d, m, sig2, rows, step, e2, kf);
    d4 qb[NT];
    kmat<NT>(pb_s, kf, qb);
    const double pi = row_dot<NT>(qb, kf);
    const double y1 = k_dot<SN>(kf, x1_s, g);
    if (g == 0) {
      const int i = wv * 16 + r16;
      const double fi = rv[i], yi = rv[64 + i], zi = rv[192 + i];
      const LapLik<FAM> lik(fi, yi, rv[256 + i]);
      const double W = lik.W(), W3 = lik.W3();
      const double iz = 1.0 / zi;
      const double bi = 1.0 / (zi - 1.0 / W);
      const double D = W - 1.0 / zi;
      const double coef = iz * (1.0 / D);
      const double comp4 = -(1.0 / D) + coef * coef * pi;
      const double sv = comp4 * (-W3) * (-1.0 / W);
      w3_s[i] = iv ? iz * (fi - rv[128 + i]) - iz * y1 : 0.0;
      w3_s[MM + i] = iv ? lik.d1(yi) : 0.0;
      w3_s[2 * MM + i] = iv ? bi * sv : 0.0;
    }
    put_ktile<SN>(wt, kf);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * q + g;
      const double w0 = w3_s[wv * 16 + i], w1 = w3_s[MM + wv * 16 + i],
                   w2 = w3_s[2 * MM + wv * 16 + i];
#pragma unroll
      for (int b = 0; b < NT; ++b) {
        const double k1 = wt[i * FXS + 16 * b + r16];
        tacc[0][b] = fma(k1, w0, tacc[0][b]);
        tacc[1][b] = fma(k1, w1, tacc[1][b]);
        tacc[2][b] = fma(k1, w2, tacc[2][b]);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < 3; ++v) fold_tacc<NT>(tacc[v], tw + v * 4 * MM);
  __syncthreads();
  for (int q = tid; q < 3 * MM; q += 256) {
    const int v = q >> 6, j = q & 63;
    if (j < Mp) rec[v * MM + j] = wave_sum4(tw + v * 4 * MM, j);
  }
}

template <int FAM>
__global__ void __launch_bounds__(256) k_bl_ga(BatchArgs a, BatchLapArgs l) {
  __shared__ __attribute__((aligned(16))) double xu_s[SGP_MAXD * MM], pb_s[MM * MM];
  __shared__ double vec_s[9 * MM + SGP_MAXD], xs[SGP_MAXD * 64], wt_s[4 * 16 * FXS],
      tw[12 * MM];
  const int seg = blockIdx.x;
  const int prob = a.seg_prob[seg];
  if (bl_skip(a, l, prob, false)) return;
  const double* P = a.par + (int64_t)prob * a.pst;
  const double* lw = l.lw + (int64_t)prob * BATCH_LW;
  const int it = (int)l.lc[(int64_t)prob * BATCH_LC + LC_IT];
  const double* Cm = lw + LW_C + ((it - 1) & 1) * BR_T;   // C at the mode
  const int64_t row0 = a.seg_row0[seg], loc = l.seg_loc[seg];
  const int rows = a.seg_rows[seg];
  double* rec = l.lrec + (int64_t)seg * BATCH_LREC;
  SGP_BATCH_NT(P[BP_M], bl_ga_body<NT, FAM>(a, l, P, lw, Cm, row0, loc, rows, rec, xu_s, pb_s,
                                            vec_s, xs, wt_s, tw))
}

// ------------------------------------------------------------------------------ s, GG, C w
template <int FAM>
__global__ void __launch_bounds__(256) k_bl_gm(BatchArgs a, BatchLapArgs l) {
  __shared__ double b_s[3 * MM], x_s[MM], r_s[MM];
  const int prob = blockIdx.x, tid = threadIdx.x;
  if (bl_skip(a, l, prob, false)) return;
  const double* P = a.par + (int64_t)prob * a.pst;
  const int m = (int)P[BP_M];
  const int seg0 = (int)P[BP_SEG0], nseg = (int)P[BP_NSEG];
  double* lw = l.lw + (int64_t)prob * BATCH_LW;
  const int it = (int)l.lc[(int64_t)prob * BATCH_LC + LC_IT];
  const double* Cm = lw + LW_C + ((it - 1) & 1) * BR_T;
  const double* rec = l.lrec + (int64_t)seg0 * BATCH_LREC;
  for (int q = tid; q < 3 * MM; q += 256)
    if ((q & 63) < m) b_s[q] = rec_sum(rec + q, BATCH_LREC, nseg);
  __syncthreads();
  if (tid < m) {
    lw[LW_S + tid] = mat_vec_row(lw + LW_A, b_s, tid, m);
    lw[LW_GG + tid] = mat_vec_row(lw + LW_A, b_s + MM, tid, m);
  }
  solve_refined<FAM>(lw + LW_BB, Cm, b_s + 2 * MM, x_s, r_s, m);
  if (tid < m) lw[LW_CW + tid] = x_s[tid];
}

// ------------------------------------------------------------------------------ gradient, part b
template <int NT, bool ARD, int FAM>
__device__ __forceinline__ void bl_gb_body(const BatchArgs& a, const BatchLapArgs& l,
                                           const double* __restrict__ P,
                                           const double* __restrict__ lw,
                                           const double* __restrict__ Cm, int64_t row0,
                                           int64_t loc, int rows, double* __restrict__ rec,
                                           double* xu_s, double* pa_s, double* pb_s,
                                           double* vec_s, double* xs, double* wt_s, double* red,
                                           double* el_s) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2];
  double* x1_s = vec_s;              // [g][s] each
  double* cw_s = vec_s + MM;
  double* s_s = vec_s + 2 * MM;
  double* gg_s = vec_s + 3 * MM;
  double* rv = vec_s + 4 * MM;       // 5 x 64
  double* om_s = vec_s + 9 * MM;     // 64: a
  double* rl_s = vec_s + 10 * MM;    // d
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  double* wt = wt_s + wv * 16 * FXS;

  stage_knots(P, d, Mp, SN, xu_s, rl_s);
  stage_vec(lw + LW_X1, m, Mp, SN, x1_s);
  stage_vec(lw + LW_CW, m, Mp, SN, cw_s);
  stage_vec(lw + LW_S, m, Mp, SN, s_s);
  stage_vec(lw + LW_GG, m, Mp, SN, gg_s);
  stage_mat(lw + LW_A, m, Mp, pa_s);
  stage_mat(Cm, m, Mp, pb_s);
  if (ARD)
    for (int q = tid; q < d * 64; q += 256) el_s[q] = 0.0;

  d4 acc[NT * (NT + 1) / 2];
#pragma unroll
  for (int p = 0; p < NT * (NT + 1) / 2; ++p) acc[p] = d4{0.0, 0.0, 0.0, 0.0};
  double esig = 0.0, el = 0.0, csum = 0.0, som = 0.0;

  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();
    stage_rows(a, l, row0, loc, rows, step, xs, rv);
    __syncthreads();

    double e2[SN], kf[SN];
    const bool iv = rows_k<SN>(xs, xu_s, rl_s, d, m, sig2, rows, step, e2, kf);
    d4 qa[NT], qb[NT];
    kmat2<NT>(pa_s, pb_s, kf, qa, qb);
    const double pi = row_dot<NT>(qb, kf);
    const double y1 = k_dot<SN>(kf, x1_s, g);
    const double y3 = k_dot<SN>(kf, cw_s, g);
    // the row's terms, in every lane of the row (k_lap_grad_a / k_lap_grad_b's expressions)
    double c2, hi, bi, ai;
    {
      const int i = wv * 16 + r16;
      const double fi = rv[i], yi = rv[64 + i], zi = rv[192 + i];
      const LapLik<FAM> lik(fi, yi, rv[256 + i]);
      const double W = lik.W(), W3 = lik.W3();
      const double iz = 1.0 / zi;
      bi = 1.0 / (zi - 1.0 / W);
      c2 = iz * (fi - rv[128 + i]) - iz * y1;
      const double gi = lik.d1(yi);
      const double dMt = bi - bi * bi * pi;
      const double D = W - 1.0 / zi;
      const double coef = iz * (1.0 / D);
      const double comp4 = -(1.0 / D) + coef * coef * pi;
      const double sv = comp4 * (-W3) * (-1.0 / W);
      hi = bi * sv - bi * y3;
      ai = -0.5 * dMt + 0.5 * c2 * c2 - 0.5 * hi * gi;
      if (!iv) c2 = hi = bi = ai = 0.0;
      if (g == 0) {
        som += ai;
        om_s[i] = ai;
      }
    }
    // G = c2 s^T - h GG^T - B K C - 2 a K A
    grad_terms<NT, ARD>(
        [&](int cb, int r, int s) {
          return fma(c2, s_s[g * SN + s],
                     -fma(hi, gg_s[g * SN + s], fma(bi, qb[cb][r], 2.0 * ai * qa[cb][r])));
        },
        kf, e2, iv, m, d, xs, xu_s, rl_s, el_s, esig, el, csum);
    put_ktile<SN>(wt, kf);
    __syncthreads();   // the k tile and a are read across the wave's lanes
    rank_update_signed<NT>(wt, om_s, acc);   // S_a
  }

  store_pairs<NT>(acc, pa_s, rec);   // over A, which is dead
  grad_tail<ARD>(esig, el, csum, som, d, red, el_s, rec);
}

template <bool ARD, int FAM>
__global__ void __launch_bounds__(256) k_bl_gb(BatchArgs a, BatchLapArgs l) {
  __shared__ __attribute__((aligned(16))) double xu_s[SGP_MAXD * MM], pa_s[MM * MM], pb_s[MM * MM];
  __shared__ double vec_s[10 * MM + SGP_MAXD], xs[SGP_MAXD * 64], wt_s[4 * 16 * FXS], red[256];
  __shared__ double el_s[ARD ? SGP_MAXD * 64 : 1];
  const int seg = blockIdx.x;
  const int prob = a.seg_prob[seg];
  if (bl_skip(a, l, prob, false)) return;
  const double* P = a.par + (int64_t)prob * a.pst;
  const double* lw = l.lw + (int64_t)prob * BATCH_LW;
  const int it = (int)l.lc[(int64_t)prob * BATCH_LC + LC_IT];
  const double* Cm = lw + LW_C + ((it - 1) & 1) * BR_T;
  const int64_t row0 = a.seg_row0[seg], loc = l.seg_loc[seg];
  const int rows = a.seg_rows[seg];
  double* rec = a.rec4 + (int64_t)seg * BATCH_REC4;
  SGP_BATCH_NT(P[BP_M], bl_gb_body<NT, ARD, FAM>(a, l, P, lw, Cm, row0, loc, rows, rec, xu_s, pa_s,
                                                 pb_s, vec_s, xs, wt_s, red, el_s))
}

// ------------------------------------------------------------------------------ G22 and finish
// G22 = (K22^-1 - C) / 2 - s s^T / 2 + (C w GG^T + GG (C w)^T) / 4 + K22^-1 S_a K22^-1, contracted
// with dK22 / dlog theta (contract_h; tau: 2 tau^2 where two knots coincide, the diagonal
// included: quirk Q5), then dlogq_dcov_par's gradient from the segments' sums (A1 = 2 sigma^2
// for sigma, 2 tau^2 for tau)
__global__ void __launch_bounds__(256) k_bl_gf(BatchArgs a, BatchLapArgs l) {
  __shared__ __attribute__((aligned(16))) double A[MM * MM], Ci[MM * MM], S[MM * MM], T[MM * MM];
  __shared__ double s_s[MM], gg_s[MM], cw_s[MM], red[256], r2[SGP_MAXD + 4], g22[SGP_MAXD + 2];
  const int prob = blockIdx.x, tid = threadIdx.x;
  if (bl_skip(a, l, prob, false)) return;
  const double* P = a.par + (int64_t)prob * a.pst;
  double* out = a.out + (int64_t)prob * BATCH_OUT;
  const int d = a.d, m = (int)P[BP_M];
  const int L = a.ard ? d : 1;
  const double* lw = l.lw + (int64_t)prob * BATCH_LW;
  const int it = (int)l.lc[(int64_t)prob * BATCH_LC + LC_IT];
  const double* Cm = lw + LW_C + ((it - 1) & 1) * BR_T;
  const double sig2 = P[BP_SIG2], tau2 = P[BP_TAU2];
  const int seg0 = (int)P[BP_SEG0], nseg = (int)P[BP_NSEG];
  const double* rec = a.rec4 + (int64_t)seg0 * BATCH_REC4;
  for_mm(m, [&](int i, int j) {
    A[i * MM + j] = lw[LW_A + i * MM + j];
    Ci[i * MM + j] = Cm[i * MM + j];
    S[i * MM + j] = rec_sum(rec + i * MM + j, BATCH_REC4, nseg);
  });
  if (tid < m) {
    s_s[tid] = lw[LW_S + tid];
    gg_s[tid] = lw[LW_GG + tid];
    cw_s[tid] = lw[LW_CW + tid];
  }
  if (tid < L + 3) r2[tid] = rec_sum(rec + BQ_W + tid, BATCH_REC4, nseg);
  __syncthreads();
  sandwich(A, S, T, m);
  double cg = 0.0;   // G22 over the coincident knot pairs
  for_mm(m, [&](int i, int j) {
    const double s = dot_mm(T, A, i, j, m);
    const double gv = 0.5 * (A[i * MM + j] - Ci[i * MM + j]) - 0.5 * s_s[i] * s_s[j] +
                      0.25 * (cw_s[i] * gg_s[j] + gg_s[i] * cw_s[j]) + s;
    bool same = true;
    for (int c = 0; c < d; ++c) same = same && P[BP_U + c * MM + i] == P[BP_U + c * MM + j];
    if (same) cg += gv;
    S[i * MM + j] = gv * kuu(P, d, i, j, sig2);   // H: S is dead once T stands
  });
  __syncthreads();
  const double cgs = block_sum(cg, red);
  if (tid == 0) g22[SGP_MAXD + 1] = cgs;
  contract_h(P, d, m, a.ard, S, red, g22);
  __syncthreads();
  const double suma = r2[2 + L];
  if (tid == 0) out[2] = 2.0 * r2[0] + g22[0] + 2.0 * sig2 * suma;
  if (tid >= 1 && tid <= L) out[2 + tid] = r2[tid] + g22[tid];
  if (tid == L + 1)
    out[2 + tid] = 2.0 * tau2 * r2[1 + L] + 2.0 * tau2 * g22[SGP_MAXD + 1] + 2.0 * tau2 * suma;
}

}  // namespace

hipError_t launch_batch_laplace(int stage, const BatchArgs& a, const BatchLapArgs& l,
                                hipStream_t s) {
  if (a.B < 1 || a.nseg < 1 || a.d < 1 || a.d > SGP_MAXD || !l.f || !l.zv || !l.lw || !l.lc ||
      !l.lrec || !l.objs || !l.count || !l.seg_loc || !a.rec1 || !a.rec4 ||
      (l.family != SGP_FAM_POISSON && l.family != SGP_FAM_BERNOULLI))
    return hipErrorInvalidValue;
  const dim3 pb((unsigned)a.B), sg((unsigned)a.nseg), th(256);
  const bool bern = l.family == SGP_FAM_BERNOULLI;
#define SGP_BL_FAM(K, GRID, ...)                                                              \
  do {                                                                                        \
    if (bern) hipLaunchKernelGGL(K<SGP_FAM_BERNOULLI>, GRID, th, 0, s, a, l, ##__VA_ARGS__);  \
    else hipLaunchKernelGGL(K<SGP_FAM_POISSON>, GRID, th, 0, s, a, l, ##__VA_ARGS__);         \
  } while (0)
  switch (stage) {
    case BL_K22: hipLaunchKernelGGL(k_bl_k22, pb, th, 0, s, a, l); break;
    case BL_PASSZ: hipLaunchKernelGGL(k_bl_passz, sg, th, 0, s, a, l); break;
    case BL_MMZ: hipLaunchKernelGGL(k_bl_mmz, pb, th, 0, s, a, l); break;
    case BL_OBJ0: SGP_BL_FAM(k_bl_obj, sg, 0); break;
    case BL_MM0: SGP_BL_FAM(k_bl_mm, pb, 1); break;
    case BL_NRA: SGP_BL_FAM(k_bl_nra, sg); break;
    case BL_X2: SGP_BL_FAM(k_bl_x2, pb); break;
    case BL_UPD: SGP_BL_FAM(k_bl_obj, sg, 1); break;
    case BL_MM: SGP_BL_FAM(k_bl_mm, pb, 0); break;
    case BL_COUNT: hipLaunchKernelGGL(k_bl_count, dim3(1), th, 0, s, a, l); break;
    case BL_GA: SGP_BL_FAM(k_bl_ga, sg); break;
    case BL_GM: SGP_BL_FAM(k_bl_gm, pb); break;
    case BL_GB:
      if (a.ard) {
        if (bern) hipLaunchKernelGGL((k_bl_gb<true, SGP_FAM_BERNOULLI>), sg, th, 0, s, a, l);
        else hipLaunchKernelGGL((k_bl_gb<true, SGP_FAM_POISSON>), sg, th, 0, s, a, l);
      } else {
        if (bern) hipLaunchKernelGGL((k_bl_gb<false, SGP_FAM_BERNOULLI>), sg, th, 0, s, a, l);
        else hipLaunchKernelGGL((k_bl_gb<false, SGP_FAM_POISSON>), sg, th, 0, s, a, l);
      }
      break;
    case BL_GF: hipLaunchKernelGGL(k_bl_gf, pb, th, 0, s, a, l); break;
    default: return hipErrorInvalidValue;
  }
#undef SGP_BL_FAM
  return hipGetLastError();
}
