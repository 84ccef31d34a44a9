// Batched small-knot FITC evaluation (sgp_batch_eval_fitc): B independent
// problems, each with its own rows, theta and m <= 64 knots, in five launches for the whole batch
// (three with SGP_FLAG_OBJ_ONLY).  Per problem the semantics are sgp_eval_fitc's: obj_fun_norm
// (R/laplace_approx_obj_funs.R:6-52) on the driver's Z (R/laplace_gradient_ascent.R:1238-1263) and
// dlogp_dcov_par (R/laplace_approx_gradient.R:720-971) in adjoint form:
//   A = K22^-1, log|K22|, K22 = Kuu + delta I                    k_bf_k22, per problem, in LDS
//   q_i = k_i^T A k_i, Z_i = sigma^2 + tau^2 + delta - q_i, w_i = 1 / Z_i,
//   S = sum w_i k_i k_i^T, t = sum w_i r_i k_i, sum log Z_i, sum w_i r_i^2
//                                                                k_bf_pass1, per segment
//   Bm = K22 + S, Bm^-1, log|Bm|, u = Bm^-1 t, the objective     k_bf_mm, per problem, in LDS
//   alpha_i = w_i (r_i - k_i^T u), p_i = k_i^T Bm^-1 k_i, omega_i = alpha_i^2 - (w_i - w_i^2 p_i),
//   G_i. = alpha_i u^T - w_i k_i^T Bm^-1 - omega_i k_i^T A, W = G o K and its per-parameter sums,
//   sum omega_i, the coincident G_ij, S_omega = sum omega_i k_i k_i^T
//                                                                k_bf_pass2, per segment
//   G22 = -1/2 u u^T + 1/2 (A - Bm^-1) + 1/2 A S_omega A, H = G22 o Kuu, the gradient
//                                                                k_bf_g22, per problem, in LDS
// The segments, the 64-row steps and the per-row bounds test are the VI batch's (k_batch.hip).
// Both row passes are built from sgp_batch_dev.h's pieces: k in k_fit_scan's operand layout of
// v_mfma_f64_16x16x4_f64 (rows_k), in which K A and K Bm^-1 are MFMAs against an operand in LDS
// (kmat) and q, p and k^T u are fma chains in the lane and one xor-shuffle over the four lane
// groups (row_dot, k_dot); the wave's 16 x Mp tile of k turned through wave-private LDS for the
// nb (nb + 1) / 2 block pairs of the rank update: both operands scaled by sqrt(w_i) for S
// (rank_update_root), one operand scaled by omega_i for S_omega, whose weights take both signs
// (rank_update_signed); the tails (pass1_tail, grad_terms, grad_tail).  This file keeps the row
// terms and G.  The row weights are recomputed from k in each pass, so nothing is indexed by the
// resident row and aliased row ranges need no work vector.  Every sum has a fixed order, no
// kernel uses atomics, and nothing a problem computes reads another problem's data.
#include <math.h>

#include "sgp_internal.h"
#include "sgp_batch_dev.h"

namespace {

// ------------------------------------------------------------------------------ K22's stage
__global__ void __launch_bounds__(256) k_bf_k22(BatchArgs a) {
  __shared__ __attribute__((aligned(16))) double A[MM * MM];
  __shared__ double ck[MM];
  const int prob = blockIdx.x, tid = threadIdx.x;
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  const int m = (int)P[BP_M];
  double* out = a.out + (int64_t)prob * BATCH_OUT;
  double* fw = a.fw + (int64_t)prob * BATCH_FW;
  double ld22 = 0.0;
  const int st = k22_inverse(P, a.d, P[BP_DELTA], A, ck, &ld22);
  if (tid == 0) {
    out[0] = st ? NAN : 0.0;
    out[1] = (double)st;
    fw[BF_LD] = ld22;
    fw[BF_BAD] = 0.0;
  }
  if (st) return;
  for_mm(m, [&](int i, int j) { fw[BF_A + i * MM + j] = A[i * MM + j]; });
}

// the step's r = y - mu, zero beyond the segment
__device__ __forceinline__ void stage_r(const BatchArgs& a, int64_t row0, int rows, int step,
                                        double* rs) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const int row = step * 64 + tid;
    rs[tid] = row < rows ? a.y[row0 + row] - a.mu[row0 + row] : 0.0;
  }
}

// ------------------------------------------------------------------------------ row pass 1
template <int NT>
__device__ __forceinline__ void bf_pass1_body(const BatchArgs& a, const double* __restrict__ P,
                                              const double* __restrict__ fw, int64_t row0, int rows,
                                              double* __restrict__ rec, double* xu_s, double* pa_s,
                                              double* vec_s, double* xs, double* wt_s, double* tw) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2];
  const double c0 = (sig2 + P[BP_TAU2]) + P[BP_DELTA];
  double* rs = vec_s;              // 64: r of this step's rows
  double* sw_s = vec_s + MM;       // 64: sqrt(w)
  double* wr_s = vec_s + 2 * MM;   // 64: w r
  double* red = vec_s + 3 * MM;    // 3 x 64
  double* rl_s = vec_s + 6 * MM;   // d
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  double* wt = wt_s + wv * 16 * FXS;   // the wave's own k tile [row][knot]

  stage_knots(P, d, Mp, SN, xu_s, rl_s);
  stage_mat(fw + BF_A, m, Mp, pa_s);

  d4 acc[NT * (NT + 1) / 2];
#pragma unroll
  for (int p = 0; p < NT * (NT + 1) / 2; ++p) acc[p] = d4{0.0, 0.0, 0.0, 0.0};
  double tacc[NT];
#pragma unroll
  for (int b = 0; b < NT; ++b) tacc[b] = 0.0;
  double swrr = 0.0, slz = 0.0, bad = 0.0;

  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();   // the staging above / the previous step's reads of xs, the vectors and wt
    stage_x(a.X, a.ldx, row0, rows, step, d, xs);
    stage_r(a, row0, rows, step, rs);
    __syncthreads();

    double e2[SN], kf[SN];
    const bool iv = rows_k<SN>(xs, xu_s, rl_s, d, m, sig2, rows, step, e2, kf);
    d4 qa[NT];
    kmat<NT>(pa_s, kf, qa);
    const double z = c0 - row_dot<NT>(qa, kf);
    const double w = 1.0 / z;
    if (g == 0) {
      const int i = wv * 16 + r16;
      const double ri = rs[i];
      if (iv) {
        if (!(z > 0.0 && z <= 1.79769313486231570815e308)) bad += 1.0;
        slz += log(z);
        swrr = fma(w * ri, ri, swrr);
      }
      sw_s[i] = iv ? sqrt(w) : 0.0;
      wr_s[i] = iv ? w * ri : 0.0;
    }
    put_ktile<SN>(wt, kf);
    __syncthreads();   // the k tile and the weights are read across the wave's lanes
    rank_update_root<NT, true>(wt, sw_s, wr_s, acc, tacc);
  }

  store_pairs<NT>(acc, pa_s, rec);   // over A, which is dead
  pass1_tail<NT>(tacc, swrr, slz, bad, tw, red, rec);
}

__global__ void __launch_bounds__(256) k_bf_pass1(BatchArgs a) {
  __shared__ __attribute__((aligned(16))) double xu_s[SGP_MAXD * MM], pa_s[MM * MM];
  __shared__ double vec_s[6 * MM + SGP_MAXD], xs[SGP_MAXD * 64], wt_s[4 * 16 * FXS], tw[4 * MM];
  const int seg = blockIdx.x;
  const int prob = a.seg_prob[seg];
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  if (a.out[(int64_t)prob * BATCH_OUT + 1] != 0.0) return;   // the problem failed in k_bf_k22
  const double* fw = a.fw + (int64_t)prob * BATCH_FW;
  const int64_t row0 = a.seg_row0[seg];
  const int rows = a.seg_rows[seg];
  double* rec = a.rec1 + (int64_t)seg * BATCH_REC1;
  SGP_BATCH_NT(P[BP_M],
               bf_pass1_body<NT>(a, P, fw, row0, rows, rec, xu_s, pa_s, vec_s, xs, wt_s, tw))
}

// ------------------------------------------------------------------------------ Bm's stage
__global__ void __launch_bounds__(256) k_bf_mm(BatchArgs a) {
  __shared__ __attribute__((aligned(16))) double Bm[MM * MM];
  __shared__ double t_s[MM], u_s[MM], ck[MM], red[256];
  const int prob = blockIdx.x, tid = threadIdx.x;
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  double* out = a.out + (int64_t)prob * BATCH_OUT;
  if (out[1] != 0.0) return;   // the problem failed in k_bf_k22
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2], delta = P[BP_DELTA];
  const double n = P[BP_NROW];
  const int seg0 = (int)P[BP_SEG0], nseg = (int)P[BP_NSEG];
  double* fw = a.fw + (int64_t)prob * BATCH_FW;
  const double* rec = a.rec1 + (int64_t)seg0 * BATCH_REC1;

  // the segment records, in segment order
  const double wrr = rec_sum(rec + BR_RR, BATCH_REC1, nseg);
  const double slz = rec_sum(rec + BR_LZ, BATCH_REC1, nseg);
  const double bad = rec_sum(rec + BR_BAD, BATCH_REC1, nseg);
  if (bad != 0.0) {   // some Z_i is not positive and finite: the reference's log(Z) is NaN
    if (tid == 0) {
      out[0] = NAN;
      fw[BF_BAD] = 1.0;
    }
    return;
  }
  for_mm(m, [&](int i, int j) {
    const double s = rec_sum(rec + i * MM + j, BATCH_REC1, nseg);
    Bm[i * MM + j] = k22(P, d, i, j, sig2, delta) + s;
  });
  if (tid < m) t_s[tid] = rec_sum(rec + BR_T + tid, BATCH_REC1, nseg);

  double ldB = 0.0;
  const int st = sweep_spd(Bm, m, ck, &ldB);
  if (st) {
    if (tid == 0) {
      out[0] = NAN;
      out[1] = (double)-st;
    }
    return;
  }
  if (tid < m) u_s[tid] = mat_vec_row(Bm, t_s, tid, m);
  __syncthreads();
  const double tu = block_sum(tid < m ? t_s[tid] * u_s[tid] : 0.0, red);

  // obj_fun_norm (laplace_approx_obj_funs.R:40-50)
  const double ld22 = fw[BF_LD];
  const double logdet22 = P[BP_RDET] != 0.0 ? log(exp(ld22)) : ld22;
  const double quad = -0.5 * wrr + 0.5 * tu;
  const double det_part = -0.5 * (slz - logdet22 + ldB);
  if (tid == 0) out[0] = quad + det_part - (n / 2.0) * log(2.0 * M_PI);
  store_post(a, prob, P, Bm, u_s, m);   // where the VI evaluation leaves it
  if (a.obj_only) return;
  for_mm(m, [&](int i, int j) { fw[BF_B + i * MM + j] = Bm[i * MM + j]; });
  if (tid < m) fw[BF_U + tid] = u_s[tid];
}

// ------------------------------------------------------------------------------ row pass 2
template <int NT, bool ARD>
__device__ __forceinline__ void bf_pass2_body(const BatchArgs& a, const double* __restrict__ P,
                                              const double* __restrict__ fw, int64_t row0, int rows,
                                              double* __restrict__ rec, double* xu_s, double* pa_s,
                                              double* pb_s, double* vec_s, double* xs, double* wt_s,
                                              double* red, double* el_s) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2];
  const double c0 = (sig2 + P[BP_TAU2]) + P[BP_DELTA];
  double* u_s = vec_s;             // [g][s]
  double* rs = vec_s + MM;         // 64: r of this step's rows
  double* om_s = vec_s + 2 * MM;   // 64: omega
  double* rl_s = vec_s + 3 * MM;   // d
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  double* wt = wt_s + wv * 16 * FXS;   // the wave's own k tile [row][knot]

  stage_knots(P, d, Mp, SN, xu_s, rl_s);
  stage_mat(fw + BF_A, m, Mp, pa_s);
  stage_mat(fw + BF_B, m, Mp, pb_s);
  stage_vec(fw + BF_U, m, Mp, SN, u_s);
  if (ARD)
    for (int q = tid; q < d * 64; q += 256) el_s[q] = 0.0;

  d4 acc[NT * (NT + 1) / 2];
#pragma unroll
  for (int p = 0; p < NT * (NT + 1) / 2; ++p) acc[p] = d4{0.0, 0.0, 0.0, 0.0};
  double esig = 0.0, el = 0.0, csum = 0.0, som = 0.0;

  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();   // the staging above / the previous step's reads of xs, the vectors and wt
    stage_x(a.X, a.ldx, row0, rows, step, d, xs);
    stage_r(a, row0, rows, step, rs);
    __syncthreads();

    double e2[SN], kf[SN];
    const bool iv = rows_k<SN>(xs, xu_s, rl_s, d, m, sig2, rows, step, e2, kf);
    d4 qa[NT], qb[NT];
    kmat2<NT>(pa_s, pb_s, kf, qa, qb);
    const double ku = k_dot<SN>(kf, u_s, g);
    const double z = c0 - row_dot<NT>(qa, kf);   // pass 1's bits
    const double pi = row_dot<NT>(qb, kf);
    const double wi = iv ? 1.0 / z : 0.0;
    const double al = wi * (rs[wv * 16 + r16] - ku);
    const double om = al * al - (wi - wi * wi * pi);
    if (g == 0) {
      som += om;
      om_s[wv * 16 + r16] = om;
    }
    // G = alpha u^T - w K Bm^-1 - omega K A
    grad_terms<NT, ARD>(
        [&](int cb, int r, int s) {
          return fma(al, u_s[g * SN + s], -fma(wi, qb[cb][r], om * qa[cb][r]));
        },
        kf, e2, iv, m, d, xs, xu_s, rl_s, el_s, esig, el, csum);
    put_ktile<SN>(wt, kf);
    __syncthreads();   // the k tile and omega are read across the wave's lanes
    rank_update_signed<NT>(wt, om_s, acc);   // S_omega
  }

  store_pairs<NT>(acc, pa_s, rec);   // over A, which is dead
  grad_tail<ARD>(esig, el, csum, som, d, red, el_s, rec);
}

template <bool ARD>
__global__ void __launch_bounds__(256) k_bf_pass2(BatchArgs a) {
  __shared__ __attribute__((aligned(16))) double xu_s[SGP_MAXD * MM], pa_s[MM * MM], pb_s[MM * MM];
  __shared__ double vec_s[3 * MM + SGP_MAXD], xs[SGP_MAXD * 64], wt_s[4 * 16 * FXS], red[256];
  __shared__ double el_s[ARD ? SGP_MAXD * 64 : 1];
  const int seg = blockIdx.x;
  const int prob = a.seg_prob[seg];
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  if (a.out[(int64_t)prob * BATCH_OUT + 1] != 0.0) return;   // not positive definite
  const double* fw = a.fw + (int64_t)prob * BATCH_FW;
  if (fw[BF_BAD] != 0.0) return;
  const int64_t row0 = a.seg_row0[seg];
  const int rows = a.seg_rows[seg];
  double* rec = a.rec4 + (int64_t)seg * BATCH_REC4;
  SGP_BATCH_NT(P[BP_M], bf_pass2_body<NT, ARD>(a, P, fw, row0, rows, rec, xu_s, pa_s, pb_s, vec_s,
                                               xs, wt_s, red, el_s))
}

// ------------------------------------------------------------------------------ G22 and finish
// G22 = -1/2 u u^T + 1/2 (K22^-1 - Bm^-1) + 1/2 K22^-1 S_omega K22^-1, contracted with
// dK22 / dlog theta (contract_h; tau: none, laplace_approx_gradient.R:899-902), then
// dlogp_dcov_par's gradient from the segments' sums
__global__ void __launch_bounds__(256) k_bf_g22(BatchArgs a) {
  __shared__ __attribute__((aligned(16))) double A[MM * MM], Bi[MM * MM], S[MM * MM], T[MM * MM];
  __shared__ double u_s[MM], red[256], r2[SGP_MAXD + 4], g22[SGP_MAXD + 1];
  const int prob = blockIdx.x, tid = threadIdx.x;
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  double* out = a.out + (int64_t)prob * BATCH_OUT;
  if (out[1] != 0.0) return;
  const int d = a.d, m = (int)P[BP_M];
  const int L = a.ard ? d : 1;
  const double* fw = a.fw + (int64_t)prob * BATCH_FW;
  if (fw[BF_BAD] != 0.0) {
    if (tid < L + 2) out[2 + tid] = NAN;
    return;
  }
  const double sig2 = P[BP_SIG2], tau2 = P[BP_TAU2];
  const int seg0 = (int)P[BP_SEG0], nseg = (int)P[BP_NSEG];
  const double* rec = a.rec4 + (int64_t)seg0 * BATCH_REC4;
  for_mm(m, [&](int i, int j) {
    A[i * MM + j] = fw[BF_A + i * MM + j];
    Bi[i * MM + j] = fw[BF_B + i * MM + j];
    S[i * MM + j] = rec_sum(rec + i * MM + j, BATCH_REC4, nseg);
  });
  if (tid < m) u_s[tid] = fw[BF_U + tid];
  if (tid < L + 3) r2[tid] = rec_sum(rec + BQ_W + tid, BATCH_REC4, nseg);
  __syncthreads();
  sandwich(A, S, T, m);
  for_mm(m, [&](int i, int j) {
    const double s = dot_mm(T, A, i, j, m);
    const double gv = -0.5 * u_s[i] * u_s[j] + 0.5 * (A[i * MM + j] - Bi[i * MM + j]) + 0.5 * s;
    S[i * MM + j] = gv * kuu(P, d, i, j, sig2);   // H: S is dead once T stands
  });
  __syncthreads();
  contract_h(P, d, m, a.ard, S, red, g22);
  __syncthreads();
  const double som = r2[2 + L];
  if (tid == 0) out[2] = 2.0 * r2[0] + g22[0] + sig2 * som;
  if (tid >= 1 && tid <= L) out[2 + tid] = r2[tid] + g22[tid];
  if (tid == L + 1) out[2 + tid] = 2.0 * tau2 * r2[1 + L] + tau2 * som;
}

}  // namespace

hipError_t launch_batch_eval_fitc(const BatchArgs& a, hipStream_t s, hipEvent_t* ev) {
  if (a.B < 1 || a.nseg < 1 || a.d < 1 || a.d > SGP_MAXD || !a.fw || !a.rec4)
    return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  if (ev && (e = hipEventRecord(ev[0], s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_bf_k22, dim3((unsigned)a.B), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[1], s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_bf_pass1, dim3((unsigned)a.nseg), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[2], s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_bf_mm, dim3((unsigned)a.B), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[3], s)) != hipSuccess) return e;
  if (!a.obj_only) {
    if (a.ard) hipLaunchKernelGGL(k_bf_pass2<true>, dim3((unsigned)a.nseg), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_bf_pass2<false>, dim3((unsigned)a.nseg), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[4], s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_bf_g22, dim3((unsigned)a.B), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  } else if (ev && (e = hipEventRecord(ev[4], s)) != hipSuccess) {
    return e;
  }
  if (ev) e = hipEventRecord(ev[5], s);
  return e;
}
