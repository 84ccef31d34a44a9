// Batched small-knot Titsias-VI evaluation (sgp_batch_eval_vi): B independent
// problems, each with its own rows, theta and m <= 64 knots, in four launches for the whole batch.
// Per problem the semantics are sgp_eval_vi's (elbo_fun R/vi_functions.R:64-121, trace_term_fun
// l.14-27, delbo_dcov_par l.126-419):
//   S = K^T K, t = K^T r, r^T r                                  k_batch_pass1, per segment
//   K22 = Kuu + delta I, Bm = K22 + S / z, their inverses and log-dets, u = Bm^-1 t / z,
//   P' = K22^-1 / tau^2 - Bm^-1 / z - u u^T / z, the objective, the G22 : dK22 terms
//                                                                k_batch_mm, per problem, in LDS
//   G = (r / z) u^T + K P', W = G o K, sum W dK/dlog theta       k_batch_pass2, per segment
//   the gradient                                                 k_batch_finish, per problem
// A segment is a run of at most SGP_BATCH_SEG_ROWS rows of one problem, counted from the problem's
// first row, so a problem's segments do not depend on what else the batch holds.  A workgroup of
// four waves takes 64 rows per step and forms k in registers in an operand layout of
// v_mfma_f64_16x16x4_f64: pass 1 with lane l on knot 16 b + (l & 15) and rows 4 q + (l >> 4) (k
// is then both operands of S += k k^T, and only the nb (nb + 1) / 2 block pairs are formed), pass
// 2 with lane l on row l & 15 and knots 4 s + (l >> 4), the layout of k_fit_scan, whose result
// layout meets it again for W = G o K.  Every sum has a fixed order, no kernel uses atomics, and
// nothing a problem computes reads another problem's data: results are bit-identical whatever
// the batch, the position, `active` or the repeat.
// Held-out prediction and scoring from that state (sgp_batch_predict), below
// the evaluation's kernels: k_batch_pred_mm per problem, k_batch_predict per test segment,
// k_batch_pred_finish per problem, under the same rules.
// The knot gradient (sgp_batch_eval_vi_knots) at the end of the file:
// k_batch_knot_pass per segment and k_batch_knot_finish per problem, after the evaluation's four
// launches, under the same rules again.
// The FITC evaluation of the same batch (sgp_batch_eval_fitc) is
// k_batch_fitc.hip; it leaves Bm^-1, u and the parameter block in `post` as k_batch_mm does, with
// the objective at BP_OBJ, so k_batch_post serves it unchanged and k_batch_pred_mm only chooses
// predict_laplace's constant (no delta) for it.
// The Laplace evaluation (sgp_batch_eval_laplace) is k_batch_laplace.hip; it leaves
// (K22 + S_B)^-1 and x1 there with BP_OBJ = 2, for which k_batch_post and k_batch_pred_mm put
// tau^2 + delta on K22's diagonal.
// sgp_batch_dev.h holds what the three files share: the fixed-order sums, the NT dispatch, the
// pieces of the m x m stages (for_mm, the sweep, Kuu, the sandwich's first half, the contraction
// of H, the posterior store) and of the row passes in pass 2's layout (the staging, rows_k, kmat,
// row_dot, k_dot, store_pairs).  Pass 1's knot-major k, pass 2's per-thread ARD slots and its
// coincidence counts, the prediction's statistics and the knot pass are this file's own.
#include <math.h>

#include "sgp_internal.h"
#include "sgp_batch_dev.h"
#include "sgp_quad.h"

namespace {

// ------------------------------------------------------------------------------ row pass 1
template <int NT>
__device__ __forceinline__ void pass1_body(const BatchArgs& a, const double* __restrict__ P,
                                           int64_t row0, int rows, double* __restrict__ rec,
                                           double* lds, double* tw, double* rrs, double* rl_s) {
  constexpr int Mp = 16 * NT;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2];
  double* u_s = lds;             // [c][Mp]
  double* xs = lds + d * MM;     // [c][64]
  double* rs = rrs + 64;         // 64: this step's r
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;

  for (int q = tid; q < d * Mp; q += 256) {
    const int c = q / Mp, j = q - c * Mp;
    u_s[c * Mp + j] = P[BP_U + c * MM + j];
  }
  for (int q = tid; q < d; q += 256) rl_s[q] = P[BP_RL + q];

  d4 acc[NT * (NT + 1) / 2];
#pragma unroll
  for (int p = 0; p < NT * (NT + 1) / 2; ++p) acc[p] = d4{0.0, 0.0, 0.0, 0.0};
  double tacc[NT];
#pragma unroll
  for (int b = 0; b < NT; ++b) tacc[b] = 0.0;
  double rracc = 0.0;

  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();   // the staging above / the previous step's reads of xs and rs
    stage_x(a.X, a.ldx, row0, rows, step, d, xs);
    if (tid < 64) {
      const int row = step * 64 + tid;
      const double r = row < rows ? a.y[row0 + row] - a.mu[row0 + row] : 0.0;
      rs[tid] = r;
      rracc = fma(r, r, rracc);
    }
    __syncthreads();

    double kf[NT][4];
#pragma unroll
    for (int b = 0; b < NT; ++b)
#pragma unroll
      for (int q = 0; q < 4; ++q) kf[b][q] = 0.0;
    const double* xr = xs + wv * 16 + g;
    for (int c = 0; c < d; ++c) {
      const double rl = rl_s[c];
      double xv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) xv[q] = xr[c * 64 + 4 * q];
#pragma unroll
      for (int b = 0; b < NT; ++b) {
        const double uv = u_s[c * Mp + 16 * b + r16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double t = (xv[q] - uv) * rl;   // the raw difference first
          kf[b][q] = fma(t, t, kf[b][q]);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      const bool jv = 16 * b + r16 < m;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool iv = step * 64 + wv * 16 + 4 * q + g < rows;
        const double v = sig2 * sgp_exp_nonpos(-0.5 * kf[b][q]);
        kf[b][q] = (jv && iv) ? v : 0.0;
        tacc[b] = fma(kf[b][q], rs[wv * 16 + 4 * q + g], tacc[b]);
      }
    }
    // S[16 bi + i][16 bj + j] += sum over the wave's 16 rows: A[i][row] = B[row][j] = k
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int p = 0;
#pragma unroll
      for (int bi = 0; bi < NT; ++bi)
#pragma unroll
        for (int bj = bi; bj < NT; ++bj, ++p)
          acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(kf[bi][q], kf[bj][q], acc[p], 0, 0, 0);
    }
  }

  // tw and rrs are arrays of their own, written before store_pairs so that its last barrier
  // serves them too; S goes over the dead knots and rows
  fold_tacc<NT>(tacc, tw);
  if (tid < 64) rrs[tid] = rracc;
  store_pairs<NT>(acc, lds, rec);
  if (tid < Mp) rec[BR_T + tid] = wave_sum4(tw, tid);
  if (tid == 0) {
    double rr = 0.0;
    for (int q = 0; q < 64; ++q) rr += rrs[q];
    rec[BR_RR] = rr;
  }
}

__global__ void __launch_bounds__(256) k_batch_pass1(BatchArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[MM * MM];
  __shared__ double tw[4 * MM], rrs[128], rl_s[SGP_MAXD];
  const int seg = blockIdx.x;
  const int prob = a.seg_prob[seg];
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  const int64_t row0 = a.seg_row0[seg];
  const int rows = a.seg_rows[seg];
  double* rec = a.rec1 + (int64_t)seg * BATCH_REC1;
  SGP_BATCH_NT(P[BP_M], pass1_body<NT>(a, P, row0, rows, rec, lds, tw, rrs, rl_s))
}

// ------------------------------------------------------------------------------ m x m stage
__global__ void __launch_bounds__(256) k_batch_mm(BatchArgs a) {
  __shared__ __attribute__((aligned(16))) double A[MM * MM], Bm[MM * MM], S[MM * MM], T[MM * MM];
  __shared__ double t_s[MM], u_s[MM], ck[MM], red[256];
  const int prob = blockIdx.x, tid = threadIdx.x;
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2], tau2 = P[BP_TAU2], z = P[BP_Z], delta = P[BP_DELTA];
  const double n = P[BP_NROW];
  const int seg0 = (int)P[BP_SEG0], nseg = (int)P[BP_NSEG];
  double* out = a.out + (int64_t)prob * BATCH_OUT;
  double* sc = a.sc + (int64_t)prob * BATCH_SC;

  // the segment records, in segment order
  for_mm(m, [&](int i, int j) {
    const double s = rec_sum(a.rec1 + (int64_t)seg0 * BATCH_REC1 + i * MM + j, BATCH_REC1, nseg);
    S[i * MM + j] = s;
    const double kd = k22(P, d, i, j, sig2, delta);
    A[i * MM + j] = kd;
    Bm[i * MM + j] = kd + s / z;
  });
  if (tid < m) t_s[tid] = rec_sum(a.rec1 + (int64_t)seg0 * BATCH_REC1 + BR_T + tid, BATCH_REC1, nseg);
  const double rr = rec_sum(a.rec1 + (int64_t)seg0 * BATCH_REC1 + BR_RR, BATCH_REC1, nseg);

  double ld22 = 0.0, ldB = 0.0;
  int st = sweep_spd(A, m, ck, &ld22);
  if (!st) st = -sweep_spd(Bm, m, ck, &ldB);
  if (st) {
    if (tid == 0) {
      out[0] = NAN;
      out[1] = (double)st;
    }
    return;
  }
  // A = K22^-1, Bm = Bm^-1
  if (tid < m) u_s[tid] = mat_vec_row(Bm, t_s, tid, m) / z;
  __syncthreads();
  const double su = tid < m ? mat_vec_row(S, u_s, tid, m) : 0.0;
  const double tu = block_sum(tid < m ? t_s[tid] * u_s[tid] : 0.0, red);
  const double uSu = block_sum(tid < m ? u_s[tid] * su : 0.0, red);
  double p1 = 0.0, p2 = 0.0;
  for_mm(m, [&](int i, int j) {
    p1 = fma(A[i * MM + j], S[i * MM + j], p1);
    p2 = fma(Bm[i * MM + j], S[i * MM + j], p2);
  });
  const double trKS = block_sum(p1, red);
  const double trBS = block_sum(p2, red);

  // elbo_fun (vi_functions.R:102-118)
  const double quad = -0.5 * rr / z + 0.5 * tu / z;
  const double logdet22 = P[BP_RDET] != 0.0 ? log(exp(ld22)) : ld22;
  const double det_part = -0.5 * (n * log(z) - logdet22 + ldB);
  const double trace_term = -(1.0 / (2.0 * tau2)) * (n * (sig2 + delta) - trKS);
  if (tid == 0) {
    out[0] = quad + det_part - (n / 2.0) * log(2.0 * M_PI) + trace_term;
    out[1] = 0.0;
    sc[BS_TRACE] = trace_term;
    sc[BS_TRBS] = trBS;
    sc[BS_ATA] = (rr - 2.0 * tu + uSu) / (z * z);
  }
  // what sgp_batch_posterior_u needs: Bm^-1, u and the problem's parameters and knots
  store_post(a, prob, P, Bm, u_s, m);
  if (a.obj_only) return;

  double* pm = a.pm + (int64_t)prob * BATCH_PM;
  for_mm(m, [&](int i, int j) {
    pm[i * MM + j] = A[i * MM + j] / tau2 - Bm[i * MM + j] / z - u_s[i] * u_s[j] / z;
  });
  if (tid < m) {
    pm[BPM_U + tid] = u_s[tid];
    pm[BPM_KD + tid] = A[tid * MM + tid];
  }
  // G22 = -1/2 u u^T + 1/2 (K22^-1 - Bm^-1) - K22^-1 S K22^-1 / (2 tau^2), contracted with
  // dK22 / dlog theta (contract_h; tau: none)
  sandwich(A, S, T, m);
  for_mm(m, [&](int i, int j) {
    const double s = dot_mm(T, A, i, j, m);
    const double g22 = -0.5 * u_s[i] * u_s[j] + 0.5 * (A[i * MM + j] - Bm[i * MM + j]) -
                       s / (2.0 * tau2);
    Bm[i * MM + j] = g22 * kuu(P, d, i, j, sig2);   // H: a thread rewrites only what it read
  });
  __syncthreads();
  if (a.hk) {   // sgp_batch_eval_vi_knots only: k_batch_knot_finish contracts H with the knots
    double* hk = a.hk + (int64_t)prob * BR_T;
    for_mm(m, [&](int i, int j) { hk[i * MM + j] = Bm[i * MM + j]; });
  }
  contract_h(P, d, m, a.ard, Bm, red, sc + BS_G22);
}

// ------------------------------------------------------------------------------ row pass 2
template <int NT, bool ARD>
__device__ __forceinline__ void pass2_body(const BatchArgs& a, const double* __restrict__ P,
                                           const double* __restrict__ pm, int64_t row0, int rows,
                                           double* __restrict__ rec, double* xu_s, double* pp_s,
                                           double* vec_s, double* xs, double* red, double* el_s) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2], rz = 1.0 / P[BP_Z];
  double* u_s = vec_s;             // [g][s]
  double* kd_s = vec_s + MM;       // [g][s]: the diagonal of K22^-1
  double* rs = vec_s + 2 * MM;     // 64: r / z of this step's rows
  double* rl_s = vec_s + 3 * MM;   // d
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;

  stage_knots(P, d, Mp, SN, xu_s, rl_s);
  stage_mat(pm, m, Mp, pp_s);
  stage_vec(pm + BPM_U, m, Mp, SN, u_s);
  stage_vec(pm + BPM_KD, m, Mp, SN, kd_s);
  if (ARD)
    for (int c = 0; c < d; ++c) el_s[c * 256 + tid] = 0.0;

  double esig = 0.0, el = 0.0, csum = 0.0, ccnt = 0.0, cdg = 0.0;
  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();
    stage_x(a.X, a.ldx, row0, rows, step, d, xs);
    if (tid < 64) {
      const int row = step * 64 + tid;
      rs[tid] = row < rows ? (a.y[row0 + row] - a.mu[row0 + row]) * rz : 0.0;
    }
    __syncthreads();

    double e2[SN], kf[SN];
    const bool iv = rows_k<SN>(xs, xu_s, rl_s, d, m, sig2, rows, step, e2, kf);
    const double* xr = xs + wv * 16 + r16;
    d4 acc[NT];
    kmat<NT>(pp_s, kf, acc);
    const double ri = rs[wv * 16 + r16];
    double w[SN];
#pragma unroll
    for (int cb = 0; cb < NT; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = 4 * cb + r;
        const double gv = fma(ri, u_s[g * SN + s], acc[cb][r]);   // G = (r / z) u^T + K P'
        w[s] = gv * kf[s];
        esig += w[s];
        if (!ARD) el = fma(w[s], e2[s], el);
        // quirk Q5: the tau derivative of a pair whose raw differences are all zero
        if (e2[s] == 0.0 && iv && 4 * s + g < m) {
          csum += gv;
          ccnt += 1.0;
          cdg += kd_s[g * SN + s];
        }
      }
    if (ARD)
      for (int c = 0; c < d; ++c) {
        const double xc = xr[c * 64], rl = rl_s[c];
        const double* u = xu_s + (c * 4 + g) * SN;
        double v = 0.0;
#pragma unroll
        for (int s = 0; s < SN; ++s) {
          const double t = (xc - u[s]) * rl;
          v = fma(w[s], t * t, v);
        }
        el_s[c * 256 + tid] += v;   // the thread's own slot
      }
  }

  const double e0 = block_sum(esig, red);
  const double e1 = block_sum(csum, red);
  const double e2s = block_sum(ccnt, red);
  const double e3 = block_sum(cdg, red);
  const int L = ARD ? d : 1;
  if (ARD) {
    for (int st = 128; st > 0; st >>= 1) {
      __syncthreads();
      for (int q = tid; q < d * st; q += 256) {
        const int c = q / st, i = q - c * st;
        el_s[c * 256 + i] += el_s[c * 256 + i + st];
      }
    }
    __syncthreads();
    if (tid < d) rec[1 + tid] = el_s[tid * 256];
  } else {
    const double e4 = block_sum(el, red);
    if (tid == 0) rec[1] = e4;
  }
  if (tid == 0) {
    rec[0] = e0;
    rec[1 + L] = e1;
    rec[2 + L] = e2s;
    rec[3 + L] = e3;
  }
}

template <bool ARD>
__global__ void __launch_bounds__(256) k_batch_pass2(BatchArgs a) {
  __shared__ __attribute__((aligned(16))) double xu_s[SGP_MAXD * MM], pp_s[MM * MM];
  __shared__ double vec_s[3 * MM + SGP_MAXD], xs[SGP_MAXD * 64], red[256];
  __shared__ double el_s[ARD ? SGP_MAXD * 256 : 1];
  const int seg = blockIdx.x;
  const int prob = a.seg_prob[seg];
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  if (a.out[(int64_t)prob * BATCH_OUT + 1] != 0.0) return;   // the problem failed in k_batch_mm
  const double* pm = a.pm + (int64_t)prob * BATCH_PM;
  const int64_t row0 = a.seg_row0[seg];
  const int rows = a.seg_rows[seg];
  double* rec = a.rec2 + (int64_t)seg * BATCH_REC2;
  SGP_BATCH_NT(P[BP_M],
               pass2_body<NT, ARD>(a, P, pm, row0, rows, rec, xu_s, pp_s, vec_s, xs, red, el_s))
}

// ------------------------------------------------------------------------------ finish
// delbo_dcov_par (vi_functions.R:259-419) in adjoint form, as sgp_vi_finish composes it
__global__ void __launch_bounds__(64) k_batch_finish(BatchArgs a) {
  __shared__ double r2[SGP_MAXD + 4];
  const int prob = blockIdx.x, tid = threadIdx.x;
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  double* out = a.out + (int64_t)prob * BATCH_OUT;
  if (out[1] != 0.0) return;
  const int L = a.ard ? a.d : 1;
  const int seg0 = (int)P[BP_SEG0], nseg = (int)P[BP_NSEG];
  if (tid < L + 4) r2[tid] = rec_sum(a.rec2 + (int64_t)seg0 * BATCH_REC2 + tid, BATCH_REC2, nseg);
  __syncthreads();
  const double* sc = a.sc + (int64_t)prob * BATCH_SC;
  const double sig2 = P[BP_SIG2], tau2 = P[BP_TAU2], z = P[BP_Z], delta = P[BP_DELTA];
  const double n = P[BP_NROW];
  if (tid == 0) out[2] = 2.0 * r2[0] + sc[BS_G22] - n * sig2 / tau2;
  if (tid >= 1 && tid <= L) out[2 + tid] = r2[tid] + sc[BS_G22 + tid];
  if (tid == L + 1) {
    const double c_sum = r2[1 + L], c_cnt = r2[2 + L], c_dg = r2[3 + L];
    const double trSinv = n / z - sc[BS_TRBS] / (z * z);
    const double trW = 0.5 * (sc[BS_ATA] - trSinv);
    out[2 + tid] = 2.0 * tau2 * (c_sum - (c_cnt - delta * c_dg) / tau2) + 2.0 * tau2 * trW -
                   2.0 * sc[BS_TRACE];
  }
}

// ------------------------------------------------------------------------------ posterior
// vi_functions.R:1161-1180 as sgp_posterior_u evaluates it: u_mean - muu = K22 u,
// u_var = K22 Bm^-1 K22, from the state the problem's last successful evaluation left
__global__ void __launch_bounds__(256) k_batch_post(BatchArgs a, double* __restrict__ res) {
  __shared__ __attribute__((aligned(16))) double A[MM * MM], Bm[MM * MM], T[MM * MM];
  __shared__ double u_s[MM];
  const int prob = blockIdx.x, tid = threadIdx.x;
  const double* post = a.post + (int64_t)prob * a.post_stride;
  const double* P = post + MM * MM + MM;
  if (P[BP_ACTIVE] == 0.0) return;   // no successful evaluation yet (the state starts zeroed)
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2];
  // K22's diagonal: delta, and tau^2 + delta where the evaluation was a Laplace one (quirk Q1)
  const double delta = P[BP_OBJ] == 2.0 ? P[BP_TAU2] + P[BP_DELTA] : P[BP_DELTA];
  for_mm(m, [&](int i, int j) {
    A[i * MM + j] = k22(P, d, i, j, sig2, delta);
    Bm[i * MM + j] = post[i * MM + j];
  });
  if (tid < m) u_s[tid] = post[MM * MM + tid];
  __syncthreads();
  sandwich(A, Bm, T, m);
  double* r = res + (int64_t)prob * (MM * MM + MM);
  for_mm(m, [&](int i, int j) { r[i * MM + j] = dot_mm(T, A, i, j, m); });
  if (tid < m) r[MM * MM + tid] = mat_vec_row(A, u_s, tid, m);
}

// ------------------------------------------------------------------------------ prediction
// sgp_batch_predict: predict_vi (R/vi_functions.R:1222-1336) on the state the
// problem's last successful evaluation left in `post`.  With u_mean - muu = K22 u and u_var =
// K22 Bm^-1 K22 the reference's Sigma22^-1 (u_mean - muu) is u and its Sigma22^-1 u_var Sigma22^-1
// - Sigma22^-1 is T = Bm^-1 - K22^-1:
//   pred_mean_i = mu_i + k_i^T u,   pred_var_i = (tau^2 + sigma^2) + delta + k_i^T T k_i
// K22 is rebuilt as k_batch_mm built it and swept by the same code, so the sweep succeeds as it
// did there.
__global__ void __launch_bounds__(256) k_batch_pred_mm(BatchArgs a, BatchPredArgs p) {
  __shared__ __attribute__((aligned(16))) double A[MM * MM];
  __shared__ double ck[MM];
  const int prob = blockIdx.x, tid = threadIdx.x;
  if (!p.act[prob]) return;
  const double* post = a.post + (int64_t)prob * a.post_stride;
  const double* P = post + MM * MM + MM;
  if (P[BP_ACTIVE] == 0.0) return;   // no successful evaluation (the host refuses this before)
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2], tau2 = P[BP_TAU2], delta = P[BP_DELTA];
  // predict_laplace(family != "gaussian") keeps tau^2 on Sigma22's diagonal (sec. 0s)
  const double dg = P[BP_OBJ] == 2.0 ? tau2 + delta : delta;
  double ld22 = 0.0;
  const int st = k22_inverse(P, d, dg, A, ck, &ld22);
  double* w = p.pw + (int64_t)prob * BATCH_PW;
  // predict_laplace's constant has no delta (laplace_approx_prediction.R:3-123; sec. 0q)
  if (tid == 0)
    w[BPW_C0] = st ? NAN : (P[BP_OBJ] != 0.0 ? tau2 + sig2 : (tau2 + sig2) + delta);
  if (st) return;
  for_mm(m, [&](int i, int j) { w[i * MM + j] = post[i * MM + j] - A[i * MM + j]; });
}

// One test segment: 64 rows per step in pass 2's layout (lane l on row l & 15 and knots
// 4 s + (l >> 4)); Q = K T by MFMA with T the A operand from LDS, whose result layout meets k's
// again at s = 4 cb + r, so k^T T k = sum_j Q_ij K_ij and k^T u are fma chains over s in the lane
// and one xor-shuffle over the four lane groups.  sv: 4 x 64, the step's rows' stats terms; the
// four sums go over the rows in row order (thread q < 4 owns sum q).
template <int NT>
__device__ __forceinline__ void predict_body(const BatchArgs& a, const BatchPredArgs& p,
                                             const double* __restrict__ post,
                                             const double* __restrict__ w, int64_t row0, int rows,
                                             int64_t out0, double* __restrict__ rec, double* xu_s,
                                             double* pp_s, double* vec_s, double* xs, double* sv) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const double* P = post + MM * MM + MM;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2], c0 = w[BPW_C0], tau = sqrt(P[BP_TAU2]);
  double* u_s = vec_s;             // [g][s]
  double* mus = vec_s + MM;        // 64: mu of this step's rows
  double* ys = vec_s + 2 * MM;     // 64: y of this step's rows
  double* rl_s = vec_s + 3 * MM;   // d
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  const bool score = p.score != 0;

  stage_knots(P, d, Mp, SN, xu_s, rl_s);
  stage_mat(w, m, Mp, pp_s);
  stage_vec(post + MM * MM, m, Mp, SN, u_s);

  double ssum = 0.0;   // thread q < 4: stats term q over the rows so far
  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();   // the staging above / the previous step's reads of xs and writes of sv
    stage_x(p.Xt, p.ldxt, row0, rows, step, d, xs);
    if (tid < 64) {
      const int row = step * 64 + tid;
      mus[tid] = row < rows ? p.mut[row0 + row] : 0.0;
      ys[tid] = (score && row < rows) ? p.yt[row0 + row] : 0.0;
    }
    if (score && step > 0 && tid < 4)   // the previous step's 64 rows
      for (int i = 0; i < 64; ++i) ssum += sv[tid * 64 + i];
    __syncthreads();

    const int row = step * 64 + wv * 16 + r16;
    double e2[SN], kf[SN];
    const bool iv = rows_k<SN>(xs, xu_s, rl_s, d, m, sig2, rows, step, e2, kf);
    d4 acc[NT];
    kmat<NT>(pp_s, kf, acc);
    const double ku = k_dot<SN>(kf, u_s, g), kq = row_dot<NT>(acc, kf);
    if (g == 0) {
      const int i = wv * 16 + r16;
      const double mean = mus[i] + ku, var = c0 + kq;
      if (iv) {
        p.pm[out0 + row] = mean;
        p.pv[out0 + row] = var;
      }
      if (score) {
        const double y = ys[i];
        const double v = quad_nlp_gaussian(y, mean, var, tau);
        if (iv) p.nlp[out0 + row] = v;
        const bool fin = iv && fabs(v) <= 1.79769313486231570815e308;
        const double e = mean - y;
        sv[i] = fin ? v : 0.0;
        sv[64 + i] = fin ? 1.0 : 0.0;
        sv[128 + i] = (iv && v != v) ? 1.0 : 0.0;
        sv[192 + i] = iv ? e * e : 0.0;
      }
    }
  }
  if (score) {
    __syncthreads();
    if (tid < 4) {
      const int last = rows - ((rows - 1) >> 6) * 64;   // the rows of the last step
      for (int i = 0; i < last; ++i) ssum += sv[tid * 64 + i];
      rec[tid] = ssum;
    }
  }
}

__global__ void __launch_bounds__(256) k_batch_predict(BatchArgs a, BatchPredArgs p) {
  __shared__ __attribute__((aligned(16))) double xu_s[SGP_MAXD * MM], pp_s[MM * MM];
  __shared__ double vec_s[3 * MM + SGP_MAXD], xs[SGP_MAXD * 64], sv[4 * 64];
  const int seg = blockIdx.x;
  const int prob = p.seg_prob[seg];
  if (!p.act[prob]) return;
  const double* post = a.post + (int64_t)prob * a.post_stride;
  if (post[MM * MM + MM + BP_ACTIVE] == 0.0) return;
  const double* w = p.pw + (int64_t)prob * BATCH_PW;
  const int64_t row0 = p.seg_row0[seg], out0 = p.seg_out[seg];
  const int rows = p.seg_rows[seg];
  double* rec = p.rec + (int64_t)seg * BATCH_PREC;
  SGP_BATCH_NT(post[MM * MM + MM + BP_M],
               predict_body<NT>(a, p, post, w, row0, rows, out0, rec, xu_s, pp_s, vec_s, xs, sv))
}

// the segments' records, in segment order
__global__ void __launch_bounds__(64) k_batch_pred_finish(BatchArgs a, BatchPredArgs p) {
  const int prob = blockIdx.x, tid = threadIdx.x;
  if (!p.act[prob]) return;
  if (a.post[(int64_t)prob * a.post_stride + MM * MM + MM + BP_ACTIVE] == 0.0) return;
  const int seg0 = p.prob_seg[2 * prob], nseg = p.prob_seg[2 * prob + 1];
  if (tid < 4)
    p.stats[4 * prob + tid] = rec_sum(p.rec + (int64_t)seg0 * BATCH_PREC + tid, BATCH_PREC, nseg);
}

// ------------------------------------------------------------------------------ knot gradient
// sgp_batch_eval_vi_knots: delbo_dcov_par's knot branch
// (R/vi_functions.R:425-593) with dsqexp_dx2 / dsqexp_dx2_ard
// (R/covariance_function_derivatives.R:178-302) in adjoint form.  With W = G o K of pass 2 and
// H = G22 o Kuu of the m x m stage,
//   R_kc = sum_i W_ik (x_ic - u_kc),  Q_kc = 2 sum_l H_kl (u_lc - u_kc),
//   dELBO / du_kc = (R_kc + Q_kc) / l_c^2, times the bounded transform's factor (quirk Q8).
// The row pass forms T = W^T (X - o) and the column sums of W per segment, with o the problem's
// first knot, so R_kc = T_kc - (u_kc - o_c) sum_i W_ik loses nothing to the size of the
// coordinates.  k, G and W are rebuilt as pass2_body builds them; each wave then turns its
// 16 x Mp tile of W through wave-private LDS into the A operand (knot on l & 15, rows
// 4 q + (l >> 4)) and takes the staged x tile as the B operand (coordinate on l & 15), so the
// MFMA contracts over the rows.
constexpr int KXS = 68;   // the x tile's coordinate stride and the W tile's row stride (doubles)

template <int NT, int NCB>
__device__ __forceinline__ void knot_body(const BatchArgs& a, const double* __restrict__ P,
                                          const double* __restrict__ pm, int64_t row0, int rows,
                                          double* __restrict__ rec, double* xu_s, double* pp_s,
                                          double* vec_s, double* xs, double* wt_s) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2], rz = 1.0 / P[BP_Z];
  double* u_s = vec_s;             // [g][s]
  double* rs = vec_s + MM;         // 64: r / z of this step's rows
  double* rl_s = vec_s + 2 * MM;   // d
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  double* wt = wt_s + wv * 16 * KXS;   // the wave's own W tile [row][knot]

  stage_knots(P, d, Mp, SN, xu_s, rl_s);
  stage_mat(pm, m, Mp, pp_s);
  stage_vec(pm + BPM_U, m, Mp, SN, u_s);
  double ob[NCB];   // the offset of this lane's coordinate in block cb
  bool cv[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    cv[cb] = 16 * cb + r16 < d;
    ob[cb] = cv[cb] ? P[BP_U + (16 * cb + r16) * MM] : 0.0;
  }

  d4 racc[NT][NCB];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) racc[t][cb] = d4{0.0, 0.0, 0.0, 0.0};
  double cs[SN];
#pragma unroll
  for (int s = 0; s < SN; ++s) cs[s] = 0.0;

  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();   // the staging above / the previous step's reads of xs, rs and wt
    stage_x(a.X, a.ldx, row0, rows, step, d, xs, KXS);
    if (tid < 64) {
      const int row = step * 64 + tid;
      rs[tid] = row < rows ? (a.y[row0 + row] - a.mu[row0 + row]) * rz : 0.0;
    }
    __syncthreads();

    double e2[SN], kf[SN];
    rows_k<SN>(xs, xu_s, rl_s, d, m, sig2, rows, step, e2, kf, KXS);
    d4 acc[NT];
    kmat<NT>(pp_s, kf, acc);
    const double ri = rs[wv * 16 + r16];
#pragma unroll
    for (int cb = 0; cb < NT; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = 4 * cb + r;
        const double gv = fma(ri, u_s[g * SN + s], acc[cb][r]);   // G = (r / z) u^T + K P'
        const double w = gv * kf[s];
        cs[s] += w;
        wt[r16 * KXS + 4 * s + g] = w;
      }
    __syncthreads();   // the W tile is read across the wave's lanes
    // T[16 t + i][16 cb + j] += sum over the wave's 16 rows: A[i][row] = W, B[row][j] = x - o
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double bx[NCB];
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
        bx[cb] = cv[cb] ? xs[(16 * cb + r16) * KXS + wv * 16 + 4 * q + g] - ob[cb] : 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const double aw = wt[(4 * q + g) * KXS + 16 * t + r16];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
          racc[t][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(aw, bx[cb], racc[t][cb], 0, 0, 0);
      }
    }
  }

  // the four waves' partial T, added in wave order into LDS (over P', which is dead), and the
  // column sums: over the lane's rows in step order, the 16 lanes by xor-shuffle, the waves in
  // wave order
  double* tb = pp_s;   // [knot][32]
  double* cw = wt_s;   // [wave][64]
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wv == w) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double* s = tb + (16 * t + 4 * r + g) * SGP_MAXD + 16 * cb + r16;
            *s = w ? *s + racc[t][cb][r] : racc[t][cb][r];
          }
    }
  }
#pragma unroll
  for (int s = 0; s < SN; ++s) {
    double v = cs[s];
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    if (r16 == 0) cw[wv * MM + 4 * s + g] = v;
  }
  __syncthreads();
  for (int q = tid; q < m * d; q += 256) {
    const int k = q / d, c = q - k * d;
    rec[k * SGP_MAXD + c] = tb[k * SGP_MAXD + c];
  }
  if (tid < m) rec[BK_CS + tid] = wave_sum4(cw, tid);
}

__global__ void __launch_bounds__(256) k_batch_knot_pass(BatchArgs a) {
  __shared__ __attribute__((aligned(16))) double xu_s[SGP_MAXD * MM], pp_s[MM * MM];
  __shared__ double vec_s[2 * MM + SGP_MAXD], xs[SGP_MAXD * KXS], wt_s[4 * 16 * KXS];
  const int seg = blockIdx.x;
  const int prob = a.seg_prob[seg];
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  if (a.out[(int64_t)prob * BATCH_OUT + 1] != 0.0) return;   // the problem failed in k_batch_mm
  const double* pm = a.pm + (int64_t)prob * BATCH_PM;
  const int64_t row0 = a.seg_row0[seg];
  const int rows = a.seg_rows[seg];
  double* rec = a.rec3 + (int64_t)seg * BATCH_REC3;
  SGP_BATCH_NT(
      P[BP_M],
      if (a.d > 16) knot_body<NT, 2>(a, P, pm, row0, rows, rec, xu_s, pp_s, vec_s, xs, wt_s);
      else knot_body<NT, 1>(a, P, pm, row0, rows, rec, xu_s, pp_s, vec_s, xs, wt_s))
}

// The segments' records in segment order, the K22 part from H and the knots, 1 / l_c^2 and the
// chain factor of the bounded transform; problem b's m d values go out knot-major (quirk Q16) at
// its offset in the packed result.
__global__ void __launch_bounds__(256) k_batch_knot_finish(BatchArgs a) {
  __shared__ double H[MM * MM], cs[MM];
  const int prob = blockIdx.x, tid = threadIdx.x;
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  if (a.out[(int64_t)prob * BATCH_OUT + 1] != 0.0) return;
  const int d = a.d, m = (int)P[BP_M];
  const int seg0 = (int)P[BP_SEG0], nseg = (int)P[BP_NSEG];
  const double* rec = a.rec3 + (int64_t)seg0 * BATCH_REC3;
  const double* hk = a.hk + (int64_t)prob * BR_T;
  for_mm(m, [&](int i, int j) { H[i * MM + j] = hk[i * MM + j]; });
  if (tid < m) cs[tid] = rec_sum(rec + BK_CS + tid, BATCH_REC3, nseg);
  __syncthreads();
  double* gk = a.gk + (int64_t)P[BP_GOFF];
  const double* bnd = a.bnd ? a.bnd + (int64_t)prob * 2 * d : nullptr;   // [lower | upper], d each
  for (int q = tid; q < m * d; q += 256) {
    const int k = q / d, c = q - k * d;
    const double* u = P + BP_U + c * MM;
    const double ukc = u[k];
    const double r = rec_sum(rec + k * SGP_MAXD + c, BATCH_REC3, nseg) - (ukc - u[0]) * cs[k];
    double h = 0.0;
    for (int l = 0; l < m; ++l) h = fma(H[k * MM + l], u[l] - ukc, h);
    const double rl = P[BP_RL + c];
    double v = (r + 2.0 * h) * (rl * rl);
    if (bnd) {
      const double lb = bnd[c], ub = bnd[d + c];
      v *= (ub - lb) / ((ukc - lb) * (ub - ukc) + 1e-4);
    }
    gk[q] = v;
  }
}

}  // namespace

hipError_t launch_batch_eval(const BatchArgs& a, hipStream_t s, hipEvent_t* ev) {
  if (a.B < 1 || a.nseg < 1 || a.d < 1 || a.d > SGP_MAXD) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  if (ev) e = hipEventRecord(ev[0], s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_batch_pass1, dim3((unsigned)a.nseg), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[1], s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_batch_mm, dim3((unsigned)a.B), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[2], s)) != hipSuccess) return e;
  if (!a.obj_only) {
    if (a.ard) hipLaunchKernelGGL(k_batch_pass2<true>, dim3((unsigned)a.nseg), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_batch_pass2<false>, dim3((unsigned)a.nseg), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (ev && (e = hipEventRecord(ev[3], s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_batch_finish, dim3((unsigned)a.B), dim3(64), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  } else if (ev && (e = hipEventRecord(ev[3], s)) != hipSuccess) {
    return e;
  }
  if (ev) e = hipEventRecord(ev[4], s);
  return e;
}

hipError_t launch_batch_post(const BatchArgs& a, double* res, hipStream_t s) {
  if (a.B < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_batch_post, dim3((unsigned)a.B), dim3(256), 0, s, a, res);
  return hipGetLastError();
}

hipError_t launch_batch_predict(const BatchArgs& a, const BatchPredArgs& p, hipStream_t s,
                                hipEvent_t* ev) {
  if (a.B < 1 || p.nseg < 0 || a.d < 1 || a.d > SGP_MAXD) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  if (ev && (e = hipEventRecord(ev[0], s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_batch_pred_mm, dim3((unsigned)a.B), dim3(256), 0, s, a, p);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[1], s)) != hipSuccess) return e;
  if (p.nseg > 0) {
    hipLaunchKernelGGL(k_batch_predict, dim3((unsigned)p.nseg), dim3(256), 0, s, a, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev && (e = hipEventRecord(ev[2], s)) != hipSuccess) return e;
  if (p.score) {
    hipLaunchKernelGGL(k_batch_pred_finish, dim3((unsigned)a.B), dim3(64), 0, s, a, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (ev) e = hipEventRecord(ev[3], s);
  return e;
}

hipError_t launch_batch_knots(const BatchArgs& a, hipStream_t s, hipEvent_t* ev) {
  if (a.B < 1 || a.nseg < 1 || a.d < 1 || a.d > SGP_MAXD || !a.hk || !a.rec3 || !a.gk)
    return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  if (ev && (e = hipEventRecord(ev[0], s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_batch_knot_pass, dim3((unsigned)a.nseg), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev && (e = hipEventRecord(ev[1], s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_batch_knot_finish, dim3((unsigned)a.B), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (ev) e = hipEventRecord(ev[2], s);
  return e;
}
