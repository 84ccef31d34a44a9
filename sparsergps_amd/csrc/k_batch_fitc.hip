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
// The segments, the 64-row steps and the per-row bounds test are k_batch.hip's.  Both row passes
// form k in k_fit_scan's operand layout of v_mfma_f64_16x16x4_f64 (lane l on row l & 15 and knots
// 4 s + (l >> 4)), in which K A and K Bm^-1 are MFMAs against an operand in LDS and q, p and
// k^T u are fma chains in the lane and one xor-shuffle over the four lane groups.  Each wave
// then turns its 16 x Mp tile of k through wave-private LDS into pass 1's layout (knot on l & 15,
// rows 4 q + (l >> 4)) for the nb (nb + 1) / 2 block pairs of the rank-update: both operands
// scaled by sqrt(w_i) for S, one operand scaled by omega_i for S_omega, whose weights take both
// signs.  The row weights are recomputed from k in each pass, so nothing is indexed by the
// resident row and aliased row ranges need no work vector.  Every sum has a fixed order, no
// kernel uses atomics, and nothing a problem computes reads another problem's data.
#include <math.h>

#include "sgp_internal.h"
#include "sgp_batch_dev.h"

namespace {

constexpr int FXS = 68;   // the wave-private k tile's row stride (doubles)

// ------------------------------------------------------------------------------ K22's stage
__global__ void __launch_bounds__(256) k_bf_k22(BatchArgs a) {
  __shared__ __attribute__((aligned(16))) double A[MM * MM];
  __shared__ double ck[MM];
  const int prob = blockIdx.x, tid = threadIdx.x;
  const double* P = a.par + (int64_t)prob * a.pst;
  if (P[BP_ACTIVE] == 0.0) return;
  const int d = a.d, m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2], delta = P[BP_DELTA];
  double* out = a.out + (int64_t)prob * BATCH_OUT;
  double* fw = a.fw + (int64_t)prob * BATCH_FW;
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    A[i * MM + j] = sig2 * sgp_exp_nonpos(-0.5 * knot_dist2(P, d, i, j)) + (i == j ? delta : 0.0);
  }
  double ld22 = 0.0;
  const int st = sweep_spd(A, m, ck, &ld22);
  if (tid == 0) {
    out[0] = st ? NAN : 0.0;
    out[1] = (double)st;
    fw[BF_LD] = ld22;
    fw[BF_BAD] = 0.0;
  }
  if (st) return;
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    fw[BF_A + i * MM + j] = A[i * MM + j];
  }
}

// k of the step's rows in k_fit_scan's layout: e2[s] the scaled squared distance of row r16 of
// the wave's 16 and knot 4 s + g, kf[s] the covariance (zero beyond the rows and the knots)
#define SGP_BF_ROWS_K()                                                            \
  const bool iv = step * 64 + wv * 16 + r16 < rows;                                \
  const double* xr = xs + wv * 16 + r16;                                           \
  double e2[SN], kf[SN];                                                           \
  _Pragma("unroll") for (int s = 0; s < SN; ++s) e2[s] = 0.0;                      \
  for (int c = 0; c < d; ++c) {                                                    \
    const double xc = xr[c * 64], rl = rl_s[c];                                    \
    const double* u = xu_s + (c * 4 + g) * SN;                                     \
    _Pragma("unroll") for (int s = 0; s < SN; ++s) {                               \
      const double t = (xc - u[s]) * rl; /* the raw difference first, as in pass 2 */ \
      e2[s] = fma(t, t, e2[s]);                                                    \
    }                                                                              \
  }                                                                                \
  _Pragma("unroll") for (int s = 0; s < SN; ++s) {                                 \
    const double v = sig2 * sgp_exp_nonpos(-0.5 * e2[s]);                          \
    kf[s] = (iv && 4 * s + g < m) ? v : 0.0;                                       \
  }

// sum over the lane's knots of acc o k, then over the four lane groups: every lane of a row
// ends with the same bits
template <int NT>
__device__ __forceinline__ double row_dot(const d4* acc, const double* kf) {
  double v = 0.0;
#pragma unroll
  for (int cb = 0; cb < NT; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) v = fma(acc[cb][r], kf[4 * cb + r], v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// the four waves' partial block pairs, added in wave order into lds (row stride 64), mirrored
// into rec (row stride 64)
template <int NT>
__device__ __forceinline__ void store_pairs(const d4* acc, double* lds, double* __restrict__ rec) {
  constexpr int Mp = 16 * NT;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wv == w) {
      int p = 0;
#pragma unroll
      for (int bi = 0; bi < NT; ++bi)
#pragma unroll
        for (int bj = bi; bj < NT; ++bj, ++p)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double* s = lds + (16 * bi + 4 * r + g) * MM + 16 * bj + r16;
            *s = w ? *s + acc[p][r] : acc[p][r];
          }
    }
  }
  __syncthreads();
  for (int q = tid; q < Mp * Mp; q += 256) {
    const int i = q / Mp, j = q - i * Mp;
    rec[i * MM + j] = (i >> 4) > (j >> 4) ? lds[j * MM + i] : lds[i * MM + j];
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

  for (int q = tid; q < d * Mp; q += 256) {
    const int c = q / Mp, j = q - c * Mp;
    xu_s[(c * 4 + (j & 3)) * SN + (j >> 2)] = P[BP_U + c * MM + j];
  }
  for (int q = tid; q < Mp * Mp; q += 256) {
    const int i = q / Mp, j = q - i * Mp;
    pa_s[q] = (i < m && j < m) ? fw[BF_A + i * MM + j] : 0.0;
  }
  for (int q = tid; q < d; q += 256) rl_s[q] = P[BP_RL + q];

  d4 acc[NT * (NT + 1) / 2];
#pragma unroll
  for (int p = 0; p < NT * (NT + 1) / 2; ++p) acc[p] = d4{0.0, 0.0, 0.0, 0.0};
  double tacc[NT];
#pragma unroll
  for (int b = 0; b < NT; ++b) tacc[b] = 0.0;
  double swrr = 0.0, slz = 0.0, bad = 0.0;

  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();   // the staging above / the previous step's reads of xs, the vectors and wt
    for (int q = tid; q < d * 64; q += 256) {
      const int c = q >> 6, i = q & 63;
      const int row = step * 64 + i;
      xs[q] = row < rows ? a.X[(int64_t)c * a.ldx + row0 + row] : 0.0;
    }
    if (tid < 64) {
      const int row = step * 64 + tid;
      rs[tid] = row < rows ? a.y[row0 + row] - a.mu[row0 + row] : 0.0;
    }
    __syncthreads();

    SGP_BF_ROWS_K()
    d4 qa[NT];
#pragma unroll
    for (int cb = 0; cb < NT; ++cb) qa[cb] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < SN; ++s)
#pragma unroll
      for (int cb = 0; cb < NT; ++cb)
        qa[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa_s[(4 * s + g) * Mp + 16 * cb + r16],
                                                      kf[s], qa[cb], 0, 0, 0);
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
#pragma unroll
    for (int s = 0; s < SN; ++s) wt[r16 * FXS + 4 * s + g] = kf[s];
    __syncthreads();   // the k tile and the weights are read across the wave's lanes
    // S[16 bi + i][16 bj + j] += sum over the wave's 16 rows: A[i][row] = B[row][j] = sqrt(w) k
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

  store_pairs<NT>(acc, pa_s, rec);   // over A, which is dead
#pragma unroll
  for (int b = 0; b < NT; ++b) {
    double t = tacc[b];
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    if (g == 0) tw[wv * MM + 16 * b + r16] = t;
  }
  if (g == 0) {
    red[wv * 16 + r16] = swrr;
    red[MM + wv * 16 + r16] = slz;
    red[2 * MM + wv * 16 + r16] = bad;
  }
  __syncthreads();
  if (tid < Mp) rec[BR_T + tid] = ((tw[tid] + tw[MM + tid]) + tw[2 * MM + tid]) + tw[3 * MM + tid];
  if (tid < 3) {
    double v = 0.0;
    for (int q = 0; q < 64; ++q) v += red[tid * MM + q];
    rec[BR_RR + tid] = v;
  }
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
  switch (((int)P[BP_M] + 15) >> 4) {
    case 1: bf_pass1_body<1>(a, P, fw, row0, rows, rec, xu_s, pa_s, vec_s, xs, wt_s, tw); break;
    case 2: bf_pass1_body<2>(a, P, fw, row0, rows, rec, xu_s, pa_s, vec_s, xs, wt_s, tw); break;
    case 3: bf_pass1_body<3>(a, P, fw, row0, rows, rec, xu_s, pa_s, vec_s, xs, wt_s, tw); break;
    default: bf_pass1_body<4>(a, P, fw, row0, rows, rec, xu_s, pa_s, vec_s, xs, wt_s, tw); break;
  }
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
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    const double s = rec_sum(rec + i * MM + j, BATCH_REC1, nseg);
    const double kuu = sig2 * sgp_exp_nonpos(-0.5 * knot_dist2(P, d, i, j));
    Bm[i * MM + j] = (kuu + (i == j ? delta : 0.0)) + s;
  }
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
  if (tid < m) {
    double s = 0.0;
    for (int k = 0; k < m; ++k) s = fma(Bm[tid * MM + k], t_s[k], s);
    u_s[tid] = s;
  }
  __syncthreads();
  const double tu = block_sum(tid < m ? t_s[tid] * u_s[tid] : 0.0, red);

  // obj_fun_norm (laplace_approx_obj_funs.R:40-50)
  const double ld22 = fw[BF_LD];
  const double logdet22 = P[BP_RDET] != 0.0 ? log(exp(ld22)) : ld22;
  const double quad = -0.5 * wrr + 0.5 * tu;
  const double det_part = -0.5 * (slz - logdet22 + ldB);
  if (tid == 0) out[0] = quad + det_part - (n / 2.0) * log(2.0 * M_PI);
  // what sgp_batch_posterior_u and sgp_batch_predict need, where the VI evaluation leaves it
  double* post = a.post + (int64_t)prob * a.post_stride;
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    post[i * MM + j] = Bm[i * MM + j];
  }
  if (tid < m) post[MM * MM + tid] = u_s[tid];
  for (int q = tid; q < a.pst; q += 256) post[MM * MM + MM + q] = P[q];
  if (a.obj_only) return;
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    fw[BF_B + i * MM + j] = Bm[i * MM + j];
  }
  if (tid < m) fw[BF_U + tid] = u_s[tid];
}

// ------------------------------------------------------------------------------ row pass 2
// el_s (ARD): [c][wave][16] slots, one per row lane of a wave: the lane groups are folded by
// shuffles first, so the d running sums take 16 KiB beside the two m x m operands
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

  for (int q = tid; q < d * Mp; q += 256) {
    const int c = q / Mp, j = q - c * Mp;
    xu_s[(c * 4 + (j & 3)) * SN + (j >> 2)] = P[BP_U + c * MM + j];
  }
  for (int q = tid; q < Mp * Mp; q += 256) {
    const int i = q / Mp, j = q - i * Mp;
    const bool in = i < m && j < m;
    pa_s[q] = in ? fw[BF_A + i * MM + j] : 0.0;
    pb_s[q] = in ? fw[BF_B + i * MM + j] : 0.0;
  }
  for (int q = tid; q < Mp; q += 256) u_s[(q & 3) * SN + (q >> 2)] = q < m ? fw[BF_U + q] : 0.0;
  for (int q = tid; q < d; q += 256) rl_s[q] = P[BP_RL + q];
  if (ARD)
    for (int q = tid; q < d * 64; q += 256) el_s[q] = 0.0;

  d4 acc[NT * (NT + 1) / 2];
#pragma unroll
  for (int p = 0; p < NT * (NT + 1) / 2; ++p) acc[p] = d4{0.0, 0.0, 0.0, 0.0};
  double esig = 0.0, el = 0.0, csum = 0.0, som = 0.0;

  for (int step = 0; step * 64 < rows; ++step) {
    __syncthreads();   // the staging above / the previous step's reads of xs, the vectors and wt
    for (int q = tid; q < d * 64; q += 256) {
      const int c = q >> 6, i = q & 63;
      const int row = step * 64 + i;
      xs[q] = row < rows ? a.X[(int64_t)c * a.ldx + row0 + row] : 0.0;
    }
    if (tid < 64) {
      const int row = step * 64 + tid;
      rs[tid] = row < rows ? a.y[row0 + row] - a.mu[row0 + row] : 0.0;
    }
    __syncthreads();

    SGP_BF_ROWS_K()
    d4 qa[NT], qb[NT];
#pragma unroll
    for (int cb = 0; cb < NT; ++cb) qa[cb] = qb[cb] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < SN; ++s)
#pragma unroll
      for (int cb = 0; cb < NT; ++cb) {
        qa[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa_s[(4 * s + g) * Mp + 16 * cb + r16],
                                                      kf[s], qa[cb], 0, 0, 0);
        qb[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(pb_s[(4 * s + g) * Mp + 16 * cb + r16],
                                                      kf[s], qb[cb], 0, 0, 0);
      }
    double ku = 0.0;
#pragma unroll
    for (int s = 0; s < SN; ++s) ku = fma(kf[s], u_s[g * SN + s], ku);
    ku += __shfl_xor(ku, 16, 64);
    ku += __shfl_xor(ku, 32, 64);
    const double z = c0 - row_dot<NT>(qa, kf);   // pass 1's bits
    const double pi = row_dot<NT>(qb, kf);
    const double wi = iv ? 1.0 / z : 0.0;
    const double al = wi * (rs[wv * 16 + r16] - ku);
    const double om = al * al - (wi - wi * wi * pi);
    if (g == 0) {
      som += om;
      om_s[wv * 16 + r16] = om;
    }
    double w[SN];
#pragma unroll
    for (int cb = 0; cb < NT; ++cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = 4 * cb + r;
        // G = alpha u^T - w K Bm^-1 - omega K A
        const double gv = fma(al, u_s[g * SN + s], -fma(wi, qb[cb][r], om * qa[cb][r]));
        w[s] = gv * kf[s];
        esig += w[s];
        if (!ARD) el = fma(w[s], e2[s], el);
        // quirk Q5: the tau derivative of a pair whose raw differences are all zero
        if (e2[s] == 0.0 && iv && 4 * s + g < m) csum += gv;
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
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (g == 0) el_s[(c * 4 + wv) * 16 + r16] += v;   // the lane's own slot
      }
#pragma unroll
    for (int s = 0; s < SN; ++s) wt[r16 * FXS + 4 * s + g] = kf[s];
    __syncthreads();   // the k tile and omega are read across the wave's lanes
    // S_omega[16 bi + i][16 bj + j] += sum over the wave's 16 rows: A[i][row] = omega k,
    // B[row][j] = k: omega takes both signs, so only one operand carries it
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = 4 * q + g;
      const double oi = om_s[wv * 16 + i];
      double k1[NT], ko[NT];
#pragma unroll
      for (int b = 0; b < NT; ++b) {
        k1[b] = wt[i * FXS + 16 * b + r16];
        ko[b] = k1[b] * oi;
      }
      int p = 0;
#pragma unroll
      for (int bi = 0; bi < NT; ++bi)
#pragma unroll
        for (int bj = bi; bj < NT; ++bj, ++p)
          acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(ko[bi], k1[bj], acc[p], 0, 0, 0);
    }
  }

  store_pairs<NT>(acc, pa_s, rec);   // over A, which is dead
  const double e0 = block_sum(esig, red);
  const double e1 = block_sum(csum, red);
  const double e2s = block_sum(som, red);
  const int L = ARD ? d : 1;
  if (ARD) {
    __syncthreads();
    if (tid < d) {
      double v = 0.0;
      for (int q = 0; q < 64; ++q) v += el_s[tid * 64 + q];   // wave, then row lane
      rec[BQ_W + 1 + tid] = v;
    }
  } else {
    const double e3 = block_sum(el, red);
    if (tid == 0) rec[BQ_W + 1] = e3;
  }
  if (tid == 0) {
    rec[BQ_W] = e0;
    rec[BQ_W + 1 + L] = e1;
    rec[BQ_W + 2 + L] = e2s;
  }
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
#define SGP_BF_CASE(NT) \
  bf_pass2_body<NT, ARD>(a, P, fw, row0, rows, rec, xu_s, pa_s, pb_s, vec_s, xs, wt_s, red, el_s); \
  break;
  switch (((int)P[BP_M] + 15) >> 4) {
    case 1: SGP_BF_CASE(1)
    case 2: SGP_BF_CASE(2)
    case 3: SGP_BF_CASE(3)
    default: SGP_BF_CASE(4)
  }
#undef SGP_BF_CASE
}

// ------------------------------------------------------------------------------ G22 and finish
// G22 = -1/2 u u^T + 1/2 (K22^-1 - Bm^-1) + 1/2 K22^-1 S_omega K22^-1, contracted with
// dK22 / dlog theta (sigma: 2 Kuu; l: Kuu |D|^2 / l^2; l_c: Kuu (D_c / l_c)^2; tau: none,
// laplace_approx_gradient.R:899-902), then dlogp_dcov_par's gradient from the segments' sums
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
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    A[i * MM + j] = fw[BF_A + i * MM + j];
    Bi[i * MM + j] = fw[BF_B + i * MM + j];
    S[i * MM + j] = rec_sum(rec + i * MM + j, BATCH_REC4, nseg);
  }
  if (tid < m) u_s[tid] = fw[BF_U + tid];
  if (tid < L + 3) r2[tid] = rec_sum(rec + BQ_W + tid, BATCH_REC4, nseg);
  __syncthreads();
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s = fma(A[i * MM + k], S[k * MM + j], s);
    T[i * MM + j] = s;
  }
  __syncthreads();
  for (int e = tid; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s = fma(T[i * MM + k], A[k * MM + j], s);
    const double gv = -0.5 * u_s[i] * u_s[j] + 0.5 * (A[i * MM + j] - Bi[i * MM + j]) + 0.5 * s;
    const double kuu = sig2 * sgp_exp_nonpos(-0.5 * knot_dist2(P, d, i, j));
    S[i * MM + j] = gv * kuu;   // H: S is dead once T stands
  }
  __syncthreads();
  double h = 0.0;
  for (int e = tid; e < m * MM; e += 256)
    if ((e & (MM - 1)) < m) h += S[e];
  const double hs = block_sum(h, red);
  if (tid == 0) g22[0] = 2.0 * hs;
  if (a.ard) {
    for (int c = 0; c < d; ++c) {
      double v = 0.0;
      for (int e = tid; e < m * MM; e += 256) {
        const int i = e >> 6, j = e & (MM - 1);
        if (j >= m) continue;
        const double t = (P[BP_U + c * MM + i] - P[BP_U + c * MM + j]) * P[BP_RL + c];
        v = fma(S[i * MM + j], t * t, v);
      }
      const double vs = block_sum(v, red);
      if (tid == 0) g22[1 + c] = vs;
    }
  } else {
    double v = 0.0;
    for (int e = tid; e < m * MM; e += 256) {
      const int i = e >> 6, j = e & (MM - 1);
      if (j >= m) continue;
      v = fma(S[i * MM + j], knot_dist2(P, d, i, j), v);
    }
    const double vs = block_sum(v, red);
    if (tid == 0) g22[1] = vs;
  }
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
