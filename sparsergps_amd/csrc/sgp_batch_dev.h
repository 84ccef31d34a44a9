// Device code shared by the batch kernels (k_batch.hip, k_batch_fitc.hip, k_batch_laplace.hip).
// Every piece that more than one of them needs is defined here, once:
//   sums        block_sum, rec_sum, fold_groups, wave_sum4: the fixed-order sums
//   dispatch    SGP_BATCH_NT: a row-pass body by the problem's count of 16-knot blocks
//   m x m       for_mm (the thread-to-entry map of every m x m loop), sweep_spd, knot_dist2, kuu,
//               k22, k22_inverse, dot_mm, mat_vec_row, sandwich, contract_h, store_post
//   row passes  the staging (stage_knots, stage_vec, stage_mat, stage_x), the rows' covariances
//               (rows_k) and their MFMA product with an LDS operand (kmat), the per-row dots
//               (row_dot, k_dot), the transposition and the two rank updates (put_ktile,
//               rank_update_root, rank_update_signed, store_pairs), the objective passes' tail
//               (fold_tacc, pass1_tail) and the gradient passes' W = G o K sums (grad_terms,
//               grad_tail)
// The files keep their kernels, their row terms and their expression for G.  A kernel's bits
// follow from the order of the operations written here, so a change to a piece changes every
// kernel that uses it in the same way; the same source inlined into two kernels is still not
// guaranteed the same fma contraction, which tests/test_gpu_batch_bits.py watches.
// Internal linkage: each translation unit compiles its own copy.
#pragma once
#include <math.h>

#include "sgp_internal.h"

namespace {

constexpr int MM = SGP_BATCH_MMAX;   // 64: the LDS matrices' row stride
constexpr int FXS = 68;              // the wave-private k tile's row stride (doubles)

// A row-pass body by NT = the problem's count of 16-knot blocks: the statement sees NT as a
// constant, SGP_BATCH_NT(P[BP_M], body<NT>(...)).  The macro declares NT; the argument is one
// statement (an if / else counts) without its final `;`, and the call takes none either.  Commas
// in template arguments are safe: the arguments are rejoined.
#define SGP_BATCH_NT(M, ...)                                \
  switch (((int)(M) + 15) >> 4) {                           \
    case 1: { constexpr int NT = 1; __VA_ARGS__; } break;   \
    case 2: { constexpr int NT = 2; __VA_ARGS__; } break;   \
    case 3: { constexpr int NT = 3; __VA_ARGS__; } break;   \
    default: { constexpr int NT = 4; __VA_ARGS__; } break;  \
  }

// ------------------------------------------------------------------------------ sums
// sum of v over the 256 threads in a fixed tree order; red: 256 doubles
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  return red[0];
}

// sum of rec[q * stride], q = 0 .. n - 1, in that order; the loads go out eight at a time
__device__ __forceinline__ double rec_sum(const double* __restrict__ rec, int64_t stride, int n) {
  double s = 0.0;
  int q = 0;
  for (; q + 8 <= n; q += 8) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = rec[(q + k) * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  for (; q < n; ++q) s += rec[q * stride];
  return s;
}

// v summed over the four lane groups of a row (lanes l, l ^ 16, l ^ 32, l ^ 48): every lane of the
// row ends with the same bits
__device__ __forceinline__ double fold_groups(double v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// the four waves' entries j of tw (row stride 64), in wave order
__device__ __forceinline__ double wave_sum4(const double* tw, int j) {
  return ((tw[j] + tw[MM + j]) + tw[2 * MM + j]) + tw[3 * MM + j];
}

// ------------------------------------------------------------------------------ m x m stages
// f(i, j) over the leading m x m of a matrix of row stride 64: thread t takes the entries
// e = t, t + 256, ... of the row-major m x 64, in that order
template <class F>
__device__ __forceinline__ void for_mm(int m, F f) {
  for (int e = threadIdx.x; e < m * MM; e += 256) {
    const int i = e >> 6, j = e & (MM - 1);
    if (j >= m) continue;
    f(i, j);
  }
}

// The sweep operator on the leading m x m of A (row stride 64, in LDS): after the m sweeps A holds
// -A^-1.  On an SPD matrix the pivot of sweep k is the ratio of the leading minors of order k + 1
// and k (the square of Cholesky's k-th diagonal), so the first pivot that is not positive gives
// chol()'s "leading minor of order k + 1".  Returns 0 or that order; *ld = the log-determinant.
__device__ int sweep_spd(double* A, int m, double* ck, double* ld) {
  const int tid = threadIdx.x;
  double l = 0.0;
  for (int k = 0; k < m; ++k) {
    __syncthreads();
    const double dk = A[k * MM + k];
    if (!(dk > 0.0)) return k + 1;
    l += log(dk);
    if (tid < m) ck[tid] = A[tid * MM + k];   // = row k: A stays symmetric
    __syncthreads();
    const double rd = 1.0 / dk;
    for_mm(m, [&](int i, int j) {
      double v;
      if (i == k) v = j == k ? -rd : ck[j] * rd;
      else if (j == k) v = ck[i] * rd;
      else v = A[i * MM + j] - ck[i] * (ck[j] * rd);
      A[i * MM + j] = v;
    });
  }
  __syncthreads();
  for_mm(m, [&](int i, int j) { A[i * MM + j] = -A[i * MM + j]; });
  __syncthreads();
  *ld = l;
  return 0;
}

// (U_i - U_j) scaled, squared and summed: the exponent's -2 x
__device__ __forceinline__ double knot_dist2(const double* __restrict__ P, int d, int i, int j) {
  double s = 0.0;
  for (int c = 0; c < d; ++c) {
    const double t = (P[BP_U + c * MM + i] - P[BP_U + c * MM + j]) * P[BP_RL + c];
    s = fma(t, t, s);
  }
  return s;
}

// Kuu's entry (i, j), and K22's: Kuu plus diag on the diagonal
__device__ __forceinline__ double kuu(const double* __restrict__ P, int d, int i, int j,
                                      double sig2) {
  return sig2 * sgp_exp_nonpos(-0.5 * knot_dist2(P, d, i, j));
}
__device__ __forceinline__ double k22(const double* __restrict__ P, int d, int i, int j,
                                      double sig2, double diag) {
  return kuu(P, d, i, j, sig2) + (i == j ? diag : 0.0);
}

// A = K22^-1 in LDS and *ld = log|K22|; returns sweep_spd's status
__device__ __forceinline__ int k22_inverse(const double* __restrict__ P, int d, double diag,
                                           double* A, double* ck, double* ld) {
  const int m = (int)P[BP_M];
  const double sig2 = P[BP_SIG2];
  for_mm(m, [&](int i, int j) { A[i * MM + j] = k22(P, d, i, j, sig2, diag); });
  return sweep_spd(A, m, ck, ld);
}

// sum_k L[i][k] R[k][j] and sum_k M[i][k] v[k], k = 0 .. m - 1 in that order (row stride 64)
__device__ __forceinline__ double dot_mm(const double* L, const double* R, int i, int j, int m) {
  double s = 0.0;
  for (int k = 0; k < m; ++k) s = fma(L[i * MM + k], R[k * MM + j], s);
  return s;
}
__device__ __forceinline__ double mat_vec_row(const double* __restrict__ M, const double* v_s,
                                              int i, int m) {
  double s = 0.0;
  for (int k = 0; k < m; ++k) s = fma(M[i * MM + k], v_s[k], s);
  return s;
}

// T = A S, the first half of A S A, and the barrier; the second half, dot_mm(T, A, i, j, m),
// stays fused with each kernel's own use of it
__device__ __forceinline__ void sandwich(const double* A, const double* S, double* T, int m) {
  for_mm(m, [&](int i, int j) { T[i * MM + j] = dot_mm(A, S, i, j, m); });
  __syncthreads();
}

// H = G22 o Kuu (in LDS) contracted with dK22 / dlog theta: out[0] = 2 sum H (sigma), then
// sum H |D|^2 / l^2 (out[1]) or, with ard, sum H (D_c / l_c)^2 (out[1 + c]); one block_sum per
// value, written by thread 0
__device__ __forceinline__ void contract_h(const double* __restrict__ P, int d, int m, int ard,
                                           const double* H, double* red, double* out) {
  const int tid = threadIdx.x;
  double h = 0.0;
  for_mm(m, [&](int i, int j) { h += H[i * MM + j]; });
  const double hs = block_sum(h, red);
  if (tid == 0) out[0] = 2.0 * hs;
  if (ard) {
    for (int c = 0; c < d; ++c) {
      double v = 0.0;
      for_mm(m, [&](int i, int j) {
        const double t = (P[BP_U + c * MM + i] - P[BP_U + c * MM + j]) * P[BP_RL + c];
        v = fma(H[i * MM + j], t * t, v);
      });
      const double vs = block_sum(v, red);
      if (tid == 0) out[1 + c] = vs;
    }
  } else {
    double v = 0.0;
    for_mm(m, [&](int i, int j) { v = fma(H[i * MM + j], knot_dist2(P, d, i, j), v); });
    const double vs = block_sum(v, red);
    if (tid == 0) out[1] = vs;
  }
}

// what sgp_batch_posterior_u and sgp_batch_predict need: the inverse (row stride 64), the m-vector
// and the problem's parameters and knots
__device__ __forceinline__ void store_post(const BatchArgs& a, int prob,
                                           const double* __restrict__ P, const double* Bi,
                                           const double* u, int m) {
  const int tid = threadIdx.x;
  double* post = a.post + (int64_t)prob * a.post_stride;
  for_mm(m, [&](int i, int j) { post[i * MM + j] = Bi[i * MM + j]; });
  if (tid < m) post[MM * MM + tid] = u[tid];
  for (int q = tid; q < a.pst; q += 256) post[MM * MM + MM + q] = P[q];
}

// ------------------------------------------------------------------------------ row passes: staging
// A workgroup of four waves takes 64 rows per step; lane l of a wave is on row r16 = l & 15 of the
// wave's 16 and on knots 4 s + g, g = l >> 4 (k_fit_scan's operand layout of
// v_mfma_f64_16x16x4_f64).  An m-vector in that layout is v_s[g * SN + s] = v[4 s + g].

// the knots ([c][g][s]) and the reciprocal length scales
__device__ __forceinline__ void stage_knots(const double* __restrict__ P, int d, int Mp, int SN,
                                            double* xu_s, double* rl_s) {
  const int tid = threadIdx.x;
  for (int q = tid; q < d * Mp; q += 256) {
    const int c = q / Mp, j = q - c * Mp;
    xu_s[(c * 4 + (j & 3)) * SN + (j >> 2)] = P[BP_U + c * MM + j];
  }
  for (int q = tid; q < d; q += 256) rl_s[q] = P[BP_RL + q];
}
__device__ __forceinline__ void stage_vec(const double* __restrict__ src, int m, int Mp, int SN,
                                          double* v_s) {
  for (int q = threadIdx.x; q < Mp; q += 256) v_s[(q & 3) * SN + (q >> 2)] = q < m ? src[q] : 0.0;
}
// the leading m x m of src (row stride 64) as an Mp x Mp MFMA operand, zero beyond m
__device__ __forceinline__ void stage_mat(const double* __restrict__ src, int m, int Mp,
                                          double* p_s) {
  for (int q = threadIdx.x; q < Mp * Mp; q += 256) {
    const int i = q / Mp, j = q - i * Mp;
    p_s[q] = (i < m && j < m) ? src[i * MM + j] : 0.0;
  }
}
// the step's rows of X (column stride ldx) as xs[c * xst + row], zero beyond the segment
__device__ __forceinline__ void stage_x(const double* __restrict__ X, int64_t ldx, int64_t row0,
                                        int rows, int step, int d, double* xs, int xst = 64) {
  for (int q = threadIdx.x; q < d * 64; q += 256) {
    const int c = q >> 6, i = q & 63;
    const int row = step * 64 + i;
    xs[c * xst + i] = row < rows ? X[(int64_t)c * ldx + row0 + row] : 0.0;
  }
}

// ------------------------------------------------------------------------------ row passes: k
// k of the step's rows: e2[s] the scaled squared distance of the lane's row and knot 4 s + g,
// kf[s] the covariance (zero beyond the rows and the knots); returns whether the row exists
template <int SN>
__device__ __forceinline__ bool rows_k(const double* xs, const double* xu_s, const double* rl_s,
                                       int d, int m, double sig2, int rows, int step, double* e2,
                                       double* kf, int xst = 64) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  const bool iv = step * 64 + wv * 16 + r16 < rows;
  const double* xr = xs + wv * 16 + r16;
#pragma unroll
  for (int s = 0; s < SN; ++s) e2[s] = 0.0;
  for (int c = 0; c < d; ++c) {
    const double xc = xr[c * xst], rl = rl_s[c];
    const double* u = xu_s + (c * 4 + g) * SN;
#pragma unroll
    for (int s = 0; s < SN; ++s) {
      const double t = (xc - u[s]) * rl;   // the raw difference first: coincidence stays exact
      e2[s] = fma(t, t, e2[s]);
    }
  }
#pragma unroll
  for (int s = 0; s < SN; ++s) {
    const double v = sig2 * sgp_exp_nonpos(-0.5 * e2[s]);
    kf[s] = (iv && 4 * s + g < m) ? v : 0.0;
  }
  return iv;
}

// acc = K P for the wave's 16 x Mp tile of k and the Mp x Mp operand p_s in LDS; the result
// layout meets k's again: acc[cb][r] belongs to knot 4 (4 cb + r) + g
template <int NT>
__device__ __forceinline__ void kmat(const double* p_s, const double* kf, d4* acc) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int cb = 0; cb < NT; ++cb) acc[cb] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < SN; ++s)
#pragma unroll
    for (int cb = 0; cb < NT; ++cb)
      acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(p_s[(4 * s + g) * Mp + 16 * cb + r16], kf[s],
                                                     acc[cb], 0, 0, 0);
}
// the same for two operands, their MFMAs issued alternately
template <int NT>
__device__ __forceinline__ void kmat2(const double* pa_s, const double* pb_s, const double* kf,
                                      d4* qa, d4* qb) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int cb = 0; cb < NT; ++cb) qa[cb] = qb[cb] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < SN; ++s)
#pragma unroll
    for (int cb = 0; cb < NT; ++cb) {
      qa[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa_s[(4 * s + g) * Mp + 16 * cb + r16], kf[s],
                                                    qa[cb], 0, 0, 0);
      qb[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(pb_s[(4 * s + g) * Mp + 16 * cb + r16], kf[s],
                                                    qb[cb], 0, 0, 0);
    }
}

// sum over the lane's knots of acc o k, then over the four lane groups
template <int NT>
__device__ __forceinline__ double row_dot(const d4* acc, const double* kf) {
  double v = 0.0;
#pragma unroll
  for (int cb = 0; cb < NT; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) v = fma(acc[cb][r], kf[4 * cb + r], v);
  return fold_groups(v);
}

// k_i^T v for a vector staged by stage_vec
template <int SN>
__device__ __forceinline__ double k_dot(const double* kf, const double* v_s, int g) {
  double v = 0.0;
#pragma unroll
  for (int s = 0; s < SN; ++s) v = fma(kf[s], v_s[g * SN + s], v);
  return fold_groups(v);
}

// ------------------------------------------------------------------------------ row passes: rank updates
// Each wave turns its 16 x Mp tile of k through wave-private LDS (wt, row stride FXS) into the
// layout with the knot on l & 15 and rows 4 q + (l >> 4), in which k is both operands of
// S += sum_i w_i k_i k_i^T; only the NT (NT + 1) / 2 block pairs bi <= bj are formed.
template <int SN>
__device__ __forceinline__ void put_ktile(double* wt, const double* kf) {
  const int lane = threadIdx.x & 63, r16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int s = 0; s < SN; ++s) wt[r16 * FXS + 4 * s + g] = kf[s];
}

// S[16 bi + i][16 bj + j] += sum over the wave's 16 rows: A[i][row] = B[row][j] = sw k, for a
// positive weight whose root is sw_s[row]; with TV also tacc[b] += k wr_s[row]
template <int NT, bool TV>
__device__ __forceinline__ void rank_update_root(const double* wt, const double* sw_s,
                                                 const double* wr_s, d4* acc, double* tacc) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = 4 * q + g;
    const double sq = sw_s[wv * 16 + i], wr = TV ? wr_s[wv * 16 + i] : 0.0;
    double kw[NT];
#pragma unroll
    for (int b = 0; b < NT; ++b) {
      const double k1 = wt[i * FXS + 16 * b + r16];
      if (TV) tacc[b] = fma(k1, wr, tacc[b]);
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

// the same with A[i][row] = o k, B[row][j] = k: the weight o_s[row] takes both signs, so only one
// operand carries it
template <int NT>
__device__ __forceinline__ void rank_update_signed(const double* wt, const double* o_s, d4* acc) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = 4 * q + g;
    const double oi = o_s[wv * 16 + i];
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

// ------------------------------------------------------------------------------ row passes: tails
// K^T v of a wave's rows: tacc[b] (knot 16 b + r16, the lane's rows) over the four lane groups
// into tw[wave][knot]
template <int NT>
__device__ __forceinline__ void fold_tacc(const double* tacc, double* tw) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int b = 0; b < NT; ++b) {
    const double t = fold_groups(tacc[b]);
    if (g == 0) tw[wv * MM + 16 * b + r16] = t;
  }
}

// an objective pass's record beside S: rec[BR_T ...] = K^T v, the waves in wave order, and
// rec[BR_RR + q] = the sum of r_q, q < 3, over the 64 row lanes (wave, then lane); red: 3 x 64
template <int NT>
__device__ __forceinline__ void pass1_tail(const double* tacc, double r0, double r1, double r2,
                                           double* tw, double* red, double* __restrict__ rec) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;
  fold_tacc<NT>(tacc, tw);
  if (g == 0) {
    red[wv * 16 + r16] = r0;
    red[MM + wv * 16 + r16] = r1;
    red[2 * MM + wv * 16 + r16] = r2;
  }
  __syncthreads();
  if (tid < 16 * NT) rec[BR_T + tid] = wave_sum4(tw, tid);
  if (tid < 3) {
    double v = 0.0;
    for (int q = 0; q < 64; ++q) v += red[tid * MM + q];
    rec[BR_RR + tid] = v;
  }
}

// A gradient pass's sums of W = G o K over the lane's entries, G_{row, 4 s + g} = gvf(cb, r, s)
// with s = 4 cb + r: esig += W, el += W e2 (sqexp) or el_s[c][wave][row lane] += the row's
// sum of W (D_c / l_c)^2 (ARD: the lane groups folded by shuffles first, so the d running sums
// take 16 KiB), csum += G where the raw differences are all zero (quirk Q5: the tau derivative)
template <int NT, bool ARD, class GV>
__device__ __forceinline__ void grad_terms(GV gvf, const double* kf, const double* e2, bool iv,
                                           int m, int d, const double* xs, const double* xu_s,
                                           const double* rl_s, double* el_s, double& esig,
                                           double& el, double& csum) {
  constexpr int SN = 4 * NT;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  double w[SN];
#pragma unroll
  for (int cb = 0; cb < NT; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int s = 4 * cb + r;
      const double gv = gvf(cb, r, s);
      w[s] = gv * kf[s];
      esig += w[s];
      if (!ARD) el = fma(w[s], e2[s], el);
      if (e2[s] == 0.0 && iv && 4 * s + g < m) csum += gv;
    }
  if (ARD) {
    const double* xr = xs + wv * 16 + r16;
    for (int c = 0; c < d; ++c) {
      const double xc = xr[c * 64], rl = rl_s[c];
      const double* u = xu_s + (c * 4 + g) * SN;
      double v = 0.0;
#pragma unroll
      for (int s = 0; s < SN; ++s) {
        const double t = (xc - u[s]) * rl;
        v = fma(w[s], t * t, v);
      }
      v = fold_groups(v);
      if (g == 0) el_s[(c * 4 + wv) * 16 + r16] += v;   // the lane's own slot
    }
  }
}

// the segment's record of those sums: rec[BQ_W] = sum W, then the L length-scale sums, the
// coincident sum and the sum of the rows' weights som
template <bool ARD>
__device__ __forceinline__ void grad_tail(double esig, double el, double csum, double som, int d,
                                          double* red, const double* el_s,
                                          double* __restrict__ rec) {
  const int tid = threadIdx.x;
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

}  // namespace
