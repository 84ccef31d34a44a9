// EGO knot proposal: the expected-improvement scan over the context's resident rows
// (sgp_ego_scan).
//
// The reference refits a small meta-model GP of the objective (T <= 128 points Xm with values v)
// and then, in an R loop over every data row, solves against its T x T covariance
// (R/vi_functions.R:1927-1950, 2074-2097; R/knot_proposal_functions.R:355-379, 457-478, 832-855,
// 964-985):
//   pred_i = v_1 + k_i^T alpha,            alpha = K22^-1 (v - v_1)
//   var_i  = sigma^2 + tau^2 - k_i^T A k_i,    A = K22^-1
//   EI_i   = sqrt(var_i) (z Phi(z) + phi(z)),  z = (pred_i - max v) / sqrt(var_i)   if var_i > tau^2
//          = 0                                                                       otherwise
//   proposal = the row of xy_setminus_xu with the largest EI (which.max: first of equals)
// Here it is one pass over X.  A workgroup of four waves takes 64 rows per step; each wave forms
// its 16 x Tp block of k in registers, directly in the operand layout of v_mfma_f64_16x16x4_f64
// (lane l: row l & 15, meta points 4 s + (l >> 4)), multiplies it against A on the matrix cores as
// P = A K^T (Tp x 16), and contracts P with the same registers: the result layout (lane l: data
// row l & 15, meta points 16 cb + (l >> 4) + 4 r) meets k's operand layout at s = 4 cb + r, so the
// n x T matrix never leaves the register file.  Two cross-lane adds finish k^T A k and k^T alpha;
// the 16 lanes of group 0 then evaluate EI, test the row against the sorted exclusion list
// (binary search on coordinate 0, the other coordinates only on a hit) and keep a running
// (EI, row) maximum.  Every sum has a fixed order and the maximum is taken under a total order
// (larger EI, then lower row), so the result is bit-identical on repeat and independent of the
// grid.  No atomics.
#include <math.h>

#include "sgp_argmax.h"
#include "sgp_internal.h"

namespace {

constexpr int EGO_ROWS = 64;   // rows per workgroup step: 4 waves x 16

// NT = Tp / 16 column blocks of the padded meta-model; ALDS: A staged in LDS (else read through
// L1 / L2 from its 128 x 128 home)
template <int NT, bool ALDS>
__global__ void __launch_bounds__(256) k_ego_scan(EgoScan a, int ntiles) {
  constexpr int Tp = 16 * NT, SN = 4 * NT;
  extern __shared__ __attribute__((aligned(16))) double ego_lds[];
  const int d = a.d;
  double* xm_s = ego_lds;            // [c][g][s]: meta point 4 s + g, coordinate c
  double* al_s = xm_s + d * Tp;      // [g][s]
  double* xs = al_s + Tp;            // [c][64]: this step's rows
  double* red = xs + d * EGO_ROWS;   // 8
  double* A_s = red + 8;             // Tp x Tp (ALDS)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;

  for (int q = tid; q < d * Tp; q += 256) {
    const int c = q / Tp, j = q - c * Tp;
    xm_s[(c * 4 + (j & 3)) * SN + (j >> 2)] = a.xm[c * SGP_EGO_TMAX + j];
  }
  for (int q = tid; q < Tp; q += 256) al_s[(q & 3) * SN + (q >> 2)] = a.alpha[q];
  if (ALDS)
    for (int q = tid; q < Tp * Tp; q += 256) {
      const int j = q / Tp;
      A_s[q] = a.Ainv[j * SGP_EGO_TMAX + (q - j * Tp)];
    }

  double bkey = -INFINITY, brow = -1.0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = (int64_t)tile * EGO_ROWS;
    __syncthreads();   // the staging above / the previous step's reads of xs
    for (int q = tid; q < d * (EGO_ROWS / 2); q += 256) {
      const int c = q >> 5, p = q & 31;
      const double2 v = *reinterpret_cast<const double2*>(a.X + (int64_t)c * a.ldx + row0 + 2 * p);
      *reinterpret_cast<double2*>(xs + c * EGO_ROWS + 2 * p) = v;
    }
    __syncthreads();

    const double* xr = xs + wv * 16 + r16;
    double kf[SN];
#pragma unroll
    for (int s = 0; s < SN; ++s) kf[s] = 0.0;
    if (a.kexp) {
      for (int c = 0; c < d; ++c) {
        const double xc = xr[c * EGO_ROWS];
        const double* m = xm_s + (c * 4 + g) * SN;
#pragma unroll
        for (int s = 0; s < SN; ++s) kf[s] += fabs(xc - m[s]);
      }
    } else {
      for (int c = 0; c < d; ++c) {
        const double xc = xr[c * EGO_ROWS];
        const double* m = xm_s + (c * 4 + g) * SN;
#pragma unroll
        for (int s = 0; s < SN; ++s) {
          const double t = xc - m[s];
          kf[s] = fma(t, t, kf[s]);
        }
      }
    }
    double pm = 0.0;
#pragma unroll
    for (int s = 0; s < SN; ++s) {
      const double v = a.sig2 * sgp_exp_nonpos(a.coef * kf[s]);
      kf[s] = (4 * s + g < a.T) ? v : 0.0;
      pm = fma(kf[s], al_s[g * SN + s], pm);
    }

    d4 acc[NT];
#pragma unroll
    for (int cb = 0; cb < NT; ++cb) acc[cb] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < SN; ++s) {
#pragma unroll
      for (int cb = 0; cb < NT; ++cb) {
        // A[16 cb + r16][4 s + g] read as its transpose's entry: k^T A k = k^T A^T k
        const double af = ALDS ? A_s[(4 * s + g) * Tp + 16 * cb + r16]
                               : a.Ainv[(4 * s + g) * SGP_EGO_TMAX + 16 * cb + r16];
        acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, kf[s], acc[cb], 0, 0, 0);
      }
    }
    double qf = 0.0;
#pragma unroll
    for (int cb = 0; cb < NT; ++cb) {
      qf = fma(acc[cb][0], kf[4 * cb + 0], qf);
      qf = fma(acc[cb][1], kf[4 * cb + 1], qf);
      qf = fma(acc[cb][2], kf[4 * cb + 2], qf);
      qf = fma(acc[cb][3], kf[4 * cb + 3], qf);
    }
    qf += __shfl_xor(qf, 16, 64);
    qf += __shfl_xor(qf, 32, 64);
    pm += __shfl_xor(pm, 16, 64);
    pm += __shfl_xor(pm, 32, 64);

    const int64_t row = row0 + wv * 16 + r16;
    if (g == 0 && row < a.n) {
      const double mean = a.v1 + pm;
      const double var = a.c0 - qf;
      double ei = 0.0;
      if (var > a.tau2) {
        const double sd = sqrt(var);
        const double z = (mean - a.vmax) / sd;
        ei = sd * (z * (0.5 * erfc(-z * 0.70710678118654752440)) +
                   0.39894228040143267794 * exp(-0.5 * z * z));
      }
      const bool excluded = ego_excluded(a.ex, a.E, d, xr, EGO_ROWS);
      if (a.mean_out) a.mean_out[row] = mean;
      if (a.var_out) a.var_out[row] = var;
      if (a.ei_out) a.ei_out[row] = excluded ? (double)NAN : ei;
      if (!excluded) {
        const double key = ei == ei ? ei : -INFINITY;   // a NaN never wins
        if (brow < 0.0 || key > bkey) { bkey = key; brow = (double)row; }
      }
    }
  }
  __syncthreads();
  ego_block_max(bkey, brow, red);
  if (tid == 0) {
    a.rec[2 * blockIdx.x] = bkey;
    a.rec[2 * blockIdx.x + 1] = brow;
  }
}

// out = [best EI (NaN when the winner's EI is), its row or -1, the K22 chain's status]
__global__ void __launch_bounds__(256) k_ego_final(const double* __restrict__ rec, int nblk,
                                                   const int* __restrict__ status,
                                                   double* __restrict__ out) {
  __shared__ double red[8];
  double key = -INFINITY, row = -1.0;
  for (int q = threadIdx.x; q < nblk; q += 256)
    if (ego_better(rec[2 * q], rec[2 * q + 1], key, row)) { key = rec[2 * q]; row = rec[2 * q + 1]; }
  ego_block_max(key, row, red);
  if (threadIdx.x == 0) {
    out[0] = (row >= 0.0 && key == -INFINITY) ? (double)NAN : key;
    out[1] = row;
    out[2] = (double)status[0];
  }
}

template <int NT>
hipError_t ego_launch_nt(const EgoScan& a, int ntiles, int grid, hipStream_t s) {
  constexpr int Tp = 16 * NT;
  const size_t base = sizeof(double) * (size_t)(a.d * Tp + Tp + a.d * EGO_ROWS + 8);
  const size_t with_a = base + sizeof(double) * Tp * Tp;
  if (with_a <= 64 * 1024)
    hipLaunchKernelGGL((k_ego_scan<NT, true>), dim3(grid), dim3(256), with_a, s, a, ntiles);
  else
    hipLaunchKernelGGL((k_ego_scan<NT, false>), dim3(grid), dim3(256), base, s, a, ntiles);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_ego_scan(const EgoScan& a, int max_blocks, const int* status, double* out,
                           hipStream_t s) {
  if (a.T < 1 || a.T > SGP_EGO_TMAX || a.d < 1 || a.d > SGP_MAXD || a.n < 1 || max_blocks < 1)
    return hipErrorInvalidValue;
  const int64_t nt64 = (a.n + EGO_ROWS - 1) / EGO_ROWS;
  if (nt64 > INT32_MAX) return hipErrorInvalidValue;
  const int ntiles = (int)nt64;
  const int grid = ntiles < max_blocks ? ntiles : max_blocks;
  const int nt = (a.T + 15) / 16;
  hipError_t e;
  if (nt <= 1) e = ego_launch_nt<1>(a, ntiles, grid, s);
  else if (nt == 2) e = ego_launch_nt<2>(a, ntiles, grid, s);
  else if (nt == 3) e = ego_launch_nt<3>(a, ntiles, grid, s);
  else if (nt == 4) e = ego_launch_nt<4>(a, ntiles, grid, s);
  else if (nt <= 6) e = ego_launch_nt<6>(a, ntiles, grid, s);
  else e = ego_launch_nt<8>(a, ntiles, grid, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ego_final, dim3(1), dim3(256), 0, s, a.rec, grid, status, out);
  return hipGetLastError();
}
