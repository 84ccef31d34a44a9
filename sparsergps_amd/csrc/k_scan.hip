// The cheap knot proposals' scan over the context's resident rows (sgp_fit_scan; DESIGN.md
// sec. 0k): knot_prop_var / knot_prop_error (R/knot_proposal_functions.R:4-42) predict at every
// training row with predict_laplace, full_cov = FALSE (R/laplace_approx_prediction.R:3-123), and
// take the row of the largest variance, or of the largest |exp(f) - exp(mean)|:
//   mean_i = mu_i + k_i^T w,                  w = K22^-1 (u_mean - muu)
//   var_i  = sigma^2 + tau^2 - k_i^T A k_i,   A = K22^-1 - K22^-1 u_var K22^-1
// with k_i the cross covariance of row i and the m <= 128 knots (no nugget).  The pass has the
// shape of k_ego_scan (k_ego.hip): a workgroup of four waves takes 64 rows per step; each wave
// forms its 16 x mp block of k in registers in the operand layout of v_mfma_f64_16x16x4_f64
// (lane l: row l & 15, knots 4 s + (l >> 4)), multiplies it against A on the matrix cores as
// P = A K^T (mp x 16) and contracts P with the same registers (the result layout -- lane l: data
// row l & 15, knots 16 cb + (l >> 4) + 4 r -- meets k's operand layout at s = 4 cb + r).  Two
// cross-lane adds finish k^T A k and k^T w; the 16 lanes of group 0 form mean, var and the key,
// test the row against the sorted exclusion list and keep a running (key, row) maximum.  Beyond
// k_ego_scan: per-coordinate scales 1 / l_c ("ard") staged in LDS beside the knots, a per-row mu,
// a per-row f in error mode, and the two keys.  Every sum has a fixed order and the maximum is
// taken under a total order (sgp_argmax.h), so the result is bit-identical on repeat and
// independent of the grid.  No atomics.
#include <math.h>

#include "sgp_argmax.h"
#include "sgp_internal.h"

namespace {

constexpr int SCAN_ROWS = 64;   // rows per workgroup step: 4 waves x 16

// NT = mp / 16 column blocks of the padded knot set; ALDS: A staged in LDS (else read through
// L1 / L2 from its 128 x 128 home)
template <int NT, bool ALDS>
__global__ void __launch_bounds__(256) k_fit_scan(FitScan a, int ntiles) {
  constexpr int Mp = 16 * NT, SN = 4 * NT;
  extern __shared__ __attribute__((aligned(16))) double scan_lds[];
  const int d = a.d;
  double* xu_s = scan_lds;            // [c][g][s]: knot 4 s + g, coordinate c
  double* w_s = xu_s + d * Mp;        // [g][s]
  double* xs = w_s + Mp;              // [c][64]: this step's rows
  double* red = xs + d * SCAN_ROWS;   // 8
  double* rl_s = red + 8;             // d scales, padded to an even count
  double* A_s = rl_s + ((d + 1) & ~1);   // Mp x Mp (ALDS)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, g = lane >> 4;

  for (int q = tid; q < d * Mp; q += 256) {
    const int c = q / Mp, j = q - c * Mp;
    xu_s[(c * 4 + (j & 3)) * SN + (j >> 2)] = a.xu[c * SGP_EGO_TMAX + j];
  }
  for (int q = tid; q < Mp; q += 256) w_s[(q & 3) * SN + (q >> 2)] = a.w[q];
  for (int q = tid; q < d; q += 256) rl_s[q] = a.rl[q];
  if (ALDS)
    for (int q = tid; q < Mp * Mp; q += 256) {
      const int j = q / Mp;
      A_s[q] = a.A[j * SGP_EGO_TMAX + (q - j * Mp)];
    }

  double bkey = -INFINITY, brow = -1.0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = (int64_t)tile * SCAN_ROWS;
    __syncthreads();   // the staging above / the previous step's reads of xs
    for (int q = tid; q < d * (SCAN_ROWS / 2); q += 256) {
      const int c = q >> 5, p = q & 31;
      const double2 v = *reinterpret_cast<const double2*>(a.X + (int64_t)c * a.ldx + row0 + 2 * p);
      *reinterpret_cast<double2*>(xs + c * SCAN_ROWS + 2 * p) = v;
    }
    __syncthreads();

    const double* xr = xs + wv * 16 + r16;
    double kf[SN];
#pragma unroll
    for (int s = 0; s < SN; ++s) kf[s] = 0.0;
    for (int c = 0; c < d; ++c) {
      const double xc = xr[c * SCAN_ROWS], rl = rl_s[c];
      const double* u = xu_s + (c * 4 + g) * SN;
#pragma unroll
      for (int s = 0; s < SN; ++s) {
        const double t = (xc - u[s]) * rl;   // the raw difference first: coincidence stays exact
        kf[s] = fma(t, t, kf[s]);
      }
    }
    double pm = 0.0;
#pragma unroll
    for (int s = 0; s < SN; ++s) {
      const double v = a.sig2 * sgp_exp_nonpos(a.coef * kf[s]);
      kf[s] = (4 * s + g < a.m) ? v : 0.0;
      pm = fma(kf[s], w_s[g * SN + s], pm);
    }

    d4 acc[NT];
#pragma unroll
    for (int cb = 0; cb < NT; ++cb) acc[cb] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < SN; ++s) {
#pragma unroll
      for (int cb = 0; cb < NT; ++cb) {
        // A[16 cb + r16][4 s + g] read as its transpose's entry: k^T A k = k^T A^T k
        const double af = ALDS ? A_s[(4 * s + g) * Mp + 16 * cb + r16]
                               : a.A[(4 * s + g) * SGP_EGO_TMAX + 16 * cb + r16];
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
      const double mean = a.mu[row] + pm;
      const double var = a.c0 - qf;
      // R/knot_proposal_functions.R:38: abs(exp(f) - exp(pred_mean)), for every family
      const double kv = a.mode ? fabs(exp(a.f[row]) - exp(mean)) : var;
      const bool excluded = ego_excluded(a.ex, a.E, d, xr, SCAN_ROWS);
      if (a.mean_out) a.mean_out[row] = mean;
      if (a.var_out) a.var_out[row] = var;
      if (a.key_out) a.key_out[row] = excluded ? (double)NAN : kv;
      if (!excluded) {
        const double key = kv == kv ? kv : -INFINITY;   // a NaN never wins
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

// out = [best key (NaN when the winner's key is), its row or -1, the K22 chain's status]
__global__ void __launch_bounds__(256) k_fit_scan_final(const double* __restrict__ rec, int nblk,
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
hipError_t scan_launch_nt(const FitScan& a, int ntiles, int grid, hipStream_t s) {
  constexpr int Mp = 16 * NT;
  const size_t base =
      sizeof(double) * (size_t)(a.d * Mp + Mp + a.d * SCAN_ROWS + 8 + ((a.d + 1) & ~1));
  const size_t with_a = base + sizeof(double) * Mp * Mp;
  if (with_a <= 64 * 1024)
    hipLaunchKernelGGL((k_fit_scan<NT, true>), dim3(grid), dim3(256), with_a, s, a, ntiles);
  else
    hipLaunchKernelGGL((k_fit_scan<NT, false>), dim3(grid), dim3(256), base, s, a, ntiles);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_fit_scan(const FitScan& a, int max_blocks, const int* status, double* out,
                           hipStream_t s) {
  if (a.m < 1 || a.m > SGP_EGO_TMAX || a.d < 1 || a.d > SGP_MAXD || a.n < 1 || max_blocks < 1 ||
      (a.mode != 0 && a.mode != 1) ||
      (a.mode && !a.f) || !a.mu || !a.rl)
    return hipErrorInvalidValue;
  const int64_t nt64 = (a.n + SCAN_ROWS - 1) / SCAN_ROWS;
  if (nt64 > INT32_MAX) return hipErrorInvalidValue;
  const int ntiles = (int)nt64;
  const int grid = ntiles < max_blocks ? ntiles : max_blocks;
  const int nt = (a.m + 15) / 16;
  hipError_t e;
  if (nt <= 1) e = scan_launch_nt<1>(a, ntiles, grid, s);
  else if (nt == 2) e = scan_launch_nt<2>(a, ntiles, grid, s);
  else if (nt == 3) e = scan_launch_nt<3>(a, ntiles, grid, s);
  else if (nt == 4) e = scan_launch_nt<4>(a, ntiles, grid, s);
  else if (nt <= 6) e = scan_launch_nt<6>(a, ntiles, grid, s);
  else e = scan_launch_nt<8>(a, ntiles, grid, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_fit_scan_final, dim3(1), dim3(256), 0, s, a.rec, grid, status, out);
  return hipGetLastError();
}
