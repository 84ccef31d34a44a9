// Held-out scoring (sgp_nlp, sgp_predict_nlp): the reference's my_nlp
// (R/evaluation_functions.R:12-145) over n test rows, one launch instead of one adaptive
// integrate() call per row.
//
// k_nlp_rows<FAM> reads y, pred_mean, pred_var (and a per-row exposure) and writes nlp[i] -- the
// arithmetic of sgp_quad.h, one row per lane (several lanes per row, each repeating the mode and
// level-set steps and sharing the rule's points, were measured and are slower from 1e5 rows up:
// profiles/nlp/README.md).  A workgroup of 256 threads takes a tile of 256 rows per step and
// leaves, per tile, four partials: the sum and the count of the finite nlp values, the count of
// NaN rows and sum (pred_mean - y)^2.
// The partials belong to tiles, not to workgroups, and k_nlp_final adds them in tile order in one
// block: results are bit-identical on repeat and independent of the grid.  No atomics.
//
// k_pred_finish forms pred_mean = mu_pred + y and pred_var = c0 + q on the device, the two sums
// sgp_predict forms on the host after its readback (one IEEE addition each: the same bits).
#include <math.h>

#include "sgp_internal.h"
#include "sgp_quad.h"

namespace {

constexpr int NLP_THREADS = 256;

// the sum over the 256 threads in a fixed order; valid in thread 0.  red: 4 doubles of LDS
__device__ __forceinline__ double nlp_block_sum(double v, double* red) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  const int wv = threadIdx.x >> 6;
  __syncthreads();   // the previous use of red
  if ((threadIdx.x & 63) == 0) red[wv] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <int FAM>
__global__ void __launch_bounds__(NLP_THREADS) k_nlp_rows(NlpArgs a, int ntiles) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row = (int64_t)tile * NLP_THREADS + tid;
    const bool live = row < a.n;
    // a lane past the end scores a harmless row, so that its wave's loops stay uniform
    const double y = live ? a.y[row] : (FAM == SGP_QUAD_GAUSSIAN ? 0.0 : 1.0);
    const double mu = live ? a.pm[row] : 0.0;
    const double s2 = live ? a.pv[row] : 1.0;
    double v;
    if (FAM == SGP_QUAD_GAUSSIAN) {
      v = quad_nlp_gaussian(y, mu, s2, a.par);
    } else {
      const double m = (FAM == SGP_QUAD_POISSON && a.expo && live) ? a.expo[row] : a.par;
      v = quad_nlp_row(FAM, y, mu, s2, m);
    }
    if (live) a.nlp[row] = v;
    const bool fin = live && fabs(v) <= 1.79769313486231570815e308;
    const double e = mu - y;
    const double s0 = nlp_block_sum(fin ? v : 0.0, red);
    const double s1 = nlp_block_sum(fin ? 1.0 : 0.0, red);
    const double s2n = nlp_block_sum((live && v != v) ? 1.0 : 0.0, red);
    const double s3 = nlp_block_sum(live ? e * e : 0.0, red);
    if (tid == 0) {
      double* o = a.part + 4 * (int64_t)tile;
      o[0] = s0;
      o[1] = s1;
      o[2] = s2n;
      o[3] = s3;
    }
  }
}

// stats[k] = sum over tiles of part[4 tile + k]: thread t adds tiles t, t + 256, ... in order,
// then the fixed-order block sum
__global__ void __launch_bounds__(NLP_THREADS) k_nlp_final(const double* __restrict__ part,
                                                           int ntiles, double* __restrict__ stats) {
  __shared__ double red[4];
  for (int k = 0; k < 4; ++k) {
    double v = 0.0;
    for (int q = threadIdx.x; q < ntiles; q += NLP_THREADS) v += part[4 * (int64_t)q + k];
    const double s = nlp_block_sum(v, red);
    if (threadIdx.x == 0) stats[k] = s;
  }
}

__global__ void __launch_bounds__(256) k_pred_finish(const double* __restrict__ mu_pred,
                                                     const double* __restrict__ yv,
                                                     const double* __restrict__ q, double c0,
                                                     int64_t np, double* __restrict__ pm,
                                                     double* __restrict__ pv) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < np) {
    pm[i] = mu_pred[i] + yv[i];
    pv[i] = c0 + q[i];
  }
}

template <int FAM>
hipError_t nlp_launch(const NlpArgs& a, int max_blocks, double* stats, hipStream_t s) {
  const int64_t nt64 = (a.n + NLP_THREADS - 1) / NLP_THREADS;
  if (nt64 > INT32_MAX) return hipErrorInvalidValue;
  const int ntiles = (int)nt64;
  const int grid = ntiles < max_blocks ? ntiles : max_blocks;
  hipLaunchKernelGGL(k_nlp_rows<FAM>, dim3(grid), dim3(NLP_THREADS), 0, s, a, ntiles);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_nlp_final, dim3(1), dim3(NLP_THREADS), 0, s, a.part, ntiles, stats);
  return hipGetLastError();
}

}  // namespace

int64_t nlp_part_doubles(int64_t n) { return 4 * ((n + NLP_THREADS - 1) / NLP_THREADS); }

hipError_t launch_nlp_rows(int fam, const NlpArgs& a, int max_blocks, double* stats,
                           hipStream_t s) {
  if (a.n < 1 || max_blocks < 1 || !a.y || !a.pm || !a.pv || !a.nlp || !a.part || !stats)
    return hipErrorInvalidValue;
  if (fam == SGP_QUAD_POISSON) return nlp_launch<SGP_QUAD_POISSON>(a, max_blocks, stats, s);
  if (fam == SGP_QUAD_BERNOULLI) return nlp_launch<SGP_QUAD_BERNOULLI>(a, max_blocks, stats, s);
  if (fam == SGP_QUAD_GAUSSIAN) return nlp_launch<SGP_QUAD_GAUSSIAN>(a, max_blocks, stats, s);
  return hipErrorInvalidValue;
}

hipError_t launch_pred_finish(const double* mu_pred, const double* yv, const double* q, double c0,
                              int64_t np, double* pm, double* pv, hipStream_t s) {
  if (np < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_pred_finish, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, mu_pred,
                     yv, q, c0, np, pm, pv);
  return hipGetLastError();
}
