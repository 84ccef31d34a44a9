// The row scans' (key, row) maximum and exclusion test, shared by k_ego.hip (sgp_ego_scan) and
// k_scan.hip (sgp_fit_scan).  The maximum is taken under a total order -- larger key, then lower
// row (R's which.max) -- so a result does not depend on the grid or on the order of the
// reduction.  Rows travel as doubles (exact below 2^53); row < 0 marks "no row yet".
#ifndef SGP_ARGMAX_H
#define SGP_ARGMAX_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// a beats b: b empty, or a's key larger, or equal keys and a's row lower (R's which.max)
__device__ __forceinline__ bool ego_better(double ka, double ra, double kb, double rb) {
  if (rb < 0.0) return ra >= 0.0;
  if (ra < 0.0) return false;
  return ka > kb || (ka == kb && ra < rb);
}

// (key, row) maximum over the 256 threads; red: 8 doubles of LDS.  Valid in thread 0.
__device__ __forceinline__ void ego_block_max(double& key, double& row, double* red) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double k2 = __shfl_xor(key, off, 64), r2 = __shfl_xor(row, off, 64);
    if (ego_better(k2, r2, key, row)) { key = k2; row = r2; }
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[2 * wv] = key; red[2 * wv + 1] = row; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w)
      if (ego_better(red[2 * w], red[2 * w + 1], key, row)) { key = red[2 * w]; row = red[2 * w + 1]; }
}

// Is the row whose coordinate c sits at xr[c * stride] one of the E rows of ex (E x d,
// column-major with ld E, sorted by coordinate 0)?  Binary search on coordinate 0, the other
// coordinates only on a hit; all d coordinates must be equal (==).
__device__ __forceinline__ bool ego_excluded(const double* __restrict__ ex, int64_t E, int d,
                                             const double* xr, int stride) {
  bool excluded = false;
  if (E > 0) {
    const double x0 = xr[0];
    int64_t lo = 0, hi = E;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (ex[mid] < x0) lo = mid + 1;
      else hi = mid;
    }
    for (int64_t k = lo; k < E && !excluded && ex[k] == x0; ++k) {
      bool all = true;
      for (int c = 1; c < d && all; ++c) all = ex[(int64_t)c * E + k] == xr[c * stride];
      excluded = all;
    }
  }
  return excluded;
}

#endif  // SGP_ARGMAX_H
